// Wave-level primitives of gfx950 that the kernels share: address-space pointers, counted waits, buffer resources, the LDS-DMA copy
// of a contiguous image, and the 64-lane sums.  Nothing here knows a kernel's layout (rows.hpp holds the 32 x 32 accumulator's).
#pragma once
#include "common.hpp"

namespace kvq {

// the operand types of __builtin_amdgcn_global_load_lds / raw_ptr_buffer_load_lds
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef __attribute__((address_space(1))) const void* gbl_ptr_t;

// s_waitcnt with a compile-time count: at most N vector-memory loads (LDS-DMA included) / LDS and scalar operations still in flight
template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int N>
__device__ __forceinline__ void wait_lgkmcnt() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory"); }

// buffer resource over [base, base + bytes): raw (stride 0), out-of-range reads return 0
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, size_t bytes) {
  const unsigned nr = bytes > 0xffffffffull ? 0xffffffffu : (unsigned)bytes;
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)nr, 0x00020000);
}

// A contiguous image global -> LDS in 1 KB wave-loads (16 bytes per lane, no registers): this wave takes pieces first, first + STEP, ...
// below n_pieces.  Nothing waits here: the caller counts the loads (wait_vmcnt) and owns the barrier.
template <int STEP>
__device__ __forceinline__ void lds_dma_image(unsigned char* dst, const unsigned char* src, int first, int n_pieces, int lane) {
  for (int q = first; q < n_pieces; q += STEP)
    __builtin_amdgcn_global_load_lds((gbl_ptr_t)(src + q * 1024 + lane * 16), (lds_ptr_t)(dst + q * 1024), 16, 0, 0);
}

// Sum over the 64 lanes of a wave, the same value in every lane.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// Workgroup-wide sum of one float per thread (256 threads), the same value in every thread: wave butterflies, then the four wave sums
// in a fixed order.  wsum: 4 floats of LDS, reusable after the call returns in every thread.
__device__ __forceinline__ float block_sum(float v, float* wsum) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  return (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

}  // namespace kvq
