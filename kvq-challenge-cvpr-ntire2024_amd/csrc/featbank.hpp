// What csrc/featbank.hip, csrc/headtrain.hip and csrc/simple_headtrain.hip share: the element types of a feature bank, the widening
// quad load, the index clamp, and the host checks of a step's bank.
#pragma once
#include "common.hpp"
#include "wave.hpp"

namespace kvq {

typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;

// ---- a bank row's elements: float, _Float16 or __bf16.  Widening to fp32 is exact for both 16-bit types.
// Four consecutive elements at p (16-byte aligned for float, 8-byte for the 16-bit types) as fp32.
__device__ __forceinline__ f32x4 bank_load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 bank_load4(const _Float16* p) {
  const f16x4 v = *reinterpret_cast<const f16x4*>(p);
  return (f32x4){(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
__device__ __forceinline__ f32x4 bank_load4(const __bf16* p) {
  const u32x2 v = *reinterpret_cast<const u32x2*>(p);
  return (f32x4){__uint_as_float(v[0] << 16), __uint_as_float(v[0] & 0xffff0000u), __uint_as_float(v[1] << 16),
                 __uint_as_float(v[1] & 0xffff0000u)};
}

// The bank row of batch position b: index[b] clamped into [0, n_rows), so that no index value can cause a read outside the bank.
__device__ __forceinline__ long bank_row(const int32_t* __restrict__ index, long n_rows, long b) {
  const long r = index[b];
  return r < 0 ? 0 : (r < n_rows ? r : n_rows - 1);
}

static inline bool bank_dtype_ok(int dtype) { return dtype == KVQ_DT_FP32 || dtype == KVQ_DT_FP16 || dtype == KVQ_DT_BF16; }
static inline size_t bank_elem_bytes(int dtype) { return dtype == KVQ_DT_FP32 ? 4 : 2; }

// f(float{}), f(_Float16{}) or f(__bf16{}) for a dtype that passed bank_dtype_ok: a launch site names its kernel once, as
// kernel<decltype(e), ...>
template <class F>
int with_bank_elem(int dtype, F&& f) {
  if (dtype == KVQ_DT_FP32) return f(float{});
  return dtype == KVQ_DT_FP16 ? f(_Float16{}) : f(__bf16{});
}

// ---- what the two training steps share on the host
// The checks of a step's bank and index, made before the head's own: NULL args, rows or index; the bank's dtype, alignment and shape; the
// index's alignment; (L, C) of the bank against the step's; the 32-bit batch position.
int headtrain_bank_check(const KvqHeadTrainBankArgs* a, const char* who);

// The flat parameter (or gradient) vector W1 [hidden][C] | b1 [hidden] | w2 [hidden] | b2 [1]
struct HeadParams {
  const float *w1, *b1, *w2, *b2;
};
inline HeadParams head_params(const float* flat, int hidden, int C) {
  const float* b1 = flat + (size_t)hidden * C;
  return {flat, b1, b1 + hidden, b1 + 2 * hidden};
}

}  // namespace kvq
