// kvq_jpeg_entropy: the baseline-JPEG Huffman decode of T compressed frames on the device, ONE LANE PER SEGMENT (a restart interval,
// or the whole scan of a frame without DRI), into the dense int16 hand-over kvq_jpeg_idct_i420 reads.  The decode itself is
// jpeg_huff.hpp, the one definition shared with kvq_jpeg_entropy_host (jpeg.cpp): what bounds its loops, reads and writes is
// stated there.
//
// Shape: a 64-lane workgroup (one wave) takes 64 consecutive segments of ONE frame (blockIdx.y), so its lanes share one table set,
// which the workgroup copies into LDS once (12 bytes + 1364 per distinct table: 5.5 KB for the usual four); the symbol lookups are LDS
// reads at lane-private addresses.  The stream is read through the lane's own unaligned 4-byte loads (bytes when the word holds an
// 0xFF or the segment's end is near), the non-zero coefficients leave as 2-byte scatters straight to global memory, which the entry
// has zero-filled on the same stream.  No per-thread block array, no scratch.  The grid's x extent covers the largest segment count a
// frame of this size can have (one per MCU); a workgroup past its frame's nseg leaves at once.  The lanes' loop lengths differ with
// their segments' contents: the divergence is inherent in one-lane-per-segment, and a frame without DRI is one active lane.
#include "common.hpp"
#include "jpeg_huff.hpp"

namespace kvq {

constexpr int JPEG_ENTROPY_LANES = 64;

struct JpegEntropyParams {
  const uint8_t* bytes;
  const uint32_t* frames;
  const uint32_t* segs;
  const KvqJpegTables* tables;
  int16_t* coef;
  int32_t* status;
  uint64_t nbytes;
  uint32_t nsegs, ntables;
  JpegGeom g;
};

__global__ __launch_bounds__(JPEG_ENTROPY_LANES) void jpeg_entropy_kernel(JpegEntropyParams p) {
  __shared__ __attribute__((aligned(16))) KvqJpegTables set;
  const int t = blockIdx.y;
  uint32_t f[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) f[i] = p.frames[5 * (size_t)t + i];
  const uint32_t s = blockIdx.x * JPEG_ENTROPY_LANES + threadIdx.x;
  if (blockIdx.x * JPEG_ENTROPY_LANES >= f[2] || f[1] > p.nsegs || f[2] > p.nsegs - f[1]) return;      // uniform: nothing of this frame here
  const bool frame_ok = jpeg_frame_ok(f, p.nbytes, p.nsegs, p.ntables, p.g);                           // uniform
  if (frame_ok) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(p.tables + f[4]);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&set);
    int ntab = (int)src[0];
    ntab = ntab < 0 ? 0 : (ntab > 6 ? 6 : ntab);
    const int words = 3 + ntab * (int)(sizeof(KvqJpegHuffTable) / 4);
    for (int i = threadIdx.x; i < words; i += JPEG_ENTROPY_LANES) dst[i] = src[i];
  }
  __syncthreads();
  if (s >= f[2]) return;
  p.status[f[1] + s] = jpeg_entropy_segment(f, s, &set, p.bytes, p.nbytes, p.segs, p.nsegs, p.ntables, p.g, p.coef + (size_t)t * p.g.blocks * 64);
}

}  // namespace kvq

extern "C" int kvq_jpeg_entropy(const void* bytes, size_t nbytes, const void* frames, const void* segs, size_t nsegs, const void* tables,
                                size_t ntables, int T, int H, int W, void* coef_out, void* status_out, void* stream) {
  using namespace kvq;
  KVQ_REQUIRE(bytes && frames && segs && tables && coef_out && status_out, KVQ_ERR_NULL, "kvq_jpeg_entropy: NULL pointer");
  KVQ_REQUIRE(T > 0 && T < 65536 && jpeg_size_ok(H, W), KVQ_ERR_SHAPE, "kvq_jpeg_entropy: %d frames of %dx%d", T, H, W);
  KVQ_REQUIRE(nbytes < ((size_t)1 << 32) && nsegs < ((size_t)1 << 32) && ntables > 0 && ntables < ((size_t)1 << 32), KVQ_ERR_SHAPE,
              "kvq_jpeg_entropy: %zu bytes, %zu segments, %zu table sets", nbytes, nsegs, ntables);
  KVQ_REQUIRE(((uintptr_t)coef_out & 15) == 0 && (((uintptr_t)frames | (uintptr_t)segs | (uintptr_t)tables | (uintptr_t)status_out) & 3) == 0,
              KVQ_ERR_SHAPE, "kvq_jpeg_entropy: coef_out must be 16-byte aligned, frames, segs, tables and status_out 4-byte aligned");
  JpegEntropyParams p{};
  p.bytes = (const uint8_t*)bytes; p.frames = (const uint32_t*)frames; p.segs = (const uint32_t*)segs;
  p.tables = (const KvqJpegTables*)tables; p.coef = (int16_t*)coef_out; p.status = (int32_t*)status_out;
  p.nbytes = nbytes; p.nsegs = (uint32_t)nsegs; p.ntables = (uint32_t)ntables; p.g = jpeg_geom(H, W);
  KVQ_CHECK_HIP(hipMemsetAsync(coef_out, 0, (size_t)T * p.g.blocks * 64 * sizeof(int16_t), (hipStream_t)stream));
  if (nsegs) KVQ_CHECK_HIP(hipMemsetAsync(status_out, 0xFF, nsegs * sizeof(int32_t), (hipStream_t)stream));
  return launch("jpeg_entropy_kernel", jpeg_entropy_kernel, dim3((unsigned)ceil_div(p.g.nc, JPEG_ENTROPY_LANES), (unsigned)T),
                dim3(JPEG_ENTROPY_LANES), 0, stream, p);
}
