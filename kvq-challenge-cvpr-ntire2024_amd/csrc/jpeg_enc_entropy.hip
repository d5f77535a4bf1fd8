// kvq_jpeg_encode_scans: the baseline-JPEG Huffman CODING of T frames of coefficients on the device, ONE LANE PER 8 x 8 BLOCK, into
// the frames' byte-stuffed scans packed back to back.  What a lane does in each phase is jpeg_enc_huff.hpp, the one definition shared
// with kvq_jpeg_encode_scans_host (jpeg_enc.cpp); this file holds the launches and the two reductions.
//
// Shape: the per-block phases (count, ffcount, write) run 256-lane workgroups over (blocks of a frame, frame); a lane loads its
// block's 128 bytes with eight 16-byte loads into registers (every index is a constant once the coder's loop is unrolled: no
// scratch) and looks its codes up in the 4 KB of Annex K tables the workgroup copied into LDS.  The two prefix sums (bit positions,
// 0xFF counts) run ONE 1024-lane workgroup per frame that walks the frame in chunks of 1024 blocks with a running carry: a wave64
// scan by __shfl_up, the sixteen wave totals through LDS.  The position scan is not a plain sum — an interval starts on a byte
// boundary — but its elements combine associatively (JpegScanSeg), so it is one scan all the same, and a frame without restart
// markers is as parallel as one with them.  The per-frame table (frames) is one lane walking T entries.  No intermediate stream:
// a lane regenerates the bytes it owns (a byte belongs to the block its first bit lies in), so every output byte has ONE writer,
// two runs give equal bytes, and the only atomic is the integer OR of a frame's range verdict.
#include "common.hpp"
#include "jpeg_enc_huff.hpp"

namespace kvq {

constexpr int JES_LANES = 256;
constexpr int JES_SCAN_LANES = 1024;

__constant__ JpegEncTables jes_tables = jpeg_enc_tables();

__device__ __forceinline__ void jes_tables_to_lds(uint32_t* tab) {
  const uint32_t* src = &jes_tables.t[0][0];
  for (int i = threadIdx.x; i < 1024; i += JES_LANES) tab[i] = src[i];
  __syncthreads();
}

__global__ __launch_bounds__(JES_LANES) void jpeg_scans_count_kernel(JpegScansPlan p) {
  __shared__ uint32_t tab[1024];
  jes_tables_to_lds(tab);
  const uint32_t s = blockIdx.x * JES_LANES + threadIdx.x;
  if (s < (uint32_t)p.g.blocks) jpeg_scans_count(p, tab, blockIdx.y, s);
}

__global__ __launch_bounds__(JES_LANES) void jpeg_scans_ffcount_kernel(JpegScansPlan p) {
  __shared__ uint32_t tab[1024];
  jes_tables_to_lds(tab);
  const uint32_t s = blockIdx.x * JES_LANES + threadIdx.x;
  if (s < (uint32_t)p.g.blocks) jpeg_scans_ffcount(p, tab, blockIdx.y, s);
}

__global__ __launch_bounds__(JES_LANES) void jpeg_scans_write_kernel(JpegScansPlan p) {
  __shared__ uint32_t tab[1024];
  jes_tables_to_lds(tab);
  const uint32_t s = blockIdx.x * JES_LANES + threadIdx.x;
  if (s < (uint32_t)p.g.blocks) jpeg_scans_write(p, tab, blockIdx.y, s);
}

__global__ void jpeg_scans_frames_kernel(JpegScansPlan p) {
  if (threadIdx.x == 0 && blockIdx.x == 0) jpeg_scans_frames(p);
}

__device__ __forceinline__ JpegScanSeg jes_shfl_up(const JpegScanSeg& v, int d) {
  return JpegScanSeg{(uint32_t)__shfl_up((int)v.a, d), (uint32_t)__shfl_up((int)v.b, d), (uint32_t)__shfl_up((int)v.e, d)};
}

// FF = false: cnt (code lengths) -> pos, the frame's bytes.  FF = true: cnt (0xFF counts) -> their exclusive prefix in place, their sum.
template <bool FF>
__global__ __launch_bounds__(JES_SCAN_LANES) void jpeg_scans_scan_kernel(JpegScansPlan p) {
  __shared__ JpegScanSeg wave_total[JES_SCAN_LANES / 64];
  const uint32_t t = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t blocks = (uint32_t)p.g.blocks;
  const bool bad = p.fr32[2 * (size_t)t] != 0u;
  uint64_t carry = 0;
  for (uint32_t s0 = 0; s0 < blocks; s0 += JES_SCAN_LANES) {      // uniform trip count: every lane takes part in every shuffle
    const uint32_t s = s0 + threadIdx.x;
    const size_t gi = (size_t)t * blocks + s;
    JpegScanSeg mine{0u, 0u, 0u};
    if (s < blocks) mine = FF ? JpegScanSeg{p.cnt[gi], 0u, 0u} : jpeg_scans_seg(p, bad, t, s);
    JpegScanSeg inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const JpegScanSeg o = jes_shfl_up(inc, d);
      if (lane >= (uint32_t)d) inc = jpeg_scan_combine(o, inc);
    }
    if (lane == 63u) wave_total[wave] = inc;
    JpegScanSeg exc = jes_shfl_up(inc, 1);
    if (lane == 0u) exc = JpegScanSeg{0u, 0u, 0u};
    __syncthreads();
    JpegScanSeg before{0u, 0u, 0u}, total{0u, 0u, 0u};
    for (uint32_t w = 0; w < JES_SCAN_LANES / 64; ++w) {
      if (w == wave) before = total;
      total = jpeg_scan_combine(total, wave_total[w]);
    }
    const uint64_t x = jpeg_scan_apply(jpeg_scan_combine(before, exc), carry);
    if (s < blocks) {
      if (FF) p.cnt[gi] = (uint32_t)x;
      else p.pos[gi] = mine.e ? (x + 7u) & ~(uint64_t)7 : x;
    }
    carry = jpeg_scan_apply(total, carry);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (FF) p.fr32[2 * (size_t)t + 1] = (uint32_t)carry;
    else p.fr64[2 * (size_t)t] = (carry + 7u) >> 3;
  }
}

}  // namespace kvq

extern "C" int kvq_jpeg_encode_scans(const void* coef, int T, int H, int W, int restart_interval, void* out, size_t cap, void* frames_out,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  using namespace kvq;
  KVQ_REQUIRE(coef && out && frames_out && workspace, KVQ_ERR_NULL, "kvq_jpeg_encode_scans: NULL pointer");
  KVQ_REQUIRE(T > 0 && T < 65536 && jpeg_size_ok(H, W), KVQ_ERR_SHAPE, "kvq_jpeg_encode_scans: %d frames of %dx%d", T, H, W);
  KVQ_REQUIRE(restart_interval >= 0 && restart_interval <= 65535, KVQ_ERR_SHAPE, "kvq_jpeg_encode_scans: restart interval %d is outside 0..65535",
              restart_interval);
  KVQ_REQUIRE(cap < ((size_t)1 << 32), KVQ_ERR_SHAPE, "kvq_jpeg_encode_scans: a capacity of %zu bytes; offsets are 32-bit", cap);
  KVQ_REQUIRE((((uintptr_t)coef | (uintptr_t)workspace) & 15) == 0 && ((uintptr_t)frames_out & 3) == 0, KVQ_ERR_SHAPE,
              "kvq_jpeg_encode_scans: coef and workspace must be 16-byte aligned, frames_out 4-byte aligned");
  JpegScansPlan p{};
  p.coef = (const int16_t*)coef; p.out = (uint8_t*)out; p.frames_out = (uint32_t*)frames_out;
  p.cap = cap; p.T = (uint32_t)T; p.ri = (uint32_t)restart_interval; p.g = jpeg_geom(H, W);
  KVQ_REQUIRE(workspace_bytes >= jpeg_scans_workspace((size_t)T, p.g), KVQ_ERR_WORKSPACE,
              "kvq_jpeg_encode_scans: a workspace of %zu bytes; %d frames of %dx%d need %zu (kvq_jpeg_scans_workspace_bytes)", workspace_bytes, T, H, W,
              jpeg_scans_workspace((size_t)T, p.g));
  jpeg_scans_layout(p, workspace);
  KVQ_CHECK_HIP(hipMemsetAsync(p.fr32, 0, 8 * (size_t)T, (hipStream_t)stream));
  const dim3 per_block((unsigned)ceil_div(p.g.blocks, JES_LANES), (unsigned)T), lanes(JES_LANES);
  int rc = launch("jpeg_scans_count_kernel", jpeg_scans_count_kernel, per_block, lanes, 0, stream, p);
  if (rc == KVQ_OK) rc = launch("jpeg_scans_scan_kernel", jpeg_scans_scan_kernel<false>, dim3((unsigned)T), dim3(JES_SCAN_LANES), 0, stream, p);
  if (rc == KVQ_OK) rc = launch("jpeg_scans_ffcount_kernel", jpeg_scans_ffcount_kernel, per_block, lanes, 0, stream, p);
  if (rc == KVQ_OK) rc = launch("jpeg_scans_scan_kernel", jpeg_scans_scan_kernel<true>, dim3((unsigned)T), dim3(JES_SCAN_LANES), 0, stream, p);
  if (rc == KVQ_OK) rc = launch("jpeg_scans_frames_kernel", jpeg_scans_frames_kernel, dim3(1), dim3(64), 0, stream, p);
  if (rc == KVQ_OK) rc = launch("jpeg_scans_write_kernel", jpeg_scans_write_kernel, per_block, lanes, 0, stream, p);
  return rc;
}
