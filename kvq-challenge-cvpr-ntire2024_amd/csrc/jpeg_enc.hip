// kvq_jpeg_fdct: T frames (uint8 R G B planes, or BT.601 full-range I420) -> T frames of quantised JPEG coefficients in the dense
// int16 hand-over kvq_jpeg_idct_i420 reads: the mirror of jpeg.hip.  Per 8 x 8 block: level shift, the two-pass integer forward DCT
// and the quantiser of jpeg_fdct.hpp (the ONE definition, shared with the host twin in jpeg_enc.cpp).  An RGB source is converted
// where its pixels are loaded: no YCbCr or I420 frame goes to HBM.
//
// Memory-bound: 1 B (I420: 1.5 per pixel) or 3 B (RGB) read per pixel, 2 B written per coefficient.  The unit of work is the 16 x 16
// MCU, because that is the footprint of a chroma block of an RGB source: 32 lanes make an MCU, a 256-thread workgroup 8 MCUs that
// are neighbours in a row of MCUs.
//   load     lane (k, l) of an MCU owns ROW l of Y block k: 8 bytes of Y, or 8 bytes each of R, G and B — the 16 lanes of the 8 MCUs
//            that share a pixel row read 128 consecutive bytes of it.  RGB: the lane converts its 8 pixels to Y, Cb, Cr, adds the Cb
//            and Cr of horizontal neighbours, swaps one of the two sums with the lane of the row below or above (lane ^ 1) and so
//            ends up with 4 finished samples of one chroma row: Cb on even rows, Cr on odd ones.  They go to LDS, level-shifted.
//            I420: lanes 0..15 load row l of the Cb / Cr block as well.  An MCU that crosses the right or bottom edge of the
//            picture takes jpeg_src_sample per sample instead (clamped coordinates: the padding rule).
//   pass 1   on the Y row in registers, before it is written to LDS; lanes 0..15 then read ROW l of a chroma block, transform it and
//            write it back to the slots they read.
//   pass 2   lane (k, l) reads COLUMN l of Y block k (8 ds_read_b32), transforms it, quantises with the reciprocals of the frame's
//            tables — 192 of them, prepared once per workgroup in LDS, one division per thread and 2048 coefficients — and writes
//            the column back; lanes 0..15 do the same for the chroma blocks.
//   store    lane (k, l) reads ROW l (2 ds_read_b128), packs 8 int16: one 16-byte store; a row of Y blocks is written 256
//            consecutive bytes per MCU, 2 KiB per workgroup.
// LDS image: [MCU][6 blocks][8][8] int32 with a block stride of 72 dwords, as in jpeg.hip: the four Y blocks of an MCU start 8 banks
// apart, so the column accesses are conflict-free.  The exchanges are fenced by workgroup barriers that every thread reaches (a
// thread without an MCU only skips the memory accesses).  Rows of a frame are not 8-byte aligned in general: byte-aligned vector
// loads, as the stores of jpeg.hip.
#include "common.hpp"
#include "jpeg_fdct.hpp"

namespace kvq {

typedef u32x2 __attribute__((aligned(1))) u32x2u;

constexpr int FDCT_MCUS_PER_WG = 8;
constexpr int FDCT_BLOCK_STRIDE = 72;                        // dwords per block: 64 + 8
constexpr int FDCT_MCU_STRIDE = 6 * FDCT_BLOCK_STRIDE;

struct JpegFdctParams {
  const uint8_t* src;
  const uint16_t* qt;
  int16_t* coef;
  int T, H, W;
  JpegGeom g;
};

__device__ __forceinline__ void fdct_put_row(int32_t* row, const int32_t v[8]) {
  *reinterpret_cast<i32x4*>(row) = (i32x4){v[0], v[1], v[2], v[3]};
  *reinterpret_cast<i32x4*>(row + 4) = (i32x4){v[4], v[5], v[6], v[7]};
}
__device__ __forceinline__ void fdct_get_row(const int32_t* row, int32_t v[8]) {
  const i32x4 a = *reinterpret_cast<const i32x4*>(row), d = *reinterpret_cast<const i32x4*>(row + 4);
  v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = d[0]; v[5] = d[1]; v[6] = d[2]; v[7] = d[3];
}
// 8 consecutive bytes from any address -> level-shifted samples
__device__ __forceinline__ void fdct_load8(const uint8_t* s, int32_t v[8]) {
  const u32x2 w = *reinterpret_cast<const u32x2u*>(s);
#pragma unroll
  for (int u = 0; u < 8; ++u) v[u] = (int32_t)((w[u >> 2] >> (8 * (u & 3))) & 255u);
}
// pass 2 and the quantiser on column l of a block, in place
__device__ __forceinline__ void fdct_column(int32_t* blk, int l, const uint32_t* recip, const uint32_t* half) {
  int32_t v[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = blk[8 * r + l];
  jpeg_fdct_pass2(v);
#pragma unroll
  for (int r = 0; r < 8; ++r) blk[8 * r + l] = jpeg_quantise(v[r], recip[8 * r + l], half[8 * r + l]);
}
// row l of a finished block -> 16 bytes of the hand-over
__device__ __forceinline__ void fdct_store_row(const int32_t* blk, int l, int16_t* dst) {
  int32_t v[8];
  fdct_get_row(blk + 8 * l, v);
  u32x4 w;
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = ((uint32_t)v[2 * i] & 0xFFFFu) | ((uint32_t)v[2 * i + 1] << 16);
  *reinterpret_cast<u32x4*>(dst + 8 * l) = w;
}

template <bool RGB>
__global__ __launch_bounds__(256) void jpeg_fdct_kernel(JpegFdctParams p) {
  __shared__ __attribute__((aligned(16))) int32_t lds[FDCT_MCUS_PER_WG * FDCT_MCU_STRIDE];
  __shared__ uint32_t recip[192], half[192];
  const int tid = threadIdx.x, t = blockIdx.y;
  if (tid < 192) {
    const uint32_t q = p.qt[(size_t)t * 192 + tid];
    recip[tid] = jpeg_quant_recip(q);
    half[tid] = 4u * jpeg_quant_clamp(q);
  }
  const int lane = tid & 31, slot = tid >> 5, k = lane >> 3, l = lane & 7;
  const int m = blockIdx.x * FDCT_MCUS_PER_WG + slot;
  const bool live = m < p.g.nc;
  const int my = m / p.g.mx, mx = m - my * p.g.mx;
  int32_t* ws = lds + slot * FDCT_MCU_STRIDE;
  const int cj = lane >> 3 & 1;                              // lanes 0..15: the chroma block (0 Cb, 1 Cr) they serve after the load
  int32_t* cblk = ws + (4 + cj) * FDCT_BLOCK_STRIDE;
  int32_t v[8];
  if (live) {
    const int y = 16 * my + 8 * (k >> 1) + l, x0 = 16 * mx + 8 * (k & 1);
    if (16 * mx + 16 <= p.W && 16 * my + 16 <= p.H) {        // the whole MCU lies inside the picture
      if (RGB) {
        const size_t plane = (size_t)p.T * p.H * p.W;
        const uint8_t* s = p.src + ((size_t)t * p.H + y) * p.W + x0;
        int32_t r[8], g[8], b[8], sb[4], sr[4];
        fdct_load8(s, r);
        fdct_load8(s + plane, g);
        fdct_load8(s + 2 * plane, b);
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = jpeg_rgb_y(r[u], g[u], b[u]) - 128;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          sb[j] = jpeg_rgb_cb(r[2 * j], g[2 * j], b[2 * j]) + jpeg_rgb_cb(r[2 * j + 1], g[2 * j + 1], b[2 * j + 1]);
          sr[j] = jpeg_rgb_cr(r[2 * j], g[2 * j], b[2 * j]) + jpeg_rgb_cr(r[2 * j + 1], g[2 * j + 1], b[2 * j + 1]);
        }
        // rows 2 i and 2 i + 1 sit in lanes l and l ^ 1: the even row keeps Cb and hands over its Cr sums, the odd row the reverse
        const int odd = l & 1;
        i32x4 c4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int32_t other = __shfl_xor(odd ? sb[j] : sr[j], 1);
          c4[j] = (((odd ? sr[j] : sb[j]) + other + 1 + (j & 1)) >> 2) - 128;
        }
        *reinterpret_cast<i32x4*>(ws + (4 + odd) * FDCT_BLOCK_STRIDE + 8 * (4 * (k >> 1) + (l >> 1)) + 4 * (k & 1)) = c4;
      } else {
        const size_t ysize = (size_t)p.H * p.W, cw = (size_t)((p.W + 1) >> 1), csize = (size_t)((p.H + 1) >> 1) * cw;
        const uint8_t* f = p.src + (size_t)t * (ysize + 2 * csize);
        fdct_load8(f + (size_t)y * p.W + x0, v);
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] -= 128;
        if (lane < 16) {
          int32_t c[8];
          fdct_load8(f + ysize + cj * csize + (size_t)(8 * my + l) * cw + 8 * mx, c);
#pragma unroll
          for (int u = 0; u < 8; ++u) c[u] -= 128;
          fdct_put_row(cblk + 8 * l, c);
        }
      }
    } else {
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = jpeg_src_sample(p.src, RGB, p.T, p.H, p.W, t, 0, y, x0 + u) - 128;
      if (lane < 16) {
        int32_t c[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) c[u] = jpeg_src_sample(p.src, RGB, p.T, p.H, p.W, t, 1 + cj, 8 * my + l, 8 * mx + u) - 128;
        fdct_put_row(cblk + 8 * l, c);
      }
    }
    jpeg_fdct_pass1(v);
    fdct_put_row(ws + k * FDCT_BLOCK_STRIDE + 8 * l, v);
  }
  __syncthreads();
  if (live && lane < 16) {
    fdct_get_row(cblk + 8 * l, v);
    jpeg_fdct_pass1(v);
    fdct_put_row(cblk + 8 * l, v);
  }
  __syncthreads();
  if (live) {
    fdct_column(ws + k * FDCT_BLOCK_STRIDE, l, recip, half);
    if (lane < 16) fdct_column(cblk, l, recip + 64 * (1 + cj), half + 64 * (1 + cj));
  }
  __syncthreads();
  if (!live) return;
  int16_t* out = p.coef + (size_t)t * p.g.blocks * 64;
  fdct_store_row(ws + k * FDCT_BLOCK_STRIDE, l, out + ((size_t)(2 * my + (k >> 1)) * (2 * p.g.mx) + 2 * mx + (k & 1)) * 64);
  if (lane < 16) fdct_store_row(cblk, l, out + ((size_t)p.g.ny + (size_t)cj * p.g.nc + m) * 64);
}

}  // namespace kvq

extern "C" int kvq_jpeg_fdct(const void* src, int src_format, int T, int H, int W, const void* qt, void* coef_out, void* stream) {
  using namespace kvq;
  KVQ_REQUIRE(src && qt && coef_out, KVQ_ERR_NULL, "kvq_jpeg_fdct: NULL pointer");
  KVQ_REQUIRE(src_format == KVQ_SRC_U8 || src_format == KVQ_SRC_I420_BT601_FULL, KVQ_ERR_UNSUPPORTED,
              "kvq_jpeg_fdct: source format %d — uint8 R G B planes (KVQ_SRC_U8) or BT.601 full-range I420 frames "
              "(KVQ_SRC_I420_BT601_FULL) only; convert anything else first (kvq_yuv420_to_rgb)", src_format);
  KVQ_REQUIRE(T > 0 && T < 65536 && jpeg_size_ok(H, W), KVQ_ERR_SHAPE, "kvq_jpeg_fdct: %d frames of %dx%d", T, H, W);
  KVQ_REQUIRE(((uintptr_t)coef_out & 15) == 0 && ((uintptr_t)qt & 15) == 0, KVQ_ERR_SHAPE,
              "kvq_jpeg_fdct: coef_out and qt must be 16-byte aligned");
  JpegFdctParams p{};
  p.src = (const uint8_t*)src; p.qt = (const uint16_t*)qt; p.coef = (int16_t*)coef_out; p.T = T; p.H = H; p.W = W; p.g = jpeg_geom(H, W);
  const dim3 grid((unsigned)ceil_div(p.g.nc, FDCT_MCUS_PER_WG), (unsigned)T);
  return src_format == KVQ_SRC_U8 ? launch("jpeg_fdct_kernel<rgb>", jpeg_fdct_kernel<true>, grid, dim3(256), 0, stream, p)
                                  : launch("jpeg_fdct_kernel<i420>", jpeg_fdct_kernel<false>, grid, dim3(256), 0, stream, p);
}
