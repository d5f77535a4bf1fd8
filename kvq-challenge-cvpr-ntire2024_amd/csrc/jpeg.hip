// kvq_jpeg_idct_i420: T frames of quantised JPEG coefficients (the dense int16 hand-over of csrc/jpeg.cpp) -> T I420 frames.  Per 8 x 8
// block: dequantise, the two-pass integer inverse DCT of jpeg_idct.hpp (the ONE definition, shared with the host twin), + 128, clamp,
// store, the MCU padding at the right and bottom edges cropped.
//
// Memory-bound: 2 B read per coefficient, 1 B written per sample.  Eight lanes make a block, a 256-thread workgroup 32 blocks:
//   load     lane l of a block reads ROW l of its coefficients, 16 bytes — a wave reads 1 KiB of consecutive bytes per instruction —
//            and the same row of the quantiser table (384 B per frame: cache hits), and writes the 8 products to LDS as int32.
//   pass 1   lane l reads COLUMN l (8 ds_read_b32), transforms it in registers, writes it back to the slots it read.
//   pass 2   lane l reads ROW l (2 ds_read_b128), transforms it, packs 8 bytes: one 8-byte store, or byte stores at a cropped edge.
// LDS image: [block][8][8] int32 with a block stride of 72 dwords: the four blocks of a 32-lane group then start 8 banks apart, so
// the column accesses (lane l of block b on bank 8 b + l + 8 r mod 32) are conflict-free.  The lanes of a block sit in one wave; the
// two exchanges are still fenced by workgroup barriers, which every thread reaches (a thread without a block only skips the memory
// accesses).  Rows of an odd-width plane are not 8-byte aligned: byte-aligned vector stores, as in yuv.hip.
#include "common.hpp"
#include "jpeg_idct.hpp"
#include "yuv.hpp"

namespace kvq {

typedef u32x2 __attribute__((aligned(1))) u32x2u;

constexpr int JPEG_BLOCKS_PER_WG = 32;
constexpr int JPEG_LDS_STRIDE = 72;      // dwords per block: 64 + 8

struct JpegIdctParams {
  const int16_t* coef;
  const uint16_t* qt;
  uint8_t* out;
  int H, W;
  JpegGeom g;
};

__global__ __launch_bounds__(256) void jpeg_idct_i420_kernel(JpegIdctParams p) {
  __shared__ __attribute__((aligned(16))) int32_t lds[JPEG_BLOCKS_PER_WG * JPEG_LDS_STRIDE];
  const int l = threadIdx.x & 7, slot = threadIdx.x >> 3, t = blockIdx.y;
  const int b = blockIdx.x * JPEG_BLOCKS_PER_WG + slot;
  const bool live = b < p.g.blocks;
  int32_t* ws = lds + slot * JPEG_LDS_STRIDE;
  const int c = b < p.g.ny ? 0 : (b < p.g.ny + p.g.nc ? 1 : 2);
  int32_t v[8];
  if (live) {
    const u32x4 cw = *reinterpret_cast<const u32x4*>(p.coef + ((size_t)t * p.g.blocks + b) * 64 + 8 * l);
    const u32x4 qw = *reinterpret_cast<const u32x4*>(p.qt + ((size_t)t * 3 + c) * 64 + 8 * l);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int32_t cf = (int16_t)(cw[u >> 1] >> (16 * (u & 1)));
      const int32_t q = (int32_t)((qw[u >> 1] >> (16 * (u & 1))) & 0xFFFFu);
      v[u] = jw_mul(cf, q);
    }
    *reinterpret_cast<i32x4*>(ws + 8 * l) = (i32x4){v[0], v[1], v[2], v[3]};
    *reinterpret_cast<i32x4*>(ws + 8 * l + 4) = (i32x4){v[4], v[5], v[6], v[7]};
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = ws[8 * r + l];
    jpeg_idct_pass1(v);
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[8 * r + l] = v[r];
  }
  __syncthreads();
  if (!live) return;
  const I420Geom geo = i420_geom(p.H, p.W);
  const int id = c == 0 ? b : b - p.g.ny - (c - 1) * p.g.nc;
  const int bpr = c == 0 ? 2 * p.g.mx : p.g.mx;
  const int ph = c == 0 ? p.H : (p.H + 1) >> 1, pw = c == 0 ? p.W : geo.cw;
  const int by = id / bpr, bx = id - by * bpr;
  const int y = 8 * by + l, x0 = 8 * bx;
  if (y >= ph || x0 >= pw) return;                       // MCU padding
  const i32x4 a = *reinterpret_cast<const i32x4*>(ws + 8 * l), d = *reinterpret_cast<const i32x4*>(ws + 8 * l + 4);
  v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = d[0]; v[5] = d[1]; v[6] = d[2]; v[7] = d[3];
  jpeg_idct_pass2(v);
  uint8_t* o = p.out + (size_t)t * geo.frame + (c == 0 ? 0 : geo.ysize + (c - 1) * geo.csize) + (size_t)y * pw + x0;
  if (x0 + 8 <= pw) {
    uint32_t w[2] = {0, 0};
#pragma unroll
    for (int u = 0; u < 8; ++u) w[u >> 2] |= (uint32_t)v[u] << (8 * (u & 3));
    *reinterpret_cast<u32x2u*>(o) = (u32x2){w[0], w[1]};
  } else {
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (x0 + u < pw) o[u] = (uint8_t)v[u];
  }
}

}  // namespace kvq

extern "C" int kvq_jpeg_idct_i420(const void* coef, const void* qt, int T, int H, int W, uint8_t* frames_out, void* stream) {
  using namespace kvq;
  KVQ_REQUIRE(coef && qt && frames_out, KVQ_ERR_NULL, "kvq_jpeg_idct_i420: NULL pointer");
  KVQ_REQUIRE(T > 0 && T < 65536 && jpeg_size_ok(H, W), KVQ_ERR_SHAPE, "kvq_jpeg_idct_i420: %d frames of %dx%d", T, H, W);
  KVQ_REQUIRE(((uintptr_t)coef & 15) == 0 && ((uintptr_t)qt & 15) == 0, KVQ_ERR_SHAPE,
              "kvq_jpeg_idct_i420: coef and qt must be 16-byte aligned");
  JpegIdctParams p{};
  p.coef = (const int16_t*)coef; p.qt = (const uint16_t*)qt; p.out = frames_out; p.H = H; p.W = W; p.g = jpeg_geom(H, W);
  return launch("jpeg_idct_i420_kernel", jpeg_idct_i420_kernel, dim3((unsigned)ceil_div(p.g.blocks, JPEG_BLOCKS_PER_WG), (unsigned)T),
                dim3(256), 0, stream, p);
}
