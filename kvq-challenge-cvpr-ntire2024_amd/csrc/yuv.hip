// kvq_yuv420_to_rgb: T planar YUV 4:2:0 frames (I420, frame-major) -> uint8 (3, T, H, W), for the consumers that take whole frames anyway
// (the resize views, the upsample fallback, fp32 consumers).  The arithmetic is yuv.hpp's: the one conversion of every I420 consumer.
//
// Bandwidth-bound: 1.5 B/pixel read, 3 B/pixel written.  A work item owns 16 consecutive pixels of a PAIR of luma rows 2r, 2r + 1 —
// the two rows share one chroma row, so it is loaded once: two 16-byte Y loads, two 8-byte chroma loads, six 16-byte stores.  Rows of
// an odd width are not 16-byte aligned: the loads and stores are byte-aligned vector accesses (gfx950 takes them; a wave's 64 items
// still cover 1 KiB of consecutive bytes per row).  The last items of a row (W % 16 != 0) and the last row of an odd height go byte
// by byte; no access leaves the frame it belongs to.
#include "yuv.hpp"

namespace kvq {

typedef u32x4 __attribute__((aligned(1))) u32x4u;
typedef u32x2 __attribute__((aligned(1))) u32x2u;

struct YuvParams {
  const uint8_t* frames;
  uint8_t* out;
  int T, H, W, groups, pairs;     // 16-pixel groups per row, row pairs per frame
  YuvCoef k;
};

__global__ __launch_bounds__(256) void yuv420_to_rgb_kernel(YuvParams p) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  const int r = q / p.groups, g = q - r * p.groups, t = blockIdx.y;
  if (r >= p.pairs) return;
  const I420Geom geo = i420_geom(p.H, p.W);
  const uint8_t* f = p.frames + (size_t)t * geo.frame;
  const int x0 = 16 * g, y0 = 2 * r;
  const int nx = min(16, p.W - x0), ny = min(2, p.H - y0);      // >= 1 each
  const int cx0 = x0 >> 1, nc = (nx + 1) >> 1;
  const uint8_t* urow = f + geo.ysize + (size_t)r * geo.cw + cx0;
  const uint8_t* vrow = urow + geo.csize;
  uint32_t uw[2] = {0, 0}, vw[2] = {0, 0};                       // 8 chroma samples each, byte e of word e >> 2
  if (nc == 8) {
    const u32x2 a = *reinterpret_cast<const u32x2u*>(urow), b = *reinterpret_cast<const u32x2u*>(vrow);
    uw[0] = a[0]; uw[1] = a[1]; vw[0] = b[0]; vw[1] = b[1];
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e < nc) {
        uw[e >> 2] |= (uint32_t)urow[e] << (8 * (e & 3));
        vw[e >> 2] |= (uint32_t)vrow[e] << (8 * (e & 3));
      }
  }
  YuvChroma ch[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) ch[c] = yuv_chroma(p.k, (int)((uw[c >> 2] >> (8 * (c & 3))) & 255u), (int)((vw[c >> 2] >> (8 * (c & 3))) & 255u));
  const size_t plane = (size_t)p.T * geo.ysize;
  for (int j = 0; j < ny; ++j) {
    const uint8_t* yrow = f + (size_t)(y0 + j) * p.W + x0;
    uint32_t yw[4] = {0, 0, 0, 0};
    if (nx == 16) {
      const u32x4 a = *reinterpret_cast<const u32x4u*>(yrow);
      yw[0] = a[0]; yw[1] = a[1]; yw[2] = a[2]; yw[3] = a[3];
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < nx) yw[e >> 2] |= (uint32_t)yrow[e] << (8 * (e & 3));
    }
    uint32_t rw[4] = {0, 0, 0, 0}, gw[4] = {0, 0, 0, 0}, bw[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int l = yuv_luma(p.k, (int)((yw[e >> 2] >> (8 * (e & 3))) & 255u));
      rw[e >> 2] |= (uint32_t)yuv_out(l, ch[e >> 1].r) << (8 * (e & 3));
      gw[e >> 2] |= (uint32_t)yuv_out(l, ch[e >> 1].g) << (8 * (e & 3));
      bw[e >> 2] |= (uint32_t)yuv_out(l, ch[e >> 1].b) << (8 * (e & 3));
    }
    uint8_t* o = p.out + (size_t)t * geo.ysize + (size_t)(y0 + j) * p.W + x0;
    if (nx == 16) {
      *reinterpret_cast<u32x4u*>(o) = (u32x4){rw[0], rw[1], rw[2], rw[3]};
      *reinterpret_cast<u32x4u*>(o + plane) = (u32x4){gw[0], gw[1], gw[2], gw[3]};
      *reinterpret_cast<u32x4u*>(o + 2 * plane) = (u32x4){bw[0], bw[1], bw[2], bw[3]};
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < nx) {
          o[e] = (uint8_t)(rw[e >> 2] >> (8 * (e & 3)));
          o[plane + e] = (uint8_t)(gw[e >> 2] >> (8 * (e & 3)));
          o[2 * plane + e] = (uint8_t)(bw[e >> 2] >> (8 * (e & 3)));
        }
    }
  }
}

}  // namespace kvq

extern "C" int kvq_yuv420_coeffs(int format, int32_t out6[6]) {
  using namespace kvq;
  KVQ_REQUIRE(out6, KVQ_ERR_NULL, "kvq_yuv420_coeffs: NULL pointer");
  KVQ_REQUIRE(yuv_format_ok(format), KVQ_ERR_UNSUPPORTED, "kvq_yuv420_coeffs: format %d is not a KVQ_SRC_I420_* value", format);
  const YuvCoef k = yuv420_coeffs(format);
  out6[0] = k.qy; out6[1] = k.qrv; out6[2] = k.qgu; out6[3] = k.qgv; out6[4] = k.qbu; out6[5] = k.yoff;
  return KVQ_OK;
}

extern "C" int kvq_yuv420_to_rgb(const void* frames, int T, int H, int W, int format, uint8_t* rgb_out, void* stream) {
  using namespace kvq;
  KVQ_REQUIRE(frames && rgb_out, KVQ_ERR_NULL, "kvq_yuv420_to_rgb: NULL pointer");
  KVQ_REQUIRE(yuv_format_ok(format), KVQ_ERR_UNSUPPORTED, "kvq_yuv420_to_rgb: format %d is not a KVQ_SRC_I420_* value", format);
  KVQ_REQUIRE(T > 0 && T < 65536 && i420_size_ok(H, W), KVQ_ERR_SHAPE,
              "kvq_yuv420_to_rgb: %d frames of %dx%d", T, H, W);
  YuvParams p{};
  p.frames = (const uint8_t*)frames; p.out = rgb_out; p.T = T; p.H = H; p.W = W;
  p.groups = ceil_div(W, 16); p.pairs = (H + 1) / 2; p.k = yuv420_coeffs(format);
  return launch("yuv420_to_rgb_kernel", yuv420_to_rgb_kernel, dim3((unsigned)ceil_div(p.groups * p.pairs, 256), (unsigned)T), dim3(256), 0,
                stream, p);
}
