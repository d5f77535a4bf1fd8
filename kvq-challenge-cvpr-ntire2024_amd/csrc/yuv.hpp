// Planar YUV 4:2:0 (I420, frame-major) -> RGB: the ONE definition of the conversion every consumer of an I420 source uses
// (kvq_yuv420_to_rgb, the fragment gathers, the fused embedding read, the overlay of the quality paint) and the host reads back
// through kvq_yuv420_coeffs.  Integer arithmetic with 16 fractional bits, nearest chroma (pixel (y, x) takes sample (y >> 1, x >> 1)):
//   R = clamp((qy (Y - yoff) + qrv (V - 128) + 32768) >> 16, 0, 255)        G: qgu (U - 128) + qgv (V - 128)        B: qbu (U - 128)
// |terms| < 2^25: int32 never overflows.  The shift of a negative sum is arithmetic (floor).
#pragma once
#include "common.hpp"

namespace kvq {

struct YuvCoef {
  int32_t qy, qrv, qgu, qgv, qbu, yoff;
};

static inline bool yuv_format_ok(int format) { return format >= KVQ_SRC_I420_BT601_LIMITED && format <= KVQ_SRC_I420_BT709_FULL; }

// q = floor(c * 65536 + 0.5) of the five coefficients derived from (Kr, Kb); limited range: luma (Y - 16) * 255 / 219, chroma * 255 / 224.
// Evaluated on the host only: the launches carry the six integers as parameters.
static inline YuvCoef yuv420_coeffs(int format) {
  const bool bt709 = format == KVQ_SRC_I420_BT709_LIMITED || format == KVQ_SRC_I420_BT709_FULL;
  const bool full = format == KVQ_SRC_I420_BT601_FULL || format == KVQ_SRC_I420_BT709_FULL;
  const double kr = bt709 ? 0.2126 : 0.299, kb = bt709 ? 0.0722 : 0.114, kg = 1.0 - kr - kb;
  const double sy = full ? 1.0 : 255.0 / 219.0, sc = full ? 1.0 : 255.0 / 224.0;
  auto q = [](double c) { return (int32_t)__builtin_floor(c * 65536.0 + 0.5); };
  YuvCoef k;
  k.qy = q(sy);
  k.qrv = q(2.0 * (1.0 - kr) * sc);
  k.qgu = q(-2.0 * (1.0 - kb) * kb / kg * sc);
  k.qgv = q(-2.0 * (1.0 - kr) * kr / kg * sc);
  k.qbu = q(2.0 * (1.0 - kb) * sc);
  k.yoff = full ? 0 : 16;
  return k;
}

__host__ __device__ __forceinline__ int yuv_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// A pixel = the luma term of its Y (rounding offset included) + the chroma terms of its (U, V) sample, which every pixel of the
// sample's 2 x 2 block shares: computed once per sample where a consumer holds several of its pixels.
struct YuvChroma {
  int r, g, b;
};
__host__ __device__ __forceinline__ int yuv_luma(const YuvCoef& k, int Y) { return k.qy * (Y - k.yoff) + 32768; }
__host__ __device__ __forceinline__ YuvChroma yuv_chroma(const YuvCoef& k, int U, int V) {
  return YuvChroma{k.qrv * (V - 128), k.qgu * (U - 128) + k.qgv * (V - 128), k.qbu * (U - 128)};
}
__host__ __device__ __forceinline__ int yuv_out(int luma, int chroma) { return yuv_clamp8((luma + chroma) >> 16); }
__host__ __device__ __forceinline__ int yuv_channel(const YuvCoef& k, int c, int Y, int U, int V) {
  const YuvChroma ch = yuv_chroma(k, U, V);
  return yuv_out(yuv_luma(k, Y), c == 0 ? ch.r : (c == 1 ? ch.g : ch.b));
}

// geometry of one I420 frame: Y (H x W) | U | V (ceil(H/2) x ceil(W/2) each), contiguous
struct I420Geom {
  int H, W, cw;
  int ysize, csize, frame;     // bytes; a frame stays far below 2^31 (i420_size_ok, checked by the entry points)
};
static inline bool i420_size_ok(int H, int W) { return H > 0 && W > 0 && (long)H * W < (1L << 29); }
__host__ __device__ __forceinline__ I420Geom i420_geom(int H, int W) {
  I420Geom g;
  g.H = H; g.W = W; g.cw = (W + 1) >> 1;
  g.ysize = H * W;
  g.csize = ((H + 1) >> 1) * g.cw;
  g.frame = g.ysize + 2 * g.csize;
  return g;
}
// channel c of pixel (y, x) of the frame at `f`: three byte loads, all inside the frame
__device__ __forceinline__ int i420_pixel(const uint8_t* f, const I420Geom& g, const YuvCoef& k, int c, int y, int x) {
  const uint8_t* u = f + g.ysize + (size_t)(y >> 1) * g.cw + (x >> 1);
  return yuv_channel(k, c, f[(size_t)y * g.W + x], u[0], u[g.csize]);
}

}  // namespace kvq
