// The ONE definition of the JPEG block reconstruction (dequantise, 8 x 8 inverse DCT, level shift, clamp) that kvq_jpeg_idct_i420
// (jpeg.hip), its scalar twin kvq_jpeg_idct_i420_host (jpeg.cpp) and the numpy restatement (tests/jpeg_ref.py) share, and the
// geometry of the coefficient hand-over between the entropy decoders / coders and the DCT launches (JpegGeom and the two index maps
// below it).  No HIP dependency: jpeg.cpp includes it under the host compiler alone.
//
// Arithmetic: the "slow integer" IDCT of the Independent JPEG Group's library (Loeffler-Ligtenberg-Moschytz, 12 multiplies per 1-D
// pass, constants with CONST_BITS = 13 fractional bits), whose output is what the common decoders produce:
//   d[r][c]  = coef[r][c] * q[r][c]                                                     (natural order, r = vertical frequency)
//   pass 1   : every COLUMN c:  ws[.][c] = (idct8(d[.][c]) + 2^10) >> 11                (keeps PASS1_BITS = 2 fractional bits)
//   pass 2   : every ROW r:     px[r][.] = clamp(((idct8(ws[r][.]) + 2^17) >> 18) + 128, 0, 255)
// idct8 is jpeg_idct8 below: the even part from inputs 0 2 4 6, the odd part from 1 3 5 7, outputs scaled by 2^13 * sqrt(8).
// Every operation is int32 with two's-complement wrap-around (carried out in uint32_t: no undefined behaviour), >> of a negative
// value is arithmetic.
//
// Defined range: the value is the exact-integer evaluation of the formulas whenever the block's dequantised coefficients satisfy
//   sum over the 64 positions of |coef * q| <= 8192
// (no single input's multiplier inside a pass exceeds 2^15, pass-1 outputs are below 5.6 x their column's sum + 1, so no
// intermediate reaches 2^31; the bound is sufficient, not necessary, and covers the DCT of any block of 8-bit samples, whose
// coefficients have an L2 norm <= 1024).  What the entropy decoder can emit (|coef| < 2^15) times an 8-bit quantiser can wrap an
// intermediate: the result is then an UNSPECIFIED value in 0..255 — still the same value in all three implementations — and
// nothing is read or written out of bounds.  The library of the IJG masks its result into a 1024-entry table instead of clamping:
// the two agree for |idct| < 512, which every stream inside the defined range satisfies up to clamped overshoot.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KVQ_JPEG_HD __host__ __device__ inline __attribute__((always_inline))
#define KVQ_JPEG_HD_MEMBER __host__ __device__ inline __attribute__((always_inline))
#else
#define KVQ_JPEG_HD static inline
#define KVQ_JPEG_HD_MEMBER inline
#endif

namespace kvq {

// wrap-around int32 arithmetic
KVQ_JPEG_HD int32_t jw_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
KVQ_JPEG_HD int32_t jw_sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
KVQ_JPEG_HD int32_t jw_mul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
KVQ_JPEG_HD int32_t jw_shl(int32_t a, int n) { return (int32_t)((uint32_t)a << n); }

// One 1-D pass on v[0..7] in place: v[k] <- sum_u c(u) v[u] cos((2k + 1) u pi / 16) * 2^13 * sqrt(8) in fixed point, NOT descaled.
KVQ_JPEG_HD void jpeg_idct8(int32_t v[8]) {
  // even part
  int32_t z1 = jw_mul(jw_add(v[2], v[6]), 4433);                       // FIX(0.541196100)
  const int32_t t2 = jw_add(z1, jw_mul(v[6], -15137));                 // FIX(1.847759065)
  const int32_t t3 = jw_add(z1, jw_mul(v[2], 6270));                   // FIX(0.765366865)
  const int32_t t0 = jw_shl(jw_add(v[0], v[4]), 13), t1 = jw_shl(jw_sub(v[0], v[4]), 13);
  const int32_t t10 = jw_add(t0, t3), t13 = jw_sub(t0, t3), t11 = jw_add(t1, t2), t12 = jw_sub(t1, t2);
  // odd part
  int32_t o0 = v[7], o1 = v[5], o2 = v[3], o3 = v[1];
  z1 = jw_add(o0, o3);
  int32_t z2 = jw_add(o1, o2), z3 = jw_add(o0, o2), z4 = jw_add(o1, o3);
  const int32_t z5 = jw_mul(jw_add(z3, z4), 9633);                     // FIX(1.175875602)
  o0 = jw_mul(o0, 2446);                                               // FIX(0.298631336)
  o1 = jw_mul(o1, 16819);                                              // FIX(2.053119869)
  o2 = jw_mul(o2, 25172);                                              // FIX(3.072711026)
  o3 = jw_mul(o3, 12299);                                              // FIX(1.501321110)
  z1 = jw_mul(z1, -7373);                                              // FIX(0.899976223)
  z2 = jw_mul(z2, -20995);                                             // FIX(2.562915447)
  z3 = jw_add(jw_mul(z3, -16069), z5);                                 // FIX(1.961570560)
  z4 = jw_add(jw_mul(z4, -3196), z5);                                  // FIX(0.390180644)
  o0 = jw_add(o0, jw_add(z1, z3));
  o1 = jw_add(o1, jw_add(z2, z4));
  o2 = jw_add(o2, jw_add(z2, z3));
  o3 = jw_add(o3, jw_add(z1, z4));
  v[0] = jw_add(t10, o3); v[7] = jw_sub(t10, o3);
  v[1] = jw_add(t11, o2); v[6] = jw_sub(t11, o2);
  v[2] = jw_add(t12, o1); v[5] = jw_sub(t12, o1);
  v[3] = jw_add(t13, o0); v[4] = jw_sub(t13, o0);
}

// pass 1 on a column of dequantised coefficients, pass 2 on a row of pass-1 outputs (then v[k] is the sample, 0..255)
KVQ_JPEG_HD void jpeg_idct_pass1(int32_t v[8]) {
  jpeg_idct8(v);
  for (int k = 0; k < 8; ++k) v[k] = jw_add(v[k], 1 << 10) >> 11;
}
KVQ_JPEG_HD void jpeg_idct_pass2(int32_t v[8]) {
  jpeg_idct8(v);
  for (int k = 0; k < 8; ++k) {
    const int32_t s = jw_add(jw_add(v[k], 1 << 17) >> 18, 128);
    v[k] = s < 0 ? 0 : (s > 255 ? 255 : s);
  }
}

// Geometry of one frame's coefficients: 16 x 16 MCUs, mx x my of them; int16 blocks of 64 in natural order, per-plane block raster:
// Y (2 my rows of 2 mx blocks) | Cb (my rows of mx blocks) | Cr.  768 bytes per MCU.
struct JpegGeom {
  int mx, my;          // MCUs across, down
  int ny, nc;          // blocks of the Y plane, of one chroma plane
  int blocks;          // per frame: ny + 2 nc
};
KVQ_JPEG_HD JpegGeom jpeg_geom(int H, int W) {
  JpegGeom g;
  g.mx = (W + 15) >> 4; g.my = (H + 15) >> 4;
  g.nc = g.mx * g.my; g.ny = 4 * g.nc;
  g.blocks = 6 * g.nc;
  return g;
}
static inline bool jpeg_size_ok(int H, int W) { return H > 0 && W > 0 && H <= 65535 && W <= 65535 && (long)H * W < (1L << 28); }

// Scan order -> hand-over: block k (0..5: Y00 Y01 Y10 Y11 Cb Cr) of the MCU in MCU row y, MCU column x, as its index in the frame
KVQ_JPEG_HD uint32_t jpeg_mcu_block(const JpegGeom& g, uint32_t y, uint32_t x, uint32_t k) {
  if (k >= 4u) return (uint32_t)g.ny + (k - 4u) * (uint32_t)g.nc + y * (uint32_t)g.mx + x;
  return (2u * y + (k >> 1)) * (2u * (uint32_t)g.mx) + 2u * x + (k & 1u);
}
// Hand-over -> picture: block b (< g.blocks) of the frame is block (by, bx) of component c's plane
struct JpegPlaneBlock {
  int c, by, bx;
};
KVQ_JPEG_HD JpegPlaneBlock jpeg_plane_block(const JpegGeom& g, int b) {
  JpegPlaneBlock p;
  p.c = b < g.ny ? 0 : (b < g.ny + g.nc ? 1 : 2);
  const int id = p.c == 0 ? b : b - g.ny - (p.c - 1) * g.nc;
  const int bpr = p.c == 0 ? 2 * g.mx : g.mx;
  p.by = id / bpr;
  p.bx = id - p.by * bpr;
  return p;
}

}  // namespace kvq
