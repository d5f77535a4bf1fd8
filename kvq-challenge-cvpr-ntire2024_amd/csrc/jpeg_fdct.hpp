// The ONE definition of the JPEG block analysis (colour conversion, chroma averaging, MCU padding, level shift, 8 x 8 forward DCT,
// quantisation) that kvq_jpeg_fdct (jpeg_enc.hip), its scalar twin kvq_jpeg_fdct_host (jpeg_enc.cpp) and the numpy restatement
// (tests/jpeg_enc_ref.py) share: the mirror of jpeg_idct.hpp, whose geometry, constants and wrap-around helpers it uses.  No HIP
// dependency.  All integers; the values are those of the Independent JPEG Group's library with its default ("slow integer") method,
// to the bit, wherever a sample of the picture is involved.
//
// Source samples, 8-bit:
//   RGB (BT.601 full range, what JFIF fixes; 16 fractional bits):
//     Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//     Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
//     Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
//   chroma planes hold ceil(H/2) x ceil(W/2) samples; sample (cy, cx) = (a + b + c + d + bias) >> 2 over the Cb (Cr) of the pixels
//   (2cy, 2cx), (2cy, 2cx+1), (2cy+1, 2cx), (2cy+1, 2cx+1), bias = 1 in even cx and 2 in odd; a pixel past the last column or row
//   (odd W or H) is the last one.  An I420 source supplies its three planes as they are.
// Padding to whole 16 x 16 MCUs: sample (y, x) of a padded plane is sample (min(y, ph - 1), min(x, pw - 1)) of the plane.
// Per 8 x 8 block s[r][c] (r = row):
//   d[r][c]  = s[r][c] - 128
//   pass 1   : every ROW r:     ws[r][.] = fdct8(d[r][.]), outputs 0 and 4 scaled by 2^2, the others descaled by 2^11 (rounded)
//   pass 2   : every COLUMN c:  F[.][c]  = fdct8(ws[.][c]), outputs 0 and 4 descaled by 2^2, the others by 2^15   -> 8 x the DCT
//   coef[v][u] = sign(F) * ((|F| + (d >> 1)) / d),  d = q[v][u] << 3                    (natural order, v = vertical frequency)
// |F| < 2^15, every multiplicand of a pass stays below 2^18 and no intermediate reaches 2^27.  The division is carried out as a
// multiplication: with m = floor(2^29 / q) + 1 (jpeg_quant_recip: = floor(2^32 / d) + 1, one per table entry, prepared once per
// table) floor(n / d) = (n * m) >> 32 for every n < 2^16 — m d = 2^32 + e with 0 < e <= d, so n m / 2^32 = n / d + n e / (d 2^32)
// and the excess stays below 1 / d while n e < 2^32; here n <= 32767 + 1020 and e <= 2040.  Quantiser entries are 8-bit
// (baseline): 1..255.
#pragma once
#include "jpeg_idct.hpp"

namespace kvq {

// a * c for |a| < 2^23 and a 16-bit constant c, product inside int32.  On the device a is passed through a 24-bit sign extension
// (the identity on such a value): the compiler then takes the full-rate 24-bit multiply instead of the quarter-rate 32-bit one
KVQ_JPEG_HD int32_t jf_mul(int32_t a, int32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return ((int32_t)((uint32_t)a << 8) >> 8) * c;
#else
  return a * c;
#endif
}

// One 1-D pass on v[0..7] in place.  S0: v[0] and v[4] are shifted left (S0 > 0) or descaled (S0 < 0) by |S0| bits; SN: the other
// six are descaled by SN bits.  Pass 1 is <2, 11>, pass 2 <-2, 15>.
KVQ_JPEG_HD int32_t jpeg_descale(int32_t x, int n) { return jw_add(x, 1 << (n - 1)) >> n; }
template <int S0, int SN>
KVQ_JPEG_HD void jpeg_fdct8(int32_t v[8]) {
  const int32_t t0 = v[0] + v[7], t7 = v[0] - v[7], t1 = v[1] + v[6], t6 = v[1] - v[6];
  const int32_t t2 = v[2] + v[5], t5 = v[2] - v[5], t3 = v[3] + v[4], t4 = v[3] - v[4];
  // even part
  const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  v[0] = S0 > 0 ? jw_shl(t10 + t11, S0) : jpeg_descale(t10 + t11, -S0);
  v[4] = S0 > 0 ? jw_shl(t10 - t11, S0) : jpeg_descale(t10 - t11, -S0);
  int32_t z1 = jf_mul(t12 + t13, 4433);                                // FIX(0.541196100)
  v[2] = jpeg_descale(jw_add(z1, jf_mul(t13, 6270)), SN);              // FIX(0.765366865)
  v[6] = jpeg_descale(jw_add(z1, jf_mul(t12, -15137)), SN);            // FIX(1.847759065)
  // odd part
  z1 = t4 + t7;
  int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int32_t z5 = jf_mul(z3 + z4, 9633);                            // FIX(1.175875602)
  const int32_t o4 = jf_mul(t4, 2446);                                 // FIX(0.298631336)
  const int32_t o5 = jf_mul(t5, 16819);                                // FIX(2.053119869)
  const int32_t o6 = jf_mul(t6, 25172);                                // FIX(3.072711026)
  const int32_t o7 = jf_mul(t7, 12299);                                // FIX(1.501321110)
  z1 = jf_mul(z1, -7373);                                              // FIX(0.899976223)
  z2 = jf_mul(z2, -20995);                                             // FIX(2.562915447)
  z3 = jw_add(jf_mul(z3, -16069), z5);                                 // FIX(1.961570560)
  z4 = jw_add(jf_mul(z4, -3196), z5);                                  // FIX(0.390180644)
  v[7] = jpeg_descale(jw_add(o4, jw_add(z1, z3)), SN);
  v[5] = jpeg_descale(jw_add(o5, jw_add(z2, z4)), SN);
  v[3] = jpeg_descale(jw_add(o6, jw_add(z2, z3)), SN);
  v[1] = jpeg_descale(jw_add(o7, jw_add(z1, z4)), SN);
}
// pass 1 on a row of level-shifted samples, pass 2 on a column of pass-1 outputs
KVQ_JPEG_HD void jpeg_fdct_pass1(int32_t v[8]) { jpeg_fdct8<2, 11>(v); }
KVQ_JPEG_HD void jpeg_fdct_pass2(int32_t v[8]) { jpeg_fdct8<-2, 15>(v); }

// the quantiser: q is brought into 1..255 (a table entry outside it is not baseline; the entries that validate refuse it)
KVQ_JPEG_HD uint32_t jpeg_quant_clamp(uint32_t q) { return q < 1u ? 1u : (q > 255u ? 255u : q); }
KVQ_JPEG_HD uint32_t jpeg_quant_recip(uint32_t q) { return (1u << 29) / jpeg_quant_clamp(q) + 1u; }
KVQ_JPEG_HD uint32_t jpeg_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }      // one v_mul_hi_u32
// F = a pass-2 output, |F| <= 32767; recip = jpeg_quant_recip(q), half = 4 q (= (q << 3) >> 1)
KVQ_JPEG_HD int32_t jpeg_quantise(int32_t F, uint32_t recip, uint32_t half) {
  const uint32_t a = (uint32_t)(F < 0 ? -F : F);
  const int32_t m = (int32_t)jpeg_mulhi(a + half, recip);
  return F < 0 ? -m : m;
}

// RGB -> Y, Cb, Cr of one pixel
KVQ_JPEG_HD int32_t jpeg_rgb_y(int32_t r, int32_t g, int32_t b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
KVQ_JPEG_HD int32_t jpeg_rgb_cb(int32_t r, int32_t g, int32_t b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
KVQ_JPEG_HD int32_t jpeg_rgb_cr(int32_t r, int32_t g, int32_t b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// Sample (y, x) of padded plane c (0 Y, 1 Cb, 2 Cr) of frame t, by the rules above.  rgb: planar uint8 (3, T, H, W), else T I420 frames.
KVQ_JPEG_HD int32_t jpeg_src_sample(const uint8_t* src, bool rgb, int T, int H, int W, int t, int c, int y, int x) {
  const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
  const int ph = c == 0 ? H : ch, pw = c == 0 ? W : cw;
  y = y < ph ? y : ph - 1;
  x = x < pw ? x : pw - 1;
  if (!rgb) {
    const size_t frame = (size_t)H * W + 2 * (size_t)ch * cw;
    return src[(size_t)t * frame + (c == 0 ? 0 : (size_t)H * W + (size_t)(c - 1) * ch * cw) + (size_t)y * pw + x];
  }
  const size_t plane = (size_t)T * H * W;
  const uint8_t* r = src + (size_t)t * H * W;
  if (c == 0) {
    const size_t o = (size_t)y * W + x;
    return jpeg_rgb_y(r[o], r[plane + o], r[2 * plane + o]);
  }
  const int y1 = 2 * y + 1 < H ? 2 * y + 1 : H - 1, x1 = 2 * x + 1 < W ? 2 * x + 1 : W - 1;
  int32_t s = 1 + (x & 1);
  for (int k = 0; k < 4; ++k) {
    const size_t o = (size_t)(k < 2 ? 2 * y : y1) * W + ((k & 1) ? x1 : 2 * x);
    s += c == 1 ? jpeg_rgb_cb(r[o], r[plane + o], r[2 * plane + o]) : jpeg_rgb_cr(r[o], r[plane + o], r[2 * plane + o]);
  }
  return s >> 2;
}

}  // namespace kvq
