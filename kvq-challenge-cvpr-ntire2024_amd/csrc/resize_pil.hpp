// Tap tables of kvq_resize_pil (resize_pil.hip): Pillow's Image.resize(size, BILINEAR) on uint8 images, one axis in -> out.  Host code
// only, in double, no HIP dependency: the launch carries the tables as device arrays (kernels.py uploads them once per (in, out)) and
// never derives them, and the host entry kvq_resize_pil_taps (resize_pil.cpp) compiles with the host compiler alone.
//
//   scale = in / out, fs = support = max(scale, 1); output index i: center = (i + 0.5) scale,
//   window [xmin, xmax) = [max(int(center - support + 0.5), 0), min(int(center + support + 0.5), in)),
//   w_j = max(0, 1 - |(j + xmin - center + 0.5) / fs|), normalised by their sum, k_j = (int)(w_j 2^22 + 0.5) ((int)(w_j 2^22 - 0.5) for w_j < 0).
//   One pass: clip8((sum_j px_j k_j + 2^21) >> 22).  The coefficients of an index sum to 2^22 within a few units, so the sum stays
//   below 2^31.
#pragma once
#include <stdint.h>

namespace kvq {

constexpr int PIL_BITS = 22;

struct PilWindow {
  int start, size;
};

static inline double pil_support(int in, int out) {
  const double scale = (double)in / (double)out;
  return scale < 1.0 ? 1.0 : scale;
}

// capacity of one output index's tap list: the window spans at most 2 support + 1 source indices
static inline int pil_kmax(int in, int out) {
  const double s = pil_support(in, out);
  int c = (int)s;
  if ((double)c < s) ++c;
  return 2 * c + 1;
}

static inline PilWindow pil_window(int i, int in, int out) {
  const double scale = (double)in / (double)out, support = pil_support(in, out);
  const double center = ((double)i + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in) xmax = in;
  return PilWindow{xmin, xmax - xmin};
}

// taps of output index i: the window, and its coefficients into k[0 .. size); size <= kmax = pil_kmax(in, out)
static inline PilWindow pil_taps(int i, int in, int out, int kmax, int32_t* k) {
  const double scale = (double)in / (double)out, fs = pil_support(in, out);
  const double center = ((double)i + 0.5) * scale;
  PilWindow win = pil_window(i, in, out);
  if (win.size > kmax) win.size = kmax;          // never binds: the window is at most 2 ceil(support) + 1 wide
  if (win.size < 0) win.size = 0;
  auto weight = [&](int j) {
    double x = ((double)(j + win.start) - center + 0.5) / fs;
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
  };
  double total = 0.0;
  for (int j = 0; j < win.size; ++j) total += weight(j);
  for (int j = 0; j < win.size; ++j) {             // evaluated again, not buffered: the same double both times
    double wj = weight(j);
    if (total != 0.0) wj /= total;
    k[j] = wj < 0.0 ? (int32_t)(wj * (double)(1 << PIL_BITS) - 0.5) : (int32_t)(wj * (double)(1 << PIL_BITS) + 0.5);
  }
  return win;
}

}  // namespace kvq
