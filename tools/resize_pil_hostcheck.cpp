// Stand-alone check of csrc/resize_pil.cpp (kvq_resize_pil_taps, the tap tables of kvq_resize_pil) under the host sanitizers: no HIP,
// no Python.  Every axis of the list — the ones the tests compare with the numpy restatement, plus extremes — is built into heap
// buffers of exactly out and out * kmax entries (an overrun is the sanitizer's to catch); every window must lie inside the axis,
// every coefficient list must sum to 2^22 within its length (one rounding per tap), hold no negative value and be zero past its
// size; 255 times the sum must stay below 2^31 (the kernel accumulates in int32).  Then a white row and a white column go through
// one pass each and must stay white, and the argument checks must refuse what the header says they refuse.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include
//       tools/resize_pil_hostcheck.cpp kvq-challenge-cvpr-ntire2024_amd/csrc/resize_pil.cpp -o /tmp/resize_pil_hostcheck
//   /tmp/resize_pil_hostcheck
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "jpeg_hostcheck_common.hpp"      // set_error / kvq_last_error (g_err)

static int fail(int in, int out, const char* what, long i) {
  fprintf(stderr, "FAIL %d -> %d: %s (index %ld, message '%s')\n", in, out, what, i, g_err);
  return 1;
}

static int check_axis(int in, int out) {
  int32_t K = 0;
  if (kvq_resize_pil_taps(in, out, &K, nullptr, nullptr, nullptr) != KVQ_OK || K < 3) return fail(in, out, "capacity query", K);
  int32_t* start = (int32_t*)malloc(sizeof(int32_t) * (size_t)out);
  int32_t* size = (int32_t*)malloc(sizeof(int32_t) * (size_t)out);
  int32_t* coef = (int32_t*)malloc(sizeof(int32_t) * (size_t)out * K);
  int bad = 0;
  if (kvq_resize_pil_taps(in, out, &K, start, size, coef) != KVQ_OK) bad = fail(in, out, "build", -1);
  int prev_start = 0, prev_end = 0;
  for (int i = 0; i < out && !bad; ++i) {
    const int32_t* k = coef + (size_t)i * K;
    if (start[i] < 0 || size[i] < 1 || size[i] > K || start[i] + size[i] > in) bad = fail(in, out, "window outside the axis", i);
    if (!bad && (start[i] < prev_start || start[i] + size[i] < prev_end)) bad = fail(in, out, "windows do not move forward", i);
    prev_start = start[i];
    prev_end = start[i] + size[i];
    int64_t sum = 0;
    for (int j = 0; j < K && !bad; ++j) {
      if (k[j] < 0) bad = fail(in, out, "negative coefficient", i);
      if (j >= size[i] && k[j] != 0) bad = fail(in, out, "coefficient past the window", i);
      sum += k[j];
    }
    if (!bad && (sum < (1 << 22) - size[i] || sum > (1 << 22) + size[i])) bad = fail(in, out, "coefficients do not sum to 2^22", i);
    if (!bad && 255 * sum + (1 << 21) >= ((int64_t)1 << 31)) bad = fail(in, out, "a white window overflows int32", i);
    // one pass over a white axis stays white
    if (!bad && ((255 * sum + (1 << 21)) >> 22) != 255) bad = fail(in, out, "white does not stay white", i);
  }
  if (!bad) printf("clean    %5d -> %5d  kmax %d\n", in, out, K);
  free(start);
  free(size);
  free(coef);
  return bad;
}

int main() {
  static const int axes[][2] = {{1920, 224}, {1080, 224}, {960, 224}, {540, 224}, {30, 32}, {9, 224}, {224, 224}, {53, 32}, {70, 16}, {45, 16},
                                {3840, 224}, {2160, 224}, {7, 5}, {1, 1}, {1, 7}, {7, 1}, {65535, 3}, {3, 4099}, {4099, 4098}};
  int bad = 0;
  for (const auto& a : axes) bad |= check_axis(a[0], a[1]);
  int32_t K = 0, one = 0;
  if (kvq_resize_pil_taps(4, 4, nullptr, nullptr, nullptr, nullptr) != KVQ_ERR_NULL) bad |= fail(4, 4, "NULL kmax accepted", -1);
  if (kvq_resize_pil_taps(0, 4, &K, nullptr, nullptr, nullptr) != KVQ_ERR_SHAPE) bad |= fail(0, 4, "empty axis accepted", -1);
  if (kvq_resize_pil_taps(4, -1, &K, nullptr, nullptr, nullptr) != KVQ_ERR_SHAPE) bad |= fail(4, -1, "negative axis accepted", -1);
  if (kvq_resize_pil_taps(KVQ_RESIZE_PIL_MAX_AXIS + 1, 4, &K, nullptr, nullptr, nullptr) != KVQ_ERR_SHAPE) bad |= fail(65536, 4, "long axis accepted", -1);
  if (kvq_resize_pil_taps(4, 4, &K, &one, nullptr, nullptr) != KVQ_ERR_NULL) bad |= fail(4, 4, "half a table set accepted", -1);
  if (bad) return 1;
  printf("resize_pil_hostcheck: all clean\n");
  return 0;
}
