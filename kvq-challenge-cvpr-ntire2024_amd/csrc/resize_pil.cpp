// kvq_resize_pil_taps: the tap tables of kvq_resize_pil for one axis, built on the host in double (resize_pil.hpp) — the tables
// kernels.py uploads for the launch and the tests compare with the numpy restatement of Pillow's resize (tests/pil_resize_ref.py).
// Plain C++17, no HIP call and no HIP header: tools/resize_pil_hostcheck.cpp builds this file with the host compiler alone under the
// address and undefined-behaviour sanitizers.
#include <stdint.h>

#include "../../include/kvq_hip.h"
#include "jpeg_host.hpp"          // kvq::set_error, declared without a HIP dependency
#include "resize_pil.hpp"

extern "C" int kvq_resize_pil_taps(int in_size, int out_size, int32_t* kmax, int32_t* start, int32_t* size, int32_t* coef) {
  using namespace kvq;
  JPEG_REQUIRE(kmax, KVQ_ERR_NULL, "kvq_resize_pil_taps: NULL kmax");
  JPEG_REQUIRE(in_size > 0 && out_size > 0, KVQ_ERR_SHAPE, "kvq_resize_pil_taps: sizes must be positive");
  JPEG_REQUIRE(in_size <= KVQ_RESIZE_PIL_MAX_AXIS && out_size <= KVQ_RESIZE_PIL_MAX_AXIS, KVQ_ERR_SHAPE,
               "kvq_resize_pil_taps: an axis of %d -> %d is longer than %d", in_size, out_size, KVQ_RESIZE_PIL_MAX_AXIS);
  const int K = pil_kmax(in_size, out_size);
  *kmax = K;
  if (!start && !size && !coef) return KVQ_OK;
  JPEG_REQUIRE(start && size && coef, KVQ_ERR_NULL, "kvq_resize_pil_taps: start / size / coef must all be given");
  for (int i = 0; i < out_size; ++i) {
    int32_t* k = coef + (size_t)i * K;
    for (int j = 0; j < K; ++j) k[j] = 0;
    const PilWindow w = pil_taps(i, in_size, out_size, K, k);
    start[i] = w.start;
    size[i] = w.size;
  }
  return KVQ_OK;
}
