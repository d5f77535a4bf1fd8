// What the host halves of the Motion-JPEG code (jpeg.cpp, jpeg_enc.cpp) share beyond the codec itself: the error text and the
// refusal macro.  No HIP dependency.
#pragma once

namespace kvq {
void set_error(const char* fmt, ...);      // common.cpp (tools/jpeg_hostcheck_common.hpp for the stand-alone check programs)
}

#define JPEG_REQUIRE(cond, code, ...)  \
  do {                                 \
    if (!(cond)) {                     \
      kvq::set_error(__VA_ARGS__);     \
      return code;                     \
    }                                  \
  } while (0)
