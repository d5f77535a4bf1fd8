// What the four stand-alone check programs of the Motion-JPEG host code (tools/jpeg*_hostcheck.cpp) share: the error text that
// common.cpp provides inside the library, and the reading of their input files.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "kvq_hip.h"

static thread_local char g_err[512] = "";
namespace kvq {
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace kvq
extern "C" const char* kvq_last_error(void) { return g_err; }

// the whole file; false: it cannot be opened
static bool read_file(const char* path, std::vector<uint8_t>& data) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  data.clear();
  uint8_t chunk[4096];
  for (size_t n; (n = fread(chunk, 1, sizeof(chunk), f)) > 0;) data.insert(data.end(), chunk, chunk + n);
  fclose(f);
  return true;
}

// a raw interleaved RGB picture whose name ends in _<H>x<W>_q<quality>.rgb, as R G B planes.  0, or what is wrong with the file
static const char* read_rgb_planar(const char* path, int& H, int& W, int& q, std::vector<uint8_t>& planar) {
  const char* us = strrchr(path, 'x');
  while (us && us > path && us[-1] >= '0' && us[-1] <= '9') --us;
  if (!us || sscanf(us, "%dx%d_q%d.rgb", &H, &W, &q) != 3) return "name does not end in _<H>x<W>_q<quality>.rgb";
  std::vector<uint8_t> rgb;
  if (!read_file(path, rgb)) return "cannot open";
  if (rgb.size() < (size_t)H * W * 3) return "shorter than H x W x 3 bytes";
  planar.resize((size_t)H * W * 3);
  for (size_t i = 0; i < (size_t)H * W; ++i)
    for (int c = 0; c < 3; ++c) planar[(size_t)c * H * W + i] = rgb[3 * i + c];
  return nullptr;
}
