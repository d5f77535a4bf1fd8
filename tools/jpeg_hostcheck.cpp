// Stand-alone check of csrc/jpeg.cpp under the host sanitizers: no HIP, no Python.  Every JPEG file named on the command line goes
// through kvq_jpeg_probe; a decodable one through kvq_jpeg_coeffs into a heap buffer of exactly kvq_jpeg_coef_bytes (an overrun is
// the sanitizer's to catch) and through kvq_jpeg_idct_i420_host, then EVERY byte-length prefix of it — each in a heap copy of exactly
// that length, so a read past the prefix is caught too — must come back as an error; a refused one must be KVQ_ERR_UNSUPPORTED from
// both entries.  Random coefficients over the whole int16 range go through the IDCT twin last (wrap-around, no undefined behaviour).
//
//   mkdir -p /tmp/jpeg_fixtures && python -c "import numpy as np; g = np.load('tests/golden/mjpeg.npz');
//       [g[k].tofile('/tmp/jpeg_fixtures/' + k[:-4] + '.jpg') for k in g.files if k.endswith('_jpg')]"
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include
//       tools/jpeg_hostcheck.cpp kvq-challenge-cvpr-ntire2024_amd/csrc/jpeg.cpp -o /tmp/jpeg_hostcheck
//   /tmp/jpeg_hostcheck /tmp/jpeg_fixtures/*.jpg
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "jpeg_hostcheck_common.hpp"      // set_error / kvq_last_error (g_err), read_file, read_rgb_planar

static int fail(const char* file, const char* what, long k, int rc) {
  fprintf(stderr, "FAIL %s: %s (prefix %ld, status %d, message '%s')\n", file, what, k, rc, g_err);
  return 1;
}

static int check_file(const char* path) {
  std::vector<uint8_t> data;
  if (!read_file(path, data)) return fail(path, "cannot open", -1, 0);
  KvqJpegInfo info;
  const int rc = kvq_jpeg_probe(data.data(), data.size(), &info);
  uint16_t qt[192];
  if (rc == KVQ_ERR_UNSUPPORTED) {
    int16_t one[64];
    if (kvq_jpeg_coeffs(data.data(), data.size(), one, sizeof(one), qt) != KVQ_ERR_UNSUPPORTED) return fail(path, "refused by the probe only", -1, rc);
    printf("refused  %-28s %s\n", path, g_err);
    return 0;
  }
  if (rc != KVQ_OK || info.frame_bytes != (int64_t)data.size()) return fail(path, "probe", -1, rc);
  const size_t bytes = kvq_jpeg_coef_bytes(info.height, info.width);
  int16_t* coef = (int16_t*)malloc(bytes);
  const size_t fb = (size_t)info.height * info.width + 2 * (size_t)((info.height + 1) / 2) * ((info.width + 1) / 2);
  uint8_t* frame = (uint8_t*)malloc(fb);
  int bad = 0;
  if (kvq_jpeg_coeffs(data.data(), data.size(), coef, bytes, qt) != KVQ_OK) bad = fail(path, "decode", -1, -1);
  if (!bad && kvq_jpeg_idct_i420_host(coef, qt, 1, info.height, info.width, frame) != KVQ_OK) bad = fail(path, "idct", -1, -1);
  if (!bad && kvq_jpeg_coeffs(data.data(), data.size(), coef, bytes - 2, qt) != KVQ_ERR_WORKSPACE) bad = fail(path, "short capacity accepted", -1, -1);
  unsigned sum = 0;
  for (size_t i = 0; i < fb && !bad; ++i) sum = sum * 31u + frame[i];
  for (size_t k = 0; k < data.size() && !bad; ++k) {
    uint8_t* prefix = (uint8_t*)malloc(k ? k : 1);
    memcpy(prefix, data.data(), k);
    const int r = kvq_jpeg_coeffs(prefix, k, coef, bytes, qt);
    if (r != KVQ_ERR_SHAPE || !g_err[0]) bad = fail(path, "a prefix decoded", (long)k, r);
    KvqJpegInfo pi;
    const int pr = kvq_jpeg_probe(prefix, k, &pi);
    if (!(pr == KVQ_ERR_SHAPE || (pr == KVQ_OK && pi.frame_bytes == 0))) bad = fail(path, "a prefix probed as a whole image", (long)k, pr);
    free(prefix);
  }
  free(coef);
  free(frame);
  if (!bad) printf("ok       %-28s %d x %d, restart %d, %zu prefixes, frame checksum %08x\n", path, info.width, info.height, info.restart_interval, data.size(), sum);
  return bad;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s file.jpg ...\n", argv[0]);
    return 2;
  }
  int bad = 0;
  for (int i = 1; i < argc; ++i) bad |= check_file(argv[i]);
  // the IDCT twin on anything an entropy decoder could hand it: whole int16 range x 8-bit quantisers, odd sizes
  uint32_t s = 12345;
  auto next = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
  const int H = 45, W = 70, T = 2;
  const size_t bytes = kvq_jpeg_coef_bytes(H, W);
  std::vector<int16_t> coef(T * bytes / 2);
  std::vector<uint16_t> qt(T * 192);
  std::vector<uint8_t> frames(T * ((size_t)H * W + 2 * 23 * 35));
  for (auto& c : coef) c = (int16_t)(next() & 0xFFFF);
  for (auto& q : qt) q = (uint16_t)(1 + next() % 255);
  if (kvq_jpeg_idct_i420_host(coef.data(), qt.data(), T, H, W, frames.data()) != KVQ_OK) bad |= fail("random coefficients", "idct", -1, -1);
  printf(bad ? "jpeg_hostcheck: FAILED\n" : "jpeg_hostcheck: all clean\n");
  return bad;
}
