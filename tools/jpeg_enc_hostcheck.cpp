// Stand-alone check of csrc/jpeg_enc.cpp under the host sanitizers: no HIP, no Python.  Every file named on the command line is a
// raw interleaved RGB picture whose name ends in _<H>x<W>_q<quality>.rgb; it goes through kvq_jpeg_fdct_host into a heap buffer of
// exactly kvq_jpeg_coef_bytes and through kvq_jpeg_encode twice — with no capacity, which must be KVQ_ERR_WORKSPACE and report the
// length, then into a heap buffer of exactly that length (an overrun of either is the sanitizer's to catch) — and back through
// kvq_jpeg_coeffs (csrc/jpeg.cpp), which must return the coefficients and tables that went in.  Random frames of odd sizes from both
// source kinds, with restart markers and without DHT, and coefficients outside baseline's categories go through the same last.
//
//   mkdir -p /tmp/jpeg_enc_fixtures && python -c "import numpy as np; g = np.load('tests/golden/mjpeg_enc.npz');
//       [g[k].tofile('/tmp/jpeg_enc_fixtures/' + k[:-4] + '.rgb') for k in g.files if k.endswith('_rgb')]"
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include tools/jpeg_enc_hostcheck.cpp
//       kvq-challenge-cvpr-ntire2024_amd/csrc/jpeg_enc.cpp kvq-challenge-cvpr-ntire2024_amd/csrc/jpeg.cpp -o /tmp/jpeg_enc_hostcheck
//   /tmp/jpeg_enc_hostcheck /tmp/jpeg_enc_fixtures/*.rgb
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "jpeg_hostcheck_common.hpp"      // set_error / kvq_last_error (g_err), read_file, read_rgb_planar

static int fail(const char* what, const char* step, int rc) {
  fprintf(stderr, "FAIL %s: %s (status %d, message '%s')\n", what, step, rc, g_err);
  return 1;
}

// one frame: src in `format` -> coefficients -> image -> coefficients.  0 = clean
static int check_frame(const char* what, const uint8_t* src, int format, int H, int W, const uint16_t* qt, int restart, int flags) {
  const size_t bytes = kvq_jpeg_coef_bytes(H, W);
  int16_t* coef = (int16_t*)malloc(bytes);
  int16_t* back = (int16_t*)malloc(bytes);
  int bad = 0, rc;
  if ((rc = kvq_jpeg_fdct_host(src, format, 1, H, W, qt, coef)) != KVQ_OK) bad = fail(what, "fdct", rc);
  size_t n = 0, n2 = 0;
  uint8_t none = 0;
  if (!bad && ((rc = kvq_jpeg_encode(coef, qt, H, W, restart, flags, &none, 0, &n)) != KVQ_ERR_WORKSPACE || n == 0)) bad = fail(what, "no capacity accepted", rc);
  if (!bad && n > kvq_jpeg_encode_bound(H, W)) bad = fail(what, "longer than the bound", 0);
  uint8_t* image = (uint8_t*)malloc(n ? n : 1);
  if (!bad && ((rc = kvq_jpeg_encode(coef, qt, H, W, restart, flags, image, n, &n2)) != KVQ_OK || n2 != n)) bad = fail(what, "encode", rc);
  if (!bad && kvq_jpeg_encode(coef, qt, H, W, restart, flags, image, n - 1, &n2) != KVQ_ERR_WORKSPACE) bad = fail(what, "short capacity accepted", 0);
  uint16_t qt_back[192];
  KvqJpegInfo info;
  if (!bad && ((rc = kvq_jpeg_probe(image, n, &info)) != KVQ_OK || info.frame_bytes != (int64_t)n || info.height != H || info.width != W))
    bad = fail(what, "probe of the image", rc);
  if (!bad && (rc = kvq_jpeg_coeffs(image, n, back, bytes, qt_back)) != KVQ_OK) bad = fail(what, "decode of the image", rc);
  if (!bad && (memcmp(coef, back, bytes) != 0 || memcmp(qt, qt_back, sizeof(qt_back)) != 0)) bad = fail(what, "the image does not decode to its input", 0);
  if (!bad) printf("ok       %-40s %d x %d, restart %d, flags %d, %zu bytes\n", what, W, H, restart, flags, n);
  free(coef); free(back); free(image);
  return bad;
}

static int check_file(const char* path) {
  int H = 0, W = 0, q = 0;
  std::vector<uint8_t> planar;
  if (const char* why = read_rgb_planar(path, H, W, q, planar)) return fail(path, why, 0);
  uint16_t qt[192];
  if (kvq_jpeg_quant_tables(q, qt) != KVQ_OK) return fail(path, "tables", 0);
  return check_frame(path, planar.data(), KVQ_SRC_U8, H, W, qt, 0, 0);
}

int main(int argc, char** argv) {
  int bad = 0;
  for (int i = 1; i < argc; ++i) bad |= check_file(argv[i]);
  uint32_t s = 12345;
  auto next = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
  const int sizes[][2] = {{1, 1}, {7, 9}, {16, 16}, {45, 70}, {33, 17}, {64, 31}};
  for (const auto& hw : sizes)
    for (int format : {(int)KVQ_SRC_U8, (int)KVQ_SRC_I420_BT601_FULL}) {
      const int H = hw[0], W = hw[1];
      const size_t n = format == KVQ_SRC_U8 ? (size_t)3 * H * W : (size_t)H * W + 2 * (size_t)((H + 1) / 2) * ((W + 1) / 2);
      uint8_t* src = (uint8_t*)malloc(n);                    // exactly the source's size: a read past it is caught
      for (size_t i = 0; i < n; ++i) src[i] = (uint8_t)next();
      uint16_t qt[192];
      for (auto& q : qt) q = (uint16_t)(2 + next() % 254);   // DC differences stay inside baseline's range for q >= 2
      char what[64];
      snprintf(what, sizeof(what), "random %s", format == KVQ_SRC_U8 ? "RGB" : "I420");
      bad |= check_frame(what, src, format, H, W, qt, (int)(next() % 4), (int)(next() & 1));
      free(src);
    }
  // coefficients an analysis cannot produce: the whole int16 range -> refused or encoded, never a write past the capacity
  const int H = 45, W = 70;
  const size_t bytes = kvq_jpeg_coef_bytes(H, W), cap = kvq_jpeg_encode_bound(H, W);
  int16_t* coef = (int16_t*)malloc(bytes);
  uint8_t* image = (uint8_t*)malloc(cap);
  uint16_t qt[192];
  kvq_jpeg_quant_tables(50, qt);
  int refused = 0, encoded = 0;
  for (int round = 0; round < 64; ++round) {
    for (size_t i = 0; i < bytes / 2; ++i) coef[i] = (int16_t)((next() % 7 == 0) ? (int)(next() & 0xFFFF) - 32768 >> (round % 8) : 0);
    size_t n = 0;
    const int rc = kvq_jpeg_encode(coef, qt, H, W, round % 3, 0, image, cap, &n);
    if (rc == KVQ_ERR_UNSUPPORTED && g_err[0]) ++refused;
    else if (rc == KVQ_OK && n <= cap) ++encoded;
    else bad |= fail("random coefficients", "encode", rc);
  }
  printf("random coefficients: %d images encoded, %d refused as outside baseline\n", encoded, refused);
  if (!encoded || !refused) bad |= fail("random coefficients", "one of the two outcomes never happened", 0);
  free(coef); free(image);
  printf(bad ? "jpeg_enc_hostcheck: FAILED\n" : "jpeg_enc_hostcheck: all clean\n");
  return bad;
}
