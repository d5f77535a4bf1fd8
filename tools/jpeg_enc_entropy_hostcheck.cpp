// Stand-alone check of kvq_jpeg_encode_header and kvq_jpeg_encode_scans_host (csrc/jpeg_enc.cpp through csrc/jpeg_enc_huff.hpp — the
// per-block functions the device launch runs from its lanes) under the host sanitizers: no HIP, no Python.  Every case goes through
// the host twin into heap buffers of EXACTLY the sizes it is told (an overrun of out, of frames_out or of the workspace is the
// sanitizer's to catch), and header + scan + FF D9 must equal what kvq_jpeg_encode writes.  The small cases run again at EVERY capacity
// from 0 to the needed one and at EVERY workspace size from 0 up to kvq_jpeg_scans_workspace_bytes: a status, or a refusal that stores nothing.
// Every file named on the command line is a raw interleaved RGB picture whose name ends in _<H>x<W>_q<quality>.rgb.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include tools/jpeg_enc_entropy_hostcheck.cpp
//       kvq-challenge-cvpr-ntire2024_amd/csrc/jpeg_enc.cpp -o /tmp/jpeg_enc_entropy_hostcheck
//   /tmp/jpeg_enc_entropy_hostcheck /tmp/jpeg_enc_fixtures/*.rgb
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "jpeg_hostcheck_common.hpp"      // set_error / kvq_last_error (g_err), read_file, read_rgb_planar

// int16 coefficients of one frame: 6 blocks of 64 per 16 x 16 MCU (kvq_jpeg_coef_bytes lives in csrc/jpeg.cpp, which this does not link)
static size_t coef_elems(int H, int W) { return (size_t)((H + 15) / 16) * ((W + 15) / 16) * 384; }

static int fail(const char* what, const char* step, long v) {
  fprintf(stderr, "FAIL %s: %s (%ld, message '%s')\n", what, step, v, g_err);
  return 1;
}

// one call into heap buffers of exactly cap, 12 T and ws bytes (the workspace 16-byte aligned, through posix_memalign with its exact size)
struct Run {
  int rc;
  std::vector<uint8_t> out;
  std::vector<uint32_t> frames;
};
static Run run(const int16_t* coef, int T, int H, int W, int ri, size_t cap, size_t ws) {
  Run r;
  uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
  uint32_t* frames = (uint32_t*)malloc(12 * (size_t)T);
  void* work = nullptr;
  if (posix_memalign(&work, 16, ws ? ws : 1) != 0) abort();
  memset(out, 0xA5, cap ? cap : 1);
  memset(frames, 0xA5, 12 * (size_t)T);
  r.rc = kvq_jpeg_encode_scans_host(coef, T, H, W, ri, out, cap, frames, work, ws);
  r.out.assign(out, out + cap);
  r.frames.assign(frames, frames + 3 * (size_t)T);
  free(out); free(frames); free(work);
  return r;
}

// T frames of coefficients; ok[t]: inside baseline's range.  exhaustive: every capacity and every workspace size.  0 = clean
static int check_case(const char* what, const int16_t* coef, int T, int H, int W, const uint16_t* qt, int ri, int flags, bool exhaustive) {
  const size_t per = coef_elems(H, W), bound = kvq_jpeg_encode_bound(H, W);
  const size_t ws_full = kvq_jpeg_scans_workspace_bytes(T, H, W);
  if (!ws_full) return fail(what, "workspace size", (long)ws_full);
  // the header, into exactly its length
  size_t hn = 0, hn2 = 0;
  uint8_t none = 0;
  if (kvq_jpeg_encode_header(qt, H, W, ri, flags, &none, 0, &hn) != KVQ_ERR_WORKSPACE || !hn) return fail(what, "header without capacity accepted", (long)hn);
  std::vector<uint8_t> head(hn);
  if (kvq_jpeg_encode_header(qt, H, W, ri, flags, head.data(), hn, &hn2) != KVQ_OK || hn2 != hn) return fail(what, "header", (long)hn2);
  // what every frame must be
  std::vector<std::vector<uint8_t>> want(T);
  std::vector<uint8_t> image(bound);
  size_t total = 0;
  for (int t = 0; t < T; ++t) {
    size_t n = 0;
    const int rc = kvq_jpeg_encode(coef + (size_t)t * per, qt, H, W, ri, flags, image.data(), bound, &n);
    if (rc == KVQ_OK) {
      if (n < hn + 2 || memcmp(image.data(), head.data(), hn) != 0) return fail(what, "the image does not start with the header", t);
      want[t].assign(image.begin() + hn, image.begin() + n - 2);
    } else if (rc != KVQ_ERR_UNSUPPORTED) return fail(what, "kvq_jpeg_encode", rc);
    total += want[t].size();
  }
  auto verify = [&](const Run& r, size_t cap, const char* step) -> int {
    if (r.rc != KVQ_OK) return fail(what, step, r.rc);
    size_t off = 0;
    for (int t = 0; t < T; ++t) {
      const uint32_t* f = &r.frames[3 * (size_t)t];
      const bool refused = want[t].empty();
      if (f[0] != off || f[1] != want[t].size()) return fail(what, "offset / length", t);
      const uint32_t st = refused ? 1u : (off + want[t].size() > cap ? 2u : 0u);
      if (f[2] != st) return fail(what, "status", (long)f[2]);
      if (st == 0 && memcmp(r.out.data() + off, want[t].data(), want[t].size()) != 0) return fail(what, "scan bytes", t);
      off += want[t].size();
    }
    return 0;
  };
  int bad = verify(run(coef, T, H, W, ri, total, ws_full), total, "exact capacity");
  if (!bad && total) bad = verify(run(coef, T, H, W, ri, total - 1, ws_full), total - 1, "capacity - 1");
  if (!bad && exhaustive) {
    for (size_t cap = 0; cap <= total && !bad; ++cap) bad = verify(run(coef, T, H, W, ri, cap, ws_full), cap, "every capacity");
    for (size_t ws = 0; ws <= ws_full && !bad; ++ws) {      // below what it needs: refused, nothing touched; with it: the scans
      const Run r = run(coef, T, H, W, ri, total, ws);
      if (ws < ws_full) {
        if (r.rc != KVQ_ERR_WORKSPACE || r.frames[0] != 0xA5A5A5A5u) bad = fail(what, "a workspace below the need accepted", (long)ws);
      } else bad = verify(r, total, "the workspace that is enough");
    }
  }
  if (!bad) printf("ok       %-44s %d x %d x %d, restart %d, flags %d, %zu scan bytes%s\n", what, T, W, H, ri, flags, total, exhaustive ? ", exhaustive" : "");
  return bad;
}

static int check_pixels(const char* what, const uint8_t* planar, int T, int H, int W, int quality, int ri, int flags, bool exhaustive) {
  uint16_t qt[192];
  if (kvq_jpeg_quant_tables(quality, qt) != KVQ_OK) return fail(what, "tables", quality);
  std::vector<uint16_t> qts;
  for (int t = 0; t < T; ++t) qts.insert(qts.end(), qt, qt + 192);
  const size_t per = coef_elems(H, W);
  void* mem = nullptr;
  if (posix_memalign(&mem, 16, per * 2 * T) != 0) abort();
  int16_t* coef = (int16_t*)mem;
  int bad = 0;
  if (kvq_jpeg_fdct_host(planar, KVQ_SRC_U8, T, H, W, qts.data(), coef) != KVQ_OK) bad = fail(what, "fdct", 0);
  if (!bad) bad = check_case(what, coef, T, H, W, qt, ri, flags, exhaustive);
  free(coef);
  return bad;
}

static int check_file(const char* path) {
  int H = 0, W = 0, q = 0;
  std::vector<uint8_t> planar;
  if (const char* why = read_rgb_planar(path, H, W, q, planar)) return fail(path, why, 0);
  return check_pixels(path, planar.data(), 1, H, W, q, 0, 0, false);
}

int main(int argc, char** argv) {
  int bad = 0;
  for (int i = 1; i < argc; ++i) bad |= check_file(argv[i]);
  uint32_t s = 12345;
  auto next = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
  // pixels: {T, H, W, quality, restart, flags, exhaustive}
  const int px[][7] = {{1, 16, 16, 75, 0, 0, 1},     {1, 48, 64, 50, 0, 0, 1},  {1, 48, 64, 50, 1, 0, 1},  {1, 48, 48, 100, 1, 0, 0}, {1, 45, 70, 100, 5, 0, 0},
                       {1, 64, 80, 100, 0, 0, 0},    {1, 64, 80, 100, 5, 1, 0}, {1, 45, 70, 75, 100, 0, 0}, {1, 45, 70, 75, 65535, 1, 0}, {2, 16, 32, 100, 1, 0, 1},
                       {3, 272, 480, 75, 0, 0, 0},   {3, 272, 480, 75, 7, 0, 0}, {3, 272, 480, 75, 30, 0, 0}, {1, 7, 9, 90, 0, 0, 1},    {2, 33, 17, 60, 2, 0, 0}};
  for (const auto& c : px) {
    const int T = c[0], H = c[1], W = c[2];
    std::vector<uint8_t> src((size_t)3 * T * H * W);
    const bool grey = c[3] == 50;
    for (auto& v : src) v = grey ? (uint8_t)128 : (uint8_t)next();
    char what[64];
    snprintf(what, sizeof(what), "%s q%d", grey ? "grey" : "noise", c[3]);
    bad |= check_pixels(what, src.data(), T, H, W, c[3], c[4], c[5], c[6] != 0);
  }
  // crafted coefficients, 16 x 32 (two MCUs), natural order inside a block
  uint16_t qt[192];
  kvq_jpeg_quant_tables(50, qt);
  const int H = 16, W = 32;
  const size_t per = coef_elems(H, W);
  void* mem = nullptr;
  if (posix_memalign(&mem, 16, per * 2 * 3) != 0) abort();
  int16_t* coef = (int16_t*)mem;
  // every block 1660 bits: all AC +-1023, DC differences of category 11
  for (size_t b = 0; b < 12; ++b)
    for (int i = 0; i < 64; ++i) coef[b * 64 + i] = (int16_t)(i == 0 ? ((b & 1) ? 0 : 2047) : ((i & 1) ? 1023 : -1023));
  bad |= check_case("every block at its longest", coef, 1, H, W, qt, 0, 0, true);
  memset(coef, 0, per * 2);
  for (size_t b = 0; b < 12; ++b) coef[b * 64 + 63] = (int16_t)(b & 1 ? -1023 : 1);
  bad |= check_case("only position 63", coef, 1, H, W, qt, 1, 0, true);
  memset(coef, 0, per * 2);
  coef[0] = -1024; coef[64] = 1024;
  bad |= check_case("DC difference of 2048: refused", coef, 1, H, W, qt, 0, 0, true);
  // the whole int16 range -> status 1 or coded as kvq_jpeg_encode codes it, three frames a call, never a store past a capacity
  int coded = 0, refused = 0;
  for (int round = 0; round < 48; ++round) {
    for (size_t i = 0; i < 3 * per; ++i) coef[i] = (int16_t)((next() % 7 == 0) ? ((int)(next() & 0xFFFF) - 32768) >> (4 + round % 8) : 0);
    size_t n = 0;
    std::vector<uint8_t> image(kvq_jpeg_encode_bound(H, W));
    for (int t = 0; t < 3; ++t) (kvq_jpeg_encode(coef + t * per, qt, H, W, round % 3, 0, image.data(), image.size(), &n) == KVQ_OK ? coded : refused)++;
    bad |= check_case("random coefficients", coef, 3, H, W, qt, round % 3, 0, round < 4);
  }
  printf("random coefficients: %d frames coded, %d refused as outside baseline\n", coded, refused);
  if (!coded || !refused) bad |= fail("random coefficients", "one of the two outcomes never happened", 0);
  free(coef);
  printf(bad ? "jpeg_enc_entropy_hostcheck: FAILED\n" : "jpeg_enc_entropy_hostcheck: all clean\n");
  return bad;
}
