// Stand-alone check of the entropy decode that runs on the device (csrc/jpeg_huff.hpp through kvq_jpeg_entropy_host, and the segment
// index kvq_jpeg_index, both in csrc/jpeg.cpp) under the host sanitizers: no HIP, no Python.  This is how the decoder's memory safety
// on hostile input is established — the kernel is the same header compiled for the device.  Every JPEG file named on the command
// line is taken as it is, then as EVERY byte-length prefix, then with EVERY single byte of its scan replaced by 0x00, by 0xFF and by
// its complement.  Every input lives in a heap copy of exactly its length, its segment table, coefficients and status words in heap
// buffers of exactly their sizes, so that a step outside any of them is the sanitizer's to catch.  For every input:
//   kvq_jpeg_coeffs OK and all statuses 0   =>  the coefficients are equal
//   kvq_jpeg_coeffs not OK                  =>  the index refused, or some status is not 0   (never laxer than the host decoder)
//
//   mkdir -p /tmp/jpeg_fixtures && python -c "import numpy as np; g = np.load('tests/golden/mjpeg.npz');
//       [g[k].tofile('/tmp/jpeg_fixtures/' + k[:-4] + '.jpg') for k in g.files if k.endswith('_jpg')]"
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include
//       tools/jpeg_entropy_hostcheck.cpp kvq-challenge-cvpr-ntire2024_amd/csrc/jpeg.cpp -o /tmp/jpeg_entropy_hostcheck
//   /tmp/jpeg_entropy_hostcheck /tmp/jpeg_fixtures/*.jpg          (files the library does not decode are skipped)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "jpeg_hostcheck_common.hpp"      // set_error / kvq_last_error (g_err), read_file, read_rgb_planar

struct Counts {
  long inputs = 0, both_ok = 0, host_only = 0, refused = 0;
};

// one input of n bytes for a frame of H x W; nseg_cap: the segment capacity the whole file needed.  0: the two assertions hold
static int check_input(const uint8_t* src, size_t n, int H, int W, size_t nseg_cap, Counts& c, const char* what, long k) {
  uint8_t* data = (uint8_t*)malloc(n ? n : 1);
  memcpy(data, src, n);
  const size_t bytes = kvq_jpeg_coef_bytes(H, W);
  int16_t* want = (int16_t*)malloc(bytes);
  int16_t* got = (int16_t*)malloc(bytes);
  uint32_t* segs = (uint32_t*)malloc(nseg_cap * 8);
  KvqJpegTables* tables = (KvqJpegTables*)malloc(sizeof(KvqJpegTables));
  uint16_t qt[192], qt2[192];
  KvqJpegInfo info;
  size_t nseg = 0;
  int bad = 0;
  const int hrc = kvq_jpeg_coeffs(data, n, want, bytes, qt);
  const int irc = kvq_jpeg_index(data, n, &info, segs, nseg_cap, &nseg, tables, qt2);
  bool all_zero = false;
  ++c.inputs;
  if (irc == KVQ_OK && info.width == W && info.height == H) {
    int32_t* status = (int32_t*)malloc(nseg * 4);
    uint32_t* exact = (uint32_t*)malloc(nseg * 8);                   // exactly nseg entries
    memcpy(exact, segs, nseg * 8);
    const uint32_t frame[5] = {0, 0, (uint32_t)nseg, (uint32_t)info.restart_interval, 0};
    if (kvq_jpeg_entropy_host(data, n, frame, exact, nseg, tables, 1, 1, H, W, got, status) != KVQ_OK) bad = 1;
    all_zero = !bad;
    for (size_t s = 0; s < nseg && !bad; ++s) all_zero = all_zero && status[s] == 0;
    free(status);
    free(exact);
  }
  if (bad) {
    fprintf(stderr, "FAIL %s %ld: the host twin returned an error: %s\n", what, k, g_err);
  } else if (hrc == KVQ_OK && all_zero) {
    ++c.both_ok;
    if (memcmp(want, got, bytes) != 0 || memcmp(qt, qt2, sizeof(qt)) != 0) {
      fprintf(stderr, "FAIL %s %ld: both decoded, the coefficients differ\n", what, k);
      bad = 1;
    }
  } else if (hrc == KVQ_OK) {
    ++c.host_only;                                                   // stricter than the host decoder: allowed (the reader falls back)
  } else {
    ++c.refused;
    if (all_zero) {
      fprintf(stderr, "FAIL %s %ld: kvq_jpeg_coeffs refuses it, the index and every segment accept it\n", what, k);
      bad = 1;
    }
  }
  free(tables);
  free(segs);
  free(got);
  free(want);
  free(data);
  return bad;
}

static int check_file(const char* path) {
  std::vector<uint8_t> data;
  if (!read_file(path, data)) {
    fprintf(stderr, "FAIL %s: cannot open\n", path);
    return 1;
  }
  KvqJpegInfo info;
  if (kvq_jpeg_probe(data.data(), data.size(), &info) != KVQ_OK) {
    printf("skipped  %-28s %s\n", path, g_err);
    return 0;
  }
  const int H = info.height, W = info.width;
  std::vector<uint32_t> segs(2 * (kvq_jpeg_coef_bytes(H, W) / 768));
  KvqJpegTables tables;
  uint16_t qt[192];
  size_t nseg = 0;
  if (kvq_jpeg_index(data.data(), data.size(), &info, segs.data(), segs.size() / 2, &nseg, &tables, qt) != KVQ_OK) {
    fprintf(stderr, "FAIL %s: the index refuses the file: %s\n", path, g_err);
    return 1;
  }
  const size_t scan = segs[0];
  Counts c;
  int bad = check_input(data.data(), data.size(), H, W, nseg, c, path, -1);
  if (!bad && c.both_ok != 1) {
    fprintf(stderr, "FAIL %s: the file itself does not decode both ways\n", path);
    bad = 1;
  }
  for (size_t k = 0; k < data.size() && !bad; ++k) bad = check_input(data.data(), k, H, W, nseg, c, "prefix", (long)k);
  std::vector<uint8_t> mod(data);
  for (size_t k = scan; k < data.size() && !bad; ++k) {
    const uint8_t v[3] = {0x00, 0xFF, (uint8_t)~data[k]};
    for (int i = 0; i < 3 && !bad; ++i) {
      if (v[i] == data[k]) continue;
      mod[k] = v[i];
      bad = check_input(mod.data(), mod.size(), H, W, nseg, c, i == 0 ? "byte -> 00" : i == 1 ? "byte -> FF" : "byte -> complement", (long)k);
    }
    mod[k] = data[k];
  }
  if (!bad)
    printf("ok       %-28s %d x %d, restart %d, %zu segments: %ld inputs, %ld decoded both ways and equal, %ld by the host decoder only, "
           "%ld refused by both\n", path, W, H, info.restart_interval, nseg, c.inputs, c.both_ok, c.host_only, c.refused);
  return bad;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s file.jpg ...\n", argv[0]);
    return 2;
  }
  int bad = 0;
  for (int i = 1; i < argc; ++i) bad |= check_file(argv[i]);
  printf(bad ? "jpeg_entropy_hostcheck: FAILED\n" : "jpeg_entropy_hostcheck: all clean\n");
  return bad;
}
