// What the host and the kernels of csrc/simple_headtrain.hip share: the split of the rows and channels and the workspace layout.
#pragma once
#include <stddef.h>

namespace kvq {

constexpr int SH_HID = 128;        // simpleVQAHead's hidden width: the one that is built
constexpr int SH_SEG = 1024;       // forward: channels of one (row, segment) dot product, one wave each
constexpr int SH_MIN_CHUNK = 32;   // backward: rows of one partial column sum, at least
constexpr int SH_MAX_CHUNKS = 32;  // ... and partials per channel, at most

// The N = B*T feature rows are cut into nchunks runs of `chunk` rows (a multiple of 8; the last may be shorter, none is empty) and the C
// channels into nseg segments of SH_SEG (the last may be shorter), from (B, T, C) alone.
struct SimpleHeadTrainPlan {
  long N;
  int nseg, chunk, nchunks;
  // offsets into the workspace, in floats (each a multiple of 4)
  size_t u, part, g, gpart, total;
};

inline SimpleHeadTrainPlan simple_headtrain_plan(int B, int T, int C) {
  SimpleHeadTrainPlan p;
  p.N = (long)B * T;
  p.nseg = (C + SH_SEG - 1) / SH_SEG;
  long per = (p.N + SH_MAX_CHUNKS - 1) / SH_MAX_CHUNKS;
  per = (per + 7) / 8 * 8;
  if (per < SH_MIN_CHUNK) per = SH_MIN_CHUNK;
  p.chunk = (int)per;
  p.nchunks = (int)((p.N + per - 1) / per);
  p.u = 0;                                                        // u [C] = W1^T w2
  p.part = p.u + (size_t)C;                                       // [N][nseg] dot products of the forward
  p.g = p.part + ((size_t)p.N * p.nseg + 3) / 4 * 4;              // g [C]
  p.gpart = p.g + (size_t)C;                                      // [nchunks][C] partial column sums
  p.total = p.gpart + (size_t)p.nchunks * C;
  return p;
}

}  // namespace kvq
