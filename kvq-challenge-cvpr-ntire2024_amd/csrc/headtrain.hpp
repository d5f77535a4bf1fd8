// What the host and the kernels of csrc/headtrain.hip share: the dropout mask hash, the chunk plan and the workspace layout.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KVQ_HT_HD __host__ __device__ __forceinline__
#else
#define KVQ_HT_HD inline
#endif

namespace kvq {

// ---- the dropout mask.  Element `idx` (uint32: [b][l][c] order for the dropout in front of fc_hid, which = 0; [b][l][h] order for the one
// behind the GELU, which = 1) of optimisation step `step` under `seed` is KEPT iff  ht_bits(ht_key(seed, step, which), idx) >= ht_threshold(p).
// All arithmetic is uint32 (wrapping).  ht_mix is the 32-bit finaliser of MurmurHash3 with a second key word added between its two
// multiplies, so that two keys do not give xor-shifted copies of one pattern.  A kept value is multiplied by ht_scale(p) = 1 / (1 - p);
// p == 0 keeps everything and scales by exactly 1.  tests/headtrain_ref.py restates this in numpy.
KVQ_HT_HD uint32_t ht_fmix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}
KVQ_HT_HD uint32_t ht_key(uint32_t seed, uint32_t step, uint32_t which) { return ht_fmix(seed ^ ht_fmix(2u * step + which + 0x9E3779B9u)); }
KVQ_HT_HD uint32_t ht_bits(uint32_t key, uint32_t idx) {
  uint32_t x = idx ^ key;
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x += (key << 13) | (key >> 19);
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}
// floor(p * 2^32), p in [0, 1) as the float the caller passed
inline uint32_t ht_threshold(float p) {
  const double t = (double)p * 4294967296.0;
  return t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
}
inline float ht_scale(float p) { return (float)(1.0 / (1.0 - (double)p)); }

// ---- the chunk plan of the backward: the B*L tokens are cut into nchunks runs of `chunk` tokens (a multiple of 16; the last run may be
// shorter, none is empty) from B*L alone; every chunk writes fp32 partial gradients that one launch adds in ascending chunk order.
// db1 and dw2 are cheap per token (no GEMM), so their launch cuts every chunk again into hsub runs of HT_SUB_TOKENS tokens: nsub =
// nchunks * hsub partials in token order (a run past its chunk's end is empty and writes zeros).
constexpr int HT_SUB_TOKENS = 64;
struct HeadTrainPlan {
  long T;           // B * L tokens
  int nchunks, chunk;
  int hsub, nsub;
  // offsets into the workspace, in floats (each a multiple of 4)
  size_t z, dz, tok, part_w1, part_b1, part_w2, total;
};

inline HeadTrainPlan headtrain_plan(int B, int L, int C, int hidden) {
  HeadTrainPlan p;
  p.T = (long)B * L;
  long want = (p.T + 255) / 256;
  if (want > 64) want = 64;
  if (want < 1) want = 1;
  long per = (p.T + want - 1) / want;
  per = (per + 15) / 16 * 16;
  p.chunk = (int)per;
  p.nchunks = (int)((p.T + per - 1) / per);
  p.hsub = (p.chunk + HT_SUB_TOKENS - 1) / HT_SUB_TOKENS;
  p.nsub = p.nchunks * p.hsub;
  const size_t T4 = (size_t)(p.T + 3) / 4 * 4;
  p.z = 0;
  p.dz = p.z + (size_t)p.T * hidden;
  p.tok = p.dz + (size_t)p.T * hidden;
  p.part_w1 = p.tok + T4;
  p.part_b1 = p.part_w1 + (size_t)p.nchunks * hidden * C;
  p.part_w2 = p.part_b1 + (size_t)p.nsub * hidden;
  p.total = p.part_w2 + (size_t)p.nsub * hidden;
  return p;
}

}  // namespace kvq
