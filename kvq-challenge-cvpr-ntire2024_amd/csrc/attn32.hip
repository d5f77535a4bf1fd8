// Window attention for head_dim 32 on gfx950 with the bias PRE-BUILT per (window type, head): 32 x 32 score blocks, running row maximum.
//
// Replaces WindowAttention3D.forward's core (swin_backbone.py:261-322).  The bias of a (window, head) depends only on the block's tables
// and the window's position in the clip, not on the clip: it is built once per weight set and plan geometry by bias32_build_kernel and
// streamed from HBM / L2 (2 B per score; one image per window TYPE: un-shifted windows that differ only in their depth index share one)
// while the kernel is bound by per-score VALU issue.  attn.hip keeps the exact per-score gather path (tables past max |bias| 16, or images
// that would dwarf the activations).  What the kernel is built around:
//   * S^T = K Q^T on v_mfma_f32_32x32x16 (two k-steps of 16 = head_dim 32): a lane holds 16 keys of ONE query (lane & 31) per 32-key
//     block — half the matrix-pipe issue time per flop of a 16 x 16 tiling and a quarter of its LDS fragment reads;
//   * the bias tile (fp16, row-max shifted: the entries that carry the probability mass sit next to 0, where fp16 resolves them to
//     <= 2^-11; the -100 shift mask and the "key >= N" exclusion, -60000, baked in) is widened, scaled by log2(e) and shifted by the row's
//     RUNNING maximum in one v_fma_mix_f32 per score — it is the MFMA's C operand, so the accumulator comes out as the exponent argument:
//     no subtract, no separate conversion.  q arrives scaled by head_dim^-0.5 * log2(e) (the qkv epilogue's scale): S is in log2 units;
//   * the running maximum is the flash-attention scheme with a deferred rescale: a block whose scores stay within 2^THR of the current
//     maximum is exponentiated as it is (P <= 2^THR: fp16 / bf16 hold that at full relative precision, and the normaliser is the sum of the
//     ROUNDED probabilities, so the scale cancels); only a growth past THR — or the row's first block — takes the rescale path (O, l and the
//     scores of the block move by the same 2^-d).  Masked scores (-100) and padding keys leave the exponential as zeros whatever the maximum;
//   * row sums by v_dot2c on the packed probabilities (one VALU per two scores); P V as O^T = V^T P^T with the packed P registers as the B
//     operand and V through the hardware transpose read (row-major V in LDS = a plain copy of the global rows);
//   * the key-block loop is software-pipelined inside the wave: the score MFMAs of block t+1 and the P V MFMAs of block t-1 are in the matrix
//     pipe while the VALU runs max / exp / pack of block t; bias tiles are requested two blocks ahead, the next q-block's ticket, q fragments
//     and first tile while the current one is computed.
// One workgroup (4 waves) per (window, head, clip[, q-part]), three per CU (52 KB of LDS): K (16-B chunks XOR-swizzled by (row >> 2) & 3)
// and V staged once by buffer-resource LDS-DMA (rows past N read zeros), 32-query blocks pulled from an LDS ticket.  FUSED (un-padded
// C = 96 stage): the workgroup computes its own q | k | v from the window's norm1 rows, k / v straight into the LDS images.
//
// Round 4 measured this body in three launch geometries (profiles/r04_attn_ab.txt): this one; a persistent form (one workgroup per CU, a
// loader wave streaming K | V into a three-slot LDS ring ahead of eight consumer waves) that wins alone on the chip with a warm image
// (71 vs 85-90 us at stage 0 un-fused) and loses inside the trunk, where the image is HBM-cold and the late stages hold few units; and the
// 16 x 16 tiling it replaces (attn.hip's dense kernel of rounds 2-3: 475 -> 449 us of attention per 4-clip step).
#include <stdlib.h>

#include "common.hpp"
#include "wave.hpp"

#ifndef A32_ABL
#define A32_ABL 0           // diagnostic builds (tools/ubench/attn32_loop.hip), bit mask: 1 no bias stream, 2 no exponentials, 4 no P V MFMAs,
#endif                      // 8 no growth check, 16 no LDS fragment reads, 32 no v_fma_mix, 64 no row sums, 128 no row-maximum chain
#ifndef A32_SUM
#define A32_SUM 0           // row sums: 0 = v_dot2c on the packed probabilities, 1 = v_pk_add_f32 on the fp32 exponentials (round 5: loop bench 399 -> 392 cycles per block, standalone -1..3 %, 4-lane bench line unchanged; the error against the fp32 softmax grows 1.5x: not taken)
#endif
#if (A32_ABL & 2)
#define A32_EXP(x) ((x) * 0.001f + 1.0f)
#else
#define A32_EXP(x) __builtin_amdgcn_exp2f(x)
#endif

// timing probes of -DKVQ_DIAG builds (garbage scores; profiles/r06_traffic_probes.txt): compiled out of the product library
#ifdef KVQ_DIAG
#define A32_DIAG_FLAG(x) (x)
#else
#define A32_DIAG_FLAG(x) false
#endif

namespace kvq {

constexpr int A32_KB = 13;                         // 32-key blocks: 416 key positions (N <= 400 supported, 392 used)
constexpr int A32_ROWS = 400;                      // key rows the LDS images hold; rows 400..415 of the 13th block come from the zero block
constexpr int A32_K_BYTES = A32_ROWS * 64;         // 25 600: K rows (XOR-swizzled 16-B chunks), then as many of V (row-major)
constexpr int A32_SLOT = 2 * A32_K_BYTES;
constexpr int A32_WAVES = 4;                       // per workgroup (eight: round 5, profiles/r05_attn_geometry_ab.txt)
constexpr int A32_OFF_ZERO = A32_SLOT;             // 1 KB of zeros, then the q-block ticket
constexpr int A32_OFF_CTR = A32_OFF_ZERO + 1024;
constexpr int A32_LDS = A32_OFF_CTR + 16;          // 52 240 B: three workgroups per CU
constexpr int A32_BDEPTH = 2;                      // bias tiles requested ahead of the block being multiplied (3 / 5 / 7 measured: no gain)
constexpr float A32_THR = 8.0f;                    // log2 units: a block is exponentiated against a maximum at most 2^8 too small
constexpr float A32_OFF = -60000.0f;               // padding keys: exp2 underflows to exactly 0

typedef __attribute__((ext_vector_type(4))) short a32_s4;
typedef __attribute__((address_space(3))) a32_s4* a32_tr_t;

// A 32-query block keeps a row in lanes q and q + 32: v_permlane32_swap hands each half the other's value without an LDS round
// trip (new vdst = {own low half, partner's low half}, new vsrc = {partner's high half, own high half}: every lane sees both values)
__device__ __forceinline__ float a32_pair_max(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float a32_pair_sum(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// One 32-query block against the LEN key blocks [t0, t0 + LEN) of the LDS images at `slot`.  Compile-time LENGTH: the score / probability /
// bias registers rotate through statically indexed sets (by t - t0); the first block `t0` may be a run-time value — it only offsets the K
// fragment base, the V transpose-read base and the bias tile pointer.  LAST: the range ends at block 12, the one block whose handling is
// tied to its absolute index (rows 400..415 from the zero block, the SHORT registers, the two V fragments nobody reads); t0 is then 13 - LEN.
// SHORT (round 6; N = 385..392, i.e. the (8,7,7) window): the 13th key block holds 8 valid keys, and they are registers 0..3 of both lane halves
// (key = 384 + (r & 3) + 8 (r >> 2) + 4 hi) — its bias widening, row maximum, exponentials, packs and row sums run on those four registers only
// (16 of the block's 56 VALU instructions; the MFMAs are whole tiles either way).  A KERNEL-level template argument: a launch holds one form of
// the body (round 5's run-time select between both forms in one kernel cost more in code size than the short block saved).

// normalise + store.  Lane (query q, half hi) holds features 8j + 4hi .. +3, j = 0..3: four 8-byte pieces of the row's 64 bytes,
// interleaved with the partner lane's.  Two v_permlane32_swap per dword pair hand lane q features 0..15 and lane q + 32 features
// 16..31: two 16-byte stores of 32 contiguous bytes per lane instead of four 8-byte ones (the store tail is issue-bound).
// `ls` = the ROW's sum (both halves).
template <typename E>
__device__ __forceinline__ void a32_finish(const f32x16& O, float ls, uint16_t* orow, const bool store) {
  const int hi = (threadIdx.x & 63) >> 5;
  const float inv = __builtin_amdgcn_rcpf(ls);          // >= 2^-THR-ish and finite: the row maximum contributes >= 2^-THR
  uint32_t pk[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    pk[j][0] = E::pack2(O[4 * j] * inv, O[4 * j + 1] * inv);
    pk[j][1] = E::pack2(O[4 * j + 2] * inv, O[4 * j + 3] * inv);
  }
  u32x4 w0, w1;
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    // swap(vdst = piece j, vsrc = piece j + 2): low lanes end with {own piece j, partner's piece j}, high lanes with {partner's piece
    // j + 2, own piece j + 2} — in both cases consecutive features
    const auto a = __builtin_amdgcn_permlane32_swap(pk[0][d], pk[2][d], false, false);
    const auto b = __builtin_amdgcn_permlane32_swap(pk[1][d], pk[3][d], false, false);
    w0[d] = a[0]; w0[2 + d] = a[1];
    w1[d] = b[0]; w1[2 + d] = b[1];
  }
  if (store) {
    *reinterpret_cast<u32x4*>(orow + 16 * hi) = w0;
    *reinterpret_cast<u32x4*>(orow + 16 * hi + 8) = w1;
  }
}

template <typename E, int LEN, bool LAST, bool SHORT = false>
__device__ __forceinline__ void a32_qblock(const unsigned char* slot, const int zero, const u32x4* bd0, const int t0, const typename E::v8 qf0,
                                           const typename E::v8 qf1, const u32x4 (&pre)[2], uint16_t* orow, const bool store) {
  using V8 = typename E::v8;
  static_assert(LEN >= 1 && LEN <= A32_KB && (LAST || LEN < A32_KB) && (LAST || !SHORT), "key block range");
  constexpr int T0 = 0, T1 = LEN;                    // t below counts from the range's first block
  const int lane = threadIdx.x & 63, q = lane & 31, hi = lane >> 5;
  const float kLog2e = 1.4426950408889634f;
  const int sw = (q >> 2) & 3;
  const u32x4* Ks = reinterpret_cast<const u32x4*>(slot);
  const u32x4* bd = bd0 + t0 * 128;
  const int ka0 = q * 4 + (hi ^ sw) + t0 * 128, ka1 = q * 4 + ((2 + hi) ^ sw) + t0 * 128;          // + 128 per key block
  // the 13th block: rows 384..399 of the slot, then the zero block (`zero` = its offset from the slot, in 16-B units)
  const int kz0 = q < 16 ? ka0 + (LEN - 1) * 128 : zero + (q - 16) * 4 + (hi ^ sw), kz1 = q < 16 ? ka1 + (LEN - 1) * 128 : zero + (q - 16) * 4 + ((2 + hi) ^ sw);
  const a32_tr_t vtr = (a32_tr_t)(slot + A32_K_BYTES + (4 * hi + ((lane & 15) >> 2)) * 64 + ((lane >> 4) & 1) * 32 + (lane & 3) * 8) + t0 * 256;
  const uint32_t one2 = (uint32_t)E::cvt(1.0f) * 0x10001u;

  constexpr int BR = A32_BDEPTH + 1;
  constexpr int LASTB = LAST ? LEN - 1 : -1;         // the range's index of block 12, if it holds it
#define A32_NR(t) ((SHORT && (t) == LASTB) ? 4 : 16)      // live score registers of key block t
  u32x4 braw[BR][2];
  auto load_bias = [&](int t) __attribute__((always_inline)) {
#if (A32_ABL & 1)     // diagnostic: no bias stream (one tile, loaded once per q-block)
    if (t != T0) { braw[t % BR][0] = braw[T0 % BR][0]; braw[t % BR][1] = braw[T0 % BR][1]; return; }
#endif
    braw[t % BR][0] = bd[t * 128];
    if (A32_NR(t) > 8) braw[t % BR][1] = bd[t * 128 + 64];
  };
  // C operand of block t: bias * log2(e) - m, straight from the packed fp16 pairs (v_fma_mix_f32)
  auto mix = [&](int t, float nm, const f32x16& stale) __attribute__((always_inline)) -> f32x16 {
    f32x16 c;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (r >= A32_NR(t)) { c[r] = stale[r]; continue; }      // rows of padding keys, never read: whatever the destination registers hold (no moves)
      const uint32_t u = braw[t % BR][r >> 3][(r & 7) >> 1];
      const _Float16 hv = __builtin_bit_cast(_Float16, (uint16_t)((r & 1) ? (u >> 16) : (u & 0xffffu)));
      c[r] = (A32_ABL & 32) ? nm : __builtin_fmaf((float)hv, kLog2e, nm);
    }
    return c;
  };
  auto kfrag = [&](int t, int m) __attribute__((always_inline)) -> V8 {
    if (t == LASTB) return __builtin_bit_cast(V8, Ks[(m ? kz1 : kz0)]);          // key rows 400..415 come from the zero block
    return __builtin_bit_cast(V8, Ks[(m ? ka1 : ka0) + ((A32_ABL & 16) ? 0 : t) * 128]);
  };

  f32x16 S[2];
  uint32_t P[2][8];
  a32_s4 vf[2][4];                                                            // V fragments of block t: read during block t, used by P V one block later
  f32x16 O;
#pragma unroll
  for (int r = 0; r < 16; ++r) O[r] = 0.f;
  float ls = 0.f, ls1 = 0.f, nm = 0.f;                                        // nm = -(running maximum), log2 units
  f32x2 lv0 = {0.f, 0.f}, lv1 = {0.f, 0.f};                                   // A32_SUM == 1: the row sum as two packed fp32 chains

  braw[T0 % BR][0] = pre[0]; braw[T0 % BR][1] = pre[1];        // block T0: requested while the previous q-block was computed
#pragma unroll
  for (int a = 1; a < A32_BDEPTH; ++a)
    if (T0 + a < T1) load_bias(T0 + a);
  {
    const V8 k0 = kfrag(T0, 0), k1 = kfrag(T0, 1);
    const f32x16 c = mix(T0, 0.f, O);
    S[T0 & 1] = E::mfma32(k0, qf0, c);
    S[T0 & 1] = E::mfma32(k1, qf1, S[T0 & 1]);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int t = T0; t <= T1; ++t) {
    const int cur = t & 1, nxt = cur ^ 1;
    // ---- requests first: K fragments of block t+1, V fragments of block t, the bias of block t+2 ----
    V8 kn0, kn1;
    if (t + 1 < T1) { kn0 = kfrag(t + 1, 0); kn1 = kfrag(t + 1, 1); }
    if (t < T1 && !((A32_ABL & 16) && t > T0)) {
      vf[cur][0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(vtr + t * 256);
      vf[cur][1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(vtr + t * 256 + 64);
      if (t != LASTB) {                                  // keys 400..415 are padding whatever N <= 400 is: their probabilities are zeros
        vf[cur][2] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(vtr + t * 256 + 128);
        vf[cur][3] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(vtr + t * 256 + 192);
      }
    }
    if (t + A32_BDEPTH < T1) load_bias(t + A32_BDEPTH);
    // ---- P V of block t-1 in the matrix pipe under the row maximum of block t (two new scores per v_max3_f32) ----
    float mx = 0.f;
    if (t > T0 && !(A32_ABL & 4))
      O = E::mfma32(__builtin_bit_cast(V8, __builtin_shufflevector(vf[(A32_ABL & 16) ? (T0 & 1) : nxt][0], vf[(A32_ABL & 16) ? (T0 & 1) : nxt][1], 0, 1, 2, 3, 4, 5, 6, 7)),
                    __builtin_bit_cast(V8, (u32x4){P[nxt][0], P[nxt][1], P[nxt][2], P[nxt][3]}), O);
    if (t < T1) {
      mx = fmaxf(fmaxf(S[cur][0], S[cur][1]), S[cur][2]);
#pragma unroll
      for (int r = 3; r < ((A32_ABL & 128) ? 4 : A32_NR(t) - 1); r += 2) mx = fmaxf(fmaxf(mx, S[cur][r]), S[cur][r + 1]);
      mx = fmaxf(mx, S[cur][A32_NR(t) - 1]);
    }
    if (t > T0 && t - 1 != LASTB && !(A32_ABL & 4))
      O = E::mfma32(__builtin_bit_cast(V8, __builtin_shufflevector(vf[(A32_ABL & 16) ? (T0 & 1) : nxt][2], vf[(A32_ABL & 16) ? (T0 & 1) : nxt][3], 0, 1, 2, 3, 4, 5, 6, 7)),
                    __builtin_bit_cast(V8, (u32x4){P[nxt][4], P[nxt][5], P[nxt][6], P[nxt][7]}), O);
    if (t == T1) break;
    __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
    __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    if (t == T0 || (!(A32_ABL & 8) && __builtin_amdgcn_ballot_w64(mx > A32_THR) != 0)) {
      // rescale path: the row's first block (exact maximum) or a growth past THR.  Everything still at the old maximum moves by
      // the same 2^-d: O and l (they hold blocks .. t-1 completely) and the scores of block t; block t+1's C operand is built below
      const float mr = a32_pair_max(mx);                            // the row lives in lanes q and q + 32
      const float d = (t == T0 || mr > A32_THR) ? mr : 0.f;
#pragma unroll
      for (int r = 0; r < A32_NR(t); ++r) S[cur][r] -= d;
      if (t != T0) {                       // the first block: O = l = 0, and 2^-d may be infinite (a masked row start)
        const float f = __builtin_amdgcn_exp2f(-d);
#pragma unroll
        for (int r = 0; r < 16; ++r) O[r] *= f;
        ls *= f;
        ls1 *= f;
        lv0 *= f;
        lv1 *= f;
      }
      nm -= d;
    }
    // ---- the score block t+1 in the matrix pipe under exp / pack / row sum of block t ----
    if (t + 1 < T1) {
      const f32x16 cn = mix(t + 1, nm, S[nxt]);
      S[nxt] = E::mfma32(kn0, qf0, cn);
    }
#if A32_SUM == 1
    // row sums on the fp32 exponentials, two per v_pk_add_f32, two chains (the v_dot2c form on the packed pairs cost 53 of the body's
    // 400 cycles per block in the loop bench).  The normaliser is then the sum of the UN-rounded probabilities: against the sum of the
    // rounded ones it differs by the mean of N independent 16-bit roundings, 2^-12 / sqrt(N) relative for fp16
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x2 e = {A32_EXP(S[cur][2 * i]), A32_EXP(S[cur][2 * i + 1])};
      P[cur][i] = E::pack2_raw(e[0], e[1]);
      if (!(A32_ABL & 64) || i == 0) { if (i & 1) lv1 += e; else lv0 += e; }
    }
    if (t + 1 < T1) S[nxt] = E::mfma32(kn1, qf1, S[nxt]);
#pragma unroll
    for (int i = 4; i < 8; ++i) {
      const f32x2 e = {A32_EXP(S[cur][2 * i]), A32_EXP(S[cur][2 * i + 1])};
      P[cur][i] = E::pack2_raw(e[0], e[1]);
      if (!(A32_ABL & 64)) { if (i & 1) lv1 += e; else lv0 += e; }
    }
#else
#pragma unroll
    for (int i = 0; i < 4; ++i) P[cur][i] = 2 * i < A32_NR(t) ? E::pack2_raw(A32_EXP(S[cur][2 * i]), A32_EXP(S[cur][2 * i + 1])) : 0u;
    if (t + 1 < T1) S[nxt] = E::mfma32(kn1, qf1, S[nxt]);
#pragma unroll
    for (int i = 4; i < 8; ++i) P[cur][i] = 2 * i < A32_NR(t) ? E::pack2_raw(A32_EXP(S[cur][2 * i]), A32_EXP(S[cur][2 * i + 1])) : 0u;
#pragma unroll
    for (int i = 0; i < ((A32_ABL & 64) ? 1 : A32_NR(t) / 2); i += 2) {          // two chains: v_dot2c accumulates in place
      ls = E::dot2(P[cur][i], one2, ls);
      ls1 = E::dot2(P[cur][i + 1], one2, ls1);
    }
#endif
    if (t + 1 < T1) {
      __builtin_amdgcn_sched_group_barrier(0x002, 16, 1);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);
      __builtin_amdgcn_sched_group_barrier(0x002, 12, 1);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  ls += ls1;
  if (A32_SUM == 1) ls = (lv0[0] + lv0[1]) + (lv1[0] + lv1[1]);
  ls = a32_pair_sum(ls);                                 // the row lives in lanes q and q + 32
  a32_finish<E>(O, ls, orow, store);
#undef A32_NR
}

struct Attn32Params {
  const uint16_t* qkv;         // [3][nH][BW*N][32], q scaled by head_dim^-0.5 * log2(e)
  const u32x4* image;          // [n_types*nH][ceil(N/32)][13][2][64 lanes] x 16 B (kvq_attn_bias32_build)
  int BW, nW, N, nH, n_types, qsplit;
  uint16_t* out;               // [BW*N][nH*32]
  const uint32_t* tile_skip;   // optional [nW]: bit t = rows 16t..16t+15 of the window are padding only
  int dsplit_from;             // >= 0: windows >= it are depth-split at token 196 of 392
  const uint8_t* ranges;       // optional [nW][13][2]: first and last 32-key block q-block qb of window w needs (kvq_attn32_key_ranges)
  // fused qkv projection (x_ln != NULL)
  const uint16_t* x_ln;        // [BW*N][C] 16-bit, window order
  const uint16_t* w_qkv;       // [3C][C]
  const float* b_qkv;          // [3C]
  float q_scale;               // head_dim^-0.5 * log2(e)
  uint16_t* q_out;             // = the q third of qkv
  const uint32_t* pad_mask;    // optional [nW][13]: bit r & 31 of word r >> 5 = window row r is a padding row (k | v = b_qkv's thirds, q = 0)
  bool no_q_store;             // -DKVQ_DIAG timing probe (KVQ_NO_Q_STORE=1): the fused projection does not write q (garbage scores: the q scratch's write-back gone)
  bool image_one;              // -DKVQ_DIAG timing probe (KVQ_IMAGE_ONE_TYPE=1): every window reads the images of type 0 — garbage scores, the images' traffic gone
};

// q | k | v of one (window, head) from the window's norm1 rows (C = 32 KS): D^T[feature][row] = W[feature][:] . x[row][:] on
// v_mfma_f32_16x16x32 — a lane ends up with 4 consecutive features of one row: + bias (q: x q_scale), the 16-bit rounding the qkv GEMM's
// epilogue applies, then 8 bytes into the K image (rows of 64 B, 16-B chunks XOR-swizzled by (row >> 2) & 3), the V image (plain rows) or
// the q scratch.  Wave w takes row tiles w, w + 4, ...; all six 16-feature column tiles (q0 q1 k0 k1 v0 v1) in one pass over the rows.
template <typename E, int KS>
__device__ __forceinline__ void a32_fused_qkv(const Attn32Params& p, unsigned char* slot, int bw, int h, int N) {
  using V8 = typename E::v8;
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int C = KS * 32;
  const size_t Mtot = (size_t)p.BW * N;
  const uint16_t* xw = p.x_ln + (size_t)bw * N * C;
  uint16_t* qo = p.q_out + ((size_t)h * Mtot + (size_t)bw * N) * 32;
  V8 wf[6][KS];
  float bias[6][4];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const int which = c >> 1, half = c & 1, frow = which * C + h * 32 + half * 16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) wf[c][ks] = *reinterpret_cast<const V8*>(p.w_qkv + (size_t)(frow + j) * C + 32 * ks + 8 * g);
    const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.b_qkv + frow + 4 * g);
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[c][r] = b4[r];
  }
  const int nrt = (N + 15) / 16;
  V8 xn[KS];
  {
    const int rowc = min(16 * wave + j, N - 1);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) xn[ks] = *reinterpret_cast<const V8*>(xw + (size_t)rowc * C + 32 * ks + 8 * g);
  }
#pragma unroll 1
  for (int rt = wave; rt < nrt; rt += A32_WAVES) {
    const int row = 16 * rt + j;
    V8 xf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) xf[ks] = xn[ks];
    if (rt + A32_WAVES < nrt) {                            // the next tile's rows are requested before this one is multiplied
      const int rowc = min(row + 16 * A32_WAVES, N - 1);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) xn[ks] = *reinterpret_cast<const V8*>(xw + (size_t)rowc * C + 32 * ks + 8 * g);
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const int which = c >> 1, half = c & 1;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = E::mfma16(wf[c][ks], xf[ks], acc);
      const float sc = which == 0 ? p.q_scale : 1.f;
      const u32x2 v = {E::pack2((acc[0] + bias[c][0]) * sc, (acc[1] + bias[c][1]) * sc),
                       E::pack2((acc[2] + bias[c][2]) * sc, (acc[3] + bias[c][3]) * sc)};
      if (row < N) {
        if (which == 0) {
          if (!A32_DIAG_FLAG(p.no_q_store)) *reinterpret_cast<u32x2*>(qo + (size_t)row * 32 + half * 16 + 4 * g) = v;
        } else if (which == 1) {                                   // features 16 half + 4g ..: chunk 2 half + (g >> 1), 8 bytes into it
          *reinterpret_cast<u32x2*>(slot + row * 64 + (((2 * half + (g >> 1)) ^ ((row >> 2) & 3)) << 4) + (g & 1) * 8) = v;
        } else {
          *reinterpret_cast<u32x2*>(slot + A32_K_BYTES + row * 64 + (16 * half + 4 * g) * 2) = v;
        }
      }
    }
  }
}

// Four waves, three workgroups per CU (rounds 4-6).
// MODE: which key blocks a q-block runs against — kAllKeys: all 13; kDepthSplit: dsplit_from's halves; kRanges: the table's range, widened
// outward to the nearest body length the kernel holds (4, 7 or 13 blocks: the extra blocks are masked or padding ones, computed as every
// block was before).  A launch holds the bodies of ONE mode.
enum { kAllKeys = 0, kDepthSplit = 1, kRanges = 2 };
template <typename E, bool FUSED, int MODE, bool SHORT = false>
__global__ __launch_bounds__(A32_WAVES * 64, 3) __attribute__((amdgpu_waves_per_eu(3, 3))) void window_attention32_kernel(Attn32Params p) {
  fp16_saturate_mode();
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int* ticket = reinterpret_cast<int*>(smem + A32_OFF_CTR);
  using V8 = typename E::v8;
  // Block order as attn.hip's dense kernel: the workgroups that share one (window type, head) bias run on the SAME XCD back to back
  // (workgroup b -> XCD b % 8); FUSED: an XCD takes whole window types, heads fastest (they read the same norm1 rows).
  const int nclip = p.BW / p.nW, nrep = p.nW / p.n_types, npair = p.n_types * p.nH, per_pair = nclip * nrep * p.qsplit;
  const int xcd = blockIdx.x & 7, slot_i = blockIdx.x >> 3;
  int pair, clip, rep, part;
  if (FUSED) {
    const int per_type = p.nH * nclip * nrep, wt_ = (slot_i / per_type) * 8 + xcd, sub = slot_i % per_type;
    if (wt_ >= p.n_types) return;
    const int h_ = sub % p.nH, rest = sub / p.nH;
    pair = wt_ * p.nH + h_; clip = rest % nclip; rep = rest / nclip; part = 0;
  } else {
    const int sub = slot_i % per_pair;
    pair = (slot_i / per_pair) * 8 + xcd;
    clip = sub % nclip; rep = (sub / nclip) % nrep; part = sub / (nclip * nrep);
  }
  if (pair >= npair) return;
  const int wt = pair / p.nH, h = pair - wt * p.nH, w = rep * p.n_types + wt, bw = clip * p.nW + w;
  const int tid = threadIdx.x, lane = tid & 63, N = p.N, nqb = (N + 31) >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t Mtot = (size_t)p.BW * N;
  const int C = p.nH * 32;
  const uint16_t* Qg = p.qkv + ((size_t)h * Mtot + (size_t)bw * N) * 32;

  // kRanges: lane qb of every wave holds q-block qb's widened range, t0 | len << 8 — read once per wave, ahead of the K | V staging, and
  // handed out by v_readlane: no load stands between a ticket and the first bias tile of its q-block
  int range_of_lane = 0;
  if (MODE == kRanges) {
    const uint8_t* rg = p.ranges + ((size_t)w * A32_KB + min(lane, A32_KB - 1)) * 2;
    const int first = rg[0], need = (int)rg[1] - first + 1;
    const int len = need <= 4 ? 4 : need <= 7 ? 7 : A32_KB;
    range_of_lane = min(first, A32_KB - len) | (len << 8);
  }
  if (tid < 64) *reinterpret_cast<u32x4*>(smem + A32_OFF_ZERO + tid * 16) = (u32x4){0u, 0u, 0u, 0u};
  if (FUSED) {
    // rows N..399 of both images: zeros (the projection writes rows < N only)
    for (int i = tid; i < (A32_ROWS - N) * 8; i += A32_WAVES * 64)
      *reinterpret_cast<u32x4*>(smem + (i & 4 ? A32_K_BYTES : 0) + (N + (i >> 3)) * 64 + (i & 3) * 16) = (u32x4){0u, 0u, 0u, 0u};
    a32_fused_qkv<E, 3>(p, smem, bw, h, N);
  } else {
    // K | V by buffer-resource LDS-DMA (rows past N read zeros): K with its 16-B chunks XOR-swizzled by (row >> 2) & 3, V as it lies
    const uint16_t* Kg = p.qkv + ((size_t)(1 * p.nH + h) * Mtot + (size_t)bw * N) * 32;
    const uint16_t* Vg = p.qkv + ((size_t)(2 * p.nH + h) * Mtot + (size_t)bw * N) * 32;
    const __amdgpu_buffer_rsrc_t rk = make_rsrc(Kg, (unsigned)(N * 64));
    const __amdgpu_buffer_rsrc_t rv = make_rsrc(Vg, (unsigned)(N * 64));
    const unsigned vo_k = (unsigned)(lane >> 2) * 64u + (unsigned)((lane & 3) ^ ((lane >> 4) & 3)) * 16u, vo_v = (unsigned)lane * 16u;
    for (int it = wave; it < A32_ROWS / 16; it += A32_WAVES) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (lds_ptr_t)(smem + it * 1024), 16, vo_k, it * 1024, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (lds_ptr_t)(smem + A32_K_BYTES + it * 1024), 16, vo_v, it * 1024, 0, 0);
    }
  }
  const int q_lo = part * nqb / p.qsplit, q_hi = (part + 1) * nqb / p.qsplit;
  if (tid == 0) *ticket = q_lo;
  wait_vmcnt<0>();
  __syncthreads();
  if (!FUSED && p.pad_mask) {
    // padded partition: the padding rows of the window are keys with k | v = qkv(0) = the bias (swin_backbone.py:416-449); their rows of
    // the qkv buffer were never written — the images get the 16-bit rounding of the bias here (thread = one 16-B chunk of a row)
    const uint32_t* pm = p.pad_mask + (size_t)w * A32_KB;
    const int c = tid & 3;
    const float* kb = p.b_qkv + C + h * 32 + 8 * c;
    const float* vb = p.b_qkv + 2 * C + h * 32 + 8 * c;
    const u32x4 kc = {E::pack2(kb[0], kb[1]), E::pack2(kb[2], kb[3]), E::pack2(kb[4], kb[5]), E::pack2(kb[6], kb[7])};
    const u32x4 vc = {E::pack2(vb[0], vb[1]), E::pack2(vb[2], vb[3]), E::pack2(vb[4], vb[5]), E::pack2(vb[6], vb[7])};
    for (int r = tid >> 2; r < N; r += A32_WAVES * 16)
      if ((pm[r >> 5] >> (r & 31)) & 1u) {
        *reinterpret_cast<u32x4*>(smem + r * 64 + ((c ^ ((r >> 2) & 3)) << 4)) = kc;
        *reinterpret_cast<u32x4*>(smem + A32_K_BYTES + r * 64 + c * 16) = vc;
      }
    __syncthreads();
  }

  const int q = lane & 31, hi = lane >> 5;
  const uint32_t skip = p.tile_skip ? p.tile_skip[w] : 0u;
  const bool dsplit = MODE == kDepthSplit && p.dsplit_from >= 0 && w >= p.dsplit_from;
  // the key blocks [t0, t0 + len) q-block qb runs against
  auto key_range = [&](int qb, int& t0, int& len) __attribute__((always_inline)) {
    t0 = 0; len = A32_KB;
    if (MODE == kDepthSplit && dsplit && qb != 6) { t0 = qb < 6 ? 0 : 6; len = 7; }      // N = 392, halves of 196 tokens: q-block 6 sees both
    if (MODE == kRanges) {
      const int r = __builtin_amdgcn_readlane(range_of_lane, qb);
      t0 = r & 0xff; len = r >> 8;
    }
  };
  auto take = [&]() -> int {
    int qb_;
    do {                                                        // q-blocks whose two 16-row tiles are padding only are passed over
      qb_ = 0;
      if (lane == 0) qb_ = atomicAdd(ticket, 1);
      qb_ = __builtin_amdgcn_readfirstlane(qb_);
    } while (qb_ < q_hi && ((skip >> (2 * qb_)) & 1u) && (((skip >> (2 * qb_ + 1)) & 1u) || 32 * qb_ + 16 >= N));
    return qb_;
  };
  const u32x4* img = p.image + (size_t)(A32_DIAG_FLAG(p.image_one) ? h : pair) * nqb * (A32_KB * 128) + lane;
  // the ticket, the q fragments and the first bias tile of the NEXT q-block are requested while this one is computed
  struct Req { V8 qf0, qf1; u32x4 pre[2]; int t0, len; };
  auto request = [&](int qb, Req& r) __attribute__((always_inline)) {
    const int qrow = min(32 * qb + q, N - 1);
    r.qf0 = *reinterpret_cast<const V8*>(Qg + (size_t)qrow * 32 + 8 * hi);
    r.qf1 = *reinterpret_cast<const V8*>(Qg + (size_t)qrow * 32 + 16 + 8 * hi);
    if (!FUSED && p.pad_mask && ((p.pad_mask[(size_t)w * A32_KB + qb] >> q) & 1u)) {      // a padding row's q was never written: take zero
      r.qf0 = __builtin_bit_cast(V8, (u32x4){0u, 0u, 0u, 0u});
      r.qf1 = r.qf0;
    }
    key_range(min(qb, nqb - 1), r.t0, r.len);                   // the first bias tile of what will run
    const u32x4* bd = img + (size_t)min(qb, nqb - 1) * (A32_KB * 128) + r.t0 * 128;
    r.pre[0] = bd[0]; r.pre[1] = bd[64];
  };
  auto run = [&](int qb, const Req& r) __attribute__((always_inline)) {
    const u32x4* bd = img + (size_t)qb * (A32_KB * 128);
    uint16_t* orow = p.out + ((size_t)bw * N + 32 * qb + q) * C + h * 32;
    const bool store = 32 * qb + q < N;
    const int zero = A32_OFF_ZERO >> 4;
    // a range that ends at block 12 starts at 13 - len; the others start at a run-time block (the depth split's: block 0)
    const int t0 = MODE == kRanges ? r.t0 : 0;
    if (MODE != kAllKeys && r.len == 7) {
      if (r.t0 == A32_KB - 7) a32_qblock<E, 7, true, SHORT>(smem, zero, bd, A32_KB - 7, r.qf0, r.qf1, r.pre, orow, store);
      else a32_qblock<E, 7, false>(smem, zero, bd, t0, r.qf0, r.qf1, r.pre, orow, store);
    } else if (MODE == kRanges && r.len == 4) {
      if (r.t0 == A32_KB - 4) a32_qblock<E, 4, true, SHORT>(smem, zero, bd, A32_KB - 4, r.qf0, r.qf1, r.pre, orow, store);
      else a32_qblock<E, 4, false>(smem, zero, bd, t0, r.qf0, r.qf1, r.pre, orow, store);
    } else {
      a32_qblock<E, A32_KB, true, SHORT>(smem, zero, bd, 0, r.qf0, r.qf1, r.pre, orow, store);
    }
  };
  // ONE inlined body per kind of ticket (rounds 4-5 unrolled the loop twice to rotate two request sets; the copy below is 16 moves per q-block)
  Req cur, nxt;
  int ta = take();
  if (ta < q_hi) request(ta, cur);
  while (ta < q_hi) {
    const int tn = take();
    if (tn < q_hi) request(tn, nxt);
    run(ta, cur);
    ta = tn;
    cur = nxt;
  }
}

// The image builder (one workgroup per (window type, head)): attn.hip's bias arithmetic — idx = code_q - code_k + center,
// b = fma(gate, r - f, f), the shift mask REPLACES it by -100 — minus the row maximum over the un-masked keys, fp16, in the
// kernel's accumulator layout: [qb][kb][half][lane (q = lane & 31, hi = lane >> 5)][8]: register r = 8 half + e of the
// 32 x 32 score block = key 32 kb + (r & 3) + 8 (r >> 2) + 4 hi.
struct Bias32BuildParams {
  const int32_t* tok;
  const float* rpb;
  const float* fpb;
  int table_len, center, nW, N, nH, use_mask;
  uint16_t* out;
  unsigned* max_abs;
};

__global__ __launch_bounds__(256) void bias32_build_kernel(Bias32BuildParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bsm[];
  f32x2* tab = reinterpret_cast<f32x2*>(bsm);
  int2* tokL = reinterpret_cast<int2*>(bsm + (size_t)p.table_len * 8);
  float* rmax = reinterpret_cast<float*>(bsm + (size_t)p.table_len * 8 + (size_t)p.N * 8);
  const int h = blockIdx.x, w = blockIdx.y, tid = threadIdx.x, N = p.N;
  for (int i = tid; i < p.table_len; i += 256) {
    const float r = p.rpb[(size_t)i * p.nH + h];
    const float f = p.fpb ? p.fpb[(size_t)i * p.nH + h] : r;
    tab[i] = (f32x2){f, p.fpb ? r - f : 0.f};
  }
  for (int i = tid; i < N; i += 256) tokL[i] = *reinterpret_cast<const int2*>(p.tok + ((size_t)w * N + i) * 2);
  __syncthreads();
  auto value = [&](int2 tq, int key, bool* masked) -> float {
    const int2 tk = tokL[key];
    const f32x2 e = tab[tq.x - tk.x + p.center];
    const float gate = (float)__builtin_amdgcn_sad_u8((unsigned)(tq.y & 0xffff), (unsigned)(tk.y & 0xffff), 0u);
    *masked = p.use_mask && ((tq.y >> 16) & 0xff) != ((tk.y >> 16) & 0xff);
    return fmaf(gate, e[1], e[0]);
  };
  float big = 0.f;
  for (int qq = tid; qq < N; qq += 256) {
    const int2 tq = tokL[qq];
    float mx = -INFINITY;
    for (int key = 0; key < N; ++key) {
      bool masked;
      const float b = value(tq, key, &masked);
      if (!masked) { mx = fmaxf(mx, b); big = fmaxf(big, fabsf(b)); }
    }
    rmax[qq] = mx;
  }
  if (p.max_abs) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) big = fmaxf(big, __shfl_xor(big, o));
    if ((tid & 63) == 0) atomicMax(p.max_abs, __float_as_uint(big));
  }
  __syncthreads();
  const int nqb = (N + 31) >> 5, lane = tid & 63, wave = tid >> 6, ql = lane & 31, hi = lane >> 5;
  uint16_t* img = p.out + ((size_t)w * p.nH + h) * nqb * A32_KB * 1024;
  for (int tile = wave; tile < nqb * A32_KB * 2; tile += 4) {
    const int half = tile & 1, blk = tile >> 1, qb = blk / A32_KB, kb = blk - qb * A32_KB, qq = 32 * qb + ql;
    const int2 tq = tokL[qq < N ? qq : N - 1];
    const float shift = rmax[qq < N ? qq : N - 1];
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int r = 8 * half + e, key = 32 * kb + (r & 3) + 8 * (r >> 2) + 4 * hi;
      float b = 0.f;
      if (key >= N) {
        b = A32_OFF;
      } else if (qq < N) {
        bool masked;
        b = value(tq, key, &masked);
        if (masked) b = -100.0f;
        b -= shift;
      }
      v[e] = b;
    }
    *reinterpret_cast<u32x4*>(img + (size_t)tile * 512 + lane * 8) =
        (u32x4){Fp16::pack2_raw(v[0], v[1]), Fp16::pack2_raw(v[2], v[3]), Fp16::pack2_raw(v[4], v[5]), Fp16::pack2_raw(v[6], v[7])};
  }
}

template <typename E, bool FUSED, int MODE, bool SHORT>
static int launch_attn32_form(const Attn32Params& p, hipStream_t st) {
  const int nclip = p.BW / p.nW, nrep = p.nW / p.n_types, npair = p.n_types * p.nH;
  unsigned grid = (unsigned)(8 * ceil_div(npair, 8) * nclip * nrep * p.qsplit);
  if (FUSED) grid = (unsigned)(8 * ceil_div(p.n_types, 8) * p.nH * nclip * nrep);      // XCDs take whole window types
  return launch("window_attention32_kernel", window_attention32_kernel<E, FUSED, MODE, SHORT>, dim3(grid), dim3(A32_WAVES * 64), A32_LDS, st, p);
}

template <typename E, bool FUSED, int MODE>
static int launch_attn32(const Attn32Params& p, hipStream_t st) {
  // N = 385..392 (the (8,7,7) window): the 13th key block holds 8 valid keys (SHORT; results agree to the last bit with the generic block)
  return p.N > 384 && p.N <= 392 ? launch_attn32_form<E, FUSED, MODE, true>(p, st) : launch_attn32_form<E, FUSED, MODE, false>(p, st);
}

template <typename E>
static int launch_attn32_e(const Attn32Params& p, hipStream_t st) {
  if (p.ranges) return p.x_ln ? launch_attn32<E, true, kRanges>(p, st) : launch_attn32<E, false, kRanges>(p, st);
  if (p.x_ln) return p.dsplit_from >= 0 ? launch_attn32<E, true, kDepthSplit>(p, st) : launch_attn32<E, true, kAllKeys>(p, st);
  return p.dsplit_from >= 0 ? launch_attn32<E, false, kDepthSplit>(p, st) : launch_attn32<E, false, kAllKeys>(p, st);
}

}  // namespace kvq

extern "C" size_t kvq_attn_bias32_bytes(int n_types, int N, int num_heads) {
  if (n_types <= 0 || N < 1 || N > 400 || num_heads <= 0) return 0;
  return (size_t)n_types * num_heads * ((N + 31) / 32) * kvq::A32_KB * 2048 + 2048;     // + one block: the kernel requests block t0 + 1 unconditionally
}

extern "C" int kvq_attn_bias32_build(const int32_t* tok, const float* rpb, const float* fpb, int table_len, int center,
                                          int nW, int N, int num_heads, int use_mask, void* out, float* max_abs, void* stream) {
  using namespace kvq;
  KVQ_REQUIRE(tok && rpb && out, KVQ_ERR_NULL, "kvq_attn_bias32_build: NULL pointer");
  KVQ_REQUIRE(kvq_attn_bias32_bytes(nW, N, num_heads) > 0 && table_len > 0, KVQ_ERR_SHAPE,
              "kvq_attn_bias32_build: bad shape nW=%d N=%d nH=%d", nW, N, num_heads);
  KVQ_REQUIRE(((size_t)out & 15) == 0, KVQ_ERR_SHAPE, "kvq_attn_bias32_build: out must be 16-byte aligned");
  Bias32BuildParams p{tok, rpb, fpb, table_len, center, nW, N, num_heads, use_mask, (uint16_t*)out, (unsigned*)max_abs};
  const size_t lds = (size_t)table_len * 8 + (size_t)N * 12;
  KVQ_REQUIRE(lds <= 64 * 1024, KVQ_ERR_UNSUPPORTED, "kvq_attn_bias32_build: table of %d entries does not fit the builder's LDS", table_len);
  return launch("bias32_build_kernel", bias32_build_kernel, dim3((unsigned)num_heads, (unsigned)nW), dim3(256), lds, stream, p);
}

// ---- region order and key ranges of shifted windows (host; the plan's and the tests' one source of both) ------------------------------
// A window's rows sorted by the shift-mask region of their descriptor (stable: raster order inside a region): every region is one
// contiguous run of rows, so the keys a 32-query block can see are one contiguous range of 32-key blocks.
extern "C" int kvq_attn32_row_order(const int32_t* tok_host, int n_windows, int N, int32_t* order) {
  KVQ_REQUIRE(tok_host && order, KVQ_ERR_NULL, "kvq_attn32_row_order: NULL pointer");
  KVQ_REQUIRE(n_windows > 0 && N >= 1, KVQ_ERR_SHAPE, "kvq_attn32_row_order: bad shape n_windows=%d N=%d", n_windows, N);
  for (int w = 0; w < n_windows; ++w) {
    const int32_t* tk = tok_host + (size_t)w * N * 2;
    int32_t* o = order + (size_t)w * N;
    int count[257] = {0};                                           // counting sort by the 8-bit region id: stable
    for (int n = 0; n < N; ++n) ++count[((tk[2 * n + 1] >> 16) & 0xff) + 1];
    for (int r = 0; r < 256; ++r) count[r + 1] += count[r];
    for (int n = 0; n < N; ++n) o[count[(tk[2 * n + 1] >> 16) & 0xff]++] = n;
  }
  return KVQ_OK;
}

// ranges[w][qb] = {first, last} 32-key block that holds a key (< N) some valid query row of the block is not masked against, read off the
// descriptors of the rows AS STORED — no geometry formula: whatever the row order, a block outside the range holds only scores the image
// stores as -100 (or padding keys), which leave the exponential as zeros.  Entries of q-blocks past the window's last are the full range.
extern "C" int kvq_attn32_key_ranges(const int32_t* tok_host, int n_windows, int N, int use_mask, uint8_t* ranges) {
  using namespace kvq;
  KVQ_REQUIRE(tok_host && ranges, KVQ_ERR_NULL, "kvq_attn32_key_ranges: NULL pointer");
  KVQ_REQUIRE(n_windows > 0 && N >= 1 && N <= 400, KVQ_ERR_SHAPE, "kvq_attn32_key_ranges: bad shape n_windows=%d N=%d", n_windows, N);
  const int nkb = (N + 31) / 32;
  for (int w = 0; w < n_windows; ++w) {
    const int32_t* tk = tok_host + (size_t)w * N * 2;
    for (int qb = 0; qb < A32_KB; ++qb) {
      int first = 0, last = nkb - 1;
      if (use_mask && qb < nkb) {
        bool in_block[256] = {false};                              // the regions of the block's query rows
        for (int qq = 32 * qb; qq < N && qq < 32 * qb + 32; ++qq) in_block[(tk[2 * qq + 1] >> 16) & 0xff] = true;
        first = nkb; last = -1;
        for (int key = 0; key < N; ++key)
          if (in_block[(tk[2 * key + 1] >> 16) & 0xff]) { first = first < (key >> 5) ? first : key >> 5; last = key >> 5; }
      }
      ranges[((size_t)w * A32_KB + qb) * 2] = (uint8_t)first;
      ranges[((size_t)w * A32_KB + qb) * 2 + 1] = (uint8_t)last;
    }
  }
  return KVQ_OK;
}

static int window_attention32(const char* who, const KvqAttnDenseArgs* a, const uint8_t* ranges, void* stream) {
  using namespace kvq;
  KVQ_REQUIRE(a && a->qkv && a->bias_dense && a->out, KVQ_ERR_NULL, "%s: NULL pointer", who);
  const int BW = a->BW, nW = a->nW, N = a->N, num_heads = a->num_heads, n_types = a->n_types;
  KVQ_REQUIRE(BW > 0 && nW > 0 && BW % nW == 0 && num_heads > 0 && n_types > 0 && nW % n_types == 0, KVQ_ERR_SHAPE,
              "%s: bad shape BW=%d nW=%d n_types=%d nH=%d", who, BW, nW, n_types, num_heads);
  KVQ_REQUIRE(N >= 1 && N <= 400, KVQ_ERR_UNSUPPORTED, "%s: window of %d tokens unsupported (1..400)", who, N);
  KVQ_REQUIRE(((size_t)a->bias_dense & 15) == 0, KVQ_ERR_SHAPE, "%s: the bias image must be 16-byte aligned", who);
  KVQ_REQUIRE_OPERAND(who, a->dtype);
  KVQ_REQUIRE(a->dsplit_from < 0 || (N == 392 && a->dsplit_from < nW), KVQ_ERR_UNSUPPORTED,
              "%s: depth-split windows need the (8,7,7) window (N = 392); got N=%d from=%d", who, N, a->dsplit_from);
  const int units = BW * num_heads, nqb = (N + 31) / 32;
  int qsplit = units >= 768 ? 1 : 768 / units;        // 768 = 256 CUs x 3 resident workgroups
  // Round 5: no q-split by default.  Splitting a (window, head) unit over 2-4 workgroups fills the chip when the launch is alone on it
  // (stages 2-3: 384 / 192 units) and re-stages K | V in every part; in the 4-lane bench line the un-split form is +1.2 % (397.6 -> 402.2
  // videos/s, three alternating pairs, profiles/r05_qsplit_streams_ab.txt): what counts there is CU x time.  KVQ_LATENCY=1: up to 4 (rounds 3-4).
  const int qsplit_max = latency_mode() ? 4 : 1;      // (results do not depend on it)
  qsplit = qsplit > qsplit_max ? qsplit_max : qsplit;
  qsplit = qsplit > nqb ? nqb : qsplit;
  Attn32Params p{a->qkv, (const u32x4*)a->bias_dense, BW, nW, N, num_heads, n_types, qsplit, a->out, a->tile_skip,
                     a->dsplit_from < 0 ? -1 : a->dsplit_from};
#ifdef KVQ_DIAG
  { static const bool one = getenv("KVQ_IMAGE_ONE_TYPE") && atoi(getenv("KVQ_IMAGE_ONE_TYPE")) == 1; p.image_one = one; }
  { static const bool nq = getenv("KVQ_NO_Q_STORE") && atoi(getenv("KVQ_NO_Q_STORE")) == 1; p.no_q_store = nq; }
#endif
  if (a->pad_mask) {
    KVQ_REQUIRE(a->b_qkv && !a->x_ln, KVQ_ERR_NULL, "%s: pad_mask needs b_qkv (and excludes the fused projection)", who);
    p.pad_mask = a->pad_mask; p.b_qkv = a->b_qkv;
  }
  if (a->x_ln) {
    const int C = 32 * num_heads;
    KVQ_REQUIRE(a->w_qkv && a->b_qkv, KVQ_ERR_NULL, "%s: x_ln without w_qkv / b_qkv", who);
    KVQ_REQUIRE(C == 96, KVQ_ERR_UNSUPPORTED, "%s: the fused qkv projection is built for C = 96 (got %d)", who, C);
    KVQ_REQUIRE((((size_t)a->x_ln | (size_t)a->w_qkv | (size_t)a->b_qkv) & 15) == 0, KVQ_ERR_SHAPE,
                "%s: x_ln / w_qkv / b_qkv must be 16-byte aligned", who);
    p.qsplit = 1;       // one workgroup per (window, head) whatever the batch: a block's path must not depend on what shares the launch
    p.x_ln = a->x_ln; p.w_qkv = a->w_qkv; p.b_qkv = a->b_qkv; p.q_scale = a->q_scale; p.q_out = const_cast<uint16_t*>(a->qkv);
  }
  if (ranges) {
    KVQ_REQUIRE(a->dsplit_from < 0 && !a->pad_mask, KVQ_ERR_UNSUPPORTED, "%s: key ranges exclude dsplit_from and pad_mask (un-padded partitions only)", who);
    p.ranges = ranges;
  }
  return with_operand(a->dtype, [&](auto e) { return launch_attn32_e<decltype(e)>(p, (hipStream_t)stream); });
}

extern "C" int kvq_window_attention32(const KvqAttnDenseArgs* a, void* stream) {
  return window_attention32("kvq_window_attention32", a, nullptr, stream);
}

extern "C" int kvq_window_attention32_ranges(const KvqAttnDenseArgs* a, const uint8_t* ranges, void* stream) {
  KVQ_REQUIRE(ranges, KVQ_ERR_NULL, "kvq_window_attention32_ranges: NULL ranges");
  return window_attention32("kvq_window_attention32_ranges", a, ranges, stream);
}
