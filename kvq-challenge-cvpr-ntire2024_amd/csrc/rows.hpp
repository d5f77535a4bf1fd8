// What the fused token launches (embed.hip, merge.hip, tail.hip, tailmm.hip) and the SlowFast block kernels (bottleneck.hip, slowneck.hip)
// share around the 32 x 32 accumulator: per-channel vectors at its addresses (acc_piece), a token's LayerNorm statistics (token_row_stats),
// and the accumulator-to-row epilogues (tile_store16_pairswap, norm_rows_store, stream_row_store).  wave.hpp, included here, holds what
// knows no layout: pointer types, counted waits, the LDS-DMA image copy, the wave sums.
// A wave holds 32 tokens as the columns of v_mfma_f32_32x32x16: lane (col, h = lane >> 5) owns one token, and register 4 q + e of a
// 32-channel tile is channel 8 q + 4 h + e of it.  The helpers write such tiles out as rows; a kernel hands them a lambda that returns
// the four values of a register group, so its own arithmetic (norm formula, bias, scale, ReLU) stays at the call site.
//
// Sites that stay written out, because through the helper their kernels gained an instruction, a register or scratch (same compile,
// same comparison: profiles/rows_refactor_isa.txt, profiles/token_blocks_refactor_isa.txt):
//   pair swap          tailmm.hip q | k | v panel and norm1 rows, bottleneck.hip output rows (another length, 98 -> 100 VGPRs)
//   lds_dma_image      tail.hip parameter image (+ 2 instructions in all 18 block_tail_kernel: the inlined loop lands in front of the code
//                      behind it and the p.gather test is made twice); tail.hip ring `issue` (a counted number of loads per wave: the
//                      helper's trip count is not a constant, the kernels change length and <*, 3, 4, 2> takes 58 SGPRs for 57);
//                      merge.hip issue_chunk (patch_merge_kernel<*, false, 128 | 192, false> 34 -> 42 SGPRs); slowneck.hip conv_c image
//                      (same size, but the has_tile branch behind the loop is formed from a second compare, not from its saved mask)
//   wave_sum           conv.hip block_sum8 (mean_std_pool_vec8_kernel<Fp16> 606 -> 607 instructions); misc.hip vqa_head_token_kernel's
//                      eight token sums (same size, another schedule: a wait becomes a nop)
//   acc_piece          tail.hip proj bias from the global image (lane half folded into the pointer; block_tail_kernel<*, 3, 4, 2> 152 -> 164
//                      VGPRs); tailmm.hip norm1 gamma | beta (one index for both global vectors; the EMIT kernels change length,
//                      <*, 1, 3, 256> + 11 / + 9 instructions, <*, 1, 4, 256> 48 -> 72 bytes of scratch); tailmm.hip fp16-stream read
//                      (the same address in a 16-bit row, 8 bytes wide)
//   norm_rows_store    merge.hip (the 12 EMIT kernels + 17 .. + 53 instructions, F by reference or by value)
//   stream_row_store   merge.hip residual-stream row with the emit sum t1 in the lambda (+ 266 .. + 1336 instructions, 94 -> 154 | 218 VGPRs;
//                      its loop also carries a scheduling barrier per tile that the helper has not)
//   token_row_stats    merge.hip (shifted one-pass statistics, and a two-pass over outv) and tailmm.hip (cross-wave token_sums) are
//                      other algorithms
#pragma once
#include <stddef.h>

#include "common.hpp"
#include "wave.hpp"

namespace kvq {

// ---- the next block's norm1 rows, emitted by the launch in front of it (EMIT): launch-parameter fields and their validation.
// Packed to its 36 bytes: the member behind it in a kernel's parameters (eps) keeps the slot it had when these five fields were
// declared in place, and with it every kernel its code (the pointers still land on 8-byte offsets).
struct __attribute__((packed, aligned(4))) NextRows {
  const float* nn_w;         // next block's norm1
  const float* nn_b;
  const int32_t* next_dst;   // token -> window row of the next block's partition
  uint16_t* next_ln;         // [n_batch*next_rows][C]
  int next_rows;
};
static_assert(sizeof(NextRows) == 36, "NextRows: five fields, no padding");
// in every parameter struct that embeds it: the pointers stay on 8-byte offsets
#define KVQ_NEXT_ROWS_ALIGNED(S) static_assert(offsetof(S, nr) % 8 == 0, #S "::nr must start on an 8-byte offset")

// from the public argument struct of `entry` (KvqPatchEmbedArgs, KvqPatchMergeArgs, KvqBlockTailArgs)
template <typename A>
static inline int next_rows_fill(NextRows& n, const A* a, const char* entry) {
  KVQ_REQUIRE(!a->next_ln || (a->next_norm_w && a->next_norm_b && a->next_dst && a->next_rows > 0), KVQ_ERR_NULL,
              "%s: next_ln without its norm / map", entry);
  n.nn_w = a->next_norm_w; n.nn_b = a->next_norm_b; n.next_dst = a->next_dst; n.next_ln = (uint16_t*)a->next_ln; n.next_rows = a->next_rows;
  return KVQ_OK;
}

// norm1's gamma | beta as one [2 C] fp32 vector (the s_nn of a kernel: gamma at 0, beta at C): floats 4 tid .. + 3 of it, tid < C / 2
template <int C>
__device__ __forceinline__ const f32x4* next_norm_piece(const NextRows& n, int tid) {
  return reinterpret_cast<const f32x4*>((tid < C / 4 ? n.nn_w : n.nn_b - C) + 4 * tid);
}

// ---- a per-channel fp32 vector at the accumulator layout's addresses: the four values that meet register group q (registers 4 q .. + 3)
// of tile i in lane half h, channels 32 i + 8 q + 4 h .. + 3 of `vec` (LDS or global, 16-byte aligned)
__device__ __forceinline__ f32x4 acc_piece(const float* vec, int i, int q, int h) {
  return *reinterpret_cast<const f32x4*>(vec + 32 * i + 8 * q + 4 * h);
}

// ---- LayerNorm statistics of a token over NT accumulator tiles (C = 32 NT channels), two-pass as ln.hip: in-lane sums, one exchange
// with lane ^ 32, biased variance, eps inside the rsqrt.  `mean` comes back through an opaque copy: without it CSE merges the
// variance pass's (x - mean) with the normalise pass's and keeps C / 2 differences live (spills).
template <int NT>
__device__ __forceinline__ void token_row_stats(const f32x16 (&acc)[NT], float eps, float& mean, float& rstd) {
  constexpr int C = 32 * NT;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int r = 0; r < 16; r += 4) s += (acc[i][r] + acc[i][r + 1]) + (acc[i][r + 2] + acc[i][r + 3]);
  s += __shfl_xor(s, 32);
  mean = s / (float)C;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float d = acc[i][r] - mean;
      sq += d * d;
    }
  sq += __shfl_xor(sq, 32);
  rstd = rsqrtf(sq / (float)C + eps);
  asm volatile("" : "+v"(mean));
}

// ---- one 32-channel tile of a token's 16-bit row, 16 bytes per lane.  val(q) -> the four values of register group q.  The lane pair
// (h = 0 | 1) of a token holds 4 + 4 consecutive channels of every 8; it exchanges the 8-byte pieces of (q, q + 1) by v_permlane32_swap,
// lane h then owns channels 8 (2 t + h) .. + 7 of the tile — half the row-divergent store instructions (one row per cycle in the
// addresser).  Every lane takes part in the swaps; `live` masks the store alone.  FENCE: a scheduling barrier behind every piece.
template <typename E, bool FENCE, typename F>
__device__ __forceinline__ void tile_store16_pairswap(uint16_t* tile_base, int h, bool live, F&& val) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    uint32_t pk[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const f32x4 y = val(2 * t + u);
      pk[u][0] = E::pack2(y[0], y[1]);
      pk[u][1] = E::pack2(y[2], y[3]);
    }
    const auto s0 = __builtin_amdgcn_permlane32_swap(pk[0][0], pk[1][0], false, false);
    const auto s1 = __builtin_amdgcn_permlane32_swap(pk[0][1], pk[1][1], false, false);
    if (live) *reinterpret_cast<u32x4*>(tile_base + 8 * (2 * t + h)) = (u32x4){s0[0], s1[0], s0[1], s1[1]};
    if (FENCE) __builtin_amdgcn_sched_barrier(0);
  }
}

// ---- the next block's norm1 rows: NT tiles through tile_store16_pairswap, val(i, q) -> the normalised register group q of tile i.  The
// kernels' formulas differ on purpose (two fma in tail.hip, (x - mean) rstd g + b in embed.hip, outv in merge.hip), so each keeps its own.
template <typename E, bool FENCE, int NT, typename F>
__device__ __forceinline__ void norm_rows_store(uint16_t* o, int h, bool live, F&& val) {
#pragma unroll
  for (int i = 0; i < NT; ++i)
    tile_store16_pairswap<E, FENCE>(o + 32 * i, h, live, [&](int q) __attribute__((always_inline)) -> f32x4 { return val(i, q); });
}

// ---- NT tiles of a token's residual-stream row from the accumulator layout: fp32 (16 bytes per register group), or F16 with the range
// detector (common.hpp).  `stream` is the base pointer, `off` the element index of the lane's first channel (row * C + 4 h), the
// same in either format; val(i, q) -> register group q of tile i.  `live` masks every store; a caller that has branched on it already
// passes true (embed.hip, tailmm.hip: the per-store test there costs instructions).  Returns the running range maximum (rmax for fp32).
template <bool F16, int NT, typename F>
__device__ __forceinline__ uint32_t stream_row_store(float* stream, size_t off, bool live, uint32_t rmax, F&& val) {
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 y = val(i, q);
      if (F16) {
        const u32x2 v = {Fp16::pack2(y[0], y[1]), Fp16::pack2(y[2], y[3])};
        if (live) {
          *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(stream) + off + 32 * i + 8 * q) = v;
          rmax = range_fold(range_fold(rmax, v[0]), v[1]);
        }
      } else if (live) {
        *reinterpret_cast<f32x4*>(stream + off + 32 * i + 8 * q) = y;
      }
    }
  return rmax;
}

}  // namespace kvq
