// One optimisation step of simpleVQAHead on features of a frozen trunk (gfx950): the reference's head (head.py:10-31: Linear(C -> 128),
// Linear(128 -> 1) per frame, no activation, no dropout, then the mean over the frames), the gradients of its four parameters; the losses
// and AdamW + EMA are the launches of headtrain.hip, unchanged.
//
//   features  B rows of a feature bank [n_rows][T][C] in fp32, fp16 or bf16, picked by a device index and widened to fp32 in registers
//             (featbank.hpp): simple_fwd_rows and simple_bwd_g are templates over the element type.  C % 64 == 0, hidden == 128,
//             2 <= B <= 1024.  A dense fp32 batch is an fp32 bank of B rows with the index 0 .. B-1
//   params    one flat fp32 vector: W1 [128][C] | b1 [128] | w2 [128] | b2 [1]; the gradients and the AdamW state have the same layout
//
// The head is linear, so both directions collapse:
//
//   forward   u = W1^T w2 [C];  score[b] = (sum_t X[b,t,:] . u) / T + (w2 . b1 + b2)
//   backward  ds[b,t] = dscore[b] / T;  g = sum_{b,t} ds X[b,t,:] [C];  S = sum_b dscore
//             dW1 = w2 (x) g,  dw2 = W1 g + b1 S,  db1 = w2 S,  db2 = S
//
// X is read once per direction and W1 once per direction; no [rows][128] tensor exists, and the backward needs nothing of the forward.
// Everything is fp32 (no matrix product is left: the two of the two-stage form are a 128-term and a C-term dot product here).  No
// atomics: every sum has one fixed order that depends on (B, T, C) alone, two runs are bit-equal.  Launches of a step:
//
//   simple_fwd_u      per 64 channels: u, sixteen 8-row partial sums met in LDS in a fixed tree
//   simple_fwd_rows   one wave per (row, segment of 1024 channels): a partial X . u
//   simple_fwd_score  one wave per video: its T * nseg partials, strided then a butterfly; adds w2 . b1 + b2
//   headtrain_loss    (headtrain.hip)
//   simple_bwd_g      per (128 channels, run of rows): the run's partial g, eight row phases met in LDS
//   simple_bwd_w1     per (256 channels, 16 hidden units): g = the run partials in four segments of ascending runs, met as
//                     (s0 + s1) + (s2 + s3); writes dW1 rows w2[j] * g and (first row group) g
//   simple_bwd_small  per hidden unit j: dw2[j] = W1[j,:] . g + b1[j] S, db1[j], and (j == 0) db2
//   headtrain_adamw   (headtrain.hip)
#include "common.hpp"
#include "featbank.hpp"
#include "simple_headtrain.hpp"

namespace kvq {

__device__ __forceinline__ f32x4 sh_fma4(float a, f32x4 x, f32x4 acc) {
  return (f32x4){fmaf(a, x[0], acc[0]), fmaf(a, x[1], acc[1]), fmaf(a, x[2], acc[2]), fmaf(a, x[3], acc[3])};
}
__device__ __forceinline__ f32x4 sh_fma4(f32x4 a, f32x4 x, f32x4 acc) {
  return (f32x4){fmaf(a[0], x[0], acc[0]), fmaf(a[1], x[1], acc[1]), fmaf(a[2], x[2], acc[2]), fmaf(a[3], x[3], acc[3])};
}

// grid C / 64, 256 threads: thread = (channel quad tid & 15, row group tid >> 4).  u[c] = sum_j w2[j] W1[j][c]: a thread adds its rows
// 8 jg .. 8 jg + 7 in ascending order (eight 16-byte loads in flight), the sixteen groups meet in LDS in a balanced tree.
__global__ __launch_bounds__(256) void simple_fwd_u_kernel(const float* __restrict__ w1, const float* __restrict__ w2, int C,
                                                           float* __restrict__ u) {
  __shared__ f32x4 red[16][16];
  const int q = threadIdx.x & 15, jg = threadIdx.x >> 4;
  const int c = blockIdx.x * 64 + 4 * q;                           // < C: C % 64 == 0 and the grid is C / 64
  f32x4 v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = *reinterpret_cast<const f32x4*>(w1 + (size_t)(8 * jg + k) * C + c);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 8; ++k) acc = sh_fma4(w2[8 * jg + k], v[k], acc);
  red[jg][q] = acc;
  __syncthreads();
  if (threadIdx.x < 16) {
    f32x4 s[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) s[k] = red[k][q];
#pragma unroll
    for (int w = 1; w < 16; w *= 2)
#pragma unroll
      for (int k = 0; k < 16; k += 2 * w) s[k] += s[k + w];
    *reinterpret_cast<f32x4*>(u + c) = s[0];
  }
}

// grid ceil(N * nseg / 4), 256 threads: wave = one (row n, segment sg) of the [N][nseg] partials.  A lane multiplies up to four channel
// quads (c = 1024 sg + 256 k + 4 lane) into four running sums, adds them as (0 + 1) + (2 + 3); the lanes meet in a butterfly.
// Row n = (b, t) reads row bank_row(b) of feat.
template <typename E>
__global__ __launch_bounds__(256) void simple_fwd_rows_kernel(const E* __restrict__ feat, const int32_t* __restrict__ index, long n_rows,
                                                              int T, const float* __restrict__ u, long N, int C, int nseg,
                                                              float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= N * nseg) return;                                   // a whole wave; no barrier follows
  const long n = item / nseg;
  const int sg = (int)(item % nseg);
  const long b = n / T;
  const long nsrc = bank_row(index, n_rows, b) * T + (n - b * T);
  const E* xr = feat + (size_t)nsrc * C;
  f32x4 x[4], w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = sg * SH_SEG + 256 * k + 4 * lane;
    x[k] = w[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (c < C) {                                                   // c % 4 == 0 and C % 4 == 0: the quad is inside the row
      x[k] = bank_load4(xr + c);
      w[k] = *reinterpret_cast<const f32x4*>(u + c);
    }
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) acc = sh_fma4(x[k], w[k], acc);
  const float s = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
  if (lane == 0) part[item] = s;
}

// grid B, 64 threads.  score[b] = (sum of the video's T * nseg partials) / T + (w2 . b1 + b2).
__global__ __launch_bounds__(64) void simple_fwd_score_kernel(const float* __restrict__ part, int per, int T, const float* __restrict__ b1,
                                                              const float* __restrict__ w2, const float* __restrict__ b2,
                                                              float* __restrict__ score) {
  const int lane = threadIdx.x;
  const float* src = part + (size_t)blockIdx.x * per;
  float s = 0.f;
  for (int i = lane; i < per; i += 64) s += src[i];
  s = wave_sum(s);
  const float c0 = wave_sum(fmaf(w2[lane], b1[lane], w2[lane + 64] * b1[lane + 64]));
  if (lane == 0) score[blockIdx.x] = s / (float)T + (c0 + b2[0]);
}

// grid (ceil(C / 128), nchunks), 256 threads: thread = (channel quad tid & 31, row phase tid >> 5).  The run's partial
// g[c] = sum_n dscore[n / T] / T * X[n][c]: a thread adds its rows r0 + ph, r0 + ph + 8, ... in ascending order, the eight phases meet in
// LDS as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)).
// Row r = (b, t) reads row bank_row(b) of feat, as in the forward.
template <typename E>
__global__ __launch_bounds__(256) void simple_bwd_g_kernel(const E* __restrict__ feat, const int32_t* __restrict__ index, long n_rows,
                                                           const float* __restrict__ dscore, long N, int T, int C, int chunk,
                                                           float* __restrict__ gpart) {
  __shared__ f32x4 red[8][32];
  const int q = threadIdx.x & 31, ph = threadIdx.x >> 5;
  const int c = blockIdx.x * 128 + 4 * q;
  const bool in = c < C;
  const long r0 = (long)blockIdx.y * chunk, r1 = min(r0 + chunk, N);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (in) {
#pragma unroll 4
    for (long r = r0 + ph; r < r1; r += 8) {
      const long b = r / T;
      const float d = dscore[b] / (float)T;
      const long rsrc = bank_row(index, n_rows, b) * T + (r - b * T);
      acc = sh_fma4(d, bank_load4(feat + (size_t)rsrc * C + c), acc);
    }
  }
  red[ph][q] = acc;
  __syncthreads();
  if (threadIdx.x < 32 && in)
    *reinterpret_cast<f32x4*>(gpart + (size_t)blockIdx.y * C + c) =
        ((red[0][q] + red[1][q]) + (red[2][q] + red[3][q])) + ((red[4][q] + red[5][q]) + (red[6][q] + red[7][q]));
}

// grid (ceil(C / 256), 8), 256 threads: thread = (channel quad tid & 63, wave jw).  The nchunks <= 32 run partials are cut into four
// segments of consecutive runs; wave jw adds its segment in ascending order (at most eight loads, all in flight), the segments meet in
// LDS as (s0 + s1) + (s2 + s3).  Wave jw then writes dW1 rows j = 16 blockIdx.y + 4 jw .. + 3 as w2[j] * g; row group 0 keeps g.
__global__ __launch_bounds__(256) void simple_bwd_w1_kernel(const float* __restrict__ gpart, const float* __restrict__ w2, int C,
                                                            int nchunks, float* __restrict__ g, float* __restrict__ dw1) {
  __shared__ f32x4 red[4][64];
  const int q = threadIdx.x & 63, jw = threadIdx.x >> 6;
  const int c = blockIdx.x * 256 + 4 * q;
  const bool in = c < C;
  const int per = (nchunks + 3) / 4, lo = jw * per, hi = min(lo + per, nchunks);
  f32x4 v[8], s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    // a run past the segment's end adds an exact zero; its load is unconditional (of the first quad, always there): eight conditional
    // loads kept every partial state of the chain alive, 170 VGPRs against 40
    const bool live = in && lo + k < hi;
    const f32x4 t = *reinterpret_cast<const f32x4*>(gpart + (live ? (size_t)(lo + k) * C + c : (size_t)0));
    v[k] = live ? t : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) s += v[k];
  red[jw][q] = s;
  __syncthreads();
  if (!in) return;
  const f32x4 gv = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
  if (blockIdx.y == 0 && jw == 0) *reinterpret_cast<f32x4*>(g + c) = gv;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = 16 * blockIdx.y + 4 * jw + r;                    // < 128 = 8 * 16
    const float w = w2[j];
    *reinterpret_cast<f32x4*>(dw1 + (size_t)j * C + c) = (f32x4){w * gv[0], w * gv[1], w * gv[2], w * gv[3]};
  }
}

// grid 128, 256 threads: hidden unit j = blockIdx.x.  out = the flat gradient behind dW1: db1 [128] | dw2 [128] | db2.
// S = sum_b dscore (B <= 1024: thread t owns t, t + 256, t + 512, t + 768), W1[j,:] . g with a thread's quads in ascending order.
__global__ __launch_bounds__(256) void simple_bwd_small_kernel(const float* __restrict__ w1, const float* __restrict__ b1,
                                                               const float* __restrict__ w2, const float* __restrict__ g,
                                                               const float* __restrict__ dscore, int B, int C, float* __restrict__ out) {
  __shared__ float wsum[4];
  const int j = blockIdx.x, tid = threadIdx.x;
  float d[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) d[k] = tid + 256 * k < B ? dscore[tid + 256 * k] : 0.f;
  const float S = block_sum((d[0] + d[1]) + (d[2] + d[3]), wsum);
  const float* wr = w1 + (size_t)j * C;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int c = 4 * tid; c < C; c += 1024)
    acc = sh_fma4(*reinterpret_cast<const f32x4*>(wr + c), *reinterpret_cast<const f32x4*>(g + c), acc);
  const float dot = block_sum((acc[0] + acc[1]) + (acc[2] + acc[3]), wsum);
  if (tid == 0) {
    out[j] = w2[j] * S;
    out[SH_HID + j] = fmaf(b1[j], S, dot);
    if (j == 0) out[2 * SH_HID] = S;
  }
}

// Every host check of a step but those of its outputs.  The bank part has refused misaligned rows.
static int simple_headtrain_check(const KvqHeadTrainBankArgs* a, const char* who, SimpleHeadTrainPlan* plan) {
  if (int rc = headtrain_bank_check(a, who)) return rc;
  KVQ_REQUIRE(a->params && a->workspace, KVQ_ERR_NULL, "%s: NULL pointer", who);
  KVQ_REQUIRE(a->B >= 2 && a->B <= 1024 && a->L >= 1, KVQ_ERR_SHAPE, "%s: B %d outside 2 .. 1024 or T %d below 1", who, a->B, a->L);
  KVQ_REQUIRE((long)a->B * a->L <= (1L << 24), KVQ_ERR_SHAPE, "%s: B*T = %ld rows exceed 2^24", who, (long)a->B * a->L);
  KVQ_REQUIRE(a->hidden == SH_HID, KVQ_ERR_UNSUPPORTED, "%s: hidden %d (128 is built)", who, a->hidden);
  KVQ_REQUIRE(a->C >= 64 && a->C % 64 == 0, KVQ_ERR_UNSUPPORTED, "%s: C %d is not a multiple of 64", who, a->C);
  KVQ_REQUIRE(a->p_drop == 0.f, KVQ_ERR_UNSUPPORTED, "%s: p_drop %g (simpleVQAHead has no dropout: 0)", who, (double)a->p_drop);
  KVQ_REQUIRE((((uintptr_t)a->params | (uintptr_t)a->workspace) & 15) == 0, KVQ_ERR_UNSUPPORTED,
              "%s: feat, params and workspace must be 16-byte aligned", who);
  *plan = simple_headtrain_plan(a->B, a->L, a->C);
  KVQ_REQUIRE(a->workspace_bytes >= plan->total * sizeof(float), KVQ_ERR_WORKSPACE, "%s: workspace %zu bytes, %zu needed", who,
              a->workspace_bytes, plan->total * sizeof(float));
  return KVQ_OK;
}

}  // namespace kvq

extern "C" size_t kvq_simple_headtrain_workspace_bytes(int B, int T, int C, int hidden) {
  if (B < 2 || B > 1024 || T < 1 || (long)B * T > (1L << 24) || C < 64 || C % 64 || hidden != kvq::SH_HID) return 0;
  return kvq::simple_headtrain_plan(B, T, C).total * sizeof(float);
}

namespace kvq {

static int simple_headtrain_forward_call(const KvqHeadTrainBankArgs* a, const char* who, void* stream) {
  SimpleHeadTrainPlan pl;
  if (int rc = simple_headtrain_check(a, who, &pl)) return rc;
  KVQ_REQUIRE(a->score, KVQ_ERR_NULL, "%s: NULL pointer", who);
  float* ws = static_cast<float*>(a->workspace);
  const HeadParams p = head_params(a->params, SH_HID, a->C);
  if (int rc = launch("simple_fwd_u_kernel", simple_fwd_u_kernel, dim3((unsigned)(a->C / 64)), dim3(256), 0, stream, p.w1, p.w2, a->C,
                      ws + pl.u))
    return rc;
  if (int rc = with_bank_elem(a->bank.dtype, [&](auto e) {
        using E = decltype(e);
        return launch("simple_fwd_rows_kernel", simple_fwd_rows_kernel<E>, grid_1d(pl.N * pl.nseg, 4), dim3(256), 0, stream,
                      static_cast<const E*>(a->bank.rows), a->index, (long)a->bank.n_rows, a->L, ws + pl.u, pl.N, a->C, pl.nseg, ws + pl.part);
      }))
    return rc;
  return launch("simple_fwd_score_kernel", simple_fwd_score_kernel, dim3((unsigned)a->B), dim3(64), 0, stream, ws + pl.part, a->L * pl.nseg,
                a->L, p.b1, p.w2, p.b2, a->score);
}

static int simple_headtrain_backward_call(const KvqHeadTrainBankArgs* a, const char* who, void* stream) {
  SimpleHeadTrainPlan pl;
  if (int rc = simple_headtrain_check(a, who, &pl)) return rc;
  KVQ_REQUIRE(a->dscore && a->grads, KVQ_ERR_NULL, "%s: NULL pointer", who);
  KVQ_REQUIRE(((uintptr_t)a->grads & 15) == 0, KVQ_ERR_UNSUPPORTED, "%s: grads must be 16-byte aligned", who);
  float* ws = static_cast<float*>(a->workspace);
  const HeadParams p = head_params(a->params, SH_HID, a->C);
  if (int rc = with_bank_elem(a->bank.dtype, [&](auto e) {
        using E = decltype(e);
        return launch("simple_bwd_g_kernel", simple_bwd_g_kernel<E>, dim3((unsigned)((a->C + 127) / 128), (unsigned)pl.nchunks), dim3(256), 0,
                      stream, static_cast<const E*>(a->bank.rows), a->index, (long)a->bank.n_rows, a->dscore, pl.N, a->L, a->C, pl.chunk,
                      ws + pl.gpart);
      }))
    return rc;
  if (int rc = launch("simple_bwd_w1_kernel", simple_bwd_w1_kernel, dim3((unsigned)((a->C + 255) / 256), 8u), dim3(256), 0, stream, ws + pl.gpart,
                      p.w2, a->C, pl.nchunks, ws + pl.g, a->grads))
    return rc;
  return launch("simple_bwd_small_kernel", simple_bwd_small_kernel, dim3((unsigned)SH_HID), dim3(256), 0, stream, p.w1, p.b1, p.w2, ws + pl.g,
                a->dscore, a->B, a->C, a->grads + (size_t)SH_HID * a->C);
}

}  // namespace kvq

extern "C" int kvq_simple_headtrain_bank_forward(const KvqHeadTrainBankArgs* a, void* stream) {
  return kvq::simple_headtrain_forward_call(a, "kvq_simple_headtrain_bank_forward", stream);
}

extern "C" int kvq_simple_headtrain_bank_backward(const KvqHeadTrainBankArgs* a, void* stream) {
  return kvq::simple_headtrain_backward_call(a, "kvq_simple_headtrain_bank_backward", stream);
}
