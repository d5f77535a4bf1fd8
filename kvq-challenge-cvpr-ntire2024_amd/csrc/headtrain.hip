// One optimisation step of VQAHead on features of a frozen trunk (gfx950): the reference's train-mode head (head.py:60-68), its losses
// (trainer.py:337-354), the gradients of the four head parameters and torch's AdamW with the EMA copy (trainer.py:163-172).
//
//   features  B rows of a feature bank [n_rows][L][C], channels-last, in fp32, fp16 or bf16, picked by a device index and widened to
//             fp32 in registers (featbank.hpp): the two launches that read features are templates over the element type.  C % 64 == 0,
//             hidden == 64, one class, no pre-pool, B >= 2.  A dense fp32 batch is an fp32 bank of B rows with the index 0 .. B-1
//   params    one flat fp32 vector: W1 [64][C] | b1 [64] | w2 [64] | b2 [1]; the gradients and the AdamW state have the same layout
//   score[b]  = mean_l( w2 . (m2 * gelu(W1 (m1 * f) + b1)) ) + b2,   m1, m2 the scaled dropout masks of headtrain.hpp
//
// Everything is fp32: operands, products (fp32 MFMA, v_mfma_f32_16x16x4_f32, as vqa_head_mfma_kernel of misc.hip) and sums.  The masks
// are recomputed from the hash wherever they are needed: no mask tensor exists.  No atomics: every sum has one fixed order, two runs are
// bit-equal.  Launches of a step:
//
//   headtrain_fwd        16 tokens per workgroup, the four waves split the channels (the layout of vqa_head_mfma_kernel); keeps the
//                        pre-activations z [B*L][64] and writes the token scores
//   headtrain_score      score[b] = mean of the token scores + b2, one workgroup per clip
//   headtrain_loss       one workgroup: PLCC loss, rank loss, their sum and dscore
//   headtrain_bwd_hidden per run of 64 tokens: dz = dscore/L * w2 * m2 * gelu'(z), and the run's partial db1, dw2
//   headtrain_bwd_sum_small  db1, dw2: the run partials in eight segments of ascending runs, the segments in a fixed tree
//   headtrain_bwd_w1     per (64 channels, token chunk): partial dW1 = dz^T (m1 * f) on the matrix pipe, K = the chunk's tokens
//   headtrain_bwd_sum    dW1: adds the chunk partials in ascending order into the flat gradient; db2 = sum_b dscore
//   headtrain_adamw      elementwise AdamW + EMA over the flat vector
#include "common.hpp"
#include "featbank.hpp"
#include "headtrain.hpp"

namespace kvq {

constexpr int HT_HID = 64;

__global__ __launch_bounds__(256) void headtrain_mask_kernel(uint32_t key, uint32_t thr, long n, uint8_t* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = ht_bits(key, (uint32_t)i) >= thr ? 1 : 0;
}

// grid ceil(B*L / 16), 256 threads.  vqa_head_mfma_kernel with the two masks and the pre-activations kept.  Token tk = (b, l) reads
// row bank_row(b) of feat; the masks are indexed by the batch position tk.
template <typename E>
__global__ __launch_bounds__(256) void headtrain_fwd_kernel(const E* __restrict__ feat, const int32_t* __restrict__ index, long n_rows,
                                                            int L, long total, int C, const float* __restrict__ w1,
                                                            const float* __restrict__ b1, const float* __restrict__ w2, uint32_t key1,
                                                            uint32_t key2, uint32_t thr, float scale, float* __restrict__ z,
                                                            float* __restrict__ tok_score) {
  __shared__ float part[4][64][17];
  __shared__ float red[4][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tok = lane & 15, kq = lane >> 4;
  const long tk = min((long)blockIdx.x * 16 + tok, total - 1);
  const int cw = C / 4, c0 = wave * cw;
  const long b = tk / L;
  const long tsrc = bank_row(index, n_rows, b) * L + (tk - b * L);   // the token's place in feat, in tokens
  const E* xr = feat + (size_t)tsrc * C + c0 + 4 * kq;
  const uint32_t e0 = (uint32_t)((size_t)tk * C) + (uint32_t)(c0 + 4 * kq);      // element index of xr[0]
  const float* wr = w1 + (size_t)tok * C + c0 + 4 * kq;          // + 16 hb rows
  const size_t hbs = (size_t)16 * C;
  f32x4 acc[4];
#pragma unroll
  for (int hb = 0; hb < 4; ++hb) acc[hb] = (f32x4){0.f, 0.f, 0.f, 0.f};
  f32x4 xv = bank_load4(xr), wv[4];
#pragma unroll
  for (int hb = 0; hb < 4; ++hb) wv[hb] = *reinterpret_cast<const f32x4*>(wr + hb * hbs);
  for (int c = 0; c < cw; c += 16) {
    f32x4 xn = xv, wn[4] = {wv[0], wv[1], wv[2], wv[3]};
    if (c + 16 < cw) {                                             // the next macro-step's operands, under this one's MFMAs
      xn = bank_load4(xr + c + 16);
#pragma unroll
      for (int hb = 0; hb < 4; ++hb) wn[hb] = *reinterpret_cast<const f32x4*>(wr + hb * hbs + c + 16);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float xm = ht_bits(key1, e0 + (uint32_t)(c + s)) >= thr ? xv[s] * scale : 0.f;
#pragma unroll
      for (int hb = 0; hb < 4; ++hb) acc[hb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[hb][s], xm, acc[hb], 0, 0, 0);
    }
    xv = xn;
#pragma unroll
    for (int hb = 0; hb < 4; ++hb) wv[hb] = wn[hb];
  }
#pragma unroll
  for (int hb = 0; hb < 4; ++hb)
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wave][16 * hb + 4 * kq + r][tok] = acc[hb][r];
  __syncthreads();
  // thread = (token tid & 15, hidden quad tid >> 4): channel partials in wave order, bias, mask, GELU, times w2
  const int t2 = tid & 15, hg = tid >> 4;
  const long tk2 = (long)blockIdx.x * 16 + t2;
  const bool live = tk2 < total;
  float v = 0.f;
  f32x4 zq;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int h = 4 * hg + r;
    const float full = (part[0][h][t2] + part[1][h][t2]) + (part[2][h][t2] + part[3][h][t2]);
    zq[r] = full + b1[h];
    const float m2 = ht_bits(key2, (uint32_t)(tk2 * HT_HID + h)) >= thr ? scale : 0.f;
    v = fmaf(w2[h], gelu_erf(zq[r]) * m2, v);
  }
  if (live) *reinterpret_cast<f32x4*>(z + (size_t)tk2 * HT_HID + 4 * hg) = zq;
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  if (lane < 16) red[wave][lane] = v;
  __syncthreads();
  if (tid < 16 && (long)blockIdx.x * 16 + tid < total)
    tok_score[(long)blockIdx.x * 16 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// score[b] = mean_l tok_score[b*L + l] + b2: strided partial sums, then one fixed tree.  grid B, 256 threads.
__global__ __launch_bounds__(256) void headtrain_score_kernel(const float* __restrict__ tok, int L, const float* __restrict__ b2,
                                                              float* __restrict__ score) {
  __shared__ float wsum[4];
  const int b = blockIdx.x;
  float s = 0.f;
  for (int l = threadIdx.x; l < L; l += 256) s += tok[(size_t)b * L + l];
  const float t = block_sum(s, wsum);
  if (threadIdx.x == 0) score[b] = t / (float)L + b2[0];
}

// One workgroup of 256 threads, B <= 1024: thread t owns clips t, t + 256, t + 512, t + 768.
//   plcc (trainer.py:346-354): a = (p - mean p) / (std p + 1e-8), t the same of the labels (biased std);
//        loss0 = mean((a - t)^2) / 4, rho = mean(a t), loss1 = mean((rho a - t)^2) / 4, plcc = (loss0 + loss1) / 2
//   rank (trainer.py:337-344): R[i][j] = relu((p_i - p_j) sign(y_j - y_i)), rank = sum R / B / (B - 1) / (1 + max R)
// R is symmetric (both factors change sign), so row i alone gives dp_i of the sum: 2 sum_j [R_ij > 0] sign(y_j - y_i); the maximum is
// taken at the first (i, j) in row-major order, and its mirror (j, i) has the same derivatives, so the gradient through 1 + max R does
// not depend on which of the two carries it.  out3 = {plcc + rank_weight * rank, plcc, rank}.
__global__ __launch_bounds__(256) void headtrain_loss_kernel(const float* __restrict__ score, const float* __restrict__ label, int B,
                                                             float rank_weight, float* __restrict__ out3, float* __restrict__ dscore) {
  __shared__ float sp[1024], sy[1024];
  __shared__ float wsum[4];
  __shared__ float mval[256];
  __shared__ int midx[256];
  const int tid = threadIdx.x;
  const float n = (float)B;
  float p[4], y[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = tid + 256 * k;
    p[k] = i < B ? score[i] : 0.f;
    y[k] = i < B ? label[i] : 0.f;
    if (i < B) {
      sp[i] = p[k];
      sy[i] = y[k];
    }
  }
  const float mp = block_sum((p[0] + p[1]) + (p[2] + p[3]), wsum) / n;
  const float my = block_sum((y[0] + y[1]) + (y[2] + y[3]), wsum) / n;
  float dp[4], dy[4], qp = 0.f, qy = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool in = tid + 256 * k < B;
    dp[k] = in ? p[k] - mp : 0.f;
    dy[k] = in ? y[k] - my : 0.f;
    qp = fmaf(dp[k], dp[k], qp);
    qy = fmaf(dy[k], dy[k], qy);
  }
  const float sdp = sqrtf(block_sum(qp, wsum) / n), sdy = sqrtf(block_sum(qy, wsum) / n);
  const float ip = 1.0f / (sdp + 1e-8f), iy = 1.0f / (sdy + 1e-8f);
  float a[4], t[4], s_at = 0.f, s0 = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    a[k] = dp[k] * ip;
    t[k] = dy[k] * iy;
    s_at = fmaf(a[k], t[k], s_at);
    s0 = fmaf(a[k] - t[k], a[k] - t[k], s0);
  }
  const float rho = block_sum(s_at, wsum) / n;
  const float loss0 = block_sum(s0, wsum) / n * 0.25f;
  float s1 = 0.f, sS = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float e = fmaf(rho, a[k], -t[k]);
    s1 = fmaf(e, e, s1);
    sS = fmaf(e, a[k], sS);
  }
  const float loss1 = block_sum(s1, wsum) / n * 0.25f;
  const float S = block_sum(sS, wsum);
  const float plcc = (loss0 + loss1) * 0.5f;
  // d plcc / d a, then through a = (p - mean) / (std + eps)
  float ga[4], sgd = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool in = tid + 256 * k < B;
    const float e = fmaf(rho, a[k], -t[k]);
    ga[k] = in ? ((a[k] - t[k]) + fmaf(rho, e, S * t[k] / n)) / (4.0f * n) : 0.f;
    sgd = fmaf(ga[k], dp[k], sgd);
  }
  const float G = block_sum(sgd, wsum);
  const float cstd = sdp > 0.f ? G * ip * ip / (n * sdp) : 0.f;
  // the gradient to d = p - mean (through the quotient and through the std), centred LAST as autograd does for the mean: the loss does not
  // move when every score moves by the same amount, and the centring keeps sum_b dscore = db2 at the rounding of this one subtraction
  float gpl[4], sgp = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    gpl[k] = tid + 256 * k < B ? fmaf(-dp[k], cstd, ga[k] * ip) : 0.f;
    sgp += gpl[k];
  }
  const float mgp = block_sum(sgp, wsum) / n;
#pragma unroll
  for (int k = 0; k < 4; ++k) gpl[k] -= mgp;

  // rank loss: row i of R per owned clip
  float rsum = 0.f, cnt[4], best = 0.f;
  int besti = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = tid + 256 * k;
    cnt[k] = 0.f;
    if (i < B) {
      float rs = 0.f;
      for (int j = 0; j < B; ++j) {
        const float d = sy[j] - y[k];
        const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        const float r = (p[k] - sp[j]) * sg;
        if (r > 0.f) {
          rs += r;
          cnt[k] += 2.f * sg;
          if (r > best) {
            best = r;
            besti = i * B + j;
          }
        }
      }
      rsum += rs;
    }
  }
  const float Rsum = block_sum(rsum, wsum);
  mval[tid] = best;
  midx[tid] = besti;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      const float ov = mval[tid + o];
      const int oi = midx[tid + o];
      if (ov > mval[tid] || (ov == mval[tid] && oi < midx[tid])) {
        mval[tid] = ov;
        midx[tid] = oi;
      }
    }
    __syncthreads();
  }
  const float M = mval[0];
  const int mi = M > 0.f ? midx[0] / B : -1, mj = M > 0.f ? midx[0] % B : -1;
  const float rscale = 1.0f + M, nn = n * (n - 1.0f);
  const float rank = Rsum / n / (n - 1.0f) / rscale;
  float msg = 0.f;
  if (M > 0.f) {
    const float d = sy[mj] - sy[mi];
    msg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  }
  const float cmax = Rsum / (nn * rscale * rscale);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = tid + 256 * k;
    if (i < B) {
      float gr = cnt[k] / (nn * rscale);
      if (i == mi) gr -= cmax * msg;
      if (i == mj) gr += cmax * msg;
      dscore[i] = fmaf(rank_weight, gr, gpl[k]);
    }
  }
  if (tid == 0) {
    out3[0] = fmaf(rank_weight, rank, plcc);
    out3[1] = plcc;
    out3[2] = rank;
  }
}

// grid (hsub, nchunks), 256 threads: a run of HT_SUB_TOKENS tokens of a chunk; thread = (hidden unit tid & 63, token phase tid >> 6).
// dz[t][h] = dscore[b] / L * w2[h] * m2 * gelu'(z), gelu'(z) = Phi(z) + z phi(z); the run's partial db1[h] = sum_t dz, dw2[h] = sum_t
// dscore[b] / L * m2 * gelu(z), a thread's tokens in ascending order, the four phases as (0 + 1) + (2 + 3).
__global__ __launch_bounds__(256) void headtrain_bwd_hidden_kernel(const float* __restrict__ z, const float* __restrict__ dscore,
                                                                   const float* __restrict__ w2, long total, int L, int chunk, uint32_t key2,
                                                                   uint32_t thr, float scale, float* __restrict__ dz,
                                                                   float* __restrict__ part_b1, float* __restrict__ part_w2) {
  __shared__ float rb[4][HT_HID], rw[4][HT_HID];
  const int h = threadIdx.x & 63, q = threadIdx.x >> 6;
  const long c1 = min((long)(blockIdx.y + 1) * chunk, total);                // the chunk's end
  const long t0 = (long)blockIdx.y * chunk + (long)blockIdx.x * HT_SUB_TOKENS;
  const long t1 = min(t0 + HT_SUB_TOKENS, c1);                               // <= t0: an empty run, zeros
  const float w = w2[h];
  float ab = 0.f, aw = 0.f;
#pragma unroll 4
  for (long t = t0 + q; t < t1; t += 4) {
    const float zv = z[(size_t)t * HT_HID + h];
    const float g = dscore[t / L] / (float)L;
    const float m2 = ht_bits(key2, (uint32_t)(t * HT_HID + h)) >= thr ? scale : 0.f;
    const float Phi = 0.5f * (1.0f + erff(zv * 0.70710678118654752440f));
    const float phi = 0.39894228040143267794f * expf(-0.5f * zv * zv);
    const float gm = g * m2;
    const float d = gm * w * fmaf(zv, phi, Phi);
    dz[(size_t)t * HT_HID + h] = d;
    ab += d;
    aw = fmaf(gm, zv * Phi, aw);
  }
  rb[q][h] = ab;
  rw[q][h] = aw;
  __syncthreads();
  if (q == 0) {
    const size_t run = (size_t)blockIdx.y * gridDim.x + blockIdx.x;          // runs in token order
    part_b1[run * HT_HID + h] = (rb[0][h] + rb[1][h]) + (rb[2][h] + rb[3][h]);
    part_w2[run * HT_HID + h] = (rw[0][h] + rw[1][h]) + (rw[2][h] + rw[3][h]);
  }
}

// One workgroup of 1024 threads: thread = (element tid & 127 of db1 | dw2, segment tid >> 7).  The nsub run partials are cut into eight
// segments of consecutive runs; a thread adds its segment in ascending order (eight loads in flight), the segments meet in LDS as
// ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)).
__global__ __launch_bounds__(1024) void headtrain_bwd_sum_small_kernel(const float* __restrict__ part_b1, const float* __restrict__ part_w2,
                                                                       int nsub, float* __restrict__ out) {
  __shared__ float red[8][2 * HT_HID];
  const int e = threadIdx.x & 127, seg = threadIdx.x >> 7;
  const float* src = (e < HT_HID ? part_b1 : part_w2) + (e & 63);
  const int per = (nsub + 7) / 8, lo = seg * per, hi = min(lo + per, nsub);
  float s = 0.f;
  for (int c = lo; c < hi; c += 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = c + k < hi ? src[(size_t)(c + k) * HT_HID] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += v[k];
  }
  red[seg][e] = s;
  __syncthreads();
  if (threadIdx.x < 2 * HT_HID)
    out[e] = ((red[0][e] + red[1][e]) + (red[2][e] + red[3][e])) + ((red[4][e] + red[5][e]) + (red[6][e] + red[7][e]));
}

// grid (C / 64, nchunks), 256 threads.  part[chunk][h][c] = sum over the chunk's tokens of dz[t][h] * (m1 * f)[t][c] for 64 channels, by
// v_mfma_f32_16x16x4_f32 with the tokens as k: a k-step is 4 tokens; lane (j = lane & 15, kq = lane >> 4) loads four consecutive channels
// c0 + 4 j .. + 3 of token kq (one 16-byte load: a token's 64 channels are one 256-byte row piece) and dz of hidden units 16 hb + j.  MFMA
// (hb, s) takes element s of every lane's quad, so its 16 output columns are the channels c0 + 4 j + s and a lane's four tiles s = 0 .. 3
// hold four consecutive channels again.  The four waves take the k-steps in turn (wave w: steps w, w + 4, ...) and meet in LDS, added as
// (w0 + w1) + (w2 + w3); wave w then stores the hidden units 16 w .. 16 w + 15.
// Token t = (b, l) reads row bank_row(b) of feat, as in the forward; dz and the mask are indexed by t.
template <typename E>
__global__ __launch_bounds__(256) void headtrain_bwd_w1_kernel(const E* __restrict__ feat, const int32_t* __restrict__ index, long n_rows,
                                                               int L, const float* __restrict__ dz, long total, int C, int chunk,
                                                               uint32_t key1, uint32_t thr, float scale, float* __restrict__ part) {
  __shared__ float red[4][3][16][64];                      // [owner hb][source slot][s * 4 + r][lane]: 48 KiB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  const int c0 = blockIdx.x * 64;
  const long t0 = (long)blockIdx.y * chunk;
  const long t1 = min(t0 + chunk, total);
  f32x4 acc[4][4];
#pragma unroll
  for (int hb = 0; hb < 4; ++hb)
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[hb][s] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // a k-step's operands: the lane's token (clamped into the chunk, zeroed when past its end), its feature quad and its four dz values
  struct Step {
    f32x4 x;
    float d[4];
    uint32_t e0;
    bool in;
  };
  auto fetch = [&](long ts) {
    Step o;
    const long t = ts + kq;
    o.in = t < t1;
    const long tc = o.in ? t : t1 - 1;
    const long b = tc / L;
    const long tsrc = bank_row(index, n_rows, b) * L + (tc - b * L);
    o.x = bank_load4(feat + (size_t)tsrc * C + c0 + 4 * j);
    o.e0 = (uint32_t)((size_t)tc * C) + (uint32_t)(c0 + 4 * j);
#pragma unroll
    for (int hb = 0; hb < 4; ++hb) o.d[hb] = dz[(size_t)tc * HT_HID + 16 * hb + j];
    return o;
  };
  long ts = t0 + 4 * wave;
  if (ts < t1) {
    Step cur = fetch(ts);
    for (; ts < t1; ts += 16) {
      Step nxt = cur;
      if (ts + 16 < t1) nxt = fetch(ts + 16);              // the next k-step's operands, under this one's MFMAs
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float xm = (cur.in && ht_bits(key1, cur.e0 + (uint32_t)s) >= thr) ? cur.x[s] * scale : 0.f;
#pragma unroll
        for (int hb = 0; hb < 4; ++hb)
          acc[hb][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.in ? cur.d[hb] : 0.f, xm, acc[hb][s], 0, 0, 0);
      }
      cur = nxt;
    }
  }
#pragma unroll
  for (int hb = 0; hb < 4; ++hb) {
    if (hb != wave) {
      const int slot = wave < hb ? wave : wave - 1;
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[hb][slot][4 * s + r][lane] = acc[hb][s][r];
    }
  }
  __syncthreads();
#pragma unroll
  for (int hb = 0; hb < 4; ++hb) {
    if (hb == wave) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        f32x4 o;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          float v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = u == hb ? acc[hb][s][r] : red[hb][u < hb ? u : u - 1][4 * s + r][lane];
          o[s] = (v[0] + v[1]) + (v[2] + v[3]);
        }
        const int h = 16 * hb + 4 * kq + r;
        *reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.y * HT_HID + h) * C + c0 + 4 * j) = o;
      }
    }
  }
}

// dW1 of the flat gradient: element quads are the chunk partials added in ascending order; db2 = sum_b dscore (one wave: strided sums,
// then a butterfly).  grid 64 C / 4 / 256 + 1 workgroups, the last one for db2.
__global__ __launch_bounds__(256) void headtrain_bwd_sum_kernel(const float* __restrict__ part_w1, const float* __restrict__ dscore, int B,
                                                                int C, int nchunks, float* __restrict__ grads) {
  const size_t nw1 = (size_t)HT_HID * C;
  if (blockIdx.x == gridDim.x - 1) {
    if (threadIdx.x >= 64) return;
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += 64) s += dscore[b];
    s = wave_sum(s);
    if (threadIdx.x == 0) grads[nw1 + 2 * HT_HID] = s;
    return;
  }
  const size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e >= nw1) return;
  const float* src = part_w1 + e;
  const size_t stride = nw1;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < nchunks; c += 8) {                   // eight loads in flight; a chunk past the end adds an exact zero
    f32x4 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      v[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (c + k < nchunks) v[k] = *reinterpret_cast<const f32x4*>(src + (size_t)(c + k) * stride);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s += v[k];
  }
  *reinterpret_cast<f32x4*>(grads + e) = s;                // grads is 16-byte aligned (host check), e a multiple of 4
}

// torch.optim.AdamW (betas 0.9, 0.999; eps 1e-8; no amsgrad) on one flat vector, in torch's order of operations:
//   p *= 1 - lr wd;  m += (g - m)(1 - b1);  v = v b2 + (1 - b2) g g;  p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// then ema = 0.999 ema + 0.001 p (trainer.py:170-172) when ema != NULL.  The scalars are computed on the host in double.
__global__ __launch_bounds__(256) void headtrain_adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                              float* __restrict__ v, float* __restrict__ ema, long n, float decay,
                                                              float step_size, float bc2_sqrt) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float gi = g[i];
  float pi = p[i] * decay;
  const float mi = fmaf(gi - m[i], 0.1f, m[i]);
  const float vi = fmaf(gi * gi, 0.001f, v[i] * 0.999f);
  const float denom = sqrtf(vi) / bc2_sqrt + 1e-8f;
  pi = fmaf(-step_size, mi / denom, pi);
  p[i] = pi;
  m[i] = mi;
  v[i] = vi;
  if (ema) ema[i] = fmaf(0.001f, pi, ema[i] * 0.999f);
}

// Every host check of a step but those of its outputs.  The bank part has refused misaligned rows and B * L * C past the 32-bit mask index.
static int headtrain_check(const KvqHeadTrainBankArgs* a, const char* who, HeadTrainPlan* plan) {
  if (int rc = headtrain_bank_check(a, who)) return rc;
  KVQ_REQUIRE(a->params && a->workspace, KVQ_ERR_NULL, "%s: NULL pointer", who);
  KVQ_REQUIRE(a->hidden == HT_HID, KVQ_ERR_UNSUPPORTED, "%s: hidden %d (64 is built)", who, a->hidden);
  KVQ_REQUIRE(a->C >= 64 && a->C % 64 == 0, KVQ_ERR_UNSUPPORTED, "%s: C %d is not a multiple of 64", who, a->C);
  KVQ_REQUIRE(a->p_drop >= 0.f && a->p_drop < 1.f, KVQ_ERR_UNSUPPORTED, "%s: dropout probability %g outside [0, 1)", who, (double)a->p_drop);
  KVQ_REQUIRE(a->B >= 2 && a->L >= 1, KVQ_ERR_SHAPE, "%s: B %d (at least 2 clips: the loss of one is constant), L %d", who, a->B, a->L);
  KVQ_REQUIRE((((uintptr_t)a->params | (uintptr_t)a->workspace) & 15) == 0, KVQ_ERR_UNSUPPORTED,
              "%s: feat, params and workspace must be 16-byte aligned", who);
  *plan = headtrain_plan(a->B, a->L, a->C, a->hidden);
  KVQ_REQUIRE(a->workspace_bytes >= plan->total * sizeof(float), KVQ_ERR_WORKSPACE, "%s: workspace %zu bytes, %zu needed", who,
              a->workspace_bytes, plan->total * sizeof(float));
  return KVQ_OK;
}

}  // namespace kvq

extern "C" size_t kvq_headtrain_workspace_bytes(int B, int L, int C, int hidden) {
  if (B < 2 || L < 1 || C < 64 || C % 64 || hidden != kvq::HT_HID) return 0;
  return kvq::headtrain_plan(B, L, C, hidden).total * sizeof(float);
}

extern "C" int kvq_headtrain_mask(uint32_t seed, uint32_t step, int which, float p, int64_t n, uint8_t* out, void* stream) {
  using namespace kvq;
  KVQ_REQUIRE(out, KVQ_ERR_NULL, "kvq_headtrain_mask: NULL pointer");
  KVQ_REQUIRE((which == 0 || which == 1) && p >= 0.f && p < 1.f, KVQ_ERR_UNSUPPORTED, "kvq_headtrain_mask: which %d, p %g", which, (double)p);
  KVQ_REQUIRE(n >= 1 && n <= 4294967296LL, KVQ_ERR_SHAPE, "kvq_headtrain_mask: n %lld outside the 32-bit mask index", (long long)n);
  return launch("headtrain_mask_kernel", headtrain_mask_kernel, grid_1d(n), dim3(256), 0, stream, ht_key(seed, step, (uint32_t)which),
                ht_threshold(p), (long)n, out);
}

namespace kvq {

static int headtrain_forward_call(const KvqHeadTrainBankArgs* a, const char* who, void* stream) {
  HeadTrainPlan pl;
  if (int rc = headtrain_check(a, who, &pl)) return rc;
  KVQ_REQUIRE(a->score, KVQ_ERR_NULL, "%s: NULL pointer", who);
  float* ws = static_cast<float*>(a->workspace);
  const HeadParams p = head_params(a->params, HT_HID, a->C);
  const uint32_t thr = ht_threshold(a->p_drop);
  if (int rc = with_bank_elem(a->bank.dtype, [&](auto e) {
        using E = decltype(e);
        return launch("headtrain_fwd_kernel", headtrain_fwd_kernel<E>, grid_1d(pl.T, 16), dim3(256), 0, stream,
                      static_cast<const E*>(a->bank.rows), a->index, (long)a->bank.n_rows, a->L, pl.T, a->C, p.w1, p.b1, p.w2,
                      ht_key(a->seed, a->step, 0), ht_key(a->seed, a->step, 1), thr, ht_scale(a->p_drop), ws + pl.z, ws + pl.tok);
      }))
    return rc;
  return launch("headtrain_score_kernel", headtrain_score_kernel, dim3((unsigned)a->B), dim3(256), 0, stream, ws + pl.tok, a->L, p.b2,
                a->score);
}

static int headtrain_backward_call(const KvqHeadTrainBankArgs* a, const char* who, void* stream) {
  HeadTrainPlan pl;
  if (int rc = headtrain_check(a, who, &pl)) return rc;
  KVQ_REQUIRE(a->dscore && a->grads, KVQ_ERR_NULL, "%s: NULL pointer", who);
  float* ws = static_cast<float*>(a->workspace);
  const float* w2 = head_params(a->params, HT_HID, a->C).w2;
  const uint32_t thr = ht_threshold(a->p_drop);
  const float scale = ht_scale(a->p_drop);
  KVQ_REQUIRE(((uintptr_t)a->grads & 15) == 0, KVQ_ERR_UNSUPPORTED, "%s: grads must be 16-byte aligned", who);
  const size_t nw1 = (size_t)HT_HID * a->C;
  if (int rc = launch("headtrain_bwd_hidden_kernel", headtrain_bwd_hidden_kernel, dim3((unsigned)pl.hsub, (unsigned)pl.nchunks), dim3(256), 0,
                      stream, ws + pl.z, a->dscore, w2, pl.T, a->L, pl.chunk, ht_key(a->seed, a->step, 1), thr, scale, ws + pl.dz,
                      ws + pl.part_b1, ws + pl.part_w2))
    return rc;
  if (int rc = launch("headtrain_bwd_sum_small_kernel", headtrain_bwd_sum_small_kernel, dim3(1), dim3(1024), 0, stream, ws + pl.part_b1,
                      ws + pl.part_w2, pl.nsub, a->grads + nw1))
    return rc;
  if (int rc = with_bank_elem(a->bank.dtype, [&](auto e) {
        using E = decltype(e);
        return launch("headtrain_bwd_w1_kernel", headtrain_bwd_w1_kernel<E>, dim3((unsigned)(a->C / 64), (unsigned)pl.nchunks), dim3(256), 0,
                      stream, static_cast<const E*>(a->bank.rows), a->index, (long)a->bank.n_rows, a->L, ws + pl.dz, pl.T, a->C, pl.chunk,
                      ht_key(a->seed, a->step, 0), thr, scale, ws + pl.part_w1);
      }))
    return rc;
  const long quads = (long)nw1 / 4;
  return launch("headtrain_bwd_sum_kernel", headtrain_bwd_sum_kernel, dim3((unsigned)((quads + 255) / 256 + 1)), dim3(256), 0, stream,
                ws + pl.part_w1, a->dscore, a->B, a->C, pl.nchunks, a->grads);
}

}  // namespace kvq

extern "C" int kvq_headtrain_bank_forward(const KvqHeadTrainBankArgs* a, void* stream) {
  return kvq::headtrain_forward_call(a, "kvq_headtrain_bank_forward", stream);
}

extern "C" int kvq_headtrain_loss(const float* score, const float* label, int B, float rank_weight, float* out3, float* dscore,
                                  void* stream) {
  using namespace kvq;
  KVQ_REQUIRE(score && label && out3 && dscore, KVQ_ERR_NULL, "kvq_headtrain_loss: NULL pointer");
  KVQ_REQUIRE(B >= 2 && B <= 1024, KVQ_ERR_SHAPE, "kvq_headtrain_loss: B %d outside 2 .. 1024", B);
  return launch("headtrain_loss_kernel", headtrain_loss_kernel, dim3(1), dim3(256), 0, stream, score, label, B, rank_weight, out3, dscore);
}

extern "C" int kvq_headtrain_bank_backward(const KvqHeadTrainBankArgs* a, void* stream) {
  return kvq::headtrain_backward_call(a, "kvq_headtrain_bank_backward", stream);
}

extern "C" int kvq_headtrain_adamw(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, float lr,
                                   float wd, int step, void* stream) {
  using namespace kvq;
  KVQ_REQUIRE(params && grads && exp_avg && exp_avg_sq, KVQ_ERR_NULL, "kvq_headtrain_adamw: NULL pointer");
  KVQ_REQUIRE(n >= 1 && step >= 1, KVQ_ERR_SHAPE, "kvq_headtrain_adamw: n %lld, step %d (steps count from 1)", (long long)n, step);
  const double bc1 = 1.0 - pow(0.9, (double)step), bc2 = 1.0 - pow(0.999, (double)step);
  return launch("headtrain_adamw_kernel", headtrain_adamw_kernel, grid_1d(n), dim3(256), 0, stream, params, grads, exp_avg, exp_avg_sq, ema,
                (long)n, (float)(1.0 - (double)lr * (double)wd), (float)((double)lr / bc1), (float)sqrt(bc2));
}
