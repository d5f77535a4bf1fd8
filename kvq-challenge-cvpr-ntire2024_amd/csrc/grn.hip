// Global Response Normalization between the two pointwise GEMMs of a ConvNeXt-V2 3D block (gfx950): BlockV23D.grn of the reference
// (conv_backbone.py:7-18, :245).  The reference calls its 2D GRN module on a (N, T, H, W, C) tensor, so torch.norm(dim=(1, 2)) reduces
// over T and H only: one norm per (sample, w column, channel).  over_w = 1 also sums over w (the GRN of the ConvNeXt-V2 paper in 3D).
//
//   x      16-bit rows [B*D*H*W][N] as the GELU GEMM writes them, tokens in (b, d, h, w) order, N = 4C in {384, 768, 1536, 3072}
//   Gx     [b][w][n] = sqrt(sum over (d, h) of x^2)            (over_w: [b][n], summed over w as well)
//   y      round16(x * (1 + gamma[n] * Gx / (mean_n Gx + 1e-6)) + beta[n]), in place or into a second buffer
//
// For a fixed (b, d, h) the (w, n) slab is L = W*N contiguous values, so the statistics are the column sums of squares of a
// [B][R = D*H][L] matrix over its middle axis.  Three launches (four with over_w), all fp32 arithmetic, no atomics and no counters:
//
//   grn_sumsq      a workgroup of four waves owns 512 columns (a lane: 8 consecutive ones, one 16-B load per row) and a chunk of rows,
//                  which the waves take in turn; the four wave sums are added in a fixed order through LDS: fp32 partial sums of
//                  squares part[b][chunk][L].  The host cuts R into chunks from the shape alone (grn_plan), not from B.
//   grn_finalize   one workgroup per (b, w), a thread owns 4 consecutive n: adds the chunk partials in ascending order (eight loads in
//                  flight), takes the square roots, reduces the mean over n (wave butterflies, then the wave sums in a fixed order
//                  through LDS) and writes scale[b][w][n] = 1 + gamma[n] * Nx.  B*W*N floats: all the apply launch needs besides x.
//                  over_w: it writes the sums of squares instead, and grn_finalize_w (one workgroup per b) adds them over w in
//                  ascending order and writes the one scale per (b, n) to every w.
//   grn_apply      a lane owns 8 consecutive columns and a chunk of rows: scale and beta of the columns stay in 16 registers, the rows
//                  stream through (16-B load, 8 FMAs, 16-B store, four rows in flight).
//
// kvq_grn_stats enqueues all but the last, kvq_grn_apply the last.  Every sum has one fixed order: two runs are bit-equal, and a sample's
// result does not depend on the batch it is in.  An all-zero column has Gx = 0 and, if the whole (b, w) slab is zero, Nx = 0 / 1e-6 = 0.
#include "common.hpp"
#include "wave.hpp"

namespace kvq {

constexpr int GRN_THREADS = 128;                 // apply: 2 waves; 8 columns per lane = 1024 columns per workgroup
constexpr int GRN_COLS = GRN_THREADS * 8;
constexpr int GRN_SUM_THREADS = 256;             // statistics: 4 waves on the same 512 columns, rows interleaved
constexpr int GRN_SUM_COLS = 64 * 8;
constexpr int GRN_FIN_THREADS = 256;
constexpr int GRN_MAX_N = 3072;                  // = 3 float4 per thread of the finalize launches

struct GrnPlan {
  long L;            // W * N
  long R;            // D * H
  int sgroups;       // statistics: ceil(L / GRN_SUM_COLS) column groups,
  int nchunks, rpc;  //   chunks of rpc rows (the last one may be shorter, none is empty)
  int colgroups;     // apply: ceil(L / GRN_COLS) column groups,
  int achunks, arpc; //   its own cut of the rows
};

// Cut the R rows into chunks so that about `target` workgroups exist, but never fewer than `min_rows` rows per chunk: the partials cost
// 4 bytes per column and chunk against 2 bytes per column and row of x.
static void grn_cut(long R, long groups, long target, int min_rows, int* nchunks, int* rpc) {
  long want = (target + groups - 1) / groups;
  const long cap = (R + min_rows - 1) / min_rows;
  if (want > cap) want = cap;
  if (want < 1) want = 1;
  const long per = (R + want - 1) / want;
  *rpc = (int)per;
  *nchunks = (int)((R + per - 1) / per);
}

static GrnPlan grn_plan(int B, int D, int H, int W, int N) {
  GrnPlan p;
  p.L = (long)W * N;
  p.R = (long)D * H;
  p.sgroups = (int)((p.L + GRN_SUM_COLS - 1) / GRN_SUM_COLS);
  p.colgroups = (int)((p.L + GRN_COLS - 1) / GRN_COLS);
  // about 512 workgroups of four waves, at least four rows per wave.  The statistics' cut does not look at B: a sample's sums are added
  // in the same order whatever batch it travels in
  grn_cut(p.R, (long)p.sgroups, 512, 16, &p.nchunks, &p.rpc);
  grn_cut(p.R, (long)p.colgroups * B, 2048, 4, &p.achunks, &p.arpc);
  return p;
}

template <typename E>
__device__ __forceinline__ void grn_unpack8(const u32x4 v, float f[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = E::to_f32((uint16_t)(v[i] & 0xffffu));
    f[2 * i + 1] = E::to_f32((uint16_t)(v[i] >> 16));
  }
}

// grid (ceil(L / 512), nchunks, B), 256 threads: the four waves share 512 columns and take the rows of the chunk in turn (wave q: rows
// r0 + q, r0 + q + 4, ...), four loads in flight each; the four wave sums meet in LDS and are added as (w0 + w1) + (w2 + w3).
template <typename E>
__global__ __launch_bounds__(GRN_SUM_THREADS) void grn_sumsq_kernel(const uint16_t* __restrict__ x, float* __restrict__ part, long R, long L,
                                                                     int rpc) {
  __shared__ __attribute__((aligned(16))) float red[4][GRN_SUM_COLS];
  const int tid = threadIdx.x, q = tid >> 6, lane = tid & 63;
  const long col = (long)blockIdx.x * GRN_SUM_COLS + lane * 8;
  const bool live = col < L;                             // L % 8 == 0: a lane's 8 columns are all inside or all outside
  const long r0 = (long)blockIdx.y * rpc;
  const long r1 = r0 + rpc < R ? r0 + rpc : R;
  const int b = blockIdx.z;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) {
    const uint16_t* src = x + ((size_t)b * R + r0 + q) * L + col;
    long r = r0 + q;
    for (; r + 12 < r1; r += 16) {                       // rows r, r + 4, r + 8, r + 12: four loads in flight, added in row order
      u32x4 v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const u32x4*>(src + (size_t)(4 * k) * L);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float f[8];
        grn_unpack8<E>(v[k], f);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = fmaf(f[i], f[i], acc[i]);
      }
      src += (size_t)16 * L;
    }
    for (; r < r1; r += 4) {
      float f[8];
      grn_unpack8<E>(*reinterpret_cast<const u32x4*>(src), f);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = fmaf(f[i], f[i], acc[i]);
      src += (size_t)4 * L;
    }
  }
  *reinterpret_cast<f32x4*>(&red[q][lane * 8]) = (f32x4){acc[0], acc[1], acc[2], acc[3]};
  *reinterpret_cast<f32x4*>(&red[q][lane * 8 + 4]) = (f32x4){acc[4], acc[5], acc[6], acc[7]};
  __syncthreads();
  const long c2 = (long)blockIdx.x * GRN_SUM_COLS + 2 * tid;      // thread t adds columns 2t, 2t + 1 of the four waves
  if (c2 < L) {                                                   // L is even
    const f32x2 a0 = *reinterpret_cast<const f32x2*>(&red[0][2 * tid]), a1 = *reinterpret_cast<const f32x2*>(&red[1][2 * tid]);
    const f32x2 a2 = *reinterpret_cast<const f32x2*>(&red[2][2 * tid]), a3 = *reinterpret_cast<const f32x2*>(&red[3][2 * tid]);
    *reinterpret_cast<f32x2*>(part + ((size_t)b * gridDim.y + blockIdx.y) * L + c2) = (a0 + a1) + (a2 + a3);
  }
}

// Sum of part[b][c][w][n .. n+3] over the chunks c, ascending, eight loads in flight (a chunk past the end adds an exact zero).
__device__ __forceinline__ f32x4 grn_sum_chunks(const float* p, size_t stride, int count) {
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < count; c += 8) {
    f32x4 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      v[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (c + k < count) v[k] = *reinterpret_cast<const f32x4*>(p + (size_t)(c + k) * stride);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s += v[k];
  }
  return s;
}

// Workgroup-wide sum of one float per thread, the same value in every thread: wave butterflies, then the four wave sums in a fixed order.
// Not wave.hpp's block_sum: no barrier in front (wsum is written once per launch) and the wave sums are added left to right.
__device__ __forceinline__ float grn_block_sum(float v, float* wsum) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// grid (W, B), 256 threads, a thread owns 4 consecutive n.  over_w = 0: scale[b][w][n] = 1 + gamma[n] * Nx.  over_w = 1: only the sums
// of squares over the chunks, sq[b][w][n], into the same table; grn_finalize_w_kernel turns them into the scale.
__global__ __launch_bounds__(GRN_FIN_THREADS) void grn_finalize_kernel(const float* __restrict__ part, const float* __restrict__ gamma,
                                                                        float* __restrict__ scale, int nchunks, int W, int N, int over_w) {
  __shared__ float wsum[GRN_FIN_THREADS / 64];
  const int tid = threadIdx.x, w = blockIdx.x, b = blockIdx.y;
  const size_t L = (size_t)W * N;
  const float* pb = part + (size_t)b * nchunks * L + (size_t)w * N;
  float* sc = scale + (size_t)b * L + (size_t)w * N;
  f32x4 g[GRN_MAX_N / (4 * GRN_FIN_THREADS)];
  float local = 0.f;
#pragma unroll
  for (int j = 0; j < GRN_MAX_N / (4 * GRN_FIN_THREADS); ++j) {
    const int n = 4 * (tid + j * GRN_FIN_THREADS);
    g[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (n < N) {
      const f32x4 s = grn_sum_chunks(pb + n, L, nchunks);
      if (over_w) {
        *reinterpret_cast<f32x4*>(sc + n) = s;
      } else {
        g[j] = (f32x4){sqrtf(s[0]), sqrtf(s[1]), sqrtf(s[2]), sqrtf(s[3])};
        local += (g[j][0] + g[j][1]) + (g[j][2] + g[j][3]);
      }
    }
  }
  if (over_w) return;
  const float inv = 1.0f / (grn_block_sum(local, wsum) / (float)N + 1e-6f);
#pragma unroll
  for (int j = 0; j < GRN_MAX_N / (4 * GRN_FIN_THREADS); ++j) {
    const int n = 4 * (tid + j * GRN_FIN_THREADS);
    if (n < N) {
      const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + n);
      f32x4 s;
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] = fmaf(gm[k], g[j][k] * inv, 1.0f);
      *reinterpret_cast<f32x4*>(sc + n) = s;
    }
  }
}

// over_w = 1 only.  grid (B), 256 threads: sq[b][w][n] summed over w in ascending order, the roots, the mean over n, and the one scale
// per (b, n) written to every w of scale[b][w][n] (each thread overwrites only what it has read itself).
__global__ __launch_bounds__(GRN_FIN_THREADS) void grn_finalize_w_kernel(const float* __restrict__ gamma, float* scale, int W, int N) {
  __shared__ float wsum[GRN_FIN_THREADS / 64];
  const int tid = threadIdx.x, b = blockIdx.x;
  float* sc = scale + (size_t)b * W * N;
  f32x4 g[GRN_MAX_N / (4 * GRN_FIN_THREADS)];
  float local = 0.f;
#pragma unroll
  for (int j = 0; j < GRN_MAX_N / (4 * GRN_FIN_THREADS); ++j) {
    const int n = 4 * (tid + j * GRN_FIN_THREADS);
    g[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (n < N) {
      const f32x4 s = grn_sum_chunks(sc + n, (size_t)N, W);
      g[j] = (f32x4){sqrtf(s[0]), sqrtf(s[1]), sqrtf(s[2]), sqrtf(s[3])};
      local += (g[j][0] + g[j][1]) + (g[j][2] + g[j][3]);
    }
  }
  const float inv = 1.0f / (grn_block_sum(local, wsum) / (float)N + 1e-6f);
#pragma unroll
  for (int j = 0; j < GRN_MAX_N / (4 * GRN_FIN_THREADS); ++j) {
    const int n = 4 * (tid + j * GRN_FIN_THREADS);
    if (n < N) {
      const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + n);
      f32x4 s;
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] = fmaf(gm[k], g[j][k] * inv, 1.0f);
      for (int w = 0; w < W; ++w) *reinterpret_cast<f32x4*>(sc + (size_t)w * N + n) = s;
    }
  }
}

template <typename E>
__global__ __launch_bounds__(GRN_THREADS) void grn_apply_kernel(const uint16_t* x, uint16_t* y,      // may alias (in place)
                                                                 const float* __restrict__ scale, const float* __restrict__ beta, long R,
                                                                 long L, int N, int rpc) {
  fp16_saturate_mode();
  const long col = ((long)blockIdx.x * GRN_THREADS + threadIdx.x) * 8;
  if (col >= L) return;
  const long r0 = (long)blockIdx.y * rpc;
  const long r1 = r0 + rpc < R ? r0 + rpc : R;
  const int b = blockIdx.z;
  const int n0 = (int)(col % N);                         // N % 8 == 0: the 8 columns are 8 consecutive channels of one w
  float s[8], be[8];
  {
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(scale + (size_t)b * L + col);
    const f32x4 s1 = *reinterpret_cast<const f32x4*>(scale + (size_t)b * L + col + 4);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + n0);
    const f32x4 b1 = *reinterpret_cast<const f32x4*>(beta + n0 + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s[i] = s0[i]; s[i + 4] = s1[i];
      be[i] = b0[i]; be[i + 4] = b1[i];
    }
  }
  const size_t off = ((size_t)b * R + r0) * L + col;
  const uint16_t* src = x + off;
  uint16_t* dst = y + off;
  auto one = [&](const u32x4 v, uint16_t* d) {
    float f[8];
    grn_unpack8<E>(v, f);
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = E::pack2(fmaf(f[2 * i], s[2 * i], be[2 * i]), fmaf(f[2 * i + 1], s[2 * i + 1], be[2 * i + 1]));
    *reinterpret_cast<u32x4*>(d) = o;
  };
  long r = r0;
  for (; r + 4 <= r1; r += 4) {
    u32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const u32x4*>(src + (size_t)k * L);
#pragma unroll
    for (int k = 0; k < 4; ++k) one(v[k], dst + (size_t)k * L);
    src += (size_t)4 * L;
    dst += (size_t)4 * L;
  }
  for (; r < r1; ++r) {
    one(*reinterpret_cast<const u32x4*>(src), dst);
    src += L;
    dst += L;
  }
}

static int grn_check(const KvqGrnArgs* a, const char* who) {
  KVQ_REQUIRE(a && a->x && a->gamma && a->beta && a->ws, KVQ_ERR_NULL, "%s: NULL pointer", who);
  KVQ_REQUIRE_OPERAND(who, a->dtype);
  KVQ_REQUIRE((((uintptr_t)a->x | (uintptr_t)a->y | (uintptr_t)a->ws | (uintptr_t)a->gamma | (uintptr_t)a->beta) & 15) == 0, KVQ_ERR_UNSUPPORTED,
              "%s: x, y, ws, gamma and beta must be 16-byte aligned", who);
  KVQ_REQUIRE(a->B >= 1 && kvq_grn_supported(a->N, a->D, a->H, a->W), KVQ_ERR_UNSUPPORTED,
              "%s: unsupported shape (B=%d D=%d H=%d W=%d N=%d; N in {384,768,1536,3072})", who, a->B, a->D, a->H, a->W, a->N);
  const long L = (long)a->W * a->N, R = (long)a->D * a->H;
  KVQ_REQUIRE(a->B <= 65535 && a->W <= 65535 && L < (1L << 31) && R < (1L << 31), KVQ_ERR_SHAPE,
              "%s: B=%d, D*H=%ld or W*N=%ld exceed the grid", who, a->B, R, L);
  return KVQ_OK;
}

}  // namespace kvq

extern "C" int kvq_grn_supported(int N, int D, int H, int W) {
  return (N == 384 || N == 768 || N == 1536 || N == 3072) && D >= 1 && H >= 1 && W >= 1;
}

extern "C" size_t kvq_grn_workspace_bytes(int B, int D, int H, int W, int N) {
  if (B < 1 || !kvq_grn_supported(N, D, H, W)) return 0;
  const kvq::GrnPlan p = kvq::grn_plan(B, D, H, W, N);
  return sizeof(float) * (size_t)B * (size_t)p.L * (size_t)(1 + p.nchunks);     // scale[B][W][N], then part[B][nchunks][W][N]
}

extern "C" int kvq_grn_stats(const KvqGrnArgs* a, void* stream) {
  using namespace kvq;
  if (int rc = grn_check(a, "kvq_grn_stats")) return rc;
  const GrnPlan p = grn_plan(a->B, a->D, a->H, a->W, a->N);
  KVQ_REQUIRE(p.nchunks <= 65535, KVQ_ERR_SHAPE, "kvq_grn_stats: %d row chunks exceed the grid", p.nchunks);
  float* scale = a->ws;
  float* part = a->ws + (size_t)a->B * p.L;
  dim3 grid((unsigned)p.sgroups, (unsigned)p.nchunks, (unsigned)a->B), block(GRN_SUM_THREADS);
  if (int rc = with_operand(a->dtype, [&](auto e) {
        return launch("grn_sumsq_kernel", grn_sumsq_kernel<decltype(e)>, grid, block, 0, stream, a->x, part, p.R, p.L, p.rpc);
      }))
    return rc;
  dim3 fgrid((unsigned)a->W, (unsigned)a->B), fblock(GRN_FIN_THREADS);
  if (int rc = launch("grn_finalize_kernel", grn_finalize_kernel, fgrid, fblock, 0, stream, part, a->gamma, scale, p.nchunks, a->W, a->N,
                      a->over_w ? 1 : 0))
    return rc;
  if (!a->over_w) return KVQ_OK;
  return launch("grn_finalize_w_kernel", grn_finalize_w_kernel, dim3((unsigned)a->B), fblock, 0, stream, a->gamma, scale, a->W, a->N);
}

extern "C" int kvq_grn_apply(const KvqGrnArgs* a, void* stream) {
  using namespace kvq;
  if (int rc = grn_check(a, "kvq_grn_apply")) return rc;
  const GrnPlan p = grn_plan(a->B, a->D, a->H, a->W, a->N);
  KVQ_REQUIRE(p.achunks <= 65535, KVQ_ERR_SHAPE, "kvq_grn_apply: %d row chunks exceed the grid", p.achunks);
  uint16_t* y = a->y ? a->y : const_cast<uint16_t*>(a->x);
  dim3 grid((unsigned)p.colgroups, (unsigned)p.achunks, (unsigned)a->B), block(GRN_THREADS);
  return with_operand(a->dtype, [&](auto e) {
    return launch("grn_apply_kernel", grn_apply_kernel<decltype(e)>, grid, block, 0, stream, a->x, y, a->ws, a->beta, p.R, p.L, a->N, p.arpc);
  });
}
