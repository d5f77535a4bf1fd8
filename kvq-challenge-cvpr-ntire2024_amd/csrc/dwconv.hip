// Depthwise (kt,7,7) 3D convolution + LayerNorm over C, one launch (gfx950): Block3D.dwconv + Block3D.norm of the ConvNeXt-3D trunk
// (conv_backbone.py:166-167, :177-179).
//
//   x     fp32 channels-last (B, T, H, W, C) — the residual stream, read only
//   w     fp32 [kt*7*7][C], tap-major (tap = (dt*7 + ky)*7 + kx): the four channels of a lane are one 16-B load
//   out   rows [B*T*H*W][C]: LN_C(conv(x) + bias) * ln_w + ln_b, 16-bit operand rows or fp32
//
// Work split.  A lane owns four consecutive channels (NQ = C/4 lanes cover a token) and a STRIP of seven consecutive output pixels of
// one row; a workgroup of 192 threads holds NS = 768/C strips (8 / 4 / 2 / 1 at C = 96 / 192 / 384 / 768), so every channel of a token
// is live in ONE workgroup at the same time and the conv result never leaves the registers: the row statistics are reduced over the
// NQ lanes (xor butterflies inside aligned groups of NQ/3 lanes, the three group sums through 672 B of LDS, added in a fixed order).
// Per (slice dt, kernel row ky) a lane loads the 13 input pixels its strip sees and the 7 taps of the row (coalesced 16-B loads,
// NQ lanes = 16 C contiguous bytes per pixel) and runs 7 x 7 x 4 FMAs with the window sliding along W in registers.  Zero padding is a
// predicate on the load; the batch element is part of the strip index, so no halo can cross a clip.  Taps are accumulated in the one
// order (dt, ky, kx): two launches are bit-equal.  Statistics: two passes over the registers (mean, then centred squares), biased
// variance, eps inside the rsqrt — the formula of ln.hip.
#include "common.hpp"

namespace kvq {

struct DwParams {
  const float* x;
  const float* w;
  const float* bias;
  const float* gamma;
  const float* beta;
  int B, T, H, W, C, kt;
  int nsx;            // strips per row = ceil(W / 7)
  long n_strips;      // B * T * H * nsx
  float eps;
  uint16_t* out_h;
  float* out_f32;
};

constexpr int DW_S = 7;             // output pixels per strip
constexpr int DW_IN = DW_S + 6;     // input pixels a strip sees per row
constexpr int DW_THREADS = 192;

template <typename E, int NQ>
__global__ __launch_bounds__(DW_THREADS) void dwconv3d_ln_kernel(DwParams p) {
  fp16_saturate_mode();
  constexpr int NS = DW_THREADS / NQ;      // strips per workgroup
  constexpr int GW = NQ / 3;               // reduction group: 8 / 16 / 32 / 64 lanes, aligned inside a wave
  constexpr int NG = DW_THREADS / GW;      // groups per workgroup = 3 NS
  __shared__ float part[2][NG][DW_S];

  const int tid = threadIdx.x;
  const int slot = tid / NQ, q = tid - slot * NQ, c0 = 4 * q;
  long strip = (long)blockIdx.x * NS + slot;
  const bool live = strip < p.n_strips;
  if (!live) strip = p.n_strips - 1;       // clamp: every lane stays in the shuffles and the barriers
  const int sx = (int)(strip % p.nsx);
  long r = strip / p.nsx;
  const int y = (int)(r % p.H); r /= p.H;
  const int t = (int)(r % p.T);
  const int b = (int)(r / p.T);
  const int x0 = sx * DW_S;

  f32x4 acc[DW_S];
  {
    const f32x4 bs = *reinterpret_cast<const f32x4*>(p.bias + c0);
#pragma unroll
    for (int j = 0; j < DW_S; ++j) acc[j] = bs;
  }
  const int pt = p.kt / 2;
  for (int dt = 0; dt < p.kt; ++dt) {
    const int it = t + dt - pt;
    if ((unsigned)it >= (unsigned)p.T) continue;
    for (int ky = 0; ky < 7; ++ky) {
      const int iy = y + ky - 3;
      if ((unsigned)iy >= (unsigned)p.H) continue;
      const float* row = p.x + (((size_t)b * p.T + it) * p.H + iy) * (size_t)p.W * p.C + c0;
      f32x4 in[DW_IN];
#pragma unroll
      for (int i = 0; i < DW_IN; ++i) {
        const int ix = x0 - 3 + i;
        in[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if ((unsigned)ix < (unsigned)p.W) in[i] = *reinterpret_cast<const f32x4*>(row + (size_t)ix * p.C);
      }
      const float* wr = p.w + (size_t)((dt * 7 + ky) * 7) * p.C + c0;
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + (size_t)kx * p.C);
#pragma unroll
        for (int j = 0; j < DW_S; ++j)
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[j][k] = fmaf(in[j + kx][k], wv[k], acc[j][k]);
      }
    }
  }

  // ---- LayerNorm over the NQ lanes of the strip, seven tokens at once
  const int grp = tid / GW, g0 = 3 * slot;
  float s[DW_S];
#pragma unroll
  for (int j = 0; j < DW_S; ++j) {
    s[j] = (acc[j][0] + acc[j][1]) + (acc[j][2] + acc[j][3]);
#pragma unroll
    for (int o = GW / 2; o > 0; o >>= 1) s[j] += __shfl_xor(s[j], o, GW);
  }
  if (tid % GW == 0) {
#pragma unroll
    for (int j = 0; j < DW_S; ++j) part[0][grp][j] = s[j];
  }
  __syncthreads();
  float mean[DW_S];
#pragma unroll
  for (int j = 0; j < DW_S; ++j) mean[j] = ((part[0][g0][j] + part[0][g0 + 1][j]) + part[0][g0 + 2][j]) / (float)p.C;
#pragma unroll
  for (int j = 0; j < DW_S; ++j) {
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = acc[j][k] - mean[j];
      sq += d * d;
    }
#pragma unroll
    for (int o = GW / 2; o > 0; o >>= 1) sq += __shfl_xor(sq, o, GW);
    s[j] = sq;
  }
  if (tid % GW == 0) {
#pragma unroll
    for (int j = 0; j < DW_S; ++j) part[1][grp][j] = s[j];
  }
  __syncthreads();
  if (!live) return;
  const f32x4 gm = *reinterpret_cast<const f32x4*>(p.gamma + c0);
  const f32x4 be = *reinterpret_cast<const f32x4*>(p.beta + c0);
  const size_t tok0 = (((size_t)b * p.T + t) * p.H + y) * (size_t)p.W + x0;
#pragma unroll
  for (int j = 0; j < DW_S; ++j) {
    if (x0 + j >= p.W) break;
    const float rstd = rsqrtf(((part[1][g0][j] + part[1][g0 + 1][j]) + part[1][g0 + 2][j]) / (float)p.C + p.eps);
    f32x4 yv;
#pragma unroll
    for (int k = 0; k < 4; ++k) yv[k] = (acc[j][k] - mean[j]) * rstd * gm[k] + be[k];
    if (p.out_h) {
      const u32x2 o = {E::pack2(yv[0], yv[1]), E::pack2(yv[2], yv[3])};
      *reinterpret_cast<u32x2*>(p.out_h + (tok0 + j) * p.C + c0) = o;
    } else {
      *reinterpret_cast<f32x4*>(p.out_f32 + (tok0 + j) * p.C + c0) = yv;
    }
  }
}

template <typename E, int NQ>
static int launch_dw(const DwParams& p, hipStream_t st) {
  return launch("dwconv3d_ln_kernel", dwconv3d_ln_kernel<E, NQ>, grid_1d(p.n_strips, DW_THREADS / NQ), dim3(DW_THREADS), 0, st, p);
}

template <typename E>
static int launch_dw_c(const DwParams& p, hipStream_t st) {
  switch (p.C) {
    case 96: return launch_dw<E, 24>(p, st);
    case 192: return launch_dw<E, 48>(p, st);
    case 384: return launch_dw<E, 96>(p, st);
    default: return launch_dw<E, 192>(p, st);
  }
}

}  // namespace kvq

extern "C" int kvq_dwconv3d_ln_supported(int C, int kt, int T, int H, int W) {
  return (C == 96 || C == 192 || C == 384 || C == 768) && (kt == 1 || kt == 3) && T >= 1 && H >= 1 && W >= 1;
}

extern "C" int kvq_dwconv3d_ln(const KvqDwconvLnArgs* a, void* stream) {
  using namespace kvq;
  KVQ_REQUIRE(a && a->x && a->w && a->bias && a->ln_w && a->ln_b, KVQ_ERR_NULL, "kvq_dwconv3d_ln: NULL pointer");
  KVQ_REQUIRE((a->out_h != nullptr) != (a->out_f32 != nullptr), KVQ_ERR_NULL,
              "kvq_dwconv3d_ln: exactly one of out_h/out_f32 must be set");
  KVQ_REQUIRE(a->out_f32 || a->dtype == KVQ_DT_BF16 || a->dtype == KVQ_DT_FP16, KVQ_ERR_UNSUPPORTED, "kvq_dwconv3d_ln: dtype %d", a->dtype);
  KVQ_REQUIRE(a->B >= 1 && kvq_dwconv3d_ln_supported(a->C, a->kt, a->T, a->H, a->W), KVQ_ERR_UNSUPPORTED,
              "kvq_dwconv3d_ln: unsupported shape (B=%d T=%d H=%d W=%d C=%d kt=%d; C in {96,192,384,768}, kt in {1,3})", a->B, a->T, a->H,
              a->W, a->C, a->kt);
  DwParams p{a->x, a->w, a->bias, a->ln_w, a->ln_b, a->B, a->T, a->H, a->W, a->C, a->kt};
  p.nsx = ceil_div(a->W, DW_S);
  p.n_strips = (long)a->B * a->T * a->H * p.nsx;
  KVQ_REQUIRE(p.n_strips < (1L << 31), KVQ_ERR_SHAPE, "kvq_dwconv3d_ln: %ld strips exceed the grid", p.n_strips);
  p.eps = a->eps; p.out_h = a->out_h; p.out_f32 = a->out_f32;
  return with_operand(a->dtype, [&](auto e) { return launch_dw_c<decltype(e)>(p, (hipStream_t)stream); });
}
