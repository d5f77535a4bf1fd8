// Antialiased bilinear resize (+ crop + normalise): torchvision >= 0.17's Resize on a tensor == F.interpolate(mode="bilinear",
// align_corners=False, antialias=True) (get_resize_function, fusion_datasets.py:229-241), with the same crop, round_u8 and
// (v-mean)/std tail as kvq_resize_bilinear (misc.hip).
//
// Separable triangle filter whose support grows with the downscale factor, per axis: scale = in/out, support = max(scale, 1),
// center = scale*(i+0.5), window [xmin, xmin+xsize) with xmin = max(int(center-support+0.5), 0), xsize = min(int(center+support+0.5),
// in) - xmin, weight_j = max(0, 1 - |(j+xmin-center+0.5)/max(scale,1)|), normalised to sum 1.  Width first, then height, in fp32.
//
// One launch, no workspace.  A workgroup owns one (c, t) plane and a band of output rows: it builds both tap tables in LDS
// (aa_taps below, shared with the host entry kvq_resize_aa_taps), streams the band's source rows through a 16 KiB LDS stage in
// coalesced 16-B loads (the next chunk in flight in registers while the current one is filtered), keeps the width-filtered
// rows [rows][ow] in LDS and finishes with the height filter straight into the fp32 output.  Adjacent bands of a plane share the
// rows where their windows overlap; they are neighbours in the grid, so that re-read meets the L2.
#include "common.hpp"

namespace kvq {

constexpr int AA_THREADS = 256;
constexpr int AA_NV = 4;                                  // 16-B vectors per thread per staged chunk
constexpr int AA_STAGE = AA_THREADS * AA_NV * 16;         // 16 KiB of source bytes per chunk
constexpr int AA_HBUF = 48 * 1024;                        // width-filtered rows of a band (2 workgroups per CU)
constexpr int AA_MIN_BLOCKS = 512;

struct AaTaps {
  int start, size;
};

__host__ __device__ inline float aa_support(int in, int out) {
  const float scale = (float)in / (float)out;
  return scale >= 1.f ? scale : 1.f;
}

// capacity of one output index's tap list: xsize <= 2*support + 1 (+1 for the fp32 rounding of center)
__host__ __device__ inline int aa_kmax(int in, int out) { return (int)ceilf(2.f * aa_support(in, out)) + 2; }

// taps of output index i of an (in -> out) axis: window start / length, normalised weights into w[0..size)
__host__ __device__ inline AaTaps aa_taps(int i, int in, int out, int kmax, float* w) {
  const float scale = (float)in / (float)out;
  const float support = scale >= 1.f ? scale : 1.f;
  const float invscale = scale >= 1.f ? 1.f / scale : 1.f;
  const float center = scale * ((float)i + 0.5f);
  int xmin = (int)(center - support + 0.5f);
  xmin = xmin > 0 ? xmin : 0;
  int xmax = (int)(center + support + 0.5f);
  xmax = xmax < in ? xmax : in;
  int n = xmax - xmin;
  n = n < kmax ? n : kmax;
  float total = 0.f;
  for (int j = 0; j < n; ++j) {
    const float x = fabsf(((float)(j + xmin) - center + 0.5f) * invscale);
    const float wj = x < 1.f ? 1.f - x : 0.f;
    w[j] = wj;
    total += wj;
  }
  if (total != 0.f)
    for (int j = 0; j < n; ++j) w[j] /= total;
  return {xmin, n};
}

struct AaParams {
  const uint8_t* src;                       // the whole (C,T,H,W) tensor, as bytes
  const uint8_t* src_end;
  int T, H, W, rh, rw, cy, cx, oh, ow;
  int kx, ky;                               // tap capacities of the width / height tables
  int band, nbands;                         // output rows per workgroup, workgroups per plane
  int cap_rows;                             // rows of the width-filtered buffer
  int rch;                                  // source rows per staged chunk
  int round_u8, normalise;
  float mean[4], std[4];
  float* out;
};

template <typename S>
__device__ __forceinline__ float aa_ld(const uint8_t* stage, int elem_off) {
  if constexpr (sizeof(S) == 1) return (float)stage[elem_off];
  else return *reinterpret_cast<const float*>(stage + (size_t)elem_off * 4);
}

template <typename S>
__global__ __launch_bounds__(AA_THREADS) void resize_aa_kernel(AaParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  constexpr int ES = (int)sizeof(S);
  const int tid = threadIdx.x;
  const int ow = p.ow, W = p.W;
  uint8_t* stage = lds;
  float* wx = reinterpret_cast<float*>(lds + AA_STAGE);     // [ow][kx]
  int* xs = reinterpret_cast<int*>(wx + (size_t)ow * p.kx);  // [ow]
  int* xn = xs + ow;                                         // [ow]
  float* wy = reinterpret_cast<float*>(xn + ow);             // [band][ky]
  int* ys = reinterpret_cast<int*>(wy + (size_t)p.band * p.ky);
  int* yn = ys + p.band;
  float* hbuf = reinterpret_cast<float*>(yn + p.band);       // [cap_rows][ow]

  const int bi = blockIdx.x % p.nbands, plane = blockIdx.x / p.nbands;
  const int c = plane / p.T;
  const int oy0 = bi * p.band;
  const int nb = min(p.band, p.oh - oy0);
  for (int i = tid; i < ow; i += AA_THREADS) {
    const AaTaps t = aa_taps(i + p.cx, W, p.rw, p.kx, wx + (size_t)i * p.kx);
    xs[i] = t.start; xn[i] = t.size;
  }
  for (int i = tid; i < nb; i += AA_THREADS) {
    const AaTaps t = aa_taps(oy0 + i + p.cy, p.H, p.rh, p.ky, wy + (size_t)i * p.ky);
    ys[i] = t.start; yn[i] = t.size;
  }
  __syncthreads();
  const int ry0 = ys[0];
  const int ry1 = min(ys[nb - 1] + yn[nb - 1], ry0 + p.cap_rows);   // the host sized cap_rows for the band: the min never binds
  const int nrows = ry1 - ry0;
  const int nchunks = (nrows + p.rch - 1) / p.rch;
  const uintptr_t lo = reinterpret_cast<uintptr_t>(p.src), hi = reinterpret_cast<uintptr_t>(p.src_end);
  const uintptr_t plane_b = lo + (uintptr_t)plane * p.H * W * ES;

  // chunk k = source rows [ry0 + k*rch, min(+rch, ry1)): one contiguous byte run, staged from its 16-B aligned start
  u32x4 reg[AA_NV];
  auto fetch = [&](int k) {
    const int r0 = ry0 + k * p.rch, r1 = min(r0 + p.rch, ry1);
    const uintptr_t gs = plane_b + (uintptr_t)r0 * W * ES, ge = plane_b + (uintptr_t)r1 * W * ES;
    const uintptr_t A = gs & ~(uintptr_t)15;
#pragma unroll
    for (int v = 0; v < AA_NV; ++v) {
      const uintptr_t a = A + (uintptr_t)(v * AA_THREADS + tid) * 16;
      if (a >= ge) continue;
      if (a >= lo && a + 16 <= hi) {
        reg[v] = *reinterpret_cast<const u32x4*>(a);
      } else {                                  // a vector across the tensor's first / last byte: only the bytes inside
        union { u32x4 q; uint8_t b[16]; } u;
        for (int e = 0; e < 16; ++e) u.b[e] = (a + e >= lo && a + e < hi) ? *reinterpret_cast<const uint8_t*>(a + e) : 0;
        reg[v] = u.q;
      }
    }
  };
  fetch(0);
  for (int k = 0; k < nchunks; ++k) {
    const int r0 = ry0 + k * p.rch, r1 = min(r0 + p.rch, ry1), rows = r1 - r0;
    const uintptr_t gs = plane_b + (uintptr_t)r0 * W * ES, ge = plane_b + (uintptr_t)r1 * W * ES;
    const uintptr_t A = gs & ~(uintptr_t)15;
    __syncthreads();                            // the previous chunk's readers are done with the stage
#pragma unroll
    for (int v = 0; v < AA_NV; ++v) {
      const int o = (v * AA_THREADS + tid) * 16;
      if (A + o < ge) *reinterpret_cast<u32x4*>(stage + o) = reg[v];
    }
    __syncthreads();
    if (k + 1 < nchunks) fetch(k + 1);          // in flight while this chunk is filtered
    // width filter: a work item = 4 rows x one output column, the column's weights read once for the 4 rows
    const int base = (int)(gs - A) / ES;        // element offset of (r0, 0) in the stage
    const int groups = (rows + 3) >> 2;
    for (int i = tid; i < groups * ow; i += AA_THREADS) {
      const int g = i / ow, ox = i - g * ow;
      const int x0 = xs[ox], n = xn[ox];
      const float* w = wx + (size_t)ox * p.kx;
      int off[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) off[rr] = base + min(g * 4 + rr, rows - 1) * W + x0;
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < n; ++j) {
        const float wj = w[j];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) acc[rr] += wj * aa_ld<S>(stage, off[rr] + j);
      }
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        if (g * 4 + rr < rows) hbuf[(size_t)(r0 - ry0 + g * 4 + rr) * ow + ox] = acc[rr];
    }
  }
  __syncthreads();
  // height filter + round / normalise; ox fastest -> coalesced rows of the output
  const float m = p.mean[c], sd = p.std[c];
  float* dst = p.out + ((size_t)plane * p.oh + oy0) * ow;
  for (int i = tid; i < nb * ow; i += AA_THREADS) {
    const int oyl = i / ow, ox = i - oyl * ow;
    const float* w = wy + (size_t)oyl * p.ky;
    const int y0 = ys[oyl] - ry0, n = yn[oyl];
    float v = 0.f;
    for (int j = 0; j < n; ++j) v += w[j] * hbuf[(size_t)min(y0 + j, nrows - 1) * ow + ox];
    if (p.round_u8) v = fminf(fmaxf(rintf(v), 0.f), 255.f);
    if (p.normalise) v = (v - m) / sd;
    dst[i] = v;
  }
}

}  // namespace kvq

extern "C" int kvq_resize_aa_taps(int in_size, int out_size, int32_t* kmax, int32_t* start, int32_t* size, float* weights) {
  using namespace kvq;
  KVQ_REQUIRE(kmax, KVQ_ERR_NULL, "kvq_resize_aa_taps: NULL kmax");
  KVQ_REQUIRE(in_size > 0 && out_size > 0, KVQ_ERR_SHAPE, "kvq_resize_aa_taps: sizes must be positive");
  const int K = aa_kmax(in_size, out_size);
  *kmax = K;
  if (!start && !size && !weights) return KVQ_OK;
  KVQ_REQUIRE(start && size && weights, KVQ_ERR_NULL, "kvq_resize_aa_taps: start / size / weights must all be given");
  for (int i = 0; i < out_size; ++i) {
    float* w = weights + (size_t)i * K;
    for (int j = 0; j < K; ++j) w[j] = 0.f;
    const AaTaps t = aa_taps(i, in_size, out_size, K, w);
    start[i] = t.start;
    size[i] = t.size;
  }
  return KVQ_OK;
}

extern "C" int kvq_resize_bilinear_aa(const void* video, int src_is_u8, int C, int T, int H, int W, int rh, int rw, int cy,
                                      int cx, int oh, int ow, int round_u8, const float* host_mean, const float* host_std,
                                      float* out, void* stream) {
  using namespace kvq;
  KVQ_REQUIRE(src_is_u8 == KVQ_SRC_F32 || src_is_u8 == KVQ_SRC_U8, KVQ_ERR_UNSUPPORTED, "kvq_resize_bilinear_aa: frame type %d (convert I420 frames first: kvq_yuv420_to_rgb)", src_is_u8);
  KVQ_REQUIRE(video && out, KVQ_ERR_NULL, "kvq_resize_bilinear_aa: NULL pointer");
  KVQ_REQUIRE(C > 0 && C <= 4 && T > 0 && H > 0 && W > 0 && rh > 0 && rw > 0 && oh > 0 && ow > 0 && cy >= 0 && cx >= 0 &&
                  cy + oh <= rh && cx + ow <= rw,
              KVQ_ERR_SHAPE, "kvq_resize_bilinear_aa: bad shape / crop outside the resized frame");
  const int es = src_is_u8 ? 1 : 4;
  KVQ_REQUIRE((long)W * es + 15 <= AA_STAGE, KVQ_ERR_UNSUPPORTED, "kvq_resize_bilinear_aa: a source row of %d B exceeds the %d B stage",
              W * es, AA_STAGE - 15);
  AaParams p{};
  p.src = reinterpret_cast<const uint8_t*>(video);
  p.src_end = p.src + (size_t)C * T * H * W * es;
  p.T = T; p.H = H; p.W = W; p.rh = rh; p.rw = rw; p.cy = cy; p.cx = cx; p.oh = oh; p.ow = ow;
  p.kx = aa_kmax(W, rw);
  p.ky = aa_kmax(H, rh);
  // rows a band of b output rows reads: scale*(b-1) + 2*support + 1, +2 for the fp32 rounding of the window ends
  const float sy = (float)H / (float)rh, supy = aa_support(H, rh);
  auto rows_for = [&](int b) { return std::min(H, (int)ceilf(sy * (float)(b - 1) + 2.f * supy) + 3); };
  const int planes = C * T;
  const int want_bands = (AA_MIN_BLOCKS + planes - 1) / planes;
  int band = std::max(1, (oh + want_bands - 1) / want_bands);
  while (band > 1 && (long)rows_for(band) * ow * 4 > AA_HBUF) --band;
  p.band = band;
  p.nbands = (oh + band - 1) / band;
  p.cap_rows = rows_for(band);
  const int rch = std::max(1, std::min(p.cap_rows, (AA_STAGE - 15) / (W * es)));
  p.rch = rch >= 4 ? rch & ~3 : rch;
  p.round_u8 = round_u8; p.normalise = host_std != nullptr; p.out = out;
  for (int c = 0; c < C; ++c) {
    p.mean[c] = host_mean ? host_mean[c] : 0.f;
    p.std[c] = host_std ? host_std[c] : 1.f;
  }
  const long lds = (long)AA_STAGE + (long)ow * p.kx * 4 + (long)ow * 8 + (long)band * p.ky * 4 + (long)band * 8 +
                   (long)p.cap_rows * ow * 4;
  KVQ_REQUIRE(lds <= 160 * 1024, KVQ_ERR_UNSUPPORTED, "kvq_resize_bilinear_aa: %ld B of LDS for %dx%d -> %dx%d (ow %d)", lds, H, W,
              rh, rw, ow);
  const long blocks = (long)planes * p.nbands;
  KVQ_REQUIRE(blocks < (1L << 31), KVQ_ERR_SHAPE, "kvq_resize_bilinear_aa: grid too large");
  return launch("resize_aa_kernel", src_is_u8 ? resize_aa_kernel<uint8_t> : resize_aa_kernel<float>, dim3((unsigned)blocks), dim3(AA_THREADS),
                (size_t)lds, stream, p);
}
