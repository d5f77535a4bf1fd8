// Quality paint (kvq_quality_paint, kvq_quality_paint_regions): the head's per-token scores drawn back onto the geometry of the source frames the fragment
// sampler read them from.  Store-bound, and most of what it stores is zeros.
//
// A gather: every output pixel finds the token rectangles that meet it, so there are no atomics and the result is a defined bit
// pattern.  One workgroup takes a (clip, depth slice, band of output rows).  It first compacts, in token order, the rectangles of the
// slice that meet the band's source rows into LDS (origin + score; a band no rectangle meets is plain zero fill), then every work
// item owns 4 consecutive output pixels and walks that short list.  The 4 pixels are aligned to 16 bytes in the FLAT output (a row
// of ceil(Ws / cell) floats need not be a multiple of 4 long): one 16-byte store each for heat and cover, scalar stores at the ends
// of a row.  The map is specified to the bit (include/kvq_hip.h): separately rounded multiplies and adds.  hipcc contracts
// a * b + c by default, and HIP's __fmul_rn / __fadd_rn are plain * and + that contract like any other (measured: the first build
// of this file differed from the numpy reference in the last bit), so the file is built with -ffp-contract=off (_build.EXTRA).  A
// file-scope "#pragma clang fp contract(off)" is NOT enough: it does not reach the header's inlined functions (checked in the ISA).
#include "common.hpp"
#include "yuv.hpp"

namespace kvq {

constexpr int QM_THREADS = 256;
constexpr int QM_MAX_TOK = 1024;

struct PaintParams {
  const void* video[KVQ_FRAG_MAX_CLIPS];
  const int32_t* hoff[KVQ_FRAG_MAX_CLIPS];
  const int32_t* woff[KVQ_FRAG_MAX_CLIPS];
  const void* const* table;     // KvqFragmentSource.indirect, or nullptr
  const float* tok;
  float* heat;
  float* cover;
  uint8_t* overlay;
  const float* range;
  long chan_stride;
  int Hs, Ws, Fw, fsh, fsw, aligned, nt;
  int D, Hf, Wf, sh, sw, cell, Ho, Wo;
  int band, groups;             // output rows per workgroup; 4-pixel groups per output row (alignment slack included)
  int vec;                      // heat and cover are 16-byte aligned
  int n_ov, alpha, dim;
  int ov_depth[16];
  // kvq_quality_paint_regions only (the REGION instantiations): the token grid covers one window of the canvas per clip frame
  int i420;                     // the overlay's frames are I420 (video[b] = the clip's first frame), converted with `yuv` (yuv.hpp)
  YuvCoef yuv;
  const int32_t* region;        // [n_clips][T] window index, row-major over nry x nrx window origins
  int T, anchor, nry, nrx, phase;
};

struct ActiveList {
  int r0[QM_MAX_TOK];
  int c0[QM_MAX_TOK];
  float s[QM_MAX_TOK];
  int cnt[QM_THREADS / 64];
};

// The rectangles of slice (b, d) that meet source rows [y0, y1), compacted in increasing token order.  All QM_THREADS threads call it.
// REGION: the token grid starts at the canvas origin of the window region[b][2d + phase] names instead of (0, 0); a value that names
// no window leaves the slice without rectangles (the same for every thread of the workgroup: it returns in front of the barriers).
template <bool REGION>
__device__ __forceinline__ int build_active(const PaintParams& p, int b, int d, int y0, int y1, ActiveList& a) {
  const int ntok = p.Hf * p.Wf, tt = (2 * d) / p.aligned;
  int oy = 0, ox = 0;
  if (REGION) {
    const int reg = p.region[(size_t)b * p.T + 2 * d + p.phase];
    if (reg < 0 || reg >= p.nry * p.nrx) return 0;
    const int ry = reg / p.nrx;
    oy = ry * p.anchor; ox = (reg - ry * p.nrx) * p.anchor;
  }
  const int32_t* ho = p.table ? reinterpret_cast<const int32_t*>(p.table[KVQ_FRAG_MAX_CLIPS + b]) : p.hoff[b];
  const int32_t* wo = p.table ? reinterpret_cast<const int32_t*>(p.table[2 * KVQ_FRAG_MAX_CLIPS + b]) : p.woff[b];
  const float* tok = p.tok + ((size_t)b * p.D + d) * ntok;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int total = 0;
  for (int base = 0; base < ntok; base += QM_THREADS) {
    const int k = base + threadIdx.x;
    bool on = false;
    int r0 = 0, c0 = 0;
    if (k < ntok) {
      const int ip = k / p.Wf, jp = k - ip * p.Wf;
      const int yy = oy + ip * p.sh, xx = ox + jp * p.sw;
      const int i = yy / p.fsh, j = xx / p.fsw;
      const int o = (i * p.Fw + j) * p.nt + tt;
      r0 = ho[o] + (yy - i * p.fsh);
      c0 = wo[o] + (xx - j * p.fsw);
      on = min(r0 + p.sh, y1) > max(r0, y0);
    }
    const unsigned long long m = __ballot(on);
    if (lane == 0) a.cnt[wave] = __popcll(m);
    __syncthreads();
    int off = total, all = 0;
#pragma unroll
    for (int w = 0; w < QM_THREADS / 64; ++w) {
      if (w < wave) off += a.cnt[w];
      all += a.cnt[w];
    }
    if (on) {
      const int at = off + __popcll(m & ((1ull << lane) - 1ull));
      a.r0[at] = r0; a.c0[at] = c0; a.s[at] = tok[k];
    }
    total += all;
    __syncthreads();
  }
  return total;
}

// sum_k area_k and sum_k float(area_k) * s_k over the list, for the source block [y0, y1) x [x0, x1)
__device__ __forceinline__ void gather_block(const PaintParams& p, const ActiveList& a, int n, int y0, int y1, int x0, int x1,
                                             int& area, float& acc) {
  area = 0; acc = 0.f;
  for (int k = 0; k < n; ++k) {
    const int r0 = a.r0[k], c0 = a.c0[k];
    const int ah = min(r0 + p.sh, y1) - max(r0, y0), aw = min(c0 + p.sw, x1) - max(c0, x0);
    if (ah > 0 && aw > 0) {
      area += ah * aw;
      acc = __fadd_rn(acc, __fmul_rn((float)(ah * aw), a.s[k]));
    }
  }
}

template <bool REGION>
__global__ __launch_bounds__(QM_THREADS) void quality_paint_kernel(PaintParams p) {
  __shared__ ActiveList a;
  const int b = blockIdx.z, d = blockIdx.y, Y0 = blockIdx.x * p.band;
  const int rows = min(p.band, p.Ho - Y0);
  const int n = build_active<REGION>(p, b, d, Y0 * p.cell, min((Y0 + rows) * p.cell, p.Hs), a);
  const size_t plane = ((size_t)b * p.D + d) * p.Ho;
  for (int item = threadIdx.x; item < rows * p.groups; item += QM_THREADS) {
    const int row = item / p.groups, g = item - row * p.groups;
    const int Y = Y0 + row;
    const size_t o = (plane + Y) * (size_t)p.Wo;
    const int X0 = 4 * g - (p.vec ? (int)(o & 3) : 0);      // o + X0 is a multiple of 4 elements
    if (X0 >= p.Wo) continue;
    const int y0 = Y * p.cell, y1 = min(y0 + p.cell, p.Hs);
    float h[4], c[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int X = X0 + e;
      h[e] = 0.f; c[e] = 0.f;
      if (n > 0 && X >= 0 && X < p.Wo) {
        const int x0 = X * p.cell, x1 = min(x0 + p.cell, p.Ws);
        int area; float acc;
        gather_block(p, a, n, y0, y1, x0, x1, area, acc);
        if (area > 0) {
          h[e] = __fdiv_rn(acc, (float)area);
          c[e] = __fdiv_rn((float)area, (float)((y1 - y0) * (x1 - x0)));
        }
      }
    }
    if (p.vec && X0 >= 0 && X0 + 4 <= p.Wo) {
      *reinterpret_cast<f32x4*>(p.heat + o + X0) = (f32x4){h[0], h[1], h[2], h[3]};
      *reinterpret_cast<f32x4*>(p.cover + o + X0) = (f32x4){c[0], c[1], c[2], c[3]};
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (X0 + e >= 0 && X0 + e < p.Wo) { p.heat[o + X0 + e] = h[e]; p.cover[o + X0 + e] = c[e]; }
    }
  }
}

// Overlay: one workgroup = (clip, overlay slice, band of source rows); a work item owns 4 consecutive pixels of a row in all three
// channel planes.  Integer blend, see kvq_hip.h.  REGION: the slice is drawn on the frame whose window it was painted with.
template <bool REGION>
__global__ __launch_bounds__(QM_THREADS) void quality_overlay_kernel(PaintParams p) {
  __shared__ ActiveList a;
  const int b = blockIdx.z, ov = blockIdx.y, y_lo = blockIdx.x * p.band;
  const int d = p.ov_depth[ov];
  const int rows = min(p.band, p.Hs - y_lo);
  const int n = build_active<REGION>(p, b, d, y_lo, y_lo + rows, a);
  const float lo = p.range[0], inv = __fdiv_rn(1.f, __fsub_rn(p.range[1], lo));
  const uint8_t* vid = reinterpret_cast<const uint8_t*>(p.table ? p.table[b] : p.video[b]);
  const size_t frame = (size_t)(2 * d + (REGION ? p.phase : 0)) * p.Hs * p.Ws, hw = (size_t)p.Hs * p.Ws;
  const I420Geom geo = i420_geom(p.Hs, p.Ws);
  const uint8_t* yuv_frame = vid + (size_t)(2 * d + (REGION ? p.phase : 0)) * geo.frame;      // i420 only
  uint8_t* out = p.overlay + ((size_t)b * p.n_ov + ov) * 3 * hw;
  for (int item = threadIdx.x; item < rows * p.groups; item += QM_THREADS) {
    const int row = item / p.groups, g = item - row * p.groups;
    const int y = y_lo + row, x0 = 4 * g;
    int col[4];             // -1: uncovered, else q
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      col[e] = -1;
      const int x = x0 + e;
      if (n > 0 && x < p.Ws) {
        int area; float acc;
        gather_block(p, a, n, y, y + 1, x, x + 1, area, acc);
        if (area > 0) {
          const float s = __fdiv_rn(acc, (float)area);
          const float t = fminf(fmaxf(__fmul_rn(__fsub_rn(s, lo), inv), 0.f), 1.f);
          col[e] = (int)rintf(__fmul_rn(t, 255.f));
        }
      }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const uint8_t* s8 = vid + (size_t)ch * p.chan_stride + frame + (size_t)y * p.Ws + x0;
      uint8_t* o8 = out + (size_t)ch * hw + (size_t)y * p.Ws + x0;
      uint32_t px[4], packed = 0;
      const bool full = x0 + 4 <= p.Ws;
      if (p.i420) {
#pragma unroll
        for (int e = 0; e < 4; ++e) px[e] = x0 + e < p.Ws ? (uint32_t)i420_pixel(yuv_frame, geo, p.yuv, ch, y, x0 + e) : 0u;
      } else if (full && ((size_t)s8 & 3) == 0) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(s8);
#pragma unroll
        for (int e = 0; e < 4; ++e) px[e] = (w >> (8 * e)) & 255u;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) px[e] = x0 + e < p.Ws ? s8[e] : 0u;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int q = col[e];
        const uint32_t colour = ch == 0 ? 255 - q : (ch == 1 ? q : 0);
        const uint32_t v = q < 0 ? (px[e] * p.dim + 128u) >> 8 : (px[e] * (256u - p.alpha) + colour * p.alpha + 128u) >> 8;
        px[e] = v;
        packed |= v << (8 * e);
      }
      if (full && ((size_t)o8 & 3) == 0) {
        *reinterpret_cast<uint32_t*>(o8) = packed;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (x0 + e < p.Ws) o8[e] = (uint8_t)px[e];
      }
    }
  }
}

// wh x ww: the part of the canvas the token grid covers — all of it (kvq_quality_paint) or one window (kvq_quality_paint_regions)
static bool paint_geometry_ok(const KvqFragmentSource* f, int T, int D, int Hf, int Wf, int cell, long wh, long ww) {
  if (!f || T <= 0 || D <= 0 || Hf <= 0 || Wf <= 0) return false;
  if (f->n_clips < 1 || f->n_clips > KVQ_FRAG_MAX_CLIPS) return false;
  if (f->Hs <= 0 || f->Ws <= 0 || f->Fh <= 0 || f->Fw <= 0 || f->fs_h <= 0 || f->fs_w <= 0 || f->aligned <= 0) return false;
  if (!(cell == 1 || cell == 2 || cell == 4 || cell == 8 || cell == 16 || cell == 32)) return false;
  if (T != 2 * D || f->aligned % 2 != 0 || T % f->aligned != 0) return false;
  if ((long)Hf * Wf > QM_MAX_TOK) return false;
  if (wh % Hf != 0 || ww % Wf != 0) return false;
  const long sh = wh / Hf, sw = ww / Wf;
  return f->fs_h % sh == 0 && f->fs_w % sw == 0;
}

static bool paint_canvas_ok(const KvqFragmentSource* f, int T, int D, int Hf, int Wf, int cell) {
  return f && f->Fh > 0 && f->Fw > 0 && f->fs_h > 0 && f->fs_w > 0 &&
         paint_geometry_ok(f, T, D, Hf, Wf, cell, (long)f->Fh * f->fs_h, (long)f->Fw * f->fs_w);
}

static bool paint_regions_ok(const KvqFragmentSource* f, int T, int D, int Hf, int Wf, int cell, int anchor, int kh, int kw) {
  if (!f || anchor <= 0 || kh <= 0 || kw <= 0) return false;
  if (!paint_geometry_ok(f, T, D, Hf, Wf, cell, (long)kh * anchor, (long)kw * anchor)) return false;
  const long ch = (long)f->Fh * f->fs_h, cw = (long)f->Fw * f->fs_w;
  if (ch % anchor != 0 || cw % anchor != 0 || kh > ch / anchor || kw > cw / anchor) return false;
  const long sh = (long)kh * anchor / Hf, sw = (long)kw * anchor / Wf;
  return anchor % sh == 0 && anchor % sw == 0;
}

// Both entry points: `rg` NULL paints the token grid over the whole canvas, else over the window of each frame.
static int paint_run(const char* who, const KvqQualityPaintArgs* a, const KvqQualityPaintRegionArgs* rg, void* stream) {
  const KvqFragmentSource* f = a->src;
  PaintParams p{};
  p.table = f->indirect;
  for (int b = 0; b < f->n_clips && !f->indirect; ++b) {
    KVQ_REQUIRE(f->hoff[b] && f->woff[b], KVQ_ERR_NULL, "%s: clip %d has a NULL draw pointer", who, b);
    p.video[b] = f->video[b]; p.hoff[b] = f->hoff[b]; p.woff[b] = f->woff[b];
  }
  p.tok = a->tok_map; p.heat = a->heat; p.cover = a->cover;
  p.chan_stride = f->chan_stride ? f->chan_stride : (long)a->T * f->Hs * f->Ws;
  p.Hs = f->Hs; p.Ws = f->Ws; p.Fw = f->Fw; p.fsh = f->fs_h; p.fsw = f->fs_w; p.aligned = f->aligned; p.nt = a->T / f->aligned;
  p.D = a->D; p.Hf = a->Hf; p.Wf = a->Wf; p.sh = f->Fh * f->fs_h / a->Hf; p.sw = f->Fw * f->fs_w / a->Wf; p.cell = a->cell;
  if (rg) {
    p.region = rg->region; p.T = a->T; p.anchor = rg->anchor; p.phase = rg->phase;
    p.sh = rg->kh * rg->anchor / a->Hf; p.sw = rg->kw * rg->anchor / a->Wf;
    p.nry = f->Fh * f->fs_h / rg->anchor - rg->kh + 1; p.nrx = f->Fw * f->fs_w / rg->anchor - rg->kw + 1;
  }
  p.Ho = ceil_div(f->Hs, a->cell); p.Wo = ceil_div(f->Ws, a->cell);
  KVQ_REQUIRE((long)f->n_clips * a->D * p.Ho * (long)p.Wo < (1L << 40) && a->D < 65536, KVQ_ERR_SHAPE, "%s: output too large", who);
  p.vec = (((size_t)a->heat | (size_t)a->cover) & 15) == 0;
  p.groups = ceil_div(p.Wo + 3, 4);
  p.band = QM_THREADS / p.groups > 0 ? QM_THREADS / p.groups : 1;
  if (p.band > p.Ho) p.band = p.Ho;
  if (a->overlay) {
    KVQ_REQUIRE(a->range, KVQ_ERR_NULL, "%s: an overlay needs the value range", who);
    KVQ_REQUIRE(f->src_is_u8 >= KVQ_SRC_U8 && f->src_is_u8 <= KVQ_SRC_I420_BT709_FULL, KVQ_ERR_UNSUPPORTED,
                "%s: the overlay is drawn on uint8 or I420 frames", who);
    p.i420 = yuv_format_ok(f->src_is_u8);
    KVQ_REQUIRE(!p.i420 || i420_size_ok(f->Hs, f->Ws), KVQ_ERR_SHAPE, "%s: I420 frames of %dx%d", who, f->Hs, f->Ws);
    if (p.i420) p.yuv = yuv420_coeffs(f->src_is_u8);
    KVQ_REQUIRE(a->n_ov >= 1 && a->n_ov <= 16 && a->alpha >= 0 && a->alpha <= 256 && a->dim >= 0 && a->dim <= 256, KVQ_ERR_SHAPE,
                "%s: n_ov %d (1..16), alpha %d, dim %d (0..256)", who, a->n_ov, a->alpha, a->dim);
    for (int n = 0; n < a->n_ov; ++n) {
      KVQ_REQUIRE(a->ov_depth[n] >= 0 && a->ov_depth[n] < a->D, KVQ_ERR_SHAPE, "%s: overlay depth %d outside 0..%d", who, a->ov_depth[n], a->D - 1);
      p.ov_depth[n] = a->ov_depth[n];
    }
    for (int b = 0; b < f->n_clips && !f->indirect; ++b)
      KVQ_REQUIRE(f->video[b], KVQ_ERR_NULL, "%s: clip %d has no frames", who, b);
  }
  const dim3 grid((unsigned)ceil_div(p.Ho, p.band), (unsigned)a->D, (unsigned)f->n_clips);
  if (int rc = launch("quality_paint_kernel", rg ? quality_paint_kernel<true> : quality_paint_kernel<false>, grid, dim3(QM_THREADS), 0, stream, p))
    return rc;
  if (!a->overlay) return KVQ_OK;
  p.overlay = a->overlay; p.range = a->range; p.n_ov = a->n_ov; p.alpha = a->alpha; p.dim = a->dim;
  p.groups = ceil_div(p.Ws, 4);
  p.band = QM_THREADS / p.groups > 0 ? QM_THREADS / p.groups : 1;
  if (p.band > p.Hs) p.band = p.Hs;
  const dim3 ogrid((unsigned)ceil_div(p.Hs, p.band), (unsigned)a->n_ov, (unsigned)f->n_clips);
  return launch("quality_overlay_kernel", rg ? quality_overlay_kernel<true> : quality_overlay_kernel<false>, ogrid, dim3(QM_THREADS), 0, stream, p);
}

}  // namespace kvq

extern "C" int kvq_quality_paint_supported(const KvqFragmentSource* src, int T, int D, int Hf, int Wf, int cell) {
  return kvq::paint_canvas_ok(src, T, D, Hf, Wf, cell) ? 1 : 0;
}

extern "C" int kvq_quality_paint(const KvqQualityPaintArgs* a, void* stream) {
  using namespace kvq;
  KVQ_REQUIRE(a && a->src && a->tok_map && a->heat && a->cover, KVQ_ERR_NULL, "kvq_quality_paint: NULL pointer");
  KVQ_REQUIRE(paint_canvas_ok(a->src, a->T, a->D, a->Hf, a->Wf, a->cell), KVQ_ERR_UNSUPPORTED,
              "kvq_quality_paint: geometry outside kvq_quality_paint_supported (T %d, token grid %d x %d x %d, cell %d)", a->T, a->D,
              a->Hf, a->Wf, a->cell);
  return paint_run("kvq_quality_paint", a, nullptr, stream);
}

extern "C" int kvq_quality_paint_regions_supported(const KvqFragmentSource* src, int T, int D, int Hf, int Wf, int cell, int anchor,
                                                   int kh, int kw) {
  return kvq::paint_regions_ok(src, T, D, Hf, Wf, cell, anchor, kh, kw) ? 1 : 0;
}

extern "C" int kvq_quality_paint_regions(const KvqQualityPaintRegionArgs* r, void* stream) {
  using namespace kvq;
  KVQ_REQUIRE(r && r->paint.src && r->paint.tok_map && r->paint.heat && r->paint.cover && r->region, KVQ_ERR_NULL,
              "kvq_quality_paint_regions: NULL pointer");
  const KvqQualityPaintArgs* a = &r->paint;
  KVQ_REQUIRE(paint_regions_ok(a->src, a->T, a->D, a->Hf, a->Wf, a->cell, r->anchor, r->kh, r->kw) && (r->phase == 0 || r->phase == 1),
              KVQ_ERR_UNSUPPORTED,
              "kvq_quality_paint_regions: geometry outside kvq_quality_paint_regions_supported (T %d, token grid %d x %d x %d, cell %d, "
              "windows of %d x %d anchors of %d, phase %d)", a->T, a->D, a->Hf, a->Wf, a->cell, r->kh, r->kw, r->anchor, r->phase);
  return paint_run("kvq_quality_paint_regions", a, r, stream);
}
