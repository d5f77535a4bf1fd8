// kvq_resize_pil: Pillow's Image.resize((ow, oh), BILINEAR) on uint8 RGB frames, to the bit — the frame transform of the motion-feature
// extractor (datasets/slowfast_clips.py: Resize([r, r]) on a PIL image, ToTensor, Normalize) without the host.  A fixed-point two-pass
// triangle filter: per axis 22-bit integer coefficients (resize_pil.hpp: built on the host in double, handed in as device tables, never
// derived here), one pass = clip8((sum px k + 2^21) >> 22), the width pass first and its result a uint8 image, the height pass on that
// image.  An axis that keeps its size has the coefficients {2^22, 0}: the pass returns its input, which is Pillow skipping it.  Every
// resized byte leaves through a 256-entry fp32 table of the caller's (ToTensor + Normalize evaluated once per byte value by the
// expression the host path uses; 0..255 gives the bytes back), into fp32 (T, 3, oh, ow) with caller-given frame and channel strides.
//
// Sources: uint8 frame-major interleaved (T, H, W, 3) — what the frame readers hand over, no permute copy — or I420 frames, converted
// where they are first loaded by the one conversion of yuv.hpp (bit-equal to kvq_yuv420_to_rgb + the uint8 path; no RGB frame in HBM).
//
// One launch, no workspace beyond the tables, no atomics, no data-dependent loop.  As resize_aa.hip: a workgroup owns one frame and
// a band of output rows.  It streams the band's source rows through a 16 KiB LDS stage of interleaved RGB — uint8 frames as one
// contiguous byte run in coalesced 16-byte loads, the next chunk in flight in registers while the current one is filtered; I420 rows
// 16 pixels per work item (one 16-byte luma load, two 8-byte chroma loads, three 16-byte LDS stores) — keeps the width-filtered rows
// as uint8 [rows][3][ow] in LDS and runs the height pass from there straight into the output.  At 1080 -> 224 a band of 8 output rows
// reads about 50 source rows: 33 KB of width-filtered bytes.  Adjacent bands share the rows where their windows overlap; they are
// neighbours in the grid, so that re-read meets the L2.
//
// The tables are device memory the host cannot read: every window is clamped to its axis and to the tap capacity where it is loaded,
// and every row index to the band's rows, so a table that does not belong to the geometry gives wrong pixels, never a wild address.
#include "resize_pil.hpp"
#include "yuv.hpp"

namespace kvq {

constexpr int PIL_THREADS = 256;
constexpr int PIL_NV = 4;                                   // 16-B vectors per thread per staged chunk
constexpr int PIL_STAGE = PIL_THREADS * PIL_NV * 16;        // 16 KiB of interleaved RGB per chunk
constexpr int PIL_HBUF = 48 * 1024;                         // width-filtered rows of a band (2 workgroups per CU)
constexpr int PIL_MIN_BLOCKS = 512;
constexpr int PIL_LDS_MAX = 160 * 1024;
constexpr int PIL_HALF = 1 << (PIL_BITS - 1);

typedef u32x4 __attribute__((aligned(1))) pil_u32x4u;
typedef u32x2 __attribute__((aligned(1))) pil_u32x2u;

struct PilParams {
  const uint8_t* src;                        // (T, H, W, 3) bytes, or T I420 frames
  const uint8_t* src_end;
  int T, H, W, oh, ow;
  int kx, ky;                                // tap capacities of the width / height tables
  int band, nbands;                          // output rows per workgroup, workgroups per frame
  int cap_rows;                              // rows of the width-filtered buffer
  int rch;                                   // source rows per staged chunk
  int pitch;                                 // bytes of one staged row
  const int32_t *xs, *xn, *xk, *ys, *yn, *yk;
  const float* lut;
  float* out;
  long frame_stride, chan_stride;            // elements
  YuvCoef k;
};

// bytes of one staged source row: the row itself (uint8 frames: rows stay back to back, as in memory), or whole 16-pixel groups (I420)
static inline int pil_pitch(int W, bool yuv) { return yuv ? ceil_div(W, 16) * 48 : W * 3; }

__device__ __forceinline__ int pil_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// A converted channel (clamp8(sum >> 16), yuv.hpp) as a value the compiler cannot look into — no instruction.  Packing pairs of them
// into bytes otherwise compiles to v_ashr_pk_u8_i32 (shift + saturate + pack, new on gfx950), and with it this launch's pixels
// differed from kvq_yuv420_to_rgb's on the device (brighter, as if negative sums saturated high) while the same source gives equal
// bytes on the host; kvq_yuv420_to_rgb, whose code has no such instruction, is the reference.
__device__ __forceinline__ uint32_t pil_opaque(int v) {
  asm volatile("" : "+v"(v));
  return (uint32_t)v;
}

template <bool YUV>
__global__ __launch_bounds__(PIL_THREADS) void resize_pil_kernel(PilParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x;
  const int ow = p.ow, W = p.W, H = p.H, kx = p.kx, ky = p.ky, pitch = p.pitch;
  uint8_t* stage = lds;
  float* lut = reinterpret_cast<float*>(lds + PIL_STAGE);      // [256]
  int32_t* xk = reinterpret_cast<int32_t*>(lut + 256);         // [ow][kx]
  int32_t* xs = xk + (size_t)ow * kx;                          // [ow]
  int32_t* xn = xs + ow;                                       // [ow]
  int32_t* yk = xn + ow;                                       // [band][ky]
  int32_t* ys = yk + (size_t)p.band * ky;                      // [band]
  int32_t* yn = ys + p.band;                                   // [band]
  uint8_t* hbuf = reinterpret_cast<uint8_t*>(yn + p.band);     // [cap_rows][3][ow]

  const int bi = blockIdx.x % p.nbands, t = blockIdx.x / p.nbands;
  const int oy0 = bi * p.band;
  const int nb = min(p.band, p.oh - oy0);
  lut[tid] = p.lut[tid];                                       // PIL_THREADS == 256
  for (int i = tid; i < ow; i += PIL_THREADS) {
    const int s = min(max(p.xs[i], 0), W - 1);
    xs[i] = s;
    xn[i] = min(max(p.xn[i], 0), min(kx, W - s));
  }
  for (int i = tid; i < ow * kx; i += PIL_THREADS) xk[i] = p.xk[i];
  for (int i = tid; i < nb; i += PIL_THREADS) {
    const int s = min(max(p.ys[oy0 + i], 0), H - 1);
    ys[i] = s;
    yn[i] = min(max(p.yn[oy0 + i], 0), min(ky, H - s));
  }
  for (int i = tid; i < nb * ky; i += PIL_THREADS) yk[i] = p.yk[(size_t)oy0 * ky + i];
  __syncthreads();
  const int ry0 = ys[0];                                        // <= H - 1
  const int ry1 = min(max(ys[nb - 1] + yn[nb - 1], ry0 + 1), min(ry0 + p.cap_rows, H));   // the host sized cap_rows for the band
  const int nrows = ry1 - ry0;                                  // >= 1
  const int nchunks = (nrows + p.rch - 1) / p.rch;

  // ---- uint8 frames: chunk k = source rows [ry0 + k rch, min(+rch, ry1)), one contiguous byte run staged from its 16-B aligned start
  const uintptr_t lo = reinterpret_cast<uintptr_t>(p.src), hi = reinterpret_cast<uintptr_t>(p.src_end);
  const uintptr_t frame_b = lo + (uintptr_t)t * H * W * 3;
  u32x4 reg[PIL_NV];
  auto fetch = [&](int k) {
    const int r0 = ry0 + k * p.rch, r1 = min(r0 + p.rch, ry1);
    const uintptr_t gs = frame_b + (uintptr_t)r0 * pitch, ge = frame_b + (uintptr_t)r1 * pitch;
    const uintptr_t A = gs & ~(uintptr_t)15;
#pragma unroll
    for (int v = 0; v < PIL_NV; ++v) {
      const uintptr_t a = A + (uintptr_t)(v * PIL_THREADS + tid) * 16;
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
  // ---- I420 frames: a work item converts 16 pixels of one row where it loads them; every access stays inside the frame
  const I420Geom geo = i420_geom(H, W);
  const uint8_t* f420 = p.src + (size_t)t * geo.frame;
  auto convert = [&](int r0, int rows) {
    const int groups = (W + 15) >> 4;
    for (int i = tid; i < rows * groups; i += PIL_THREADS) {
      const int row = i / groups, g = i - row * groups;
      const int x0 = 16 * g, y = r0 + row;
      const int nx = min(16, W - x0), nc = (nx + 1) >> 1;
      const uint8_t* yrow = f420 + (size_t)y * W + x0;
      const uint8_t* urow = f420 + geo.ysize + (size_t)(y >> 1) * geo.cw + (x0 >> 1);
      const uint8_t* vrow = urow + geo.csize;
      uint32_t yw[4] = {0, 0, 0, 0}, uw[2] = {0, 0}, vw[2] = {0, 0};
      if (nx == 16) {
        const u32x4 a = *reinterpret_cast<const pil_u32x4u*>(yrow);
        const u32x2 b = *reinterpret_cast<const pil_u32x2u*>(urow), c = *reinterpret_cast<const pil_u32x2u*>(vrow);
        yw[0] = a[0]; yw[1] = a[1]; yw[2] = a[2]; yw[3] = a[3];
        uw[0] = b[0]; uw[1] = b[1]; vw[0] = c[0]; vw[1] = c[1];
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (e < nx) yw[e >> 2] |= (uint32_t)yrow[e] << (8 * (e & 3));
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (e < nc) {
            uw[e >> 2] |= (uint32_t)urow[e] << (8 * (e & 3));
            vw[e >> 2] |= (uint32_t)vrow[e] << (8 * (e & 3));
          }
      }
      uint32_t o[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};      // 16 pixels, R G B interleaved
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int s = e >> 1;
        const YuvChroma ch = yuv_chroma(p.k, (int)((uw[s >> 2] >> (8 * (s & 3))) & 255u), (int)((vw[s >> 2] >> (8 * (s & 3))) & 255u));
        const int l = yuv_luma(p.k, (int)((yw[e >> 2] >> (8 * (e & 3))) & 255u));
        o[(3 * e) >> 2] |= pil_opaque(yuv_out(l, ch.r)) << (8 * ((3 * e) & 3));
        o[(3 * e + 1) >> 2] |= pil_opaque(yuv_out(l, ch.g)) << (8 * ((3 * e + 1) & 3));
        o[(3 * e + 2) >> 2] |= pil_opaque(yuv_out(l, ch.b)) << (8 * ((3 * e + 2) & 3));
      }
      u32x4* d = reinterpret_cast<u32x4*>(stage + (size_t)row * pitch + 48 * g);      // pitch = 48 groups: 16-B aligned, inside the row
      d[0] = (u32x4){o[0], o[1], o[2], o[3]};
      d[1] = (u32x4){o[4], o[5], o[6], o[7]};
      d[2] = (u32x4){o[8], o[9], o[10], o[11]};
    }
  };

  if constexpr (!YUV) fetch(0);
  for (int k = 0; k < nchunks; ++k) {
    const int r0 = ry0 + k * p.rch, r1 = min(r0 + p.rch, ry1), rows = r1 - r0;
    int base = 0;                               // byte offset of (r0, 0) in the stage
    __syncthreads();                            // the previous chunk's readers are done with the stage
    if constexpr (YUV) {
      convert(r0, rows);
      __syncthreads();
    } else {
      const uintptr_t gs = frame_b + (uintptr_t)r0 * pitch, ge = frame_b + (uintptr_t)r1 * pitch;
      const uintptr_t A = gs & ~(uintptr_t)15;
#pragma unroll
      for (int v = 0; v < PIL_NV; ++v) {
        const int o = (v * PIL_THREADS + tid) * 16;
        if (A + o < ge) *reinterpret_cast<u32x4*>(stage + o) = reg[v];
      }
      __syncthreads();
      if (k + 1 < nchunks) fetch(k + 1);        // in flight while this chunk is filtered
      base = (int)(gs - A);
    }
    // width pass: a work item = 2 rows x one output column x 3 channels, the column's coefficients read once for the 2 rows
    const int groups = (rows + 1) >> 1;
    for (int i = tid; i < groups * ow; i += PIL_THREADS) {
      const int g = i / ow, ox = i - g * ow;
      const int x0 = xs[ox], n = xn[ox];
      const int32_t* kp = xk + (size_t)ox * kx;
      const int ra = 2 * g, rb = min(2 * g + 1, rows - 1);
      const uint8_t* pa = stage + base + (size_t)ra * pitch + 3 * x0;
      const uint8_t* pb = stage + base + (size_t)rb * pitch + 3 * x0;
      int a0 = 0, a1 = 0, a2 = 0, b0 = 0, b1 = 0, b2 = 0;
      for (int j = 0; j < n; ++j) {
        const int kj = kp[j];
        a0 += kj * pa[3 * j]; a1 += kj * pa[3 * j + 1]; a2 += kj * pa[3 * j + 2];
        b0 += kj * pb[3 * j]; b1 += kj * pb[3 * j + 1]; b2 += kj * pb[3 * j + 2];
      }
      uint8_t* ha = hbuf + (size_t)(r0 - ry0 + ra) * 3 * ow + ox;
      ha[0] = (uint8_t)pil_clip8((a0 + PIL_HALF) >> PIL_BITS);
      ha[ow] = (uint8_t)pil_clip8((a1 + PIL_HALF) >> PIL_BITS);
      ha[2 * ow] = (uint8_t)pil_clip8((a2 + PIL_HALF) >> PIL_BITS);
      if (2 * g + 1 < rows) {
        uint8_t* hb = ha + 3 * ow;
        hb[0] = (uint8_t)pil_clip8((b0 + PIL_HALF) >> PIL_BITS);
        hb[ow] = (uint8_t)pil_clip8((b1 + PIL_HALF) >> PIL_BITS);
        hb[2 * ow] = (uint8_t)pil_clip8((b2 + PIL_HALF) >> PIL_BITS);
      }
    }
  }
  __syncthreads();
  // height pass + table; ox fastest -> coalesced rows of the output
  float* dst = p.out + (size_t)t * p.frame_stride + (size_t)oy0 * ow;
  const int per = nb * ow;
  for (int i = tid; i < 3 * per; i += PIL_THREADS) {
    const int c = i / per, r = i - c * per;
    const int oyl = r / ow, ox = r - oyl * ow;
    const int32_t* kp = yk + (size_t)oyl * ky;
    const int y0 = ys[oyl] - ry0, n = yn[oyl];
    int v = 0;
    for (int j = 0; j < n; ++j) v += kp[j] * hbuf[((size_t)min(max(y0 + j, 0), nrows - 1) * 3 + c) * ow + ox];
    dst[(size_t)c * p.chan_stride + r] = lut[pil_clip8((v + PIL_HALF) >> PIL_BITS)];
  }
}

// the launch geometry of a shape, or what rules it out: decided on the host before anything is enqueued
struct PilPlan {
  int kx, ky, band, nbands, cap_rows, rch, pitch;
  long lds;
  const char* why;                           // NULL: supported
};

static PilPlan pil_plan(int format, int T, int H, int W, int oh, int ow) {
  PilPlan q{};
  const bool yuv = format != KVQ_SRC_U8;
  q.pitch = pil_pitch(W, yuv);
  if ((long)q.pitch + (yuv ? 0 : 15) > PIL_STAGE) {
    q.why = "a source row exceeds the 16 KiB stage";
    return q;
  }
  q.kx = pil_kmax(W, ow);
  q.ky = pil_kmax(H, oh);
  // rows a band of b output rows reads: from the first row's window start to the last row's window end (both grow with the index)
  auto rows_for = [&](int b) {
    int m = 1;
    for (int y = 0; y < oh; y += b) {
      const PilWindow w0 = pil_window(y, H, oh), w1 = pil_window(std::min(y + b, oh) - 1, H, oh);
      m = std::max(m, w1.start + w1.size - w0.start);
    }
    return std::min(m, H);
  };
  const int want_bands = (PIL_MIN_BLOCKS + T - 1) / T;
  int band = std::max(1, (oh + want_bands - 1) / want_bands);
  while (band > 1 && (long)rows_for(band) * 3 * ow > PIL_HBUF) --band;
  q.band = band;
  q.nbands = (oh + band - 1) / band;
  q.cap_rows = rows_for(band);
  int rch = std::max(1, std::min(q.cap_rows, (PIL_STAGE - (yuv ? 0 : 15)) / q.pitch));
  q.rch = rch >= 2 ? rch & ~1 : rch;
  q.lds = (long)PIL_STAGE + 256 * 4 + ((long)ow * q.kx + 2L * ow + (long)band * q.ky + 2L * band) * 4 + (long)q.cap_rows * 3 * ow;
  if (q.lds > PIL_LDS_MAX) q.why = "the tables and one band of width-filtered rows exceed the LDS";
  return q;
}

static bool pil_format_ok(int format) { return format == KVQ_SRC_U8 || yuv_format_ok(format); }
static bool pil_shape_ok(int T, int H, int W, int oh, int ow) {
  return T > 0 && T < 65536 && i420_size_ok(H, W) && H <= KVQ_RESIZE_PIL_MAX_AXIS && W <= KVQ_RESIZE_PIL_MAX_AXIS && oh > 0 && ow > 0 &&
         oh <= KVQ_RESIZE_PIL_MAX_AXIS && ow <= KVQ_RESIZE_PIL_MAX_AXIS && (long)oh * ow < (1L << 29);
}

}  // namespace kvq

extern "C" int kvq_resize_pil_supported(int src_format, int T, int H, int W, int oh, int ow) {
  using namespace kvq;
  if (!pil_format_ok(src_format) || !pil_shape_ok(T, H, W, oh, ow)) return 0;
  return pil_plan(src_format, T, H, W, oh, ow).why == nullptr;
}

extern "C" int kvq_resize_pil(const void* frames, int src_format, int T, int H, int W, int oh, int ow, const int32_t* xstart,
                              const int32_t* xsize, const int32_t* xcoef, const int32_t* ystart, const int32_t* ysize,
                              const int32_t* ycoef, const float* lut256, float* out, int64_t frame_stride, int64_t chan_stride,
                              void* stream) {
  using namespace kvq;
  KVQ_REQUIRE(pil_format_ok(src_format), KVQ_ERR_UNSUPPORTED,
              "kvq_resize_pil: frame type %d (uint8 (T,H,W,3) frames = KVQ_SRC_U8, or a KVQ_SRC_I420_* value)", src_format);
  KVQ_REQUIRE(frames && xstart && xsize && xcoef && ystart && ysize && ycoef && lut256 && out, KVQ_ERR_NULL, "kvq_resize_pil: NULL pointer");
  KVQ_REQUIRE(pil_shape_ok(T, H, W, oh, ow), KVQ_ERR_SHAPE, "kvq_resize_pil: %d frames of %dx%d -> %dx%d", T, H, W, oh, ow);
  auto al4 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3) == 0; };
  KVQ_REQUIRE(al4(xstart) && al4(xsize) && al4(xcoef) && al4(ystart) && al4(ysize) && al4(ycoef) && al4(lut256) && al4(out), KVQ_ERR_SHAPE,
              "kvq_resize_pil: the tables, the look-up table and the output must be 4-byte aligned");
  // one writer per element: the planes of a frame inside the frame stride, or the frames of a plane inside the channel stride
  const long plane = (long)oh * ow;
  KVQ_REQUIRE(frame_stride >= plane && chan_stride >= plane &&
                  (frame_stride <= chan_stride ? (T - 1) * (long)frame_stride + plane <= chan_stride || T == 1
                                               : 2 * (long)chan_stride + plane <= frame_stride),
              KVQ_ERR_SHAPE, "kvq_resize_pil: output strides (frame %ld, channel %ld) overlap for %d frames of 3 x %dx%d", (long)frame_stride,
              (long)chan_stride, T, oh, ow);
  const PilPlan q = pil_plan(src_format, T, H, W, oh, ow);
  KVQ_REQUIRE(q.why == nullptr, KVQ_ERR_UNSUPPORTED, "kvq_resize_pil: %dx%d -> %dx%d: %s (%ld B of %d)", H, W, oh, ow, q.why, q.lds, PIL_LDS_MAX);
  const bool yuv = src_format != KVQ_SRC_U8;
  PilParams p{};
  p.src = reinterpret_cast<const uint8_t*>(frames);
  p.src_end = p.src + (yuv ? (size_t)T * i420_geom(H, W).frame : (size_t)T * H * W * 3);
  p.T = T; p.H = H; p.W = W; p.oh = oh; p.ow = ow;
  p.kx = q.kx; p.ky = q.ky; p.band = q.band; p.nbands = q.nbands; p.cap_rows = q.cap_rows; p.rch = q.rch; p.pitch = q.pitch;
  p.xs = xstart; p.xn = xsize; p.xk = xcoef; p.ys = ystart; p.yn = ysize; p.yk = ycoef;
  p.lut = lut256; p.out = out; p.frame_stride = (long)frame_stride; p.chan_stride = (long)chan_stride;
  if (yuv) p.k = yuv420_coeffs(src_format);
  const long blocks = (long)T * q.nbands;
  KVQ_REQUIRE(blocks < (1L << 31), KVQ_ERR_SHAPE, "kvq_resize_pil: grid too large");
  return launch("resize_pil_kernel", yuv ? resize_pil_kernel<true> : resize_pil_kernel<false>, dim3((unsigned)blocks), dim3(PIL_THREADS),
                (size_t)q.lds, stream, p);
}
