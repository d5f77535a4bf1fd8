// The ONE definition of the baseline Huffman CODING of one 8 x 8 block of the coefficient hand-over (jpeg_idct.hpp: JpegGeom), shared
// by kvq_jpeg_encode_scans (jpeg_enc_entropy.hip, one lane per block), its host twin kvq_jpeg_encode_scans_host and the whole-image
// coder kvq_jpeg_encode (both jpeg_enc.cpp):
// the scan order, the DC predictor, the code length, the emission into a bit sink and the range verdict — and the phases that turn
// T frames of coefficients into their byte-stuffed scans, one function per phase and per block, which the launch calls from a lane
// and the twin from a loop.  No HIP header: the one device-only construct, the integer atomic OR (a compiler builtin), sits
// behind __HIP_DEVICE_COMPILE__.  The bytes are those of kvq_jpeg_encode between its SOS header and its EOI; the tests pin them to a numpy
// restatement (tests/jpeg_enc_ref.py) and to libjpeg's (tests/golden/mjpeg_enc.npz).
//
// Scan order of a frame: MCU raster, within an MCU Y00 Y01 Y10 Y11 Cb Cr: scan index s = 6 mcu + k.  Restart interval i holds the
// MCUs [i ri, (i + 1) ri); without DRI (ri = 0) the frame is one interval.  A block's DC predictor is the DC of the previous block
// of its component in scan order, 0 at the first MCU of an interval.  A block takes at most 11 + 11 bits of DC and 63 x (16 + 10)
// of AC = 1660 bits.
//
// Phases.  A frame's UNSTUFFED stream — its intervals' codes, each interval padded with 1 bits to a whole byte, back to
// back, before byte stuffing and without markers — is never stored: a block OWNS the bytes of it whose first bit lies in the block and
// regenerates them from the coefficients whenever they are needed, so no two lanes ever write one address and there is no atomic
// on the data path.
//   count    block -> its code length (cnt), range verdict ORed into the frame's `bad`
//   scan     exclusive prefix of the lengths in scan order, rounded up to a byte in front of every interval -> pos, per frame its bytes
//   ffcount  block -> the number of 0xFF among the bytes it owns
//   scan     exclusive prefix of those counts per frame (cnt in place), per frame their sum
//   frames   {offset, length, status} of every frame
//   write    block -> its owned bytes at offset + (byte in the frame) + FFs before + 2 i, a 00 behind every FF; the first block of
//            interval i >= 1 puts RSTn, n = (i - 1) & 7, in front.  Every store is compared against the capacity first.
#pragma once
#include <stdint.h>
#include <string.h>

#include "jpeg_idct.hpp"
#include "jpeg_tables.hpp"

#if defined(__clang__)
#define KVQ_JPEG_UNROLL _Pragma("unroll")
#else
#define KVQ_JPEG_UNROLL
#endif

namespace kvq {

constexpr int JPEG_ENC_BLOCK_BITS = 1660;     // the longest block
constexpr int JPEG_ENC_BLOCK_BYTES = 208;      // its bytes, and room for the padding of an interval per six blocks
enum { JPEG_SCAN_OK = 0, JPEG_SCAN_RANGE = 1, JPEG_SCAN_CAPACITY = 2 };

// (length << 16) | code of every symbol of the four Annex K tables: DC lum, DC chroma, AC lum, AC chroma
struct JpegEncTables {
  uint32_t t[4][256];
};
constexpr void jpeg_enc_fill(uint32_t* t, const uint8_t* bits, const uint8_t* vals) {
  uint32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l - 1]; ++i) t[vals[k++]] = ((uint32_t)l << 16) | code++;
    code <<= 1;
  }
}
constexpr JpegEncTables jpeg_enc_tables() {
  JpegEncTables e{};
  jpeg_enc_fill(e.t[0], STD_DC_LUM_BITS, STD_DC_VALS);
  jpeg_enc_fill(e.t[1], STD_DC_CHR_BITS, STD_DC_VALS);
  jpeg_enc_fill(e.t[2], STD_AC_LUM_BITS, STD_AC_LUM_VALS);
  jpeg_enc_fill(e.t[3], STD_AC_CHR_BITS, STD_AC_CHR_VALS);
  return e;
}

// ---------------------------------------------------------------------------------------------------------------- scan order
// the block of scan index s (< g.blocks) in the hand-over
KVQ_JPEG_HD uint32_t jpeg_enc_block_index(const JpegGeom& g, uint32_t s) {
  const uint32_t mcu = s / 6u, y = mcu / (uint32_t)g.mx;
  return jpeg_mcu_block(g, y, mcu - y * (uint32_t)g.mx, s - 6u * mcu);
}
// true: MCU `mcu` opens a restart interval (the first MCU of the frame included)
KVQ_JPEG_HD bool jpeg_enc_interval_start(uint32_t mcu, uint32_t ri) { return mcu == 0u || (ri && mcu % ri == 0u); }
// the scan index of the block whose DC predicts block s, -1: none (the predictor is 0)
KVQ_JPEG_HD int64_t jpeg_enc_pred_scan(uint32_t s, uint32_t ri) {
  const uint32_t mcu = s / 6u, k = s - 6u * mcu;
  if (k >= 1u && k <= 3u) return (int64_t)s - 1;
  if (jpeg_enc_interval_start(mcu, ri)) return -1;
  return k == 0u ? (int64_t)s - 3 : (int64_t)s - 6;
}
KVQ_JPEG_HD uint32_t jpeg_enc_intervals(const JpegGeom& g, uint32_t ri) { return ri ? ((uint32_t)g.nc + ri - 1u) / ri : 1u; }

// ------------------------------------------------------------------------------------------------------------ one block's codes
KVQ_JPEG_HD int jpeg_enc_category(int32_t a) { return a ? 32 - __builtin_clz((uint32_t)a) : 0; }      // a >= 0: bits of its magnitude

// the 64 coefficients of a block, natural order, from 16-byte aligned memory into a local array (registers on the device: every
// index below is a constant once the loops are unrolled)
struct alignas(16) JpegEncQuad { uint32_t w[4]; };
KVQ_JPEG_HD void jpeg_enc_load(const int16_t* src, int16_t v[64]) {
  const JpegEncQuad* q = reinterpret_cast<const JpegEncQuad*>(src);
KVQ_JPEG_UNROLL
  for (int i = 0; i < 8; ++i) {
    const JpegEncQuad x = q[i];
KVQ_JPEG_UNROLL
    for (int j = 0; j < 4; ++j) {
      v[8 * i + 2 * j] = (int16_t)(x.w[j] & 0xFFFFu);
      v[8 * i + 2 * j + 1] = (int16_t)(x.w[j] >> 16);
    }
  }
}

// The codes of one block, most significant bit first, into sink.put(code, length) (length 0..16, code below 2^length).  blk: natural
// order; pred: the predictor's DC; tab = JpegEncTables::t.  false: a DC difference of category > 11 or an AC of category > 10 —
// baseline has no code for it; what the sink received is then of no use (the categories are clamped so that it stays in its bounds).
template <class Sink>
KVQ_JPEG_HD bool jpeg_enc_block(const int16_t* blk, int32_t pred, bool chroma, const uint32_t* tab, Sink& sink) {
  const uint32_t* dct = tab + (chroma ? 256 : 0);
  const uint32_t* act = tab + (chroma ? 768 : 512);
  bool ok = true;
  const int32_t diff = (int32_t)blk[0] - pred;
  int s = jpeg_enc_category(diff < 0 ? -diff : diff);
  if (s > 11) { ok = false; s = 11; }
  sink.put(dct[s] & 0xFFFFu, (int)(dct[s] >> 16));
  if (s) sink.put((uint32_t)(diff < 0 ? diff + (1 << s) - 1 : diff) & ((1u << s) - 1u), s);
  int run = 0;
KVQ_JPEG_UNROLL
  for (int i = 1; i < 64; ++i) {
    const int32_t v = blk[ZIGZAG[i]];
    if (v == 0) { ++run; continue; }
    for (; run > 15; run -= 16) sink.put(act[0xF0] & 0xFFFFu, (int)(act[0xF0] >> 16));
    s = jpeg_enc_category(v < 0 ? -v : v);
    if (s > 10) { ok = false; s = 10; }
    const uint32_t e = act[(run << 4) | s];
    sink.put(e & 0xFFFFu, (int)(e >> 16));
    sink.put((uint32_t)(v < 0 ? v + (1 << s) - 1 : v) & ((1u << s) - 1u), s);
    run = 0;
    if (sink.full()) return ok;                                  // a sink that wanted only the block's first bits
  }
  if (run) sink.put(act[0] & 0xFFFFu, (int)(act[0] >> 16));      // EOB: zeros up to coefficient 63
  return ok;
}

struct JpegBitCount {
  uint32_t n = 0;
  KVQ_JPEG_HD_MEMBER void put(uint32_t, int len) { n += (uint32_t)len; }
  KVQ_JPEG_HD_MEMBER bool full() const { return false; }
};

// The bits it is given, cut into the bytes of a stream in which they start `skip` bits (0..7) in front of a byte boundary: the first
// `skip` bits belong to a byte that started earlier and are dropped, every byte completed after them goes to f(byte).  After
// close_after_byte() the sink takes bits only until the byte under way is complete (it is `full()` then, and drops the rest).
template <class F>
struct JpegByteSink {
  F f;
  uint32_t acc = 0;      // the low n bits are pending
  int n = 0, skip = 0;
  bool tail = false, done = false;
  KVQ_JPEG_HD_MEMBER bool full() const { return done; }
  KVQ_JPEG_HD_MEMBER void close_after_byte() { tail = true; done = n == 0; }
  KVQ_JPEG_HD_MEMBER void put(uint32_t code, int len) {      // len 0..16
    if (done) return;
    if (skip) {
      const int drop = skip < len ? skip : len;
      skip -= drop;
      len -= drop;
      code &= (1u << len) - 1u;
    }
    acc = (acc << len) | code;
    n += len;
    while (n >= 8) {
      n -= 8;
      f((uint8_t)(acc >> n));
      if (tail) { done = true; n = 0; return; }
    }
    acc &= (1u << n) - 1u;
  }
};

// ------------------------------------------------------------------------------------------------------------------ the phases
// What a call works on.  N = T g.blocks, global scan index gi = t g.blocks + s.  A frame's UNSTUFFED stream: its intervals' codes,
// each interval padded with 1 bits to a whole byte, back to back; it is never stored — a block regenerates the bytes it owns.
struct JpegScansPlan {
  const int16_t* coef;
  uint8_t* out;
  uint32_t* frames_out;      // [T][3] {offset, length, status}
  uint64_t* pos;             // [N] bit position of the block in its frame's unstuffed stream
  uint32_t* cnt;             // [N] code length; then 0xFF bytes owned; then their exclusive prefix in the frame
  uint64_t* fr64;            // [T][2] {the frame's unstuffed bytes, its offset in out}
  uint32_t* fr32;            // [T][2] {bad, the frame's 0xFF bytes}
  uint64_t cap;
  uint32_t T, ri;
  JpegGeom g;
};

KVQ_JPEG_HD size_t jpeg_scans_up16(size_t n) { return (n + 15) & ~(size_t)15; }
// the workspace: 12 bytes per block and 24 per frame
KVQ_JPEG_HD size_t jpeg_scans_workspace(size_t T, const JpegGeom& g) {
  const size_t N = T * (size_t)g.blocks;
  return jpeg_scans_up16(8 * N) + jpeg_scans_up16(4 * N) + jpeg_scans_up16(16 * T) + jpeg_scans_up16(8 * T);
}
// workspace (16-byte aligned, jpeg_scans_workspace bytes) -> the plan's pointers; the entry zero-fills fr32 (8 T bytes)
KVQ_JPEG_HD void jpeg_scans_layout(JpegScansPlan& p, void* workspace) {
  const size_t T = p.T, N = T * (size_t)p.g.blocks;
  uint8_t* w = (uint8_t*)workspace;
  p.pos = (uint64_t*)w; w += jpeg_scans_up16(8 * N);
  p.cnt = (uint32_t*)w; w += jpeg_scans_up16(4 * N);
  p.fr64 = (uint64_t*)w; w += jpeg_scans_up16(16 * T);
  p.fr32 = (uint32_t*)w;
}

KVQ_JPEG_HD uint32_t jpeg_scans_sat32(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

// block s of frame t with its predictor, into sink
template <class Sink>
KVQ_JPEG_HD bool jpeg_scans_code(const JpegScansPlan& p, const uint32_t* tab, uint32_t t, uint32_t s, Sink& sink) {
  const int16_t* frame = p.coef + (size_t)t * p.g.blocks * 64;
  int16_t v[64];
  jpeg_enc_load(frame + (size_t)jpeg_enc_block_index(p.g, s) * 64, v);
  const int64_t ps = jpeg_enc_pred_scan(s, p.ri);
  const int32_t pred = ps < 0 ? 0 : frame[(size_t)jpeg_enc_block_index(p.g, (uint32_t)ps) * 64];
  return jpeg_enc_block(v, pred, s % 6u >= 4u, tab, sink);
}

KVQ_JPEG_HD void jpeg_scans_count(const JpegScansPlan& p, const uint32_t* tab, uint32_t t, uint32_t s) {
  JpegBitCount c;
  const bool ok = jpeg_scans_code(p, tab, t, s, c);
  p.cnt[(size_t)t * p.g.blocks + s] = c.n;
  if (!ok) {
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_fetch_or(p.fr32 + 2 * (size_t)t, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    p.fr32[2 * (size_t)t] |= 1u;
#endif
  }
}

// one element of the position scan and its associative combination.  An element maps a start position x to x + a, or — e set: a
// byte boundary lies inside — to roundup8(x + a) + b.  A block is {length, 0, 0}; one that opens an interval {0, length, 1}.
struct JpegScanSeg {
  uint32_t a, b, e;
};
KVQ_JPEG_HD JpegScanSeg jpeg_scan_combine(const JpegScanSeg& l, const JpegScanSeg& r) {      // l first, then r
  JpegScanSeg o;
  if (!l.e) { o.a = l.a + r.a; o.b = r.b; o.e = r.e; }
  else { o.a = l.a; o.e = 1u; o.b = r.e ? ((l.b + r.a + 7u) & ~7u) + r.b : l.b + r.a; }
  return o;
}
KVQ_JPEG_HD uint64_t jpeg_scan_apply(const JpegScanSeg& s, uint64_t x) { return s.e ? ((x + s.a + 7u) & ~(uint64_t)7) + s.b : x + s.a; }
KVQ_JPEG_HD JpegScanSeg jpeg_scans_seg(const JpegScansPlan& p, bool bad, uint32_t t, uint32_t s) {
  const uint32_t n = bad ? 0u : p.cnt[(size_t)t * p.g.blocks + s];
  const bool opens = s % 6u == 0u && s && jpeg_enc_interval_start(s / 6u, p.ri);
  return opens ? JpegScanSeg{0u, n, 1u} : JpegScanSeg{n, 0u, 0u};
}

// the end of block s of frame t: the next block's position, or the frame's end
KVQ_JPEG_HD uint64_t jpeg_scans_end(const JpegScansPlan& p, uint32_t t, uint32_t s) {
  return s + 1u < (uint32_t)p.g.blocks ? p.pos[(size_t)t * p.g.blocks + s + 1] : 8 * p.fr64[2 * (size_t)t];
}
// true: block s is the last of its restart interval
KVQ_JPEG_HD bool jpeg_scans_closes(const JpegScansPlan& p, uint32_t s) {
  const uint32_t mcu = s / 6u;
  return s % 6u == 5u && (mcu + 1u == (uint32_t)p.g.nc || jpeg_enc_interval_start(mcu + 1u, p.ri));
}

// The bytes block s of frame t OWNS in the frame's unstuffed stream — those whose first bit lies in the block: bytes
// [ceil(pos / 8), ceil(end / 8)) — in order to f(byte).  The block codes itself; the bits in front of its first byte boundary are
// another owner's.  A last byte it starts but does not finish is completed by what follows in the stream: the next blocks of the
// interval (coded until that byte is whole, no further) or the 1 bits that pad the interval.
template <class F>
KVQ_JPEG_HD void jpeg_scans_owned(const JpegScansPlan& p, const uint32_t* tab, uint32_t t, uint32_t s, F f) {
  const uint64_t at = p.pos[(size_t)t * p.g.blocks + s];
  if (((at + 7u) >> 3) == ((jpeg_scans_end(p, t, s) + 7u) >> 3)) return;
  JpegByteSink<F> sink{f};
  sink.skip = (int)((8u - (uint32_t)(at & 7u)) & 7u);
  jpeg_scans_code(p, tab, t, s, sink);
  sink.close_after_byte();
  for (uint32_t u = s; !sink.full();) {
    if (jpeg_scans_closes(p, u)) {
      sink.put(0xFFu >> sink.n, 8 - sink.n);
      break;
    }
    jpeg_scans_code(p, tab, t, ++u, sink);
  }
}

struct JpegCountFF {
  uint32_t* n;
  KVQ_JPEG_HD_MEMBER void operator()(uint8_t b) const { *n += b == 0xFFu; }
};
KVQ_JPEG_HD void jpeg_scans_ffcount(const JpegScansPlan& p, const uint32_t* tab, uint32_t t, uint32_t s) {
  uint32_t n = 0;
  if (!p.fr32[2 * (size_t)t]) jpeg_scans_owned(p, tab, t, s, JpegCountFF{&n});
  p.cnt[(size_t)t * p.g.blocks + s] = n;
}

// {offset, length, status} of every frame, sequential over the frames (T of them: one lane on the device)
KVQ_JPEG_HD void jpeg_scans_frames(const JpegScansPlan& p) {
  const uint32_t nint = jpeg_enc_intervals(p.g, p.ri);
  uint64_t off = 0;
  for (uint32_t t = 0; t < p.T; ++t) {
    const bool bad = p.fr32[2 * (size_t)t] != 0u;
    const uint64_t len = bad ? 0u : p.fr64[2 * (size_t)t] + p.fr32[2 * (size_t)t + 1] + 2u * (uint64_t)(nint - 1u);
    p.fr64[2 * (size_t)t + 1] = off;
    p.frames_out[3 * (size_t)t] = jpeg_scans_sat32(off);
    p.frames_out[3 * (size_t)t + 1] = jpeg_scans_sat32(len);
    p.frames_out[3 * (size_t)t + 2] = bad ? JPEG_SCAN_RANGE : (off + len > p.cap ? JPEG_SCAN_CAPACITY : JPEG_SCAN_OK);
    off += len;
  }
}

// a byte of out, and the 00 behind an FF; nothing is stored at or past cap
struct JpegStuffedOut {
  uint8_t* out;
  uint64_t cap;
  uint64_t* at;
  KVQ_JPEG_HD_MEMBER void byte(uint8_t b) const {
    if (*at < cap) out[*at] = b;
    ++*at;
  }
  KVQ_JPEG_HD_MEMBER void operator()(uint8_t b) const {
    byte(b);
    if (b == 0xFFu) byte(0u);
  }
};
// block s of frame t -> its owned bytes at offset + (byte in the frame) + FFs before + 2 i, RSTn in front when it opens interval i >= 1
KVQ_JPEG_HD void jpeg_scans_write(const JpegScansPlan& p, const uint32_t* tab, uint32_t t, uint32_t s) {
  if (p.frames_out[3 * (size_t)t + 2] != JPEG_SCAN_OK) return;
  const size_t gi = (size_t)t * p.g.blocks + s;
  const uint32_t mcu = s / 6u, i = p.ri ? mcu / p.ri : 0u;
  uint64_t at = p.fr64[2 * (size_t)t + 1] + ((p.pos[gi] + 7u) >> 3) + p.cnt[gi] + 2u * (uint64_t)i;
  const JpegStuffedOut o{p.out, p.cap, &at};
  if (i && s % 6u == 0u && mcu % p.ri == 0u) {
    at -= 2;
    o.byte(0xFFu);
    o.byte((uint8_t)(0xD0u + ((i - 1u) & 7u)));
  }
  jpeg_scans_owned(p, tab, t, s, o);
}

}  // namespace kvq
