// The ONE definition of the baseline-JPEG entropy decode of a SEGMENT — one restart interval, or the whole scan of a frame without
// DRI — that kvq_jpeg_entropy (jpeg_entropy.hip, one lane per segment) and its host twin kvq_jpeg_entropy_host (jpeg.cpp) share: the
// bit reader, the symbol decode and the block decode.  No HIP dependency: jpeg.cpp includes it under the host compiler alone
// (tools/jpeg_entropy_hostcheck.cpp runs it under the address and undefined-behaviour sanitizers on hostile input).
//
// A segment is the byte range [begin, end) of a buffer: it starts byte-aligned with the DC predictors at 0 and `end` is the first
// 0xFF of the marker that closes it (kvq_jpeg_index finds both).  It holds n_mcu MCUs of six blocks (Y Y Y Y Cb Cr) from MCU
// first_mcu of the frame on.  The non-zero quantised coefficients go as int16 into the frame's dense hand-over (jpeg_idct.hpp:
// per-plane block raster, natural order, the DC kept to 16 bits) — the caller has zero-filled it.
//
// What bounds every access, whatever the bytes, the tables and the counts hold:
//   loops    n_mcu x 6 blocks of at most 64 coefficient steps each (one loop of at most n_mcu x 6 x 64 steps: jpeg_huff_segment);
//            7 steps per long code (lengths 10..16; the 9-bit lookahead resolves the shorter ones); at most 8 byte steps per refill
//   reads    the stream at buf[pos] with begin <= pos < end only: the 4-byte refill is taken when pos + 4 <= end, otherwise (and
//            whenever the word holds an 0xFF) the reader goes by bytes; look[] at a 9-bit index; vals[] at an index masked to 8 bits;
//            the range arrays at length - 10 in 0..6
//   writes   coef[blk * 64 + zigzag[k]] with k in 0..63 and blk computed from an MCU number that the caller has checked to be below
//            the frame's g.nc, so below g.blocks: inside kvq_jpeg_coef_bytes(H, W)
//   bits     none is taken from beyond `end`: an 0xFF that is not followed by 0x00 inside the segment ends the supply
// Status: 0, or JPEG_ST_* | (the frame's MCU number at which the decode stopped << 8).  The causes are the ones kvq_jpeg_coeffs
// knows, and the end is STRICT: after the last MCU fewer than 8 bits may remain before `end` (kvq_jpeg_coeffs drops up to a
// refill's worth of whole bytes there).  Stricter than the host decoder in that one place, laxer nowhere.
//
// The table layout, the symbol decode (jpeg_huff_symbol), the sign extension and the zigzag order are also kvq_jpeg_coeffs's.  Its
// bit reader and block loop (Bits, decode_block in jpeg.cpp) stay a second pair on purpose: that byte-wise reader accepts a few stray
// bytes in front of a marker where this one reports JPEG_ST_TRAILING, and the frame reader relies on "device strict, host final".
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/kvq_hip.h"
#include "jpeg_idct.hpp"
#include "jpeg_tables.hpp"

namespace kvq {

enum {
  JPEG_ST_OK = 0,
  JPEG_ST_TRUNCATED = 1,      // bits exhausted
  JPEG_ST_BAD_CODE = 2,       // a code that is in no table
  JPEG_ST_BAD_DC = 3,         // a DC category above 15
  JPEG_ST_BAD_RUN = 4,        // a zero run past coefficient 63
  JPEG_ST_TRAILING = 5,       // 8 or more bits left before `end` after the last MCU
  JPEG_ST_BAD_SEGMENT = 6,    // the descriptors do not fit the buffers or the frame (nothing was read through them)
};
constexpr int32_t JPEG_ST_UNWRITTEN = -1;      // what the entries fill status_out with before the decode

KVQ_JPEG_HD int32_t jpeg_status(int cause, int mcu) { return (int32_t)((uint32_t)cause | ((uint32_t)mcu << 8)); }

KVQ_JPEG_HD int jpeg_zigzag(int k) { return ZIGZAG[k & 63]; }

// the segment's bits, most significant first; `end` (or an 0xFF that no 0x00 follows) ends the supply, asking for more is an error
struct JpegBits {
  const uint8_t* buf;
  uint32_t pos, end;
  uint64_t acc;
  int nbits;              // valid low bits of acc, 0..64
  static constexpr bool own_tables = false;     // the tables come from the caller's memory: what is read from them is masked

  KVQ_JPEG_HD_MEMBER void fill() {
    if (nbits > 32) return;
    if (end - pos >= 4) {                                               // pos <= end always
      uint32_t w;
      memcpy(&w, buf + pos, 4);                                         // one unaligned load
      w = __builtin_bswap32(w);
      const uint32_t x = ~w;                                            // a zero byte of x is an 0xFF of w
      if (!((x - 0x01010101u) & ~x & 0x80808080u)) {
        acc = (acc << 32) | w;
        nbits += 32;
        pos += 4;
        return;
      }
    }
    for (int i = 0; i < 8 && nbits <= 56 && pos < end; ++i) {
      const uint8_t v = buf[pos];
      if (v == 0xFF) {
        if (end - pos < 2 || buf[pos + 1] != 0x00) return;              // no stuffed byte: stay in front of it
        pos += 2;
      } else {
        pos += 1;
      }
      acc = (acc << 8) | v;
      nbits += 8;
    }
  }
  // the next 16 bits, zero-padded where the supply has ended
  KVQ_JPEG_HD_MEMBER uint32_t peek16() {
    if (nbits < 16) fill();
    return nbits >= 16 ? (uint32_t)(acc >> (nbits - 16)) & 0xFFFFu : (uint32_t)(acc << (16 - nbits)) & 0xFFFFu;
  }
  // k in 0..16
  KVQ_JPEG_HD_MEMBER bool take(int k, uint32_t& out) {
    if (nbits < k) fill();
    if (nbits < k) return false;
    out = k ? (uint32_t)(acc >> (nbits - k)) & ((1u << k) - 1u) : 0u;
    nbits -= k;
    return true;
  }
};

// a symbol 0..255, or -JPEG_ST_TRUNCATED / -JPEG_ST_BAD_CODE.  Bits: peek16() as above, nbits, from which the code's length is taken,
// and own_tables — false: the table may hold anything, so a length from look[] is masked to 0..15 and the index into vals[] to 8 bits
template <class Bits>
KVQ_JPEG_HD int jpeg_huff_symbol(Bits& b, const KvqJpegHuffTable* h) {
  const uint32_t w = b.peek16();
  const uint32_t e = h->look[w >> 7];
  constexpr int len_mask = Bits::own_tables ? 255 : 15, val_mask = Bits::own_tables ? -1 : 255;
  int len = (int)(e >> 8) & len_mask, sym = (int)(e & 255);
  if (!len) {
    len = 17;
    for (int l = 10; l <= 16; ++l) {
      const int32_t code = (int32_t)(w >> (16 - l));
      if (code <= h->maxcode[l - 10] && code >= h->mincode[l - 10]) {
        sym = h->vals[(h->valptr[l - 10] + code - h->mincode[l - 10]) & val_mask];
        len = l;
        break;
      }
    }
    if (len > 16) return b.nbits < 16 ? -JPEG_ST_TRUNCATED : -JPEG_ST_BAD_CODE;
  }
  if (len > b.nbits) return -JPEG_ST_TRUNCATED;
  b.nbits -= len;
  return sym;
}

KVQ_JPEG_HD int32_t jpeg_extend(uint32_t v, int s) { return v < (1u << (s - 1)) ? (int32_t)v - (1 << s) + 1 : (int32_t)v; }

// The segment buf[begin, end) of the frame whose table set is `t` (jpeg_tables_ok: its dc / ac indices are below ntab <= 6): MCUs
// first_mcu .. first_mcu + n_mcu - 1, which the caller has checked to lie inside g.nc, into the frame's coefficients `coef`.
// ONE loop, one symbol per step — the DC symbol of a block (k = 0) or an AC symbol (k = 1..63: the next zigzag position) — so that
// the lanes of a wave, each in its own segment, share the loop body whatever block and coefficient each has reached: which table,
// which predictor and which block a step uses is data, not control flow.  Every step moves k forward by at least 1 or closes the
// block, so a block takes at most 64 steps and the segment at most n_mcu x 6 x 64, which bounds the loop.
KVQ_JPEG_HD int32_t jpeg_huff_segment(const uint8_t* buf, uint32_t begin, uint32_t end, const KvqJpegTables* t, int first_mcu, int n_mcu,
                                      const JpegGeom& g, int16_t* coef) {
  JpegBits b;
  b.buf = buf; b.pos = begin; b.end = end; b.acc = 0; b.nbits = 0;
  // the six table indices, four bits each: component c's DC table at 8 c, its AC table at 8 c + 4
  const uint32_t tabs = (uint32_t)t->dc[0] | (uint32_t)t->ac[0] << 4 | (uint32_t)t->dc[1] << 8 | (uint32_t)t->ac[1] << 12 |
                        (uint32_t)t->dc[2] << 16 | (uint32_t)t->ac[2] << 20;
  int32_t pred0 = 0, pred1 = 0, pred2 = 0;
  int y = first_mcu / g.mx, x = first_mcu - y * g.mx;
  int m = 0, j = 0, k = 0;                                            // MCU of the segment, block of the MCU (0..5), coefficient step
  const long steps = (long)n_mcu * 6 * 64;
  for (long step = 0; step < steps && m < n_mcu; ++step) {
    const int c = j < 4 ? 0 : j - 3;
    const bool dc = k == 0;
    const int sym = jpeg_huff_symbol(b, &t->tab[(tabs >> (8 * c + (dc ? 0 : 4))) & 7u]);
    if (sym < 0) return jpeg_status(-sym, first_mcu + m);
    if (dc && sym > 15) return jpeg_status(JPEG_ST_BAD_DC, first_mcu + m);
    const int size = dc ? sym : (sym & 15), run = dc ? 0 : (sym >> 4);
    uint32_t v = 0;
    if (!b.take(size, v)) return jpeg_status(JPEG_ST_TRUNCATED, first_mcu + m);
    int32_t value = size ? jpeg_extend(v, size) : 0;
    bool close = false;
    if (dc) {
      const int32_t p = (int16_t)((c == 0 ? pred0 : c == 1 ? pred1 : pred2) + value);      // kept to 16 bits, as it is stored
      pred0 = c == 0 ? p : pred0; pred1 = c == 1 ? p : pred1; pred2 = c == 2 ? p : pred2;
      value = p;
    } else if (size == 0) {
      if (run != 15) {
        close = true;                                                 // EOB
      } else {
        k += 16;                                                      // ZRL
        if (k > 64) return jpeg_status(JPEG_ST_BAD_RUN, first_mcu + m);
        close = k == 64;
      }
    } else {
      k += run;
      if (k > 63) return jpeg_status(JPEG_ST_BAD_RUN, first_mcu + m);
    }
    if (value) {                                                      // an AC value is never 0 (size >= 1); a DC of 0 is not stored
      coef[(size_t)jpeg_mcu_block(g, (uint32_t)y, (uint32_t)x, (uint32_t)j) * 64 + jpeg_zigzag(k)] = (int16_t)value;
    }
    if (dc || size) close = ++k == 64;
    if (close) {
      k = 0;
      if (++j == 6) {
        j = 0;
        ++m;
        if (++x == g.mx) { x = 0; ++y; }
      }
    }
  }
  if (m < n_mcu) return jpeg_status(JPEG_ST_TRUNCATED, first_mcu + m);            // unreachable: the step bound is never the one that ends the loop
  if (b.pos != b.end || b.nbits >= 8) return jpeg_status(JPEG_ST_TRAILING, first_mcu + n_mcu - 1);
  return JPEG_ST_OK;
}

// The descriptor checks both entries make before a segment is decoded.  frame = {byte offset of the image, first entry in segs, nseg,
// restart interval, table set}; s = the segment's number inside the frame (< nseg).  true: first_mcu / n_mcu are set and everything
// the decode touches lies inside the buffers; false: JPEG_ST_BAD_SEGMENT.
KVQ_JPEG_HD uint32_t jpeg_expected_segments(uint32_t ri, const JpegGeom& g) { return ri ? ((uint32_t)g.nc + ri - 1) / ri : 1u; }

KVQ_JPEG_HD bool jpeg_frame_ok(const uint32_t* frame, uint64_t nbytes, uint32_t nsegs, uint32_t ntables, const JpegGeom& g) {
  return frame[0] <= nbytes && frame[1] <= nsegs && frame[2] <= nsegs - frame[1] && frame[4] < ntables &&
         frame[2] == jpeg_expected_segments(frame[3], g);
}
KVQ_JPEG_HD bool jpeg_tables_ok(const KvqJpegTables* t) {
  const int n = t->ntab;
  return n >= 1 && n <= 6 && t->dc[0] < n && t->dc[1] < n && t->dc[2] < n && t->ac[0] < n && t->ac[1] < n && t->ac[2] < n;
}
KVQ_JPEG_HD bool jpeg_segment_ok(const uint32_t* frame, const uint32_t* seg, uint64_t nbytes) {
  return seg[0] <= seg[1] && (uint64_t)seg[1] <= nbytes - frame[0];
}

// Segment s of the frame f, for both entries: the descriptor checks, then the decode into `coef`, the frame's coefficients.  The
// caller has checked s < f[2] and f[1] <= nsegs, f[2] <= nsegs - f[1] (the frame's entries lie in segs); `set` is the frame's table
// set, tables + f[4] or a copy of it, and is read only where jpeg_frame_ok holds.
KVQ_JPEG_HD int32_t jpeg_entropy_segment(const uint32_t* f, uint32_t s, const KvqJpegTables* set, const uint8_t* bytes, uint64_t nbytes,
                                         const uint32_t* segs, uint32_t nsegs, uint32_t ntables, const JpegGeom& g, int16_t* coef) {
  const uint32_t sg[2] = {segs[2 * ((size_t)f[1] + s)], segs[2 * ((size_t)f[1] + s) + 1]};
  if (!(jpeg_frame_ok(f, nbytes, nsegs, ntables, g) && jpeg_tables_ok(set) && jpeg_segment_ok(f, sg, nbytes))) return jpeg_status(JPEG_ST_BAD_SEGMENT, 0);
  const uint32_t first = f[3] ? s * f[3] : 0u;                          // < g.nc: s < nseg = ceil(nc / ri)
  const uint32_t left = (uint32_t)g.nc - first;
  return jpeg_huff_segment(bytes + f[0], sg[0], sg[1], set, (int)first, (int)(f[3] && f[3] < left ? f[3] : left), g, coef);
}

}  // namespace kvq
