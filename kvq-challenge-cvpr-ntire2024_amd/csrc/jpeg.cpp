// Host half of the Motion-JPEG reader (include/kvq_hip.h, "Baseline JPEG"): segment walk (kvq_jpeg_probe), baseline Huffman entropy
// decode into the dense int16 coefficient hand-over (kvq_jpeg_coeffs), the scalar twin of the IDCT launch
// (kvq_jpeg_idct_i420_host), and for the entropy decode on the device the segment index (kvq_jpeg_index: the marker walk and the
// table sets) and the launch's host twin (kvq_jpeg_entropy_host, from csrc/jpeg_huff.hpp).  Plain C++17: no HIP call and no HIP header, so the file also compiles with the host compiler alone
// (tools/jpeg_hostcheck.cpp builds it under the address and undefined-behaviour sanitizers).  Every read of the stream goes through
// a bounds check against n; every coefficient is written at an index computed from the frame's own geometry, inside the
// kvq_jpeg_coef_bytes(H, W) that coef_cap was checked against.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/kvq_hip.h"
#include "jpeg_host.hpp"
#include "jpeg_huff.hpp"
#include "jpeg_idct.hpp"
#include "jpeg_tables.hpp"

namespace {

using namespace kvq;

// one Huffman table of the stream, in the layout both decoders read (include/kvq_hip.h: KvqJpegHuffTable)
struct Huff {
  bool present;
  KvqJpegHuffTable t;
};

// canonical code: the codes of length l are `code` .. code + cnt - 1; those of 1..9 bits go into the lookahead, the ranges of 10..16 are kept
bool huff_build(Huff& h, const uint8_t bits[16], const uint8_t* vals, int nvals) {
  memset(&h, 0, sizeof(h));
  memcpy(h.t.vals, vals, (size_t)nvals);
  int32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int cnt = bits[l - 1];
    if (code + cnt > (1 << l)) return false;          // more codes of this length than the prefix code has room for
    if (l <= 9) {
      for (int i = 0; i < cnt; ++i)
        for (int f = 0; f < (1 << (9 - l)); ++f) h.t.look[((code + i) << (9 - l)) | f] = (uint16_t)((l << 8) | vals[k + i]);
    } else {
      h.t.valptr[l - 10] = k;
      h.t.mincode[l - 10] = code;
      h.t.maxcode[l - 10] = cnt ? code + cnt - 1 : -1;
    }
    code = (code + cnt) << 1;
    k += cnt;
  }
  h.present = true;
  return true;
}

struct Comp {
  int id, h, v, tq, td, ta;
};

struct Parsed {
  KvqJpegInfo info;
  Comp comp[4];
  uint16_t qt[4][64];      // natural order
  bool qt_present[4];
  Huff dc[4], ac[4];
  size_t scan;             // offset of the first entropy-coded byte
  int why_rank;            // the strongest reason the image is outside what the library decodes
  char why[200];
};

void refuse(Parsed& p, int rank, const char* fmt, ...) {
  if (rank <= p.why_rank) return;
  p.why_rank = rank;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(p.why, sizeof(p.why), fmt, ap);
  va_end(ap);
}

// the marker at data[pos]: 0xFF, any number of fill 0xFF, the code; pos moves past it.  false: no marker there / cut short
bool read_marker(const uint8_t* d, size_t n, size_t& pos, int& marker) {
  if (pos >= n || d[pos] != 0xFF) return false;
  while (pos < n && d[pos] == 0xFF) ++pos;
  if (pos >= n) return false;
  marker = d[pos++];
  return marker != 0;
}

// entropy-coded bytes from pos: the offset of the next marker's 0xFF (stuffed FF 00 and RSTn are data), n if there is none
size_t skip_scan(const uint8_t* d, size_t n, size_t pos) {
  while (pos + 1 < n) {
    if (d[pos] != 0xFF) { ++pos; continue; }
    const int b = d[pos + 1];
    if (b == 0x00 || (b >= 0xD0 && b <= 0xD7)) { pos += 2; continue; }
    if (b == 0xFF) { ++pos; continue; }
    return pos;
  }
  return n;
}

int parse(const uint8_t* d, size_t n, Parsed& p, const char* who) {
  memset(&p.info, 0, sizeof(p.info));
  memset(p.qt_present, 0, sizeof(p.qt_present));
  memset(p.comp, 0, sizeof(p.comp));
  for (int i = 0; i < 4; ++i) p.dc[i].present = p.ac[i].present = false;
  p.scan = 0; p.why_rank = 0; p.why[0] = 0;
  JPEG_REQUIRE(n >= 4 && d[0] == 0xFF && d[1] == 0xD8, KVQ_ERR_SHAPE, "%s: not a JPEG image (no SOI marker at its start)", who);
  size_t pos = 2;
  bool have_sof = false;
  for (;;) {
    int m = 0;
    const size_t at = pos;
    JPEG_REQUIRE(read_marker(d, n, pos, m), KVQ_ERR_SHAPE, "%s: no marker at byte %zu (the stream is cut short or not a JPEG image)", who, at);
    JPEG_REQUIRE(m != 0xD9 && m != 0xD8 && !(m >= 0xD0 && m <= 0xD7) && m != 0x01, KVQ_ERR_SHAPE,
                 "%s: marker FF%02X at byte %zu before any scan", who, m, at);
    JPEG_REQUIRE(pos + 2 <= n, KVQ_ERR_SHAPE, "%s: segment FF%02X at byte %zu is cut short", who, m, at);
    const size_t L = ((size_t)d[pos] << 8) | d[pos + 1];
    JPEG_REQUIRE(L >= 2 && pos + L <= n, KVQ_ERR_SHAPE, "%s: segment FF%02X at byte %zu is cut short (length %zu)", who, m, at, L);
    const uint8_t* s = d + pos + 2;
    const size_t sl = L - 2;
    pos += L;
    if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {           // SOFn
      JPEG_REQUIRE(!have_sof, KVQ_ERR_SHAPE, "%s: a second frame header at byte %zu", who, at);
      JPEG_REQUIRE(sl >= 6 && sl >= 6 + 3 * (size_t)s[5], KVQ_ERR_SHAPE, "%s: frame header at byte %zu is cut short", who, at);
      have_sof = true;
      if (m == 0xC2) refuse(p, 9, "%s: progressive JPEG (SOF2) is not decoded, baseline only", who);
      else if (m != 0xC0) refuse(p, 9, "%s: SOF%d (%s) is not decoded, baseline SOF0 only", who, m - 0xC0,
                                 m == 0xC1 ? "extended sequential" : m == 0xC3 ? "lossless" : m >= 0xC9 ? "arithmetic coding" : "hierarchical");
      if (s[0] != 8) refuse(p, 8, "%s: %d-bit sample precision is not decoded, 8-bit only", who, (int)s[0]);
      p.info.height = (s[1] << 8) | s[2];
      p.info.width = (s[3] << 8) | s[4];
      p.info.ncomp = s[5];
      JPEG_REQUIRE(p.info.width > 0 && p.info.height > 0, KVQ_ERR_SHAPE, "%s: frame header with size %d x %d", who, p.info.width, p.info.height);
      JPEG_REQUIRE(p.info.ncomp >= 1 && p.info.ncomp <= 4, KVQ_ERR_SHAPE, "%s: frame header with %d components", who, p.info.ncomp);
      for (int c = 0; c < p.info.ncomp; ++c) {
        Comp& k = p.comp[c];
        k.id = s[6 + 3 * c]; k.h = s[7 + 3 * c] >> 4; k.v = s[7 + 3 * c] & 15; k.tq = s[8 + 3 * c];
        p.info.hsamp[c] = k.h; p.info.vsamp[c] = k.v;
        JPEG_REQUIRE(k.tq <= 3 && k.h >= 1 && k.h <= 4 && k.v >= 1 && k.v <= 4, KVQ_ERR_SHAPE, "%s: frame header component %d is malformed", who, c);
      }
      if (p.info.ncomp != 3)
        refuse(p, 7, "%s: %d component%s (%s) — three components Y Cb Cr only", who, p.info.ncomp, p.info.ncomp == 1 ? "" : "s",
               p.info.ncomp == 1 ? "grayscale" : p.info.ncomp == 4 ? "CMYK / YCCK" : "two planes");
      else if (!(p.comp[0].h == 2 && p.comp[0].v == 2 && p.comp[1].h == 1 && p.comp[1].v == 1 && p.comp[2].h == 1 && p.comp[2].v == 1))
        refuse(p, 6, "%s: sampling factors Y %dx%d Cb %dx%d Cr %dx%d — 4:2:0 (Y 2x2 Cb 1x1 Cr 1x1) only", who, p.comp[0].h, p.comp[0].v,
               p.comp[1].h, p.comp[1].v, p.comp[2].h, p.comp[2].v);
    } else if (m == 0xDB) {                                                           // DQT, any number of tables
      size_t q = 0;
      while (q < sl) {
        const int pq = s[q] >> 4, tq = s[q] & 15;
        const size_t need = 1 + (pq ? 128 : 64);
        JPEG_REQUIRE(pq <= 1 && tq <= 3 && q + need <= sl, KVQ_ERR_SHAPE, "%s: quantiser table segment at byte %zu is malformed", who, at);
        if (pq) refuse(p, 5, "%s: 16-bit quantiser table %d is not decoded, 8-bit tables only", who, tq);
        for (int i = 0; i < 64; ++i) p.qt[tq][ZIGZAG[i]] = pq ? (uint16_t)((s[q + 1 + 2 * i] << 8) | s[q + 2 + 2 * i]) : s[q + 1 + i];
        p.qt_present[tq] = true;
        q += need;
      }
    } else if (m == 0xC4) {                                                           // DHT, any number of tables
      size_t q = 0;
      while (q < sl) {
        JPEG_REQUIRE(q + 17 <= sl, KVQ_ERR_SHAPE, "%s: Huffman table segment at byte %zu is cut short", who, at);
        const int tc = s[q] >> 4, th = s[q] & 15;
        int cnt = 0;
        for (int i = 0; i < 16; ++i) cnt += s[q + 1 + i];
        JPEG_REQUIRE(tc <= 1 && th <= 3 && cnt <= 256 && q + 17 + (size_t)cnt <= sl, KVQ_ERR_SHAPE,
                     "%s: Huffman table segment at byte %zu is malformed", who, at);
        JPEG_REQUIRE(huff_build(tc ? p.ac[th] : p.dc[th], s + q + 1, s + q + 17, cnt), KVQ_ERR_SHAPE,
                     "%s: Huffman table %d/%d at byte %zu is not a prefix code", who, tc, th, at);
        p.info.has_dht = 1;
        q += 17 + (size_t)cnt;
      }
    } else if (m == 0xDD) {                                                           // DRI
      JPEG_REQUIRE(sl >= 2, KVQ_ERR_SHAPE, "%s: restart interval segment at byte %zu is cut short", who, at);
      p.info.restart_interval = (s[0] << 8) | s[1];
    } else if (m == 0xEE) {                                                           // APP14
      if (sl >= 12 && memcmp(s, "Adobe", 5) == 0 && s[11] == 0)
        refuse(p, 4, "%s: Adobe APP14 segment with transform 0 (RGB or CMYK samples, no Y Cb Cr)", who);
    } else if (m == 0xDA) {                                                           // SOS
      JPEG_REQUIRE(have_sof, KVQ_ERR_SHAPE, "%s: scan at byte %zu before any frame header", who, at);
      JPEG_REQUIRE(sl >= 1 && sl >= 4 + 2 * (size_t)s[0], KVQ_ERR_SHAPE, "%s: scan header at byte %zu is cut short", who, at);
      const int ns = s[0];
      if (ns != p.info.ncomp) refuse(p, 3, "%s: a scan of %d of the %d components (non-interleaved) is not decoded", who, ns, p.info.ncomp);
      for (int c = 0; c < ns && c < p.info.ncomp; ++c) {
        if (s[1 + 2 * c] != p.comp[c].id) refuse(p, 3, "%s: scan components are not in frame-header order", who);
        p.comp[c].td = s[2 + 2 * c] >> 4; p.comp[c].ta = s[2 + 2 * c] & 15;
        JPEG_REQUIRE(p.comp[c].td <= 3 && p.comp[c].ta <= 3, KVQ_ERR_SHAPE, "%s: scan header at byte %zu names Huffman table %d/%d", who, at,
                     p.comp[c].td, p.comp[c].ta);
      }
      p.scan = pos;
      break;
    }                                                                                 // APPn, COM and everything else: skipped
  }
  // the image's length: entropy-coded data, then whatever segments and further scans follow, up to EOI
  size_t e = skip_scan(d, n, pos);
  while (e < n) {
    int m = 0;
    if (!read_marker(d, n, e, m)) break;
    if (m == 0xD9) { p.info.frame_bytes = (int64_t)e; break; }
    if (e + 2 > n) break;
    const size_t L = ((size_t)d[e] << 8) | d[e + 1];
    if (L < 2 || e + L > n) break;
    e += L;
    if (m == 0xDA) e = skip_scan(d, n, e);
  }
  if (p.why_rank) {
    kvq::set_error("%s", p.why);
    return KVQ_ERR_UNSUPPORTED;
  }
  p.info.supported = 1;
  return KVQ_OK;
}

// the scan's bits, most significant first; a marker or the end of the buffer ends the supply, and asking for more is an error
struct Bits {
  const uint8_t* d;
  size_t pos, n;
  uint64_t acc;
  int nbits;
  static constexpr bool own_tables = true;                    // huff_build's (lengths 0..9, indices below 256): no masks, 3 % at q50
  void fill() {
    while (nbits <= 56 && pos < n) {
      const uint8_t b = d[pos];
      if (b == 0xFF) {
        if (pos + 1 >= n || d[pos + 1] != 0x00) return;      // a marker (or the cut): stay in front of it
        pos += 2;
      } else {
        ++pos;
      }
      acc = (acc << 8) | b;
      nbits += 8;
    }
  }
  // the next 16 bits, zero-padded where the supply has ended
  uint32_t peek16() {
    if (nbits < 16) fill();
    return nbits >= 16 ? (uint32_t)(acc >> (nbits - 16)) & 0xFFFFu : (uint32_t)(acc << (16 - nbits)) & 0xFFFFu;
  }
  bool take(int k, uint32_t& out) {                           // k in 0..16
    if (nbits < k) fill();
    if (nbits < k) return false;
    out = k ? (uint32_t)(acc >> (nbits - k)) & ((1u << k) - 1u) : 0u;
    nbits -= k;
    return true;
  }
};

// one block into blk[64] (zeroed by the caller), natural order.  0, or the error text's cause
const char* decode_block(Bits& b, const Huff& dc, const Huff& ac, int32_t& pred, int16_t* blk) {
  int t = jpeg_huff_symbol(b, &dc.t);
  if (t == -JPEG_ST_TRUNCATED) return "the entropy-coded data is truncated";
  if (t == -JPEG_ST_BAD_CODE) return "a code that is in no Huffman table";
  if (t > 15) return "a DC difference of more than 15 bits";
  uint32_t v = 0;
  if (!b.take(t, v)) return "the entropy-coded data is truncated";
  pred = (int16_t)(pred + (t ? jpeg_extend(v, t) : 0));           // kept to 16 bits, as it is stored
  blk[0] = (int16_t)pred;
  int k = 1;
  while (k < 64) {
    const int rs = jpeg_huff_symbol(b, &ac.t);
    if (rs == -JPEG_ST_TRUNCATED) return "the entropy-coded data is truncated";
    if (rs == -JPEG_ST_BAD_CODE) return "a code that is in no Huffman table";
    const int r = rs >> 4, s = rs & 15;
    if (s == 0) {
      if (r != 15) break;                                     // EOB
      k += 16;                                                // ZRL
      if (k > 64) return "a zero run past coefficient 63";
      continue;
    }
    k += r;
    if (k > 63) return "a zero run past coefficient 63";
    if (!b.take(s, v)) return "the entropy-coded data is truncated";
    blk[ZIGZAG[k]] = (int16_t)jpeg_extend(v, s);
    ++k;
  }
  return nullptr;
}

// between restart intervals and at the end: drop the padding bits, then the marker `want` must stand at the read position
bool expect_marker(Bits& b, int want, int& got) {
  b.acc = 0; b.nbits = 0;
  got = -1;
  size_t pos = b.pos;
  if (!read_marker(b.d, b.n, pos, got)) { got = -1; return false; }
  if (got != want) return false;
  b.pos = pos;
  return true;
}

// the verdict on what stands where RST(want - 0xD0) before MCU `mcu` or, `last`, EOI belongs: got < 0 = no marker at all
int marker_verdict(const char* who, bool last, int want, int got, long mcu) {
  if (last && got < 0) set_error("%s: missing EOI after the last MCU (the stream is truncated)", who);
  else if (last) set_error("%s: marker FF%02X after the last MCU where EOI belongs", who, got);
  else if (got < 0) set_error("%s: missing RST%d before MCU %ld (the stream is truncated or has no marker there)", who, want - 0xD0, mcu);
  else set_error("%s: wrong restart marker FF%02X before MCU %ld, expected RST%d", who, got, mcu, want - 0xD0);
  return KVQ_ERR_SHAPE;
}

// ITU-T T.81 Annex K.3, what a stream without any DHT segment implies: DC lum, DC chroma, AC lum, AC chroma
struct StdTables {
  Huff h[4];
  StdTables() {
    huff_build(h[0], STD_DC_LUM_BITS, STD_DC_VALS, 12);
    huff_build(h[1], STD_DC_CHR_BITS, STD_DC_VALS, 12);
    huff_build(h[2], STD_AC_LUM_BITS, STD_AC_LUM_VALS, 162);
    huff_build(h[3], STD_AC_CHR_BITS, STD_AC_CHR_VALS, 162);
  }
};

// the tables the scan of a parsed image uses: per component its DC and AC table, and its quantiser table into qt_out[64 c ..]
int resolve_tables(const Parsed& p, const char* who, const Huff* dc[3], const Huff* ac[3], uint16_t* qt_out) {
  static const StdTables std_tab;
  for (int c = 0; c < 3; ++c) {
    JPEG_REQUIRE(p.qt_present[p.comp[c].tq], KVQ_ERR_SHAPE, "%s: quantiser table %d of component %d is not defined", who, p.comp[c].tq, c);
    if (p.info.has_dht) {
      dc[c] = &p.dc[p.comp[c].td]; ac[c] = &p.ac[p.comp[c].ta];
      JPEG_REQUIRE(dc[c]->present && ac[c]->present, KVQ_ERR_SHAPE, "%s: Huffman table %d/%d of component %d is not defined", who, p.comp[c].td,
                   p.comp[c].ta, c);
    } else {                                                    // no DHT at all: table 0 = luminance, any other = chrominance
      dc[c] = &std_tab.h[p.comp[c].td ? 1 : 0]; ac[c] = &std_tab.h[p.comp[c].ta ? 3 : 2];
    }
    for (int i = 0; i < 64; ++i) qt_out[64 * c + i] = p.qt[p.comp[c].tq][i];
  }
  return KVQ_OK;
}

}  // namespace

extern "C" size_t kvq_jpeg_coef_bytes(int H, int W) {
  if (!kvq::jpeg_size_ok(H, W)) return 0;
  return (size_t)kvq::jpeg_geom(H, W).blocks * 64 * sizeof(int16_t);
}

extern "C" int kvq_jpeg_probe(const uint8_t* data, size_t n, KvqJpegInfo* info) {
  JPEG_REQUIRE(data && info, KVQ_ERR_NULL, "kvq_jpeg_probe: NULL pointer");
  static thread_local Parsed p;
  const int rc = parse(data, n, p, "kvq_jpeg_probe");
  *info = p.info;
  return rc;
}

extern "C" int kvq_jpeg_coeffs(const uint8_t* data, size_t n, int16_t* coef_out, size_t coef_cap, uint16_t* qt_out) {
  using namespace kvq;
  JPEG_REQUIRE(data && coef_out && qt_out, KVQ_ERR_NULL, "kvq_jpeg_coeffs: NULL pointer");
  static thread_local Parsed p;
  if (const int rc = parse(data, n, p, "kvq_jpeg_coeffs")) return rc;
  const int H = p.info.height, W = p.info.width;
  JPEG_REQUIRE(jpeg_size_ok(H, W), KVQ_ERR_SHAPE, "kvq_jpeg_coeffs: frame of %d x %d", W, H);
  const JpegGeom g = jpeg_geom(H, W);
  const size_t bytes = (size_t)g.blocks * 64 * sizeof(int16_t);
  JPEG_REQUIRE(coef_cap >= bytes, KVQ_ERR_WORKSPACE, "kvq_jpeg_coeffs: coef_out holds %zu bytes, a %d x %d frame needs %zu", coef_cap, W, H, bytes);
  const Huff* dc[3];
  const Huff* ac[3];
  if (const int rc = resolve_tables(p, "kvq_jpeg_coeffs", dc, ac, qt_out)) return rc;
  memset(coef_out, 0, bytes);
  Bits b{data, p.scan, n, 0, 0};
  int32_t pred[3] = {0, 0, 0};
  const int ri = p.info.restart_interval;
  int mcu = 0, got = 0;
  for (int y = 0; y < g.my; ++y)
    for (int x = 0; x < g.mx; ++x, ++mcu) {
      if (ri && mcu && mcu % ri == 0) {
        const int want = 0xD0 + ((mcu / ri - 1) & 7);
        if (!expect_marker(b, want, got)) return marker_verdict("kvq_jpeg_coeffs", false, want, got, mcu);
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int k = 0; k < 6; ++k) {
        const int c = k < 4 ? 0 : k - 3;
        int16_t* blk = coef_out + (size_t)jpeg_mcu_block(g, (uint32_t)y, (uint32_t)x, (uint32_t)k) * 64;
        if (const char* why = decode_block(b, *dc[c], *ac[c], pred[c], blk)) {
          set_error("kvq_jpeg_coeffs: %s (MCU %d of %d, block %d)", why, mcu, g.nc, k);
          return KVQ_ERR_SHAPE;
        }
      }
    }
  if (!expect_marker(b, 0xD9, got)) return marker_verdict("kvq_jpeg_coeffs", true, 0xD9, got, mcu);
  return KVQ_OK;
}

// ---- entropy decode on the device: the host's share ---------------------------------------------------------------------------------
namespace {

// `t` into the set unless an identical table is there: its index
int tables_add(KvqJpegTables& set, const KvqJpegHuffTable& t) {
  for (int i = 0; i < set.ntab; ++i)
    if (memcmp(&set.tab[i], &t, sizeof(t)) == 0) return i;
  set.tab[set.ntab] = t;
  return set.ntab++;
}

}  // namespace

extern "C" int kvq_jpeg_index(const uint8_t* data, size_t n, KvqJpegInfo* info, uint32_t* seg_out, size_t seg_cap, size_t* nseg_out,
                              KvqJpegTables* tables_out, uint16_t* qt_out) {
  using namespace kvq;
  JPEG_REQUIRE(data && info && seg_out && nseg_out && tables_out && qt_out, KVQ_ERR_NULL, "kvq_jpeg_index: NULL pointer");
  static thread_local Parsed p;
  const int rc = parse(data, n, p, "kvq_jpeg_index");
  *info = p.info;
  if (rc) return rc;
  const int H = p.info.height, W = p.info.width;
  JPEG_REQUIRE(jpeg_size_ok(H, W), KVQ_ERR_SHAPE, "kvq_jpeg_index: frame of %d x %d", W, H);
  JPEG_REQUIRE(n < ((size_t)1 << 32), KVQ_ERR_SHAPE, "kvq_jpeg_index: an image of %zu bytes (offsets are 32-bit)", n);
  const JpegGeom g = jpeg_geom(H, W);
  const uint32_t ri = (uint32_t)p.info.restart_interval;
  const size_t nseg = jpeg_expected_segments(ri, g);
  *nseg_out = nseg;
  JPEG_REQUIRE(seg_cap >= nseg, KVQ_ERR_WORKSPACE, "kvq_jpeg_index: seg_out holds %zu segments, the frame has %zu", seg_cap, nseg);
  const Huff* dc[3];
  const Huff* ac[3];
  uint16_t qt[192];                                          // qt_out is written once the walk has succeeded
  if (const int rc = resolve_tables(p, "kvq_jpeg_index", dc, ac, qt)) return rc;
  // the marker walk: every 0xFF that no 0x00 follows closes a segment
  size_t pos = p.scan;
  for (size_t s = 0; s < nseg; ++s) {
    const size_t begin = pos;
    size_t end = n;
    while (pos < n) {
      const uint8_t* f = (const uint8_t*)memchr(data + pos, 0xFF, n - pos);
      if (!f) break;
      const size_t q = (size_t)(f - data);
      if (q + 1 < n && data[q + 1] == 0x00) { pos = q + 2; continue; }
      end = q;
      break;
    }
    const bool last = s + 1 == nseg;
    const int want = last ? 0xD9 : 0xD0 + (int)(s & 7);
    int got = -1;
    size_t after = end;
    if (!read_marker(data, n, after, got)) got = -1;
    if (got != want) return marker_verdict("kvq_jpeg_index", last, want, got, (long)(s + 1) * (long)ri);
    seg_out[2 * s] = (uint32_t)begin;
    seg_out[2 * s + 1] = (uint32_t)end;
    pos = after;
  }
  memset(tables_out, 0, sizeof(*tables_out));
  for (int c = 0; c < 3; ++c) {
    tables_out->dc[c] = (uint8_t)tables_add(*tables_out, dc[c]->t);
    tables_out->ac[c] = (uint8_t)tables_add(*tables_out, ac[c]->t);
  }
  memcpy(qt_out, qt, sizeof(qt));
  return KVQ_OK;
}

extern "C" int kvq_jpeg_entropy_host(const uint8_t* bytes, size_t nbytes, const uint32_t* frames, const uint32_t* segs, size_t nsegs,
                                     const KvqJpegTables* tables, size_t ntables, int T, int H, int W, int16_t* coef_out, int32_t* status_out) {
  using namespace kvq;
  JPEG_REQUIRE(bytes && frames && segs && tables && coef_out && status_out, KVQ_ERR_NULL, "kvq_jpeg_entropy_host: NULL pointer");
  JPEG_REQUIRE(T > 0 && T < 65536 && jpeg_size_ok(H, W), KVQ_ERR_SHAPE, "kvq_jpeg_entropy_host: %d frames of %dx%d", T, H, W);
  JPEG_REQUIRE(nbytes < ((size_t)1 << 32) && nsegs < ((size_t)1 << 32) && ntables > 0 && ntables < ((size_t)1 << 32), KVQ_ERR_SHAPE,
               "kvq_jpeg_entropy_host: %zu bytes, %zu segments, %zu table sets", nbytes, nsegs, ntables);
  const JpegGeom g = jpeg_geom(H, W);
  memset(coef_out, 0, (size_t)T * g.blocks * 64 * sizeof(int16_t));
  for (size_t i = 0; i < nsegs; ++i) status_out[i] = JPEG_ST_UNWRITTEN;
  for (int t = 0; t < T; ++t) {
    const uint32_t* f = frames + 5 * (size_t)t;
    if (f[2] == 0 || f[1] > nsegs || f[2] > nsegs - f[1]) continue;
    const KvqJpegTables* set = tables + (f[4] < ntables ? f[4] : 0);      // a table set that does not exist is refused before it is read
    for (uint32_t s = 0; s < f[2]; ++s)
      status_out[f[1] + s] = jpeg_entropy_segment(f, s, set, bytes, nbytes, segs, (uint32_t)nsegs, (uint32_t)ntables, g,
                                                  coef_out + (size_t)t * g.blocks * 64);
  }
  return KVQ_OK;
}

extern "C" int kvq_jpeg_idct_i420_host(const int16_t* coef, const uint16_t* qt, int T, int H, int W, uint8_t* frames_out) {
  using namespace kvq;
  JPEG_REQUIRE(coef && qt && frames_out, KVQ_ERR_NULL, "kvq_jpeg_idct_i420_host: NULL pointer");
  JPEG_REQUIRE(T > 0 && T < 65536 && jpeg_size_ok(H, W), KVQ_ERR_SHAPE, "kvq_jpeg_idct_i420_host: %d frames of %dx%d", T, H, W);
  const JpegGeom g = jpeg_geom(H, W);
  const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
  const size_t frame = (size_t)H * W + 2 * (size_t)ch * cw;
  for (int t = 0; t < T; ++t) {
    const int16_t* cf = coef + (size_t)t * g.blocks * 64;
    for (int b = 0; b < g.blocks; ++b) {
      const JpegPlaneBlock pb = jpeg_plane_block(g, b);
      const int c = pb.c, by = pb.by, bx = pb.bx, ph = c == 0 ? H : ch, pw = c == 0 ? W : cw;
      if (8 * by >= ph || 8 * bx >= pw) continue;            // a block that lies wholly in the MCU padding
      const uint16_t* q = qt + ((size_t)t * 3 + c) * 64;
      int32_t ws[8][8], v[8];
      for (int u = 0; u < 8; ++u) {
        for (int r = 0; r < 8; ++r) v[r] = jw_mul(cf[(size_t)b * 64 + 8 * r + u], q[8 * r + u]);
        jpeg_idct_pass1(v);
        for (int r = 0; r < 8; ++r) ws[r][u] = v[r];
      }
      uint8_t* out = frames_out + (size_t)t * frame + (c == 0 ? 0 : (size_t)H * W + (size_t)(c - 1) * ch * cw);
      for (int r = 0; r < 8 && 8 * by + r < ph; ++r) {
        for (int u = 0; u < 8; ++u) v[u] = ws[r][u];
        jpeg_idct_pass2(v);
        for (int u = 0; u < 8 && 8 * bx + u < pw; ++u) out[(size_t)(8 * by + r) * pw + 8 * bx + u] = (uint8_t)v[u];
      }
    }
  }
  return KVQ_OK;
}
