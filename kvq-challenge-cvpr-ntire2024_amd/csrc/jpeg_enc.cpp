// Host half of the Motion-JPEG writer (include/kvq_hip.h, "Baseline JPEG, writing"): the quantiser tables of a quality
// (kvq_jpeg_quant_tables), the scalar twin of the forward-DCT launch (kvq_jpeg_fdct_host, the arithmetic of jpeg_fdct.hpp) and the
// baseline Huffman entropy coder that turns one frame of the dense coefficient hand-over into a JFIF image (kvq_jpeg_encode).
// Plain C++17 like jpeg.cpp: no HIP call and no HIP header (tools/jpeg_enc_hostcheck.cpp builds it under the host sanitizers).
// The Huffman coding of a block is jpeg_enc_huff.hpp's jpeg_enc_block, for kvq_jpeg_encode as for the scans.  Every byte of the image
// goes through Out::put, which compares against the capacity first.
#include <stdint.h>
#include <string.h>

#include "../../include/kvq_hip.h"
#include "jpeg_enc_huff.hpp"
#include "jpeg_fdct.hpp"
#include "jpeg_host.hpp"
#include "jpeg_tables.hpp"

namespace {

using namespace kvq;

// ITU-T T.81 Annex K.1, natural order
const uint8_t STD_Q_LUM[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                               14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t STD_Q_CHR[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                               47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                               99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// the image under construction: nothing is stored at or past cap, pos keeps counting so that the caller learns what was needed
struct Out {
  uint8_t* d;
  size_t cap, pos;
  uint64_t acc;      // the low nbits bits are pending, most significant first
  int nbits;
  void put(uint8_t b) {
    if (pos < cap) d[pos] = b;
    ++pos;
  }
  void put16(unsigned v) { put((uint8_t)(v >> 8)); put((uint8_t)v); }
  void bytes(const uint8_t* s, size_t n) { for (size_t i = 0; i < n; ++i) put(s[i]); }
  bool full() const { return false; }                          // a sink of jpeg_enc_block that takes every block whole
  void put(uint32_t code, int len) {                           // len in 0..27
    acc = (acc << len) | code;
    nbits += len;
    while (nbits >= 8) {
      const uint8_t b = (uint8_t)(acc >> (nbits - 8));
      put(b);
      if (b == 0xFF) put(0);
      nbits -= 8;
    }
  }
  void flush() {                                               // pad the last byte with 1 bits
    if (nbits) put((1u << (8 - nbits)) - 1u, 8 - nbits);
    acc = 0;
  }
};

const JpegEncTables ENC = jpeg_enc_tables();      // jpeg_enc_huff.hpp

}  // namespace

extern "C" int kvq_jpeg_quant_tables(int quality, uint16_t* out) {
  JPEG_REQUIRE(out, KVQ_ERR_NULL, "kvq_jpeg_quant_tables: NULL pointer");
  JPEG_REQUIRE(quality >= 1 && quality <= 100, KVQ_ERR_SHAPE, "kvq_jpeg_quant_tables: quality %d is outside 1..100", quality);
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int c = 0; c < 3; ++c)
    for (int i = 0; i < 64; ++i) {
      const int v = ((c ? STD_Q_CHR[i] : STD_Q_LUM[i]) * s + 50) / 100;
      out[64 * c + i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
  return KVQ_OK;
}

extern "C" int kvq_jpeg_quantise_host(const int32_t* F, size_t n, int q, int16_t* out) {
  JPEG_REQUIRE(F && out, KVQ_ERR_NULL, "kvq_jpeg_quantise_host: NULL pointer");
  JPEG_REQUIRE(q >= 1 && q <= 255, KVQ_ERR_SHAPE, "kvq_jpeg_quantise_host: quantiser %d is outside 1..255", q);
  const uint32_t recip = jpeg_quant_recip((uint32_t)q), half = 4u * (uint32_t)q;
  for (size_t i = 0; i < n; ++i) {
    JPEG_REQUIRE(F[i] >= -32767 && F[i] <= 32767, KVQ_ERR_SHAPE, "kvq_jpeg_quantise_host: value %d at %zu is outside +-32767", F[i], i);
    out[i] = (int16_t)jpeg_quantise(F[i], recip, half);
  }
  return KVQ_OK;
}

extern "C" int kvq_jpeg_fdct_host(const uint8_t* src, int src_format, int T, int H, int W, const uint16_t* qt, int16_t* coef_out) {
  JPEG_REQUIRE(src && qt && coef_out, KVQ_ERR_NULL, "kvq_jpeg_fdct_host: NULL pointer");
  JPEG_REQUIRE(src_format == KVQ_SRC_U8 || src_format == KVQ_SRC_I420_BT601_FULL, KVQ_ERR_UNSUPPORTED,
               "kvq_jpeg_fdct_host: source format %d — uint8 R G B planes (KVQ_SRC_U8) or BT.601 full-range I420 frames "
               "(KVQ_SRC_I420_BT601_FULL) only; convert anything else first (kvq_yuv420_to_rgb)", src_format);
  JPEG_REQUIRE(T > 0 && T < 65536 && jpeg_size_ok(H, W), KVQ_ERR_SHAPE, "kvq_jpeg_fdct_host: %d frames of %dx%d", T, H, W);
  const JpegGeom g = jpeg_geom(H, W);
  const bool rgb = src_format == KVQ_SRC_U8;
  for (int t = 0; t < T; ++t) {
    uint32_t recip[192], half[192];
    for (int i = 0; i < 192; ++i) {
      recip[i] = jpeg_quant_recip(qt[(size_t)t * 192 + i]);
      half[i] = 4u * jpeg_quant_clamp(qt[(size_t)t * 192 + i]);
    }
    int16_t* cf = coef_out + (size_t)t * g.blocks * 64;
    for (int b = 0; b < g.blocks; ++b) {
      const JpegPlaneBlock pb = jpeg_plane_block(g, b);
      const int c = pb.c, by = pb.by, bx = pb.bx;
      int32_t ws[8][8], v[8];
      for (int r = 0; r < 8; ++r) {
        for (int u = 0; u < 8; ++u) v[u] = jpeg_src_sample(src, rgb, T, H, W, t, c, 8 * by + r, 8 * bx + u) - 128;
        jpeg_fdct_pass1(v);
        for (int u = 0; u < 8; ++u) ws[r][u] = v[u];
      }
      for (int u = 0; u < 8; ++u) {
        for (int r = 0; r < 8; ++r) v[r] = ws[r][u];
        jpeg_fdct_pass2(v);
        for (int r = 0; r < 8; ++r) cf[(size_t)b * 64 + 8 * r + u] = (int16_t)jpeg_quantise(v[r], recip[64 * c + 8 * r + u], half[64 * c + 8 * r + u]);
      }
    }
  }
  return KVQ_OK;
}

extern "C" size_t kvq_jpeg_encode_bound(int H, int W) {
  if (!jpeg_size_ok(H, W)) return 0;
  const JpegGeom g = jpeg_geom(H, W);
  // per block at most 11 + 11 bits of DC and 63 x (16 + 10) of AC = 1660 bits, every byte of them stuffed; per MCU a restart marker
  // and its padding byte; the segments around the scan take 700 bytes
  return 1024 + (size_t)g.blocks * 416 + (size_t)g.nc * 4;
}

// SOI .. SOS of the image kvq_jpeg_encode writes, through o
static void put_header(Out& o, const uint16_t* qt, int H, int W, int restart_interval, int flags) {
  static const uint8_t APP0[] = {0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  o.put16(0xFFD8);
  o.bytes(APP0, sizeof(APP0));
  const bool one_chroma = memcmp(qt + 64, qt + 128, 64 * sizeof(uint16_t)) == 0;
  for (int c = 0; c < (one_chroma ? 2 : 3); ++c) {
    o.put16(0xFFDB); o.put16(67); o.put((uint8_t)c);
    for (int i = 0; i < 64; ++i) o.put((uint8_t)qt[64 * c + ZIGZAG[i]]);
  }
  o.put16(0xFFC0); o.put16(17); o.put(8); o.put16((unsigned)H); o.put16((unsigned)W); o.put(3);
  o.put(1); o.put(0x22); o.put(0);
  o.put(2); o.put(0x11); o.put(1);
  o.put(3); o.put(0x11); o.put(one_chroma ? 1 : 2);
  if (!(flags & KVQ_JPEG_NO_DHT)) {
    const struct { uint8_t tcth; const uint8_t* bits; const uint8_t* vals; int n; } dht[4] = {
        {0x00, STD_DC_LUM_BITS, STD_DC_VALS, 12}, {0x10, STD_AC_LUM_BITS, STD_AC_LUM_VALS, 162},
        {0x01, STD_DC_CHR_BITS, STD_DC_VALS, 12}, {0x11, STD_AC_CHR_BITS, STD_AC_CHR_VALS, 162}};
    for (const auto& h : dht) {
      o.put16(0xFFC4); o.put16(19 + (unsigned)h.n); o.put(h.tcth);
      o.bytes(h.bits, 16);
      o.bytes(h.vals, (size_t)h.n);
    }
  }
  if (restart_interval) { o.put16(0xFFDD); o.put16(4); o.put16((unsigned)restart_interval); }
  static const uint8_t SOS[] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  o.bytes(SOS, sizeof(SOS));
}

// the checks kvq_jpeg_encode and kvq_jpeg_encode_header share; `who` names the entry in the message
static int check_image_args(const char* who, const uint16_t* qt, int H, int W, int restart_interval, int flags) {
  JPEG_REQUIRE(jpeg_size_ok(H, W), KVQ_ERR_SHAPE, "%s: frame of %d x %d", who, W, H);
  JPEG_REQUIRE(restart_interval >= 0 && restart_interval <= 65535, KVQ_ERR_SHAPE, "%s: restart interval %d is outside 0..65535", who, restart_interval);
  JPEG_REQUIRE((flags & ~KVQ_JPEG_NO_DHT) == 0, KVQ_ERR_SHAPE, "%s: unknown flags 0x%x", who, flags);
  for (int i = 0; i < 192; ++i)
    JPEG_REQUIRE(qt[i] >= 1 && qt[i] <= 255, KVQ_ERR_UNSUPPORTED, "%s: quantiser %d (table %d, entry %d) — baseline tables are 8-bit, 1..255", who,
                 (int)qt[i], i / 64, i % 64);
  return KVQ_OK;
}

extern "C" int kvq_jpeg_encode_header(const uint16_t* qt, int H, int W, int restart_interval, int flags, uint8_t* out, size_t cap, size_t* n_out) {
  JPEG_REQUIRE(qt && out && n_out, KVQ_ERR_NULL, "kvq_jpeg_encode_header: NULL pointer");
  *n_out = 0;
  if (const int rc = check_image_args("kvq_jpeg_encode_header", qt, H, W, restart_interval, flags)) return rc;
  Out o{out, cap, 0, 0, 0};
  put_header(o, qt, H, W, restart_interval, flags);
  *n_out = o.pos;
  JPEG_REQUIRE(o.pos <= cap, KVQ_ERR_WORKSPACE, "kvq_jpeg_encode_header: out holds %zu bytes, the header needs %zu", cap, o.pos);
  return KVQ_OK;
}

extern "C" int kvq_jpeg_encode(const int16_t* coef, const uint16_t* qt, int H, int W, int restart_interval, int flags, uint8_t* out,
                               size_t cap, size_t* n_out) {
  JPEG_REQUIRE(coef && qt && out && n_out, KVQ_ERR_NULL, "kvq_jpeg_encode: NULL pointer");
  *n_out = 0;
  if (const int rc = check_image_args("kvq_jpeg_encode", qt, H, W, restart_interval, flags)) return rc;
  const JpegGeom g = jpeg_geom(H, W);
  Out o{out, cap, 0, 0, 0};
  put_header(o, qt, H, W, restart_interval, flags);
  int32_t pred[3] = {0, 0, 0};
  int mcu = 0;
  for (int y = 0; y < g.my; ++y)
    for (int x = 0; x < g.mx; ++x, ++mcu) {
      if (restart_interval && mcu && mcu % restart_interval == 0) {
        o.flush();
        o.put16(0xFFD0u + (unsigned)((mcu / restart_interval - 1) & 7));
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int k = 0; k < 6; ++k) {
        const int c = k < 4 ? 0 : k - 3;
        const size_t b = jpeg_mcu_block(g, (uint32_t)y, (uint32_t)x, (uint32_t)k);
        const int16_t* blk = coef + b * 64;
        const int32_t diff = blk[0] - pred[c];
        const bool ok = jpeg_enc_block(blk, pred[c], c != 0, &ENC.t[0][0], o);
        pred[c] = blk[0];
        if (ok) continue;
        // baseline has no code for a value of this block: name the first one in coding order
        const size_t bi = b - (c == 0 ? 0 : (size_t)g.ny + (size_t)(c - 1) * g.nc);      // the block inside its plane
        JPEG_REQUIRE(jpeg_enc_category(diff < 0 ? -diff : diff) <= 11, KVQ_ERR_UNSUPPORTED,
                     "kvq_jpeg_encode: DC difference %d (plane %d, block %zu) is outside baseline's +-2047", diff, c, bi);
        int i = 1;
        for (int32_t v; i < 63 && (v = blk[ZIGZAG[i]], jpeg_enc_category(v < 0 ? -v : v) <= 10);) ++i;
        JPEG_REQUIRE(false, KVQ_ERR_UNSUPPORTED, "kvq_jpeg_encode: coefficient %d (plane %d, block %zu, zigzag position %d) is outside baseline's +-1023",
                     (int)blk[ZIGZAG[i]], c, bi, i);
      }
    }
  o.flush();
  o.put16(0xFFD9);
  *n_out = o.pos;
  JPEG_REQUIRE(o.pos <= cap, KVQ_ERR_WORKSPACE, "kvq_jpeg_encode: out holds %zu bytes, this %d x %d frame needs %zu (kvq_jpeg_encode_bound: %zu)",
               cap, W, H, o.pos, kvq_jpeg_encode_bound(H, W));
  return KVQ_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The scans of T frames, the phases of jpeg_enc_huff.hpp in loops: the twin of kvq_jpeg_encode_scans (jpeg_enc_entropy.hip)

extern "C" size_t kvq_jpeg_scans_workspace_bytes(int T, int H, int W) {
  if (T <= 0 || T >= 65536 || !jpeg_size_ok(H, W)) return 0;
  return jpeg_scans_workspace((size_t)T, jpeg_geom(H, W));
}

extern "C" int kvq_jpeg_encode_scans_host(const int16_t* coef, int T, int H, int W, int restart_interval, uint8_t* out, size_t cap,
                                          uint32_t* frames_out, void* workspace, size_t workspace_bytes) {
  JPEG_REQUIRE(coef && out && frames_out && workspace, KVQ_ERR_NULL, "kvq_jpeg_encode_scans_host: NULL pointer");
  JPEG_REQUIRE(T > 0 && T < 65536 && jpeg_size_ok(H, W), KVQ_ERR_SHAPE, "kvq_jpeg_encode_scans_host: %d frames of %dx%d", T, H, W);
  JPEG_REQUIRE(restart_interval >= 0 && restart_interval <= 65535, KVQ_ERR_SHAPE, "kvq_jpeg_encode_scans_host: restart interval %d is outside 0..65535",
               restart_interval);
  JPEG_REQUIRE(cap < ((size_t)1 << 32), KVQ_ERR_SHAPE, "kvq_jpeg_encode_scans_host: a capacity of %zu bytes; offsets are 32-bit", cap);
  JPEG_REQUIRE((((uintptr_t)coef | (uintptr_t)workspace) & 15) == 0 && ((uintptr_t)frames_out & 3) == 0, KVQ_ERR_SHAPE,
               "kvq_jpeg_encode_scans_host: coef and workspace must be 16-byte aligned, frames_out 4-byte aligned");
  JpegScansPlan p{};
  p.coef = coef; p.out = out; p.frames_out = frames_out;
  p.cap = cap; p.T = (uint32_t)T; p.ri = (uint32_t)restart_interval; p.g = jpeg_geom(H, W);
  JPEG_REQUIRE(workspace_bytes >= jpeg_scans_workspace((size_t)T, p.g), KVQ_ERR_WORKSPACE,
               "kvq_jpeg_encode_scans_host: a workspace of %zu bytes; %d frames of %dx%d need %zu (kvq_jpeg_scans_workspace_bytes)", workspace_bytes, T, H,
               W, jpeg_scans_workspace((size_t)T, p.g));
  jpeg_scans_layout(p, workspace);
  memset(p.fr32, 0, 8 * (size_t)T);
  const uint32_t* tab = &ENC.t[0][0];
  const uint32_t blocks = (uint32_t)p.g.blocks;
  for (uint32_t t = 0; t < p.T; ++t)
    for (uint32_t s = 0; s < blocks; ++s) jpeg_scans_count(p, tab, t, s);
  for (uint32_t t = 0; t < p.T; ++t) {
    uint64_t x = 0;
    for (uint32_t s = 0; s < blocks; ++s) {
      const JpegScanSeg e = jpeg_scans_seg(p, p.fr32[2 * (size_t)t] != 0u, t, s);
      p.pos[(size_t)t * blocks + s] = e.e ? (x + 7u) & ~(uint64_t)7 : x;
      x = jpeg_scan_apply(e, x);
    }
    p.fr64[2 * (size_t)t] = (x + 7u) >> 3;
  }
  for (uint32_t t = 0; t < p.T; ++t)
    for (uint32_t s = 0; s < blocks; ++s) jpeg_scans_ffcount(p, tab, t, s);
  for (uint32_t t = 0; t < p.T; ++t) {
    uint32_t x = 0;
    for (uint32_t s = 0; s < blocks; ++s) {
      const uint32_t n = p.cnt[(size_t)t * blocks + s];
      p.cnt[(size_t)t * blocks + s] = x;
      x += n;
    }
    p.fr32[2 * (size_t)t + 1] = x;
  }
  jpeg_scans_frames(p);
  for (uint32_t t = 0; t < p.T; ++t)
    for (uint32_t s = 0; s < blocks; ++s) jpeg_scans_write(p, tab, t, s);
  return KVQ_OK;
}
