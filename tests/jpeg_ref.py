"""The baseline-JPEG reader of include/kvq_hip.h restated in Python / numpy, independent of the library: the segment walk, the
Huffman entropy decode into the dense coefficient hand-over (per-plane block raster, natural order), the two-pass integer inverse
DCT of csrc/jpeg_idct.hpp (int32 with wrap-around, which is what numpy int32 arrays do), and — for the tests that need many frames
without an encoder library — an entropy ENCODER that writes given quantised coefficients as a baseline 4:2:0 stream with the
Annex K Huffman tables, plus writers of the three containers (raw stream, AVI, directory)."""
import os
import struct

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])

# ITU-T T.81 Annex K.3
STD_DC_LUM = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
STD_DC_CHR = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
STD_AC_LUM = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
              [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240,
               36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72,
               73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131,
               132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170,
               178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216,
               217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250])
STD_AC_CHR = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
              [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240,
               21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70,
               71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121,
               122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167,
               168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213,
               214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250])


class JpegError(ValueError):
    pass


def geom(H, W):
    """(mx, my, ny, nc, blocks): MCUs across / down, blocks of the Y plane, of one chroma plane, of a frame"""
    mx, my = (W + 15) // 16, (H + 15) // 16
    return mx, my, 4 * mx * my, mx * my, 6 * mx * my


def coef_bytes(H, W):
    return geom(H, W)[4] * 128


def frame_bytes(H, W):
    return H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)


def _codes(bits, vals):
    """canonical code of a (counts per length, symbols) table: {(length, code): symbol}"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[(length, code)] = vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return out


def parse(data):
    """segments up to SOS -> dict(W, H, comps [(id, h, v, tq)], qt {tq: uint16[64] natural}, huff {(tc, th): codes}, ri, scan, sof,
    precision, adobe_transform, q16)"""
    d = bytes(data)
    if d[:2] != b"\xff\xd8":
        raise JpegError("no SOI")
    p = dict(qt={}, huff={}, ri=0, sof=None, adobe_transform=None, q16=False)
    pos = 2
    while True:
        if d[pos] != 0xFF:
            raise JpegError(f"no marker at {pos}")
        while d[pos] == 0xFF:
            pos += 1
        m = d[pos]
        pos += 1
        L = struct.unpack(">H", d[pos:pos + 2])[0]
        s = d[pos + 2:pos + L]
        if len(s) != L - 2:
            raise JpegError("segment cut short")
        pos += L
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            p["sof"], p["precision"] = m - 0xC0, s[0]
            p["H"], p["W"] = struct.unpack(">HH", s[1:5])
            p["comps"] = [(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(s[5])]
        elif m == 0xDB:
            q = 0
            while q < len(s):
                pq, tq = s[q] >> 4, s[q] & 15
                raw = np.frombuffer(s[q + 1:q + 1 + (128 if pq else 64)], ">u2" if pq else np.uint8).astype(np.uint16)
                p["q16"] |= bool(pq)
                nat = np.zeros(64, np.uint16)
                nat[ZIGZAG] = raw
                p["qt"][tq] = nat
                q += 1 + (128 if pq else 64)
        elif m == 0xC4:
            q = 0
            while q < len(s):
                bits = list(s[q + 1:q + 17])
                n = sum(bits)
                p["huff"][(s[q] >> 4, s[q] & 15)] = _codes(bits, list(s[q + 17:q + 17 + n]))
                q += 17 + n
        elif m == 0xDD:
            p["ri"] = struct.unpack(">H", s[:2])[0]
        elif m == 0xEE and s[:5] == b"Adobe":
            p["adobe_transform"] = s[11]
        elif m == 0xDA:
            p["scan_tables"] = [(s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15) for c in range(s[0])]
            p["scan"] = pos
            return p


def supported(p):
    return (p["sof"] == 0 and p["precision"] == 8 and not p["q16"] and [c[1:3] for c in p["comps"]] == [(2, 2), (1, 1), (1, 1)]
            and p["adobe_transform"] != 0)


class _Bits:
    def __init__(self, d, pos):
        self.d, self.pos, self.acc, self.n = d, pos, 0, 0

    def need(self, k):
        d = self.d
        while self.n < k:
            if self.pos >= len(d):
                raise JpegError("truncated")
            b = d[self.pos]
            if b == 0xFF:
                if self.pos + 1 >= len(d) or d[self.pos + 1] != 0:
                    raise JpegError("truncated (marker inside the data)")
                self.pos += 2
            else:
                self.pos += 1
            self.acc = ((self.acc << 8) | b) & 0xFFFFFFFFFF
            self.n += 8

    def bit(self):
        self.need(1)
        self.n -= 1
        return (self.acc >> self.n) & 1

    def take(self, k):
        if k == 0:
            return 0
        self.need(k)
        self.n -= k
        return (self.acc >> self.n) & ((1 << k) - 1)

    def symbol(self, codes):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            s = codes.get((length, code))
            if s is not None:
                return s
        raise JpegError("code not in table")

    def marker(self):
        """drop the padding bits; the marker at the read position"""
        self.acc = self.n = 0
        d = self.d
        if self.pos >= len(d) or d[self.pos] != 0xFF:
            raise JpegError("no marker")
        while self.pos < len(d) and d[self.pos] == 0xFF:
            self.pos += 1
        if self.pos >= len(d):
            raise JpegError("no marker")
        self.pos += 1
        return d[self.pos - 1]


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def _wrap16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def decode_coeffs(data):
    """one baseline 4:2:0 image -> (coef int16 (blocks, 64), qt uint16 (3, 64), parse dict)"""
    d = bytes(data)
    p = parse(d)
    if not supported(p):
        raise JpegError("unsupported")
    H, W = p["H"], p["W"]
    mx, my, ny, nc, blocks = geom(H, W)
    std = {(0, 0): STD_DC_LUM, (0, 1): STD_DC_CHR, (1, 0): STD_AC_LUM, (1, 1): STD_AC_CHR}
    tabs = []
    for c in range(3):
        td, ta = p["scan_tables"][c]
        if p["huff"]:
            tabs.append((p["huff"][(0, td)], p["huff"][(1, ta)]))
        else:
            tabs.append((_codes(*std[(0, min(td, 1))]), _codes(*std[(1, min(ta, 1))])))
    qt = np.stack([p["qt"][p["comps"][c][3]] for c in range(3)])
    coef = np.zeros((blocks, 64), np.int16)
    base = (0, ny, ny + nc)
    bits = _Bits(d, p["scan"])
    pred = [0, 0, 0]
    mcu = 0
    for y in range(my):
        for x in range(mx):
            if p["ri"] and mcu and mcu % p["ri"] == 0:
                if bits.marker() != 0xD0 + ((mcu // p["ri"] - 1) & 7):
                    raise JpegError("wrong RSTn")
                pred = [0, 0, 0]
            for k in range(6):
                c = 0 if k < 4 else k - 3
                blk = base[c] + ((2 * y + (k >> 1)) * 2 * mx + 2 * x + (k & 1) if c == 0 else y * mx + x)
                dc, ac = tabs[c]
                t = bits.symbol(dc)
                pred[c] = _wrap16(pred[c] + (_extend(bits.take(t), t) if t else 0))
                row = coef[blk]
                row[0] = pred[c]
                i = 1
                while i < 64:
                    rs = bits.symbol(ac)
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        i += 16
                        if i > 64:
                            raise JpegError("run past 63")
                        continue
                    i += r
                    if i > 63:
                        raise JpegError("run past 63")
                    row[ZIGZAG[i]] = _extend(bits.take(s), s)
                    i += 1
            mcu += 1
    if bits.marker() != 0xD9:
        raise JpegError("missing EOI")
    p["frame_bytes"] = bits.pos
    return coef, qt, p


def _idct8(v):
    """csrc/jpeg_idct.hpp jpeg_idct8 on int32 arrays v[0..7] (each any shape): wrap-around int32 throughout"""
    c = np.int32
    z1 = (v[2] + v[6]) * c(4433)
    t2 = z1 + v[6] * c(-15137)
    t3 = z1 + v[2] * c(6270)
    t0, t1 = (v[0] + v[4]) << c(13), (v[0] - v[4]) << c(13)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * c(9633)
    o0, o1, o2, o3 = o0 * c(2446), o1 * c(16819), o2 * c(25172), o3 * c(12299)
    z1, z2 = z1 * c(-7373), z2 * c(-20995)
    z3, z4 = z3 * c(-16069) + z5, z4 * c(-3196) + z5
    o0, o1, o2, o3 = o0 + (z1 + z3), o1 + (z2 + z4), o2 + (z2 + z3), o3 + (z1 + z4)
    return [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]


def idct_blocks(coef, q):
    """coef int16 (n, 64), q uint16 (n, 64) or (64,) -> uint8 (n, 8, 8) samples"""
    with np.errstate(over="ignore"):
        d = (coef.astype(np.int32) * np.asarray(q).astype(np.int32)).reshape(-1, 8, 8)
        ws = np.stack(_idct8([d[:, r, :] for r in range(8)]), axis=1)                    # pass 1: along the vertical frequency
        ws = (ws + np.int32(1 << 10)) >> np.int32(11)
        px = np.stack(_idct8([ws[:, :, u] for u in range(8)]), axis=2)                   # pass 2: along the rows
        px = ((px + np.int32(1 << 17)) >> np.int32(18)) + np.int32(128)
    return np.clip(px, 0, 255).astype(np.uint8)


def idct_i420(coef, qt, H, W):
    """one frame's coefficients (blocks, 64) + tables (3, 64) -> the I420 frame (frame_bytes,) uint8, MCU padding cropped"""
    mx, my, ny, nc, blocks = geom(H, W)
    coef = np.asarray(coef).reshape(blocks, 64)
    out = []
    for c, (lo, n, bpr, ph, pw) in enumerate(((0, ny, 2 * mx, H, W), (ny, nc, mx, (H + 1) // 2, (W + 1) // 2),
                                              (ny + nc, nc, mx, (H + 1) // 2, (W + 1) // 2))):
        px = idct_blocks(coef[lo:lo + n], np.asarray(qt).reshape(3, 64)[c])
        plane = px.reshape(n // bpr, bpr, 8, 8).transpose(0, 2, 1, 3).reshape(n // bpr * 8, bpr * 8)
        out.append(plane[:ph, :pw].reshape(-1))
    return np.concatenate(out)


def decode_i420(data):
    """one image -> (I420 frame bytes, H, W)"""
    coef, qt, p = decode_coeffs(data)
    return idct_i420(coef, qt, p["H"], p["W"]), p["H"], p["W"]


def planes(frame, H, W):
    ch, cw = (H + 1) // 2, (W + 1) // 2
    return frame[:H * W].reshape(H, W), frame[H * W:H * W + ch * cw].reshape(ch, cw), frame[H * W + ch * cw:].reshape(ch, cw)


# ---- an entropy encoder: given quantised coefficients -> a baseline 4:2:0 stream with the Annex K tables ---------------------------
def _enc_table(bits, vals):
    return {sym: (length, code) for (length, code), sym in _codes(bits, vals).items()}


def encode_baseline(coef, qt, H, W, restart=0, dht=True):
    """coef int16 (blocks, 64) in the hand-over layout (|AC| < 1024, DC differences < 2048), qt (3, 64) 8-bit -> bytes"""
    mx, my, ny, nc, blocks = geom(H, W)
    coef = np.asarray(coef, np.int64).reshape(blocks, 64)
    qt = np.asarray(qt).reshape(3, 64)
    out = bytearray(b"\xff\xd8")
    for c in range(3 if not np.array_equal(qt[1], qt[2]) else 2):
        out += b"\xff\xdb" + struct.pack(">HB", 67, c) + bytes(int(v) for v in qt[c][ZIGZAG])
    tq = (0, 1, 2) if not np.array_equal(qt[1], qt[2]) else (0, 1, 1)
    out += b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, H, W, 3) + bytes([1, 0x22, tq[0], 2, 0x11, tq[1], 3, 0x11, tq[2]])
    if dht:
        for tcth, (bits, vals) in ((0x00, STD_DC_LUM), (0x10, STD_AC_LUM), (0x01, STD_DC_CHR), (0x11, STD_AC_CHR)):
            out += b"\xff\xc4" + struct.pack(">HB", 19 + len(vals), tcth) + bytes(bits) + bytes(vals)
    if restart:
        out += b"\xff\xdd" + struct.pack(">HH", 4, restart)
    out += b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    enc = [(_enc_table(*STD_DC_LUM), _enc_table(*STD_AC_LUM)), (_enc_table(*STD_DC_CHR), _enc_table(*STD_AC_CHR))]
    acc, n = 0, 0
    body = bytearray()

    def put(length, code):
        nonlocal acc, n
        acc, n = (acc << length) | code, n + length
        while n >= 8:
            b = (acc >> (n - 8)) & 255
            body.append(b)
            if b == 255:
                body.append(0)
            n -= 8
        acc &= (1 << n) - 1

    def flush():
        nonlocal acc, n
        if n:
            put(8 - n, (1 << (8 - n)) - 1)

    def value(v):
        s = int(abs(v)).bit_length()
        return s, (v if v >= 0 else v + (1 << s) - 1)

    base = (0, ny, ny + nc)
    pred = [0, 0, 0]
    mcu = 0
    for y in range(my):
        for x in range(mx):
            if restart and mcu and mcu % restart == 0:
                flush()
                body.extend(bytes([0xFF, 0xD0 + ((mcu // restart - 1) & 7)]))
                pred = [0, 0, 0]
            for k in range(6):
                c = 0 if k < 4 else k - 3
                blk = coef[base[c] + ((2 * y + (k >> 1)) * 2 * mx + 2 * x + (k & 1) if c == 0 else y * mx + x)]
                dc, ac = enc[min(c, 1)]
                s, bits_ = value(int(blk[0]) - pred[c])
                pred[c] = int(blk[0])
                put(*dc[s])
                if s:
                    put(s, bits_)
                zz = blk[ZIGZAG]
                run = 0
                last = int(np.max(np.nonzero(zz)[0])) if zz.any() else 0
                for i in range(1, last + 1):
                    v = int(zz[i])
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        put(*ac[0xF0])
                        run -= 16
                    s, bits_ = value(v)
                    put(*ac[(run << 4) | s])
                    put(s, bits_)
                    run = 0
                if last < 63:
                    put(*ac[0x00])
            mcu += 1
    flush()
    return bytes(out + body + b"\xff\xd9")


def synthetic_coefficients(seed, T, H, W, budget=8192):
    """(coef int16 (T, blocks, 64), qt uint16 (T, 3, 64)): random sparse blocks whose sum |coef * q| stays within ``budget`` (the
    defined range of csrc/jpeg_idct.hpp), per-frame tables, DC values spread so that both clamps are reached"""
    g = np.random.Generator(np.random.PCG64(seed))
    blocks = geom(H, W)[4]
    qt = g.integers(1, 40, (T, 3, 64)).astype(np.uint16)
    qt[:, :, 0] = g.integers(1, 17, (T, 3))
    coef = np.zeros((T, blocks, 64), np.int64)
    qb = np.concatenate([np.repeat(qt[:, c:c + 1], n, axis=1) for c, n in enumerate((geom(H, W)[2], geom(H, W)[3], geom(H, W)[3]))], axis=1)
    coef[:, :, 0] = g.integers(-1000, 1001, (T, blocks)) // qb[:, :, 0].astype(np.int64)
    for _ in range(6):
        pos = g.integers(1, 64, (T, blocks))
        val = g.integers(-400, 401, (T, blocks))
        q = np.take_along_axis(qb, pos[..., None], axis=2)[..., 0].astype(np.int64)
        np.put_along_axis(coef, pos[..., None], (val // q)[..., None], axis=2)
    assert int((np.abs(coef) * qb).sum(axis=2).max()) <= budget
    return coef.astype(np.int16), qt


# ---- containers -------------------------------------------------------------------------------------------------------------------
def write_mjpeg(path, frames):
    with open(path, "wb") as f:
        for b in frames:
            f.write(b)


def write_dir(path, frames, names=None):
    os.makedirs(path, exist_ok=True)
    for i, b in enumerate(frames):
        with open(os.path.join(path, names[i] if names else f"{i + 1}.jpg"), "wb") as f:
            f.write(b)


def write_avi(path, frames, W, H, rate=30000, scale=1001, idx1=True, handler=b"MJPG", compression=b"MJPG"):
    """a minimal RIFF AVI: hdrl (avih, one strl with strh + strf), movi of 00dc chunks (an empty ``frames`` entry = a zero-length chunk,
    a repeat of the previous frame), idx1 when asked"""
    def chunk(fcc, payload):
        return fcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")

    def lst(kind, payload):
        return b"LIST" + struct.pack("<I", 4 + len(payload)) + kind + payload

    n = len(frames)
    avih = struct.pack("<14I", int(1e6 * scale / rate), 0, 0, 0x10 if idx1 else 0, n, 0, 1, 0, W, H, 0, 0, 0, 0)
    strh = b"vids" + handler + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, scale, rate, 0, n, 0, 0xFFFFFFFF, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, compression, W * H * 3, 0, 0, 0, 0)
    hdrl = lst(b"hdrl", chunk(b"avih", avih) + lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf)))
    movi, index, off = b"", b"", 4
    for b in frames:
        index += b"00dc" + struct.pack("<III", 0x10, off, len(b))
        c = chunk(b"00dc", bytes(b))
        movi += c
        off += len(c)
    body = hdrl + lst(b"movi", movi) + (chunk(b"idx1", index) if idx1 else b"")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + len(body)) + b"AVI " + body)
