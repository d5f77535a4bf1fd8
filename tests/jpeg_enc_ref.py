"""The baseline-JPEG writer of include/kvq_hip.h restated in Python / numpy, independent of the library: the quality -> quantiser
table scaling, the block analysis of csrc/jpeg_fdct.hpp (RGB -> YCbCr, 2 x 2 chroma averaging, MCU padding by clamped coordinates,
level shift, the two-pass integer forward DCT, the quantiser — here as the plain division the header's reciprocal form must equal)
and the byte layout of the image ``kvq_jpeg_encode`` writes: that of ``jpeg_ref.encode_baseline`` with a JFIF APP0 segment behind
SOI."""
import numpy as np

import jpeg_ref

# ITU-T T.81 Annex K.1, natural order
STD_Q_LUM = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                      80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                      95, 98, 112, 100, 103, 99])
STD_Q_CHR = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99] + [99] * 36)
APP0 = b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
SRC_U8, SRC_I420_BT601_FULL = 1, 3


def quant_tables(quality):
    """uint16 (3, 64): Y, Cb, Cr tables of an IJG quality 1..100"""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    lum, chr_ = (np.clip((b * s + 50) // 100, 1, 255).astype(np.uint16) for b in (STD_Q_LUM, STD_Q_CHR))
    return np.stack([lum, chr_, chr_])


def rgb_planes(rgb):
    """uint8 (3, H, W) -> int64 Y (H, W), Cb, Cr (ceil(H/2), ceil(W/2))"""
    r, g, b = (rgb[c].astype(np.int64) for c in range(3))
    H, W = r.shape
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    ch, cw = (H + 1) // 2, (W + 1) // 2
    ys, xs = np.minimum(np.arange(2 * ch), H - 1), np.minimum(np.arange(2 * cw), W - 1)
    bias = 1 + (np.arange(cw) & 1)
    out = [y]
    for p in (cb, cr):
        p = p[ys][:, xs]
        out.append((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias[None, :]) >> 2)
    return out


def i420_planes(frame, H, W):
    return [p.astype(np.int64) for p in jpeg_ref.planes(np.asarray(frame).reshape(-1), H, W)]


def _fdct8(v, s0, sn):
    """csrc/jpeg_fdct.hpp jpeg_fdct8 on int64 arrays v[0..7] (no intermediate leaves int32)"""
    def ds(x, n):
        return (x + (1 << (n - 1))) >> n
    t0, t7, t1, t6, t2, t5, t3, t4 = v[0] + v[7], v[0] - v[7], v[1] + v[6], v[1] - v[6], v[2] + v[5], v[2] - v[5], v[3] + v[4], v[3] - v[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    o[0] = (t10 + t11) << s0 if s0 > 0 else ds(t10 + t11, -s0)
    o[4] = (t10 - t11) << s0 if s0 > 0 else ds(t10 - t11, -s0)
    z1 = (t12 + t13) * 4433
    o[2], o[6] = ds(z1 + t13 * 6270, sn), ds(z1 + t12 * -15137, sn)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    o4, o5, o6, o7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = ds(o4 + z1 + z3, sn), ds(o5 + z2 + z4, sn), ds(o6 + z2 + z3, sn), ds(o7 + z1 + z4, sn)
    for x in o:
        assert np.abs(x).max(initial=0) < 2 ** 31
    return o


def fdct_blocks(samples):
    """samples (n, 8, 8) in 0..255 -> 8 x their DCT, int64 (n, 8, 8), index [v][u]"""
    d = np.asarray(samples, np.int64) - 128
    ws = np.stack(_fdct8([d[:, :, u] for u in range(8)], 2, 11), axis=2)                # pass 1: along the rows
    return np.stack(_fdct8([ws[:, r, :] for r in range(8)], -2, 15), axis=1)            # pass 2: down the columns


def quantise(F, q):
    """sign(F) * ((|F| + (d >> 1)) // d), d = q << 3: the plain division"""
    F, d = np.asarray(F, np.int64), np.asarray(q, np.int64) << 3
    return np.sign(F) * ((np.abs(F) + (d >> 1)) // d)


def fdct_frame(planes, qt, H, W):
    """[Y, Cb, Cr] planes of one frame -> int16 (blocks, 64) in the hand-over layout"""
    mx, my, ny, nc, blocks = jpeg_ref.geom(H, W)
    out = []
    for c, p in enumerate(planes):
        ph, pw = (16 * my, 16 * mx) if c == 0 else (8 * my, 8 * mx)
        p = p[np.minimum(np.arange(ph), p.shape[0] - 1)][:, np.minimum(np.arange(pw), p.shape[1] - 1)]
        b = p.reshape(ph // 8, 8, pw // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
        out.append(quantise(fdct_blocks(b), np.asarray(qt).reshape(3, 8, 8)[c][None]).reshape(-1, 64))
    return np.concatenate(out).astype(np.int16)


def fdct(src, src_format, T, H, W, qt):
    """src: uint8 (3, T, H, W) for SRC_U8, (T, frame_bytes) for SRC_I420_BT601_FULL; qt (T, 3, 64) -> int16 (T, blocks * 64)"""
    qt = np.asarray(qt).reshape(T, 3, 64)
    src = np.asarray(src)
    return np.stack([fdct_frame(rgb_planes(src[:, t]) if src_format == SRC_U8 else i420_planes(src[t], H, W), qt[t], H, W).reshape(-1)
                     for t in range(T)])


def picture_blocks(H, W):
    """bool (blocks,): the blocks whose coefficients are fixed by the picture alone, whatever an encoder pads with — every Y block that
    holds at least one sample, every chroma block that lies wholly inside its plane"""
    mx, my, ny, nc, blocks = jpeg_ref.geom(H, W)
    ch, cw = (H + 1) // 2, (W + 1) // 2
    y = (8 * np.arange(2 * my)[:, None] < H) & (8 * np.arange(2 * mx)[None, :] < W)
    c = (8 * np.arange(my)[:, None] + 8 <= ch) & (8 * np.arange(mx)[None, :] + 8 <= cw)
    return np.concatenate([y.reshape(-1), c.reshape(-1), c.reshape(-1)])


def encode(coef, qt, H, W, restart=0, dht=True):
    """the bytes ``kvq_jpeg_encode`` writes for one frame"""
    b = jpeg_ref.encode_baseline(coef, qt, H, W, restart=restart, dht=dht)
    return b[:2] + APP0 + b[2:]
