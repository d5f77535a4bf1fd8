"""What tests/test_mjpeg_entropy_cpu.py and tests/test_gpu_mjpeg_entropy.py share: the synthetic corpus (frames written by
tests/jpeg_ref.py's encoder from seeded coefficients), a numpy marker search that restates the segment index, the packing of several
frames into the arguments of ``kernels.jpeg_entropy`` / ``jpeg_entropy_host``, and the hand-made malformed segments.  Expected
coefficients never come from here: they are ``kvq_jpeg_coeffs``' and the restatement's."""
import numpy as np

from kvq_amd import kernels

import jpeg_ref

FIXTURES = ["noise_q100", "noise_q5", "odd", "odd_no_dht", "odd_optimize", "odd_restart", "one_mcu", "sub_mcu", "video_0", "video_1", "video_2"]
# (H, W, restart, dht): 130 x 150 is 10 x 9 = 90 MCUs — restart 1: 90 segments, more than one wave, RSTn wrapping past 7 eleven times;
# 7 does not divide 90: a short last segment; 10 = one MCU row; 200: a DRI and no marker — one MCU; an unaligned size
SYNTHETIC = [(130, 150, ri, dht) for ri in (0, 1, 7, 10, 200) for dht in (True, False)] + [(16, 16, 0, True), (16, 16, 1, False),
                                                                                             (45, 70, 0, True), (45, 70, 3, False)]
# (130, 150): a seed whose luminance DC quantiser is 1, so that DC differences reach category 10 (the corpus test checks it)
SEEDS = {(130, 150): 7, (16, 16): 5, (45, 70): 6}


def case_id(c):
    return "%dx%d-ri%d-%s" % (c[0], c[1], c[2], "dht" if c[3] else "nodht")


_coef_cache = {}


def coefficients(H, W):
    """the seeded coefficients (blocks, 64) and tables (3, 64) of the synthetic frames of H x W"""
    if (H, W) not in _coef_cache:
        coef, qt = jpeg_ref.synthetic_coefficients(SEEDS[(H, W)], 1, H, W)
        _coef_cache[(H, W)] = (coef[0], qt[0])
    return _coef_cache[(H, W)]


def synthetic(c):
    H, W, ri, dht = c
    coef, qt = coefficients(H, W)
    return jpeg_ref.encode_baseline(coef, qt, H, W, restart=ri, dht=dht)


def host_coeffs(jpg, H, W):
    """``kvq_jpeg_coeffs``: (status, coefficients (blocks, 64), tables, message)"""
    coef, qt = np.zeros(kernels.jpeg_coef_bytes(H, W) // 2, np.int16), np.zeros((3, 64), np.uint16)
    rc, msg = kernels.jpeg_coeffs(np.frombuffer(bytes(jpg), np.uint8), coef, qt)
    return rc, coef.reshape(-1, 64), qt, msg


def marker_search(jpg):
    """the segments of the image's scan by a numpy search: every 0xFF of the entropy-coded bytes that no 0x00 follows starts a marker
    (the test streams have no fill bytes) -> (uint32 (nseg, 2) byte ranges, the markers' codes)"""
    d = np.frombuffer(bytes(jpg), np.uint8)
    scan = jpeg_ref.parse(bytes(jpg))["scan"]
    ff = np.nonzero((d[scan:-1] == 0xFF) & (d[scan + 1:] != 0x00))[0] + scan
    begins = np.concatenate([[scan], ff[:-1] + 2])
    return np.stack([begins, ff], 1).astype(np.uint32), d[ff + 1]


def index(jpg, cap=None):
    """``kernels.jpeg_index`` with room for ``cap`` segments (None: the MCU count, which is always enough)"""
    if cap is None:
        p = jpeg_ref.parse(bytes(jpg))
        cap = jpeg_ref.geom(p["H"], p["W"])[3]
    segs, tables, qt = np.zeros((cap, 2), np.uint32), np.zeros(kernels.JPEG_TABLES_BYTES, np.uint8), np.zeros((3, 64), np.uint16)
    rc, info, nseg, msg = kernels.jpeg_index(np.frombuffer(bytes(jpg), np.uint8), segs, tables, qt)
    return rc, info, segs[:nseg] if rc == 0 else segs, tables, qt, msg


def pack(jpgs, front=0):
    """the arguments of the entropy decode for the frames ``jpgs`` (all of one size): data uint8 with ``front`` bytes of 0xFF before
    the first image, frames uint32 (T, 5), segs uint32 (nsegs, 2), tables uint8 (ntables, JPEG_TABLES_BYTES) with identical sets once,
    qt uint16 (T, 3, 64)"""
    data, frames, segs, sets, qts = [b"\xff" * front], [], [], [], []
    off = front
    for jpg in jpgs:
        rc, info, sg, tables, qt, msg = index(jpg)
        assert rc == 0, msg
        key = tables.tobytes()
        if key not in sets:
            sets.append(key)
        frames.append((off, sum(len(s) for s in segs), len(sg), info.restart_interval, sets.index(key)))
        segs.append(sg)
        qts.append(qt)
        data.append(bytes(jpg))
        off += len(jpg)
    return (np.frombuffer(b"".join(data), np.uint8).copy(), np.array(frames, np.uint32), np.ascontiguousarray(np.concatenate(segs)),
            np.stack([np.frombuffer(s, np.uint8) for s in sets]), np.stack(qts))


def mcu_blocks(H, W):
    """int (MCUs, 6): the blocks of the hand-over that every MCU of the frame holds, MCU raster order"""
    mx, my, ny, nc, _ = jpeg_ref.geom(H, W)
    y, x = np.divmod(np.arange(nc), mx)
    lum = [(2 * y + (k >> 1)) * 2 * mx + 2 * x + (k & 1) for k in range(4)]
    return np.stack(lum + [ny + y * mx + x, ny + nc + y * mx + x], 1)


def segment_blocks(H, W, ri, s):
    """the blocks that segment ``s`` of a frame with restart interval ``ri`` holds"""
    mb = mcu_blocks(H, W)
    return mb[s * ri:(s + 1) * ri].reshape(-1) if ri else mb.reshape(-1)


def stuffed(bits):
    """a bit string, padded with ones to whole bytes, as entropy-coded bytes"""
    bits = bits.ljust(-(-len(bits) // 8) * 8, "1")
    return int(bits, 2).to_bytes(len(bits) // 8, "big").replace(b"\xff", b"\xff\x00")


# with the Annex K tables: DC category 0 is 00 in the luminance table; sixteen ones are no luminance AC code; ZRL is 11111111001
NO_SUCH_CODE = stuffed("00" + "1" * 16 + "00")
RUN_PAST_63 = stuffed("00" + "11111111001" * 4)
