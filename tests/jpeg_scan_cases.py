"""The inputs of the entropy-CODER tests (tests/test_mjpeg_write_entropy_cpu.py, tests/test_gpu_mjpeg_write_entropy.py), shared so that
the host twin and the launch see the same cases, and what they must equal: ``kvq_jpeg_encode`` — pinned to libjpeg by
tests/test_mjpeg_write_cpu.py — and, independently, the restatement ``jpeg_enc_ref.encode``; never the code under test.

A case is ``Case(name, H, W, ri, qt, coef, rgb, ok)``: coef int16 (T, blocks * 64) on the host — from the scalar twin of the forward DCT
when the case has pixels (``rgb`` uint8 (3, T, H, W), else None), written directly when it is crafted —, ``ok`` (T,) bool: the frame is
inside baseline's range.  All random inputs are PCG64(0) uniform noise."""
import functools
from collections import namedtuple

import numpy as np

from kvq_amd import kernels

import jpeg_enc_ref
import jpeg_ref

Case = namedtuple("Case", "name H W ri qt coef rgb ok")
FIXTURES = ["noise_32x48_q5", "noise_32x48_q50", "noise_32x48_q100", "picture_48x64_q30", "picture_48x64_q95", "noise_16x16_q75", "noise_64x80_q85",
            "picture_45x70_q90", "picture_7x9_q90", "picture_33x17_q75", "noise_24x40_q100"]
ZZ = jpeg_ref.ZIGZAG
# the position scan of the launch walks a frame in chunks of this many blocks (csrc/jpeg_enc_entropy.hip, JES_SCAN_LANES)
SCAN_CHUNK = 1024
SOS = bytes([0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])      # the scan header: the scan follows it, FF D9 ends the image


def _noise(T, H, W):
    return np.random.Generator(np.random.PCG64(0)).integers(0, 256, (3, T, H, W), dtype=np.uint8)


def _pixels(name, rgb, quality, ri):
    _, T, H, W = rgb.shape
    qt = kernels.jpeg_quant_tables(quality)
    return Case(name, H, W, ri, qt, kernels.jpeg_fdct_host(rgb, qt, H, W), rgb, np.ones(T, bool))


def _crafted(name, H, W, ri, blocks, ok=None):
    """blocks: (T, blocks, 64) in SCAN order (MCU raster, Y00 Y01 Y10 Y11 Cb Cr), zig-zag order inside a block -> hand-over layout"""
    blocks = np.asarray(blocks, np.int16)
    T = blocks.shape[0]
    mx, my, ny, nc, nb = jpeg_ref.geom(H, W)
    assert blocks.shape == (T, nb, 64)
    coef = np.zeros((T, nb, 64), np.int16)
    for s in range(nb):
        mcu, k = divmod(s, 6)
        y, x = divmod(mcu, mx)
        bi = (2 * y + (k >> 1)) * 2 * mx + 2 * x + (k & 1) if k < 4 else ny + (k - 4) * nc + mcu
        coef[:, bi, ZZ] = blocks[:, s]
    return Case(name, H, W, ri, kernels.jpeg_quant_tables(50), coef.reshape(T, -1), None, np.ones(T, bool) if ok is None else np.asarray(ok, bool))


def pixel_cases(golden):
    grey = np.full((3, 1, 48, 64), 128, np.uint8)
    out = [_pixels("noise 16x16 q75 ri0", _noise(1, 16, 16), 75, 0),
           _pixels("grey 48x64 q50 ri0", grey, 50, 0),
           _pixels("grey 48x64 q50 ri1", grey, 50, 1),
           _pixels("noise 48x48 q100 ri1", _noise(1, 48, 48), 100, 1),
           _pixels("noise 45x70 q100 ri5 (row)", _noise(1, 45, 70), 100, 5),
           _pixels("noise 64x80 q100 ri0", _noise(1, 64, 80), 100, 0),
           _pixels("noise 64x80 q100 ri5 (row)", _noise(1, 64, 80), 100, 5),
           _pixels("noise 48x64 q75 ri4 (row)", _noise(1, 48, 64), 75, 4),
           _pixels("noise 45x70 q75 ri100 > MCUs", _noise(1, 45, 70), 75, 100),
           _pixels("noise 16x16 q75 ri7 > MCUs", _noise(1, 16, 16), 75, 7),
           _pixels("noise 45x70 q75 ri65535", _noise(1, 45, 70), 75, 65535)]
    g = golden("mjpeg_enc.npz")
    for name in FIXTURES:
        rgb = np.ascontiguousarray(g[name + "_rgb"].transpose(2, 0, 1)[:, None])
        out.append(_pixels("fixture " + name, rgb, int(g[name + "_q"]), 0))
    big = _noise(3, 272, 480)                                  # 510 MCUs = 3060 blocks per frame: a segment spans three chunks of the scan
    assert big.shape[1] == 3 and not np.array_equal(big[:, 0], big[:, 1]) and 3060 > 2 * SCAN_CHUNK
    out += [_pixels(f"noise 272x480 q75 T3 ri{ri}", big, 75, ri) for ri in (0, 7, 30)]
    return out


def crafted_cases():
    H, W = 16, 32                                              # two MCUs, twelve blocks
    out = []
    full = np.zeros((1, 12, 64), np.int16)
    full[0, :, 1:] = np.where(np.arange(63) % 2 == 0, 1023, -1023)
    full[0, :, 0] = [2047, 0, 2047, 0, 2047, -2047, 2047, 0, 2047, 0, 0, 0]      # every DC difference has category 11
    out.append(_crafted("every block 1660 bits", H, W, 0, full))
    last = np.zeros((1, 12, 64), np.int16)
    last[0, :, 63] = [1, -1, 5, -300, 1023, -1023] * 2
    out.append(_crafted("only position 63: three ZRL, no EOB", H, W, 0, last))
    runs = np.zeros((1, 12, 64), np.int16)
    runs[0, :, 1], runs[0, :, 17], runs[0, :, 34] = 3, -2, 7   # 15 zeros, then 16 zeros
    out.append(_crafted("zero runs of 15 and 16", H, W, 1, runs))
    dc = np.zeros((1, 12, 64), np.int16)
    dc[0, :, 0] = [5, -5, 100, 0, -1, 1, 1000, -1000, 0, 0, 3, -3]
    out.append(_crafted("DC only", H, W, 0, dc))
    edge = np.zeros((1, 12, 64), np.int16)
    edge[0, :, 0] = [-1023, 1023, -1023, 1023, -1023, 1023, 1023, -1023, 1023, -1023, 1023, -1023]
    out.append(_crafted("DC differences of 2046", H, W, 0, edge))
    over = edge.copy()
    over[0, :4, 0] = [-1024, 1024, -1024, 1024]
    out.append(_crafted("DC difference of 2048", H, W, 0, over, ok=[False]))
    three = np.concatenate([runs, dc, full])
    three[1, 7, 20] = 1024
    out.append(_crafted("AC 1024 in the middle frame of three", H, W, 0, three, ok=[True, False, True]))
    return out


@functools.lru_cache(maxsize=None)
def _restated(coef_bytes, qt_bytes, H, W, ri, dht):
    return jpeg_enc_ref.encode(np.frombuffer(coef_bytes, np.int16).reshape(-1, 64), np.frombuffer(qt_bytes, np.uint16).reshape(3, 64), H, W, ri, dht)


def expected_images(case, dht=True):
    """per frame the bytes of the whole image, or None for a frame outside baseline's range (which the host coder must refuse); the host
    coder's and the restatement's bytes are asserted equal here"""
    out = []
    for t in range(case.coef.shape[0]):
        if not case.ok[t]:
            with np.testing.assert_raises(Exception):
                kernels.jpeg_encode(case.coef[t], case.qt, case.H, case.W, case.ri, dht)
            out.append(None)
            continue
        image = kernels.jpeg_encode(case.coef[t], case.qt, case.H, case.W, case.ri, dht).tobytes()
        assert image == _restated(case.coef[t].tobytes(), case.qt.tobytes(), case.H, case.W, case.ri, dht), (case.name, t)
        out.append(image)
    return out


def expected_scans(case):
    """(the scans packed back to back, frames uint32 (T, 3)) that the code under test must produce with room for everything"""
    body, table = b"", []
    for image in expected_images(case):
        scan = b"" if image is None else image[image.index(SOS) + len(SOS):-2]
        table.append((len(body), len(scan), 1 if image is None else 0))
        body += scan
    return body, np.array(table, np.uint32)
