"""Writes tests/golden/mjpeg.npz: the JPEG streams the Motion-JPEG tests decode, produced by Pillow (libjpeg-turbo) with exactly the
options below, and libjpeg's own Y plane of each (``Image.draft("YCbCr", size)``, channel 0: the luminance samples before any colour
conversion or chroma upsampling).  The tests need no Pillow; this script does.  It also runs the restatement (tests/jpeg_ref.py) over
every case and asserts that its Y plane is within +-1 of libjpeg's on every sample — the accuracy ITU-T T.83 allows an IDCT — and that
decoding a case twice gives the same coefficients; it prints the largest difference and the share of samples that differ.

    python tests/golden/make_mjpeg_golden.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_ref  # noqa: E402


def picture(H, W, seed):
    """gradient + noise, deterministic"""
    g = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([255.0 * x / max(W - 1, 1), 255.0 * y / max(H - 1, 1), 255.0 * (x + y) / max(H + W - 2, 1)], axis=-1)
    return np.clip(base + g.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)


def noise(H, W, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (H, W, 3), dtype=np.uint8)


def jpeg(arr, mode="RGB", **opts):
    b = io.BytesIO()
    Image.fromarray(arr).convert(mode).save(b, "JPEG", **opts)
    return b.getvalue()


def libjpeg_y(data):
    im = Image.open(io.BytesIO(data))
    im.draft("YCbCr", im.size)
    assert im.mode == "YCbCr", im.mode
    return np.asarray(im)[..., 0].copy()


def cut_dht(data):
    """the stream without its DHT segments: what AVI 'MJPG' frames of hardware encoders look like"""
    out, pos = bytearray(data[:2]), 2
    while True:
        assert data[pos] == 0xFF
        m, n = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        if m == 0xDA:
            return bytes(out + data[pos:])
        if m != 0xC4:
            out += data[pos:pos + 2 + n]
        pos += 2 + n


def main():
    decodable = {
        "one_mcu": jpeg(picture(16, 16, 1), quality=90, subsampling=2),
        "odd": jpeg(picture(45, 70, 2), quality=90, subsampling=2),
        "odd_optimize": jpeg(picture(45, 70, 2), quality=50, optimize=True, subsampling=2),
        "odd_restart": jpeg(picture(45, 70, 2), quality=95, restart_marker_blocks=2, subsampling=2),
        "sub_mcu": jpeg(picture(7, 9, 3), quality=90, subsampling=2),
        "noise_q100": jpeg(noise(24, 40, 4), quality=100, subsampling=2),
        "noise_q5": jpeg(noise(24, 40, 4), quality=5, subsampling=2),
        "video_0": jpeg(picture(48, 64, 5), quality=30, subsampling=2),
        "video_1": jpeg(picture(48, 64, 6), quality=75, subsampling=2),
        "video_2": jpeg(picture(48, 64, 7), quality=95, subsampling=2),
    }
    decodable["odd_no_dht"] = cut_dht(decodable["odd"])
    refused = {
        "progressive": jpeg(picture(45, 70, 2), quality=90, progressive=True, subsampling=2),
        "s422": jpeg(picture(45, 70, 2), quality=90, subsampling=1),
        "s444": jpeg(picture(45, 70, 2), quality=90, subsampling=0),
        "gray": jpeg(picture(45, 70, 2)[..., 0], mode="L", quality=90),
        "cmyk": jpeg(picture(45, 70, 2), mode="CMYK", quality=90),
    }
    out = {"decodable": np.array(sorted(decodable)), "refused": np.array(sorted(refused))}
    worst, differ, total = 0, 0, 0
    for name, data in decodable.items():
        want = libjpeg_y(data if name != "odd_no_dht" else decodable["odd"])      # the same picture: only the tables' transport differs
        coef, qt, p = jpeg_ref.decode_coeffs(data)
        coef2, qt2, _ = jpeg_ref.decode_coeffs(data)
        assert np.array_equal(coef, coef2) and np.array_equal(qt, qt2), name
        assert (p["H"], p["W"]) == want.shape and p["frame_bytes"] == len(data), name
        got = jpeg_ref.planes(jpeg_ref.idct_i420(coef, qt, p["H"], p["W"]), p["H"], p["W"])[0]
        d = np.abs(got.astype(np.int16) - want.astype(np.int16))
        assert int(d.max()) <= 1, (name, int(d.max()))
        worst, differ, total = max(worst, int(d.max())), differ + int(np.count_nonzero(d)), total + d.size
        out[name + "_jpg"], out[name + "_y"] = np.frombuffer(data, np.uint8), want
    for name, data in refused.items():
        assert not jpeg_ref.supported(jpeg_ref.parse(data)), name
        out[name + "_jpg"] = np.frombuffer(data, np.uint8)
    path = os.path.join(HERE, "mjpeg.npz")
    np.savez_compressed(path, **out)
    print(f"restatement vs libjpeg Y: largest difference {worst}, {differ} of {total} samples differ ({differ / total:.2e})")
    print(f"{path}: {os.path.getsize(path)} bytes, Pillow {Image.__version__}")


if __name__ == "__main__":
    main()
