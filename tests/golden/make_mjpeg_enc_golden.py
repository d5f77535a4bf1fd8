"""Writes tests/golden/mjpeg_enc.npz: RGB pictures, a quality, and the JPEG image Pillow (libjpeg-turbo) makes of them with
``subsampling=2`` and no ``optimize`` — the yardstick of the Motion-JPEG writer's block analysis.  The tests need no Pillow; this
script does.  It runs the restatement (tests/jpeg_enc_ref.py) over every case and asserts what the tests assert of the library:
  aligned cases (H and W multiples of 16): every quantised coefficient and both quantiser tables equal libjpeg's;
  unaligned cases: every Y block that holds a sample and every chroma block wholly inside its plane equal libjpeg's (the rest is
  padding, which libjpeg fills by another rule).
It prints the counts, and whether the restatement's whole image, entropy-coded segment included, equals Pillow's from SOS on.

    python tests/golden/make_mjpeg_enc_golden.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_enc_ref  # noqa: E402
import jpeg_ref  # noqa: E402
from make_mjpeg_golden import noise, picture  # noqa: E402

ALIGNED = [("noise", 32, 48, 5), ("noise", 32, 48, 50), ("noise", 32, 48, 100), ("picture", 48, 64, 30), ("picture", 48, 64, 95),
           ("noise", 16, 16, 75), ("noise", 64, 80, 85)]
UNALIGNED = [("picture", 45, 70, 90), ("picture", 7, 9, 90), ("picture", 33, 17, 75), ("noise", 24, 40, 100)]


def main():
    out = {"aligned": [], "unaligned": []}
    for group, cases in (("aligned", ALIGNED), ("unaligned", UNALIGNED)):
        for i, (kind, H, W, q) in enumerate(cases):
            name = f"{kind}_{H}x{W}_q{q}"
            rgb = (noise if kind == "noise" else picture)(H, W, (100 if group == "aligned" else 200) + i)
            b = io.BytesIO()
            Image.fromarray(rgb).save(b, "JPEG", quality=q, subsampling=2)
            data = b.getvalue()
            want, qt, p = jpeg_ref.decode_coeffs(data)
            assert (p["H"], p["W"]) == (H, W)
            assert np.array_equal(qt, jpeg_enc_ref.quant_tables(q)), name
            got = jpeg_enc_ref.fdct(rgb.transpose(2, 0, 1)[:, None], jpeg_enc_ref.SRC_U8, 1, H, W, qt[None])[0].reshape(-1, 64)
            mask = jpeg_enc_ref.picture_blocks(H, W)
            assert group != "aligned" or mask.all()
            bad = int(np.count_nonzero(got[mask] != want[mask]))
            print(f"{name:24s} {int(mask.sum()):3d} of {mask.size:3d} blocks compared, {bad} of {int(mask.sum()) * 64} coefficients differ", end="")
            assert bad == 0, name
            if group == "aligned":
                ours = jpeg_enc_ref.encode(got, qt, H, W)
                print(f"; scan {'equal to' if ours[ours.index(bytes([0xFF, 0xDA])):] == data[data.index(bytes([0xFF, 0xDA])):] else 'differs from'} Pillow's"
                      f" ({len(ours)} bytes against {len(data)})", end="")
            print()
            out[group].append(name)
            out[name + "_rgb"], out[name + "_q"], out[name + "_jpg"] = rgb, np.int32(q), np.frombuffer(data, np.uint8)
    out["aligned"], out["unaligned"] = np.array(out["aligned"]), np.array(out["unaligned"])
    path = os.path.join(HERE, "mjpeg_enc.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, Pillow {Image.__version__}")


if __name__ == "__main__":
    main()
