"""Writes tests/golden/pil_resize.npz: Pillow's ``Image.resize((ow, oh), BILINEAR)`` outputs for the geometries of
tests/pil_resize_ref.py (``GOLDEN_GEOMS``).  Outputs only: every input regenerates from its PCG64 seed (``golden_input``).

    python tests/golden/make_pil_resize_golden.py        (needs Pillow; the fixture records its version)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pil_resize_ref as R  # noqa: E402


def main():
    import PIL
    from PIL import Image
    out = {"pillow_version": np.array(PIL.__version__)}
    for geom in R.GOLDEN_GEOMS:
        H, W, oh, ow = geom
        out[R.golden_key(geom)] = np.asarray(Image.fromarray(R.golden_input(geom)).resize((ow, oh), Image.BILINEAR), np.uint8)
    path = os.path.join(HERE, "pil_resize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
