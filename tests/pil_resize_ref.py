"""Pillow's ``Image.resize(size, BILINEAR)`` on uint8 images restated in numpy: the reference of ``kvq_resize_pil``
(csrc/resize_pil.hip) and of its tap tables (``kvq_resize_pil_taps``, csrc/resize_pil.hpp).

A fixed-point, two-pass triangle filter.  Per axis ``n_in -> n_out``, in double: scale = n_in / n_out, fs = support = max(scale, 1);
output index i has center = (i + 0.5) scale, the window [xmin, xmax) with xmin = max(int(center - support + 0.5), 0) and
xmax = min(int(center + support + 0.5), n_in), the weights w_j = max(0, 1 - |(j + xmin - center + 0.5) / fs|) normalised by their
sum and turned into integers with 22 fractional bits, (int)(w 2^22 + 0.5) ((int)(w 2^22 - 0.5) for a negative w).  One pass is
clip8((sum_j px_j k_j + 2^21) >> 22).  The width pass runs first and its result is a uint8 image; the height pass runs on that
image.  An axis with n_in == n_out is skipped."""
import numpy as np

PRECISION_BITS = 22

# (H, W, oh, ow) of the geometries whose Pillow outputs tests/golden/pil_resize.npz holds (make_pil_resize_golden.py), and the
# one that is compared with a live Pillow only (its 1080p input regenerates from the seed, its output is small, but the fixture
# stays well below the size limit without it)
GOLDEN_GEOMS = [(45, 70, 16, 16), (37, 53, 32, 32), (20, 30, 32, 32), (224, 224, 224, 224), (540, 960, 224, 224), (64, 48, 16, 24),
                (33, 224, 224, 224), (224, 31, 224, 224), (7, 9, 5, 224)]
LIVE_ONLY_GEOMS = [(1080, 1920, 224, 224)]


def golden_key(geom):
    return "pil_%dx%d_to_%dx%d" % geom


def golden_input(geom):
    """the uint8 (H, W, 3) input of a geometry: PCG64 seeded by the geometry itself"""
    H, W, oh, ow = geom
    g = np.random.Generator(np.random.PCG64(1000003 * H + 1009 * W + 31 * oh + ow))
    return g.integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def taps(n_in: int, n_out: int):
    """(start int32 [n_out], size int32 [n_out], coefficients int32 [n_out, kmax], zero past size) of one axis"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    kmax = int(np.ceil(support)) * 2 + 1
    start, size = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32)
    coef = np.zeros((n_out, kmax), np.int32)
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        n = xmax - xmin
        w = [max(0.0, 1.0 - abs((j + xmin - center + 0.5) / fs)) for j in range(n)]
        total = 0.0
        for v in w:
            total += v
        w = [v / total for v in w] if total != 0.0 else w
        start[i], size[i] = xmin, n
        coef[i, :n] = [int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5) for v in w]
    return start, size, coef


def _pass(img, n_out, axis):
    """one pass along ``axis`` of a uint8 array -> uint8"""
    n_in = img.shape[axis]
    if n_in == n_out:
        return img
    start, size, coef = taps(n_in, n_out)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.uint8)
    for i in range(n_out):
        k = coef[i, :size[i]].astype(np.int64).reshape((-1,) + (1,) * (src.ndim - 1))
        acc = (src[start[i]:start[i] + size[i]] * k).sum(0) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """uint8 (..., H, W, C) -> uint8 (..., oh, ow, C): the width pass, then the height pass on its uint8 result"""
    assert img.dtype == np.uint8 and img.ndim >= 3
    return _pass(_pass(img, ow, img.ndim - 2), oh, img.ndim - 3)


def resize_planar_f32(frames: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """uint8 (T, H, W, 3) -> fp32 (T, 3, oh, ow) holding the resized bytes: what the kernel writes through the table 0..255"""
    return np.ascontiguousarray(resize(frames, oh, ow).transpose(0, 3, 1, 2)).astype(np.float32)
