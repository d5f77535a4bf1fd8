"""CPU: the antialiased resize's tap tables (kvq_resize_aa_taps: the fp32 code the kernel runs, evaluated on the host) against
ATen's F.interpolate(mode="bilinear", align_corners=False, antialias=True), and the ``antialias`` plumbing of the dataset views."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kvq_amd  # noqa: F401
from kvq_amd import _abi, kernels
from kvq_amd.datasets import fusion_datasets as fd

# (in, out): downscales (KSVQE key frames, non-integer ratios), the unchanged axis, upscales (SimpleVQA's 520 of a 360 source)
AXES = [(1080, 112), (1920, 112), (540, 224), (960, 224), (333, 112), (517, 97), (640, 520), (100, 100), (360, 520), (7, 16),
        (1, 3), (5, 1)]


def _formula64(n_in, n_out):
    """The window / weight formula in float64 (the issue's statement of ATen's antialiased bilinear)."""
    scale = n_in / n_out
    support = max(scale, 1.0)
    rows = []
    for i in range(n_out):
        center = scale * (i + 0.5)
        xmin = max(int(center - support + 0.5), 0)
        xsize = min(int(center + support + 0.5), n_in) - xmin
        w = np.array([max(0.0, 1.0 - abs((j + xmin - center + 0.5) / support)) for j in range(xsize)])
        rows.append((xmin, xsize, w / w.sum()))
    return rows


def _dense(start, size, w, n_in):
    m = np.zeros((len(start), n_in))
    for i, (s, n) in enumerate(zip(start, size)):
        m[i, s:s + n] = w[i, :n]
    return m


def _aten_matrix(n_in, n_out, dtype=torch.float64):
    """The (out, in) matrix ATen applies along one axis: F.interpolate of the identity's rows (in float32: its fp32 weights exactly)."""
    eye = torch.eye(n_in, dtype=dtype).reshape(n_in, 1, 1, n_in)
    return F.interpolate(eye, size=(1, n_out), mode="bilinear", align_corners=False, antialias=True).reshape(n_in, n_out).T.numpy()


@pytest.mark.parametrize("n_in,n_out", AXES)
def test_taps_equal_aten(n_in, n_out):
    start, size, w = kernels.resize_aa_taps(n_in, n_out)
    assert w.shape[0] == n_out and w.shape[1] >= size.max()
    assert (start >= 0).all() and (size >= 1).all() and (start + size <= n_in).all()
    assert np.abs(w.sum(1) - 1).max() <= 1e-6
    # the dense matrix the kernel applies is ATen's fp32 one (bit-equal but for an odd last-place difference), and its float64 one
    # to fp32 rounding: the rounding of center = scale*(i+0.5) moves the upscaled taps' fractions by up to 4e-5
    m = _dense(start, size, w, n_in)
    assert np.abs(m - _aten_matrix(n_in, n_out, torch.float32)).max() <= 1e-7
    assert np.abs(m - _aten_matrix(n_in, n_out)).max() <= 5e-5
    # windows equal the float64 statement of the formula, except where fp32 moves a window end onto a zero-weight tap
    for i, (s64, n64, w64) in enumerate(_formula64(n_in, n_out)):
        if (start[i], size[i]) != (s64, n64):
            lo, hi = min(start[i], s64), max(start[i] + size[i], s64 + n64)
            a = np.zeros(hi - lo); a[start[i] - lo:start[i] - lo + size[i]] = w[i, :size[i]]
            b = np.zeros(hi - lo); b[s64 - lo:s64 - lo + n64] = w64
            assert np.abs(a - b).max() <= 5e-5, (i, start[i], size[i], s64, n64)
        else:
            assert np.abs(w[i, :size[i]] - w64).max() <= 5e-5 and not w[i, size[i]:].any()


def test_formula_is_aten_in_float64():
    """The formula the kernel restates is ATen's, to float64 rounding (downscale, non-integer, unchanged, upscale)."""
    for n_in, n_out in AXES:
        rows = _formula64(n_in, n_out)
        m = _dense([r[0] for r in rows], [r[1] for r in rows], np.stack([np.pad(r[2], (0, 64 - r[1])) for r in rows]), n_in)
        assert np.abs(m - _aten_matrix(n_in, n_out)).max() <= 1e-12, (n_in, n_out)


def test_upscale_taps_are_plain_bilinear():
    """On an upscaled axis the antialiased weights are the plain bilinear ones (antialias=False)."""
    start, size, w = kernels.resize_aa_taps(360, 520)
    eye = torch.eye(360, dtype=torch.float64).reshape(360, 1, 1, 360)
    plain = F.interpolate(eye, size=(1, 520), mode="bilinear", align_corners=False).reshape(360, 520).T.numpy()
    assert np.abs(_dense(start, size, w, 360) - plain).max() <= 5e-5


@pytest.mark.parametrize("shape,size", [((2, 2, 60, 90), (13, 17)), ((3, 1, 36, 64), (52, 52)), ((1, 1, 40, 30), (40, 12))])
def test_separable_taps_reproduce_interpolate(shape, size):
    """Width then height with the product's tables == F.interpolate(antialias=True) on CPU tensors (mixed axes included)."""
    g = np.random.Generator(np.random.PCG64(7))
    x = g.integers(0, 256, size=shape).astype(np.float32)
    mh = _dense(*kernels.resize_aa_taps(shape[2], size[0]), shape[2])
    mw = _dense(*kernels.resize_aa_taps(shape[3], size[1]), shape[3])
    got = np.einsum("oh,cthw,pw->ctop", mh, x.astype(np.float64), mw)
    ref = F.interpolate(torch.from_numpy(x), size=size, mode="bilinear", align_corners=False, antialias=True).numpy()
    assert np.abs(got - ref).max() <= 2e-3        # ATen's fp32 sums against float64 sums of the same fp32 taps


def test_taps_argument_checks():
    handle = _abi.lib()
    import ctypes as C
    k = C.c_int32()
    assert handle.kvq_resize_aa_taps(0, 4, C.byref(k), None, None, None) == -2
    assert handle.kvq_resize_aa_taps(4, 4, None, None, None, None) == -1
    assert handle.kvq_resize_aa_taps(1920, 112, C.byref(k), None, None, None) == 0 and k.value >= 36
    # the launch entry validates before touching a pointer: NULL and a crop outside the frame are refused without a GPU
    assert handle.kvq_resize_bilinear_aa(None, 1, 3, 1, 8, 8, 4, 4, 0, 0, 4, 4, 1, None, None, None, None) == -1
    assert handle.kvq_resize_bilinear_aa(1, 1, 3, 1, 8, 8, 4, 4, 1, 0, 4, 4, 1, None, None, 1, None) == -2


class _Spy:
    def __init__(self):
        self.calls = []

    def __call__(self, video, rh, rw, **kw):
        self.calls.append((rh, rw, kw))
        return video


@pytest.mark.parametrize("antialias", [False, True])
def test_views_pass_antialias(monkeypatch, antialias):
    spy = _Spy()
    monkeypatch.setattr(fd.kernels, "resize_bilinear", spy)
    v = torch.zeros(3, 2, 8, 8, dtype=torch.uint8)
    fd.get_single_view(v, "aesthetic", size_h=4, size_w=6, antialias=antialias)
    fd.get_single_view(v, "simpleVQA", resize=6, crop=4, antialias=antialias)
    fd.get_resized_video(v, 4, 4, antialias=antialias)
    fd.get_resizecrop_video(v, 6, 4, antialias=antialias)
    assert [c[2]["antialias"] for c in spy.calls] == [antialias] * 4
    assert spy.calls[0][:2] == (4, 6) and spy.calls[1][2]["crop"] == (1, 1, 4, 4)


def test_views_default_is_plain_bilinear(monkeypatch):
    spy = _Spy()
    monkeypatch.setattr(fd.kernels, "resize_bilinear", spy)
    v = torch.zeros(3, 2, 8, 8, dtype=torch.uint8)
    fd.get_single_view(v, "aesthetic", size_h=4, size_w=4)
    fd.get_single_view(v, "simpleVQA", resize=6, crop=4, phase="test")
    assert [c[2]["antialias"] for c in spy.calls] == [False, False]
