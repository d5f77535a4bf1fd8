"""CPU: the pieces of the Pillow-exact frame resize that need no GPU — the numpy restatement (tests/pil_resize_ref.py) against
Pillow's recorded outputs (tests/golden/pil_resize.npz) and against a live Pillow, the tap tables of ``kvq_resize_pil_taps`` against
the restatement's, the transform's look-up table against ``pil_transform``, the ABI, the option checks, and the table builder under
the host sanitizers as a program of its own."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import kvq_amd  # noqa: F401
from kvq_amd import _abi, kernels

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pil_resize_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = [(1920, 224), (1080, 224), (960, 224), (30, 32), (9, 224), (224, 224), (53, 32)]


@pytest.mark.parametrize("geom", R.GOLDEN_GEOMS, ids=[R.golden_key(g) for g in R.GOLDEN_GEOMS])
def test_restatement_equals_the_recorded_pillow_outputs(golden, geom):
    ref = golden("pil_resize.npz")[R.golden_key(geom)]
    got = R.resize(R.golden_input(geom), geom[2], geom[3])
    assert got.dtype == np.uint8 and got.shape == ref.shape and np.array_equal(got, ref)


@pytest.mark.parametrize("geom", R.GOLDEN_GEOMS + R.LIVE_ONLY_GEOMS, ids=[R.golden_key(g) for g in R.GOLDEN_GEOMS + R.LIVE_ONLY_GEOMS])
def test_restatement_equals_a_live_pillow(geom):
    Image = pytest.importorskip("PIL.Image")
    x = R.golden_input(geom)
    ref = np.asarray(Image.fromarray(x).resize((geom[3], geom[2]), Image.BILINEAR), np.uint8)
    assert np.array_equal(R.resize(x, geom[2], geom[3]), ref)


@pytest.mark.parametrize("n_in,n_out", AXES)
def test_tap_tables_equal_the_restatement(n_in, n_out):
    start, size, coef = kernels.resize_pil_taps(n_in, n_out)
    rs, rn, rk = R.taps(n_in, n_out)
    assert coef.shape == rk.shape and coef.dtype == np.int32
    assert np.array_equal(start, rs) and np.array_equal(size, rn) and np.array_equal(coef, rk)
    assert (start >= 0).all() and (size >= 1).all() and (start + size <= n_in).all()


def test_an_axis_that_keeps_its_size_is_the_identity():
    """Pillow skips such an axis; its coefficients {2^22, 0} give every byte back, so the kernel needs no second form"""
    start, size, coef = kernels.resize_pil_taps(224, 224)
    assert np.array_equal(start, np.arange(224)) and (coef[:, 0] == 1 << 22).all() and not coef[:, 1:].any()
    px = np.arange(256, dtype=np.int64)
    assert np.array_equal((px * (1 << 22) + (1 << 21)) >> 22, px)


def test_lut_equals_pil_transform_for_every_byte():
    pytest.importorskip("PIL.Image")
    from kvq_amd.datasets.slowfast_clips import pil_transform
    lut = kernels.slowfast_lut()
    assert lut.dtype == torch.float32 and lut.shape == (256,)
    tr = pil_transform(4)
    for b in range(256):
        out = tr(np.full((4, 4, 3), b, np.uint8))                 # a constant image stays constant under the resize
        assert out.shape == (3, 4, 4) and bool((out.view(torch.int32) == lut[b].view(torch.int32)).all()), b
    assert torch.equal(kernels.identity_lut(), torch.arange(256).float())


def test_abi_declares_the_entries_and_keeps_its_version():
    header = open(os.path.join(ROOT, "include", "kvq_hip.h")).read()
    handle = _abi.lib()
    for name in ("kvq_resize_pil", "kvq_resize_pil_taps", "kvq_resize_pil_supported"):
        assert name + "(" in header and name in _abi.SYMBOLS and hasattr(handle, name)
    assert _abi.ABI_VERSION == 32 and handle.kvq_abi_version() == 32 and "#define KVQ_ABI_VERSION 32" in header


def test_entry_checks_on_the_host_before_any_launch():
    handle = _abi.lib()
    k = C.c_int32()
    assert handle.kvq_resize_pil_taps(0, 4, C.byref(k), None, None, None) == -2
    assert handle.kvq_resize_pil_taps(4, 4, None, None, None, None) == -1
    assert handle.kvq_resize_pil_taps(1920, 224, C.byref(k), None, None, None) == 0 and k.value == 19
    P, Q = 4096, 4098                                                # never dereferenced: every refusal below comes first
    ok = (P, _abi.SRC_U8, 2, 45, 70, 16, 16, P, P, P, P, P, P, P, P, 3 * 256, 256, None)
    assert handle.kvq_resize_pil(*((None,) + ok[1:])) == -1 and b"NULL" in handle.kvq_last_error()
    assert handle.kvq_resize_pil(*(ok[:1] + (_abi.SRC_F32,) + ok[2:])) == -3
    assert handle.kvq_resize_pil(*(ok[:2] + (0,) + ok[3:])) == -2                                   # no frame
    assert handle.kvq_resize_pil(*(ok[:14] + (Q,) + ok[15:])) == -2 and b"aligned" in handle.kvq_last_error()
    assert handle.kvq_resize_pil(*(ok[:15] + (256, 256) + ok[17:])) == -2 and b"strides" in handle.kvq_last_error()
    assert handle.kvq_resize_pil(*(ok[:15] + (256, 2 * 256 - 1) + ok[17:])) == -2                    # the second frame inside the first's planes
    assert handle.kvq_resize_pil(*(ok[:4] + (5500,) + ok[5:])) == -3 and b"stage" in handle.kvq_last_error()
    # what the launch would take, answered without one
    sup = handle.kvq_resize_pil_supported
    assert sup(_abi.SRC_U8, 1, 2160, 3840, 224, 224) == 1 and sup(_abi.SRC_I420_BT601_FULL, 64, 2160, 3840, 224, 224) == 1
    assert sup(_abi.SRC_U8, 64, 1080, 1920, 224, 224) == 1 and sup(_abi.SRC_U8, 1, 8, 5500, 4, 4) == 0
    assert sup(_abi.SRC_F32, 1, 8, 8, 4, 4) == 0 and sup(_abi.SRC_U8, 1, 8, 8, 4, 20000) == 0      # the width table alone exceeds the LDS


def test_wrapper_refuses_host_tensors_and_other_layouts():
    lut = kernels.identity_lut()
    with pytest.raises(ValueError, match="uint8"):
        kernels.resize_pil(torch.zeros(3, 2, 8, 8, dtype=torch.uint8), 4, 4, lut)                  # planar (C, T, H, W)
    with pytest.raises(_abi.KvqError, match="HIP device"):
        kernels.resize_pil(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), 4, 4, lut)


def test_unknown_motion_feature_source_is_refused_at_construction(tmp_path):
    from kvq_amd.datasets import ViewDecompositionDataset_add_forSimpleVQA
    (tmp_path / "v.csv").write_text("filename,score\na.mp4,1\n")
    st = {"simpleVQA": dict(resize=130, crop=112, clip_len=8, frame_interval=10, t_frag=8, num_clips=1)}
    base = dict(anno_file=str(tmp_path / "v.csv"), data_prefix=str(tmp_path), feature_type="SlowFast", phase="test", sample_types=st)
    with pytest.raises(ValueError, match="motion_features.source"):
        ViewDecompositionDataset_add_forSimpleVQA(dict(base, motion_features={"source": "disk"}), device="cpu")
    with pytest.raises(ValueError, match="motion_features"):
        ViewDecompositionDataset_add_forSimpleVQA(dict(base, motion_features={"source": "inline", "size": 224}), device="cpu")
    with pytest.raises(KeyError):                                   # files (the default) needs data_prefix_3D, as before
        ViewDecompositionDataset_add_forSimpleVQA(dict(base), device="cpu")
    with pytest.raises(KeyError):
        ViewDecompositionDataset_add_forSimpleVQA(dict(base, motion_features={"source": "files"}), device="cpu")
    ds = ViewDecompositionDataset_add_forSimpleVQA(dict(base, motion_features={"source": "inline", "resize": 64}), device="cpu")
    assert ds.data_prefix_3D is None and ds.motion["resize"] == 64 and ds.motion["weights"] is None and len(ds) == 1


def test_inline_yml_parses_and_names_the_key():
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "kwai_simpleVQA_inline_test.yml")))
    args = cfg["data"]["val"]["args"]
    assert args["motion_features"]["source"] == "inline" and "data_prefix_3D" not in args and cfg["model"]["type"] == "simpleVQA"


def test_cli_refuses_an_unknown_transform():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "SlowFast_features.py"), "--transform", "gpu", "--synthetic", "1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--transform" in r.stderr and "invalid choice" in r.stderr


def _sanitizer_compiler():
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        return None, "no host C++ compiler"
    probe = subprocess.run([cxx, "-x", "c++", "-", "-fsanitize=address,undefined", "-o", os.devnull], input="int main() { return 0; }",
                           capture_output=True, text=True)
    return (cxx, "") if probe.returncode == 0 else (None, f"{cxx} has no address / undefined-behaviour sanitizer runtimes")


def test_hostcheck_under_the_sanitizers(tmp_path):
    """tools/resize_pil_hostcheck.cpp: a program of its own, the host compiler alone, -fsanitize=address,undefined, over the axes above"""
    cxx, why = _sanitizer_compiler()
    if cxx is None:
        pytest.skip(why)
    exe = str(tmp_path / "resize_pil_hostcheck")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                        os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "resize_pil_hostcheck.cpp"),
                        os.path.join(os.path.dirname(kvq_amd.__file__), "csrc", "resize_pil.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "resize_pil_hostcheck: all clean" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    for n_in, n_out in AXES:
        assert f"{n_in:5d} -> {n_out:5d}" in r.stdout, (n_in, n_out)
