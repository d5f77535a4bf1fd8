"""GPU: kvq_jpeg_fdct against its host twin, to the bit, from both source kinds; the same launches inside guard bands; the round trip
frames -> jpeg_fdct -> jpeg_encode -> a container -> MjpegFrameReader -> jpeg_idct_i420 against the host twins; the harness with the yml
key quality_maps.overlay_video against the overlays it puts into the .npz without it.  Nothing here depends on a number measured on
the GPU."""
import os

import numpy as np
import pytest
import torch

import kvq_amd  # noqa: F401
from kvq_amd import _abi, kernels
from kvq_amd.datasets import fusion_datasets as fd

import jpeg_ref
from guarded import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(16, 16), (7, 9), (45, 70), (33, 17), (48, 64)]
T = 3


def _case(H, W, source, extra=0):
    """(host source, format, tables (T, 3, 64)): random frames, the first all 0 and the last all 255 in its top-left quarter; per-frame
    tables.  ``extra`` frames in front and behind for the I420 view."""
    g = np.random.Generator(np.random.PCG64(H * 977 + W + (source == "rgb")))
    qt = np.stack([kernels.jpeg_quant_tables(q) for q in (35, 90, 100)])
    qt[1] = g.integers(1, 256, (3, 64))
    if source == "rgb":
        src = g.integers(0, 256, (3, T, H, W), dtype=np.uint8)
        src[:, 0] = 0
        src[:, 2, :H // 2 + 1, :W // 2 + 1] = 255
        return src, _abi.SRC_U8, qt
    src = g.integers(0, 256, (T + 2 * extra, jpeg_ref.frame_bytes(H, W)), dtype=np.uint8)
    src[extra] = 0
    src[extra + 2, :H * W // 2] = 255
    return src, _abi.SRC_I420_BT601_FULL, qt


def _dev_qt(qt):
    return torch.from_numpy(np.ascontiguousarray(qt).view(np.int16)).to(DEV).view(torch.uint16)


@pytest.fixture(scope="module")
def twin():
    """(H, W, source) -> (host source, format, tables, the host twin's coefficients), computed once"""
    out = {}
    for H, W in SIZES:
        for source in ("rgb", "i420"):
            src, fmt, qt = _case(H, W, source, extra=1)
            frames = src if source == "rgb" else src[1:T + 1]
            out[(H, W, source)] = (src, fmt, qt, kernels.jpeg_fdct_host(frames, qt, H, W, fmt))
    return out


def _frames_on_device(src, fmt, H, W):
    if fmt == _abi.SRC_U8:
        return torch.from_numpy(src).to(DEV)
    whole = kernels.I420Frames(torch.from_numpy(src).to(DEV), H, W, fmt)
    return whole.frames(1, T + 1)                                     # a run of frames of a longer video: still one pointer, any alignment


@pytest.mark.parametrize("source", ["rgb", "i420"])
@pytest.mark.parametrize("H,W", SIZES)
def test_kernel_equals_the_host_twin(twin, H, W, source):
    src, fmt, qt, want = twin[(H, W, source)]
    got = kernels.jpeg_fdct(_frames_on_device(src, fmt, H, W), _dev_qt(qt))
    assert got.dtype == torch.int16 and tuple(got.shape) == want.shape == (T, kernels.jpeg_coef_bytes(H, W) // 2)
    assert np.array_equal(got.cpu().numpy(), want), int(np.count_nonzero(got.cpu().numpy() != want))


def test_one_table_serves_every_frame_and_the_output_feeds_the_idct(twin):
    H, W = 45, 70
    src, fmt, _, _ = twin[(H, W, "rgb")]
    qt = kernels.jpeg_quant_tables(75)
    coef = kernels.jpeg_fdct(torch.from_numpy(src).to(DEV), _dev_qt(qt))
    want = kernels.jpeg_fdct_host(src, qt, H, W)
    assert np.array_equal(coef.cpu().numpy(), want)
    back = kernels.jpeg_idct_i420(coef, _dev_qt(np.broadcast_to(qt, (T, 3, 64))), H, W)
    assert np.array_equal(back.data.cpu().numpy(), kernels.jpeg_idct_i420_host(want, np.broadcast_to(qt, (T, 3, 64)), H, W))


@pytest.mark.parametrize("source", ["rgb", "i420"])
@pytest.mark.parametrize("H,W", SIZES)
def test_launch_inside_guard_bands(twin, H, W, source):
    """nothing is written in front of or behind coef_out, the bands around the inputs are intact, and every coefficient is written:
    the result does not follow the payload the output was allocated with"""
    src, fmt, qt, want = twin[(H, W, source)]
    for payload in (0xFF, 0x00):
        with guarded("cuda", payload=payload) as G:
            if fmt == _abi.SRC_U8:
                frames = G.wrap(torch.from_numpy(src).to(DEV), name="frames")
            else:
                frames = kernels.I420Frames(G.wrap(torch.from_numpy(src[1:T + 1]).to(DEV), name="frames"), H, W, fmt)
            tables = G.wrap(_dev_qt(qt).view(torch.int16), name="qt").view(torch.uint16)
            got = kernels.jpeg_fdct(frames, tables)                   # the wrapper's torch.empty is guarded too
            report = G.intact()
        assert report, repr(report)
        assert np.array_equal(got.cpu().numpy(), want), payload


def test_launch_refusals():
    lib = _abi.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    assert p % 16 == 0
    for fmt in (_abi.SRC_F32, _abi.SRC_I420_BT601_LIMITED, _abi.SRC_I420_BT709_LIMITED, _abi.SRC_I420_BT709_FULL):
        assert lib.kvq_jpeg_fdct(p, fmt, 1, 16, 16, p + 1024, p + 2048, None) == -3 and f"format {fmt}" in lib.kvq_last_error().decode()
    assert lib.kvq_jpeg_fdct(p, _abi.SRC_U8, 1, 16, 16, p + 1024 + 2, p + 2048, None) == -2
    assert lib.kvq_jpeg_fdct(p, _abi.SRC_U8, 1, 16, 16, p + 1024, p + 2048 + 8, None) == -2
    assert lib.kvq_jpeg_fdct(p, _abi.SRC_U8, 0, 16, 16, p + 1024, p + 2048, None) == -2
    with pytest.raises(ValueError, match=r"to_rgb\(\)"):
        kernels.jpeg_fdct(kernels.I420Frames(buf[:384].view(1, 384), 16, 16, _abi.SRC_I420_BT709_FULL), _dev_qt(kernels.jpeg_quant_tables(50)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("container", [".mjpeg", ".avi", "_dir"])
@pytest.mark.parametrize("source", ["rgb", "i420"])
def test_round_trip_on_the_device(tmp_path, twin, container, source):
    H, W = 45, 70
    src, fmt, _, _ = twin[(H, W, source)]
    path = str(tmp_path / ("clip" + container))
    with fd.MjpegWriter(path, 30000 / 1001, quality=85, restart_interval=3 if container == ".avi" else 0) as w:
        w.write(_frames_on_device(src, fmt, H, W))
    vr = fd.open_video(path)
    assert isinstance(vr, fd.MjpegFrameReader) and (len(vr), vr.H, vr.W) == (T, H, W)
    got = fd._frames_to_device(vr, np.arange(T), DEV)
    assert isinstance(got, kernels.I420Frames) and got.format == _abi.SRC_I420_BT601_FULL
    qt = np.broadcast_to(kernels.jpeg_quant_tables(85), (T, 3, 64))
    frames = src if source == "rgb" else src[1:T + 1]
    want = kernels.jpeg_idct_i420_host(kernels.jpeg_fdct_host(frames, qt, H, W, fmt), qt, H, W)
    assert np.array_equal(got.data.cpu().numpy(), want)


# ---- harness: yml quality_maps.overlay_video ------------------------------------------------------------------------------------
def _harness_cfg(tmp, mode, graph):
    """the tiny synthetic setting of tests/test_gpu_quality_map.py; mode: None (no quality_maps), "npz", or "avi" """
    import yaml
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "kwai_swin_grpb_qmap_test.yml")))
    a = cfg["data"]["val"]["args"]
    a.update(num_videos=7, frames=64, height=300, width=400, seed_per_item=True)
    a["sample_types"]["technical"].update(clip_len=32, num_clips=2)
    cfg.update(hipgraph=graph, streams=2)
    if mode is None:
        cfg.pop("quality_maps")
    else:
        cfg["quality_maps"].update(dir=str(tmp / f"maps_{mode}_{graph}"), overlay_frames=2)
        if mode != "npz":
            cfg["quality_maps"].update(overlay_video=mode, overlay_quality=80)
    return cfg


def _run_harness(tmp, monkeypatch, mode, graph):
    import types
    from kvq_amd.trainer import Trainer
    run = tmp / f"run_{mode}_{graph}"
    run.mkdir()
    monkeypatch.chdir(run)
    torch.manual_seed(0)                                # the network's own initialisation: the same weights in every run
    t = Trainer(types.SimpleNamespace(gpu_id="0"), _harness_cfg(tmp, mode, graph))
    t.inferece_test()
    torch.cuda.synchronize()
    return t, (run / "output.txt").read_bytes()


@pytest.mark.parametrize("graph", ["on", "off"])
def test_harness_writes_the_overlays_as_video(tmp_path, monkeypatch, graph):
    _, plain = _run_harness(tmp_path, monkeypatch, None, graph)
    _, with_npz = _run_harness(tmp_path, monkeypatch, "npz", graph)
    t, with_avi = _run_harness(tmp_path, monkeypatch, "avi", graph)
    assert with_avi == with_npz == plain                                 # output.txt: byte-identical
    if graph == "on":
        replays, eager = t.graph_stats
        assert replays > 0 and eager == 0                                # the FDCT launches are part of the recorded forward
    names = [l.split(",")[0] for l in plain.decode().strip().splitlines()]
    ndir, adir = tmp_path / f"maps_npz_{graph}", tmp_path / f"maps_avi_{graph}"
    assert len(names) == 7 and sorted(os.listdir(adir)) == sorted([n + ".npz" for n in names] + [n + ".overlay.avi" for n in names])
    qt = np.broadcast_to(kernels.jpeg_quant_tables(80), (4, 3, 64))
    for name in names:
        a, z = np.load(ndir / (name + ".npz")), np.load(adir / (name + ".npz"))
        assert set(z.files) == (set(a.files) - {"overlay"}) | {"overlay_frame_inds"}
        for k in set(a.files) - {"overlay"}:
            assert a[k].dtype == z[k].dtype and a[k].shape == z[k].shape and a[k].tobytes() == z[k].tobytes(), k
        assert np.array_equal(z["overlay_frame_inds"], z["frame_inds"][:, [4, 12], 0]) and z["overlay_frame_inds"].shape == (2, 2)
        vr = fd.open_video(str(adir / (name + ".overlay.avi")))
        assert (len(vr), vr.H, vr.W, vr.fps) == (4, 300, 400, 2.0)
        overlay = a["overlay"].reshape(4, 3, 300, 400)                   # all clips in order, their slices in depth order
        want = kernels.jpeg_idct_i420_host(kernels.jpeg_fdct_host(np.ascontiguousarray(overlay.transpose(1, 0, 2, 3)), qt, 300, 400), qt, 300, 400)
        for i in range(4):
            assert np.array_equal(vr.i420(i), want[i]), (name, i)
