"""GPU: the device entropy coder (csrc/jpeg_enc_entropy.hip, one lane per block) against its host twin and, through it, against
``kvq_jpeg_encode`` and the restatement: the same bytes, no tolerance, on the cases of tests/jpeg_scan_cases.py; guard bands; the
writer's device path against its host path in the three containers; the transcode tool."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import kvq_amd  # noqa: F401
from kvq_amd import _abi, kernels
from kvq_amd.datasets import fusion_datasets as fd

import jpeg_ref
import jpeg_scan_cases as jc
from guarded import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev_qt(qt):
    return torch.from_numpy(np.ascontiguousarray(qt).view(np.int16)).to(DEV).view(torch.uint16)


def _dev_coef(case):
    """the case's coefficients on the device: from ``kernels.jpeg_fdct`` where it has pixels"""
    if case.rgb is None:
        return torch.from_numpy(case.coef).to(DEV)
    coef = kernels.jpeg_fdct(torch.from_numpy(case.rgb).to(DEV), _dev_qt(case.qt))
    assert np.array_equal(coef.cpu().numpy(), case.coef), case.name
    return coef


@pytest.fixture(scope="module")
def cases(golden):
    """[(case, the expected scans, the expected table)]: computed once, by the host coder and the restatement"""
    return [(c,) + jc.expected_scans(c) for c in jc.pixel_cases(golden) + jc.crafted_cases()]


def test_launch_equals_the_twin_on_every_case_twice(cases):
    for case, body, table in cases:
        coef = _dev_coef(case)
        want_out, want_frames = kernels.jpeg_encode_scans_host(case.coef, case.H, case.W, case.ri, cap=len(body))
        assert want_out.tobytes() == body and np.array_equal(want_frames, table), case.name
        runs = [kernels.jpeg_encode_scans(coef, case.H, case.W, case.ri, cap=len(body)) for _ in range(2)]
        for out, frames in runs:
            assert np.array_equal(frames.cpu().numpy().view(np.uint32), want_frames), (case.name, frames, want_frames)
            got = out.cpu().numpy()
            bad = np.nonzero(got != want_out)[0]
            assert bad.size == 0, (case.name, bad.size, bad[:8], got[bad[:8]], want_out[bad[:8]])
        # the default capacities: a quarter of the coefficient bytes; whatever the status, the words are the twin's
        out, frames = kernels.jpeg_encode_scans(coef, case.H, case.W, case.ri)
        want_out, want_frames = kernels.jpeg_encode_scans_host(case.coef, case.H, case.W, case.ri)
        assert np.array_equal(frames.cpu().numpy().view(np.uint32), want_frames), case.name
        if (want_frames[:, 2] <= 1).all():
            assert out.cpu().numpy()[:len(body)].tobytes() == body, case.name


def test_statuses_of_the_launch(cases):
    by = {c.name: (c, b, t) for c, b, t in cases}
    case, body, table = by["AC 1024 in the middle frame of three"]
    out, frames = kernels.jpeg_encode_scans(_dev_coef(case), case.H, case.W, case.ri, cap=len(body))
    assert frames.cpu()[:, 2].tolist() == [0, 1, 0] and out.cpu().numpy().tobytes() == body      # frames 0 and 2 are the host coder's
    case, body, table = by["DC difference of 2048"]
    assert kernels.jpeg_encode_scans(_dev_coef(case), case.H, case.W, case.ri)[1].cpu().tolist() == [[0, 0, 1]]
    case, body, table = by["noise 272x480 q75 T3 ri7"]
    coef = _dev_coef(case)
    need = kernels.jpeg_scans_workspace_bytes(3, case.H, case.W)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    with pytest.raises(Exception, match="workspace"):                                          # refused before anything is enqueued
        kernels.jpeg_encode_scans(coef, case.H, case.W, case.ri, workspace=ws[:need - 16])
    out, frames = kernels.jpeg_encode_scans(coef, case.H, case.W, case.ri, cap=len(body), workspace=ws)
    assert np.array_equal(frames.cpu().numpy().view(np.uint32), table) and out.cpu().numpy().tobytes() == body


def test_launch_inside_guard_bands(cases):
    for case, body, table in cases:
        need = len(body)
        if need == 0:
            continue
        T = case.coef.shape[0]
        for cap in (need, need - 1):
            with guarded() as G:
                coef = G.wrap(torch.from_numpy(case.coef).to(DEV), name="coef")
                ws = torch.empty(kernels.jpeg_scans_workspace_bytes(T, case.H, case.W), dtype=torch.uint8, device=DEV)
                out, frames = kernels.jpeg_encode_scans(coef, case.H, case.W, case.ri, cap=cap, workspace=ws)
                assert G.intact(), (case.name, cap, G.intact())
                got = frames.cpu().numpy().view(np.uint32)
                want = table.copy()
                want[(table[:, 0] + table[:, 1] > cap) & (table[:, 2] == 0), 2] = 2
                assert np.array_equal(got, want), (case.name, cap, got)
                assert int(got[-1, 0]) + int(got[-1, 1]) == need
                written = int(max((o + n for o, n, s in want.tolist() if s == 0), default=0))    # the end of the last frame that fits
                assert out[:written].cpu().numpy().tobytes() == body[:written], (case.name, cap)
                if written < cap:
                    assert G.untouched(out[written:]), (case.name, cap, G.untouched(out[written:]))
                assert (cap == need) == (written == need)


def _clip(T, H, W, source):
    g = np.random.Generator(np.random.PCG64(T * 7 + H))
    if source == "rgb":
        return torch.from_numpy(g.integers(0, 256, (3, T, H, W), dtype=np.uint8)).to(DEV)
    data = torch.from_numpy(g.integers(0, 256, (T, jpeg_ref.frame_bytes(H, W)), dtype=np.uint8)).to(DEV)
    return kernels.I420Frames(data, H, W, _abi.SRC_I420_BT601_FULL)


def _written(path):
    if os.path.isdir(path):
        return [(f, open(os.path.join(path, f), "rb").read()) for f in sorted(os.listdir(path))]
    return open(path, "rb").read()


@pytest.mark.parametrize("container", [".mjpeg", ".avi", "_dir"])
@pytest.mark.parametrize("source", ["rgb", "i420"])
@pytest.mark.parametrize("ri", [0, "row"])
def test_writer_device_files_equal_host_files(tmp_path, container, source, ri):
    T, H, W = 5, 45, 70
    frames = _clip(T, H, W, source)
    files = {}
    for mode in ("host", "device"):
        path = str(tmp_path / (mode + container))
        with fd.MjpegWriter(path, 25, quality=90, restart_interval=(W + 15) // 16 if ri == "row" else 0, entropy=mode) as w:
            w.write(frames)
            w.write(frames.frames(1, 3) if source == "i420" else frames[:, 1:3].contiguous())      # a second call appends
        assert w.frames == T + 2
        files[mode] = _written(path)
    assert files["device"] == files["host"] and len(files["host"]) > 0
    vr = {mode: fd.open_video(str(tmp_path / (mode + container))) for mode in files}
    got = {mode: fd._frames_to_device(v, np.arange(T + 2), DEV).data.cpu() for mode, v in vr.items()}
    assert len(vr["device"]) == T + 2 and torch.equal(got["device"], got["host"])


def test_writer_retries_with_the_capacity_the_table_names(tmp_path, monkeypatch):
    """q100 noise takes more than the default quarter of the coefficient bytes: status 2, then one call with the capacity it names"""
    frames = _clip(2, 48, 64, "rgb")
    calls = []
    real = kernels.jpeg_encode_scans
    monkeypatch.setattr(kernels, "jpeg_encode_scans", lambda *a, **k: calls.append(a[4]) or real(*a, **k))
    for mode in ("host", "device"):
        with fd.MjpegWriter(str(tmp_path / (mode + ".mjpeg")), 25, quality=100, entropy=mode) as w:
            w.write(frames)
    assert _written(str(tmp_path / "device.mjpeg")) == _written(str(tmp_path / "host.mjpeg"))
    size = os.path.getsize(str(tmp_path / "host.mjpeg"))
    head = len(kernels.jpeg_encode_header(kernels.jpeg_quant_tables(100), 48, 64))
    assert len(calls) == 2 and calls[0] is None and calls[1] == size - 2 * (head + 2)      # the exact capacity, once


def test_out_of_range_frame_raises_the_host_coders_message(tmp_path, monkeypatch):
    case = [c for c in jc.crafted_cases() if c.name == "AC 1024 in the middle frame of three"][0]
    coef = torch.from_numpy(case.coef).to(DEV)
    monkeypatch.setattr(kernels, "jpeg_fdct", lambda frames, qt: coef)      # no picture has such a coefficient: hand them in
    frames = _clip(3, case.H, case.W, "rgb")
    said = {}
    for mode in ("host", "device"):
        with pytest.raises(Exception) as e:
            with fd.MjpegWriter(str(tmp_path / (mode + ".mjpeg")), 25, quality=50, entropy=mode) as w:
                w.write(frames)
        said[mode] = (type(e.value), str(e.value))
    assert said["device"] == said["host"] and "1024" in said["host"][1] and "outside baseline" in said["host"][1]


def test_transcode_tool_entropy_option(tmp_path, monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location("transcode_mjpeg", os.path.join(ROOT, "tools", "transcode_mjpeg.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src = str(tmp_path / "src.npy")
    np.save(src, np.random.Generator(np.random.PCG64(3)).integers(0, 256, (4, 33, 50, 3), dtype=np.uint8))
    out = {}
    for mode in ("host", "device"):
        dst = str(tmp_path / (mode + ".avi"))
        monkeypatch.setattr(sys, "argv", ["transcode_mjpeg.py", src, dst, "--quality", "75", "--restart-interval", "row", "--device", "cuda",
                                          "--entropy", mode])
        tool.main()
        assert "4 frames" in capsys.readouterr().out
        out[mode] = open(dst, "rb").read()
    assert out["device"] == out["host"]
    with pytest.raises(ValueError, match="frames"):
        tool.transcode(src, str(tmp_path / "cpu.avi"), device="cpu", entropy="device")
