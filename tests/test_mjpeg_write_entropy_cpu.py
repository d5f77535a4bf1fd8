"""CPU: the host twin of the device entropy coder (``kvq_jpeg_encode_scans_host``: the phases of csrc/jpeg_enc_huff.hpp in loops) and
``kvq_jpeg_encode_header`` against ``kvq_jpeg_encode`` and the restatement tests/jpeg_enc_ref.py — the same bytes, no tolerance — on
the cases of tests/jpeg_scan_cases.py; capacities, the workspace, the writer's ``entropy`` argument, the ABI surface and the stand-alone
check under the host sanitizers.  The launch itself: tests/test_gpu_mjpeg_write_entropy.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import kvq_amd
from kvq_amd import _abi, kernels
from kvq_amd.datasets import fusion_datasets as fd

import jpeg_scan_cases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -3, -4
NEW_SYMBOLS = ["kvq_jpeg_encode_header", "kvq_jpeg_scans_workspace_bytes", "kvq_jpeg_encode_scans_host", "kvq_jpeg_encode_scans"]


@pytest.fixture(scope="module")
def cases(golden):
    return jc.pixel_cases(golden) + jc.crafted_cases()


def by_name(cases, name):
    (c,) = [c for c in cases if c.name == name]
    return c


def raw_call(case, cap, workspace_bytes, canary=64):
    """kvq_jpeg_encode_scans_host into buffers of exactly ``cap`` and ``workspace_bytes`` bytes with 0xA5 behind each -> (rc, out, frames);
    asserts both canaries are untouched"""
    T = case.coef.shape[0]
    coef = kernels._aligned16(case.coef.size, np.int16)
    coef[:] = case.coef.reshape(-1)
    out = np.full(cap + canary, 0xA5, np.uint8)
    ws = kernels._aligned16(workspace_bytes + canary, np.uint8)
    ws[:] = 0xA5
    frames = np.full((T + 1, 3), 0xA5A5A5A5, np.uint32)
    rc = _abi.lib().kvq_jpeg_encode_scans_host(coef.ctypes.data, T, case.H, case.W, case.ri, out.ctypes.data, cap, frames.ctypes.data, ws.ctypes.data,
                                               workspace_bytes)
    assert (out[cap:] == 0xA5).all() and (ws[workspace_bytes:] == 0xA5).all() and (frames[T] == 0xA5A5A5A5).all(), case.name
    return rc, out[:cap], frames[:T]


def test_header_scan_eoi_is_the_image_on_every_case(cases):
    for case in cases:
        body, table = jc.expected_scans(case)
        out, frames = kernels.jpeg_encode_scans_host(case.coef, case.H, case.W, case.ri, cap=len(body))
        assert np.array_equal(frames, table), (case.name, frames, table)
        assert out.tobytes() == body, case.name
        assert (table[:, 2] == 1).tolist() == (~case.ok).tolist()
        for dht in (True, False):
            head = kernels.jpeg_encode_header(case.qt, case.H, case.W, case.ri, dht).tobytes()
            for t, image in enumerate(jc.expected_images(case, dht)):
                if image is not None:
                    o, n = int(table[t, 0]), int(table[t, 1])
                    assert head + body[o:o + n] + b"\xff\xd9" == image, (case.name, t, dht)
                    assert (b"\xff\xc4" in head) == dht and (b"\xff\xdd\x00\x04" in head) == (case.ri != 0)


def test_the_cases_hold_what_they_are_there_for(cases):
    """each condition re-asserted on the host coder's output"""
    scan = lambda name: jc.expected_scans(by_name(cases, name))[0]      # noqa: E731
    grey = scan("grey 48x64 q50 ri0")
    assert len(grey) < 72, len(grey)                                    # blocks far shorter than a byte: many share a 32-bit word
    ri1 = scan("grey 48x64 q50 ri1")
    assert [ri1[i + 1] for i in range(len(ri1) - 1) if ri1[i] == 0xFF and ri1[i + 1] != 0] == [0xD0 + (k & 7) for k in range(11)]
    # RSTn wraps past RST7; a grey MCU is 4 x (2 + 4) + 2 x (2 + 2) = 32 bits, so an interval is exactly four bytes and needs no padding
    assert len(ri1) == 12 * 4 + 2 * 11 and len(grey) == 48
    for name in ("noise 48x48 q100 ri1", "noise 45x70 q100 ri5 (row)", "noise 64x80 q100 ri0", "noise 64x80 q100 ri5 (row)"):
        n = scan(name).count(b"\xff\x00")
        print(name, "stuffed bytes:", n)
        assert n >= 1, name
    assert (70 + 15) // 16 == 5 and (64 + 15) // 16 == 4 and 15 % 5 == 0 and (45 + 15) // 16 * 5 == 15      # ri = mx; 15 MCUs
    assert 12 % 5 != 0 and (48 + 15) // 16 * ((48 + 15) // 16) == 9                                          # and intervals that do not divide the frame
    full = by_name(cases, "every block 1660 bits")
    assert len(jc.expected_scans(full)[0]) >= 12 * 1660 // 8            # more than 200 bytes from every block
    last = scan("only position 63: three ZRL, no EOB")
    assert len(last) > 0
    big = jc.expected_scans(by_name(cases, "noise 272x480 q75 T3 ri7"))[1]
    assert (big[:, 1] > 0).all() and len(set(big[:, 1].tolist())) == 3 and big[2, 0] == big[0, 1] + big[1, 1]


def test_statuses_and_table_words(cases):
    over = by_name(cases, "DC difference of 2048")
    out, frames = kernels.jpeg_encode_scans_host(over.coef, over.H, over.W, over.ri)
    assert frames.tolist() == [[0, 0, 1]]
    edge = by_name(cases, "DC differences of 2046")
    assert kernels.jpeg_encode_scans_host(edge.coef, edge.H, edge.W, edge.ri)[1][0, 2] == 0
    three = by_name(cases, "AC 1024 in the middle frame of three")
    body, table = jc.expected_scans(three)
    out, frames = kernels.jpeg_encode_scans_host(three.coef, three.H, three.W, three.ri, cap=len(body))
    assert frames[:, 2].tolist() == [0, 1, 0] and frames[1, 1] == 0 and frames[2, 0] == frames[0, 1] and out.tobytes() == body


def test_short_capacity_and_short_workspace(cases):
    lib = _abi.lib()
    for case in cases:
        T = case.coef.shape[0]
        body, table = jc.expected_scans(case)
        need = len(body)
        full = lib.kvq_jpeg_scans_workspace_bytes(T, case.H, case.W)
        blocks = kernels.jpeg_coef_bytes(case.H, case.W) // 128
        assert full == (8 * T * blocks + 15) // 16 * 16 + (4 * T * blocks + 15) // 16 * 16 + 16 * T + (8 * T + 15) // 16 * 16      # whatever the data
        rc, out, frames = raw_call(case, need, full)
        assert rc == OK and out.tobytes() == body and np.array_equal(frames, table), case.name
        # below the need: refused, nothing stored anywhere (the canaries are raw_call's to check)
        for ws in (full - 1, full // 2, 0):
            rc, out, frames = raw_call(case, need, ws)
            assert rc == ERR_WORKSPACE and "workspace" in lib.kvq_last_error().decode() and (frames == 0xA5A5A5A5).all() and (out == 0xA5).all()
        if need == 0:
            continue
        rc, out, frames = raw_call(case, need - 1, full)                 # the frames that end past cap: status 2, the need still exact
        want = table.copy()
        want[(table[:, 0] + table[:, 1] > need - 1) & (table[:, 2] == 0), 2] = 2
        assert rc == OK and np.array_equal(frames, want) and (want[:, 2] == 2).any(), (case.name, frames)
        assert int(frames[-1, 0] + frames[-1, 1]) == need
        last = int(np.nonzero(want[:, 2] == 2)[0][0])
        assert out[:table[last, 0]].tobytes() == body[:table[last, 0]], case.name      # the frames in front of it are whole
        assert (out[table[last, 0]:] == 0xA5).all(), case.name                          # and nothing of the frame that does not fit is stored


def test_refusals():
    lib = _abi.lib()
    coef, out, frames, ws = kernels._aligned16(384, np.int16), np.zeros(64, np.uint8), np.zeros(3, np.uint32), kernels._aligned16(4096, np.uint8)
    call = lambda T=1, H=16, W=16, ri=0, cap=64, c=coef, w=ws: lib.kvq_jpeg_encode_scans_host(      # noqa: E731
        c.ctypes.data, T, H, W, ri, out.ctypes.data, cap, frames.ctypes.data, w.ctypes.data, w.size)
    coef[:] = 0
    assert call() == OK and frames.tolist()[2] == 0
    assert call(T=0) == ERR_SHAPE and call(H=0) == ERR_SHAPE and call(ri=65536) == ERR_SHAPE and call(ri=-1) == ERR_SHAPE and call(cap=1 << 32) == ERR_SHAPE
    assert lib.kvq_jpeg_encode_scans_host(coef.ctypes.data + 2, 1, 16, 16, 0, out.ctypes.data, 64, frames.ctypes.data, ws.ctypes.data, ws.size) == ERR_SHAPE
    assert lib.kvq_jpeg_encode_scans_host(None, 1, 16, 16, 0, out.ctypes.data, 64, frames.ctypes.data, ws.ctypes.data, ws.size) == ERR_NULL
    assert lib.kvq_jpeg_encode_scans(None, 1, 16, 16, 0, None, 0, None, None, 0, None) == ERR_NULL                  # checked before any HIP call
    qt, n = kernels.jpeg_quant_tables(50), C.c_size_t(0)
    assert lib.kvq_jpeg_encode_header(qt.ctypes.data, 16, 16, 0, 2, out.ctypes.data, 64, C.byref(n)) == ERR_SHAPE
    assert lib.kvq_jpeg_encode_header(qt.ctypes.data, 16, 16, 0, 0, out.ctypes.data, 64, C.byref(n)) == ERR_WORKSPACE and n.value > 64
    bad = qt.copy()
    bad[1, 3] = 256
    assert lib.kvq_jpeg_encode_header(bad.ctypes.data, 16, 16, 0, 0, out.ctypes.data, 64, C.byref(n)) == ERR_UNSUPPORTED
    assert "kvq_jpeg_encode_header" in lib.kvq_last_error().decode()
    assert lib.kvq_jpeg_scans_workspace_bytes(0, 16, 16) == 0 and lib.kvq_jpeg_scans_workspace_bytes(1, 0, 16) == 0


def test_encode_still_writes_the_fixtures_image(golden):
    """kvq_jpeg_encode calls kvq_jpeg_encode_header's code now: the header it writes is that entry's, and the image is the restatement's"""
    g = golden("mjpeg_enc.npz")
    for name in jc.FIXTURES:
        rgb = np.ascontiguousarray(g[name + "_rgb"].transpose(2, 0, 1)[:, None])
        H, W = rgb.shape[2:]
        qt = kernels.jpeg_quant_tables(int(g[name + "_q"]))
        coef = kernels.jpeg_fdct_host(rgb, qt, H, W)[0]
        for ri, dht in ((0, True), (3, False)):
            image = kernels.jpeg_encode(coef, qt, H, W, ri, dht).tobytes()
            assert image == jc.jpeg_enc_ref.encode(coef.reshape(-1, 64), qt, H, W, ri, dht), name
            head = kernels.jpeg_encode_header(qt, H, W, ri, dht).tobytes()
            assert image.startswith(head) and head.endswith(jc.SOS), name


def _rgb(T, H, W):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(5)).integers(0, 256, (3, T, H, W), dtype=np.uint8))


def test_writer_entropy_argument(tmp_path):
    frames = _rgb(3, 45, 70)
    with pytest.raises(ValueError, match="frames"):
        with fd.MjpegWriter(str(tmp_path / "d.mjpeg"), 25, entropy="device") as w:
            w.write(frames)
    with pytest.raises(ValueError, match="auto, host, device"):
        fd.MjpegWriter(str(tmp_path / "e.mjpeg"), 25, entropy="gpu")
    assert fd.JPEG_WRITE_ENTROPY in fd.JPEG_ENTROPY_MODES
    qt = kernels.jpeg_quant_tables(80)
    coef = kernels.jpeg_fdct_host(frames.numpy(), qt, 45, 70)
    today = b"".join(kernels.jpeg_encode(c, qt, 45, 70, 5).tobytes() for c in coef)
    for name, kw in (("none", {}), ("host", {"entropy": "host"}), ("auto", {"entropy": "auto"})):
        path = str(tmp_path / (name + ".mjpeg"))
        with fd.MjpegWriter(path, 25, quality=80, restart_interval=5, **kw) as w:
            w.write(frames)
        assert open(path, "rb").read() == today, name


def test_new_entries_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "kvq_hip.h")).read()
    declared = set(re.findall(r"\b(kvq_[a-z0-9_]+)\s*\(", header))
    handle = _abi.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _abi.SYMBOLS and hasattr(handle, name), name
    assert handle.kvq_abi_version() == _abi.ABI_VERSION == 32 and "#define KVQ_ABI_VERSION 32" in header
    from kvq_amd import _build
    assert "jpeg_enc_entropy.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "jpeg_enc_huff.hpp"))


def test_hostcheck_under_the_sanitizers(tmp_path, golden):
    """tools/jpeg_enc_entropy_hostcheck.cpp: a program of its own, the host compiler alone, -fsanitize=address,undefined: header + host twin
    into exact-size heap buffers, the small cases at every capacity and every workspace size"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    probe = subprocess.run([cxx, "-x", "c++", "-", "-fsanitize=address,undefined", "-o", os.devnull], input="int main() { return 0; }",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip(f"{cxx} has no address / undefined-behaviour sanitizer runtimes")
    exe = str(tmp_path / "jpeg_enc_entropy_hostcheck")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                        os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "jpeg_enc_entropy_hostcheck.cpp"),
                        os.path.join(os.path.dirname(kvq_amd.__file__), "csrc", "jpeg_enc.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    g = golden("mjpeg_enc.npz")
    files = []
    for name in jc.FIXTURES:
        files.append(str(tmp_path / (name + ".rgb")))
        g[name + "_rgb"].tofile(files[-1])
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    assert r.returncode == 0 and "jpeg_enc_entropy_hostcheck: all clean" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
