"""GPU: kvq_jpeg_entropy (one lane per restart interval) against its host twin and kvq_jpeg_coeffs to the bit, inside guard bands; three
malformed segments whose status the host twin has produced first; the Motion-JPEG reader with the entropy decode on the device against
the host path, its fall-back to the host decoder and its errors.  Expected coefficients are kvq_jpeg_coeffs' and tests/jpeg_ref.py's."""
import numpy as np
import pytest
import torch

import kvq_amd  # noqa: F401
from kvq_amd import _abi, kernels
from kvq_amd.datasets import fusion_datasets as fd

import jpeg_ref
import jpeg_entropy_cases as jc
from guarded import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _launch(data, frames, segs, tables, T, H, W):
    """``kernels.jpeg_entropy`` with every buffer between guard bands and the outputs pre-filled with 0x55 -> (coef (T, blocks, 64),
    status) as numpy, after the guards have been found intact"""
    with guarded() as G:
        d = G.wrap(torch.from_numpy(data).to(DEV), name="bytes")
        f = G.wrap(torch.from_numpy(frames.view(np.int32)).to(DEV), name="frames")
        s = G.wrap(torch.from_numpy(segs.view(np.int32)).to(DEV), name="segs")
        t = G.wrap(torch.from_numpy(tables).to(DEV), poison="zero", name="tables")
        coef = G.alloc((T, kernels.jpeg_coef_bytes(H, W) // 2), torch.int16, DEV, name="coef")
        status = G.alloc((segs.shape[0],), torch.int32, DEV, name="status")
        coef.fill_(0x5555)
        status.fill_(0x55555555)
        c, st = kernels.jpeg_entropy(d, f, s, t, T, H, W, coef=coef, status=status)
        report = G.intact()
        assert report, report
        assert c.data_ptr() == coef.data_ptr() and st.data_ptr() == status.data_ptr()
        return coef.cpu().numpy().reshape(T, -1, 64), status.cpu().numpy()


def _check(jpgs, front=0):
    p = jpeg_ref.parse(jpgs[0])
    H, W = p["H"], p["W"]
    data, frames, segs, tables, _ = jc.pack(jpgs, front)
    coef, status = _launch(data, frames, segs, tables, len(jpgs), H, W)
    twin, twin_status = kernels.jpeg_entropy_host(data, frames, segs, tables, len(jpgs), H, W)
    assert (status == 0).all() and np.array_equal(status, twin_status), status
    for t, jpg in enumerate(jpgs):
        rc, want, _, msg = jc.host_coeffs(jpg, H, W)
        assert rc == 0, msg
        assert np.array_equal(coef[t], want), t                     # bit-equal; what the stream does not set reads 0, not 0x5555
        assert np.array_equal(coef[t], twin[t].reshape(-1, 64)), t
    return tables


@pytest.mark.parametrize("name", jc.FIXTURES)
def test_kernel_equals_the_decoder_on_the_fixtures(golden, name):
    _check([golden("mjpeg.npz")[name + "_jpg"].tobytes()])


@pytest.mark.parametrize("case", jc.SYNTHETIC, ids=jc.case_id)
def test_kernel_equals_the_decoder_on_synthetic_frames(case):
    _check([jc.synthetic(case)])


def test_one_launch_of_frames_with_different_restart_intervals_and_table_sets(golden):
    """T = 5 of 45 x 70: restart 0 / 1 / 7, with and without DHT, and one frame with optimised tables — two table sets, the second
    one used by the middle frame; the images do not start at offset 0"""
    coef, qt = jc.coefficients(45, 70)
    jpgs = [jpeg_ref.encode_baseline(coef, qt, 45, 70, restart=ri, dht=dht) for ri, dht in ((0, True), (1, False), (7, True))]
    jpgs = jpgs[:2] + [golden("mjpeg.npz")["odd_optimize_jpg"].tobytes()] + jpgs[2:] + [golden("mjpeg.npz")["odd_restart_jpg"].tobytes()]
    tables = _check(jpgs, front=5)
    assert tables.shape[0] == 2


def test_malformed_segments_get_the_host_twins_status_and_touch_nothing_else():
    H, W, ri = 130, 150, 10
    jpg = jc.synthetic((H, W, ri, True))
    _, want, _, _ = jc.host_coeffs(jpg, H, W)
    data, frames, segs, tables, _ = jc.pack([jpg])
    s = 4
    others = np.setdiff1d(np.arange(want.shape[0]), jc.segment_blocks(H, W, ri, s))
    for what, cause in (("cut", (1, 2, 4)), ("code", (2,)), ("run", (4,))):
        d, sg = data.copy(), segs.copy()
        if what == "cut":
            sg[s, 1] -= 3                                            # three bytes short, the range shortened to match
        elif what == "code":
            d[sg[s, 0]:sg[s, 0] + len(jc.NO_SUCH_CODE)] = np.frombuffer(jc.NO_SUCH_CODE, np.uint8)
        else:
            d[sg[s, 0]:sg[s, 0] + len(jc.RUN_PAST_63)] = np.frombuffer(jc.RUN_PAST_63, np.uint8)
        # the host twin first, in exact-size buffers between guards of its own: a status, and nothing outside its buffers
        guard = np.concatenate([np.full(64, 0xFF, np.uint8), d, np.full(64, 0xFF, np.uint8)])
        fr = frames.copy()
        fr[0, 0] += 64
        twin, twin_status = kernels.jpeg_entropy_host(guard, fr, sg, tables, 1, H, W)
        assert twin_status[s] != 0 and (twin_status[s] & 255) in cause and (np.delete(twin_status, s) == 0).all(), (what, twin_status)
        assert np.array_equal(twin[0].reshape(-1, 64)[others], want[others]), what
        coef, status = _launch(d, frames, sg, tables, 1, H, W)
        assert np.array_equal(status, twin_status), (what, status, twin_status)
        assert np.array_equal(coef[0][others], want[others]), what
        assert np.array_equal(coef[0], twin[0].reshape(-1, 64)), what


def test_launch_rejects_bad_arguments():
    lib = _abi.lib()
    buf = torch.zeros(16384, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    args = lambda **kw: [kw.get(k, v) for k, v in (("bytes", p), ("nbytes", 64), ("frames", p), ("segs", p), ("nsegs", 1), ("tables", p),     # noqa: E731
                                                   ("ntables", 1), ("T", 1), ("H", 16), ("W", 16), ("coef", p), ("status", p), ("stream", None))]
    assert lib.kvq_jpeg_entropy(*args(bytes=None)) == -1
    assert lib.kvq_jpeg_entropy(*args(T=0)) == -2 and lib.kvq_jpeg_entropy(*args(H=0)) == -2 and lib.kvq_jpeg_entropy(*args(ntables=0)) == -2
    assert lib.kvq_jpeg_entropy(*args(nbytes=1 << 32)) == -2
    assert lib.kvq_jpeg_entropy(*args(coef=p + 2)) == -2 and b"aligned" in lib.kvq_last_error()
    assert lib.kvq_jpeg_entropy(*args(segs=p + 2)) == -2 and b"aligned" in lib.kvq_last_error()
    torch.cuda.synchronize()


# ---- the reader ---------------------------------------------------------------------------------------------------------------------
def _clip(T, H, W, restart, seed=31):
    coef, qt = jpeg_ref.synthetic_coefficients(seed, T, H, W)
    jpgs = [jpeg_ref.encode_baseline(coef[t], qt[t], H, W, restart=restart(t) if callable(restart) else restart, dht=t % 3 != 2) for t in range(T)]
    return jpgs, np.stack([jpeg_ref.idct_i420(coef[t], qt[t], H, W) for t in range(T)])


@pytest.fixture()
def counted(monkeypatch):
    """``kernels.jpeg_entropy`` behind a counting wrapper"""
    calls, real = [], kernels.jpeg_entropy

    def wrapper(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(kernels, "jpeg_entropy", wrapper)
    return calls


@pytest.mark.parametrize("container", ["mjpeg", "avi"])
def test_device_entropy_equals_the_host_path(tmp_path, counted, container):
    H, W = 48, 64
    jpgs, frames = _clip(9, H, W, 3)
    path = str(tmp_path / ("clip." + container))
    if container == "mjpeg":
        jpeg_ref.write_mjpeg(path, jpgs)
    else:
        jpeg_ref.write_avi(path, jpgs, W, H, rate=24, scale=1)
    r = fd.open_video(path)
    assert list(r.restart_intervals) == [3] * 9
    uniq = np.array([0, 1, 2, 4, 7, 8])
    a = fd._frames_to_device(r, uniq, DEV, "device")
    assert len(counted) == 1
    b = fd._frames_to_device(r, uniq, DEV, "host")
    assert len(counted) == 1
    assert isinstance(a, kernels.I420Frames) and a.format == b.format == _abi.SRC_I420_BT601_FULL and a.shape == b.shape
    assert torch.equal(a.data, b.data) and np.array_equal(a.data.cpu().numpy(), frames[uniq])
    a2 = fd._frames_to_device(r, uniq[::2], DEV, "device")          # the second staging buffer, other frames
    assert np.array_equal(a2.data.cpu().numpy(), frames[uniq[::2]])


def test_device_entropy_on_a_file_without_dri(tmp_path, counted):
    H, W = 48, 64
    jpgs, frames = _clip(4, H, W, 0)
    path = str(tmp_path / "clip.mjpeg")
    jpeg_ref.write_mjpeg(path, jpgs)
    r = fd.open_video(path)
    assert not r.restart_intervals.any()
    a = fd._frames_to_device(r, np.arange(4), DEV, "device")
    assert len(counted) == 1 and np.array_equal(a.data.cpu().numpy(), frames)
    assert torch.equal(a.data, fd._frames_to_device(r, np.arange(4), DEV, "host").data)


def test_auto_takes_the_host_path_when_a_frame_has_no_restart_interval(tmp_path, counted):
    H, W = 48, 64
    jpgs, frames = _clip(5, H, W, lambda t: 0 if t == 3 else 4)
    path = str(tmp_path / "clip.mjpeg")
    jpeg_ref.write_mjpeg(path, jpgs)
    r = fd.open_video(path)
    assert list(r.restart_intervals) == [4, 4, 4, 0, 4]
    a = fd._frames_to_device(r, np.arange(5), DEV)                   # the module default: auto
    assert fd.JPEG_ENTROPY == "auto" and len(counted) == 0 and np.array_equal(a.data.cpu().numpy(), frames)
    b = fd._frames_to_device(r, np.array([0, 1, 4]), DEV, "auto")    # every frame of THIS call has one
    assert len(counted) == (1 if fd._JPEG_ENTROPY_AUTO_DEVICE else 0) and np.array_equal(b.data.cpu().numpy(), frames[[0, 1, 4]])
    c = fd._frames_to_device(r, np.array([0, 1, 4]), "cpu", "auto")  # a CPU target: always the host
    assert len(counted) == (1 if fd._JPEG_ENTROPY_AUTO_DEVICE else 0) and np.array_equal(c.data.numpy(), frames[[0, 1, 4]])


def test_a_frame_only_the_host_decoder_accepts_comes_back_equal(tmp_path, counted):
    """one byte too many in front of EOI: kvq_jpeg_coeffs drops it with the padding, the strict end of the device decode does not"""
    H, W = 48, 64
    jpgs, frames = _clip(3, H, W, 3)
    extra = jpgs[1][:-2] + b"\x00" + jpgs[1][-2:]
    rc, want, _, msg = jc.host_coeffs(extra, H, W)
    assert rc == 0 and np.array_equal(want, jc.host_coeffs(jpgs[1], H, W)[1]), msg
    data, fr, segs, tables, _ = jc.pack([extra])
    _, status = kernels.jpeg_entropy_host(data, fr, segs, tables, 1, H, W)
    assert status[-1] & 255 == 5 and (status[:-1] == 0).all()
    path = str(tmp_path / "clip.mjpeg")
    jpeg_ref.write_mjpeg(path, [jpgs[0], extra, jpgs[2]])
    r = fd.open_video(path)
    a = fd._frames_to_device(r, np.arange(3), DEV, "device")
    assert len(counted) == 1 and np.array_equal(a.data.cpu().numpy(), frames)
    assert torch.equal(a.data, fd._frames_to_device(r, np.arange(3), DEV, "host").data)


def test_a_corrupted_segment_is_the_host_decoders_value_error(tmp_path, counted):
    H, W = 48, 64
    jpgs, _ = _clip(3, H, W, 3)
    assert b"\xff\xc4" in jpgs[1]                                    # its tables are the Annex K ones the code was made for
    segs, _ = jc.marker_search(jpgs[1])
    bad = bytearray(jpgs[1])
    bad[segs[2, 0]:segs[2, 0] + len(jc.NO_SUCH_CODE)] = jc.NO_SUCH_CODE
    data, fr, sg, tables, _ = jc.pack([bytes(bad)])
    _, status = kernels.jpeg_entropy_host(data, fr, sg, tables, 1, H, W)      # the host twin first: a status, inside its buffers
    assert status[2] == (2 | (6 << 8)) and (np.delete(status, 2) == 0).all()
    path = str(tmp_path / "clip.mjpeg")
    jpeg_ref.write_mjpeg(path, [jpgs[0], bytes(bad), jpgs[2]])
    r = fd.open_video(path)
    for mode in ("device", "host"):
        with pytest.raises(ValueError, match=r"clip\.mjpeg: frame 1: kvq_jpeg_coeffs: a code that is in no Huffman table \(MCU 6 of 12, block 0\)"):
            fd._frames_to_device(r, np.arange(3), DEV, mode)
    assert len(counted) == 1
    torch.cuda.synchronize()
