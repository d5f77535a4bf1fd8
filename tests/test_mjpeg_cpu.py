"""CPU: the host half of the Motion-JPEG reader (csrc/jpeg.cpp) against its restatement (tests/jpeg_ref.py) on the Pillow-made
fixtures of tests/golden/mjpeg.npz: probe, entropy decode (every coefficient), the scalar IDCT twin (bit-equal to the restatement, within
+-1 of libjpeg's Y), the refusals, a prefix sweep (no prefix decodes, nothing is written past coef_cap), the three containers through
``open_video`` and the ABI surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kvq_amd  # noqa: F401
from kvq_amd import _abi, kernels
from kvq_amd.datasets import fusion_datasets as fd

import jpeg_ref
import yuv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODABLE = ["noise_q100", "noise_q5", "odd", "odd_no_dht", "odd_optimize", "odd_restart", "one_mcu", "sub_mcu", "video_0", "video_1", "video_2"]
REFUSED = {"progressive": "progressive", "s422": "Y 2x1 Cb 1x1 Cr 1x1", "s444": "Y 1x1 Cb 1x1 Cr 1x1", "gray": "1 component", "cmyk": "4 components"}
OK, ERR_SHAPE, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -2, -3, -4


@pytest.fixture(scope="module")
def cases(golden):
    g = golden("mjpeg.npz")
    assert sorted(g["decodable"].tolist()) == DECODABLE and sorted(g["refused"].tolist()) == sorted(REFUSED)
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def restated(cases):
    """name -> (coef, qt, parse dict, I420 frame) by the restatement, computed once"""
    out = {}
    for name in DECODABLE:
        coef, qt, p = jpeg_ref.decode_coeffs(cases[name + "_jpg"].tobytes())
        out[name] = (coef, qt, p, jpeg_ref.idct_i420(coef, qt, p["H"], p["W"]))
    return out


def lib_decode(data, canary=64):
    """kvq_jpeg_coeffs on a uint8 array -> (rc, coef (blocks, 64), qt (3, 64)); asserts the canary behind coef_cap is untouched"""
    rc, info, _ = kernels.jpeg_probe(data)
    assert rc == OK
    n = kernels.jpeg_coef_bytes(info.height, info.width) // 2
    buf = np.full(n + canary, 0x5A5A, np.int16)
    qt = np.zeros((3, 64), np.uint16)
    rc = _abi.lib().kvq_jpeg_coeffs(data.ctypes.data, data.size, buf.ctypes.data, 2 * n, qt.ctypes.data)
    assert (buf[n:] == 0x5A5A).all()
    return rc, buf[:n].reshape(-1, 64), qt


@pytest.mark.parametrize("name", DECODABLE)
def test_probe_and_coefficients_equal_the_restatement(cases, restated, name):
    data = cases[name + "_jpg"]
    coef, qt, p, _ = restated[name]
    rc, info, msg = kernels.jpeg_probe(data)
    assert rc == OK and info.supported == 1, msg
    assert (info.width, info.height, info.ncomp, info.restart_interval) == (p["W"], p["H"], 3, p["ri"])
    assert (list(info.hsamp)[:3], list(info.vsamp)[:3]) == ([2, 1, 1], [2, 1, 1])
    assert info.frame_bytes == data.size == p["frame_bytes"] and info.has_dht == (name != "odd_no_dht")
    assert kernels.jpeg_coef_bytes(p["H"], p["W"]) == jpeg_ref.coef_bytes(p["H"], p["W"]) == 768 * ((p["W"] + 15) // 16) * ((p["H"] + 15) // 16)
    rc, got, got_qt = lib_decode(data)
    assert rc == OK
    assert np.array_equal(got_qt, qt)
    assert np.array_equal(got, coef)
    if name == "odd_restart":
        assert p["ri"] > 0 and any(bytes([0xFF, 0xD0 + k]) in data.tobytes() for k in range(8))
    if name == "odd_optimize":
        assert p["huff"][(1, 0)] != jpeg_ref._codes(*jpeg_ref.STD_AC_LUM)        # custom tables, not Annex K's
    if name == "noise_q100":
        assert (qt == 1).all() and np.count_nonzero(coef) > coef.size // 2


def test_the_stream_without_dht_decodes_with_the_annex_k_tables(restated):
    assert np.array_equal(restated["odd_no_dht"][0], restated["odd"][0]) and np.array_equal(restated["odd_no_dht"][3], restated["odd"][3])


@pytest.mark.parametrize("name", DECODABLE)
def test_host_idct_is_bit_equal_to_the_restatement_and_within_one_of_libjpeg(cases, restated, name):
    coef, qt, p, frame = restated[name]
    H, W = p["H"], p["W"]
    got = kernels.jpeg_idct_i420_host(coef[None], qt[None], H, W)
    assert got.shape == (1, kernels.i420_frame_bytes(H, W)) and np.array_equal(got[0], frame)
    want = cases[("odd" if name == "odd_no_dht" else name) + "_y"]
    d = np.abs(jpeg_ref.planes(got[0], H, W)[0].astype(np.int16) - want.astype(np.int16))
    assert want.shape == (H, W) and int(d.max()) <= 1


def test_host_idct_on_synthetic_coefficients_in_the_defined_range():
    for H, W in ((16, 16), (7, 9), (45, 70), (33, 17)):
        coef, qt = jpeg_ref.synthetic_coefficients(H * 131 + W, 3, H, W)
        want = np.stack([jpeg_ref.idct_i420(coef[t], qt[t], H, W) for t in range(3)])
        assert np.array_equal(kernels.jpeg_idct_i420_host(coef, qt, H, W), want)
        assert want.min() == 0 and want.max() == 255 or (H, W) == (7, 9)


def test_out_of_range_coefficients_stay_in_bounds_and_agree():
    """beyond the defined range the value is unspecified but the same everywhere: int32 wrap-around on both sides"""
    g = np.random.Generator(np.random.PCG64(9))
    H, W = 24, 40
    coef = g.integers(-32768, 32768, (2, jpeg_ref.geom(H, W)[4], 64)).astype(np.int16)
    qt = g.integers(1, 256, (2, 3, 64)).astype(np.uint16)
    want = np.stack([jpeg_ref.idct_i420(coef[t], qt[t], H, W) for t in range(2)])
    assert np.array_equal(kernels.jpeg_idct_i420_host(coef, qt, H, W), want)


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_name_their_cause(cases, name):
    data = cases[name + "_jpg"]
    rc, info, msg = kernels.jpeg_probe(data)
    assert rc == ERR_UNSUPPORTED and info.supported == 0
    assert REFUSED[name] in msg, msg
    assert (info.width, info.height) == (70, 45) and info.frame_bytes == data.size
    coef, qt = np.zeros(jpeg_ref.coef_bytes(45, 70) // 2, np.int16), np.zeros((3, 64), np.uint16)
    rc, msg = kernels.jpeg_coeffs(data, coef, qt)
    assert rc == ERR_UNSUPPORTED and REFUSED[name] in msg and not coef.any()


def _patched(data, find, replace):
    b = data.tobytes()
    at = b.index(find)
    return np.frombuffer(b[:at] + replace + b[at + len(find):], np.uint8)


def test_other_refusals_and_tolerated_segments(cases, restated):
    data = cases["odd_jpg"]
    sof = b"\xff\xc0\x00\x11\x08"
    rc, _, msg = kernels.jpeg_probe(_patched(data, sof, b"\xff\xc0\x00\x11\x0c"))
    assert rc == ERR_UNSUPPORTED and "12-bit" in msg
    rc, _, msg = kernels.jpeg_probe(_patched(data, sof, b"\xff\xc1\x00\x11\x08"))
    assert rc == ERR_UNSUPPORTED and "SOF1" in msg
    rc, _, msg = kernels.jpeg_probe(_patched(data, sof, b"\xff\xc9\x00\x11\x08"))
    assert rc == ERR_UNSUPPORTED and "arithmetic" in msg
    b = data.tobytes()
    dqt = b.index(b"\xff\xdb")
    q16 = b[:dqt] + b"\xff\xdb\x00\x83\x12" + bytes(128) + b[dqt:]                 # a 16-bit table 2 ahead of the real ones
    rc, _, msg = kernels.jpeg_probe(np.frombuffer(q16, np.uint8))
    assert rc == ERR_UNSUPPORTED and "16-bit quantiser" in msg
    adobe = b[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + b[2:]
    rc, _, msg = kernels.jpeg_probe(np.frombuffer(adobe, np.uint8))
    assert rc == ERR_UNSUPPORTED and "Adobe APP14" in msg and "transform 0" in msg
    # tolerated: a COM segment that holds FF D8 FF D9, an APP5, an Adobe segment with transform 1, fill bytes before markers
    extra = (b[:2] + b"\xff\xfe\x00\x08\xff\xd8\xff\xd9ab" + b"\xff\xff\xff\xe5\x00\x04zz" + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01"
             + b[2:dqt] + b"\xff\xff" + b[dqt:])
    arr = np.frombuffer(extra, np.uint8)
    rc, info, msg = kernels.jpeg_probe(arr)
    assert rc == OK and info.frame_bytes == arr.size, msg
    rc, got, _ = lib_decode(arr)
    assert rc == OK and np.array_equal(got, restated["odd"][0])
    rc, _, msg = kernels.jpeg_probe(np.frombuffer(b"\x89PNG\r\n\x1a\n" + bytes(32), np.uint8))
    assert rc == ERR_SHAPE and "not a JPEG" in msg
    assert _abi.lib().kvq_jpeg_probe(None, 0, None) == -1
    n = kernels.jpeg_coef_bytes(45, 70)
    assert _abi.lib().kvq_jpeg_coeffs(data.ctypes.data, data.size, np.zeros(n // 2, np.int16).ctypes.data, n - 2, np.zeros(192, np.uint16).ctypes.data) == ERR_WORKSPACE


def test_corrupt_entropy_data_is_an_error_with_a_message(cases):
    lib = _abi.lib()
    data = cases["odd_restart_jpg"]
    b = data.tobytes()
    first = min(b.index(bytes([0xFF, 0xD0 + k])) for k in range(8) if bytes([0xFF, 0xD0 + k]) in b)
    assert b[first + 1] == 0xD0
    wrong = np.frombuffer(b[:first + 1] + b"\xd3" + b[first + 2:], np.uint8)
    rc, coef, _ = lib_decode(wrong)
    assert rc == ERR_SHAPE and "wrong restart marker" in lib.kvq_last_error().decode()
    no_eoi = np.frombuffer(b[:-2] + b"\x00\x00", np.uint8)
    rc, _, _ = lib_decode(no_eoi)
    assert rc == ERR_SHAPE and "EOI" in lib.kvq_last_error().decode()
    # a run past coefficient 63 and a code that is in no table, written with the Annex K tables by hand
    H = W = 16
    coef = np.zeros((6, 64), np.int16)
    good = jpeg_ref.encode_baseline(coef, np.ones((3, 64), np.uint16), H, W)
    scan = good.index(b"\xff\xda") + 14
    assert good[scan:] == b"\x28\xa2\x8a\x00\xff\xd9"                            # Y: DC 0 (00) + EOB (1010), four times; Cb, Cr: 00 + 00
    # DC category 0 (00), then ZRL (11111111001) four times: k = 1 + 64 > 64
    bits = "00" + "11111111001" * 4
    bad = good[:scan] + int(bits.ljust(48, "1"), 2).to_bytes(6, "big").replace(b"\xff", b"\xff\x00") + b"\xff\xd9"
    rc, _, _ = lib_decode(np.frombuffer(bad, np.uint8))
    assert rc == ERR_SHAPE and "run past coefficient 63" in lib.kvq_last_error().decode()
    # DC category 0, then AC 15/10 (1111111111111110) followed by... sixteen ones is no luminance AC code
    bits = "00" + "1" * 16
    bad = good[:scan] + int(bits.ljust(32, "1"), 2).to_bytes(4, "big").replace(b"\xff", b"\xff\x00") + b"\xff\xd9"
    rc, _, _ = lib_decode(np.frombuffer(bad, np.uint8))
    assert rc == ERR_SHAPE and "no Huffman table" in lib.kvq_last_error().decode()


@pytest.mark.parametrize("name", ["one_mcu", "odd_restart"])
def test_no_prefix_decodes_and_none_writes_past_the_capacity(cases, name):
    lib = _abi.lib()
    data = cases[name + "_jpg"]
    H, W = cases[name + "_y"].shape
    n = kernels.jpeg_coef_bytes(H, W) // 2
    buf = np.empty(n + 64, np.int16)
    qt = np.zeros((3, 64), np.uint16)
    info = _abi.KvqJpegInfo()
    for k in range(data.size):
        prefix = np.array(data[:k])                         # its own allocation: a read past k would leave it
        buf[:] = 0x5A5A
        rc = lib.kvq_jpeg_coeffs(prefix.ctypes.data, k, buf.ctypes.data, 2 * n, qt.ctypes.data)
        assert rc in (ERR_SHAPE, -1), (k, rc)
        assert lib.kvq_last_error() != b"" and (buf[n:] == 0x5A5A).all(), k
        rc = lib.kvq_jpeg_probe(prefix.ctypes.data, k, C.byref(info))
        assert rc == ERR_SHAPE or (rc == OK and info.frame_bytes == 0), (k, rc)


# ---- containers -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def video(cases, restated):
    """the three 64 x 48 frames of different quality: (jpeg bytes, I420 frames by the restatement, RGB frames)"""
    names = ["video_0", "video_1", "video_2"]
    frames = np.stack([restated[n][3] for n in names])
    rgb = [yuv_ref.frame_rgb(f, 48, 64, _abi.SRC_I420_BT601_FULL) for f in frames]
    return [cases[n + "_jpg"].tobytes() for n in names], frames, rgb


def _check_reader(r, order, video, fps):
    _, frames, rgb = video
    assert isinstance(r, fd.MjpegFrameReader) and len(r) == len(order) and (r.H, r.W) == (48, 64)
    assert r.fps == fps and r.format == _abi.SRC_I420_BT601_FULL and r.frame_bytes == kernels.i420_frame_bytes(48, 64)
    for i, k in enumerate(order):
        got = r[i]
        assert got.dtype == np.uint8 and got.shape == (48, 64, 3) and np.array_equal(got, rgb[k]), i
        assert np.array_equal(r.i420(i), frames[k])
    idx = list(range(len(order)))[::-1]
    coef, qt = np.zeros((len(idx), r.coef_bytes // 2), np.int16), np.zeros((len(idx), 3, 64), np.uint16)
    r.read_jpeg_into(idx, coef, qt)
    assert np.array_equal(kernels.jpeg_idct_i420_host(coef, qt, 48, 64), frames[[order[i] for i in idx]])
    dev = fd._frames_to_device(r, np.array([0, len(order) - 1]), "cpu")                   # no device: the scalar twin
    assert isinstance(dev, kernels.I420Frames) and np.array_equal(dev.data.numpy(), frames[[order[0], order[-1]]])


def test_raw_stream(tmp_path, video):
    jpgs = video[0]
    tricky = jpgs[1][:2] + b"\xff\xe1\x00\x08\xff\xd8\xff\xd9\xff\xd8" + jpgs[1][2:]      # FF D8 / FF D9 inside an APP1 payload
    for ext in (".mjpeg", ".mjpg"):
        path = str(tmp_path / ("clip" + ext))
        jpeg_ref.write_mjpeg(path, [jpgs[0], tricky, jpgs[2], jpgs[0]])
        _check_reader(fd.open_video(path), [0, 1, 2, 0], video, None)


@pytest.mark.parametrize("idx1", [True, False])
def test_avi(tmp_path, video, idx1):
    jpgs = video[0]
    path = str(tmp_path / "clip.avi")
    jpeg_ref.write_avi(path, [jpgs[0], jpgs[1], b"", jpgs[2]], 64, 48, rate=30000, scale=1001, idx1=idx1)
    _check_reader(fd.open_video(path), [0, 1, 1, 2], video, 30000 / 1001)
    jpeg_ref.write_avi(path, [jpgs[2], jpgs[0]], 64, 48, rate=25, scale=1, idx1=idx1, handler=b"mjpg", compression=b"MJPG")
    _check_reader(fd.open_video(path), [2, 0], video, 25.0)


def test_directory_in_natural_order(tmp_path, video):
    jpgs = video[0]
    path = str(tmp_path / "frames")
    jpeg_ref.write_dir(path, [jpgs[0], jpgs[1], jpgs[2]], names=["10.jpg", "2.jpg", "1.JPEG"])
    open(os.path.join(path, "notes.txt"), "w").write("not a frame")
    _check_reader(fd.open_video(path), [2, 1, 0], video, None)


def test_an_avi_of_another_codec_goes_the_old_way(tmp_path, video, monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "decord", None)
    monkeypatch.setitem(sys.modules, "cv2", None)
    path = str(tmp_path / "clip.avi")
    jpeg_ref.write_avi(path, [b"\x00\x00\x01\xb6" + bytes(20)], 64, 48, handler=b"XVID", compression=b"XVID")
    with pytest.raises(ImportError, match="decord or OpenCV"):
        fd.open_video(path)
    open(path, "wb").write(b"not a RIFF file at all")
    with pytest.raises(ImportError, match="decord or OpenCV"):
        fd.open_video(path)


def test_bad_frames_are_value_errors_naming_file_and_frame(tmp_path, video, cases):
    jpgs = video[0]
    other = cases["odd_jpg"].tobytes()
    path = str(tmp_path / "clip.mjpeg")
    jpeg_ref.write_mjpeg(path, [jpgs[0], jpgs[1], other])
    with pytest.raises(ValueError, match=r"clip\.mjpeg: frame 2: a frame of 70 x 45 in a video of 64 x 48"):
        fd.open_video(path)
    jpeg_ref.write_mjpeg(path, [jpgs[0], jpgs[1], jpgs[2][:-40]])
    with pytest.raises(ValueError, match=r"clip\.mjpeg: frame 2 "):
        fd.open_video(path)
    jpeg_ref.write_mjpeg(path, [jpgs[0], cases["progressive_jpg"].tobytes()])
    with pytest.raises(ValueError, match=r"clip\.mjpeg: frame 1: .*progressive"):
        fd.open_video(path)
    avi = str(tmp_path / "clip.avi")
    jpeg_ref.write_avi(avi, [jpgs[0], jpgs[1][:-40]], 64, 48)
    with pytest.raises(ValueError, match=r"clip\.avi: frame 1: "):
        fd.open_video(avi)
    jpeg_ref.write_avi(avi, [b"", jpgs[1]], 64, 48)
    with pytest.raises(ValueError, match=r"clip\.avi: frame 0: a zero-length chunk"):
        fd.open_video(avi)
    d = str(tmp_path / "frames")
    jpeg_ref.write_dir(d, [jpgs[0], other], names=["a1.jpg", "a2.jpg"])
    with pytest.raises(ValueError, match=r"a2\.jpg: frame 1: a frame of 70 x 45"):
        fd.open_video(d)
    empty = str(tmp_path / "empty")
    os.makedirs(empty)
    with pytest.raises(ValueError, match=r"empty: frame 0: the directory holds no"):
        fd.open_video(empty)
    # a frame whose entropy data is damaged passes the probe and fails where it is decoded, naming file and frame
    b = bytearray(jpgs[1])
    b[-30:-2] = b"\xff\xd5" * 14
    jpeg_ref.write_mjpeg(path, [jpgs[0], bytes(b)])
    r = fd.open_video(path)
    with pytest.raises(ValueError, match=r"clip\.mjpeg: frame 1: kvq_jpeg_coeffs: "):
        r[1]


def test_the_encoder_of_the_restatement_round_trips():
    """tests/jpeg_ref.py's entropy encoder (the many-frame GPU tests use it): its streams decode to the coefficients they were made of,
    by the library and by the restatement, with and without restart markers and DHT segments"""
    H, W = 33, 17
    coef, qt = jpeg_ref.synthetic_coefficients(5, 2, H, W)
    for t, (restart, dht) in enumerate(((0, True), (1, False))):
        data = np.frombuffer(jpeg_ref.encode_baseline(coef[t], qt[t], H, W, restart=restart, dht=dht), np.uint8)
        c2, q2, p = jpeg_ref.decode_coeffs(data.tobytes())
        assert np.array_equal(c2, coef[t]) and np.array_equal(q2, qt[t]) and p["ri"] == restart
        rc, got, got_qt = lib_decode(data)
        assert rc == OK and np.array_equal(got, coef[t]) and np.array_equal(got_qt, qt[t])


def test_abi_surface():
    header = open(os.path.join(ROOT, "include", "kvq_hip.h")).read()
    handle = _abi.lib()
    for name in ("kvq_jpeg_coef_bytes", "kvq_jpeg_probe", "kvq_jpeg_coeffs", "kvq_jpeg_idct_i420_host", "kvq_jpeg_idct_i420"):
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _abi.SYMBOLS and hasattr(handle, name)
    assert "typedef struct KvqJpegInfo" in header and C.sizeof(_abi.KvqJpegInfo) == 64
    assert handle.kvq_abi_version() == _abi.ABI_VERSION == 32 and "#define KVQ_ABI_VERSION 32" in header
    assert handle.kvq_jpeg_coef_bytes(16, 16) == 768 and handle.kvq_jpeg_coef_bytes(0, 16) == 0
    buf = np.zeros(16, np.uint8)
    assert handle.kvq_jpeg_idct_i420(None, None, 1, 16, 16, None, None) == -1
    assert handle.kvq_jpeg_idct_i420_host(buf.ctypes.data, buf.ctypes.data, 0, 16, 16, buf.ctypes.data) == ERR_SHAPE
