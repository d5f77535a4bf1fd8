"""CPU: the host half of the Motion-JPEG writer (csrc/jpeg_fdct.hpp, csrc/jpeg_enc.cpp) against its restatement
(tests/jpeg_enc_ref.py) and against libjpeg through the Pillow-made fixtures of tests/golden/mjpeg_enc.npz: the quantiser's reciprocal
form over its whole range, the scalar twin of the forward-DCT launch, the entropy coder byte for byte, its refusals, a foreign decoder,
the three containers through ``open_video`` and the ABI surface."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
import torch

import kvq_amd  # noqa: F401
from kvq_amd import _abi, kernels
from kvq_amd.datasets import fusion_datasets as fd

import jpeg_enc_ref
import jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(16, 16), (7, 9), (45, 70), (33, 17), (48, 64)]
ALIGNED = ["noise_32x48_q5", "noise_32x48_q50", "noise_32x48_q100", "picture_48x64_q30", "picture_48x64_q95", "noise_16x16_q75", "noise_64x80_q85"]
UNALIGNED = ["picture_45x70_q90", "picture_7x9_q90", "picture_33x17_q75", "noise_24x40_q100"]
OK, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -3, -4
NEW_SYMBOLS = ["kvq_jpeg_quant_tables", "kvq_jpeg_quantise_host", "kvq_jpeg_fdct_host", "kvq_jpeg_fdct", "kvq_jpeg_encode_bound", "kvq_jpeg_encode"]


@pytest.fixture(scope="module")
def cases(golden):
    g = golden("mjpeg_enc.npz")
    assert g["aligned"].tolist() == ALIGNED and g["unaligned"].tolist() == UNALIGNED
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def analysed(cases):
    """name -> (H, W, libjpeg's coefficients (blocks, 64), its tables (3, 64), the host twin's coefficients of the RGB input)"""
    out = {}
    for name in ALIGNED + UNALIGNED:
        rgb = cases[name + "_rgb"]
        H, W = rgb.shape[:2]
        data = cases[name + "_jpg"]
        want = np.empty(kernels.jpeg_coef_bytes(H, W) // 2, np.int16)
        qt = np.empty((3, 64), np.uint16)
        rc, msg = kernels.jpeg_coeffs(data, want, qt)
        assert rc == OK, msg
        got = kernels.jpeg_fdct_host(np.ascontiguousarray(rgb.transpose(2, 0, 1)[:, None]), qt, H, W)[0]
        out[name] = (H, W, want.reshape(-1, 64), qt, got.reshape(-1, 64))
    return out


def lib_encode(coef, qt, H, W, restart=0, flags=0, cap=None, canary=64):
    """kvq_jpeg_encode into a buffer of ``cap`` bytes (None: the bound) -> (rc, n, bytes written); asserts the canary behind cap is untouched"""
    coef, qt = np.ascontiguousarray(coef, np.int16), np.ascontiguousarray(qt, np.uint16)
    cap = kernels.jpeg_encode_bound(H, W) if cap is None else cap
    buf = np.full(cap + canary, 0xA5, np.uint8)
    n = C.c_size_t(0)
    rc = _abi.lib().kvq_jpeg_encode(coef.ctypes.data, qt.ctypes.data, H, W, restart, flags, buf.ctypes.data, cap, C.byref(n))
    assert (buf[cap:] == 0xA5).all()
    return rc, n.value, buf[:min(n.value, cap)].tobytes()


def test_the_reciprocal_quantiser_equals_the_division_over_its_whole_range():
    F = np.arange(-32767, 32768, dtype=np.int32)
    for q in range(1, 256):
        assert np.array_equal(kernels.jpeg_quantise_host(F, q), jpeg_enc_ref.quantise(F, q)), q
    rc = _abi.lib().kvq_jpeg_quantise_host(F.ctypes.data, F.size, 256, np.empty(F.size, np.int16).ctypes.data)
    assert rc == ERR_SHAPE


@pytest.mark.parametrize("quality", [1, 5, 24, 25, 49, 50, 51, 75, 90, 99, 100])
def test_quant_tables_equal_the_restatement(quality):
    qt = kernels.jpeg_quant_tables(quality)
    assert qt.dtype == np.uint16 and np.array_equal(qt, jpeg_enc_ref.quant_tables(quality))
    assert qt.min() >= 1 and qt.max() <= 255 and (quality != 100 or (qt == 1).all())


def test_quant_tables_refuse_a_quality_outside_1_to_100():
    out = np.zeros((3, 64), np.uint16)
    for q in (0, 101, -3):
        assert _abi.lib().kvq_jpeg_quant_tables(q, out.ctypes.data) == ERR_SHAPE
    assert _abi.lib().kvq_jpeg_quant_tables(50, None) == ERR_NULL


def _sources(H, W, T, seed, kind):
    """(rgb uint8 (3, T, H, W), I420 frames uint8 (T, frame_bytes)) — random, all 0 or all 255"""
    g = np.random.Generator(np.random.PCG64(seed))
    fb = jpeg_ref.frame_bytes(H, W)
    if kind == "random":
        return g.integers(0, 256, (3, T, H, W), dtype=np.uint8), g.integers(0, 256, (T, fb), dtype=np.uint8)
    v = 0 if kind == "zeros" else 255
    return np.full((3, T, H, W), v, np.uint8), np.full((T, fb), v, np.uint8)


@pytest.mark.parametrize("kind", ["random", "zeros", "ones"])
@pytest.mark.parametrize("H,W", SIZES)
def test_fdct_host_equals_the_restatement(H, W, kind):
    T = 1 + (H + W) % 3
    g = np.random.Generator(np.random.PCG64(H * 1000 + W))
    qt = np.stack([kernels.jpeg_quant_tables(int(q)) for q in g.integers(1, 101, T)])
    qt[0] = g.integers(1, 256, (3, 64))                                                   # any 8-bit table, not only the scaled Annex K ones
    rgb, i420 = _sources(H, W, T, H * 100 + W, kind)
    for src, fmt in ((rgb, _abi.SRC_U8), (i420, _abi.SRC_I420_BT601_FULL)):
        got = kernels.jpeg_fdct_host(src, qt, H, W, fmt)
        want = jpeg_enc_ref.fdct(src, fmt, T, H, W, qt)
        assert got.shape == want.shape == (T, jpeg_ref.coef_bytes(H, W) // 2) and np.array_equal(got, want), (fmt, np.count_nonzero(got != want))
    if kind != "random":                                                                  # a flat picture: DC only, the same in every block
        blocks = got.reshape(T, -1, 64)
        assert not blocks[:, :, 1:].any() and (blocks[:, :, 0] != 0).all()


def test_fdct_host_refusals():
    lib = _abi.lib()
    src, qt, out = np.zeros(3 * 256, np.uint8), np.ones(192, np.uint16), np.zeros(6 * 64, np.int16)
    call = lambda fmt, T, H, W, s=src: lib.kvq_jpeg_fdct_host(s.ctypes.data, fmt, T, H, W, qt.ctypes.data, out.ctypes.data)    # noqa: E731
    for fmt in (_abi.SRC_F32, _abi.SRC_I420_BT601_LIMITED, _abi.SRC_I420_BT709_LIMITED, _abi.SRC_I420_BT709_FULL, 9):
        assert call(fmt, 1, 16, 16) == ERR_UNSUPPORTED and f"format {fmt}" in lib.kvq_last_error().decode()
    assert call(_abi.SRC_U8, 0, 16, 16) == ERR_SHAPE and call(_abi.SRC_U8, 1, 0, 16) == ERR_SHAPE and call(_abi.SRC_U8, 1, 16, 65536) == ERR_SHAPE
    assert lib.kvq_jpeg_fdct_host(None, _abi.SRC_U8, 1, 16, 16, qt.ctypes.data, out.ctypes.data) == ERR_NULL
    assert lib.kvq_jpeg_fdct(None, _abi.SRC_U8, 1, 16, 16, None, None, None) == ERR_NULL             # checked before any HIP call


@pytest.mark.parametrize("name", ALIGNED)
def test_aligned_fixture_every_coefficient_equals_libjpeg(cases, analysed, name):
    H, W, want, qt, got = analysed[name]
    assert H % 16 == 0 and W % 16 == 0
    assert np.array_equal(qt, kernels.jpeg_quant_tables(int(cases[name + "_q"])))
    assert np.array_equal(got, want), np.count_nonzero(got != want)


@pytest.mark.parametrize("name", UNALIGNED)
def test_unaligned_fixture_every_block_of_the_picture_equals_libjpeg(cases, analysed, name):
    H, W, want, qt, got = analysed[name]
    assert np.array_equal(qt, kernels.jpeg_quant_tables(int(cases[name + "_q"])))
    mask = jpeg_enc_ref.picture_blocks(H, W)
    assert 0 < mask.sum() < mask.size
    assert np.array_equal(got[mask], want[mask]), np.count_nonzero(got[mask] != want[mask])


def _clipped_synthetic(seed, H, W):
    coef, qt = jpeg_ref.synthetic_coefficients(seed, 1, H, W)
    coef = np.clip(coef[0], -1023, 1023)
    coef[:, 0] = np.clip(coef[:, 0], -1000, 1000)                                         # DC differences within +-2047
    return coef, np.clip(qt[0], 1, 255)


@pytest.mark.parametrize("restart,dht", [(0, True), (0, False), (1, True), (3, False), (5, True)])
@pytest.mark.parametrize("H,W", [(16, 16), (45, 70), (48, 64)])
def test_encode_equals_the_restatement_and_decodes_to_its_input(H, W, restart, dht):
    coef, qt = _clipped_synthetic(H + W + restart, H, W)
    rc, n, got = lib_encode(coef, qt, H, W, restart, 0 if dht else _abi.JPEG_NO_DHT)
    assert rc == OK and n == len(got) <= kernels.jpeg_encode_bound(H, W)
    assert got == jpeg_enc_ref.encode(coef, qt, H, W, restart=restart, dht=dht)
    assert (b"\xff\xc4" in got[:700]) == dht and got[:2] == b"\xff\xd8" and got[2:20] == jpeg_enc_ref.APP0 and got[-2:] == b"\xff\xd9"
    data = np.frombuffer(got, np.uint8)
    rc, info, msg = kernels.jpeg_probe(data)
    assert rc == OK and (info.height, info.width, info.restart_interval, info.has_dht, info.frame_bytes) == (H, W, restart, int(dht), n), msg
    back, qt_back = np.empty(coef.size, np.int16), np.empty((3, 64), np.uint16)
    rc, msg = kernels.jpeg_coeffs(data, back, qt_back)
    assert rc == OK and np.array_equal(back.reshape(-1, 64), coef) and np.array_equal(qt_back, qt), msg
    assert np.array_equal(kernels.jpeg_encode(np.ascontiguousarray(coef), np.ascontiguousarray(qt), H, W, restart, dht), data)


@pytest.mark.parametrize("name", ALIGNED + UNALIGNED)
def test_encode_fixture_cases(analysed, name):
    H, W, _, qt, coef = analysed[name]
    rc, n, got = lib_encode(coef, qt, H, W)
    assert rc == OK and got == jpeg_enc_ref.encode(coef, qt, H, W)
    back, qt_back = np.empty(coef.size, np.int16), np.empty((3, 64), np.uint16)
    rc, msg = kernels.jpeg_coeffs(np.frombuffer(got, np.uint8), back, qt_back)
    assert rc == OK and np.array_equal(back.reshape(-1, 64), coef) and np.array_equal(qt_back, qt), msg


def test_encode_bound_holds_for_the_densest_block():
    """every AC coefficient in category 10 behind the longest codes, DC differences in category 11, 0xFF bytes stuffed"""
    H, W = 32, 16
    coef = np.full((12, 64), -1023, np.int16)
    coef[:, 0] = np.where(np.arange(12) % 2, -1023, 1023)
    rc, n, got = lib_encode(coef, np.full((3, 64), 255, np.uint16), H, W, restart=1)
    assert rc == OK and n <= kernels.jpeg_encode_bound(H, W)
    assert _abi.lib().kvq_jpeg_encode_bound(0, 16) == 0 and _abi.lib().kvq_jpeg_encode_bound(16, 65536) == 0


def test_encode_refusals():
    lib = _abi.lib()
    H, W = 16, 32
    coef, qt = _clipped_synthetic(3, H, W)
    rc, n, whole = lib_encode(coef, qt, H, W)
    assert rc == OK
    for cap in (0, 1, 19, 300, n - 1):                                                    # short capacity: the canary is checked by lib_encode
        rc, need, _ = lib_encode(coef, qt, H, W, cap=cap)
        assert rc == ERR_WORKSPACE and need == n and "needs" in lib.kvq_last_error().decode()
    assert lib_encode(coef, qt, H, W, cap=n)[0] == OK
    bad = coef.copy()
    bad[7, 5] = 1024                                                                      # an AC coefficient of category 11
    rc, _, _ = lib_encode(bad, qt, H, W)
    assert rc == ERR_UNSUPPORTED and "block 7" in lib.kvq_last_error().decode()
    bad = coef.copy()
    bad[8, 0], bad[9, 0] = -1100, 1100                                                    # the Cb blocks (8 Y blocks before them): the first DC
    rc, _, _ = lib_encode(bad, qt, H, W)                                                  # fits as a difference to 0, the second to the first not
    assert rc == ERR_UNSUPPORTED and "DC difference 2200 (plane 1, block 1)" in lib.kvq_last_error().decode()
    for v in (0, 256):
        q = qt.copy()
        q[2, 63] = v
        assert lib_encode(coef, q, H, W)[0] == ERR_UNSUPPORTED and "table 2, entry 63" in lib.kvq_last_error().decode()
    assert lib_encode(coef, qt, H, W, restart=65536)[0] == ERR_SHAPE and lib_encode(coef, qt, H, W, flags=2)[0] == ERR_SHAPE
    assert lib_encode(coef, qt, 0, W, cap=64)[0] == ERR_SHAPE
    c, q, o, k = np.ascontiguousarray(coef), np.ascontiguousarray(qt), np.zeros(64, np.uint8), C.c_size_t(0)
    for args in ((None, q.ctypes.data, o.ctypes.data, C.byref(k)), (c.ctypes.data, None, o.ctypes.data, C.byref(k)),
                 (c.ctypes.data, q.ctypes.data, None, C.byref(k)), (c.ctypes.data, q.ctypes.data, o.ctypes.data, None)):
        assert lib.kvq_jpeg_encode(args[0], args[1], H, W, 0, 0, args[2], 64, args[3]) == ERR_NULL


@pytest.mark.parametrize("ac_fault", [True, False])
def test_encode_names_the_first_value_without_a_baseline_code_in_coding_order(ac_fault):
    """one MCU (six blocks).  Block 1's DC difference has category 12; with ``ac_fault`` block 0 also carries AC values of category 11 at
    zigzag positions 5 and 9, and block 0, position 5 comes first in coding order"""
    lib = _abi.lib()
    H = W = 16
    coef = np.zeros((6, 64), np.int16)
    coef[1:4, 0] = 2048                                                                   # Y01 against Y00's 0; Y10, Y11 repeat it: difference 0
    if ac_fault:
        coef[0, jpeg_ref.ZIGZAG[5]], coef[0, jpeg_ref.ZIGZAG[9]] = -1500, 1024
    rc, n, _ = lib_encode(coef, kernels.jpeg_quant_tables(50), H, W)
    msg = lib.kvq_last_error().decode()
    assert rc == ERR_UNSUPPORTED and n == 0
    if ac_fault:
        assert msg == "kvq_jpeg_encode: coefficient -1500 (plane 0, block 0, zigzag position 5) is outside baseline's +-1023", msg
    else:
        assert msg == "kvq_jpeg_encode: DC difference 2048 (plane 0, block 1) is outside baseline's +-2047", msg


@pytest.mark.parametrize("name", UNALIGNED)
def test_a_foreign_decoder_opens_what_the_library_writes(analysed, name):
    Image = pytest.importorskip("PIL.Image")
    H, W, _, qt, coef = analysed[name]
    data = kernels.jpeg_encode(np.ascontiguousarray(coef.reshape(-1)), qt, H, W)
    im = Image.open(io.BytesIO(data.tobytes()))
    assert im.size == (W, H) and im.format == "JPEG"
    im.draft("YCbCr", im.size)
    assert im.mode == "YCbCr"
    theirs = np.asarray(im)[..., 0].astype(np.int16)
    ours = kernels.jpeg_idct_i420_host(coef.reshape(1, -1), qt[None], H, W)[0][:H * W].reshape(H, W).astype(np.int16)
    d = int(np.abs(theirs - ours).max())
    print(f"{name}: largest difference of libjpeg's Y to the library's IDCT of the same stream: {d}")
    assert d <= 1


# ---- containers -----------------------------------------------------------------------------------------------------------------
def _video(T, H, W, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([255.0 * x / (W - 1), 255.0 * y / (H - 1), 127.0 + 0 * x])
    return np.clip(base[:, None] + g.normal(0, 20, (3, T, H, W)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("ext,fps", [(".mjpeg", 25.0), (".avi", 29.97), (".avi", 2.0), ("_frames", 30.0)])
def test_writer_containers_read_back_through_open_video(tmp_path, ext, fps):
    T, H, W = 5, 45, 70
    rgb = _video(T, H, W, 1)
    path = str(tmp_path / ("clip" + ext))
    qt = kernels.jpeg_quant_tables(80)
    coef = kernels.jpeg_fdct_host(rgb, qt, H, W)
    with fd.MjpegWriter(path, fps, quality=80, restart_interval=2) as w:
        w.write_coefficients(coef[:2], H, W)                  # the host-only path ...
        w.write(torch.from_numpy(rgb[:, 2:]))                 # ... and host frames through the scalar twin
        with pytest.raises(ValueError, match="70 x 45"):
            w.write_coefficients(np.zeros((1, 6 * 64), np.int16), 16, 16)
    assert w.frames == T
    vr = fd.open_video(path)
    assert isinstance(vr, fd.MjpegFrameReader) and (len(vr), vr.H, vr.W) == (T, H, W)
    assert vr.fps == (fps if ext == ".avi" else None)
    back, qt_back = np.empty((T, coef.shape[1]), np.int16), np.empty((T, 3, 64), np.uint16)
    vr.read_jpeg_into(range(T), back, qt_back)
    assert np.array_equal(back, coef) and (qt_back == qt[None]).all()
    want = kernels.jpeg_idct_i420_host(coef, np.broadcast_to(qt, (T, 3, 64)), H, W)
    for i in range(T):
        assert np.array_equal(vr.i420(i), want[i])
    if ext == "_frames":
        assert sorted(os.listdir(path)) == ["%06d.jpg" % i for i in range(T)]
    if ext == ".avi":
        hdr = fd._avi_index(path)
        assert (hdr["handler"], hdr["compression"], hdr["W"], hdr["H"]) == (b"MJPG", b"MJPG", W, H) and len(hdr["frames"]) == T
        size = os.path.getsize(path)
        raw = open(path, "rb").read()
        assert int.from_bytes(raw[4:8], "little") == size - 8 and raw.count(b"idx1") == 1
        assert fd.MjpegFrameReader(path)._index == [(path, o, n) for o, n in hdr["frames"]]
    with pytest.raises(ValueError, match="after close"):
        w.write_coefficients(coef[:1], H, W)


def test_writer_refuses_an_avi_past_the_limit_before_the_frame_is_written(tmp_path, monkeypatch):
    T, H, W = 4, 32, 48
    coef = kernels.jpeg_fdct_host(_video(T, H, W, 2), kernels.jpeg_quant_tables(90), H, W)
    path = str(tmp_path / "big.avi")
    w = fd.MjpegWriter(path, 10, quality=90)
    w.write_coefficients(coef[:2], H, W)
    size = w._file.tell()
    monkeypatch.setattr(fd.MjpegWriter, "AVI_LIMIT", size + 200)      # room for the index, not for another frame
    with pytest.raises(ValueError, match="OpenDML"):
        w.write_coefficients(coef[2:], H, W)
    assert w._file.tell() == size and w.frames == 2
    w.close()
    vr = fd.open_video(path)
    assert len(vr) == 2 and vr.fps == 10 and os.path.getsize(path) <= fd.MjpegWriter.AVI_LIMIT


def test_writer_refuses_other_i420_formats_and_odd_arguments(tmp_path):
    H, W = 16, 16
    frames = torch.zeros(1, kernels.i420_frame_bytes(H, W), dtype=torch.uint8)
    with fd.MjpegWriter(str(tmp_path / "a.mjpeg"), 25) as w:
        for fmt in (_abi.SRC_I420_BT601_LIMITED, _abi.SRC_I420_BT709_LIMITED, _abi.SRC_I420_BT709_FULL):
            with pytest.raises(ValueError, match=r"to_rgb\(\)"):
                w.write(kernels.I420Frames(frames, H, W, fmt))
        with pytest.raises(ValueError, match="uint8"):
            w.write(torch.zeros(3, 1, H, W))
        w.write(kernels.I420Frames(frames, H, W, _abi.SRC_I420_BT601_FULL))
    assert len(fd.open_video(str(tmp_path / "a.mjpeg"))) == 1
    with pytest.raises(ValueError, match="fps"):
        fd.MjpegWriter(str(tmp_path / "b.mjpeg"), 0)
    with pytest.raises(_abi.KvqError, match="quality"):
        fd.MjpegWriter(str(tmp_path / "c.mjpeg"), 25, quality=0)


def test_transcode_tool_writes_what_the_writer_writes(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("transcode_mjpeg", os.path.join(ROOT, "tools", "transcode_mjpeg.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    T, H, W = 3, 33, 17
    rgb = _video(T, H, W, 3)
    np.save(tmp_path / "clip.npy", np.ascontiguousarray(rgb.transpose(1, 2, 3, 0)))
    n = tool.transcode(str(tmp_path / "clip.npy"), str(tmp_path / "clip.avi"), quality=70, fps=12.5, device="cpu")
    vr = fd.open_video(str(tmp_path / "clip.avi"))
    assert n == len(vr) == T and vr.fps == 12.5
    coef = kernels.jpeg_fdct_host(rgb, kernels.jpeg_quant_tables(70), H, W)
    back, qt = np.empty_like(coef), np.empty((T, 3, 64), np.uint16)
    vr.read_jpeg_into(range(T), back, qt)
    assert np.array_equal(back, coef)
    m = tool.transcode(str(tmp_path / "clip.avi"), str(tmp_path / "again.mjpeg"), quality=70, fps=None, device="cpu")   # MJPEG in: I420 frames
    assert m == T and len(fd.open_video(str(tmp_path / "again.mjpeg"))) == T


# ---- harness: the yml keys and the file writer ------------------------------------------------------------------------------
def _bare_trainer(config):
    from kvq_amd.trainer import Trainer
    t = Trainer.__new__(Trainer)
    t.config = config
    return t


def test_overlay_video_yml_keys_parse_beside_quality_maps():
    import yaml
    qm = {"dir": "x", "overlay_frames": 2, "overlay_video": "avi", "overlay_quality": 75}
    t = _bare_trainer({"quality_maps": qm})
    assert t._quality_maps() == {"dir": "x", "cell": 8, "overlay_frames": 2}              # as before: the new keys are not part of it
    assert t._overlay_video() == {"ext": "avi", "quality": 75}
    assert _bare_trainer({"quality_maps": dict(qm, overlay_video="MJPEG")})._overlay_video() == {"ext": "mjpeg", "quality": 75}
    assert _bare_trainer({"quality_maps": {"dir": "x", "overlay_frames": 1, "overlay_video": "jpg"}})._overlay_video() == {"ext": "jpg", "quality": 90}
    for cfg in ({}, {"quality_maps": None}, {"quality_maps": {"dir": "x", "overlay_frames": 2}}):
        assert _bare_trainer(cfg)._overlay_video() is None
    yml = yaml.safe_load(open(os.path.join(ROOT, "config", "kwai_swin_grpb_qmap_test.yml")))
    assert _bare_trainer(yml)._overlay_video() is None and _bare_trainer(yml)._quality_maps() == {"dir": "quality_maps", "cell": 8, "overlay_frames": 0}
    assert "overlay_video" in open(os.path.join(ROOT, "config", "kwai_swin_grpb_qmap_test.yml")).read()     # documented there, as a comment
    for bad in (dict(qm, overlay_video="mp4"), dict(qm, overlay_quality=0), dict(qm, overlay_quality=101), dict(qm, overlay_frames=0)):
        with pytest.raises(ValueError):
            _bare_trainer({"quality_maps": bad})._overlay_video()
    with pytest.raises(ValueError):
        _bare_trainer({"quality_maps": dict(qm, colour=1)})._quality_maps()


@pytest.mark.parametrize("ext", ["avi", "mjpeg", "jpg"])
def test_map_writer_puts_the_overlay_coefficients_into_a_video(tmp_path, ext):
    H, W, n_clips, n_ov, D = 33, 17, 2, 2, 4
    cfgqm = {"dir": str(tmp_path / "maps"), "overlay_frames": n_ov, "overlay_video": ext, "overlay_quality": 60}
    t = _bare_trainer({"model": {"type": "swin_tiny_grpb"}, "quality_maps": cfgqm})
    rgb = _video(n_clips * n_ov, H, W, 5)
    coef = kernels.jpeg_fdct_host(rgb, kernels.jpeg_quant_tables(60), H, W)
    tok = torch.arange(n_clips * D * 7 * 7, dtype=torch.float32).reshape(n_clips, D, 7, 7)
    host = {"pred": torch.tensor([[1.0], [2.0]]), "swin_tiny_grpb/token_map": tok, "swin_tiny_grpb/timeline": tok.mean((2, 3)),
            "swin_tiny_grpb/overlay_coef": torch.from_numpy(coef).reshape(n_clips, n_ov, -1), "score": 1.5}
    fi = np.arange(n_clips * D * 2) * 3
    path = t._maps_write(t._quality_maps(), "clips/video_7.mp4", host, {"frame_inds": fi, "overlay_size": (H, W)})
    z = np.load(path)
    assert set(z.files) == {"score", "token_map", "timeline", "frame_inds", "overlay_frame_inds"}
    assert np.array_equal(z["overlay_frame_inds"], fi.reshape(n_clips, D, 2)[:, [1, 3], 0])
    assert sorted(os.listdir(tmp_path / "maps")) == ["video_7.mp4.npz", f"video_7.mp4.overlay.{ext}"]
    vr = fd.open_video(str(tmp_path / "maps" / f"video_7.mp4.overlay.{ext}"))
    assert (len(vr), vr.H, vr.W) == (n_clips * n_ov, H, W) and vr.fps == (2.0 if ext == "avi" else None)
    back, qt = np.empty_like(coef), np.empty((n_clips * n_ov, 3, 64), np.uint16)
    vr.read_jpeg_into(range(n_clips * n_ov), back, qt)
    assert np.array_equal(back, coef)


# ---- ABI --------------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "kvq_hip.h")).read()
    declared = set(re.findall(r"\b(kvq_[a-z0-9_]+)\s*\(", header))
    handle = _abi.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _abi.SYMBOLS and hasattr(handle, name), name
    assert "KVQ_JPEG_NO_DHT = 1" in header and _abi.JPEG_NO_DHT == 1
    assert handle.kvq_abi_version() == _abi.ABI_VERSION == 32 and "#define KVQ_ABI_VERSION 32" in header
    from kvq_amd import _build
    assert {"jpeg_enc.cpp", "jpeg_enc.hip"} <= set(_build.SOURCES)
