"""CPU: the YUV 4:2:0 -> RGB conversion's integers (kvq_yuv420_coeffs against (Kr, Kb), tests/yuv_ref.py against the rounded float64
conversion over every byte triplet), the Y4M reader, and the ABI surface the I420 source formats add (nothing existing moves)."""
import ctypes as C

import numpy as np
import pytest

import kvq_amd  # noqa: F401
from kvq_amd import _abi, kernels
from kvq_amd.datasets import fusion_datasets as fd

import yuv_ref

FORMAT_NAMES = {2: ("bt601", False), 3: ("bt601", True), 4: ("bt709", False), 5: ("bt709", True)}


@pytest.mark.parametrize("fmt", yuv_ref.FORMATS)
def test_coefficients_are_the_rounded_kr_kb_matrix(fmt):
    out = (C.c_int32 * 6)()
    assert _abi.lib().kvq_yuv420_coeffs(fmt, C.byref(out)) == 0
    assert tuple(out) == yuv_ref.coeffs(fmt) == kernels.yuv420_coeffs(fmt)
    matrix, full = FORMAT_NAMES[fmt]
    assert _abi.i420_format(matrix, full) == fmt and fmt in _abi.I420_FORMATS
    # worst case of every sum stays inside int32
    qy, qrv, qgu, qgv, qbu, yoff = yuv_ref.coeffs(fmt)
    worst = abs(qy) * 255 + 32768 + 128 * max(abs(qrv), abs(qgu) + abs(qgv), abs(qbu))
    assert worst < 2 ** 31


def test_coefficient_entry_rejects_other_formats():
    out = (C.c_int32 * 6)()
    for fmt in (-1, 0, 1, 6):
        assert _abi.lib().kvq_yuv420_coeffs(fmt, C.byref(out)) == -3
    assert _abi.lib().kvq_yuv420_coeffs(2, None) == -1
    with pytest.raises(ValueError, match="bt601"):
        _abi.i420_format("bt2020")


@pytest.mark.parametrize("fmt", yuv_ref.FORMATS)
def test_integer_conversion_is_within_one_of_the_rounded_float_conversion(fmt):
    """all 2^24 (Y, U, V) triplets: |integer - floor(float64 + 0.5)| <= 1, and they differ in fewer than 3e-4 of the values"""
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst, differ = 0, 0
    for y in range(256):
        d = np.abs(yuv_ref.convert(y, u, v, fmt).astype(np.int16) - yuv_ref.convert_float(y, u, v, fmt).astype(np.int16))
        worst, differ = max(worst, int(d.max())), differ + int(np.count_nonzero(d))
    assert worst <= 1
    assert differ / (3 * 2 ** 24) < 3e-4


@pytest.mark.parametrize("fmt", yuv_ref.FORMATS)
def test_host_conversion_of_the_package_equals_the_reference(fmt):
    H, W = 5, 7
    frame = yuv_ref.random_frames(3, 1, H, W)[0]
    got = fd.yuv420_to_rgb_host(*yuv_ref.planes(frame, H, W), kernels.yuv420_coeffs(fmt))
    assert got.dtype == np.uint8 and np.array_equal(got, yuv_ref.frame_rgb(frame, H, W, fmt))


@pytest.mark.parametrize("H,W", [(16, 24), (15, 24), (16, 23), (9, 13), (1, 1)])
@pytest.mark.parametrize("chroma", ["C420", "C420jpeg", "C420mpeg2", "C420paldv", None])
def test_y4m_round_trip(tmp_path, H, W, chroma):
    T = 5
    frames = yuv_ref.random_frames(H * 100 + W, T, H, W)
    path = str(tmp_path / "clip.y4m")
    yuv_ref.write_y4m(path, frames, H, W, chroma=chroma)
    r = fd.open_video(path)
    assert isinstance(r, fd.Y4mFrameReader) and len(r) == T and (r.H, r.W) == (H, W)
    assert r.format == _abi.SRC_I420_BT601_LIMITED and r.frame_bytes == yuv_ref.frame_bytes(H, W) == kernels.i420_frame_bytes(H, W)
    for i in range(T):
        rgb = r[i]
        assert rgb.shape == (H, W, 3) and rgb.dtype == np.uint8
        assert np.array_equal(rgb, yuv_ref.frame_rgb(frames[i], H, W, r.format))
    idx = [4, 0, 0, 3]
    out = np.zeros((len(idx), r.frame_bytes), np.uint8)
    r.read_i420_into(idx, out)
    assert np.array_equal(out, frames[idx])


@pytest.mark.parametrize("matrix,extra,fmt", [("bt601", ("XCOLORRANGE=FULL",), 3), ("bt709", (), 4), ("bt709", ("XYSCSS=420JPEG", "XCOLORRANGE=FULL"), 5),
                                              ("bt601", ("XCOLORRANGE=LIMITED",), 2)])
def test_y4m_range_tag_and_matrix_select_the_format(tmp_path, matrix, extra, fmt):
    H, W = 6, 10
    frames = yuv_ref.random_frames(9, 2, H, W)
    path = str(tmp_path / "clip.y4m")
    yuv_ref.write_y4m(path, frames, H, W, extra=extra, frame_header=b"FRAME Ip\n")      # frame parameters are legal
    r = fd.open_video(path, yuv_matrix=matrix)
    assert r.format == fmt and len(r) == 2
    assert np.array_equal(r[1], yuv_ref.frame_rgb(frames[1], H, W, fmt))


@pytest.mark.parametrize("tag", ["C422", "C444", "C420p10", "Cmono"])
def test_y4m_rejects_other_chroma_formats_by_name(tmp_path, tag):
    path = str(tmp_path / "clip.y4m")
    yuv_ref.write_y4m(path, yuv_ref.random_frames(1, 2, 8, 8), 8, 8, chroma=tag)
    with pytest.raises(ValueError, match=tag):
        fd.open_video(path)


def test_y4m_rejects_truncated_and_malformed_files(tmp_path):
    H, W = 8, 12
    frames = yuv_ref.random_frames(2, 3, H, W)
    path = str(tmp_path / "cut.y4m")
    yuv_ref.write_y4m(path, frames, H, W, truncate=7)
    with pytest.raises(ValueError, match="truncated"):
        fd.open_video(path)
    yuv_ref.write_y4m(path, frames, H, W, truncate=3 * (6 + yuv_ref.frame_bytes(H, W)))      # header only
    with pytest.raises(ValueError, match="no frame"):
        fd.open_video(path)
    # a FRAME line that differs from the first one (same length): found by the per-frame validation
    blob = bytearray(open(_write(tmp_path, frames, H, W), "rb").read())
    second = blob.index(b"FRAME\n", blob.index(b"FRAME\n") + 1)
    blob[second:second + 5] = b"FRAMX"
    bad = str(tmp_path / "bad.y4m")
    open(bad, "wb").write(bytes(blob))
    with pytest.raises(ValueError, match="frame 1"):
        fd.open_video(bad)
    open(bad, "wb").write(b"RIFF not a y4m\n")
    with pytest.raises(ValueError, match="YUV4MPEG2"):
        fd.open_video(bad)


def _write(tmp_path, frames, H, W):
    path = str(tmp_path / "ok.y4m")
    # planes without the byte 'F', so that the search for the second FRAME line cannot land inside a payload
    yuv_ref.write_y4m(path, np.where(frames == ord("F"), 0, frames).astype(np.uint8), H, W)
    return path


def test_abi_surface_is_additive():
    handle = _abi.lib()
    assert handle.kvq_abi_version() == _abi.ABI_VERSION == 32
    assert C.sizeof(_abi.KvqFragmentSource) == 3 * 16 * 8 + 8 + 10 * 4 + 2 * 16 + 8
    for name in ("kvq_yuv420_coeffs", "kvq_yuv420_to_rgb"):
        assert hasattr(handle, name) and name in _abi.SYMBOLS
    assert (_abi.SRC_F32, _abi.SRC_U8) == (0, 1) and _abi.I420_FORMATS == (2, 3, 4, 5)


def test_fused_read_eligibility_takes_the_i420_formats():
    """kvq_patch_embed_fragments_supported (host logic): the four I420 formats with three channels; chan_stride is ignored for them"""
    handle = _abi.lib()
    f = _abi.KvqFragmentSource()
    f.n_clips, f.src_is_u8, f.Hs, f.Ws, f.Fh, f.Fw, f.fs_h, f.fs_w, f.aligned = 4, 1, 541, 961, 7, 7, 32, 32, 8
    ok = lambda *a: handle.kvq_patch_embed_fragments_supported(f, *a)          # noqa: E731  (B, in_chans, pd, T, H, W)
    assert ok(4, 3, 2, 32, 224, 224) == 1
    for fmt in _abi.I420_FORMATS:
        f.src_is_u8 = fmt
        assert ok(4, 3, 2, 32, 224, 224) == 1
        assert ok(4, 1, 2, 32, 224, 224) == 0          # R, G, B only
        f.chan_stride = 5
        assert ok(4, 3, 2, 32, 224, 224) == 1
        f.chan_stride = 0
    for fmt in (6, -1, 0):
        f.src_is_u8 = fmt
        assert ok(4, 3, 2, 32, 224, 224) == 0


def test_i420_frames_checks_its_layout():
    import torch
    H, W = 5, 7
    fb = kernels.i420_frame_bytes(H, W)
    assert fb == 35 + 2 * 12
    data = torch.zeros(4, fb, dtype=torch.uint8)
    fr = kernels.I420Frames(data, H, W, _abi.SRC_I420_BT709_FULL)
    assert fr.shape == (3, 4, H, W) and fr.dtype == torch.uint8
    run = fr.frames(1, 3)
    assert run.shape == (3, 2, H, W) and run.data_ptr() == data.data_ptr() + fb and run.format == fr.format
    for bad in (lambda: kernels.I420Frames(data[:, :-1], H, W, 2), lambda: kernels.I420Frames(data[::2], H, W, 2),
                lambda: kernels.I420Frames(data, H, W, 1), lambda: kernels.I420Frames(data.float(), H, W, 2)):
        with pytest.raises(ValueError):
            bad()


def test_sampled_clips_stage_the_i420_payload_as_it_is(tmp_path):
    """_sampled_clips on a .y4m file (host part, device = cpu): per view an I420Frames whose rows are the sampled frames' payload bytes —
    1.5 B/pixel staged, no conversion, no layout change"""
    import torch
    H, W, T = 9, 14, 12
    frames = yuv_ref.random_frames(8, T, H, W)
    path = str(tmp_path / "v.y4m")
    yuv_ref.write_y4m(path, frames, H, W, extra=("XCOLORRANGE=FULL",))
    samplers = {"a": lambda n, train: np.array([3, 3, 7, 1], np.int32), "b": lambda n, train: np.array([11, 0], np.int32)}
    video, inds = fd._sampled_clips(path, samplers, False, torch.device("cpu"), "bt709")
    for k, want in (("a", [3, 3, 7, 1]), ("b", [11, 0])):
        v = video[k]
        assert isinstance(v, kernels.I420Frames) and v.format == _abi.SRC_I420_BT709_FULL and v.shape == (3, len(want), H, W)
        assert np.array_equal(v.data.numpy(), frames[want]) and np.array_equal(inds[k], want)


def test_y4m_header_long_tags_frame_rate_and_malformed_sizes(tmp_path):
    """a stream header longer than any fixed read (X tags are free-form), the F tag as the reader's frame rate (what the SlowFast
    clip assembly asks a reader for), and size / rate tags that are not numbers: a ValueError naming the file"""
    from kvq_amd.datasets.slowfast_clips import frame_rate_of
    H, W = 4, 6
    frames = yuv_ref.random_frames(4, 3, H, W)
    path = str(tmp_path / "long.y4m")
    yuv_ref.write_y4m(path, frames, H, W, extra=("XCOMMENT=" + "x" * 5000, "XCOLORRANGE=FULL"), frame_header=b"FRAME X" + b"y" * 3000 + b"\n")
    r = fd.open_video(path)
    assert len(r) == 3 and r.format == _abi.SRC_I420_BT601_FULL and r.fps == 30.0
    assert np.array_equal(r[2], yuv_ref.frame_rgb(frames[2], H, W, 3))
    assert frame_rate_of(r, path, None) == 30
    blob = open(path, "rb").read()
    for old, new, what in ((b" F30:1 ", b" F30000:1001 ", 30), (b" F30:1 ", b" F0:0 ", None)):
        open(path, "wb").write(blob.replace(old, new, 1))
        r = fd.open_video(path)
        assert (round(r.fps) if r.fps else None) == what
    with pytest.raises(ValueError, match="frame rate unknown"):
        frame_rate_of(r, path, None)
    for old, new in ((b" W6 ", b" Wsix "), (b" H4 ", b" H-4 "), (b" F30:1 ", b" F30 ")):
        open(path, "wb").write(blob.replace(old, new, 1))
        with pytest.raises(ValueError, match="long.y4m.*malformed"):
            fd.open_video(path)
