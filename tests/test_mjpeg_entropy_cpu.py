"""CPU: the host's share of the entropy decode on the device — the segment index (kvq_jpeg_index) against a numpy marker search, the
launch's host twin (kvq_jpeg_entropy_host, compiled from csrc/jpeg_huff.hpp as the launch is) against kvq_jpeg_coeffs and the
restatement to the bit, the reader's ``jpeg_entropy`` option with a CPU target, and the stand-alone sanitizer check.  Expected
coefficients are kvq_jpeg_coeffs' and tests/jpeg_ref.py's, never the code under test's."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import kvq_amd  # noqa: F401
from kvq_amd import _abi, kernels
from kvq_amd.datasets import fusion_datasets as fd

import jpeg_ref
import jpeg_entropy_cases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_SHAPE, ERR_WORKSPACE = 0, -2, -4


@pytest.fixture(scope="module")
def fixtures(golden):
    g = golden("mjpeg.npz")
    return {name: g[name + "_jpg"].tobytes() for name in jc.FIXTURES}


def _size(jpg):
    p = jpeg_ref.parse(jpg)
    return p["H"], p["W"], p["ri"]


def _twin(jpgs):
    H, W, _ = _size(jpgs[0])
    data, frames, segs, tables, qt = jc.pack(jpgs)
    coef, status = kernels.jpeg_entropy_host(data, frames, segs, tables, len(jpgs), H, W)
    return coef.reshape(len(jpgs), -1, 64), status, qt


# ---- the index ----------------------------------------------------------------------------------------------------------------------
def _check_index(jpg):
    H, W, ri = _size(jpg)
    nc = jpeg_ref.geom(H, W)[3]
    rc, info, segs, tables, qt, msg = jc.index(jpg)
    assert rc == OK, msg
    want, markers = jc.marker_search(jpg)
    nseg = -(-nc // ri) if ri else 1
    assert len(segs) == len(want) == nseg and np.array_equal(segs, want)
    assert list(markers) == [0xD0 + (s & 7) for s in range(nseg - 1)] + [0xD9]
    assert (info.width, info.height, info.restart_interval, info.supported, info.frame_bytes) == (W, H, ri, 1, len(jpg))
    _, _, want_qt, _ = jc.host_coeffs(jpg, H, W)
    assert np.array_equal(qt, want_qt)
    t = _abi.KvqJpegTables.from_buffer_copy(tables.tobytes())
    assert 2 <= t.ntab <= 6 and all(i < t.ntab for i in list(t.dc)[:3] + list(t.ac)[:3])
    return nseg


@pytest.mark.parametrize("name", jc.FIXTURES)
def test_index_of_the_fixtures_equals_a_marker_search(fixtures, name):
    _check_index(fixtures[name])


@pytest.mark.parametrize("case", jc.SYNTHETIC, ids=jc.case_id)
def test_index_of_synthetic_frames_equals_a_marker_search(case):
    nseg = _check_index(jc.synthetic(case))
    H, W, ri, _ = case
    if ri == 0 or ri == 200:
        assert nseg == 1                                             # no DRI; a restart interval larger than the MCU count
    if (H, W, ri) == (130, 150, 1):
        assert nseg == 90
    if (H, W, ri) == (130, 150, 7):
        assert nseg == 13


def test_the_annex_k_set_stores_identical_tables_once():
    a, b = jc.index(jc.synthetic((130, 150, 7, True))), jc.index(jc.synthetic((130, 150, 7, False)))
    assert np.array_equal(a[3], b[3])                                # the DHT segments of the encoder are the Annex K tables
    t = _abi.KvqJpegTables.from_buffer_copy(a[3].tobytes())
    assert t.ntab == 4 and (t.dc[1], t.ac[1]) == (t.dc[2], t.ac[2]) and t.dc[0] != t.dc[1] and t.ac[0] != t.ac[1]


def test_index_refuses_what_the_decoder_refuses():
    jpg = jc.synthetic((130, 150, 7, True))
    H, W = 130, 150
    segs, markers = jc.marker_search(jpg)
    assert len(segs) == 13 and jc.host_coeffs(jpg, H, W)[0] == OK
    m = int(segs[4, 1])                                              # the marker that closes segment 4: RST4
    assert jpg[m:m + 2] == b"\xff\xd4"
    cases = {
        "wrong number": (jpg[:m + 1] + b"\xd5" + jpg[m + 2:], r"wrong restart marker FFD5 before MCU 35, expected RST4"),
        "one removed": (jpg[:m] + jpg[m + 2:], r"wrong restart marker FFD5 before MCU 35, expected RST4|truncated|no Huffman|run past"),
        "one too many": (jpg[:-2] + b"\xff\xd4\xff\xd9", r"marker FFD4 after the last MCU where EOI belongs"),
        "EOI cut": (jpg[:-2], r"missing EOI after the last MCU"),
        "cut inside the last marker": (jpg[:-1], r"missing EOI after the last MCU"),
        "cut in the scan": (jpg[:m], r"missing RST4 before MCU 35"),
    }
    for what, (bad, text) in cases.items():
        rc, info, _, _, _, msg = jc.index(bad)
        hrc, _, _, hmsg = jc.host_coeffs(bad, H, W)
        assert hrc == ERR_SHAPE, (what, hmsg)                        # the yardstick refuses it
        if what == "one removed":                                    # two segments run together: the index sees only the marker count
            assert rc == ERR_SHAPE and "wrong restart marker FFD5 before MCU 35, expected RST4" in msg, (what, msg)
        else:
            assert rc == ERR_SHAPE and re.search(text, msg) and msg.startswith("kvq_jpeg_index: "), (what, msg)
            assert hmsg.replace("kvq_jpeg_coeffs: ", "") == msg.replace("kvq_jpeg_index: ", ""), (what, hmsg, msg)


def test_the_decoder_and_the_index_word_the_four_marker_faults_alike():
    H, W, ri = 45, 70, 3                                             # 15 MCUs: five segments
    jpg = jc.synthetic((H, W, ri, False))
    segs, _ = jc.marker_search(jpg)
    assert len(segs) == 5 and jc.host_coeffs(jpg, H, W)[0] == OK and jc.index(jpg)[0] == OK
    m = int(segs[1, 1])                                              # the marker that closes segment 1: RST1, before MCU 6
    assert jpg[m:m + 2] == b"\xff\xd1" and jpg[-2:] == b"\xff\xd9"
    faults = {
        "missing RSTn": (jpg[:m], "missing RST1 before MCU 6 (the stream is truncated or has no marker there)"),
        "wrong RSTn": (jpg[:m + 1] + b"\xd5" + jpg[m + 2:], "wrong restart marker FFD5 before MCU 6, expected RST1"),
        "missing EOI": (jpg[:-2], "missing EOI after the last MCU (the stream is truncated)"),
        "another marker where EOI belongs": (jpg[:-1] + b"\xe0", "marker FFE0 after the last MCU where EOI belongs"),
    }
    for what, (bad, text) in faults.items():
        rc, _, _, _, _, msg = jc.index(bad)
        hrc, _, _, hmsg = jc.host_coeffs(bad, H, W)
        assert rc == ERR_SHAPE and hrc == ERR_SHAPE, (what, msg, hmsg)
        assert msg == "kvq_jpeg_index: " + text and hmsg == "kvq_jpeg_coeffs: " + text, (what, msg, hmsg)


def test_index_parses_like_the_probe(golden):
    g = golden("mjpeg.npz")
    for name in ("progressive", "s422", "s444", "gray", "cmyk"):
        data = g[name + "_jpg"]
        rc, info, pmsg = kernels.jpeg_probe(data)
        irc, iinfo, _, _, _, imsg = jc.index(data.tobytes(), cap=4096)
        assert irc == rc == -3 and imsg.replace("kvq_jpeg_index", "kvq_jpeg_probe") == pmsg and bytes(iinfo) == bytes(info)
    irc, _, _, _, _, imsg = jc.index(b"\xff\xd8\xff", cap=4)
    assert irc == ERR_SHAPE and "not a JPEG image" in imsg


def test_a_short_segment_capacity_is_a_workspace_error_and_nothing_is_written():
    jpg = np.frombuffer(jc.synthetic((130, 150, 7, True)), np.uint8)
    segs, tables, qt = np.full((32, 2), 0xA5A5A5A5, np.uint32), np.full(kernels.JPEG_TABLES_BYTES, 0xA5, np.uint8), np.full((3, 64), 0xA5A5, np.uint16)
    rc, info, nseg, msg = kernels.jpeg_index(jpg, segs[8:20], tables, qt)               # 12 of 13
    assert rc == ERR_WORKSPACE and nseg == 13 and "13" in msg
    assert (segs == 0xA5A5A5A5).all() and (tables == 0xA5).all() and (qt == 0xA5A5).all()
    rc, info, nseg, msg = kernels.jpeg_index(jpg, segs[8:21], tables, qt)               # exactly 13
    assert rc == OK and nseg == 13 and (segs[:8] == 0xA5A5A5A5).all() and (segs[21:] == 0xA5A5A5A5).all()
    assert np.array_equal(segs[8:21], jc.marker_search(jpg.tobytes())[0])


def test_no_prefix_is_indexed_and_no_read_leaves_it():
    jpg = np.frombuffer(jc.synthetic((45, 70, 3, False)), np.uint8)
    segs, tables, qt = np.zeros((16, 2), np.uint32), np.zeros(kernels.JPEG_TABLES_BYTES, np.uint8), np.zeros((3, 64), np.uint16)
    for k in range(jpg.size):
        prefix = np.array(jpg[:k])                                   # its own allocation
        rc, _, _, msg = kernels.jpeg_index(prefix, segs, tables, qt)
        assert rc == ERR_SHAPE and msg, k


# ---- the host twin against kvq_jpeg_coeffs and the restatement ----------------------------------------------------------------------
def _check_twin(jpg):
    H, W, _ = _size(jpg)
    rc, want, want_qt, msg = jc.host_coeffs(jpg, H, W)
    assert rc == OK, msg
    assert np.array_equal(want, jpeg_ref.decode_coeffs(jpg)[0])
    coef, status, qt = _twin([jpg])
    assert (status == 0).all(), status
    assert np.array_equal(coef[0], want) and np.array_equal(qt[0], want_qt)


@pytest.mark.parametrize("name", jc.FIXTURES)
def test_host_twin_equals_the_decoder_on_the_fixtures(fixtures, name):
    _check_twin(fixtures[name])


@pytest.mark.parametrize("case", jc.SYNTHETIC, ids=jc.case_id)
def test_host_twin_equals_the_decoder_on_synthetic_frames(case):
    jpg = jc.synthetic(case)
    _check_twin(jpg)
    coef, _ = jc.coefficients(case[0], case[1])
    assert np.array_equal(jc.host_coeffs(jpg, case[0], case[1])[1], coef)


def test_host_twin_on_several_frames_with_different_table_sets(fixtures):
    """odd and odd_optimize are the same 45 x 70 picture with the Annex K tables and with optimised ones: two sets in one call"""
    jpgs = [fixtures["odd"], fixtures["odd_optimize"], fixtures["odd_restart"], fixtures["odd_no_dht"]]
    data, frames, segs, tables, qt = jc.pack(jpgs, front=3)
    assert tables.shape[0] == 2 and list(frames[:, 4]) == [0, 1, 0, 0] and frames[0, 0] == 3
    coef, status = kernels.jpeg_entropy_host(data, frames, segs, tables, 4, 45, 70)
    assert (status == 0).all()
    for t, jpg in enumerate(jpgs):
        assert np.array_equal(coef[t].reshape(-1, 64), jc.host_coeffs(jpg, 45, 70)[1]), t


def _ac_code_lengths(table):
    bits, vals = table
    return dict(zip(vals, [length for length in range(1, 17) for _ in range(bits[length - 1])]))


def test_the_corpus_holds_what_the_decode_must_get_right():
    """computed here from the coefficients and the Annex K code lengths: an AC symbol longer than the 9-bit lookahead in each AC table, a
    ZRL, a block whose coefficient 63 is not zero (no EOB), a DC category of 10 or more, and a stuffed FF 00"""
    H, W = 130, 150
    coef, _ = jc.coefficients(H, W)
    mx, my, ny, nc, _ = jpeg_ref.geom(H, W)
    longest = {0: 0, 1: 0}
    zrl = last = False
    for b in range(coef.shape[0]):
        zz = coef[b][jpeg_ref.ZIGZAG].astype(int)
        lengths = _ac_code_lengths(jpeg_ref.STD_AC_LUM if b < ny else jpeg_ref.STD_AC_CHR)
        run = 0
        for k in range(1, 64):
            if zz[k] == 0:
                run += 1
                continue
            zrl |= run > 15
            longest[int(b >= ny)] = max(longest[int(b >= ny)], lengths[((run & 15) << 4) | int(abs(zz[k])).bit_length()])
            run = 0
        last |= zz[63] != 0
    assert longest[0] > 9 and longest[1] > 9 and zrl and last, (longest, zrl, last)
    blocks = jc.mcu_blocks(H, W)                                     # DC differences in coding order, no restart
    dc_y = coef[blocks[:, :4].reshape(-1), 0].astype(int)
    assert int(np.abs(np.diff(dc_y)).max()).bit_length() >= 10
    assert any(b"\xff\x00" in jc.synthetic(c)[jpeg_ref.parse(jc.synthetic(c))["scan"]:] for c in jc.SYNTHETIC if c[:2] == (H, W))


# ---- malformed segments: a status, never a step outside the buffers -----------------------------------------------------------------
def test_host_twin_flags_malformed_segments_and_leaves_the_others_alone():
    H, W, ri = 130, 150, 10
    jpg = jc.synthetic((H, W, ri, True))
    _, want, _, _ = jc.host_coeffs(jpg, H, W)
    data, frames, segs, tables, _ = jc.pack([jpg])
    s = 4
    assert segs[s, 1] - segs[s, 0] > 16
    others = np.setdiff1d(np.arange(want.shape[0]), jc.segment_blocks(H, W, ri, s))
    for what, cause in (("cut", (1, 2, 4)), ("code", (2,)), ("run", (4,)), ("trailing", (5,)), ("range", (6,))):
        d, sg = data.copy(), segs.copy()
        if what == "cut":
            sg[s, 1] -= 3
        elif what == "code":
            d[sg[s, 0]:sg[s, 0] + len(jc.NO_SUCH_CODE)] = np.frombuffer(jc.NO_SUCH_CODE, np.uint8)
        elif what == "run":
            d[sg[s, 0]:sg[s, 0] + len(jc.RUN_PAST_63)] = np.frombuffer(jc.RUN_PAST_63, np.uint8)
        elif what == "trailing":
            sg[s, 1] += 2                                            # the RSTn marker itself: an 0xFF no 0x00 follows ends the supply
        else:
            sg[s, 1] = data.size + 64 + 1                            # past the end of the buffer, trailing guard included
        guard = np.concatenate([np.full(64, 0xFF, np.uint8), d, np.full(64, 0xFF, np.uint8)])
        fr = frames.copy()
        fr[0, 0] += 64
        coef, status = kernels.jpeg_entropy_host(guard, fr, sg, tables, 1, H, W)
        assert status[s] != 0 and (status[s] & 255) in cause and (np.delete(status, s) == 0).all(), (what, status)
        if what in ("code", "run"):
            assert status[s] >> 8 == s * ri                          # the MCU at which it stopped: the segment's first
        assert np.array_equal(coef[0].reshape(-1, 64)[others], want[others]), what


def test_host_twin_refuses_descriptors_that_do_not_fit():
    H, W = 45, 70
    jpg = jc.synthetic((H, W, 3, False))
    data, frames, segs, tables, _ = jc.pack([jpg])
    nseg = segs.shape[0]
    for field, value in ((0, data.size + 1), (2, nseg - 1), (3, 2), (4, 1)):          # offset, nseg, restart interval, table set
        fr = frames.copy()
        fr[0, field] = value
        coef, status = kernels.jpeg_entropy_host(data, fr, segs, tables, 1, H, W)
        assert ((status & 255) == 6)[:fr[0, 2]].all() and not coef.any(), (field, status)
    fr = frames.copy()
    fr[0, 1] = 1                                                     # the frame's segments would end past the table
    coef, status = kernels.jpeg_entropy_host(data, fr, segs, tables, 1, H, W)
    assert (status == -1).all() and not coef.any()
    bad = tables.copy()
    bad[0, 4] = 9                                                    # dc[0] names a table the set does not have
    coef, status = kernels.jpeg_entropy_host(data, frames, segs, bad, 1, H, W)
    assert ((status & 255) == 6).all() and not coef.any()
    lib = _abi.lib()
    assert lib.kvq_jpeg_entropy_host(None, 0, None, None, 0, None, 0, 1, H, W, None, None) == -1
    z = np.zeros(64, np.uint32)
    assert lib.kvq_jpeg_entropy_host(z.ctypes.data, 4, z.ctypes.data, z.ctypes.data, 0, z.ctypes.data, 1, 0, H, W, z.ctypes.data, z.ctypes.data) == ERR_SHAPE


# ---- the reader ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def mixed(tmp_path):
    """a 45 x 70 stream whose frames differ in restart interval and tables"""
    cases = [(45, 70, 3, False), (45, 70, 0, True), (45, 70, 1, True), (45, 70, 3, True)]
    path = str(tmp_path / "mixed.mjpeg")
    jpeg_ref.write_mjpeg(path, [jc.synthetic(c) for c in cases])
    return path, cases


def test_reader_keeps_the_restart_intervals_and_every_mode_agrees_on_a_cpu_target(mixed):
    path, cases = mixed
    r = fd.open_video(path)
    assert list(r.restart_intervals) == [3, 0, 1, 3] and list(r.segment_counts([0, 1, 2, 3])) == [5, 1, 15, 5]
    uniq = np.array([0, 1, 3])
    coef, qt = jc.coefficients(45, 70)
    want = np.stack([jpeg_ref.idct_i420(coef, qt, 45, 70)] * 3)
    for mode in (None, "auto", "host", "device"):
        got = fd._frames_to_device(r, uniq, "cpu", mode)
        assert isinstance(got, kernels.I420Frames) and got.format == _abi.SRC_I420_BT601_FULL and np.array_equal(got.data.numpy(), want), mode
    with pytest.raises(ValueError, match="'auto', 'host', 'device'"):
        fd._frames_to_device(r, uniq, "cpu", "gpu")


def test_the_device_path_hands_what_it_cannot_decode_to_the_host_decoder(tmp_path):
    """on a CPU target the host twins stand in for the launches: a frame whose segment carries one byte too many decodes on the host
    (the strict end refuses it, kvq_jpeg_coeffs does not); a corrupt frame is the host decoder's ValueError"""
    H, W = 45, 70
    good = jc.synthetic((H, W, 3, True))
    extra = good[:-2] + b"\x00" + good[-2:]
    assert jc.host_coeffs(extra, H, W)[0] == OK and jc.index(extra)[0] == OK
    _, status, _ = _twin([extra])
    assert status[-1] & 255 == 5 and (status[:-1] == 0).all()
    segs, _ = jc.marker_search(good)
    corrupt = bytearray(good)
    corrupt[segs[2, 0]:segs[2, 0] + len(jc.NO_SUCH_CODE)] = jc.NO_SUCH_CODE
    no_eoi = good[:-2] + b"\xff\xd7"
    path = str(tmp_path / "clip")
    jpeg_ref.write_dir(path, [good, extra, bytes(corrupt), no_eoi + b"\xff\xd9"])
    r = fd.open_video(path)
    a, b = fd._frames_to_device(r, np.array([0, 1]), "cpu", "device"), fd._frames_to_device(r, np.array([0, 1]), "cpu", "host")
    assert np.array_equal(a.data.numpy(), b.data.numpy()) and np.array_equal(a.data.numpy()[0], a.data.numpy()[1])
    for mode in ("host", "device"):
        with pytest.raises(ValueError, match=r"3\.jpg: frame 2: kvq_jpeg_coeffs: a code that is in no Huffman table \(MCU 6 of 15, block 0\)"):
            fd._frames_to_device(r, np.array([0, 2]), "cpu", mode)
        with pytest.raises(ValueError, match=r"4\.jpg: frame 3: kvq_jpeg_coeffs: marker FFD7 after the last MCU where EOI belongs"):
            fd._frames_to_device(r, np.array([3]), "cpu", mode)


def test_the_yml_key_reaches_the_reader(mixed, monkeypatch):
    from kvq_amd.datasets import ViewDecompositionDataset_KVQ
    path, _ = mixed
    d = os.path.dirname(path)
    with open(os.path.join(d, "anno.txt"), "w") as f:
        f.write("mixed.mjpeg,1,3,2.5\n")
    seen = []

    class Reached(Exception):
        pass

    def spy(vr, uniq, device, entropy=None):                         # the rest of an item needs a device: stop here
        seen.append(entropy)
        raise Reached

    monkeypatch.setattr(fd, "_jpeg_frames_to_device", spy)
    opt = dict(anno_file=os.path.join(d, "anno.txt"), data_prefix=d, phase="test", seed_per_item=True,
               sample_types={"aesthetic": dict(size_h=32, size_w=32, clip_len=2, frame_interval=1, num_clips=1)})
    for value in ("device", "host", None):
        o = dict(opt) if value is None else dict(opt, jpeg_entropy=value)
        with pytest.raises(Reached):
            ViewDecompositionDataset_KVQ(o, device="cpu")[0]
        assert seen[-1] == value
    assert fd.JPEG_ENTROPY == "auto" and fd.jpeg_entropy_mode(None) == "auto"         # a yml without the key behaves as auto
    with pytest.raises(ValueError, match="'auto', 'host', 'device'"):
        ViewDecompositionDataset_KVQ(dict(opt, jpeg_entropy="fast"), device="cpu")


def test_transcode_tool_accepts_row_as_the_restart_interval():
    import importlib.util
    spec = importlib.util.spec_from_file_location("transcode_mjpeg", os.path.join(ROOT, "tools", "transcode_mjpeg.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.restart_mcus("row", 960) == 60 and tool.restart_mcus("row", 70) == 5 and tool.restart_mcus("7", 960) == 7
    assert tool.restart_mcus("0", 960) == 0
    with pytest.raises(ValueError):
        tool.restart_mcus("column", 960)


# ---- ABI and the stand-alone check --------------------------------------------------------------------------------------------------
def test_abi_surface():
    header = open(os.path.join(ROOT, "include", "kvq_hip.h")).read()
    handle = _abi.lib()
    for name in ("kvq_jpeg_index", "kvq_jpeg_entropy_host", "kvq_jpeg_entropy"):
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _abi.SYMBOLS and hasattr(handle, name)
    assert "typedef struct KvqJpegTables" in header and C.sizeof(_abi.KvqJpegHuffTable) == 1364 and C.sizeof(_abi.KvqJpegTables) == 8196
    assert handle.kvq_abi_version() == _abi.ABI_VERSION == 32
    assert handle.kvq_jpeg_entropy(None, 0, None, None, 0, None, 0, 1, 16, 16, None, None, None) == -1


def _sanitizer_compiler():
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        return None, "no host C++ compiler"
    probe = subprocess.run([cxx, "-x", "c++", "-", "-fsanitize=address,undefined", "-o", os.devnull], input="int main() { return 0; }",
                           capture_output=True, text=True)
    return (cxx, "") if probe.returncode == 0 else (None, f"{cxx} has no address / undefined-behaviour sanitizer runtimes")


def test_hostcheck_under_the_sanitizers(tmp_path, fixtures):
    """tools/jpeg_entropy_hostcheck.cpp: a program of its own, the host compiler alone, -fsanitize=address,undefined; every fixture, every
    prefix, every byte of the scan replaced three ways"""
    cxx, why = _sanitizer_compiler()
    if cxx is None:
        pytest.skip(why)
    exe = str(tmp_path / "jpeg_entropy_hostcheck")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                        os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "jpeg_entropy_hostcheck.cpp"),
                        os.path.join(os.path.dirname(kvq_amd.__file__), "csrc", "jpeg.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    files = []
    for name in jc.FIXTURES:
        files.append(str(tmp_path / (name + ".jpg")))
        with open(files[-1], "wb") as f:
            f.write(fixtures[name])
    files.append(str(tmp_path / "synthetic_ri1.jpg"))
    with open(files[-1], "wb") as f:
        f.write(jc.synthetic((45, 70, 1, False)))
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    assert r.returncode == 0 and "jpeg_entropy_hostcheck: all clean" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
