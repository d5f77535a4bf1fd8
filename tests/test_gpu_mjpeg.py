"""GPU: kvq_jpeg_idct_i420 against the numpy restatement (tests/jpeg_ref.py) and its host twin, to the bit; the Motion-JPEG readers
through the staging path against the .y4m twin of the same frames; dataset items and the CLI's output.txt of a Motion-JPEG tree against
its .y4m twin tree.  Nothing here depends on a number measured on the GPU."""
import argparse
import os

import numpy as np
import pytest
import torch
import yaml

import kvq_amd  # noqa: F401
from kvq_amd import _abi, kernels
from kvq_amd.datasets import fusion_datasets as fd

import jpeg_ref
import yuv_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
DECODABLE = ["noise_q100", "noise_q5", "odd", "odd_no_dht", "odd_optimize", "odd_restart", "one_mcu", "sub_mcu", "video_0", "video_1", "video_2"]


def _launch(coef, qt, H, W, guard=False):
    """kernels.jpeg_idct_i420 on numpy coefficients (T, blocks, 64) / tables (T, 3, 64) -> numpy (T, frame_bytes); ``guard``: the
    output sits between two rows of 0xA5 that must come back untouched"""
    T = qt.shape[0]
    c = torch.from_numpy(np.ascontiguousarray(coef.reshape(T, -1))).to(DEV)
    q = torch.from_numpy(np.ascontiguousarray(qt).view(np.int16)).to(DEV).view(torch.uint16)
    fb = kernels.i420_frame_bytes(H, W)
    big = torch.full((T + 2, fb), 0xA5, dtype=torch.uint8, device=DEV)
    fr = kernels.jpeg_idct_i420(c, q, H, W, out=big[1:T + 1])
    assert isinstance(fr, kernels.I420Frames) and fr.format == _abi.SRC_I420_BT601_FULL and fr.shape == (3, T, H, W)
    host = big.cpu().numpy()
    assert (host[0] == 0xA5).all() and (host[T + 1] == 0xA5).all()
    return host[1:T + 1]


@pytest.fixture(scope="module")
def restated(golden):
    g = golden("mjpeg.npz")
    out = {}
    for name in DECODABLE:
        coef, qt, p = jpeg_ref.decode_coeffs(g[name + "_jpg"].tobytes())
        out[name] = (g[name + "_jpg"].tobytes(), coef, qt, p["H"], p["W"], jpeg_ref.idct_i420(coef, qt, p["H"], p["W"]))
    return out


@pytest.mark.parametrize("name", DECODABLE)
def test_kernel_equals_the_restatement_and_the_host_twin_on_the_fixtures(restated, name):
    _, coef, qt, H, W, frame = restated[name]
    got = _launch(coef[None], qt[None], H, W)
    assert np.array_equal(got[0], frame)
    assert np.array_equal(got, kernels.jpeg_idct_i420_host(coef[None], qt[None], H, W))


@pytest.mark.parametrize("H,W", [(16, 16), (7, 9), (45, 70), (33, 17)])
def test_kernel_on_synthetic_coefficients_with_per_frame_tables(H, W):
    coef, qt = jpeg_ref.synthetic_coefficients(H * 131 + W, 3, H, W)
    assert not np.array_equal(qt[0], qt[1])
    want = np.stack([jpeg_ref.idct_i420(coef[t], qt[t], H, W) for t in range(3)])
    got = _launch(coef, qt, H, W)
    assert np.array_equal(got, want)
    assert np.array_equal(got, kernels.jpeg_idct_i420_host(coef, qt, H, W))


def test_a_saturating_dc_clamps_at_both_ends():
    H = W = 16
    coef = np.zeros((1, 6, 64), np.int16)
    coef[0, 0, 0], coef[0, 1, 0], coef[0, 2, 0], coef[0, 3, 0] = 2000, -2000, 1016, -1024      # 128 + 250, 128 - 250, 255, 0
    coef[0, 4, 0], coef[0, 5, 0] = 1017, -1025
    qt = np.ones((1, 3, 64), np.uint16)
    got = _launch(coef, qt, H, W)
    y, u, v = jpeg_ref.planes(got[0], H, W)
    assert (y[:8, :8] == 255).all() and (y[:8, 8:] == 0).all() and (y[8:, :8] == 255).all() and (y[8:, 8:] == 0).all()
    assert (u == 255).all() and (v == 0).all()
    assert np.array_equal(got[0], jpeg_ref.idct_i420(coef[0], qt[0], H, W))


def test_out_of_range_coefficients_stay_in_bounds_and_agree_with_the_host():
    g = np.random.Generator(np.random.PCG64(9))
    H, W = 24, 40
    coef = g.integers(-32768, 32768, (2, jpeg_ref.geom(H, W)[4], 64)).astype(np.int16)
    qt = g.integers(1, 256, (2, 3, 64)).astype(np.uint16)
    assert np.array_equal(_launch(coef, qt, H, W), kernels.jpeg_idct_i420_host(coef, qt, H, W))


def test_launch_rejects_bad_arguments():
    lib = _abi.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    assert lib.kvq_jpeg_idct_i420(None, buf.data_ptr(), 1, 16, 16, buf.data_ptr(), None) == -1
    assert lib.kvq_jpeg_idct_i420(buf.data_ptr(), buf.data_ptr(), 0, 16, 16, buf.data_ptr(), None) == -2
    assert lib.kvq_jpeg_idct_i420(buf.data_ptr(), buf.data_ptr(), 1, 0, 16, buf.data_ptr(), None) == -2
    assert lib.kvq_jpeg_idct_i420(buf.data_ptr() + 2, buf.data_ptr(), 1, 16, 16, buf.data_ptr(), None) == -2 and b"aligned" in lib.kvq_last_error()


# ---- staging: the three containers against the .y4m twin -------------------------------------------------------------------------
def _clip(seed, T, H, W, distinct=None):
    """(jpeg frames, their I420 frames by the restatement's IDCT): T frames encoded from seeded coefficients; ``distinct`` < T encodes
    that many and repeats them in a seeded order"""
    n = distinct or T
    coef, qt = jpeg_ref.synthetic_coefficients(seed, n, H, W)
    jpgs = [jpeg_ref.encode_baseline(coef[t], qt[t], H, W, restart=(3 if t % 2 else 0), dht=t % 3 != 2) for t in range(n)]
    planes = np.stack([jpeg_ref.idct_i420(coef[t], qt[t], H, W) for t in range(n)])
    order = np.arange(T) if distinct is None else np.random.Generator(np.random.PCG64(seed)).integers(0, n, T)
    return [jpgs[i] for i in order], planes[order]


def _write_y4m(path, frames, H, W):
    yuv_ref.write_y4m(path, frames, H, W, chroma="C420jpeg", extra=("XCOLORRANGE=FULL",))


@pytest.mark.parametrize("container", ["mjpeg", "avi", "dir"])
def test_staging_equals_the_y4m_twin(tmp_path, restated, container):
    H, W = 48, 64
    jpgs = [restated[n][0] for n in ("video_0", "video_1", "video_2")]
    frames = [jpeg_ref.decode_i420(b)[0] for b in jpgs]                       # the restatement end to end: entropy decode + IDCT
    more, more_frames = _clip(77, 9, H, W)
    assert np.array_equal(jpeg_ref.decode_i420(more[1])[0], more_frames[1])
    jpgs, frames = jpgs + more, np.concatenate([np.stack(frames), more_frames])
    path = str(tmp_path / {"mjpeg": "clip.mjpeg", "avi": "clip.avi", "dir": "clip"}[container])
    if container == "mjpeg":
        jpeg_ref.write_mjpeg(path, jpgs)
    elif container == "avi":
        jpeg_ref.write_avi(path, jpgs, W, H, rate=24, scale=1)
    else:
        jpeg_ref.write_dir(path, jpgs)
    _write_y4m(str(tmp_path / "twin.y4m"), frames, H, W)
    r, twin = fd.open_video(path), fd.open_video(str(tmp_path / "twin.y4m"))
    assert isinstance(r, fd.MjpegFrameReader) and isinstance(twin, fd.Y4mFrameReader) and len(r) == len(twin) == 12
    assert r.format == twin.format == _abi.SRC_I420_BT601_FULL and (r.H, r.W, r.frame_bytes) == (twin.H, twin.W, twin.frame_bytes)
    assert r.fps == (24.0 if container == "avi" else None)
    uniq = np.array([0, 1, 2, 4, 7, 8, 11])
    a, b = fd._frames_to_device(r, uniq, DEV), fd._frames_to_device(twin, uniq, DEV)
    assert isinstance(a, kernels.I420Frames) and a.format == b.format and a.shape == b.shape
    assert torch.equal(a.data, b.data) and np.array_equal(a.data.cpu().numpy(), frames[uniq])
    assert torch.equal(a.to_rgb(), b.to_rgb())
    assert np.array_equal(r[4], twin[4])                                      # the host path: reader[i]


# ---- datasets and the CLI: a Motion-JPEG tree against its .y4m twin tree ---------------------------------------------------------
def _two_trees(tmp_path, T, H, W, distinct=None, as_dir=False):
    """two clips, as Motion-JPEG under mjpeg/ and as their .y4m twins under y4m/.  ``as_dir``: the Motion-JPEG videos are directories
    of frames that carry the twins' NAMES (a directory of frames may have any name), so that the two output.txt files, which
    quote the names, can be compared byte for byte"""
    for sub in ("mjpeg", "y4m"):
        os.makedirs(str(tmp_path / sub))
    for i in range(2):
        jpgs, frames = _clip(900 + i, T, H, W, distinct)
        if as_dir:
            jpeg_ref.write_dir(str(tmp_path / "mjpeg" / f"clip{i}.y4m"), jpgs)
        else:
            jpeg_ref.write_mjpeg(str(tmp_path / "mjpeg" / f"clip{i}.mjpeg"), jpgs)
        _write_y4m(str(tmp_path / "y4m" / f"clip{i}.y4m"), frames, H, W)
    for sub in ("mjpeg", "y4m"):
        ext = "y4m" if as_dir or sub == "y4m" else "mjpeg"
        (tmp_path / sub / "anno.txt").write_text("".join(f"clip{i}.{ext},1,{3 + i},{2.5 + i}\n" for i in range(2)))


def _tensor(v):
    return v.materialise() if isinstance(v, kernels.FragmentSource) else v


def test_dataset_items_of_a_mjpeg_tree_equal_those_of_its_y4m_twin(tmp_path):
    from kvq_amd.datasets import ViewDecompositionDataset_KVQ
    _two_trees(tmp_path, 64, 96, 128)
    topt = dict(fragments_h=3, fragments_w=3, fsize_h=32, fsize_w=32, aligned=8, clip_len=32, frame_interval=1, num_clips=1,
                size_h=224, size_w=224, lazy=True)
    aopt = dict(size_h=224, size_w=224, clip_len=32, frame_interval=2, num_clips=1)
    items = {}
    for sub in ("mjpeg", "y4m"):
        ds = ViewDecompositionDataset_KVQ(dict(anno_file=str(tmp_path / sub / "anno.txt"), data_prefix=str(tmp_path / sub), phase="test",
                                               sample_types={"technical": topt, "aesthetic": aopt}, seed_per_item=True))
        assert isinstance(fd.open_video(ds.video_infos[0]["filename"]), fd.MjpegFrameReader if sub == "mjpeg" else fd.Y4mFrameReader)
        items[sub] = [ds[i] for i in range(2)]
    for a, b in zip(items["mjpeg"], items["y4m"]):
        assert set(a) == set(b)
        assert isinstance(a["technical"], kernels.FragmentSource) and a["technical"].frame_format == b["technical"].frame_format == _abi.SRC_I420_BT601_FULL
        assert isinstance(a["technical"].videos[0], kernels.I420Frames) and torch.equal(a["technical"].videos[0].data, b["technical"].videos[0].data)
        for k in a:
            x, y = a[k], b[k]
            if k in ("technical", "aesthetic", "fragment", "resize_video", "ori_fragment"):
                assert torch.equal(_tensor(x), _tensor(y)), k
            elif k == "frame_inds":
                assert all(np.array_equal(x[s], y[s]) for s in x), k
            elif k in ("name", "video_name"):
                assert os.path.splitext(os.path.basename(x))[0] == os.path.splitext(os.path.basename(y))[0]
            else:
                assert x == y, k
    assert not torch.equal(_tensor(items["mjpeg"][0]["technical"]), _tensor(items["mjpeg"][1]["technical"]))
    assert not np.array_equal(items["mjpeg"][0]["frame_inds"]["technical"], items["mjpeg"][0]["frame_inds"]["aesthetic"])


def _network():
    from kvq_amd.models import VQA_Network
    from kvq_amd.utils import synth
    net = VQA_Network({"model": {"args": {"swin_tiny_grpb": {"head": {"in_channels": 768, "hidden_channels": 64}}}}})
    sd = {f"swin_tiny_grpb_backbone.{k}": torch.from_numpy(v) for k, v in synth.synth_swin_weights(synth.SWIN_T_GRPB, 0, "stress").items()}
    sd.update({f"swin_tiny_grpb_head.{k}": torch.from_numpy(v) for k, v in synth.synth_vqa_head_weights(768, 64, 0, "stress").items()})
    net.load_state_dict(sd, strict=False)
    return net


def test_harness_output_of_a_mjpeg_tree_is_byte_identical_to_its_y4m_twin(tmp_path, monkeypatch):
    """config/kwai_swin_grpb_synthetic_test.yml's model and lazily sampled view on the reference's dataset class, seed_per_item:
    output.txt of the Motion-JPEG tree == output.txt of the .y4m twin tree"""
    from kvq_amd.trainer import Trainer
    _two_trees(tmp_path, 32, 224, 240, distinct=6, as_dir=True)
    cfg0 = yaml.safe_load(open(os.path.join(ROOT, "config", "kwai_swin_grpb_synthetic_test.yml")))
    assert cfg0["data"]["val"]["args"]["sample_types"]["technical"]["lazy"] is True
    ck = tmp_path / "w.pth"
    torch.save({"module." + k: v for k, v in _network().state_dict().items()}, str(ck))
    texts = {}
    for sub in ("mjpeg", "y4m"):
        cfg = yaml.safe_load(yaml.safe_dump(cfg0))
        tech = dict(cfg["data"]["val"]["args"]["sample_types"]["technical"], num_clips=1)
        cfg["data"]["val"] = dict(type="ViewDecompositionDataset_KVQ",
                                  args=dict(anno_file=str(tmp_path / sub / "anno.txt"), data_prefix=str(tmp_path / sub), phase="test",
                                            sample_types={"technical": tech}, seed_per_item=True))
        cfg["load_path"] = str(ck)
        monkeypatch.chdir(tmp_path / sub)
        tr = Trainer(argparse.Namespace(opt="-", target_set="val", gpu_id="0"), cfg)
        assert isinstance(fd.open_video(tr.val_dataset.video_infos[0]["filename"]), fd.MjpegFrameReader if sub == "mjpeg" else fd.Y4mFrameReader)
        scores = tr.inferece_test()
        torch.cuda.synchronize()
        assert len(scores) == 2 and np.isfinite(np.asarray(scores, np.float64)).all()
        texts[sub] = (tmp_path / sub / "output.txt").read_bytes()
    lines = texts["mjpeg"].decode().strip().splitlines()
    assert [l.split(",")[0] for l in lines] == ["clip0.y4m", "clip1.y4m"] and lines[0].split(",")[1] != lines[1].split(",")[1]
    assert texts["mjpeg"] == texts["y4m"]
