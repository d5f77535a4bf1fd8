"""GPU: ``kernels.resize_pil`` (kvq_resize_pil, csrc/resize_pil.hip) against the numpy restatement of Pillow's uint8 bilinear resize
(tests/pil_resize_ref.py, itself pinned to Pillow's outputs by tests/test_resize_pil_cpu.py) — every byte equal — and the paths
built on it: clip assembly on the device, ``SlowFast_features.py --transform device``, SimpleVQA's inline motion features."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import kvq_amd  # noqa: F401
from kvq_amd import _abi, kernels

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pil_resize_ref as R  # noqa: E402
import yuv_ref  # noqa: E402
from guarded import guarded  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, W, oh, ow, T)
GEOMS = [(45, 70, 16, 16, 2), (37, 53, 32, 32, 1), (20, 30, 32, 32, 2), (33, 224, 224, 224, 1), (224, 31, 224, 224, 1), (64, 64, 64, 64, 1),
         (7, 9, 5, 224, 1), (540, 960, 224, 224, 3), (1080, 1920, 224, 224, 1)]
IDS = ["down", "down-odd", "up", "height-only", "width-only", "no-pass", "tiny-mixed", "540p-3-frames", "1080p"]


def _frames(T, H, W, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(T, H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("H,W,oh,ow,T", GEOMS, ids=IDS)
def test_kernel_equals_the_restatement_inside_guard_bands(H, W, oh, ow, T):
    v = _frames(T, H, W, 7 * H + W + oh)
    ref = R.resize_planar_f32(v, oh, ow)
    with guarded() as G:
        src = G.wrap(torch.from_numpy(v).cuda(), name="frames")
        lut = G.wrap(kernels.identity_lut().cuda(), name="lut")
        out = kernels.resize_pil(src, oh, ow, lut)
        assert G.intact(), G.intact()
        assert not bool(G.payload_left(out).any())            # every element written (0xFF payload = NaN)
    got = out.cpu().numpy()
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), (np.abs(got - ref).max(), (got != ref).mean())


@pytest.mark.parametrize("H,W,oh,ow,T", [(46, 70, 16, 16, 2), (540, 960, 224, 224, 2)], ids=["46x70", "540p"])
@pytest.mark.parametrize("fmt", [_abi.SRC_I420_BT601_LIMITED, _abi.SRC_I420_BT709_FULL], ids=["bt601-limited", "bt709-full"])
def test_i420_source_equals_to_rgb_and_the_restatement(H, W, oh, ow, T, fmt):
    raw = yuv_ref.random_frames(31 * H + W + fmt, T, H, W)
    with guarded() as G:
        frames = kernels.I420Frames(G.wrap(torch.from_numpy(raw).cuda(), name="i420"), H, W, fmt)
        lut = kernels.identity_lut().cuda()
        out = kernels.resize_pil(frames, oh, ow, lut)
        assert G.intact(), G.intact()
        assert not bool(G.payload_left(out).any())
    rgb = frames.to_rgb()                                      # uint8 (3, T, H, W), the library's conversion
    assert np.array_equal(rgb.cpu().numpy(), yuv_ref.frames_rgb(raw, H, W, fmt))
    thwc = rgb.permute(1, 2, 3, 0).contiguous()
    assert torch.equal(out, kernels.resize_pil(thwc, oh, ow, lut))
    assert np.array_equal(out.cpu().numpy(), R.resize_planar_f32(thwc.cpu().numpy(), oh, ow))


def test_clip_layout_output_view_and_the_slowfast_table():
    """a (3, T, oh, ow) buffer written through its (T, 3, oh, ow) view — the layout ``extract_video`` stacks clips into — and the
    transform's table: the values are ``pil_transform``'s, bit for bit"""
    from kvq_amd.datasets.slowfast_clips import pil_transform
    T, H, W, r = 5, 45, 70, 16
    v = _frames(T, H, W, 3)
    lut = kernels.slowfast_lut().cuda()
    with guarded() as G:
        buf = torch.empty(3, T, r, r, dtype=torch.float32, device="cuda")
        out = kernels.resize_pil(torch.from_numpy(v).cuda(), r, r, lut, out=buf.permute(1, 0, 2, 3))
        assert G.intact(), G.intact()
        assert not bool(G.payload_left(buf).any())
    assert out.data_ptr() == buf.data_ptr() and not out.is_contiguous()
    tr = pil_transform(r)
    ref = torch.stack([tr(f) for f in v])
    assert torch.equal(out.cpu(), ref) and torch.equal(buf.cpu(), ref.permute(1, 0, 2, 3))
    overlapping = torch.empty(T * 3 * r * r, dtype=torch.float32, device="cuda").as_strided((T, 3, r, r), (r * r, r * r, r, 1))
    with pytest.raises(_abi.KvqError, match="strides"):
        kernels.resize_pil(torch.from_numpy(v).cuda(), r, r, lut, out=overlapping)


def test_limits_are_refused_before_any_launch():
    lut = kernels.identity_lut().cuda()
    wide = torch.zeros(1, 2, 5500, 3, dtype=torch.uint8, device="cuda")
    assert not kernels.resize_pil_supported(wide, 2, 16)
    with pytest.raises(_abi.KvqError, match="status -3"):
        kernels.resize_pil(wide, 2, 16, lut)
    # the largest frame the issue names works: 2160 x 3840 -> 224 x 224, one output row per workgroup
    v = _frames(1, 2160, 3840, 11)
    got = kernels.resize_pil(torch.from_numpy(v).cuda(), 224, 224, lut).cpu().numpy()
    assert np.array_equal(got, R.resize_planar_f32(v, 224, 224))


# ------------------------------------------------------------------------------------------------------- clips on the device
def _host_and_device_clips(root, name, resize, fps):
    from kvq_amd.datasets.fusion_datasets import open_video
    from kvq_amd.datasets.slowfast_clips import VideoDataset_NR_SlowFast_feature, device_clips
    (root / "v.csv").write_text(f"filename,score\n{name},3.5\n")
    ds = VideoDataset_NR_SlowFast_feature(types.SimpleNamespace(resize=resize, fps=fps), None, str(root), str(root / "v.csv"))
    host, vname = ds[0]
    assert vname == name
    path = os.path.join(str(root), name)
    return host, device_clips(open_video(path), path, resize, "cuda", fps)


def _same_clips(host, dev, n_distinct):
    assert len(dev) == len(host) == 8 and all(d.is_cuda and d.dtype == torch.float32 and d.shape == h.shape for d, h in zip(dev, host))
    for k, (d, h) in enumerate(zip(dev, host)):
        assert torch.equal(d.cpu(), h), (k, float((d.cpu() - h).abs().max()))
    assert all(dev[k] is dev[n_distinct - 1] for k in range(n_distinct, 8))              # the padding clips: one tensor object
    assert len({id(d) for d in dev}) == n_distinct


def test_device_clips_equal_the_host_dataset_on_a_frame_stack(tmp_path):
    """the data of tests/test_slowfast.py's host test: 70 frames of 36 x 48 at 29.97 fps, resize 16 -> 2 clips + 6 repeats"""
    frames = np.random.Generator(np.random.PCG64(5)).integers(0, 256, size=(70, 36, 48, 3), dtype=np.uint8)
    np.save(str(tmp_path / "a.mp4.npy"), frames)
    (tmp_path / "a.mp4.fps").write_text("29.97")
    host, dev = _host_and_device_clips(tmp_path, "a.mp4", 16, None)
    _same_clips(host, dev, 2)
    assert dev[0].shape == (32, 3, 16, 16)


def test_device_clips_equal_the_host_dataset_on_a_y4m_file(tmp_path):
    """I420 frames stay I420 up to the resize launch; 20 fps: the third clip starts at frame 40 and repeats frame 69 twice"""
    raw = yuv_ref.random_frames(6, 70, 36, 48)
    yuv_ref.write_y4m(str(tmp_path / "b.y4m"), raw, 36, 48, extra=("F20:1",))
    host, dev = _host_and_device_clips(tmp_path, "b.y4m", 16, None)
    _same_clips(host, dev, 3)
    assert torch.equal(dev[2][29], dev[2][31]) and not torch.equal(dev[2][28], dev[2][29])


def test_device_clips_equal_the_host_dataset_on_a_mjpeg_file(tmp_path):
    """Motion-JPEG written by the project's writer with restart markers: entropy decode, IDCT, conversion and resize all on the device"""
    from kvq_amd.datasets.fusion_datasets import MjpegWriter
    frames = np.random.Generator(np.random.PCG64(5)).integers(0, 256, size=(70, 36, 48, 3), dtype=np.uint8)
    smooth = torch.from_numpy(frames).cuda().permute(3, 0, 1, 2).contiguous()
    with MjpegWriter(str(tmp_path / "c.mjpeg"), fps=20, quality=90, restart_interval=2) as w:
        w.write(smooth)
    (tmp_path / "c.mjpeg.fps").write_text("20")
    host, dev = _host_and_device_clips(tmp_path, "c.mjpeg", 16, None)
    _same_clips(host, dev, 3)


# ------------------------------------------------------------------------------------------ features: the tool and the dataset
def _cli_config(root, transform, folder):
    return types.SimpleNamespace(num_workers=0, resize=64, gpu_ids=None, database="kvq", video_root=str(root), video_csv=str(root / "v.csv"),
                                 feature_save_folder=str(folder), weights=str(root / "w.pth"), fps=30.0, synthetic=0,
                                 video_name="synthetic_00000", seed=0, small_grid_mean=True, transform=transform)


@pytest.fixture(scope="module")
def feature_trees(tmp_path_factory):
    """two small frame stacks and their feature trees, written in-process by ``SlowFast_features.main`` with --transform host (twice)
    and --transform device: the --resize 64 --small_grid_mean set-up of tests/test_slowfast.py's CLI test"""
    from kvq_amd.utils import synth
    from oracle import slowfast_oracle as SF
    sys.path.insert(0, ROOT)
    import SlowFast_features as cli
    root = tmp_path_factory.mktemp("pil_features")
    g = np.random.Generator(np.random.PCG64(9))
    for name, n in (("a.mp4", 100), ("b.mp4", 45)):
        np.save(str(root / f"{name}.npy"), g.integers(0, 256, size=(n, 60, 80, 3), dtype=np.uint8))
    (root / "b.mp4.fps").write_text("15")
    (root / "v.csv").write_text("filename,score\na.mp4,1\nb.mp4,2\n")
    w = synth.synth_params(SF.param_shapes(), 3, "stress", prefix="sf.")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, str(root / "w.pth"))
    for sub, transform in (("host", "host"), ("host2", "host"), ("device", "device")):
        cli.main(_cli_config(root, transform, root / sub), str(root), str(root / "v.csv"))
    return root


def _tree(root, sub):
    out = {}
    for name in ("a.mp4", "b.mp4"):
        d = root / sub / "kvq" / name
        out[name] = {f: np.load(str(d / f)) for f in sorted(os.listdir(d))}
    return out


def test_tool_with_transform_device_writes_the_features_of_transform_host(feature_trees):
    """same file tree; values within 2e-3 max|feature|, the bound tests/test_slowfast.py's CLI test uses between two evaluations of
    the same clips.  The clips are bit-equal (the tests above), so what is left is the network's own run-to-run difference: the
    figures of device against host and of host against host are printed before the assertions.  On an MI355X both were 0.0 — two
    host-path runs are bit-equal there — so where host equals host in every bit, device must equal host in every bit too."""
    host, host2, dev = (_tree(feature_trees, s) for s in ("host", "host2", "device"))
    worst = {"device-host": 0.0, "host-host": 0.0}
    for name in ("a.mp4", "b.mp4"):
        assert sorted(dev[name]) == sorted(host[name]) and len(dev[name]) == 16
        for f, ref in host[name].items():
            assert dev[name][f].shape == ref.shape == ((1, 2048, 1, 1, 1) if "slow" in f else (1, 256, 1, 1, 1))
            scale = np.abs(ref).max()
            worst["device-host"] = max(worst["device-host"], float(np.abs(dev[name][f] - ref).max() / scale))
            worst["host-host"] = max(worst["host-host"], float(np.abs(host2[name][f] - ref).max() / scale))
    print("max |difference| / max |feature|:", worst)
    for name in ("a.mp4", "b.mp4"):
        for f, ref in host[name].items():
            assert np.allclose(dev[name][f], ref, rtol=0, atol=2e-3 * np.abs(ref).max()), (name, f)
    if worst["host-host"] == 0.0:
        assert worst["device-host"] == 0.0, worst


def _inline_dataset(root, feature_type, source="inline"):
    from kvq_amd.datasets import ViewDecompositionDataset_add_forSimpleVQA
    opt = dict(anno_file=str(root / "v.csv"), data_prefix=str(root), feature_type=feature_type, phase="test",
               sample_types={"simpleVQA": dict(resize=130, crop=112, clip_len=8, frame_interval=10, t_frag=8, num_clips=1)})
    if source == "inline":
        opt["motion_features"] = dict(source="inline", weights=str(root / "w.pth"), resize=64, fps=30.0, small_grid_mean=True)
    else:
        opt["data_prefix_3D"] = str(root / "device" / "kvq")
    return ViewDecompositionDataset_add_forSimpleVQA(opt, device="cuda")


def test_inline_motion_features_equal_the_feature_files(feature_trees):
    """``feat`` of ``source: inline`` against ``feat`` read from the files ``--transform device`` wrote with the same weights, under the
    bound of the test above (on an MI355X the printed figures were 0.0); ``feature_type`` selects the slow / fast columns"""
    inline, files = _inline_dataset(feature_trees, "SlowFast"), _inline_dataset(feature_trees, "SlowFast", "files")
    feats = []
    for i in range(2):
        item, ref = inline[i], files[i]
        feat = item["feat"]
        assert feat.is_cuda and feat.dtype == torch.float32 and feat.shape == (8, 2304)
        assert set(item) == set(ref) and item["simpleVQA"].shape == ref["simpleVQA"].shape
        r = ref["feat"].numpy()
        for lo, hi in ((0, 2048), (2048, 2304)):                     # slow and fast columns, each against its own scale
            d = np.abs(feat.cpu().numpy()[:, lo:hi] - r[:, lo:hi]).max(1)
            print("video", i, "columns", lo, hi, "max |difference| / max |feature| per clip", (d / np.abs(r[:, lo:hi]).max(1)).max())
            assert (d <= 2e-3 * np.abs(r[:, lo:hi]).max(1)).all()
        feats.append(feat)
    for ftype, cols in (("Slow", slice(0, 2048)), ("Fast", slice(2048, 2304))):
        ds = _inline_dataset(feature_trees, ftype)
        ds._motion_model = inline.motion_model()                    # the same network: built once for the three datasets
        got = ds[0]["feat"]
        ref = feats[0][:, cols]
        assert got.shape == ref.shape and got.is_cuda
        assert bool(((got - ref).abs().max(1).values <= 2e-3 * ref.abs().max(1).values).all())


def test_trainer_scores_the_tree_with_the_inline_yml(feature_trees, tmp_path, monkeypatch):
    """config/kwai_simpleVQA_inline_test.yml on the two-video tree (reduced sizes), ``hipgraph: auto`` = recorded forwards for SimpleVQA:
    ``Trainer.inferece_test`` completes with a device-resident ``feat``"""
    import argparse
    import yaml
    from kvq_amd.trainer import Trainer
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "kwai_simpleVQA_inline_test.yml")))
    args = cfg["data"]["val"]["args"]
    assert args["motion_features"]["source"] == "inline" and "data_prefix_3D" not in args and "hipgraph" not in cfg
    args.update(anno_file=str(feature_trees / "v.csv"), data_prefix=str(feature_trees))
    args["motion_features"].update(weights=str(feature_trees / "w.pth"), resize=64, fps=30.0, small_grid_mean=True)
    args["sample_types"]["simpleVQA"].update(resize=130, crop=112)
    cfg["load_path"] = cfg["test_load_path"] = None
    monkeypatch.chdir(tmp_path)
    tr = Trainer(argparse.Namespace(opt="-", target_set="val", gpu_id="0"), cfg)
    scores = tr.inferece_test()
    torch.cuda.synchronize()
    assert len(scores) == 2 and np.isfinite(np.asarray(scores, np.float64)).all()
    assert tuple(tr.graph_stats) == (2, 0)                         # (replays, eager runs): both forwards were recorded ones
    lines = (tmp_path / "output.txt").read_text().strip().splitlines()
    assert [l.split(",")[0] for l in lines] == ["a.mp4", "b.mp4"]
