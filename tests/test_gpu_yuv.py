"""GPU: I420 (planar YUV 4:2:0) sources.  kvq_yuv420_to_rgb against tests/yuv_ref.py, and every consumer of an I420 source — the
gathers, the fused embedding read, the trunk forward (eager and under graph replay), the quality paint, the harness on .y4m files —
BIT-EQUAL to the same consumer on uint8 frames made by yuv_ref from the same bytes: they share one conversion and, behind it, the
uint8 path's arithmetic."""
import argparse
import functools
import os
import random
import sys

import numpy as np
import pytest
import torch
import yaml

import kvq_amd  # noqa: F401
from kvq_amd import _abi, kernels
from kvq_amd.utils import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KVQ_MEAN, KVQ_STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


@pytest.mark.parametrize("shape", [(3, 64, 96), (2, 37, 53), (1, 2, 2)])
@pytest.mark.parametrize("fmt", yuv_ref.FORMATS)
def test_yuv420_to_rgb_equals_the_numpy_reference(fmt, shape):
    T, H, W = shape
    frames = yuv_ref.random_frames(17 * fmt + H, T, H, W)
    fr = kernels.I420Frames(torch.from_numpy(frames).to(DEV), H, W, fmt)
    rgb = fr.to_rgb()
    assert rgb.shape == (3, T, H, W) and rgb.dtype == torch.uint8 and fr.to_rgb() is rgb          # converted once
    assert np.array_equal(rgb.cpu().numpy(), yuv_ref.frames_rgb(frames, H, W, fmt))
    if T > 1:                                                                                      # a run of frames: a view, same pixels
        run = fr.frames(1, T)
        assert run.data_ptr() == fr.data_ptr() + yuv_ref.frame_bytes(H, W) and torch.equal(run.to_rgb(), rgb[:, 1:])


def test_yuv420_to_rgb_rejects_bad_arguments():
    buf = torch.zeros(64, dtype=torch.uint8, device=DEV)
    lib = _abi.lib()
    assert lib.kvq_yuv420_to_rgb(buf.data_ptr(), 1, 2, 2, 1, buf.data_ptr(), None) == -3          # uint8 is not an I420 format
    assert lib.kvq_yuv420_to_rgb(buf.data_ptr(), 0, 2, 2, 2, buf.data_ptr(), None) == -2
    assert lib.kvq_yuv420_to_rgb(None, 1, 2, 2, 2, buf.data_ptr(), None) == -1


@functools.lru_cache(maxsize=None)
def _pair(seed, n_clips, T, Hs, Ws, grid, fs, aligned, fmt, corner=False):
    """(I420 clips, their uint8 conversion by yuv_ref, draws): made once per geometry and shared, never modified.
    ``corner``: the last frame group of the last mini-patch of the last clip sits at (Hs - fs, Ws - fs), the frame's last row/column"""
    frames = [yuv_ref.random_frames(seed + i, T, Hs, Ws) for i in range(n_clips)]
    i420 = [kernels.I420Frames(torch.from_numpy(f).to(DEV), Hs, Ws, fmt) for f in frames]
    rgb = [torch.from_numpy(yuv_ref.frames_rgb(f, Hs, Ws, fmt)).to(DEV) for f in frames]
    g = torch.Generator().manual_seed(seed)
    gh = torch.tensor([min(Hs // grid * i, Hs - fs) for i in range(grid)]).view(grid, 1, 1)
    gw = torch.tensor([min(Ws // grid * i, Ws - fs) for i in range(grid)]).view(1, grid, 1)
    hs = [(torch.randint(max(1, Hs // grid - fs), (grid, grid, T // aligned), generator=g) + gh).int() for _ in range(n_clips)]
    ws = [(torch.randint(max(1, Ws // grid - fs), (grid, grid, T // aligned), generator=g) + gw).int() for _ in range(n_clips)]
    if corner:
        hs[-1][-1, -1, -1], ws[-1][-1, -1, -1] = Hs - fs, Ws - fs
    return i420, rgb, [h.to(DEV) for h in hs], [w.to(DEV) for w in ws]


def _sources(pair, grid, fs, aligned, normalise=True):
    i420, rgb, hs, ws = pair
    mean, std = (KVQ_MEAN, KVQ_STD) if normalise else (None, None)
    return (kernels.FragmentSource(i420, hs, ws, grid, grid, fs, fs, aligned, mean=mean, std=std),
            kernels.FragmentSource(rgb, hs, ws, grid, grid, fs, fs, aligned, mean=mean, std=std))


def _parities(offs):
    return {int(v) & 1 for o in offs for v in o.flatten().tolist()}


@pytest.mark.parametrize("fmt", yuv_ref.FORMATS)
def test_gathers_on_i420_equal_the_gathers_on_the_converted_frames(fmt):
    geom = dict(T=16, Hs=151, Ws=191, grid=4, fs=32, aligned=4)
    pair = _pair(21, 3, fmt=fmt, **geom)
    for normalise in (True, False):
        yuv, rgb = _sources(pair, geom["grid"], geom["fs"], geom["aligned"], normalise)
        assert yuv.frame_format == fmt and rgb.frame_format == _abi.SRC_U8 and yuv.shape == rgb.shape == (3, 3, 16, 128, 128)
        want = rgb.materialise()
        assert torch.equal(yuv.materialise(), want)                                          # kvq_fragment_gather_batch
        for b, (v, h, w) in enumerate(zip(yuv.videos, yuv.hoffs, yuv.woffs)):                # kvq_fragment_gather
            assert torch.equal(kernels.fragment_gather(v, h, w, *yuv.geometry, mean=yuv.mean, std=yuv.std), want[b])
        halves, rgb_halves = yuv.split_clips(2), rgb.split_clips(2)                          # frame-run views
        assert halves.shape == (6, 3, 8, 128, 128) and halves.videos[1].data_ptr() == yuv.videos[0].data_ptr() + 8 * yuv_ref.frame_bytes(151, 191)
        assert torch.equal(halves.materialise(), rgb_halves.materialise())
    assert _parities(pair[2]) == {0, 1} and _parities(pair[3]) == {0, 1}
    # the single-channel fast path of the uint8 gather has no I420 form: anything but three channels is refused
    out = torch.empty(1, 16, 128, 128, device=DEV)
    rc = _abi.lib().kvq_fragment_gather(pair[0][0].data_ptr(), fmt, 1, 16, 151, 191, pair[2][0].data_ptr(), pair[3][0].data_ptr(), 4, 4, 32, 32,
                                        4, None, None, out.data_ptr(), None)
    assert rc == -3


# (geometry, E, I420 format, corner): the issue's four geometries; the formats rotate over them
EMBED_GEOMS = [(dict(T=16, Hs=270, Ws=480, grid=7, fs=32, aligned=8), 96, 2, False),
               (dict(T=4, Hs=91, Ws=131, grid=5, fs=16, aligned=2), 128, 3, True),          # + the hand-written odd corner origin
               (dict(T=6, Hs=64, Ws=64, grid=2, fs=32, aligned=1), 128, 4, False),           # the source IS the canvas: patches end on
               (dict(T=16, Hs=80, Ws=100, grid=2, fs=32, aligned=4), 96, 5, False)]          # the last row / column; then: frame runs


def _embed_weights(E, half):
    g = np.random.Generator(np.random.PCG64(6))
    w = torch.from_numpy((g.standard_normal((E, 96)) * 0.1).astype(np.float32)).to(DEV).to(half)
    b, lw, lb = (torch.from_numpy(a.astype(np.float32)).to(DEV)
                 for a in (g.standard_normal(E) * 0.2, 1 + 0.2 * g.standard_normal(E), 0.2 * g.standard_normal(E)))
    return w, b, lw, lb


@pytest.mark.parametrize("normalise", [True, False], ids=["normalised", "raw"])
@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", range(len(EMBED_GEOMS)))
def test_fused_embedding_read_of_i420_equals_the_read_of_the_converted_frames(case, half, normalise):
    """the 16-bit operands are the numbers the uint8 read produces from the converted frame (same s_tab lookup): every output bit is"""
    geom, E, fmt, corner = EMBED_GEOMS[case]
    pair = _pair(40 + case, 2, fmt=fmt, corner=corner, **geom)
    yuv, rgb = _sources(pair, geom["grid"], geom["fs"], geom["aligned"], normalise)
    w = _embed_weights(E, half)
    if case == 3:                                            # clips that are runs of frames of a longer video
        yuv, rgb = yuv.split_clips(2), rgb.split_clips(2)
        assert yuv.shape[0] == 4 and yuv.shape[2] == 8
    assert yuv.c_struct().src_is_u8 == fmt and yuv.c_struct().chan_stride == 0
    want, _ = kernels.patch_embed(rgb, *w, (2, 4, 4))
    got, _ = kernels.patch_embed(yuv, *w, (2, 4, 4))
    assert torch.equal(got, want)
    hs, ws = pair[2], pair[3]
    if corner:
        Hs, Ws, fs = geom["Hs"], geom["Ws"], geom["fs"]
        assert (Hs - fs) % 2 == 1 and (Ws - fs) % 2 == 1                       # both odd, on the frame's last row and column,
        assert int(hs[-1][-1, -1, -1]) == Hs - fs and int(ws[-1][-1, -1, -1]) == Ws - fs
        assert pair[0][-1].data.shape[0] == geom["T"]                          # ... of the last frame of a tensor that ends with it
        assert pair[0][-1].data.untyped_storage().nbytes() == geom["T"] * yuv_ref.frame_bytes(Hs, Ws)
    if geom["Hs"] // geom["grid"] > geom["fs"]:                                # (the 64 x 64 source leaves the sampler no choice: origins 0, 32)
        assert _parities(hs) == {0, 1} and _parities(ws) == {0, 1}             # odd and even origins in both axes: the chroma index
    else:                                                                      # paths of the read are all exercised
        assert case == 2 and _parities(hs) == {0}


def test_fused_embedding_read_with_the_next_norm_rows():
    """the trunk's variant of the launch (+ block 0's norm1 rows): as the uint8 read, bit for bit"""
    from oracle import swin3d_oracle as O
    geom, E, fmt, _ = EMBED_GEOMS[0]
    yuv, rgb = _sources(_pair(40, 2, fmt=fmt, corner=False, **geom), geom["grid"], geom["fs"], geom["aligned"])
    w, b, lw, lb = _embed_weights(E, torch.float16)
    lay = O.window_layout(8, 56, 56, (8, 7, 7), (0, 0, 0))
    L = 8 * 56 * 56
    dst = np.empty(L, np.int32)
    dst[lay["src"]] = np.arange(L, dtype=np.int32)
    kw = dict(next_norm=(lw, lb), next_dst=torch.from_numpy(dst).to(DEV), next_rows=L)
    out_a, nxt_a = kernels.patch_embed(rgb, w, b, lw, lb, (2, 4, 4), **kw)
    out_b, nxt_b = kernels.patch_embed(yuv, w, b, lw, lb, (2, 4, 4), **kw)
    assert torch.equal(out_a, out_b) and torch.equal(nxt_a, nxt_b)


def _network(dtype="fp16"):
    from kvq_amd.models import VQA_Network
    cfg = synth.SWIN_T_GRPB
    net = VQA_Network({"model": {"args": {"swin_tiny_grpb": {"backbone": {}, "head": {"in_channels": cfg.num_features, "hidden_channels": 64}}}}})
    sd = {f"swin_tiny_grpb_backbone.{k}": torch.from_numpy(v) for k, v in synth.synth_swin_weights(cfg, 0, "stress").items()}
    sd.update({f"swin_tiny_grpb_head.{k}": torch.from_numpy(v) for k, v in synth.synth_vqa_head_weights(cfg.num_features, 64, 0, "stress").items()})
    net.load_state_dict(sd, strict=False)
    net.swin_tiny_grpb_backbone.operand_dtype = _abi.dtype_code(dtype)
    return net.to(DEV).eval()


FORWARD_GEOM = dict(T=32, Hs=300, Ws=420, grid=7, fs=32, aligned=8)          # test_forward_on_a_fragment_source_equals_sampler_then_forward's


def test_trunk_forward_on_an_i420_source_is_bit_equal_to_the_uint8_source():
    yuv, rgb = _sources(_pair(77, 2, fmt=_abi.SRC_I420_BT709_LIMITED, **FORWARD_GEOM), 7, 32, 8)
    net = _network()
    bb = net.swin_tiny_grpb_backbone
    dev = torch.device(DEV)
    with torch.no_grad():
        s_rgb, f_rgb = net(inputs={"technical": rgb}, return_pooled_feats=True)
        bb.profile(2, 32, 224, 224, dev, True)
        s_yuv, f_yuv = net(inputs={"technical": yuv}, return_pooled_feats=True)
        recs = bb.profile_read(2, 32, 224, 224, dev)
        bb.profile(2, 32, 224, 224, dev, False)
    flat = lambda x: [x] if torch.is_tensor(x) else [t for y in (x.values() if isinstance(x, dict) else x) for t in flat(y)]      # noqa: E731
    a, b = flat(s_rgb) + flat(f_rgb), flat(s_yuv) + flat(f_yuv)
    assert len(a) == len(b) >= 2 and all(torch.equal(x, y) for x, y in zip(a, b))
    emb = [r["kernel"] for r in recs if r["kind"] == "embed"]
    assert emb == ["patch_embed_i420_kernel<kvq::Fp16, 3, 6, true>"]           # ONE embedding launch, reading the I420 frames


def test_recorded_forward_reads_i420_videos_through_a_slot():
    from kvq_amd.graph import LaneGraphs
    fmt = _abi.SRC_I420_BT601_FULL
    pairs = [_pair(90 + i, 2, fmt=fmt, **FORWARD_GEOM) for i in range(2)]                   # two videos
    srcs = [_sources(p, 7, 32, 8) for p in pairs]
    net = _network()
    with torch.no_grad():
        eager = [net(inputs={"technical": rgb}, reduce_scores=True).clone() for _, rgb in srcs]
        assert not torch.equal(eager[0], eager[1])
        slot = kernels.FragmentSlot(srcs[0][0])
        assert slot.c_struct().src_is_u8 == fmt
        for i in (0, 1, 0):
            slot.load(srcs[i][0])
            assert torch.equal(net(inputs={"technical": slot}, reduce_scores=True), eager[i])
        # a slot serves ONE frame format: uint8 planes, or the same bytes declared with another matrix / range, are refused
        other = kernels.FragmentSource([kernels.I420Frames(v.data, v.H, v.W, _abi.SRC_I420_BT601_LIMITED) for v in srcs[1][0].videos],
                                       srcs[1][0].hoffs, srcs[1][0].woffs, 7, 7, 32, 32, 8, mean=KVQ_MEAN, std=KVQ_STD)
        for bad in (srcs[1][1], other):
            with pytest.raises(ValueError, match="frame format"):
                slot.load(bad)
        lanes = [torch.cuda.Stream(device=DEV)]
        graphs = LaneGraphs(lambda inp: net(inputs=inp, reduce_scores=True), lanes)
        outs = []
        for i in (0, 1, 1, 0):
            o = graphs.run(0, {"technical": srcs[i][0]})
            with torch.cuda.stream(lanes[0]):
                outs.append((i, o.clone()))
        o = graphs.run(0, {"technical": srcs[0][1]})                                       # uint8 planes: another signature, own recording
        with torch.cuda.stream(lanes[0]):
            outs.append((0, o.clone()))
        torch.cuda.synchronize()
    assert graphs.eager_runs == 0 and graphs.replays == 5
    for i, o in outs:
        assert torch.equal(o, eager[i])
    from kvq_amd.graph import _signature
    assert _signature({"technical": srcs[0][0]}) == _signature({"technical": srcs[1][0]}) != _signature({"technical": srcs[0][1]})
    assert _signature({"technical": srcs[1][0]}) != _signature({"technical": other})


def test_quality_paint_on_an_i420_source_equals_the_uint8_source():
    geom = dict(T=16, Hs=151, Ws=191, grid=4, fs=32, aligned=4)
    pair = _pair(21, 3, fmt=_abi.SRC_I420_BT601_LIMITED, **geom)
    i420, rgb8, hs, ws = pair
    yuv = kernels.FragmentSource(i420, hs, ws, 4, 4, 32, 32, 4)
    rgb = kernels.FragmentSource(rgb8, hs, ws, 4, 4, 32, 32, 4)
    tok = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).standard_normal((3, 8, 4, 4)).astype(np.float32)).to(DEV)
    assert kernels.quality_paint_supported(yuv, (8, 4, 4), 8)
    for src_a, src_b in ((yuv, rgb), (kernels.FragmentSlot(yuv), kernels.FragmentSlot(rgb))):
        for cell in (1, 8):
            a = kernels.quality_paint(src_a, tok, cell=cell, overlay_depths=(0, 7))
            b = kernels.quality_paint(src_b, tok, cell=cell, overlay_depths=(0, 7))
            assert len(a) == len(b) == 3
            for name, x, y in zip(("heat", "cover", "overlay"), a, b):
                assert torch.equal(x, y), name
            assert a[2].shape == (3, 2, 3, 151, 191) and float(a[1].mean()) > 0
    # one QRS window per frame (kvq_quality_paint_regions): 2 x 2 anchors of 32 out of the 128 x 128 canvas, both phases
    region = torch.from_numpy(np.random.Generator(np.random.PCG64(4)).integers(0, 9, (3, 16)).astype(np.int32)).to(DEV)
    tok2 = tok[:, :, :2, :2].contiguous()
    assert kernels.quality_paint_regions_supported(yuv, (8, 2, 2), 32, 2, 2, 8)
    for phase in (0, 1):
        a = kernels.quality_paint_regions(yuv, tok2, region, 32, 2, 2, phase=phase, cell=8, overlay_depths=(3,))
        b = kernels.quality_paint_regions(rgb, tok2, region, 32, 2, 2, phase=phase, cell=8, overlay_depths=(3,))
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# ---- harness: the same two videos as .y4m and as .npy stacks of yuv_ref's frames ---------------------------------------------------
def _two_trees(tmp_path, n=2, T=40, H=300, W=320, fmt=_abi.SRC_I420_BT601_LIMITED):
    """the sizes of the KSVQE CLI test's fake tree; both trees name their videos clip<i>.y4m (a .npy stack stands in for the file)"""
    for sub in ("y4m", "npy"):
        os.makedirs(str(tmp_path / sub))
    for i in range(n):
        frames = yuv_ref.random_frames(500 + i, T, H, W)
        yuv_ref.write_y4m(str(tmp_path / "y4m" / f"clip{i}.y4m"), frames, H, W)
        rgb = yuv_ref.frames_rgb(frames, H, W, fmt)                                         # (3, T, H, W)
        np.save(str(tmp_path / "npy" / f"clip{i}.y4m.npy"), np.ascontiguousarray(rgb.transpose(1, 2, 3, 0)))
    anno = "".join(f"clip{i}.y4m,1,{3 + i},{2.5 + i}\n" for i in range(n))
    for sub in ("y4m", "npy"):
        (tmp_path / sub / "anno.txt").write_text(anno)


def _tensor(v):
    return v.materialise() if isinstance(v, kernels.FragmentSource) else v


def test_dataset_items_of_a_y4m_tree_equal_those_of_the_decoded_tree(tmp_path):
    from kvq_amd.datasets import ViewDecompositionDataset_KVQ
    from kvq_amd.datasets import fusion_datasets as fd
    _two_trees(tmp_path)
    topt = dict(fragments_h=7, fragments_w=7, fsize_h=32, fsize_w=32, aligned=8, clip_len=32, frame_interval=1, num_clips=1,
                size_h=224, size_w=224, lazy=True)
    items = {}
    for sub in ("y4m", "npy"):
        ds = ViewDecompositionDataset_KVQ(dict(anno_file=str(tmp_path / sub / "anno.txt"), data_prefix=str(tmp_path / sub), phase="test",
                                               sample_types={"technical": topt}, seed_per_item=True))
        assert isinstance(fd.open_video(ds.video_infos[0]["filename"]), fd.Y4mFrameReader if sub == "y4m" else fd.NpyFrameReader)
        items[sub] = [ds[i] for i in range(2)]
    for a, b in zip(items["y4m"], items["npy"]):
        assert set(a) == set(b)
        assert isinstance(a["technical"], kernels.FragmentSource) and a["technical"].frame_format == _abi.SRC_I420_BT601_LIMITED
        assert isinstance(a["technical"].videos[0], kernels.I420Frames) and b["technical"].frame_format == _abi.SRC_U8
        for k in a:
            x, y = a[k], b[k]
            if k in ("technical", "fragment", "resize_video", "ori_fragment"):
                assert torch.equal(_tensor(x), _tensor(y)), k
            elif k == "frame_inds":
                assert all(np.array_equal(x[s], y[s]) for s in x), k
            elif k == "name":
                assert os.path.basename(x) == os.path.basename(y)
            else:
                assert x == y, k
    # an unsampled draw differs between the items: the comparison above is not one of constants
    assert not torch.equal(_tensor(items["y4m"][0]["technical"]), _tensor(items["y4m"][1]["technical"]))
    # yuv_matrix reaches the reader: bt709 converts the same bytes to other pixels
    ds709 = ViewDecompositionDataset_KVQ(dict(anno_file=str(tmp_path / "y4m" / "anno.txt"), data_prefix=str(tmp_path / "y4m"), phase="test",
                                              sample_types={"technical": topt}, seed_per_item=True, yuv_matrix="bt709"))
    it = ds709[0]
    assert it["technical"].frame_format == _abi.SRC_I420_BT709_LIMITED
    assert not torch.equal(_tensor(it["technical"]), _tensor(items["y4m"][0]["technical"]))


def test_harness_output_of_a_y4m_tree_is_byte_identical_to_the_decoded_tree(tmp_path, monkeypatch):
    """``swin_tiny_grpb`` with the lazily sampled view (config/kwai_swin_grpb_synthetic_test.yml's model and sampler on the reference's
    dataset class), seed_per_item: output.txt of the .y4m tree == output.txt of the .npy tree of yuv_ref's frames"""
    from kvq_amd.trainer import Trainer
    _two_trees(tmp_path)
    cfg0 = yaml.safe_load(open(os.path.join(ROOT, "config", "kwai_swin_grpb_synthetic_test.yml")))
    assert cfg0["data"]["val"]["args"]["sample_types"]["technical"]["lazy"] is True
    net = _network()
    ck = tmp_path / "w.pth"
    torch.save({"module." + k: v for k, v in net.state_dict().items()}, str(ck))
    texts = {}
    for sub in ("y4m", "npy"):
        cfg = yaml.safe_load(yaml.safe_dump(cfg0))
        tech = dict(cfg["data"]["val"]["args"]["sample_types"]["technical"], num_clips=1)
        cfg["data"]["val"] = dict(type="ViewDecompositionDataset_KVQ",
                                  args=dict(anno_file=str(tmp_path / sub / "anno.txt"), data_prefix=str(tmp_path / sub), phase="test",
                                            sample_types={"technical": tech}, seed_per_item=True))
        cfg["load_path"] = str(ck)
        monkeypatch.chdir(tmp_path / sub)
        tr = Trainer(argparse.Namespace(opt="-", target_set="val", gpu_id="0"), cfg)
        scores = tr.inferece_test()
        torch.cuda.synchronize()
        assert len(scores) == 2 and np.isfinite(np.asarray(scores, np.float64)).all()
        texts[sub] = (tmp_path / sub / "output.txt").read_bytes()
    lines = texts["y4m"].decode().strip().splitlines()
    assert [l.split(",")[0] for l in lines] == ["clip0.y4m", "clip1.y4m"] and lines[0].split(",")[1] != lines[1].split(",")[1]
    assert texts["y4m"] == texts["npy"]
