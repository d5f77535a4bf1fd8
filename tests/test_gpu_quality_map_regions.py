"""GPU: quality maps through KSVQE's region windows — the paint that composes the sampler's draws with the QRS window of every frame
(bit for bit against tests/qmap_regions_ref.py, whose rectangles test_quality_map_regions_cpu.py pins to the reference's sampler and
RegionNet_CLIP), KSVQE's `regions`, and the harness that writes the files."""
import os
import random
import sys
import types

import numpy as np
import pytest
import torch
import yaml

import kvq_amd  # noqa: F401
from kvq_amd import _abi, kernels
from kvq_amd.utils import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qmap_regions_ref as RR  # noqa: E402
from test_gpu_harness import _fake_kvq_tree  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_CASES = ("300x340_a8", "288x288_a2")


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _fixture_geometry(g, case):
    """two clips that are frame runs of ONE longer video: clip 0 with the fixture's draws and windows, clip 1 with the draws permuted
    inside the grid and other windows"""
    T, H, W, aligned, Hf, Wf, Fh, Fw, fs, anchor, kh, kw = (int(v) for v in g[f"{case}/meta"])
    hoff, woff = g[f"{case}/hoff"], g[f"{case}/woff"]
    hoff2 = np.concatenate([hoff, np.roll(hoff, 3, axis=1)], 2)
    woff2 = np.concatenate([woff, np.roll(woff, 2, axis=0)], 2)
    regions = np.stack([g[f"{case}/regions"], np.asarray([8, 0, 3, 3, 1, 7, 5, 2], np.int32)]).astype(np.int32)
    return dict(T=T, H=H, W=W, aligned=aligned, Hf=Hf, Wf=Wf, Fh=Fh, Fw=Fw, fs=fs, anchor=anchor, kh=kh, kw=kw), hoff2, woff2, regions


def _small_geometry():
    """4 x 4 mini-patches of 32, windows of 2 x 2 anchors of 32 (3 x 3 origins), a 4 x 4 token grid (sh = sw = 16: two token rows per
    anchor), a 131 x 157 source (neither a multiple of the cell nor of 4), aligned 2"""
    d = dict(T=8, H=131, W=157, aligned=2, Hf=4, Wf=4, Fh=4, Fw=4, fs=32, anchor=32, kh=2, kw=2)
    rng = np.random.Generator(np.random.PCG64(11))
    nt = 2 * d["T"] // d["aligned"]
    gy = np.minimum(d["H"] // 4 * np.arange(4), d["H"] - 32)
    gx = np.minimum(d["W"] // 4 * np.arange(4), d["W"] - 32)
    hoff = (gy[:, None, None] + np.zeros((4, 4, nt), np.int64)).astype(np.int32)              # 131 // 4 == 32: no room to draw
    woff = (gx[None, :, None] + rng.integers(0, d["W"] // 4 - 32, (4, 4, nt))).astype(np.int32)
    regions = rng.integers(0, 9, (2, d["T"])).astype(np.int32)
    regions[0, :4] = [0, 8, 4, 4]
    return d, hoff, woff, regions


def _geometry(golden, case):
    return _small_geometry() if case == "small" else _fixture_geometry(golden("qmap_regions.npz"), case)


def _source(d, hoff2, woff2, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    video = rng.integers(0, 256, (3, 2 * d["T"], d["H"], d["W"])).astype(np.uint8)
    src = kernels.FragmentSource([torch.from_numpy(video).cuda()], [torch.from_numpy(hoff2).cuda()], [torch.from_numpy(woff2).cuda()],
                                 d["Fh"], d["Fw"], d["fs"], d["fs"], d["aligned"]).split_clips(2)
    assert src.videos[1].stride(0) == 2 * d["T"] * d["H"] * d["W"] and src.shape[0] == 2
    tok = rng.standard_normal((2, d["T"] // 2, d["Hf"], d["Wf"])).astype(np.float32)
    return src, video, tok


def _expected(d, video, hoff2, woff2, regions, tok, cell, phase, depths, lo, hi, alpha=128, dim=96):
    T, nt = d["T"], d["T"] // d["aligned"]
    heat, cover, ov = [], [], []
    for b in range(2):
        r = RR.token_rects_regions(hoff2[:, :, b * nt:(b + 1) * nt], woff2[:, :, b * nt:(b + 1) * nt], regions[b], T // 2, d["Hf"], d["Wf"],
                                   d["fs"], d["fs"], d["aligned"], d["anchor"], d["kh"], d["kw"], phase)
        h, c = RR.paint(*r, tok[b], d["H"], d["W"], cell)
        heat.append(h), cover.append(c)
        ov.append(RR.overlays(video[:, b * T:(b + 1) * T], *r, tok[b], depths, phase, lo, hi, alpha, dim))
    return np.stack(heat), np.stack(cover), np.stack(ov)


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("cell", [1, 8])
@pytest.mark.parametrize("case", FIXTURE_CASES + ("small",))
def test_paint_is_bit_equal_to_the_numpy_reference(golden, case, cell, phase):
    d, hoff2, woff2, regions = _geometry(golden, case)
    src, video, tok = _source(d, hoff2, woff2, 60 + cell + 2 * phase)
    D = d["T"] // 2
    depths = (0, D - 1)
    tok_d, reg_d = torch.from_numpy(tok).cuda(), torch.from_numpy(regions).cuda()
    win = (d["anchor"], d["kh"], d["kw"])
    assert kernels.quality_paint_regions_supported(src, (D, d["Hf"], d["Wf"]), *win, cell)
    heat, cover, ov = kernels.quality_paint_regions(src, tok_d, reg_d, *win, phase=phase, cell=cell, overlay_depths=depths)
    want = _expected(d, video, hoff2, woff2, regions, tok, cell, phase, depths, tok.min(), tok.max())
    for name, a, b in zip(("heat", "cover", "overlay"), (heat, cover, ov), want):
        a = a.cpu().numpy()
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert np.array_equal(_bits(a), _bits(b)), name
    assert 0 < float(cover.mean()) <= 1
    # an explicit range, other blend weights; without overlays the call returns two tensors
    heat2, cover2, ov2 = kernels.quality_paint_regions(src, tok_d, reg_d, *win, phase=phase, cell=cell, overlay_depths=(1,),
                                                       value_range=(-0.5, 1.25), alpha=200, dim=31)
    want2 = _expected(d, video, hoff2, woff2, regions, tok, cell, phase, (1,), -0.5, 1.25, 200, 31)
    assert torch.equal(heat2, heat) and torch.equal(cover2, cover) and np.array_equal(ov2.cpu().numpy(), want2[2])
    assert len(kernels.quality_paint_regions(src, tok_d, reg_d, *win, phase=phase, cell=cell)) == 2
    # through a FragmentSlot (the pointer table a recorded forward reads): identical; and again after the slot is re-pointed
    slot = kernels.FragmentSlot(src)
    for a, b in zip(kernels.quality_paint_regions(slot, tok_d, reg_d, *win, phase=phase, cell=cell, overlay_depths=depths), (heat, cover, ov)):
        assert torch.equal(a, b)
    other = kernels.FragmentSource(src.videos[::-1], src.hoffs[::-1], src.woffs[::-1], *src.geometry)
    slot.load(other)
    swapped = kernels.quality_paint_regions(slot, tok_d.flip(0).contiguous(), reg_d.flip(0).contiguous(), *win, phase=phase, cell=cell,
                                            overlay_depths=depths)
    for a, b in zip(swapped, (heat, cover, ov)):
        assert torch.equal(a.flip(0), b)
    torch.cuda.synchronize()


@pytest.mark.parametrize("cell", [1, 8])
@pytest.mark.parametrize("case", ["240x300_a8", "231x257_a2"])
def test_a_window_that_is_the_canvas_paints_what_the_existing_paint_paints(golden, case, cell):
    g = golden("qmap.npz")
    T, H, W, aligned, Hf, Wf, Fh, Fw, fs = (int(v) for v in g[f"paint/{case}/meta"])
    assert (Fh, Fw, Hf, Wf) == (7, 7, 7, 7)
    d = dict(T=T, H=H, W=W, aligned=aligned, Hf=Hf, Wf=Wf, Fh=Fh, Fw=Fw, fs=fs)
    hoff, woff = g[f"paint/{case}/hoff"], g[f"paint/{case}/woff"]
    src, _, tok = _source(d, np.concatenate([hoff, np.roll(hoff, 3, axis=1)], 2), np.concatenate([woff, np.roll(woff, 2, axis=0)], 2), 70 + cell)
    tok_d = torch.from_numpy(tok).cuda()
    regions = torch.zeros(2, T, dtype=torch.int32, device="cuda")            # 7 x 7 anchors of a 7 x 7 canvas: the one window
    depths = (0, T // 2 - 1)
    assert kernels.quality_paint_regions_supported(src, (T // 2, 7, 7), 32, 7, 7, cell)
    got = kernels.quality_paint_regions(src, tok_d, regions, 32, 7, 7, phase=0, cell=cell, overlay_depths=depths)
    want = kernels.quality_paint(src, tok_d, cell=cell, overlay_depths=depths)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    torch.cuda.synchronize()


def test_region_values_that_name_no_window_leave_their_slices_uncovered():
    d, hoff2, woff2, regions = _small_geometry()
    src, video, tok = _source(d, hoff2, woff2, 80)
    tok_d = torch.from_numpy(tok).cuda()
    win, D, T = (32, 2, 2), 4, 8
    depths = (0, 1, 2, 3)
    base = kernels.quality_paint_regions(src, tok_d, torch.from_numpy(regions).cuda(), *win, cell=1, overlay_depths=depths, value_range=(-1.0, 1.0))
    bad = regions.copy()
    bad[0, 2], bad[1, 6] = -1, 9                        # clip 0 slice 1, clip 1 slice 3 (phase 0 reads frame 2d); 9 == 3 * 3 windows
    bad[0, 1], bad[1, 3] = 2 ** 30, -2 ** 31            # odd frames: phase 0 never reads them
    got = kernels.quality_paint_regions(src, tok_d, torch.from_numpy(bad).cuda(), *win, cell=1, overlay_depths=depths, value_range=(-1.0, 1.0))
    torch.cuda.synchronize()                            # defined behaviour: nothing is read through the value, no error
    heat, cover, ov = (t.cpu().numpy() for t in got)
    heat0, cover0, ov0 = (t.cpu().numpy() for t in base)
    for b, s in ((0, 1), (1, 3)):
        assert not heat[b, s].any() and not cover[b, s].any()
        assert np.array_equal(ov[b, s], ((video[:, b * T + 2 * s].astype(np.int64) * 96 + 128) >> 8).astype(np.uint8))
        heat0[b, s], cover0[b, s], ov0[b, s] = heat[b, s], cover[b, s], ov[b, s]
    assert np.array_equal(_bits(heat), _bits(heat0)) and np.array_equal(_bits(cover), _bits(cover0)) and np.array_equal(ov, ov0)
    want = _expected(d, video, hoff2, woff2, bad, tok, 8, 1, (0,), -1.0, 1.0)          # phase 1 reads the odd frames' values
    got8 = kernels.quality_paint_regions(src, tok_d, torch.from_numpy(bad).cuda(), *win, phase=1, cell=8, overlay_depths=(0,), value_range=(-1.0, 1.0))
    torch.cuda.synchronize()
    for a, b in zip(got8, want):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b))
    assert not got8[1][0, 0].any() and not got8[1][1, 1].any()


def test_paint_refuses_what_it_does_not_cover(golden):
    d, hoff2, woff2, regions = _geometry(golden, FIXTURE_CASES[0])
    src, _, tok = _source(d, hoff2, woff2, 7)
    tok_d, reg_d = torch.from_numpy(tok).cuda(), torch.from_numpy(regions).cuda()
    assert not kernels.quality_paint_regions_supported(src, (4, 7, 7), 64, 7, 7)
    assert not kernels.quality_paint_regions_supported(src, (4, 7, 7), 32, 10, 10)
    for kwargs in (dict(anchor=64, kh=7, kw=7), dict(anchor=32, kh=10, kw=10), dict(anchor=32, kh=7, kw=7, phase=2),
                   dict(anchor=32, kh=7, kw=7, phase=-1), dict(anchor=32, kh=6, kw=7)):
        with pytest.raises(_abi.KvqError, match="kvq_quality_paint_regions"):
            kernels.quality_paint_regions(src, tok_d, reg_d, **kwargs)
    with pytest.raises(_abi.KvqError, match="kvq_quality_paint_regions"):
        kernels.quality_paint_regions(src, tok_d[:, :3].contiguous(), reg_d, 32, 7, 7)         # T != 2 D
    with pytest.raises(_abi.KvqError):
        kernels.quality_paint_regions(src, tok_d, reg_d, 32, 7, 7, cell=3)
    with pytest.raises(_abi.KvqError, match="region"):
        kernels.quality_paint_regions(src, tok_d, reg_d.long(), 32, 7, 7)
    with pytest.raises(_abi.KvqError, match="region"):
        kernels.quality_paint_regions(src, tok_d, reg_d[:, :4].contiguous(), 32, 7, 7)
    with pytest.raises(_abi.KvqError, match="overlay depth"):
        kernels.quality_paint_regions(src, tok_d, reg_d, 32, 7, 7, overlay_depths=(4,))
    torch.cuda.synchronize()


# ---- model and harness: a fake KVQ tree, a seeded KSVQE checkpoint ---------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from kvq_amd.models import VQA_Network
    root = tmp_path_factory.mktemp("kvq_tree")
    _fake_kvq_tree(root, n=2, T=24, H=300, W=320)
    (root / "anno.txt").write_text("clip0.mp4,1,3,2.5\nclip1.mp4,0,4,4.0\n")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "Kwai_KSVQE_qmap_test.yml")))
    net = VQA_Network(cfg)
    sd = {"KSVQE_backbone." + k: torch.from_numpy(v) for k, v in synth.synth_ksvqe_weights(3).items()}
    sd.update({"KSVQE_head." + k: torch.from_numpy(v) for k, v in synth.synth_vqa_head_weights(768, 64, 3, "stress").items()})
    assert not net.load_state_dict(sd, strict=False).unexpected_keys
    torch.save(net.state_dict(), str(root / "ksvqe.pth"))
    return root, net.cuda().eval()


def _cfg(root, maps, graph, tmp=None, lazy=True):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "Kwai_KSVQE_qmap_test.yml")))
    a = cfg["data"]["val"]["args"]
    a.update(anno_file=str(root / "anno.txt"), data_prefix=str(root))
    a["sample_types"]["technical"].update(clip_len=16, num_clips=1, frame_interval=1, lazy=lazy)
    cfg.update(load_path=str(root / "ksvqe.pth"), hipgraph=graph, streams=1, prefetch=0)     # one lane: its recording serves both videos
    if maps:
        cfg["quality_maps"].update(dir=str(tmp / f"maps_{graph}_{int(lazy)}"), cell=1, overlay_frames=2)
    else:
        cfg.pop("quality_maps")
    return cfg


def _seed(n):
    np.random.seed(n), random.seed(n), torch.manual_seed(n)


def _recomputed_regions(net, item):
    """the window of every frame, from the backbone's own CLIP map: what RegionNet_CLIP.forward computes and used to drop"""
    from kvq_amd.models.backbones import ksvqe_modules as KM
    bb = net.KSVQE_backbone
    revideo = item["resize_video"].unsqueeze(0).float()
    group_id, key = KM.obtain_keyframes(revideo)
    cls_attn, _, _ = bb.CLIP_tool(key.reshape((key.shape[1],) + tuple(key.shape[2:])).contiguous())
    gs = int(round(cls_attn.reshape(key.shape[1], -1).shape[1] ** 0.5))
    idx = kernels.qrs_top_region(cls_attn.to(torch.float32).reshape(key.shape[1], gs, gs).contiguous(), 9, 9, 7, 7)
    return KM.extend_by_group(idx.reshape(1, -1), group_id), group_id


def test_ksvqe_returns_its_regions_and_the_paint_reads_them(tree):
    from kvq_amd.datasets import ViewDecompositionDataset_KVQ
    root, net = tree
    ds = ViewDecompositionDataset_KVQ(_cfg(root, False, "off")["data"]["val"]["args"], None, device="cuda:0")
    _seed(4)
    item = ds[1]
    src = item["fragment"]
    assert isinstance(src, kernels.FragmentSource) and not src.upsampled and src.shape == (1, 3, 16, 288, 288)
    inp = dict(resize_video=item["resize_video"].unsqueeze(0), fragment=src.materialise(), dis_label=torch.tensor([item["dis_label"]]))
    with torch.no_grad():
        plain, _ = net(inputs=dict(inp), reduce_scores=True)
        (pred, _), maps = net(inputs=dict(inp), reduce_scores=True, return_maps=True)
        want_regions, group_id = _recomputed_regions(net, item)
    assert torch.equal(pred, plain)                                         # the score keeps its bits
    m = maps["KSVQE"]
    regions, tok = m["regions"], m["token_map"]
    assert regions.shape == (1, 16) and regions.dtype == torch.int32 and regions.is_cuda and tok.shape == (1, 8, 7, 7)
    assert regions is net.KSVQE_backbone.last_regions
    assert torch.equal(regions, want_regions.to(torch.int32))
    assert group_id[0].tolist() == [0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 3]
    reg = regions.cpu().numpy()
    assert ((reg >= 0) & (reg < 9)).all()
    assert kernels.quality_paint_regions_supported(src, tok.shape[1:], 32, 7, 7, 8)
    frames = src.videos[0].cpu().numpy()
    for phase in (0, 1):
        heat, cover, ov = kernels.quality_paint_regions(src, tok, regions, 32, 7, 7, phase=phase, cell=8, overlay_depths=(1, 6))
        r = RR.token_rects_regions(src.hoffs[0].cpu().numpy(), src.woffs[0].cpu().numpy(), reg[0], 8, 7, 7, 32, 32, 8, 32, 7, 7, phase)
        tk = tok[0].cpu().numpy()
        h, c = RR.paint(*r, tk, 300, 320, 8)
        assert np.array_equal(_bits(heat[0].cpu().numpy()), _bits(h)) and np.array_equal(_bits(cover[0].cpu().numpy()), _bits(c))
        assert np.array_equal(ov[0].cpu().numpy(), RR.overlays(frames, *r, tk, (1, 6), phase, tk.min(), tk.max()))
    torch.cuda.synchronize()


def _run_harness(root, tmp, monkeypatch, maps, graph, lazy=True):
    from kvq_amd.trainer import Trainer
    run = tmp / f"run_{int(maps)}_{graph}_{int(lazy)}"
    run.mkdir()
    monkeypatch.chdir(run)
    _seed(9)                                              # the samplers' draws: the same in every run
    t = Trainer(types.SimpleNamespace(gpu_id="0"), _cfg(root, maps, graph, tmp, lazy))
    t.inferece_test()
    torch.cuda.synchronize()
    return t, (run / "output.txt").read_bytes()


def test_harness_paints_ksvqe_and_graph_replay_writes_the_same_files(tree, tmp_path, monkeypatch):
    root, _ = tree
    files = {}
    _, plain = _run_harness(root, tmp_path, monkeypatch, False, "on")         # the run without the key (graph replay, KSVQE's default)
    for graph in ("on", "off"):
        t, with_maps = _run_harness(root, tmp_path, monkeypatch, True, graph)
        assert with_maps == plain                                            # output.txt: byte-identical
        if graph == "on":
            replays, eager = t.graph_stats
            assert replays == 2 and eager == 0
        lines = with_maps.decode().strip().splitlines()
        mdir = tmp_path / f"maps_{graph}_1"
        assert sorted(os.listdir(mdir)) == sorted(l.split(",")[0] + ".npz" for l in lines) and len(lines) == 2
        for line in lines:
            name, score = line.split(",")
            z = np.load(mdir / (name + ".npz"))
            assert set(z.files) == {"score", "token_map", "timeline", "frame_inds", "heat", "cover", "overlay", "regions"}
            files[graph, name] = {k: z[k] for k in z.files}
            tok, reg = z["token_map"], z["regions"]
            assert float(z["score"]) == float(score)
            assert tok.shape == (1, 8, 7, 7) and z["frame_inds"].shape == (1, 8, 2)
            assert reg.shape == (1, 16, 2) and reg.dtype == np.int32 and ((reg >= 0) & (reg <= 2)).all()
            assert z["heat"].shape == z["cover"].shape == (1, 8, 300, 320) and z["overlay"].shape == (1, 2, 3, 300, 320)
            for d in range(8):                                               # cell 1: a copy of the scores under the window's rectangles
                assert int((z["cover"][0, d] > 0).sum()) == 7 * 7 * 32 * 32
                assert set(np.unique(z["heat"][0, d][z["cover"][0, d] > 0]).tolist()) <= set(tok[0, d].ravel().tolist())
    for (graph, name), arrays in files.items():
        if graph == "on":
            for k, v in arrays.items():
                assert np.array_equal(_bits(v), _bits(files["off", name][k])), (name, k)


def test_harness_lazy_false_gets_the_token_maps_only(tree, tmp_path, monkeypatch, capfd):
    root, _ = tree
    _run_harness(root, tmp_path, monkeypatch, True, "off", lazy=False)
    files = sorted(os.listdir(tmp_path / "maps_off_0"))
    assert len(files) == 2
    z = np.load(tmp_path / "maps_off_0" / files[0])
    assert set(z.files) == {"score", "token_map", "timeline", "frame_inds"}
    err = capfd.readouterr().err
    assert err.count("quality maps:") == 1 and "lazy: false" in err
