"""GPU: local quality maps — the head that keeps its per-token map, the paint onto source-frame geometry (bit for bit against
tests/qmap_ref.py, whose rectangles test_quality_map_cpu.py pins to the reference's sampler) and the harness that writes them."""
import os
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
import qmap_ref as QR  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("240x300_a8", "270x480_a4", "540x960_a8", "224x224_a8", "231x257_a2", "270x480_a4_s16")

# Summation-order noise of the head's arithmetic: the largest |fp32 - fp64| over the per-token map of a CPU evaluation of the
# reference's VQAHead(768, 64) on the fixture feature (tests/golden/make_qmap_golden.py stores it as head/fp32_noise).
# Measured: 9.351375723776201e-07.  The map is held to 4 x that against the reference's stored map.
HEAD_FP32_NOISE = 9.351375723776201e-07
HEAD_MAP_TOL = 4 * HEAD_FP32_NOISE


def _head_inputs():
    feat = np.random.Generator(np.random.PCG64(5)).standard_normal((2, 768, 4, 7, 7)).astype(np.float32)
    w = {k: torch.from_numpy(v).cuda() for k, v in synth.synth_vqa_head_weights(768, 64, 5, "stress").items()}
    return torch.from_numpy(feat).cuda(), w


@pytest.mark.parametrize("layout", ["channels_first_valu", "channels_last_mfma"])
def test_head_map_keeps_the_score_bits_and_matches_the_reference_map(golden, layout):
    g = golden("qmap.npz")
    assert float(g["head/fp32_noise"]) == HEAD_FP32_NOISE
    feat, w = _head_inputs()
    if layout == "channels_last_mfma":
        # (B, D, H, W, C) memory viewed as (B, C, D, H, W): stride_c == 1 -> the fp32 MFMA kernel; 2 * 196 tokens = 24.5 tiles of 16
        feat = feat.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
        assert feat.stride(1) == 1 and (feat.shape[0] * 196) % 16 != 0
    args = (feat, w["fc_hid.weight"], w["fc_hid.bias"], w["fc_last.weight"].reshape(-1), w["fc_last.bias"])
    plain = kernels.vqa_head(*args)
    score, tok, depth = kernels.vqa_head(*args, return_map=True)
    torch.cuda.synchronize()
    assert torch.equal(score, plain) and score.shape == (2, 1)
    assert tok.shape == (2, 4, 7, 7) and depth.shape == (2, 4)
    tok64, L = tok.double().cpu().numpy(), 196
    # any fp32 summation of L values errs by at most L * 2^-24 * max|v| (the division and the bias add: a few ulp more)
    bound = (L + 8) * 2.0 ** -24 * max(1.0, float(np.abs(tok64).max()))
    got = score.double().cpu().numpy().ravel()
    print("map mean - score", (tok64.reshape(2, -1).mean(1) - got).tolist(), "depth mean - score",
          (depth.double().cpu().numpy().mean(1) - got).tolist(), "bound", bound)
    assert np.abs(tok64.reshape(2, -1).mean(1) - got).max() <= bound
    assert np.abs(depth.double().cpu().numpy().mean(1) - got).max() <= bound
    assert np.abs(depth.double().cpu().numpy() - tok64.reshape(2, 4, -1).mean(2)).max() <= bound
    err = float(np.abs(tok.cpu().numpy() - g["head/map"]).max())
    print("max |map - reference map|", err, "tolerance", HEAD_MAP_TOL)
    assert err <= HEAD_MAP_TOL
    assert np.abs(score.cpu().numpy() - g["head/score"]).max() <= HEAD_MAP_TOL


def test_head_map_shape_errors():
    feat, w = _head_inputs()
    a = (w["fc_hid.weight"].reshape(64, -1).t().contiguous(), w["fc_hid.bias"], w["fc_last.weight"].reshape(-1), w["fc_last.bias"])
    tok, score = torch.empty(2 * 196, device="cuda"), torch.empty(2, device="cuda")
    rc = _abi.lib().kvq_vqa_head_map(feat.data_ptr(), 2, 196, 768, 768 * 196, 1, 196, a[0].data_ptr(), None, a[1].data_ptr(), 64,
                                     a[2].data_ptr(), a[3].data_ptr(), 5, tok.data_ptr(), None, score.data_ptr(), None)
    assert rc == -2                                                  # 196 tokens do not split into 5 depth slices


def _case_source(g, case, seed):
    """two clips that are frame runs of ONE longer video (split_clips: chan_stride != T Hs Ws): clip 0 with the fixture's draws,
    clip 1 with the same draws permuted inside the grid (rows of hoff keep their grid row, columns of woff their grid column)"""
    T, H, W, aligned, Hf, Wf, Fh, Fw, fs = (int(v) for v in g[f"paint/{case}/meta"])
    hoff, woff = g[f"paint/{case}/hoff"], g[f"paint/{case}/woff"]
    hoff2 = np.concatenate([hoff, np.roll(hoff, 3, axis=1)], 2)
    woff2 = np.concatenate([woff, np.roll(woff, 2, axis=0)], 2)
    rng = np.random.Generator(np.random.PCG64(seed))
    video = rng.integers(0, 256, (3, 2 * T, H, W)).astype(np.uint8)
    src = kernels.FragmentSource([torch.from_numpy(video).cuda()], [torch.from_numpy(hoff2).cuda()], [torch.from_numpy(woff2).cuda()],
                                 Fh, Fw, fs, fs, aligned).split_clips(2)
    assert src.videos[1].stride(0) == 2 * T * H * W and src.shape[0] == 2
    tok = rng.standard_normal((2, T // 2, Hf, Wf)).astype(np.float32)
    return src, video, (hoff2, woff2), tok, (T, H, W, aligned, Hf, Wf, fs)


def _expected(video, draws, tok, dims, cell, depths, lo, hi, alpha, dim):
    T, H, W, aligned, Hf, Wf, fs = dims
    nt = T // aligned
    heat, cover, ov = [], [], []
    for b in range(2):
        r0, c0, sh, sw = QR.token_rects(draws[0][:, :, b * nt:(b + 1) * nt], draws[1][:, :, b * nt:(b + 1) * nt], T // 2, Hf, Wf, fs, fs, aligned)
        h, c = QR.paint(r0, c0, sh, sw, tok[b], H, W, cell)
        heat.append(h), cover.append(c)
        h1, c1 = (h, c) if cell == 1 else QR.paint(r0, c0, sh, sw, tok[b], H, W, 1)
        ov.append(np.stack([QR.overlay(video[:, b * T + 2 * d], h1[d], c1[d], lo, hi, alpha, dim) for d in depths]))
    return np.stack(heat), np.stack(cover), np.stack(ov)


@pytest.mark.parametrize("cell", [1, 8])
@pytest.mark.parametrize("case", CASES)
def test_paint_is_bit_equal_to_the_numpy_reference(golden, case, cell):
    g = golden("qmap.npz")
    src, video, draws, tok, dims = _case_source(g, case, 40 + cell)
    D = dims[0] // 2
    depths = (0, D - 1)
    tok_d = torch.from_numpy(tok).cuda()
    assert kernels.quality_paint_supported(src, (D, dims[4], dims[5]), cell)
    heat, cover, ov = kernels.quality_paint(src, tok_d, cell=cell, overlay_depths=depths)
    want = _expected(video, draws, tok, dims, cell, depths, tok.min(), tok.max(), 128, 96)
    for name, a, b in zip(("heat", "cover", "overlay"), (heat, cover, ov), want):
        a = a.cpu().numpy()
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), name
    assert 0 < float(cover.mean()) <= 1
    # an explicit range, other blend weights; without overlays the call returns two tensors
    heat2, cover2, ov2 = kernels.quality_paint(src, tok_d, cell=cell, overlay_depths=(1,), value_range=(-0.5, 1.25), alpha=200, dim=31)
    want2 = _expected(video, draws, tok, dims, cell, (1,), -0.5, 1.25, 200, 31)
    assert torch.equal(heat2, heat) and torch.equal(cover2, cover) and np.array_equal(ov2.cpu().numpy(), want2[2])
    assert len(kernels.quality_paint(src, tok_d, cell=cell)) == 2
    # through a FragmentSlot (the pointer table a recorded forward reads): identical; and again after the slot is re-pointed
    slot = kernels.FragmentSlot(src)
    for a, b in zip(kernels.quality_paint(slot, tok_d, cell=cell, overlay_depths=depths), (heat, cover, ov)):
        assert torch.equal(a, b)
    other = kernels.FragmentSource(src.videos[::-1], src.hoffs[::-1], src.woffs[::-1], *src.geometry)
    slot.load(other)
    swapped = kernels.quality_paint(slot, tok_d.flip(0).contiguous(), cell=cell, overlay_depths=depths)
    for a, b in zip(swapped, (heat, cover, ov)):
        assert torch.equal(a.flip(0), b)
    torch.cuda.synchronize()


def test_paint_refuses_what_it_does_not_cover(golden):
    g = golden("qmap.npz")
    src, _, _, tok, dims = _case_source(g, "240x300_a8", 7)
    tok_d = torch.from_numpy(tok).cuda()
    with pytest.raises(_abi.KvqError):
        kernels.quality_paint(src, tok_d, cell=3)
    with pytest.raises(_abi.KvqError, match="kvq_quality_paint"):
        kernels.quality_paint(src, tok_d[:, :3].contiguous())                 # T != 2 D
    with pytest.raises(_abi.KvqError, match="kvq_quality_paint"):
        kernels.quality_paint(src, torch.zeros(2, 4, 5, 7, device="cuda"))    # 224 rows do not split into 5 token rows
    with pytest.raises(_abi.KvqError):
        kernels.quality_paint(src, tok_d[:1].contiguous())                    # one map for two clips
    with pytest.raises(_abi.KvqError, match="overlay depth"):
        kernels.quality_paint(src, tok_d, overlay_depths=(4,))
    v = torch.zeros(3, 8, 240, 300, dtype=torch.uint8, device="cuda")
    z = torch.zeros(7, 7, 8, dtype=torch.int32, device="cuda")
    odd = kernels.FragmentSource([v], [z], [z], 7, 7, 32, 32, 1)              # aligned = 1
    assert not kernels.quality_paint_supported(odd, (4, 7, 7))
    with pytest.raises(_abi.KvqError, match="kvq_quality_paint"):
        kernels.quality_paint(odd, tok_d[:1].contiguous())
    torch.cuda.synchronize()


# ---- harness ---------------------------------------------------------------------------------------------------------------------
def _harness_cfg(tmp, maps, graph):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "kwai_swin_grpb_qmap_test.yml")))
    a = cfg["data"]["val"]["args"]
    a.update(num_videos=7, frames=64, height=300, width=400, seed_per_item=True)
    a["sample_types"]["technical"].update(clip_len=32, num_clips=2)
    cfg.update(hipgraph=graph, streams=2)            # 3 - 4 videos per lane: each lane's two pinned buffer sets are reused
    if maps:
        cfg["quality_maps"].update(dir=str(tmp / f"maps_{graph}"), overlay_frames=2)
    else:
        cfg.pop("quality_maps")
    return cfg


def _run_harness(tmp, monkeypatch, maps, graph):
    from kvq_amd.trainer import Trainer
    run = tmp / f"run_{int(maps)}_{graph}"
    run.mkdir()
    monkeypatch.chdir(run)
    torch.manual_seed(0)                                # the network's own initialisation: the same weights in every run
    t = Trainer(types.SimpleNamespace(gpu_id="0"), _harness_cfg(tmp, maps, graph))
    t.inferece_test()
    torch.cuda.synchronize()
    return t, (run / "output.txt").read_bytes()


@pytest.mark.parametrize("graph", ["on", "off"])
def test_harness_writes_one_file_per_video_and_leaves_the_scores_alone(tmp_path, monkeypatch, graph):
    from kvq_amd.datasets import SyntheticKVQDataset
    _, plain = _run_harness(tmp_path, monkeypatch, False, graph)
    t, with_maps = _run_harness(tmp_path, monkeypatch, True, graph)
    assert with_maps == plain                                            # output.txt: byte-identical
    if graph == "on":
        replays, eager = t.graph_stats
        assert replays > 0 and eager == 0
    lines = with_maps.decode().strip().splitlines()
    mdir = tmp_path / f"maps_{graph}"
    assert sorted(os.listdir(mdir)) == sorted(l.split(",")[0] + ".npz" for l in lines) and len(lines) == 7
    cfg = _harness_cfg(tmp_path, True, graph)
    ds = SyntheticKVQDataset(cfg["data"]["val"]["args"], None, device="cuda:0")
    for i, line in enumerate(lines):
        name, score = line.split(",")
        z = np.load(mdir / (name + ".npz"))
        assert set(z.files) == {"score", "token_map", "timeline", "frame_inds", "heat", "cover", "overlay"}
        tok = z["token_map"]
        assert tok.shape == (2, 16, 7, 7) and z["timeline"].shape == (2, 16) and z["frame_inds"].shape == (2, 16, 2)
        assert float(z["score"]) == float(score)
        # fp32 rounding of a mean of 2 * 784 values of this size
        bound = (tok.size + 8) * 2.0 ** -24 * max(1.0, float(np.abs(tok).max()))
        assert abs(float(tok.astype(np.float64).mean()) - float(score)) <= bound
        assert np.abs(z["timeline"].astype(np.float64) - tok.astype(np.float64).mean((2, 3))).max() <= bound
        assert z["heat"].shape == z["cover"].shape == (2, 16, 38, 50) and z["overlay"].shape == (2, 2, 3, 300, 400)
        if i in (0, 3, 6):                                               # the item's own draws, through the numpy reference
            item = ds[i]
            assert np.array_equal(z["frame_inds"].reshape(-1), np.asarray(item["frame_inds"]).reshape(-1))
            src = item["technical"].split_clips(2)
            for b in range(2):
                r0, c0, sh, sw = QR.token_rects(src.hoffs[b].cpu().numpy(), src.woffs[b].cpu().numpy(), 16, 7, 7, 32, 32, 8)
                heat, cover = QR.paint(r0, c0, sh, sw, tok[b], 300, 400, 8)
                assert np.array_equal(z["heat"][b].view(np.uint32), heat.view(np.uint32)) and np.array_equal(z["cover"][b], cover)
                h1, c1 = QR.paint(r0, c0, sh, sw, tok[b], 300, 400, 1)
                frames = src.videos[b].cpu().numpy()
                for n, d in enumerate((4, 12)):
                    assert np.array_equal(z["overlay"][b, n], QR.overlay(frames[:, 2 * d], h1[d], c1[d], tok.min(), tok.max()))


def test_harness_lazy_false_gets_the_token_maps_only(tmp_path, monkeypatch, capfd):
    from kvq_amd.trainer import Trainer
    cfg = _harness_cfg(tmp_path, True, "off")
    cfg["data"]["val"]["args"]["sample_types"]["technical"]["lazy"] = False
    cfg["data"]["val"]["args"]["num_videos"] = 3
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    Trainer(types.SimpleNamespace(gpu_id="0"), cfg).inferece_test()
    files = sorted(os.listdir(tmp_path / "maps_off"))
    assert len(files) == 3
    z = np.load(tmp_path / "maps_off" / files[0])
    assert set(z.files) == {"score", "token_map", "timeline", "frame_inds"}
    err = capfd.readouterr().err
    assert err.count("quality maps:") == 1 and "lazy: false" in err
