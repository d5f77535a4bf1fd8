"""Quality maps through KSVQE's region windows, host side (no GPU): the C entry points, the geometry rule, the restated token
rectangles against the reference's own sampler and RegionNet_CLIP (tests/golden/qmap_regions.npz), the network's `regions` entry and
the Trainer's notes and file writer."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import kvq_amd  # noqa: F401
from kvq_amd import _abi, _build, kernels
from kvq_amd.trainer import Trainer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qmap_ref as QR  # noqa: E402
import qmap_regions_ref as RR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kvq_quality_paint_regions_supported", "kvq_quality_paint_regions")
CASES = ("300x340_a8", "288x288_a2")
STRADDLING = (0, 1, 2)             # T = 8: key frames 1, 3, 5 -> the frame pairs of depth slices 0, 1, 2 lie in two groups each


def _src(Hs=300, Ws=340, Fh=9, Fw=9, fs_h=32, fs_w=32, aligned=8, n_clips=1):
    f = _abi.KvqFragmentSource()
    f.n_clips, f.src_is_u8, f.Hs, f.Ws = n_clips, 1, Hs, Ws
    f.Fh, f.Fw, f.fs_h, f.fs_w, f.aligned = Fh, Fw, fs_h, fs_w, aligned
    return f


def test_entry_points_are_declared_and_exported():
    header = open(_build.HEADER).read()
    declared = set(re.findall(r"\b(kvq_[a-z0-9_]+)\s*\(", header))
    handle = _abi.lib()
    for name in NEW:
        assert name in declared and name in _abi.SYMBOLS
        assert hasattr(handle, name)
    assert "KvqQualityPaintRegionArgs" in header
    assert handle.kvq_abi_version() == 32 and "#define KVQ_ABI_VERSION 32" in header
    # the structs the existing entry points take keep their sizes; the new one is the old one plus its five fields
    assert C.sizeof(_abi.KvqQualityPaintRegionArgs) == C.sizeof(_abi.KvqQualityPaintArgs) + 8 + 4 * 4
    # NULL arguments: an error code, never a crash
    assert handle.kvq_quality_paint_regions(None, None) == -1
    assert handle.kvq_quality_paint_regions(C.byref(_abi.KvqQualityPaintRegionArgs()), None) == -1
    assert handle.kvq_quality_paint_regions_supported(None, 8, 4, 7, 7, 8, 32, 7, 7) == 0
    f = _src()
    a = _abi.KvqQualityPaintRegionArgs()
    a.paint.src = C.pointer(f)
    a.paint.T, a.paint.D, a.paint.Hf, a.paint.Wf, a.paint.cell = 8, 4, 7, 7, 8
    a.anchor, a.kh, a.kw = 32, 7, 7
    a.paint.tok_map = a.paint.heat = a.paint.cover = 64            # never read: the region pointer is still NULL
    assert handle.kvq_quality_paint_regions(C.byref(a), None) == -1


# (T, D, Hf, Wf, cell, anchor, kh, kw, source, want)
TABLE = [
    (8, 4, 7, 7, 8, 32, 7, 7, dict(), 1),                                          # KSVQE: 9 x 9 canvas, 7 x 7 window
    (8, 4, 7, 7, 1, 32, 7, 7, dict(Hs=288, Ws=288, aligned=2), 1),
    (8, 4, 14, 14, 8, 32, 7, 7, dict(), 1),                                        # sh = 16
    (8, 4, 4, 4, 8, 32, 2, 2, dict(Hs=131, Ws=157, Fh=4, Fw=4), 1),                # the small synthetic geometry
    (8, 4, 7, 7, 8, 32, 9, 9, dict(), 0),                                          # 288 / 7 is no integer
    (8, 4, 9, 9, 8, 32, 9, 9, dict(), 1),                                          # kh == gh: one window
    (8, 4, 10, 10, 8, 32, 10, 10, dict(), 0),                                      # kh > gh
    (8, 4, 7, 7, 8, 32, 7, 10, dict(), 0),                                         # kw > gw
    (8, 4, 7, 7, 8, 32, 0, 7, dict(), 0),                                          # kh < 1
    (8, 4, 7, 7, 8, 0, 7, 7, dict(), 0),
    (8, 4, 7, 7, 8, 64, 7, 7, dict(), 0),                                          # 288 % 64: the canvas is no whole number of anchors
    (8, 4, 2, 2, 8, 48, 2, 2, dict(Fh=3, Fw=3), 0),                                # anchor 48, sh 48: fs_h % sh != 0
    (8, 4, 2, 2, 8, 24, 4, 4, dict(Hs=240, Ws=300, Fh=2, Fw=2, fs_h=48, fs_w=48), 0),   # sh = 48 divides fs, but anchor % sh != 0
    (8, 4, 3, 3, 8, 24, 2, 2, dict(Hs=240, Ws=300, Fh=2, Fw=2, fs_h=48, fs_w=48), 0),   # sh = 16 divides fs 48, but anchor 24 % 16 != 0
    (8, 4, 6, 6, 8, 24, 2, 2, dict(Hs=240, Ws=300, Fh=2, Fw=2, fs_h=48, fs_w=48), 1),   # sh = 8: divides anchor 24 and fs 48
    (8, 4, 7, 5, 8, 32, 7, 7, dict(), 0),                                          # 224 / 5 is no integer
    (8, 4, 7, 7, 3, 32, 7, 7, dict(), 0),                                          # cell
    (8, 8, 7, 7, 8, 32, 7, 7, dict(), 0),                                          # T != 2 D
    (8, 4, 7, 7, 8, 32, 7, 7, dict(aligned=1), 0),                                 # odd aligned
    (8, 4, 7, 7, 8, 32, 7, 7, dict(aligned=16), 0),                                # T % aligned
    (8, 4, 56, 28, 8, 32, 7, 7, dict(), 0),                                        # Hf Wf > 1024
    (8, 4, 7, 7, 8, 32, 7, 7, dict(n_clips=17), 0),
    (8, 4, 7, 7, 8, 32, 7, 7, dict(n_clips=0), 0),
    # the region-free geometries of the existing paint's table, with the window equal to the canvas
    (8, 4, 7, 7, 8, 32, 7, 7, dict(Hs=240, Ws=300, Fh=7, Fw=7, aligned=8), 1),
    (8, 4, 7, 7, 1, 32, 7, 7, dict(Hs=270, Ws=480, Fh=7, Fw=7, aligned=4), 1),
    (16, 8, 7, 7, 8, 32, 7, 7, dict(Hs=540, Ws=960, Fh=7, Fw=7, aligned=8), 1),
    (8, 4, 7, 7, 32, 32, 7, 7, dict(Hs=224, Ws=224, Fh=7, Fw=7, aligned=8), 1),
    (8, 4, 7, 7, 8, 32, 7, 7, dict(Hs=231, Ws=257, Fh=7, Fw=7, aligned=2), 1),
    (8, 4, 14, 14, 8, 32, 7, 7, dict(Hs=270, Ws=480, Fh=7, Fw=7, aligned=4), 1),
    (8, 4, 3, 3, 8, 48, 2, 2, dict(Hs=240, Ws=300, Fh=2, Fw=2, fs_h=48, fs_w=48, aligned=8), 0),   # sh = 32: a token straddles two patches
    (8, 4, 6, 6, 8, 48, 2, 2, dict(Hs=240, Ws=300, Fh=2, Fw=2, fs_h=48, fs_w=48, aligned=8), 1),
    (8, 4, 32, 32, 8, 32, 1, 1, dict(Hs=240, Ws=300, Fh=1, Fw=1, aligned=8), 1),                   # one pixel per token
    (8, 4, 28, 28, 8, 32, 7, 7, dict(Hs=240, Ws=300, Fh=7, Fw=7, aligned=8), 1),
]


@pytest.mark.parametrize("T,D,Hf,Wf,cell,anchor,kh,kw,kwargs,want", TABLE)
def test_regions_supported_truth_table(T, D, Hf, Wf, cell, anchor, kh, kw, kwargs, want):
    f = _src(**kwargs)
    got = _abi.lib().kvq_quality_paint_regions_supported(C.byref(f), T, D, Hf, Wf, cell, anchor, kh, kw)
    assert got == want
    assert RR.supported(T, D, Hf, Wf, f.Fh, f.Fw, f.fs_h, f.fs_w, f.aligned, anchor, kh, kw, cell, f.n_clips) == bool(want)
    if kh * anchor == f.Fh * f.fs_h and kw * anchor == f.Fw * f.fs_w and f.fs_h % anchor == 0 and f.fs_w % anchor == 0 and want:
        # the window is the canvas: what the existing paint supports
        assert _abi.lib().kvq_quality_paint_supported(C.byref(f), T, D, Hf, Wf, cell) == 1
        assert QR.supported(T, D, Hf, Wf, f.Fh, f.Fw, f.fs_h, f.fs_w, f.aligned, cell, f.n_clips)


@pytest.mark.parametrize("phase,want", [(0, None), (1, None), (2, -3), (-1, -3)])
def test_the_call_refuses_a_phase_outside_0_1(phase, want):
    """the supported query has no phase argument: the call checks it, in front of anything it would read or launch"""
    assert RR.supported(8, 4, 7, 7, 9, 9, 32, 32, 8, 32, 7, 7, phase=phase) == (want is None)
    if want is None:
        return                                         # a supported call would launch: that is the GPU tests' ground
    f = _src()
    a = _abi.KvqQualityPaintRegionArgs()
    a.paint.src = C.pointer(f)
    a.paint.T, a.paint.D, a.paint.Hf, a.paint.Wf, a.paint.cell = 8, 4, 7, 7, 8
    a.paint.tok_map = a.paint.heat = a.paint.cover = a.region = 64           # never read: the geometry check comes first
    a.anchor, a.kh, a.kw, a.phase = 32, 7, 7, phase
    assert _abi.lib().kvq_quality_paint_regions(C.byref(a), None) == want
    a.phase, a.kh = 0, 10
    assert _abi.lib().kvq_quality_paint_regions(C.byref(a), None) == -3


@pytest.mark.parametrize("case", CASES)
def test_token_rectangles_are_the_reference_windows(golden, case):
    """for each phase, the rectangles restated in qmap_regions_ref (and kvq_hip.h), built from the draws and the window indices, cover
    exactly the source pixels the reference's get_spatial_fragments + RegionNet_CLIP handed to each token on clip frame 2d + phase"""
    g = golden("qmap_regions.npz")
    T, H, W, aligned, Hf, Wf, Fh, Fw, fs, anchor, kh, kw = (int(v) for v in g[f"{case}/meta"])
    tokid, regions = g[f"{case}/tokid"], g[f"{case}/regions"]
    assert tokid.shape == (T, H, W) and tokid.dtype == np.int16 and regions.shape == (T,)
    assert len(set(regions[[0, 1, 3, 5]].tolist())) == 4              # a different window on every key-frame group
    D = T // 2
    rects = {}
    for phase in (0, 1):
        assert RR.supported(T, D, Hf, Wf, Fh, Fw, fs, fs, aligned, anchor, kh, kw, phase=phase)
        r0, c0, sh, sw, valid = RR.token_rects_regions(g[f"{case}/hoff"], g[f"{case}/woff"], regions, D, Hf, Wf, fs, fs, aligned,
                                                       anchor, kh, kw, phase)
        assert valid.all() and (sh, sw) == (32, 32)
        assert np.array_equal(RR.token_ids(r0, c0, sh, sw, valid, H, W), tokid[phase::2])
        rects[phase] = (r0, c0)
        # the paint at cell 1 is that map read as scores
        scores = np.random.Generator(np.random.PCG64(3 + phase)).standard_normal((D, Hf, Wf)).astype(np.float32)
        heat, cover = RR.paint(r0, c0, sh, sw, valid, scores, H, W, 1)
        flat = np.concatenate([np.zeros((D, 1), np.float32), scores.reshape(D, -1)], 1)
        want = np.take_along_axis(flat, tokid[phase::2].reshape(D, -1).astype(np.int64), 1).reshape(D, H, W)
        assert np.array_equal(heat, want) and np.array_equal(cover, (tokid[phase::2] > 0).astype(np.float32))
    for d in range(D):
        same = np.array_equal(rects[0][0][d], rects[1][0][d]) and np.array_equal(rects[0][1][d], rects[1][1][d])
        assert same == (d not in STRADDLING), d
        assert (regions[2 * d] != regions[2 * d + 1]) == (d in STRADDLING)


def test_a_region_value_that_names_no_window_leaves_its_slice_uncovered(golden):
    g = golden("qmap_regions.npz")
    case = CASES[0]
    T, H, W, aligned, Hf, Wf, Fh, Fw, fs, anchor, kh, kw = (int(v) for v in g[f"{case}/meta"])
    assert RR.window_grid(Fh, Fw, fs, fs, anchor, kh, kw) == (3, 3)
    regions = g[f"{case}/regions"].copy()
    regions[2], regions[6] = -1, 9
    r0, c0, sh, sw, valid = RR.token_rects_regions(g[f"{case}/hoff"], g[f"{case}/woff"], regions, T // 2, Hf, Wf, fs, fs, aligned,
                                                   anchor, kh, kw, 0)
    assert valid.tolist() == [True, False, True, False]
    heat, cover = RR.paint(r0, c0, sh, sw, valid, np.ones((T // 2, Hf, Wf), np.float32), H, W, 8)
    assert not heat[1].any() and not cover[3].any() and cover[0].any() and heat[2].any()


# ---- network: `regions` rides in the maps of a backbone that keeps them ---------------------------------------------------------
class _Backbone(torch.nn.Module):
    def __init__(self, with_regions):
        super().__init__()
        self.kwargs, self.with_regions = None, with_regions
        if with_regions:
            self.last_regions = None

    def forward(self, inputs, multi=False, layer=-1, **kwargs):
        self.kwargs = kwargs
        feat = inputs["feat5"]
        if self.with_regions:                                  # set BY the forward: the network must read it afterwards
            self.last_regions = torch.arange(feat.shape[0] * 2 * feat.shape[2], dtype=torch.int32).reshape(feat.shape[0], -1)
        return feat, None


def _fake_vqa_head(feat, w1, b1, w2, b2, w1t=None, return_map=False):
    B = feat.shape[0]
    tok = feat.mean(1)
    score = tok.mean((1, 2, 3)).reshape(B, 1)
    return (score, tok, tok.mean((2, 3))) if return_map else score


def _net(monkeypatch, with_regions):
    from kvq_amd.models import head as head_mod
    from kvq_amd.models.model import VQA_Network
    monkeypatch.setattr(head_mod.kernels, "vqa_head", _fake_vqa_head)
    net = VQA_Network.__new__(VQA_Network)
    torch.nn.Module.__init__(net)
    net.key_names, net.multi, net.layer = ["KSVQE"], False, -1
    net.KSVQE_backbone, net.KSVQE_head = _Backbone(with_regions), head_mod.VQAHead(8, 4)
    return net


def test_network_maps_carry_the_regions_of_a_backbone_that_keeps_them(monkeypatch):
    x = {"feat5": torch.arange(2 * 8 * 2 * 3 * 3, dtype=torch.float32).reshape(2, 8, 2, 3, 3)}
    net = _net(monkeypatch, True)
    plain = net(inputs=x, reduce_scores=True)
    (pred, loss), maps = net(inputs=x, reduce_scores=True, return_maps=True)
    assert loss is None and torch.equal(pred, plain[0]) and set(maps) == {"KSVQE"}
    m = maps["KSVQE"]
    assert set(m) == {"token_map", "timeline", "regions"}
    assert m["regions"] is net.KSVQE_backbone.last_regions and m["regions"].shape == (2, 4) and m["regions"].dtype == torch.int32
    assert net.KSVQE_backbone.kwargs == {}                       # nothing new is passed into the backbone
    net = _net(monkeypatch, False)
    (_, _), maps = net(inputs=x, reduce_scores=True, return_maps=True)
    assert set(maps["KSVQE"]) == {"token_map", "timeline"}


def test_ksvqe_keeps_the_regions_as_an_attribute_not_as_state():
    from kvq_amd.models.backbones import ksvqe_modules as KM
    net = KM.RegionNet_CLIP(k=49, anchor_size=32, stride=1)
    assert net.last_regions is None and dict(net.state_dict()) == {}
    from kvq_amd.models.backbones.KSVQE_model import KSVQE
    assert isinstance(KSVQE.last_regions, property)


# ---- Trainer ---------------------------------------------------------------------------------------------------------------------
def _bare_trainer(config):
    t = Trainer.__new__(Trainer)
    t.config = config
    return t


def _lazy_item(upsampled=False):
    src = kernels.FragmentSource.__new__(kernels.FragmentSource)
    src.upsampled = upsampled
    return {"fragment": src}


def test_ksvqe_notes_one_line_per_reason(capsys):
    t = _bare_trainer({"model": {"type": "KSVQE"}})
    out = {"pred": None, "KSVQE/token_map": None}
    t._maps_note(out, {})
    t._maps_note(dict(out, **{"KSVQE/heat": None}), {"fragment": torch.zeros(1)})
    assert capsys.readouterr().err == ""                       # no fragment entry / a painted sample: silence
    for _ in range(3):
        t._maps_note(out, {"fragment": torch.zeros(1)})
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "lazy: false" in err and "token_map, timeline and frame_inds only" in err
    for _ in range(2):
        t._maps_note(out, _lazy_item(upsampled=True))
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "upsample fallback" in err
    for _ in range(2):
        t._maps_note(out, _lazy_item())
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "does not cover this sampler geometry" in err
    t._maps_note(out, {"fragment": torch.zeros(1)})
    assert capsys.readouterr().err == ""                       # every reason was said once


def test_map_files_decode_the_regions(tmp_path):
    t = _bare_trainer({"model": {"type": "KSVQE"}})
    t._region_row = {"KSVQE": 3}
    qm = {"dir": str(tmp_path), "cell": 8, "overlay_frames": 0}
    tok = torch.zeros(1, 4, 7, 7)
    host = {"pred": torch.tensor([[1.0]]), "KSVQE/token_map": tok, "KSVQE/timeline": tok.mean((2, 3)),
            "KSVQE/heat": torch.zeros(1, 4, 38, 43), "KSVQE/cover": torch.zeros(1, 4, 38, 43),
            "KSVQE/regions": torch.tensor([[2, 4, 4, 6, 6, 5, 5, 5]], dtype=torch.int32), "score": 1.0}
    z = np.load(t._maps_write(qm, "v.mp4", host, {"frame_inds": np.arange(8)}))
    assert set(z.files) == {"score", "token_map", "timeline", "frame_inds", "heat", "cover", "regions"}
    assert z["regions"].dtype == np.int32 and z["regions"].shape == (1, 8, 2)
    assert z["regions"][0].tolist() == [[0, 2], [1, 1], [1, 1], [2, 0], [2, 0], [1, 2], [1, 2], [1, 2]]


def test_the_ksvqe_qmap_yml_is_the_ksvqe_yml_plus_the_key():
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "Kwai_KSVQE_qmap_test.yml")))
    base = yaml.safe_load(open(os.path.join(ROOT, "config", "Kwai_KSVQE_test.yml")))
    assert _bare_trainer(cfg)._quality_maps() == {"dir": "quality_maps", "cell": 8, "overlay_frames": 0}
    assert _bare_trainer(base)._quality_maps() is None
    cfg.pop("quality_maps")
    assert cfg["data"]["val"]["args"]["sample_types"]["technical"].pop("lazy") is True
    assert cfg == base
