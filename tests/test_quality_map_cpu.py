"""Local quality maps, host side (no GPU): the C entry points, the paint's geometry rule, the restated token rectangles against the
reference's own sampler (tests/golden/qmap.npz), the network's return structures and the Trainer's yml key and file writer."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import kvq_amd  # noqa: F401
from kvq_amd import _abi, _build
from kvq_amd.trainer import Trainer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qmap_ref as QR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kvq_vqa_head_map", "kvq_quality_paint_supported", "kvq_quality_paint")
CASES = ("240x300_a8", "270x480_a4", "540x960_a8", "224x224_a8", "231x257_a2", "270x480_a4_s16")


def test_entry_points_are_declared_and_exported():
    header = open(_build.HEADER).read()
    declared = set(re.findall(r"\b(kvq_[a-z0-9_]+)\s*\(", header))
    handle = _abi.lib()
    for name in NEW:
        assert name in declared and name in _abi.SYMBOLS
        assert hasattr(handle, name)
    assert handle.kvq_abi_version() == 32 and "#define KVQ_ABI_VERSION 32" in header
    # NULL arguments: an error code, never a crash
    assert handle.kvq_vqa_head_map(None, 1, 4, 8, 0, 0, 0, None, None, None, 8, None, None, 2, None, None, None, None) == -1
    assert handle.kvq_quality_paint(None, None) == -1
    assert handle.kvq_quality_paint(C.byref(_abi.KvqQualityPaintArgs()), None) == -1
    assert handle.kvq_quality_paint_supported(None, 8, 4, 7, 7, 8) == 0


def _src(Hs, Ws, Fh=7, Fw=7, fs_h=32, fs_w=32, aligned=8, n_clips=1):
    f = _abi.KvqFragmentSource()
    f.n_clips, f.src_is_u8, f.Hs, f.Ws = n_clips, 1, Hs, Ws
    f.Fh, f.Fw, f.fs_h, f.fs_w, f.aligned = Fh, Fw, fs_h, fs_w, aligned
    return f


@pytest.mark.parametrize("T,D,Hf,Wf,cell,kw,want", [
    (8, 4, 7, 7, 8, dict(Hs=240, Ws=300, aligned=8), 1),
    (8, 4, 7, 7, 1, dict(Hs=270, Ws=480, aligned=4), 1),
    (16, 8, 7, 7, 8, dict(Hs=540, Ws=960, aligned=8), 1),
    (8, 4, 7, 7, 32, dict(Hs=224, Ws=224, aligned=8), 1),
    (8, 4, 7, 7, 8, dict(Hs=231, Ws=257, aligned=2), 1),
    (8, 4, 14, 14, 8, dict(Hs=270, Ws=480, aligned=4), 1),        # two token rows per mini-patch
    (8, 4, 7, 7, 8, dict(Hs=240, Ws=300, aligned=1), 0),          # odd aligned: a token's two frames could differ in their draws
    (9, 3, 7, 7, 8, dict(Hs=240, Ws=300, aligned=3), 0),
    (8, 8, 7, 7, 8, dict(Hs=240, Ws=300, aligned=8), 0),          # T != 2 D
    (8, 4, 7, 7, 8, dict(Hs=240, Ws=300, aligned=16), 0),         # T % aligned
    (8, 4, 3, 3, 8, dict(Hs=240, Ws=300, Fh=2, Fw=2, fs_h=48, fs_w=48, aligned=8), 0),   # fs = 48, sh = 32: a token straddles two patches
    (8, 4, 6, 6, 8, dict(Hs=240, Ws=300, Fh=2, Fw=2, fs_h=48, fs_w=48, aligned=8), 1),   # fs = 48, sh = 16
    (8, 4, 5, 7, 8, dict(Hs=240, Ws=300, aligned=8), 0),          # 224 / 5 is no integer
    (8, 4, 7, 7, 3, dict(Hs=240, Ws=300, aligned=8), 0),          # cell
    (8, 4, 7, 7, 64, dict(Hs=240, Ws=300, aligned=8), 0),
    (8, 4, 56, 28, 8, dict(Hs=240, Ws=300, aligned=8), 0),        # Hf Wf > 1024
    (8, 4, 32, 32, 8, dict(Hs=240, Ws=300, Fh=1, Fw=1, aligned=8), 1),   # Hf Wf == 1024 (one pixel per token)
    (8, 4, 28, 28, 8, dict(Hs=240, Ws=300, aligned=8), 1),
    (8, 4, 7, 7, 8, dict(Hs=240, Ws=300, aligned=8, n_clips=17), 0),
    (8, 4, 7, 7, 8, dict(Hs=240, Ws=300, aligned=8, n_clips=0), 0),
])
def test_paint_supported_truth_table(T, D, Hf, Wf, cell, kw, want):
    f = _src(**kw)
    got = _abi.lib().kvq_quality_paint_supported(C.byref(f), T, D, Hf, Wf, cell)
    assert got == want
    assert QR.supported(T, D, Hf, Wf, f.Fh, f.Fw, f.fs_h, f.fs_w, f.aligned, cell, f.n_clips) == bool(want)


@pytest.mark.parametrize("case", CASES)
def test_token_rectangles_are_the_reference_samplers(golden, case):
    """the rectangles restated in qmap_ref (and kvq_hip.h), built from the draws, cover exactly the source pixels the reference's
    get_spatial_fragments handed to each token"""
    g = golden("qmap.npz")
    T, H, W, aligned, Hf, Wf, Fh, Fw, fs = (int(v) for v in g[f"paint/{case}/meta"])
    tokid = g[f"paint/{case}/tokid"]
    assert tokid.shape == (T // 2, H, W) and tokid.dtype == np.int16
    assert QR.supported(T, T // 2, Hf, Wf, Fh, Fw, fs, fs, aligned)
    r0, c0, sh, sw = QR.token_rects(g[f"paint/{case}/hoff"], g[f"paint/{case}/woff"], T // 2, Hf, Wf, fs, fs, aligned)
    assert np.array_equal(QR.token_ids(r0, c0, sh, sw, H, W), tokid)
    # ... and the paint at cell 1 is that map read as scores: heat = score of the token that saw the pixel, cover = seen or not
    scores = np.random.Generator(np.random.PCG64(3)).standard_normal((T // 2, Hf, Wf)).astype(np.float32)
    heat, cover = QR.paint(r0, c0, sh, sw, scores, H, W, 1)
    flat = np.concatenate([np.zeros((T // 2, 1), np.float32), scores.reshape(T // 2, -1)], 1)
    want = np.take_along_axis(flat, tokid.reshape(T // 2, -1).astype(np.int64), 1).reshape(tokid.shape)
    assert np.array_equal(heat, want) and np.array_equal(cover, (tokid > 0).astype(np.float32))
    # a coarser cell conserves the painted mass: sum(heat * cover * block) == sum over the seen pixels, to fp32 rounding
    heat8, cover8 = QR.paint(r0, c0, sh, sw, scores, H, W, 8)
    assert heat8.shape == (T // 2, -(-H // 8), -(-W // 8))
    ky, kx = np.arange(heat8.shape[1]), np.arange(heat8.shape[2])
    block = np.outer(np.minimum(ky * 8 + 8, H) - ky * 8, np.minimum(kx * 8 + 8, W) - kx * 8)
    assert np.allclose((heat8.astype(np.float64) * cover8 * block).sum(), want.astype(np.float64).sum(), rtol=0, atol=1e-2)
    assert np.array_equal(np.rint(cover8 * block).astype(np.int64).sum((1, 2)), (tokid > 0).sum((1, 2)))


def test_overlay_arithmetic():
    frames = np.random.Generator(np.random.PCG64(1)).integers(0, 256, (3, 4, 5)).astype(np.uint8)
    heat = np.linspace(-1, 2, 20, dtype=np.float32).reshape(4, 5)
    cover = np.ones((4, 5), np.float32)
    cover[0] = 0
    out = QR.overlay(frames, heat, cover, 0.0, 1.0, alpha=256, dim=0)
    assert (out[:, 0] == 0).all()                                        # uncovered, dim 0
    assert (out[2, 1:] == 0).all() and (out[0, 1:].astype(int) + out[1, 1:] == 255).all()     # alpha 256: the colour alone
    assert out[1, 3, 4] == 255 and out[1, 1, 0] == 0                      # clamped at both ends
    same = QR.overlay(frames, heat, cover, 0.0, 1.0, alpha=0, dim=256)
    assert np.array_equal(same, frames)
    flat = QR.overlay(frames, np.full((4, 5), 0.5, np.float32), cover, 0.5, 0.5)      # hi == lo == s: 0 * inf counts as q = 0
    assert (flat[1, 1:] == (frames[1, 1:].astype(int) * 128 + 128) >> 8).all()


# ---- network: the default return structures are untouched ----------------------------------------------------------------------
class _Backbone(torch.nn.Module):
    def __init__(self, ksvqe):
        super().__init__()
        self.ksvqe, self.kwargs = ksvqe, None

    def forward(self, inputs, multi=False, layer=-1, **kwargs):
        self.kwargs = kwargs
        feat = inputs["feat5"]
        return (feat, None) if self.ksvqe else feat


def _fake_vqa_head(feat, w1, b1, w2, b2, w1t=None, return_map=False):
    B, _, D, H, W = feat.shape
    tok = feat.mean(1)
    score = tok.mean((1, 2, 3)).reshape(B, 1)
    return (score, tok, tok.mean((2, 3))) if return_map else score


def _net(monkeypatch, keys=("swin_tiny_grpb",)):
    from kvq_amd.models import head as head_mod
    from kvq_amd.models.model import VQA_Network
    monkeypatch.setattr(head_mod.kernels, "vqa_head", _fake_vqa_head)
    net = VQA_Network.__new__(VQA_Network)
    torch.nn.Module.__init__(net)
    net.key_names, net.multi, net.layer = list(keys), False, -1
    for k in keys:
        setattr(net, k + "_backbone", _Backbone(k == "KSVQE"))
        setattr(net, k + "_head", head_mod.VQAHead(8, 4))
    return net


def test_network_forward_default_return_is_unchanged(monkeypatch):
    x = {"feat5": torch.arange(2 * 8 * 2 * 3 * 3, dtype=torch.float32).reshape(2, 8, 2, 3, 3)}
    net = _net(monkeypatch)
    s = net(inputs=x, reduce_scores=True)
    assert torch.is_tensor(s) and s.shape == (2, 1)
    assert isinstance(net(inputs=x), list) and len(net(inputs=x)) == 1
    sf = net(inputs=x, reduce_scores=True, return_pooled_feats=True)
    assert isinstance(sf, tuple) and len(sf) == 2 and set(sf[1]) == {"swin_tiny_grpb"}
    out, maps = net(inputs=x, reduce_scores=True, return_maps=True)
    assert torch.equal(out, s) and set(maps) == {"swin_tiny_grpb"}
    m = maps["swin_tiny_grpb"]
    assert set(m) == {"token_map", "timeline"} and m["token_map"].shape == (2, 2, 3, 3) and m["timeline"].shape == (2, 2)
    assert net.swin_tiny_grpb_backbone.kwargs == {}                     # return_maps does not leak into the backbone's kwargs
    (out, feats), maps = net(inputs=x, reduce_scores=True, return_pooled_feats=True, return_maps=True)
    assert torch.equal(out, s) and set(feats) == set(maps)
    # KSVQE: (scores, loss) stays (scores, loss); its VQAHead gives maps too
    net = _net(monkeypatch, ("KSVQE",))
    pred, loss = net(inputs=x, reduce_scores=True)
    assert loss is None and torch.equal(pred, s)
    (pred, loss), maps = net(inputs=x, reduce_scores=True, return_maps=True)
    assert loss is None and torch.equal(pred, s) and set(maps) == {"KSVQE"}


def test_head_map_refuses_the_other_branches(monkeypatch):
    from kvq_amd.models import head as head_mod
    monkeypatch.setattr(head_mod.kernels, "vqa_head_classes", lambda *a, **k: torch.zeros(1, 3))
    x = torch.zeros(1, 8, 2, 3, 3)
    with pytest.raises(NotImplementedError, match="pre_pool"):
        head_mod.VQAHead(8, 4, pre_pool=True)(x, return_map=True)
    with pytest.raises(NotImplementedError, match="num_class"):
        head_mod.VQAHead(8, 4, num_class=3)(x, return_map=True)
    assert head_mod.VQAHead(8, 4, num_class=3)(x).shape == (1, 3)        # without the map they run as before


# ---- Trainer: yml key and the file writer --------------------------------------------------------------------------------------
def _bare_trainer(config):
    t = Trainer.__new__(Trainer)
    t.config = config
    return t


def test_quality_maps_yml_key(tmp_path):
    import yaml
    assert _bare_trainer({})._quality_maps() is None
    assert _bare_trainer({"quality_maps": None})._quality_maps() is None
    assert _bare_trainer({"quality_maps": {"dir": "x"}})._quality_maps() == {"dir": "x", "cell": 8, "overlay_frames": 0}
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "kwai_swin_grpb_qmap_test.yml")))
    assert _bare_trainer(cfg)._quality_maps() == {"dir": "quality_maps", "cell": 8, "overlay_frames": 0}
    base = yaml.safe_load(open(os.path.join(ROOT, "config", "kwai_swin_grpb_synthetic_test.yml")))
    assert _bare_trainer(base)._quality_maps() is None
    cfg.pop("quality_maps"), cfg.pop("name"), base.pop("name")
    assert cfg == base                                                   # the qmap yml is the synthetic yml plus the key
    for bad in ({"cell": 8}, {"dir": "x", "cell": 3}, {"dir": "x", "overlay_frames": 17}, {"dir": "x", "colour": 1}, "x"):
        with pytest.raises(ValueError):
            _bare_trainer({"quality_maps": bad})._quality_maps()
    assert Trainer.overlay_depths(16, 0) == [] and Trainer.overlay_depths(16, 1) == [8]
    assert Trainer.overlay_depths(16, 4) == [2, 6, 10, 14] and Trainer.overlay_depths(2, 5) == [0, 1]


def test_map_files_one_model_key(tmp_path):
    t = _bare_trainer({"model": {"type": "swin_tiny_grpb"}})
    qm = {"dir": str(tmp_path / "maps"), "cell": 8, "overlay_frames": 0}
    tok = torch.arange(2 * 4 * 7 * 7, dtype=torch.float32).reshape(2, 4, 7, 7)
    host = {"pred": torch.tensor([[1.0], [2.0]]), "swin_tiny_grpb/token_map": tok, "swin_tiny_grpb/timeline": tok.mean((2, 3)),
            "swin_tiny_grpb/heat": torch.zeros(2, 4, 30, 38), "swin_tiny_grpb/cover": torch.ones(2, 4, 30, 38), "score": 1.5}
    path = t._maps_write(qm, "clips/video_7.mp4", host, {"frame_inds": np.arange(16) * 3})
    assert path == str(tmp_path / "maps" / "video_7.mp4.npz") and os.listdir(tmp_path / "maps") == ["video_7.mp4.npz"]
    z = np.load(path)
    assert set(z.files) == {"score", "token_map", "timeline", "frame_inds", "heat", "cover"}
    assert z["score"].dtype == np.float32 and float(z["score"]) == 1.5
    assert z["token_map"].shape == (2, 4, 7, 7) and z["timeline"].shape == (2, 4)
    assert z["frame_inds"].shape == (2, 4, 2) and z["frame_inds"][1, 0].tolist() == [24, 27]
    # a frame list that does not split into (clips, depth, 2) is left out; a dict of lists is read by view name
    z = np.load(t._maps_write(qm, "v", host, {"frame_inds": np.arange(7)}))
    assert "frame_inds" not in z.files
    z = np.load(t._maps_write(qm, "v", host, {"frame_inds": {"technical": np.arange(16)}}))
    assert z["frame_inds"].shape == (2, 4, 2)


def test_map_files_several_model_keys(tmp_path):
    t = _bare_trainer({"model": {"type": "a,b"}})
    qm = {"dir": str(tmp_path), "cell": 8, "overlay_frames": 0}
    tok = torch.zeros(1, 2, 7, 7)
    host = {"pred": torch.tensor([[3.0]]), "a/token_map": tok, "a/timeline": tok.mean((2, 3)), "b/token_map": tok + 1,
            "b/timeline": tok.mean((2, 3)) + 1}
    z = np.load(t._maps_write(qm, "v.mp4", host, {"frame_inds": np.arange(4)}))
    assert set(z.files) == {f"{k}/{n}" for k in "ab" for n in ("score", "token_map", "timeline", "frame_inds")}
    assert float(z["a/score"]) == float(z["b/score"]) == 3.0


def test_notes_say_why_a_sample_has_no_heat_once(capsys):
    t = _bare_trainer({"model": {"type": "swin_tiny_grpb"}})
    out = {"pred": None, "swin_tiny_grpb/token_map": None}
    for _ in range(3):
        t._maps_note(out, {"technical": torch.zeros(1)})
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "lazy: false" in err and "token_map, timeline and frame_inds only" in err
    t._maps_note(dict(out, **{"swin_tiny_grpb/heat": None}), {"technical": torch.zeros(1)})
    _bare_trainer({"model": {"type": "KSVQE"}})._maps_note(out, {})
    assert capsys.readouterr().err == ""
