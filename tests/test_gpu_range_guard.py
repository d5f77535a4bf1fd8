"""Range guard of the fp16 residual stream (kvq_swin3d_set_range_flags, SwinTransformer3D.range_flags, Trainer's re-score).

A writer of an fp16 stream stores a value past +-65504 as +-65504 (MODE.FP16_OVFL): each case below pushes exactly one stage's stream
out of range through one writer — the patch embedding, a token-per-lane tail, a wide tail, the fused PatchMerging, the reduction GEMM of
an un-fused merge — by a bias vector of 1e5 scale, checks that the fp32 stream really leaves the range, that exactly that stage's bit is
set, that the clamped score is wrong (beyond the 1e-3 gate) and that the fp32-stream score (residual16 = False) matches the CPU oracle."""
import types

import numpy as np
import pytest
import torch

import kvq_amd  # noqa: F401
from kvq_amd import _abi
from kvq_amd.utils import synth
from oracle import swin3d_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCORE_TOL = 1e-3
FP16_MAX = 65504.0


def _net(cfgn, wts, hw, dtype="fp16"):
    """the trunk of a synth config + the VQA head -> (clip -> scores, trunk)"""
    from kvq_amd.models.backbones.swin_backbone import SwinTransformer3D
    from kvq_amd.models.head import VQAHead
    cfg = getattr(synth, cfgn)
    bb = SwinTransformer3D(embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads), window_size=cfg.window,
                           frag_biases=cfg.frag_biases, operand_dtype=dtype)
    r = bb.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in wts.items()}, strict=False)
    assert not r.unexpected_keys
    head = VQAHead(in_channels=cfg.num_features, hidden_channels=64)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in hw.items()})
    bb, head = bb.to(DEV).eval(), head.to(DEV).eval()
    return (lambda x: head(bb({"technical": x}))), bb


def _score(net, bb, x, residual16=True):
    bb.residual16 = residual16
    bb.clear_range_flags()
    with torch.no_grad():
        s = net(x).float().cpu()
    flags = int(bb.range_flags().item())          # (synchronises)
    bb.residual16 = True
    return s, flags


TRUNK_T = ["t_grpb_stress_8x80", "t_grpb_stress_16x64", "t_plain_stress_16x96", "t_grpb_stress_10x50x70", "t_grpb_stress_32x224",
           "t_grpb_init_32x224"]


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("case", TRUNK_T)
def test_clean_weights_leave_the_word_zero_and_features_unchanged(golden, case, dtype):
    g = golden("trunk.npz")
    wseed, cseed, B, T, H, W = (int(v) for v in g[f"{case}/meta"])
    cfgn, scheme = str(g[f"{case}/cfg"]), str(g[f"{case}/scheme"])
    cfg = getattr(synth, cfgn)
    net, bb = _net(cfgn, synth.synth_swin_weights(cfg, wseed, scheme), synth.synth_vqa_head_weights(cfg.num_features, 64, wseed, scheme), dtype)
    x = torch.from_numpy(synth.synth_clip(cseed, T, H, W, batch=B)).to(DEV)
    bb.clear_range_flags()
    with torch.no_grad():
        f_on = bb({"technical": x}).clone()
        assert int(bb.range_flags().item()) == 0
        handle = bb._plan(B, T, H, W, torch.device(DEV))[0]
        _abi.check(_abi.lib().kvq_swin3d_set_range_flags(handle, None), "kvq_swin3d_set_range_flags")
        try:
            f_off = bb({"technical": x}).clone()
        finally:
            _abi.check(_abi.lib().kvq_swin3d_set_range_flags(handle, _abi.ptr(bb.range_flags())), "kvq_swin3d_set_range_flags")
    assert torch.equal(f_on, f_off)


def _oracle_block_max(x, wts, cfg):
    """fp32 CPU oracle: max |stream| behind the patch embedding and behind every Swin block, in block order"""
    seen = []
    blk, emb = O.swin_block, O.patch_embed

    def rec_blk(*a, **k):
        y = blk(*a, **k)
        seen.append(float(y.abs().max()))
        return y

    def rec_emb(*a, **k):
        y = emb(*a, **k)
        seen.append(float(y.abs().max()))
        return y
    O.swin_block, O.patch_embed = rec_blk, rec_emb
    try:
        with torch.no_grad():
            feat = O.swin3d_trunk(x, wts, cfg)
    finally:
        O.swin_block, O.patch_embed = blk, emb
    return seen, feat


def _outlier(n, seed=7):
    return (1e5 * np.random.Generator(np.random.PCG64(seed)).standard_normal(n)).astype(np.float32)


def _merge_bias(red_w, target=1e5, seed=9, cap=3e4):
    """norm bias u S of a PatchMerging with rms(red_w . u S) = target, every entry within +-cap (a 16-bit operand after the
    un-fused LayerNorm); red_w is scaled up instead where S would pass the cap"""
    u = np.random.Generator(np.random.PCG64(seed)).standard_normal(red_w.shape[1]).astype(np.float32)
    s = target / float(np.sqrt(np.mean((red_w @ u) ** 2)))
    f = max(1.0, s * float(np.abs(u).max()) / cap)
    return (u * s / f).astype(np.float32), (red_w * f).astype(np.float32)


# (writer, config, clip geometry, stage bit): B = 1, the smallest clips that keep every stage's stream in fp16
WRITERS = [
    ("embed", "SWIN_T_GRPB", (16, 64, 64), 0),
    ("tail_stage0", "SWIN_T_GRPB", (16, 64, 64), 0),
    ("tail_stage1", "SWIN_T_GRPB", (16, 64, 64), 1),
    ("tailmm_stage2", "SWIN_T_GRPB", (16, 64, 64), 2),
    ("fused_merge", "SWIN_T_GRPB", (16, 64, 64), 1),
    ("merge_gemm", "SWIN_B_GRPB", (16, 64, 64), 2),
    ("merge_gemm_one_channel", "SWIN_B_GRPB", (16, 64, 64), 2),
]

FEEDS_FUSED_MERGE = {"embed", "tail_stage0", "tail_stage1", "fused_merge"}


def _craft(writer, cfg, wts):
    w = {k: v.copy() for k, v in wts.items()}
    if writer == "embed":                          # stage 0 through the embedding's LayerNorm bias
        w["patch_embed.norm.bias"] = _outlier(cfg.embed_dim)
        return w, 0
    if writer.startswith("tail"):                  # fc2 bias of the first block of the stage
        st = {"tail_stage0": 0, "tail_stage1": 1, "tailmm_stage2": 2}[writer]
        k = f"layers.{st}.blocks.0.mlp.fc2.bias"
        w[k] = _outlier(w[k].shape[0])
        return w, 1 + sum(cfg.depths[:st])
    if writer == "merge_gemm_one_channel":
        # ONE output channel of the reduction GEMM out of range: channel 4 (~ +1.0e5) in every row, channel 2 (~ -1.0e3) negative in every
        # row — in the epilogue's 8-column chunk of a lane they are the low halves of packed pairs 2 and 1, so a fold that let a raw
        # negative half into the running max would lose channel 4.  The first stage-2 block's fc2 bias brings channel 4 back into range
        # (fp16 stream: 65504 - 5e4, fp32: 1.0e5 - 5e4), so no tail re-stores a saturated value: the GEMM alone has to set the bit
        w["layers.1.downsample.norm.bias"] = np.full(1024, 100.0, np.float32)
        r = w["layers.1.downsample.reduction.weight"].copy()
        r[4], r[2] = 1.0, -0.01
        w["layers.1.downsample.reduction.weight"] = r
        b = w["layers.2.blocks.0.mlp.fc2.bias"].copy()
        b[4] = -5e4
        w["layers.2.blocks.0.mlp.fc2.bias"] = b
        return w, None
    i = 0 if writer == "fused_merge" else 1        # merge 0 (C = 96, fused) / merge 1 of Swin-B (C = 256, LayerNorm + GEMM)
    b, r = _merge_bias(w[f"layers.{i}.downsample.reduction.weight"])
    w[f"layers.{i}.downsample.norm.bias"], w[f"layers.{i}.downsample.reduction.weight"] = b, r
    return w, None


@pytest.mark.parametrize("writer,cfgn,geom,bit", WRITERS, ids=[w[0] for w in WRITERS])
def test_each_stream_writer_flags_its_stage(writer, cfgn, geom, bit):
    cfg = getattr(synth, cfgn)
    wts, probe = _craft(writer, cfg, synth.synth_swin_weights(cfg, 0, "stress"))
    hw = synth.synth_vqa_head_weights(cfg.num_features, 64, 0, "stress")
    T, H, W = geom
    x = torch.from_numpy(synth.synth_clip(21, T, H, W, batch=1))
    net, bb = _net(cfgn, wts, hw)
    xd = x.to(DEV)
    # precondition: the fp32 stream really leaves the fp16 range — read through a tap (a tapped forward keeps fp32 rows) where the
    # writer's output is a tap (the embedding: feats[0]; a merge: feats[i + 1]), through the fp32 CPU oracle inside a stage
    seen, feat_or = _oracle_block_max(x, wts, cfg)
    bb.residual16 = False
    with torch.no_grad():
        if writer == "embed":
            assert bb({"technical": xd}, layer=0).abs().max().item() > FP16_MAX
        elif probe is None:
            assert bb({"technical": xd}, layer=bit).abs().max().item() > FP16_MAX
    bb.residual16 = True
    assert seen[probe if probe is not None else 0] > FP16_MAX or probe is None
    s16, f16 = _score(net, bb, xd)
    s32, f32 = _score(net, bb, xd, residual16=False)
    assert f16 == 1 << bit, (writer, f16)
    assert f32 == 0                                # no fp16 stream, no bit
    # the hazard is real: the clamped stream gives another score
    assert (s16 - s32).abs().max().item() > SCORE_TOL, (s16, s32)
    # the fp32-stream score vs the CPU oracle.  A stage-0 / stage-1 stream feeds the fused PatchMerging, whose 16-bit MFMA operand is the
    # row itself (d = x - K, csrc/merge.hip): with fp16 operands an entry past 65504 saturates THERE whatever the stream's type (operand
    # saturation inside a GEMM is not what the range word reports) — those cases are held against the oracle run at the engine's rounding
    # points (fp16 operands, the fused merge's operands), the others against the fp32 oracle itself
    if writer in FEEDS_FUSED_MERGE:
        with torch.no_grad():
            feat_or = O.swin3d_trunk(x, wts, cfg, operand_dtype=torch.float16, kernel_order=True)
    ref = O.vqa_head(feat_or, hw)
    assert (s32 - ref).abs().max().item() <= SCORE_TOL, (s32, ref)


# ---- the harness: Trainer re-scores exactly the videos whose stream overflowed -------------------------------------------------------
N_VID, BRIGHT = 8, (1, 2, 5, 6)


def _bright_dark_weights():
    """Swin-T stress weights whose embedding turns a bright clip's channel 0 into ~ 17.7 G after its LayerNorm (out of range) and a
    dark one's into ~ -1.7 G (in range): the trigger depends on the data"""
    cfg = synth.SWIN_T_GRPB
    w = synth.synth_swin_weights(cfg, 4, "stress")
    G = 5000.0
    pw = w["patch_embed.proj.weight"].copy()
    pw[0] = 1.0
    pb = w["patch_embed.proj.bias"].copy()
    pb[0] = 0.0
    g, b = w["patch_embed.norm.weight"].copy(), w["patch_embed.norm.bias"].copy()
    g[0], b[0] = G, 8.0 * G
    w.update({"patch_embed.proj.weight": pw, "patch_embed.proj.bias": pb, "patch_embed.norm.weight": g, "patch_embed.norm.bias": b})
    return w


def _trainer(tmp_path, hipgraph, streams, guard=True):
    from kvq_amd.trainer import Trainer
    cfg = {"name": "range_guard", "num_workers": 0, "range_guard": guard, "hipgraph": hipgraph, "streams": streams,
           "data": {"val": {"type": "ViewDecompositionDataset_KVQ",
                            "args": {"anno_file": str(tmp_path / "anno.txt"), "data_prefix": str(tmp_path), "phase": "test",
                                     "sample_types": {"technical": dict(fragments_h=2, fragments_w=2, fsize_h=32, fsize_w=32, aligned=8,
                                                                        clip_len=16, frame_interval=1, num_clips=1,
                                                                        size_h=48, size_w=64)}}}},
           "model": {"type": "swin_tiny_grpb", "args": {"swin_tiny_grpb": {"backbone": {}, "head": {"in_channels": 768, "hidden_channels": 64}}}},
           "load_path": None}
    tr = Trainer(types.SimpleNamespace(gpu_id="0"), cfg)
    sd = {f"swin_tiny_grpb_backbone.{k}": torch.from_numpy(v) for k, v in _bright_dark_weights().items()}
    sd.update({f"swin_tiny_grpb_head.{k}": torch.from_numpy(v) for k, v in synth.synth_vqa_head_weights(768, 64, 4, "stress").items()})
    tr.model.load_state_dict(sd, strict=False)
    tr._lane_graphs = None
    return tr


def test_trainer_rescores_exactly_the_overflowing_videos(tmp_path, capfd):
    # constant-colour clips: every fragment draw sees the same pixels, so a re-score samples the same input
    lines = []
    for i in range(N_VID):
        level = 225 + 3 * i if i in BRIGHT else 15 + 3 * i
        np.save(str(tmp_path / f"v{i}.mp4.npy"), np.full((32, 96, 96, 3), level, dtype=np.uint8))
        lines.append(f"v{i}.mp4,0,0,{1.0 + i / 4}")
    (tmp_path / "anno.txt").write_text("\n".join(lines) + "\n")
    tr = _trainer(tmp_path, "on", 4)
    graph = tr._score_all()
    flags = tr.range_flags.copy()
    assert sorted(np.nonzero(flags)[0].tolist()) == list(BRIGHT), flags
    assert all(int(flags[j]) == 1 for j in BRIGHT)                       # stage 0 only
    assert "range guard: 4 video(s) re-scored" in capfd.readouterr().err
    tr.config["hipgraph"], tr.config["streams"] = "off", 3
    eager = tr._score_all()
    assert np.array_equal(tr.range_flags, flags)
    assert np.array_equal(graph, eager)
    # back on graph lanes (the recordings of the first call are replayed), then with fp32 streams: a change of residual16 records anew
    tr.config["hipgraph"], tr.config["streams"], tr.config["range_guard"] = "on", 4, False
    plain = tr._score_all()
    assert tr.range_flags is None
    bb = tr.model.swin_tiny_grpb_backbone
    bb.residual16 = False
    try:
        fp32 = tr._score_all()
    finally:
        bb.residual16 = True
    dark = [j for j in range(N_VID) if j not in BRIGHT]
    assert np.array_equal(graph[list(BRIGHT)], fp32[list(BRIGHT)])
    assert np.array_equal(graph[dark], plain[dark])
    assert np.abs(plain[list(BRIGHT)] - fp32[list(BRIGHT)]).max() > SCORE_TOL      # the guard changed what it had to
