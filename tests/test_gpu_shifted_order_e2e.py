"""GPU, end to end: the Swin-T (GRPB) trunk at clips whose shifted partitions are un-padded — window rows stored sorted by mask region,
attention on key-block ranges — against the CPU oracle, at the bounds tests/test_gpu_e2e.py applies to its oracle comparisons.

  32 x 112 x 112: stage 0 = 2 x 4 x 4 windows (all eight kinds of window, fused projection), stage 1 = 2 x 2 x 2 windows, stage 2 = the
                  depth split only, stage 3 = a clamped window
  16 x 112 x 112: stage 0 without a depth shift (the window clamps D): H / W edges only"""
import numpy as np
import pytest
import torch

import kvq_amd  # noqa: F401
from kvq_amd import _abi
from kvq_amd.models import VQA_Network
from kvq_amd.utils import synth
from oracle import swin3d_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCORE_TOL = {"fp16": 1e-3, "bf16": 8e-3}       # test_gpu_e2e.py: SCORE_TOL; bf16 on the "stress" weights is format-limited (BF16_STRESS_TOL)
FEAT_REL_L2 = {"fp16": 4e-3, "bf16": 2e-2}
WSEED = 23
CLIPS = {"32x112": (61, 32, 112, 112), "16x112": (62, 16, 112, 112)}


def build_network(dtype):
    cfg = synth.SWIN_T_GRPB
    net = VQA_Network({"model": {"args": {"swin_tiny_grpb": {"backbone": {}, "head": {"in_channels": cfg.num_features, "hidden_channels": 64}}}}})
    sd = {f"swin_tiny_grpb_backbone.{k}": torch.from_numpy(v) for k, v in synth.synth_swin_weights(cfg, WSEED, "stress").items()}
    sd.update({f"swin_tiny_grpb_head.{k}": torch.from_numpy(v) for k, v in synth.synth_vqa_head_weights(cfg.num_features, 64, WSEED, "stress").items()})
    missing = net.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys
    net.swin_tiny_grpb_backbone.operand_dtype = _abi.dtype_code(dtype)
    return net.to(DEV).eval()


_oracle = {}


def oracle(clip):
    """(clip tensor, oracle feature map, oracle score): computed once per clip, shared by both operand types"""
    if clip not in _oracle:
        cseed, T, H, W = CLIPS[clip]
        cfg = synth.SWIN_T_GRPB
        x = torch.from_numpy(synth.synth_clip(cseed, T, H, W, batch=1))
        with torch.no_grad():
            feat = O.swin3d_trunk(x, synth.synth_swin_weights(cfg, WSEED, "stress"), cfg)
            score = O.vqa_head(feat, synth.synth_vqa_head_weights(cfg.num_features, 64, WSEED, "stress"))
        _oracle[clip] = (x, feat, score)
    return _oracle[clip]


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("clip", list(CLIPS))
def test_trunk_feature_and_score_vs_oracle(clip, dtype):
    x, f_ref, s_ref = oracle(clip)
    net = build_network(dtype)
    with torch.no_grad():
        score = net(inputs={"technical": x.to(DEV)}, reduce_scores=True)
        feat = net.swin_tiny_grpb_backbone({"technical": x.to(DEV)}).cpu()
    assert feat.shape == f_ref.shape
    rel = ((feat - f_ref).norm() / f_ref.norm()).item()
    d = (score.cpu() - s_ref).abs().max().item()
    print(f"{clip} {dtype}: feature rel L2 {rel:.3e}, |score - oracle| {d:.3e}")
    assert rel <= FEAT_REL_L2[dtype], rel
    assert d <= SCORE_TOL[dtype], (score.cpu().ravel(), s_ref.ravel())


def test_stage_split_forward_equals_whole_forward():
    """forward_stages (0-1, 2, 3) at 32 x 112 x 112 against the whole forward, at the bound of test_forward_stages_equals_whole_forward."""
    _, T, H, W = CLIPS["32x112"]
    x = oracle("32x112")[0].to(DEV)
    bb = build_network("fp16").swin_tiny_grpb_backbone
    with torch.no_grad():
        whole = bb({"technical": x})
        s = bb.forward_stages(x, 0, 1)
        s = bb.forward_stages(s, 2, 2, geometry=(T, H, W))
        s, feat = bb.forward_stages(s, 3, 3, geometry=(T, H, W), want_feat=True)
    d = (feat - whole).abs().max().item()
    print(f"stage-split vs whole: {d:.3e} of {whole.abs().max().item():.3e}")
    assert d <= 2e-3 * whole.abs().max().item()
