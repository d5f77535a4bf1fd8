"""The Swin trunk's host-side sequencing (swin_run, csrc/plan.hip): which launches a forward enqueues, and that a forward refused
for incomplete weights enqueues none of them."""
import importlib.util
import json
import os

import pytest
import torch

import kvq_amd  # noqa: F401
from kvq_amd import _abi
from kvq_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("swin_launch_records", os.path.join(ROOT, "tools", "swin_launch_records.py"))
LR = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(LR)


@pytest.mark.parametrize("name", LR.CONFIGS)
def test_swin_launch_sequence_is_pinned(name):
    """Every profile record (kind, kernel, flops, bytes) of one forward per configuration, in order, as recorded in
    tests/swin_launch_records.json (tools/swin_launch_records.py)."""
    with open(LR.OUT) as f:
        want = json.load(f)[name]
    assert LR.records(name) == want


@pytest.mark.parametrize("hole", ["block_fc1", "merge_reduction"])
def test_incomplete_weights_enqueue_nothing(hole):
    """A forward whose weights miss a later block's fc1 or a merge's reduction is refused before its first launch: KvqError and
    no profile record (the embedding launch is bracketed, so anything enqueued before the check would show)."""
    bb = LR._trunk(synth.SWIN_T_GRPB, "fp16")
    B, T, H, W = 1, 16, 64, 64
    x = torch.from_numpy(synth.synth_clip(5, T, H, W, batch=B)).to(DEV)
    dev = torch.device(DEV)
    with torch.no_grad():
        bb({"technical": x})
        w = bb._weights(dev)
        if hole == "block_fc1":
            bb._wcache[3][5].fc1_w = None               # stage 2, second block
        else:
            w.merges[1].red_w = None                    # stage 1 -> 2
        bb.profile(B, T, H, W, dev, True)
        with pytest.raises(_abi.KvqError, match="weights"):
            bb({"technical": x})
        torch.cuda.synchronize()
        recs = bb.profile_read(B, T, H, W, dev)
        bb.profile(B, T, H, W, dev, False)
    assert recs == []
