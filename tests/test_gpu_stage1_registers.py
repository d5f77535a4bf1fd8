"""The token-per-lane launches of stages 0-1 (csrc/tail.hip, csrc/merge.hip) compute what they computed before their register
allocation was reworked to fit the register file without scratch: every output is compared TO THE BIT with
tests/golden/stage1_bits.npz, recorded on an MI355X from the build of the commit before that rework by
tests/golden/make_stage1_bits.py (the same seeded cases, imported from there).  A SHA-256 of the raw output bytes per case; for
the two smallest cases the raw rows too, so a failure says how many values moved and by how much.  The oracle-tolerance tests of
these launches (test_gpu_kernels.py: test_block_tail*, test_patch_merge_*; test_gpu_e2e.py) remain the parity yardstick."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import kvq_amd  # noqa: F401
from kvq_amd import kernels

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_stage1_bits", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_stage1_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

CASES = dict(bits.cases())


@pytest.fixture(scope="module")
def recorded(golden):
    z = golden("stage1_bits.npz")
    keys = [str(k) for k in z["keys"]]
    sha = {k: str(s) for k, s in zip(keys, z["sha256"])}
    raw = {k: z[f"raw_{i}"] for i, k in enumerate(keys) if f"raw_{i}" in z.files}
    return sha, raw


def test_recording_covers_every_case(recorded):
    sha, raw = recorded
    want = set()
    for name in CASES:
        for hname in bits.HALVES:
            outs = ["x"] if name.startswith("tail") else ["out"]
            if "-m1-" in name or "-emit-" in name:
                outs.append("norm1")
            if "-m2-" in name:
                outs.append("qkv")
            want |= {f"{name}/{hname}/{o}" for o in outs}
    assert set(sha) == want
    assert {k.split("/")[0] for k in raw} == set(bits.RAW)


@pytest.mark.parametrize("hname", list(bits.HALVES))
@pytest.mark.parametrize("name", list(CASES))
def test_stage1_bits_unchanged(name, hname, recorded):
    sha, raw = recorded
    outs = CASES[name](bits.HALVES[hname])
    torch.cuda.synchronize()
    for oname, t in outs.items():
        key = f"{name}/{hname}/{oname}"
        got = bits.digest(t)
        if key in raw:
            g = bits.raw_bytes(t)
            assert g.shape == raw[key].shape, key
            if not np.array_equal(g, raw[key]):
                a = torch.from_numpy(g.copy()).view(t.dtype).float()
                b = torch.from_numpy(raw[key].copy()).view(t.dtype).float()
                pytest.fail(f"{key}: {int((a != b).sum())} of {a.numel()} values differ, max |d| {float((a - b).abs().max())}")
        print(key, got[:16], "recorded", sha[key][:16])
        assert got == sha[key], key


def test_c96_tail_cannot_emit_qkv():
    """MODE 2 at C = 96 has no launch: 3C / 32 = 9 qkv panels do not pair into ring items, the pack is refused (so the C = 96 bit cases
    are MODE 1 on both stream types; the MODE 2 instantiation is covered by the compile-time resource test only)."""
    w = torch.zeros(288, 96, dtype=torch.float16, device="cuda:0")
    assert kernels.block_tail_qkv_pack(w, 384) is None
