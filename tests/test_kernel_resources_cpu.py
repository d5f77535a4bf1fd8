"""Register budget of the token-per-lane launches (csrc/tail.hip, csrc/merge.hip), read from the compiler's own resource remarks
(-Rpass-analysis=kernel-resource-usage through tools/kres_units.py: the library's flags, device code only, no GPU).  The C = 192 tails
and merges and the emitting C = 96 tails used to spill to scratch — 100 MB of HBM traffic per step of the flagship workload that no
operand list accounted for; they must stay at zero scratch, and the fix must not have been paid for by the other instantiations."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
pytestmark = [pytest.mark.slow, pytest.mark.skipif(HIPCC is None, reason="needs hipcc")]

# (VGPRs + AGPRs with fp16 operands, with bf16 operands, waves per SIMD) of every instantiation at the commit before the spills were
# removed; profiles/stage1_noscratch_kres.txt has the full tables
BEFORE = {
    "block_tail_kernel<E, 3, 4, 0>": (165, 165, 3), "block_tail_kernel<E, 3, 4, 1>": (168, 168, 3), "block_tail_kernel<E, 3, 4, 2>": (168, 168, 3),
    "block_tail_kernel<E, 4, 4, 0>": (212, 212, 2), "block_tail_kernel<E, 4, 4, 1>": (218, 218, 2), "block_tail_kernel<E, 4, 4, 2>": (218, 218, 2),
    "block_tail_kernel<E, 6, 4, 0>": (256, 256, 2), "block_tail_kernel<E, 6, 4, 1>": (256, 256, 2), "block_tail_kernel<E, 6, 4, 2>": (256, 256, 2),
    "patch_merge_kernel<E, false, 96, false>": (201, 210, 2), "patch_merge_kernel<E, false, 96, true>": (172, 171, 2),
    "patch_merge_kernel<E, true, 96, false>": (212, 212, 2), "patch_merge_kernel<E, true, 96, true>": (212, 212, 2),
    "patch_merge_kernel<E, false, 128, false>": (346, 346, 1), "patch_merge_kernel<E, false, 128, true>": (320, 320, 1),
    "patch_merge_kernel<E, true, 128, false>": (398, 398, 1), "patch_merge_kernel<E, true, 128, true>": (398, 398, 1),
    "patch_merge_kernel<E, false, 192, false>": (512, 512, 1), "patch_merge_kernel<E, false, 192, true>": (512, 512, 1),
    "patch_merge_kernel<E, true, 192, false>": (512, 512, 1), "patch_merge_kernel<E, true, 192, true>": (512, 512, 1),
}


@pytest.fixture(scope="module")
def table():
    import kres_units
    rows = kres_units.unit_rows(["tail.hip", "merge.hip"])
    out = {}
    for unit in rows.values():
        for name, vgpr, agpr, scratch, occ in unit:
            if name.startswith(("block_tail_kernel<", "patch_merge_kernel<")):
                out[name] = (vgpr, agpr, scratch, occ)
    return out


def _forms(table, pattern):
    got = {n: r for n, r in table.items() if n.replace("kvq::Fp16", "E").replace("kvq::Bf16", "E") == pattern}
    assert len(got) == 2, (pattern, sorted(table))       # fp16 and bf16 operands
    return got


def test_every_instantiation_is_listed(table):
    assert {n.replace("kvq::Fp16", "E").replace("kvq::Bf16", "E") for n in table} == set(BEFORE)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_c192_tail_fits_the_register_file(table, mode):
    for name, (vgpr, agpr, scratch, occ) in _forms(table, f"block_tail_kernel<E, 6, 4, {mode}>").items():
        print(name, vgpr, agpr, scratch, occ)
        assert scratch == 0 and vgpr + agpr <= 256 and occ == 2, (name, vgpr, agpr, scratch, occ)


@pytest.mark.parametrize("emit", ["false", "true"])
@pytest.mark.parametrize("x16", ["false", "true"])
def test_c192_merge_fits_the_register_file(table, emit, x16):
    for name, (vgpr, agpr, scratch, occ) in _forms(table, f"patch_merge_kernel<E, {emit}, 192, {x16}>").items():
        print(name, vgpr, agpr, scratch, occ)
        assert scratch == 0 and vgpr + agpr <= 512 and occ >= 1, (name, vgpr, agpr, scratch, occ)


@pytest.mark.parametrize("mode", [1, 2])
def test_c96_emitting_tail_has_no_scratch(table, mode):
    for name, (vgpr, agpr, scratch, occ) in _forms(table, f"block_tail_kernel<E, 3, 4, {mode}>").items():
        print(name, vgpr, agpr, scratch, occ)
        assert scratch == 0 and vgpr + agpr <= 168 and occ == 3, (name, vgpr, agpr, scratch, occ)


def test_no_instantiation_paid_for_it(table):
    """nothing in the two units spills, loses an occupancy step or gains more than 2 registers against the commit before"""
    bad = []
    for name, (vgpr, agpr, scratch, occ) in sorted(table.items()):
        f0, b0, occ0 = BEFORE[name.replace("kvq::Fp16", "E").replace("kvq::Bf16", "E")]
        regs0 = f0 if "kvq::Fp16" in name else b0
        print(name, vgpr, agpr, scratch, occ, "before", regs0, occ0)
        if scratch != 0 or occ < occ0 or vgpr + agpr > regs0 + 2:
            bad.append((name, vgpr, agpr, scratch, occ, regs0, occ0))
    assert not bad, bad
