"""GPU: the kernel forms KVQ_LATENCY=1 selects (csrc/common.cpp: latency_mode) — the q-split attention launch, the HC = 256 tails at
C = 384 / 512, stage 3 as a GEMM chain — against the same references and bounds as the default forms.

The library reads the switch once per process, so one child interpreter per session (tests/latency_mode_child.py) runs the cases of
tests/latency_cases.py with the switch set and saves their outputs; every comparison is made here, case by case, against inputs
rebuilt from the same seeds and — where the two modes must agree — against the same launches run in this process in the default mode.
A child that fails, is killed or times out fails every test of this module before any of them touches the GPU."""
import json
import os
import re
import signal
import subprocess
import sys
import time
import types

import numpy as np
import pytest
import torch

import kvq_amd  # noqa: F401
import latency_cases as LC
import test_gpu_e2e as TE
import test_gpu_kernels as TK
from kvq_amd.utils import synth
from oracle import swin3d_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "latency_mode_child.py")
CHILD_SECONDS = 6.4                     # measured: the child's whole run on an MI355X (start-up 2.4 s, the 74 cases 4.0 s)
CHILD_TIMEOUT = 3 * CHILD_SECONDS
CASES = LC.all_cases()
EPS = TK.EPS


def of_kind(kind):
    return [c for c in CASES if c.kind == kind]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    outdir = str(tmp_path_factory.mktemp("latency_mode"))
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, CHILD, outdir], env=dict(os.environ, KVQ_LATENCY="1", PYTHONPATH=ROOT), timeout=CHILD_TIMEOUT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired as e:
        said = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail(f"the latency-mode child did not finish in {CHILD_TIMEOUT:.1f} s and was killed.  The limit is 3 x ONE measured run of "
                    f"{CHILD_SECONDS} s (of which 2.4 s are interpreter, torch and library start-up): on a loaded machine a slow start alone can "
                    f"exceed it — look at where the output ends before suspecting a hang.  Its output ends:\n{said[-3000:]}")
    seconds = time.time() - t0
    print(f"latency-mode child: {seconds:.1f} s\n{r.stdout[-6000:]}")
    manifest = []
    if os.path.exists(os.path.join(outdir, "manifest.txt")):
        with open(os.path.join(outdir, "manifest.txt")) as f:
            manifest = f.read().split()
    if r.returncode != 0:
        how = f"killed by {signal.Signals(-r.returncode).name}" if r.returncode < 0 else f"exit status {r.returncode}"
        pytest.fail(f"the latency-mode child failed ({how}) after {len(manifest)} of {len(CASES)} cases; its output ends:\n{r.stdout[-3000:]}")
    return types.SimpleNamespace(outdir=outdir, manifest=manifest, seconds=seconds)


def outputs(child, case):
    assert case.name in child.manifest, f"{case.name} is missing from the child's manifest"
    return LC.load(os.path.join(child.outdir, case.name + ".npz"))


def same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(-1).view(torch.uint8), b.view(-1).view(torch.uint8))


def test_child_was_in_latency_mode_and_this_process_is_not(child):
    """kvq_block_tail_supported(768, 3072) / (384, 1536) / kvq_block_tail_pack_bytes(768, 3072): 0 / 1 / 0 in the child, 1 / 1 / > 0 here —
    the bit-equality assertions below compare two different launches only if both hold"""
    with open(os.path.join(child.outdir, "mode.json")) as f:
        assert json.load(f) == [0, 1, 0]
    here = LC.mode_probe()
    assert here[:2] == [1, 1] and here[2] > 0, here


def test_manifest_is_the_case_list(child):
    assert child.manifest == [c.name for c in CASES]


TAILMM = re.compile(r"block_tailmm_kernel<kvq::\w+, (\d+), (\d+), (\d+), (\d+)>")      # MODE, CF, HC, token tiles (swin_backbone.py: profile_read)


@pytest.mark.parametrize("case", [c for c in of_kind("trunk") if c.profile], ids=repr)
def test_profile_records_show_the_latency_forms(child, case):
    """One profiled forward of the smallest golden trunk case.  Every stage-2 (C = 384, CF = 3) tail record carries geometry code 22
    (csrc/tailmm.hip: tailmm_geometry_code = (HC / 128) * 10 + token tiles; 12 is the default form), and stage 3 has no fused-tail
    record (CF = 6) but, per block, the proj / fc1 / fc2 GEMM records and the LayerNorm record of the chain."""
    assert case.name in child.manifest
    with open(os.path.join(child.outdir, case.name + ".json")) as f:
        recs = json.load(f)
    tails = [tuple(int(v) for v in TAILMM.fullmatch(r[1]).groups()) for r in recs if r[0] == "tail" and TAILMM.fullmatch(r[1])]
    stage2 = [t for t in tails if t[1] == 3]
    assert len(stage2) == synth.SWIN_T_GRPB.depths[2], recs
    assert all((hc // 128) * 10 + tt == 22 for _, _, hc, tt in stage2), stage2
    assert not [t for t in tails if t[1] == 6], tails
    last_merge = max(i for i, r in enumerate(recs) if r[0] in ("merge", "gemm_merge"))
    stage3 = [r[0] for r in recs[last_merge + 1:]]
    assert "tail" not in stage3, stage3
    depth = synth.SWIN_T_GRPB.depths[3]
    assert [stage3.count(k) for k in ("gemm_proj", "gemm_fc1", "gemm_fc2")] == [depth] * 3, stage3
    assert stage3.count("layernorm") >= depth, stage3                  # norm2 of every block (+ norm1 rows, the final norm)


@pytest.mark.parametrize("case", of_kind("attn"), ids=repr)
def test_attention_under_qsplit(child, case):
    """(1) the child's output against O.attention_core on the same rounded operands, at the bounds of
    test_window_attention32_vs_oracle_and_gather_path (the extremes inputs: of test_window_attention32_extremes_and_rescale);
    (2) bit for bit the default mode's output on the same inputs — a q-block's arithmetic does not depend on which workgroup runs it
    (csrc/attn32.hip: "results do not depend on it"), so this is derived, not measured; (3) tile_skip: skipped rows keep the sentinel,
    all others equal the un-skipped launch."""
    inp = case.inputs()
    lat = outputs(child, case)
    half, out = case.half, lat["out"].float()
    qs, starts = case.qsplit()
    keep = inp.get("keep", torch.ones(out.shape[0], dtype=torch.bool))               # pad_mask: every row that is not a padding row
    assert torch.isfinite(out[keep]).all()
    ref_img, ref = case.oracle(inp)
    e_img, e_ref = (out - ref_img)[keep].abs().max().item(), (ref_img - ref)[keep].abs().max().item()
    e_max, e_mean = (out - ref)[keep].abs().max().item(), (out - ref)[keep].abs().mean().item()
    print(f"{case.name}: qsplit {qs}, parts start at q-blocks {starts}: |out - oracle(image)| {e_img:.3e}, image rounding {e_ref:.3e}, "
          f"|out - oracle| max {e_max:.3e} mean {e_mean:.3e}")
    if case.how == "extremes":
        assert e_max <= TK.ATTN32_MAX * EPS[half] + TK.IMAGE_ROUNDING
        assert e_img <= TK.ATTN32_MAX * EPS[half] + TK.IMAGE_ROUNDING
    else:
        assert e_img <= TK.ATTN32_MAX * EPS[half]
        assert e_ref <= TK.IMAGE_ROUNDING
        assert e_mean <= TK.ATTN32_MEAN * EPS[half]
    here = case.run(inp)
    for k in lat:
        assert same_bits(lat[k], here[k]), (f"{case.name}: '{k}' differs from the default mode in "
                                            f"{int((lat[k].float() != here[k].float().cpu()).any(1).sum())} rows")
    if case.how == "tile_skip":
        skipped = case.skipped_rows(inp)
        assert bool(skipped.any()) and not bool(skipped.all())
        part = lat["part"].float()
        assert bool((part[skipped] == LC.SENTINEL).all()) and torch.equal(part[~skipped], out[~skipped])


def rms(a, b):
    return float((a.double() - b).pow(2).mean().sqrt())


RMS_MARGIN = 1.5


@pytest.mark.parametrize("case", of_kind("tail"), ids=repr)
def test_tail_hc256(child, case):
    """block_tailmm_kernel<E, MODE, 3 | 4, 256> against test_gpu_kernels._tail_reference at test_block_tail's bound, its emitted rows at
    the bounds of test_block_tail / test_block_tail_emits_next_qkv, the token-walking launch bit-equal to the scatter launch; and the rms
    error against the float64 evaluation of the same composition (latency_cases.tail_reference64) at most RMS_MARGIN x the default
    (HC = 128) form's on the same inputs: the two forms round to 16 bits at the same points and differ in the fp32 summation order over
    hidden at most.  Ratios observed on an MI355X: 1.000000 in all 18 cases (fp16 rms 2.1e-4 .. 3.2e-4, bf16 4.8e-4 .. 1.1e-3 in both forms),
    and no element of x differs between the forms.  That is derivable too: both forms feed an output element's accumulator the same
    32 x 32 x 16 MFMAs in the same order — over C in fc1, over hidden in fc2, a chunk boundary is not a boundary of the sum — and share the
    proj / norm2 / GELU code, so the HC = 256 output is asserted bit-equal to the HC = 128 one.  A form whose accumulation order is changed
    on purpose drops that assertion and keeps the rms margin."""
    inp = case.inputs()
    lat = outputs(child, case)
    half, C, (D, H, W), B = case.half, case.C, case.dims, case.B
    wts = case.weights(inp)
    got = lat["x"]
    ref = TK._tail_reference(inp["A"], inp["x"], wts, half, case.lay, B, case.dims)
    scale, err = ref.abs().max().item(), (got - ref).abs().max().item()
    assert torch.isfinite(got).all()
    assert err <= TK.tail_bound(half, scale), (err, scale)
    if case.gather:
        assert torch.equal(lat["xg"], got)
    if case.emit:
        ln = torch.nn.functional.layer_norm(got, (C,), inp["gn"], inp["bn"]).reshape(B, D, H, W, C)
        rows = O.gather_windows(ln, case.lay2).reshape(-1, C)
    if case.emit == "norm":
        d = (lat["emitted"].float() - rows).abs().max().item()
        assert d <= TK.emitted_bound(half, rows.abs().max().item()), d
    if case.emit == "qkv":
        qkv, nH = lat["emitted"], C // 32
        assert torch.equal(lat["x_ln"], got) and qkv.shape == (3, nH, B * case.L, 32)
        gemm = lat["gemm"].reshape(3, nH, B * case.L, 32).float()
        d = (qkv.float() - gemm).abs().max().item()
        assert d <= TK.emitted_bound(half, gemm.abs().max().item()), d
        full = TK.rnd(rows, half) @ inp["Wq"].t() + inp["bq"]
        full[:, :C] *= case.QS
        want = full.reshape(B * case.L, 3, nH, 32).permute(1, 2, 0, 3)
        assert (qkv.float() - want).abs().max().item() <= TK.tail_bound(half, want.abs().max().item())
    ref64 = LC.tail_reference64(inp["A"], inp["x"], wts, half, case.lay, B, case.dims)
    here = case.run(inp)["x"].cpu()
    r_lat, r_here = rms(got, ref64), rms(here, ref64)
    print(f"{case.name}: max error {err:.3e} of {scale:.2f}; rms vs float64 HC=256 {r_lat:.6e}, HC=128 {r_here:.6e}, ratio {r_lat / r_here:.6f}; "
          f"{int((got != here).sum())} of {got.numel()} elements differ between the forms")
    assert r_here > 0 and r_lat <= RMS_MARGIN * r_here, (r_lat, r_here)
    assert torch.equal(got, here)


@pytest.mark.parametrize("case", of_kind("tail16"), ids=repr)
def test_tail_hc256_fp16_residual_stream(child, case):
    """test_block_tail_fp16_residual_stream's C = 384 cases in the HC = 256 form.  (1) As that test asserts: the fp16-stream launch is the
    fp32-stream launch on the widened input rounded once to fp16, bit for bit, and what the two emit is identical.  Both of those come
    from the same form, so (2) the fp32-stream output is held against test_gpu_kernels._tail_reference on the widened input at
    test_block_tail's bound — over all rows (the bound scales with row 0's 60000) and over the rows behind row 0 at their own, ordinary
    scale — (3) its rms error against the float64 composition is at most RMS_MARGIN x the default (HC = 128) form's, and (4) both
    streams are bit-equal to the default form's, as in test_tail_hc256.  Ratios observed on an MI355X: 1.000000 in the four cases."""
    inp = case.inputs()
    lat = outputs(child, case)
    xh, x32 = lat["xh"], lat["x32"]
    half, wts, xw = case.half, case.weights(inp), inp["x16"].float()
    ref = TK._tail_reference(inp["A"], xw, wts, half, case.lay, case.B, case.dims)
    err, rest = (x32 - ref).abs().max().item(), (x32 - ref)[1:].abs().max().item()
    assert torch.isfinite(x32).all()
    assert err <= TK.tail_bound(half, ref.abs().max().item()), (err, ref.abs().max().item())
    assert rest <= TK.tail_bound(half, ref[1:].abs().max().item()), (rest, ref[1:].abs().max().item())
    ref64 = LC.tail_reference64(inp["A"], xw, wts, half, case.lay, case.B, case.dims)
    here = {k: v.cpu() for k, v in case.run(inp).items()}
    r_lat, r_here = rms(x32, ref64), rms(here["x32"], ref64)
    print(f"{case.name}: max error {err:.3e} of {ref.abs().max().item():.1f}, behind row 0 {rest:.3e} of {ref[1:].abs().max().item():.2f}; "
          f"rms vs float64 HC=256 {r_lat:.6e}, HC=128 {r_here:.6e}, ratio {r_lat / r_here:.6f}")
    assert r_here > 0 and r_lat <= RMS_MARGIN * r_here, (r_lat, r_here)
    assert torch.equal(x32, here["x32"]) and torch.equal(xh, here["xh"])
    assert xh.dtype == torch.float16 and torch.equal(xh, x32.clamp(-65504.0, 65504.0).to(torch.float16))
    assert torch.isfinite(xh.float()).all()
    assert ("n32" in lat) == (case.nxt is not None)
    if "n32" in lat:
        assert torch.equal(lat["n16"], lat["n32"])


@pytest.mark.parametrize("case", of_kind("trunk"), ids=repr)
def test_trunk_vs_reference_golden(child, golden, case):
    """stage 2 through the HC = 256 tails, stage 3 as a GEMM chain, every attention launch q-split: the features and the score against
    tests/golden/trunk.npz at the tolerances of test_trunk_and_score_vs_reference_golden"""
    lat = outputs(child, case)
    g, name, dtype = golden("trunk.npz"), case.golden_case, case.dtype
    B = int(g[f"{name}/meta"][2])
    scheme = str(g[f"{name}/scheme"])
    feat = lat["feat"].numpy()
    assert tuple(g[f"{name}/feat/shape"]) == feat.shape
    ref_vals = g[f"{name}/feat/val"]
    rel = np.linalg.norm(np.ascontiguousarray(feat).reshape(-1)[g[f"{name}/feat/idx"]] - ref_vals) / np.linalg.norm(ref_vals)
    assert lat["score"].shape == (B, 1)
    d = np.abs(lat["score"].numpy() - g[f"{name}/score"]).max()
    print(f"{case.name}: feature rel-L2 {rel:.3e}, |score - golden| {d:.3e}")
    assert rel <= TE.FEAT_REL_L2[dtype], rel
    assert d <= (TE.SCORE_TOL if (dtype == "fp16" or scheme == "init") else TE.BF16_STRESS_TOL), d


@pytest.mark.parametrize("case", of_kind("bounds"), ids=repr)
def test_guarded_run_is_clean(child, case):
    """tests/test_gpu_bounds.py's ``check`` in the child: guards intact, guarded run byte-equal to the plain one, nothing skipped, and the
    ``Keep`` masks (skipped rows, the image's spare block) still hold the payload"""
    assert case.name in child.manifest
    with open(os.path.join(child.outdir, case.name + ".txt")) as f:
        assert f.read() == "clean"
