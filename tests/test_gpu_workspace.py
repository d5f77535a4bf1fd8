"""GPU: the plan workspaces of the end-to-end forwards — no stale reads, no overruns, no aliased live slots.

``kvq_swin3d_forward*`` carves one caller buffer into x0 | x1 | ln | big | o | sk; ``kvq_convnet_forward`` places activation slots
at their first write, recycles them after their last reader and, in two-lane plans, orders ops of different lanes that touch the
same bytes.  The guard-band tests of the single entry points never see these buffers from the inside, and a value test sees a
wrong number only when a live value is damaged.  Four families, every comparison an equality of bits (no floating-point atomics
in csrc, deterministic forwards):

A. ``test_*_forward_does_not_depend_on_the_workspace``: run a clip, overwrite the cached workspace with 0xFF (NaN in fp16 / bf16 /
   fp32), 0x7B (large and finite: 61 280 / 1.3e36 — ``v_max`` drops a NaN operand, so a row maximum hides a NaN score), 0x00, and
   the residue of a forward on another clip, and require the same features, taps and stage outputs each time; then once more
   with the outputs allocated through ``guarded()``: no written element may still hold the payload.
   These workspaces hold activations and split-K partials only — in ``swin_run`` (csrc/plan.hip) every pointer derived from the
   workspace (cur / oth, bln, bbig, bo) is a stream, LayerNorm rows, q | k | v / hidden rows or attention output, and every index
   map (d_src, d_dst, d_pad, d_tok, d_merge, ...) is a separate device allocation of the plan; in ``kvq_convnet_forward``
   (csrc/convnet.hip) ``ptr_of`` hands out activation slots and ``sk_ws`` the split-K partials, the tap tables are allocations
   of the plan.  So a stale read yields a wrong VALUE, never an address.  Buffers whose contents become offsets or addresses (the
   JPEG scan workspace's pos / cnt, index maps, token tables) are left out on purpose, as §9 leaves the integer tables.
B. ``test_whole_model_forward_under_guard_bands``: each backbone's forward plainly, inside ``guarded(payload=0xFF)`` and inside
   ``guarded(payload=0x00)``, a fresh module each time, so that the workspace, weight images, bias images and per-call tensors are
   all guarded allocations: every guard intact, the three outputs equal.  (Guards are capped at 1 MiB here: the default "32 rows"
   of a flat byte buffer would be 32 times the workspace.)  No integer table is allocated through ``torch.empty`` by these
   forwards: their flat uint8 buffers are the workspace, the weight images and the bias images.
C. ``test_swin_workspace_regions_cover_the_restated_need``: ``kvq_swin3d_workspace_regions`` against tests/workspace_ref.py.
D. ``test_convnet_layout_passes_the_independent_checker``: ``kvq_convnet_layout`` against tests/plan_layout_check.py.
"""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import kvq_amd  # noqa: F401
import plan_layout_check as PLC
import workspace_ref as WR
from guarded import guarded
from kvq_amd import _abi
from kvq_amd.utils import synth
from oracle import slowfast_oracle as SF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("swin_launch_records", os.path.join(ROOT, "tools", "swin_launch_records.py"))
LR = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(LR)

FILLS = (0xFF, 0x7B, 0x00, "residue")
MAX_GUARD = 1 << 20
HOT_TABLE = "layers.1.blocks.0.attn.relative_position_bias_table"


def _flat(out):
    if torch.is_tensor(out):
        return [out]
    if isinstance(out, dict):
        return [t for k in sorted(out) for t in _flat(out[k])]
    return [t for o in out for t in _flat(o)]


def _same(want, got, what):
    assert len(want) == len(got)
    for k, (a, b) in enumerate(zip(want, got)):
        assert a.shape == b.shape
        if not torch.equal(a, b):
            bad = (a != b) | (a.isnan() != b.isnan())
            raise AssertionError(f"{what}: output {k} of shape {tuple(a.shape)} differs in {int(bad.sum())} of {a.numel()} elements, "
                                 f"{int(b.isnan().sum())} of them NaN")


def check_workspace_independence(run, run_other, workspaces):
    """A of the module docstring.  ``run()`` -> tensors (any nesting) of the clip under test, ``run_other()`` the same forward on
    another clip of the same geometry, ``workspaces()`` -> the cached workspace tensors (called after the first forward)."""
    with torch.no_grad():
        want = [t.clone() for t in _flat(run())]
        assert want and all(bool(torch.isfinite(t).all()) for t in want)
        wss = workspaces()
        assert wss and all(w.dtype == torch.uint8 and w.numel() > 0 for w in wss)
        for fill in FILLS:
            if fill == "residue":
                other = _flat(run_other())
                assert not torch.equal(other[0], want[0])
            else:
                for w in wss:
                    w.fill_(fill)
            _same(want, _flat(run()), f"workspace filled with {fill if fill == 'residue' else hex(fill)}")
        assert [w.data_ptr() for w in workspaces()] == [w.data_ptr() for w in wss]       # the forwards above ran on THESE buffers
        with guarded(max_guard=MAX_GUARD) as G:
            got = _flat(run())
            assert G.intact(), G.intact()
        # the plan is cached: what a forward allocates now are its outputs and taps (forward_stages also drops an ``io`` that is
        # smaller than its input stream unused); every returned tensor lies in one of them and holds no payload any more
        for k, t in enumerate(got):
            home = [a for a in G.allocs if a.view.data_ptr() <= t.data_ptr() < a.view.data_ptr() + a.nbytes]
            assert len(home) == 1, f"output {k} is not a guarded allocation"
            left = int(G.payload_left(t).sum())
            assert left == 0, f"output {k} in {home[0].name}: {left} elements the forward never wrote"
        _same(want, got, "outputs pre-filled with the payload")


# ------------------------------------------------------------------------------------------------------------- A: the Swin trunk
@functools.lru_cache(maxsize=None)
def _trunk(dtype, wseed=0, hot_table=None):
    return LR._trunk(synth.SWIN_T_GRPB, dtype, wseed, hot_table)


def _clips(B, T, H, W):
    return tuple(torch.from_numpy(synth.synth_clip(seed, T, H, W, batch=B)).to(DEV) for seed in (5, 6))


def _swin_check(bb, geometry, B, forward=None, residual16=True, fused=True):
    bb.residual16, bb.fused_tail, bb.dense_bias = residual16, fused, fused
    x, y = _clips(B, *geometry)
    forward = forward or (lambda clip: bb({"technical": clip}))
    check_workspace_independence(lambda: forward(x), lambda: forward(y), lambda: [e[2] for e in bb._plans.values()])


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("geometry", [(32, 56, 56), (10, 50, 70), (16, 84, 84)], ids=lambda g: "x".join(map(str, g)))
def test_swin_fused_forward_does_not_depend_on_the_workspace(geometry, dtype):
    """Swin-T GRPB, fused launches, B = 2.  32x56x56: un-padded, two depth slabs (region-ordered shifted partitions), attention
    projecting its own q | k | v at C = 96, tails emitting q | k | v.  10x50x70: padded partitions, ``pad_mask``, ``tile_skip``, the
    odd 13 x 18 grid into the merge.  16x84x84: the un-padded 21 x 21 grid, merge parts of -1."""
    _swin_check(_trunk(dtype), geometry, 2)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_swin_padded_forward_on_the_bias_image_does_not_depend_on_the_workspace(dtype):
    """10x50x70 with EVERY block on the bias image.  Half of the "stress" bias tables pass +-16, so in the test above their blocks
    (padded stages 0-1 among them) keep the gather path; here the limit is lifted — the exactness of the fp16 image is not the
    point, the launches are: attention writing the padding rows' k | v itself (``pad_mask``), passing over the q-tiles that are
    padding only (``tile_skip``: 3 such tiles in stage 0, 1 in stage 1), tails emitting q | k | v through a padded partition."""
    bb = _trunk(dtype, 1)
    bb.dense_bias_max_abs = float("inf")
    _swin_check(bb, (10, 50, 70), 2)
    assert bb._dense and all(b is not None for bufs in bb._dense.values() for b in bufs)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("geometry", [(32, 56, 56), (10, 50, 70)], ids=lambda g: "x".join(map(str, g)))
def test_swin_fp32_stream_forward_does_not_depend_on_the_workspace(geometry, dtype):
    """``residual16 = False``: fp32 residual streams in every stage"""
    _swin_check(_trunk(dtype), geometry, 2, residual16=False)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("geometry,B", [((10, 50, 70), 2), ((16, 84, 84), 1)], ids=["10x50x70", "16x84x84"])
def test_swin_unfused_forward_does_not_depend_on_the_workspace(geometry, B, dtype):
    """``fused_tail = dense_bias = False``: im2col / GEMM / LayerNorm chain, gather attention, ``kvq_qkv_fill_pad`` on the padded
    partitions of 10x50x70; at 16x84x84 the un-fused merge's LayerNorm writes more rows than the stage has tokens."""
    _swin_check(_trunk(dtype), geometry, B, fused=False)


def test_swin_forward_with_one_gather_block_does_not_depend_on_the_workspace():
    """one block's bias table past +-16: that block alone takes the gather path between fused launches"""
    _swin_check(_trunk("fp16", 11, HOT_TABLE), (8, 64, 64), 2)


def _stage_split(bb, geometry):
    def run(clip):
        s1 = bb.forward_stages(clip, 0, 1)
        s2 = bb.forward_stages(s1, 2, 2, geometry=geometry)
        s3, feat = bb.forward_stages(s2, 3, 3, geometry=geometry, want_feat=True)
        return s1, s2, s3, feat
    return run


@pytest.mark.parametrize("mode", ["multi", "layer", "stages", "adaptive"])
def test_swin_taps_stage_split_and_adaptive_window_do_not_depend_on_the_workspace(mode):
    """``multi=True`` / ``layer=k`` (feature taps: fp32 streams, D2D copies out of the workspace), the stage-split entry as KSVQE
    calls it (stages 0-1, 2, 3: every stage output compared) and ``adaptive_window_size=True``, at the adaptive goldens' smallest
    geometry"""
    bb, geometry = _trunk("fp16"), (16, 160, 160)
    forward = {"multi": lambda clip: bb({"technical": clip}, multi=True),
               "layer": lambda clip: [bb({"technical": clip}, layer=k) for k in (0, 2, 4)],
               "stages": _stage_split(bb, geometry),
               "adaptive": lambda clip: bb({"technical": clip}, adaptive_window_size=True)}[mode]
    _swin_check(bb, geometry, 2, forward)


@functools.lru_cache(maxsize=None)
def _trunk_b():
    return LR._trunk(synth.SWIN_B_GRPB, "fp16")


def test_swin_b_forward_does_not_depend_on_the_workspace():
    """Swin-B (C = 128 ... 1024) at the clip of test_config5_swin_b_padded_windows_vs_oracle: window padding at every stage, the
    token-walking wide tails, un-fused merges writing fp16"""
    _swin_check(_trunk_b(), (16, 128, 128), 1)


# -------------------------------------------------------------------------------------------------------- A: the conv-net plans
def _make_resnet():
    from kvq_amd.models.backbones.simpleVQA_model import resnet50
    m = resnet50()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_resnet50_weights(4, "stress").items()})
    return m.to(DEV).eval()


_resnet = functools.lru_cache(maxsize=None)(_make_resnet)


def _resnet_inputs():
    rng = np.random.Generator(np.random.PCG64(55))
    draw = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV)      # noqa: E731
    return [{"simpleVQA": draw(2, 3, 3, 64, 80), "feat": draw(2, 3, 2304)} for _ in range(2)]


def _make_slowfast(two_lanes, split_k):
    import kvq_amd.models.backbones.slowfast_model as M
    m = M.slowfast(two_lanes=two_lanes)
    m.head_small_grid = "mean"              # reduced-size clip: final grid under the head's (8,7,7) kernel
    m.split_k = split_k
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_params(SF.param_shapes(), 3, "stress", prefix="sf.").items()})
    return m.to(DEV).eval()


_slowfast = functools.lru_cache(maxsize=None)(_make_slowfast)


def _slowfast_clips():
    return [torch.from_numpy(synth.synth_clip(70 + i, 16, 96, 64, batch=2)).to(DEV) for i in range(2)]


@pytest.mark.parametrize("split_k", [True, False], ids=["splitk", "no_splitk"])
def test_simplevqa_forward_does_not_depend_on_the_workspace(split_k):
    """SimpleVQA's ResNet-50 plan (2 x 3 frames of 64 x 80, the smallest clip of tests/test_resnet.py), split-K on and off"""
    m = _resnet()
    a, b = _resnet_inputs()
    with torch.no_grad():
        m(a)
    for handle, *_ in m._nets.values():
        _abi.check(_abi.lib().kvq_convnet_splitk(handle, int(split_k)), "kvq_convnet_splitk")
    try:
        check_workspace_independence(lambda: m(a), lambda: m(b), lambda: [e[1] for e in m._nets.values()])
    finally:
        for handle, *_ in m._nets.values():
            _abi.check(_abi.lib().kvq_convnet_splitk(handle, 1), "kvq_convnet_splitk")


@pytest.mark.parametrize("split_k", [True, False], ids=["splitk", "no_splitk"])
@pytest.mark.parametrize("two_lanes", [False, True], ids=["one_lane", "two_lanes"])
def test_slowfast_forward_does_not_depend_on_the_workspace(two_lanes, split_k):
    """the SlowFast plan (2 clips of 16 x 96 x 64, the smallest of tests/test_slowfast.py), one-lane and two-lane, split-K on and off"""
    m = _slowfast(two_lanes, split_k)
    a, b = _slowfast_clips()
    check_workspace_independence(lambda: m.forward_clips(a), lambda: m.forward_clips(b), lambda: [e[1] for e in m._nets.values()])


# ------------------------------------------------------------------------------------------- B: whole models under guard bands
def _swin_t_fresh(fused):
    bb = LR._trunk(synth.SWIN_T_GRPB, "fp16")
    bb.fused_tail = bb.dense_bias = fused
    return bb


def _conv_net(key, weights):
    from kvq_amd.models.model import VQA_Network
    net = VQA_Network({"model": {"args": {key: {"backbone": {"pretrained": False} if key == "conv_tiny" else {},
                                                "head": {"in_channels": 768, "hidden_channels": 64}}}}})
    bb = getattr(net, key + "_backbone")
    bb.load_state_dict({k: torch.from_numpy(v) for k, v in weights(3, "stress").items()})
    return bb.to(DEV).eval()


def _clip_tool():
    from kvq_amd.models.backbones.clip_visual import CLIP_extractor_addadapter_cls
    m = CLIP_extractor_addadapter_cls(CLIP_location=8, cls_use=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_clip_visual_weights(7).items()}, strict=True)
    return m.to(DEV).eval()


def _guard_cases():
    swin = lambda g, B: (lambda: _clips(B, *g)[0], lambda m, x: m({"technical": x}))                     # noqa: E731
    conv_x = lambda: _clips(2, 8, 64, 96)[0]                                                                   # noqa: E731
    return {
        "swin_t_fused_32x56x56": (lambda: _swin_t_fresh(True),) + swin((32, 56, 56), 2),
        "swin_t_fused_10x50x70": (lambda: _swin_t_fresh(True),) + swin((10, 50, 70), 2),
        "swin_t_fused_16x84x84": (lambda: _swin_t_fresh(True),) + swin((16, 84, 84), 2),
        "swin_t_unfused_10x50x70": (lambda: _swin_t_fresh(False),) + swin((10, 50, 70), 2),
        "swin_t_unfused_16x84x84": (lambda: _swin_t_fresh(False),) + swin((16, 84, 84), 1),
        "conv_tiny": (lambda: _conv_net("conv_tiny", synth.synth_convnext_weights), conv_x, lambda m, x: m({"aesthetic": x})),
        "conv_v2_tiny": (lambda: _conv_net("conv_v2_tiny", synth.synth_convnextv2_weights), conv_x, lambda m, x: m({"aesthetic": x})),
        "clip_visual": (_clip_tool, lambda: torch.from_numpy(np.random.Generator(np.random.PCG64(1)).standard_normal((2, 3, 64, 80))
                                                             .astype(np.float32)).to(DEV), lambda m, x: m(x)),
        "simplevqa": (_make_resnet, lambda: _resnet_inputs()[0], lambda m, x: m(x)),
        "slowfast_one_lane": (lambda: _make_slowfast(False, True), lambda: _slowfast_clips()[0], lambda m, x: m.forward_clips(x)),
        "slowfast_two_lanes": (lambda: _make_slowfast(True, True), lambda: _slowfast_clips()[0], lambda m, x: m.forward_clips(x)),
    }


@pytest.mark.parametrize("name", sorted(_guard_cases()))
def test_whole_model_forward_under_guard_bands(name):
    """B of the module docstring"""
    make, clip, forward = _guard_cases()[name]
    with torch.no_grad():
        x = clip()
        want = [t.clone() for t in _flat(forward(make(), x))]
        assert want and all(bool(torch.isfinite(t.float()).all()) for t in want)
        for payload in (0xFF, 0x00):
            with guarded(payload=payload, max_guard=MAX_GUARD) as G:
                m = make()
                got = _flat(forward(m, x))
                report = G.intact()
            assert report, report
            big = [a for a in G.allocs if a.view.dtype == torch.uint8 and a.nbytes >= 1 << 16]
            assert big or name in ("conv_tiny", "conv_v2_tiny", "clip_visual"), "the workspace was not a guarded allocation"
            _same(want, got, f"guarded, payload {hex(payload)}")
            del m


# ------------------------------------------------------------------------------------------------------ C: the Swin regions
@functools.lru_cache(maxsize=None)
def _cfg_module(which):
    from kvq_amd.models.backbones.swin_backbone import SwinTransformer3D
    cfg = {"t": synth.SWIN_T_GRPB, "b": synth.SWIN_B_GRPB}[which]
    return SwinTransformer3D(embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads), window_size=cfg.window,
                             frag_biases=list(cfg.frag_biases))


def _regions(which, B, T, H, W, aw=None):
    bb, lib = _cfg_module(which), _abi.lib()
    cfg, handle = bb.cfg_struct(aw), C.c_void_p()
    _abi.check(lib.kvq_swin3d_plan_create(C.byref(cfg), B, T, H, W, _abi.DT_FP16, C.byref(handle)), "kvq_swin3d_plan_create")
    try:
        out = (C.c_uint64 * 12)()
        _abi.check(lib.kvq_swin3d_workspace_regions(handle, C.byref(out)), "kvq_swin3d_workspace_regions")
        return {name: (int(out[2 * r]), int(out[2 * r + 1])) for r, name in enumerate(WR.REGIONS)}, int(lib.kvq_swin3d_workspace_bytes(handle))
    finally:
        lib.kvq_swin3d_plan_destroy(handle)


REGION_CASES = [("t", 2, (32, 56, 56), None), ("t", 2, (10, 50, 70), None), ("t", 2, (16, 84, 84), None), ("t", 1, (16, 84, 84), None),
                ("t", 2, (8, 64, 64), None), ("t", 2, (16, 160, 160), None), ("t", 2, (16, 160, 160), (4, 5, 5)), ("b", 1, (16, 128, 128), None),
                ("t", 1, (16, 28, 28), None), ("t", 1, (16, 140, 140), None), ("t", 1, (16, 196, 84), None), ("t", 2, (16, 196, 84), None),
                ("t", 1, (32, 224, 224), None), ("t", 1, (16, 64, 64), None)]


@pytest.mark.parametrize("which,B,geometry,aw", REGION_CASES, ids=[f"{w}_b{B}_{'x'.join(map(str, g))}{'_adaptive' if a else ''}" for w, B, g, a in REGION_CASES])
def test_swin_workspace_regions_cover_the_restated_need(which, B, geometry, aw):
    """Host arithmetic on a created plan (nothing is launched): the regions are ordered, disjoint, 256-byte aligned and inside
    ``kvq_swin3d_workspace_bytes``, and each holds at least what tests/workspace_ref.py restates from the geometry — the un-fused
    merge's B Ln 4C LayerNorm rows in ``ln`` included, which an ``ln`` sized for max(B Lp C, B L C) misses at 16x84x84 (66 048 B at
    B = 1), 16x28x28, 16x140x140 and 16x196x84.  On grids that stay even down the stages 4 Ln == L and every region is exactly its
    restated need: covering the merge rows moved nothing there."""
    cfg = {"t": synth.SWIN_T_GRPB, "b": synth.SWIN_B_GRPB}[which]
    regions, total = _regions(which, B, *geometry, aw)
    needs = WR.region_needs(B, *geometry, embed_dim=cfg.embed_dim, num_stages=len(cfg.depths), window=tuple(cfg.window), adaptive=aw)
    assert WR.check_regions(regions, total, needs) == []
    assert total == regions["sk"][0] + -(-regions["sk"][1] // 256) * 256
    grids = WR.stage_grids(*geometry, (2, 4, 4), len(cfg.depths))
    if all(h % 2 == 0 and w % 2 == 0 for _, h, w in grids[:-1]):
        assert {n: regions[n][1] for n in WR.REGIONS[:5]} == {n: max(needs[n]) for n in WR.REGIONS[:5]}


# ---------------------------------------------------------------------------------------------------- D: the conv-net layouts
def read_layout(handle):
    """``kvq_convnet_layout`` as the dict tests/plan_layout_check.py takes, plus ``uses_scratch`` per op"""
    lib, info = _abi.lib(), _abi.KvqNetLayoutInfo()
    _abi.check(lib.kvq_convnet_layout(handle, C.byref(info), None, 0, None, 0), "kvq_convnet_layout")
    slots, ops = (_abi.KvqNetSlotLayout * info.n_slots)(), (_abi.KvqNetOpLayout * info.n_ops)()
    _abi.check(lib.kvq_convnet_layout(handle, C.byref(info), slots, info.n_slots, ops, info.n_ops), "kvq_convnet_layout")
    assert info.ws_bytes == lib.kvq_convnet_workspace_bytes(handle)
    return {"ws_bytes": int(info.ws_bytes), "n_lanes": int(info.n_lanes),
            "scratch": [(int(info.sk_off + lane * info.sk_stride), int(info.sk_bytes)) for lane in range(info.n_lanes)],
            "slots": [(int(s.off), int(s.bytes), bool(s.in_workspace)) for s in slots],
            "ops": [{"lane": int(o.lane), "reads": list(o.reads[:o.n_reads]), "writes": list(o.writes[:o.n_writes]), "wait": int(o.wait_op),
                     "uses_scratch": bool(o.uses_scratch)} for o in ops]}


def _recycled_pairs(lay):
    s = [x for x in lay["slots"] if x[2] and x[1]]
    return sum(1 for i, a in enumerate(s) for b in s[i + 1:] if a[0] < b[0] + b[1] and b[0] < a[0] + a[1])


@pytest.mark.parametrize("plan", ["simplevqa", "slowfast_one_lane", "slowfast_two_lanes"])
def test_convnet_layout_passes_the_independent_checker(plan):
    """Slots inside the workspace and clear of the split-K scratch, no two live slots on the same bytes, and — two lanes — every
    cross-lane conflict ordered by program order plus the wait edges (tests/plan_layout_check.py; tests/test_plan_layout_cpu.py
    shows the checker naming each of these defects).  The plans are those of A; the layout must be one the checks can bite on:
    recycled bytes, the internal slot of the packed stem input, wait edges between the lanes."""
    with torch.no_grad():
        if plan == "simplevqa":
            m = _resnet()
            m(_resnet_inputs()[0])
        else:
            m = _slowfast(plan == "slowfast_two_lanes", True)
            m.forward_clips(_slowfast_clips()[0])
    (handle, ws, *_), = m._nets.values()
    lay = read_layout(handle)
    assert lay["ws_bytes"] == ws.numel()
    problems = PLC.check(lay)
    assert problems == [], "\n".join(problems)
    assert _recycled_pairs(lay) > 0 and lay["scratch"][0][1] > 0
    assert any(op["uses_scratch"] for op in lay["ops"]) and all(op["writes"] for op in lay["ops"] if op["uses_scratch"])
    if plan == "simplevqa":
        assert lay["n_lanes"] == 1 and any(set(op["reads"]) & set(op["writes"]) for op in lay["ops"])        # STEM8's packed input
    elif plan == "slowfast_one_lane":
        assert lay["n_lanes"] == 1 and all(op["lane"] == 0 and op["wait"] == -1 for op in lay["ops"])
    else:
        waits = [(i, op["wait"]) for i, op in enumerate(lay["ops"]) if op["wait"] >= 0]
        assert lay["n_lanes"] == 2 and {op["lane"] for op in lay["ops"]} == {0, 1} and waits
        assert all(lay["ops"][i]["lane"] != lay["ops"][w]["lane"] for i, w in waits)
        # the checker sees the lateral connections: without the wait edges it reports races
        bare = dict(lay, ops=[dict(op, wait=-1) for op in lay["ops"]])
        assert any("no ordering between the lanes" in p for p in PLC.check(bare))
