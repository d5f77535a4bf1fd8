"""GPU: attention32 on region-ordered shifted windows with the key-block ranges of kvq_attn32_key_ranges
(kvq_window_attention32_ranges) against the fp32 oracle on the same rows and against the launch that runs every key block."""
import numpy as np
import pytest
import torch

import kvq_amd  # noqa: F401
import attn_ranges_ref as AR
from kvq_amd import _abi, kernels
from oracle import swin3d_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}     # half-ulp relative rounding error


@pytest.fixture(params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def half(request):
    return request.param


def rnd(t, half):
    return t.to(half).to(torch.float32)


def dev(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(a)
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def region_ordered(dims, window, shift):
    """layout, raster descriptors, the region order [nW, N], the descriptors in that order, the key ranges [nW, 13, 2]"""
    lay = O.window_layout(*dims, window, shift)
    N, nW = lay["N"], lay["nW"]
    Wd, Wh, Ww = window
    n = np.arange(N)
    code = (n // (Wh * Ww)) * (2 * Wh - 1) * (2 * Ww - 1) + ((n // Ww) % Wh) * (2 * Ww - 1) + n % Ww
    desc = lay["frag"][:, 0] | (lay["frag"][:, 1] << 8) | (lay["region"] << 16)
    tok = np.stack([np.tile(code, nW), desc], -1).astype(np.int32)
    order = kernels.attn32_row_order(tok, nW, N)
    tok_o = np.ascontiguousarray(tok.reshape(nW, N, 2)[np.arange(nW)[:, None], order].reshape(nW * N, 2))
    ranges = kernels.attn32_key_ranges(tok_o, nW, N, True)
    center = (Wd - 1) * (2 * Wh - 1) * (2 * Ww - 1) + (Wh - 1) * (2 * Ww - 1) + (Ww - 1)
    return lay, tok_o, order, ranges, center


def starts_at_block_0(ranges, N, BW):
    """bool [BW*N]: the rows whose q-block's range, widened as the kernel widens it (4 | 7 | 13 blocks), starts at key block 0 —
    every row whose range in the table starts at block 0 is one of them"""
    t0 = np.array([[AR.widened(int(f), int(l))[0] for f, l in win] for win in ranges])            # [nW, 13]
    assert ((t0 == 0) | (ranges[:, :, 0] > 0)).all()
    nW = ranges.shape[0]
    rows = np.arange(BW * N)
    return torch.from_numpy(t0[(rows // N) % nW, (rows % N) // 32] == 0)


def to_order(t, order, BW, N):
    """rows of t [BW, ..., N, ...] (window rows on axis -2) from raster into the region order"""
    nW = order.shape[0]
    idx = torch.from_numpy(order.astype(np.int64))[torch.arange(BW) % nW]            # [BW, N]
    return torch.stack([t[b].index_select(-2, idx[b]) for b in range(BW)])


def ranges_operands(dims, window, lay, nH, half):
    """(q2, k, v [BW, nH, N, 32] rounded to ``half``, in raster order; rpb, fpb) of one clip (BW = nW), q scaled by 0.6 log2(e)"""
    g = np.random.Generator(np.random.PCG64(sum(dims) + sum(window) + 300))
    N, BW = lay["N"], lay["nW"]
    tl = (2 * window[0] - 1) * (2 * window[1] - 1) * (2 * window[2] - 1)
    q2 = rnd(torch.from_numpy(g.standard_normal((BW, nH, N, 32)).astype(np.float32)) * (0.6 * kernels.LOG2E), half)
    k = rnd(torch.from_numpy(g.standard_normal((BW, nH, N, 32)).astype(np.float32)), half)
    v = rnd(torch.from_numpy(g.standard_normal((BW, nH, N, 32)).astype(np.float32)), half)
    rpb = torch.from_numpy((0.5 * g.standard_normal((tl, nH))).astype(np.float32))
    fpb = torch.from_numpy((0.5 * g.standard_normal((tl, nH))).astype(np.float32))
    return q2, k, v, rpb, fpb


# (dims, window, shift): eight (8,7,7) windows, one of each last / not-last combination along D, H and W (N = 392: the SHORT body); N < 385
# (the generic body): the smallest window with two regions on an axis, and a seven-block window whose ranges start past block 0
GEOMETRIES = [((16, 14, 14), (8, 7, 7), (4, 3, 3)), ((4, 4, 4), (2, 2, 2), (1, 1, 1)), ((8, 14, 14), (4, 7, 7), (2, 3, 3))]


@pytest.mark.parametrize("dims,window,shift", GEOMETRIES, ids=["w877", "w222", "w477"])
def test_ranges_launch_vs_oracle_and_full_launch(dims, window, shift, half):
    """nH = 2, BW = 8 (one clip).  Against O.attention_core on the same rows at the bounds of
    test_window_attention32_vs_oracle_and_gather_path; against kvq_window_attention32 (every key block, dsplit_from = -1) on the same
    inputs: rows whose range starts at block 0 bit for bit (the blocks passed over come last and add exact zeros), the others within
    the bound test_window_attention32_depth_split allows its second-half rows."""
    lay, tok_o, order, ranges, center = region_ordered(dims, window, shift)
    N, nW, nH = lay["N"], lay["nW"], 2
    BW = nW
    assert BW == 8
    q2, k, v, rpb, fpb = ranges_operands(dims, window, lay, nH, half)
    # the oracle works in raster order; its output rows move into the region order with the inputs
    ref = to_order(O.attention_core(q2 / kernels.LOG2E, k, v, rpb, fpb, window, lay), order, BW, N).reshape(BW * N, nH * 32)
    ref_img = to_order(O.attention_core(q2 / kernels.LOG2E, k, v, rpb, fpb, window, lay, image=True), order, BW, N).reshape(BW * N, nH * 32)
    qo, ko, vo = (to_order(t, order, BW, N) for t in (q2, k, v))
    qkv = dev(torch.stack([qo, ko, vo]).permute(0, 2, 1, 3, 4).reshape(3, nH, BW * N, 32).contiguous(), half)
    image = kernels.attn_bias32(dev(tok_o), dev(rpb), dev(fpb), center, nW, N, True)
    rng_d = dev(np.ascontiguousarray(ranges))
    out = kernels.window_attention32(qkv, image, nW, N, ranges=rng_d)
    full = kernels.window_attention32(qkv, image, nW, N)
    outf = out.float().cpu()
    assert torch.isfinite(outf).all()
    e_img, e_ref, e_mean = (outf - ref_img).abs().max().item(), (ref_img - ref).abs().max().item(), (outf - ref).abs().mean().item()
    same = starts_at_block_0(ranges, N, BW)
    d_full = (out.float() - full.float()).abs().max().item()
    print(f"N={N} {half}: |out - oracle(image)| {e_img:.3e}, image rounding {e_ref:.3e}, mean |out - oracle| {e_mean:.3e}, "
          f"|ranges - full| {d_full:.3e}, rows from block 0: {int(same.sum())} of {same.numel()}")
    assert e_img <= 6.4 * EPS[half]
    assert e_ref <= 2.0 ** -7
    assert e_mean <= 0.5 * EPS[half]
    assert torch.equal(out.cpu()[same], full.cpu()[same])
    assert d_full <= 2.0 * EPS[half] * float(full.float().abs().max())
    if N == 392:
        assert 0 < int(same.sum()) < same.numel()                        # both kinds of rows are exercised
        with pytest.raises(RuntimeError, match="ranges"):                # the depth split is a case of the ranges, not an addition to them
            kernels.window_attention32(qkv, image, nW, N, ranges=rng_d, dsplit_from=4)


def test_ranges_launch_with_fused_projection(half):
    """The fused-projection form (C = 96: three heads) on region-ordered rows with the ranges: against the oracle fed the q | k | v of the
    qkv GEMM on the same rows, and against the fused launch without ranges."""
    dims, window, shift = GEOMETRIES[0]
    C = 96
    g = np.random.Generator(np.random.PCG64(C + 41))
    lay, tok_o, order, ranges, center = region_ordered(dims, window, shift)
    N, nW, nH = lay["N"], lay["nW"], C // 32
    BW = nW
    x = rnd(torch.from_numpy(g.standard_normal((BW * N, C)).astype(np.float32)), half)             # rows in the region order
    Wq = rnd(torch.from_numpy((g.standard_normal((3 * C, C)) / np.sqrt(C)).astype(np.float32)), half)
    bq = torch.from_numpy(0.3 * g.standard_normal(3 * C).astype(np.float32))
    scale = 32 ** -0.5 * kernels.LOG2E
    rpb = torch.from_numpy((0.5 * g.standard_normal((2535, nH))).astype(np.float32))
    fpb = torch.from_numpy((0.5 * g.standard_normal((2535, nH))).astype(np.float32))
    image = kernels.attn_bias32(dev(tok_o), dev(rpb), dev(fpb), center, nW, N, True)
    qkv = kernels.gemm(dev(x, half), dev(Wq, half), dev(bq), _abi.EPI_QKV_BF16, num_heads=nH, q_scale=scale)      # [3, nH, BW*N, 32]
    # back to raster order for the oracle, its output into the region order again
    inv = np.argsort(order, axis=1)
    q2, k, v = (to_order(qkv[i].float().cpu().reshape(nH, BW, N, 32).permute(1, 0, 2, 3), inv, BW, N) for i in range(3))
    ref_img = to_order(O.attention_core(q2 / kernels.LOG2E, k, v, rpb, fpb, window, lay, image=True), order, BW, N).reshape(BW * N, C)
    ref = to_order(O.attention_core(q2 / kernels.LOG2E, k, v, rpb, fpb, window, lay), order, BW, N).reshape(BW * N, C)
    fused = dict(x_ln=dev(x, half), w_qkv=dev(Wq, half), b_qkv=dev(bq), q_scale=scale)
    rng_d = dev(np.ascontiguousarray(ranges))
    scratch = torch.full((1, nH, BW * N, 32), float("nan"), dtype=half, device=DEV)
    out = kernels.window_attention32(scratch, image, nW, N, ranges=rng_d, **fused)
    full = kernels.window_attention32(torch.empty_like(scratch), image, nW, N, **fused)
    outf = out.float().cpu()
    assert torch.isfinite(outf).all()
    e_img, e_ref, e_mean = (outf - ref_img).abs().max().item(), (ref_img - ref).abs().max().item(), (outf - ref).abs().mean().item()
    d_full = (out.float() - full.float()).abs().max().item()
    print(f"fused {half}: |out - oracle(image)| {e_img:.3e}, image rounding {e_ref:.3e}, mean |out - oracle| {e_mean:.3e}, |ranges - full| {d_full:.3e}")
    assert e_img <= 6.4 * EPS[half]
    assert e_ref <= 2.0 ** -7
    assert e_mean <= 0.5 * EPS[half]
    same = starts_at_block_0(ranges, N, BW)
    assert torch.equal(out.cpu()[same], full.cpu()[same])
    assert d_full <= 2.0 * EPS[half] * float(full.float().abs().max())
    assert (scratch[0].float() - qkv[0].float()).abs().max().item() <= 2.0 * EPS[half] * qkv[0].float().abs().max().item()
