"""GPU: every main loop of kvq_gemm_bf16 / kvq_conv_implicit against a reference at kernel level — the seven ring tiles, the 2-slice
QKV ring, the eight-phase kernel, the implicit-GEMM forms (tap walk and tap table) and split-K wrapped around the big tiles.

The shapes come from tests/gemm_forms.py; every case first asserts, through ``kernels.gemm_kernel_choice``, that its shape reaches
the form it is named after (tests/test_gemm_choice_cpu.py pins the same table without a GPU), so no case can pass on another kernel.

Bit-exact cases (tolerance zero).  A and W hold integers in [-3, 3], the bias integers in [-8, 8], the residual input integers in
[-64, 64], col_scale values of {-0.25, 0.5, 1, 2}, q_scale = 0.25.  With K <= 1600 every product and partial sum is an integer below
9 * 1600 + 72 < 2^24: the fp32 accumulation is exact in ANY order, under split-K as well, and every operand is exact in fp16 and
bf16.  The reference is the fp64 product on the CPU (exact too); an fp32 output must equal it, a 16-bit output must equal it
narrowed by round-to-nearest-even (bf16 meets real ties: integers above 256 have a 2, 4, ... spacing).  Any wrong, missing, doubled
or misplaced k-slice, row or column changes an integer and fails the case.

Rounded cases: GELU and QuickGELU on Gaussian operands rounded to the type, against fp64, within the bound
tests/test_gpu_kernels.py states for the GELU epilogue (one 16-bit rounding of the result + 1e-4 for the fp32 accumulation and the
fast exponential); QuickGELU is the same chain (fp32 value, one rounding) and takes the same bound.

Skipped cases: none."""
import contextlib
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kvq_amd  # noqa: F401
from gemm_forms import BY_NAME, CONV, GEMM, QKV, conv_rows
from kvq_amd import _abi, kernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}     # half-ulp relative rounding error
SENTINEL = 0x7E5A                                                 # 16-bit pattern no case computes (fp16: a NaN, bf16: 4.5e37)


@pytest.fixture(params=[torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def half(request):
    return request.param


def gen(seed):
    return np.random.Generator(np.random.PCG64(seed))


def ints(g, lo, hi, *shape):
    return torch.from_numpy(g.integers(lo, hi + 1, size=shape)).double()


def dev(t, dtype=None):
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def narrowed(ref, half):
    """the exact fp64 reference (every value is exact in fp32) as the 16-bit type holds it: round to nearest even"""
    return ref.to(torch.float32).to(half)


def same(got, want, what):
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    first = tuple(bad[0].tolist())
    raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ, first wrong index {first}: got {got[first].item()}, "
                         f"want {want[first].item()}")


@contextlib.contextmanager
def form(c, epi=_abi.EPI_BIAS_BF16):
    """sets the case's tile mode, asserts that the launch takes the case's main loop, restores the mode"""
    mode = getattr(c, "mode", -1)
    prev = kernels.gemm_tile_mode(mode)
    try:
        if hasattr(c, "shape"):
            assert kernels.gemm_kernel_choice(conv_rows(c), c.Cout, c.Kpad, epi, True) == c.code
        else:
            assert kernels.gemm_kernel_choice(c.M, c.N, c.K, epi) == c.code
            assert (_abi.lib().kvq_gemm_splitk_factor(c.M, c.N, c.K) > 1) == c.split
        yield
    finally:
        kernels.gemm_tile_mode(prev)


def batches(M):
    return next(b for b in (3, 2, 1) if M % b == 0)


@functools.lru_cache(maxsize=None)
def exact(M, N, K):
    """integer operands of a shape and their exact product, shared by every case and type of that shape (never modified)"""
    g = gen(M * 7 + N * 3 + K)
    A, W = ints(g, -3, 3, M, K), ints(g, -3, 3, N, K)
    return dict(A=A, W=W, b=ints(g, -8, 8, N), x=ints(g, -64, 64, M, N), ref=A @ W.t(),
                cs=torch.from_numpy(g.choice(np.array([-0.25, 0.5, 1.0, 2.0]), size=N)).double())


@functools.lru_cache(maxsize=None)
def gaussian(M, N, K, half):
    g = gen(M + N + K)
    A = torch.from_numpy(g.standard_normal((M, K)).astype(np.float32)).to(half)
    W = torch.from_numpy((g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)).to(half)
    b = torch.from_numpy(g.standard_normal(N).astype(np.float32))
    return A, W, b, A.double() @ W.double().t() + b.double()


PLAIN = pytest.mark.parametrize("c", GEMM, ids=lambda c: c.name)


# ------------------------------------------------------------------------------------------------------------ plain GEMMs
@PLAIN
def test_store_bias_and_placement_exact(c, half):
    """STORE_F32 with and without bias, the 16-bit BIAS store; a padded identity against an asymmetric W (a transposed C write, swapped
    operands or a shifted tile move an element); split-K: two identical calls are bit-equal."""
    e = exact(c.M, c.N, c.K)
    A, W, b = dev(e["A"], half), dev(e["W"], half), dev(e["b"], torch.float32)
    with form(c, _abi.EPI_STORE_F32):
        same(kernels.gemm(A, W, b, _abi.EPI_STORE_F32), (e["ref"] + e["b"]).float(), "STORE_F32 + bias")
        out = kernels.gemm(A, W, None, _abi.EPI_STORE_F32)
        same(out, e["ref"].float(), "STORE_F32")
        if c.split:
            assert torch.equal(out, kernels.gemm(A, W, None, _abi.EPI_STORE_F32))
        same(kernels.gemm(A, W, b, _abi.EPI_BIAS_BF16), narrowed(e["ref"] + e["b"], half), "BIAS")
        eye = torch.zeros(c.M, c.K)
        d = min(c.M, c.K)
        eye[range(d), range(d)] = 1.0
        Wa = torch.arange(c.N * c.K, dtype=torch.float32).reshape(c.N, c.K) % 251 - 125          # |.| <= 125: exact in bf16
        want = torch.zeros(c.M, c.N)
        want[:d] = Wa.t()[:d]
        same(kernels.gemm(dev(eye, half), dev(Wa, half), None, _abi.EPI_STORE_F32), want, "padded identity x asymmetric W")


@PLAIN
def test_relu_and_identity_branches_exact(c, half):
    """conv_gemm's ReLU epilogue: plain, with the 16-bit identity branch, with the fp32 identity branch and the fp32 copy"""
    e = exact(c.M, c.N, c.K)
    A, W, b = dev(e["A"], half), dev(e["W"], half), dev(e["b"], torch.float32)
    y = e["ref"] + e["b"]
    with form(c, _abi.EPI_RELU_BF16):
        same(kernels.conv_gemm(A, W, b, True), narrowed(torch.relu(y), half), "RELU")
        same(kernels.conv_gemm(A, W, b, True, resid=dev(e["x"], half)), narrowed(torch.relu(y + e["x"]), half), "RELU + 16-bit identity")
        y16, y32 = kernels.conv_gemm(A, W, b, True, resid_f32=dev(e["x"], torch.float32), want_f32=True)
        same(y32, torch.relu(y + e["x"]).float(), "RELU + fp32 identity: the fp32 copy")
        same(y16, narrowed(torch.relu(y + e["x"]), half), "RELU + fp32 identity")


@PLAIN
def test_residual_epilogues_exact(c, half):
    """RESID_F32 with the identity map, with a scatter map that permutes rows and drops some (their rows of x stay as they were),
    with a row gather of A; RESID_SCALE_F32."""
    e = exact(c.M, c.N, c.K)
    M, N = c.M, c.N
    A, W, b = dev(e["A"], half), dev(e["W"], half), dev(e["b"], torch.float32)
    y = e["ref"] + e["b"]
    g = gen(c.M + 11)
    B = batches(M)
    R = M // B
    with form(c, _abi.EPI_RESID_F32):
        x = dev(e["x"], torch.float32)
        kernels.gemm(A, W, b, _abi.EPI_RESID_F32, out=x)
        same(x, (e["x"] + y).float(), "RESID_F32")
        # GEMM row b*R + r -> output row b*L + smap[r], smap a random injection of the kept rows; ~7 % of the rows dropped
        L = R - R // 14
        smap = np.full(R, -1, np.int64)
        smap[g.permutation(R)[:L]] = g.permutation(L)
        x0 = ints(g, -64, 64, B * L, N)
        want = x0.clone().reshape(B, L, N)
        kept = torch.from_numpy(smap >= 0)
        want[:, torch.from_numpy(smap[smap >= 0])] += y.reshape(B, R, N)[:, kept]
        x = dev(x0, torch.float32)
        kernels.gemm(A, W, b, _abi.EPI_RESID_F32, out=x, scatter_map=dev(torch.from_numpy(smap.astype(np.int32))), map_rows=R, out_rows=L)
        same(x, want.reshape(B * L, N).float(), "RESID_F32 + scatter map")
        # row b*R + r of the GEMM reads row b*P + gmap[r] of a taller A whose other rows hold other integers
        P = R + 37
        gmap = g.permutation(P)[:R]
        Ap = ints(g, -3, 3, B, P, c.K)
        Ap[:, torch.from_numpy(gmap)] = e["A"].reshape(B, R, c.K)
        x = dev(e["x"], torch.float32)
        kernels.gemm(dev(Ap.reshape(B * P, c.K), half), W, b, _abi.EPI_RESID_F32, out=x, a_gather=dev(torch.from_numpy(gmap.astype(np.int32))),
                     a_rows=R, rows=M)
        same(x, (e["x"] + y).float(), "RESID_F32 + a_gather")
    with form(c, _abi.EPI_RESID_SCALE_F32):
        x = dev(e["x"], torch.float32)
        kernels.gemm(A, W, b, _abi.EPI_RESID_F32, out=x, col_scale=dev(e["cs"], torch.float32))
        same(x, (e["x"] + e["cs"] * y).float(), "RESID_SCALE_F32")


@PLAIN
def test_gelu_and_quick_gelu_rounded(c, half):
    A, W, b, ref = gaussian(c.M, c.N, c.K, half)
    Ad, Wd, bd = dev(A), dev(W), dev(b)
    ref_g = F.gelu(ref.float())
    ref_q = (ref * torch.sigmoid(1.702 * ref)).float()
    with form(c, _abi.EPI_GELU_BF16):
        err = (kernels.gemm(Ad, Wd, bd, _abi.EPI_GELU_BF16).float().cpu() - ref_g).abs().max().item()
        bound = EPS[half] * ref_g.abs().max().item() + 1e-4
        print(f"{c.name} GELU max err {err:.3e} bound {bound:.3e}")
        assert err <= bound
    with form(c, _abi.EPI_QGELU_BF16):
        err = (kernels.gemm(Ad, Wd, bd, _abi.EPI_QGELU_BF16).float().cpu() - ref_q).abs().max().item()
        bound = EPS[half] * ref_q.abs().max().item() + 1e-4
        print(f"{c.name} QGELU max err {err:.3e} bound {bound:.3e}")
        assert err <= bound


# ------------------------------------------------------------------------------------------------------------ QKV epilogue
@pytest.mark.parametrize("c", QKV, ids=lambda c: c.name)
def test_qkv_epilogue_exact(c, half):
    """head-major q | k | v with q scaled; with a token -> window-row scatter map the rows no token lands in keep the sentinel"""
    e = exact(c.M, c.N, c.K)
    M, nH = c.M, c.nH
    A, W, b = dev(e["A"], half), dev(e["W"], half), dev(e["b"], torch.float32)
    ref = (e["ref"] + e["b"]).reshape(M, 3, nH, 32).permute(1, 2, 0, 3).clone()
    ref[0] *= 0.25
    ref = narrowed(ref, half)
    g = gen(c.M + 13)
    B = batches(M)
    L = M // B
    Lp = L + L // 10
    inv = np.sort(g.permutation(Lp)[:L]) if L % 2 else g.permutation(Lp)[:L]
    with form(c, _abi.EPI_QKV_BF16):
        same(kernels.gemm(A, W, b, _abi.EPI_QKV_BF16, num_heads=nH, q_scale=0.25), ref, "QKV")
        out = torch.empty(3, nH, B * Lp, 32, dtype=half, device=DEV)
        out.view(torch.int16).fill_(SENTINEL)
        kernels.gemm(A, W, b, _abi.EPI_QKV_BF16, num_heads=nH, q_scale=0.25, out=out, scatter_map=dev(torch.from_numpy(inv.astype(np.int32))),
                     map_rows=L, out_rows=Lp)
    out = out.cpu().reshape(3, nH, B, Lp, 32)
    hit = torch.zeros(Lp, dtype=torch.bool)
    hit[torch.from_numpy(inv)] = True
    same(out[:, :, :, torch.from_numpy(inv)], ref.reshape(3, nH, B, L, 32), "QKV + scatter map")
    assert bool((out[:, :, :, ~hit].contiguous().view(torch.int16) == SENTINEL).all()), "QKV + scatter map wrote a row no token maps to"


# ------------------------------------------------------------------------------------------------------- implicit GEMM
@functools.lru_cache(maxsize=None)
def conv_exact(name):
    c = BY_NAME[name]
    g = gen(sum(c.shape) + c.Cout)
    Cc, N, M = c.shape[-1], c.Cout, conv_rows(c)
    x, w5, b = ints(g, -3, 3, *c.shape), ints(g, -3, 3, N, Cc, *c.kernel), ints(g, -8, 8, N)
    K = w5[0].numel()
    wk = torch.zeros(N, c.Kpad, dtype=torch.float64)
    wk[:, :K] = w5.permute(0, 2, 3, 4, 1).reshape(N, K)                 # the (kd, kh, kw, c) column order of im2col_nd
    ref = F.conv3d(x.permute(0, 4, 1, 2, 3), w5, b, 1, c.pad).permute(0, 2, 3, 4, 1).reshape(M, N).contiguous()
    return dict(x=x, wk=wk, b=b, r=ints(g, -64, 64, M, N), ref=ref)


def both_tap_forms(c, call, what):
    """``call`` with the walked taps (C % 32 == 0) and with the tap table: bit-equal; C % 32 != 0 has the table only"""
    assert not kernels.TAP_TABLE
    outs = [call()] if c.shape[-1] % 32 == 0 else []
    kernels.TAP_TABLE = True
    try:
        outs.append(call())
    finally:
        kernels.TAP_TABLE = False
    if len(outs) == 2:
        assert torch.equal(outs[0], outs[1]), f"{what}: walked taps differ from the tap table"
    return outs[0]


@pytest.mark.parametrize("c", CONV, ids=lambda c: c.name)
def test_conv_implicit_exact(c, half):
    """ReLU, ReLU + the 16-bit identity branch and the fp32 store against F.conv3d in fp64 on the integer operands, through the
    walked taps and the tap table; split-K: two identical calls are bit-equal.  The smallest C % 32 != 0 geometry that reaches a
    big tile (conv-128x128-table) lies below the size cap and runs like the others, on the table alone."""
    e = conv_exact(c.name)
    M, N = conv_rows(c), c.Cout
    x, w, b = dev(e["x"], half), dev(e["wk"], half), dev(e["b"], torch.float32)
    k, s, p = c.kernel, (1, 1, 1), c.pad
    with form(c):
        got = both_tap_forms(c, lambda: kernels.conv_implicit(x, w, b, k, s, p, True), "ReLU")
        same(got.reshape(M, N), narrowed(torch.relu(e["ref"]), half), "conv ReLU")
        if c.split:
            assert torch.equal(got, kernels.conv_implicit(x, w, b, k, s, p, True))
        r = dev(e["r"], half)
        got = both_tap_forms(c, lambda: kernels.conv_implicit(x, w, b, k, s, p, True, resid=r), "ReLU + identity")
        same(got.reshape(M, N), narrowed(torch.relu(e["ref"] + e["r"]), half), "conv ReLU + identity")
        got = both_tap_forms(c, lambda: kernels.conv_implicit(x, w, b, k, s, p, False, store_f32=True), "store_f32")
        same(got, e["ref"].float(), "conv store_f32")


# ------------------------------------------------------------------------------------------------------- ldc / col_off
def sentinel_rows(M, ldc, half):
    out = torch.empty(M, ldc, dtype=half, device=DEV)
    out.view(torch.int16).fill_(SENTINEL)
    return out


def placed(out, plain, col_off, what):
    """columns col_off .. col_off+N-1 of ``out`` are bit-equal to the plain launch, every other column still holds the sentinel"""
    N = plain.shape[-1]
    bits = out.view(torch.int16)
    assert torch.equal(bits[:, col_off:col_off + N], plain.reshape(out.shape[0], N).view(torch.int16)), f"{what}: the placed columns differ"
    assert bool((bits[:, :col_off] == SENTINEL).all()) and bool((bits[:, col_off + N:] == SENTINEL).all()), f"{what}: wrote outside its columns"


@pytest.mark.parametrize("name", ["64x64x32", "192x128x64", "256x256x64", "splitk-128x64x32"])
def test_gemm_channel_concatenation_store(name, half):
    """The 16-bit epilogues writing their N columns at column col_off of rows of ldc elements (csrc/convnet.hip's channel
    concatenation), on the 64 x 64 tile, a big ring tile, the eight-phase kernel and through the split-K reduce."""
    c = BY_NAME[name]
    e = exact(c.M, c.N, c.K)
    A, W, b, r = dev(e["A"], half), dev(e["W"], half), dev(e["b"], torch.float32), dev(e["x"], half)
    ldc, off = c.N + 40, 16
    Ag, Wg, bg, _ = gaussian(c.M, c.N, c.K, half)
    with form(c):
        for what, plain, into in [
                ("BIAS", lambda: kernels.gemm(A, W, b, _abi.EPI_BIAS_BF16), lambda o: kernels.gemm(A, W, b, _abi.EPI_BIAS_BF16, out=o, ldc=ldc, col_off=off)),
                ("GELU", lambda: kernels.gemm(dev(Ag), dev(Wg), dev(bg), _abi.EPI_GELU_BF16),
                 lambda o: kernels.gemm(dev(Ag), dev(Wg), dev(bg), _abi.EPI_GELU_BF16, out=o, ldc=ldc, col_off=off)),
                ("QGELU", lambda: kernels.gemm(dev(Ag), dev(Wg), dev(bg), _abi.EPI_QGELU_BF16),
                 lambda o: kernels.gemm(dev(Ag), dev(Wg), dev(bg), _abi.EPI_QGELU_BF16, out=o, ldc=ldc, col_off=off)),
                ("RELU + identity", lambda: kernels.conv_gemm(A, W, b, True, resid=r),
                 lambda o: kernels.conv_gemm(A, W, b, True, resid=r, out=o, ldc=ldc, col_off=off))]:
            out = sentinel_rows(c.M, ldc, half)
            into(out)
            placed(out, plain(), off, f"{name} {what}")
        # the last columns of the rows, and a destination exactly as wide as N at offset 0
        out = sentinel_rows(c.M, ldc, half)
        kernels.gemm(A, W, b, _abi.EPI_BIAS_BF16, out=out, ldc=ldc, col_off=40)
        placed(out, kernels.gemm(A, W, b, _abi.EPI_BIAS_BF16), 40, f"{name} BIAS at the row's end")
        same(kernels.gemm(A, W, b, _abi.EPI_BIAS_BF16, out=sentinel_rows(c.M, c.N, half), ldc=c.N), narrowed(e["ref"] + e["b"], half), "ldc = N")


@pytest.mark.parametrize("name", ["conv-128x64", "conv-splitk-128x128"])
def test_conv_implicit_channel_concatenation_store(name, half):
    c = BY_NAME[name]
    e = conv_exact(name)
    M, N = conv_rows(c), c.Cout
    x, w, b, r = dev(e["x"], half), dev(e["wk"], half), dev(e["b"], torch.float32), dev(e["r"], half)
    ldc, off = N + 24, 8
    with form(c):
        for relu, resid in [(True, r), (False, None)]:
            out = sentinel_rows(M, ldc, half)
            assert kernels.conv_implicit(x, w, b, c.kernel, (1, 1, 1), c.pad, relu, resid=resid, out=out, ldc=ldc, col_off=off) is out
            placed(out, kernels.conv_implicit(x, w, b, c.kernel, (1, 1, 1), c.pad, relu, resid=resid), off, f"{name} relu={relu}")


def test_channel_concatenation_refusals(half):
    """what the library refuses: col_off without ldc, ldc with an fp32 or the QKV epilogue, offsets and pitches that are no multiple
    of 8, columns past the row's end — each before any launch (the destination keeps its sentinel)"""
    c = BY_NAME["64x64x32"]
    e = exact(c.M, c.N, c.K)
    M, N = c.M, c.N
    A, W, b = dev(e["A"], half), dev(e["W"], half), dev(e["b"], torch.float32)
    ldc = N + 40
    out = sentinel_rows(M, ldc, half)
    x32 = torch.zeros(M, ldc, device=DEV)
    for kw in [dict(col_off=16), dict(ldc=ldc, col_off=12), dict(ldc=ldc, col_off=48), dict(ldc=ldc, col_off=-8)]:
        with pytest.raises(_abi.KvqError, match="col_off"):
            kernels.gemm(A, W, b, _abi.EPI_BIAS_BF16, out=out, **kw)
        with pytest.raises(_abi.KvqError, match="col_off"):
            kernels.conv_gemm(A, W, b, True, out=out, **kw)
    with pytest.raises(_abi.KvqError, match="col_off"):
        kernels.gemm(A, W, b, _abi.EPI_BIAS_BF16, out=torch.empty(M, ldc + 4, dtype=half, device=DEV), ldc=ldc + 4, col_off=8)
    for epi in (_abi.EPI_STORE_F32, _abi.EPI_RESID_F32):
        with pytest.raises(_abi.KvqError, match="ldc"):
            kernels.gemm(A, W, b, epi, out=x32, ldc=ldc, col_off=8)
    with pytest.raises(_abi.KvqError, match="ldc"):
        kernels.gemm(A, W, b, _abi.EPI_RESID_F32, out=x32, ldc=ldc, col_scale=torch.ones(N, device=DEV))
    q = BY_NAME["qkv-128x64x32"]
    with pytest.raises(_abi.KvqError, match="ldc"):
        kernels.gemm(dev(torch.zeros(64, q.K), half), dev(torch.zeros(q.N, q.K), half), None, _abi.EPI_QKV_BF16, num_heads=q.nH,
                     out=torch.empty(3, q.nH, 64, 32, dtype=half, device=DEV), ldc=q.N, col_off=0)
    cc = BY_NAME["conv-64x64"]
    ce = conv_exact(cc.name)
    Mc = conv_rows(cc)
    xc, wc = dev(ce["x"], half), dev(ce["wk"], half)
    oc = sentinel_rows(Mc, cc.Cout + 24, half)
    for kw in [dict(col_off=8), dict(ldc=cc.Cout + 24, col_off=4), dict(ldc=cc.Cout + 24, col_off=32)]:
        with pytest.raises(_abi.KvqError, match="col_off"):
            kernels.conv_implicit(xc, wc, None, cc.kernel, (1, 1, 1), cc.pad, True, out=oc, **kw)
    with pytest.raises(_abi.KvqError, match="ldc"):
        kernels.conv_implicit(xc, wc, None, cc.kernel, (1, 1, 1), cc.pad, False, store_f32=True, ldc=cc.Cout + 24, col_off=8)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == SENTINEL).all()) and bool((oc.view(torch.int16) == SENTINEL).all()) and not bool(x32.any())
