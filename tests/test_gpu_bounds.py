"""GPU: no kernel writes, reads or skips outside its tensors' bounds (tests/guarded.py; DESIGN.md, "Memory bounds").

Every case runs one entry point of kvq_amd/kernels.py twice on the same inputs: once on plain device tensors, once inside
``guarded()`` with every input and every caller-supplied output copied into a guard-band buffer and every allocation the wrapper
makes (outputs, split-K scratch, weight packs, workspaces) guarded as well.  Asserted:

  (a) every guard of every allocation of the call is intact                           -> no store past an end or in front of a start
  (b) the written region of every output is byte-equal to the plain run               -> no result depends on memory outside an input
      (a wrapped floating input is surrounded by NaN; there are no floating atomics in csrc, so the launches are bit-reproducible)
  (c) no written element still holds the 0xFF payload, every floating output is finite -> no element is skipped
      (byte outputs, where 255 is a value: a third run with a 0x00 payload must give the same bytes)
  (d) rows / columns an entry point documents it leaves alone still hold the payload

The shapes are the smallest ragged ones of the value tests (tests/test_gpu_kernels.py and friends) and, for the GEMM and the
implicit-GEMM convolution, one ragged shape per big main loop of tests/gemm_forms.py (each case asserts the form its shape reaches)
with the ldc / col_off store; values are random, no reference is needed here.  Integer tables are wrapped with ZERO guards (tests/guarded.py: the blind spot), so an over-read of an index table is
not detected.  The end-to-end forwards allocate through the plan's workspaces and are out of scope.

Skipped cases: none.
"""
import contextlib

import numpy as np
import pytest
import torch

import kvq_amd  # noqa: F401
from gemm_forms import BY_NAME, conv_rows
from gemm_forms import CONV as CONV_FORMS
from gemm_forms import QKV as QKV_FORMS
from guarded import guarded
from kvq_amd import _abi, kernels
from kvq_amd.utils import synth
from oracle import sampler_oracle as SO
from oracle import swin3d_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HALVES = {"fp16": torch.float16, "bf16": torch.bfloat16}
WIN = (8, 7, 7)


class Out:
    """a caller-supplied output buffer: handed to the call holding the payload pattern (plain run: filled by hand)"""

    def __init__(self, *shape, dtype):
        self.shape, self.dtype = shape, dtype


class Keep:
    """output ``index`` keeps the elements ``mask`` (bool, the output's shape): they still hold the payload — or, with ``like``, the
    bytes of that input (an in-place tensor)"""

    def __init__(self, index, mask, like=None):
        self.index, self.mask, self.like = index, mask, like


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8).view(-1, t.element_size())


def _listify(r):
    if torch.is_tensor(r):
        return [r]
    return [t for t in r if t is not None]


def _plain_inputs(inputs):
    out = {}
    for k, v in inputs.items():
        if isinstance(v, Out):
            out[k] = torch.empty(*v.shape, dtype=v.dtype, device=DEV)
            out[k].view(-1).view(torch.uint8).fill_(0xFF)
        else:
            out[k] = v.clone() if torch.is_tensor(v) else v
    return out


def _guarded_run(inputs, call, payload):
    with guarded("cuda", payload=payload) as G:
        t = {}
        for k, v in inputs.items():
            if isinstance(v, Out):
                t[k] = torch.empty(*v.shape, dtype=v.dtype, device=DEV)
            else:
                t[k] = G.wrap(v, name=k) if torch.is_tensor(v) else v
        got = _listify(call(t))
        report = G.intact()
    return G, got, report


def check(inputs, call, keeps=()):
    inputs = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in inputs.items()}
    plain = _listify(call(_plain_inputs(inputs)))
    torch.cuda.synchronize()
    G, got, report = _guarded_run(inputs, call, 0xFF)
    assert report, f"(a) {report!r}"
    assert len(plain) == len(got) > 0
    keep = {k.index: k for k in keeps}
    masks = []
    for i, (p, q) in enumerate(zip(plain, got)):
        assert p.shape == q.shape and p.dtype == q.dtype, i
        k = keep.get(i)
        written = torch.ones(q.shape, dtype=torch.bool, device=q.device)
        if k is not None:
            m = k.mask.to(q.device).expand(q.shape)
            assert bool(m.any()) and not bool(m.all()), i
            if k.like is None:
                written = ~m
                assert G.untouched(q, m), f"(d) output {i}: {G.untouched(q, m)!r}"
            else:
                assert torch.equal(_bytes(q).view(*q.shape, -1)[m], _bytes(inputs[k.like]).view(*q.shape, -1)[m]), f"(d) output {i}"
        w = written.reshape(-1)
        masks.append(written)
        if q.element_size() > 1:
            left = G.payload_left(q).reshape(-1)[w]
            assert not bool(left.any()), f"(c) output {i} {tuple(q.shape)}: {int(left.sum())} written elements still hold the payload"
        if q.dtype.is_floating_point:
            assert bool(torch.isfinite(q.reshape(-1)[w]).all()), f"(c) output {i}: not finite"
        pb, qb = _bytes(p)[w], _bytes(q)[w]
        same = (pb == qb).all(1)
        assert bool(same.all()), (f"(b) output {i} {tuple(q.shape)} {q.dtype}: {int((~same).sum())} of {same.numel()} written elements differ from "
                                  f"the plain run, first at flat index {int(w.nonzero()[int((~same).nonzero()[0])])}")
    if any(q.element_size() == 1 for q in got):
        _, again, report = _guarded_run(inputs, call, 0x00)
        assert report, f"(a) {report!r}"
        for i, (q, r) in enumerate(zip(got, again)):
            if q.element_size() == 1:
                assert torch.equal(q[masks[i]], r[masks[i]]), f"(c) output {i}: bytes follow the payload (never written)"


# ------------------------------------------------------------------------------------------------------------ input helpers
def gen(seed):
    return np.random.Generator(np.random.PCG64(seed))


def f32(g, *shape, sc=1.0, off=0.0):
    return torch.from_numpy((g.standard_normal(shape) * sc + off).astype(np.float32))


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))


def layout(dims, shift, window=WIN):
    lay = O.window_layout(*dims, window, shift)
    L = dims[0] * dims[1] * dims[2]
    src = lay["src"].astype(np.int64)
    inv = np.zeros(L, np.int32)
    inv[src[src >= 0]] = np.nonzero(src >= 0)[0].astype(np.int32)
    return lay, lay["nW"] * lay["N"], L, inv


def tok_table(lay, window):
    N, nW = lay["N"], lay["nW"]
    Wd, Wh, Ww = window
    n = np.arange(N)
    code = (n // (Wh * Ww)) * (2 * Wh - 1) * (2 * Ww - 1) + ((n // Ww) % Wh) * (2 * Ww - 1) + n % Ww
    desc = lay["frag"][:, 0] | (lay["frag"][:, 1] << 8) | (lay["region"] << 16)
    tok = np.stack([np.tile(code, nW), desc], -1).astype(np.int32)
    center = (Wd - 1) * (2 * Wh - 1) * (2 * Ww - 1) + (Wh - 1) * (2 * Ww - 1) + (Ww - 1)
    return tok, center, (2 * Wd - 1) * (2 * Wh - 1) * (2 * Ww - 1)


def merge_map(D, H, W):
    Hn, Wn = (H + 1) // 2, (W + 1) // 2
    mp = np.full((D, Hn, Wn, 4), -1, np.int32)
    for d in range(D):
        for h2 in range(Hn):
            for w2 in range(Wn):
                for part, (dh, dw) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)]):
                    hh, ww = 2 * h2 + dh, 2 * w2 + dw
                    if hh < H and ww < W:
                        mp[d, h2, w2, part] = (d * H + hh) * W + ww
    return mp.reshape(-1, 4), Hn, Wn


def next_dst(dims, shift):
    lay2 = O.window_layout(*dims, WIN, shift)
    L = dims[0] * dims[1] * dims[2]
    assert (lay2["src"] >= 0).all()
    dst = np.empty(L, np.int32)
    dst[lay2["src"]] = np.arange(L, dtype=np.int32)
    return dst, L


def row_mask(shape, axis, rows):
    """bool [shape]: True on the entries ``rows`` (bool vector) of ``axis``"""
    view = [1] * len(shape)
    view[axis] = shape[axis]
    return torch.as_tensor(rows).reshape(view).expand(shape)


@pytest.fixture(params=list(HALVES), ids=list(HALVES))
def half(request):
    return HALVES[request.param]


@pytest.fixture(params=[-1, 1], ids=["by-shape", "wide8p"])
def tile_mode(request):
    prev = kernels.gemm_tile_mode(request.param)
    yield request.param
    kernels.gemm_tile_mode(prev)


# ------------------------------------------------------------------------------------------------------------------- GEMM
GEMM_SHAPES = [(200, 96, 96), (130, 768, 3072), (98, 768, 3072), (196, 256, 1536)]          # the last two cut K (split-K scratch)


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_epilogues(M, N, K, half, tile_mode):
    g = gen(M + N + K)
    inputs = dict(A=f32(g, M, K).to(half), W=f32(g, N, K, sc=K ** -0.5).to(half), b=f32(g, N), x=f32(g, M, N))

    def call(t):
        outs = [kernels.gemm(t["A"], t["W"], t["b"], e) for e in (_abi.EPI_STORE_F32, _abi.EPI_BIAS_BF16, _abi.EPI_GELU_BF16, _abi.EPI_QGELU_BF16)]
        outs.append(kernels.gemm(t["A"], t["W"], None, _abi.EPI_STORE_F32))
        outs.append(kernels.gemm(t["A"], t["W"], t["b"], _abi.EPI_RESID_F32, out=t["x"]))
        return outs
    check(inputs, call)


@pytest.mark.parametrize("M,N,K", [(200, 96, 96), (98, 768, 3072)])
def test_conv_gemm_resid_f32_and_fp32_copy(M, N, K, half, tile_mode):
    g = gen(M + N + K + 1)
    inputs = dict(A=f32(g, M, K).to(half), W=f32(g, N, K, sc=K ** -0.5).to(half), b=f32(g, N), r=f32(g, M, N), r16=f32(g, M, N).to(half))

    def call(t):
        y16, y32 = kernels.conv_gemm(t["A"], t["W"], t["b"], True, resid_f32=t["r"], want_f32=True)
        return [y16, y32, kernels.conv_gemm(t["A"], t["W"], t["b"], True, resid=t["r16"]), kernels.conv_gemm(t["A"], t["W"], t["b"], False)]
    check(inputs, call)


def test_gemm_qkv_epilogue(half, tile_mode):
    g = gen(5)
    nH, M = 3, 392 * 2
    C = 32 * nH
    inputs = dict(A=f32(g, M, C).to(half), W=f32(g, 3 * C, C, sc=0.2).to(half), b=f32(g, 3 * C))
    check(inputs, lambda t: kernels.gemm(t["A"], t["W"], t["b"], _abi.EPI_QKV_BF16, num_heads=nH, q_scale=32 ** -0.5))


def test_gemm_qkv_scatter_and_row_gather_over_a_padded_partition(half, tile_mode):
    g = gen(61)
    C, B = 96, 2
    nH = C // 32
    lay, Lp, L, inv = layout((4, 10, 9), (4, 3, 3))
    pad = lay["src"] < 0
    inputs = dict(tok=f32(g, B * L, C).to(half), W=f32(g, 3 * C, C, sc=0.2).to(half), b=f32(g, 3 * C), inv=i32(inv),
                  qkv=Out(3, nH, B * Lp, 32, dtype=half),
                  A=f32(g, B * Lp, C).to(half), Wp=f32(g, C, C, sc=0.2).to(half), bp=f32(g, C), x=f32(g, B * L, C), x2=f32(g, B * L, C),
                  src=i32(lay["src"]))

    def call(t):
        kernels.gemm(t["tok"], t["W"], t["b"], _abi.EPI_QKV_BF16, num_heads=nH, q_scale=32 ** -0.5, out=t["qkv"], scatter_map=t["inv"],
                     map_rows=L, out_rows=Lp)
        kernels.gemm(t["A"], t["Wp"], t["bp"], _abi.EPI_RESID_F32, out=t["x"], a_gather=t["inv"], a_rows=L, rows=B * L)
        kernels.gemm(t["A"], t["Wp"], t["bp"], _abi.EPI_RESID_F32, out=t["x2"], scatter_map=t["src"], map_rows=Lp, out_rows=L)
        return [t["qkv"], t["x"], t["x2"]]
    check(inputs, call, [Keep(0, row_mask((3, nH, B * Lp, 32), 2, np.tile(pad, B)))])


def test_qkv_fill_pad(half):
    g = gen(62)
    C, B = 96, 2
    nH = C // 32
    lay, Lp, L, _ = layout((4, 10, 9), (4, 3, 3))
    pad = lay["src"] < 0
    inputs = dict(qkv=Out(3, nH, B * Lp, 32, dtype=half), b=f32(g, 3 * C), pad=i32(np.nonzero(pad)[0]))
    check(inputs, lambda t: kernels.qkv_fill_pad(t["qkv"], t["b"], t["pad"], B, 32 ** -0.5),
          [Keep(0, row_mask((3, nH, B * Lp, 32), 2, np.tile(~pad, B)))])


@contextlib.contextmanager
def form(c):
    """a row of tests/gemm_forms.py: its tile mode set and restored, its main loop asserted before anything is launched"""
    prev = kernels.gemm_tile_mode(getattr(c, "mode", -1))
    try:
        if hasattr(c, "shape"):
            assert kernels.gemm_kernel_choice(conv_rows(c), c.Cout, c.Kpad, _abi.EPI_RELU_BF16, True) == c.code
        else:
            assert kernels.gemm_kernel_choice(c.M, c.N, c.K, _abi.EPI_QKV_BF16 if c.nH else _abi.EPI_BIAS_BF16) == c.code
            assert (_abi.lib().kvq_gemm_splitk_factor(c.M, c.N, c.K) > 1) == c.split
        yield
    finally:
        kernels.gemm_tile_mode(prev)


BIG_FORMS = ["128x128x64", "128x128x32-mode0", "128x64x32", "192x128x64", "128x256x64", "splitk-128x128x32", "splitk-128x64x32"]


@pytest.mark.parametrize("name", BIG_FORMS)
def test_gemm_epilogues_on_the_big_ring_tiles(name, half):
    """one ragged shape per big ring tile (the 192-row tile over M = 3000, the 256-column tile over N = 2520, the shape mode 0 takes
    off the wide tile) and split-K around the two big 32-deep tiles: the last row and column tiles of every epilogue"""
    c = BY_NAME[name]
    M, N, K = c.M, c.N, c.K
    g = gen(M + N + K)
    inputs = dict(A=f32(g, M, K).to(half), W=f32(g, N, K, sc=K ** -0.5).to(half), b=f32(g, N), x=f32(g, M, N), r16=f32(g, M, N).to(half))

    def call(t):
        outs = [kernels.gemm(t["A"], t["W"], t["b"], e) for e in (_abi.EPI_STORE_F32, _abi.EPI_BIAS_BF16, _abi.EPI_GELU_BF16)]
        outs.append(kernels.conv_gemm(t["A"], t["W"], t["b"], True, resid=t["r16"]))
        outs.append(kernels.gemm(t["A"], t["W"], t["b"], _abi.EPI_RESID_F32, out=t["x"]))
        return outs
    with form(c):
        check(inputs, call)


@pytest.mark.parametrize("name", [c.name for c in QKV_FORMS])
def test_gemm_qkv_epilogue_on_the_big_ring_tiles(name, half):
    """the head-major store from the 256-column tile (N = 96 nH = 12 tiles), the 128 x 64 tile and the 2-slice ring; with the scatter
    map the rows no token lands in keep the payload"""
    c = BY_NAME[name]
    M, N, K, nH = c.M, c.N, c.K, c.nH
    g = gen(M + N + K)
    B = 2
    L = M // B
    Lp = L + 100
    inv = np.sort(g.permutation(Lp)[:L])
    hit = np.zeros(Lp, bool)
    hit[inv] = True
    inputs = dict(A=f32(g, M, K).to(half), W=f32(g, N, K, sc=K ** -0.5).to(half), b=f32(g, N), inv=i32(inv), qkv=Out(3, nH, B * Lp, 32, dtype=half))

    def call(t):
        kernels.gemm(t["A"], t["W"], t["b"], _abi.EPI_QKV_BF16, num_heads=nH, q_scale=32 ** -0.5, out=t["qkv"], scatter_map=t["inv"], map_rows=L,
                     out_rows=Lp)
        return [t["qkv"], kernels.gemm(t["A"], t["W"], t["b"], _abi.EPI_QKV_BF16, num_heads=nH, q_scale=32 ** -0.5)]
    with form(c):
        check(inputs, call, [Keep(0, row_mask((3, nH, B * Lp, 32), 2, np.tile(~hit, B)))])


@pytest.mark.parametrize("name", ["64x64x32", "192x128x64", "256x256x64", "splitk-128x128x32"])
def test_gemm_channel_concatenation_leaves_the_other_columns_alone(name, half):
    """ldc / col_off: the N columns land inside rows of ldc elements; the columns in front of and behind them keep the payload"""
    c = BY_NAME[name]
    M, N, K = c.M, c.N, c.K
    g = gen(M + N + K + 2)
    ldc, off = N + 40, 16
    inputs = dict(A=f32(g, M, K).to(half), W=f32(g, N, K, sc=K ** -0.5).to(half), b=f32(g, N), r16=f32(g, M, N).to(half),
                  o1=Out(M, ldc, dtype=half), o2=Out(M, ldc, dtype=half))
    cols = np.ones(ldc, bool)
    cols[off:off + N] = False

    def call(t):
        kernels.gemm(t["A"], t["W"], t["b"], _abi.EPI_GELU_BF16, out=t["o1"], ldc=ldc, col_off=off)
        kernels.conv_gemm(t["A"], t["W"], t["b"], True, resid=t["r16"], out=t["o2"], ldc=ldc, col_off=off)
        return [t["o1"], t["o2"]]
    with form(c):
        check(inputs, call, [Keep(0, row_mask((M, ldc), 1, cols)), Keep(1, row_mask((M, ldc), 1, cols))])


# -------------------------------------------------------------------------------------------------------------- LayerNorm
def test_layernorm_identity(half):
    g = gen(96)
    C, M = 96, 333
    inputs = dict(x=f32(g, M, C, sc=3, off=1.5), ga=f32(g, C, sc=0.1, off=1), be=f32(g, C, sc=0.1))
    check(inputs, lambda t: [kernels.layernorm_rows(t["x"], t["ga"], t["be"], out_dtype=torch.float32),
                             kernels.layernorm_rows(t["x"], t["ga"], t["be"], out_dtype=half)])


def test_layernorm_window_gather_writes_zeros_into_padding_rows(half):
    g = gen(23)
    C, B = 96, 2
    lay, Lp, L, _ = layout((4, 10, 9), (4, 3, 3))
    inputs = dict(x=f32(g, B * L, C), ga=f32(g, C, sc=0.1, off=1), be=f32(g, C, sc=0.1), src=i32(lay["src"]))
    pad = torch.from_numpy(np.tile(lay["src"] < 0, B))
    outs = []

    def call(t):
        outs[:] = [kernels.layernorm_rows(t["x"], t["ga"], t["be"], index_map=t["src"], n_batch=B, rows_out=Lp, out_dtype=dt)
                   for dt in (torch.float32, half)]
        return outs
    check(inputs, call)
    for o in outs:                                   # the guarded run's outputs: padding rows are written, as zeros
        assert bool((o[pad.to(o.device)] == 0).all())


def test_layernorm_merge_gather_odd_dims(half):
    g = gen(9)
    B, D, H, W, C = 2, 3, 5, 7, 96
    mp, Hn, Wn = merge_map(D, H, W)
    inputs = dict(x=f32(g, B * D * H * W, C), ga=f32(g, 4 * C, sc=0.1, off=1), be=f32(g, 4 * C, sc=0.1), mp=i32(mp))
    check(inputs, lambda t: [kernels.layernorm_rows(t["x"], t["ga"], t["be"], index_map=t["mp"], nparts=4, n_batch=B, rows_out=D * Hn * Wn,
                                                    out_dtype=dt) for dt in (torch.float32, half)])


# ------------------------------------------------------------------------------------------------------- window attention
def _attn_inputs(seed, dims, window, shift, nH, B, half, gated=True, q_scale=0.6):
    g = gen(seed)
    lay = O.window_layout(*dims, window, shift)
    N, nW = lay["N"], lay["nW"]
    tok, center, tl = tok_table(lay, window)
    qkv = f32(g, 3, nH, B * nW * N, 32)
    qkv[0] *= q_scale
    inputs = dict(qkv=qkv.to(half), tok=i32(tok), rpb=f32(g, tl, nH, sc=0.5))
    if gated:
        inputs["fpb"] = f32(g, tl, nH, sc=0.5)
    return inputs, lay, center


ATTN_GEOMS = [((4, 10, 9), WIN, (4, 3, 3), 1), ((8, 8, 8), (4, 4, 4), (2, 2, 2), 2)]         # N = 196 with padding rows; N = 64


@pytest.mark.parametrize("dims,window,shift,nH", ATTN_GEOMS, ids=["N196-padded", "N64"])
def test_window_attention(dims, window, shift, nH, half):
    inputs, lay, center = _attn_inputs(sum(dims) + nH, dims, window, shift, nH, 2, half)
    check(inputs, lambda t: kernels.window_attention(t["qkv"], t["tok"], t["rpb"], t["fpb"], center, lay["nW"], lay["N"], True))


def guarded_attn_bias32_and_window_attention32(dims, window, shift, nH, half):
    inputs, lay, center = _attn_inputs(sum(dims) + nH + 200, dims, window, shift, nH, 3, half, q_scale=0.6 * kernels.LOG2E)
    N, nW = lay["N"], lay["nW"]

    def call(t):
        image = kernels.attn_bias32(t["tok"], t["rpb"], t["fpb"], center, nW, N, True)
        return [image, kernels.window_attention32(t["qkv"], image, nW, N)]
    # the image ends with one 2048-byte block the builder leaves alone: the attention kernel requests block t0 + 1 unconditionally and
    # discards it behind the last one (kvq_attn_bias32_bytes) — what it holds (0xFF here, 0x00 in the third run) must not reach the output
    nb = _abi.lib().kvq_attn_bias32_bytes(nW, N, nH)
    check(inputs, call, [Keep(0, torch.arange(nb) >= nb - 2048)])


@pytest.mark.parametrize("dims,window,shift,nH", ATTN_GEOMS, ids=["N196-padded", "N64"])
def test_attn_bias32_and_window_attention32(dims, window, shift, nH, half):
    guarded_attn_bias32_and_window_attention32(dims, window, shift, nH, half)


def guarded_window_attention32_tile_skip(half):
    dims, nH, B = (4, 10, 9), 1, 3
    inputs, lay, center = _attn_inputs(77, dims, WIN, (4, 3, 3), nH, B, half, q_scale=0.6 * kernels.LOG2E)
    N, nW = lay["N"], lay["nW"]
    g = gen(78)
    nqt = -(-N // 16)
    skip = np.array([int(g.integers(0, 1 << nqt)) & ~3 for _ in range(nW)], np.int32)          # q-block 0 always runs
    skip[0] |= 0b1100                                                                         # ... and one q-block is skipped for certain
    rows = np.arange(B * nW * N)
    t0 = 2 * ((rows % N) // 32)
    sk = skip[(rows // N) % nW]
    both = (((sk >> t0) & 1) & (((sk >> (t0 + 1)) & 1) | (16 * (t0 + 1) >= N))).astype(bool)
    inputs.update(skip=i32(skip), out=Out(B * nW * N, nH * 32, dtype=half))

    def call(t):
        image = kernels.attn_bias32(t["tok"], t["rpb"], t["fpb"], center, nW, N, True)
        return kernels.window_attention32(t["qkv"], image, nW, N, tile_skip=t["skip"], out=t["out"])
    check(inputs, call, [Keep(0, row_mask((B * nW * N, nH * 32), 0, both))])


def test_window_attention32_tile_skip_leaves_skipped_rows_alone(half):
    guarded_window_attention32_tile_skip(half)


def guarded_window_attention32_depth_split(half):
    dims, nH, B = (16, 14, 14), 3, 2
    inputs, lay, center = _attn_inputs(51, dims, WIN, (4, 3, 3), nH, B, half, q_scale=0.7)
    N, nW = lay["N"], lay["nW"]
    first = nW - nW // 2

    def call(t):
        image = kernels.attn_bias32(t["tok"], t["rpb"], t["fpb"], center, nW, N, True)
        return kernels.window_attention32(t["qkv"], image, nW, N, dsplit_from=first)
    check(inputs, call)


def test_window_attention32_depth_split(half):
    guarded_window_attention32_depth_split(half)


def test_window_attention32_fused_projection_fills_the_q_scratch(half):
    dims, C, B = (8, 21, 14), 96, 2
    g = gen(131)
    lay = O.window_layout(*dims, WIN, (0, 0, 0))
    N, nW, nH = lay["N"], lay["nW"], C // 32
    BW = B * nW
    tok, center, tl = tok_table(lay, WIN)
    n_types = nW // (-(-dims[0] // lay["ws"][0]))
    inputs = dict(x=f32(g, BW * N, C).to(half), Wq=f32(g, 3 * C, C, sc=C ** -0.5).to(half), bq=f32(g, 3 * C, sc=0.3), tok=i32(tok[: n_types * N]),
                  rpb=f32(g, tl, nH, sc=0.5), q=Out(1, nH, BW * N, 32, dtype=half))

    def call(t):
        image = kernels.attn_bias32(t["tok"], t["rpb"], None, center, n_types, N, False)
        out = kernels.window_attention32(t["q"], image, nW, N, n_types, x_ln=t["x"], w_qkv=t["Wq"], b_qkv=t["bq"], q_scale=32 ** -0.5 * kernels.LOG2E)
        return [out, t["q"]]
    check(inputs, call)


def guarded_window_attention32_pad_mask(half):
    dims, nH, B = (8, 10, 9), 2, 2
    inputs, lay, center = _attn_inputs(177, dims, WIN, (4, 3, 3), nH, B, half, gated=False, q_scale=0.7)
    N, nW = lay["N"], lay["nW"]
    pad = lay["src"].reshape(nW, N) < 0
    assert pad.any() and not pad.all(1).any()
    inputs["qkv"][:, :, torch.from_numpy(np.tile(pad.reshape(-1), B))] = float("nan")          # rows the launch must not read
    mask = np.zeros((nW, 13), np.uint32)
    for wv in range(nW):
        for r in np.nonzero(pad[wv])[0]:
            mask[wv, r >> 5] |= np.uint32(1) << np.uint32(r & 31)
    inputs.update(bq=f32(gen(178), 3 * 32 * nH, sc=0.4), mask=torch.from_numpy(mask.view(np.int32)))

    def call(t):
        image = kernels.attn_bias32(t["tok"], t["rpb"], None, center, nW, N, True)
        return kernels.window_attention32(t["qkv"], image, nW, N, b_qkv=t["bq"], pad_mask=t["mask"])
    check(inputs, call)


def test_window_attention32_pad_mask_does_not_read_padding_rows(half):
    guarded_window_attention32_pad_mask(half)


def guarded_window_attention32_ranges(dims, window, shift, half):
    from test_gpu_attn_ranges import region_ordered
    g = gen(300)
    lay, tok_o, order, ranges, center = region_ordered(dims, window, shift)
    N, nW, nH = lay["N"], lay["nW"], 2
    tl = (2 * window[0] - 1) * (2 * window[1] - 1) * (2 * window[2] - 1)
    qkv = f32(g, 3, nH, nW * N, 32)
    qkv[0] *= 0.6 * kernels.LOG2E
    inputs = dict(qkv=qkv.to(half), tok=i32(tok_o), rpb=f32(g, tl, nH, sc=0.5), fpb=f32(g, tl, nH, sc=0.5),
                  ranges=torch.from_numpy(np.ascontiguousarray(ranges)))

    def call(t):
        image = kernels.attn_bias32(t["tok"], t["rpb"], t["fpb"], center, nW, N, True)
        return kernels.window_attention32(t["qkv"], image, nW, N, ranges=t["ranges"])
    check(inputs, call)


def test_window_attention32_ranges(half):
    guarded_window_attention32_ranges((4, 4, 4), (2, 2, 2), (1, 1, 1), half)


# --------------------------------------------------------------------------------------------------- fused token launches
def _tail_weights(g, C, half):
    hidden = 4 * C
    w = dict(Wp=f32(g, C, C, sc=0.15).to(half), bp=f32(g, C, sc=0.3), g2=f32(g, C, sc=0.2, off=1), b2n=f32(g, C, sc=0.2),
             W1=f32(g, hidden, C, sc=0.15).to(half), b1=f32(g, hidden, sc=0.3), W2=f32(g, C, hidden, sc=0.08).to(half), b2=f32(g, C, sc=0.3))
    d = {k: v.to(DEV) for k, v in w.items()}
    return kernels.block_tail_pack(d["Wp"], d["bp"], d["g2"], d["b2n"], d["W1"], d["b1"], d["W2"], d["b2"])


TAILS = [  # C, dims (None: identity over 333 rows), shift, mode, next shift, emit, fp16 stream
    (96, None, None, "identity", None, None, False),
    (192, (3, 5, 7), (0, 0, 0), "scatter", None, None, False),
    (384, (4, 10, 9), (4, 3, 3), "scatter", None, None, False),
    (384, (4, 10, 9), (4, 3, 3), "gather", None, None, False),
    (768, (16, 7, 7), (0, 0, 0), "scatter", None, None, False),
    (96, (8, 14, 14), (0, 0, 0), "scatter", (4, 3, 3), "norm", False),
    (192, (8, 14, 14), (0, 0, 0), "scatter", (4, 3, 3), "qkv", False),
    (96, (8, 14, 7), (4, 3, 3), "scatter", None, None, True),
]


@pytest.mark.parametrize("C,dims,shift,mode,nxt,emit,x16", TAILS,
                         ids=["C96-333rows", "C192-357", "C384-4109-scatter", "C384-4109-gather", "C768-1677", "C96-next-norm", "C192-next-qkv",
                              "C96-fp16-stream"])
def test_block_tail(C, dims, shift, mode, nxt, emit, x16, half):
    guarded_block_tail(C, dims, shift, mode, nxt, emit, x16, half)


def guarded_block_tail(C, dims, shift, mode, nxt, emit, x16, half):
    g = gen(C + (sum(dims) if dims else 0) + len(mode))
    hidden, B = 4 * C, 2
    inputs = dict(pack=_tail_weights(g, C, half))
    kw = {}
    if dims is None:
        M = rows_x = 333
    else:
        lay, Lp, L, inv = layout(dims, shift)
        M, rows_x = B * Lp, B * L
        if mode == "scatter":
            inputs["map"] = i32(lay["src"])
        else:
            inputs["map"] = i32(inv)
        kw = dict(map_rows=Lp, out_rows=L)
    inputs["A"] = f32(g, M, C).to(half)
    inputs["x"] = f32(g, rows_x, C, sc=2.0).to(torch.float16 if x16 else torch.float32)
    if emit:
        dst, Ln = next_dst(dims, nxt)
        inputs.update(gn=f32(g, C, sc=0.2, off=1), bn=f32(g, C, sc=0.2), dst=i32(dst))
        kw["next_rows"] = Ln
        if emit == "qkv":
            inputs.update(qpack=kernels.block_tail_qkv_pack(f32(g, 3 * C, C, sc=0.1).to(half).to(DEV), hidden), bq=f32(g, 3 * C, sc=0.3))

    def call(t):
        k = dict(kw)
        if "map" in t:
            k["scatter_map" if mode == "scatter" else "attn_gather"] = t["map"]
        if emit:
            k.update(next_norm=(t["gn"], t["bn"]), next_dst=t["dst"])
        if emit == "qkv":
            k["next_qkv"] = (t["qpack"], t["bq"], 0.25)
        nx = kernels.block_tail(t["A"], t["x"], t["pack"], hidden, **k)
        return [t["x"], nx]
    check(inputs, call)


@pytest.mark.parametrize("dims,emit", [((1, 3, 5, 7), False), ((2, 4, 8, 8), True)], ids=["1357", "2488-emit"])
def test_patch_merge(dims, emit, half):
    B, D, H, W = dims
    C = 96
    g = gen(sum(dims) + C)
    mp, Hn, Wn = merge_map(D, H, W)
    Ln = D * Hn * Wn
    inputs = dict(x=f32(g, B * D * H * W, C, sc=1.5), mp=i32(mp), red=f32(g, 2 * C, 4 * C, sc=(4 * C) ** -0.5), nw=f32(g, 4 * C, sc=0.2, off=1),
                  nb=f32(g, 4 * C, sc=0.2))
    if emit:
        dst, _ = next_dst((D, Hn, Wn), (0, 0, 0))
        inputs.update(gn=f32(g, 2 * C, sc=0.2, off=1), bn=f32(g, 2 * C, sc=0.2), dst=i32(dst))

    def call(t):
        kw = dict(next_norm=(t["gn"], t["bn"]), next_dst=t["dst"], next_rows=Ln) if emit else {}
        return kernels.patch_merge(t["x"], t["mp"], B, t["red"], t["nw"], t["nb"], out_dtype=half, **kw)
    check(inputs, call)


def test_patch_embed(half):
    shape, E = (1, 3, 6, 28, 44), 96
    g = gen(sum(shape) + E)
    inputs = dict(x=f32(g, *shape, sc=1.5), w=f32(g, E, 96, sc=0.1).to(half), b=f32(g, E, sc=0.2), lw=f32(g, E, sc=0.2, off=1), lb=f32(g, E, sc=0.2))
    check(inputs, lambda t: kernels.patch_embed(t["x"], t["w"], t["b"], t["lw"], t["lb"], (2, 4, 4)))


def _sampler_inputs(seed, T, Hs, Ws, grid, fs, aligned):
    g = torch.Generator().manual_seed(seed)
    gh = torch.tensor([min(Hs // grid * i, Hs - fs) for i in range(grid)]).view(grid, 1, 1)
    gw = torch.tensor([min(Ws // grid * i, Ws - fs) for i in range(grid)]).view(1, grid, 1)
    return dict(video=torch.randint(0, 256, (3, T, Hs, Ws), dtype=torch.uint8, generator=g),
                hoff=(torch.randint(max(1, Hs // grid - fs), (grid, grid, T // aligned), generator=g) + gh).int(),
                woff=(torch.randint(max(1, Ws // grid - fs), (grid, grid, T // aligned), generator=g) + gw).int())


def test_patch_embed_reads_through_the_sampler(half):
    geom = dict(T=6, Hs=64, Ws=64, grid=2, fs=32, aligned=1)
    E = 128
    g = gen(6)
    inputs = _sampler_inputs(43, **geom)
    inputs.update(w=f32(g, E, 96, sc=0.1).to(half), b=f32(g, E, sc=0.2), lw=f32(g, E, sc=0.2, off=1), lb=f32(g, E, sc=0.2))

    def call(t):
        src = kernels.FragmentSource([t["video"]], [t["hoff"]], [t["woff"]], 2, 2, 32, 32, 1, mean=synth.KVQ_MEAN, std=synth.KVQ_STD)
        return kernels.patch_embed(src, t["w"], t["b"], t["lw"], t["lb"], (2, 4, 4))
    check(inputs, call)


def test_patch_im2col(half):
    shape = (1, 3, 7, 30, 27)
    check(dict(x=f32(gen(sum(shape)), *shape)), lambda t: kernels.patch_im2col(t["x"], (2, 4, 4), out_dtype=half))


def test_fragment_gather():
    T, H, W, Fh, Fw, fs, al = 8, 224, 230, 7, 7, 32, 4
    g = gen(T + H)
    video = g.integers(0, 256, size=(3, T, H, W), dtype=np.uint8)
    rh, rw = synth.synth_fragment_offsets(T, T, H, W, Fh, Fw, fs, fs, al)
    hoff = rh + SO.fragment_grid(H, Fh, fs)[:, None, None].astype(np.int32)
    woff = rw + SO.fragment_grid(W, Fw, fs)[None, :, None].astype(np.int32)
    inputs = dict(v=torch.from_numpy(video), vf=torch.from_numpy(video.astype(np.float32)), hoff=i32(hoff), woff=i32(woff))

    def call(t):
        args = (t["hoff"], t["woff"], Fh, Fw, fs, fs, al)
        return [kernels.fragment_gather(t["v"], *args, mean=synth.KVQ_MEAN, std=synth.KVQ_STD), kernels.fragment_gather(t["vf"], *args)]
    check(inputs, call)


# ------------------------------------------------------------------------------------------------------------ conv stacks
CONVS = [((1, 4, 7, 7, 8), 8, (1, 1, 1), (1, 1, 1), (0, 0, 0)), ((1, 6, 9, 9, 8), 16, (3, 3, 3), (1, 1, 1), (1, 1, 1)),
         ((2, 1, 29, 31, 128), 136, (1, 3, 3), (1, 2, 2), (0, 1, 1))]


@pytest.mark.parametrize("shape,Cout,k,stride,pad", CONVS, ids=["1x1-C8", "3x3x3-C8", "3x3-s2-C128"])
def test_conv_implicit_and_im2col(shape, Cout, k, stride, pad, half):
    g = gen(sum(shape) + Cout)
    B, D, H, W, Cc = shape
    K = k[0] * k[1] * k[2] * Cc
    kpad = -(-K // 32) * 32
    wk = torch.zeros(Cout, kpad)
    wk[:, :K] = f32(g, Cout, K, sc=K ** -0.5)
    Do, Ho, Wo = kernels.conv_out_dims((D, H, W), k, stride, pad)
    M = B * Do * Ho * Wo
    inputs = dict(x=f32(g, *shape).to(half), w=wk.to(half), b=f32(g, Cout), r=f32(g, M, Cout))

    def call(t):
        cols, _ = kernels.im2col_nd(t["x"], (B, Cc, D, H, W), (D * H * W * Cc, 1, H * W * Cc, W * Cc, Cc), k, stride, pad, half, kpad)
        y16, y32 = kernels.conv_implicit(t["x"], t["w"], t["b"], k, stride, pad, True, resid_f32=t["r"], want_f32=True)
        return [cols, y16, y32, kernels.conv_implicit(t["x"], t["w"], t["b"], k, stride, pad, False),
                kernels.conv_implicit(t["x"], t["w"], t["b"], k, stride, pad, False, store_f32=True)]
    check(inputs, call)


@pytest.mark.parametrize("name", [c.name for c in CONV_FORMS if c.code != 1132])
def test_conv_implicit_on_the_big_ring_tiles(name, half):
    """the 128 x 128 and 128 x 64 implicit-GEMM tiles (walked taps, and the tap table: the only form of C % 32 != 0), split-K around
    the 128 x 128 one, and the channel-concatenation store with the other channels keeping the payload"""
    c = BY_NAME[name]
    g = gen(sum(c.shape) + c.Cout)
    N, M, Cc = c.Cout, conv_rows(c), c.shape[-1]
    K = c.kernel[0] * c.kernel[1] * c.kernel[2] * Cc
    wk = torch.zeros(N, c.Kpad)
    wk[:, :K] = f32(g, N, K, sc=K ** -0.5)
    ldc, off = N + 24, 8
    inputs = dict(x=f32(g, *c.shape).to(half), w=wk.to(half), b=f32(g, N), r=f32(g, M, N), o=Out(M, ldc, dtype=half))
    cols = np.ones(ldc, bool)
    cols[off:off + N] = False
    k, s1, pad = c.kernel, (1, 1, 1), c.pad

    def call(t):
        y16, y32 = kernels.conv_implicit(t["x"], t["w"], t["b"], k, s1, pad, True, resid_f32=t["r"], want_f32=True)
        kernels.conv_implicit(t["x"], t["w"], t["b"], k, s1, pad, True, out=t["o"], ldc=ldc, col_off=off)
        outs = [t["o"], y16, y32, kernels.conv_implicit(t["x"], t["w"], t["b"], k, s1, pad, False, store_f32=True)]
        if Cc % 32 == 0:
            kernels.TAP_TABLE = True
            try:
                outs.append(kernels.conv_implicit(t["x"], t["w"], t["b"], k, s1, pad, True))
            finally:
                kernels.TAP_TABLE = False
        return outs
    with form(c):
        check(inputs, call, [Keep(0, row_mask((M, ldc), 1, cols))])


@pytest.mark.parametrize("C", [40, 6])
def test_pool_nd(C, half):
    g = gen(40 + C)
    check(dict(x=f32(g, 3, 2, 9, 11, C).to(half)),
          lambda t: [kernels.pool_nd(t["x"], (1, 3, 3), (1, 2, 2), (0, 1, 1), True), kernels.pool_nd(t["x"], (2, 3, 3), (1, 2, 2), (0, 0, 0), False),
                     kernels.pool_nd(t["x"], (2, 9, 11), (1, 1, 1), (0, 0, 0), False)])


def test_pack_channels_last8(half):
    b, c, T, h, w = 2, 3, 3, 10, 13
    check(dict(x=f32(gen(8), b, c, T, h, w)),
          lambda t: kernels.pack_channels_last8(t["x"], (b, T, c, h, w), (c * T * h * w, h * w, T * h * w, w, 1), half))


@pytest.mark.parametrize("rows,HW,C", [(3, 300, 40), (1, 1500, 20), (2, 196, 128)])
def test_mean_std_pool_changes_its_two_column_ranges_only(rows, HW, C, half):
    g = gen(rows + HW + C)
    width, mo, so = 2 * C + 7, 1, C + 4
    cols = np.ones(width, bool)
    cols[mo:mo + C] = False
    cols[so:so + C] = False
    inputs = dict(x=f32(g, rows, HW, C, sc=2, off=0.5).to(half), out=Out(rows, width, dtype=torch.float32))
    check(inputs, lambda t: kernels.mean_std_pool(t["x"], t["out"], mo, so), [Keep(0, row_mask((rows, width), 1, cols))])


def test_slow_bottleneck_leaves_the_other_channels_alone(half):
    from kvq_amd.models.backbones.slowfast_model import pack_slow_bottleneck
    cin, ci, cout, out_c = 256, 64, 256, 320
    B, T, H, W = 2, 3, 17, 30
    g = gen(sum((B, T, H, W)) + out_c)
    wgt = lambda r, k: f32(g, r, k, sc=(2.0 / k) ** 0.5).to(half).to(DEV)      # noqa: E731
    pack = pack_slow_bottleneck(wgt(ci, cin), f32(g, ci, sc=0.2).to(DEV), wgt(ci, 9 * ci), f32(g, ci, sc=0.2).to(DEV), wgt(cout, ci),
                                f32(g, cout, sc=0.2).to(DEV))
    inputs = dict(x=f32(g, B, T, H, W, cin).to(half), pack=pack, out=Out(B, T, H, W, out_c, dtype=half))
    check(inputs, lambda t: [kernels.slow_bottleneck(t["x"], t["pack"], ci, cout, out=t["out"]), kernels.slow_bottleneck(t["x"], t["pack"], ci, cout)],
          [Keep(0, row_mask((B, T, H, W, out_c), 4, np.arange(out_c) >= cout))])


@pytest.mark.parametrize("cin,ci,cout,proj,stride", [(8, 8, 32, True, 1), (32, 8, 32, False, 1), (32, 16, 64, True, 2)])
def test_fast_bottleneck(cin, ci, cout, proj, stride, half):
    from kvq_amd.models.backbones.slowfast_model import pack_fast_bottleneck
    g = gen(cin * 1000 + ci)
    B, T, H, W = 2, 5, 17, 30

    def wgt(rows, k):
        w = torch.zeros(rows, -(-k // 32) * 32)
        w[:, :k] = f32(g, rows, k, sc=(2.0 / k) ** 0.5)
        return w.to(half).to(DEV)
    bias = lambda n: f32(g, n, sc=0.2).to(DEV)      # noqa: E731
    ws, bs = (wgt(cout, cin), bias(cout)) if proj else (None, None)
    pack = pack_fast_bottleneck(wgt(ci, 3 * cin), bias(ci), wgt(ci, 9 * ci), bias(ci), wgt(cout, ci), bias(cout), cin, ws, bs, stride=stride)
    check(dict(x=f32(g, B, T, H, W, cin).to(half), pack=pack), lambda t: kernels.fast_bottleneck(t["x"], t["pack"], ci, cout, proj, stride))


def _stem_weight(g, cout, cin, kernel):
    K = kernel[0] * kernel[1] * kernel[2] * cin
    w5 = f32(g, cout, cin, *kernel, sc=K ** -0.5)
    return w5.permute(2, 3, 4, 1, 0).reshape(K, cout).contiguous()


@pytest.mark.parametrize("shape,kernel,stride,pad,cout", [((1, 3, 3, 12, 18), (1, 7, 7), (1, 2, 2), (0, 3, 3), 16),
                                                          ((2, 3, 6, 30, 46), (5, 7, 7), (1, 2, 2), (2, 3, 3), 8)], ids=["cout16", "fast-stem"])
def test_conv_stem_direct(shape, kernel, stride, pad, cout, half):
    g = gen(sum(shape) + cout)
    inputs = dict(x=f32(g, *shape), w=_stem_weight(g, cout, shape[1], kernel), b=f32(g, cout))
    check(inputs, lambda t: kernels.conv_stem_direct(t["x"], t["w"], t["b"], kernel, stride, pad, True, half))


@pytest.mark.parametrize("shape,kernel,stride,pad", [((1, 2, 3, 9, 16), (3, 3, 7), (2, 1, 2), (1, 1, 3)),
                                                     ((2, 3, 6, 30, 46), (5, 7, 7), (1, 2, 2), (2, 3, 3))], ids=["two-channels", "fast-stem"])
def test_conv_stem_mfma(shape, kernel, stride, pad, half):
    g = gen(sum(shape))
    wp = kernels.stem_mfma_pack_weight(_stem_weight(g, 8, shape[1], kernel).to(DEV), kernel, shape[1], half)
    check(dict(x=f32(g, *shape), wp=wp, b=f32(g, 8)), lambda t: kernels.conv_stem_mfma(t["x"], t["wp"], t["b"], kernel, stride, pad, True))


@pytest.mark.parametrize("shape,kd", [((1, 3, 4, 21, 20), 1), ((2, 3, 6, 30, 48), 5)], ids=["odd-H-kd1", "ragged-tile-kd5"])
def test_conv_stem_pool(shape, kd, half):
    g = gen(sum(shape) + kd)
    wp = kernels.stem_mfma_pack_weight(_stem_weight(g, 8, 3, (kd, 7, 7)).to(DEV), (kd, 7, 7), 3, half)
    check(dict(x=f32(g, *shape), wp=wp, b=f32(g, 8)), lambda t: kernels.conv_stem_pool(t["x"], t["wp"], t["b"], kd, True))


@pytest.mark.parametrize("shape,t_index,coff", [((1, 3, 2, 21, 20), None, 0), ((1, 3, 4, 50, 220), [3, 0], 16), ((2, 3, 8, 30, 48), [0, 2, 5, 7], 0)],
                         ids=["odd-H-all-frames", "channel-slice", "ragged-tile"])
def test_conv_stem64_pool_leaves_the_other_channels_alone(shape, t_index, coff, half):
    g = gen(sum(shape))
    w5 = f32(g, 64, 3, 1, 7, 7, sc=147 ** -0.5)
    wimg = kernels.stem64_pack_weight(w5.permute(0, 2, 3, 4, 1).reshape(64, 147).contiguous().to(DEV), half)
    B, _, T, H, W = shape
    F_ = T if t_index is None else len(t_index)
    hp, wp_ = ((H - 1) // 2 + 1 - 1) // 2 + 1, ((W - 1) // 2 + 1 - 1) // 2 + 1
    inputs = dict(x=f32(g, *shape), wimg=wimg, b=f32(g, 64))
    if coff:
        inputs["out"] = Out(B, F_, hp, wp_, 96, dtype=half)
        ch = np.ones(96, bool)
        ch[coff:coff + 64] = False
        check(inputs, lambda t: kernels.conv_stem64_pool(t["x"], t_index, t["wimg"], t["b"], True, out=t["out"], out_coff=coff),
              [Keep(0, row_mask((B, F_, hp, wp_, 96), 4, ch))])
    else:
        check(inputs, lambda t: kernels.conv_stem64_pool(t["x"], t_index, t["wimg"], t["b"], True))


# --------------------------------------------------------------------------------------------------------------- ConvNeXt
@pytest.mark.parametrize("kt", [1, 3])
@pytest.mark.parametrize("shape", [(2, 1, 2, 3), (1, 1, 1, 1), (2, 3, 9, 11)], ids=["2x1x2x3", "1x1x1x1", "2x3x9x11"])
def test_dwconv3d_ln(shape, kt, half):
    Cc = 96
    assert kernels.dwconv3d_ln_supported(Cc, kt, *shape[1:])
    g = gen(Cc + kt + sum(shape))
    inputs = dict(x=f32(g, *shape, Cc), w=f32(g, kt * 49, Cc, sc=0.1), b=f32(g, Cc, sc=0.2), lw=f32(g, Cc, sc=0.2, off=1), lb=f32(g, Cc, sc=0.2))
    check(inputs, lambda t: [kernels.dwconv3d_ln(t["x"], t["w"], t["b"], t["lw"], t["lb"], eps=1e-6, out_dtype=dt) for dt in (half, torch.float32)])


@pytest.mark.parametrize("over", ["th", "thw"])
@pytest.mark.parametrize("N,shape", [(384, (2, 3, 5, 7)), (3072, (2, 2, 9, 11)), (384, (1, 1, 1, 1))], ids=["N384", "N3072", "one-token"])
def test_grn_in_place_and_out_of_place(N, shape, over, half):
    assert kernels.grn_supported(N, *shape[1:])
    g = gen(N + sum(shape))
    rows = shape[0] * shape[1] * shape[2] * shape[3]
    inputs = dict(x=f32(g, rows, N).to(half), x2=f32(g, rows, N).to(half), ga=f32(g, N, sc=0.3), be=f32(g, N, sc=0.3), out=Out(rows, N, dtype=half))
    check(inputs, lambda t: [kernels.grn(t["x"], shape, t["ga"], t["be"], over=over), kernels.grn(t["x2"], shape, t["ga"], t["be"], over=over, out=t["out"]),
                             t["x2"]])


# --------------------------------------------------------------------------------------------------- small ViT / CDM kernels
@pytest.mark.parametrize("B,L,heads", [(1, 7, 2), (2, 197, 2)])
def test_mha_small(B, L, heads, half):
    g = gen(B * 1000 + L)
    check(dict(qkv=f32(g, B * L, 3 * heads * 64, sc=0.7).to(half)), lambda t: kernels.mha_small(t["qkv"], B, L, heads))


@pytest.mark.parametrize("B,Lq,Lk,heads", [(2, 100, 7, 3), (1, 64, 320, 1), (2, 50, 3, 2), (1, 130, 9, 1)])
def test_mha_cross_on_the_interleaved_kv_buffer(B, Lq, Lk, heads, half):
    g = gen(Lq * 100 + Lk)
    D = heads * 64
    inputs = dict(q=f32(g, B * Lq, D).to(half), kv=f32(g, B * Lk, 2 * D + 8).to(half))

    def call(t):
        t["kv"][:, 2 * D:] = float("nan")                     # the 8 spare columns belong to no row of k or v
        return kernels.mha_cross(t["q"], t["kv"][:, :D], t["kv"][:, D:2 * D], B, heads, 0.05)
    check(inputs, call)


def test_vit_embed_ln_cosine_cls_gather_and_mix(half):
    g = gen(5)
    B, G, D = 3, 49, 768
    inputs = dict(tok=f32(g, B * G, D), cls=f32(g, D), pos=f32(g, G + 1, D), lw=f32(g, D, sc=0.1, off=1), lb=f32(g, D, sc=0.1),
                  x=f32(g, B, G + 1, D), a=f32(g, B, D).to(half))
    rows = np.arange(G + 1) >= 1

    def call(t):
        return [kernels.vit_embed_ln(t["tok"], t["cls"], t["pos"], t["lw"], t["lb"], B), kernels.cosine_cls(t["x"]), kernels.cls_gather(t["x"], half),
                kernels.cls_mix(t["x"], t["a"], 0.5)]
    check(inputs, call, [Keep(3, row_mask((B, G + 1, D), 1, rows), like="x")])


@pytest.mark.parametrize("n", list(range(1, 10)) + [1027])
def test_convert(n, half):
    g = gen(n)
    check(dict(x=f32(g, n, sc=3.0), h=f32(g, n, sc=3.0).to(half)), lambda t: [kernels.to_half(t["x"], half), kernels.to_float(t["h"])])


@pytest.mark.parametrize("M,C", [(1, 64), (98, 768), (5, 100)])
def test_modulate_normalize_axpby(M, C, half):
    g = gen(M + C)
    B, rows = 2, 3
    inputs = dict(x=f32(g, M, C), inp=f32(g, M, C), wg=f32(g, C, sc=C ** -0.5), wb=f32(g, C, sc=C ** -0.5), d_in=f32(g, B, rows, C),
                  gl=f32(g, B, C, sc=2.0).to(half), beta=f32(g, B, C).to(half))

    def call(t):
        return [kernels.sem_modulate(t["x"], t["inp"], t["wg"], 0.3, t["wb"], -0.2), kernels.dist_modulate(t["d_in"], t["gl"], t["beta"]),
                kernels.l2_normalize_rows(t["x"], half), kernels.axpby(t["x"], t["inp"], 0.2, 0.8)]
    check(inputs, call)


def test_crop_regions_both_paths_and_qrs_top_region():
    g = gen(3)
    inputs = dict(score=f32(g, 8, 7, 7))
    for tag, (anchor, grid, k) in (("s", (6, 5, 3)), ("v", (32, 4, 2))):
        nx = grid - k + 1
        inputs["x" + tag] = f32(g, 2, 3, 4, grid * anchor, grid * anchor)
        inputs["r" + tag] = i32(g.integers(0, nx * nx, size=8))

    def call(t):
        return [kernels.crop_regions(t["xs"], t["rs"], 6, 3, 3), kernels.crop_regions(t["xv"], t["rv"], 32, 2, 2),
                kernels.qrs_top_region(t["score"], 9, 9, 7, 7), kernels.qrs_top_region(t["score"], 7, 7, 5, 5)]
    check(inputs, call)


# ------------------------------------------------------------------------------------------------------ heads and resizers
@pytest.mark.parametrize("shape,hidden", [((3, 768, 4, 7, 7), 64), ((2, 1024, 1, 5, 5), 64), ((1, 768, 2, 3, 3), 32), ((2, 96, 2, 4, 4), 64)])
def test_vqa_head_both_layouts(shape, hidden):
    g = gen(77 + shape[1])
    B, Cc, D, H, W = shape
    w1 = f32(g, hidden, Cc, sc=Cc ** -0.5)
    inputs = dict(cf=f32(g, *shape), cl=f32(g, B, D, H, W, Cc), w1=w1, w1t=w1.t().contiguous(), b1=f32(g, hidden, sc=0.1), w2=f32(g, hidden, sc=0.2),
                  b2=f32(g, 1))

    def call(t):
        args = (t["w1"], t["b1"], t["w2"], t["b2"], t["w1t"])
        s, tok_map, depth = kernels.vqa_head(t["cl"].permute(0, 4, 1, 2, 3), *args, return_map=True)
        return [kernels.vqa_head(t["cf"], *args), kernels.vqa_head(t["cl"].permute(0, 4, 1, 2, 3), *args), s, tok_map, depth]
    check(inputs, call)


@pytest.mark.parametrize("K,pool", [(1, True), (3, False), (5, True)])
def test_vqa_head_classes(K, pool):
    g = gen(77 + K)
    B, Cc, D, H, W, hidden = 3, 768, 4, 7, 7, 64
    inputs = dict(cf=f32(g, B, Cc, D, H, W), cl=f32(g, B, D, H, W, Cc), w1=f32(g, hidden, Cc, sc=Cc ** -0.5), b1=f32(g, hidden, sc=0.1),
                  w2=f32(g, K, hidden, sc=0.2), b2=f32(g, K))
    check(inputs, lambda t: [kernels.vqa_head_classes(t["cf"], t["w1"], t["b1"], t["w2"], t["b2"], pre_pool=pool),
                             kernels.vqa_head_classes(t["cl"].permute(0, 4, 1, 2, 3), t["w1"], t["b1"], t["w2"], t["b2"], pre_pool=pool)])


def test_simple_vqa_head():
    g = gen(78)
    Cin, hid = 9472, 128
    inputs = dict(feat=f32(g, 2, 8, Cin), w1=f32(g, hid, Cin, sc=Cin ** -0.5), b1=f32(g, hid, sc=0.1), w2=f32(g, hid, sc=0.2), b2=f32(g, 1))
    check(inputs, lambda t: kernels.simple_vqa_head(t["feat"], t["w1"], t["b1"], t["w2"], t["b2"]))


def test_headtrain_step_on_fixture_case_a(golden):
    """forward -> loss -> backward -> AdamW with ``ema=None``: the workspace, the gradient and the three optimiser vectors are
    guarded; nothing else is written"""
    from test_gpu_headtrain import case
    import headtrain_ref as R
    c = case(golden, "a")
    n = kernels.headtrain_param_count(c.C)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))      # noqa: E731
    inputs = dict(x=f(c.x), prm=f(c.prm), y=f(c.y), m=torch.zeros(n), v=torch.zeros(n), p2=f(c.prm))

    def call(t):
        ws = kernels.headtrain_workspace(c.B, c.L, c.C)
        score = kernels.headtrain_forward(t["x"], t["prm"], c.p, c.seed, 0, ws)
        out3, dscore = kernels.headtrain_loss(score, t["y"], c.rw)
        grads = kernels.headtrain_backward(t["x"], t["prm"], c.p, c.seed, 0, ws, dscore)
        kernels.headtrain_adamw(t["p2"], grads, t["m"], t["v"], None, c.lr * R.lr_factor(1, c.wu, c.mx), c.wd, 1)
        return [score, out3, dscore, grads, t["p2"], t["m"], t["v"], kernels.headtrain_mask(c.seed, 0, 0, c.p, c.B * c.L * c.C)]
    check(inputs, call)


@pytest.mark.parametrize("antialias", [False, True], ids=["plain", "antialias"])
def test_resize_bilinear(antialias):
    g = gen(64)
    v = g.integers(0, 256, size=(3, 3, 64, 64), dtype=np.uint8)
    inputs = dict(u8=torch.from_numpy(v), f=torch.from_numpy(v.astype(np.float32)))

    def call(t):
        return [kernels.resize_bilinear(t["u8"], 150, 97, antialias=antialias),
                kernels.resize_bilinear(t["f"], 150, 97, crop=(3, 5, 100, 64), mean=synth.KVQ_MEAN, std=synth.KVQ_STD, antialias=antialias),
                kernels.resize_bilinear(t["u8"], 33, 21, antialias=antialias)]
    check(inputs, call)


def test_upsample_frames():
    g = gen(65)
    v = g.integers(0, 256, size=(3, 2, 37, 53), dtype=np.uint8)
    check(dict(u8=torch.from_numpy(v), f=torch.from_numpy(v.astype(np.float32))),
          lambda t: [kernels.upsample_frames(t["u8"], 1.7), kernels.upsample_frames(t["f"], 1.7)])


@pytest.mark.parametrize("cell", [8, 1])
def test_quality_paint(cell):
    T, Hs, Ws, D, Hf, Wf = 2, 37, 41, 1, 8, 8
    inputs = _sampler_inputs(66, T, Hs, Ws, 1, 32, 2)
    inputs["tok"] = f32(gen(67), 1, D, Hf, Wf)

    def call(t):
        src = kernels.FragmentSource([t["video"]], [t["hoff"]], [t["woff"]], 1, 1, 32, 32, 2)
        assert kernels.quality_paint_supported(src, (D, Hf, Wf), cell)
        return kernels.quality_paint(src, t["tok"], cell=cell, overlay_depths=(0,), value_range=(-1.0, 1.0))
    check(inputs, call)
