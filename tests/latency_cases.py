"""The cases of the KVQ_LATENCY=1 run: tests/latency_mode_child.py executes them, in this order, in a fresh interpreter that has the
switch set, and saves what they compute; tests/test_gpu_latency_mode.py rebuilds the same inputs (builders take a seed and return CPU
tensors, so both processes hold the same bits), runs the same launches in the default mode and does every comparison.

What the mode changes (csrc/common.cpp: latency_mode) and which cases reach it:
  * window_attention32 splits a (window, head) unit's q-blocks over qsplit = min(4, 768 / (BW nH), ceil(N / 32)) workgroups; part p
    takes q-blocks [p nqb / qsplit, (p + 1) nqb / qsplit)                                                               -> ``Attn``
  * the C = 384 / 512 tails take the HC = 256 forms (block_tailmm_kernel<E, 0 | 1 | 2, 3 | 4, 256>)                     -> ``Tail``, ``TailF16``
  * C = 768 has no fused tail: stage 3 runs proj / norm2 / fc1 / fc2 as launches of their own                           -> ``Trunk``
  * all of them inside guard bands (tests/guarded.py)                                                                  -> ``Bounds``
This is not a test module and holds no assertion on results: ``execute`` computes and saves."""
import json
import os

import numpy as np
import torch

import kvq_amd  # noqa: F401
import test_gpu_attn_ranges as TR
import test_gpu_bounds as TB
import test_gpu_kernels as TK
from kvq_amd import _abi, kernels
from oracle import swin3d_oracle as O

DEV = "cuda:0"
HALVES = {"fp16": torch.float16, "bf16": torch.bfloat16}
WIN = (8, 7, 7)
SENTINEL = 7.0
MODE_PROBES = [("kvq_block_tail_supported", 768, 3072), ("kvq_block_tail_supported", 384, 1536), ("kvq_block_tail_pack_bytes", 768, 3072)]


def mode_probe():
    """[supported(768), supported(384), pack_bytes(768)]: host entry points only; 0 / 1 / 0 in latency mode, 1 / 1 / > 0 otherwise"""
    return [int(getattr(_abi.lib(), name)(C, hidden)) for name, C, hidden in MODE_PROBES]


def save(path, outs):
    """tensors -> one .npz; the 16-bit floats as their bits (numpy has no bfloat16)"""
    arrs = {}
    for k, t in outs.items():
        t = t.detach().cpu().contiguous()
        if t.dtype in (torch.float16, torch.bfloat16):
            arrs[f"{k}|{str(t.dtype).replace('torch.', '')}"] = t.view(torch.int16).numpy()
        else:
            arrs[f"{k}|"] = t.numpy()
    np.savez(path, **arrs)


def load(path):
    out = {}
    with np.load(path, allow_pickle=False) as z:
        for key in z.files:
            k, tag = key.split("|")
            t = torch.from_numpy(z[key])
            out[k] = t.view(getattr(torch, tag)) if tag else t
    return out


def _dev(inp):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in inp.items()}


class Case:
    """``name`` = the manifest entry and the stem of the file(s) ``execute`` writes into ``outdir``"""
    kind = ""

    def __init__(self, name, half):
        self.name, self.half = f"{name}-{half}", HALVES[half]

    def execute(self, outdir):
        save(os.path.join(outdir, self.name + ".npz"), self.run(self.inputs()))

    def __repr__(self):
        return self.name


# ------------------------------------------------------------------------------------------------------------------------- attention
class Attn(Case):
    """kvq_window_attention32 / _ranges, non-fused.  ``how``: plain | pad_mask | tile_skip | dsplit | ranges | extremes.
    ``inputs`` -> CPU tensors (qkv in the launch's dtype and row order); ``oracle`` -> (image-bias oracle, exact-bias oracle) on those rows."""
    kind = "attn"

    def __init__(self, name, half, dims, window, shifted, gated, nH, B, how="plain", seed=0):
        super().__init__(name, half)
        self.dims, self.window, self.gated, self.nH, self.B, self.how, self.seed = dims, window, gated, nH, B, how, seed
        self.shift = tuple(w // 2 for w in window) if shifted else (0, 0, 0)

    def inputs(self):
        half = self.half
        if self.how == "ranges":
            return self._ranges_inputs()
        if self.how == "extremes":
            q2, k, v, rpb, window, lay = TK._extremes_inputs(half)
            tok, self.center = TK._tok_table(lay, window)
            self.lay = lay
            return dict(qkv=torch.stack([q2, k, v]).permute(0, 2, 1, 3, 4).reshape(3, self.nH, lay["nW"] * lay["N"], 32).contiguous().to(half),
                        tok=TB.i32(tok), rpb=rpb)
        inp, self.lay, self.center = TB._attn_inputs(self.seed, self.dims, self.window, self.shift, self.nH, self.B, half, gated=self.gated,
                                                     q_scale=0.6 * kernels.LOG2E)
        N, nW = self.lay["N"], self.lay["nW"]
        if self.how == "tile_skip":                       # the mask of test_window_attention32_vs_oracle_and_gather_path, from a generator of its own
            inp["skip"] = TB.i32(TK._tile_skip_mask(TB.gen(self.seed + 1), nW, N))
        if self.how == "pad_mask":                        # as test_window_attention32_writes_padding_rows_itself
            pad = self.lay["src"].reshape(nW, N) < 0
            assert pad.any() and not pad.all(1).any()
            rows = torch.from_numpy(np.tile(pad.reshape(-1), self.B))
            C = 32 * self.nH
            bq = TB.f32(TB.gen(self.seed + 1), 3 * C, sc=0.4)
            filled = inp["qkv"].clone()                   # what the oracle sees: k | v of a padding row = the rounded bias, its q = 0
            for which in (1, 2):
                filled[which][:, rows] = bq[which * C:(which + 1) * C].reshape(self.nH, 1, 32).to(half)
            filled[0][:, rows] = 0
            mask = TK._pad_mask_words(pad)
            inp["qkv"][:, :, rows] = float("nan")         # rows the launch must not read
            inp.update(filled=filled, bq=bq, mask=torch.from_numpy(mask.view(np.int32)), keep=~rows)
        return inp

    def _ranges_inputs(self):                             # as test_ranges_launch_vs_oracle_and_full_launch
        half, dims, window, nH = self.half, self.dims, self.window, self.nH
        self.lay, tok_o, self.order, ranges, self.center = TR.region_ordered(dims, window, self.shift)
        N, BW = self.lay["N"], self.lay["nW"]
        q2, k, v, rpb, fpb = TR.ranges_operands(dims, window, self.lay, nH, half)
        qo, ko, vo = (TR.to_order(t, self.order, BW, N) for t in (q2, k, v))
        return dict(qkv=torch.stack([qo, ko, vo]).permute(0, 2, 1, 3, 4).reshape(3, nH, BW * N, 32).contiguous().to(half), tok=TB.i32(tok_o),
                    rpb=rpb, fpb=fpb, ranges=torch.from_numpy(np.ascontiguousarray(ranges)), raster=torch.stack([q2, k, v]))

    def qsplit(self):
        """(qsplit, the first q-block of every part and nqb) of this case's launch in latency mode (csrc/attn32.hip)"""
        N, units = self.lay["N"], self.B * self.lay["nW"] * self.nH
        nqb = -(-N // 32)
        qs = min(4, max(1, 768 // units), nqb)
        return qs, [p * nqb // qs for p in range(qs + 1)]

    def run(self, inp):
        t = _dev({k: v for k, v in inp.items() if k not in ("filled", "keep", "raster")})
        N, nW = self.lay["N"], self.lay["nW"]
        use_mask = any(s > 0 for s in self.lay["ss"])
        image = kernels.attn_bias32(t["tok"], t["rpb"], t.get("fpb"), self.center, nW, N, use_mask)
        kw = {}
        if self.how == "pad_mask":
            kw = dict(b_qkv=t["bq"], pad_mask=t["mask"])
        if self.how == "dsplit":
            kw = dict(dsplit_from=nW - nW // 2)
        if self.how == "ranges":
            kw = dict(ranges=t["ranges"])
        outs = dict(out=kernels.window_attention32(t["qkv"], image, nW, N, **kw))
        if self.how == "tile_skip":
            sentinel = torch.full((self.B * nW * N, self.nH * 32), SENTINEL, dtype=self.half, device=DEV)
            outs["part"] = kernels.window_attention32(t["qkv"], image, nW, N, tile_skip=t["skip"], out=sentinel)
        return outs

    def oracle(self, inp):
        N, nW, nH = self.lay["N"], self.lay["nW"], self.nH
        if self.how == "ranges":
            q2, k, v = inp["raster"]
            BW = nW
            return tuple(TR.to_order(O.attention_core(q2 / kernels.LOG2E, k, v, inp["rpb"], inp["fpb"], self.window, self.lay, image=im),
                                     self.order, BW, N).reshape(BW * N, nH * 32) for im in (True, False))
        qkv = inp["filled" if self.how == "pad_mask" else "qkv"].float()
        BW = qkv.shape[2] // N
        q2, k, v = qkv.reshape(3, nH, BW, N, 32).permute(0, 2, 1, 3, 4)
        return tuple(O.attention_core(q2 / kernels.LOG2E, k, v, inp["rpb"], inp.get("fpb"), self.window, self.lay, image=im).reshape(BW * N, nH * 32)
                     for im in (True, False))

    def skipped_rows(self, inp):
        """bool [BW * N]: rows of q-blocks whose two 16-row tiles are both marked in tile_skip"""
        N, nW = self.lay["N"], self.lay["nW"]
        return TK._tile_skipped_rows(inp["skip"].numpy(), self.B * nW, nW, N)


def attention_cases(half):
    A = lambda *a, **k: Attn(a[0], half, *a[1:], **k)      # noqa: E731
    return [
        # N = 392, nqb = 13; 12 units: qsplit 4, parts start at q-blocks 0 / 3 / 6 / 9 (3 / 3 / 3 / 4 blocks); the last block has 8 valid rows
        A("attn-81414-B1", (8, 14, 14), WIN, True, True, 3, 1, seed=401),
        # the same, 96 units: still qsplit 4, 384 workgroups (more than one round over the XCDs)
        A("attn-81414-B8", (8, 14, 14), WIN, True, True, 3, 8, seed=402),
        # stage-1 like, 32 windows x 6 heads: 192 units -> qsplit 4 (0 / 3 / 6 / 9); 384 units -> qsplit 2 (0 / 6): several entries per workgroup slot
        A("attn-162828-B1", (16, 28, 28), WIN, True, True, 6, 1, seed=403),
        A("attn-162828-B2", (16, 28, 28), WIN, True, True, 6, 2, seed=404),
        # N = 196 (clamped depth, padded partition), nqb = 7; 8 units: qsplit 4, parts start at 0 / 1 / 3 / 5 (1 / 2 / 2 / 2 blocks)
        A("attn-4109-padmask", (4, 10, 9), WIN, True, True, 1, 2, how="pad_mask", seed=405),
        A("attn-4109-tileskip", (4, 10, 9), WIN, True, True, 1, 2, how="tile_skip", seed=406),
        # N = 64, nqb = 2; 32 units: qsplit clamped to 2, one q-block per part
        A("attn-888-w444", (8, 8, 8), (4, 4, 4), True, False, 2, 2, seed=407),
        # N = 98 (window clamped to (2,7,7)), nqb = 4; 24 units: qsplit 4, one q-block per part, the last with 2 valid rows
        A("attn-21414-N98", (2, 14, 14), WIN, True, True, 3, 2, seed=408),
        # depth split, 48 units: qsplit 4 (0 / 3 / 6 / 9): q-block 6, which sees both halves, is the first block of part 2
        A("attn-161414-dsplit", (16, 14, 14), WIN, True, True, 3, 2, how="dsplit", seed=409),
        # the ranges launch on the geometries of tests/test_gpu_attn_ranges.py, BW = 8, nH = 2, 16 units: w877 nqb = 13, qsplit 4 (0 / 3 / 6 / 9),
        # bodies of 7 and 13; w222 N = 8, one q-block, qsplit 1; w477 N = 196, nqb = 7, qsplit 4 (0 / 1 / 3 / 5), bodies of 4 and 7
        A("attn-ranges-w877", *TR.GEOMETRIES[0][:2], True, True, 2, 1, how="ranges"),
        A("attn-ranges-w222", *TR.GEOMETRIES[1][:2], True, True, 2, 1, how="ranges"),
        A("attn-ranges-w477", *TR.GEOMETRIES[2][:2], True, True, 2, 1, how="ranges"),
        # rows that start masked, a key in block 9 that dominates; 16 units: qsplit 4 — part 3 begins at q-block 9 with an empty running state
        A("attn-extremes", (16, 14, 14), WIN, True, False, 2, 1, how="extremes"),
    ]


# ----------------------------------------------------------------------------------------------------------------------------- tails
def tail_reference64(A, x, wts, half, lay, B, dims):
    """test_gpu_kernels._tail_reference evaluated in float64: the same composition, the same two 16-bit rounding points"""
    Wp, bp, g2, b2n, W1, b1, W2, b2 = (w.double() for w in wts)
    A, x = A.double(), x.double()
    y = A @ Wp.t() + bp
    if lay is not None:
        D, H, W = dims
        L, C = D * H * W, x.shape[1]
        y = O.scatter_windows(y.reshape(B, -1, C), lay, B, D, H, W).reshape(B * L, C)
    x1 = x + y
    h = torch.nn.functional.layer_norm(x1, (x.shape[1],), g2, b2n).to(half).double()
    hid = torch.nn.functional.gelu(h @ W1.t() + b1).to(half).double()
    return x1 + hid @ W2.t() + b2


WEIGHT_KEYS = ("Wp", "bp", "g2", "b2n", "W1", "b1", "W2", "b2")      # the order of test_gpu_kernels._tail_draws / _tail_reference


class Tail(Case):
    """kernels.block_tail at C = 384 / 512 on the fp32 stream, inputs drawn by test_gpu_kernels._tail_draws as test_block_tail draws them.
    ``emit``: None (MODE 0) | "norm" (MODE 1) | "qkv" (MODE 2, through block_tail_qkv_pack); ``gather``: the padded partition is run
    with scatter_map and again with attn_gather (the token-walking launch)."""
    kind = "tail"

    def __init__(self, name, half, C, dims, shift, nxt, emit=None, gather=False, B=2):
        super().__init__(name, half)
        self.C, self.dims, self.shift, self.nxt, self.emit, self.gather, self.B = C, dims, shift, nxt, emit, gather, B
        assert (emit is None) == (nxt is None)

    def inputs(self):
        half, C, (D, H, W), B = self.half, self.C, self.dims, self.B
        g = TK.rng(C + D + H + W + (5 if self.emit == "qkv" else 0))
        self.lay = lay = O.window_layout(D, H, W, WIN, self.shift)
        self.Lp, self.L = Lp, L = lay["nW"] * lay["N"], D * H * W
        t, A, x, wts = TK._tail_draws(g, C, B * Lp, B * L, half)
        inp = dict(zip(WEIGHT_KEYS, wts), A=A, x=x)
        src = lay["src"].astype(np.int64)
        inp["src"] = TB.i32(src)
        if self.gather:
            assert Lp != L
            inv = np.zeros(L, np.int32)
            inv[src[src >= 0]] = np.nonzero(src >= 0)[0].astype(np.int32)
            inp["inv"] = TB.i32(inv)
        if self.emit:
            self.lay2 = lay2 = O.window_layout(D, H, W, WIN, self.nxt)
            assert Lp == L
            if self.emit == "qkv":                        # drawn ahead of the next norm1, as test_block_tail_emits_next_qkv draws them
                inp.update(Wq=TK.rnd(t(3 * C, C, sc=0.1), half), bq=t(3 * C, sc=0.3))
            inp.update(gn=1 + 0.2 * t(C), bn=0.2 * t(C), dst=TB.i32(TK._next_dst(lay2, L)))
        return inp

    def weights(self, inp):
        return tuple(inp[k] for k in WEIGHT_KEYS)

    QS = 0.25

    def run(self, inp):
        half, hidden = self.half, 4 * self.C
        t = _dev(inp)
        h = lambda k: t[k].to(half)      # noqa: E731
        pack = kernels.block_tail_pack(h("Wp"), t["bp"], t["g2"], t["b2n"], h("W1"), t["b1"], h("W2"), t["b2"])
        kw = dict(map_rows=self.Lp, out_rows=self.L)
        if self.emit:
            kw.update(next_norm=(t["gn"], t["bn"]), next_dst=t["dst"], next_rows=self.L)
        if self.emit == "qkv":
            qpack = kernels.block_tail_qkv_pack(h("Wq").contiguous(), hidden)
            assert qpack is not None
            kw["next_qkv"] = (qpack, t["bq"], self.QS)
        x = t["x"].clone()
        emitted = kernels.block_tail(h("A"), x, pack, hidden, scatter_map=t["src"], **kw)
        outs = dict(x=x)
        if self.emit:
            outs["emitted"] = emitted
        if self.emit == "qkv":                            # as test_block_tail_emits_next_qkv: the launch without the q | k | v emission, and the
            kw.pop("next_qkv")                            # qkv GEMM launch on the norm1 rows it emits
            x_ln = t["x"].clone()
            ln_rows = kernels.block_tail(h("A"), x_ln, pack, hidden, scatter_map=t["src"], **kw)
            outs.update(x_ln=x_ln, gemm=kernels.gemm(ln_rows, h("Wq").contiguous(), t["bq"], _abi.EPI_QKV_BF16, num_heads=self.C // 32, q_scale=self.QS))
        if self.gather:
            xg = t["x"].clone()
            kernels.block_tail(h("A"), xg, pack, hidden, attn_gather=t["inv"], **kw)
            outs["xg"] = xg
        return outs


class TailF16(Case):
    """C = 384 on the fp16 residual stream: test_block_tail_fp16_residual_stream's inputs (test_gpu_kernels._tail_draws, _fp16_stream: row 0
    holds +-60000) and its two launches — the fp32 stream on the widened input (``x32``), the fp16 stream (``xh``)"""
    kind = "tail16"
    B = 2

    def __init__(self, name, half, C, dims, shift, nxt, qkv):
        super().__init__(name, half)
        self.C, self.dims, self.shift, self.nxt, self.qkv = C, dims, shift, nxt, qkv

    def inputs(self):
        half, C, (D, H, W), B = self.half, self.C, self.dims, self.B
        g = TK.rng(7 * C + D + H + W)
        self.lay = lay = O.window_layout(D, H, W, WIN, self.shift)
        self.Lp, self.L = Lp, L = lay["nW"] * lay["N"], D * H * W
        t, A, x, wts = TK._tail_draws(g, C, B * Lp, B * L, half)
        inp = dict(zip(WEIGHT_KEYS, wts), A=A, x16=TK._fp16_stream(x))
        inp["src"] = TB.i32(lay["src"])
        if self.nxt is not None:
            lay2 = O.window_layout(D, H, W, WIN, self.nxt)
            inp.update(gn=1 + 0.2 * t(C), bn=0.2 * t(C), dst=TB.i32(TK._next_dst(lay2, L)))
            if self.qkv:
                inp.update(Wq=TK.rnd(t(3 * C, C, sc=0.1), half), bq=t(3 * C, sc=0.2))
        return inp

    def weights(self, inp):
        return tuple(inp[k] for k in WEIGHT_KEYS)

    def run(self, inp):
        half, hidden = self.half, 4 * self.C
        t = _dev(inp)
        h = lambda k: t[k].to(half)      # noqa: E731
        pack = kernels.block_tail_pack(h("Wp"), t["bp"], t["g2"], t["b2n"], h("W1"), t["b1"], h("W2"), t["b2"])
        kw = dict(map_rows=self.Lp, out_rows=self.L)
        if self.nxt is not None:
            kw.update(next_norm=(t["gn"], t["bn"]), next_dst=t["dst"], next_rows=self.L)
            if self.qkv:
                kw["next_qkv"] = (kernels.block_tail_qkv_pack(h("Wq").contiguous(), hidden), t["bq"], 0.25)
        x32 = t["x16"].float()
        n32 = kernels.block_tail(h("A"), x32, pack, hidden, scatter_map=t["src"], **kw)
        xh = t["x16"].clone()
        n16 = kernels.block_tail(h("A"), xh, pack, hidden, scatter_map=t["src"], **kw)
        outs = dict(x32=x32, xh=xh)
        if n32 is not None:
            outs.update(n32=n32, n16=n16)
        return outs


def tail_cases(half):
    T = lambda *a, **k: Tail(a[0], half, *a[1:], **k)      # noqa: E731
    return [
        T("tail-c384-81414-norm", 384, (8, 14, 14), (0, 0, 0), (4, 3, 3), emit="norm"),
        T("tail-c384-81414-qkv", 384, (8, 14, 14), (0, 0, 0), (4, 3, 3), emit="qkv"),
        T("tail-c384-877-norm", 384, (8, 7, 7), (0, 0, 0), (0, 0, 0), emit="norm"),
        T("tail-c384-4109-padded", 384, (4, 10, 9), (4, 3, 3), None, gather=True),
        T("tail-c512-8147-norm", 512, (8, 14, 7), (0, 0, 0), (4, 3, 3), emit="norm"),
        T("tail-c512-8147-qkv", 512, (8, 14, 7), (0, 0, 0), (4, 3, 0), emit="qkv"),
        T("tail-c512-4109-padded", 512, (4, 10, 9), (4, 3, 3), None, gather=True),
        # 2 x 105 = 210 rows: three whole 64-token workgroups (MMc<CF, 256>::TOK) and one of 18 tokens
        T("tail-c384-357-ragged", 384, (3, 5, 7), (0, 0, 0), None),
        T("tail-c512-357-ragged", 512, (3, 5, 7), (0, 0, 0), None),
        TailF16("tail16-c384-81414-qkv", half, 384, (8, 14, 14), (0, 0, 0), (4, 3, 3), True),
        TailF16("tail16-c384-877", half, 384, (8, 7, 7), (4, 3, 3), None, False),
    ]


# ---------------------------------------------------------------------------------------------------------------------------- bounds
def _bounds_tail(C, emit):
    return lambda half: TB.guarded_block_tail(C, (8, 14, 7), (0, 0, 0), "scatter", (4, 3, 3) if emit else None, emit, False, half)


class Bounds(Case):
    """One guarded run (tests/test_gpu_bounds.py: ``check`` with its ``Keep`` masks) of a launch the mode changes.  ``execute`` writes the
    outcome as text — "clean", or what ``check`` found, and then raises: nothing is launched after a broken guard."""
    kind = "bounds"

    def __init__(self, name, half, fn):
        super().__init__(name, half)
        self.fn = fn

    def execute(self, outdir):
        text, failure = "clean", None
        try:
            self.fn(self.half)
        except AssertionError as e:
            text, failure = f"{e}" or "assertion failed", e
        with open(os.path.join(outdir, self.name + ".txt"), "w") as f:
            f.write(text)
        if failure is not None:
            raise failure


def bounds_cases(half):
    # every attention case: qsplit 4 (12 / 12 / 16 / 48 / 16 units, nqb = 7 / 7 / 13 / 13 / 13)
    cases = [
        Bounds("bounds-attn-plain", half, lambda h: TB.guarded_attn_bias32_and_window_attention32(*TB.ATTN_GEOMS[0], h)),
        Bounds("bounds-attn-tileskip", half, TB.guarded_window_attention32_tile_skip),      # Keep: the skipped rows
        Bounds("bounds-attn-padmask", half, TB.guarded_window_attention32_pad_mask),       # NaN in the padding rows
        Bounds("bounds-attn-dsplit", half, TB.guarded_window_attention32_depth_split),
        Bounds("bounds-attn-ranges", half, lambda h: TB.guarded_window_attention32_ranges(*TR.GEOMETRIES[0], h)),      # w877: N = 392
    ]
    for C in (384, 512):
        for emit in (None, "norm", "qkv"):
            cases.append(Bounds(f"bounds-tail-c{C}-{emit or 'plain'}", half, _bounds_tail(C, emit)))
    return cases


# ----------------------------------------------------------------------------------------------------------------------------- trunk
TRUNK_GOLDEN = ["t_grpb_stress_8x80", "t_grpb_stress_16x64"]      # the two smallest cases of tests/golden/trunk.npz


class Trunk(Case):
    """VQA_Network forward of a golden case (stage 3 as a GEMM chain, stage 2 through the HC = 256 tails); ``profile``: one more forward
    with the plan's profile records on, saved as <name>.json"""
    kind = "trunk"

    def __init__(self, golden_case, half, profile=False):
        super().__init__("trunk-" + golden_case, half)
        self.golden_case, self.dtype, self.profile = golden_case, half, profile

    def execute(self, outdir):
        import test_gpu_e2e as TE
        from kvq_amd.utils import synth
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trunk.npz"), allow_pickle=False)
        case = self.golden_case
        wseed, cseed, B, T, H, W = (int(v) for v in g[f"{case}/meta"])
        net, key = TE.build_network(str(g[f"{case}/cfg"]), wseed, str(g[f"{case}/scheme"]), self.dtype)
        x = torch.from_numpy(synth.synth_clip(cseed, T, H, W, batch=B)).to(DEV)
        with torch.no_grad():
            score, feats = net(inputs={"technical": x}, reduce_scores=True, return_pooled_feats=True)
            save(os.path.join(outdir, self.name + ".npz"), dict(score=score, feat=feats[key]))
            if self.profile:
                bb, dev = getattr(net, key + "_backbone"), torch.device(DEV)
                bb.profile(B, T, H, W, dev, True)
                bb({"technical": x})
                torch.cuda.synchronize()
                recs = bb.profile_read(B, T, H, W, dev)
                bb.profile(B, T, H, W, dev, False)
                with open(os.path.join(outdir, self.name + ".json"), "w") as f:
                    json.dump([[r["kind"], r["kernel"], r["flops"], r["bytes"]] for r in recs], f)


def trunk_cases(half):
    return [Trunk(c, half, profile=(c == TRUNK_GOLDEN[0])) for c in TRUNK_GOLDEN]


def all_cases():
    """the fixed order of the child's run"""
    out = []
    for half in HALVES:
        out += attention_cases(half) + tail_cases(half) + bounds_cases(half) + trunk_cases(half)
    return out
