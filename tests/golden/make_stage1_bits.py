"""Recorded bits of the stage-1 (C = 192) token-per-lane launches: block tail (csrc/tail.hip) and patch merge (csrc/merge.hip).

    python tests/golden/make_stage1_bits.py [out.npz]        (on the GPU; default tests/golden/stage1_bits.npz)

stage1_bits.npz was written by this script on an MI355X from the build of the commit BEFORE the register-allocation rework of the two
units (the one that removed their scratch spills).  That rework changes no floating-point operation, so every output below must stay
identical to the bit: tests/test_gpu_stage1_registers.py runs the same seeded cases and compares a SHA-256 of each output's raw bytes,
plus the raw rows of the two smallest cases (so a mismatch can be sized, not only detected).  The inputs are numpy PCG64 draws rounded
on the CPU: they do not depend on the GPU or its libraries.
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda:0"
HALVES = {"fp16": torch.float16, "bf16": torch.bfloat16}
WINDOW = (8, 7, 7)
RAW = ("tail192-3x5x7-m0-x16", "merge192-3x5x7-plain-x32-o32")      # cases whose raw output rows are recorded too


def _dev(t, dtype=None):
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def raw_bytes(t):
    """the tensor's storage as a flat uint8 numpy array (bf16 has no numpy dtype: reinterpreted, not converted)"""
    t = t.detach().contiguous().cpu()
    return t.view(torch.uint8).reshape(-1).numpy() if t.dtype != torch.uint8 else t.reshape(-1).numpy()


def digest(t):
    return hashlib.sha256(raw_bytes(t).tobytes()).hexdigest()


def _inverse(src, L):
    dst = np.empty(L, np.int32)
    dst[src] = np.arange(L, dtype=np.int32)
    return dst


def tail_case(C, dims, B, shift, nxt_shift, mode, x16, half, gather=False, seed=0):
    """one kvq_block_tail launch -> {name: tensor}: the residual stream and what MODE 1 / 2 emit"""
    from kvq_amd import kernels
    from oracle import swin3d_oracle as O
    g = np.random.Generator(np.random.PCG64(1000 + seed))
    D, H, W = dims
    hidden = 4 * C
    lay = O.window_layout(D, H, W, WINDOW, shift)
    Lp, L = lay["nW"] * lay["N"], D * H * W
    t = lambda *s, sc=1.0: torch.from_numpy((g.standard_normal(s) * sc).astype(np.float32))      # noqa: E731
    A = t(B * Lp, C)
    x = t(B * L, C, sc=2.0)
    Wp, W1, W2 = t(C, C, sc=0.15), t(hidden, C, sc=0.15), t(C, hidden, sc=0.08)
    bp, b1, b2, g2, b2n = t(C, sc=0.3), t(hidden, sc=0.3), t(C, sc=0.3), 1 + 0.2 * t(C), 0.2 * t(C)
    gn, bn, Wq, bq = 1 + 0.2 * t(C), 0.2 * t(C), t(3 * C, C, sc=0.1), t(3 * C, sc=0.3)
    pack = kernels.block_tail_pack(_dev(Wp, half), _dev(bp), _dev(g2), _dev(b2n), _dev(W1, half), _dev(b1), _dev(W2, half), _dev(b2))
    kw = {}
    if mode:
        lay2 = O.window_layout(D, H, W, WINDOW, nxt_shift)
        assert Lp == L and (lay2["src"] >= 0).all()
        kw = dict(next_norm=(_dev(gn), _dev(bn)), next_dst=_dev(torch.from_numpy(_inverse(lay2["src"], L))), next_rows=L)
        if mode == 2:
            kw["next_qkv"] = (kernels.block_tail_qkv_pack(_dev(Wq, half), hidden), _dev(bq), 0.25)
            assert kw["next_qkv"][0] is not None
    src = lay["src"].astype(np.int64)
    if gather:       # the launch that walks the tokens: attn_gather = the inverse of the scatter map
        inv = np.zeros(L, np.int32)
        inv[src[src >= 0]] = np.nonzero(src >= 0)[0].astype(np.int32)
        kw.update(attn_gather=_dev(torch.from_numpy(inv)))
    else:
        kw.update(scatter_map=_dev(torch.from_numpy(src.astype(np.int32))))
    xd = _dev(x.to(torch.float16) if x16 else x.clone())
    nxt = kernels.block_tail(_dev(A, half), xd, pack, hidden, map_rows=Lp, out_rows=L, **kw)
    out = {"x": xd}
    if mode:
        out["qkv" if mode == 2 else "norm1"] = nxt
    return out


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


def merge_case(C, dims, B, emit, x16, out16, half, seed=0):
    """one kvq_patch_merge launch -> {name: tensor}: the merged stream and, with emit, the next norm1 rows"""
    from kvq_amd import kernels
    from oracle import swin3d_oracle as O
    g = np.random.Generator(np.random.PCG64(2000 + seed))
    D, H, W = dims
    x = torch.from_numpy((g.standard_normal((B * D * H * W, C)) * 1.5 + 0.3 * g.standard_normal((1, C))).astype(np.float32))
    red = torch.from_numpy((g.standard_normal((2 * C, 4 * C)) / np.sqrt(4 * C)).astype(np.float32))
    gm = torch.from_numpy((1 + 0.2 * g.standard_normal(4 * C)).astype(np.float32))
    be = torch.from_numpy((0.2 * g.standard_normal(4 * C)).astype(np.float32))
    gn = torch.from_numpy((1 + 0.2 * g.standard_normal(2 * C)).astype(np.float32))
    bn = torch.from_numpy((0.2 * g.standard_normal(2 * C)).astype(np.float32))
    mp, Hn, Wn = merge_map(D, H, W)
    Ln = D * Hn * Wn
    kw = {}
    if emit:
        lay = O.window_layout(D, Hn, Wn, WINDOW, (0, 0, 0))
        assert (lay["src"] >= 0).all()
        kw = dict(next_norm=(_dev(gn), _dev(bn)), next_dst=_dev(torch.from_numpy(_inverse(lay["src"], Ln))), next_rows=Ln)
    out, nxt = kernels.patch_merge(_dev(x.to(torch.float16) if x16 else x), _dev(torch.from_numpy(mp)), B, _dev(red), _dev(gm), _dev(be),
                                   out_dtype=half, out_f16=out16, **kw)
    res = {"out": out}
    if emit:
        res["norm1"] = nxt
    return res


def cases():
    """[(case id without the operand type, function(half) -> {name: tensor})]; every case runs for fp16 and bf16 operands"""
    cs = []
    add = lambda name, fn, *a, **k: cs.append((name, lambda half, fn=fn, a=a, k=k: fn(*a, half=half, **k)))      # noqa: E731
    # C = 192, hidden 768.  (3,5,7) x 2 clips: 210 rows = one full and one ragged 128-token tile, a window clamped to the volume
    add("tail192-3x5x7-m0-x32", tail_case, 192, (3, 5, 7), 2, (0, 0, 0), None, 0, False, seed=1)
    add("tail192-3x5x7-m0-x16", tail_case, 192, (3, 5, 7), 2, (0, 0, 0), None, 0, True, seed=1)
    add("tail192-8x14x7-m1-x16", tail_case, 192, (8, 14, 7), 1, (0, 0, 0), (4, 3, 3), 1, True, seed=2)
    add("tail192-8x14x7-m2-x16", tail_case, 192, (8, 14, 7), 1, (0, 0, 0), (4, 3, 3), 2, True, seed=2)
    # a padded partition: through the scatter map (window rows, dead lanes on the padding) and through attn_gather (token rows)
    add("tail192-4x10x9-m0-gather", tail_case, 192, (4, 10, 9), 2, (4, 3, 3), None, 0, False, gather=True, seed=3)
    add("tail192-4x10x9-m0-scatter", tail_case, 192, (4, 10, 9), 2, (4, 3, 3), None, 0, False, seed=3)
    # C = 96.  (MODE 2 does not exist at this width: 3C / 32 = 9 panels do not pair into ring items and kvq_block_tail_qkv_pack_bytes is 0;
    # tests/test_gpu_stage1_registers.py asserts that refusal instead)
    add("tail96-8x14x14-m1-x16", tail_case, 96, (8, 14, 14), 1, (0, 0, 0), (4, 3, 3), 1, True, seed=4)
    add("tail96-8x14x14-m1-x32", tail_case, 96, (8, 14, 14), 1, (0, 0, 0), (4, 3, 3), 1, False, seed=4)
    for dims, B, sd in (((8, 14, 14), 2, 5), ((3, 5, 7), 2, 6)):       # (3,5,7): odd H and W, -1 neighbours; 72 merged tokens
        for emit in (False, True):
            for x16, out16 in ((False, False), (True, False), (True, True), (False, True)):
                name = f"merge192-{dims[0]}x{dims[1]}x{dims[2]}-{'emit' if emit else 'plain'}-x{16 if x16 else 32}-o{16 if out16 else 32}"
                add(name, merge_case, 192, dims, B, emit, x16, out16, seed=sd)
    return cs


def run_all():
    """{"<case>/<operand type>/<output>": (sha256 hex, raw uint8 array or None)}"""
    res = {}
    for name, fn in cases():
        for hname, half in HALVES.items():
            for oname, t in fn(half).items():
                res[f"{name}/{hname}/{oname}"] = (digest(t), raw_bytes(t).copy() if name in RAW else None)
    torch.cuda.synchronize()
    return res


def main():
    import kvq_amd  # noqa: F401
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "stage1_bits.npz")
    res = run_all()
    keys = sorted(res)
    arrays = {"keys": np.array(keys), "sha256": np.array([res[k][0] for k in keys])}
    for i, k in enumerate(keys):       # raw rows under the index of their key
        if res[k][1] is not None:
            arrays[f"raw_{i}"] = res[k][1]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print(f"{len(keys)} outputs -> {out} ({os.path.getsize(out)} bytes)")
    for k in keys:
        print(res[k][0][:16], k)


if __name__ == "__main__":
    main()
