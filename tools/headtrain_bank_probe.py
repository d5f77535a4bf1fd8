#!/usr/bin/env python
"""The feature bank of head fine-tuning on the GPU: what a training step costs when it reads its batch in place from an fp32, fp16 or
bf16 bank, beside the step of before (gather the batch with index_select, then the dense step); what the store launch costs beside the
torch ops it replaces; what a bank weighs; and how far three steps on a 16-bit bank move the parameters from three steps on the fp32
bank.  Writes profiles/headtrain_bank_probe.txt (or --out).  Reported, not gated: the reason for the bank is capacity (K draws fit on the
card at 16 bits) and the training regime, not speed.

  - VQAHead step at B = 16 and 256 clips of L = 16 x 7 x 7 tokens, C = 768, dropout 0.5; simpleVQAHead step at B = 16 and 256 videos of
    T = 8 rows, C = 9472.  The bank holds 4 B rows, the batch is a shuffled index into it.
  - 'index_select + step': feats.index_select(0, idx) on the fp32 rows, then forward, loss, backward, AdamW + EMA through the dense wrappers
    (the bank step on the gathered batch under an identity index); 'indexed': the same launches on the bank itself, no gathered copy.
    Both include the three scalars read back per step.
  - store: the store launch from a channels-last trunk output view into the bank, beside feat.to(dtype) plus the copy into the bank's rows
    (for fp32: the .contiguous() layout copy plus the torch.cat share of one video).

MEASURED: every time (us, hipEvent brackets, median of three windows of --iters calls per variant after --warmup calls, the variants
taken in turn inside each of the three rounds, all in this one process) and the parameter differences.  DERIVED from the shapes, not
measured: the bank bytes, the bytes a step reads, and the capacity table at the end."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch

import kvq_amd  # noqa: F401
from kvq_amd import kernels

DEV = "cuda:0"
DTYPES = (("fp32", torch.float32), ("fp16", torch.float16), ("bf16", torch.bfloat16))


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def alternating(variants, warmup, iters, rounds=3):
    """{name: fn} -> {name: median over ``rounds`` of one window of ``iters`` calls}; every round times every variant in turn"""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            got[k].append(window(fn, iters))
    return {k: sorted(v)[len(v) // 2] for k, v in got.items()}


class Step:
    """one training step of either head on dense features or on bank rows, with its own optimiser state"""

    def __init__(self, simple, B, L, C, g):
        self.simple, self.it = simple, 0
        hid = 128 if simple else 64
        n = hid * C + 2 * hid + 1
        self.p = torch.cat([0.05 * torch.randn(hid * C, device=DEV, generator=g), 0.1 * torch.randn(hid, device=DEV, generator=g),
                            0.3 * torch.randn(hid, device=DEV, generator=g), torch.zeros(1, device=DEV)]).contiguous()
        self.m, self.v, self.ema, self.grads = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), self.p.clone(), torch.empty(n, device=DEV)
        self.ws = (kernels.simple_headtrain_workspace if simple else kernels.headtrain_workspace)(B, L, C)
        self.score, self.out3, self.dscore = torch.empty(B, device=DEV), torch.empty(3, device=DEV), torch.empty(B, device=DEV)

    def _tail(self):
        kernels.headtrain_adamw(self.p, self.grads, self.m, self.v, self.ema, 1e-4, 0.05, self.it + 1)
        self.it += 1
        return self.out3.tolist()                  # the step's one read-back, as _Finetuner.step does

    def dense(self, x, y):
        if self.simple:
            kernels.simple_headtrain_forward(x, self.p, self.ws, self.score)
        else:
            kernels.headtrain_forward(x, self.p, 0.5, 0, self.it, self.ws, self.score)
        kernels.headtrain_loss(self.score, y, 0.0, self.out3, self.dscore)
        if self.simple:
            kernels.simple_headtrain_backward(x, self.p, self.ws, self.dscore, self.grads)
        else:
            kernels.headtrain_backward(x, self.p, 0.5, 0, self.it, self.ws, self.dscore, self.grads)
        return self._tail()

    def indexed(self, bank, idx, y):
        if self.simple:
            kernels.simple_headtrain_bank_forward(bank, idx, self.p, self.ws, self.score)
        else:
            kernels.headtrain_bank_forward(bank, idx, self.p, 0.5, 0, self.it, self.ws, self.score)
        kernels.headtrain_loss(self.score, y, 0.0, self.out3, self.dscore)
        if self.simple:
            kernels.simple_headtrain_bank_backward(bank, idx, self.p, self.ws, self.dscore, self.grads)
        else:
            kernels.headtrain_bank_backward(bank, idx, self.p, 0.5, 0, self.it, self.ws, self.dscore, self.grads)
        return self._tail()


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def golden_case_b_drift():
    """three chained steps of golden case b (B 5, L 196, C 768, p 0.5) on its fixture input stored in an fp32, fp16 and bf16 bank: the
    relative L2 difference of the parameters (and of their movement p - p0) between each 16-bit bank and the fp32 bank"""
    import headtrain_ref as R
    g = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "headtrain.npz"))
    B, D, H, W, Cc, seed = (int(v) for v in g["b/meta"])
    p_drop, rw = (float(v) for v in g["b/pw"])
    lr, wd, wu, mx = (float(v) for v in g["hyper"])
    x, y, prm = R.make_case(seed, B, D * H * W, Cc)
    x, y = torch.from_numpy(x.astype(np.float32)).to(DEV), torch.from_numpy(y.astype(np.float32)).to(DEV)
    idx = torch.arange(B, dtype=torch.int32, device=DEV)
    out = {}
    for name, dt in DTYPES:
        bank = kernels.FeatureBank(B, D * H * W, Cc, dt, device=DEV)
        kernels.feature_bank_store(x, bank, 0)
        p = torch.from_numpy(prm.astype(np.float32)).to(DEV)
        m, v, ema, ws = torch.zeros_like(p), torch.zeros_like(p), p.clone(), kernels.headtrain_workspace(B, D * H * W, Cc)
        for k in range(3):
            score = kernels.headtrain_bank_forward(bank, idx, p, p_drop, seed, k, ws)
            _, dscore = kernels.headtrain_loss(score, y, rw)
            grads = kernels.headtrain_bank_backward(bank, idx, p, p_drop, seed, k, ws, dscore)
            kernels.headtrain_adamw(p, grads, m, v, ema, lr * R.lr_factor(k, int(wu), int(mx)), wd, k + 1)
        out[name] = p
    p0 = torch.from_numpy(prm.astype(np.float32)).to(DEV)
    return {n: (rel_l2(out[n], out["fp32"]), rel_l2(out[n] - p0, out["fp32"] - p0)) for n in ("fp16", "bf16")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "headtrain_bank_probe.txt"))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=40)
    args = ap.parse_args()
    if args.iters < 30:
        raise SystemExit("headtrain_bank_probe: at least 30 timed repetitions per window")
    if not torch.cuda.is_available():
        raise SystemExit("headtrain_bank_probe: no HIP device (times are only ever taken on the GPU)")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:             # rewritten line by line: a run cut short keeps what it measured
            f.write("\n".join(lines) + "\n")

    say(f"device: {kernels.device_name()}")
    say(f"MEASURED: times in us per call, hipEvent brackets, median of 3 windows of {args.iters} calls per variant after {args.warmup} warm-up "
        "calls, the variants in turn inside each round, one process; the parameter differences")
    say("DERIVED from the shapes, not measured: bank bytes, bytes read per step, the capacity table")
    g = torch.Generator(device=DEV).manual_seed(0)
    for simple, L, C in ((False, 16 * 7 * 7, 768), (True, 8, 9472)):
        for B in (16, 256):
            rows = 4 * B
            base = torch.randn(rows, L, C, device=DEV, generator=g)
            y = torch.rand(B, device=DEV, generator=g) * 4 + 1
            idx = torch.randperm(rows, device=DEV, generator=g)[:B].contiguous()
            idx32 = idx.to(torch.int32)
            banks = {name: kernels.FeatureBank.of(base.to(dt)) for name, dt in DTYPES}
            st = {k: Step(simple, B, L, C, g) for k in ("index_select + step", "indexed fp32", "indexed fp16", "indexed bf16")}
            variants = {"index_select + step": lambda: st["index_select + step"].dense(base.index_select(0, idx), y)}
            for name, _ in DTYPES:
                variants[f"indexed {name}"] = (lambda n: lambda: st[f"indexed {n}"].indexed(banks[n], idx32, y))(name)
            t = alternating(variants, args.warmup, args.iters)
            head = "simpleVQAHead" if simple else "VQAHead"
            say()
            say(f"{head} step, B = {B}, {'T' if simple else 'L'} = {L}, C = {C}: batch {B * L * C * 4 / 2 ** 20:.1f} MiB in fp32; index_select reads and "
                f"writes it once more ({2 * B * L * C * 4 / 2 ** 20:.1f} MiB, derived)")
            ref = t["index_select + step"]
            for k, v in t.items():
                say(f"  {k:22s} {v:9.1f} us   {v / ref:5.2f} x index_select + step")
            say("  bank of 4 B rows (derived): " + "  ".join(f"{n} {banks[n].nbytes / 2 ** 20:.1f} MiB" for n, _ in DTYPES))
            del banks, st, variants, base
            torch.cuda.empty_cache()
    # the store launch beside the torch ops it replaces: one video of 4 clips, channels-last behind (4, C, 16, 7, 7)
    n, L, C = 4, 16 * 7 * 7, 768
    store = torch.randn(n, L, C, device=DEV, generator=g)
    feat5 = store.reshape(n, 16, 7, 7, C).permute(0, 4, 1, 2, 3)
    view = feat5.permute(0, 2, 3, 4, 1).reshape(n, L, C)
    assert view.data_ptr() == store.data_ptr()
    say()
    say(f"store of one video ({n} clips x {L} x {C}, {n * L * C * 4 / 2 ** 20:.1f} MiB fp32) into row 8 of a 16-row bank")
    for name, dt in DTYPES:
        bank = kernels.FeatureBank(16, L, C, dt, device=DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)

        def torch_way():
            f = feat5.to(torch.float32).reshape(n, C, -1).transpose(1, 2).contiguous()       # the layout copy of before
            bank.tensor[8:8 + n].copy_(f.to(dt))

        t = alternating({"store launch": lambda: kernels.feature_bank_store(view, bank, 8, flag), "torch": torch_way}, args.warmup, args.iters)
        say(f"  {name}: store launch {t['store launch']:7.1f} us   layout copy + .to({name}) + copy into the rows {t['torch']:7.1f} us   "
            f"({t['store launch'] / t['torch']:4.2f} x)")
    d = golden_case_b_drift()
    say()
    say("three chained steps of golden case b (B 5, L 196, C 768, p 0.5), the fixture input stored in a 16-bit bank against the fp32 bank (measured):")
    for name, (dp, dm) in d.items():
        say(f"  {name}: relative L2 of the parameters {dp:.3e}, of their movement p - p0 {dm:.3e}")
    say()
    say("capacity (derived): 10 000 videos x 4 clips x 784 x 768")
    for draws in (1, 4):
        say(f"  {draws} draw(s): fp32 {draws * 40000 * 784 * 768 * 4 / 1e9:6.1f} GB   16-bit {draws * 40000 * 784 * 768 * 2 / 1e9:6.1f} GB   (the card has 288 GB)")


if __name__ == "__main__":
    main()
