"""Emit tests/golden/simple_headtrain.npz: three optimisation steps of the reference's simpleVQAHead on fixed features, run by the
reference's own code.  Runs ONLY where the reference is present (imported through _ref_import.py); the fixture is arrays only.

What runs: the reference's ``simpleVQAHead`` (models/head.py) in float64; ``Trainer.plcc_loss`` / ``Trainer.rank_loss``; the optimiser
and the LambdaLR that ``Trainer.build_optimizer`` builds (torch.optim.AdamW, one parameter group, warmup 2 iterations, max 10); the EMA
update of trainer.py:166-172.  The reference's losses end in ``.float()``, which would round the float64 run's loss values to fp32:
``torch.Tensor.float`` is the identity while the float64 run computes its losses.

Inputs and initial parameters of a case come from ``simple_headtrain_ref.make_case(seed, B, T, C)`` (numpy PCG64), so a test rebuilds
them.  Stored per case ``<name>/``:

  meta                      B, T, C, seed                         rank_weight: ``rw``;  lr, wd, warmup, max: ``hyper``
  x_head, x_sum, params0_sub, params0_small, labels
                            the first 256 features and their float64 sum, the [3::16, 5::64] subsample of W1, b1 | w2 | b2: to check the rebuild
  score, losses, dscore     [3 steps][...], float64 ({loss, plcc, rank})
  dW1_sub, dW1_norm, dW1_sum, db1, dW2, db2       [3 steps]: gradients; W1-shaped tensors as the subsample, L2 norm and sum
  W1_sub, W1_norm, small    [3 steps]: parameters after each step (small = b1 | w2 | b2);  ema_W1_sub, ema_W1_norm, ema_small likewise
  ref32_err/<tensor>        [3 steps]: relative L2 of the SAME run in float32 (the reference in fp32, on the full tensors) against float64;
                            tensors: score, losses, dscore, dW1, dW2 and dp = (W1 | w2 of p - p0) after the step
  alt32_err/<tensor>        the same for the float32 run with the feature channels and W1's columns reversed: the same mathematics in
                            another summation order (its dW1 and W1 are reversed back before they are compared)
  db1_32, db2_32            [2 runs][3 steps]: max |db1| and |db2| of the two float32 runs (analytically zero)
  adamw32_err               relative L2 of (W1 | w2 of p - p0) and of the EMA's W1 | w2 after 3 steps of torch's fp32 AdamW fed the
                            fp32-rounded float64 gradients
lr_factors: the scheduler's factor at iterations 0 .. 11.

W1-shaped tensors are stored as a subsample because a committed fixture stays below 1 MiB (one float64 W1 is 9.7 MB at C = 9472); the
test compares the numpy restatement with the subsample, the norm and the sum, and the GPU tests compare full tensors with the restatement.

The generator asserts, and moves to the next seed otherwise (20 seeds at most: beyond that the input scale of make_case is wrong):
relative error <= 5e-6 for dW1 and dW2 at every step in BOTH float32 runs; no two scores closer than 1e-6; score std >= 0.1.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_simple_headtrain_golden.py
"""
import contextlib
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch
import torch.nn as nn

from _ref_import import import_reference
import simple_headtrain_ref as R

# name -> (B, T, C, rank_weight, first seed).  a - d, c_rank: the smallest shapes at which the launches can go wrong (row tiles, tails, odd T,
# C an odd multiple of 64);  e: more than 256 videos and 1200 rows, where the backward's runs are longer than their 32-row minimum
CASES = {"a": (4, 8, 9472, 0.0, 100), "b": (5, 3, 9472, 0.0, 200), "c": (7, 1, 192, 0.0, 300), "d": (33, 8, 704, 0.0, 400),
         "c_rank": (7, 1, 192, 0.3, 300), "e": (300, 4, 192, 0.0, 500)}
LR, WD, STEPS, HID = 1e-3, 0.05, 3, 128
SCHED = {"warmup_epochs": 2, "num_epochs": 6, "l_num_epochs": 4}          # one batch per epoch: warmup 2 iterations, max 10
SUB = (slice(3, None, 16), slice(5, None, 64))


@contextlib.contextmanager
def float_is_identity():
    saved = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self
    try:
        yield
    finally:
        torch.Tensor.float = saved


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def run(ref, case, seed, dtype, reverse=False):
    """three steps -> per-step dicts in the ORIGINAL channel order"""
    B, T, C, rw, _ = case
    x, y, prm = R.make_case(seed, B, T, C)
    W1, b1, w2, b2 = R.unflat(prm, C)
    flip = (lambda a: np.ascontiguousarray(a[..., ::-1])) if reverse else (lambda a: a)
    head = ref.head.simpleVQAHead(in_channels=C, hidden_channels=HID).to(dtype)
    with torch.no_grad():
        head.quality[0].weight.copy_(torch.from_numpy(flip(W1)))
        head.quality[0].bias.copy_(torch.from_numpy(b1))
        head.quality[1].weight.copy_(torch.from_numpy(w2).reshape(1, HID))
        head.quality[1].bias.copy_(torch.from_numpy(b2))
    ema = [q.detach().clone() for q in head.parameters()]
    fake = types.SimpleNamespace(model=nn.ModuleDict({"head": head}), train_loader=[0],
                                 config=dict(SCHED, optimizer={"lr": LR, "wd": WD, "backbone_lr_mult": 0}))
    ref.trainer.Trainer.build_optimizer(fake)
    Tr = ref.trainer.Trainer
    xt = torch.from_numpy(flip(x)).to(dtype)
    yt = torch.from_numpy(y).to(dtype).reshape(B, 1)

    def flat(ps):
        W, bb, w, b = (q.detach().double().numpy() for q in ps)
        return R.flat(flip(W), bb, w, b)

    out = []
    head.train()
    for k in range(STEPS):
        fake.optimizer.zero_grad()
        score = head(xt)
        score.retain_grad()
        with (float_is_identity() if dtype == torch.float64 else contextlib.nullcontext()):
            pl, rk = Tr.plcc_loss(None, score, yt), Tr.rank_loss(None, score, yt)
            loss = pl + rw * rk
        loss.backward()
        g = flat([q.grad for q in head.parameters()])
        fake.optimizer.step()
        fake.scheduler.step()
        with torch.no_grad():
            for e, q in zip(ema, head.parameters()):
                e.mul_(0.999).add_(q.data, alpha=1 - 0.999)
        out.append(dict(score=score.detach().double().numpy().reshape(-1), losses=np.array([loss.item(), pl.item(), rk.item()]),
                        dscore=score.grad.double().numpy().reshape(-1), grads=g, params=flat(list(head.parameters())), ema=flat(ema)))
    return out, (x, y, prm), fake.scheduler


def trained(v, nW):
    """W1 | w2 of a flat vector: the parameters whose gradients are not analytically zero"""
    return np.concatenate([v[:nW], v[nW + HID:nW + 2 * HID]])


def adamw32_err(steps64, prm0, nW):
    """torch's own fp32 AdamW on the fp32-rounded float64 gradients, against the float64 run"""
    p = nn.Parameter(torch.from_numpy(prm0).float())
    opt = torch.optim.AdamW([p], lr=LR, weight_decay=WD)
    ema = p.detach().clone()
    for k, st in enumerate(steps64):
        for grp in opt.param_groups:
            grp["lr"] = LR * R.lr_factor(k, 2, 10)
        p.grad = torch.from_numpy(st["grads"]).float()
        opt.step()
        ema.mul_(0.999).add_(p.data, alpha=1 - 0.999)
    last = steps64[-1]
    return np.array([rel(trained(p.detach().double().numpy() - prm0, nW), trained(last["params"] - prm0, nW)),
                     rel(trained(ema.double().numpy(), nW), trained(last["ema"], nW))])


def errors(s32, s64, prm, nW):
    cut = {"dW1": slice(0, nW), "dW2": slice(nW + HID, nW + 2 * HID)}
    errs = {k: [rel(a["grads"][c], b["grads"][c]) for a, b in zip(s32, s64)] for k, c in cut.items()}
    for k in ("score", "losses", "dscore"):
        errs[k] = [rel(a[k], b[k]) for a, b in zip(s32, s64)]
    # step 1 runs at lr 0: p = p0
    errs["dp"] = [0.0] + [rel(trained(a["params"] - prm, nW), trained(b["params"] - prm, nW)) for a, b in zip(s32[1:], s64[1:])]
    return errs


def main():
    ref = import_reference()
    torch.manual_seed(0)
    out = {"hyper": np.array([LR, WD, 2, 10], np.float64)}
    factors = None
    for name, case in CASES.items():
        B, T, C, rw, seed = case
        nW = HID * C
        for _ in range(20):
            s64, (x, y, prm), sched = run(ref, case, seed, torch.float64)
            s32, _, _ = run(ref, case, seed, torch.float32)
            a32, _, _ = run(ref, case, seed, torch.float32, reverse=True)
            e_ref, e_alt = errors(s32, s64, prm, nW), errors(a32, s64, prm, nW)
            sc = np.sort(s64[0]["score"])
            worst = max(max(e[k]) for e in (e_ref, e_alt) for k in ("dW1", "dW2"))
            ok = worst <= 5e-6 and np.diff(sc).min() > 1e-6 and s64[0]["score"].std() >= 0.1
            print(name, "seed", seed, "ok" if ok else "REJECTED", "ref", {k: ["%.2e" % e for e in v] for k, v in e_ref.items()},
                  "alt", {k: ["%.2e" % e for e in v] for k, v in e_alt.items()}, "score std %.3f" % s64[0]["score"].std())
            if ok:
                break
            seed += 1
        else:
            raise SystemExit(f"case {name}: no seed among 20 passes; the input scale of make_case is wrong")
        sub = lambda v: np.ascontiguousarray(v[:nW].reshape(HID, C)[SUB])        # noqa: E731
        o = {"meta": np.array([B, T, C, seed], np.int64), "rw": np.array(rw, np.float64),
             "x_head": x.reshape(-1)[:256].copy(), "x_sum": np.array(x.astype(np.float64).sum()), "labels": y, "params0_sub": sub(prm),
             "params0_small": prm[nW:],
             "score": np.stack([s["score"] for s in s64]), "losses": np.stack([s["losses"] for s in s64]),
             "dscore": np.stack([s["dscore"] for s in s64]),
             "dW1_sub": np.stack([sub(s["grads"]) for s in s64]), "dW1_norm": np.array([np.linalg.norm(s["grads"][:nW]) for s in s64]),
             "dW1_sum": np.array([s["grads"][:nW].sum() for s in s64]),
             "db1": np.stack([s["grads"][nW:nW + HID] for s in s64]), "dW2": np.stack([s["grads"][nW + HID:nW + 2 * HID] for s in s64]),
             "db2": np.array([s["grads"][-1] for s in s64]),
             "db1_32": np.array([[np.abs(s["grads"][nW:nW + HID]).max() for s in r] for r in (s32, a32)]),
             "db2_32": np.array([[abs(s["grads"][-1]) for s in r] for r in (s32, a32)]),
             "W1_sub": np.stack([sub(s["params"]) for s in s64]), "W1_norm": np.array([np.linalg.norm(s["params"][:nW]) for s in s64]),
             "small": np.stack([s["params"][nW:] for s in s64]),
             "ema_W1_sub": np.stack([sub(s["ema"]) for s in s64]), "ema_W1_norm": np.array([np.linalg.norm(s["ema"][:nW]) for s in s64]),
             "ema_small": np.stack([s["ema"][nW:] for s in s64]), "adamw32_err": adamw32_err(s64, prm, nW)}
        for k, v in e_ref.items():
            o[f"ref32_err/{k}"] = np.array(v)
        for k, v in e_alt.items():
            o[f"alt32_err/{k}"] = np.array(v)
        out.update({f"{name}/{k}": v for k, v in o.items()})
        if factors is None:
            factors = np.array([sched.lr_lambdas[0](i) for i in range(12)], np.float64)
    out["lr_factors"] = factors
    path = os.path.join(HERE, "simple_headtrain.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
