"""Emit tests/golden/headtrain.npz: three optimisation steps of the reference's VQAHead on fixed features, run by the reference's own
code.  Runs ONLY where the reference is present (imported through _ref_import.py); the fixture is arrays only.

What runs: the reference's ``VQAHead`` (models/head.py) in train mode and float64, its ``dropout`` attribute replaced by a module that
multiplies by a given mask (chosen by the input's channel count; the masks are the numpy restatement of the hash of csrc/headtrain.hpp,
tests/headtrain_ref.py); ``Trainer.plcc_loss`` / ``Trainer.rank_loss``; the optimiser and the LambdaLR that ``Trainer.build_optimizer``
builds (torch.optim.AdamW, one parameter group, warmup 2 iterations, max 10); the EMA update of trainer.py:166-172.  The reference's
losses end in ``.float()``, which would round the float64 run's loss values to fp32: ``torch.Tensor.float`` is the identity while the
float64 run computes its losses.

Inputs and initial parameters of a case come from ``headtrain_ref.make_case(seed, B, L, C)`` (numpy PCG64), so a test rebuilds them;
labels from the same generator.  Stored per case ``<name>/``:

  meta                      B, D, H, W, C, seed                   p, rank_weight, lr, wd: ``hyper``
  x_head, x_sum, params0_sub, params0_small, labels
                            the first 256 features and their float64 sum, the [:, 5::32] subsample of W1, b1 | w2 | b2: to check the rebuild
  m1_bits, m2_bits          step 0: the first 65536 mask bits of the feature dropout and all of the hidden one, np.packbits
  score, losses, dscore     [3 steps][...], float64 ({loss, plcc, rank})
  dW1_sub, dW1_norm, dW1_sum, db1, dW2, db2       [3 steps]: gradients; W1-shaped tensors as the subsample [:, 5::32], L2 norm and sum
  W1_sub, W1_norm, small    [3 steps]: parameters after each step (small = b1 | w2 | b2);  ema_W1_sub, ema_W1_norm, ema_small likewise
  ref32_err/<tensor>        [3 steps]: relative L2 of the SAME run in float32 (the reference in fp32, on the full tensors) against float64;
                            tensors: score, losses, dscore, dW1, db1, dW2 and dp = (W1 | b1 | w2 of p - p0) after the step
  db2_32                    [3 steps]: |db2| of the float32 run (analytically zero)
  adamw32_err               relative L2 of p - p0 and of the EMA after 3 steps of torch's fp32 AdamW fed the fp32-rounded float64 gradients
lr_factors: the scheduler's factor at iterations 0 .. 11.

W1-shaped tensors are stored as a subsample because a committed fixture stays below 1 MiB (one float64 W1 is 393 KB); the test compares
the numpy restatement with the subsample, the norm and the sum, and the GPU tests compare full tensors with the restatement.

The generator asserts, and moves to the next seed otherwise: ref32_err <= 5e-6 for dW1, db1, dW2; no two scores closer than 1e-6;
score std >= 0.1; B >= 3.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_headtrain_golden.py
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
import headtrain_ref as R

# name -> (B, D, H, W, C, p, rank_weight, first seed)
CASES = {"a": (4, 2, 3, 3, 768, 0.5, 0.0, 100), "b": (5, 4, 7, 7, 768, 0.5, 0.0, 200), "c": (6, 3, 7, 7, 768, 0.0, 0.0, 300),
         "d": (7, 1, 7, 7, 768, 0.5, 0.0, 400), "e": (4, 2, 3, 3, 128, 0.5, 0.0, 500), "e_rank": (4, 2, 3, 3, 128, 0.5, 0.3, 500)}
LR, WD, STEPS, HID = 1e-3, 0.05, 3, 64
SCHED = {"warmup_epochs": 2, "num_epochs": 6, "l_num_epochs": 4}          # one batch per epoch: warmup 2 iterations, max 10


class MaskDropout(nn.Module):
    def __init__(self):
        super().__init__()
        self.masks = {}

    def forward(self, x):
        return x * self.masks[x.shape[1]]


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


def run(ref, case, seed, dtype):
    B, D, H, W, C, p, rw, _ = case
    L = D * H * W
    x, y, prm = R.make_case(seed, B, L, C)
    head = ref.head.VQAHead(in_channels=C, hidden_channels=HID, dropout_ratio=0.5).to(dtype)
    W1, b1, w2, b2 = R.unflat(prm, C, HID)
    with torch.no_grad():
        head.fc_hid.weight.copy_(torch.from_numpy(W1).reshape(HID, C, 1, 1, 1))
        head.fc_hid.bias.copy_(torch.from_numpy(b1))
        head.fc_last.weight.copy_(torch.from_numpy(w2).reshape(1, HID, 1, 1, 1))
        head.fc_last.bias.copy_(torch.from_numpy(b2))
    head.dropout = MaskDropout()
    ema = [q.detach().clone() for q in head.parameters()]
    fake = types.SimpleNamespace(model=nn.ModuleDict({"head": head}), train_loader=[0],
                                 config=dict(SCHED, optimizer={"lr": LR, "wd": WD, "backbone_lr_mult": 0}))
    ref.trainer.Trainer.build_optimizer(fake)
    T = ref.trainer.Trainer
    xt = torch.from_numpy(x).to(dtype).reshape(B, D, H, W, C).permute(0, 4, 1, 2, 3)
    yt = torch.from_numpy(y).to(dtype).reshape(B, 1)
    s = R.mask_scale(p)
    out = []
    head.train()
    for k in range(STEPS):
        m1 = R.mask(seed, k, 0, p, B * L * C).reshape(B, D, H, W, C)
        m2 = R.mask(seed, k, 1, p, B * L * HID).reshape(B, D, H, W, HID)
        head.dropout.masks = {C: (torch.from_numpy(m1).to(dtype) * s).permute(0, 4, 1, 2, 3),
                              HID: (torch.from_numpy(m2).to(dtype) * s).permute(0, 4, 1, 2, 3)}
        fake.optimizer.zero_grad()
        score = head(xt)
        score.retain_grad()
        with (float_is_identity() if dtype == torch.float64 else contextlib.nullcontext()):
            pl, rk = T.plcc_loss(None, score, yt), T.rank_loss(None, score, yt)
            loss = pl + rw * rk
        loss.backward()
        g = [q.grad.detach().clone().double().numpy() for q in head.parameters()]
        fake.optimizer.step()
        fake.scheduler.step()
        with torch.no_grad():
            for e, q in zip(ema, head.parameters()):
                e.mul_(0.999).add_(q.data, alpha=1 - 0.999)
        out.append(dict(score=score.detach().double().numpy().reshape(-1), losses=np.array([loss.item(), pl.item(), rk.item()]),
                        dscore=score.grad.double().numpy().reshape(-1), grads=R.flat(*g),
                        params=R.flat(*[q.detach().double().numpy() for q in head.parameters()]),
                        ema=R.flat(*[e.double().numpy() for e in ema]),
                        m1=m1.reshape(-1), m2=m2.reshape(-1)))
    return out, (x, y, prm), fake.scheduler


def adamw32_err(steps64, prm0):
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
    return np.array([rel(p.detach().double().numpy() - prm0, last["params"] - prm0), rel(ema.double().numpy(), last["ema"])])


def main():
    ref = import_reference()
    torch.manual_seed(0)
    out = {"hyper": np.array([LR, WD, 2, 10], np.float64)}
    factors = None
    for name, case in CASES.items():
        B, D, H, W, C, p, rw, seed = case
        assert B >= 3
        while True:
            s64, (x, y, prm), sched = run(ref, case, seed, torch.float64)
            s32, _, _ = run(ref, case, seed, torch.float32)
            nW = HID * C
            cut = {"dW1": slice(0, nW), "db1": slice(nW, nW + HID), "dW2": slice(nW + HID, nW + 2 * HID)}
            errs = {k: [rel(a["grads"][c], b["grads"][c]) for a, b in zip(s32, s64)] for k, c in cut.items()}
            for k in ("score", "losses", "dscore"):
                errs[k] = [rel(a[k], b[k]) for a, b in zip(s32, s64)]
            # W1 | b1 | w2 of p - p0 after steps 2 and 3 (step 1 runs at lr 0: p = p0); b2 follows the rounding noise of a zero gradient
            errs["dp"] = [0.0] + [rel((a["params"] - prm)[:nW + 2 * HID], (b["params"] - prm)[:nW + 2 * HID]) for a, b in zip(s32[1:], s64[1:])]
            sc = np.sort(s64[0]["score"])
            ok = (max(max(errs[k]) for k in cut) <= 5e-6 and np.diff(sc).min() > 1e-6 and s64[0]["score"].std() >= 0.1)
            print(name, "seed", seed, "ok" if ok else "REJECTED", {k: ["%.2e" % e for e in v] for k, v in errs.items()},
                  "score std %.3f" % s64[0]["score"].std())
            if ok:
                break
            seed += 1
        sub = lambda v: np.ascontiguousarray(v[:nW].reshape(HID, C)[:, 5::32])        # noqa: E731
        o = {"meta": np.array([B, D, H, W, C, seed], np.int64), "pw": np.array([p, rw], np.float64),
             "x_head": x.reshape(-1)[:256].copy(), "x_sum": np.array(x.astype(np.float64).sum()), "labels": y, "params0_sub": sub(prm), "params0_small": prm[nW:],
             "m1_bits": np.packbits(s64[0]["m1"][:65536]), "m2_bits": np.packbits(s64[0]["m2"]),
             "score": np.stack([s["score"] for s in s64]), "losses": np.stack([s["losses"] for s in s64]),
             "dscore": np.stack([s["dscore"] for s in s64]),
             "dW1_sub": np.stack([sub(s["grads"]) for s in s64]), "dW1_norm": np.array([np.linalg.norm(s["grads"][:nW]) for s in s64]),
             "dW1_sum": np.array([s["grads"][:nW].sum() for s in s64]),
             "db1": np.stack([s["grads"][cut["db1"]] for s in s64]), "dW2": np.stack([s["grads"][cut["dW2"]] for s in s64]),
             "db2": np.array([s["grads"][-1] for s in s64]), "db2_32": np.array([abs(s["grads"][-1]) for s in s32]),
             "W1_sub": np.stack([sub(s["params"]) for s in s64]), "W1_norm": np.array([np.linalg.norm(s["params"][:nW]) for s in s64]),
             "small": np.stack([s["params"][nW:] for s in s64]),
             "ema_W1_sub": np.stack([sub(s["ema"]) for s in s64]), "ema_W1_norm": np.array([np.linalg.norm(s["ema"][:nW]) for s in s64]),
             "ema_small": np.stack([s["ema"][nW:] for s in s64]), "adamw32_err": adamw32_err(s64, prm)}
        for k, v in errs.items():
            o[f"ref32_err/{k}"] = np.array(v)
        out.update({f"{name}/{k}": v for k, v in o.items()})
        if factors is None:
            factors = np.array([sched.lr_lambdas[0](i) for i in range(12)], np.float64)
    out["lr_factors"] = factors
    path = os.path.join(HERE, "headtrain.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
