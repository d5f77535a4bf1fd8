"""Numpy float64 restatement of the simpleVQAHead training step (csrc/simple_headtrain.hip), written from the formulas:

  forward  h[b,t,:] = W1 X[b,t,:] + b1;  s[b,t] = w2 . h[b,t,:] + b2;  score[b] = mean_t s[b,t]
  backward ds[b,t] = dscore[b] / T;  dW1 = sum ds (w2 (x) X[b,t,:]);  db1 = w2 sum ds;  dw2 = sum ds h[b,t,:];  db2 = sum ds
           (the two-stage form, on purpose: the kernels use the collapsed one)

The losses, AdamW, the EMA update and the schedule are those of tests/headtrain_ref.py.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from headtrain_ref import adamw, ema_update, loss_and_dscore, lr_factor, plcc_loss, rank_loss  # noqa: E402,F401

HID = 128


def forward(x, W1, b1, w2, b2):
    """x [B][T][C], W1 [H][C], b1 [H], w2 [H], b2 scalar -> score [B], cache for backward()"""
    x = np.asarray(x, np.float64)
    h = x @ np.asarray(W1, np.float64).T + np.asarray(b1, np.float64)
    s = h @ np.asarray(w2, np.float64) + float(np.asarray(b2).reshape(-1)[0])
    return s.mean(axis=1), dict(x=x, h=h, w2=np.asarray(w2, np.float64))


def backward(cache, dscore):
    """-> dW1 [H][C], db1 [H], dw2 [H], db2"""
    x, h, w2 = cache["x"], cache["h"], cache["w2"]
    B, T, _ = x.shape
    ds = np.repeat(np.asarray(dscore, np.float64) / T, T).reshape(B, T)
    dh = ds[:, :, None] * w2
    dW1 = np.einsum("bth,btc->hc", dh, x)
    return dW1, dh.sum(axis=(0, 1)), np.einsum("bt,bth->h", ds, h), float(ds.sum())


def flat(W1, b1, w2, b2):
    return np.concatenate([np.asarray(W1, np.float64).reshape(-1), np.asarray(b1, np.float64).reshape(-1),
                           np.asarray(w2, np.float64).reshape(-1), np.asarray(b2, np.float64).reshape(-1)])


def unflat(p, C, H=HID):
    return p[:H * C].reshape(H, C), p[H * C:H * C + H], p[H * C + H:H * C + 2 * H], p[H * C + 2 * H:]


def make_case(seed, B, T, C):
    """the fixture's inputs: unit-variance fp32 features [B][T][C], labels in 1 .. 5 and the flat float64 initial parameters (fp32
    values: W1 std 0.02, b1 std 0.1, w2 std 0.1, b2 0.5), from PCG64(seed).  The scales give scores a spread of
    sqrt(128 C / T) * 0.02 * 0.1 (0.8 at C = 9472, T = 8; 0.3 at C = 192, T = 1), so the PLCC loss's division by the score std does not
    amplify rounding."""
    g = np.random.Generator(np.random.PCG64(seed))
    x = g.standard_normal((B, T, C)).astype(np.float32)
    y = g.uniform(1.0, 5.0, B).astype(np.float32).astype(np.float64)
    W1 = (0.02 * g.standard_normal((HID, C))).astype(np.float32)
    b1 = (0.1 * g.standard_normal(HID)).astype(np.float32)
    w2 = (0.1 * g.standard_normal(HID)).astype(np.float32)
    return x, y, flat(W1, b1, w2, np.array([0.5], np.float32))


def train_steps(x, y, params, n_steps, lr, wd, warmup_iters, max_iters, rank_weight=0.0, zero_grads=None):
    """``n_steps`` full steps from the flat float64 ``params`` (AdamW state and EMA start as torch's: zeros, a copy); the LR of optimiser
    step k (1-based) is lr * lr_factor(k - 1).  -> list of per-step dicts.
    ``zero_grads``: per step, the values [H + 1] AdamW sees as the gradients of b1 | b2 instead of this run's.  Those gradients are
    analytically zero and whatever an implementation gets is its rounding noise, which Adam's normalisation turns into a full-size step
    of either sign; a caller that follows another implementation's parameters hands its noise over (the step's own values stay in
    ``grads``)."""
    x = np.asarray(x, np.float64)
    C = x.shape[2]
    nW = HID * C
    prm, m, v, ema = params.copy(), np.zeros_like(params), np.zeros_like(params), params.copy()
    out = []
    for k in range(n_steps):
        score, cache = forward(x, *unflat(prm, C))
        losses, dscore = loss_and_dscore(score, y, rank_weight)
        g = flat(*backward(cache, dscore))
        lr_k = lr * lr_factor(k, warmup_iters, max_iters)
        g_opt = g.copy()
        if zero_grads is not None:
            g_opt[nW:nW + HID] = zero_grads[k][:HID]
            g_opt[-1] = zero_grads[k][HID]
        prm, m, v = adamw(prm, g_opt, m, v, lr_k, wd, k + 1)
        ema = ema_update(ema, prm)
        out.append(dict(score=score, losses=np.asarray(losses), dscore=dscore, grads=g, params=prm.copy(), ema=ema.copy(), lr=lr_k))
    return out
