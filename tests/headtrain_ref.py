"""Numpy float64 restatement of the VQAHead training step (csrc/headtrain.hip), written from the formulas:

  mask     element idx of dropout ``which`` at (seed, step) is kept iff bits(key(seed, step, which), idx) >= floor(p * 2^32), all uint32
  forward  score_b = mean_l( w2 . (m2 * gelu(W1 (m1 * f) + b1)) ) + b2, m = keep / (1 - p), gelu(z) = z Phi(z)
  plcc     a = (s - mean s) / (std s + 1e-8), t likewise of the labels (biased std); ((mean (a - t)^2) / 4 + (mean (rho a - t)^2) / 4) / 2,
           rho = mean(a t)
  rank     R_ij = relu((s_i - s_j) sign(y_j - y_i)); sum R / B / (B - 1) / (1 + max R)
  backward analytic, gelu'(z) = Phi(z) + z phi(z)
  AdamW    torch's: p *= 1 - lr wd; m += (g - m)(1 - b1); v = b2 v + (1 - b2) g^2; p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
  EMA      e = 0.999 e + 0.001 p
  LR       it / warmup while it <= warmup, else 0.5 (1 + cos(pi (it - warmup) / max_iters))
"""
import math

import numpy as np

try:
    from scipy.special import erf as _erf
except ImportError:                                    # pragma: no cover
    _erf = np.vectorize(math.erf, otypes=[np.float64])

U32 = np.uint32


def _fmix(x):
    x = x.astype(U32) if isinstance(x, np.ndarray) else np.asarray(x, dtype=np.uint64).astype(U32)
    with np.errstate(over="ignore"):
        x = x ^ (x >> U32(16))
        x = x * U32(0x85EBCA6B)
        x = x ^ (x >> U32(13))
        x = x * U32(0xC2B2AE35)
        x = x ^ (x >> U32(16))
    return x


def mask_key(seed, step, which):
    inner = _fmix((2 * int(step) + int(which) + 0x9E3779B9) & 0xFFFFFFFF)
    return int(_fmix((int(seed) & 0xFFFFFFFF) ^ int(inner)))


def mask_bits(key, idx):
    """idx: uint32 array"""
    key = int(key)
    rot = U32(((key << 13) | (key >> 19)) & 0xFFFFFFFF)
    with np.errstate(over="ignore"):
        x = idx.astype(U32) ^ U32(key)
        x = x ^ (x >> U32(16))
        x = x * U32(0x85EBCA6B)
        x = x + rot
        x = x ^ (x >> U32(13))
        x = x * U32(0xC2B2AE35)
        x = x ^ (x >> U32(16))
    return x


def mask_threshold(p):
    t = float(np.float32(p)) * 4294967296.0
    return 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def mask(seed, step, which, p, n):
    """uint8 [n]: 1 = kept"""
    bits = mask_bits(mask_key(seed, step, which), np.arange(n, dtype=np.uint64).astype(U32))
    return (bits >= U32(mask_threshold(p))).astype(np.uint8)


def mask_scale(p):
    return 1.0 / (1.0 - float(np.float32(p)))


def gelu(z):
    return 0.5 * z * (1.0 + _erf(z / math.sqrt(2.0)))


def dgelu(z):
    return 0.5 * (1.0 + _erf(z / math.sqrt(2.0))) + z * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def forward(x, W1, b1, w2, b2, m1=None, m2=None, p=0.0):
    """x [B][L][C], W1 [H][C], b1 [H], w2 [H], b2 scalar; m1 [B][L][C], m2 [B][L][H] keep masks (None: all kept).
    -> score [B], cache for backward()"""
    x = np.asarray(x, np.float64)
    s = mask_scale(p)
    k1 = np.ones_like(x) if m1 is None else np.asarray(m1, np.float64).reshape(x.shape) * s
    xd = x * k1
    z = xd @ np.asarray(W1, np.float64).T + np.asarray(b1, np.float64)
    k2 = np.ones_like(z) if m2 is None else np.asarray(m2, np.float64).reshape(z.shape) * s
    hd = gelu(z) * k2
    tok = hd @ np.asarray(w2, np.float64)
    score = tok.mean(axis=1) + float(np.asarray(b2).reshape(-1)[0])
    return score, dict(xd=xd, z=z, k2=k2, hd=hd, w2=np.asarray(w2, np.float64))


def backward(cache, dscore):
    """-> dW1 [H][C], db1 [H], dw2 [H], db2"""
    xd, z, k2, hd, w2 = (cache[k] for k in ("xd", "z", "k2", "hd", "w2"))
    B, L, _ = xd.shape
    g = (np.asarray(dscore, np.float64) / L).reshape(B, 1, 1)
    dw2 = (g * hd).sum(axis=(0, 1))
    dz = g * w2 * k2 * dgelu(z)
    db1 = dz.sum(axis=(0, 1))
    dW1 = np.einsum("blh,blc->hc", dz, xd)
    return dW1, db1, dw2, float(np.asarray(dscore, np.float64).sum())


def _norm(v):
    return (v - v.mean()) / (v.std() + 1e-8)


def plcc_loss(s, y):
    a, t = _norm(np.asarray(s, np.float64)), _norm(np.asarray(y, np.float64))
    rho = (a * t).mean()
    return (((a - t) ** 2).mean() / 4 + ((rho * a - t) ** 2).mean() / 4) / 2


def rank_loss(s, y):
    s, y = np.asarray(s, np.float64), np.asarray(y, np.float64)
    R = np.maximum((s[:, None] - s[None, :]) * np.sign(y[None, :] - y[:, None]), 0.0)
    n = len(s)
    return R.sum() / n / (n - 1) / (1 + R.max())


def loss_and_dscore(s, y, rank_weight=0.0):
    """-> (loss, plcc, rank), dscore: analytic derivative of plcc + rank_weight * rank, the 1 + max R of the rank loss included"""
    s, y = np.asarray(s, np.float64), np.asarray(y, np.float64)
    n = len(s)
    d = s - s.mean()
    sd = d.std()
    a, t = d / (sd + 1e-8), _norm(y)
    rho = (a * t).mean()
    e = rho * a - t
    ga = ((a - t) + rho * e + (e * a).sum() * t / n) / (4 * n)
    gp = (ga - ga.mean()) / (sd + 1e-8) - d * (ga * d).sum() / (n * sd * (sd + 1e-8) ** 2)
    sg = np.sign(y[None, :] - y[:, None])
    arg = (s[:, None] - s[None, :]) * sg
    R = np.maximum(arg, 0.0)
    pos = arg > 0
    M, tot = R.max(), R.sum()
    gr = 2 * (pos * sg).sum(axis=1) / (n * (n - 1) * (1 + M))
    if M > 0:
        i, j = np.unravel_index(np.argmax(R), R.shape)
        c = tot / (n * (n - 1) * (1 + M) ** 2)
        gr[i] -= c * sg[i, j]
        gr[j] += c * sg[i, j]
    pl, rk = plcc_loss(s, y), rank_loss(s, y)
    return (pl + rank_weight * rk, pl, rk), gp + rank_weight * gr


def adamw(p, g, m, v, lr, wd, step, beta1=0.9, beta2=0.999, eps=1e-8):
    """one torch.optim.AdamW step on float64 arrays; returns (p, m, v)"""
    p = p * (1 - lr * wd)
    m = m + (g - m) * (1 - beta1)
    v = v * beta2 + (1 - beta2) * g * g
    denom = np.sqrt(v) / math.sqrt(1 - beta2 ** step) + eps
    return p - (lr / (1 - beta1 ** step)) * m / denom, m, v


def ema_update(e, p):
    return 0.999 * e + 0.001 * p


def lr_factor(it, warmup_iters, max_iters):
    return it / warmup_iters if it <= warmup_iters else 0.5 * (1 + math.cos(math.pi * (it - warmup_iters) / max_iters))


def make_case(seed, B, L, C, hidden=64):
    """the fixture's inputs: unit-variance fp32 features [B][L][C], labels in 1 .. 5 and the flat float64 initial parameters (fp32
    values: W1 std 0.05, b1 std 0.1, w2 std 0.3, b2 0.5), from PCG64(seed)"""
    g = np.random.Generator(np.random.PCG64(seed))
    x = g.standard_normal((B, L, C)).astype(np.float32)
    y = g.uniform(1.0, 5.0, B).astype(np.float32).astype(np.float64)
    W1 = (0.05 * g.standard_normal((hidden, C))).astype(np.float32)
    b1 = (0.1 * g.standard_normal(hidden)).astype(np.float32)
    w2 = (0.3 * g.standard_normal(hidden)).astype(np.float32)
    return x, y, flat(W1, b1, w2, np.array([0.5], np.float32))


def flat(W1, b1, w2, b2):
    return np.concatenate([np.asarray(W1, np.float64).reshape(-1), np.asarray(b1, np.float64).reshape(-1),
                           np.asarray(w2, np.float64).reshape(-1), np.asarray(b2, np.float64).reshape(-1)])


def unflat(p, C, H=64):
    return p[:H * C].reshape(H, C), p[H * C:H * C + H], p[H * C + H:H * C + 2 * H], p[H * C + 2 * H:]


def train_steps(x, y, params, n_steps, lr, wd, warmup_iters, max_iters, p=0.0, seed=0, rank_weight=0.0, hidden=64, db2=None):
    """``n_steps`` full steps from the flat float64 ``params`` (AdamW state and EMA start as torch's: zeros, a copy), masks from the hash
    at steps 0, 1, ...; the LR of optimiser step k (1-based) is lr * lr_factor(k - 1).  -> list of per-step dicts.
    ``db2``: per step, the value AdamW sees as b2's gradient instead of sum(dscore).  That sum is analytically zero and whatever an
    implementation gets is its rounding noise, which Adam's normalisation turns into a full-size step of either sign; a caller that
    follows another implementation's parameters hands its noise over (the step's own value stays in ``grads``)."""
    x = np.asarray(x, np.float64)
    B, L, C = x.shape
    prm, m, v, ema = params.copy(), np.zeros_like(params), np.zeros_like(params), params.copy()
    out = []
    for k in range(n_steps):
        W1, b1, w2, b2 = unflat(prm, C, hidden)
        m1 = mask(seed, k, 0, p, B * L * C) if p > 0 else None
        m2 = mask(seed, k, 1, p, B * L * hidden) if p > 0 else None
        score, cache = forward(x, W1, b1, w2, b2, m1, m2, p)
        losses, dscore = loss_and_dscore(score, y, rank_weight)
        g = flat(*backward(cache, dscore))
        lr_k = lr * lr_factor(k, warmup_iters, max_iters)
        g_opt = g.copy()
        if db2 is not None:
            g_opt[-1] = db2[k]
        prm, m, v = adamw(prm, g_opt, m, v, lr_k, wd, k + 1)
        ema = ema_update(ema, prm)
        out.append(dict(score=score, losses=np.asarray(losses), dscore=dscore, grads=g, params=prm.copy(), ema=ema.copy(), lr=lr_k))
    return out
