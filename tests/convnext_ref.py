"""Torch-CPU restatement of the ConvNeXt-3D trunk (model key ``conv_tiny``), written from the layer definitions: stem 2x4x4 conv +
LayerNorm, per stage [LayerNorm + (1,2,2) conv] and blocks of depthwise (kt,7,7) conv -> LayerNorm -> Linear -> GELU -> Linear ->
gamma -> residual add, final LayerNorm (all LayerNorms over C, eps 1e-6, biased variance).

``dtype`` is the arithmetic (float64 = the reference the GPU tests compare against, float32 = what the golden test compares with the
real reference).  ``emul`` (torch.float16 / torch.bfloat16) rounds to that format at exactly the points the HIP path rounds:

    "stem"     the clip and the stem weight (operands of the patch-embedding MFMA)
    "ln1"      the LayerNorm rows entering pwconv1
    "gelu"     the GELU output entering pwconv2
    "down"     the LayerNorm rows entering a downsample conv
    "weights"  pwconv1 / pwconv2 / downsample-conv weights

``points`` restricts the rounding to a subset of these names (to find which rounding carries an error)."""
import torch
import torch.nn.functional as F

POINTS = ("stem", "ln1", "gelu", "down", "weights")
EPS_LN = 1e-6


def _q(t, emul, on=True):
    if emul is None or not on:
        return t
    if emul == torch.float16:
        t = t.clamp(-65504.0, 65504.0)
    return t.to(emul).to(t.dtype)


def _ln(x, w, b):
    """LayerNorm over the last axis"""
    return F.layer_norm(x, (x.shape[-1],), w, b, EPS_LN)


def dwconv_ln(x_cl, w, bias, ln_w, ln_b):
    """x_cl (B, T, H, W, C) channels-last, w (C, 1, kt, 7, 7) -> rows [B*T*H*W, C] = LN_C(dwconv(x) + bias)."""
    kt = w.shape[2]
    y = F.conv3d(x_cl.permute(0, 4, 1, 2, 3), w, bias, padding=(kt // 2, 3, 3), groups=w.shape[0])
    return _ln(y.permute(0, 2, 3, 4, 1), ln_w, ln_b).reshape(-1, w.shape[0])


def block(x_cl, p, emul=None, points=POINTS):
    """One Block3D on a channels-last stream; p: dict with dwconv.weight, dwconv.bias, norm.*, pwconv1.*, pwconv2.*, gamma (or None)."""
    C = x_cl.shape[-1]
    rows = _q(dwconv_ln(x_cl, p["dwconv.weight"], p["dwconv.bias"], p["norm.weight"], p["norm.bias"]), emul, "ln1" in points)
    h = F.gelu(rows @ _q(p["pwconv1.weight"], emul, "weights" in points).t() + p["pwconv1.bias"])
    h = _q(h, emul, "gelu" in points)
    y = h @ _q(p["pwconv2.weight"], emul, "weights" in points).t() + p["pwconv2.bias"]
    if p.get("gamma") is not None:
        y = p["gamma"] * y
    return x_cl + y.reshape(x_cl.shape[:-1] + (C,))


def downsample(x_cl, ln_w, ln_b, w, bias, emul=None, points=POINTS):
    """LayerNorm over C, then the (1,2,2)/(1,2,2) conv; channels-last in and out."""
    rows = _q(_ln(x_cl, ln_w, ln_b), emul, "down" in points)
    y = F.conv3d(rows.permute(0, 4, 1, 2, 3), _q(w, emul, "weights" in points), bias, stride=(1, 2, 2))
    return y.permute(0, 2, 3, 4, 1)


def forward(weights, x, depths=(3, 3, 9, 3), dtype=torch.float64, emul=None, points=POINTS, multi=False, details=False):
    """weights: state_dict-keyed arrays / tensors; x (B, 3, T, H, W).  Returns feat (B, C3, T/2, H/32, W/32) — or the 672-channel
    ``multi`` concatenation — and with ``details`` also (per-stage output norms, per-block ||out - in|| / ||in||)."""
    w = {k: torch.as_tensor(v).to(dtype) for k, v in weights.items()}
    x = torch.as_tensor(x).to(dtype)
    y = F.conv3d(_q(x, emul, "stem" in points), _q(w["downsample_layers.0.0.weight"], emul, "stem" in points),
                 w["downsample_layers.0.0.bias"], stride=(2, 4, 4))
    cur = _ln(y.permute(0, 2, 3, 4, 1), w["downsample_layers.0.1.weight"], w["downsample_layers.0.1.bias"])
    outs, norms, ratios = [], [], []
    for i in range(4):
        if i > 0:
            pre = f"downsample_layers.{i}."
            cur = downsample(cur, w[pre + "0.weight"], w[pre + "0.bias"], w[pre + "1.weight"], w[pre + "1.bias"], emul, points)
        for j in range(depths[i]):
            pre = f"stages.{i}.{j}."
            p = {k[len(pre):]: v for k, v in w.items() if k.startswith(pre)}
            nxt = block(cur, p, emul, points)
            ratios.append(float((nxt - cur).norm() / cur.norm()))
            cur = nxt
        outs.append(cur)
        norms.append(float(cur.norm()))
    if multi:
        size = outs[-1].shape[1:4]
        res = torch.cat([F.interpolate(o.permute(0, 4, 1, 2, 3), size=size, mode="trilinear") for o in outs[:-1]], 1)
    else:
        res = _ln(cur, w["norm.weight"], w["norm.bias"]).permute(0, 4, 1, 2, 3)
    return (res, norms, ratios) if details else res


def head_score(hw, feat):
    """VQAHead in eval mode: mean over tokens of fc_last(gelu(fc_hid(f))); hw: synth_vqa_head_weights."""
    w = {k: torch.as_tensor(v).to(feat.dtype) for k, v in hw.items()}
    f = feat.permute(0, 2, 3, 4, 1)
    h = F.gelu(f @ w["fc_hid.weight"].reshape(w["fc_hid.weight"].shape[0], -1).t() + w["fc_hid.bias"])
    s = h @ w["fc_last.weight"].reshape(w["fc_last.weight"].shape[0], -1).t() + w["fc_last.bias"]
    return s.mean((1, 2, 3))


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())
