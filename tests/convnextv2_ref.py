"""Torch-CPU restatement of the ConvNeXt-V2 3D trunk (model key ``conv_v2_tiny``), written from the layer definitions on top of
tests/convnext_ref.py: the stem, the downsample layers and the final LayerNorm are ConvNeXt-3D's; a block is depthwise (kt,7,7) conv ->
LayerNorm -> Linear -> GELU -> GRN -> Linear -> residual add, without a layer scale.

GRN on the channels-last hidden tensor x (B, T, H, W, N):

    Gx = sqrt(sum of x^2 over ``axes``)         axes = "th": (T, H) — one norm per (b, w, n), what the reference's 2D GRN module
    Nx = Gx / (mean over n of Gx + 1e-6)        computes on a 5-D tensor (torch.norm(dim=(1, 2))); "thw": (T, H, W), one per (b, n)
    y  = gamma * (x * Nx) + beta + x

``emul`` rounds where the HIP path rounds: ConvNeXt-3D's points plus "grn", the GRN output entering pwconv2 (the GELU output it reads
is rounded too: point "gelu")."""
import torch
import torch.nn.functional as F

from convnext_ref import EPS_LN, _ln, _q, downsample, dwconv_ln, head_score, rel_l2  # noqa: F401

POINTS = ("stem", "ln1", "gelu", "grn", "down", "weights")
AXES = {"th": (1, 2), "thw": (1, 2, 3)}


def grn_parts(x, gamma, beta, axes="th"):
    """x (B, T, H, W, N) -> (Nx broadcastable to x, the GRN term gamma * x * Nx + beta)"""
    gx = (x * x).sum(AXES[axes], keepdim=True).sqrt()
    nx = gx / (gx.mean(-1, keepdim=True) + 1e-6)
    return nx, gamma.reshape(-1) * (x * nx) + beta.reshape(-1)


def grn(x, gamma, beta, axes="th"):
    return grn_parts(x, gamma, beta, axes)[1] + x


def block(x_cl, p, emul=None, points=POINTS, axes="th", details=False):
    """One BlockV23D on a channels-last stream; p: dwconv.*, norm.*, pwconv1.*, grn.gamma, grn.beta, pwconv2.*"""
    C = x_cl.shape[-1]
    rows = _q(dwconv_ln(x_cl, p["dwconv.weight"], p["dwconv.bias"], p["norm.weight"], p["norm.bias"]), emul, "ln1" in points)
    h = F.gelu(rows @ _q(p["pwconv1.weight"], emul, "weights" in points).t() + p["pwconv1.bias"])
    h = _q(h, emul, "gelu" in points).reshape(x_cl.shape[:-1] + (4 * C,))
    _, term = grn_parts(h, p["grn.gamma"], p["grn.beta"], axes)
    g = _q(term + h, emul, "grn" in points)
    y = g.reshape(-1, 4 * C) @ _q(p["pwconv2.weight"], emul, "weights" in points).t() + p["pwconv2.bias"]
    out = x_cl + y.reshape(x_cl.shape)
    return (out, float(term.norm() / h.norm())) if details else out


def forward(weights, x, depths=(3, 3, 9, 3), dtype=torch.float64, emul=None, points=POINTS, multi=False, details=False, axes="th"):
    """weights: state_dict-keyed arrays / tensors (``head.*`` is ignored); x (B, 3, T, H, W).  Returns feat or the 672-channel ``multi``
    concatenation — with ``details`` also (per-stage output norms, per-block ||out - in|| / ||in||, per-block ||GRN term|| / ||x||)."""
    w = {k: torch.as_tensor(v).to(dtype) for k, v in weights.items() if not k.startswith("head.")}
    x = torch.as_tensor(x).to(dtype)
    y = F.conv3d(_q(x, emul, "stem" in points), _q(w["downsample_layers.0.0.weight"], emul, "stem" in points),
                 w["downsample_layers.0.0.bias"], stride=(2, 4, 4))
    cur = _ln(y.permute(0, 2, 3, 4, 1), w["downsample_layers.0.1.weight"], w["downsample_layers.0.1.bias"])
    outs, norms, ratios, terms = [], [], [], []
    for i in range(4):
        if i > 0:
            pre = f"downsample_layers.{i}."
            cur = downsample(cur, w[pre + "0.weight"], w[pre + "0.bias"], w[pre + "1.weight"], w[pre + "1.bias"], emul, points)
        for j in range(depths[i]):
            pre = f"stages.{i}.{j}."
            p = {k[len(pre):]: v for k, v in w.items() if k.startswith(pre)}
            nxt, term = block(cur, p, emul, points, axes, details=True)
            ratios.append(float((nxt - cur).norm() / cur.norm()))
            terms.append(term)
            cur = nxt
        outs.append(cur)
        norms.append(float(cur.norm()))
    if multi:
        size = outs[-1].shape[1:4]
        res = torch.cat([F.interpolate(o.permute(0, 4, 1, 2, 3), size=size, mode="trilinear") for o in outs[:-1]], 1)
    else:
        res = _ln(cur, w["norm.weight"], w["norm.bias"]).permute(0, 4, 1, 2, 3)
    return (res, norms, ratios, terms) if details else res
