"""Emit tests/golden/convnext.npz: what the ConvNeXt-3D tests pin against the real reference.  Runs ONLY where the reference is
present (it is imported through _ref_import.py); the fixture is arrays only.

  <case>/feat, multi      the reference's ConvNeXt3D (full ConvNeXt-T, stress weights) on a PCG64 clip: forward() and forward(multi=True)
  <case>/stage_norms      ||output of stage i||, i = 0..3 (to localise a failure)
  <case>/score            the reference's VQAHead(768, 64) on feat
  <case>/err_fp32, err_fp32_multi, err_emul_fp16, err_emul_bf16, err_emul_fp16_multi, err_emul_bf16_multi
                          rel-L2 of tests/convnext_ref.py against the reference: float32 arithmetic, and float64 arithmetic with
                          the operand roundings of the HIP path
  inflate/<key>           every tensor of a small ConvNeXt3D (dims 8/16/32/64, depths 1/2/1/1) after inflate_weights() of
                          synth_convnext2d_checkpoint

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_convnext_golden.py
"""
import importlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

import kvq_amd  # noqa: F401  (import shim)
from kvq_amd.utils import synth
from _ref_import import import_reference
import convnext_ref as R

# name -> (weight seed, clip seed, B, T, H, W)
CASES = {"A": (11, 21, 2, 8, 64, 64), "B": (12, 22, 1, 16, 96, 128)}
INFLATE = dict(seed=13, dims=(8, 16, 32, 64), depths=(1, 2, 1, 1))
MIN_BLOCK_RATIO = 0.2


def main():
    import_reference()
    cb = importlib.import_module("models.backbones.conv_backbone")
    head_mod = importlib.import_module("models.head")
    torch.manual_seed(0)
    d = {}
    for name, (wseed, cseed, B, T, H, W) in CASES.items():
        wts = synth.synth_convnext_weights(wseed, "stress")
        net = cb.ConvNeXt3D().eval()
        r = net.load_state_dict({k: torch.from_numpy(v) for k, v in wts.items()}, strict=True)
        x = torch.from_numpy(synth.synth_clip(cseed, T, H, W, batch=B))
        norms = []
        hooks = [st.register_forward_hook(lambda m, i, o: norms.append(float(o.norm()))) for st in net.stages]
        with torch.no_grad():
            feat = net({"asesthetic": x})
            for h in hooks:
                h.remove()
            multi = net({"asesthetic": x}, multi=True)
            head = head_mod.VQAHead(768, 64).eval()
            head.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_vqa_head_weights(768, 64, wseed, "stress").items()})
            score = head(feat)
            f64, n64, ratios = R.forward(wts, x, details=True)
            assert min(ratios) >= MIN_BLOCK_RATIO, f"case {name}: a block changes its input by only {min(ratios):.3f}"
            print(f"case {name}: block ratios {min(ratios):.2f}..{max(ratios):.2f}, |feat| <= {float(feat.abs().max()):.2f}, "
                  f"multi {tuple(multi.shape)}")
            d[f"{name}/meta"] = np.asarray([wseed, cseed, B, T, H, W], np.int64)
            d[f"{name}/feat"] = feat.numpy()
            d[f"{name}/multi"] = multi.numpy()
            d[f"{name}/stage_norms"] = np.asarray(norms, np.float64)
            d[f"{name}/score"] = score.numpy().reshape(-1)
            d[f"{name}/err_fp32"] = np.float64(R.rel_l2(R.forward(wts, x, dtype=torch.float32), feat))
            d[f"{name}/err_fp32_multi"] = np.float64(R.rel_l2(R.forward(wts, x, dtype=torch.float32, multi=True), multi))
            for tag, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
                d[f"{name}/err_emul_{tag}"] = np.float64(R.rel_l2(R.forward(wts, x, emul=dt), feat))
                d[f"{name}/err_emul_{tag}_multi"] = np.float64(R.rel_l2(R.forward(wts, x, emul=dt, multi=True), multi))
            print({k: float(v) for k, v in d.items() if k.startswith(name + "/err")}, "score", d[f"{name}/score"])
    net = cb.ConvNeXt3D(depths=list(INFLATE["depths"]), dims=list(INFLATE["dims"]))
    src = {k: torch.from_numpy(v) for k, v in synth.synth_convnext2d_checkpoint(INFLATE["seed"], INFLATE["depths"], INFLATE["dims"]).items()}
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        net.inflate_weights(src)
    for k, v in net.state_dict().items():
        d[f"inflate/{k}"] = v.numpy()
    out = os.path.join(HERE, "convnext.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
