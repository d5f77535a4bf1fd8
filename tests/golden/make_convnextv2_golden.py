"""Emit tests/golden/convnextv2.npz: what the ConvNeXt-V2 3D tests pin against the real reference.  Runs ONLY where the reference is
present (it is imported through _ref_import.py); the fixture is arrays only.

  <case>/feat, multi      the reference's ConvNeXtV23D (full ConvNeXt-V2-T, stress weights) on a PCG64 clip: forward() and forward(multi=True)
  <case>/stage_norms      ||output of stage i||, i = 0..3 (to localise a failure)
  <case>/score            the reference's VQAHead(768, 64) on feat
  <case>/err_fp32, err_fp32_multi, err_emul_fp16, err_emul_bf16, err_emul_fp16_multi, err_emul_bf16_multi
                          rel-L2 of tests/convnextv2_ref.py against the reference: float32 arithmetic, and float64 arithmetic with
                          the operand roundings of the HIP path
  <case>/err_emul_fp16_score, err_emul_bf16_score
                          |score of the emulation - score of the float64 restatement|, the head in float64
  <case>/err_thw          rel-L2 of the float64 restatement with GRN over (T, H, W) against the reference's feat: how far apart the two
                          definitions are on this case
  keys, shapes            the reference model's state_dict key names and shapes (shapes padded with 0 to 5 axes)
  inflate/<key>           every tensor of a small ConvNeXtV23D (dims 8/16/32/64, depths 1/2/1/1, 10 classes) after inflate_weights() of
                          synth_convnextv2_2d_checkpoint, written to a temporary file (the method takes a path)
  grn/<i>/x, gamma, beta, y   the reference GRN module's own output on two small 5-D inputs (float64)

The generator asserts what keeps the fixture from hiding a failure: every block changes its input by >= 0.2 in relative norm, in every
block the GRN term gamma * x * Nx + beta is >= 0.2 of ||x||, GRN over (T, H, W) misses the reference's feat by >= 10 x err_emul_fp16,
and fp16 operand rounding alone moves the score by <= 0.5e-3 (otherwise the GPU test's 1e-3 score gate would measure the draw).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_convnextv2_golden.py
"""
import contextlib
import importlib
import io
import os
import sys
import tempfile

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
import convnextv2_ref as R

# name -> (weight seed, clip seed, B, T, H, W)
# Weight seed of A: 31 was drawn first; there the float64 restatement with fp16 operand roundings alone moves the score by 9.1e-4 (fp16
# rounding of the weights: 8.8e-4), which leaves the 1e-3 score gate of the GPU test no room to measure the kernels (the draws 34..37
# give 1.5e-4, 1.2e-4, 8.0e-4, 4.3e-4).  34 is the next seed that passes MAX_EMUL_SCORE below; the rule looks at the restatement only.
CASES = {"A": (34, 41, 2, 8, 64, 64), "B": (32, 42, 1, 16, 96, 128)}
INFLATE = dict(seed=33, dims=(8, 16, 32, 64), depths=(1, 2, 1, 1), num_classes=10)
GRN_CASES = [(51, (2, 3, 4, 5, 6)), (52, (1, 2, 1, 3, 8))]
MIN_BLOCK_RATIO = 0.2
MIN_GRN_RATIO = 0.2
MIN_AXES_GAP = 10.0
MAX_EMUL_SCORE = 0.5e-3       # |score(fp16 emulation) - score(float64)|: half of the 1e-3 gate the GPU test puts on the fp16 score


def main():
    import_reference()
    cb = importlib.import_module("models.backbones.conv_backbone")
    head_mod = importlib.import_module("models.head")
    torch.manual_seed(0)
    d = {}
    for name, (wseed, cseed, B, T, H, W) in CASES.items():
        wts = synth.synth_convnextv2_weights(wseed, "stress")
        net = cb.convnextv2_tiny().eval()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in wts.items()}, strict=True)
        x = torch.from_numpy(synth.synth_clip(cseed, T, H, W, batch=B))
        norms = []
        hooks = [st.register_forward_hook(lambda m, i, o: norms.append(float(o.norm()))) for st in net.stages]
        with torch.no_grad():
            feat = net({"aesthetic": x})
            for h in hooks:
                h.remove()
            multi = net({"aesthetic": x}, multi=True)
            head = head_mod.VQAHead(768, 64).eval()
            head.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_vqa_head_weights(768, 64, wseed, "stress").items()})
            score = head(feat)
            f64, n64, ratios, terms = R.forward(wts, x, details=True)
            assert min(ratios) >= MIN_BLOCK_RATIO, f"case {name}: a block changes its input by only {min(ratios):.3f}"
            assert min(terms) >= MIN_GRN_RATIO, f"case {name}: a GRN term is only {min(terms):.3f} of its input"
            print(f"case {name}: block ratios {min(ratios):.2f}..{max(ratios):.2f}, GRN terms {min(terms):.2f}..{max(terms):.2f}, "
                  f"|feat| <= {float(feat.abs().max()):.2f}, multi {tuple(multi.shape)}")
            d[f"{name}/meta"] = np.asarray([wseed, cseed, B, T, H, W], np.int64)
            d[f"{name}/feat"] = feat.numpy()
            d[f"{name}/multi"] = multi.numpy()
            d[f"{name}/stage_norms"] = np.asarray(norms, np.float64)
            d[f"{name}/score"] = score.numpy().reshape(-1)
            d[f"{name}/err_fp32"] = np.float64(R.rel_l2(R.forward(wts, x, dtype=torch.float32), feat))
            d[f"{name}/err_fp32_multi"] = np.float64(R.rel_l2(R.forward(wts, x, dtype=torch.float32, multi=True), multi))
            hw = synth.synth_vqa_head_weights(768, 64, wseed, "stress")
            for tag, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
                fe = R.forward(wts, x, emul=dt)
                d[f"{name}/err_emul_{tag}"] = np.float64(R.rel_l2(fe, feat))
                d[f"{name}/err_emul_{tag}_score"] = np.float64((R.head_score(hw, fe) - R.head_score(hw, f64)).abs().max())
                d[f"{name}/err_emul_{tag}_multi"] = np.float64(R.rel_l2(R.forward(wts, x, emul=dt, multi=True), multi))
            assert float(d[f"{name}/err_emul_fp16_score"]) <= MAX_EMUL_SCORE, \
                f"case {name}: fp16 operand rounding alone moves the score by {float(d[f'{name}/err_emul_fp16_score']):.2e}"
            d[f"{name}/err_thw"] = np.float64(R.rel_l2(R.forward(wts, x, axes="thw"), feat))
            gap = float(d[f"{name}/err_thw"]) / float(d[f"{name}/err_emul_fp16"])
            assert gap >= MIN_AXES_GAP, f"case {name}: GRN over (T, H, W) is only {gap:.1f} x err_emul_fp16 away from the reference"
            print({k: float(v) for k, v in d.items() if k.startswith(name + "/err")}, "score", d[f"{name}/score"])
    sd = cb.convnextv2_tiny().state_dict()
    d["keys"] = np.asarray(list(sd))
    d["shapes"] = np.asarray([tuple(v.shape) + (0,) * (5 - v.dim()) for v in sd.values()], np.int64)
    net = cb.ConvNeXtV23D(depths=list(INFLATE["depths"]), dims=list(INFLATE["dims"]), num_classes=INFLATE["num_classes"])
    src = synth.synth_convnextv2_2d_checkpoint(INFLATE["seed"], INFLATE["depths"], INFLATE["dims"], INFLATE["num_classes"])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "convnextv2_2d.pt")
        torch.save({"model": {k: torch.from_numpy(v) for k, v in src.items()}}, path)
        with contextlib.redirect_stdout(io.StringIO()):
            net.inflate_weights(path)
    for k, v in net.state_dict().items():
        d[f"inflate/{k}"] = v.numpy()
    for i, (seed, shape) in enumerate(GRN_CASES):
        g = np.random.Generator(np.random.PCG64(seed))
        m = cb.GRN(shape[-1]).double()
        x = torch.from_numpy(g.standard_normal(shape))
        with torch.no_grad():
            m.gamma.copy_(torch.from_numpy(g.uniform(-1.5, 1.5, (1, 1, 1, shape[-1]))))
            m.beta.copy_(torch.from_numpy(0.2 * g.standard_normal((1, 1, 1, shape[-1]))))
            if i == 1:
                x[..., 3] = 0.0                 # an all-zero channel: Gx = 0 there
            y = m(x)
        d[f"grn/{i}/x"], d[f"grn/{i}/gamma"], d[f"grn/{i}/beta"], d[f"grn/{i}/y"] = x.numpy(), m.gamma.detach().numpy(), m.beta.detach().numpy(), y.numpy()
    out = os.path.join(HERE, "convnextv2.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
