#!/usr/bin/env python
"""ConvNeXt-3D (model key conv_tiny) on the GPU: what its two new launches and the whole forward cost, next to PyTorch-ROCm
running the same operators on the same device.  Writes profiles/convnext_probe.txt (or --out).

  - kvq_dwconv3d_ln at the four stage shapes of 1 and 4 clips of 32 x 224 x 224, kt = 1 and 3, fp16 rows out; beside it
    F.conv3d(groups=C) + F.layer_norm in fp32 and under fp16 autocast, and two floors derived from the shape: the FMAs at the
    157 TFLOP/s vector peak and the bytes (stream read once, 16-bit rows written once, weights) at 6.3 TB/s
  - the scaled-residual GEMM (kvq_gemm_resid_scaled) next to plain KVQ_EPI_RESID_F32 at the same shapes (M tokens, N = C, K = 4C)
  - milliseconds per clip of the whole forward, 1 and 4 clips

Every time is the mean of --iters launches between two hipEvents after --warmup launches of the same shape, in microseconds."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import kvq_amd  # noqa: F401
from kvq_amd import _abi, kernels

DEV = "cuda:0"
STAGES = [(56, 96), (28, 192), (14, 384), (7, 768)]      # (plane, C) of a 224 x 224 clip; T = 16 slices
VALU_FLOPS, HBM_BPS = 157e12, 6.3e12


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "convnext_probe.txt"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("convnext_probe: no HIP device (times are only ever taken on the GPU)")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:             # rewritten line by line: a run cut short keeps what it measured
            f.write("\n".join(lines) + "\n")

    say(f"device: {kernels.device_name()}   times: mean of {args.iters} launches between hipEvents, us")
    say()
    g = torch.Generator(device=DEV).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    cases = [(clips, hw, Cc, kt) for clips in (1, 4) for hw, Cc in STAGES for kt in (1, 3)]

    def dw_inputs(clips, hw, Cc, kt):
        return r(clips, 16, hw, hw, Cc), r(Cc, 1, kt, 7, 7) / (49 * kt) ** 0.5, r(Cc), r(Cc), r(Cc)

    ours = {}
    with torch.no_grad():
        say("kvq_dwconv3d_ln, depthwise (kt,7,7) conv + LayerNorm, T = 16, fp16 rows out:  time | VALU floor | HBM floor   [us]")
        for case in cases:
            clips, hw, Cc, kt = case
            x, w, b, lw, lb = dw_inputs(*case)
            wt = kernels.dwconv_weight_taps(w)
            ours[case] = timed(lambda: kernels.dwconv3d_ln(x, wt, b, lw, lb, eps=1e-6, out_dtype=torch.float16), args.warmup, args.iters)
            tokens = clips * 16 * hw * hw
            fl = 2.0 * tokens * Cc * 49 * kt / VALU_FLOPS * 1e6
            by = (tokens * Cc * 6.0 + 49 * kt * Cc * 4.0) / HBM_BPS * 1e6
            say(f"  clips {clips}  {hw:2d}x{hw:<2d} C {Cc:3d} kt {kt}:  {ours[case]:8.1f} | {fl:6.2f} | {by:6.2f}")
        say()
        say("pwconv2 residual GEMM (M tokens, N = C, K = 4C, fp16 operands):  scaled (kvq_gemm_resid_scaled) | plain KVQ_EPI_RESID_F32   [us]")
        for clips in (1, 4):
            for hw, Cc in STAGES:
                M = clips * 16 * hw * hw
                A, W = r(M, 4 * Cc).half(), (r(Cc, 4 * Cc) / (4 * Cc) ** 0.5).half()
                b, s, out = r(Cc), r(Cc), torch.zeros(M, Cc, device=DEV)
                ts = timed(lambda: kernels.gemm(A, W, b, _abi.EPI_RESID_F32, out=out, col_scale=s), args.warmup, args.iters)
                tp = timed(lambda: kernels.gemm(A, W, b, _abi.EPI_RESID_F32, out=out), args.warmup, args.iters)
                say(f"  clips {clips}  M {M:6d} N {Cc:3d} K {4 * Cc:4d}:  {ts:8.1f} | {tp:8.1f}")
        say()
        from kvq_amd.models.backbones.conv_backbone import convnext_3d_tiny
        net = convnext_3d_tiny(pretrained=False).to(DEV).eval()
        say("whole forward, ConvNeXt-T on clips of 32 x 224 x 224 (62 launches, enqueued eagerly), fp16 operands:")
        for clips in (1, 4):
            x = r(clips, 3, 32, 224, 224)
            t = timed(lambda: net({"aesthetic": x}), 3, 10)
            say(f"  clips {clips}: {t / 1e3:7.3f} ms per forward = {t / 1e3 / clips:7.3f} ms per clip")
        del net
        say()
        say("the same operator by PyTorch-ROCm, F.conv3d(groups=C) + F.layer_norm:  fp32 | fp16 autocast | kvq_dwconv3d_ln   [us]")
        for case in cases:
            clips, hw, Cc, kt = case
            x, w, b, lw, lb = dw_inputs(*case)
            xcf = x.permute(0, 4, 1, 2, 3).contiguous()

            def ref():
                y = F.conv3d(xcf, w, b, padding=(kt // 2, 3, 3), groups=Cc)
                return F.layer_norm(y.permute(0, 2, 3, 4, 1), (Cc,), lw, lb, 1e-6)

            def ref16():
                with torch.autocast("cuda", dtype=torch.float16):
                    return ref()
            t32, t16 = timed(ref, args.warmup, args.iters), timed(ref16, args.warmup, args.iters)
            say(f"  clips {clips}  {hw:2d}x{hw:<2d} C {Cc:3d} kt {kt}:  {t32:8.1f} | {t16:8.1f} | {ours[case]:8.1f}"
                + ("   kvq SLOWER than torch" if ours[case] > min(t32, t16) else ""))


if __name__ == "__main__":
    main()
