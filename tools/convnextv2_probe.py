#!/usr/bin/env python
"""ConvNeXt-V2 3D (model key conv_v2_tiny) on the GPU: what the GRN launches and the whole forward cost.  Writes
profiles/convnextv2_probe.txt (or --out).

  - kvq_grn_stats (two launches: partial sums of squares, then the per-(b, w) finalize), kvq_grn_apply, and both back to back, on the
    16-bit hidden rows of the four stage shapes of 1 and 4 clips of 32 x 224 x 224 (T = 16 slices, N = 4C), over = th and thw.
    Beside them the byte floor: the hidden rows read twice and written once at 6.3 TB/s.  The floor is DERIVED from the shape, not
    measured; the fp32 partials, the scale table and the launch latencies are on top of it.
  - milliseconds per forward of conv_v2_tiny next to conv_tiny in the same run, 1 and 4 clips

Every time is the median of three windows of --iters launches between two hipEvents after --warmup launches of the same shape, in
microseconds per launch (the forwards: three windows of 20)."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import kvq_amd  # noqa: F401
from kvq_amd import _abi, kernels

DEV = "cuda:0"
STAGES = [(56, 96), (28, 192), (14, 384), (7, 768)]      # (plane, C) of a 224 x 224 clip; T = 16 slices
HBM_BPS = 6.3e12


def timed(fn, warmup, iters, rounds=3):
    """median of ``rounds`` windows of ``iters`` launches between two hipEvents, after ``warmup`` launches; microseconds per launch"""
    for _ in range(warmup):
        fn()
    got = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        got.append(e0.elapsed_time(e1) * 1e3 / iters)
    return sorted(got)[len(got) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "convnextv2_probe.txt"))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("convnextv2_probe: no HIP device (times are only ever taken on the GPU)")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:             # rewritten line by line: a run cut short keeps what it measured
            f.write("\n".join(lines) + "\n")

    lib = _abi.lib()
    say(f"device: {kernels.device_name()}   times: median of 3 windows of {args.iters} launches between hipEvents, us per launch")
    say("floor = hidden rows read twice + written once at 6.3 TB/s: derived from the shape, not measured")
    say()
    g = torch.Generator(device=DEV).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    with torch.no_grad():
        say("GRN on fp16 rows [clips*16*hw*hw][N], in place:  stats (2 launches) | apply | both | floor | both / floor   [us]")
        for over in ("th", "thw"):
            for clips in (1, 4):
                for hw, Cc in STAGES:
                    N = 4 * Cc
                    hid = r(clips * 16 * hw * hw, N).half()
                    gamma, beta = r(N), 0.1 * r(N)
                    ws = torch.empty(lib.kvq_grn_workspace_bytes(clips, 16, hw, hw, N) // 4, device=DEV)
                    a = _abi.KvqGrnArgs()
                    a.x, a.y, a.gamma, a.beta, a.ws = _abi.ptr(hid), None, _abi.ptr(gamma), _abi.ptr(beta), _abi.ptr(ws)
                    a.B, a.D, a.H, a.W, a.N, a.dtype, a.over_w = clips, 16, hw, hw, N, _abi.DT_FP16, int(over == "thw")
                    st = _abi.current_stream()

                    def stats():
                        _abi.check(lib.kvq_grn_stats(C.byref(a), st), "kvq_grn_stats")

                    def apply():
                        _abi.check(lib.kvq_grn_apply(C.byref(a), st), "kvq_grn_apply")

                    def both():
                        stats()
                        apply()
                    gamma.mul_(0.0)                 # scale = 1: the rows stay what they are over the repeated in-place launches
                    beta.mul_(0.0)
                    ts, ta, tb = (timed(f, args.warmup, args.iters) for f in (stats, apply, both))
                    floor = 3.0 * hid.numel() * 2 / HBM_BPS * 1e6
                    say(f"  over {over:3s} clips {clips}  {hw:2d}x{hw:<2d} N {N:4d} ({hid.numel() * 2 / 2 ** 20:6.1f} MiB):  {ts:7.1f} | {ta:7.1f} | "
                        f"{tb:7.1f} | {floor:6.2f} | {tb / floor:5.1f}x")
            say()
        from kvq_amd.models.backbones.conv_backbone import convnext_3d_tiny, convnextv2_3d_tiny
        say("whole forward on clips of 32 x 224 x 224, enqueued eagerly, fp16 operands:  conv_v2_tiny (116 launches) | conv_tiny (62 launches)")
        v2, v1 = convnextv2_3d_tiny().to(DEV).eval(), convnext_3d_tiny(pretrained=False).to(DEV).eval()
        for clips in (1, 4):
            x = r(clips, 3, 32, 224, 224)
            t2 = timed(lambda: v2({"aesthetic": x}), 3, 20)
            t1 = timed(lambda: v1({"aesthetic": x}), 3, 20)
            say(f"  clips {clips}: {t2 / 1e3:7.3f} ms | {t1 / 1e3:7.3f} ms per forward   ({t2 / 1e3 / clips:6.3f} | {t1 / 1e3 / clips:6.3f} ms per clip, "
                f"x{t2 / t1:4.2f})")


if __name__ == "__main__":
    main()
