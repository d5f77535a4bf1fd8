#!/usr/bin/env python
"""The simpleVQAHead training step on the GPU: what one step costs, launch group by launch group, beside a byte floor and beside the
same step done by PyTorch autograd on the same GPU in the same run.  Writes profiles/simple_headtrain_probe.txt (or --out).

  - B = 16, 64 and 256 videos of T = 8 feature rows, C = 9472, hidden 128: the whole step (forward, loss, backward, AdamW + EMA), then
    the forward (3 launches), the loss, the backward (3 launches) and AdamW alone
  - floor, DERIVED from the shape at 6.3 TB/s, not measured.  head: X read twice (forward and backward), W1 read once, dW1 written once,
    (2 B T C + 2 * 128 C) * 4 bytes.  optimiser, listed apart: AdamW + EMA reads p, g, m, v, ema and writes p, m, v, ema of
    128 C + 257 elements, 9 * 4 bytes each.  At small B the optimiser's 1.2 M-parameter pass is the larger of the two.
  - PyTorch: two nn.Linear on the same features, the mean over the frames, the PLCC loss written with torch ops, loss.backward(),
    torch.optim.AdamW and the EMA loop; eager, no graph, the same launches-per-step regime as the HIP step

Every time is the median of three windows of --iters steps between two hipEvents after --warmup steps, in microseconds per step."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import kvq_amd  # noqa: F401
from kvq_amd import kernels

DEV = "cuda:0"
HBM_BPS = 6.3e12
T, C, HID = 8, 9472, 128


def timed(fn, warmup, iters, rounds=3):
    """median of ``rounds`` windows of ``iters`` calls between two hipEvents, after ``warmup`` calls; microseconds per call"""
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


def plcc_torch(s, y):
    sd, m = torch.std_mean(s, unbiased=False)
    a = (s - m) / (sd + 1e-8)
    sdy, my = torch.std_mean(y, unbiased=False)
    t = (y - my) / (sdy + 1e-8)
    rho = torch.mean(a * t)
    return (F.mse_loss(a, t) / 4 + F.mse_loss(rho * a, t) / 4) / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "simple_headtrain_probe.txt"))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("simple_headtrain_probe: no HIP device (times are only ever taken on the GPU)")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:             # rewritten line by line: a run cut short keeps what it measured
            f.write("\n".join(lines) + "\n")

    n = kernels.headtrain_param_count(C, HID)
    floor_opt = 9.0 * n * 4 / HBM_BPS * 1e6
    say(f"device: {kernels.device_name()}   times: median of 3 windows of {args.iters} steps between hipEvents, us per step")
    say(f"T = {T} rows per video, C = {C}, hidden {HID}, fp32, {n} parameters; floors at 6.3 TB/s, derived from the shape, not measured:")
    say("  head = X read twice + W1 read once + dW1 written once;  optimiser = p, g, m, v, ema read and p, m, v, ema written "
        f"= {floor_opt:.1f} us at every B")
    g = torch.Generator(device=DEV).manual_seed(0)
    for B in (16, 64, 256):
        x = torch.randn(B, T, C, device=DEV, generator=g)
        y = torch.rand(B, device=DEV, generator=g) * 4 + 1
        p = torch.cat([0.02 * torch.randn(HID * C, device=DEV, generator=g), 0.1 * torch.randn(HID, device=DEV, generator=g),
                       0.1 * torch.randn(HID, device=DEV, generator=g), torch.zeros(1, device=DEV)]).contiguous()
        m, v, ema, grads = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), p.clone(), torch.empty(n, device=DEV)
        ws = kernels.simple_headtrain_workspace(B, T, C)
        score, out3, dscore = torch.empty(B, device=DEV), torch.empty(3, device=DEV), torch.empty(B, device=DEV)
        it = [0]

        def fwd():
            kernels.simple_headtrain_forward(x, p, ws, score)

        def loss():
            kernels.headtrain_loss(score, y, 0.0, out3, dscore)

        def bwd():
            kernels.simple_headtrain_backward(x, p, ws, dscore, grads)

        def opt():
            kernels.headtrain_adamw(p, grads, m, v, ema, 1e-4, 0.05, it[0] + 1)

        def step():
            fwd()
            loss()
            bwd()
            opt()
            it[0] += 1

        t_step = timed(step, args.warmup, args.iters)
        t_fwd, t_loss, t_bwd, t_opt = (timed(f, args.warmup, args.iters) for f in (fwd, loss, bwd, opt))
        floor_head = (2.0 * B * T * C + 2.0 * HID * C) * 4 / HBM_BPS * 1e6
        floor = floor_head + floor_opt

        # the same step by autograd
        lin1, lin2 = torch.nn.Linear(C, HID).to(DEV), torch.nn.Linear(HID, 1).to(DEV)
        with torch.no_grad():
            lin1.weight.copy_(p[:HID * C].reshape(HID, C))
            lin2.weight.copy_(p[HID * C + HID:HID * C + 2 * HID].reshape(1, HID))
        prm = list(lin1.parameters()) + list(lin2.parameters())
        optim = torch.optim.AdamW(prm, lr=1e-4, weight_decay=0.05)
        ema_t = [q.detach().clone() for q in prm]
        yt = y.reshape(B, 1)

        def t_forward():
            return lin2(lin1(x)).mean(dim=1)

        def t_fb():
            optim.zero_grad(set_to_none=True)
            plcc_torch(t_forward(), yt).backward()

        def t_step_fn():
            t_fb()
            optim.step()
            with torch.no_grad():
                for e, q in zip(ema_t, prm):
                    e.mul_(0.999).add_(q, alpha=1 - 0.999)

        def t_fwd_only():
            with torch.no_grad():
                t_forward()

        tt_step, tt_fb, tt_fwd = (timed(f, args.warmup, args.iters) for f in (t_step_fn, t_fb, t_fwd_only))
        say()
        say(f"B = {B} videos ({B * T} rows, features {B * T * C * 4 / 2 ** 20:.1f} MiB)   floor {floor:6.1f} us = head {floor_head:5.1f} + "
            f"optimiser {floor_opt:4.1f}")
        say(f"  HIP     step {t_step:8.1f} us ({t_step / floor:4.1f}x floor) | forward {t_fwd:7.1f} | loss {t_loss:6.1f} | backward {t_bwd:7.1f} | "
            f"adamw+ema {t_opt:6.1f}")
        say(f"  PyTorch step {tt_step:8.1f} us ({tt_step / floor:4.1f}x floor) | forward {tt_fwd:7.1f} | forward+loss+backward {tt_fb:7.1f} | "
            f"adamw+ema {tt_step - tt_fb:6.1f} (by difference)")
        parts = {"forward": t_fwd, "loss": t_loss, "backward": t_bwd, "adamw+ema": t_opt}
        worst = max(parts, key=parts.get)
        if t_step <= tt_step:
            say(f"  HIP / PyTorch = {t_step / tt_step:4.2f}: the HIP step is not slower; its largest launch group is {worst} ({parts[worst]:.1f} us)")
        else:
            say(f"  HIP / PyTorch = {t_step / tt_step:4.2f}: the HIP step IS SLOWER; {worst} carries the largest share ({parts[worst]:.1f} us; "
                f"PyTorch forward {tt_fwd:.1f}, forward+loss+backward {tt_fb:.1f})")


if __name__ == "__main__":
    main()
