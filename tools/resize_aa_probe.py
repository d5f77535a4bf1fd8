"""Antialiased bilinear resize (kvq_resize_bilinear_aa) against the plain one (kvq_resize_bilinear) on the same uint8 frames, one
MI355X: µs per launch from HIP events over a block of back-to-back launches, and GB/s counted as the source bytes (each read once)
plus the fp32 output.  `python tools/resize_aa_probe.py [iters] [out.txt]`.

  KSVQE key frames:  3 x 32 x 1080 x 1920 -> 112 x 112, CLIP-normalised
  SimpleVQA view:    3 x 8 x 1080 x 1920 -> 520 x 520, centre crop 448, ImageNet constants on 0-255 pixels
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import kvq_amd  # noqa: E402,F401
from kvq_amd import kernels  # noqa: E402
from kvq_amd.datasets import SIMPLEVQA_MEAN, SIMPLEVQA_STD  # noqa: E402

IT = int(sys.argv[1]) if len(sys.argv) > 1 else 200
OUT = sys.argv[2] if len(sys.argv) > 2 else None
CLIP_MEAN = tuple(255.0 * m for m in (0.48145466, 0.4578275, 0.40821073))
CLIP_STD = tuple(255.0 * s for s in (0.26862954, 0.26130258, 0.27577711))
CASES = [("ksvqe 3x32x1080x1920 -> 112^2", (3, 32, 1080, 1920), (112, 112), None, CLIP_MEAN, CLIP_STD),
         ("simplevqa 3x8x1080x1920 -> 520^2 / crop 448", (3, 8, 1080, 1920), (520, 520), (36, 36, 448, 448), SIMPLEVQA_MEAN,
          SIMPLEVQA_STD)]


def time_us(fn, it):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(it):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / it


def main():
    assert torch.cuda.is_available(), "the probe needs a GPU"
    lines = [f"device: {kernels.device_name()}  iters: {IT}"]
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, shape, rs, crop, mean, std in CASES:
        v = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
        oh, ow = (crop[2], crop[3]) if crop else rs
        nbytes = v.numel() + shape[0] * shape[1] * oh * ow * 4
        res = {}
        for aa in (False, True):
            us = time_us(lambda: kernels.resize_bilinear(v, rs[0], rs[1], crop=crop, mean=mean, std=std, antialias=aa), IT)
            res[aa] = us
            lines.append(f"{name:46s} {'antialias' if aa else 'plain    '}  {us:9.1f} us  {nbytes / us / 1e3:7.1f} GB/s "
                         f"(source read once + fp32 out: {nbytes / 1e6:.1f} MB)")
        lines.append(f"{name:46s} antialias / plain = {res[True] / res[False]:.2f}x")
    text = "\n".join(lines)
    print(text)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
