#!/usr/bin/env python
"""Measurements of the local quality maps (record: profiles/quality_map_probe.txt).

    python tools/quality_map_probe.py paint       # the paint launch alone: 8 clips x 16 depth slices of 1080p, cell 1 and 8
    python tools/quality_map_probe.py noise       # CPU: summation-order noise of the head's map (max |fp32 - fp64|), no GPU
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/quality_map_probe.py head    # the head with / without the map, in its own run
    python tools/quality_map_probe.py e2e         # videos/s of config/kwai_swin_grpb_qmap_test.yml with / without quality_maps,
                                                  # one process, the two configurations alternating, three runs each
    python tools/quality_map_probe.py ksvqe       # samples/s of KSVQE on a fake decoded-frame tree: config/Kwai_KSVQE_test.yml (what the
                                                  # parent commit runs), config/Kwai_KSVQE_qmap_test.yml without and with its key
"""
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kvq_amd  # noqa: E402,F401
from kvq_amd import kernels  # noqa: E402
from kvq_amd.utils import synth  # noqa: E402

COPY_RATE = 6.3e12        # B/s: the measured device copy rate the stores are judged against


def paint():
    n, T, H, W, Fh, Fw, fs, aligned = 8, 32, 1080, 1920, 7, 7, 32, 8
    g = torch.Generator().manual_seed(1)
    video = torch.randint(0, 256, (3, T, H, W), dtype=torch.uint8, generator=g).cuda()
    grid_h = torch.tensor([min(H // Fh * i, H - fs) for i in range(Fh)]).view(-1, 1, 1)
    grid_w = torch.tensor([min(W // Fw * i, W - fs) for i in range(Fw)]).view(1, -1, 1)
    hs = [(torch.randint(0, H // Fh - fs, (Fh, Fw, T // aligned), generator=g) + grid_h).int().cuda() for _ in range(n)]
    ws = [(torch.randint(0, W // Fw - fs, (Fh, Fw, T // aligned), generator=g) + grid_w).int().cuda() for _ in range(n)]
    src = kernels.FragmentSource([video] * n, hs, ws, Fh, Fw, fs, fs, aligned)
    tok = torch.randn(n, T // 2, 7, 7, generator=g).cuda()
    print(f"paint: {n} clips x {T // 2} depth slices of {H}x{W}, 7x7 tokens per slice (coverage {49 * 32 * 32 / (H * W):.4f})")
    for cell in (1, 8):
        heat, cover = kernels.quality_paint(src, tok, cell=cell)
        torch.cuda.synchronize()
        reps = 20 if cell == 1 else 200
        t = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                kernels.quality_paint(src, tok, cell=cell)
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3 / reps)
        stored = 2 * heat.numel() * 4
        us = min(t)
        print(f"  cell {cell}: {us:9.1f} us per launch (runs {', '.join(f'{v:.1f}' for v in t)}; allocation of the outputs included), "
              f"{stored / 1e6:8.1f} MB stored, {stored / us * 1e6 / 1e12:.3f} TB/s = {100 * stored / us * 1e6 / COPY_RATE:.1f} % of the "
              f"{COPY_RATE / 1e12:.1f} TB/s copy rate; mean cover {float(cover.mean()):.4f}")


def _head_case():
    feat = np.random.Generator(np.random.PCG64(5)).standard_normal((2, 768, 4, 7, 7)).astype(np.float32)
    return feat, synth.synth_vqa_head_weights(768, 64, 5, "stress")


def noise():
    """CPU evaluation of the head on the fixture feature in fp32 and fp64: the largest difference over the per-token map"""
    feat, w = _head_case()
    def run(dt):
        f = torch.from_numpy(feat).to(dt).permute(0, 2, 3, 4, 1).reshape(-1, 768)
        w1, b1 = torch.from_numpy(w["fc_hid.weight"]).to(dt).reshape(64, 768), torch.from_numpy(w["fc_hid.bias"]).to(dt)
        w2, b2 = torch.from_numpy(w["fc_last.weight"]).to(dt).reshape(1, 64), torch.from_numpy(w["fc_last.bias"]).to(dt)
        return (torch.nn.functional.gelu(f @ w1.t() + b1) @ w2.t() + b2).double()
    print(f"head map, CPU: max |fp32 - fp64| = {float((run(torch.float32) - run(torch.float64)).abs().max()):.6e} over {2 * 196} tokens")


def head():
    feat, w = _head_case()
    w = {k: torch.from_numpy(v).cuda() for k, v in w.items()}
    x = torch.from_numpy(feat).cuda().permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)      # channels-last: the MFMA kernel
    a = (x, w["fc_hid.weight"], w["fc_hid.bias"], w["fc_last.weight"].reshape(-1), w["fc_last.bias"])
    for _ in range(50):
        kernels.vqa_head(*a)
    torch.cuda.synchronize()
    for _ in range(50):
        kernels.vqa_head(*a, return_map=True)
    torch.cuda.synchronize()
    print("head: 50 calls without the map (vqa_head_mfma_kernel + mean_rows_kernel), 50 with (vqa_head_mfma_kernel + mean_rows_map_kernel)")


def e2e():
    import yaml
    from kvq_amd.trainer import Trainer
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "kwai_swin_grpb_qmap_test.yml")))
    cfg["data"]["val"]["args"].update(num_videos=12, seed_per_item=True)
    work = tempfile.mkdtemp(prefix="qmap_probe_")
    os.chdir(work)
    cfg["quality_maps"]["dir"] = os.path.join(work, "maps")
    plain = {k: v for k, v in cfg.items() if k != "quality_maps"}
    trainers = {}
    for name, c in (("without", plain), ("with", cfg)):
        torch.manual_seed(0)
        trainers[name] = Trainer(types.SimpleNamespace(gpu_id="0"), c)
        trainers[name].inferece_test()                   # records the lanes' graphs, builds the weight images
    n = len(trainers["with"].val_dataset)
    rates = {"without": [], "with": []}
    for _ in range(3):
        for name in ("without", "with"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainers[name].inferece_test()
            torch.cuda.synchronize()
            rates[name].append(n / (time.perf_counter() - t0))
    for name in ("without", "with"):
        r = rates[name]
        print(f"e2e {name:8s} quality_maps: {np.median(r):7.2f} videos/s (runs {', '.join(f'{v:.2f}' for v in r)}; spread "
              f"{100 * (max(r) - min(r)) / np.median(r):.1f} %), graph_stats {getattr(trainers[name], 'graph_stats', None)}")
    print(f"e2e with / without: {np.median(rates['with']) / np.median(rates['without']):.3f}  ({n} videos of 256 frames 540x960, 8 clips each; "
          "dataset synthesis on the host included)")


def ksvqe():
    """KSVQE end to end on N uint8 [T,H,W,3] .npy stacks (96-frame samples, one clip per forward): the yml without the key and with
    `lazy: false` enqueues what it enqueued before this feature; `lazy: true` alone moves the sampling into the lazy path; the key adds
    the head's map launch, the region paint and the npz writer.  One process, the configurations alternating, three runs each."""
    import yaml
    from kvq_amd.trainer import Trainer
    N, T, H, W = 8, 100, 540, 960
    work = tempfile.mkdtemp(prefix="qmap_ksvqe_probe_")
    base = np.random.Generator(np.random.PCG64(5)).integers(0, 256, size=(T, H, W, 3), dtype=np.uint8)
    for i in range(N):
        np.save(os.path.join(work, f"clip{i}.mp4.npy"), np.roll(base, i, axis=1))
    open(os.path.join(work, "anno.txt"), "w").write("".join(f"clip{i}.mp4,1,{i % 5},3.0\n" for i in range(N)))
    os.chdir(work)
    sd = {"KSVQE_backbone." + k: torch.from_numpy(v) for k, v in synth.synth_ksvqe_weights(3).items()}
    sd.update({"KSVQE_head." + k: torch.from_numpy(v) for k, v in synth.synth_vqa_head_weights(768, 64, 3, "stress").items()})

    def config(name, key):
        cfg = yaml.safe_load(open(os.path.join(ROOT, "config", name)))
        cfg["data"]["val"]["args"].update(anno_file=os.path.join(work, "anno.txt"), data_prefix=work)
        if key:
            cfg["quality_maps"]["dir"] = os.path.join(work, "maps")
        else:
            cfg.pop("quality_maps", None)
        return cfg

    legs = (("Kwai_KSVQE_test.yml (lazy: false, no key)", config("Kwai_KSVQE_test.yml", False)),
            ("qmap yml without the key (lazy: true)", config("Kwai_KSVQE_qmap_test.yml", False)),
            ("qmap yml with the key (cell 8)", config("Kwai_KSVQE_qmap_test.yml", True)))
    trainers = {}
    for name, cfg in legs:
        trainers[name] = Trainer(types.SimpleNamespace(gpu_id="0"), cfg)
        trainers[name].model.load_state_dict(sd, strict=False)
        trainers[name].inferece_test()                   # records the lanes' graphs, builds the weight images, warms the page cache
    rates = {name: [] for name, _ in legs}
    for _ in range(3):
        for name, _ in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainers[name].inferece_test()
            torch.cuda.synchronize()
            rates[name].append(N / (time.perf_counter() - t0))
    print(f"ksvqe: {N} videos of {T} x {H} x {W}, one 96-frame sample each, decode (np.load) and H2D included")
    for name, _ in legs:
        r = rates[name]
        print(f"  {name:44s} {np.median(r):7.2f} samples/s (runs {', '.join(f'{v:.2f}' for v in r)}; spread "
              f"{100 * (max(r) - min(r)) / np.median(r):.1f} %), graph_stats {getattr(trainers[name], 'graph_stats', None)}")
    first = np.median(rates[legs[0][0]])
    print("  ratios to the first line: " + ", ".join(f"{np.median(rates[name]) / first:.3f}" for name, _ in legs[1:]))
    z = np.load(os.path.join(work, "maps", "clip0.mp4.npz"))
    print("  clip0.mp4.npz: " + ", ".join(f"{k} {z[k].shape}" for k in z.files))


if __name__ == "__main__":
    {"paint": paint, "noise": noise, "head": head, "e2e": e2e, "ksvqe": ksvqe}[sys.argv[1] if len(sys.argv) > 1 else "paint"]()
