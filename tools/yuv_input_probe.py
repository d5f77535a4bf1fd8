"""End-to-end harness throughput of the two decode-free inputs, same box, alternating: N videos written twice — as uint8 [T,H,W,3]
.npy stacks (3 B/pixel through the host gather and the H2D copy, then a layout pass in HBM) and as .y4m files (I420, 1.5 B/pixel,
converted where the pixels are first touched) — through ViewDecompositionDataset_KVQ -> KSVQE and -> swin_tiny_grpb with the lazily
sampled view, default harness settings.  Also the embedding launch alone for both source kinds (kvq_swin3d_profile).
`python tools/yuv_input_probe.py [N] [T] [H] [W] [rounds] > profiles/yuv_input_probe.txt`"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, yaml  # noqa: E401,E402
import kvq_amd  # noqa: F401,E402
from kvq_amd import _abi, kernels  # noqa: E402
from kvq_amd.trainer import Trainer  # noqa: E402
from kvq_amd.utils import synth  # noqa: E402

N, T, H, W, ROUNDS = (int(sys.argv[i + 1]) if len(sys.argv) > i + 1 else d for i, d in enumerate((24, 100, 540, 960, 3)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = _abi.SRC_I420_BT601_LIMITED
tmp = tempfile.mkdtemp(prefix="kvq_yuv_tree_")
fb = kernels.i420_frame_bytes(H, W)
base = np.random.Generator(np.random.PCG64(5)).integers(0, 256, size=(T, fb), dtype=np.uint8)
for sub in ("npy", "y4m"):
    os.makedirs(os.path.join(tmp, sub))
header = f"YUV4MPEG2 W{W} H{H} F30:1 Ip A1:1 C420jpeg\n".encode()
for i in range(N):
    frames = np.roll(base, 977 * i, axis=1)                      # another video: the same bytes, shifted through the planes
    with open(os.path.join(tmp, "y4m", f"clip{i}.y4m"), "wb") as f:
        f.write(header + b"".join(b"FRAME\n" + fr.tobytes() for fr in frames))
    rgb = kernels.I420Frames(torch.from_numpy(frames).cuda(), H, W, FMT).to_rgb()           # the frames the .y4m reader's consumers see
    np.save(os.path.join(tmp, "npy", f"clip{i}.y4m.npy"), rgb.permute(1, 2, 3, 0).contiguous().cpu().numpy())
for sub in ("npy", "y4m"):
    open(os.path.join(tmp, sub, "anno.txt"), "w").write("".join(f"clip{i}.y4m,1,{i % 5},3.0\n" for i in range(N)))
print(f"{N} videos of {T}x{H}x{W}: .npy RGB {T * H * W * 3 / 1e6:.0f} MB each, .y4m I420 {T * fb / 1e6:.0f} MB each; {ROUNDS} alternating rounds")


def trainer(model, sub):
    if model == "KSVQE":
        cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "Kwai_KSVQE_test.yml")))
        cfg["data"]["val"]["args"].update(anno_file=os.path.join(tmp, sub, "anno.txt"), data_prefix=os.path.join(tmp, sub), seed_per_item=True)
    else:
        cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "kwai_swin_grpb_synthetic_test.yml")))
        tech = cfg["data"]["val"]["args"]["sample_types"]["technical"]
        cfg["data"]["val"] = dict(type="ViewDecompositionDataset_KVQ",
                                  args=dict(anno_file=os.path.join(tmp, sub, "anno.txt"), data_prefix=os.path.join(tmp, sub), phase="test",
                                            sample_types={"technical": tech}, seed_per_item=True))
    tr = Trainer(argparse.Namespace(opt="-", target_set="val", gpu_id="0"), cfg)
    if model == "KSVQE":
        sd = {"KSVQE_backbone." + k: torch.from_numpy(v) for k, v in synth.synth_ksvqe_weights(3).items()}
        sd.update({"KSVQE_head." + k: torch.from_numpy(v) for k, v in synth.synth_vqa_head_weights(768, 64, 3, "stress").items()})
    else:
        c = synth.SWIN_T_GRPB
        sd = {"swin_tiny_grpb_backbone." + k: torch.from_numpy(v) for k, v in synth.synth_swin_weights(c, 0, "stress").items()}
        sd.update({"swin_tiny_grpb_head." + k: torch.from_numpy(v) for k, v in synth.synth_vqa_head_weights(c.num_features, 64, 0, "stress").items()})
    tr.load_weights(_save(sd))
    return tr


def _save(sd):
    path = os.path.join(tmp, "w.pth")
    torch.save(sd, path)
    return path


os.chdir(tmp)
for model in ("KSVQE", "swin_tiny_grpb lazy"):
    trs = {sub: trainer(model.split()[0], sub) for sub in ("npy", "y4m")}
    rates, sums = {"npy": [], "y4m": []}, {}
    for sub, tr in trs.items():                                   # warm: plans, graphs, page cache
        tr._score_all(); torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for sub, tr in trs.items():
            t0 = time.perf_counter(); s = tr._score_all(); torch.cuda.synchronize(); dt = time.perf_counter() - t0
            rates[sub].append(N / dt)
            sums[sub] = float(np.sum(s))
    for sub in ("npy", "y4m"):
        r = rates[sub]
        print(f"{model:20s} {sub}: median {statistics.median(r):7.2f} videos/s  (min {min(r):.2f}, max {max(r):.2f}; rounds "
              + " ".join(f"{v:.2f}" for v in r) + f")  checksum {sums[sub]:.6f}")
    print(f"{model:20s} checksums equal: {sums['npy'] == sums['y4m']}")
    del trs

# the embedding launch alone: 4 clips of 32 frames through the sampler, uint8 planes vs I420 frames
B, Tc = 4, 32
g = torch.Generator().manual_seed(1)
frames = [torch.from_numpy(np.roll(base[:Tc], 31 * b, axis=1)).cuda() for b in range(B)]
i420 = [kernels.I420Frames(f, H, W, FMT) for f in frames]
gh = torch.tensor([min(H // 7 * i, H - 32) for i in range(7)]).view(7, 1, 1)
gw = torch.tensor([min(W // 7 * i, W - 32) for i in range(7)]).view(1, 7, 1)
hs = [(torch.randint(H // 7 - 32, (7, 7, Tc // 8), generator=g) + gh).int().cuda() for _ in range(B)]
ws = [(torch.randint(W // 7 - 32, (7, 7, Tc // 8), generator=g) + gw).int().cuda() for _ in range(B)]
mean, std = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
srcs = {"uint8 planes": kernels.FragmentSource([v.to_rgb() for v in i420], hs, ws, 7, 7, 32, 32, 8, mean=mean, std=std),
        "I420 frames": kernels.FragmentSource(i420, hs, ws, 7, 7, 32, 32, 8, mean=mean, std=std)}
tr = trainer("swin_tiny_grpb", "y4m")
bb, dev = tr.model.swin_tiny_grpb_backbone, torch.device("cuda:0")
with torch.no_grad():
    for _ in range(3):
        for s in srcs.values():
            tr.model(inputs={"technical": s}, reduce_scores=True)
    times = {k: [] for k in srcs}
    for _ in range(10):
        for k, s in srcs.items():                                 # alternating
            bb.profile(B, Tc, 224, 224, dev, True)
            tr.model(inputs={"technical": s}, reduce_scores=True)
            times[k] += [1e3 * r["ms"] for r in bb.profile_read(B, Tc, 224, 224, dev) if r["kind"] == "embed"]
            bb.profile(B, Tc, 224, 224, dev, False)
for k, v in times.items():
    print(f"embedding launch, {B} clips x {Tc} frames of {H}x{W}, {k:12s}: median {statistics.median(v):6.1f} us  (min {min(v):.1f}, max {max(v):.1f}, n {len(v)})")
shutil.rmtree(tmp, ignore_errors=True)
