"""Motion-JPEG output, measured (profiles/mjpeg_write_probe.txt):
  1. the forward-DCT launch (kvq_jpeg_fdct) on 32 frames of 1080 x 1920 from both source kinds, hipEvent brackets, n = 30, against its
     byte floor — 4.5 B/pixel from I420 (1.5 read, 3 written), 6 B/pixel from RGB (3 read, 3 written) over the 6.3 TB/s a streaming
     kernel achieves on this chip — and against the IDCT launch (kvq_jpeg_idct_i420) on the same frames in the same run;
  2. the host entropy coder (kvq_jpeg_encode) on those frames at q50 / q75 / q90: frames/s and compressed MB/s on ONE thread;
  3. videos/s of the Swin harness loop (config/kwai_swin_grpb_qmap_test.yml, 2 overlays per clip) without quality maps, with the
     overlays in the .npz, and with ``overlay_video: avi``, alternating rounds, checksums compared.
Frames are a seeded gradient + noise picture that drifts from frame to frame.
`python tools/mjpeg_write_probe.py [N] [rounds] > profiles/mjpeg_write_probe.txt`"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, yaml  # noqa: E401,E402
import kvq_amd  # noqa: F401,E402
from kvq_amd import _abi, kernels  # noqa: E402
from kvq_amd.trainer import Trainer  # noqa: E402

N, ROUNDS = (int(sys.argv[i + 1]) if len(sys.argv) > i + 1 else d for i, d in enumerate((12, 3)))
HBM = 6.3e12
H, W, T = 1080, 1920, 32


def picture(h, w, seed, shift):
    g = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([255.0 * ((x + shift) % w) / w, 255.0 * y / h, 127.5 + 127.5 * np.sin((x + y + shift) / 37.0)])
    return np.clip(base + g.normal(0, 10, (3, h, w)), 0, 255).astype(np.uint8)


def timed(fn, n=30, warm=5):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def line(what, ms, nbytes):
    med, floor = statistics.median(ms), nbytes / HBM * 1e3
    return (f"{what}: {nbytes / 1e6:.1f} MB moved; median {med:.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}, n {len(ms)}) = "
            f"{nbytes / med / 1e9:.2f} TB/s; byte floor at 6.3 TB/s {floor:.4f} ms -> {100 * floor / med:.0f}% of the floor rate")


print(f"device: {kernels.device_name()}")

# ---- 1. the FDCT launch from both sources against its byte floor and against the IDCT launch ----------------------------------------
base = [picture(H, W, 10 + k, 0) for k in range(4)]
rgb_host = np.stack([np.roll(base[t % 4], 16 * t, axis=2) for t in range(T)], axis=1)               # (3, T, H, W)
rgb = torch.from_numpy(rgb_host).cuda()
qt90 = torch.from_numpy(kernels.jpeg_quant_tables(90).view(np.int16)).cuda().view(torch.uint16)
qtT = torch.from_numpy(np.broadcast_to(kernels.jpeg_quant_tables(90), (T, 3, 64)).copy().view(np.int16)).cuda().view(torch.uint16)
cb, fb = kernels.jpeg_coef_bytes(H, W), kernels.i420_frame_bytes(H, W)
coef = torch.empty(T, cb // 2, dtype=torch.int16, device="cuda")
ms_rgb = timed(lambda: kernels.jpeg_fdct(rgb, qtT, out=coef))
assert np.array_equal(coef[:1].cpu().numpy(), kernels.jpeg_fdct_host(rgb_host[:, :1], kernels.jpeg_quant_tables(90), H, W))
frames = kernels.jpeg_idct_i420(coef, qtT, H, W)                                                    # I420 frames of the same pictures
coef2 = torch.empty_like(coef)
ms_i420 = timed(lambda: kernels.jpeg_fdct(frames, qtT, out=coef2))
assert np.array_equal(coef2[:1].cpu().numpy(), kernels.jpeg_fdct_host(frames.data[:1].cpu().numpy(), kernels.jpeg_quant_tables(90), H, W,
                                                                       _abi.SRC_I420_BT601_FULL))
out = torch.empty(T, fb, dtype=torch.uint8, device="cuda")
ms_idct = timed(lambda: kernels.jpeg_idct_i420(coef, qtT, H, W, out=out))
print(line(f"FDCT launch from RGB planes, {T} frames of {H}x{W}", ms_rgb, T * (3 * H * W + cb + 384)))
print(line(f"FDCT launch from I420 frames, {T} frames of {H}x{W}", ms_i420, T * (fb + cb + 384)))
print(line(f"IDCT launch, the same frames", ms_idct, T * (fb + cb + 384)))
print(f"FDCT / IDCT launch time: from RGB {statistics.median(ms_rgb) / statistics.median(ms_idct):.2f} x, "
      f"from I420 {statistics.median(ms_i420) / statistics.median(ms_idct):.2f} x")

# ---- 2. host entropy coding, one thread ---------------------------------------------------------------------------------------------
buf = np.empty(kernels.jpeg_encode_bound(H, W), np.uint8)
for q in (50, 75, 90):
    qt = kernels.jpeg_quant_tables(q)
    c = kernels.jpeg_fdct(rgb[:, :4].contiguous(), torch.from_numpy(qt.view(np.int16)).cuda().view(torch.uint16)).cpu().numpy()
    sizes = [kernels.jpeg_encode(c[i], qt, H, W, out=buf).size for i in range(4)]
    reps, t0 = 5, time.perf_counter()
    for _ in range(reps):
        for i in range(4):
            kernels.jpeg_encode(c[i], qt, H, W, out=buf)
    dt = (time.perf_counter() - t0) / (reps * 4)
    size = statistics.mean(sizes)
    print(f"host entropy coding, {H}x{W} q{q}: {size / 1e3:7.1f} KB per frame, {1e3 * dt:6.2f} ms per frame = {1 / dt:6.1f} frames/s = "
          f"{size / dt / 1e6:6.1f} compressed MB/s on one thread ({cb / dt / 1e9:.2f} GB/s of coefficients read)")
del rgb, coef, coef2, out, frames

# ---- 3. the harness loop without maps, with the overlays in the .npz, with overlay_video: avi ---------------------------------------
tmp = tempfile.mkdtemp(prefix="kvq_mjpeg_write_")
os.chdir(tmp)


def trainer(mode):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "kwai_swin_grpb_qmap_test.yml")))
    cfg["data"]["val"]["args"].update(num_videos=N, seed_per_item=True)
    if mode == "none":
        cfg.pop("quality_maps")
    else:
        cfg["quality_maps"].update(dir=os.path.join(tmp, "maps_" + mode), overlay_frames=2)
        if mode == "avi":
            cfg["quality_maps"].update(overlay_video="avi", overlay_quality=90)
    torch.manual_seed(0)
    return Trainer(argparse.Namespace(opt="-", target_set="val", gpu_id="0"), cfg)


modes = ("none", "npz", "avi")
trs = {m: trainer(m) for m in modes}
a = trs["none"].config["data"]["val"]["args"]
print(f"{N} synthetic videos of {a['frames']}x{a['height']}x{a['width']}, {a['sample_types']['technical']['num_clips']} clips each, 2 overlays per clip; "
      f"{ROUNDS} alternating rounds")
rates, sums = {m: [] for m in modes}, {}
for tr in trs.values():                                           # warm: plans, graphs
    tr._score_all(); torch.cuda.synchronize()
for _ in range(ROUNDS):
    for m, tr in trs.items():
        t0 = time.perf_counter(); s = tr._score_all(); torch.cuda.synchronize(); dt = time.perf_counter() - t0
        rates[m].append(N / dt)
        sums[m] = float(np.sum(s))
for m in modes:
    r = rates[m]
    print(f"Swin harness loop, {m:4s}: median {statistics.median(r):7.2f} videos/s  (min {min(r):.2f}, max {max(r):.2f}; rounds "
          + " ".join(f"{v:.2f}" for v in r) + f")  checksum {sums[m]:.6f}")
print(f"checksums equal: {sums['none'] == sums['npz'] == sums['avi']}")
for m in ("npz", "avi"):
    d = os.path.join(tmp, "maps_" + m)
    print(f"files per video, {m}: {sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) / N / 1e6:.2f} MB")
shutil.rmtree(tmp, ignore_errors=True)
