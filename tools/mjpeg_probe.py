"""Motion-JPEG input, measured (profiles/mjpeg_probe.txt):
  1. the host entropy decode (kvq_jpeg_coeffs) of 1080 x 1920 frames at two qualities: frames/s and compressed MB/s on ONE thread;
  2. the IDCT launch (kvq_jpeg_idct_i420) on 32 such frames, hipEvent brackets, against its byte floor: 2 B per coefficient + the tables
     read, 1 B per sample written, over the 6.3 TB/s a streaming kernel achieves on this chip;
  3. videos/s of the harness loop (tools/harness_probe.py: ViewDecompositionDataset_KVQ -> KSVQE, default settings) on the same clips
     stored as .npy RGB stacks, as .y4m and as .mjpeg, alternating rounds, checksums compared.
Frames are a seeded gradient + noise picture that drifts from frame to frame, encoded by Pillow when it is importable and by
tests/jpeg_ref.py's encoder (float DCT + the Annex K tables) otherwise.
`python tools/mjpeg_probe.py [N] [T] [H] [W] [rounds] > profiles/mjpeg_probe.txt`"""
import argparse
import io
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch, yaml  # noqa: E401,E402
import kvq_amd  # noqa: F401,E402
from kvq_amd import kernels  # noqa: E402
from kvq_amd.datasets import fusion_datasets as fd  # noqa: E402
from kvq_amd.trainer import Trainer  # noqa: E402
from kvq_amd.utils import synth  # noqa: E402
import jpeg_ref  # noqa: E402

N, T, H, W, ROUNDS = (int(sys.argv[i + 1]) if len(sys.argv) > i + 1 else d for i, d in enumerate((12, 100, 540, 960, 3)))
HBM = 6.3e12
try:
    from PIL import Image
    ENCODER = f"Pillow {Image.__version__}"
except ImportError:
    Image, ENCODER = None, "tests/jpeg_ref.py (float DCT, Annex K tables)"

# the luminance / chrominance tables of ITU-T T.81 Annex K.1 / K.2, scaled as the IJG library scales them
K1 = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62, 18, 22,
               37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
K2 = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)


def picture(h, w, seed, shift):
    g = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([255.0 * ((x + shift) % w) / w, 255.0 * y / h, 127.5 + 127.5 * np.sin((x + y + shift) / 37.0)], axis=-1)
    return np.clip(base + g.normal(0, 10, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(rgb, quality):
    if Image is not None:
        b = io.BytesIO()
        Image.fromarray(rgb).save(b, "JPEG", quality=quality, subsampling=2)
        return b.getvalue()
    h, w, _ = rgb.shape
    s = 5000 / quality if quality < 50 else 200 - 2 * quality
    qt = np.stack([np.clip((k * s + 50) // 100, 1, 255) for k in (K1, K2, K2)]).astype(np.uint16)
    f = rgb.astype(np.float64)
    ycc = [0.299 * f[..., 0] + 0.587 * f[..., 1] + 0.114 * f[..., 2], 128 - 0.168736 * f[..., 0] - 0.331264 * f[..., 1] + 0.5 * f[..., 2],
           128 + 0.5 * f[..., 0] - 0.418688 * f[..., 1] - 0.081312 * f[..., 2]]
    mx, my = jpeg_ref.geom(h, w)[:2]
    k = np.arange(8)
    C = np.sqrt(0.25) * np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16)
    C[0] /= np.sqrt(2)
    out = []
    for c, p in enumerate(ycc):
        p = np.pad(p, ((0, 16 * my - h), (0, 16 * mx - w)), mode="edge")
        if c:
            p = p.reshape(8 * my, 2, 8 * mx, 2).mean(axis=(1, 3))
        blocks = (p - 128).reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).transpose(0, 2, 1, 3)
        out.append(np.rint(np.einsum("ij,abjk,lk->abil", C, blocks, C).reshape(-1, 64) / qt[c]).astype(np.int16))
    return jpeg_ref.encode_baseline(np.concatenate(out), qt, h, w)


print(f"device: {kernels.device_name()}; JPEG frames encoded by {ENCODER}")

# ---- 1. host entropy decode, one thread --------------------------------------------------------------------------------------------
HH, WW = 1080, 1920
cb = kernels.jpeg_coef_bytes(HH, WW)
coef, qt = np.empty(cb // 2, np.int16), np.empty((3, 64), np.uint16)
big = {}
for q in (50, 90):
    frames = [np.frombuffer(encode(picture(HH, WW, 10 + i, 16 * i), q), np.uint8) for i in range(4)]
    big[q] = frames
    for f in frames:
        assert kernels.jpeg_coeffs(f, coef, qt)[0] == 0
    reps, t0 = 5, time.perf_counter()
    for _ in range(reps):
        for f in frames:
            kernels.jpeg_coeffs(f, coef, qt)
    dt = (time.perf_counter() - t0) / (reps * len(frames))
    size = statistics.mean(f.size for f in frames)
    print(f"host entropy decode, {HH}x{WW} q{q}: {size / 1e3:7.1f} KB per frame, {1e3 * dt:6.2f} ms per frame = {1 / dt:6.1f} frames/s = "
          f"{size / dt / 1e6:6.1f} compressed MB/s on one thread ({cb / dt / 1e9:.2f} GB/s of coefficients written)")

# ---- 2. the IDCT launch against its byte floor -------------------------------------------------------------------------------------
TT = 32
hc, hq = np.empty((TT, cb // 2), np.int16), np.empty((TT, 3, 64), np.uint16)
for t in range(TT):
    assert kernels.jpeg_coeffs(big[90 if t % 2 else 50][t % 4], hc[t], hq[t])[0] == 0
dc, dq = torch.from_numpy(hc).cuda(), torch.from_numpy(hq.view(np.int16)).cuda().view(torch.uint16)
out = torch.empty(TT, kernels.i420_frame_bytes(HH, WW), dtype=torch.uint8, device="cuda")
for _ in range(5):
    kernels.jpeg_idct_i420(dc, dq, HH, WW, out=out)
ms = []
for _ in range(30):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); kernels.jpeg_idct_i420(dc, dq, HH, WW, out=out); b.record(); b.synchronize()
    ms.append(a.elapsed_time(b))
assert np.array_equal(out[:2].cpu().numpy(), kernels.jpeg_idct_i420_host(hc[:2], hq[:2], HH, WW))
nbytes = TT * (cb + 384 + kernels.i420_frame_bytes(HH, WW))
floor = nbytes / HBM * 1e3
print(f"IDCT launch, {TT} frames of {HH}x{WW}: {nbytes / 1e6:.1f} MB moved ({TT * cb / 1e6:.1f} read as int16 coefficients, "
      f"{TT * kernels.i420_frame_bytes(HH, WW) / 1e6:.1f} written); median {statistics.median(ms):.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}, n {len(ms)}) "
      f"= {nbytes / statistics.median(ms) / 1e9:.2f} TB/s; byte floor at 6.3 TB/s {floor:.4f} ms -> {100 * floor / statistics.median(ms):.0f}% of the floor rate")
del dc, dq, out

# ---- 3. the harness loop on .npy / .y4m / .mjpeg trees of the same clips -----------------------------------------------------------
tmp = tempfile.mkdtemp(prefix="kvq_mjpeg_tree_")
subs = ("npy", "y4m", "mjpeg")
for sub in subs:
    os.makedirs(os.path.join(tmp, sub))
header = f"YUV4MPEG2 W{W} H{H} F30:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n".encode()
sizes = []
bases = [picture(H, W, 100 + k, 0) for k in range(10)]           # a frame = one of ten pictures, drifting sideways
for i in range(N):
    jpgs = [encode(np.roll(bases[t % 10], 8 * t + 3 * i, axis=1), 75) for t in range(T)]
    path = os.path.join(tmp, "mjpeg", f"clip{i}.mjpeg")
    jpeg_ref.write_mjpeg(path, jpgs)
    sizes.append(os.path.getsize(path))
    r = fd.MjpegFrameReader(path)
    frames = np.stack([r.i420(t) for t in range(T)])
    with open(os.path.join(tmp, "y4m", f"clip{i}.y4m"), "wb") as f:
        f.write(header + b"".join(b"FRAME\n" + fr.tobytes() for fr in frames))
    rgb = kernels.I420Frames(torch.from_numpy(frames).cuda(), H, W, r.format).to_rgb()
    np.save(os.path.join(tmp, "npy", f"clip{i}.npy"), rgb.permute(1, 2, 3, 0).contiguous().cpu().numpy())
ext = {"npy": "npy", "y4m": "y4m", "mjpeg": "mjpeg"}
for sub in subs:
    open(os.path.join(tmp, sub, "anno.txt"), "w").write("".join(f"clip{i}.{ext[sub]},1,{i % 5},3.0\n" for i in range(N)))
fb = kernels.i420_frame_bytes(H, W)
print(f"{N} videos of {T}x{H}x{W} (q75): .npy RGB {T * H * W * 3 / 1e6:.0f} MB each, .y4m {T * fb / 1e6:.0f} MB, .mjpeg {statistics.mean(sizes) / 1e6:.1f} MB; "
      f"staged per sampled frame: {3 * H * W / 1e6:.2f} / {fb / 1e6:.2f} / {kernels.jpeg_coef_bytes(H, W) / 1e6:.2f} MB; {ROUNDS} alternating rounds")


def trainer(sub):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "Kwai_KSVQE_test.yml")))
    cfg["data"]["val"]["args"].update(anno_file=os.path.join(tmp, sub, "anno.txt"), data_prefix=os.path.join(tmp, sub), seed_per_item=True)
    tr = Trainer(argparse.Namespace(opt="-", target_set="val", gpu_id="0"), cfg)
    sd = {"KSVQE_backbone." + k: torch.from_numpy(v) for k, v in synth.synth_ksvqe_weights(3).items()}
    sd.update({"KSVQE_head." + k: torch.from_numpy(v) for k, v in synth.synth_vqa_head_weights(768, 64, 3, "stress").items()})
    tr.model.load_state_dict(sd, strict=False)
    return tr


os.chdir(tmp)
trs = {sub: trainer(sub) for sub in subs}
rates, sums = {s: [] for s in subs}, {}
for tr in trs.values():                                           # warm: plans, graphs, page cache
    tr._score_all(); torch.cuda.synchronize()
for _ in range(ROUNDS):
    for sub, tr in trs.items():
        t0 = time.perf_counter(); s = tr._score_all(); torch.cuda.synchronize(); dt = time.perf_counter() - t0
        rates[sub].append(N / dt)
        sums[sub] = float(np.sum(s))
for sub in subs:
    r = rates[sub]
    print(f"KSVQE harness loop {sub:6s}: median {statistics.median(r):7.2f} videos/s  (min {min(r):.2f}, max {max(r):.2f}; rounds "
          + " ".join(f"{v:.2f}" for v in r) + f")  checksum {sums[sub]:.6f}")
print(f"checksums equal: y4m == mjpeg {sums['y4m'] == sums['mjpeg']}, npy == mjpeg {sums['npy'] == sums['mjpeg']}")
# where the Motion-JPEG item's time goes: the staging step alone, one video, in line
vr = fd.open_video(os.path.join(tmp, "mjpeg", "clip0.mjpeg"))
uniq = np.unique(np.linspace(0, T - 1, 96).astype(int))
for _ in range(2):
    fd._frames_to_device(vr, uniq, "cuda:0"); torch.cuda.synchronize()
t0 = time.perf_counter(); fd._frames_to_device(vr, uniq, "cuda:0"); torch.cuda.synchronize(); dt = time.perf_counter() - t0
t1 = time.perf_counter()
c2, q2 = np.empty((len(uniq), vr.coef_bytes // 2), np.int16), np.empty((len(uniq), 3, 64), np.uint16)
vr.read_jpeg_into(uniq, c2, q2)
d1 = time.perf_counter() - t1
print(f"staging of {len(uniq)} sampled frames of one {H}x{W} video: {1e3 * dt:.1f} ms in all with {fd._COPY_THREADS} decode threads "
      f"(H2D copy of {len(uniq) * (vr.coef_bytes + 384) / 1e6:.0f} MB + one IDCT launch included); the entropy decode alone on one thread {1e3 * d1:.1f} ms")
shutil.rmtree(tmp, ignore_errors=True)
