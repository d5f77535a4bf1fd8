"""Motion-JPEG with the entropy decode on the device, measured (profiles/mjpeg_entropy_probe.txt):
  1. the entropy launch (kvq_jpeg_entropy: its two fills + the kernel) on 32 frames of 1080 x 1920 at q50 and q90, written with one
     restart interval per MCU row and with none (one lane per frame), hipEvent brackets, beside kvq_jpeg_coeffs on one host thread;
  2. the size cost of one restart interval per MCU row against none, on the clips of 3.;
  3. the staging of one clip's 96 sampled frames of 540 x 960 (q75) by phase: marker walk + copy into pinned memory on the copy pool,
     the H2D copy, the entropy launch, the IDCT launch, and what is left (the status copy and its wait, Python), against the host path;
  4. the KSVQE harness loop (ViewDecompositionDataset_KVQ -> KSVQE, Kwai_KSVQE_test.yml) on those clips as .mjpeg and as .y4m, one
     child process per run so that several TREES (checkouts of this repository, e.g. the parent commit and this one, each with its
     library built) can be compared: alternating rounds, score checksums compared to the bit.
Frames are the drifting gradient + noise pictures of tools/mjpeg_probe.py, written by MjpegWriter (the library's own encoder).
`python tools/mjpeg_entropy_probe.py [--trees A,B] [--rounds 3] [--clips 8] > profiles/mjpeg_entropy_probe.txt`
(`... loop TREE DATA PASSES` is the child: it prints one JSON line.)"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = len(sys.argv) > 1 and sys.argv[1] == "loop"
sys.path.insert(0, os.path.abspath(sys.argv[2]) if CHILD else ROOT)
import numpy as np, torch, yaml  # noqa: E401,E402
import kvq_amd  # noqa: F401,E402
from kvq_amd import kernels  # noqa: E402
from kvq_amd.datasets import fusion_datasets as fd  # noqa: E402


def loop(tree, data, passes):
    """the child: the harness loop of ``tree`` on data/mjpeg and data/y4m, one warm pass and ``passes`` timed ones of each"""
    from kvq_amd.trainer import Trainer
    from kvq_amd.utils import synth
    n = len(open(os.path.join(data, "mjpeg", "anno.txt")).read().split())
    out = {"tree": tree}
    os.chdir(data)
    for sub in ("mjpeg", "y4m"):
        cfg = yaml.safe_load(open(os.path.join(tree, "config", "Kwai_KSVQE_test.yml")))
        cfg["data"]["val"]["args"].update(anno_file=os.path.join(data, sub, "anno.txt"), data_prefix=os.path.join(data, sub), seed_per_item=True)
        tr = Trainer(argparse.Namespace(opt="-", target_set="val", gpu_id="0"), cfg)
        sd = {"KSVQE_backbone." + k: torch.from_numpy(v) for k, v in synth.synth_ksvqe_weights(3).items()}
        sd.update({"KSVQE_head." + k: torch.from_numpy(v) for k, v in synth.synth_vqa_head_weights(768, 64, 3, "stress").items()})
        tr.model.load_state_dict(sd, strict=False)
        tr._score_all(); torch.cuda.synchronize()                      # noqa: E702  warm: plans, graphs, page cache
        rates = []
        for _ in range(passes):
            t0 = time.perf_counter(); s = tr._score_all(); torch.cuda.synchronize(); dt = time.perf_counter() - t0      # noqa: E702
            rates.append(n / dt)
        out[sub] = {"rates": rates, "checksum": float(np.sum(s)).hex()}
        del tr
    print("RESULT " + json.dumps(out))


if CHILD:
    loop(os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3]), int(sys.argv[4]))
    sys.exit(0)

ap = argparse.ArgumentParser()
ap.add_argument("--trees", default=ROOT, help="comma-separated checkouts to run the harness loop of, each with its library built")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--clips", type=int, default=8)
ap.add_argument("--frames", type=int, default=100)
a = ap.parse_args()
DEV = "cuda:0"


def picture(h, w, seed, shift):
    g = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([255.0 * ((x + shift) % w) / w, 255.0 * y / h, 127.5 + 127.5 * np.sin((x + y + shift) / 37.0)], axis=-1)
    return np.clip(base + g.normal(0, 10, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(rgb, quality, ri):
    """uint8 (n, H, W, 3) -> n baseline JPEG images by the library's encoder (FDCT launch + host entropy coder)"""
    n, H, W, _ = rgb.shape
    qt = kernels.jpeg_quant_tables(quality)
    coef = kernels.jpeg_fdct(torch.from_numpy(rgb).to(DEV).permute(3, 0, 1, 2).contiguous(),
                             torch.from_numpy(qt.view(np.int16)).to(DEV).view(torch.uint16)).cpu().numpy()
    return [kernels.jpeg_encode(c, qt, H, W, ri).tobytes() for c in coef]


def events(f, reps=30, warm=5):
    for _ in range(warm):
        f()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); e1.synchronize()                # noqa: E702
        ms.append(e0.elapsed_time(e1))
    return ms


def spread(ms):
    return f"median {statistics.median(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, n {len(ms)})"


print(f"device: {kernels.device_name()}; frames written by MjpegWriter / kvq_jpeg_encode")

# ---- 1. the entropy launch -----------------------------------------------------------------------------------------------------------
sys.path.insert(0, os.path.join(ROOT, "tests"))
HH, WW, TT = 1080, 1920, 32
pics = np.stack([picture(HH, WW, 10 + i, 16 * i) for i in range(4)])
cb = kernels.jpeg_coef_bytes(HH, WW)
for q in (50, 90):
    for ri, label in (((WW + 15) // 16, "one restart interval per MCU row"), (0, "no restart interval: one lane per frame")):
        jpgs = encode(pics, q, ri)
        want, hq = np.empty((4, cb // 2), np.int16), np.empty((3, 64), np.uint16)
        t0 = time.perf_counter()
        for i in range(4):
            assert kernels.jpeg_coeffs(np.frombuffer(jpgs[i], np.uint8), want[i], hq)[0] == 0
        host_ms = 1e3 * (time.perf_counter() - t0) / 4
        blob, frames, segs, sets, off = [], [], [], [], 0
        for t in range(TT):
            j = np.frombuffer(jpgs[t % 4], np.uint8)
            sg, tb, qq = np.zeros((cb // 768, 2), np.uint32), np.zeros(kernels.JPEG_TABLES_BYTES, np.uint8), np.zeros((3, 64), np.uint16)
            rc, info, nseg, msg = kernels.jpeg_index(j, sg, tb, qq)
            assert rc == 0, msg
            if not sets:
                sets.append(tb)
            frames.append((off, sum(len(s) for s in segs), nseg, info.restart_interval, 0))
            segs.append(sg[:nseg]); blob.append(j); off += j.size      # noqa: E702
        d = torch.from_numpy(np.concatenate(blob)).to(DEV)
        f = torch.from_numpy(np.array(frames, np.uint32).view(np.int32)).to(DEV)
        s = torch.from_numpy(np.concatenate(segs).view(np.int32)).to(DEV)
        tb = torch.from_numpy(np.stack(sets)).to(DEV)
        coef, status = kernels.jpeg_entropy(d, f, s, tb, TT, HH, WW)
        ms = events(lambda: kernels.jpeg_entropy(d, f, s, tb, TT, HH, WW, coef=coef, status=status), reps=10 if ri == 0 else 30, warm=2)
        assert not status.any().item() and np.array_equal(coef[:4].cpu().numpy(), want)
        fill = events(lambda: coef.zero_())
        med = statistics.median(ms)
        print(f"entropy launch, {TT} frames of {HH}x{WW} q{q}, {label}: {off / TT / 1e3:.1f} KB per frame, {s.shape[0] // TT} segments per frame; "
              f"{spread(ms)} = {med / TT:.4f} ms per frame, of which the zero fill of {TT * cb / 1e6:.0f} MB of coefficients alone is "
              f"{statistics.median(fill):.3f} ms; kvq_jpeg_coeffs on one host thread {host_ms:.2f} ms per frame")
        del d, f, s, tb, coef, status
del pics

# ---- 2. / 3. the clips, their sizes, the staging by phase ----------------------------------------------------------------------------
H, W, T, N = 540, 960, a.frames, a.clips
row = (W + 15) // 16
data = tempfile.mkdtemp(prefix="kvq_mjpeg_entropy_")
for sub in ("mjpeg", "y4m", "plain"):
    os.makedirs(os.path.join(data, sub))
bases = [picture(H, W, 100 + k, 0) for k in range(10)]
header = f"YUV4MPEG2 W{W} H{H} F30:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n".encode()
size_row, size_0 = [], []
for i in range(N):
    rgb = torch.from_numpy(np.stack([np.roll(bases[t % 10], 8 * t + 3 * i, axis=1) for t in range(T)])).to(DEV).permute(3, 0, 1, 2).contiguous()
    for sub, ri in (("mjpeg", row), ("plain", 0)):
        with fd.MjpegWriter(os.path.join(data, sub, f"clip{i}.mjpeg"), 30, quality=75, restart_interval=ri) as w:
            w.write(rgb)
    size_row.append(os.path.getsize(os.path.join(data, "mjpeg", f"clip{i}.mjpeg")))
    size_0.append(os.path.getsize(os.path.join(data, "plain", f"clip{i}.mjpeg")))
    r = fd.MjpegFrameReader(os.path.join(data, "mjpeg", f"clip{i}.mjpeg"))
    frames = fd._frames_to_device(r, np.arange(T), DEV, "host").data.cpu().numpy()
    with open(os.path.join(data, "y4m", f"clip{i}.y4m"), "wb") as f:
        f.write(header + b"".join(b"FRAME\n" + fr.tobytes() for fr in frames))
    del rgb
for sub, ext in (("mjpeg", "mjpeg"), ("y4m", "y4m")):
    open(os.path.join(data, sub, "anno.txt"), "w").write("".join(f"clip{i}.{ext},1,{i % 5},3.0\n" for i in range(N)))
nseg = -(-H // 16)
print(f"{N} clips of {T}x{H}x{W} (q75): {statistics.mean(size_0) / 1e6:.3f} MB each without restart markers, {statistics.mean(size_row) / 1e6:.3f} MB with one "
      f"interval per MCU row ({row} MCUs, {nseg} intervals per frame): +{100 * (sum(size_row) / sum(size_0) - 1):.2f}% = "
      f"{(sum(size_row) - sum(size_0)) / (N * T * (nseg - 1)):.1f} bytes per marker (2 of marker, the rest padding and DC resets)")

vr = fd.open_video(os.path.join(data, "mjpeg", "clip0.mjpeg"))
uniq = np.unique(np.linspace(0, T - 1, 96).astype(int))
clock = {}


def timed(name, f, cuda):
    def g(*x, **kw):
        if cuda:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); out = f(*x, **kw); e1.record()                # noqa: E702
            clock.setdefault(name, []).append((e0, e1))
            return out
        t0 = time.perf_counter()
        out = f(*x, **kw)
        clock.setdefault(name, []).append((t0, time.perf_counter()))
        return out
    return g


def staging(mode, reps=7):
    """wall ms of ``_frames_to_device`` + synchronise, per repetition, and the phases the wrappers saw in each"""
    global clock
    walls, phases = [], []
    for k in range(reps + 2):
        clock = {}
        t0 = time.perf_counter(); fd._frames_to_device(vr, uniq, DEV, mode); torch.cuda.synchronize(); dt = time.perf_counter() - t0      # noqa: E702
        if k < 2:
            continue
        walls.append(1e3 * dt)
        ph = {}
        for name, spans in clock.items():
            if isinstance(spans[0][0], float):
                ph[name] = 1e3 * (max(e for _, e in spans) - min(b for b, _ in spans))       # threads: first start to last end
            else:
                ph[name] = sum(e0.elapsed_time(e1) for e0, e1 in spans)
        phases.append(ph)
    return walls, {k: statistics.median(p[k] for p in phases) for k in phases[0]}


real = (fd.MjpegFrameReader.read_jpeg_bytes_into, fd.MjpegFrameReader.read_jpeg_into, kernels.jpeg_entropy, kernels.jpeg_idct_i420)
fd.MjpegFrameReader.read_jpeg_bytes_into = timed("index + copy to pinned (copy pool)", real[0], False)
fd.MjpegFrameReader.read_jpeg_into = timed("host entropy decode (copy pool)", real[1], False)
kernels.jpeg_entropy = timed("entropy launch", real[2], True)
kernels.jpeg_idct_i420 = timed("IDCT launch", real[3], True)
for mode in ("host", "device"):
    walls, ph = staging(mode)
    staged = len(uniq) * (vr.coef_bytes + 384) if mode == "host" else sum(vr._index[int(i)][2] for i in uniq)
    print(f"staging of {len(uniq)} sampled frames of one {H}x{W} clip, jpeg_entropy={mode}: median {statistics.median(walls):.2f} ms "
          f"(min {min(walls):.2f}, max {max(walls):.2f}, n {len(walls)}), {staged / 1e6:.1f} MB through the H2D copy; "
          + "; ".join(f"{k} {v:.2f} ms" for k, v in ph.items()) + f"; the rest (H2D copy, status copy and wait, Python) "
          f"{statistics.median(walls) - sum(ph.values()):.2f} ms")
fd.MjpegFrameReader.read_jpeg_bytes_into, fd.MjpegFrameReader.read_jpeg_into, kernels.jpeg_entropy, kernels.jpeg_idct_i420 = real
pinned = torch.empty(sum(vr._index[int(i)][2] for i in uniq) + 400000, dtype=torch.uint8).pin_memory()
ms = events(lambda: pinned.to(DEV, non_blocking=True))
print(f"H2D copy of {pinned.numel() / 1e6:.1f} MB (the compressed frames, their index and tables) from pinned memory alone: {spread(ms)}")
idx_t0 = time.perf_counter()
sg, tb, qq = np.zeros((vr.coef_bytes // 768, 2), np.uint32), np.zeros(kernels.JPEG_TABLES_BYTES, np.uint8), np.zeros((3, 64), np.uint16)
for i in uniq:
    kernels.jpeg_index(np.asarray(vr._frame(i)), sg, tb, qq)
print(f"kvq_jpeg_index of the {len(uniq)} frames on one thread: {1e3 * (time.perf_counter() - idx_t0):.2f} ms")

# ---- 4. the harness loop, one child per run ------------------------------------------------------------------------------------------
trees = [os.path.abspath(t) for t in a.trees.split(",")]
torch.cuda.synchronize()
results = {t: {"mjpeg": [], "y4m": [], "sum": set()} for t in trees}
failed = False
for rnd in range(a.rounds):
    for t in trees:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "loop", t, data, "2"], capture_output=True, text=True, timeout=600)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"harness loop of {t} failed (exit {r.returncode}): {r.stderr[-1500:]}")
            failed = True
            break
        out = json.loads(line[-1][7:])
        for sub in ("mjpeg", "y4m"):
            results[t][sub] += out[sub]["rates"]
        results[t]["sum"].add((out["mjpeg"]["checksum"], out["y4m"]["checksum"]))
    if failed:
        break
if not failed:
    for t in trees:
        for sub in ("mjpeg", "y4m"):
            r = results[t][sub]
            print(f"KSVQE harness loop, tree {os.path.relpath(t, ROOT)}, {sub:5s}: median {statistics.median(r):7.2f} videos/s (min {min(r):.2f}, max {max(r):.2f}; "
                  + " ".join(f"{v:.2f}" for v in r) + ")")
    sums = set().union(*(results[t]["sum"] for t in trees))
    print(f"score checksums (mjpeg, y4m) over all runs and trees: {sorted(sums)}; all equal to the bit: {len(sums) == 1 and len(next(iter(sums))) == 2 and len(set(next(iter(sums)))) == 1}")
    if len(trees) == 2:
        old, new = results[trees[0]]["mjpeg"], results[trees[1]]["mjpeg"]
        print(f"every run of {os.path.relpath(trees[1], ROOT)} above every run of {os.path.relpath(trees[0], ROOT)}: {min(new) > max(old)} "
              f"(min {min(new):.2f} against max {max(old):.2f})")
shutil.rmtree(data, ignore_errors=True)
sys.exit(1 if failed else 0)
