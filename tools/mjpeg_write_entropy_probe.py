"""Motion-JPEG output with the entropy coder on the device, measured (profiles/mjpeg_write_entropy_probe.txt), one part per run so that
each sits under its own time limit:
  --part 1  the entry alone (kvq_jpeg_encode_scans) on 32 frames of 1080 x 1920 at q50 / q75 / q90, restart interval 0 and row: hipEvent
            brackets, n = 30 after 5 warm calls, against its byte floor — the coefficients read by the three phases that read them (count,
            ffcount, write), 12 bytes per block of positions and counts written and read twice, the output written — at the 6.3 TB/s the
            other probes use; beside
            it the host coder's ms per frame on one thread and on the copy pool's four, and the bytes each path brings down;
  --part 2  MjpegWriter.write end to end, the same frames, entropy "host" against "device", three alternating rounds, file hashes;
  --part 3  tools/transcode_mjpeg.py's transcode() on eight 100 x 540 x 960 clips from .y4m, "host" against "device", alternating.
Frames are tools/mjpeg_write_probe.py's: a seeded gradient + noise picture that drifts from frame to frame.
`python tools/mjpeg_write_entropy_probe.py --part N >> profiles/mjpeg_write_entropy_probe.txt`"""
import argparse
import hashlib
import importlib.util
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch  # noqa: E401,E402
import kvq_amd  # noqa: F401,E402
from kvq_amd import kernels  # noqa: E402
from kvq_amd.datasets import fusion_datasets as fd  # noqa: E402

HBM = 6.3e12
H, W, T = 1080, 1920, 32


def picture(h, w, seed, shift):
    g = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([255.0 * ((x + shift) % w) / w, 255.0 * y / h, 127.5 + 127.5 * np.sin((x + y + shift) / 37.0)])
    return np.clip(base + g.normal(0, 10, (3, h, w)), 0, 255).astype(np.uint8)


def clip(t, h, w):
    base = [picture(h, w, 10 + k, 0) for k in range(4)]
    return np.stack([np.roll(base[i % 4], 16 * i, axis=2) for i in range(t)], axis=1)               # (3, t, h, w)


def timed(fn, n=30, warm=5):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def dev_qt(q):
    return torch.from_numpy(kernels.jpeg_quant_tables(q).view(np.int16)).cuda().view(torch.uint16)


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]


def part1():
    rgb = torch.from_numpy(clip(T, H, W)).cuda()
    cb = kernels.jpeg_coef_bytes(H, W)
    for q in (50, 75, 90):
        qt = kernels.jpeg_quant_tables(q)
        coef = kernels.jpeg_fdct(rgb, dev_qt(q))
        host = coef.cpu().numpy()
        buf = np.empty(kernels.jpeg_encode_bound(H, W), np.uint8)
        t0 = time.perf_counter()
        sizes = [kernels.jpeg_encode(host[i], qt, H, W, out=buf).size for i in range(8)]
        one = (time.perf_counter() - t0) / 8

        def four(a, b):
            local = np.empty(kernels.jpeg_encode_bound(H, W), np.uint8)
            for i in range(a, b):
                kernels.jpeg_encode(host[i], qt, H, W, out=local)
        t0 = time.perf_counter()
        for j in [fd._copy_pool().submit(four, 8 * k, 8 * k + 8) for k in range(4)]:
            j.result()
        pool = (time.perf_counter() - t0) / T
        print(f"host coder, {H}x{W} q{q}: {1e3 * one:.2f} ms per frame on one thread, {1e3 * pool:.2f} ms per frame on the copy pool's four; "
              f"{statistics.mean(sizes) / 1e3:.1f} KB per frame; brings down {T * cb / 1e6:.1f} MB of coefficients for {T} frames")
        for ri in (0, (W + 15) // 16):
            out, frames = kernels.jpeg_encode_scans(coef, H, W, ri)
            table = frames.cpu().numpy().view(np.uint32)
            assert (table[:, 2] == 0).all(), table
            total = int(table[-1, 0]) + int(table[-1, 1])
            want = kernels.jpeg_encode(host[T - 1], qt, H, W, ri).tobytes()
            head = kernels.jpeg_encode_header(qt, H, W, ri).tobytes()
            assert head + out[int(table[-1, 0]):total].cpu().numpy().tobytes() + b"\xff\xd9" == want
            ws = torch.empty(kernels.jpeg_scans_workspace_bytes(T, H, W), dtype=torch.uint8, device="cuda")
            ms = timed(lambda: kernels.jpeg_encode_scans(coef, H, W, ri, workspace=ws))
            moved = 3 * T * cb + 3 * ws.numel() + total                  # coefficients three times; positions and counts written, read, read; the output
            med, floor = statistics.median(ms), moved / HBM * 1e3
            print(f"device entry, {T} frames of {H}x{W} q{q} restart {ri}: median {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, n {len(ms)}) = "
                  f"{med / T:.4f} ms per frame; {total / 1e6:.2f} MB of scans + {12 * T} B of table brought down; byte floor ({moved / 1e6:.0f} MB at "
                  f"6.3 TB/s) {floor:.3f} ms = {100 * floor / med:.0f}% of the measured time")


def part2():
    rgb = torch.from_numpy(clip(T, H, W)).cuda()
    tmp = tempfile.mkdtemp(prefix="kvq_mjpeg_entropy_")
    for q in (50, 75, 90):
        for ri in (0, (W + 15) // 16):
            rates, hashes = {"host": [], "device": []}, {}
            for rnd in range(4):                                        # round 0 warms both paths
                for mode in ("host", "device"):
                    path = os.path.join(tmp, f"{mode}.mjpeg")
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with fd.MjpegWriter(path, 30, quality=q, restart_interval=ri, entropy=mode) as w:
                        w.write(rgb)
                    dt = time.perf_counter() - t0
                    if rnd:
                        rates[mode].append(T / dt)
                    hashes[mode] = sha(path)
            above = all(d > h for d, h in zip(rates["device"], rates["host"]))
            print(f"MjpegWriter.write, {T} frames of {H}x{W} q{q} restart {ri}: host " + " ".join(f"{v:.1f}" for v in rates["host"])
                  + " frames/s; device " + " ".join(f"{v:.1f}" for v in rates["device"]) + f" frames/s; device above host in every round: {above}; "
                  f"file {os.path.getsize(path) / 1e6:.1f} MB, hashes equal: {hashes['host'] == hashes['device']}")
    shutil.rmtree(tmp, ignore_errors=True)


def part3():
    spec = importlib.util.spec_from_file_location("transcode_mjpeg", os.path.join(ROOT, "tools", "transcode_mjpeg.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tmp = tempfile.mkdtemp(prefix="kvq_mjpeg_entropy_")
    n, t, h, w = 8, 100, 540, 960
    frames = kernels.jpeg_idct_i420(kernels.jpeg_fdct(torch.from_numpy(clip(t, h, w)).cuda(), dev_qt(95)), dev_qt(95).repeat(t, 1, 1), h, w)
    payload = frames.data.cpu().numpy()
    for k in range(n):
        with open(os.path.join(tmp, f"{k}.y4m"), "wb") as f:
            f.write(f"YUV4MPEG2 W{w} H{h} F30:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n".encode())
            for i in range(t):
                f.write(b"FRAME\n" + np.roll(payload[i], k).tobytes())
    rates, hashes = {"host": [], "device": []}, {}
    for rnd in range(4):
        for mode in ("host", "device"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(n):
                tool.transcode(os.path.join(tmp, f"{k}.y4m"), os.path.join(tmp, f"{mode}_{k}.mjpeg"), 90, None, "row", "bt601", "cuda", mode)
            dt = time.perf_counter() - t0
            if rnd:
                rates[mode].append(n * t / dt)
            hashes[mode] = [sha(os.path.join(tmp, f"{mode}_{k}.mjpeg")) for k in range(n)]
    size = sum(os.path.getsize(os.path.join(tmp, f"host_{k}.mjpeg")) for k in range(n)) / 1e6
    print(f"transcode_mjpeg.py, {n} clips of {t}x{h}x{w} from .y4m, q90 restart row: host " + " ".join(f"{v:.1f}" for v in rates["host"])
          + " frames/s; device " + " ".join(f"{v:.1f}" for v in rates["device"]) + f" frames/s; {size:.1f} MB written per round; hashes equal: "
          f"{hashes['host'] == hashes['device']}")
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", type=int, required=True, choices=(1, 2, 3))
    part = ap.parse_args().part
    if part == 1:
        print(f"device: {kernels.device_name()}")
    {1: part1, 2: part2, 3: part3}[part]()
