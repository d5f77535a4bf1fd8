"""The frame transform of the motion-feature extractor, host against device, same box, alternating: per size one 300-frame .y4m clip
at 30 fps through (a) VideoDataset_NR_SlowFast_feature — the reader's host YUV -> RGB conversion, one PIL resize per used frame,
ToTensor + Normalize, torch.stack, in ONE process, then the clips' copy to the device (what extract_video does with them) — and
(b) slowfast_clips.device_clips — the I420 payload through pinned staging, kvq_resize_pil, index gathers.  Checksums of the clips
must be equal.  Also the resize launch alone (64 frames, I420 and uint8 RGB sources) against its byte floor at 6.3 TB/s.
`python tools/slowfast_input_probe.py [frames] [rounds] > profiles/slowfast_input_probe.txt`"""
import os
import shutil
import statistics
import sys
import tempfile
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch  # noqa: E401,E402
import kvq_amd  # noqa: F401,E402
from kvq_amd import _abi, kernels  # noqa: E402
from kvq_amd.datasets.fusion_datasets import open_video  # noqa: E402
from kvq_amd.datasets.slowfast_clips import VideoDataset_NR_SlowFast_feature, device_clips  # noqa: E402

FRAMES, ROUNDS = (int(sys.argv[i + 1]) if len(sys.argv) > i + 1 else d for i, d in enumerate((300, 3)))
SIZES, R, HBM = ((540, 960), (1080, 1920)), 224, 6.3e12
tmp = tempfile.mkdtemp(prefix="kvq_sf_input_")
print(f"{kernels.device_name()}; {FRAMES}-frame .y4m clips at 30 fps -> {R} x {R}; {ROUNDS} alternating rounds; times in ms per video")


def checksum(clips):
    return float(sum(c.double().sum() for c in {id(c): c for c in clips}.values()))


for H, W in SIZES:
    fb = kernels.i420_frame_bytes(H, W)
    base = np.random.Generator(np.random.PCG64(5)).integers(0, 256, size=(8, fb), dtype=np.uint8)
    path = os.path.join(tmp, f"clip_{H}.y4m")
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{W} H{H} F30:1 Ip A1:1 C420jpeg\n".encode())
        for i in range(FRAMES):
            f.write(b"FRAME\n" + np.roll(base[i % 8], 4099 * (i // 8)).tobytes())
    open(os.path.join(tmp, "v.csv"), "w").write(f"filename,score\nclip_{H}.y4m,1\n")
    ds = VideoDataset_NR_SlowFast_feature(types.SimpleNamespace(resize=R, fps=None), None, tmp, os.path.join(tmp, "v.csv"))

    def host():
        clips, _ = ds[0]
        return [c.cuda() for c in {id(c): c for c in clips}.values()], clips

    def device():
        clips = device_clips(open_video(path), path, R, "cuda")
        return clips, clips

    device(); torch.cuda.synchronize()                      # warm: tap tables, staging, page cache
    times, sums = {"host": [], "device": []}, {}
    for _ in range(ROUNDS):
        for name, fn in (("host", host), ("device", device)):
            t0 = time.perf_counter(); _, clips = fn(); torch.cuda.synchronize(); times[name].append(1e3 * (time.perf_counter() - t0))
            sums[name] = checksum([c.cpu() for c in clips])
    for name in ("host", "device"):
        t = times[name]
        print(f"{H:4d}x{W:4d} {name:6s}: median {statistics.median(t):9.1f}  rounds " + " ".join(f"{v:.1f}" for v in t) + f"  checksum {sums[name]:.6f}")
    wins = all(d < h for h, d in zip(times["host"], times["device"]))
    print(f"{H:4d}x{W:4d} device faster in every round: {wins}; host / device (medians) {statistics.median(times['host']) / statistics.median(times['device']):.1f}x; "
          f"checksums equal: {sums['host'] == sums['device']}")
    # the launch alone
    T = 64
    raw = torch.from_numpy(np.stack([np.roll(base[i % 8], 4099 * i) for i in range(T)])).cuda()
    i420 = kernels.I420Frames(raw, H, W, _abi.SRC_I420_BT601_LIMITED)
    rgb = i420.to_rgb().permute(1, 2, 3, 0).contiguous()
    lut, out = kernels.slowfast_lut().cuda(), torch.empty(T, 3, R, R, dtype=torch.float32, device="cuda")
    for name, src, nbytes in (("I420", i420, T * fb), ("uint8 RGB", rgb, T * H * W * 3)):
        for _ in range(3):
            kernels.resize_pil(src, R, R, lut, out=out)
        us = []
        for _ in range(20):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); kernels.resize_pil(src, R, R, lut, out=out); b.record(); b.synchronize()
            us.append(1e3 * a.elapsed_time(b))
        floor = 1e6 * (nbytes + out.numel() * 4) / HBM
        print(f"{H:4d}x{W:4d} resize launch, {T} frames, {name:9s}: median {statistics.median(us):8.1f} us (min {min(us):.1f}, max {max(us):.1f}); "
              f"byte floor {floor:.1f} us -> {statistics.median(us) / floor:.1f}x the floor")
    os.remove(path)
shutil.rmtree(tmp, ignore_errors=True)
