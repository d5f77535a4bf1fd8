"""Write any video ``open_video`` reads — a ``.npy`` frame stack, a ``.y4m`` file, Motion-JPEG in any of its containers — as
Motion-JPEG, without a codec library (``MjpegWriter``: forward DCT on the device, entropy coding on host threads; without a device the
scalar twin of the launch, bit-equal).  DST picks the container: ``*.mjpeg`` / ``*.mjpg`` a raw stream, ``*.avi`` RIFF AVI, anything
else a directory of ``%06d.jpg`` frames.  I420 sources in BT.601 full range are written from their planes as they are (no colour
round trip); any other I420 format goes through ``to_rgb()``, which needs a device.

``--restart-interval row`` writes one restart interval per MCU row (ceil(W / 16) MCUs): the setting for datasets meant to be read
back at speed, since the reader entropy-decodes the restart intervals of a frame in parallel on the device (README.md).
``--entropy`` says where the frames are entropy-CODED: ``host`` (the threads of the copy pool), ``device`` (one lane per block; needs
``--device cuda``) or ``auto`` (``MjpegWriter``'s default); the files are equal byte for byte.

    python tools/transcode_mjpeg.py SRC DST [--quality 90] [--fps F] [--restart-interval N|row] [--yuv-matrix bt601|bt709] [--device cuda|cpu]
                                    [--entropy auto|host|device]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch  # noqa: E401,E402
import kvq_amd  # noqa: F401,E402
from kvq_amd import _abi, kernels  # noqa: E402
from kvq_amd.datasets import fusion_datasets as fd  # noqa: E402

CHUNK = 32      # frames per FDCT launch and D2H copy


def restart_mcus(value, W):
    """``--restart-interval``: a number of MCUs, or ``row`` = ceil(W / 16), one interval per MCU row of a frame W pixels wide"""
    if str(value) == "row":
        return (int(W) + 15) // 16
    try:
        return int(value)
    except ValueError:
        raise ValueError(f"--restart-interval must be a number of MCUs or 'row', got {value!r}") from None


def transcode(src, dst, quality=90, fps=None, restart_interval=0, yuv_matrix="bt601", device=None, entropy=None):
    """-> the number of frames written.  ``entropy``: ``MjpegWriter``'s.  ``fps`` None: the source's rate, 30 when it has none.  ``restart_interval``: MCUs, or "row"."""
    device = device or ("cuda" if torch.cuda.is_available() else "cpu")
    vr = fd.open_video(src, yuv_matrix)
    restart_interval = restart_mcus(restart_interval, getattr(vr, "W", None) or np.asarray(vr[0]).shape[1])
    rate = fps if fps is not None else (getattr(vr, "fps", None) or 30.0)
    with fd.MjpegWriter(dst, rate, quality=quality, restart_interval=restart_interval, entropy=entropy) as w:
        for lo in range(0, len(vr), CHUNK):
            frames = fd._frames_to_device(vr, np.arange(lo, min(lo + CHUNK, len(vr))), device)
            if isinstance(frames, kernels.I420Frames):
                if frames.format != _abi.SRC_I420_BT601_FULL:
                    frames = frames.to_rgb()
            else:
                frames = frames.permute(3, 0, 1, 2).contiguous()          # (n, H, W, 3) -> (3, n, H, W)
            w.write(frames)
    return w.frames


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--fps", type=float, default=None)
    ap.add_argument("--restart-interval", default="0", help="MCUs between RSTn markers (0: none), or 'row': one interval per MCU row")
    ap.add_argument("--yuv-matrix", default="bt601", choices=("bt601", "bt709"))
    ap.add_argument("--device", default=None, choices=("cuda", "cpu"))
    ap.add_argument("--entropy", default=None, choices=fd.JPEG_ENTROPY_MODES, help="where the frames are entropy-coded (default: the writer's)")
    a = ap.parse_args()
    n = transcode(a.src, a.dst, a.quality, a.fps, a.restart_interval, a.yuv_matrix, a.device, a.entropy)
    size = (sum(os.path.getsize(os.path.join(a.dst, f)) for f in os.listdir(a.dst)) if os.path.isdir(a.dst) else os.path.getsize(a.dst))
    print(f"{a.dst}: {n} frames, {size} bytes")


if __name__ == "__main__":
    main()
