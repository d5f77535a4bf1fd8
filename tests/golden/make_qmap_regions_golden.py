"""Emit tests/golden/qmap_regions.npz: what the tests of the quality paint through KSVQE's region windows pin against the real
reference.  Runs ONLY where the reference is present (it is imported through _ref_import.py); the fixture is data only.

  <case>/*   the reference's get_spatial_fragments(9, 9, 32, 32, aligned) under torch.manual_seed on a COORDINATE video (channel 0 =
             row, 1 = column, 2 = frame) gives the 288 x 288 canvas; the reference's RegionNet_CLIP(k=49, anchor_size=32, stride=1) in
             eval mode cuts one 224 x 224 window per frame out of it, chosen from hand-made CLS maps that put a different window on
             every key frame, with the group ids of the reference's KSVQE.obtain_keyframes.  The cropped output says which source pixel
             every pixel of the trunk's input came from: scattering (token index + 1) through it gives tokid int16 [T][Hs][Ws] PER FRAME
             (0 = no token saw the pixel).  T = 8: the key frames are 1, 3 and 5, so the frame pairs (0,1), (2,3), (4,5) each straddle
             two groups.  regions [T] is the window the reference cut for each frame (found by comparing its output with the canvas);
             hoff / woff are the draws, read off the canvas.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_qmap_regions_golden.py
"""
import importlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np
import torch

from _ref_import import import_reference

# (T, H, W, aligned)
CASES = {
    "300x340_a8": (8, 300, 340, 8),
    "288x288_a2": (8, 288, 288, 2),
}
FH = FW = 9
FS = 32
ANCHOR, K = 32, 49
HF = WF = 7
# per-axis CLS profiles on the 7-cell map (nearest-upsampled to the 9 anchors by the reference) whose 7-anchor window sum peaks at
# window origin 0, 1, 2; a map is profile[row] + profile[column], so the two axes choose independently
PROFILE = {0: [2, 2, 2, 2, 2, 0, 0], 1: [1, 2, 2, 2, 2, 2, 0], 2: [0, 0, 2, 2, 2, 2, 2]}
KEY_WINDOWS = [(0, 2), (1, 1), (2, 0), (1, 2)]                   # (ry, rx) meant for key frames 0 .. 3


def cls_maps():
    maps = [np.add.outer(np.asarray(PROFILE[ry], np.float32), np.asarray(PROFILE[rx], np.float32)) for ry, rx in KEY_WINDOWS]
    return torch.from_numpy(np.stack(maps).reshape(1, len(KEY_WINDOWS), HF * WF))


def main():
    ref = import_reference()
    patchnet = importlib.import_module("models.backbones.patchnet")
    ksvqe = importlib.import_module("models.backbones.KSVQE_model")
    net = patchnet.RegionNet_CLIP(k=K, anchor_size=ANCHOR, stride=1).eval()
    kk = int(round(K ** 0.5))
    nr = FH * FS // ANCHOR - kk + 1
    d = {}
    for seed, (name, (T, H, W, aligned)) in enumerate(CASES.items()):
        vid = torch.zeros(3, T, H, W)
        vid[0] = torch.arange(H, dtype=torch.float32).view(1, H, 1)
        vid[1] = torch.arange(W, dtype=torch.float32).view(1, 1, W)
        vid[2] = torch.arange(T, dtype=torch.float32).view(T, 1, 1)
        torch.manual_seed(200 + seed)
        canvas = ref.fd.get_spatial_fragments(vid, FH, FW, FS, FS, aligned=aligned)
        assert canvas.shape == (3, T, FH * FS, FW * FS)
        group_id, _ = ksvqe.KSVQE.obtain_keyframes(None, torch.zeros(1, 3, T, 4, 4))
        with torch.no_grad():
            cut = net(canvas.unsqueeze(0), cls_maps(), 0.5, group_id)[0].numpy()
        assert cut.shape == (3, T, kk * ANCHOR, kk * ANCHOR)
        canvas = canvas.numpy()
        rows, cols, frames = (cut[c].astype(np.int64) for c in range(3))
        assert (frames == np.arange(T).reshape(T, 1, 1)).all()
        regions = np.zeros(T, np.int32)
        for t in range(T):
            hits = [r for r in range(nr * nr)
                    if np.array_equal(canvas[:, t, r // nr * ANCHOR:r // nr * ANCHOR + kk * ANCHOR, r % nr * ANCHOR:r % nr * ANCHOR + kk * ANCHOR], cut[:, t])]
            assert len(hits) == 1, "the window of a frame must be identifiable from the coordinate video"
            regions[t] = hits[0]
        gid = group_id[0].numpy().astype(np.int64)
        want = np.asarray([ry * nr + rx for ry, rx in KEY_WINDOWS])[gid]
        assert np.array_equal(regions, want), (regions, want)       # the hand-made maps chose the windows they were made for
        sh, sw = kk * ANCHOR // HF, kk * ANCHOR // WF
        yy, xx = np.meshgrid(np.arange(kk * ANCHOR), np.arange(kk * ANCHOR), indexing="ij")
        tok = ((yy // sh) * WF + xx // sw + 1).astype(np.int16)
        tokid = np.zeros((T, H, W), np.int16)
        for t in range(T):
            flat = rows[t] * W + cols[t]
            assert np.unique(flat).size == flat.size, "a source pixel is covered twice"
            tokid[t].reshape(-1)[flat.reshape(-1)] = tok.reshape(-1)
        crow, ccol = canvas[0].astype(np.int64), canvas[1].astype(np.int64)
        nt = T // aligned
        hoff = np.stack([crow[tt * aligned, ::FS, ::FS] for tt in range(nt)], -1).astype(np.int32)       # [Fh][Fw][nt]
        woff = np.stack([ccol[tt * aligned, ::FS, ::FS] for tt in range(nt)], -1).astype(np.int32)
        d[f"{name}/meta"] = np.asarray([T, H, W, aligned, HF, WF, FH, FW, FS, ANCHOR, kk, kk], np.int32)
        d[f"{name}/tokid"], d[f"{name}/hoff"], d[f"{name}/woff"], d[f"{name}/regions"] = tokid, hoff, woff, regions
        d[f"{name}/group_id"] = gid.astype(np.int32)
        print(f"{name}: regions {regions.tolist()} groups {gid.tolist()} coverage {float((tokid > 0).mean()):.3f}")
    path = os.path.join(HERE, "qmap_regions.npz")
    np.savez_compressed(path, **d)
    print(f"wrote qmap_regions.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(d)} arrays")


if __name__ == "__main__":
    main()
