"""Emit tests/golden/qmap.npz: what the quality-map tests pin against the real reference.  Runs ONLY where the reference is
present (it is imported through _ref_import.py); the fixture is data only.

  head/*          the reference's VQAHead(768, 64) in eval mode on a PCG64 feature: the per-token map BEFORE the mean (a forward
                  hook on fc_last) and the score; plus the summation-order noise of that arithmetic, max |fp32 - fp64| over the map.
  paint/<case>/*  the reference's get_spatial_fragments under torch.manual_seed on a COORDINATE video (channel 0 = row, 1 = column,
                  2 = frame): its output says which source pixel every fragment pixel came from.  Scattering (token index + 1)
                  through it gives tokid int16 [D][Hs][Ws] (0 = no token saw the pixel); the draws are read off the same output.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_qmap_golden.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np
import torch

import kvq_amd  # noqa: F401  (import shim)
from kvq_amd.utils import synth
from _ref_import import import_reference

# (T, H, W, aligned, Hf, Wf): the 7 x 7 grid of 32 x 32 mini-patches; Hf = Wf = 7 is the trunk's (2, 32, 32) stride, the last case
# a token grid of twice the resolution (sh = sw = 16: two token rows per mini-patch)
CASES = {
    "240x300_a8": (8, 240, 300, 8, 7, 7),
    "270x480_a4": (8, 270, 480, 4, 7, 7),
    "540x960_a8": (16, 540, 960, 8, 7, 7),
    "224x224_a8": (8, 224, 224, 8, 7, 7),
    "231x257_a2": (8, 231, 257, 2, 7, 7),
    "270x480_a4_s16": (8, 270, 480, 4, 14, 14),
}
FH = FW = 7
FS = 32
HEAD_SEED = 5


def head_feature():
    return np.random.Generator(np.random.PCG64(HEAD_SEED)).standard_normal((2, 768, 4, 7, 7)).astype(np.float32)


def sec_head(ref, d):
    head = ref.head.VQAHead(768, 64).eval()
    w = synth.synth_vqa_head_weights(768, 64, HEAD_SEED, "stress")
    head.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    kept = []
    head.fc_last.register_forward_hook(lambda m, i, o: kept.append(o.detach()))
    x = torch.from_numpy(head_feature())
    with torch.no_grad():
        score = head(x)
        tok = kept[0]                                            # (2, 1, 4, 7, 7): qlt_score before .mean((-3, -2, -1))
        head64 = head.double()
        kept.clear()
        head64(x.double())
        tok64 = kept[0]
    assert tok.shape == (2, 1, 4, 7, 7)
    assert float((tok.mean((-3, -2, -1)) - score).abs().max()) <= 1e-6
    d["head/map"] = tok[:, 0].numpy()
    d["head/score"] = score.numpy()
    d["head/fp32_noise"] = np.float64((tok.double() - tok64).abs().max())
    print("head: map", tuple(tok.shape), "score", score.ravel().tolist(), "max |fp32 - fp64| of the map", float(d["head/fp32_noise"]))


def sec_paint(ref, d):
    for seed, (name, (T, H, W, aligned, Hf, Wf)) in enumerate(CASES.items()):
        vid = torch.zeros(3, T, H, W)
        vid[0] = torch.arange(H, dtype=torch.float32).view(1, H, 1)
        vid[1] = torch.arange(W, dtype=torch.float32).view(1, 1, W)
        vid[2] = torch.arange(T, dtype=torch.float32).view(T, 1, 1)
        torch.manual_seed(100 + seed)
        out = ref.fd.get_spatial_fragments(vid, FH, FW, FS, FS, aligned=aligned).numpy()
        assert out.shape == (3, T, FH * FS, FW * FS)
        rows, cols, frames = (out[c].astype(np.int64) for c in range(3))
        assert (frames == np.arange(T).reshape(T, 1, 1)).all()
        D, sh, sw = T // 2, FH * FS // Hf, FW * FS // Wf
        yy, xx = np.meshgrid(np.arange(FH * FS), np.arange(FW * FS), indexing="ij")
        tok = ((yy // sh) * Wf + xx // sw + 1).astype(np.int16)
        tokid = np.zeros((D, H, W), np.int16)
        for t in range(T):
            if t % 2:                                           # the two frames of a token pair share their draws
                assert (rows[t] == rows[t - 1]).all() and (cols[t] == cols[t - 1]).all()
                continue
            flat = rows[t] * W + cols[t]
            assert np.unique(flat).size == flat.size, "a source pixel is covered twice"
            tokid[t // 2].reshape(-1)[flat.reshape(-1)] = tok.reshape(-1)
        nt = T // aligned
        hoff = np.stack([rows[tt * aligned, ::FS, ::FS] for tt in range(nt)], -1).astype(np.int32)       # [Fh][Fw][nt]
        woff = np.stack([cols[tt * aligned, ::FS, ::FS] for tt in range(nt)], -1).astype(np.int32)
        d[f"paint/{name}/meta"] = np.asarray([T, H, W, aligned, Hf, Wf, FH, FW, FS], np.int32)
        d[f"paint/{name}/tokid"], d[f"paint/{name}/hoff"], d[f"paint/{name}/woff"] = tokid, hoff, woff
        print(f"paint/{name}: coverage {float((tokid > 0).mean()):.3f}")


def main():
    ref = import_reference()
    d = {}
    sec_head(ref, d)
    sec_paint(ref, d)
    path = os.path.join(HERE, "qmap.npz")
    np.savez_compressed(path, **d)
    print(f"wrote qmap.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(d)} arrays")


if __name__ == "__main__":
    main()
