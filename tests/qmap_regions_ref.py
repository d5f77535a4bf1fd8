"""numpy restatement of the quality paint through KSVQE's region windows (include/kvq_hip.h, kvq_quality_paint_regions): which source
rectangle a feature token saw when the trunk's input was one window of the fragment canvas per clip frame.  The heat / cover /
overlay arithmetic is qmap_ref's, unchanged.  A helper for the tests, not a conftest.

The rectangles are checked against the reference's own sampler and RegionNet_CLIP through tests/golden/qmap_regions.npz
(test_quality_map_regions_cpu.py); the GPU results against this file bit for bit (test_gpu_quality_map_regions.py)."""
import numpy as np

import qmap_ref as QR

F32 = np.float32


def supported(T, D, Hf, Wf, Fh, Fw, fs_h, fs_w, aligned, anchor, kh, kw, cell=8, n_clips=1, phase=0):
    """the rule of kvq_quality_paint_regions_supported, and the call's own condition on phase"""
    if min(T, D, Hf, Wf, Fh, Fw, fs_h, fs_w, aligned, anchor, kh, kw) <= 0 or not 1 <= n_clips <= 16 or phase not in (0, 1):
        return False
    if cell not in (1, 2, 4, 8, 16, 32) or T != 2 * D or aligned % 2 or T % aligned or Hf * Wf > 1024:
        return False
    if (kh * anchor) % Hf or (kw * anchor) % Wf:
        return False
    sh, sw = kh * anchor // Hf, kw * anchor // Wf
    if fs_h % sh or fs_w % sw or anchor % sh or anchor % sw:
        return False
    if (Fh * fs_h) % anchor or (Fw * fs_w) % anchor:
        return False
    return kh <= Fh * fs_h // anchor and kw <= Fw * fs_w // anchor


def window_grid(Fh, Fw, fs_h, fs_w, anchor, kh, kw):
    """(window origins per column, per row) = (gh - kh + 1, gw - kw + 1)"""
    return Fh * fs_h // anchor - kh + 1, Fw * fs_w // anchor - kw + 1


def token_rects_regions(hoff, woff, regions, D, Hf, Wf, fs_h, fs_w, aligned, anchor, kh, kw, phase):
    """hoff / woff int [Fh][Fw][T/aligned], regions int [T] (one clip) -> (r0 [D][Hf][Wf], c0, sh, sw, valid bool [D]): token
    (d, i', j') saw source rows r0 .. r0+sh-1 and columns c0 .. c0+sw-1 on clip frame 2d + phase; a slice whose region value names no
    window is not valid (its r0 / c0 are 0 and mean nothing)"""
    hoff, woff = np.asarray(hoff, np.int64), np.asarray(woff, np.int64)
    regions = np.asarray(regions, np.int64).reshape(-1)
    Fh, Fw = hoff.shape[:2]
    nry, nrx = window_grid(Fh, Fw, fs_h, fs_w, anchor, kh, kw)
    sh, sw = kh * anchor // Hf, kw * anchor // Wf
    r0 = np.zeros((D, Hf, Wf), np.int64)
    c0 = np.zeros((D, Hf, Wf), np.int64)
    valid = np.zeros(D, bool)
    for d in range(D):
        reg = int(regions[2 * d + phase])
        if not 0 <= reg < nry * nrx:
            continue
        valid[d] = True
        ry, rx = divmod(reg, nrx)
        tt = 2 * d // aligned
        for ip in range(Hf):
            for jp in range(Wf):
                y, x = ry * anchor + ip * sh, rx * anchor + jp * sw
                r0[d, ip, jp] = hoff[y // fs_h, x // fs_w, tt] + y % fs_h
                c0[d, ip, jp] = woff[y // fs_h, x // fs_w, tt] + x % fs_w
    return r0, c0, sh, sw, valid


def token_ids(r0, c0, sh, sw, valid, Hs, Ws):
    """qmap_ref.token_ids with the slices that are not valid left at 0"""
    out = QR.token_ids(r0, c0, sh, sw, Hs, Ws) if r0.shape[0] else np.zeros((0, Hs, Ws), np.int16)
    out[~valid] = 0
    return out


def paint(r0, c0, sh, sw, valid, scores, Hs, Ws, cell):
    """qmap_ref.paint; a slice that is not valid is uncovered: heat 0, cover 0"""
    heat, cover = QR.paint(r0, c0, sh, sw, scores, Hs, Ws, cell)
    heat[~valid] = 0
    cover[~valid] = 0
    return heat, cover


def overlays(frames, r0, c0, sh, sw, valid, scores, depths, phase, lo, hi, alpha=128, dim=96):
    """frames uint8 [3][T][Hs][Ws] of one clip -> uint8 [len(depths)][3][Hs][Ws]: slice n drawn on clip frame 2 depths[n] + phase"""
    frames = np.asarray(frames)
    Hs, Ws = frames.shape[2:]
    heat1, cover1 = paint(r0, c0, sh, sw, valid, scores, Hs, Ws, 1)
    return np.stack([QR.overlay(frames[:, 2 * d + phase], heat1[d], cover1[d], lo, hi, alpha, dim) for d in depths])
