"""numpy restatement of the quality paint (include/kvq_hip.h, kvq_quality_paint): which source rectangle a feature token saw, and
the heat / cover / overlay arithmetic in the stated fp32 and integer order.  A helper for the tests, not a conftest.

The token rectangles are checked against the reference's own sampler through tests/golden/qmap.npz (test_quality_map_cpu.py);
the GPU results are checked against this file bit for bit (test_gpu_quality_map.py)."""
import numpy as np

F32 = np.float32


def supported(T, D, Hf, Wf, Fh, Fw, fs_h, fs_w, aligned, cell=8, n_clips=1):
    """the rule of kvq_quality_paint_supported"""
    if min(T, D, Hf, Wf, Fh, Fw, fs_h, fs_w, aligned) <= 0 or not 1 <= n_clips <= 16:
        return False
    if cell not in (1, 2, 4, 8, 16, 32) or T != 2 * D or aligned % 2 or T % aligned or Hf * Wf > 1024:
        return False
    if (Fh * fs_h) % Hf or (Fw * fs_w) % Wf:
        return False
    sh, sw = Fh * fs_h // Hf, Fw * fs_w // Wf
    return fs_h % sh == 0 and fs_w % sw == 0


def token_rects(hoff, woff, D, Hf, Wf, fs_h, fs_w, aligned):
    """hoff / woff int [Fh][Fw][T/aligned] absolute patch origins -> (r0 [D][Hf][Wf], c0 [D][Hf][Wf], sh, sw): token (d, i', j') saw
    source rows r0 .. r0+sh-1 and columns c0 .. c0+sw-1 on clip frames 2d and 2d+1"""
    hoff, woff = np.asarray(hoff, np.int64), np.asarray(woff, np.int64)
    Fh, Fw = hoff.shape[:2]
    sh, sw = Fh * fs_h // Hf, Fw * fs_w // Wf
    r0 = np.zeros((D, Hf, Wf), np.int64)
    c0 = np.zeros((D, Hf, Wf), np.int64)
    for d in range(D):
        tt = 2 * d // aligned
        for ip in range(Hf):
            for jp in range(Wf):
                i, j = ip * sh // fs_h, jp * sw // fs_w
                r0[d, ip, jp] = hoff[i, j, tt] + (ip * sh) % fs_h
                c0[d, ip, jp] = woff[i, j, tt] + (jp * sw) % fs_w
    return r0, c0, sh, sw


def token_ids(r0, c0, sh, sw, Hs, Ws):
    """int16 [D][Hs][Ws]: 1 + the row-major (i', j') index of the token that saw the pixel, 0 = none; asserts no pixel is seen twice"""
    D, Hf, Wf = r0.shape
    out = np.zeros((D, Hs, Ws), np.int16)
    for d in range(D):
        for ip in range(Hf):
            for jp in range(Wf):
                y, x = int(r0[d, ip, jp]), int(c0[d, ip, jp])
                assert (out[d, y:y + sh, x:x + sw] == 0).all(), "two tokens saw one pixel"
                out[d, y:y + sh, x:x + sw] = ip * Wf + jp + 1
    return out


def _overlap(lo, size, cell, n_out, limit):
    """integer overlap of [lo, lo+size) with every output block [cell k, min(cell k + cell, limit))"""
    k = np.arange(n_out, dtype=np.int64)
    b0, b1 = k * cell, np.minimum(k * cell + cell, limit)
    return np.maximum(np.minimum(lo + size, b1) - np.maximum(lo, b0), 0)


def paint(r0, c0, sh, sw, scores, Hs, Ws, cell):
    """scores fp32 [D][Hf][Wf] -> (heat, cover) fp32 [D][ceil(Hs/cell)][ceil(Ws/cell)].  Per output pixel the tokens with a
    positive overlap are summed in row-major (i', j') order from 0: acc = fl(acc + fl(float(area) * s)), area summed in integers;
    heat = fl(acc / float(sum area)) (0 where nothing overlaps), cover = fl(float(sum area) / float(block pixels))."""
    scores = np.asarray(scores, F32)
    D, Hf, Wf = r0.shape
    Ho, Wo = -(-Hs // cell), -(-Ws // cell)
    ky, kx = np.arange(Ho, dtype=np.int64), np.arange(Wo, dtype=np.int64)
    block = np.outer(np.minimum(ky * cell + cell, Hs) - ky * cell, np.minimum(kx * cell + cell, Ws) - kx * cell)
    heat, cover = np.zeros((D, Ho, Wo), F32), np.zeros((D, Ho, Wo), F32)
    for d in range(D):
        area_sum = np.zeros((Ho, Wo), np.int64)
        acc = np.zeros((Ho, Wo), F32)
        for ip in range(Hf):
            for jp in range(Wf):
                ah = _overlap(int(r0[d, ip, jp]), sh, cell, Ho, Hs)
                aw = _overlap(int(c0[d, ip, jp]), sw, cell, Wo, Ws)
                ys, xs = np.nonzero(ah)[0], np.nonzero(aw)[0]
                if ys.size == 0 or xs.size == 0:
                    continue
                sl = (slice(ys[0], ys[-1] + 1), slice(xs[0], xs[-1] + 1))        # overlaps are contiguous runs
                area = np.outer(ah[sl[0]], aw[sl[1]])
                area_sum[sl] += area
                acc[sl] = acc[sl] + area.astype(F32) * scores[d, ip, jp]          # fp32 product, then fp32 sum: two roundings
        hit = area_sum > 0
        heat[d][hit] = acc[hit] / area_sum[hit].astype(F32)
        cover[d] = area_sum.astype(F32) / block.astype(F32)
    return heat, cover


def overlay(frames, heat1, cover1, lo, hi, alpha=128, dim=96):
    """frames uint8 [3][Hs][Ws] (the source's channel order), heat1 / cover1: the cell == 1 paint of one depth slice [Hs][Ws]
    -> uint8 [3][Hs][Ws].  q = rint(min(max((s - lo) * inv, 0), 1) * 255) with inv = 1 / (hi - lo) in fp32 (fmax / fmin: a NaN from
    hi == lo counts as 0), colour (255 - q, q, 0); covered: (src (256 - alpha) + colour alpha + 128) >> 8; else (src dim + 128) >> 8."""
    lo, hi = F32(lo), F32(hi)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F32(1.0) / (hi - lo)
        t = np.fmin(np.fmax((np.asarray(heat1, F32) - lo) * inv, F32(0.0)), F32(1.0))
    q = np.rint(t * F32(255.0)).astype(np.int64)
    colour = np.stack([255 - q, q, np.zeros_like(q)])
    src = np.asarray(frames).astype(np.int64)
    covered = (src * (256 - alpha) + colour * alpha + 128) >> 8
    plain = (src * dim + 128) >> 8
    return np.where(np.asarray(cover1) > 0, covered, plain).astype(np.uint8)
