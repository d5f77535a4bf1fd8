"""Independent numpy restatement of the library's planar YUV 4:2:0 -> RGB conversion (include/kvq_hip.h: kvq_yuv420_to_rgb), written from
the specification and sharing no code with the package: the coefficients are derived here from (Kr, Kb), the frame layout is unpacked
here, and a Y4M writer for the reader tests lives here too.

Formats (KvqSrcFormat): 2 = BT.601 limited, 3 = BT.601 full, 4 = BT.709 limited, 5 = BT.709 full.
  q = floor(c * 65536 + 0.5) for the five coefficients; R = clamp((qy (Y - yoff) + qrv (V - 128) + 32768) >> 16, 0, 255), G and B alike;
  pixel (y, x) takes chroma sample (y >> 1, x >> 1); a frame is Y (H x W) | U | V (ceil(H/2) x ceil(W/2)), frames back to back.
"""
import math

import numpy as np

FORMATS = (2, 3, 4, 5)
KR_KB = {2: (0.299, 0.114), 3: (0.299, 0.114), 4: (0.2126, 0.0722), 5: (0.2126, 0.0722)}
FULL = {2: False, 3: True, 4: False, 5: True}


def float_matrix(fmt):
    """(sy, rv, gu, gv, bu, yoff) as floats"""
    kr, kb = KR_KB[fmt]
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if FULL[fmt] else (255.0 / 219.0, 255.0 / 224.0)
    return (sy, 2.0 * (1.0 - kr) * sc, -2.0 * (1.0 - kb) * kb / kg * sc, -2.0 * (1.0 - kr) * kr / kg * sc, 2.0 * (1.0 - kb) * sc,
            0 if FULL[fmt] else 16)


def coeffs(fmt):
    """(qy, qrv, qgu, qgv, qbu, yoff) as Python integers"""
    m = float_matrix(fmt)
    return tuple(int(math.floor(c * 65536.0 + 0.5)) for c in m[:5]) + (m[5],)


def convert(y, u, v, fmt):
    """integer conversion of broadcastable Y, U, V arrays -> uint8 (..., 3); int64 inside, so nothing can wrap here"""
    qy, qrv, qgu, qgv, qbu, yoff = coeffs(fmt)
    y, u, v = np.asarray(y, np.int64) - yoff, np.asarray(u, np.int64) - 128, np.asarray(v, np.int64) - 128
    luma = qy * y + 32768
    rgb = np.stack(np.broadcast_arrays(luma + qrv * v, luma + qgu * u + qgv * v, luma + qbu * u), axis=-1) >> 16
    return np.clip(rgb, 0, 255).astype(np.uint8)


def convert_float(y, u, v, fmt):
    """floor(float64 + 0.5), clamped: what the integer form approximates"""
    sy, rv, gu, gv, bu, yoff = float_matrix(fmt)
    y, u, v = np.asarray(y, np.float64) - yoff, np.asarray(u, np.float64) - 128.0, np.asarray(v, np.float64) - 128.0
    rgb = np.stack(np.broadcast_arrays(sy * y + rv * v, sy * y + gu * u + gv * v, sy * y + bu * u), axis=-1)
    return np.clip(np.floor(rgb + 0.5), 0, 255).astype(np.uint8)


def frame_bytes(H, W):
    return H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)


def planes(frame, H, W):
    """one I420 frame (frame_bytes,) -> Y (H, W), U, V (ceil(H/2), ceil(W/2))"""
    ch, cw = (H + 1) // 2, (W + 1) // 2
    assert frame.shape == (frame_bytes(H, W),)
    return frame[:H * W].reshape(H, W), frame[H * W:H * W + ch * cw].reshape(ch, cw), frame[H * W + ch * cw:].reshape(ch, cw)


def frame_rgb(frame, H, W, fmt):
    """one I420 frame -> uint8 (H, W, 3), nearest chroma"""
    y, u, v = planes(frame, H, W)
    yy, xx = np.arange(H)[:, None] >> 1, np.arange(W)[None, :] >> 1
    return convert(y, u[yy, xx], v[yy, xx], fmt)


def frames_rgb(frames, H, W, fmt):
    """I420 frames (T, frame_bytes) -> uint8 (3, T, H, W): the layout the uint8 consumers read"""
    return np.ascontiguousarray(np.stack([frame_rgb(f, H, W, fmt) for f in frames], 0).transpose(3, 0, 1, 2))


def random_frames(seed, T, H, W):
    """seeded I420 frames with the whole byte range in every plane (smooth ramps + noise would hide chroma indexing mistakes)"""
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (T, frame_bytes(H, W)), dtype=np.uint8)


def write_y4m(path, frames, H, W, chroma="C420jpeg", extra=(), frame_header=b"FRAME\n", truncate=0):
    """a YUV4MPEG2 file of the I420 frames (T, frame_bytes); ``chroma`` None omits the tag; ``truncate`` drops bytes off the end"""
    tags = ["YUV4MPEG2", f"W{W}", f"H{H}", "F30:1", "Ip", "A1:1"] + ([chroma] if chroma else []) + list(extra)
    blob = (" ".join(tags) + "\n").encode("ascii") + b"".join(frame_header + f.tobytes() for f in frames)
    with open(path, "wb") as f:
        f.write(blob[:len(blob) - truncate] if truncate else blob)
