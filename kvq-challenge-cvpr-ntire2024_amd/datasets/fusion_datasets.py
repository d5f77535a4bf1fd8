"""Host-side mirror of the sampler half of the reference's ``datasets/fusion_datasets.py``.

  get_spatial_fragments   (:22-121)   grid-mini-patch sampler -> ``kvq_fragment_gather`` (HIP)
  UnifiedFrameSampler     (:612-660)  temporal index sampler (host integers, numpy)
  ViewDecompositionDataset_KVQ (:930-1051), ViewDecompositionDataset_add_forSimpleVQA (:786-927)
                          the reference's dataset classes under their own names (annotation parsing, samplers, dict
                          keys), fed by a frame reader (Y4M files, decord if present, uint8 .npy stacks otherwise)
  Y4mFrameReader          uncompressed YUV4MPEG2 video, no codec library: its I420 frames go to the device as they are
                          (1.5 B/pixel) and are converted where the pixels are first touched (``kernels.I420Frames``)
  SyntheticKVQDataset     build-only: seeded post-decode frame stacks (no dataset/decoder is reachable
                          offline — SURVEY.md §8d); same dict keys.

The reference draws its random offsets inside the functions from global RNG state
(``torch.randint`` :87-98, ``np.random.randint`` :632-635).  The same calls are made here, in the
same order, so a seeded run draws the same offsets (SURVEY.md §0 trap 6); every function also accepts
the offsets explicitly, which is what the parity tests use.
Video *decode* (decord / cv2, :379-431) is outside the hot path (the reader selection incl. the cv2 fallback's
padding rule is reproduced, the codecs themselves are not part of this image): frames enter
as uint8/fp32 (C,T,H,W) tensors.
"""
from __future__ import annotations

import random as _pyrandom
from typing import Optional

import os
import threading

import numpy as np
import torch

from .. import kernels

KVQ_MEAN = (123.675, 116.28, 103.53)
KVQ_STD = (58.395, 57.12, 57.375)


def _grid(res: int, fragments: int, fsize: int):
    return [min(res // fragments * i, res - fsize) for i in range(fragments)]


def get_spatial_fragments(video, fragments_h=7, fragments_w=7, fsize_h=32, fsize_w=32, aligned=32, nfrags=1,
                          random=False, random_upsample=False, fallback_type="upsample", rnd_h=None, rnd_w=None,
                          mean=None, std=None, lazy=False, **kwargs):
    """video (C,T,H,W) uint8|fp32 on a HIP device, or ``kernels.I420Frames`` -> fp32 (C,T,Fh*fs,Fw*fs); ``lazy=True`` -> the draws and
    the frames as a one-entry ``kernels.FragmentSource`` (the trunk's embedding launch samples while it reads; ``.materialise()[0]`` is
    the tensor).  I420 frames stay I420 (the sampler converts the pixels it reads); only a source smaller than the canvas is converted
    first, for the upsample.

    ``rnd_h``/``rnd_w`` (Fh,Fw,T//aligned): offsets inside each grid cell; drawn with the reference's
    ``torch.randint`` calls when omitted.  ``mean``/``std`` fuse the dataset's normalisation (:1017-1020)."""
    if random or random_upsample:
        raise NotImplementedError("'random' / 'random_upsample' sampling is deprecated in the reference (:75)")
    if video.shape[1] == 1:
        aligned = 1
    T, H, W = video.shape[-3:]
    ratio = min(H / (fragments_h * fsize_h), W / (fragments_w * fsize_w))
    if ratio < 1:
        if fallback_type != "upsample":
            raise NotImplementedError(f"fallback_type {fallback_type!r}: the reference only knows 'upsample' (:43)")
        if H < fsize_h or W < fsize_w:
            raise ValueError(f"a {H}x{W} source is smaller than one {fsize_h}x{fsize_w} mini-patch (the reference indexes it "
                             "with negative offsets, :63-68)")
        # The reference upsamples the frames (F.interpolate(video / 255, scale_factor = 1 / ratio, bilinear) * 255, cast back,
        # :43-50) but keeps res_h / res_w of the ORIGINAL frames (:41) for the grid and the draws below: the patches are cut from
        # the upsampled frames at the small source's offsets.  Reproduced as it is; kvq_upsample_frames is ATen-CPU-exact.
        video = kernels.upsample_frames(_rgb_frames(video).contiguous(), 1 / ratio)
    assert T % aligned == 0, "Please provide match vclip and align index"
    nt = T // aligned
    hl, wl = H // fragments_h, W // fragments_w
    if rnd_h is None:
        rnd_h = (torch.randint(hl - fsize_h, (fragments_h, fragments_w, nt)) if hl > fsize_h
                 else torch.zeros((fragments_h, fragments_w, nt)).int())
    if rnd_w is None:
        rnd_w = (torch.randint(wl - fsize_w, (fragments_h, fragments_w, nt)) if wl > fsize_w
                 else torch.zeros((fragments_h, fragments_w, nt)).int())
    rnd_h = torch.as_tensor(np.asarray(rnd_h)) if not torch.is_tensor(rnd_h) else rnd_h
    rnd_w = torch.as_tensor(np.asarray(rnd_w)) if not torch.is_tensor(rnd_w) else rnd_w
    hoff = (rnd_h.cpu().long() + torch.tensor(_grid(H, fragments_h, fsize_h)).view(-1, 1, 1)).int()
    woff = (rnd_w.cpu().long() + torch.tensor(_grid(W, fragments_w, fsize_w)).view(1, -1, 1)).int()
    if lazy:
        src = kernels.FragmentSource([video.contiguous()], [hoff.to(video.device)], [woff.to(video.device)], fragments_h,
                                     fragments_w, fsize_h, fsize_w, aligned, mean=mean, std=std)
        src.upsampled = ratio < 1
        return src
    return kernels.fragment_gather(video.contiguous(), hoff.to(video.device), woff.to(video.device), fragments_h,
                                   fragments_w, fsize_h, fsize_w, aligned, mean=mean, std=std)


def _rgb_frames(video):
    """whole-frame consumers (the resize views, the upsample fallback) read RGB: I420 frames are converted once (cached)"""
    return video.to_rgb() if isinstance(video, kernels.I420Frames) else video


def get_resized_video(video, size_h=224, size_w=224, random_crop=False, arp=False, mean=None, std=None, antialias=False,
                      **kwargs):
    """Reference ``get_resized_video`` (:244-252) on the GPU: (C,T,H,W) -> (C,T,size_h,size_w), bilinear; ``antialias``:
    torchvision >= 0.17's Resize (antialiased) instead of the plain bilinear of earlier releases."""
    if random_crop:
        raise NotImplementedError("RandomResizedCrop is a training augmentation")
    if arp:
        ratio = video.shape[-2] / video.shape[-1]
        if ratio > 1:
            size_h = int(ratio * size_w)
        elif ratio < 1:
            size_w = int(size_h / ratio)
    return kernels.resize_bilinear(_rgb_frames(video).contiguous(), size_h, size_w, mean=mean, std=std, antialias=antialias)


def train_crop_offsets(resize: int, crop: int):
    """the reference's train-phase crop of the (resize, resize) frames (:308-312): ``rnd_h`` then ``rnd_w``, each
    ``random.randrange(resize - crop)`` of Python's global ``random``.  Host integers only.  ``resize == crop`` (or less) raises
    ValueError, as the reference's ``randrange(0)`` does."""
    if resize - crop <= 0:
        raise ValueError(f"train-phase crop of {crop} out of {resize}: the reference draws random.randrange({resize - crop}), an empty range")
    rnd_h = _pyrandom.randrange(resize - crop)
    rnd_w = _pyrandom.randrange(resize - crop)
    return rnd_h, rnd_w


def get_resizecrop_video(video, resize=520, crop=448, phase="test", mean=None, std=None, antialias=False, **kwargs):
    """Reference ``get_resizecrop_video`` (:299-316): resize to (resize,resize), then the centre crop
    [r//2-crop//2 : r//2+crop//2] (test phase) or the random crop of ``train_crop_offsets`` (train phase) — fused with the
    normalisation in one kernel: only the crop's pixels are computed."""
    if phase == "train":
        oy, ox = train_crop_offsets(resize, crop)
        n = crop
    else:
        oy = ox = resize // 2 - crop // 2
        n = (resize // 2 + crop // 2) - oy
    return kernels.resize_bilinear(_rgb_frames(video).contiguous(), resize, resize, crop=(oy, ox, n, n), mean=mean, std=std,
                                   antialias=antialias)


DRAW_SEED_STRIDE = 1000003


def _item_seed(index: int, draw: int) -> int:
    """the per-item seed of ``seed_per_item`` for train-phase draw ``draw`` (``set_draw``): draw 0 is 1234 + index"""
    return 1234 + index + DRAW_SEED_STRIDE * draw


def _seed_item(index: int, draw: int):
    s = _item_seed(index, draw)
    np.random.seed(s)
    _pyrandom.seed(s)
    torch.manual_seed(s)


def get_single_view(video, sample_type="aesthetic", antialias=False, **kwargs):
    """Reference ``get_single_view`` (:350-361); ``antialias`` reaches the two resize views (the fragments have no resize)."""
    if sample_type.startswith("aesthetic"):
        return get_resized_video(video, antialias=antialias, **kwargs)
    if sample_type.startswith("technical"):
        return get_spatial_fragments(video, **kwargs)
    if sample_type.startswith("simpleVQA"):
        return get_resizecrop_video(video, antialias=antialias, **kwargs)
    raise NotImplementedError


SIMPLEVQA_MEAN = (0.485, 0.456, 0.406)      # applied to 0-255 pixels WITHOUT /255, as the reference does
SIMPLEVQA_STD = (0.229, 0.224, 0.225)       # (fusion_datasets.py:811-812, 903)


class SyntheticSimpleVQADataset(torch.utils.data.Dataset):
    """Seeded stand-in for ``ViewDecompositionDataset_add_forSimpleVQA`` (:786-927): ``simpleVQA`` view =
    8 frames (clip_len 8 x frame_interval 10... positional quirk as in the reference) resized 520 -> centre
    crop 448, normalised with the reference's constants; ``feat`` = the (8, 2304) SlowFast features, read from
    ``data_prefix_3D/<video_name>/feature_{i}_{slow,fast}_feature.npy`` (:878-890) or, when
    ``compute_feat`` is set, produced in-process by the HIP SlowFast branch (BASELINE config C3)."""

    def __init__(self, opt, namelist=None, device=None):
        self.opt, self.device = opt, _default_device(device)
        self.n = int(opt.get("num_videos", 4))
        self.frames, self.h, self.w = int(opt.get("frames", 256)), int(opt.get("height", 540)), int(opt.get("width", 960))
        self.sopt = dict(opt["sample_types"]["simpleVQA"])
        s = self.sopt
        # reference: UnifiedFrameSampler(clip_len // t_frag, t_frag, frame_interval, num_clips) (:836-841)
        self.sampler = UnifiedFrameSampler(s["clip_len"] // s["t_frag"], s["t_frag"], s["frame_interval"], s["num_clips"])
        self.data_prefix_3D = opt.get("data_prefix_3D")
        self.slowfast = opt.get("compute_feat")
        g = np.random.Generator(np.random.PCG64(4321))
        self.labels = list(opt.get("labels") or g.uniform(1.0, 5.0, self.n))
        self.phase, self.draw = opt.get("phase", "test"), 0     # 'train': the view takes the reference's random train-phase crop

    def __len__(self):
        return self.n

    def set_draw(self, k: int):
        """train-phase draw ``k`` of every item (see ``SyntheticKVQDataset.set_draw``)"""
        self.draw = int(k)

    def _feat(self, i, frames_u8):
        import os
        name = f"synthetic_{i:05d}"
        if self.data_prefix_3D and os.path.isdir(os.path.join(self.data_prefix_3D, name)):
            rows = []
            for k in range(8):
                slow = np.load(os.path.join(self.data_prefix_3D, name, f"feature_{k}_slow_feature.npy")).squeeze()
                fast = np.load(os.path.join(self.data_prefix_3D, name, f"feature_{k}_fast_feature.npy")).squeeze()
                rows.append(np.concatenate([slow, fast]))
            return torch.from_numpy(np.stack(rows)).float()
        if self.slowfast is not None:          # 8 clips x 32 frames @224^2, mean .45 / std .225 (SlowFast_features.py:173-174)
            rows = []
            with torch.no_grad():
                for k in range(8):
                    clip = frames_u8[:, k * 32:(k + 1) * 32].to(self.device)
                    x = kernels.resize_bilinear(clip.contiguous(), 224, 224, mean=(0.45 * 255,) * 3, std=(0.225 * 255,) * 3)
                    slow, fast = self.slowfast.forward_clips(x.unsqueeze(0))
                    rows.append(torch.cat([slow.reshape(-1), fast.reshape(-1)]))
            return torch.stack(rows)
        return torch.zeros(8, 2304)

    def __getitem__(self, i):
        from ..utils import synth
        frames = torch.from_numpy(synth.synth_video_u8(1234 + i, self.frames, self.h, self.w))
        if self.opt.get("seed_per_item"):
            _seed_item(i, self.draw)
        inds = self.sampler(self.frames)
        clip = frames[:, torch.from_numpy(inds.astype(np.int64))].to(self.device)
        view = get_resizecrop_video(clip, self.sopt["resize"], self.sopt["crop"], "train" if self.phase == "train" else "test", mean=SIMPLEVQA_MEAN,
                                    std=SIMPLEVQA_STD, antialias=bool(self.sopt.get("antialias", False)))
        return {"simpleVQA": view, "feat": self._feat(i, frames).unsqueeze(0), "num_clips": {"simpleVQA": self.sopt["num_clips"]},
                "frame_inds": inds, "label": float(self.labels[i]), "name": f"synthetic_{i:05d}",
                "video_name": f"synthetic_{i:05d}.mp4"}


class UnifiedFrameSampler:
    """Reference ``UnifiedFrameSampler`` (:612-660): same constructor, same RNG calls, same indices."""

    def __init__(self, fsize_t, fragments_t, frame_interval=1, num_clips=1, drop_rate=0.0):
        self.fragments_t, self.fsize_t = fragments_t, fsize_t
        self.size_t = fragments_t * fsize_t
        self.frame_interval, self.num_clips, self.drop_rate = frame_interval, num_clips, drop_rate

    def get_frame_indices(self, num_frames, train=False):
        tgrids = np.array([num_frames // self.fragments_t * i for i in range(self.fragments_t)], dtype=np.int32)
        tlength = num_frames // self.fragments_t
        if tlength > self.fsize_t * self.frame_interval:
            rnd_t = np.random.randint(0, tlength - self.fsize_t * self.frame_interval, size=len(tgrids))
        else:
            rnd_t = np.zeros(len(tgrids), dtype=np.int32)
        ranges_t = np.arange(self.fsize_t)[None, :] * self.frame_interval + rnd_t[:, None] + tgrids[:, None]
        drop = _pyrandom.sample(list(range(self.fragments_t)), int(self.fragments_t * self.drop_rate))
        return np.concatenate([rt for i, rt in enumerate(ranges_t) if i not in drop])

    def __call__(self, total_frames, train=False, start_index=0):
        inds = np.concatenate([self.get_frame_indices(total_frames) for _ in range(self.num_clips)])
        return np.mod(inds + start_index, total_frames).astype(np.int32)


class SyntheticKVQDataset(torch.utils.data.Dataset):
    """Seeded stand-in for ``ViewDecompositionDataset_KVQ``: item i is a uint8 frame stack drawn from
    PCG64(1234+i) sampled into the ``technical`` view on the GPU.  ``args``:
    ``num_videos, frames, height, width, labels (optional list), sample_types.technical.{fragments_h,
    fragments_w, fsize_h, fsize_w, aligned, clip_len, frame_interval, num_clips}``.  An ``aesthetic`` entry in
    ``sample_types`` (``size_h, size_w, clip_len, frame_interval, num_clips[, antialias]``: the resized view the ConvNeXt-3D
    trunk reads) adds ``data["aesthetic"]`` through ``get_single_view``, from its own frame sampler as in the reference; with
    it, ``technical`` may be left out."""

    def __init__(self, opt, namelist=None, device=None):
        self.opt, self.device = opt, _default_device(device)
        self.n = int(opt.get("num_videos", 8))
        self.frames, self.h, self.w = int(opt.get("frames", 256)), int(opt.get("height", 540)), int(opt.get("width", 960))
        self.aopt = dict(opt["sample_types"]["aesthetic"]) if "aesthetic" in opt["sample_types"] else None
        self.sopt = dict(opt["sample_types"]["technical"]) if ("technical" in opt["sample_types"] or self.aopt is None) else None
        # the reference passes (clip_len, num_clips, frame_interval) positionally (fusion_datasets.py:962-964):
        # num_clips lands in fragments_t, so T = clip_len * num_clips frames, split into clips by the harness
        self.sampler, self.asampler = (None if s is None else UnifiedFrameSampler(s["clip_len"], s.get("num_clips", 1), s.get("frame_interval", 1))
                                       for s in (self.sopt, self.aopt))
        g = np.random.Generator(np.random.PCG64(4321))
        self.labels = list(opt.get("labels") or g.uniform(1.0, 5.0, self.n))
        self.draw = 0

    def __len__(self):
        return self.n

    def set_draw(self, k: int):
        """train-phase draw ``k`` of every item: with ``seed_per_item`` the item's seed moves by ``DRAW_SEED_STRIDE * k`` (draw 0: the
        items as they always were); without it the global RNGs simply move on, as in the reference"""
        self.draw = int(k)

    def __getitem__(self, i):
        from ..utils import synth
        s = self.sopt
        frames = torch.from_numpy(synth.synth_video_u8(1234 + i, self.frames, self.h, self.w))
        if self.opt.get("seed_per_item"):
            # the samplers draw from the process-global RNGs like the reference's (a1 / a2): seeding them per item makes item i
            # the same whatever rank builds it and whatever was built before (the 1-rank vs N-rank rehearsal of C4)
            _seed_item(i, self.draw)
        item = {"num_clips": {}}
        if s is not None:
            inds = self.sampler(self.frames)
            clip = frames[:, torch.from_numpy(inds.astype(np.int64))].to(self.device)
            item["technical"] = get_spatial_fragments(clip, s["fragments_h"], s["fragments_w"], s["fsize_h"], s["fsize_w"],
                                                      aligned=s.get("aligned", 8), mean=KVQ_MEAN, std=KVQ_STD, lazy=bool(s.get("lazy", False)))
            item["num_clips"]["technical"] = s.get("num_clips", 1)
            item["frame_inds"] = inds
        if self.aopt is not None:
            ainds = self.asampler(self.frames)
            clip = frames[:, torch.from_numpy(ainds.astype(np.int64))].to(self.device)
            item["aesthetic"] = get_single_view(clip, "aesthetic", mean=KVQ_MEAN, std=KVQ_STD, **self.aopt)
            item["num_clips"]["aesthetic"] = self.aopt.get("num_clips", 1)
            item.setdefault("frame_inds", ainds)
        item.update(label=float(self.labels[i]), name=f"synthetic_{i:05d}", video_name=f"synthetic_{i:05d}.mp4")
        return item


# ------------------------------------------------------------------------------------------------------------------
# The reference's dataset classes, under their own names, for its config/*.yml files (``data.val.type``).  Decode is
# outside the built scope: frames come from a reader object — decord when it is installed, a uint8
# ``[T, H, W, 3]`` ``.npy`` stack otherwise — and go to the device as uint8; sampling + normalisation run there.
class NpyFrameReader:
    """``len(reader)`` frames, ``reader[i]`` -> uint8 (H, W, 3): the slice of decord.VideoReader the datasets use."""

    def __init__(self, path):
        self.frames = np.load(path, mmap_mode="r")
        if self.frames.ndim != 4 or self.frames.shape[-1] != 3 or self.frames.dtype != np.uint8:
            raise ValueError(f"{path}: expected a uint8 [T, H, W, 3] frame stack, got {self.frames.dtype} {self.frames.shape}")

    def __len__(self):
        return self.frames.shape[0]

    def __getitem__(self, i):
        return np.asarray(self.frames[int(i)])

    def read_into(self, indices, out):
        """frames[indices] -> out (len(indices), H, W, 3) uint8, one copy straight from the mapped file"""
        np.take(self.frames, np.asarray(indices, np.int64), axis=0, out=out)


class Cv2FrameReader:
    """The reference's OpenCV fallback (fusion_datasets.py:398-431) as a frame reader: every frame of the file read in order by
    ``cv2.VideoCapture.read()`` and kept AS cv2 RETURNS IT (BGR — the reference stacks ``frame`` without a colour conversion, so the
    fallback path feeds BGR where decord feeds RGB; reproduced, not fixed), and a video of 130 frames or fewer padded with copies of
    its LAST frame until it holds 131 (``while len(video_frame_array) <= 130``, :413-415).  A file cv2 cannot read a single frame
    from makes the reference fail in ``np.stack`` on ``None``; here it is a ValueError naming the file.
    ``cv2`` is imported lazily (it is not part of this image: the logic is exercised in tests with a stand-in module)."""
    MIN_FRAMES = 131

    def __init__(self, path, cv2_module=None):
        if cv2_module is None:
            import cv2 as cv2_module  # noqa: N813
        cap = cv2_module.VideoCapture(path)
        frames, last = [], None
        while True:
            ret, frame = cap.read()
            if not ret:
                break
            last = frame
            frames.append(frame)
        if hasattr(cap, "release"):
            cap.release()
        if last is None:
            raise ValueError(f"{path}: OpenCV could not decode a single frame")
        while len(frames) < self.MIN_FRAMES:                 # 'too short' (:413-415)
            frames.append(last)
        self.frames = np.stack(frames, axis=0)
        if self.frames.dtype != np.uint8 or self.frames.ndim != 4:
            raise ValueError(f"{path}: expected uint8 (H, W, 3) frames from OpenCV, got {self.frames.dtype} {self.frames.shape[1:]}")

    def __len__(self):
        return self.frames.shape[0]

    def __getitem__(self, i):
        return self.frames[int(i)]

    def read_into(self, indices, out):
        np.take(self.frames, np.asarray(indices, np.int64), axis=0, out=out)


def yuv420_to_rgb_host(y, u, v, coeffs):
    """The library's YUV 4:2:0 -> RGB conversion in numpy (include/kvq_hip.h: kvq_yuv420_to_rgb; ``coeffs`` =
    ``kernels.yuv420_coeffs(format)``): planes y (H, W), u / v (ceil(H/2), ceil(W/2)) uint8 -> uint8 (H, W, 3)."""
    qy, qrv, qgu, qgv, qbu, yoff = (np.int32(c) for c in coeffs)
    H, W = y.shape
    up = lambda c: np.repeat(np.repeat(np.asarray(c, np.int32) - 128, 2, axis=0), 2, axis=1)[:H, :W]     # noqa: E731  nearest chroma
    uu, vv = up(u), up(v)
    luma = qy * (np.asarray(y, np.int32) - yoff) + np.int32(32768)
    rgb = np.stack([luma + qrv * vv, luma + qgu * uu + qgv * vv, luma + qbu * uu], axis=-1) >> 16
    return np.clip(rgb, 0, 255).astype(np.uint8)


class Y4mFrameReader:
    """An uncompressed YUV4MPEG2 (``.y4m``) file as a frame reader — no codec library.  8-bit 4:2:0 only (``C420``, ``C420jpeg``,
    ``C420mpeg2``, ``C420paldv``, or no ``C`` tag: the format's default); any other chroma tag is a ValueError naming it.
    ``XCOLORRANGE=FULL`` selects full range, ``matrix`` (``bt601`` | ``bt709``; the container does not say) the coefficients.
    The frames are found by a fixed stride: every ``FRAME`` line must equal the first, and the file must end with a whole frame.

    ``len(reader)`` frames; ``reader[i]`` -> uint8 RGB (H, W, 3) by the library's conversion on the host (generic consumers);
    ``read_i420_into(indices, out)`` -> the frames' payload bytes, Y | U | V, which is the device layout of ``kernels.I420Frames``."""
    CHROMA = ("420", "420jpeg", "420mpeg2", "420paldv")

    def __init__(self, path, matrix="bt601"):
        from .._abi import i420_format
        with open(path, "rb") as f:                      # two lines, however long the X tags make them
            line = f.readline(1 << 20)
            first = f.readline(1 << 20)
        end = len(line) - 1                              # offset of the stream header's newline
        tags = line[:end].split(b" ") if line.endswith(b"\n") else []
        if not tags or tags[0] != b"YUV4MPEG2":
            raise ValueError(f"{path}: not a YUV4MPEG2 stream (no 'YUV4MPEG2' signature line)")
        self.W = self.H = self.fps = None                # fps: the F tag's rate (frames per second), None when absent or 0:0
        full = False
        for tag in (t.decode("ascii", "replace") for t in tags[1:] if t):
            if tag[0] in "WH":
                if not tag[1:].isdigit():
                    raise ValueError(f"{path}: malformed frame size tag {tag!r} in the stream header")
                setattr(self, tag[0], int(tag[1:]))
            elif tag[0] == "F":
                num, _, den = tag[1:].partition(":")
                if not (num.isdigit() and den.isdigit()):
                    raise ValueError(f"{path}: malformed frame rate tag {tag!r} in the stream header")
                self.fps = int(num) / int(den) if int(num) and int(den) else None
            elif tag[0] == "C" and tag[1:] not in self.CHROMA:
                raise ValueError(f"{path}: chroma format {tag!r} is not supported (8-bit 4:2:0 only: " + ", ".join("C" + c for c in self.CHROMA) + ")")
            elif tag == "XCOLORRANGE=FULL":
                full = True
        if not self.W or not self.H:
            raise ValueError(f"{path}: the stream header gives no frame size (W / H tags)")
        self.format = i420_format(matrix, full)
        self.frame_bytes = kernels.i420_frame_bytes(self.H, self.W)
        size = os.path.getsize(path)
        if not ((first == b"FRAME\n" or first.startswith(b"FRAME ")) and first.endswith(b"\n")):
            raise ValueError(f"{path}: no FRAME header after the stream header" if size > end + 1 else f"{path}: the file holds no frame")
        stride = len(first) + self.frame_bytes
        n, rest = divmod(size - (end + 1), stride)
        if n == 0 or rest:
            raise ValueError(f"{path}: truncated — {size - (end + 1)} bytes after the stream header are not a whole number of "
                             f"{self.W}x{self.H} 4:2:0 frames of {stride} bytes ({n} whole, {rest} bytes left)")
        body = np.memmap(path, dtype=np.uint8, mode="r", offset=end + 1, shape=(n, stride))
        bad = np.nonzero((body[:, :len(first)] != np.frombuffer(first, np.uint8)).any(axis=1))[0]
        if bad.size:
            raise ValueError(f"{path}: frame {int(bad[0])} does not start with the FRAME header of frame 0 ({first!r}): frames are "
                             "found by a fixed stride")
        self.payload = body[:, len(first):]              # (n, frame_bytes) view of the mapped file
        self._coeffs = None

    def __len__(self):
        return self.payload.shape[0]

    def planes(self, i):
        """frame i as its (Y, U, V) planes: views of the mapped file"""
        H, W = self.H, self.W
        ch, cw = (H + 1) // 2, (W + 1) // 2
        p = self.payload[int(i)]
        return p[:H * W].reshape(H, W), p[H * W:H * W + ch * cw].reshape(ch, cw), p[H * W + ch * cw:].reshape(ch, cw)

    def __getitem__(self, i):
        if self._coeffs is None:
            self._coeffs = kernels.yuv420_coeffs(self.format)
        return yuv420_to_rgb_host(*self.planes(i), self._coeffs)

    def read_i420_into(self, indices, out):
        """payload[indices] -> out (len(indices), frame_bytes) uint8: one copy per frame straight from the mapped file"""
        for j, i in enumerate(indices):
            out[j] = self.payload[int(i)]


class MjpegFrameReader:
    """Motion-JPEG video as a frame reader — no codec library.  Every frame is one baseline 4:2:0 JPEG image (what
    ``kvq_jpeg_probe`` accepts: include/kvq_hip.h); MJPEG is intra-only, so only the frames a sampler picks are ever decoded.
    Three containers, indexed once as (offset, length) over a memory map:
      ``*.mjpeg`` / ``*.mjpg``  concatenated images, found by walking each image's segments to its EOI (an ``FF D8`` inside an APPn
                                payload is not a frame start)
      ``*.avi``                 RIFF AVI whose video stream's handler or compression is ``MJPG``: W, H and the rate from ``hdrl``,
                                the ``##dc`` / ``##db`` chunks of ``movi`` through ``idx1`` when present; a zero-length chunk repeats
                                the previous frame; OpenDML files that continue past the first RIFF chunk are refused
      a directory               its ``*.jpg`` / ``*.jpeg`` files in natural sort order (``2.jpg`` before ``10.jpg``); ``fps`` is None
    Every frame must be decodable and of the first frame's size: one that is not is a ValueError naming the file, the frame and the
    library's message.  JFIF fixes BT.601 full range, so ``format`` is ``SRC_I420_BT601_FULL`` and no ``yuv_matrix`` applies.

    ``len(reader)`` frames; ``reader[i]`` -> uint8 RGB (H, W, 3) on the host (entropy decode, the scalar twin of the IDCT launch,
    ``yuv420_to_rgb_host``); ``read_jpeg_into(indices, coef_out, qt_out)`` -> the quantised coefficients and quantiser tables
    ``kernels.jpeg_idct_i420`` takes; ``read_jpeg_bytes_into`` -> the compressed images and their segment index, what
    ``kernels.jpeg_entropy`` takes; ``restart_intervals``: per frame the MCUs between RSTn markers (0 = none), from the probe at open.
    ``H``, ``W``, ``fps``, ``format``, ``frame_bytes`` as ``Y4mFrameReader``."""

    def __init__(self, path):
        from .._abi import SRC_I420_BT601_FULL
        self.path, self.fps, self.format = path, None, SRC_I420_BT601_FULL
        if os.path.isdir(path):
            import re
            names = [f for f in os.listdir(path) if f.lower().endswith((".jpg", ".jpeg"))]
            names.sort(key=lambda f: [int(t) if t.isdigit() else t.lower() for t in re.split(r"(\d+)", f)])
            if not names:
                raise ValueError(f"{path}: frame 0: the directory holds no *.jpg / *.jpeg file")
            self._index = [(os.path.join(path, f), 0, os.path.getsize(os.path.join(path, f))) for f in names]
        elif path.lower().endswith(".avi"):
            hdr = _avi_index(path)
            if not hdr["mjpeg"]:
                raise ValueError(f"{path}: the video stream is {hdr['handler']!r} / {hdr['compression']!r}, not MJPG")
            self._index = [(path, o, n) for o, n in hdr["frames"]]
            self.fps = hdr["fps"]
            if not self._index:
                raise ValueError(f"{path}: frame 0: the AVI file holds no video chunk")
        else:
            self._index, size, pos = [], os.path.getsize(path), 0
            if size == 0:
                raise ValueError(f"{path}: frame 0: the file is empty")
            while pos < size:
                rc, info, msg = kernels.jpeg_probe(self._bytes(path, pos, size - pos))
                if rc == -2 or info.frame_bytes == 0:
                    raise ValueError(f"{path}: frame {len(self._index)} (at byte {pos}): " + (msg or "the image has no EOI marker: the stream is truncated"))
                self._index.append((path, pos, int(info.frame_bytes)))
                pos += int(info.frame_bytes)
        self.H = self.W = None
        self.restart_intervals = np.zeros(len(self._index), np.int64)      # per frame, MCUs between RSTn markers, 0 = none
        for i in range(len(self._index)):
            if self._index[i][2] == 0:
                raise ValueError(f"{self._index[i][0]}: frame {i}: the file is empty")
            rc, info, msg = kernels.jpeg_probe(self._frame(i))
            if rc == 0 and info.frame_bytes == 0:
                rc, msg = -2, "the image has no EOI marker: the frame is truncated"
            if rc == 0 and self.H is not None and (info.height, info.width) != (self.H, self.W):
                rc, msg = -2, f"a frame of {info.width} x {info.height} in a video of {self.W} x {self.H}"
            if rc:
                raise ValueError(f"{self._index[i][0]}: frame {i}: {msg}")
            if self.H is None:
                self.H, self.W = int(info.height), int(info.width)
            self.restart_intervals[i] = int(info.restart_interval)
        self.frame_bytes = kernels.i420_frame_bytes(self.H, self.W)
        self.coef_bytes = kernels.jpeg_coef_bytes(self.H, self.W)
        self._coeffs = None

    @staticmethod
    def _bytes(file, off, n):
        """n bytes of ``file`` from ``off`` as a read-only mapped uint8 array (a mapping of its own: safe from any thread)"""
        return np.memmap(file, dtype=np.uint8, mode="r", offset=off, shape=(n,))

    def _frame(self, i):
        return self._bytes(*self._index[int(i)])

    def _mapped(self, file, off, n):
        """as ``_bytes`` for the copy into staging: a stream or an AVI file is mapped ONCE per reader (slices of a read-only mapping
        are safe from any thread; a mapping per frame costs as much host time as indexing the frame), a directory's files one by one"""
        if file != self.path:
            return self._bytes(file, off, n)
        whole = self.__dict__.get("_whole")
        if whole is None:
            whole = self._whole = np.memmap(file, dtype=np.uint8, mode="r")
        return whole[off:off + n]

    def __len__(self):
        return len(self._index)

    def read_jpeg_into(self, indices, coef_out, qt_out):
        """entropy-decode frames[indices] -> coef_out int16 (n, coef_bytes / 2), qt_out uint16 (n, 3, 64): host numpy views (pinned
        staging); the library call releases the GIL"""
        for j, i in enumerate(indices):
            file, off, n = self._index[int(i)]
            rc, msg = kernels.jpeg_coeffs(self._bytes(file, off, n), coef_out[j], qt_out[j])
            if rc:
                raise ValueError(f"{file}: frame {int(i)}: {msg}")

    def segment_counts(self, indices):
        """per frame of ``indices`` the segments ``kvq_jpeg_index`` finds: one per restart interval, one for a frame without DRI"""
        ri = self.restart_intervals[np.asarray(indices, np.int64)]
        nc = self.coef_bytes // 768
        return np.where(ri > 0, -(-nc // np.maximum(ri, 1)), 1).astype(np.int64)

    def read_jpeg_bytes_into(self, indices, data_out, offsets, desc_out, segs_out, seg_offsets, tables_out, qt_out):
        """frames[indices] as they are, for the entropy decode on the device: the image of frame j copied to ``data_out[offsets[j]:]``
        (uint8), its segment index to ``segs_out[seg_offsets[j]:]`` (uint32 (n, 2), ``segment_counts`` entries), its table set to
        ``tables_out[j]`` (uint8 (JPEG_TABLES_BYTES,)), its quantiser tables to ``qt_out[j]`` and ``desc_out[j]`` = {offset, first
        segment, nseg, restart interval, 0}; host numpy views (pinned staging); the library call releases the GIL.  A frame the
        index refuses gets nseg = 0: the launch skips it and the caller hands it to ``kvq_jpeg_coeffs``, whose verdict counts."""
        for j, i in enumerate(indices):
            file, off, n = self._index[int(i)]
            dst = data_out[int(offsets[j]):int(offsets[j]) + n]
            dst[...] = self._mapped(file, off, n)
            s0, cap = int(seg_offsets[j]), int(seg_offsets[j + 1] - seg_offsets[j])
            rc, info, nseg, _ = kernels.jpeg_index(dst, segs_out[s0:s0 + cap], tables_out[j], qt_out[j])
            desc_out[j] = (int(offsets[j]), s0, nseg if rc == 0 and nseg == cap else 0, int(self.restart_intervals[int(i)]), 0)

    def i420(self, i):
        """frame i as its I420 bytes (frame_bytes,), decoded on the host"""
        coef, qt = np.empty((1, self.coef_bytes // 2), np.int16), np.empty((1, 3, 64), np.uint16)
        self.read_jpeg_into([i], coef, qt)
        return kernels.jpeg_idct_i420_host(coef, qt, self.H, self.W)[0]

    def __getitem__(self, i):
        if self._coeffs is None:
            self._coeffs = kernels.yuv420_coeffs(self.format)
        H, W = self.H, self.W
        ch, cw = (H + 1) // 2, (W + 1) // 2
        p = self.i420(i)
        return yuv420_to_rgb_host(p[:H * W].reshape(H, W), p[H * W:H * W + ch * cw].reshape(ch, cw), p[H * W + ch * cw:].reshape(ch, cw),
                                  self._coeffs)


def _avi_index(path, frames=True):
    """The first RIFF chunk of an AVI file -> dict(mjpeg, handler, compression, W, H, fps, frames [(offset, length)]) for its first
    video stream.  ``frames`` is filled for an MJPG stream only (from ``idx1`` when present, else by walking ``movi``)."""
    import struct
    mm = np.memmap(path, dtype=np.uint8, mode="r")
    size = mm.shape[0]
    u32 = lambda o: int.from_bytes(bytes(mm[o:o + 4]), "little")     # noqa: E731
    tag = lambda o: bytes(mm[o:o + 4])                               # noqa: E731
    if size < 12 or tag(0) != b"RIFF" or tag(8) != b"AVI ":
        raise ValueError(f"{path}: not a RIFF AVI file")
    end = min(size, 8 + u32(4))
    out = dict(mjpeg=False, handler=b"", compression=b"", W=0, H=0, fps=None, frames=[])
    stream, n_strl, movi, idx1 = None, 0, None, None

    def walk(lo, hi, depth):
        nonlocal stream, n_strl, movi, idx1
        o = lo
        while o + 8 <= hi:
            cid, n = tag(o), u32(o + 4)
            body = o + 8
            if cid == b"LIST" and body + 4 <= hi:
                kind = tag(body)
                if kind == b"movi":
                    movi = (body, min(hi, body + n))
                elif kind in (b"hdrl", b"strl"):
                    walk(body + 4, min(hi, body + n), depth + 1)
                    n_strl += kind == b"strl"
            elif cid == b"strh" and stream is None and tag(body) == b"vids" and n >= 32:
                stream = n_strl
                out["handler"] = tag(body + 4)
                scale, rate = u32(body + 20), u32(body + 24)
                out["fps"] = rate / scale if rate and scale else None
            elif cid == b"strf" and stream == n_strl and not out["W"] and n >= 20:
                out["W"], out["H"] = u32(body + 4), abs(struct.unpack("<i", bytes(mm[body + 8:body + 12]))[0])
                out["compression"] = tag(body + 16)
            elif cid == b"idx1":
                idx1 = (body, min(hi, body + n))
            o = body + n + (n & 1)

    walk(12, end, 0)
    out["mjpeg"] = stream is not None and b"MJPG" in (out["handler"].upper(), out["compression"].upper())
    if not out["mjpeg"] or not frames:
        return out
    if end + 12 <= size and tag(end) == b"RIFF" and tag(end + 8) == b"AVIX":
        raise ValueError(f"{path}: an OpenDML AVI that continues past its first RIFF chunk (AVIX) is not read")
    if movi is None:
        raise ValueError(f"{path}: frame 0: the AVI file has no movi list")
    ids = (b"%02ddc" % stream, b"%02ddb" % stream)
    chunks = []                                                       # (offset of the data, length)
    if idx1 is not None:
        ent = np.frombuffer(bytes(mm[idx1[0]:idx1[0] + (idx1[1] - idx1[0]) // 16 * 16]), dtype="<u4").reshape(-1, 4)
        base = None
        for cid_u, _, off, n in ent.tolist():
            cid = cid_u.to_bytes(4, "little")
            if cid not in ids:
                continue
            if base is None:                                          # offsets count from the 'movi' tag, or in some files from byte 0
                base = movi[0] if movi[0] + off + 8 <= size and tag(movi[0] + off) == cid else 0
            o = base + off
            if o + 8 + n > size or tag(o) != cid:
                raise ValueError(f"{path}: frame {len(chunks)}: the idx1 entry points outside the file or at no {cid.decode()} chunk")
            chunks.append((o + 8, n))
    else:
        def movi_walk(lo, hi):
            o = lo
            while o + 8 <= hi:
                cid, n = tag(o), u32(o + 4)
                if cid == b"LIST":
                    movi_walk(o + 12, min(hi, o + 8 + n))
                elif cid in ids:
                    if o + 8 + n > size:
                        raise ValueError(f"{path}: frame {len(chunks)}: the chunk is cut short by the end of the file")
                    chunks.append((o + 8, n))
                o += 8 + n + (n & 1)
        movi_walk(movi[0] + 4, movi[1])
    for k, (o, n) in enumerate(chunks):
        if n == 0:                                                    # a dropped frame: show the previous one again
            if not out["frames"]:
                raise ValueError(f"{path}: frame 0: a zero-length chunk with no frame before it")
            out["frames"].append(out["frames"][-1])
        else:
            out["frames"].append((o, n))
    return out


def open_video(path, yuv_matrix="bt601"):
    """Frame reader for ``path``: a ``*.y4m`` file by ``Y4mFrameReader`` (``yuv_matrix``: its conversion matrix); Motion-JPEG — a
    ``*.mjpeg`` / ``*.mjpg`` stream, an ``*.avi`` file whose video stream is ``MJPG``, a directory of ``*.jpg`` frames — by
    ``MjpegFrameReader`` (``yuv_matrix`` does not apply: JFIF fixes BT.601 full range); ``<path>`` itself or
    ``<path>.npy`` as a frame stack (this build's decode-free entries), else
    decord.VideoReader (fusion_datasets.py:381-383), else — decord missing, or failing on this file: the reference wraps the decord
    branch in a bare ``try`` — the OpenCV fallback (:398-431, ``Cv2FrameReader``)."""
    import os
    if os.path.isdir(path):                                                                        # a directory of frames, whatever its name
        return MjpegFrameReader(path)
    if path.endswith(".y4m") and (os.path.exists(path) or not os.path.exists(path + ".npy")):      # a missing file with a decoded
        return Y4mFrameReader(path, yuv_matrix)                                                    # .npy beside its name: the stack
    if path.lower().endswith((".mjpeg", ".mjpg")) and os.path.exists(path):
        return MjpegFrameReader(path)
    if path.lower().endswith(".avi") and os.path.isfile(path) and _avi_is_mjpeg(path):
        return MjpegFrameReader(path)
    if path.endswith(".npy"):
        return NpyFrameReader(path)
    if os.path.exists(path + ".npy"):
        return NpyFrameReader(path + ".npy")
    decord_error = None
    try:
        from decord import VideoReader
        return VideoReader(path)
    except Exception as e:  # noqa: BLE001  (the reference: ``except:`` around the whole decord branch)
        decord_error = e
    try:
        return Cv2FrameReader(path)
    except ImportError as e:
        raise ImportError(f"cannot read {path}: video decode needs decord or OpenCV (neither is part of this image: SURVEY.md §8 f2; "
                          f"decord: {type(decord_error).__name__}: {decord_error}) — or provide the decoded frames as a uint8 "
                          f"[T,H,W,3] array in {path}.npy, or the video as an uncompressed .y4m file or as Motion-JPEG (.mjpeg, MJPG .avi, "
                          f"a directory of .jpg frames)") from e


def _avi_is_mjpeg(path):
    """True: ``path`` is a RIFF AVI whose first video stream is MJPG; any other file goes the way it always went"""
    try:
        return bool(_avi_index(path, frames=False)["mjpeg"])
    except (OSError, ValueError):
        return False


class _Staging:
    """Reusable PINNED host buffers for the frames of one video (two per thread, alternating: the H2D copy of one video
    overlaps the host-side gather of the next; a buffer is rewritten only after its copy's event has completed)."""
    _local = threading.local()

    @classmethod
    def get(cls, nbytes):
        st = cls._local.__dict__.setdefault("slots", {"i": 0, "buf": [None, None], "ev": [None, None]})
        k = st["i"] = 1 - st["i"]
        if st["buf"][k] is None or st["buf"][k].numel() < nbytes:
            buf = torch.empty(int(nbytes * 1.25), dtype=torch.uint8)
            st["buf"][k] = buf.pin_memory() if torch.cuda.is_available() else buf
        elif st["ev"][k] is not None:
            st["ev"][k].synchronize()
        return st, k


_COPY_POOL = None
_COPY_THREADS = 4


def _frames_to_device(vr, uniq, device, entropy=None):
    """The sampled frames ``uniq`` of a reader -> ONE uint8 (n, H, W, 3) device tensor: gathered into pinned staging memory
    by a few host threads (numpy copies release the GIL), then a single asynchronous H2D copy on the current stream.
    A reader of I420 frames (``read_i420_into``: ``Y4mFrameReader``) stages its payload as it is — 1.5 B/pixel through the gather
    and the copy instead of 3 — and the result is a ``kernels.I420Frames`` (n, frame_bytes).
    A Motion-JPEG reader (``read_jpeg_into``: ``MjpegFrameReader``) goes through ``_jpeg_frames_to_device``; ``entropy`` ("auto" |
    "host" | "device", None: the module's ``JPEG_ENTROPY``) says where its frames are entropy-decoded and applies to no other reader."""
    if hasattr(vr, "read_jpeg_into"):
        return _jpeg_frames_to_device(vr, uniq, device, entropy)
    i420 = hasattr(vr, "read_i420_into")
    if i420:
        first, read = None, vr.read_i420_into
        n, shape = len(uniq), (vr.frame_bytes,)
    else:
        first = vr[int(uniq[0])]
        first = first.asnumpy() if hasattr(first, "asnumpy") else np.asarray(first)
        n, shape, read = len(uniq), tuple(first.shape), getattr(vr, "read_into", None)
    nbytes = n * int(np.prod(shape))
    st, k = _Staging.get(nbytes)
    stage = st["buf"][k][:nbytes].view((n,) + shape)
    host = stage.numpy()
    if read is not None:
        list(_fan_out(n, n // 8, lambda a, b: read(uniq[a:b], host[a:b])))
    elif hasattr(vr, "get_batch"):                      # decord: one decode call for all frames
        host[...] = vr.get_batch([int(i) for i in uniq]).asnumpy()
    else:
        host[0] = first
        for j in range(1, n):
            f = vr[int(uniq[j])]
            host[j] = f.asnumpy() if hasattr(f, "asnumpy") else np.asarray(f)
    dev = stage.to(device, non_blocking=True)
    if dev.is_cuda:
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev.device))
        st["ev"][k] = ev
    return kernels.I420Frames(dev, vr.H, vr.W, vr.format) if i420 else dev


def _copy_pool():
    global _COPY_POOL
    if _COPY_POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _COPY_POOL = ThreadPoolExecutor(max_workers=_COPY_THREADS, thread_name_prefix="kvq-copy")
    return _COPY_POOL


def _fan_out(n, chunks, job):
    """``job(a, b)`` on the copy pool's threads for the at most min(``_COPY_THREADS``, ``chunks``) ranges [a, b) that split range(n)
    evenly: all are submitted at once, the results come in order as they are asked for"""
    bounds = np.linspace(0, n, max(1, min(_COPY_THREADS, chunks)) + 1).astype(int)
    jobs = [_copy_pool().submit(job, a, b) for a, b in zip(bounds[:-1], bounds[1:]) if b > a]
    return map(lambda j: j.result(), jobs)


JPEG_ENTROPY = "auto"                                    # the default of ``_frames_to_device(..., jpeg_entropy=None)``
JPEG_ENTROPY_MODES = ("auto", "host", "device")
# what "auto" may choose for a GPU target when every frame of the call has a restart interval: README.md, "Motion-JPEG input"
_JPEG_ENTROPY_AUTO_DEVICE = True


def jpeg_entropy_mode(value=None):
    """``value`` (None: the module default ``JPEG_ENTROPY``) as one of "auto" | "host" | "device", else a ValueError naming the three"""
    value = JPEG_ENTROPY if value is None else value
    if value not in JPEG_ENTROPY_MODES:
        raise ValueError(f"jpeg_entropy must be one of 'auto', 'host', 'device', got {value!r}")
    return value


def _jpeg_frames_to_device(vr, uniq, device, entropy=None):
    """The sampled frames of a Motion-JPEG reader -> ``kernels.I420Frames``.  ``entropy`` (None: ``JPEG_ENTROPY``):
      "host"    the host threads of the copy pool entropy-decode the frames into pinned staging (quantised int16 coefficients,
                3 B/pixel, then the quantiser tables; the library calls release the GIL), ONE asynchronous H2D copy carries both, ONE
                ``jpeg_idct_i420`` launch on the current stream reconstructs the frames.  Without a device the scalar twin of the
                launch runs instead (bit-equal).
      "device"  ``_jpeg_frames_entropy_on_device``: the compressed bytes go up and ``jpeg_entropy`` decodes them
      "auto"    "device" for a GPU target when every frame of the call has a restart interval, "host" otherwise"""
    entropy = jpeg_entropy_mode(entropy)
    on_gpu = torch.device(device).type == "cuda"
    if entropy == "auto":
        entropy = "device" if _JPEG_ENTROPY_AUTO_DEVICE and on_gpu and bool((vr.restart_intervals[np.asarray(uniq, np.int64)] > 0).all()) else "host"
    if entropy == "device":
        return _jpeg_frames_entropy_on_device(vr, uniq, device)
    n, cb = len(uniq), vr.coef_bytes
    nbytes = n * (cb + 384)                              # cb is a multiple of 768: the tables start 16-byte aligned
    st, k = _Staging.get(nbytes)
    stage = st["buf"][k][:nbytes]
    host = stage.numpy()
    coef, qt = host[:n * cb].view(np.int16).reshape(n, cb // 2), host[n * cb:].view(np.uint16).reshape(n, 3, 64)
    list(_fan_out(n, n, lambda a, b: vr.read_jpeg_into(uniq[a:b], coef[a:b], qt[a:b])))
    if not on_gpu:
        return kernels.I420Frames(torch.from_numpy(kernels.jpeg_idct_i420_host(coef, qt, vr.H, vr.W)), vr.H, vr.W, vr.format)
    dev = stage.to(device, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev.device))
    st["ev"][k] = ev
    return kernels.jpeg_idct_i420(dev[:n * cb].view(torch.int16).view(n, cb // 2), dev[n * cb:].view(torch.uint16).view(n, 3, 64), vr.H, vr.W)


class _StatusStaging:
    """a small pinned buffer per thread for the status words of ``jpeg_entropy`` (its D2H copy is waited for before the call returns)"""
    _local = threading.local()

    @classmethod
    def get(cls, n):
        buf = getattr(cls._local, "buf", None)
        if buf is None or buf.numel() < n:
            buf = cls._local.buf = torch.empty(max(1024, int(n * 1.25)), dtype=torch.int32).pin_memory()
        return buf[:n]


def _jpeg_frames_entropy_on_device(vr, uniq, device):
    """``_jpeg_frames_to_device`` with the entropy decode on the device.  The copy pool's threads copy the COMPRESSED images into pinned
    staging and index their segments (``read_jpeg_bytes_into``: a marker walk, no decode); identical table sets are kept once; ONE
    H2D copy carries quantiser tables, descriptors, segments, bytes and table sets; ``jpeg_entropy`` decodes every restart interval
    (a frame without DRI: one segment) in one lane; ONE small D2H copy brings the status words back behind an event this function
    waits for.  Every frame with a status other than 0 — and every frame the index refused — is decoded again by
    ``kvq_jpeg_coeffs`` on the host, whose verdict is final: an error is the ValueError of the host path, a success sends that frame's
    coefficients up in place of the device's.  The unchanged ``jpeg_idct_i420`` launch follows.  Without a device the host twins of
    both launches run (bit-equal)."""
    n, cb, TB = len(uniq), vr.coef_bytes, kernels.JPEG_TABLES_BYTES
    sizes = np.array([vr._index[int(i)][2] for i in uniq], np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    seg_offsets = np.concatenate([[0], np.cumsum(vr.segment_counts(uniq))])
    nseg, ndata = int(seg_offsets[-1]), int(offsets[-1])
    o_desc = n * 384
    o_segs = o_desc + n * 20
    o_data = o_segs + nseg * 8
    o_tab = -(-(o_data + ndata) // 4) * 4
    nbytes = o_tab + n * TB                              # room for one table set per frame; what is used goes up
    if o_tab >= 1 << 32:
        raise ValueError(f"{vr.path}: {n} frames of {ndata} compressed bytes in one call (the offsets are 32-bit)")
    st, k = _Staging.get(nbytes)
    stage = st["buf"][k][:nbytes]
    host = stage.numpy()
    qt, desc = host[:o_desc].view(np.uint16).reshape(n, 3, 64), host[o_desc:o_segs].view(np.uint32).reshape(n, 5)
    segs, data = host[o_segs:o_data].view(np.uint32).reshape(nseg, 2), host[o_data:o_data + ndata]
    host[o_data + ndata:o_tab] = 0
    tables = np.empty((n, TB), np.uint8)
    list(_fan_out(n, n, lambda a, b: vr.read_jpeg_bytes_into(uniq[a:b], data, offsets[a:b], desc[a:b], segs, seg_offsets[a:b + 1], tables[a:b],
                                                             qt[a:b])))
    sets, seen = host[o_tab:].reshape(n, TB), {}
    for j in range(n):
        if desc[j, 2]:
            key = tables[j].tobytes()
            if key not in seen:
                seen[key] = len(seen)
                sets[seen[key]] = tables[j]
            desc[j, 4] = seen[key]
    nsets = max(1, len(seen))
    if not seen:
        sets[0] = 0
    used = o_tab + nsets * TB
    on_gpu = torch.device(device).type == "cuda"

    def redo(status):
        """(frame numbers to decode on the host, their coefficients): the index refused them or a segment's status is not 0"""
        bad = [j for j in range(n) if desc[j, 2] == 0 or status[seg_offsets[j]:seg_offsets[j + 1]].any()]
        coef = np.empty((len(bad), cb // 2), np.int16)
        for r, j in enumerate(bad):
            file, off, nb = vr._index[int(uniq[j])]
            rc, msg = kernels.jpeg_coeffs(vr._bytes(file, off, nb), coef[r], qt[j])
            if rc:
                raise ValueError(f"{file}: frame {int(uniq[j])}: {msg}")
        return bad, coef

    if not on_gpu:
        coef, status = kernels.jpeg_entropy_host(data, desc, segs, np.ascontiguousarray(sets[:nsets]), n, vr.H, vr.W)
        bad, again = redo(status)
        coef[bad] = again
        return kernels.I420Frames(torch.from_numpy(kernels.jpeg_idct_i420_host(coef, qt.copy(), vr.H, vr.W)), vr.H, vr.W, vr.format)
    dev = stage[:used].to(device, non_blocking=True)
    stream = torch.cuda.current_stream(dev.device)
    ev = torch.cuda.Event()
    ev.record(stream)
    st["ev"][k] = ev
    coef, status = kernels.jpeg_entropy(dev[o_data:o_data + ndata], dev[o_desc:o_segs].view(torch.int32).view(n, 5),
                                        dev[o_segs:o_data].view(torch.int32).view(nseg, 2), dev[o_tab:used].view(nsets, TB), n, vr.H, vr.W)
    back = _StatusStaging.get(nseg)
    back.copy_(status, non_blocking=True)
    done = torch.cuda.Event()
    done.record(stream)
    done.synchronize()                                   # the wait is here, not inside the library
    bad, again = redo(back.numpy())
    dqt = dev[:o_desc].view(torch.uint16).view(n, 3, 64)
    if bad:                                              # rare: pageable copies, ordered on the stream behind the entropy launch
        coef[torch.tensor(bad, device=dev.device)] = torch.from_numpy(again).to(dev.device)
        dqt = torch.from_numpy(qt.copy().view(np.int16)).to(dev.device).view(torch.uint16)
    return kernels.jpeg_idct_i420(coef, dqt, vr.H, vr.W)


JPEG_WRITE_ENTROPY = "auto"                              # the default of ``MjpegWriter(..., entropy=None)``
# what "auto" chooses for frames on the device: the device coder was above the host coder in every round of MjpegWriter.write at
# q50 / q75 / q90, with and without restart markers (README.md, "Motion-JPEG output"; profiles/mjpeg_write_entropy_probe.txt)
_JPEG_WRITE_AUTO_DEVICE = True


def jpeg_write_entropy_mode(mode):
    """``mode`` if it is one of ``JPEG_ENTROPY_MODES``, else a ValueError that names them"""
    if mode not in JPEG_ENTROPY_MODES:
        raise ValueError(f"entropy={mode!r}: one of {', '.join(JPEG_ENTROPY_MODES)}")
    return mode


class MjpegWriter:
    """Motion-JPEG video written without a codec library, the mirror of ``MjpegFrameReader``: every frame one baseline 4:2:0 JFIF
    image of IJG quality ``quality`` (``kernels.jpeg_quant_tables``), RSTn markers every ``restart_interval`` MCUs when that is not 0.
    ``path`` picks the container the reader knows:
      ``*.mjpeg`` / ``*.mjpg``  the images back to back
      ``*.avi``                 RIFF AVI: ``hdrl`` (MJPG handler and compression, W, H, the rate ``fps``), a ``movi`` list of ``00dc``
                                chunks and ``idx1``; the header and the index are completed by ``close()``.  A file that would pass
                                ``AVI_LIMIT`` (1 GiB; OpenDML, which larger files need, is not written and not read) is a ValueError
                                BEFORE the frame is written: the file stays a valid AVI of the frames so far
      anything else             a directory of ``%06d.jpg`` files, numbered from 0
    ``write(frames)``: a uint8 (3, T, H, W) tensor (R G B) or ``kernels.I420Frames`` of BT.601 full range — JFIF fixes that matrix, so
    any other I420 format is a ValueError (convert with ``to_rgb()``).  On the device: ONE ``jpeg_fdct`` launch, ONE D2H copy of the
    coefficients into pinned staging, then the entropy coder on the threads of the copy pool (the library calls release the GIL).
    Host tensors go through the scalar twin of the launch (bit-equal).  ``write_coefficients(coef, H, W)`` takes coefficients that
    are already on the host.  All frames of a video have the first frame's size.  Use as a context manager or call ``close()``.
    ``entropy`` ("auto" | "host" | "device", None: the module's ``JPEG_WRITE_ENTROPY``) says where the frames of ``write()`` are
    entropy-coded.  "host" is the path above.  "device" (device frames only; host frames are a ValueError): ``jpeg_fdct``, then
    ``kernels.jpeg_encode_scans`` — one lane per block —, the T x 12-byte table of {offset, length, status} comes down, then ONE copy
    of exactly the scans' bytes into pinned staging; an image is the header (built once per writer) + its scan + FF D9.  A table
    that reports a short capacity makes one second call with the capacity it names; a frame with a coefficient outside baseline's
    range has its coefficients brought down and goes through ``kernels.jpeg_encode``, whose refusal is the writer's.  The files of
    the two paths are equal byte for byte.  "auto": "device" for frames on the device (``_JPEG_WRITE_AUTO_DEVICE``), "host" otherwise.  ``write_coefficients`` is always the host coder."""

    AVI_LIMIT = 1 << 30
    _AVI_HEADER = 12 + 12 + 64 + 12 + 64 + 48 + 12      # RIFF, hdrl LIST, avih chunk, strl LIST, strh chunk, strf chunk, movi LIST

    def __init__(self, path, fps, quality=90, restart_interval=0, entropy=None):
        from fractions import Fraction
        self.entropy = jpeg_write_entropy_mode(JPEG_WRITE_ENTROPY if entropy is None else entropy)
        self.path, self.fps, self.quality, self.restart_interval = str(path), float(fps), int(quality), int(restart_interval)
        if not self.fps > 0:
            raise ValueError(f"MjpegWriter: fps must be positive, got {fps}")
        if not 0 <= self.restart_interval <= 65535:
            raise ValueError(f"MjpegWriter: restart_interval must be 0..65535, got {restart_interval}")
        self.qt = kernels.jpeg_quant_tables(self.quality)
        rate = Fraction(self.fps).limit_denominator(100000)
        self._rate, self._scale = rate.numerator, rate.denominator
        low = self.path.lower()
        self.kind = "stream" if low.endswith((".mjpeg", ".mjpg")) else "avi" if low.endswith(".avi") else "dir"
        self.H = self.W = None
        self.frames = 0
        self._qt_dev = {}
        self._index = []                                     # avi: (offset from the 'movi' tag, length) per frame
        if self.kind == "dir":
            os.makedirs(self.path, exist_ok=True)
            self._file = None
        else:
            self._file = open(self.path, "wb")
            if self.kind == "avi":
                self._file.write(b"\0" * self._AVI_HEADER)   # completed by close()
        self._closed = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _set_size(self, H, W):
        if self.H is None:
            self.H, self.W = int(H), int(W)
            self._bound = kernels.jpeg_encode_bound(self.H, self.W)
            self._head = kernels.jpeg_encode_header(self.qt, self.H, self.W, self.restart_interval).tobytes()
        elif (self.H, self.W) != (int(H), int(W)):
            raise ValueError(f"{self.path}: a frame of {W} x {H} in a video of {self.W} x {self.H}")

    def write(self, frames):
        if self._closed:
            raise ValueError(f"{self.path}: write() after close()")
        i420 = isinstance(frames, kernels.I420Frames)
        if i420 and frames.format != kernels._abi.SRC_I420_BT601_FULL:
            raise ValueError(f"{self.path}: I420 frames of format {frames.format} — JFIF fixes BT.601 full range; convert them with to_rgb() first")
        data = frames.data if i420 else frames
        if not (data.dtype == torch.uint8 and len(frames.shape) == 4 and frames.shape[0] == 3):
            raise ValueError(f"{self.path}: expected uint8 (3, T, H, W) frames or I420Frames, got {data.dtype} {tuple(frames.shape)}")
        _, T, H, W = frames.shape
        if self.entropy == "device" and not data.is_cuda:
            raise ValueError(f"{self.path}: entropy='device' codes frames that are on the device; `frames` is on {data.device}")
        self._set_size(H, W)
        if not data.is_cuda:
            src = data.contiguous().numpy()
            return self.write_coefficients(kernels.jpeg_fdct_host(src, self.qt, H, W, frames.format if i420 else kernels._abi.SRC_U8), H, W)
        qt = self._qt_dev.get(data.device)
        if qt is None:
            qt = self._qt_dev[data.device] = torch.from_numpy(self.qt.view(np.int16)).to(data.device).view(torch.uint16)
        coef = kernels.jpeg_fdct(frames if i420 else data.contiguous(), qt)
        if self.entropy == "device" or (self.entropy == "auto" and _JPEG_WRITE_AUTO_DEVICE):
            return self._write_scans(coef, H, W)
        st, k = _Staging.get(coef.numel() * 2)
        stage = st["buf"][k][:coef.numel() * 2].view(torch.int16).view(coef.shape)
        stage.copy_(coef, non_blocking=True)
        torch.cuda.current_stream(data.device).synchronize()
        st["ev"][k] = None
        return self.write_coefficients(stage.numpy(), H, W)

    @staticmethod
    def _down(src, nbytes, stream):
        """the first ``nbytes`` bytes of the device tensor ``src`` -> a uint8 numpy view of pinned staging, after the stream reached it"""
        st, k = _Staging.get(nbytes)
        stage = st["buf"][k][:nbytes]
        stage.copy_(src.reshape(-1).view(torch.uint8)[:nbytes], non_blocking=True)
        stream.synchronize()
        st["ev"][k] = None
        return stage.numpy()

    def _write_scans(self, coef, H, W):
        """device coefficients -> images through the device entropy coder (class docstring)"""
        T = coef.shape[0]
        stream = torch.cuda.current_stream(coef.device)
        cap = None
        for attempt in range(2):
            out, frames = kernels.jpeg_encode_scans(coef, H, W, self.restart_interval, cap)
            table = self._down(frames, T * 12, stream).view(np.uint32).reshape(T, 3).astype(np.int64)
            status, need = table[:, 2], int(table[-1, 0] + table[-1, 1])
            if not (status == kernels.JPEG_SCAN_CAPACITY).any():
                break
            if attempt:
                raise RuntimeError(f"{self.path}: the device entropy coder reports a short capacity with the {cap} bytes it asked for")
            cap = need
        bad = np.nonzero(status == kernels.JPEG_SCAN_RANGE)[0]
        again = {}
        if bad.size:                                             # rare: the host coder's verdict and message are final
            down = coef[torch.from_numpy(bad).to(coef.device)].cpu().numpy()
            buf = np.empty(self._bound, np.uint8)
            for r, j in enumerate(bad):
                again[int(j)] = kernels.jpeg_encode(down[r], self.qt, self.H, self.W, self.restart_interval, out=buf).tobytes()
        scans = self._down(out, need, stream) if need else np.empty(0, np.uint8)
        for j in range(T):
            o, n = int(table[j, 0]), int(table[j, 1])
            self._append(again[j] if j in again else self._head + scans[o:o + n].tobytes() + b"\xff\xd9")

    def _encode(self, coef):
        """frames of coefficients -> list of bytes, on one thread"""
        out = np.empty(self._bound, np.uint8)
        return [kernels.jpeg_encode(c, self.qt, self.H, self.W, self.restart_interval, out=out).tobytes() for c in coef]

    def write_coefficients(self, coef, H, W):
        """coef: int16 numpy (T, jpeg_coef_bytes / 2), quantised with this writer's tables (``self.qt``), on the host"""
        if self._closed:
            raise ValueError(f"{self.path}: write() after close()")
        self._set_size(H, W)
        coef = np.ascontiguousarray(coef, np.int16).reshape(-1, kernels.jpeg_coef_bytes(H, W) // 2)
        n = coef.shape[0]
        for images in _fan_out(n, n, lambda a, b: self._encode(coef[a:b])):
            for image in images:
                self._append(image)

    def _append(self, image):
        if self.kind == "dir":
            with open(os.path.join(self.path, "%06d.jpg" % self.frames), "wb") as f:
                f.write(image)
        elif self.kind == "stream":
            self._file.write(image)
        else:
            pos, n = self._file.tell(), len(image)
            total = pos + 8 + n + (n & 1) + 8 + 16 * (self.frames + 1)       # this chunk, then idx1
            if total > self.AVI_LIMIT:
                raise ValueError(f"{self.path}: frame {self.frames} would take the AVI file to {total} bytes, past {self.AVI_LIMIT} "
                                 "(OpenDML is not written); start another file")
            self._index.append((pos - (self._AVI_HEADER - 4), n))
            self._file.write(b"00dc" + n.to_bytes(4, "little") + image + (b"\0" if n & 1 else b""))
        self.frames += 1

    def close(self):
        if self._closed:
            return
        self._closed = True
        if self._file is None:
            return
        if self.kind == "avi":
            import struct
            f, n, W, H = self._file, self.frames, self.W or 0, self.H or 0
            end = f.tell()
            f.write(b"idx1" + struct.pack("<I", 16 * n) + b"".join(b"00dc" + struct.pack("<III", 0x10, o, s) for o, s in self._index))
            size = f.tell()
            biggest = max((s for _, s in self._index), default=0)
            avih = struct.pack("<14I", int(round(1e6 * self._scale / self._rate)), 0, 0, 0x10, n, 0, 1, biggest, W, H, 0, 0, 0, 0)
            strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, self._scale, self._rate, 0, n, biggest, 0xFFFFFFFF, 0, 0, 0, W, H)
            strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
            head = (b"RIFF" + struct.pack("<I", size - 8) + b"AVI " + b"LIST" + struct.pack("<I", 4 + 64 + 12 + 64 + 48) + b"hdrl"
                    + b"avih" + struct.pack("<I", 56) + avih + b"LIST" + struct.pack("<I", 4 + 64 + 48) + b"strl"
                    + b"strh" + struct.pack("<I", 56) + strh + b"strf" + struct.pack("<I", 40) + strf
                    + b"LIST" + struct.pack("<I", end - self._AVI_HEADER + 4) + b"movi")
            assert len(head) == self._AVI_HEADER, len(head)
            f.seek(0)
            f.write(head)
        self._file.close()


def _sampled_clips(path, samplers, is_train, device, yuv_matrix="bt601", jpeg_entropy=None, vr=None):
    """Reference ``spatial_temporal_view_decomposition`` (:376-397), decode half: one reader, every frame fetched once and
    sent to the device once, as uint8; per view a uint8 (3, T, H, W) device tensor (frame gather + layout change in HBM) +
    the sampled indices.  I420 frames (a ``.y4m`` file): per view a ``kernels.I420Frames`` — a gather of whole frames, no
    layout change and no conversion here.  ``vr``: the video already opened (a caller that reads it for more than the views)."""
    vr = open_video(path, yuv_matrix) if vr is None else vr
    frame_inds = {k: s(len(vr), is_train) for k, s in samplers.items()}
    uniq = np.unique(np.concatenate(list(frame_inds.values()), 0))
    frames = _frames_to_device(vr, uniq, device, jpeg_entropy)                 # (n, H, W, 3) uint8
    video = {}
    for k, inds in frame_inds.items():
        pos = torch.from_numpy(np.searchsorted(uniq, inds).astype(np.int64)).to(frames.device)
        video[k] = frames.select(pos) if isinstance(frames, kernels.I420Frames) else frames.index_select(0, pos).permute(3, 0, 1, 2).contiguous()
    return video, frame_inds


def _build_samplers(sample_types, phase):
    samplers = {}
    for stype, sopt in sample_types.items():
        if "t_frag" not in sopt:      # (clip_len, num_clips, frame_interval) positionally, as the reference (:962-964)
            samplers[stype] = UnifiedFrameSampler(sopt["clip_len"], sopt["num_clips"], sopt["frame_interval"])
        else:
            samplers[stype] = UnifiedFrameSampler(sopt["clip_len"] // sopt["t_frag"], sopt["t_frag"], sopt["frame_interval"],
                                                  sopt["num_clips"])
        print(stype + " branch sampled frames:", samplers[stype](40, phase == "train"))       # draws from the RNG, as there
    return samplers


def _default_device(device):
    """``None`` -> the process's CURRENT HIP device (rank r of a torch.distributed.run job has set cuda:r): the K1
    kernels are launched on the current device's stream, so the frames must live there."""
    if device is not None:
        return torch.device(device)
    return torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)


class ViewDecompositionDataset_add_forSimpleVQA(torch.utils.data.Dataset):  # noqa: N801  (reference spelling)
    """Reference class of the same name (fusion_datasets.py:786-927): csv ``filename,label`` with a header row, per
    video the ``simpleVQA`` view (resize 520 -> centre crop 448, normalised with the ImageNet constants on 0-255
    pixels — reproduced as-is) and ``feat`` = 8 rows of SlowFast features from
    ``data_prefix_3D/<video_name>/feature_{i}_{slow,fast}_feature.npy``.  Same dict keys.

    Not in the reference — ``motion_features: {source: files | inline, weights: <state_dict.pth> | null, resize: 224, fps: null,
    small_grid_mean: false}``: absent or ``source: files`` is the behaviour above.  ``inline``: ``data_prefix_3D`` may be absent and
    ``feat`` is computed from the video itself, which is opened once per item for the view and for the features: the clips of
    ``slowfast_clips.device_clips`` (frames resized on the device as Pillow resizes them) through one SlowFast-R50 that the dataset
    builds lazily on its device, the first 8 clips' features as an fp32 DEVICE tensor [8, 2304 | 2048 | 256].  ``weights`` loads as
    ``SlowFast_features.py --weights`` does; null = that tool's seeded random weights, with a warning on stderr."""

    MOTION_SOURCES = ("files", "inline")
    MOTION_KEYS = ("source", "weights", "resize", "fps", "small_grid_mean")

    def __init__(self, opt, namelist=None, device=None):
        import csv
        import os.path as osp
        super().__init__()
        self.opt, self.namelist, self.device = opt, namelist, _default_device(device)
        if opt.get("jpeg_entropy") is not None:          # yml data.<split>.args.jpeg_entropy: refused here, not at the first item
            jpeg_entropy_mode(opt["jpeg_entropy"])
        mf = opt.get("motion_features") or {}
        if not isinstance(mf, dict) or set(mf) - set(self.MOTION_KEYS):
            raise ValueError(f"motion_features: expected a mapping with the keys {', '.join(self.MOTION_KEYS)}, got {mf!r}")
        self.motion = dict(source=mf.get("source", "files"), weights=mf.get("weights"), resize=int(mf.get("resize", 224)), fps=mf.get("fps"),
                           small_grid_mean=bool(mf.get("small_grid_mean", False)))
        if self.motion["source"] not in self.MOTION_SOURCES:
            raise ValueError(f"motion_features.source must be one of {', '.join(self.MOTION_SOURCES)}, got {self.motion['source']!r}")
        self._motion_model = None
        self.ann_file, self.data_prefix = opt["anno_file"], opt["data_prefix"]
        self.data_prefix_3D = opt.get("data_prefix_3D") if self.motion["source"] == "inline" else opt["data_prefix_3D"]
        self.sample_types, self.feature_type, self.phase = opt["sample_types"], opt["feature_type"], opt["phase"]
        self.augment = opt.get("augment", False)
        if self.augment:
            raise NotImplementedError("augment: the training augmentations (RandomResizedCrop, flips) are not built; phase 'train' "
                                      "without them samples as the reference does")
        self.draw = 0
        self.samplers = _build_samplers(self.sample_types, self.phase)
        if isinstance(self.ann_file, list):
            self.video_infos = self.ann_file
        else:
            self.video_infos = []
            with open(self.ann_file, newline="") as f:
                rows = csv.reader(f)
                next(rows)
                for row in rows:
                    self.video_infos.append(dict(filename=osp.join(self.data_prefix, row[0]), label=float(row[1]), video_name=row[0]))
            scores = [v["label"] for v in self.video_infos]
            self.max, self.min = max(scores), min(scores)
        self.labels = [v["label"] for v in self.video_infos]
        self.video_names = [v["video_name"] for v in self.video_infos]

    def __len__(self):
        return len(self.video_infos)

    def set_draw(self, k: int):
        """train-phase draw ``k`` of every item (see ``SyntheticKVQDataset.set_draw``)"""
        self.draw = int(k)

    def _features(self, video_name):
        import os
        folder = os.path.join(self.data_prefix_3D, video_name)
        parts = {"Slow": ("slow",), "Fast": ("fast",), "SlowFast": ("slow", "fast")}[self.feature_type]
        rows = []
        for i in range(8):
            rows.append(torch.cat([torch.from_numpy(np.load(os.path.join(folder, f"feature_{i}_{p}_feature.npy"))).squeeze().float().reshape(-1)
                                   for p in parts]))
        return torch.stack(rows)

    def motion_model(self):
        """the SlowFast-R50 of ``motion_features.source: inline`` on the dataset's device, built at its first use"""
        if self._motion_model is None:
            import sys
            from ..models.backbones.slowfast_model import slowfast
            model = slowfast().to(self.device).eval()
            if self.motion["small_grid_mean"]:
                model.head_small_grid = "mean"
            if self.motion["weights"]:
                model.load_state_dict(torch.load(self.motion["weights"], map_location="cpu"), strict=False)
            else:
                print("motion_features.weights is null: the SlowFast features come from seeded random weights", file=sys.stderr)
            self._motion_model = model
        return self._motion_model

    def _features_inline(self, vr, path):
        """[8, 2304 | 2048 | 256] fp32 on the device: the first 8 clips of the opened video through ``device_clips`` and the network"""
        from .slowfast_clips import VIDEO_CLIP_MIN, device_clips, extract_features
        clips = device_clips(vr, path, self.motion["resize"], self.device, self.motion["fps"], self.opt.get("jpeg_entropy"))
        slow, fast = extract_features(self.motion_model(), clips[:VIDEO_CLIP_MIN], self.device)
        parts = {"Slow": (slow,), "Fast": (fast,), "SlowFast": (slow, fast)}[self.feature_type]
        return torch.cat([p.reshape(p.shape[0], -1).float() for p in parts], 1)

    def __getitem__(self, index):
        info = self.video_infos[index]
        if self.opt.get("seed_per_item"):
            _seed_item(index, self.draw)
        vr = None
        if self.motion["source"] == "inline":
            vr = open_video(info["filename"], self.opt.get("yuv_matrix", "bt601"))
            feat = self._features_inline(vr, info["filename"])
        else:
            feat = self._features(info["video_name"])
        video, frame_inds = _sampled_clips(info["filename"], self.samplers, self.phase == "train", self.device,
                                            self.opt.get("yuv_matrix", "bt601"), self.opt.get("jpeg_entropy"), vr)
        data = {}
        for stype, sopt in self.sample_types.items():
            kw = dict(sopt, phase=self.phase)
            data[stype] = get_single_view(video[stype], stype, mean=SIMPLEVQA_MEAN, std=SIMPLEVQA_STD, **kw)
        data["num_clips"] = {k: s["num_clips"] for k, s in self.sample_types.items()}
        data["clip_len"] = {k: s["clip_len"] for k, s in self.sample_types.items()}
        data["frame_inds"], data["label"], data["video_name"] = frame_inds, info["label"], info["video_name"]
        if "simpleVQA" in data:
            data["feat"] = feat
        data["name"] = info["filename"]
        return data


class ViewDecompositionDataset_KVQ(torch.utils.data.Dataset):  # noqa: N801  (reference spelling)
    """Reference class of the same name (fusion_datasets.py:930-1051): lines ``filename,cls_label,dis_label,label``;
    per video the view(s) of ``sample_types`` normalised with the KVQ constants, plus the KSVQE inputs:
    ``resize_video`` (``get_resized_video``, /255 then the CLIP constants), ``fragment`` (= the normalised view),
    ``ori_fragment`` (a second, un-normalised fragment draw, as the reference makes), ``dis_label``,
    ``original_shape``.  Same dict keys."""

    CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
    CLIP_STD = (0.26862954, 0.26130258, 0.27577711)

    def __init__(self, opt, namelist=None, device=None):
        import os.path as osp
        super().__init__()
        self.opt, self.namelist, self.device = opt, namelist, _default_device(device)
        if opt.get("jpeg_entropy") is not None:          # yml data.<split>.args.jpeg_entropy: refused here, not at the first item
            jpeg_entropy_mode(opt["jpeg_entropy"])
        self.ann_file, self.data_prefix = opt["anno_file"], opt["data_prefix"]
        self.sample_types, self.phase = opt["sample_types"], opt["phase"]
        self.augment = opt.get("augment", False)
        if self.phase == "train" or self.augment:
            # the reference's train phase draws this class's views (fragments, resized frames, frame indices) exactly as its test phase
            # does — get_spatial_fragments and UnifiedFrameSampler ignore the flag — so 'train' without augment would add nothing:
            # phase 'test' with set_draw(k) gives the train-phase draws
            raise NotImplementedError("training-phase sampling / augmentation: this is an inference engine (phase 'test' with "
                                      "set_draw(k) draws what the reference's train phase draws; its augmentations are not built)")
        self.draw = 0
        self.samplers = _build_samplers(self.sample_types, self.phase)
        if isinstance(self.ann_file, list):
            self.video_infos = self.ann_file
        else:
            self.video_infos = []
            with open(self.ann_file, "r") as f:
                for line in f:
                    filename, cls_label, dis_label, label = line.strip().split(",")
                    self.video_infos.append(dict(filename=osp.join(self.data_prefix, filename), label=float(label),
                                                 cls_label=int(float(cls_label)), dis_label=int(float(dis_label)),
                                                 video_name=filename))
            scores = [v["label"] for v in self.video_infos]
            self.max, self.min = max(scores), min(scores)
        self.labels = [v["label"] for v in self.video_infos]
        self.video_names = [v["video_name"] for v in self.video_infos]

    def __len__(self):
        return len(self.video_infos)

    def set_draw(self, k: int):
        """train-phase draw ``k`` of every item (see ``SyntheticKVQDataset.set_draw``)"""
        self.draw = int(k)

    def __getitem__(self, index):
        info = self.video_infos[index]
        if self.opt.get("seed_per_item"):
            # as SyntheticKVQDataset: the samplers draw from the process-global RNGs; seeded per item, item i is the same whatever
            # was built before it (two runs over two trees of the same videos then draw the same frames and offsets)
            _seed_item(index, self.draw)
        video, frame_inds = _sampled_clips(info["filename"], self.samplers, False, self.device, self.opt.get("yuv_matrix", "bt601"),
                                            self.opt.get("jpeg_entropy"))
        data, k = {}, None
        resize = ori = None
        for stype, sopt in self.sample_types.items():       # order of the reference's three calls per view (:455-459)
            kw = dict(sopt, phase="test")
            data[stype] = get_single_view(video[stype], stype, mean=KVQ_MEAN, std=KVQ_STD, **kw)
            resize = get_resized_video(video[stype], mean=tuple(255.0 * m for m in self.CLIP_MEAN),
                                       std=tuple(255.0 * s for s in self.CLIP_STD),
                                       **{a: b for a, b in kw.items() if a in ("size_h", "size_w", "random_crop", "arp", "antialias")})
            ori = get_spatial_fragments(video[stype], **{a: b for a, b in kw.items() if a in (
                "fragments_h", "fragments_w", "fsize_h", "fsize_w", "aligned", "nfrags")})
            k = stype
        data["resize_video"], data["fragment"], data["ori_fragment"] = resize, data[k], ori
        data["num_clips"] = {s: o["num_clips"] for s, o in self.sample_types.items()}
        data["clip_len"] = {s: o["clip_len"] for s, o in self.sample_types.items()}
        data["frame_inds"], data["dis_label"] = frame_inds, info["dis_label"]
        data["name"], data["video_name"] = info["filename"], info["video_name"]
        data["original_shape"] = tuple(video[k].shape[1:])
        data["label"] = info["label"]
        return data
