"""Inference harness mirroring the reference's ``trainer.py`` (``Trainer`` :39-361, inference half) and
the score all-gather of ``trainer_ddp.py:259-267``.

Differences that are deliberate:
  * ``inferece()`` exists (``test.py:37`` calls it; the reference's ``trainer.py`` lacks it): it runs
    ``inferece_test()`` and, when labels are present, also prints the ``inferece_val()`` metrics;
  * one process per GPU (``torch.distributed.run``) instead of ``nn.DataParallel``: videos are sharded
    ``videos[rank::world]`` and ONE all-gather of the score vector runs at the end;
  * scores stay on the device until the end (no per-video ``.item()`` sync, ``trainer.py:329``).
Training: ``finetune_head()`` fits the head (a ``VQAHead``, or the ``simpleVQAHead`` of model key ``simpleVQA``) on features of the
frozen trunk (kvq_amd/finetune.py: the reference's losses, AdamW, schedule, EMA and best-checkpoint rule); gradients into a backbone
are out of scope.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

from . import datasets as _datasets
from . import dist as kd
from . import kernels
from .models.model import VQA_Network


class _MapWriter:
    """Per lane, ``depth`` sets of pinned host buffers, each behind an event: a video's results go device -> host on the lane's
    stream with no synchronisation; the host waits only on the event of the set it is about to reuse, and writes that set's file then
    (so files appear as the run proceeds).  ``flush`` writes what is still in flight."""

    def __init__(self, trainer, qm, n_lanes, depth=2):
        self.trainer, self.qm = trainer, qm
        self.sets = [[{"event": torch.cuda.Event(), "bufs": {}, "pending": None} for _ in range(depth)] for _ in range(n_lanes)]
        self.turn = [0] * n_lanes
        self.written = 0

    def _drain(self, st):
        if st["pending"] is None:
            return
        st["event"].synchronize()
        name, frame_item, keys = st["pending"]
        host = {k: st["bufs"][k] for k in keys}
        host["score"] = float(host.pop("score_"))
        self.trainer._maps_write(self.qm, name, host, frame_item)
        self.written += 1
        st["pending"] = None

    def put(self, lane, stream, name, out, score, item):
        """enqueue the copies of ``out`` (dict of device tensors) and ``score`` (0-d device tensor) on ``stream``"""
        st = self.sets[lane][self.turn[lane]]
        self.turn[lane] = (self.turn[lane] + 1) % len(self.sets[lane])
        self._drain(st)
        todo = {k: v for k, v in out.items() if k != "pred"}
        todo["score_"] = score
        for k, v in todo.items():
            b = st["bufs"].get(k)
            if b is None or b.shape != v.shape or b.dtype != v.dtype:
                b = st["bufs"][k] = torch.empty(v.shape, dtype=v.dtype, pin_memory=True)
            b.copy_(v, non_blocking=True)
        st["event"].record(stream)
        ksvqe = self.trainer.config["model"]["type"] == "KSVQE"
        st["pending"] = (name, {"frame_inds": item.get("frame_inds"), "overlay_size": self.trainer._overlay_size(item, ksvqe)}
                         if isinstance(item, dict) else None, list(todo))

    def flush(self):
        for lane in self.sets:
            for st in lane:
                self._drain(st)


class Trainer:
    def __init__(self, args, config):
        self.args, self.config = args, config
        self.rank, self.local_rank, self.world = kd.init()
        gpu_ids = [int(i) for i in str(getattr(args, "gpu_id", "0")).split(",") if i != ""]
        dev = gpu_ids[0] if self.world == 1 and gpu_ids else self.local_rank
        self.device = torch.device(f"cuda:{dev}")
        torch.cuda.set_device(self.device)
        self.key_list = self.config["model"]["type"].split(",")
        self.build_datasets()
        self.build_models()

    def build_models(self):
        self.model = VQA_Network(self.config).to(self.device).eval()
        self._lane_graphs = None                 # recorded forwards bake the weight images in: never outlive a weight change
        path = self.config.get("load_path")
        if path:
            print("load:", self.load_weights(path))

    def load_weights(self, path):
        """load a checkpoint into the built model; drops the recorded hipGraphs (they replay the OLD weight images)."""
        self._lane_graphs = None
        return self.load_checkpoint(self.model, path)

    @staticmethod
    def load_checkpoint(model, path):
        """DataParallel / DDP checkpoints carry a 'module.' prefix (trainer.py:62-74, trainer_ddp.py:74-79);
        either the bare state dict or ``{"state_dict": ...}``; non-strict like the reference."""
        state = torch.load(path, map_location="cpu")
        state = state.get("state_dict", state)
        state = {(k[7:] if k.startswith("module.") else k): v for k, v in state.items()}
        return model.load_state_dict(state, strict=False)

    def build_datasets(self):
        cfg = self.config["data"]["val"]
        cls = getattr(_datasets, cfg["type"])
        # every dataset class stages and samples on THIS rank's device (rank r / --gpu_id N, not cuda:0): the K1 kernels run
        # on the current device's stream and must see pointers of the same device
        self.val_dataset = cls(cfg["args"], None, device=self.device)

    # ------------------------------------------------------------------------------------------
    def _model_inputs(self, data):
        """clip reshape of the dataset item (trainer.py:306-319) -> dict of DEVICE tensors, the model's inputs."""
        inputs = {}
        ksvqe = self.config["model"]["type"] == "KSVQE"
        # KSVQE reads resize_video / fragment / dis_label only (key_list = ['KSVQE'], trainer.py:56,259-260): the 'technical'
        # view (the same pixels as 'fragment', ~95 MB fp32 per 96-frame sample) is neither reshaped nor copied
        # the ConvNeXt-3D trunks (model keys conv_tiny, conv_v2_tiny) read the 'aesthetic' view
        views = ("technical", "aesthetic") if ("conv_tiny" in self.key_list or "conv_v2_tiny" in self.key_list) else ("technical",)
        for key in ([] if ksvqe else list(data)):
            if key in self.key_list or key in views:
                x = data[key]
                if isinstance(x, kernels.FragmentSource):
                    # a lazily sampled view (``lazy: true`` in its sample_types entry): the clips stay views of the uint8 frames
                    # and the trunk's embedding launch samples while it reads — no fp32 sample, no reshape copy
                    nc = int(data.get("num_clips", {}).get(key, 1)) if isinstance(data.get("num_clips"), dict) else 1
                    inputs[key] = x.split_clips(nc)
                    continue
                if not torch.is_tensor(x) or x.dim() not in (4, 5):
                    continue
                x = x.to(self.device)
                if x.dim() == 4:
                    x = x.unsqueeze(0)
                b, c, t, h, w = x.shape
                nc = int(data.get("num_clips", {}).get(key, 1)) if isinstance(data.get("num_clips"), dict) else 1
                inputs[key] = (x.reshape(b, c, nc, t // nc, h, w).permute(0, 2, 1, 3, 4, 5)
                               .reshape(b * nc, c, t // nc, h, w).contiguous())
        if ksvqe:
            # the DataLoader of the reference adds the batch dimension (batch_size 1) and the whole T-frame sample goes to
            # KSVQE as ONE clip (trainer.py:306-326): resize_video / fragment (1, 3, T, h, w), dis_label (1,)
            for k in ("resize_video", "fragment"):
                v = data[k].materialise() if isinstance(data[k], kernels.FragmentSource) else data[k].to(self.device)
                inputs[k] = v.unsqueeze(0) if v.dim() == 4 else v
            inputs["dis_label"] = torch.as_tensor(data["dis_label"]).reshape(-1).to(self.device)
            if isinstance(data["fragment"], kernels.FragmentSource) and self._quality_maps() is not None:
                # the model gets the sampled tensor as before; the quality paint reads the draws (and, for overlays, the uint8 frames)
                # the sample was made from, so the source travels with the inputs — under graph replay through a FragmentSlot.
                # KSVQE.forward reads its three keys only
                inputs["fragment_source"] = data["fragment"]
        elif "feat" in data and torch.is_tensor(data["feat"]):
            inputs["feat"] = data["feat"].to(self.device)
        return inputs

    def _run_model(self, inputs):
        """model forward (trainer.py:320-327) -> device tensor of clip scores; with the yml key ``quality_maps`` a dict of device
        tensors instead: ``pred`` and, per model key, its quality maps (``_run_model_maps``)."""
        qm = self._quality_maps()
        with torch.no_grad():
            if qm is not None:
                return self._run_model_maps(inputs, qm)
            if self.config["model"]["type"] == "KSVQE":
                pred, _ = self.model(inputs=inputs, reduce_scores=True)       # (scores, distortion contrastive loss)
                return pred
            return self.model(inputs=inputs, reduce_scores=True)

    # ---- quality maps (yml `quality_maps: {dir, cell, overlay_frames}`) -----------------------------------------------------
    def _quality_maps(self):
        """the parsed yml key, or None (absent / empty: nothing changes)"""
        qm = self.config.get("quality_maps")
        if not qm:
            return None
        if not isinstance(qm, dict) or not qm.get("dir"):
            raise ValueError("quality_maps: expected {dir: <path>, cell: 8, overlay_frames: 0}")
        unknown = set(qm) - {"dir", "cell", "overlay_frames", "overlay_video", "overlay_quality"}
        if unknown:
            raise ValueError(f"quality_maps: unknown key(s) {sorted(unknown)}")
        cell, nov = int(qm.get("cell", 8)), int(qm.get("overlay_frames", 0))
        if cell not in kernels.PAINT_CELLS:
            raise ValueError(f"quality_maps.cell must be one of {kernels.PAINT_CELLS}, got {cell}")
        if not 0 <= nov <= 16:
            raise ValueError(f"quality_maps.overlay_frames must be 0..16, got {nov}")
        return {"dir": str(qm["dir"]), "cell": cell, "overlay_frames": nov}

    OVERLAY_VIDEO = ("avi", "mjpeg", "jpg")
    OVERLAY_FPS = 2

    def _overlay_video(self):
        """yml ``quality_maps: {..., overlay_video: avi | mjpeg | jpg, overlay_quality: 90}``, parsed beside ``_quality_maps``: None, or
        {"ext", "quality"} — the overlays then leave as Motion-JPEG, ``<dir>/<video_name>.overlay.<ext>`` (an AVI file, a raw stream, a
        directory of .jpg frames), 2 frames per second, all clips in order and their slices in depth order, and the .npz carries
        ``overlay_frame_inds`` (n_clips, n_ov), the source frame numbers, instead of ``overlay``"""
        qm = self.config.get("quality_maps")
        if not isinstance(qm, dict) or not qm.get("overlay_video"):
            return None
        ext, quality = str(qm["overlay_video"]).lower(), int(qm.get("overlay_quality", 90))
        if ext not in self.OVERLAY_VIDEO:
            raise ValueError(f"quality_maps.overlay_video must be one of {self.OVERLAY_VIDEO}, got {qm['overlay_video']!r}")
        if not 1 <= quality <= 100:
            raise ValueError(f"quality_maps.overlay_quality must be 1..100, got {quality}")
        if int(qm.get("overlay_frames", 0)) == 0:
            raise ValueError("quality_maps.overlay_video needs overlay_frames >= 1")
        return {"ext": ext, "quality": quality}

    def _overlay_tables(self, quality):
        """the quantiser tables of the overlay video on the device, made once (outside any recording: ``_score_all`` asks first)"""
        cache = self.__dict__.setdefault("_overlay_qt", {})
        if quality not in cache:
            cache[quality] = torch.from_numpy(kernels.jpeg_quant_tables(quality).view(np.int16)).to(self.device).view(torch.uint16)
        return cache[quality]

    def _overlay_coefficients(self, overlay, ov):
        """painted overlays uint8 (n_clips, n_ov, 3, Hs, Ws) -> their quantised JPEG coefficients int16 (n_clips, n_ov, coef / 2): one
        forward-DCT launch per frame (each (3, Hs, Ws) slice is a one-frame R G B source), part of a recorded forward.  The same bytes
        per pixel as the overlay itself: this is what travels to the host in its place."""
        n_clips, n_ov, _, Hs, Ws = overlay.shape
        qt = self._overlay_tables(ov["quality"])
        coef = torch.empty(n_clips, n_ov, kernels.jpeg_coef_bytes(Hs, Ws) // 2, dtype=torch.int16, device=overlay.device)
        for b in range(n_clips):
            for n in range(n_ov):
                kernels.jpeg_fdct(overlay[b, n].unsqueeze(1), qt, out=coef[b, n].unsqueeze(0))
        return coef

    @staticmethod
    def _overlay_size(item, ksvqe):
        """(Hs, Ws) of the frames a video's overlays were painted on, from its dataset item"""
        if isinstance(item, dict) and item.get("overlay_size") is not None:
            return item["overlay_size"]
        view = item.get("fragment" if ksvqe else "technical") if isinstance(item, dict) else None
        vids = getattr(view, "videos", None)
        return tuple(int(v) for v in vids[0].shape[-2:]) if vids else None

    @staticmethod
    def overlay_depths(D, n):
        """``n`` evenly spaced depth slices of ``D`` (the centres of n equal parts)"""
        n = min(int(n), int(D))
        return [(2 * k + 1) * D // (2 * n) for k in range(n)]

    def _run_model_maps(self, inputs, qm):
        """the forward with the heads' maps kept, and the paint onto the source frames where the trunk read them through the sampler.
        Returns a flat dict of device tensors — what a recorded forward keeps as its static outputs.  The paint reads the batch
        through the same object the trunk did: under graph replay that is the lane's ``FragmentSlot``, so the paint launch is part
        of the recording and reads each video's frames and draws through the slot's pointer table."""
        out, maps = self.model(inputs=inputs, reduce_scores=True, return_maps=True)
        res = {"pred": out[0] if isinstance(out, tuple) else out}
        ksvqe = self.config["model"]["type"] == "KSVQE"
        src = inputs.get("fragment_source") if ksvqe else inputs.get("technical")
        for key, m in maps.items():
            tok = m["token_map"]
            res[f"{key}/token_map"], res[f"{key}/timeline"] = tok, m["timeline"]
            if not (isinstance(src, kernels.FragmentSource) and not src.upsampled and src.shape[0] == tok.shape[0]):
                continue
            depths = self.overlay_depths(tok.shape[1], qm["overlay_frames"])
            if ksvqe:
                # the trunk saw one QRS window of the canvas per frame: paint through it, slice d with the window of frame 2d (phase 0,
                # the frame the overlay shows)
                net, regions = getattr(self.model, key + "_backbone").spa_patchnet, m.get("regions")
                kk = int(round(net.k ** 0.5))
                if regions is None or not kernels.quality_paint_regions_supported(src, tok.shape[1:], net.anchor_size, kk, kk, qm["cell"]):
                    continue
                painted = kernels.quality_paint_regions(src, tok, regions, net.anchor_size, kk, kk, phase=0, cell=qm["cell"],
                                                        overlay_depths=depths)
                res[f"{key}/regions"] = regions
                # row length of the window index, for the writer's (ry, rx) decode on the host: a constant of the sampler geometry
                self.__dict__.setdefault("_region_row", {})[key] = src.geometry[1] * src.geometry[3] // net.anchor_size - kk + 1
            elif kernels.quality_paint_supported(src, tok.shape[1:], qm["cell"]):
                painted = kernels.quality_paint(src, tok, cell=qm["cell"], overlay_depths=depths)
            else:
                continue
            ov = self._overlay_video()
            for name, t in zip(("heat", "cover", "overlay"), painted):
                if name == "overlay" and ov is not None:
                    res[f"{key}/overlay_coef"] = self._overlay_coefficients(t, ov)
                else:
                    res[f"{key}/{name}"] = t
        return res

    @staticmethod
    def _pred(out):
        return out["pred"] if isinstance(out, dict) else out

    def _maps_note(self, out, item):
        """one stderr line per reason (not per video) when a sample gets no heat / cover"""
        if any(k.endswith("/heat") for k in out):
            return
        ksvqe = self.config["model"]["type"] == "KSVQE"
        view = "fragment" if ksvqe else "technical"
        if ksvqe and not (isinstance(item, dict) and "fragment" in item):
            return
        x = item.get(view) if isinstance(item, dict) else None
        if not isinstance(x, kernels.FragmentSource):
            why = f"the {view} view is not sampled lazily (lazy: false)"
        elif x.upsampled:
            why = "the source is smaller than the fragment canvas (upsample fallback)"
        else:
            why = "the paint does not cover this sampler geometry"
        seen = self.__dict__.setdefault("_maps_notes", set())
        if why not in seen:
            seen.add(why)
            print(f"quality maps: token_map, timeline and frame_inds only — {why}", file=sys.stderr)

    @staticmethod
    def _maps_frame_inds(item, n_clips, D):
        """(n_clips, D, 2): the source frame numbers of each token's frame pair, or None when the item's list does not fit"""
        fi = item.get("frame_inds") if isinstance(item, dict) else None
        if isinstance(fi, dict):
            fi = fi.get("technical", fi.get("fragment", next(iter(fi.values()), None)))
        if fi is None:
            return None
        fi = np.asarray(fi).reshape(-1)
        return fi.reshape(n_clips, D, 2).astype(np.int64) if fi.size == n_clips * D * 2 else None

    def _maps_write(self, qm, name, host, frame_item):
        """<dir>/<video_name>.npz from the host copies of one video's results"""
        arrays = {k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in host.items() if "/" in k}
        keys = sorted({k.split("/")[0] for k in arrays})
        for key in keys:
            nrx = self.__dict__.get("_region_row", {}).get(key) if f"{key}/regions" in arrays else None
            if nrx:                              # window index -> (ry, rx) in anchors, (n_clips, T, 2)
                arrays[f"{key}/regions"] = np.stack(np.divmod(arrays[f"{key}/regions"].astype(np.int32), np.int32(nrx)), -1).astype(np.int32)
        score = np.float32(host["score"]) if "score" in host else host["pred"].float().mean().numpy()
        os.makedirs(qm["dir"], exist_ok=True)
        for key in keys:
            n_clips, D = arrays[f"{key}/token_map"].shape[:2]
            fi = self._maps_frame_inds(frame_item, n_clips, D)
            if fi is not None:
                arrays[f"{key}/frame_inds"] = fi
            arrays[f"{key}/score"] = np.asarray(score, np.float32)
            coef = arrays.pop(f"{key}/overlay_coef", None)
            if coef is not None:
                # the overlay video: slice n of a clip shows clip frame 2 depth[n], the first frame of that depth's pair
                ov, depths = self._overlay_video(), self.overlay_depths(D, coef.shape[1])
                size = self._overlay_size(frame_item, self.config["model"]["type"] == "KSVQE")
                stem = os.path.basename(str(name)) + ("" if len(keys) == 1 else "." + key)
                from .datasets.fusion_datasets import MjpegWriter
                with MjpegWriter(os.path.join(qm["dir"], f"{stem}.overlay.{ov['ext']}"), self.OVERLAY_FPS, quality=ov["quality"]) as w:
                    w.write_coefficients(coef.reshape(n_clips * coef.shape[1], -1), *size)
                arrays[f"{key}/overlay_frame_inds"] = (fi[:, depths, 0] if fi is not None
                                                       else np.broadcast_to(2 * np.asarray(depths, np.int64), coef.shape[:2]).copy())
        if len(keys) == 1:                       # one model key: no prefix
            arrays = {k.split("/", 1)[1]: v for k, v in arrays.items()}
        path = os.path.join(qm["dir"], os.path.basename(str(name)) + ".npz")
        tmp = path + ".tmp.npz"
        np.savez(tmp, **arrays)
        os.replace(tmp, path)
        return path

    def _forward_video(self, data):
        return self._pred(self._run_model(self._model_inputs(data)))

    def _score_all(self):
        bb = getattr(self.model, "KSVQE_backbone", None)
        if bb is not None:
            bb.aux_loss = False                    # `pred, _ = model(...)`: the contrastive loss is never read at inference
        n = len(self.val_dataset)
        mine = kd.shard_indices(n, self.rank, self.world)
        local = torch.empty(len(mine), dtype=torch.float32, device=self.device)
        # videos are independent (batch_size 1, trainer.py:256-283): consecutive videos go to alternating HIP streams so
        # that one video's latency-bound launches fill the gaps of another's; nothing synchronises with the host per video
        main = torch.cuda.current_stream(self.device)
        # hipGraph replay of the per-video forward (kvq_amd/graph.py): default for KSVQE (~360 launches per video) and
        # SimpleVQA (~70 launches for 8 frames), which are enqueue-bound (tools/harness_probe*.py: 101 vs 62 and 283 vs 213
        # videos/s end to end); the Swin trunk alone is not (+1 %).  KVQ_GRAPH=1 / 0 forces it on / off for any model
        want = str(self.config.get("hipgraph", "auto")).lower()
        # ... and, since a recorded forward can read a LAZY sample through a pointer table (kernels.FragmentSlot: no fp32 copy of the
        # batch into a static buffer), the Swin trunk on lazy samples: +2 % on 4 lanes of 4-clip batches (bench.py, same-box A/B) and
        # a fifth of the host time per video
        try:
            st_cfg = self.config["data"]["val"]["args"].get("sample_types", {})
            lazy = any(isinstance(v, dict) and bool(v.get("lazy", False)) for v in st_cfg.values())
        except (KeyError, AttributeError, TypeError):
            lazy = False
        use_graph = want in ("1", "true", "on") or (want == "auto" and (self.config["model"]["type"] in ("KSVQE", "simpleVQA") or lazy))
        # lanes: 3 eager streams; 4 graph lanes = one per hardware queue (measured, tools/harness_probe.py: 2 / 3 / 4 / 5 lanes ->
        # 238 / 270 / 284 / 240 videos/s on 96-frame KSVQE samples: a fifth lane shares a queue and its graph serialises)
        nstream = max(1, int(self.config.get("streams", os.environ.get("KVQ_STREAMS", 4 if use_graph else 3))))
        # items are built on the device `prefetch` videos ahead by a host thread on its own stream (datasets/prefetch.py);
        # 0: in line, on the consuming stream
        # default: 2 when the forwards are enqueued eagerly (their ~6 ms of host work per video would otherwise wait for the
        # item), 0 under graph replay (a launch is 0.3 ms of host time, the replay already overlaps the next item's build;
        # measured 101 vs 92 videos/s end to end)
        depth = int(self.config.get("prefetch", 0 if use_graph else 2))
        if use_graph:
            from .graph import LaneGraphs
            cached = getattr(self, "_lane_graphs", None)           # recordings outlive one call (inferece_test + inferece_val)
            # ... but not a change of a Swin trunk's residual16: a recording replays the plans (fp16 or fp32 stream) it was made with
            r16 = tuple(bool(m.residual16) for m in self._swin_trunks())
            if cached is None or len(cached.lanes) != nstream or getattr(self, "_lane_graphs_r16", r16) != r16:
                cached = self._lane_graphs = LaneGraphs(self._run_model, [torch.cuda.Stream(device=self.device) for _ in range(nstream)])
            self._lane_graphs_r16 = r16
            graphs, lanes = cached, cached.lanes
        else:
            lanes = [main] + [torch.cuda.Stream(device=self.device) for _ in range(nstream - 1)]
            graphs = None
        # range guard (yml `range_guard`, default on): every Swin trunk ORs a bit per stage into a word of the lane's stream when its fp16
        # residual stream left the +-65504 range; after each video the lane moves the OR of its words into flags[j] and clears them, and
        # the flagged videos are scored again below with fp32 streams
        swins = self._swin_trunks() if self._range_guard() else []
        flags = torch.zeros(len(mine), dtype=torch.int32, device=self.device) if swins else None
        qm = self._quality_maps()
        writer = _MapWriter(self, qm, len(lanes)) if qm is not None else None
        if qm is not None and self._overlay_video() is not None:
            self._overlay_tables(self._overlay_video()["quality"])
        for st in lanes:
            for m in swins:
                m.clear_range_flags(st)
        for st in lanes:
            if st != main:
                st.wait_stream(main)
        if depth > 0:
            from .datasets.prefetch import DevicePrefetcher
            feed = DevicePrefetcher(self.val_dataset, mine, self.device, depth)
            items = iter(feed)
        else:
            feed, items = None, ((i, None, None) for i in mine)
        try:
            for j, (i, item, ready) in enumerate(items):
                lane = j % nstream
                with torch.cuda.stream(lanes[lane]):
                    if ready is not None:
                        lanes[lane].wait_event(ready)
                        feed.hand_over(item, lanes[lane])
                    else:
                        item = self.val_dataset[i]
                    inputs = self._model_inputs(item)
                    out = graphs.run(lane, inputs) if graphs is not None else self._run_model(inputs)
                    local[j] = self._pred(out).float().mean()     # pred.mean(0) over clips (trainer.py:282)
                    if writer is not None:
                        # device -> pinned host on this lane's stream, behind the forward (a replay's static outputs are read
                        # before the lane's next replay rewrites them: stream order); no synchronisation here
                        self._maps_note(out, item)
                        writer.put(lane, lanes[lane], self._name(i), out, local[j], item)
                    if swins:
                        self._take_range_flags(swins, lanes[lane], flags, j)
                if j == 0 and graphs is None and nstream > 1:
                    # the first forward (re)builds the lazily cached weight images (16-bit copies, packed panels, folded
                    # BatchNorms, bias images) on ITS stream; the other lanes read them — they must be complete first
                    torch.cuda.synchronize(self.device)
        finally:
            if feed is not None:
                feed.close()
        if writer is not None:
            writer.flush()
        for st in lanes:
            if st != main:
                main.wait_stream(st)
        if graphs is not None:
            self.graph_stats = (graphs.replays, graphs.eager_runs)
        self.range_flags = None                 # this rank's per-video stage bits of the last call (None: range_guard off)
        if swins:
            self.range_flags = flags.cpu().numpy()
            self._rescore_flagged(swins, self.range_flags, mine, local)
        return kd.gather_scores(local, n, self.rank, self.world).cpu().numpy()

    # ---- range guard of the fp16 residual stream ----------------------------------------------------------------------------
    def _range_guard(self) -> bool:
        v = self.config.get("range_guard", True)
        return v if isinstance(v, bool) else str(v).lower() not in ("0", "false", "off", "no")

    def _swin_trunks(self):
        from .models.backbones.swin_backbone import SwinTransformer3D
        return [m for m in self.model.modules() if isinstance(m, SwinTransformer3D)]

    @staticmethod
    def _take_range_flags(swins, stream, flags, j):
        """on `stream`, behind the video's forward (eager or a graph replay): flags[j] = OR of the trunks' words; the words are cleared"""
        words = [m.range_flags(stream) for m in swins]
        acc = words[0]
        for w in words[1:]:
            acc = acc | w
        flags[j:j + 1].copy_(acc)
        for m in swins:
            m.clear_range_flags(stream)

    @staticmethod
    def rescore_indices(flags) -> list:
        """positions j of the shard whose forward set any stage bit"""
        return [j for j, f in enumerate(np.asarray(flags).reshape(-1).tolist()) if int(f) != 0]

    def _rescore_flagged(self, swins, flags, mine, local):
        """score the flagged videos of this shard again on the current stream, eagerly, with fp32 residual streams in every trunk"""
        redo = self.rescore_indices(flags)
        if not redo:
            return
        saved = [m.residual16 for m in swins]
        try:
            for m in swins:
                m.residual16 = False
            qm = self._quality_maps()
            for j in redo:
                item = self.val_dataset[mine[j]]
                out = self._run_model(self._model_inputs(item))
                local[j] = self._pred(out).float().mean()
                if qm is not None:                 # the video's file is rewritten from the fp32-stream forward
                    host = {k: v.cpu() for k, v in out.items()}
                    host["score"] = float(local[j])
                    self._maps_write(qm, self._name(mine[j]), host, item)
        finally:
            for m, s in zip(swins, saved):
                m.residual16 = s
        bits = 0
        for j in redo:
            bits |= int(flags[j])
        stages = ",".join(str(i) for i in range(4) if bits >> i & 1)
        print(f"range guard: {len(redo)} video(s) re-scored with fp32 residual streams (fp16 stream out of range in stage(s) {stages})",
              file=sys.stderr)

    def inferece_test(self):
        scores = self._score_all()
        if self.rank == 0:
            with open("output.txt", "w") as f:
                for i, s in enumerate(scores):
                    f.write(f"{self._name(i)},{float(s)}\n")           # 'video_name,score' (trainer.py:331-334)
        return scores

    def _name(self, i):
        names = getattr(self.val_dataset, "video_names", None)
        return names[i] if names else f"synthetic_{i:05d}.mp4"

    def inferece_val(self, scores=None):
        from scipy.stats import kendalltau, pearsonr, spearmanr
        scores = self._score_all() if scores is None else scores
        labels = np.asarray(getattr(self.val_dataset, "labels"), np.float64)
        preds = self.rescale(list(scores), list(labels))
        s, p, k = spearmanr(labels, preds)[0], pearsonr(labels, preds)[0], kendalltau(labels, preds)[0]
        r = np.sqrt(((labels - preds) ** 2).mean())
        if self.rank == 0:
            print("SRCC{}PLCC{}KRCC{}RMSE{}".format(s, p, k, r))          # trainer.py:294
        return s, p, k, r

    def inferece(self):
        scores = self.inferece_test()
        if getattr(self.val_dataset, "labels", None) is not None and len(scores) > 2:
            self.inferece_val(scores)
        return scores

    # ---- head fine-tuning on the frozen trunk (the reference's train.py / train_eval_all_epoches for the head's parameters) ----------
    def finetune_head(self):
        """The reference's yml schema: ``num_epochs``, ``l_num_epochs``, ``warmup_epochs``, ``batch_size`` (samples per batch: clips of a ``VQAHead`` model, videos of ``simpleVQA``), ``ema``,
        ``save_model``, ``optimizer.{lr, wd, backbone_lr_mult}``, ``data.train`` (sampled deterministically, ``phase: test``) and
        ``data.val``.  Not in the reference — ``feature_bank: {draws: 1, dtype: fp32 | fp16 | bf16}``: the cached train features are
        ``draws`` samplings of every video (epoch e trains on draw ``e % draws``; with more than one, ``data.train`` keeps its own
        ``phase``, so ``train`` samples as the reference's training does) stored in ``dtype``; the validation cache stays fp32, one draw.  After every epoch the trained head and the EMA head are scored on ``data.val`` with the ``inferece_val``
        metrics and kept by the rule of trainer.py:223-230 in ``{resume}/{name}_head_{test_set}_{n|s}_finetuned.pth``.
        -> (best of the trained head, best of the EMA head), each (SRCC, PLCC, KRCC, RMSE)."""
        from .finetune import feature_bank_options, finetuner_for
        cfg, opt = self.config, self.config["optimizer"]
        if opt.get("backbone_lr_mult", 0) != 0:
            raise NotImplementedError(f"optimizer.backbone_lr_mult = {opt['backbone_lr_mult']}: this engine trains the head on a frozen "
                                      "trunk; set it to 0")
        if self.world > 1:
            raise NotImplementedError("finetune_head() runs on one rank")
        key = self.key_list[0]
        Finetuner = finetuner_for(getattr(self.model, key + "_head", None))       # VQAHead: HeadFinetuner; simpleVQAHead: its own
        draws, bank_dtype = feature_bank_options(cfg)
        tcfg = cfg["data"]["train"]
        targs = dict(tcfg["args"]) if draws > 1 else dict(tcfg["args"], phase="test")
        train_ds = getattr(_datasets, tcfg["type"])(targs, None, device=self.device)
        use_ema = bool(cfg.get("ema", True))
        ft = Finetuner(self.model, key, opt["lr"], opt["wd"], 1, 1, ema=use_ema, seed=int(cfg.get("seed", 0)),
                           rank_weight=float(cfg.get("rank_weight", 0.0)))
        ft.cache_features(train_ds, self, draws=draws, dtype=bank_dtype)
        n = sum(f.shape[0] for f in ft.feats)       # the samples of one draw: an epoch is one pass over one draw
        bs = int(cfg["batch_size"])
        per_epoch = n // bs + (1 if n % bs >= 3 else 0)
        ft.set_schedule(int(cfg["warmup_epochs"] * per_epoch), int((cfg["num_epochs"] + cfg["l_num_epochs"]) * per_epoch))
        val = Finetuner(self.model, key, opt["lr"], opt["wd"], 1, 1, ema=False)       # the cache of data.val's features
        val.cache_features(self.val_dataset, self)
        resume, test_set = getattr(self.args, "resume", "./checkpoint/"), getattr(self.args, "test_set", "val")
        save = bool(cfg.get("save_model", True))
        best = {"n": (-1, -1, -1, 1999), "s": (-1, -1, -1, 1999)}
        for epoch in range(int(cfg["num_epochs"])):
            log = ft.fit(1, bs)
            if log:
                print("train/total_loss", log[-1]["loss"], "train/plcc_loss", log[-1]["plcc_loss"], "lr", log[-1]["lr"])
            for suffix in ("n", "s") if use_ema else ("n",):
                scores = np.asarray([float(ft.predict(f, ema=suffix == "s").mean()) for f in val.feats])
                s, p, k, r = self.inferece_val(scores)
                bs_, bp, bk, br = best[suffix]
                if s + p > bs_ + bp and save:
                    ft.write_back(ema=suffix == "s")
                    os.makedirs(resume, exist_ok=True)
                    torch.save({"state_dict": {"module." + n_: v.detach().cpu() for n_, v in self.model.state_dict().items()},
                                "validation_results": tuple(float(v) for v in best[suffix])},       # plain floats: a weights-only load reads it
                               f"{resume}/{cfg['name']}_head_{test_set}_{suffix}_finetuned.pth")
                best[suffix] = (max(bs_, s), max(bp, p), max(bk, k), min(br, r))
                print({f"val_{suffix}/best_SRCC-{suffix}": best[suffix][0], f"val_{suffix}/best_PLCC-{suffix}": best[suffix][1],
                       f"val_{suffix}/best_KRCC-{suffix}": best[suffix][2], f"val_{suffix}/best_RMSE-{suffix}": best[suffix][3]})
        ft.write_back(ema=False)                 # the model ends with the trained head, as the reference's self.model does
        self.finetuner = ft
        return best["n"], best["s"]

    def rescale(self, pr, gt=None):
        pr = np.asarray(pr, np.float64)
        if gt is None:
            return (pr - np.mean(pr)) / np.std(pr)
        return ((pr - np.mean(pr)) / np.std(pr)) * np.std(gt) + np.mean(gt)
