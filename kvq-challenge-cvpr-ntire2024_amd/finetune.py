"""Head fine-tuning on a frozen trunk: the reference's training step (``trainer.py:129-172``) for the 49 k parameters of a ``VQAHead``,
on cached features of the frozen backbone.  Forward, loss, backward, AdamW and the EMA copy are the launches of csrc/headtrain.hip
(``kernels.headtrain_*``); nothing here goes through autograd, and no gradient reaches a backbone.

    ft = HeadFinetuner(model, "swin_tiny_grpb", lr=1e-3, wd=0.05, warmup_iters=10, max_iters=100)
    ft.cache_features(dataset, trainer)          # one frozen forward per video
    ft.fit(epochs=5, batch_size=16)
    ft.write_back()                              # the VQAHead's nn.Parameters now hold the trained weights

The dropout masks are this project's counter-based hash of (seed, step, which, element) (csrc/headtrain.hpp): torch's random stream
cannot be reproduced, and a hash needs no mask tensor.  Built: ``VQAHead`` with one class, hidden 64, no pre-pool, channels a multiple
of 64, batches of 2 .. 1024 clips.

``SimpleHeadFinetuner`` is the same for the 1.2 M parameters of a ``simpleVQAHead`` (model key ``simpleVQA``): two Linears per frame and
the mean over the frames, no dropout (csrc/simple_headtrain.hip, ``kernels.simple_headtrain_*``); a sample is one video's (T, C) feature
rows.  Built: hidden 128, channels a multiple of 64.  The two classes share everything but the head's own launches (``_Finetuner``).
"""
from __future__ import annotations

import math

import torch

from . import kernels
from .models.head import VQAHead, simpleVQAHead

HIDDEN = 64
SIMPLE_HIDDEN = 128


def lr_factor(it: int, warmup_iters: int, max_iters: int) -> float:
    """the reference's LambdaLR factor at iteration ``it`` (trainer.py:106-113)"""
    if it <= warmup_iters:
        return it / warmup_iters
    return 0.5 * (1 + math.cos(math.pi * (it - warmup_iters) / max_iters))


class _Finetuner:
    """What the finetuners of the two head types share: the flat parameter vector with its AdamW state and EMA copy, the schedule, the
    feature cache, the step around the head's own launches, the epochs and the write-back.  A subclass sets ``hidden`` and gives
    ``_check_head`` (refusals; -> in_channels), ``_head_params`` (the head's four nn.Parameters in flat order), ``_clip_features``
    (the backbone's output of one video -> [samples][L][C]), ``_forward`` / ``_backward`` (the launches) and ``predict``."""
    hidden = None

    def __init__(self, model, key, lr, wd, warmup_iters, max_iters, ema=True, seed=0, rank_weight=0.0):
        head = getattr(model, key + "_head", None)
        if head is None:
            raise KeyError(f"the model has no head '{key}_head' (model keys: {getattr(model, 'key_names', [])})")
        self.C = self._check_head(key, head)
        self.set_schedule(warmup_iters, max_iters)
        self.model, self.key, self.head = model, key, head
        self.lr, self.wd = float(lr), float(wd)
        self.seed, self.rank_weight, self.p_drop = int(seed), float(rank_weight), float(getattr(head, "dropout_ratio", 0.0))
        ps = self._head_params()
        self.device = ps[0].device
        self.params = torch.cat([p.detach().to(torch.float32).reshape(-1) for p in ps]).contiguous()
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.ema = self.params.clone() if ema else None
        self.grads = torch.empty_like(self.params)
        self.it = 0                                  # iterations done = the scheduler's counter = the mask hash's step
        self.feats, self.labels, self.names = [], [], []
        self._trainer = None
        self._ws = {}
        self._perm = torch.Generator().manual_seed(self.seed)

    def set_schedule(self, warmup_iters, max_iters):
        """the scheduler's two lengths, in iterations (a caller that counts batches only after caching sets them then)"""
        if int(warmup_iters) == 0:
            raise ValueError("warmup_iters == 0: the reference's schedule divides by it (trainer.py:110)")
        if int(warmup_iters) < 0 or int(max_iters) <= 0:
            raise ValueError(f"warmup_iters {warmup_iters} / max_iters {max_iters}: both count iterations")
        self.warmup_iters, self.max_iters = int(warmup_iters), int(max_iters)

    # ---- features of the frozen trunk ---------------------------------------------------------------------------------------------
    def cache_features(self, dataset, trainer):
        """one eval-mode forward of the frozen model per video: keeps every sample's fp32 features on the device, [samples][L][C]
        (VQAHead: a clip's feature map, channels-last; simpleVQAHead: a video's T feature rows), with the video's label"""
        self._trainer = trainer
        self.model.eval()
        self.feats, self.labels, self.names = [], [], []
        for i in range(len(dataset)):
            item = dataset[i]
            with torch.no_grad():
                out = self.model(inputs=trainer._model_inputs(item), return_pooled_feats=True, reduce_scores=True)
            feat = out[1][self.key]                  # (scores, feats[, contrastive loss]); KSVQE's (features, loss) is split by the model
            if isinstance(feat, (tuple, list)):
                feat = feat[0]
            self.feats.append(self._clip_features(feat))
            self.labels.append(float(item["label"]))
            self.names.append(item.get("video_name", str(i)) if isinstance(item, dict) else str(i))
        return len(self.feats)

    def clip_samples(self):
        """every cached clip as one sample carrying its video's label -> (feats [N][L][C], labels [N])"""
        if not self.feats:
            raise RuntimeError("no cached features: call cache_features(dataset, trainer) first")
        if len({f.shape[1:] for f in self.feats}) != 1:
            raise NotImplementedError("the cached videos have feature maps of different sizes: one batch needs one (L, C)")
        labels = torch.tensor([l for f, l in zip(self.feats, self.labels) for _ in range(f.shape[0])], dtype=torch.float32, device=self.device)
        return torch.cat(self.feats), labels

    # ---- one optimisation step -----------------------------------------------------------------------------------------------------
    def _workspace(self, B, L):
        ws = self._ws.get((B, L))
        if ws is None:
            ws = self._ws[(B, L)] = self._new_workspace(B, L)
        return ws

    def current_lr(self) -> float:
        return self.lr * lr_factor(self.it, self.warmup_iters, self.max_iters)

    def step(self, feats, labels):
        """forward, loss, backward, AdamW, scheduler, EMA on one batch: feats fp32 [B][L][C] on the device, labels [B].
        -> dict(loss, plcc_loss, rank_loss, lr), the learning rate being the one this step applied"""
        feats = feats.to(self.device, torch.float32).contiguous()
        labels = torch.as_tensor(labels, dtype=torch.float32).to(self.device).reshape(-1).contiguous()
        B, L, C = feats.shape
        if C != self.C or labels.numel() != B:
            raise ValueError(f"step(): features {tuple(feats.shape)} / {labels.numel()} labels do not fit a {self.C}-channel head")
        ws = self._workspace(B, L)
        score = self._forward(feats, ws)
        out3, dscore = kernels.headtrain_loss(score, labels, self.rank_weight)
        self._backward(feats, ws, dscore)
        lr = self.current_lr()
        kernels.headtrain_adamw(self.params, self.grads, self.exp_avg, self.exp_avg_sq, self.ema, lr, self.wd, self.it + 1)
        self.it += 1
        loss, plcc, rank = out3.tolist()
        return {"loss": loss, "plcc_loss": plcc, "rank_loss": rank, "lr": lr}

    def fit(self, epochs, batch_size):
        """``epochs`` passes over the cached clips: a seeded permutation cut into batches of ``batch_size``; a last batch shorter than 3
        is dropped (with two samples the PLCC loss is constant).  -> the list of step() results"""
        feats, labels = self.clip_samples()
        n, log = feats.shape[0], []
        for _ in range(int(epochs)):
            order = torch.randperm(n, generator=self._perm)
            for s in range(0, n, int(batch_size)):
                idx = order[s:s + int(batch_size)]
                if idx.numel() < 3:
                    continue
                idx = idx.to(self.device)
                log.append(self.step(feats.index_select(0, idx), labels.index_select(0, idx)))
        return log

    # ---- the trained head ------------------------------------------------------------------------------------------------------------
    def _split(self, flat):
        H, nW = self.hidden, self.hidden * self.C
        return flat[:nW].view(H, self.C), flat[nW:nW + H], flat[nW + H:nW + 2 * H], flat[nW + 2 * H:]

    def _weights(self, ema):
        if ema and self.ema is None:
            raise ValueError("this finetuner keeps no EMA copy (ema=False)")
        return self.ema if ema else self.params

    def write_back(self, ema=False, trainer=None):
        """copy the trained parameters (``ema``: the EMA copy) into the head's nn.Parameters: ``VQA_Network.forward`` and
        ``state_dict()`` see them, the head rebuilds its prepared images, and the trainer's recorded hipGraphs are dropped"""
        with torch.no_grad():
            for dst, src in zip(self._head_params(), self._split(self._weights(ema))):
                dst.copy_(src.reshape(dst.shape))
        trainer = trainer if trainer is not None else self._trainer
        if trainer is not None:
            trainer._lane_graphs = None


class HeadFinetuner(_Finetuner):
    hidden = HIDDEN

    def _check_head(self, key, head):
        if not isinstance(head, VQAHead):
            raise NotImplementedError(f"{key}_head is a {type(head).__name__}: HeadFinetuner is built for VQAHead only"
                                      + (" (a simpleVQAHead is trained by SimpleHeadFinetuner)" if isinstance(head, simpleVQAHead) else ""))
        if head.num_class != 1:
            raise NotImplementedError(f"{key}_head has num_class = {head.num_class}: the training step is built for one class")
        if head.pre_pool:
            raise NotImplementedError(f"{key}_head has pre_pool: the training step is built for the per-token head")
        if head.hidden_channels != HIDDEN or head.in_channels % 64:
            raise NotImplementedError(f"{key}_head is {head.in_channels} -> {head.hidden_channels}: the training step is built for "
                                      "hidden_channels 64 and in_channels a multiple of 64")
        return head.in_channels

    def _head_params(self):
        h = self.head
        return h.fc_hid.weight, h.fc_hid.bias, h.fc_last.weight, h.fc_last.bias

    def _clip_features(self, feat):
        B, C = feat.shape[:2]                        # (clips, C, D, H, W) -> channels-last [clips][L][C]
        return feat.to(torch.float32).reshape(B, C, -1).transpose(1, 2).contiguous()

    def _new_workspace(self, B, L):
        return kernels.headtrain_workspace(B, L, self.C, HIDDEN, device=self.device)

    def _forward(self, feats, ws):
        return kernels.headtrain_forward(feats, self.params, self.p_drop, self.seed, self.it, ws)

    def _backward(self, feats, ws, dscore):
        kernels.headtrain_backward(feats, self.params, self.p_drop, self.seed, self.it, ws, dscore, self.grads)

    def predict(self, feats, ema=False):
        """eval-mode scores [B] of features [B][L][C] with the current weights (``ema``: the EMA copy), by the inference launch"""
        feats = feats.to(self.device, torch.float32).contiguous()
        B, L, C = feats.shape
        w1, b1, w2, b2 = self._split(self._weights(ema))
        x = feats.as_strided((B, C, 1, 1, L), (L * C, 1, L * C, L * C, C))
        return kernels.vqa_head(x, w1, b1, w2, b2).reshape(-1)


class SimpleHeadFinetuner(_Finetuner):
    """``HeadFinetuner``'s surface for a ``simpleVQAHead``: a sample is one row of the backbone's (rows, T, C) output, the T feature rows
    of one video (``num_clips: 1``: one sample per video)."""
    hidden = SIMPLE_HIDDEN

    def _check_head(self, key, head):
        if not isinstance(head, simpleVQAHead):
            raise NotImplementedError(f"{key}_head is a {type(head).__name__}: SimpleHeadFinetuner is built for simpleVQAHead only")
        hid, cin = head.quality[0].weight.shape
        if hid != SIMPLE_HIDDEN:
            raise NotImplementedError(f"{key}_head has hidden_channels = {hid}: the training step is built for hidden_channels 128")
        if cin % 64:
            raise NotImplementedError(f"{key}_head has in_channels = {cin}: the training step is built for a multiple of 64")
        return cin

    def _head_params(self):
        q = self.head.quality
        return q[0].weight, q[0].bias, q[1].weight, q[1].bias

    def _clip_features(self, feat):
        return feat.to(torch.float32).contiguous()   # (rows, T, C) as the backbone gives it

    def _new_workspace(self, B, L):
        return kernels.simple_headtrain_workspace(B, L, self.C, SIMPLE_HIDDEN, device=self.device)

    def _forward(self, feats, ws):
        return kernels.simple_headtrain_forward(feats, self.params, ws)

    def _backward(self, feats, ws, dscore):
        kernels.simple_headtrain_backward(feats, self.params, ws, dscore, self.grads)

    def predict(self, feats, ema=False):
        """scores [B] of features [B][T][C] with the current weights (``ema``: the EMA copy), by the inference launch"""
        w1, b1, w2, b2 = self._split(self._weights(ema))
        return kernels.simple_vqa_head(feats.to(self.device, torch.float32), w1, b1, w2, b2).reshape(-1)


def finetuner_for(head):
    """the finetuner class that trains ``head``; a type without one gets HeadFinetuner's refusal"""
    return SimpleHeadFinetuner if isinstance(head, simpleVQAHead) else HeadFinetuner
