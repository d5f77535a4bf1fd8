"""Head fine-tuning on a frozen trunk: the reference's training step (``trainer.py:129-172``) for the 49 k parameters of a ``VQAHead``,
on cached features of the frozen backbone.  Forward, loss, backward, AdamW and the EMA copy are the launches of csrc/headtrain.hip
(``kernels.headtrain_*``); nothing here goes through autograd, and no gradient reaches a backbone.

    ft = HeadFinetuner(model, "swin_tiny_grpb", lr=1e-3, wd=0.05, warmup_iters=10, max_iters=100)
    ft.cache_features(dataset, trainer)          # one frozen forward per video, into the feature bank
    ft.fit(epochs=5, batch_size=16)
    ft.write_back()                              # the VQAHead's nn.Parameters now hold the trained weights

The dropout masks are this project's counter-based hash of (seed, step, which, element) (csrc/headtrain.hpp): torch's random stream
cannot be reproduced, and a hash needs no mask tensor.  Built: ``VQAHead`` with one class, hidden 64, no pre-pool, channels a multiple
of 64, batches of 2 .. 1024 clips.

The cached features live in one **feature bank** (``kernels.FeatureBank``, csrc/featbank.hip): ``[draws * samples][L][C]`` in fp32, fp16
or bf16, written by the store launch straight from the trunk's output.  ``cache_features(..., draws=K)`` samples every video K times
(``dataset.set_draw(k)``: the reference re-samples every video in every epoch); epoch ``e`` trains on draw ``e % K``.  A batch is an int32
index vector into the bank: the step's launches read the rows where they lie and widen 16-bit rows in registers, which is exact, so a
step on a bank equals the dense fp32 step on the widened rows bit for bit.

``SimpleHeadFinetuner`` is the same for the 1.2 M parameters of a ``simpleVQAHead`` (model key ``simpleVQA``): two Linears per frame and
the mean over the frames, no dropout (csrc/simple_headtrain.hip, ``kernels.simple_headtrain_*``); a sample is one video's (T, C) feature
rows.  Built: hidden 128, channels a multiple of 64.  The two classes share everything but the head's own launches (``_Finetuner``).
"""
from __future__ import annotations

import math

import torch

from . import _abi, kernels
from .models.head import VQAHead, simpleVQAHead

HIDDEN = 64
SIMPLE_HIDDEN = 128


def lr_factor(it: int, warmup_iters: int, max_iters: int) -> float:
    """the reference's LambdaLR factor at iteration ``it`` (trainer.py:106-113)"""
    if it <= warmup_iters:
        return it / warmup_iters
    return 0.5 * (1 + math.cos(math.pi * (it - warmup_iters) / max_iters))


def _widened(feats):
    """dense fp32 [B][L][C] of features on the device: 16-bit rows (a bank's) are widened by the gather launch, exactly"""
    if feats.dtype in kernels.HALF_TYPES:
        bank = kernels.FeatureBank.of(feats.contiguous())
        return kernels.feature_bank_rows(bank, torch.arange(bank.n_rows, dtype=torch.int32, device=feats.device))
    return feats.to(torch.float32).contiguous()


class _Finetuner:
    """What the finetuners of the two head types share: the flat parameter vector with its AdamW state and EMA copy, the schedule, the
    feature cache, the step around the head's own launches, the epochs and the write-back.  A subclass sets ``hidden`` and gives
    ``_check_head`` (refusals; -> in_channels), ``_head_params`` (the head's four nn.Parameters in flat order), ``_clip_features``
    (the backbone's output of one video -> [samples][L][C]), ``_forward(bank, index, ws)`` / ``_backward(bank, index, ws, dscore)``
    (the head's launches on the rows ``index`` of a bank) and ``predict``."""
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
        self.bank, self.n, self.draws, self.epoch = None, 0, 1, 0    # epoch: passes fit() has made, kept across calls: it picks the draw
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
    def cache_features(self, dataset, trainer, draws=1, dtype=torch.float32):
        """``draws`` eval-mode forwards of the frozen model per video (draw k after ``dataset.set_draw(k)``, if the dataset has it), each
        stored by one launch from the model's output into the feature bank: ``bank.tensor`` [draws * n][L][C] of ``dtype`` (fp32, fp16
        or bf16), row = draw * n + sample, n = videos * samples per video (VQAHead: a clip's feature map, channels-last; simpleVQAHead:
        a video's T feature rows).  ``feats`` is the list of per-video views of draw 0, with the video's label in ``labels``.
        An fp16 bank that would have to saturate a value, or any bank that met a NaN, raises ValueError."""
        draws = int(draws)
        if draws < 1:
            raise ValueError(f"draws = {draws}: at least one draw per video")
        code = _abi.bank_dtype_code(dtype)
        tdtype = _abi.bank_torch_dtype(code)
        self._trainer = trainer
        self.model.eval()
        self.feats, self.labels, self.names, self.bank = [], [], [], None
        videos = len(dataset)
        flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        per = None
        try:
            for k in range(draws):
                if hasattr(dataset, "set_draw"):
                    dataset.set_draw(k)
                for i in range(videos):
                    item = dataset[i]
                    with torch.no_grad():
                        out = self.model(inputs=trainer._model_inputs(item), return_pooled_feats=True, reduce_scores=True)
                    feat = out[1][self.key]          # (scores, feats[, contrastive loss]); KSVQE's (features, loss) is split by the model
                    if isinstance(feat, (tuple, list)):
                        feat = feat[0]
                    view = self._clip_features(feat)             # fp32 [samples][L][C], channel stride 1: a view where the layout allows
                    if self.bank is None:
                        per = tuple(view.shape)
                        rows = draws * videos * per[0]
                        need = rows * per[1] * per[2] * torch.empty(0, dtype=tdtype).element_size()
                        free = torch.cuda.mem_get_info(self.device)[0]
                        if need > free:
                            raise ValueError(f"a feature bank of {rows} rows x {per[1]} x {per[2]} takes {need} bytes with draws = {draws}, dtype = "
                                             f"{tdtype}: the device has {free} bytes free (fewer draws, or a 16-bit dtype)")
                        self.bank = kernels.FeatureBank(rows, per[1], per[2], tdtype, device=self.device)
                    elif tuple(view.shape) != per:
                        raise NotImplementedError("the cached videos have feature maps of different sizes: one batch needs one (L, C)")
                    kernels.feature_bank_store(view, self.bank, (k * videos + i) * per[0], flag)
                    if k == 0:
                        self.labels.append(float(item["label"]))
                        self.names.append(item.get("video_name", str(i)) if isinstance(item, dict) else str(i))
        finally:
            if hasattr(dataset, "set_draw"):
                dataset.set_draw(0)
        if videos and int(flag.item()):                          # the one synchronisation of caching
            self.bank = None
            raise ValueError(f"the features do not fit a {tdtype} bank: a value past +-65504 (fp16 would store it saturated) or a NaN was met; "
                             "use dtype bf16 or fp32")
        self.draws, self.epoch = draws, 0
        self.n = videos * per[0] if videos else 0
        self.feats = [self.bank.tensor[i * per[0]:(i + 1) * per[0]] for i in range(videos)]
        return len(self.feats)

    def sample_labels(self):
        """the label of every sample of one draw, [n] on the device: every cached clip carries its video's label"""
        return torch.tensor([l for f, l in zip(self.feats, self.labels) for _ in range(f.shape[0])], dtype=torch.float32, device=self.device)

    def clip_samples(self):
        """every cached clip of draw 0 as one sample carrying its video's label -> (feats fp32 [N][L][C], labels [N]); an fp32 bank
        gives a view of its rows, a 16-bit bank a widened copy"""
        if not self.feats:
            raise RuntimeError("no cached features: call cache_features(dataset, trainer) first")
        feats = self.bank.tensor[:self.n]
        if feats.dtype != torch.float32:
            feats = kernels.feature_bank_rows(self.bank, torch.arange(self.n, dtype=torch.int32, device=self.device))
        return feats, self.sample_labels()

    # ---- one optimisation step -----------------------------------------------------------------------------------------------------
    def _workspace(self, B, L):
        ws = self._ws.get((B, L))
        if ws is None:
            ws = self._ws[(B, L)] = self._new_workspace(B, L)
        return ws

    def current_lr(self) -> float:
        return self.lr * lr_factor(self.it, self.warmup_iters, self.max_iters)

    def _step(self, bank, index, labels):
        """one step on the rows ``index`` (int32 on the device) of ``bank``"""
        ws = self._workspace(index.numel(), bank.L)
        score = self._forward(bank, index, ws)
        out3, dscore = kernels.headtrain_loss(score, labels, self.rank_weight)
        self._backward(bank, index, ws, dscore)
        lr = self.current_lr()
        kernels.headtrain_adamw(self.params, self.grads, self.exp_avg, self.exp_avg_sq, self.ema, lr, self.wd, self.it + 1)
        self.it += 1
        loss, plcc, rank = out3.tolist()
        return {"loss": loss, "plcc_loss": plcc, "rank_loss": rank, "lr": lr}

    def step(self, feats, labels):
        """forward, loss, backward, AdamW, scheduler, EMA on one batch: feats fp32 [B][L][C] on the device, labels [B].
        -> dict(loss, plcc_loss, rank_loss, lr), the learning rate being the one this step applied"""
        feats = feats.to(self.device, torch.float32).contiguous()
        labels = torch.as_tensor(labels, dtype=torch.float32).to(self.device).reshape(-1).contiguous()
        B, L, C = feats.shape
        if C != self.C or labels.numel() != B:
            raise ValueError(f"step(): features {tuple(feats.shape)} / {labels.numel()} labels do not fit a {self.C}-channel head")
        ident = self._ws.get(B)                      # the batch as a bank: its own rows under the index 0 .. B-1, made once per B
        if ident is None:
            ident = self._ws[B] = torch.arange(B, dtype=torch.int32, device=self.device)
        return self._step(kernels.FeatureBank.of(feats), ident, labels)

    def step_indexed(self, index, labels):
        """``step`` on the bank rows ``index`` (int32 on the device, or a CPU tensor, which is checked against the bank and uploaded),
        read in place: equal to ``step(feature_bank_rows(bank, index), labels)`` bit for bit, without the gathered copy"""
        if self.bank is None:
            raise RuntimeError("no feature bank: call cache_features(dataset, trainer) first")
        index = kernels.bank_index(index, self.bank)
        labels = torch.as_tensor(labels, dtype=torch.float32).to(self.device).reshape(-1).contiguous()
        B = index.numel()
        if self.bank.C != self.C or labels.numel() != B:
            raise ValueError(f"step_indexed(): {B} rows of a bank {tuple(self.bank.tensor.shape)} / {labels.numel()} labels do not fit a "
                             f"{self.C}-channel head")
        return self._step(self.bank, index, labels)

    def fit(self, epochs, batch_size):
        """``epochs`` passes over the cached samples: pass e (counted across calls) trains on draw ``e % draws``; a seeded permutation of
        the n samples is cut into batches of ``batch_size``, each an index vector ``draw * n + order[s:s + batch_size]`` into the bank; a
        last batch shorter than 3 is dropped (with two samples the PLCC loss is constant).  -> the list of step results"""
        if not self.feats:
            raise RuntimeError("no cached features: call cache_features(dataset, trainer) first")
        labels = self.sample_labels()
        n, log = self.n, []
        for _ in range(int(epochs)):
            draw = self.epoch % self.draws
            self.epoch += 1
            order = torch.randperm(n, generator=self._perm)
            for s in range(0, n, int(batch_size)):
                idx = order[s:s + int(batch_size)]
                if idx.numel() < 3:
                    continue
                idx = idx.to(self.device)
                log.append(self.step_indexed((idx + draw * n).to(torch.int32), labels.index_select(0, idx)))
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
        # the trunk stores its output channels-last behind the (B, C, D, H, W) view: the permutation is then dense and the reshape a
        # view, which the store launch reads in place; any other layout is copied here
        return feat.to(torch.float32).permute(0, 2, 3, 4, 1).reshape(B, -1, C)

    def _new_workspace(self, B, L):
        return kernels.headtrain_workspace(B, L, self.C, HIDDEN, device=self.device)

    def _forward(self, bank, index, ws):
        return kernels.headtrain_bank_forward(bank, index, self.params, self.p_drop, self.seed, self.it, ws)

    def _backward(self, bank, index, ws, dscore):
        kernels.headtrain_bank_backward(bank, index, self.params, self.p_drop, self.seed, self.it, ws, dscore, self.grads)

    def predict(self, feats, ema=False):
        """eval-mode scores [B] of features [B][L][C] (fp32, or the 16-bit rows of a bank, widened here) with the current weights
        (``ema``: the EMA copy), by the inference launch"""
        feats = _widened(feats.to(self.device))
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
        return feat.to(torch.float32)                # (rows, T, C) as the backbone gives it

    def _new_workspace(self, B, L):
        return kernels.simple_headtrain_workspace(B, L, self.C, SIMPLE_HIDDEN, device=self.device)

    def _forward(self, bank, index, ws):
        return kernels.simple_headtrain_bank_forward(bank, index, self.params, ws)

    def _backward(self, bank, index, ws, dscore):
        kernels.simple_headtrain_bank_backward(bank, index, self.params, ws, dscore, self.grads)

    def predict(self, feats, ema=False):
        """scores [B] of features [B][T][C] with the current weights (``ema``: the EMA copy), by the inference launch"""
        w1, b1, w2, b2 = self._split(self._weights(ema))
        return kernels.simple_vqa_head(_widened(feats.to(self.device)), w1, b1, w2, b2).reshape(-1)


BANK_KEYS = ("draws", "dtype")
BANK_DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def feature_bank_options(cfg):
    """the optional top-level yml key ``feature_bank: {draws: 1, dtype: fp32 | fp16 | bf16}`` -> (draws, torch dtype); absent: (1, fp32),
    the behaviour without the key.  An unknown key or value raises ValueError naming it."""
    fb = cfg.get("feature_bank")
    if fb is None:
        return 1, torch.float32
    if not isinstance(fb, dict):
        raise ValueError(f"feature_bank: expected a mapping with the keys {', '.join(BANK_KEYS)}, got {fb!r}")
    for k in fb:
        if k not in BANK_KEYS:
            raise ValueError(f"feature_bank: unknown key {k!r} (known: {', '.join(BANK_KEYS)})")
    draws, name = fb.get("draws", 1), fb.get("dtype", "fp32")
    if isinstance(draws, bool) or not isinstance(draws, int) or draws < 1:
        raise ValueError(f"feature_bank.draws must be an integer of at least 1, got {draws!r}")
    if name not in BANK_DTYPES:
        raise ValueError(f"feature_bank.dtype must be one of {', '.join(BANK_DTYPES)}, got {name!r}")
    return draws, BANK_DTYPES[name]


def finetuner_for(head):
    """the finetuner class that trains ``head``; a type without one gets HeadFinetuner's refusal"""
    return SimpleHeadFinetuner if isinstance(head, simpleVQAHead) else HeadFinetuner
