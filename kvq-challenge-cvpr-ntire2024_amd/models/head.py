"""Host-side mirror of the reference's ``models/head.py`` (``VQAHead`` :33-68, ``simpleVQAHead``
:10-31).  Parameter names/shapes are the reference's; forward calls libkvq_hip.so.
``forward`` is the eval-mode head: dropout is the identity (``model.eval()`` in ``trainer.py:257,303``).  The train-mode head
(dropout on the features and behind the GELU), its losses and its optimiser step live in ``kvq_amd/finetune.py``
(``HeadFinetuner``, csrc/headtrain.hip), which works on a ``VQAHead``'s parameters and writes the trained ones back into them;
``SimpleHeadFinetuner`` (csrc/simple_headtrain.hip) does the same for a ``simpleVQAHead``."""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import kernels
from .._prepared import PreparedCache, to_f32
from .backbones.swin_backbone import _Affine


class VQAHead(nn.Module):
    def __init__(self, in_channels=768, hidden_channels=64, num_class=1, dropout_ratio=0.5, pre_pool=False,
                 **kwargs):
        super().__init__()
        self.in_channels, self.hidden_channels, self.num_class = in_channels, hidden_channels, num_class
        self.dropout_ratio, self.pre_pool = dropout_ratio, pre_pool
        self.fc_hid = _Affine((hidden_channels, in_channels, 1, 1, 1), (hidden_channels,))
        self.fc_last = _Affine((num_class, hidden_channels, 1, 1, 1), (num_class,))
        with torch.no_grad():
            nn.init.trunc_normal_(self.fc_hid.weight, std=0.02)
            nn.init.trunc_normal_(self.fc_last.weight, std=0.02)
        self._cache = PreparedCache()

    def _prepared(self, device):
        """fp32 device copies in the layouts the kernels stream (W1 as it is and transposed), rebuilt only when a
        parameter changed (version / data_ptr) — no per-forward conversion kernels."""
        ps = (self.fc_hid.weight, self.fc_hid.bias, self.fc_last.weight, self.fc_last.bias)

        def build():
            w1, b1, w2, b2 = (to_f32(p, device) for p in ps)
            w1 = w1.reshape(self.hidden_channels, -1)
            return w1.t().contiguous(), b1, w2.reshape(-1), b2, w1
        return self._cache.get((str(device),), ps, build)

    def forward(self, x, rois=None, return_map=False):
        """x (B, C, D, H, W) fp32 (any strides) -> (B, num_class).  ``return_map``: ``(score, token_map (B,D,H,W), timeline (B,D))``
        — fc_last's output per token (head.py:65, its mean is the score) and its mean per depth slice."""
        w1t, b1, w2, b2, w1 = self._prepared(x.device)
        if self.num_class != 1 or self.pre_pool:      # head.py:61-62, :66-67 — no reference config takes these branches
            if return_map:
                raise NotImplementedError("VQAHead(return_map=True): " + (
                    "pre_pool averages the token grid in front of the head, so there is no per-token score" if self.pre_pool
                    else "with num_class > 1 a token has a class distribution, not one score"))
            return kernels.vqa_head_classes(x.to(torch.float32), w1, b1, w2.reshape(self.num_class, -1), b2,
                                            pre_pool=self.pre_pool)
        return kernels.vqa_head(x.to(torch.float32), w1, b1, w2, b2, w1t=w1t, return_map=return_map)


class simpleVQAHead(nn.Module):  # noqa: N801  (reference spelling)
    def __init__(self, in_channels=4096 + 2048 + 1024 + 2048 + 256, hidden_channels=128):
        super().__init__()
        self.quality = nn.Sequential(_Affine((hidden_channels, in_channels), (hidden_channels,)),
                                     _Affine((1, hidden_channels), (1,)))
        with torch.no_grad():
            nn.init.trunc_normal_(self.quality[0].weight, std=0.02)
            nn.init.trunc_normal_(self.quality[1].weight, std=0.02)

    def forward(self, x):
        """x (B, T, Cin) fp32 -> (B, 1): two Linears, no activation, mean over frames."""
        f32 = lambda p: p.detach().to(device=x.device, dtype=torch.float32).contiguous()  # noqa: E731
        q0, q1 = self.quality[0], self.quality[1]
        return kernels.simple_vqa_head(x.to(torch.float32), f32(q0.weight), f32(q0.bias), f32(q1.weight).reshape(-1),
                                       f32(q1.bias))
