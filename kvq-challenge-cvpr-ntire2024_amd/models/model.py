"""Host-side mirror of the reference's ``models/model.py`` (``VQA_Network`` :18-121) — THE drop-in
boundary: same constructor (``config`` dict from config/*.yml), same attribute
names (``<key>_backbone`` / ``<key>_head``, ``key_names``, ``multi``, ``layer``), same ``forward``
signature and return structure."""
from __future__ import annotations

from functools import reduce

import torch.nn as nn

from .backbones.swin_backbone import SwinTransformer3D as VideoBackbone
from .backbones.swin_backbone import swin_3d_small, swin_3d_tiny
from .head import VQAHead, simpleVQAHead


class VQA_Network(nn.Module):  # noqa: N801  (reference spelling)
    def __init__(self, config):
        super().__init__()
        self.config = config
        self.key_names = []
        self.multi = False
        self.layer = -1
        for key, hypers in config["model"]["args"].items():
            hypers = hypers or {}
            if key == "swin_tiny":
                backbone = swin_3d_tiny(**(hypers.get("backbone") or {}))
                head = VQAHead(**(hypers.get("head") or {}))
            elif key == "swin_tiny_grpb":
                backbone = VideoBackbone()                      # GRPB trunk = FAST-VQA / the KSVQE trunk
                head = VQAHead(**(hypers.get("head") or {}))
            elif key == "swin_tiny_grpb_m":
                backbone = VideoBackbone(window_size=(4, 4, 4), frag_biases=[0, 0, 0, 0])
                head = VQAHead(**(hypers.get("head") or {}))
            elif key == "swin_small":
                backbone = swin_3d_small(**(hypers.get("backbone") or {}))
                head = VQAHead(**(hypers.get("head") or {}))
            elif key == "simpleVQA":
                from .backbones.simpleVQA_model import resnet50 as simpleVQA_Backbone
                backbone = simpleVQA_Backbone(pretrained=False)
                head = simpleVQAHead(**(hypers.get("head") or {}))
            elif key == "KSVQE":                                # the reference reads these keys one by one (model.py:59-68)
                from .backbones.KSVQE_model import KSVQE as KSVQE_Backbone
                bk = hypers["backbone"]
                backbone = KSVQE_Backbone(num_samples=bk["num_samples"], sample_type=bk["sample_type"],
                                          CLIP_location=bk["CLIP_location"], cls_use=bk["cls_use"],
                                          tuning_stage=bk["tuning_stage"], a1=bk.get("a1", 1), a2=bk.get("a2", 0),
                                          frozen_stages=bk.get("frozen_stages", -1))
                head = VQAHead(**(hypers.get("head") or {}))
            elif key == "conv_tiny":
                # the reference's key calls convnext_3d_tiny(pretrained=True) (model.py:49-50), which downloads ImageNet weights; an
                # offline engine wants the choice spelled out
                bk = hypers.get("backbone") or {}
                if "pretrained" not in bk or bk["pretrained"] is True:
                    raise NotImplementedError("conv_tiny: the reference downloads ImageNet weights from a URL here; set "
                                              "backbone.pretrained to a local checkpoint or false")
                from .backbones.conv_backbone import convnext_3d_tiny
                backbone = convnext_3d_tiny(**bk)
                head = VQAHead(**(hypers.get("head") or {}))
            elif key == "conv_v2_tiny":
                # the reference's V2 factories never download (conv_backbone.py:603-625): a missing ``pretrained`` means false
                from .backbones.conv_backbone import convnextv2_3d_tiny
                backbone = convnextv2_3d_tiny(**(hypers.get("backbone") or {}))
                head = VQAHead(**(hypers.get("head") or {}))
            else:
                raise NotImplementedError
            self.key_names.append(key)
            setattr(self, key + "_backbone", backbone)
            setattr(self, key + "_head", head)

    def forward(self, inputs, targets=None, inference=True, return_pooled_feats=False, reduce_scores=False,
                pooled=False, clip_return=False, return_maps=False, **kwargs):
        """``return_maps``: returns ``(what it returns otherwise, maps)``; ``maps[key] = {"token_map" (B,D,H,W), "timeline" (B,D)}``
        for every key whose head is a ``VQAHead`` — the head's score per feature token and its mean per depth slice — plus
        ``"regions"`` int32 (B, T) where the backbone keeps the window it cut for every frame (``KSVQE.last_regions``)."""
        scores, feats, dis_contra_loss, with_loss, maps = [], {}, None, False, {}
        for key in self.key_names:
            feat = getattr(self, key + "_backbone")(inputs, multi=self.multi, layer=self.layer, **kwargs)
            if key == "KSVQE":                                   # (features, distortion contrastive loss) (model.py:93-96)
                feat, dis_contra_loss = feat                     # loss is None when the backbone's aux_loss is off
                with_loss = True
            head = getattr(self, key + "_head")
            if return_maps and isinstance(head, VQAHead):
                score, token_map, timeline = head(feat, return_map=True)
                maps[key] = {"token_map": token_map, "timeline": timeline}
                regions = getattr(getattr(self, key + "_backbone"), "last_regions", None)      # read AFTER the forward that set it
                if regions is not None:
                    maps[key]["regions"] = regions
                scores += [score]
            else:
                scores += [head(feat)]
            if return_pooled_feats:
                feats[key] = feat
        if reduce_scores:
            scores = reduce(lambda a, b: a + b, scores) if len(scores) > 1 else scores[0]
        if return_pooled_feats:
            out = (scores, feats, dis_contra_loss) if with_loss else (scores, feats)
        elif with_loss:
            out = (scores, dis_contra_loss)
        else:
            out = scores
        return (out, maps) if return_maps else out
