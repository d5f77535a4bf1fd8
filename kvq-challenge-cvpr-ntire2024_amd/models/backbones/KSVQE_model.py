"""Host-side mirror of the reference's ``KSVQE`` (``models/backbones/KSVQE_model.py:1024-1500``): the Swin-3D(GRPB) trunk with
the quality-aware region selection in front of it and the content / distortion modulation behind its last two stages.

Same constructor arguments, module tree and ``state_dict`` keys (trunk keys at the top level as in the reference; ``CLIP_tool.*``,
``distortion_tool.*``, ``dist_adapter.*``, ``semantic_adapter.k.*``, ``distortion_adapter.k.*``, ``semantic_mod.k.*``,
``distortion_mod.k.*``, ``semantic_cross.k.*``, ``distortion_cross.k.*``, ``distortion_self.k.*``, ``a1``, ``a2``), same forward:
``x`` = the dataset dict (``resize_video`` (b,3,t,112,112), ``fragment`` (b,3,t,288,288), ``dis_label``) ->
``(feature map (b, 768, t/2, 7, 7), distortion contrastive loss)``.

Everything on the score path runs on ``libkvq_hip.so``: CLIP_tool (clip_visual.py), QRS, the CONTRIQUE branch and the CDM
modules (ksvqe_modules.py), the trunk stage by stage (``SwinTransformer3D.forward_stages``).  The reference's constructor
downloads / loads CLIP and CONTRIQUE checkpoints from absolute paths (:1068-1074); here the sub-networks are created
randomly initialised and the checkpoints arrive through ``load_state_dict`` / ``Trainer.load_checkpoint``.  The contrastive
loss (:1666-1691, returned next to the features, unused by inference) is a few torch ops on a (b·t/2·49, 128) matrix."""
from __future__ import annotations

import torch
import torch.nn as nn

from ... import _abi, _prepared, kernels
from . import ksvqe_modules as KM
from .clip_visual import build_CLIPmodel_basedadapter_cls
from .swin_backbone import SwinTransformer3D


def _adapter(cin, hidden, cout):
    return nn.Sequential(nn.Linear(cin, hidden), nn.ReLU(inplace=True), nn.Linear(hidden, cout), nn.ReLU(inplace=True))


def distortion_contrastive_supervised(distortion_feature, dis_label):
    """Reference loss (:1666-1691): supervised contrastive over all (clip, frame, patch) tokens, positives = same distortion
    label (self excluded), temperature 0.1.  Auxiliary output; plain torch on the device."""
    b, t, g, _ = distortion_feature.shape
    f = distortion_feature.reshape(b * t * g, -1)
    same = (dis_label.unsqueeze(1).repeat(1, b) == dis_label).to(torch.float32).to(f.device)
    labels = same.repeat(1, t * g).view(b * t * g, -1)
    z = nn.functional.normalize(f, p=2, dim=1)
    sim = z @ z.t() / 0.1
    n = b * t * g
    off = 1.0 - torch.eye(n, device=f.device)
    pos = (labels @ labels.t()) * off
    return torch.mean(torch.log(torch.sum(torch.exp(sim) * off, dim=1)) - torch.sum(sim * pos, dim=1) / torch.sum(pos, dim=1))


class KSVQE(SwinTransformer3D):
    def __init__(self, pretrained=None, pretrained2d=False, num_samples=500, sample_type="topkpertubation", CLIP_location=10,
                 cls_use=True, tuning_stage=2, a1=1, a2=0, checkpoint=None, qls_swin=None, frozen3D=None, contrique_residual16=None, **trunk):
        trunk.setdefault("frag_biases", (True, True, True, False))
        super().__init__(pretrained=pretrained, pretrained2d=pretrained2d, **trunk)
        depths, heads, E = self.depths, self.heads, self.embed_dim
        self.N_key = 5                                   # reference attribute; four frames are actually used (:1357-1361)
        self.CLIP_tool = build_CLIPmodel_basedadapter_cls(CLIP_location=CLIP_location, cls_use=cls_use)
        self.distortion_tool = KM.CONTRIQUE_model(KM.get_network("resnet50"), 2048, residual16=contrique_residual16)
        self.dist_adapter = _adapter(128, 32, 128)
        self.spa_patchnet = KM.RegionNet_CLIP(k=7 * 7, anchor_size=32, stride=1, num_samples=num_samples, sample_type=sample_type)
        self.sigma_max = self.sigma = 0.5
        self.tuning_stage = tuning_stage
        self.aux_loss = True
        self.semantic_adapter, self.distortion_adapter = nn.ModuleList(), nn.ModuleList()
        self.semantic_mod, self.distortion_mod = nn.ModuleList(), nn.ModuleList()
        self.semantic_cross, self.distortion_cross, self.distortion_self = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        n_tuned = len(depths) - tuning_stage
        self.a1 = nn.Parameter(torch.zeros(n_tuned, 1) + a1)
        self.a2 = nn.Parameter(torch.zeros(n_tuned, 1) + a2)
        for i in range(tuning_stage, len(depths)):
            if i + 1 > len(depths) - 1:
                i = len(depths) - 2
            c = int(E * 2 ** (i + 1))
            self.semantic_adapter.append(_adapter(768, 768 // 4, c))
            self.distortion_adapter.append(_adapter(128, 128 // 4, c))
            self.semantic_mod.append(KM.Semantic_Transformation2(c))
            self.distortion_mod.append(KM.Dist_Transformation3(c))
            self.semantic_cross.append(KM.crossattention1(c, heads[i]))
            self.distortion_cross.append(KM.crossattention1(c, heads[i]))
            self.distortion_self.append(KM.Attention(c, heads[i]))
        self._acache, self._mixc = _prepared.PreparedCache(), _prepared.PreparedCache()

    # ------------------------------------------------------------------ adapters: Linear -> ReLU -> Linear -> ReLU = two GEMMs
    def _adapters(self, device):
        half = _abi.torch_dtype(self.operand_dtype)
        mods = [self.dist_adapter] + list(self.semantic_adapter) + list(self.distortion_adapter)
        f = lambda m: (_prepared.to_operand(m.weight, half, device), _prepared.to_f32(m.bias, device))  # noqa: E731
        return self._acache.get((self.operand_dtype, str(device)), [p for m in mods for p in m.parameters()],
                                lambda: {id(m): (f(m[0]), f(m[2])) for m in mods})

    def _mix_coeffs(self):
        """(a1, a2) of every tuned stage as host floats, re-read only when the parameters change (no device sync per forward)."""
        return self._mixc.get((), (self.a1, self.a2), lambda: list(zip(self.a1.detach().cpu().reshape(-1).tolist(),
                                                                      self.a2.detach().cpu().reshape(-1).tolist())))

    def _run_adapter(self, mod, rows16):
        (w0, b0), (w2, b2) = self._adapters(rows16.device)[id(mod)]
        return kernels.conv_gemm(kernels.conv_gemm(rows16, w0, b0, True), w2, b2, True)

    def _sync_dtype(self):
        mods = [self.CLIP_tool, self.distortion_tool] + list(self.semantic_mod) + list(self.distortion_mod)
        for m in mods + list(self.semantic_cross) + list(self.distortion_cross) + list(self.distortion_self):
            m.operand_dtype = self.operand_dtype

    @property
    def last_regions(self):
        """int32 (B, T) on the device: the QRS window index of every frame of the last forward (``kvq_qrs_top_region``'s index of the
        frame's key-frame group), or None before the first one.  Overwritten by each forward; reading it synchronises nothing.  What
        ``kernels.quality_paint_regions`` takes to paint the head's token map back onto the source frames."""
        return self.spa_patchnet.last_regions

    # ------------------------------------------------------------------ forward
    def forward(self, x, multi=False, layer=-1, adaptive_window_size=False, **kwargs):
        if adaptive_window_size:
            # the reference's own branch reads ``x.shape`` of the input DICT (KSVQE_model.py:1394-1397) and raises AttributeError
            raise AttributeError("'dict' object has no attribute 'shape'")
        want_taps = bool(multi) or layer > -1
        if layer > self.num_layers:
            raise IndexError("list index out of range")              # feats[layer] in the reference (:1497)
        revideo, fragment, dis_label = x["resize_video"], x["fragment"], x["dis_label"]
        if not fragment.is_cuda:
            raise _abi.KvqError("KSVQE.forward needs its inputs on a HIP device; there is no CPU path")
        self._sync_dtype()
        half = _abi.torch_dtype(self.operand_dtype)
        dev = fragment.device
        revideo, fragment = revideo.to(dev, torch.float32), fragment.to(torch.float32).contiguous()
        if not torch.is_tensor(dis_label):
            dis_label = torch.as_tensor(dis_label)
        dis_label = dis_label.reshape(-1).to(dev)
        b, _, t = fragment.shape[:3]
        # key frames -> CLIP: the CLS-to-patch map ranks the regions, the patch tokens feed the semantic modulation
        group_id, key = KM.obtain_keyframes(revideo)
        n_key = key.shape[1]
        cls_attn, _, pat = self.CLIP_tool(key.reshape((b * n_key,) + tuple(key.shape[2:])).contiguous())
        grid = pat.shape[2]
        patch_tokens = KM.extend_by_group(pat.reshape(b, n_key, grid * pat.shape[3]), group_id).reshape(b, t, grid, -1)
        # QRS: one 224x224 window of the 288x288 fragment canvas per key frame
        x_sel_ori = self.spa_patchnet(fragment, cls_attn.reshape(b, n_key, -1), self.sigma, group_id)
        # distortion tokens of every other frame
        dist = self.distortion_tool(x_sel_ori[:, :, ::2].contiguous())                       # (b, t/2, 49, 128) fp32
        d16 = kernels.to_half(dist.reshape(-1, dist.shape[-1]).contiguous(), half)
        dist = kernels.axpby(kernels.to_float(self._run_adapter(self.dist_adapter, d16)).reshape(dist.shape), dist, 0.2, 0.8)
        # the auxiliary loss (second return value): the inference loop discards it (trainer.py:323-327), so the harness
        # switches it off (``aux_loss = False`` -> None is returned in its place); on by default, like the reference
        loss = distortion_contrastive_supervised(dist, dis_label) if self.aux_loss else None
        geom = tuple(x_sel_ori.shape[2:])
        n_st = self.num_layers
        feats = {}                                                   # the reference's ``feats`` list (:1430, :1484), filled on request
        if self.tuning_stage > 0:
            hi = min(self.tuning_stage, n_st) - 1
            if want_taps:
                x_sel, feats = self.forward_stages(x_sel_ori, 0, hi, taps=range(hi + 2))
            else:
                x_sel = self.forward_stages(x_sel_ori, 0, hi)
        else:
            x_sel = x_sel_ori
        for l in range(self.tuning_stage, n_st):
            if want_taps and l == 0:
                x_sel, feats = self.forward_stages(x_sel_ori, 0, 0, geometry=geom, taps=(0,))
            else:
                x_sel = self.forward_stages(x_sel if l > 0 else x_sel_ori, l, l, geometry=geom)
            x_sel = self._modulate(l - self.tuning_stage, x_sel, patch_tokens, dist, half)
            feats[l + 1] = x_sel                                     # a tuned stage's entry is the MODULATED stream (:1482-1484)
        n, c, d, hh, ww = x_sel.shape
        rows = x_sel.permute(0, 2, 3, 4, 1).reshape(-1, c).contiguous()
        feat = kernels.layernorm_rows(rows, self.norm.weight.detach().to(dev, torch.float32), self.norm.bias.detach().to(dev, torch.float32),
                                      out_dtype=torch.float32)
        if multi:
            # torch.cat([F.interpolate(xi, size=final (d, h, w), mode="trilinear") for xi in feats[:-1]], 1) (:1489-1495)
            srcs = [feats[i].permute(0, 2, 3, 4, 1).contiguous() for i in range(n_st)]
            ctot = sum(t.shape[-1] for t in srcs)
            out = torch.empty(n, d, hh, ww, ctot, dtype=torch.float32, device=dev)
            off = 0
            for t in srcs:
                _abi.check(_abi.lib().kvq_resize_trilinear_cl(_abi.ptr(t), n, t.shape[1], t.shape[2], t.shape[3], t.shape[4], _abi.ptr(out),
                                                             d, hh, ww, ctot, off, _abi.current_stream()), "kvq_resize_trilinear_cl")
                off += t.shape[4]
            return out.permute(0, 4, 1, 2, 3)
        if layer > -1:
            return feats[layer]                                      # :1496-1498
        return feat.reshape(n, d, hh, ww, c).permute(0, 4, 1, 2, 3), loss

    def _modulate(self, k, x_sel, patch_tokens, dist, half):
        """CDM behind a tuned stage (:1436-1482): x_sel (n, c, t', h, w) -> (a1 * distortion-modulated + a2 * semantic-modulated) / 2."""
        n, c, tt, hh, ww = x_sel.shape
        hw = hh * ww
        rows = x_sel.permute(0, 2, 3, 4, 1).reshape(n * tt * hw, c).contiguous()            # token rows, frame-major (layout only)
        frames16 = kernels.to_half(rows, half).reshape(n * tt, hw, c)       # one 16-bit copy of the frame tokens for both cross attentions
        # --- semantic: CLIP patch tokens of every other frame, adapted to c channels, cross-attended by the frame's tokens
        pt = patch_tokens[:, ::2].reshape(-1, patch_tokens.shape[-1]).contiguous()
        pt = self._run_adapter(self.semantic_adapter[k], kernels.to_half(pt, half)).reshape(n * tt, -1, c)
        enhanced, _ = self.semantic_cross[k](frames16, pt)
        x_s = kernels.sem_modulate(enhanced.reshape(-1, c).contiguous(), rows, *self.semantic_mod[k]._weights(rows.device))   # (n t' hw, c)
        # --- distortion: CONTRIQUE tokens adapted to c channels, cross-attended per frame, then self-attention over the
        # frames of every spatial position, then (mean, std)-driven channel modulation.  The chain stays in the 16-bit operand
        # type between its GEMMs (the values each next GEMM would round to anyway)
        dt = self._run_adapter(self.distortion_adapter[k], kernels.to_half(dist.reshape(-1, dist.shape[-1]).contiguous(), half))
        d_enh, _ = self.distortion_cross[k](frames16, dt.reshape(n * tt, -1, c), keep16=True)
        d_enh = d_enh.reshape(n, tt, hw, c).permute(0, 2, 1, 3).reshape(n * hw, tt, c).contiguous()
        d_enh = self.distortion_self[k](d_enh, keep16=True)                                   # (n hw, t', c) 16-bit
        x_d = self.distortion_mod[k](d_enh.reshape(n, hw * tt, c), rows.reshape(n, tt * hw, c))   # (n, t' hw, c)
        a1, a2 = self._mix_coeffs()[k]
        out = kernels.axpby(x_d.reshape(-1, c).contiguous(), x_s, a1 / 2.0, a2 / 2.0)
        return out.reshape(n, tt, hh, ww, c).permute(0, 4, 1, 2, 3)
