"""Host-side mirror of the reference's ``models/backbones/conv_backbone.py`` ``ConvNeXt3D`` (:347-434; ``Block3D`` :153-188;
factories ``convnext_3d_tiny/small``): the "aesthetic" branch of the DOVER family, model key ``conv_tiny``.

Same constructor arguments, ``forward(batch, multi=False, layer=-1)`` and state_dict keys as the reference
(``downsample_layers.i.j.*``, ``stages.i.j.{dwconv,norm,pwconv1,pwconv2}.*``, ``stages.i.j.gamma``, ``norm.*``), so a DOVER or an
inflated 2D ConvNeXt checkpoint loads by name.  The modules only hold parameters; ``forward`` enqueues libkvq_hip.so launches on
an fp32 channels-last residual stream:

    stem                 kvq_patch_embed (2x4x4 conv + LayerNorm, eps 1e-6)
    block                kvq_dwconv3d_ln -> kvq_gemm_bf16(GELU) -> kvq_gemm_resid_scaled (pwconv2, gamma, residual add)
    downsample layer     kvq_layernorm_rows (16-bit rows) -> kvq_conv_implicit (1,2,2)/(1,2,2), fp32 store
    final norm           kvq_layernorm_rows (fp32)

— 62 launches for ConvNeXt-T.  There is no PyTorch compute path and nothing is ever downloaded.

``ConvNeXtV23D`` (:437-527; ``BlockV23D`` :221-250, ``GRN`` :7-18; model key ``conv_v2_tiny``) is the ConvNeXt-V2 trunk on the same
sequencing (``_ConvNeXtTrunk``): no layer scale, and Global Response Normalization between the GELU and pwconv2 —

    block                kvq_dwconv3d_ln -> kvq_gemm_bf16(GELU) -> kvq_grn_stats + kvq_grn_apply (in place) -> kvq_gemm_bf16(residual add)

— 116 launches for ConvNeXt-V2-T (the statistics are two launches, three with grn_over="thw": csrc/grn.hip).  The reference calls
its 2D GRN module on the (N, T, H, W, C) tensor, so the norm runs over T and H only, one per (sample, w column, channel): that is
``grn_over="th"``, the default; ``grn_over="thw"`` is the ConvNeXt-V2 paper's GRN carried to 3D.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from ... import _abi, _prepared, kernels
from ..._abi import check, current_stream, lib, ptr
from .swin_backbone import _Affine


class _Block3D(nn.Module):
    def __init__(self, dim, inflate_len=3, layer_scale_init_value=1e-6):
        super().__init__()
        if layer_scale_init_value > 0:
            self.gamma = nn.Parameter(layer_scale_init_value * torch.ones(dim))
        else:
            self.gamma = None
        self.dwconv = _Affine((dim, 1, inflate_len, 7, 7), (dim,))
        self.norm = _Affine((dim,), (dim,), ones=True)
        self.pwconv1 = _Affine((4 * dim, dim), (4 * dim,))
        self.pwconv2 = _Affine((dim, 4 * dim), (dim,))


class _GRN(nn.Module):
    """parameter holder of the reference's ``GRN`` (:7-18): gamma / beta (1, 1, 1, dim), zeros"""

    def __init__(self, dim):
        super().__init__()
        self.gamma = nn.Parameter(torch.zeros(1, 1, 1, dim))
        self.beta = nn.Parameter(torch.zeros(1, 1, 1, dim))


class _BlockV23D(nn.Module):
    def __init__(self, dim, inflate_len=3):
        super().__init__()
        self.dwconv = _Affine((dim, 1, inflate_len, 7, 7), (dim,))
        self.norm = _Affine((dim,), (dim,), ones=True)
        self.pwconv1 = _Affine((4 * dim, dim), (4 * dim,))
        self.grn = _GRN(4 * dim)
        self.pwconv2 = _Affine((dim, 4 * dim), (dim,))


class _ConvNeXtTrunk(nn.Module):
    """What ConvNeXt3D and ConvNeXtV23D share: the stem and downsample layers, the stage loop, ``multi`` and the final norm.  A subclass
    says what a block holds besides the depthwise conv, the norm and the two pointwise layers (``_block_extra``) and which launches
    follow the GELU GEMM (``_enqueue_block_tail``)."""

    def _init_trunk(self, in_chans, inflate_strategy, depths, dims, operand_dtype, make_block):
        self.in_chans, self.depths, self.dims = in_chans, tuple(depths), tuple(dims)
        self.inflate_strategy = str(inflate_strategy)
        self.operand_dtype = _prepared.default_operand_dtype(operand_dtype)
        self.downsample_layers = nn.ModuleList()
        self.downsample_layers.append(nn.Sequential(_Affine((dims[0], in_chans, 2, 4, 4), (dims[0],)),
                                                    _Affine((dims[0],), (dims[0],), ones=True)))
        for i in range(3):
            self.downsample_layers.append(nn.Sequential(_Affine((dims[i],), (dims[i],), ones=True),
                                                        _Affine((dims[i + 1], dims[i], 1, 2, 2), (dims[i + 1],))))
        self.stages = nn.ModuleList()
        for i in range(4):
            self.stages.append(nn.Sequential(*[
                make_block(dims[i], int(self.inflate_strategy[j % len(self.inflate_strategy)])) for j in range(depths[i])]))
        self.norm = _Affine((dims[-1],), (dims[-1],), ones=True)

    def _init_weights(self):
        with torch.no_grad():       # the reference's _init_weights (:408-411, :501-504): every Conv3d / Linear weight trunc_normal(0.02), biases 0
            for m in self.modules():
                if isinstance(m, _Affine) and m.weight.dim() > 1:
                    nn.init.trunc_normal_(m.weight, std=0.02)
        self._cache = _prepared.PreparedCache()

    # ------------------------------------------------------------------ weights
    def _inflate(self, s_state_dict):
        mine = self.state_dict()
        for key, cur in mine.items():
            if key not in s_state_dict:
                continue
            if cur.shape != s_state_dict[key].shape:
                t = cur.shape[2]
                s_state_dict[key] = s_state_dict[key].unsqueeze(2).repeat(1, 1, t, 1, 1) / t
        self.load_state_dict(s_state_dict, strict=False)

    def _weights(self, device):
        half = _abi.torch_dtype(self.operand_dtype)
        params = list(self.parameters())

        def build():
            f32 = lambda t: _prepared.to_f32(t, device)  # noqa: E731
            op = lambda t, shape=None: _prepared.to_operand(t, half, device, shape)  # noqa: E731
            stem_c, stem_n = self.downsample_layers[0]
            E, K = self.dims[0], self.in_chans * 2 * 4 * 4
            stem_w = op(stem_c.weight, (E, K))
            pack = torch.empty(lib().kvq_patch_embed_pack_bytes(E, K), dtype=torch.uint8, device=device)
            keep = [stem_w, f32(stem_c.bias), f32(stem_n.weight), f32(stem_n.bias)]
            check(lib().kvq_patch_embed_pack(ptr(stem_w), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), E, K, ptr(pack),
                                             current_stream()), "kvq_patch_embed_pack")
            down = [None]
            for i in range(1, 4):
                n, c = self.downsample_layers[i]
                # (N, C, 1, 2, 2) -> [N][(kh, kw, c)]: the column order kvq_conv_implicit walks
                w = op(c.weight.detach().to(device, torch.float32).permute(0, 2, 3, 4, 1), (c.weight.shape[0], -1))
                down.append((f32(n.weight), f32(n.bias), w, f32(c.bias)))
            stages = []
            for st in self.stages:
                blocks = []
                for b in st:
                    blocks.append(dict(
                        dw=kernels.dwconv_weight_taps(f32(b.dwconv.weight)), dw_b=f32(b.dwconv.bias),
                        ln_w=f32(b.norm.weight), ln_b=f32(b.norm.bias),
                        w1=op(b.pwconv1.weight), b1=f32(b.pwconv1.bias), w2=op(b.pwconv2.weight), b2=f32(b.pwconv2.bias),
                        **self._block_extra(b, f32)))
                stages.append(blocks)
            return dict(pack=pack, keep=keep, down=down, stages=stages, norm=(f32(self.norm.weight), f32(self.norm.bias)))
        return self._cache.get((self.operand_dtype, str(device)), params, build)

    # ------------------------------------------------------------------ forward
    def forward_features(self, x, multi=False, layer=-1):
        if layer > -1 and not multi:
            # conv_backbone.py:425-426 reads ``xs``, which only exists with multi=True: the reference raises UnboundLocalError here
            raise NotImplementedError(f"{type(self).__name__}.forward(layer > -1) without multi is an UnboundLocalError in the reference "
                                      "(conv_backbone.py:425-426 / :518-519 read xs, defined only for multi=True); there is nothing to mirror")
        if not x.is_cuda:
            raise _abi.KvqError(f"{type(self).__name__}.forward needs the clip on a HIP device; there is no CPU path")
        x = x.to(torch.float32).contiguous()
        B, Cin, T, H, W = x.shape
        E = self.dims[0]
        if Cin != self.in_chans or not lib().kvq_patch_embed_supported(Cin, 2, 4, 4, E, T, H, W):
            raise _abi.KvqError(f"{type(self).__name__}: the stem launch needs a (B, 3, T, H, W) clip with T % 2 == 0, H % 4 == 0, W % 4 == 0 "
                                f"and dims[0] in (96, 128); got {tuple(x.shape)}, dims[0] = {E}")
        w = self._weights(x.device)
        half = _abi.torch_dtype(self.operand_dtype)
        D, Hc, Wc = T // 2, H // 4, W // 4
        cur = torch.empty(B * D * Hc * Wc, E, dtype=torch.float32, device=x.device)
        a = _abi.KvqPatchEmbedArgs()
        a.x, a.B, a.in_chans, a.T, a.H, a.W, a.pd, a.ph, a.pw, a.embed_dim = ptr(x), B, Cin, T, H, W, 2, 4, 4, E
        a.pack, a.has_norm, a.out, a.eps, a.dtype = ptr(w["pack"]), 1, ptr(cur), 1e-6, self.operand_dtype
        check(lib().kvq_patch_embed(C.byref(a), _abi.stream_of(x)), "kvq_patch_embed")
        outs = []
        for i in range(4):
            Cc = self.dims[i]
            if i > 0:
                ln_w, ln_b, cw, cb = w["down"][i]
                rows = kernels.layernorm_rows(cur, ln_w, ln_b, out_dtype=half, eps=1e-6)
                cur = kernels.conv_implicit(rows.view(B, D, Hc, Wc, self.dims[i - 1]), cw, cb, (1, 2, 2), (1, 2, 2), (0, 0, 0),
                                            relu=False, store_f32=True)
                Hc, Wc = Hc // 2, Wc // 2
                if Hc < 1 or Wc < 1:
                    raise _abi.KvqError(f"{type(self).__name__}: a {H} x {W} clip has no stage-{i} plane")
            for b in w["stages"][i]:
                rows = kernels.dwconv3d_ln(cur.view(B, D, Hc, Wc, Cc), b["dw"], b["dw_b"], b["ln_w"], b["ln_b"], eps=1e-6,
                                           out_dtype=half)
                hid = kernels.gemm(rows, b["w1"], b["b1"], _abi.EPI_GELU_BF16)
                self._enqueue_block_tail(hid, b, cur, (B, D, Hc, Wc))
            outs.append(cur.view(B, D, Hc, Wc, Cc))
        if multi:
            # torch.cat([F.interpolate(f, size=last grid, mode="trilinear") for f in xs[:-1]], 1) (:422-424): no final norm here
            ctot = sum(self.dims[:3])
            out = torch.empty(B, D, Hc, Wc, ctot, dtype=torch.float32, device=x.device)
            off = 0
            for t in outs[:3]:
                check(lib().kvq_resize_trilinear_cl(ptr(t), B, t.shape[1], t.shape[2], t.shape[3], t.shape[4], ptr(out), D, Hc, Wc,
                                                    ctot, off, current_stream()), "kvq_resize_trilinear_cl")
                off += t.shape[4]
            return out.permute(0, 4, 1, 2, 3)
        feat = kernels.layernorm_rows(cur, *w["norm"], out_dtype=torch.float32, eps=1e-6)
        return feat.view(B, D, Hc, Wc, self.dims[-1]).permute(0, 4, 1, 2, 3)      # channels-last storage, the reference's (B,C,D,H,W) view


class ConvNeXt3D(_ConvNeXtTrunk):
    def __init__(self, in_chans=3, num_classes=1000, inflate_strategy="131", depths=(3, 3, 9, 3), dims=(96, 192, 384, 768),
                 drop_path_rate=0.0, layer_scale_init_value=1e-6, head_init_scale=1.0, operand_dtype=None):
        super().__init__()
        self._init_trunk(in_chans, inflate_strategy, depths, dims, operand_dtype,
                         lambda dim, kt: _Block3D(dim, kt, layer_scale_init_value))
        self._init_weights()

    def inflate_weights(self, s_state_dict):
        """Load a 2D ConvNeXt state dict (conv_backbone.py:396-406): a tensor whose shape differs from this model's becomes
        ``unsqueeze(2).repeat(1, 1, t, 1, 1) / t``; keys the source lacks keep their values (``strict=False``).  Host-side."""
        self._inflate(s_state_dict)

    def _block_extra(self, b, f32):
        return dict(gamma=None if b.gamma is None else f32(b.gamma))

    def _enqueue_block_tail(self, hid, b, cur, shape):
        kernels.gemm(hid, b["w2"], b["b2"], _abi.EPI_RESID_F32, out=cur, col_scale=b["gamma"])

    def forward(self, batch, multi=False, layer=-1, **kwargs):
        """``batch['asesthetic']`` (the reference's spelling, :432) if present, else ``batch['aesthetic']``: fp32 (B,3,T,H,W) on a
        HIP device -> (B, dims[-1], T/2, H/32, W/32); ``multi=True``: (B, dims[0]+dims[1]+dims[2], T/2, H/32, W/32)."""
        x = batch["asesthetic"] if "asesthetic" in batch else batch["aesthetic"]
        return self.forward_features(x, multi=multi, layer=layer)


def convnext_3d_tiny(pretrained=False, **kwargs):
    """``pretrained``: False, or the path of a LOCAL 2D ConvNeXt checkpoint (``torch.load(path)["model"]`` goes through
    ``inflate_weights``).  The reference downloads ImageNet weights for ``pretrained=True``; this project never does."""
    return _make((3, 3, 9, 3), pretrained, kwargs)


def convnext_3d_small(pretrained=False, **kwargs):
    return _make((3, 3, 27, 3), pretrained, kwargs)


def _make(depths, pretrained, kwargs):
    kwargs.pop("in_22k", None)
    if pretrained is True:
        raise NotImplementedError("convnext_3d: the reference downloads ImageNet weights for pretrained=True; pass the path of a "
                                  "local 2D ConvNeXt checkpoint or False")
    model = ConvNeXt3D(depths=depths, dims=(96, 192, 384, 768), **kwargs)
    if pretrained:
        model.inflate_weights(torch.load(pretrained, map_location="cpu")["model"])
    return model


class ConvNeXtV23D(_ConvNeXtTrunk):
    """The reference's ``ConvNeXtV23D`` (:437-527).  ``grn_over``: "th" — the reference: its 2D ``GRN`` reduces ``dim=(1, 2)`` of the
    (N, T, H, W, C) tensor, one norm per (sample, w column, channel) — or "thw", one norm per (sample, channel)."""

    def __init__(self, in_chans=3, num_classes=1000, inflate_strategy="131", depths=(3, 3, 9, 3), dims=(96, 192, 384, 768),
                 drop_path_rate=0.0, head_init_scale=1.0, operand_dtype=None, grn_over="th"):
        super().__init__()
        if grn_over not in ("th", "thw"):
            raise ValueError(f"ConvNeXtV23D: grn_over must be 'th' (the reference) or 'thw', got {grn_over!r}")
        self.grn_over = grn_over
        self._init_trunk(in_chans, inflate_strategy, depths, dims, operand_dtype, _BlockV23D)
        self.head = _Affine((num_classes, dims[-1]), (num_classes,))      # the reference's classifier: loaded by name, never run (:522-526)
        self._init_weights()
        with torch.no_grad():
            self.head.weight.mul_(head_init_scale)
            self.head.bias.mul_(head_init_scale)

    def inflate_weights(self, pretrained_path):
        """``torch.load(pretrained_path)["model"]`` (a LOCAL 2D ConvNeXt-V2 checkpoint) inflated as in the reference (:487-499)."""
        self._inflate(torch.load(pretrained_path, map_location="cpu")["model"])

    def _block_extra(self, b, f32):
        return dict(grn_g=f32(b.grn.gamma).reshape(-1), grn_b=f32(b.grn.beta).reshape(-1))

    def _enqueue_block_tail(self, hid, b, cur, shape):
        kernels.grn(hid, shape, b["grn_g"], b["grn_b"], over=self.grn_over)
        kernels.gemm(hid, b["w2"], b["b2"], _abi.EPI_RESID_F32, out=cur)

    def forward(self, batch, multi=False, layer=-1, **kwargs):
        """``batch['aesthetic']`` (:525): fp32 (B,3,T,H,W) on a HIP device -> (B, dims[-1], T/2, H/32, W/32); ``multi=True``:
        (B, dims[0]+dims[1]+dims[2], T/2, H/32, W/32)."""
        return self.forward_features(batch["aesthetic"], multi=multi, layer=layer)


def convnextv2_3d_tiny(pretrained=False, **kwargs):
    """The reference's 3D ``convnextv2_tiny`` (:623-625).  ``pretrained``: False, or the path of a LOCAL 2D ConvNeXt-V2 checkpoint
    (``inflate_weights``); nothing is downloaded."""
    if pretrained is True:
        raise NotImplementedError("convnextv2_3d_tiny: pretrained is False or the path of a local 2D ConvNeXt-V2 checkpoint")
    model = ConvNeXtV23D(depths=(3, 3, 9, 3), dims=(96, 192, 384, 768), **kwargs)
    if pretrained:
        model.inflate_weights(pretrained)
    return model


def _no_widths(name, dims):
    def factory(pretrained=False, **kwargs):
        raise NotImplementedError(f"{name}: dims {dims} need a stem and a depthwise-conv launch at widths libkvq_hip.so does not have "
                                  "(kvq_patch_embed: 96 / 128; kvq_dwconv3d_ln: 96 / 192 / 384 / 768; kvq_grn: four times those)")
    factory.__name__ = name
    return factory


convnextv2_3d_atto = _no_widths("convnextv2_3d_atto", (40, 80, 160, 320))
convnextv2_3d_femto = _no_widths("convnextv2_3d_femto", (48, 96, 192, 384))
convnextv2_3d_pico = _no_widths("convnextv2_3d_pico", (64, 128, 256, 512))
convnextv2_3d_nano = _no_widths("convnextv2_3d_nano", (80, 160, 320, 640))
convnextv2_3d_base = _no_widths("convnextv2_3d_base", (128, 256, 512, 1024))
convnextv2_3d_large = _no_widths("convnextv2_3d_large", (192, 384, 768, 1536))
