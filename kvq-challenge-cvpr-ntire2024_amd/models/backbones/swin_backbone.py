"""Host-side mirror of the reference's ``models/backbones/swin_backbone.py`` trunk API.

Same class/constructor/forward/state_dict surface as the reference's ``SwinTransformer3D``
(``swin_backbone.py:736-1085``; factories ``swin_3d_tiny/small`` ``:1088-1095``), but the
modules only *hold parameters*: ``forward`` hands raw device pointers to
``kvq_swin3d_forward`` in libkvq_hip.so.  There is no PyTorch compute path.

state_dict keys are the reference's, including the
``attn.relative_position_index`` buffers, so reference checkpoints load with
``load_state_dict`` unchanged.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from ... import _abi, _prepared, kernels
from ..._abi import KvqSwinBlockW, KvqSwinCfg, KvqSwinWeights, check, current_stream, lib, ptr


def _rel_pos_index(window) -> torch.Tensor:
    """The registered buffer of WindowAttention3D (swin_backbone.py:213-235); kept only for
    state_dict compatibility — the kernels derive it from per-token position codes."""
    Wd, Wh, Ww = window
    n = torch.arange(Wd * Wh * Ww)
    c = torch.stack([n // (Wh * Ww), (n // Ww) % Wh, n % Ww])
    d = c[:, :, None] - c[:, None, :]
    return ((d[0] + Wd - 1) * (2 * Wh - 1) * (2 * Ww - 1) + (d[1] + Wh - 1) * (2 * Ww - 1) + d[2] + Ww - 1)


# test hook: False -> a FragmentSource batch is materialised (kvq_fragment_gather per clip) before the forward instead of
# being read through the sampler by the embedding launch; the two sequencings are bit-identical (tests/test_gpu_e2e.py)
FUSE_SAMPLER = True
# test hook: False -> PatchMerging runs as gather-LayerNorm + GEMM (+ the next block's LayerNorm launch) at every width
FUSE_MERGE = os.environ.get("KVQ_FUSE_MERGE", "1") != "0"


class _Affine(nn.Module):
    """weight(+bias) holder standing in for nn.Linear / nn.LayerNorm / nn.Conv3d."""

    def __init__(self, wshape, bshape=None, ones=False):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(wshape) if ones else torch.zeros(wshape))
        if bshape is not None:
            self.bias = nn.Parameter(torch.zeros(bshape))
        else:
            self.register_parameter("bias", None)


class _Attn(nn.Module):
    def __init__(self, dim, window, num_heads, frag_bias, qkv_bias=True):
        super().__init__()
        tl = (2 * window[0] - 1) * (2 * window[1] - 1) * (2 * window[2] - 1)
        self.relative_position_bias_table = nn.Parameter(torch.zeros(tl, num_heads))
        if frag_bias:
            self.fragment_position_bias_table = nn.Parameter(torch.zeros(tl, num_heads))
        self.register_buffer("relative_position_index", _rel_pos_index(window))
        self.qkv = _Affine((3 * dim, dim), (3 * dim,) if qkv_bias else None)
        self.proj = _Affine((dim, dim), (dim,))


class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = _Affine((hidden, dim), (hidden,))
        self.fc2 = _Affine((dim, hidden), (dim,))


class _Block(nn.Module):
    def __init__(self, dim, window, num_heads, mlp_ratio, frag_bias, qkv_bias=True):
        super().__init__()
        self.norm1 = _Affine((dim,), (dim,), ones=True)
        self.attn = _Attn(dim, window, num_heads, frag_bias, qkv_bias)
        self.norm2 = _Affine((dim,), (dim,), ones=True)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))


class _Merge(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.reduction = _Affine((2 * dim, 4 * dim))
        self.norm = _Affine((4 * dim,), (4 * dim,), ones=True)


class _Layer(nn.Module):
    def __init__(self, dim, depth, window, num_heads, mlp_ratio, frag_bias, downsample, qkv_bias=True):
        super().__init__()
        self.blocks = nn.ModuleList([_Block(dim, window, num_heads, mlp_ratio, frag_bias, qkv_bias)
                                     for _ in range(depth)])
        self.downsample = _Merge(dim) if downsample else None


class _PatchEmbed(nn.Module):
    def __init__(self, patch, in_chans, embed_dim, norm):
        super().__init__()
        self.proj = _Affine((embed_dim, in_chans) + tuple(patch), (embed_dim,))
        self.norm = _Affine((embed_dim,), (embed_dim,), ones=True) if norm else None


class SwinTransformer3D(nn.Module):
    """Drop-in for the reference class of the same name (inference forward only).

    Constructor kwargs follow ``swin_backbone.py:760-783``.  ``pretrained`` accepts a path to a
    checkpoint in the reference's ``load_swin`` format (``:933-1006``) or None; the reference's
    import-time/default path side effect is NOT reproduced: a missing file is an
    error only if a path is given explicitly.
    """

    def __init__(self, pretrained=None, pretrained2d=False, patch_size=(2, 4, 4), in_chans=3, embed_dim=96,
                 depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), window_size=(8, 7, 7), mlp_ratio=4.0,
                 qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1,
                 norm_layer=nn.LayerNorm, patch_norm=True, frozen_stages=-1, use_checkpoint=True,
                 jump_attention=(False, False, False, False), frag_biases=(True, True, True, False),
                 base_x_size=(32, 224, 224), operand_dtype=None):
        super().__init__()
        # 16-bit MFMA operand type (extension over the reference signature): "fp16" (default; holds the
        # 1e-3 MOS parity gate) or "bf16".  The environment sets the default, the argument overrides it (_prepared.default_operand_dtype).
        self.operand_dtype = _prepared.default_operand_dtype(operand_dtype)
        # packed weight images of the fused launches (patch embedding, proj+norm2+Mlp tail, the next block's q|k|v, PatchMerging) wherever
        # the library has a kernel for the width.  False: none, so the plan runs the unfused launches and a FragmentSource is materialised
        self.fused_tail = True          # (tests compare the two)
        # attention bias pre-built per (window, head) for each plan geometry (csrc/attn.hip, dense variant): ~1.2 GB of
        # HBM for Swin-T at 32x224x224; KVQ_DENSE_BIAS=0 (or a geometry above the cap) keeps the per-score gather path
        self.dense_bias = os.environ.get("KVQ_DENSE_BIAS", "1") != "0"
        self.dense_bias_max_bytes = 24 * 2 ** 30
        self.dense_bias_max_abs = 16.0
        self.dense_bias_bytes_per_clip = 2 * 2 ** 30
        self._dense = {}
        # residual stream x in fp16 where every producer and consumer of a stage takes fp16 rows; False: fp32 rows in
        # every stage — the exact re-score of an input whose fp16 stream left the +-65504 range (range_flags below)
        self.residual16 = True
        self._range_words: Dict[Tuple, torch.Tensor] = {}
        if isinstance(window_size, list) and window_size and isinstance(window_size[0], (list, tuple)):
            raise NotImplementedError("per-stage window sizes are not used by any reference config")
        if qk_scale is not None or any(jump_attention) or not qkv_bias:
            raise NotImplementedError("qk_scale / jump_attention / qkv_bias=False are not on the hot path")
        if int(mlp_ratio) != mlp_ratio:
            raise NotImplementedError("non-integer mlp_ratio")
        self.pretrained, self.pretrained2d = pretrained, pretrained2d
        self.num_layers = len(depths)
        self.embed_dim, self.patch_norm, self.frozen_stages = embed_dim, patch_norm, frozen_stages
        self.window_size, self.patch_size, self.base_x_size = tuple(window_size), tuple(patch_size), base_x_size
        self.depths, self.heads = tuple(depths), tuple(num_heads)
        self.mlp_ratio, self.in_chans = int(mlp_ratio), in_chans
        self.frag_biases = tuple(bool(f) for f in frag_biases)
        self.patch_embed = _PatchEmbed(self.patch_size, in_chans, embed_dim, patch_norm)
        self.layers = nn.ModuleList([
            _Layer(int(embed_dim * 2 ** i), depths[i], self.window_size, num_heads[i], mlp_ratio,
                   self.frag_biases[i], downsample=i < self.num_layers - 1) for i in range(self.num_layers)])
        self.num_features = int(embed_dim * 2 ** (self.num_layers - 1))
        self.norm = _Affine((self.num_features,), (self.num_features,), ones=True)
        self._plans: Dict[Tuple, Tuple] = {}
        self._wcache = None
        self.init_weights()

    # ------------------------------------------------------------------ weights
    def init_weights(self, pretrained=None):
        """trunc_normal(0.02) Linear weights, zero biases, unit LayerNorm, trunc_normal tables
        (swin_backbone.py:1017-1024, :242); then optionally ``load_swin``."""
        if pretrained:
            self.pretrained = pretrained
        with torch.no_grad():
            for name, p in self.named_parameters():
                leaf = name.rsplit(".", 1)[-1]
                if "relative_position_bias_table" in name:
                    nn.init.trunc_normal_(p, std=0.02)
                elif "fragment_position_bias_table" in name:
                    p.zero_()
                elif "norm" in name:
                    p.fill_(1.0) if leaf == "weight" else p.zero_()
                elif name.startswith("patch_embed.proj"):
                    # nn.Conv3d default init is kaiming-uniform in the reference; any finite init will do
                    nn.init.trunc_normal_(p, std=0.02) if leaf == "weight" else p.zero_()
                elif leaf == "weight":
                    nn.init.trunc_normal_(p, std=0.02)
                else:
                    p.zero_()
        if isinstance(self.pretrained, str):
            if self.pretrained2d:
                self.inflate_weights()
            else:
                self.load_swin(self.pretrained)
        elif self.pretrained is not None:
            raise TypeError("pretrained must be a str or None")

    def inflate_weights(self):
        """Reference ``inflate_weights`` (swin_backbone.py:858-931): load a 2D Swin checkpoint (``{"model": ...}``)
        into the 3D trunk.  ``relative_position_index`` / ``attn_mask`` entries are dropped (always re-derived);
        the patch-embed conv is repeated along the new temporal axis and divided by its depth (so a clip of
        identical frames embeds like the image did); every (L1, nH) bias table is bicubically resized to the
        (2·ws_h−1)·(2·ws_w−1) in-plane offsets when the 2D window differs, then tiled over the 2·ws_d−1 temporal
        offsets.  Tables whose head count differs are reported and still tiled as they are — load_state_dict then
        rejects them, as in the reference.  Host-side, once per load: plain torch CPU ops."""
        state = dict(torch.load(self.pretrained, map_location="cpu")["model"])
        for k in [k for k in state if "relative_position_index" in k or "attn_mask" in k]:
            del state[k]
        pt = self.patch_size[0]
        state["patch_embed.proj.weight"] = state["patch_embed.proj.weight"].unsqueeze(2).repeat(1, 1, pt, 1, 1) / pt
        own = self.state_dict()
        wd, sh, sw = self.window_size[0], 2 * self.window_size[1] - 1, 2 * self.window_size[2] - 1
        for k in [k for k in state if "relative_position_bias_table" in k]:
            tab = state[k]
            (l1, nh1), nh2 = tab.shape, own[k].shape[1]
            if nh1 != nh2:
                print(f"Error in loading {k}, passing")
            elif l1 != sh * sw:
                s1 = int(l1 ** 0.5)
                tab = torch.nn.functional.interpolate(tab.permute(1, 0).reshape(1, nh1, s1, s1), size=(sh, sw),
                                                      mode="bicubic").reshape(nh2, sh * sw).permute(1, 0)
            state[k] = tab.repeat(2 * wd - 1, 1)
        msg = self.load_state_dict(state, strict=False)
        print(msg)
        print(f"=> loaded successfully '{self.pretrained}'")
        return msg

    def load_swin(self, load_path, strict=False):
        """Reference ``load_swin`` (swin_backbone.py:933-1006): strip the 9-char ``backbone.`` prefix,
        fork every relative_position_bias_table into fragment_position_bias_table, drop
        shape-mismatched keys."""
        state = torch.load(load_path, map_location="cpu")["state_dict"]
        clean = {}
        for k, v in state.items():
            if "backbone" in k:
                ck = k[9:]
                clean[ck] = v
                if "relative_position_bias_table" in ck:
                    clean.setdefault(ck.replace("relative_position_bias_table", "fragment_position_bias_table"), v)
        own = self.state_dict()
        clean = {k: v for k, v in clean.items() if k not in own or own[k].shape == v.shape}
        return self.load_state_dict(clean, strict=strict)

    def cfg_struct(self, aw=None) -> KvqSwinCfg:
        c = KvqSwinCfg()
        c.patch[:] = self.patch_size
        c.in_chans, c.embed_dim, c.num_stages = self.in_chans, self.embed_dim, self.num_layers
        for i in range(self.num_layers):
            c.depths[i], c.num_heads[i], c.frag_bias[i] = self.depths[i], self.heads[i], int(self.frag_biases[i])
        c.window[:] = self.window_size
        c.mlp_ratio = self.mlp_ratio
        c.adaptive_window[:] = aw if aw else (0, 0, 0)
        return c

    def _weights(self, device) -> KvqSwinWeights:
        """bf16 copies of the GEMM weights + a KvqSwinWeights of raw pointers; rebuilt whenever a
        parameter was modified in place or moved (tracked through tensor versions / data_ptr)."""
        sig = _prepared.signature((self.operand_dtype, str(device), self.fused_tail, FUSE_MERGE), self.parameters())
        if self._wcache is not None and self._wcache[0] == sig:
            return self._wcache[1]
        keep = []
        half = _abi.torch_dtype(self.operand_dtype)

        def f32(p):
            keep.append(_prepared.to_f32(p, device))
            return ptr(keep[-1])

        def bf16(p, shape=None):       # GEMM weight in the 16-bit operand type
            keep.append(_prepared.to_operand(p, half, device, shape))
            return ptr(keep[-1])

        def image(nbytes, entry, *args):
            """The ``nbytes`` weight image that the library's ``entry`` writes from ``args``: kept alive with the weights, returned as a pointer."""
            keep.append(torch.empty(nbytes, dtype=torch.uint8, device=device))
            check(getattr(lib(), entry)(*args, ptr(keep[-1]), current_stream()), entry)
            return ptr(keep[-1])

        w = KvqSwinWeights()
        pe = self.patch_embed
        w.embed_w = bf16(pe.proj.weight, (self.embed_dim, -1))
        w.embed_b = f32(pe.proj.bias)
        if pe.norm is not None:
            w.embed_ln_w, w.embed_ln_b = f32(pe.norm.weight), f32(pe.norm.bias)
        K0 = pe.proj.weight[0].numel()
        nbytes = lib().kvq_patch_embed_pack_bytes(self.embed_dim, K0) if self.fused_tail else 0
        if nbytes:          # im2col + GEMM + LayerNorm (+ the first norm1) as one launch (csrc/embed.hip)
            w.embed_pack = image(nbytes, "kvq_patch_embed_pack", w.embed_w, w.embed_b, w.embed_ln_w, w.embed_ln_b, self.embed_dim, K0)
        nblk = sum(self.depths)
        blocks = (KvqSwinBlockW * nblk)()
        k = 0
        for i, layer in enumerate(self.layers):
            for blk in layer.blocks:
                b = blocks[k]
                k += 1
                b.norm1_w, b.norm1_b = f32(blk.norm1.weight), f32(blk.norm1.bias)
                b.rpb_table = f32(blk.attn.relative_position_bias_table)
                r = blk.attn.relative_position_bias_table.detach().to(device=device, dtype=torch.float32)
                if hasattr(blk.attn, "fragment_position_bias_table"):
                    b.fpb_table = f32(blk.attn.fragment_position_bias_table)
                    fr = blk.attn.fragment_position_bias_table.detach().to(device=device, dtype=torch.float32)
                    pack = torch.stack([fr, r - fr], -1)
                else:
                    pack = torch.stack([r, torch.zeros_like(r)], -1)
                pack = pack.permute(1, 0, 2)                     # [nH][table_len][2]
                if pack.shape[1] & 1:                            # even entry count -> 16-B aligned head rows
                    pack = torch.nn.functional.pad(pack, (0, 0, 0, 1))
                pack = pack.contiguous()
                keep.append(pack)
                b.bias_pack = ptr(pack)
                b.qkv_w, b.qkv_b = bf16(blk.attn.qkv.weight), f32(blk.attn.qkv.bias)
                b.proj_w, b.proj_b = bf16(blk.attn.proj.weight), f32(blk.attn.proj.bias)
                b.norm2_w, b.norm2_b = f32(blk.norm2.weight), f32(blk.norm2.bias)
                b.fc1_w, b.fc1_b = bf16(blk.mlp.fc1.weight), f32(blk.mlp.fc1.bias)
                b.fc2_w, b.fc2_b = bf16(blk.mlp.fc2.weight), f32(blk.mlp.fc2.bias)
                Cb, hid = blk.mlp.fc1.weight.shape[1], blk.mlp.fc1.weight.shape[0]
                nbytes = lib().kvq_block_tail_pack_bytes(Cb, hid) if self.fused_tail else 0
                if nbytes:      # fused proj+norm2+Mlp launch for this width (csrc/tail.hip)
                    b.tail_pack = image(nbytes, "kvq_block_tail_pack", b.proj_w, b.proj_b, b.norm2_w, b.norm2_b, b.fc1_w, b.fc1_b, b.fc2_w,
                                        b.fc2_b, Cb, hid)
                nbytes = lib().kvq_block_tail_qkv_pack_bytes(Cb, hid) if self.fused_tail else 0
                if nbytes:      # this block's qkv weight as the image the PREVIOUS block's tail streams to emit q | k | v (csrc/tailmm.hip)
                    b.qkv_pack = image(nbytes, "kvq_block_tail_qkv_pack", b.qkv_w, Cb, hid)
            if layer.downsample is not None:
                m = w.merges[i]
                m.norm_w, m.norm_b = f32(layer.downsample.norm.weight), f32(layer.downsample.norm.bias)
                m.red_w = bf16(layer.downsample.reduction.weight)
                Cm = layer.downsample.reduction.weight.shape[1] // 4
                nbytes = lib().kvq_patch_merge_pack_bytes(Cm) if self.fused_tail and FUSE_MERGE else 0
                if nbytes:      # concat + LayerNorm + reduction (+ the next norm1) as one launch for this width (csrc/merge.hip)
                    m.merge_pack = image(nbytes, "kvq_patch_merge_pack", f32(layer.downsample.reduction.weight), m.norm_w, m.norm_b, Cm,
                                         self.operand_dtype)
        w.blocks = C.cast(blocks, C.POINTER(KvqSwinBlockW))
        w.norm_w, w.norm_b = f32(self.norm.weight), f32(self.norm.bias)
        keep.append(blocks)
        self._wcache = (sig, w, keep, blocks)
        self._dense = {}                     # built from the old tables
        torch.cuda.synchronize(device)       # the packs were built on THIS stream; other streams may run the forward
        return w

    def _set_dense_bias(self, handle, geom, device, batch, aw=None):
        """Point every block at the dense attention bias of this plan geometry (built on first use).  The bias is read
        from HBM once per step whatever the batch, so it pays when enough windows share an image (one image per window TYPE and
        head): Swin-T at 32x224x224 pays at any batch, Swin-B at 64x256x256 (3.2 GB of images) pays from one clip on with the
        present kernel (5.76 -> 5.28 ms per clip at B = 1, 4.85 -> 4.29 at B = 2); the cap (2 GB per 32x224x224-equivalent of
        tokens in the batch) only fends off geometries whose images would dwarf the activations."""
        blocks = self._wcache[3]
        nblk = sum(self.depths)
        total = sum(lib().kvq_swin3d_bias_dense_bytes(handle, k) for k in range(nblk))
        # "clips" in units of the 32 x 224 x 224 clip the cap was measured on: a 96-frame KSVQE sample has three times the
        # windows per bias image (measured at T = 96, B = 1: 790 -> 480 us of attention per forward with the dense path)
        clips = batch * max(1.0, geom[0] / 32.0) * max(1.0, geom[1] * geom[2] / (224.0 * 224.0))
        if not self.dense_bias or total > clips * self.dense_bias_bytes_per_clip:
            for k in range(nblk):
                blocks[k].bias_dense = None
            return
        key = geom + (str(device), self.operand_dtype, aw)
        bufs = self._dense.get(key)
        if bufs is None:
            sizes = [lib().kvq_swin3d_bias_dense_bytes(handle, k) for k in range(nblk)]
            bufs, used = [], 0
            big = torch.zeros(nblk, dtype=torch.float32, device=device)
            for k in range(nblk):           # blocks that do not fit under the cap keep the per-score gather path
                if not sizes[k] or used + sizes[k] > self.dense_bias_max_bytes:
                    bufs.append(None)
                    continue
                t = torch.empty(sizes[k], dtype=torch.uint8, device=device)
                check(lib().kvq_swin3d_bias_dense_build(handle, k, blocks[k].rpb_table, blocks[k].fpb_table, ptr(t),
                                                        big[k:].data_ptr(), current_stream()), "kvq_swin3d_bias_dense_build")
                bufs.append(t)
                used += sizes[k]
            # the image is fp16, row-max shifted (error <= 2^-11 x distance below the row's largest bias): blocks whose
            # biases reach past +-16 keep the exact per-score gather path
            too_big = (big > self.dense_bias_max_abs).cpu().tolist()     # (also the synchronisation with the builders)
            bufs = [None if tb else b for b, tb in zip(bufs, too_big)]
            self._dense[key] = bufs
        for k in range(nblk):
            blocks[k].bias_dense = ptr(bufs[k])

    def _plan(self, B, T, H, W, device, aw=None):
        # one plan + workspace per (shape, stream): forwards issued on different streams may overlap
        key = (B, T, H, W, str(device), self.operand_dtype, current_stream(), aw, bool(self.residual16))
        hit = self._plans.get(key)
        if hit is not None:
            return hit
        handle = C.c_void_p()
        cfg = self.cfg_struct(aw)
        check(lib().kvq_swin3d_plan_create(C.byref(cfg), B, T, H, W, self.operand_dtype, C.byref(handle)),
              "kvq_swin3d_plan_create")
        if not self.residual16:
            check(lib().kvq_swin3d_plan_set_resid16(handle, 0), "kvq_swin3d_plan_set_resid16")
        check(lib().kvq_swin3d_set_range_flags(handle, ptr(self._range_word(torch.cuda.current_stream(torch.device(device))))),
              "kvq_swin3d_set_range_flags")
        dims = (C.c_int32 * 4)()
        check(lib().kvq_swin3d_out_dims(handle, C.byref(dims)), "kvq_swin3d_out_dims")
        nbytes = lib().kvq_swin3d_workspace_bytes(handle)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        entry = (handle, tuple(dims), ws)
        self._plans[key] = entry
        return entry

    # ------------------------------------------------------------------ range of the fp16 residual stream
    def _range_word(self, stream) -> torch.Tensor:
        """The int32 device word of ``stream`` that every plan of this module ORs its stage bits into (created zeroed on first use,
        before any forward of that stream is captured into a graph)."""
        key = (str(stream.device), stream.cuda_stream)
        word = self._range_words.get(key)
        if word is None:
            word = torch.zeros(1, dtype=torch.int32, device=stream.device)
            self._range_words[key] = word
        return word

    def range_flags(self, stream=None) -> torch.Tensor:
        """The range word of ``stream`` (default: the current stream) as a 1-element int32 device tensor, without synchronising.
        Bit i set: stage i's fp16 residual stream held a value that reached +-65504 (clamped there, or inf / NaN) in a forward on
        that stream since the last ``clear_range_flags``, so that forward's output is not exact; re-run it with
        ``residual16 = False``.  Sticky: only ``clear_range_flags`` zeroes it."""
        return self._range_word(stream if stream is not None else torch.cuda.current_stream())

    def clear_range_flags(self, stream=None) -> None:
        """Zero the range word of ``stream`` (default: the current stream), enqueued on that stream."""
        stream = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(stream):
            self._range_word(stream).zero_()

    def __del__(self):
        try:
            for handle, _, _ in self._plans.values():
                lib().kvq_swin3d_plan_destroy(handle)
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass

    def prepare(self, B, T, H, W, device):
        """Set-up for forwards of this geometry on the CURRENT stream, without running one: the plan (index maps: device
        allocations, i.e. implicit synchronisations), its workspace, the packed weights and the attention bias image.
        A serving loop calls it once per stream before the first request."""
        handle, _, _ = self._plan(B, T, H, W, device)
        self._weights(device)
        self._set_dense_bias(handle, (T, H, W), device, B)

    # ------------------------------------------------------------------ forward
    def forward(self, batch, multi=False, layer=-1, adaptive_window_size=False, **kwargs):
        """``batch['technical']``: fp32 (B,3,T,H,W) on a HIP device -> (B, C_out, T/2, H/32, W/32)."""
        x = batch["technical"]
        aw = None
        if adaptive_window_size:
            # get_adaptive_window_size (swin_backbone.py:54-61, :1050-1053): the window scales with the clip against base_x_size
            aw = tuple((w * xs) // bs for w, xs, bs in zip(self.window_size, tuple(x.shape[2:]), self.base_x_size))
            if any(a < 1 or a > w for a, w in zip(aw, self.window_size)):
                # the reference's relative_position_index[:d,:h,:w,:d,:h,:w] slice (:266-271) cannot serve such a window either
                raise ValueError(f"adaptive window {aw} of a {tuple(x.shape[2:])} clip does not lie inside {tuple(self.window_size)}")
        if not x.is_cuda:
            raise _abi.KvqError("SwinTransformer3D.forward needs the clip on a HIP device; there is no CPU path")
        frag = None
        if isinstance(x, kernels.FragmentSource):
            # the batch is still (frames, sampler draws): the embedding launch reads through the sampler when it can
            B, _, T, H, W = x.shape
            frag = x.c_struct() if self.fused_tail and FUSE_SAMPLER else None
            # both gates: the source fits the fused read AND the plan takes the fused embedding launch at all (embed_dim 96 / 128,
            # patch (2,4,4)); otherwise swin_run would reach the im2col branch and refuse the fragment source
            if frag is not None and not (lib().kvq_patch_embed_fragments_supported(
                    C.byref(frag), B, self.in_chans, self.patch_size[0], T, H, W)
                    and lib().kvq_patch_embed_supported(self.in_chans, *self.patch_size, self.embed_dim, T, H, W)):
                frag = None
            if frag is None:
                x = x.materialise()
        else:
            x = x.to(torch.float32).contiguous()
        B, _, T, H, W = x.shape
        handle, (Cout, D, Hh, Ww), ws = self._plan(B, T, H, W, x.device, aw)
        w = self._weights(x.device)
        self._set_dense_bias(handle, (T, H, W), x.device, B, aw)
        feat = torch.empty(B, D, Hh, Ww, Cout, dtype=torch.float32, device=x.device)
        taps = None
        if multi or layer > -1:
            # feats = [embed, stage 0, ..., stage n-1] (swin_backbone.py:1060-1064): filled by the same forward
            n = self.num_layers + 1
            if layer >= n:
                raise IndexError("list index out of range")          # feats[layer] in the reference
            want = range(n - 1) if multi else [layer]
            taps, arr = [None] * n, (C.c_void_p * n)()
            for i in want:
                d4 = (C.c_int32 * 4)()
                check(lib().kvq_swin3d_tap_dims(handle, i, C.byref(d4)), "kvq_swin3d_tap_dims")
                taps[i] = torch.empty(B, d4[1], d4[2], d4[3], d4[0], dtype=torch.float32, device=x.device)
                arr[i] = ptr(taps[i])
            check(lib().kvq_swin3d_set_taps(handle, arr), "kvq_swin3d_set_taps")
        try:
            if frag is not None:
                check(lib().kvq_swin3d_forward_fragments(handle, C.byref(w), C.byref(frag), ptr(feat), ptr(ws), ws.numel(),
                                                         current_stream()), "kvq_swin3d_forward_fragments")
            else:
                check(lib().kvq_swin3d_forward(handle, C.byref(w), ptr(x), ptr(feat), ptr(ws), ws.numel(), _abi.stream_of(x)),
                      "kvq_swin3d_forward")
        finally:
            if taps is not None:
                check(lib().kvq_swin3d_set_taps(handle, None), "kvq_swin3d_set_taps")
        if multi:
            # torch.cat([F.interpolate(f, size=final (D,H,W), mode="trilinear") for f in feats[:-1]], 1) (:1070-1075)
            ctot = sum(t.shape[-1] for t in taps if t is not None)
            out = torch.empty(B, D, Hh, Ww, ctot, dtype=torch.float32, device=x.device)
            off = 0
            for t in taps:
                if t is None:
                    continue
                check(lib().kvq_resize_trilinear_cl(ptr(t), B, t.shape[1], t.shape[2], t.shape[3], t.shape[4], ptr(out), D, Hh,
                                                    Ww, ctot, off, current_stream()), "kvq_resize_trilinear_cl")
                off += t.shape[4]
            return out.permute(0, 4, 1, 2, 3)
        if layer > -1:
            return taps[layer].permute(0, 4, 1, 2, 3)
        return feat.permute(0, 4, 1, 2, 3)      # channels-last storage, reference's (B,C,D,H,W) view

    def forward_stages(self, x, stage_lo, stage_hi, geometry=None, want_feat=False, taps=()):
        """Stages ``stage_lo..stage_hi`` only (what KSVQE.forward interleaves its modulation with, KSVQE_model.py:1433-1486).
        ``stage_lo == 0``: x is the clip (B,3,T,H,W); otherwise x is the residual stream in front of ``stage_lo`` in the
        reference's layout (B, C, D, H', W') and ``geometry`` = the clip's (T, H, W).  Returns the stream behind
        ``stage_hi`` as (B, C, D, H', W') — the permuted view of the channels-last result — and, with ``want_feat`` on the
        last stage, the final-norm feature map as ``forward`` returns it.  ``taps``: indices of the reference's ``feats`` list
        (0 = behind the embedding, i + 1 = behind stage i) this run passes; they are copied out by the same run and returned as
        a third / second value ``{index: (B, C, D, H', W') tensor}``."""
        if not x.is_cuda:
            raise _abi.KvqError("SwinTransformer3D.forward_stages needs its input on a HIP device; there is no CPU path")
        if stage_lo == 0:
            x = x.to(torch.float32).contiguous()
            B, _, T, H, W = x.shape
        else:
            B = x.shape[0]
            T, H, W = geometry
        handle, (Cout, D, Hh, Ww), ws = self._plan(B, T, H, W, x.device)
        w = self._weights(x.device)
        self._set_dense_bias(handle, (T, H, W), x.device, B)
        d4 = (C.c_int32 * 4)()
        check(lib().kvq_swin3d_tap_dims(handle, stage_hi + 1, C.byref(d4)), "kvq_swin3d_tap_dims")
        io = torch.empty(B, d4[1], d4[2], d4[3], d4[0], dtype=torch.float32, device=x.device)
        if stage_lo > 0:
            check(lib().kvq_swin3d_tap_dims(handle, stage_lo, C.byref(d4)), "kvq_swin3d_tap_dims")
            if tuple(x.shape) != (B, d4[0], d4[1], d4[2], d4[3]):
                raise _abi.KvqError(f"stage {stage_lo} expects a (B, {d4[0]}, {d4[1]}, {d4[2]}, {d4[3]}) stream, got {tuple(x.shape)}")
            src = x.to(torch.float32).permute(0, 2, 3, 4, 1).contiguous()           # channels-last (layout only)
            if src.numel() > io.numel():
                io = torch.empty(src.numel(), dtype=torch.float32, device=x.device)
            io.reshape(-1)[: src.numel()].copy_(src.reshape(-1))
        feat = torch.empty(B, D, Hh, Ww, Cout, dtype=torch.float32, device=x.device) if want_feat else None
        tapped = {}
        if taps:
            arr = (C.c_void_p * (self.num_layers + 1))()
            for i in taps:
                if not ((stage_lo == 0 and i == 0) or stage_lo < i <= stage_hi + 1):
                    raise IndexError(f"feats[{i}] is not produced by stages {stage_lo}..{stage_hi}")
                t4 = (C.c_int32 * 4)()
                check(lib().kvq_swin3d_tap_dims(handle, i, C.byref(t4)), "kvq_swin3d_tap_dims")
                tapped[i] = torch.empty(B, t4[1], t4[2], t4[3], t4[0], dtype=torch.float32, device=x.device)
                arr[i] = ptr(tapped[i])
            check(lib().kvq_swin3d_set_taps(handle, arr), "kvq_swin3d_set_taps")
        try:
            check(lib().kvq_swin3d_forward_stages(handle, C.byref(w), ptr(x) if stage_lo == 0 else None, stage_lo, stage_hi, ptr(io),
                                                  ptr(feat), ptr(ws), ws.numel(), current_stream()), "kvq_swin3d_forward_stages")
        finally:
            if taps:
                check(lib().kvq_swin3d_set_taps(handle, None), "kvq_swin3d_set_taps")
        check(lib().kvq_swin3d_tap_dims(handle, stage_hi + 1, C.byref(d4)), "kvq_swin3d_tap_dims")
        n = B * d4[0] * d4[1] * d4[2] * d4[3]
        out = io.reshape(-1)[:n].reshape(B, d4[1], d4[2], d4[3], d4[0]).permute(0, 4, 1, 2, 3)
        res = (out, feat.permute(0, 4, 1, 2, 3)) if want_feat else out
        if taps:
            tapped = {i: t.permute(0, 4, 1, 2, 3) for i, t in tapped.items()}
            return (res + (tapped,)) if want_feat else (res, tapped)
        return res

    # profiling hooks used by bench.py ------------------------------------------------------
    def profile(self, B, T, H, W, device, enable: bool):
        handle, _, _ = self._plan(B, T, H, W, device)
        check(lib().kvq_swin3d_profile(handle, int(enable)), "kvq_swin3d_profile")

    def profile_read(self, B, T, H, W, device):
        handle, _, _ = self._plan(B, T, H, W, device)
        cap = 65536
        recs = (_abi.KvqProfRecord * cap)()
        n = C.c_int32(0)
        check(lib().kvq_swin3d_profile_read(handle, recs, cap, C.byref(n)), "kvq_swin3d_profile_read")
        ename = "kvq::Fp16" if self.operand_dtype == _abi.DT_FP16 else "kvq::Bf16"
        out = []
        for r in recs[: n.value]:
            kind = _abi.K_NAMES[r.kind]
            if kind.startswith("gemm"):
                tile, epi = divmod(r.variant, 10)
                mn, bk = divmod(tile, 100)
                sym = f"gemm_kernel<{ename}, {mn // 10}, {mn % 10}, {bk}, {epi}>"
                if tile == 4464:            # the 256 x 256 x 64 eight-phase kernel (csrc/gemm256.hip)
                    sym = f"gemm8p_kernel<{ename}, {epi}>"
                elif tile == 22264:         # 128 x 128 x 64 on the 2-slice ring of the QKV epilogue (kvq_gemm_kernel_choice)
                    sym = f"gemm_kernel<{ename}, 2, 2, 64, {epi}, 2>"
            elif kind == "attn" and r.variant >= 4:
                sym = f"window_attention32_kernel<{ename}>"
            elif kind == "attn":
                sym = f"window_attention_kernel<{ename}, {str(bool(r.variant & 2)).lower()}, {str(bool(r.variant & 1)).lower()}>"
            elif kind == "layernorm":
                sym = "layernorm_rows_kernel"
            elif kind == "embed":
                sym = (f"patch_embed_kernel<{ename}, {self.embed_dim // 32}, 6, {str(bool(r.variant & 1)).lower()}, "
                       f"{str(bool(r.variant & 2)).lower()}>")          # ..., + norm1 of block 0, reads through the sampler
                if r.variant & 4:                                       # ... out of I420 frames
                    sym = f"patch_embed_i420_kernel<{ename}, {self.embed_dim // 32}, 6, {str(bool(r.variant & 1)).lower()}>"
            elif kind == "merge":
                sym = f"patch_merge_kernel<{ename}, {str(bool(r.variant)).lower()}>"
            elif kind == "tail":
                geom, rest = divmod(r.variant, 1000)       # geom (from the library): (hidden chunk / 128) * 10 + token tiles per workgroup
                cm, mode = divmod(rest, 10)                # mode 0: x only, 1: + the next block's norm1 rows, 2: + the next block's q | k | v
                sym = f"block_tail_kernel<{ename}, {cm}, 4, {mode}, false>"
                if geom:                      # C = 256 / 384 / 512 / 768: csrc/tailmm.hip (feature-sliced GEMM chain, register weight ring)
                    sym = f"block_tailmm_kernel<{ename}, {mode}, {cm // 4}, {128 * (geom // 10)}, {geom % 10}>"
            else:
                sym = "patch_im2col_kernel"
            out.append(dict(kind=kind, kernel=sym, ms=float(r.ms), flops=float(r.flops), bytes=float(r.bytes)))
        return out


def swin_3d_tiny(**kwargs):
    """``swin_backbone.py:1088-1090``: no fragment tables (the gate is computed but unused)."""
    return SwinTransformer3D(depths=[2, 2, 6, 2], frag_biases=[0, 0, 0, 0], **kwargs)


def swin_3d_small(**kwargs):
    return SwinTransformer3D(depths=[2, 2, 18, 2], frag_biases=[0, 0, 0, 0], **kwargs)
