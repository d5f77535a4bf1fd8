"""Thin per-kernel wrappers over the C-ABI (torch tensors in, torch tensors out).

Used by the parity tests (each kernel against the oracle) and by the modules.  PyTorch is
only the owner of device memory and the provider of the current HIP stream here.  The 16-bit
MFMA operand type (fp16 | bf16) is taken from the tensors' dtype.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _abi
from ._abi import check, current_stream, dtype_code, lib, ptr, stream_of
from ._prepared import to_operand

HALF_TYPES = (torch.float16, torch.bfloat16)


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _abi.KvqError("kvq_amd kernels need tensors on a HIP device (no CPU fallback exists)")


def device_name() -> str:
    buf = C.create_string_buffer(256)
    check(lib().kvq_device_name(buf, 256), "kvq_device_name")
    return buf.value.decode()


def layernorm_rows(x: torch.Tensor, gamma, beta, *, index_map: Optional[torch.Tensor] = None, nparts=1,
                   n_batch=1, rows_out: Optional[int] = None, out_dtype=torch.float16, eps=1e-5):
    """x fp32 [n_batch*rows_in, Cin]; index_map int32 [rows_out, nparts] (or None = identity).
    out_dtype: torch.float16 / torch.bfloat16 (MFMA operand) or torch.float32."""
    _need_gpu(x, gamma, beta, index_map)
    assert x.dtype == torch.float32 and x.is_contiguous()
    rows_in = x.shape[0] // n_batch
    Cin = x.shape[1]
    rows_out = rows_in if rows_out is None else rows_out
    out = torch.empty(n_batch * rows_out, nparts * Cin, dtype=out_dtype, device=x.device)
    half = out_dtype in HALF_TYPES
    check(lib().kvq_layernorm_rows(ptr(x), ptr(index_map), nparts, n_batch, rows_in, rows_out, Cin, ptr(gamma),
                                   ptr(beta), eps, ptr(out) if half else None,
                                   dtype_code(out_dtype) if half else 0, None if half else ptr(out),
                                   current_stream()), "kvq_layernorm_rows")
    return out


def _splitk_scratch(a, M: int, N: int, K: int, device):
    """Split-K scratch for a GEMM / implicit-conv launch (long K, few output tiles): the library says how much it would use;
    the buffer comes from torch's stream-ordered allocator (reused only by later work of this stream), so it may be dropped
    as soon as the launch is enqueued.  Returned so that the caller keeps it alive across the call."""
    nb = lib().kvq_gemm_splitk_bytes(M, N, K)
    if not nb:
        return None
    ws = torch.empty(nb, dtype=torch.uint8, device=device)
    a.splitk_ws, a.splitk_ws_bytes = ptr(ws), nb
    return ws


def _concat_dest(out, M: int, ldc: int, col_off: int):
    """(ldc, col_off) of a launch that writes into a wider 16-bit destination: ``out`` must then be a contiguous [M, ldc] tensor.
    Which epilogues take them, and which values, is the library's decision (it refuses the rest)."""
    if ldc and out is not None:
        assert out.is_contiguous() and out.numel() == M * ldc, "ldc: pass out= as a contiguous [M, ldc] tensor"
    return int(ldc), int(col_off)


def gemm(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], epilogue: int, *, out=None,
         num_heads=0, q_scale=1.0, scatter_map=None, map_rows=0, out_rows=0, a_gather=None, a_rows=0, rows=None, col_scale=None, ldc=0, col_off=0):
    """A [M,K], W [N,K], both fp16 or both bf16.  Returns the output tensor (allocated unless given).
    ``ldc`` / ``col_off`` (16-bit row-major epilogues, ``out`` given as [M, ldc]): the N columns land at columns col_off ..
    col_off+N-1 of rows of ldc elements; the library refuses them for the other epilogues.
    ``col_scale`` (fp32 [N], residual epilogue only): out += col_scale * (A W^T + bias) — ``kvq_gemm_resid_scaled``.
    ``a_gather`` (+ ``a_rows``, ``rows`` = GEMM rows): row m reads A row (m // a_rows) * (A rows per batch) + a_gather[m % a_rows].
    QKV epilogue with ``scatter_map``: GEMM row m lands in row (m // map_rows) * out_rows + scatter_map[m % map_rows] of a buffer
    with out_rows rows per batch element (the other rows are ``qkv_fill_pad``'s)."""
    _need_gpu(A, W, bias, out, scatter_map, a_gather, col_scale)
    assert A.dtype in HALF_TYPES and W.dtype == A.dtype and A.is_contiguous() and W.is_contiguous()
    if col_scale is not None:
        if epilogue not in (_abi.EPI_RESID_F32, _abi.EPI_RESID_SCALE_F32):
            raise ValueError("col_scale belongs to the residual epilogue")
        assert col_scale.dtype == torch.float32 and col_scale.is_contiguous() and col_scale.numel() == W.shape[0]
        epilogue = _abi.EPI_RESID_SCALE_F32
    M, K = A.shape
    a_phys = 0
    if a_gather is not None:
        a_phys = A.shape[0] // (rows // a_rows)
        M = rows
    N = W.shape[0]
    if out is None:
        if epilogue == _abi.EPI_QKV_BF16:
            out = torch.empty(3, num_heads, M if scatter_map is None else M // map_rows * out_rows, 32, dtype=A.dtype, device=A.device)
        elif epilogue in (_abi.EPI_BIAS_BF16, _abi.EPI_GELU_BF16, _abi.EPI_QGELU_BF16):
            out = torch.empty(M, N, dtype=A.dtype, device=A.device)
        elif epilogue == _abi.EPI_STORE_F32:
            out = torch.empty(M, N, dtype=torch.float32, device=A.device)
        else:
            raise ValueError("RESID epilogue accumulates into an existing tensor: pass out=")
    a = _abi.KvqGemmArgs()
    a.A, a.W, a.bias, a.M, a.N, a.K, a.epilogue = ptr(A), ptr(W), ptr(bias), M, N, K, epilogue
    if out.dtype in HALF_TYPES:
        assert out.dtype == A.dtype
        a.out_bf16 = ptr(out)
    else:
        a.out_f32 = ptr(out)
    a.num_heads, a.q_scale = num_heads, q_scale
    a.scatter_map, a.map_rows, a.out_rows = ptr(scatter_map), map_rows, out_rows
    a.a_gather, a.a_rows, a.a_phys_rows = ptr(a_gather), a_rows, a_phys
    a.ldc, a.col_off = _concat_dest(out if out.dtype in HALF_TYPES else None, M, ldc, col_off)
    a.dtype = dtype_code(A.dtype)
    _ws = _splitk_scratch(a, a.M, a.N, a.K, A.device) if (a.epilogue != _abi.EPI_QKV_BF16 and a_gather is None) else None   # noqa: F841
    if col_scale is not None:
        check(lib().kvq_gemm_resid_scaled(C.byref(a), ptr(col_scale), current_stream()), "kvq_gemm_resid_scaled")
    else:
        check(lib().kvq_gemm_bf16(C.byref(a), current_stream()), "kvq_gemm_bf16")
    return out


def dwconv3d_ln_supported(C_: int, kt: int, T: int, H: int, W: int) -> bool:
    return bool(lib().kvq_dwconv3d_ln_supported(C_, kt, T, H, W))


def dwconv_weight_taps(w: torch.Tensor) -> torch.Tensor:
    """Depthwise Conv3d weight (C, 1, kt, 7, 7) -> the tap-major fp32 [kt*7*7, C] that ``dwconv3d_ln`` streams."""
    Cc = w.shape[0]
    return w.reshape(Cc, -1).t().contiguous()


def dwconv3d_ln(x: torch.Tensor, w_taps: torch.Tensor, bias, ln_w, ln_b, *, eps=1e-6, out_dtype=torch.float16):
    """Depthwise (kt,7,7) conv (zero padding kt//2, 3, 3) + LayerNorm over C in one launch.  x fp32 channels-last (B, T, H, W, C),
    w_taps fp32 [kt*49, C] (``dwconv_weight_taps``) -> rows [B*T*H*W, C] in ``out_dtype`` (fp16 / bf16 operand rows, or fp32)."""
    _need_gpu(x, w_taps, bias, ln_w, ln_b)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 5
    assert w_taps.dtype == torch.float32 and w_taps.is_contiguous() and w_taps.shape[0] % 49 == 0
    B, T, H, W, Cc = x.shape
    kt = w_taps.shape[0] // 49
    half = out_dtype in HALF_TYPES
    a = _abi.KvqDwconvLnArgs()
    a.x, a.w, a.bias, a.ln_w, a.ln_b = ptr(x), ptr(w_taps), ptr(bias), ptr(ln_w), ptr(ln_b)
    a.B, a.T, a.H, a.W, a.C, a.kt, a.eps = B, T, H, W, Cc, kt, eps
    if w_taps.shape[1] != Cc or not lib().kvq_dwconv3d_ln_supported(Cc, kt, T, H, W):
        raise _abi.KvqError(f"kvq_dwconv3d_ln: unsupported shape (C={Cc}, kt={kt}, weight {tuple(w_taps.shape)}; C in 96/192/384/768, kt in 1/3)")
    out = torch.empty(B * T * H * W, Cc, dtype=out_dtype, device=x.device)
    a.dtype = dtype_code(out_dtype) if half else 0
    a.out_h, a.out_f32 = (ptr(out), None) if half else (None, ptr(out))
    check(lib().kvq_dwconv3d_ln(C.byref(a), current_stream()), "kvq_dwconv3d_ln")
    return out


def grn_supported(N: int, D: int, H: int, W: int) -> bool:
    return bool(lib().kvq_grn_supported(N, D, H, W))


def grn(hid: torch.Tensor, shape, gamma, beta, *, over="th", out=None):
    """Global Response Normalization of the 16-bit rows ``hid`` [B*D*H*W, N] (tokens in (b, d, h, w) order, ``shape`` = (B, D, H, W)):
    ``x * (1 + gamma * Nx) + beta`` with ``Nx = Gx / (mean_n Gx + 1e-6)`` and ``Gx`` the L2 norm over (d, h) per (b, w, n) —
    ``over="th"``, what the reference's BlockV23D computes — or over (d, h, w) per (b, n) — ``over="thw"``.  In place unless ``out`` is
    given; returns the tensor written.  gamma / beta: fp32 with N elements (any shape)."""
    _need_gpu(hid, gamma, beta)
    if over not in ("th", "thw"):
        raise ValueError(f"grn: over must be 'th' or 'thw', got {over!r}")
    B, D, H, W = (int(v) for v in shape)
    assert hid.dtype in HALF_TYPES and hid.is_contiguous() and hid.dim() == 2 and hid.shape[0] == B * D * H * W
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.is_contiguous() and beta.is_contiguous()
    N = hid.shape[1]
    if gamma.numel() != N or beta.numel() != N or not lib().kvq_grn_supported(N, D, H, W):
        raise _abi.KvqError(f"kvq_grn: unsupported shape (N={N}, (B, D, H, W)={(B, D, H, W)}, gamma {tuple(gamma.shape)}; "
                            "N in 384/768/1536/3072)")
    y = hid if out is None else out
    assert y.dtype == hid.dtype and y.shape == hid.shape and y.is_contiguous()
    ws = torch.empty(lib().kvq_grn_workspace_bytes(B, D, H, W, N) // 4, dtype=torch.float32, device=hid.device)
    a = _abi.KvqGrnArgs()
    a.x, a.y, a.gamma, a.beta, a.ws = ptr(hid), (None if out is None else ptr(out)), ptr(gamma), ptr(beta), ptr(ws)
    a.B, a.D, a.H, a.W, a.N, a.dtype, a.over_w = B, D, H, W, N, dtype_code(hid.dtype), int(over == "thw")
    check(lib().kvq_grn_stats(C.byref(a), current_stream()), "kvq_grn_stats")
    check(lib().kvq_grn_apply(C.byref(a), current_stream()), "kvq_grn_apply")
    return y


def gemm_tile_mode(mode: int) -> int:
    """-1: main loop by shape (default), 0: never the 256 x 256 eight-phase tile, 1: whenever eligible.  Returns the previous mode."""
    return lib().kvq_gemm_tile_mode(mode)


GEMM_8P, GEMM_QKV_RING2 = 4464, 22264      # kvq_gemm_kernel_choice: the eight-phase kernel; 128 x 128 x 64 on the 2-slice QKV ring


def gemm_kernel_choice(M: int, N: int, K: int, epilogue: int = _abi.EPI_BIAS_BF16, conv: bool = False) -> int:
    """The main loop ``gemm`` / ``conv_gemm`` (conv=False) or ``conv_implicit`` (conv=True, K = the weight's padded K) launch for
    this shape under the current tile mode: MI*1000 + NI*100 + BK of the ring kernel's 64 MI x 64 NI x BK tile, ``GEMM_QKV_RING2``
    or ``GEMM_8P``; 0 for a shape the launch refuses.  Host only (no GPU needed)."""
    return lib().kvq_gemm_kernel_choice(M, N, K, epilogue, int(conv))


def qkv_fill_pad(qkv: torch.Tensor, qkv_bias: torch.Tensor, pad_rows: torch.Tensor, n_batch: int, q_scale: float):
    """q | k | v = bias (q scaled) in the padding rows ``pad_rows`` (int32, window order) of every batch element of the head-major
    buffer qkv [3, nH, n_batch * rows, 32] — what the reference computes for rows padded after norm1."""
    _need_gpu(qkv, qkv_bias, pad_rows)
    assert qkv.dtype in HALF_TYPES and qkv.is_contiguous() and pad_rows.dtype == torch.int32 and qkv_bias.dtype == torch.float32
    check(lib().kvq_qkv_fill_pad(ptr(qkv), ptr(qkv_bias), ptr(pad_rows), pad_rows.numel(), n_batch, qkv.shape[2] // n_batch, qkv.shape[1],
                                 q_scale, dtype_code(qkv.dtype), stream_of(qkv)), "kvq_qkv_fill_pad")
    return qkv


def window_attention(qkv: torch.Tensor, tok: torch.Tensor, rpb: torch.Tensor, fpb: Optional[torch.Tensor],
                     center: int, nW: int, N: int, use_mask: bool, bias_pack: Optional[torch.Tensor] = None):
    """qkv fp16|bf16 [3,nH,BW*N,32] (q pre-scaled), tok int32 [nW*N,2]; returns [BW*N, nH*32]."""
    _need_gpu(qkv, tok, rpb, fpb)
    assert qkv.dtype in HALF_TYPES and qkv.is_contiguous()
    nH = qkv.shape[1]
    BW = qkv.shape[2] // N
    out = torch.empty(BW * N, nH * 32, dtype=qkv.dtype, device=qkv.device)
    check(lib().kvq_window_attention(ptr(qkv), ptr(tok), ptr(rpb), ptr(fpb), ptr(bias_pack), rpb.shape[0], center, BW, nW, N, nH,
                                     int(use_mask), dtype_code(qkv.dtype), ptr(out), current_stream()),
          "kvq_window_attention")
    return out


LOG2E = 1.4426950408889634


def attn_bias32(tok: torch.Tensor, rpb: torch.Tensor, fpb: Optional[torch.Tensor], center: int, nW: int, N: int, use_mask: bool):
    """The attention bias image of one block for ``window_attention32`` (include/kvq_hip.h); ``nW`` = the number of window TYPES
    to build (the first nW windows' descriptors of ``tok``)."""
    _need_gpu(tok, rpb, fpb)
    nH = rpb.shape[1]
    out = torch.empty(lib().kvq_attn_bias32_bytes(nW, N, nH), dtype=torch.uint8, device=rpb.device)
    big = torch.zeros(1, dtype=torch.float32, device=rpb.device)
    check(lib().kvq_attn_bias32_build(ptr(tok), ptr(rpb), ptr(fpb), rpb.shape[0], center, nW, N, nH, int(use_mask),
                                      ptr(out), ptr(big), current_stream()), "kvq_attn_bias32_build")
    out.max_abs_bias = big          # device scalar: largest un-masked |bias| (fp16 storage rounds by 2^-11 of it)
    return out


def window_attention32(qkv: torch.Tensor, image: torch.Tensor, nW: int, N: int, n_types: Optional[int] = None,
                       tile_skip: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, dsplit_from: int = -1,
                       x_ln: Optional[torch.Tensor] = None, w_qkv: Optional[torch.Tensor] = None, b_qkv: Optional[torch.Tensor] = None,
                       q_scale: float = 1.0, pad_mask: Optional[torch.Tensor] = None, ranges: Optional[torch.Tensor] = None):
    """qkv fp16|bf16 [3,nH,BW*N,32] with q scaled by head_dim^-0.5 * log2(e) + the pre-built bias image of ``attn_bias32``; returns
    [BW*N, nH*32].  ``n_types`` (default nW): window w uses bias w % n_types.  ``tile_skip`` int32 [nW]: bit t = rows 16t..16t+15 of the
    window are padding only (a 32-row q-block is passed over when both its tiles are; such rows keep what ``out`` held).
    ``dsplit_from`` >= 0: windows >= it are depth-split (shifted (8,7,7) blocks).  ``x_ln`` [BW*N, C] + ``w_qkv`` [3C, C] + ``b_qkv`` [3C]:
    the launch computes q | k | v itself (``qkv`` = a [1|3, nH, BW*N, 32] buffer whose first third receives q; ``q_scale`` =
    head_dim^-0.5 * log2(e)).  ``pad_mask`` int32 [nW, 13] (+ ``b_qkv``): bit r of window w = row r is a padding row — its k | v are
    written by the kernel (= the bias), its q taken as zero; those rows of ``qkv`` are not read.  ``ranges`` uint8 [nW, 13, 2]
    (``attn32_key_ranges``; rows in region order): a q-block passes over the key blocks outside its range."""
    _need_gpu(qkv, image, tile_skip, out, pad_mask, ranges)
    assert qkv.dtype in HALF_TYPES and qkv.is_contiguous()
    nH = qkv.shape[1]
    BW = qkv.shape[2] // N
    if out is None:
        out = torch.empty(BW * N, nH * 32, dtype=qkv.dtype, device=qkv.device)
    a = _abi.KvqAttnDenseArgs()
    a.qkv, a.bias_dense, a.n_types, a.BW, a.nW, a.N, a.num_heads = ptr(qkv), ptr(image), nW if n_types is None else n_types, BW, nW, N, nH
    a.dtype, a.out, a.tile_skip, a.dsplit_from = dtype_code(qkv.dtype), ptr(out), ptr(tile_skip), dsplit_from
    if x_ln is not None:      # fused qkv projection: ``qkv`` only lends its q third as scratch ([nH, BW*N, 32] is enough)
        _need_gpu(x_ln, w_qkv, b_qkv)
        assert x_ln.dtype == qkv.dtype == w_qkv.dtype and x_ln.is_contiguous() and w_qkv.is_contiguous() and b_qkv.dtype == torch.float32
        a.x_ln, a.w_qkv, a.b_qkv, a.q_scale = ptr(x_ln), ptr(w_qkv), ptr(b_qkv), q_scale
    if pad_mask is not None:
        _need_gpu(b_qkv)
        assert pad_mask.dtype == torch.int32 and pad_mask.is_contiguous() and (b_qkv is None or b_qkv.dtype == torch.float32)
        a.pad_mask, a.b_qkv = ptr(pad_mask), ptr(b_qkv)
    if ranges is not None:
        assert ranges.dtype == torch.uint8 and ranges.is_contiguous() and ranges.numel() == nW * 26
        check(lib().kvq_window_attention32_ranges(C.byref(a), ptr(ranges), current_stream()), "kvq_window_attention32_ranges")
        return out
    check(lib().kvq_window_attention32(C.byref(a), current_stream()), "kvq_window_attention32")
    return out


def attn32_row_order(tok, n_windows: int, N: int):
    """Host: the region order of every window's rows — int32 [n_windows, N], entry i = the index (in ``tok``'s order) of the row the
    order stores at position i (``tok`` int32 [n_windows*N, 2] descriptors, numpy or CPU tensor)."""
    import numpy as np
    tok = np.ascontiguousarray(np.asarray(tok, dtype=np.int32).reshape(n_windows * N, 2))
    order = np.empty((n_windows, N), np.int32)
    check(lib().kvq_attn32_row_order(tok.ctypes.data, n_windows, N, order.ctypes.data), "kvq_attn32_row_order")
    return order


def attn32_key_ranges(tok, n_windows: int, N: int, use_mask: bool):
    """Host: uint8 [n_windows, 13, 2] = first and last 32-key block every 32-query block needs, from the descriptors ``tok`` of the
    rows in the order they are stored (numpy or CPU tensor)."""
    import numpy as np
    tok = np.ascontiguousarray(np.asarray(tok, dtype=np.int32).reshape(n_windows * N, 2))
    ranges = np.empty((n_windows, 13, 2), np.uint8)
    check(lib().kvq_attn32_key_ranges(tok.ctypes.data, n_windows, N, int(use_mask), ranges.ctypes.data), "kvq_attn32_key_ranges")
    return ranges


def patch_im2col(x: torch.Tensor, patch: Sequence[int], out_dtype=torch.float16):
    _need_gpu(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    B, Cin, T, H, W = x.shape
    pd, ph, pw = patch
    D, Hh, Ww = -(-T // pd), -(-H // ph), -(-W // pw)
    out = torch.empty(B * D * Hh * Ww, Cin * pd * ph * pw, dtype=out_dtype, device=x.device)
    check(lib().kvq_patch_im2col(ptr(x), B, Cin, T, H, W, pd, ph, pw, dtype_code(out_dtype), ptr(out),
                                 current_stream()), "kvq_patch_im2col")
    return out


def vqa_head(feat: torch.Tensor, w1, b1, w2, b2, w1t=None, return_map=False):
    """feat fp32 (B,C,D,H,W) with ANY strides over a dense token grid -> score fp32 [B,1].
    ``w1`` [hidden,C] (what the fp32-MFMA kernel reads: hidden == 64, channels-last features) and / or ``w1t`` [C,hidden]
    (the VALU kernel's layout; made here from ``w1`` when missing).
    ``return_map``: ``(score, tok_map (B,D,H,W), depth_score (B,D))`` — the per-token scores (``b2`` included: their mean is the
    score) and their mean per depth slice (``kvq_vqa_head_map``); the score has the same bits either way."""
    _need_gpu(feat, w1, b1, w2, b2, w1t)
    assert feat.dtype == torch.float32 and feat.dim() == 5
    B, Cc, D, H, W = feat.shape
    L = D * H * W
    sb, sc, sd, sh, sw = feat.stride()
    if not (sh == W * sw and sd == H * sh):          # tokens must be addressable with one stride
        feat = feat.contiguous()
        sb, sc, sd, sh, sw = feat.stride()
    if w1 is not None:
        w1 = w1.reshape(w1.shape[0], -1).contiguous()
    if w1t is None:
        w1t = w1.t().contiguous()               # [C][hidden]: what the VALU kernel streams (kvq_hip.h)
    hidden = w1t.shape[1]
    scratch = torch.empty(B * L, dtype=torch.float32, device=feat.device)
    score = torch.empty(B, dtype=torch.float32, device=feat.device)
    if return_map:
        depth = torch.empty(B, D, dtype=torch.float32, device=feat.device)
        check(lib().kvq_vqa_head_map(ptr(feat), B, L, Cc, sb, sw, sc, ptr(w1t), ptr(w1), ptr(b1), hidden, ptr(w2), ptr(b2), D,
                                     ptr(scratch), ptr(depth), ptr(score), current_stream()), "kvq_vqa_head_map")
        return score.reshape(B, 1), scratch.reshape(B, D, H, W), depth
    check(lib().kvq_vqa_head(ptr(feat), B, L, Cc, sb, sw, sc, ptr(w1t), ptr(w1), ptr(b1), hidden, ptr(w2), ptr(b2),
                             ptr(scratch), ptr(score), current_stream()), "kvq_vqa_head")
    return score.reshape(B, 1)


def vqa_head_classes(feat: torch.Tensor, w1, b1, w2, b2, pre_pool=False):
    """VQAHead's pre_pool / num_class > 1 branches (head.py:60-68): feat fp32 (B,C,D,H,W) with any strides over a dense token grid,
    ``w1`` [hidden,C], ``w2`` [num_class,hidden], ``b2`` [num_class] -> fp32 [B,num_class] (softmax over the classes per token when
    num_class > 1, then the mean over the tokens; ``pre_pool``: the token grid is averaged first)."""
    _need_gpu(feat, w1, b1, w2, b2)
    assert feat.dtype == torch.float32 and feat.dim() == 5
    B, Cc, D, H, W = feat.shape
    L = D * H * W
    sb, sc, sd, sh, sw = feat.stride()
    if not (sh == W * sw and sd == H * sh):
        feat = feat.contiguous()
        sb, sc, sd, sh, sw = feat.stride()
    w1t = w1.reshape(w1.shape[0], -1).t().contiguous()
    hidden = w1t.shape[1]
    w2 = w2.reshape(w2.shape[0], -1).contiguous()
    K = w2.shape[0]
    assert w2.shape[1] == hidden and b2.numel() == K and w1t.shape[0] == Cc
    scratch = torch.empty(B * Cc + B * K if pre_pool else B * L * K, dtype=torch.float32, device=feat.device)
    score = torch.empty(B, K, dtype=torch.float32, device=feat.device)
    check(lib().kvq_vqa_head_classes(ptr(feat), B, L, Cc, sb, sw, sc, ptr(w1t), ptr(b1), hidden, ptr(w2), ptr(b2), K,
                                     1 if pre_pool else 0, ptr(scratch), ptr(score), current_stream()), "kvq_vqa_head_classes")
    return score


def simple_vqa_head(feat: torch.Tensor, w1, b1, w2, b2):
    _need_gpu(feat, w1, b1, w2, b2)
    assert feat.dtype == torch.float32
    feat = feat.contiguous()
    B, T, Cin = feat.shape
    scratch = torch.empty(B * T, dtype=torch.float32, device=feat.device)
    score = torch.empty(B, dtype=torch.float32, device=feat.device)
    check(lib().kvq_simple_vqa_head(ptr(feat), B, T, Cin, ptr(w1), ptr(b1), w1.shape[0], ptr(w2), ptr(b2),
                                    ptr(scratch), ptr(score), current_stream()), "kvq_simple_vqa_head")
    return score.reshape(B, 1)


def i420_frame_bytes(H: int, W: int) -> int:
    """bytes of one I420 frame: Y (H x W) | U | V (ceil(H/2) x ceil(W/2) each)"""
    return H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)


def yuv420_coeffs(fmt: int):
    """(qy, qrv, qgu, qgv, qbu, yoff): the integers of the library's YUV -> RGB conversion for an ``_abi.SRC_I420_*`` format
    (``kvq_yuv420_coeffs``, host only)"""
    out = (C.c_int32 * 6)()
    check(lib().kvq_yuv420_coeffs(int(fmt), C.byref(out)), "kvq_yuv420_coeffs")
    return tuple(out)


class I420Frames:
    """T planar YUV 4:2:0 frames on the device, "I420, frame-major": ``data`` uint8 (T, frame_bytes), every row one frame
    Y | U | V (``i420_frame_bytes``), rows back to back — what a decoder hands over, 1.5 B/pixel.  ``fmt``: an
    ``_abi.SRC_I420_*`` value (matrix and range).  Stands where a uint8 (3,T,H,W) frame tensor stands: the fragment sampler
    (``fragment_gather``, ``FragmentSource`` and through it the fused embedding read and the quality paint) reads it as it is
    and converts the pixels it touches; consumers of whole frames take ``to_rgb()``.  Bit-equal either way: one conversion."""

    dtype = torch.uint8

    def __init__(self, data: torch.Tensor, H: int, W: int, fmt: int):
        H, W, fmt = int(H), int(W), int(fmt)
        if fmt not in _abi.I420_FORMATS:
            raise ValueError(f"I420Frames: format {fmt} is not one of _abi.I420_FORMATS")
        fb = i420_frame_bytes(H, W)
        if not (data.dtype == torch.uint8 and data.dim() == 2 and data.shape[0] > 0 and data.shape[1] == fb and data.stride(1) == 1
                and (data.shape[0] == 1 or data.stride(0) == fb)):
            raise ValueError(f"I420Frames: expected uint8 (T, {fb}) with the frames back to back, got {data.dtype} {tuple(data.shape)} "
                             f"strides {data.stride()}")
        self.data, self.H, self.W, self.format = data, H, W, fmt
        self.shape = (3, data.shape[0], H, W)
        self.device, self.is_cuda = data.device, data.is_cuda
        self._rgb = None

    def data_ptr(self):
        return self.data.data_ptr()

    def contiguous(self):
        return self

    def is_contiguous(self):
        return True

    def record_stream(self, stream):
        self.data.record_stream(stream)
        if self._rgb is not None:
            self._rgb.record_stream(stream)

    def to(self, device, non_blocking=False):
        d = self.data.to(device, non_blocking=non_blocking)
        return self if d is self.data else I420Frames(d, self.H, self.W, self.format)

    def frames(self, lo: int, hi: int) -> "I420Frames":
        """frames lo .. hi-1 as a view: a run of frames of a longer video is still one pointer"""
        return I420Frames(self.data[lo:hi], self.H, self.W, self.format)

    def select(self, index: torch.Tensor) -> "I420Frames":
        """the frames ``index`` (int64, on the device) names, in that order, as new storage (one row gather)"""
        return I420Frames(self.data.index_select(0, index), self.H, self.W, self.format)

    def to_rgb(self) -> torch.Tensor:
        """uint8 (3,T,H,W): ``kvq_yuv420_to_rgb``, one launch, converted once and kept"""
        if self._rgb is None:
            _need_gpu(self.data)
            _, T, H, W = self.shape
            out = torch.empty(3, T, H, W, dtype=torch.uint8, device=self.device)
            check(lib().kvq_yuv420_to_rgb(ptr(self.data), T, H, W, self.format, ptr(out), stream_of(self.data)), "kvq_yuv420_to_rgb")
            self._rgb = out
        return self._rgb


def jpeg_coef_bytes(H: int, W: int) -> int:
    """bytes of one frame's coefficient hand-over (``kvq_jpeg_coef_bytes``): 768 per 16 x 16 MCU"""
    n = lib().kvq_jpeg_coef_bytes(int(H), int(W))
    if n == 0:
        raise ValueError(f"jpeg_coef_bytes: a frame of {W} x {H} is outside what the library decodes")
    return n


def jpeg_probe(buf):
    """``kvq_jpeg_probe`` on a uint8 numpy array (host only) -> (status, ``_abi.KvqJpegInfo``, message)"""
    info = _abi.KvqJpegInfo()
    rc = lib().kvq_jpeg_probe(buf.ctypes.data, buf.size, C.byref(info))
    return rc, info, (lib().kvq_last_error().decode("utf-8", "replace") if rc else "")


def jpeg_coeffs(buf, coef_out, qt_out):
    """``kvq_jpeg_coeffs`` (host only): the image in the uint8 numpy array ``buf`` -> ``coef_out`` int16 (jpeg_coef_bytes / 2,),
    ``qt_out`` uint16 (3, 64), both numpy views of host memory.  Returns (status, message); the ctypes call releases the GIL."""
    rc = lib().kvq_jpeg_coeffs(buf.ctypes.data, buf.size, coef_out.ctypes.data, coef_out.nbytes, qt_out.ctypes.data)
    return rc, (lib().kvq_last_error().decode("utf-8", "replace") if rc else "")


def jpeg_idct_i420_host(coef, qt, H: int, W: int):
    """the scalar twin of ``jpeg_idct_i420`` on numpy arrays: coef int16 (T, jpeg_coef_bytes / 2), qt uint16 (T, 3, 64) -> uint8
    (T, i420_frame_bytes)"""
    import numpy as np
    coef, qt = np.ascontiguousarray(coef, np.int16), np.ascontiguousarray(qt, np.uint16)
    T = qt.reshape(-1, 3, 64).shape[0]
    assert coef.size * 2 == T * jpeg_coef_bytes(H, W), (coef.shape, T, H, W)
    out = np.empty((T, i420_frame_bytes(H, W)), np.uint8)
    check(lib().kvq_jpeg_idct_i420_host(coef.ctypes.data, qt.ctypes.data, T, int(H), int(W), out.ctypes.data), "kvq_jpeg_idct_i420_host")
    return out


def jpeg_idct_i420(coef: torch.Tensor, qt: torch.Tensor, H: int, W: int, out: Optional[torch.Tensor] = None) -> "I420Frames":
    """Quantised JPEG coefficients -> ``I420Frames`` (BT.601 full range, what JFIF fixes), one launch (``kvq_jpeg_idct_i420``).
    coef int16 (T, jpeg_coef_bytes / 2) in the hand-over layout of ``kvq_jpeg_coeffs``, qt uint16 (T, 3, 64), both on the device."""
    _need_gpu(coef, qt)
    T = qt.shape[0]
    assert coef.dtype == torch.int16 and qt.dtype == torch.uint16 and coef.is_contiguous() and qt.is_contiguous()
    assert tuple(qt.shape) == (T, 3, 64) and coef.numel() * 2 == T * jpeg_coef_bytes(H, W), (tuple(coef.shape), tuple(qt.shape), H, W)
    if out is None:
        out = torch.empty(T, i420_frame_bytes(H, W), dtype=torch.uint8, device=coef.device)
    else:
        assert out.dtype == torch.uint8 and tuple(out.shape) == (T, i420_frame_bytes(H, W)) and out.is_contiguous() and out.device == coef.device
    check(lib().kvq_jpeg_idct_i420(ptr(coef), ptr(qt), T, int(H), int(W), ptr(out), stream_of(coef)), "kvq_jpeg_idct_i420")
    return I420Frames(out, H, W, _abi.SRC_I420_BT601_FULL)


JPEG_TABLES_BYTES = _abi.JPEG_TABLES_BYTES


def jpeg_index(buf, seg_out, tables_out, qt_out):
    """``kvq_jpeg_index`` (host only): the image in the uint8 numpy array ``buf`` -> its segments in ``seg_out`` uint32 (cap, 2)
    (byte ranges relative to ``buf``), its table set in ``tables_out`` uint8 (JPEG_TABLES_BYTES,), its quantiser tables in ``qt_out``
    uint16 (3, 64) -> (status, ``_abi.KvqJpegInfo``, nseg, message).  The call releases the GIL."""
    import numpy as np
    info, nseg = _abi.KvqJpegInfo(), C.c_size_t(0)
    assert seg_out.dtype == np.uint32 and seg_out.flags.c_contiguous and tables_out.nbytes == JPEG_TABLES_BYTES and qt_out.nbytes == 384
    rc = lib().kvq_jpeg_index(buf.ctypes.data, buf.size, C.byref(info), seg_out.ctypes.data, seg_out.size // 2, C.byref(nseg),
                              tables_out.ctypes.data, qt_out.ctypes.data)
    return rc, info, int(nseg.value), (lib().kvq_last_error().decode() if rc else "")


def jpeg_entropy_host(data, frames, segs, tables, T: int, H: int, W: int):
    """the host twin of ``jpeg_entropy`` on numpy arrays (``kvq_jpeg_entropy_host``): data uint8 (nbytes,), frames uint32 (T, 5), segs
    uint32 (nsegs, 2), tables uint8 (ntables, JPEG_TABLES_BYTES) -> (coef int16 (T, jpeg_coef_bytes / 2), status int32 (nsegs,))"""
    import numpy as np
    assert data.dtype == np.uint8 and frames.dtype == np.uint32 and segs.dtype == np.uint32 and tables.dtype == np.uint8
    assert all(a.flags.c_contiguous for a in (data, frames, segs, tables)) and frames.shape == (T, 5)
    assert segs.ndim == 2 and segs.shape[1] == 2 and tables.ndim == 2 and tables.shape[1] == JPEG_TABLES_BYTES
    coef = np.empty((T, jpeg_coef_bytes(H, W) // 2), np.int16)
    status = np.empty(segs.shape[0], np.int32)
    check(lib().kvq_jpeg_entropy_host(data.ctypes.data, data.size, frames.ctypes.data, segs.ctypes.data, segs.shape[0], tables.ctypes.data,
                                      tables.shape[0], int(T), int(H), int(W), coef.ctypes.data, status.ctypes.data), "kvq_jpeg_entropy_host")
    return coef, status


def jpeg_entropy(data: torch.Tensor, frames: torch.Tensor, segs: torch.Tensor, tables: torch.Tensor, T: int, H: int, W: int,
                 coef: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None):
    """Compressed baseline-JPEG frames -> their quantised coefficients, one launch, one lane per restart interval
    (``kvq_jpeg_entropy``).  data uint8 (nbytes,): the images; frames int32 (T, 5): per frame {byte offset, first segment, nseg, restart
    interval, table set}; segs int32 (nsegs, 2): byte ranges relative to the frame's image; tables uint8 (ntables, JPEG_TABLES_BYTES);
    all on the device (the int32 tensors carry uint32 values) -> (coef int16 (T, jpeg_coef_bytes / 2), zero-filled by the entry,
    status int32 (nsegs,): 0 = the segment decoded).  Only enqueues: the caller reads ``status`` after the stream has reached it."""
    _need_gpu(data, frames, segs, tables, coef, status)
    assert data.dtype == torch.uint8 and frames.dtype == torch.int32 and segs.dtype == torch.int32 and tables.dtype == torch.uint8
    assert all(a.is_contiguous() for a in (data, frames, segs, tables)) and tuple(frames.shape) == (T, 5)
    assert segs.dim() == 2 and segs.shape[1] == 2 and tables.dim() == 2 and tables.shape[1] == JPEG_TABLES_BYTES
    n = jpeg_coef_bytes(H, W) // 2
    if coef is None:
        coef = torch.empty(T, n, dtype=torch.int16, device=data.device)
    if status is None:
        status = torch.empty(segs.shape[0], dtype=torch.int32, device=data.device)
    assert coef.dtype == torch.int16 and coef.is_contiguous() and coef.numel() == T * n
    assert status.dtype == torch.int32 and status.is_contiguous() and status.numel() == segs.shape[0]
    check(lib().kvq_jpeg_entropy(ptr(data), data.numel(), ptr(frames), ptr(segs), segs.shape[0], ptr(tables), tables.shape[0], int(T), int(H),
                                 int(W), ptr(coef), ptr(status), stream_of(data)), "kvq_jpeg_entropy")
    return coef, status


def jpeg_quant_tables(quality: int):
    """uint16 (3, 64) numpy: the Y, Cb, Cr quantiser tables of an IJG quality 1..100, natural order (``kvq_jpeg_quant_tables``)"""
    import numpy as np
    out = np.empty((3, 64), np.uint16)
    check(lib().kvq_jpeg_quant_tables(int(quality), out.ctypes.data), "kvq_jpeg_quant_tables")
    return out


def jpeg_quantise_host(F, q: int):
    """the quantiser of csrc/jpeg_fdct.hpp on a numpy array of DCT outputs (|F| <= 32767), q in 1..255 -> int16 (``kvq_jpeg_quantise_host``)"""
    import numpy as np
    F = np.ascontiguousarray(F, np.int32)
    out = np.empty(F.shape, np.int16)
    check(lib().kvq_jpeg_quantise_host(F.ctypes.data, F.size, int(q), out.ctypes.data), "kvq_jpeg_quantise_host")
    return out


def _jpeg_qt_frames(qt, T: int):
    """(3, 64) tables for every frame, or (T, 3, 64) -> (T, 3, 64)"""
    if qt.numel() == 192 and T > 1:                     # copied as int16: the copy kernels know every signed type
        return qt.contiguous().view(torch.int16).reshape(1, 3, 64).expand(T, 3, 64).contiguous().view(torch.uint16)
    return qt.contiguous().reshape(T, 3, 64)


def jpeg_fdct_host(src, qt, H: int, W: int, src_format: int = _abi.SRC_U8):
    """the scalar twin of ``jpeg_fdct`` on numpy arrays: src uint8 (3, T, H, W) (``SRC_U8``) or (T, i420_frame_bytes)
    (``SRC_I420_BT601_FULL``), qt uint16 (T, 3, 64) or (3, 64) -> int16 (T, jpeg_coef_bytes / 2)"""
    import numpy as np
    src = np.ascontiguousarray(src, np.uint8)
    T = src.shape[1] if src_format == _abi.SRC_U8 else src.shape[0]
    assert src.size == (3 * T * H * W if src_format == _abi.SRC_U8 else T * i420_frame_bytes(H, W)), (src.shape, T, H, W, src_format)
    qt = np.ascontiguousarray(np.broadcast_to(np.asarray(qt, np.uint16).reshape(-1, 3, 64), (T, 3, 64)))
    out = np.empty((T, jpeg_coef_bytes(H, W) // 2), np.int16)
    check(lib().kvq_jpeg_fdct_host(src.ctypes.data, int(src_format), T, int(H), int(W), qt.ctypes.data, out.ctypes.data), "kvq_jpeg_fdct_host")
    return out


def jpeg_fdct(frames, qt: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Frames -> quantised JPEG coefficients, one launch (``kvq_jpeg_fdct``): the input of ``jpeg_encode`` and of ``jpeg_idct_i420``.
    frames: a device uint8 (3, T, H, W) tensor (R G B) or ``I420Frames`` of format ``SRC_I420_BT601_FULL`` (anything else: convert
    with ``to_rgb()``); qt uint16 (T, 3, 64) or (3, 64) on the device -> int16 (T, jpeg_coef_bytes / 2)."""
    i420 = isinstance(frames, I420Frames)
    data = frames.data if i420 else frames
    _need_gpu(data, qt)
    if i420 and frames.format != _abi.SRC_I420_BT601_FULL:
        raise ValueError(f"jpeg_fdct: I420Frames of format {frames.format}; JFIF fixes BT.601 full range — convert with to_rgb() first")
    assert data.dtype == torch.uint8 and data.is_contiguous() and len(frames.shape) == 4 and frames.shape[0] == 3, (data.dtype, tuple(frames.shape))
    _, T, H, W = frames.shape
    assert qt.dtype == torch.uint16 and qt.numel() in (192, 192 * T), (qt.dtype, tuple(qt.shape))
    qt = _jpeg_qt_frames(qt, T)
    n = jpeg_coef_bytes(H, W) // 2
    if out is None:
        out = torch.empty(T, n, dtype=torch.int16, device=data.device)
    else:
        assert out.dtype == torch.int16 and tuple(out.shape) == (T, n) and out.is_contiguous() and out.device == data.device
    check(lib().kvq_jpeg_fdct(ptr(data), _frame_format(frames), T, H, W, ptr(qt), ptr(out), stream_of(data)), "kvq_jpeg_fdct")
    return out


def jpeg_encode_bound(H: int, W: int) -> int:
    """a capacity that holds any frame of H x W written by ``jpeg_encode`` (``kvq_jpeg_encode_bound``)"""
    n = lib().kvq_jpeg_encode_bound(int(H), int(W))
    if n == 0:
        raise ValueError(f"jpeg_encode_bound: a frame of {W} x {H} is outside what the library encodes")
    return n


def jpeg_encode(coef, qt, H: int, W: int, restart_interval: int = 0, dht: bool = True, out=None):
    """``kvq_jpeg_encode`` (host only): one frame's coefficients, int16 numpy (jpeg_coef_bytes / 2,), and its tables uint16 (3, 64) ->
    the baseline JFIF image as a uint8 numpy view of ``out`` (a uint8 numpy buffer; None: a new one of ``jpeg_encode_bound``).
    ``dht=False`` leaves the Huffman tables out (AVI "MJPG" frames).  The ctypes call releases the GIL."""
    import numpy as np
    assert coef.dtype == np.int16 and coef.flags.c_contiguous and coef.size * 2 == jpeg_coef_bytes(H, W), (coef.dtype, coef.shape, H, W)
    assert qt.dtype == np.uint16 and qt.flags.c_contiguous and qt.size == 192, (qt.dtype, qt.shape)
    if out is None:
        out = np.empty(jpeg_encode_bound(H, W), np.uint8)
    n = C.c_size_t(0)
    check(lib().kvq_jpeg_encode(coef.ctypes.data, qt.ctypes.data, int(H), int(W), int(restart_interval), 0 if dht else _abi.JPEG_NO_DHT,
                                out.ctypes.data, out.size, C.byref(n)), "kvq_jpeg_encode")
    return out[:n.value]


def jpeg_encode_header(qt, H: int, W: int, restart_interval: int = 0, dht: bool = True):
    """``kvq_jpeg_encode_header`` (host only): the bytes ``jpeg_encode`` writes in front of the scan, SOI .. SOS, as a uint8 numpy array.
    An image is this + its scan (``jpeg_encode_scans``) + FF D9."""
    import numpy as np
    assert qt.dtype == np.uint16 and qt.flags.c_contiguous and qt.size == 192, (qt.dtype, qt.shape)
    out = np.empty(1024, np.uint8)
    n = C.c_size_t(0)
    check(lib().kvq_jpeg_encode_header(qt.ctypes.data, int(H), int(W), int(restart_interval), 0 if dht else _abi.JPEG_NO_DHT, out.ctypes.data,
                                       out.size, C.byref(n)), "kvq_jpeg_encode_header")
    return out[:n.value].copy()


# ``jpeg_encode_scans`` without ``cap``: room for the scans of 1 / JPEG_SCANS_FRACTION of the coefficient bytes = 32 bytes per block
# (q90 1080p takes about 14, the worst case is 208)
JPEG_SCANS_FRACTION = 4
JPEG_SCAN_OK, JPEG_SCAN_RANGE, JPEG_SCAN_CAPACITY = 0, 1, 2


def jpeg_scans_workspace_bytes(T: int, H: int, W: int) -> int:
    """workspace of ``jpeg_encode_scans`` for T frames of H x W (``kvq_jpeg_scans_workspace_bytes``): 12 bytes per block, 24 per frame"""
    n = lib().kvq_jpeg_scans_workspace_bytes(int(T), int(H), int(W))
    if n == 0:
        raise ValueError(f"jpeg_scans_workspace_bytes: {T} frames of {W} x {H} are outside what the library encodes")
    return n


def _aligned16(n: int, dtype):
    """a numpy array of n elements whose data is 16-byte aligned"""
    import numpy as np
    item = np.dtype(dtype).itemsize
    raw = np.empty(n * item + 16, np.uint8)
    o = (-raw.ctypes.data) % 16
    return raw[o:o + n * item].view(dtype)


def jpeg_encode_scans_host(coef, H: int, W: int, restart_interval: int = 0, cap: Optional[int] = None, workspace_bytes: Optional[int] = None):
    """the host twin of ``jpeg_encode_scans`` on numpy arrays (``kvq_jpeg_encode_scans_host``): coef int16 (T, jpeg_coef_bytes / 2) ->
    (out uint8 (cap,), frames uint32 (T, 3)); equal to the launch in every byte of out[:total] and every word of frames"""
    import numpy as np
    n = jpeg_coef_bytes(H, W) // 2
    coef = np.ascontiguousarray(coef, np.int16).reshape(-1, n)
    T = coef.shape[0]
    if coef.ctypes.data % 16:
        a = _aligned16(coef.size, np.int16).reshape(coef.shape)
        a[...] = coef
        coef = a
    cap = coef.nbytes // JPEG_SCANS_FRACTION if cap is None else int(cap)
    if workspace_bytes is None:
        workspace_bytes = jpeg_scans_workspace_bytes(T, H, W)
    out, frames, ws = np.empty(max(cap, 1), np.uint8), np.empty((T, 3), np.uint32), _aligned16(max(int(workspace_bytes), 1), np.uint8)
    check(lib().kvq_jpeg_encode_scans_host(coef.ctypes.data, T, int(H), int(W), int(restart_interval), out.ctypes.data, cap, frames.ctypes.data,
                                           ws.ctypes.data, int(workspace_bytes)), "kvq_jpeg_encode_scans_host")
    return out[:cap], frames


def jpeg_encode_scans(coef: torch.Tensor, H: int, W: int, restart_interval: int = 0, cap: Optional[int] = None,
                      workspace: Optional[torch.Tensor] = None):
    """Quantised coefficients -> the frames' entropy-coded scans, one lane per 8 x 8 block (``kvq_jpeg_encode_scans``): what ``jpeg_encode``
    writes between its SOS header and its FF D9, packed back to back.  coef: device int16 (T, jpeg_coef_bytes / 2) as ``jpeg_fdct`` writes
    it -> (out uint8 (cap,), frames int32 (T, 3): per frame {offset, length, status}, uint32 values; status ``JPEG_SCAN_OK``, ``_RANGE`` (a
    coefficient baseline cannot code: ``jpeg_encode`` names it), ``_CAPACITY`` (offset + length of the last frame is the ``cap`` that is
    enough)), both on the device.  ``cap`` defaults to 1 / ``JPEG_SCANS_FRACTION`` of the coefficient bytes; ``workspace``: a device
    uint8 tensor of ``jpeg_scans_workspace_bytes``.  Only
    enqueues: the caller reads ``frames`` after the stream has reached it."""
    _need_gpu(coef, workspace)
    n = jpeg_coef_bytes(H, W) // 2
    assert coef.dtype == torch.int16 and coef.is_contiguous() and coef.numel() % n == 0 and coef.numel() > 0, (coef.dtype, tuple(coef.shape), H, W)
    T = coef.numel() // n
    cap = coef.numel() * 2 // JPEG_SCANS_FRACTION if cap is None else int(cap)
    if workspace is None:
        workspace = torch.empty(jpeg_scans_workspace_bytes(T, H, W), dtype=torch.uint8, device=coef.device)
    assert workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == coef.device
    out = torch.empty(max(cap, 1), dtype=torch.uint8, device=coef.device)
    frames = torch.empty(T, 3, dtype=torch.int32, device=coef.device)
    check(lib().kvq_jpeg_encode_scans(ptr(coef), T, int(H), int(W), int(restart_interval), ptr(out), cap, ptr(frames), ptr(workspace),
                                      workspace.numel(), stream_of(coef)), "kvq_jpeg_encode_scans")
    return out[:cap], frames


def _frame_format(v) -> int:
    """KvqSrcFormat of a frame tensor / ``I420Frames``"""
    return v.format if isinstance(v, I420Frames) else int(v.dtype == torch.uint8)


def fragment_gather(video, hoff: torch.Tensor, woff: torch.Tensor, fragments_h, fragments_w,
                    fsize_h, fsize_w, aligned, mean=None, std=None, out=None):
    """video uint8/fp32 (C,T,H,W) on device, or ``I420Frames``; hoff/woff int32 (Fh,Fw,T//aligned) ABSOLUTE patch origins.
    ``out``: optional fp32 (C,T,Fh*fs,Fw*fs) destination (e.g. one clip of a batch tensor) — no allocation, no copy."""
    _need_gpu(video, hoff, woff)
    assert video.dtype in (torch.uint8, torch.float32) and video.is_contiguous()
    Cc, T, H, W = video.shape
    shape = (Cc, T, fragments_h * fsize_h, fragments_w * fsize_w)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=video.device)
    else:
        assert tuple(out.shape) == shape and out.dtype == torch.float32 and out.is_contiguous() and out.device == video.device
    m = (C.c_float * Cc)(*mean) if mean is not None else None
    s = (C.c_float * Cc)(*std) if std is not None else None
    hoff, woff = hoff.contiguous(), woff.contiguous()
    check(lib().kvq_fragment_gather(ptr(video), _frame_format(video), Cc, T, H, W, ptr(hoff), ptr(woff),
                                    fragments_h, fragments_w, fsize_h, fsize_w, aligned, m, s, ptr(out),
                                    stream_of(video)), "kvq_fragment_gather")
    return out


class FragmentSource:
    """A batch of technical-branch clips that is still (decoded uint8 frames, sampler draws): the arguments ``fragment_gather``
    would get, clip by clip.  ``SwinTransformer3D.forward`` reads its patch-embedding operand straight out of it (K1 fused
    into the embedding launch: the fp32 clip is neither written nor read back); ``materialise()`` is the two-step form, for
    consumers that want the tensor.  Bit-identical either way.

    videos: uint8 (C,T,Hs,Ws) device tensors of one shape — contiguous, or runs of frames of a longer video (frames
    contiguous, one common channel stride: what ``split_clips`` makes) — or ``I420Frames`` of one frame size and format (YUV
    4:2:0 as the decoder left it: the pixels a launch touches are converted in its registers); hoffs / woffs: int32 (Fh,Fw,T//aligned) device tensors
    of ABSOLUTE patch origins (as ``fragment_gather``)."""

    def __init__(self, videos, hoffs, woffs, fragments_h, fragments_w, fsize_h, fsize_w, aligned, mean=None, std=None):
        videos, hoffs, woffs = list(videos), [h.contiguous() for h in hoffs], [w.contiguous() for w in woffs]
        assert len(videos) == len(hoffs) == len(woffs) and 0 < len(videos)
        _need_gpu(*videos, *hoffs, *woffs)
        v0 = videos[0]
        Cc, T, Hs, Ws = v0.shape
        nt = T // aligned
        # frame_format: KvqSrcFormat; frame_stride: elements between the channel planes (0 for I420: there are none)
        self.frame_format = _frame_format(v0)
        self.frame_stride = 0 if isinstance(v0, I420Frames) else v0.stride(0)
        for v, h, w in zip(videos, hoffs, woffs):
            assert v.shape == v0.shape and v.dtype == v0.dtype and v.device == v0.device and _frame_format(v) == self.frame_format
            if not isinstance(v0, I420Frames):
                assert v.stride()[1:] == (Hs * Ws, Ws, 1) and v.stride(0) == v0.stride(0) >= T * Hs * Ws, "frames must be contiguous"
            assert h.dtype == w.dtype == torch.int32 and tuple(h.shape) == tuple(w.shape) == (fragments_h, fragments_w, nt)
        assert (mean is None) == (std is None)
        self.videos, self.hoffs, self.woffs = videos, hoffs, woffs
        self.geometry = (fragments_h, fragments_w, fsize_h, fsize_w, aligned)
        self.mean, self.std = mean, std
        self.device, self.is_cuda, self.dtype = v0.device, True, torch.float32
        self.shape = (len(videos), Cc, T, fragments_h * fsize_h, fragments_w * fsize_w)
        # True: the frames are the sampler's bilinear upsample of a source smaller than the canvas, read at the SMALL source's
        # offsets (fusion_datasets.py:43-50) — the draws no longer name pixels of the video itself (quality_paint's caller asks)
        self.upsampled = False
        self._c = None

    @staticmethod
    def cat(sources):
        """the batch of several sources (same geometry / normalisation), in order"""
        s0 = sources[0]
        assert all(s.geometry == s0.geometry and s.mean == s0.mean and s.std == s0.std for s in sources)
        out = FragmentSource([v for s in sources for v in s.videos], [h for s in sources for h in s.hoffs],
                             [w for s in sources for w in s.woffs], *s0.geometry, mean=s0.mean, std=s0.std)
        out.upsampled = any(s.upsampled for s in sources)
        return out

    def split_clips(self, num_clips):
        """every T-frame entry as ``num_clips`` clips of T/num_clips consecutive frames — the harness's clip reshape
        (trainer.py:306-319: (b,c,nc*t,h,w) -> (b*nc,c,t,h,w)) without moving a byte: the clips are views of the frames."""
        if num_clips == 1:
            return self
        _, _, T, _, _ = self.shape
        aligned = self.geometry[4]
        assert T % num_clips == 0 and (T // num_clips) % aligned == 0, "a clip must hold whole aligned frame groups"
        t, nt = T // num_clips, T // num_clips // aligned
        vs, hs, ws = [], [], []
        for v, h, w in zip(self.videos, self.hoffs, self.woffs):
            for k in range(num_clips):
                vs.append(v.frames(k * t, (k + 1) * t) if isinstance(v, I420Frames) else v[:, k * t:(k + 1) * t])
                hs.append(h[:, :, k * nt:(k + 1) * nt])
                ws.append(w[:, :, k * nt:(k + 1) * nt])
        out = FragmentSource(vs, hs, ws, *self.geometry, mean=self.mean, std=self.std)
        out.upsampled = self.upsampled
        return out

    def record_stream(self, stream):
        for t in self.videos + self.hoffs + self.woffs:
            t.record_stream(stream)

    def c_struct(self, any_dtype=False):
        """KvqFragmentSource, or None when the batch has more clips than the struct holds / the frames are not uint8 (the fused
        read; ``any_dtype``: fp32 frames too — the batched gather takes them)."""
        v0 = self.videos[0]
        if len(self.videos) > _abi.FRAG_MAX_CLIPS or (v0.dtype != torch.uint8 and not any_dtype):
            return None
        if self._c is not None:
            return self._c
        f = _abi.KvqFragmentSource()
        for i, (v, h, w) in enumerate(zip(self.videos, self.hoffs, self.woffs)):
            f.video[i], f.hoff[i], f.woff[i] = ptr(v), ptr(h), ptr(w)
        f.chan_stride = self.frame_stride
        f.n_clips, f.src_is_u8, f.Hs, f.Ws = len(self.videos), self.frame_format, v0.shape[2], v0.shape[3]
        f.Fh, f.Fw, f.fs_h, f.fs_w, f.aligned = self.geometry
        f.normalise = int(self.mean is not None)
        if self.mean is not None:
            for c in range(v0.shape[0]):
                f.mean[c], f.std[c] = self.mean[c], self.std[c]
        self._c = f
        return f

    def pointer_table(self):
        """the batch's device pointers as the table ``KvqFragmentSource.indirect`` names: int64 [3 * 16] = video | hoff | woff,
        on the device (made once; what a ``FragmentSlot`` is loaded from)"""
        if getattr(self, "_table", None) is None:
            n = _abi.FRAG_MAX_CLIPS
            assert len(self.videos) <= n
            host = torch.zeros(3 * n, dtype=torch.int64)
            for i, (v, h, w) in enumerate(zip(self.videos, self.hoffs, self.woffs)):
                host[i], host[n + i], host[2 * n + i] = ptr(v), ptr(h), ptr(w)
            self._table = host.to(self.device)
        return self._table

    def materialise(self, out=None):
        """the fp32 (B,C,T,H,W) batch: ``kvq_fragment_gather_batch`` — one launch for up to 16 clips (views included), else one
        ``fragment_gather`` per clip"""
        if out is None:
            out = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        assert tuple(out.shape) == tuple(self.shape) and out.dtype == torch.float32 and out.is_contiguous()
        f = self.c_struct(any_dtype=True)
        if f is not None:
            check(lib().kvq_fragment_gather_batch(C.byref(f), self.shape[1], self.shape[2], ptr(out), current_stream()),
                  "kvq_fragment_gather_batch")
            return out
        for b, (v, h, w) in enumerate(zip(self.videos, self.hoffs, self.woffs)):
            fragment_gather(v.contiguous(), h, w, *self.geometry, mean=self.mean, std=self.std, out=out[b])
        return out


class FragmentSlot(FragmentSource):
    """A ``FragmentSource`` whose per-video addresses live in a 384-byte DEVICE table instead of the launch parameters
    (``KvqFragmentSource.indirect``): a forward recorded into a hipGraph through a slot serves every later batch of the same
    geometry — ``load(source)`` rewrites the table on the current stream (one small device-to-device copy) in front of the replay.
    Same kernels, same arithmetic: scores are bit-identical to the forward on the source itself."""

    def __init__(self, source: FragmentSource):
        if not (type(source) is FragmentSource and source.c_struct() is not None):
            raise ValueError("FragmentSlot: uint8 or I420 frames, at most 16 clips")
        self.geometry, self.mean, self.std = source.geometry, source.mean, source.std
        self.device, self.is_cuda, self.dtype, self.shape = source.device, True, source.dtype, source.shape
        self._frame_shape, self._frame_stride, self.frame_format = tuple(source.videos[0].shape), source.frame_stride, source.frame_format
        self.frame_stride = self._frame_stride
        self.upsampled = source.upsampled
        self.table = torch.zeros(3 * _abi.FRAG_MAX_CLIPS, dtype=torch.int64, device=self.device)
        self._c = None
        self.load(source)

    def load(self, source: FragmentSource):
        """point the slot at ``source`` (same geometry, frame shape, frame format and normalisation), in stream order"""
        if not (source.geometry == self.geometry and source.shape == self.shape and source.mean == self.mean and source.std == self.std
                and tuple(source.videos[0].shape) == self._frame_shape and source.frame_stride == self._frame_stride
                and source.frame_format == self.frame_format and source.upsampled == self.upsampled):
            # a real exception (not an assert: python -O must not replay a graph recorded with other constants)
            raise ValueError("FragmentSlot.load: a slot serves one sampler geometry, frame shape / stride, frame format and one "
                             f"normalisation; got geometry {source.geometry} frames {tuple(source.videos[0].shape)} {source.videos[0].dtype} "
                             f"format {source.frame_format} (the slot's: {self.frame_format})")
        self.table.copy_(source.pointer_table(), non_blocking=True)
        self.current = source                      # keeps the frames alive while the table names them
        self.videos, self.hoffs, self.woffs = source.videos, source.hoffs, source.woffs

    def release(self, stream=None):
        """drop the slot's reference to the loaded source once the launch that reads it has been ENQUEUED on ``stream``: the caching
        allocator keeps the frames' memory until that stream passes this point (record_stream), the Python objects go now"""
        cur = getattr(self, "current", None)
        if cur is None:
            return
        if stream is not None:
            cur.record_stream(stream)
            tab = getattr(cur, "_table", None)
            if tab is not None:
                tab.record_stream(stream)
        self.current = None
        self.videos = self.hoffs = self.woffs = None

    def c_struct(self, any_dtype=False):
        if self._c is None:
            f = _abi.KvqFragmentSource()
            f.chan_stride = self._frame_stride
            f.n_clips, f.src_is_u8, f.Hs, f.Ws = self.shape[0], self.frame_format, self._frame_shape[2], self._frame_shape[3]
            f.Fh, f.Fw, f.fs_h, f.fs_w, f.aligned = self.geometry
            f.normalise = int(self.mean is not None)
            if self.mean is not None:
                for c in range(self._frame_shape[0]):
                    f.mean[c], f.std[c] = self.mean[c], self.std[c]
            f.indirect = ptr(self.table)
            self._c = f
        return self._c

    def materialise(self, out=None):
        # the two-step form reads the loaded source's own addresses: inside a recording that would freeze THIS video's pointers
        # into the graph, so a forward that cannot take the fused read fails its capture (LaneGraphs then runs it eagerly)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FragmentSlot.materialise() inside a hipGraph capture: this forward does not read the batch through the sampler")
        if getattr(self, "current", None) is None:
            raise RuntimeError("FragmentSlot.materialise(): no source loaded (load() one first)")
        return self.current.materialise(out)

    def split_clips(self, num_clips):
        assert num_clips == 1, "split the source, then load it"
        return self


PAINT_CELLS = (1, 2, 4, 8, 16, 32)


def quality_paint_supported(source, token_grid, cell=8) -> bool:
    """``kvq_quality_paint_supported`` for a ``FragmentSource`` / ``FragmentSlot`` and a token grid (D, Hf, Wf): host only"""
    f = source.c_struct(any_dtype=True)
    if f is None:
        return False
    D, Hf, Wf = (int(v) for v in token_grid)
    return bool(lib().kvq_quality_paint_supported(C.byref(f), source.shape[2], D, Hf, Wf, int(cell)))


def _paint_args(who, a, source, tok_map, cell, overlay_depths, value_range, alpha, dim):
    """fill a ``KvqQualityPaintArgs`` and allocate the outputs: (tensors the call must outlive, heat, cover, overlay or None)"""
    _need_gpu(tok_map)
    assert tok_map.dtype == torch.float32 and tok_map.dim() == 4
    tok_map = tok_map.contiguous()
    n, D, Hf, Wf = tok_map.shape
    f = source.c_struct(any_dtype=True)
    if f is None or n != source.shape[0]:
        raise _abi.KvqError(f"{who}: {n} token maps for a source of {source.shape[0]} clips (at most {_abi.FRAG_MAX_CLIPS})")
    Hs, Ws = f.Hs, f.Ws
    if cell not in PAINT_CELLS:
        raise _abi.KvqError(f"{who}: cell {cell} is not one of {PAINT_CELLS}")
    Ho, Wo = -(-Hs // cell), -(-Ws // cell)
    dev = tok_map.device
    heat = torch.empty(n, D, Ho, Wo, dtype=torch.float32, device=dev)
    cover = torch.empty(n, D, Ho, Wo, dtype=torch.float32, device=dev)
    a.src = C.pointer(f)
    a.T, a.D, a.Hf, a.Wf, a.cell = source.shape[2], D, Hf, Wf, cell
    a.tok_map, a.heat, a.cover = ptr(tok_map), ptr(heat), ptr(cover)
    overlay = rng = None
    depths = [int(d) for d in overlay_depths]
    if depths:
        if len(depths) > 16:
            raise _abi.KvqError(f"{who}: at most 16 overlay slices per call")
        if value_range is None:
            lo, hi = torch.aminmax(tok_map)
            rng = torch.stack((lo, hi))
        elif torch.is_tensor(value_range):
            rng = value_range.to(device=dev, dtype=torch.float32).contiguous()
        else:
            rng = torch.tensor([float(value_range[0]), float(value_range[1])], dtype=torch.float32).to(dev, non_blocking=True)
        assert rng.numel() == 2
        overlay = torch.empty(n, len(depths), 3, Hs, Ws, dtype=torch.uint8, device=dev)
        a.overlay, a.range, a.n_ov, a.alpha, a.dim = ptr(overlay), ptr(rng), len(depths), int(alpha), int(dim)
        for i, d in enumerate(depths):
            a.ov_depth[i] = d
    return (tok_map, rng, f), heat, cover, overlay


def quality_paint(source, tok_map: torch.Tensor, cell=8, overlay_depths=(), value_range=None, alpha=128, dim=96):
    """The token map of a forward that read ``source`` (a ``FragmentSource`` or a ``FragmentSlot``), painted onto the geometry of the
    source frames (``kvq_quality_paint``): ``tok_map`` fp32 (n_clips, D, Hf, Wf) -> ``(heat, cover)`` fp32
    (n_clips, D, ceil(Hs/cell), ceil(Ws/cell)), and with ``overlay_depths`` also ``overlay`` uint8 (n_clips, n_ov, 3, Hs, Ws): the
    frames 2 * depth of each clip blended with the red-to-green colour of the scores over ``value_range`` = (lo, hi) — floats, a
    device float[2], or None = the map's own minimum and maximum, taken on the device without a host read.  Geometries the paint
    does not cover raise ``KvqError``.  Through a slot the launch reads the pointer table: it can be recorded into a graph."""
    a = _abi.KvqQualityPaintArgs()
    keep, heat, cover, overlay = _paint_args("quality_paint", a, source, tok_map, cell, overlay_depths, value_range, alpha, dim)
    check(lib().kvq_quality_paint(C.byref(a), stream_of(tok_map)), "kvq_quality_paint")
    del keep
    return (heat, cover) if overlay is None else (heat, cover, overlay)


def quality_paint_regions_supported(source, token_grid, anchor, kh, kw, cell=8) -> bool:
    """``kvq_quality_paint_regions_supported`` for a ``FragmentSource`` / ``FragmentSlot``, a token grid (D, Hf, Wf) and windows of
    ``kh`` x ``kw`` anchors of ``anchor`` canvas pixels: host only"""
    f = source.c_struct(any_dtype=True)
    if f is None:
        return False
    D, Hf, Wf = (int(v) for v in token_grid)
    return bool(lib().kvq_quality_paint_regions_supported(C.byref(f), source.shape[2], D, Hf, Wf, int(cell), int(anchor), int(kh), int(kw)))


def quality_paint_regions(source, tok_map: torch.Tensor, region: torch.Tensor, anchor, kh, kw, phase=0, cell=8, overlay_depths=(),
                          value_range=None, alpha=128, dim=96):
    """``quality_paint`` for a trunk that saw one window of ``source``'s fragment canvas per clip frame (KSVQE's region selection,
    ``kvq_quality_paint_regions``): ``region`` int32 (n_clips, T) on the device, the window index of every clip frame as
    ``qrs_top_region`` returns it (``KSVQE.last_regions``), windows of ``kh`` x ``kw`` anchors of ``anchor`` canvas pixels.  Depth
    slice d is painted with the window of clip frame 2d + ``phase`` (0 or 1: the two frames of a token can lie in different key-frame
    groups) and overlays are drawn on that frame.  A region value that names no window leaves its slice uncovered.  Same returns
    as ``quality_paint``."""
    _need_gpu(region)
    n, T = tok_map.shape[0], source.shape[2]
    if region.dtype != torch.int32 or tuple(region.shape) != (n, T) or region.device != tok_map.device:
        raise _abi.KvqError(f"quality_paint_regions: region must be int32 ({n}, {T}) on the map's device, got {region.dtype} {tuple(region.shape)}")
    region = region.contiguous()
    r = _abi.KvqQualityPaintRegionArgs()
    keep, heat, cover, overlay = _paint_args("quality_paint_regions", r.paint, source, tok_map, cell, overlay_depths, value_range, alpha, dim)
    r.region, r.anchor, r.kh, r.kw, r.phase = ptr(region), int(anchor), int(kh), int(kw), int(phase)
    check(lib().kvq_quality_paint_regions(C.byref(r), stream_of(tok_map)), "kvq_quality_paint_regions")
    del keep
    return (heat, cover) if overlay is None else (heat, cover, overlay)


# ------------------------------------------------------------------------------------------------
# convolution front-ends (channels-last 16-bit activations (B,D,H,W,C))
# ------------------------------------------------------------------------------------------------
def _i32x(vals):
    return (C.c_int32 * len(vals))(*[int(v) for v in vals])


def conv_out_dims(dims, kernel, stride, pad):
    return tuple((d + 2 * p - k) // s + 1 for d, k, s, p in zip(dims, kernel, stride, pad))


def im2col_nd(x: torch.Tensor, dims5, strides5, kernel, stride, pad, out_dtype, k_pad=None):
    """x: device tensor (fp32 network input or 16-bit activation) addressed through ELEMENT strides5 =
    (b,c,d,h,w) over dims5 = (B,C,D,H,W).  Returns ([B*Do*Ho*Wo, Kpad] 16-bit, (Do,Ho,Wo))."""
    _need_gpu(x)
    B, Cc, D, H, W = dims5
    Do, Ho, Wo = conv_out_dims((D, H, W), kernel, stride, pad)
    K = kernel[0] * kernel[1] * kernel[2] * Cc
    k_pad = -(-K // 32) * 32 if k_pad is None else k_pad
    out = torch.empty(B * Do * Ho * Wo, k_pad, dtype=out_dtype, device=x.device)
    st = (C.c_int64 * 5)(*[int(s) for s in strides5])
    check(lib().kvq_im2col_nd(ptr(x), int(x.dtype == torch.float32), dtype_code(out_dtype), C.byref(st),
                              C.byref(_i32x(dims5)), C.byref(_i32x(kernel)), C.byref(_i32x(stride)),
                              C.byref(_i32x(pad)), k_pad, ptr(out), current_stream()), "kvq_im2col_nd")
    return out, (Do, Ho, Wo)


def pack_channels_last8(x: torch.Tensor, dims5, strides5, out_dtype):
    """fp32 frames addressed through ELEMENT strides5 = (b,t,c,h,w) over dims5 = (B,T,C,H,W), C <= 8 -> 16-bit channels-last
    (B*T, H, W, 8) with the channels >= C zero (the implicit-GEMM operand of a stem conv)."""
    _need_gpu(x)
    assert x.dtype == torch.float32
    B, T, Cc, H, W = dims5
    out = torch.empty(B * T, H, W, 8, dtype=out_dtype, device=x.device)
    st = (C.c_int64 * 5)(*[int(s) for s in strides5])
    check(lib().kvq_pack_channels_last8(ptr(x), C.byref(_i32x(dims5)), C.byref(st), dtype_code(out_dtype), ptr(out),
                                        current_stream()), "kvq_pack_channels_last8")
    return out


def pool_nd(x: torch.Tensor, kernel, stride, pad, is_max: bool):
    """x (B,D,H,W,C) channels-last 16-bit, contiguous."""
    _need_gpu(x)
    assert x.dtype in HALF_TYPES and x.is_contiguous() and x.dim() == 5
    B, D, H, W, Cc = x.shape
    Do, Ho, Wo = conv_out_dims((D, H, W), kernel, stride, pad)
    out = torch.empty(B, Do, Ho, Wo, Cc, dtype=x.dtype, device=x.device)
    check(lib().kvq_pool_nd(ptr(x), dtype_code(x.dtype), C.byref(_i32x((B, Cc, D, H, W))), C.byref(_i32x(kernel)),
                            C.byref(_i32x(stride)), C.byref(_i32x(pad)), int(is_max), ptr(out), current_stream()),
          "kvq_pool_nd")
    return out


def slow_bottleneck(x: torch.Tensor, pack: torch.Tensor, ci: int, cout: int, out=None):
    """One identity residual block of SlowFast's slow pathway (res2) in one launch (csrc/slowneck.hip).  x (B,T,H,W,cin) channels-last
    16-bit; ``pack`` from ``models.backbones.slowfast_model.pack_slow_bottleneck``; ``out`` (B,T,H,W,C >= cout) receives channels 0..cout-1."""
    _need_gpu(x, pack)
    B, T, H, W, cin = x.shape
    assert x.is_contiguous() and x.dtype in HALF_TYPES
    assert pack.numel() == lib().kvq_slow_bottleneck_pack_bytes(cin, ci, cout) > 0, "block not built / wrong image size"
    if out is None:
        out = torch.empty(B, T, H, W, cout, dtype=x.dtype, device=x.device)
    assert tuple(out.shape[:4]) == (B, T, H, W) and out.is_contiguous() and out.dtype == x.dtype
    check(lib().kvq_slow_bottleneck(ptr(x), _i32x((B, T, H, W)), cin, ci, cout, ptr(pack), dtype_code(x.dtype), ptr(out), out.shape[4],
                                    stream_of(x)), "kvq_slow_bottleneck")
    return out


def fast_bottleneck(x: torch.Tensor, pack: torch.Tensor, ci: int, cout: int, projection: bool, stride: int = 1):
    """One residual block of SlowFast's fast pathway in one launch (csrc/bottleneck.hip).  x (B,T,H,W,cin) channels-last 16-bit,
    ``pack`` the uint8 image described in include/kvq_hip.h -> (B,T,ceil(H/stride),ceil(W/stride),cout)."""
    _need_gpu(x, pack)
    assert x.dtype in HALF_TYPES and x.is_contiguous() and x.dim() == 5 and pack.dtype == torch.uint8 and pack.is_contiguous()
    B, T, H, W, cin = x.shape
    assert pack.numel() == lib().kvq_fast_bottleneck_pack_bytes(cin, ci, cout, int(projection), stride) > 0, "block not built / wrong image size"
    out = torch.empty(B, T, -(-H // stride), -(-W // stride), cout, dtype=x.dtype, device=x.device)
    check(lib().kvq_fast_bottleneck(ptr(x), _i32x((B, T, H, W)), cin, ci, cout, int(projection), stride, ptr(pack), dtype_code(x.dtype),
                                    ptr(out), stream_of(x)), "kvq_fast_bottleneck")
    return out


def mean_std_pool(x: torch.Tensor, out: torch.Tensor, mean_off: int, std_off: int):
    """x 16-bit [rows, HW, C]; writes fp32 mean/unbiased-std into out[row, mean_off:+C] / out[row, std_off:+C]."""
    _need_gpu(x, out)
    assert x.dtype in HALF_TYPES and x.is_contiguous() and out.dtype == torch.float32 and out.stride(-1) == 1
    rows, HW, Cc = x.shape
    check(lib().kvq_mean_std_pool(ptr(x), dtype_code(x.dtype), rows, HW, Cc, ptr(out), out.stride(0), mean_off, std_off,
                                  current_stream()), "kvq_mean_std_pool")
    return out


def conv_gemm(A: torch.Tensor, W: torch.Tensor, bias, relu: bool, resid=None, resid_f32=None, want_f32=False, out=None, ldc=0,
              col_off=0):
    """out[M,N] = (relu)(A @ W^T + bias (+ resid)), 16-bit operands.  ``resid`` 16-bit / ``resid_f32`` fp32
    identity branch (ReLU epilogue only).  Returns the 16-bit output, or (16-bit, fp32 copy) when
    ``want_f32`` — the fp32 copy keeps a residual stream un-rounded between blocks.  ``out`` [M, ldc] with ``ldc`` / ``col_off``:
    the N columns land at columns col_off .. col_off+N-1 of it (a channel concatenation)."""
    _need_gpu(A, W, bias, resid, resid_f32, out)
    M, N = A.shape[0], W.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=A.dtype, device=A.device)
    assert out.dtype == A.dtype and out.is_contiguous() and out.numel() >= M * N
    out32 = torch.empty(M, N, dtype=torch.float32, device=A.device) if want_f32 else None
    a = _abi.KvqGemmArgs()
    a.A, a.W, a.bias, a.M, a.N, a.K = ptr(A), ptr(W), ptr(bias), M, N, A.shape[1]
    a.epilogue = _abi.EPI_RELU_BF16 if relu else _abi.EPI_BIAS_BF16
    assert relu or (resid is None and resid_f32 is None and not want_f32), "identity add / fp32 copy: ReLU epilogue only"
    a.out_bf16, a.out_f32, a.resid_bf16, a.resid_f32 = ptr(out), ptr(out32), ptr(resid), ptr(resid_f32)
    a.ldc, a.col_off = _concat_dest(out, M, ldc, col_off)
    a.dtype = dtype_code(A.dtype)
    _ws = _splitk_scratch(a, a.M, a.N, a.K, A.device) if a.epilogue != _abi.EPI_QKV_BF16 else None   # noqa: F841
    check(lib().kvq_gemm_bf16(C.byref(a), current_stream()), "kvq_gemm_bf16")
    return (out, out32) if want_f32 else out


def vit_embed_ln(tok: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, ln_w, ln_b, B: int, eps=1e-5):
    """tok fp32 [B*G, D] (patch embeddings), cls [D], pos [1+G, D] -> LN(concat(cls, tok) + pos): fp32 (B, 1+G, D)."""
    _need_gpu(tok, cls, pos, ln_w, ln_b)
    G, D = tok.shape[0] // B, tok.shape[1]
    assert tok.dtype == torch.float32 and tok.is_contiguous() and pos.shape == (G + 1, D) and pos.is_contiguous()
    out = torch.empty(B, G + 1, D, dtype=torch.float32, device=tok.device)
    check(lib().kvq_vit_embed_ln(ptr(tok), ptr(cls), ptr(pos), ptr(ln_w), ptr(ln_b), B, G, D, eps, ptr(out), current_stream()),
          "kvq_vit_embed_ln")
    return out


def mha_small(qkv: torch.Tensor, B: int, L: int, heads: int):
    """qkv 16-bit [B*L, 3*D] (in_proj output, rows [q|k|v]) -> softmax(q k^T / sqrt(hd)) v, heads concatenated: [B*L, D]."""
    _need_gpu(qkv)
    assert qkv.dtype in HALF_TYPES and qkv.is_contiguous() and qkv.shape[0] == B * L and qkv.shape[1] % (3 * heads) == 0
    D = qkv.shape[1] // 3
    out = torch.empty(B * L, D, dtype=qkv.dtype, device=qkv.device)
    check(lib().kvq_mha_small(ptr(qkv), B, L, heads, D // heads, dtype_code(qkv.dtype), ptr(out), current_stream()), "kvq_mha_small")
    return out


def mha_cross(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, B: int, heads: int, scale: float):
    """q 16-bit [B*Lq, >= heads*64] / k, v [B*Lk, ...] (row-strided 2-D views allowed, last dim contiguous) ->
    softmax(scale q k^T) v per head: [B*Lq, heads*64]."""
    _need_gpu(q, k, v)
    for t in (q, k, v):
        assert t.dtype in HALF_TYPES and t.dim() == 2 and t.stride(1) == 1
    Lq, Lk, D = q.shape[0] // B, k.shape[0] // B, heads * 64
    out = torch.empty(B * Lq, D, dtype=q.dtype, device=q.device)
    check(lib().kvq_mha_cross(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), B, Lq, Lk, heads, 64,
                              scale, dtype_code(q.dtype), ptr(out), current_stream()), "kvq_mha_cross")
    return out


def to_half(x: torch.Tensor, out_dtype):
    """fp32 activation -> 16-bit MFMA operand (same shape)."""
    _need_gpu(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    check(lib().kvq_convert(ptr(x), ptr(out), x.numel(), 1, dtype_code(out_dtype), current_stream()), "kvq_convert")
    return out


def to_float(x: torch.Tensor):
    """16-bit activation -> fp32 (same shape)."""
    _need_gpu(x)
    assert x.dtype in HALF_TYPES and x.is_contiguous()
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(lib().kvq_convert(ptr(x), ptr(out), x.numel(), 0, dtype_code(x.dtype), current_stream()), "kvq_convert")
    return out


def sem_modulate(x: torch.Tensor, inp: torch.Tensor, w_gama, b_gama: float, w_beta, b_beta: float):
    """x, inp fp32 [M, C] token rows -> sigmoid(<w_gama, x_m> + b_gama) * inp_m + (<w_beta, x_m> + b_beta)."""
    _need_gpu(x, inp, w_gama, w_beta)
    assert x.dtype == torch.float32 and inp.dtype == torch.float32 and x.is_contiguous() and inp.is_contiguous() and x.shape == inp.shape
    out = torch.empty_like(inp)
    check(lib().kvq_sem_modulate(ptr(x), ptr(inp), ptr(w_gama), float(b_gama), ptr(w_beta), float(b_beta), x.shape[0], x.shape[1],
                                 ptr(out), current_stream()), "kvq_sem_modulate")
    return out


def dist_modulate(inp: torch.Tensor, gamma_logit: torch.Tensor, beta: torch.Tensor):
    """inp fp32 (B, rows, C); gamma_logit / beta 16-bit [B, C] -> sigmoid(gamma_logit)[:, None] * inp + beta[:, None]."""
    _need_gpu(inp, gamma_logit, beta)
    assert inp.dtype == torch.float32 and inp.is_contiguous() and gamma_logit.dtype in HALF_TYPES and beta.dtype == gamma_logit.dtype
    B, rows, Cc = inp.shape
    out = torch.empty_like(inp)
    check(lib().kvq_dist_modulate(ptr(inp), ptr(gamma_logit), ptr(beta), B, rows, Cc, dtype_code(beta.dtype), ptr(out),
                                  current_stream()), "kvq_dist_modulate")
    return out


def qrs_top_region(score: torch.Tensor, gh: int, gw: int, kh: int, kw: int):
    """score fp32 (BK, gs, gs) -> int32 [BK]: index of the kh x kw window of the (gh, gw)-upsampled map with the largest mean."""
    _need_gpu(score)
    assert score.dtype == torch.float32 and score.is_contiguous() and score.dim() == 3 and score.shape[1] == score.shape[2]
    idx = torch.empty(score.shape[0], dtype=torch.int32, device=score.device)
    check(lib().kvq_qrs_top_region(ptr(score), score.shape[0], score.shape[1], gh, gw, kh, kw, ptr(idx), current_stream()),
          "kvq_qrs_top_region")
    return idx


def crop_regions(x: torch.Tensor, region: torch.Tensor, anchor: int, kh: int, kw: int):
    """x fp32 (B, C, T, H, W), region int32 [B*T] -> (B, C, T, kh*anchor, kw*anchor): every frame's selected window."""
    _need_gpu(x, region)
    assert x.dtype == torch.float32 and x.is_contiguous() and region.dtype == torch.int32 and region.is_contiguous()
    B, Cc, T, H, W = x.shape
    out = torch.empty(B, Cc, T, kh * anchor, kw * anchor, dtype=torch.float32, device=x.device)
    check(lib().kvq_crop_regions(ptr(x), ptr(region), B, Cc, T, H, W, anchor, kh, kw, ptr(out), current_stream()), "kvq_crop_regions")
    return out


def l2_normalize_rows(x: torch.Tensor, out_dtype):
    """F.normalize(x, dim=1) of fp32 [M, D] -> 16-bit [M, D]."""
    _need_gpu(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
    out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    check(lib().kvq_l2_normalize_rows(ptr(x), x.shape[0], x.shape[1], dtype_code(out_dtype), ptr(out), current_stream()),
          "kvq_l2_normalize_rows")
    return out


def axpby(x: torch.Tensor, y: torch.Tensor, a: float, b: float):
    """a * x + b * y, fp32, same shape."""
    _need_gpu(x, y)
    assert x.dtype == torch.float32 and y.dtype == torch.float32 and x.is_contiguous() and y.is_contiguous() and x.shape == y.shape
    out = torch.empty_like(x)
    check(lib().kvq_axpby(ptr(x), ptr(y), float(a), float(b), ptr(out), x.numel(), current_stream()), "kvq_axpby")
    return out


def cls_gather(x: torch.Tensor, out_dtype):
    """x fp32 (B, L, D) -> x[:, 0] as 16-bit [B, D]."""
    _need_gpu(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 3
    B, L, D = x.shape
    out = torch.empty(B, D, dtype=out_dtype, device=x.device)
    check(lib().kvq_cls_gather(ptr(x), B, L, D, dtype_code(out_dtype), ptr(out), current_stream()), "kvq_cls_gather")
    return out


def cls_mix(x: torch.Tensor, a: torch.Tensor, ratio: float = 0.5):
    """In place: x[:, 0] = ratio * a + (1 - ratio) * x[:, 0]; x fp32 (B, L, D), a 16-bit [B, D]."""
    _need_gpu(x, a)
    assert x.dtype == torch.float32 and x.is_contiguous() and a.dtype in HALF_TYPES and a.is_contiguous()
    B, L, D = x.shape
    check(lib().kvq_cls_mix(ptr(x), ptr(a), B, L, D, ratio, dtype_code(a.dtype), current_stream()), "kvq_cls_mix")
    return x


def cosine_cls(x: torch.Tensor):
    """cosine similarity of x[:, 0] with x[:, 1:] along D: fp32 (B, L-1)."""
    _need_gpu(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 3
    B, L, D = x.shape
    out = torch.empty(B, L - 1, dtype=torch.float32, device=x.device)
    check(lib().kvq_cosine_cls(ptr(x), B, L, D, ptr(out), current_stream()), "kvq_cosine_cls")
    return out


_TAPS = {}


def live_taps(size, kernel, stride, pad):
    """Per axis, the kernel offsets that touch the image for at least one output position (the others only ever read
    padding): 3x3 / pad 1 on a 1x1 map keeps the centre tap, 3x3 / stride 2 / pad 1 on 2x2 keeps offsets {1, 2}."""
    out = []
    for n, k, s, p in zip(size, kernel, stride, pad):
        no = (n + 2 * p - k) // s + 1
        out.append([a for a in range(k) if any(0 <= o * s - p + a < n for o in range(no))])
    return out


def prune_conv_weight(W: torch.Tensor, kernel, Cc: int, live):
    """Columns of a (kd,kh,kw,c)-ordered [N][Kpad] conv weight that belong to the ``live`` taps, zero-padded to a multiple of 32."""
    kd, kh, kw = kernel
    n = W.shape[0]
    w = W[:, :kd * kh * kw * Cc].reshape(n, kd, kh, kw, Cc)
    idx = [torch.as_tensor(l, device=W.device) for l in live]
    w = w.index_select(1, idx[0]).index_select(2, idx[1]).index_select(3, idx[2]).reshape(n, -1)
    k = w.shape[1]
    out = torch.zeros(n, (k + 31) // 32 * 32, dtype=W.dtype, device=W.device)
    out[:, :k] = w
    return out


def conv_taps(kernel, Cc: int, H: int, W: int, k_pad: int, device, live=None):
    """Tap table of ``kvq_conv_implicit``: int32 [k_pad/8][4], one row per 8-channel chunk of the (kd,kh,kw,c)-ordered
    K axis: {kd, kh, kw, ((kd*H + kh)*W + kw)*C + c0}; -1 in the last column marks the zero padding of K.  ``live``:
    per-axis lists of the kernel offsets kept (``live_taps``), in which case K only spans those taps."""
    key = (tuple(kernel), Cc, H, W, k_pad, str(device), None if live is None else tuple(map(tuple, live)))
    t = _TAPS.get(key)
    if t is None:
        import numpy as np
        kd, kh, kw = kernel
        la, lb, lc = live if live is not None else (range(kd), range(kh), range(kw))
        rows = np.full((k_pad // 8, 4), -1, np.int32)
        q = 0
        for a in la:
            for b in lb:
                for c in lc:
                    for c0 in range(0, Cc, 8):
                        rows[q] = (a, b, c, ((a * H + b) * W + c) * Cc + c0)
                        q += 1
        rows[q:, :3] = 0
        t = _TAPS[key] = torch.from_numpy(rows).to(device)
    return t


TAP_TABLE = False      # test hook: True = always hand kvq_conv_implicit a tap table (tap walk vs table: bit-identical)


def conv_implicit(x: torch.Tensor, W: torch.Tensor, bias, kernel, stride, pad, relu: bool, resid=None, resid_f32=None,
                  want_f32=False, store_f32=False, live=None, out=None, ldc=0, col_off=0):
    """Conv (+ folded BN, + identity, + ReLU) on a channels-last 16-bit activation x (B, D, H, W, C), C % 8 == 0, without a
    patch matrix: W [N][Kpad] with the (kd,kh,kw,c) column order of ``im2col_nd``.  Returns the (B, Do, Ho, Wo, N) 16-bit
    output, or (output, fp32 copy [M][N]) when ``want_f32``; ``store_f32``: only the fp32 [M][N] result (no ReLU).
    ``live`` (``live_taps``): W holds the columns of those taps only (``prune_conv_weight``).
    ``out`` [M, ldc] with ``ldc`` / ``col_off``: the N channels land at channels col_off .. col_off+N-1 of it, and ``out`` is
    returned as it was given."""
    _need_gpu(x, W, bias, resid, resid_f32, out)
    assert x.dtype in HALF_TYPES and x.is_contiguous() and x.dim() == 5 and W.dtype == x.dtype and W.is_contiguous()
    B, D, H, Wd, Cc = x.shape
    if Cc % 8:
        raise _abi.KvqError(f"kvq_conv_implicit: channels-last input needs C % 8 == 0 (got C={Cc})")
    Do, Ho, Wo = conv_out_dims((D, H, Wd), kernel, stride, pad)
    N, k_pad = W.shape
    M = B * Do * Ho * Wo
    given = out is not None
    if not given and not store_f32:
        out = torch.empty(M, N, dtype=x.dtype, device=x.device)
    assert out is None or (out.dtype == x.dtype and out.is_contiguous() and out.numel() >= M * N)
    out32 = torch.empty(M, N, dtype=torch.float32, device=x.device) if (want_f32 or store_f32) else None
    assert relu or (resid is None and resid_f32 is None and not want_f32), "identity add / fp32 copy: ReLU epilogue only"
    a = _abi.KvqConvArgs()
    # a tap table only where it is needed: pruned taps (the table DEFINES K) or C % 32 != 0; otherwise the kernel walks the full
    # tap set with wave-uniform counters (no table loads between the slice DMAs)
    table = conv_taps(kernel, Cc, H, Wd, k_pad, x.device, live) if (live is not None or Cc % 32 or TAP_TABLE) else None
    a.x, a.W, a.bias, a.taps = ptr(x), ptr(W), ptr(bias), ptr(table)
    a.dims5[:] = (B, Cc, D, H, Wd)
    a.kernel3[:], a.stride3[:], a.pad3[:] = tuple(kernel), tuple(stride), tuple(pad)
    a.Kpad, a.N = k_pad, N
    a.epilogue = _abi.EPI_STORE_F32 if store_f32 else (_abi.EPI_RELU_BF16 if relu else _abi.EPI_BIAS_BF16)
    a.dtype = dtype_code(x.dtype)
    a.out_bf16, a.out_f32, a.resid_bf16, a.resid_f32 = ptr(out), ptr(out32), ptr(resid), ptr(resid_f32)
    a.ldc, a.col_off = _concat_dest(out, M, ldc, col_off)
    _ws = _splitk_scratch(a, x.shape[0] * Do * Ho * Wo, N, k_pad, x.device)   # noqa: F841
    check(lib().kvq_conv_implicit(C.byref(a), current_stream()), "kvq_conv_implicit")
    if store_f32:
        return out32
    if not given:
        out = out.reshape(B, Do, Ho, Wo, N)
    return (out, out32) if want_f32 else out


def resize_bilinear(video: torch.Tensor, rh: int, rw: int, crop=None, mean=None, std=None, round_u8=None, antialias=False):
    """video u8|fp32 (C,T,H,W) -> bilinear resize to (rh,rw) [-> crop (cy,cx,oh,ow)] [-> (v-mean)/std], fp32.
    ``antialias=True``: F.interpolate(..., antialias=True), what torchvision >= 0.17's Resize does to tensors
    (``kvq_resize_bilinear_aa``); False: the plain bilinear of torchvision < 0.17 (``kvq_resize_bilinear``)."""
    _need_gpu(video)
    assert video.dtype in (torch.uint8, torch.float32) and video.is_contiguous()
    Cc, T, H, W = video.shape
    cy, cx, oh, ow = crop if crop is not None else (0, 0, rh, rw)
    out = torch.empty(Cc, T, oh, ow, dtype=torch.float32, device=video.device)
    m = (C.c_float * Cc)(*mean) if mean is not None else None
    s = (C.c_float * Cc)(*std) if std is not None else None
    rnd = int(video.dtype == torch.uint8) if round_u8 is None else int(round_u8)
    fn, name = (lib().kvq_resize_bilinear_aa, "kvq_resize_bilinear_aa") if antialias else (lib().kvq_resize_bilinear,
                                                                                           "kvq_resize_bilinear")
    check(fn(ptr(video), int(video.dtype == torch.uint8), Cc, T, H, W, rh, rw, cy, cx, oh, ow, rnd, m, s, ptr(out),
             stream_of(video)), name)
    return out


def resize_aa_taps(in_size: int, out_size: int):
    """The tap tables of one axis of ``resize_bilinear(antialias=True)``, evaluated on the host by the code the kernel runs:
    (start int32 [out], size int32 [out], weights fp32 [out, kmax]; zero past size)."""
    import numpy as np
    k = C.c_int32()
    check(lib().kvq_resize_aa_taps(in_size, out_size, C.byref(k), None, None, None), "kvq_resize_aa_taps")
    start, size = np.zeros(out_size, np.int32), np.zeros(out_size, np.int32)
    w = np.zeros((out_size, k.value), np.float32)
    check(lib().kvq_resize_aa_taps(in_size, out_size, C.byref(k), start.ctypes.data, size.ctypes.data, w.ctypes.data),
          "kvq_resize_aa_taps")
    return start, size, w


def resize_pil_taps(in_size: int, out_size: int):
    """The tap tables of one axis of ``resize_pil`` (``kvq_resize_pil_taps``: built on the host in double):
    (start int32 [out], size int32 [out], coefficients int32 [out, kmax] with 22 fractional bits; zero past size)."""
    import numpy as np
    k = C.c_int32()
    check(lib().kvq_resize_pil_taps(in_size, out_size, C.byref(k), None, None, None), "kvq_resize_pil_taps")
    start, size = np.zeros(out_size, np.int32), np.zeros(out_size, np.int32)
    coef = np.zeros((out_size, k.value), np.int32)
    check(lib().kvq_resize_pil_taps(in_size, out_size, C.byref(k), start.ctypes.data, size.ctypes.data, coef.ctypes.data),
          "kvq_resize_pil_taps")
    return start, size, coef


_PIL_TAPS = {}          # (in, out, device) -> (start, size, coef) on the device


def _resize_pil_taps_on(in_size: int, out_size: int, device):
    """the tables of an axis on ``device``: built and uploaded once per (in, out)"""
    key = (int(in_size), int(out_size), str(device))
    if key not in _PIL_TAPS:
        _PIL_TAPS[key] = tuple(torch.from_numpy(a).to(device) for a in resize_pil_taps(in_size, out_size))
    return _PIL_TAPS[key]


def slowfast_lut() -> torch.Tensor:
    """The 256-entry table of the motion-feature transform (``datasets/slowfast_clips.py::pil_transform``): ToTensor + Normalize(.45,
    .225) of every byte value, by the torch expression the host path applies, on the CPU — so the device never restates ATen's scalar
    arithmetic (a CPU ``div`` by a scalar multiplies by the reciprocal) and equals the host path by construction."""
    t = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    return (t - 0.45) / 0.225


def identity_lut() -> torch.Tensor:
    """0..255 as fp32: ``resize_pil`` gives the resized bytes back"""
    return torch.arange(256, dtype=torch.float32)


def resize_pil_supported(frames, oh: int, ow: int) -> bool:
    i420 = isinstance(frames, I420Frames)
    T, H, W = (frames.shape[1], frames.H, frames.W) if i420 else frames.shape[:3]
    return bool(lib().kvq_resize_pil_supported(frames.format if i420 else _abi.SRC_U8, T, H, W, oh, ow))


def resize_pil(frames, oh: int, ow: int, lut: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Pillow's ``Image.resize((ow, oh), BILINEAR)`` of every frame, to the bit, each resized byte written as ``lut[byte]``
    (``kvq_resize_pil``, one launch).  ``frames``: uint8 (T, H, W, 3) interleaved on the device, or ``I420Frames`` (converted where
    the launch loads them).  ``lut``: fp32 (256,) on the device (``slowfast_lut()``, ``identity_lut()``).  -> fp32 (T, 3, oh, ow);
    ``out``: an fp32 (T, 3, oh, ow) view to write instead, with any frame and channel strides and contiguous oh x ow planes."""
    i420 = isinstance(frames, I420Frames)
    if i420:
        src, fmt, T, H, W = frames.data, frames.format, frames.shape[1], frames.H, frames.W
    else:
        src, fmt = frames, _abi.SRC_U8
        if not (torch.is_tensor(src) and src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3 and src.is_contiguous()):
            raise ValueError("resize_pil: expected contiguous uint8 (T, H, W, 3) frames or I420Frames, got "
                             f"{getattr(src, 'dtype', type(src))} {tuple(getattr(src, 'shape', ()))}")
        T, H, W = src.shape[:3]
    _need_gpu(src, lut, out)
    oh, ow = int(oh), int(ow)
    if not (lut.dtype == torch.float32 and lut.numel() == 256 and lut.is_contiguous() and lut.device == src.device):
        raise ValueError("resize_pil: lut must be 256 contiguous fp32 values on the frames' device")
    if out is None:
        out = torch.empty(T, 3, oh, ow, dtype=torch.float32, device=src.device)
    elif not (out.dtype == torch.float32 and tuple(out.shape) == (T, 3, oh, ow) and out.device == src.device
              and (out.stride(3) == 1 or ow == 1) and (out.stride(2) == ow or oh == 1)):
        raise ValueError(f"resize_pil: out must be an fp32 ({T}, 3, {oh}, {ow}) view with contiguous planes on the frames' device")
    xs, xn, xk = _resize_pil_taps_on(W, ow, src.device)
    ys, yn, yk = _resize_pil_taps_on(H, oh, src.device)
    check(lib().kvq_resize_pil(ptr(src), fmt, T, H, W, oh, ow, ptr(xs), ptr(xn), ptr(xk), ptr(ys), ptr(yn), ptr(yk), ptr(lut), ptr(out),
                               out.stride(0) if T > 1 else 3 * max(out.stride(1), oh * ow), out.stride(1), stream_of(src)), "kvq_resize_pil")
    return out


def upsample_frames(video: torch.Tensor, scale_factor: float):
    """get_spatial_fragments' small-source fallback (fusion_datasets.py:43-50): F.interpolate(video / 255.0, scale_factor,
    mode="bilinear") * 255.0 cast back to the frame type, ATen-CPU-exact.  video u8|fp32 (C,T,H,W) -> same type, upsampled."""
    _need_gpu(video)
    assert video.dtype in (torch.uint8, torch.float32) and video.is_contiguous()
    Cc, T, H, W = video.shape
    od = (C.c_int32 * 2)()
    check(lib().kvq_upsample_frames_out_dims(H, W, float(scale_factor), od), "kvq_upsample_frames_out_dims")
    out = torch.empty(Cc, T, od[0], od[1], dtype=video.dtype, device=video.device)
    check(lib().kvq_upsample_frames(ptr(video), int(video.dtype == torch.uint8), Cc, T, H, W, float(scale_factor), ptr(out),
                                    stream_of(video)), "kvq_upsample_frames")
    return out


def block_tail_pack(proj_w, proj_b, norm2_w, norm2_b, fc1_w, fc1_b, fc2_w, fc2_b):
    """Weight image of the fused proj+norm2+Mlp launch (include/kvq_hip.h: kvq_block_tail_pack)."""
    _need_gpu(proj_w, proj_b, norm2_w, norm2_b, fc1_w, fc1_b, fc2_w, fc2_b)
    assert proj_w.dtype in HALF_TYPES and fc1_w.dtype == proj_w.dtype and fc2_w.dtype == proj_w.dtype
    Cc, hidden = proj_w.shape[0], fc1_w.shape[0]
    nbytes = lib().kvq_block_tail_pack_bytes(Cc, hidden)
    if not nbytes:
        raise _abi.KvqError(f"kvq_block_tail: unsupported width C={Cc}, hidden={hidden}")
    pack = torch.empty(nbytes, dtype=torch.uint8, device=proj_w.device)
    check(lib().kvq_block_tail_pack(ptr(proj_w.contiguous()), ptr(proj_b), ptr(norm2_w), ptr(norm2_b),
                                    ptr(fc1_w.contiguous()), ptr(fc1_b), ptr(fc2_w.contiguous()), ptr(fc2_b), Cc, hidden,
                                    ptr(pack), current_stream()), "kvq_block_tail_pack")
    return pack


def block_tail_qkv_pack(qkv_w: torch.Tensor, hidden: int):
    """Image of a block's qkv weight (16-bit [3C][C]) that the PREVIOUS block's fused tail streams to emit q | k | v
    (include/kvq_hip.h: kvq_block_tail_qkv_pack); None when this width's tail cannot."""
    _need_gpu(qkv_w)
    assert qkv_w.dtype in HALF_TYPES and qkv_w.is_contiguous()
    Cc = qkv_w.shape[1]
    nbytes = lib().kvq_block_tail_qkv_pack_bytes(Cc, hidden)
    if not nbytes:
        return None
    pack = torch.empty(nbytes, dtype=torch.uint8, device=qkv_w.device)
    check(lib().kvq_block_tail_qkv_pack(ptr(qkv_w), Cc, hidden, ptr(pack), current_stream()), "kvq_block_tail_qkv_pack")
    return pack


def _set_next(a, next_norm, next_dst, next_rows):
    """the next block's norm1 and window map on the args struct of a launch that emits its rows (next_ln / qkv_out: the caller's)"""
    a.next_norm_w, a.next_norm_b, a.next_dst, a.next_rows = ptr(next_norm[0]), ptr(next_norm[1]), ptr(next_dst), next_rows


def block_tail(attn: torch.Tensor, x: torch.Tensor, pack: torch.Tensor, hidden: int, *, scatter_map=None, map_rows=0,
               out_rows=0, next_norm=None, next_dst=None, next_rows=0, eps=1e-5, attn_gather=None, next_qkv=None):
    """x (fp32 [n_batch*out_rows, C], in place — or fp16 at C <= 192: the round-6 residual stream of stages 0-1, ``x_f16``)
    += proj(attn) scattered; x += Mlp(norm2(x)).
    ``next_norm=(gamma, beta)`` + ``next_dst`` additionally returns norm1_next(x) in the next window order — or, with
    ``next_qkv=(qkv_pack, qkv_bias, q_scale)``, the next block's q | k | v, head-major [3][C/32][n_batch*next_rows][32]."""
    _need_gpu(attn, x, pack, scatter_map, next_dst)
    assert attn.dtype in HALF_TYPES and attn.is_contiguous() and x.dtype in (torch.float32, torch.float16) and x.is_contiguous()
    M, Cc = attn.shape
    a = _abi.KvqBlockTailArgs()
    a.x_f16 = int(x.dtype == torch.float16)
    a.attn, a.x, a.scatter_map, a.attn_gather = ptr(attn), ptr(x), ptr(scatter_map), ptr(attn_gather)
    a.map_rows, a.out_rows = (map_rows, out_rows) if (scatter_map is not None or attn_gather is not None) else (M, M)
    a.M, a.C, a.hidden, a.pack, a.eps, a.dtype = M, Cc, hidden, ptr(pack), eps, dtype_code(attn.dtype)
    nxt = None
    if next_norm is not None:
        n_batch = x.shape[0] // a.out_rows
        _set_next(a, next_norm, next_dst, next_rows)
        if next_qkv is not None:
            nxt = torch.empty(3, Cc // 32, n_batch * next_rows, 32, dtype=attn.dtype, device=x.device)
            a.next_qkv_pack, a.next_qkv_b, a.qkv_out, a.q_scale, a.num_heads = ptr(next_qkv[0]), ptr(next_qkv[1]), ptr(nxt), float(next_qkv[2]), Cc // 32
        else:
            nxt = torch.empty(n_batch * next_rows, Cc, dtype=attn.dtype, device=x.device)
            a.next_ln = ptr(nxt)
    check(lib().kvq_block_tail(C.byref(a), current_stream()), "kvq_block_tail")
    return nxt


def patch_embed(x, w: torch.Tensor, bias, ln_w, ln_b, patch, *, next_norm=None, next_dst=None, next_rows=0,
                eps=1e-5, out_f16=False):
    """PatchEmbed3D as one launch: x fp32 (B,Cin,T,H,W) or a ``FragmentSource``, w 16-bit [E][Cin*pd*ph*pw] -> fp32
    [B*D0*H0*W0, E] (+ the first block's norm1 rows when ``next_norm=(gamma, beta)`` / ``next_dst`` are given)."""
    frag = None
    if isinstance(x, FragmentSource):
        frag = x.c_struct()
        if frag is None:
            raise _abi.KvqError("kvq_patch_embed: this FragmentSource has no fused read (materialise() it)")
        _need_gpu(w, bias, ln_w, ln_b, next_dst)
    else:
        _need_gpu(x, w, bias, ln_w, ln_b, next_dst)
        assert x.dtype == torch.float32 and x.is_contiguous()
    assert w.dtype in HALF_TYPES and w.is_contiguous()
    B, Cin, T, H, W = x.shape
    pd, ph, pw = patch
    Ed, K = w.shape
    if not lib().kvq_patch_embed_supported(Cin, pd, ph, pw, Ed, T, H, W):
        raise _abi.KvqError("kvq_patch_embed: unsupported shape (use patch_im2col + gemm + layernorm_rows)")
    pack = torch.empty(lib().kvq_patch_embed_pack_bytes(Ed, K), dtype=torch.uint8, device=x.device)
    check(lib().kvq_patch_embed_pack(ptr(w), ptr(bias), ptr(ln_w), ptr(ln_b), Ed, K, ptr(pack), current_stream()),
          "kvq_patch_embed_pack")
    L0 = (T // pd) * (H // ph) * (W // pw)
    out = torch.empty(B * L0, Ed, dtype=torch.float16 if out_f16 else torch.float32, device=x.device)      # out_f16: the fp16 residual stream
    a = _abi.KvqPatchEmbedArgs()
    a.out_f16 = int(out_f16)
    a.x, a.B, a.in_chans, a.T, a.H, a.W, a.pd, a.ph, a.pw, a.embed_dim = (None if frag else ptr(x)), B, Cin, T, H, W, pd, ph, pw, Ed
    if frag is not None:
        a.frag = C.pointer(frag)
    a.pack, a.has_norm, a.out, a.eps, a.dtype = ptr(pack), int(ln_w is not None), ptr(out), eps, dtype_code(w.dtype)
    nxt = None
    if next_norm is not None:
        nxt = torch.empty(B * next_rows, Ed, dtype=w.dtype, device=x.device)
        _set_next(a, next_norm, next_dst, next_rows)
        a.next_ln = ptr(nxt)
    check(lib().kvq_patch_embed(C.byref(a), current_stream()), "kvq_patch_embed")
    return out, nxt


def patch_merge(x: torch.Tensor, merge_map: torch.Tensor, n_batch: int, red_w: torch.Tensor, norm_w, norm_b, out_dtype=torch.float16, *,
                next_norm=None, next_dst=None, next_rows=0, eps=1e-5, out_f16=False):
    """PatchMerging as one launch (C = 96 / 128 / 192): x fp32 (or fp16: the round-6 residual stream; ``out_f16``: the merged one too) [n_batch*L, C], merge_map int32 [Ln, 4] (-1 = zero padding), red_w fp32 [2C, 4C]
    -> fp32 [n_batch*Ln, 2C] (+ the next block's norm1 rows, ``out_dtype``, when ``next_norm=(gamma, beta)`` / ``next_dst`` are given)."""
    _need_gpu(x, merge_map, red_w, norm_w, norm_b, next_dst)
    assert x.dtype in (torch.float32, torch.float16) and x.is_contiguous() and merge_map.dtype == torch.int32 and merge_map.is_contiguous()
    assert red_w.dtype == torch.float32 and red_w.is_contiguous()
    Cc = x.shape[1]
    L, Ln = x.shape[0] // n_batch, merge_map.shape[0]
    nb = lib().kvq_patch_merge_pack_bytes(Cc)
    if not nb:
        raise _abi.KvqError("kvq_patch_merge: unsupported width (use layernorm_rows + gemm)")
    pack = torch.empty(nb, dtype=torch.uint8, device=x.device)
    check(lib().kvq_patch_merge_pack(ptr(red_w), ptr(norm_w), ptr(norm_b), Cc, dtype_code(out_dtype), ptr(pack), current_stream()),
          "kvq_patch_merge_pack")
    out = torch.empty(n_batch * Ln, 2 * Cc, dtype=torch.float16 if out_f16 else torch.float32, device=x.device)
    a = _abi.KvqPatchMergeArgs()
    a.x_f16, a.out_f16 = int(x.dtype == torch.float16), int(out_f16)
    a.x, a.merge_map, a.B, a.L, a.Ln, a.C, a.pack, a.out = ptr(x), ptr(merge_map), n_batch, L, Ln, Cc, ptr(pack), ptr(out)
    a.eps, a.dtype = eps, dtype_code(out_dtype)
    nxt = None
    if next_norm is not None:
        nxt = torch.empty(n_batch * next_rows, 2 * Cc, dtype=out_dtype, device=x.device)
        _set_next(a, next_norm, next_dst, next_rows)
        a.next_ln = ptr(nxt)
    check(lib().kvq_patch_merge(C.byref(a), current_stream()), "kvq_patch_merge")
    return out, nxt


def stem_mfma_pack_weight(w_kc: torch.Tensor, kernel, cin: int, out_dtype):
    """[K][Cout] fp32 stem weight (K ordered kd,kh,kw,c; Cout <= 8, kw = 7, cin <= 4) -> the 16-bit [kd*kh][16][32] image of
    ``kvq_conv_stem_mfma``: k = tap * 4 + c, zero rows / taps / channels as padding."""
    kd, kh, kw = kernel
    cout = w_kc.shape[1]
    assert kw == 7 and cin <= 4 and cout <= 8 and w_kc.shape[0] == kd * kh * kw * cin
    w = w_kc.reshape(kd * kh, kw, cin, cout).permute(0, 3, 1, 2)                 # [slice][o][tap][c]
    img = torch.zeros(kd * kh, 16, 8, 4, dtype=torch.float32, device=w_kc.device)
    img[:, :cout, :kw, :cin] = w
    return to_operand(img, out_dtype, img.device, (kd * kh, 16, 32))


def conv_stem_mfma(x: torch.Tensor, wpack: torch.Tensor, bias8: torch.Tensor, kernel, stride, pad, relu: bool):
    """Conv3d(C <= 4 -> 8, (kd, kh, 7), stride (sd, sh, 2), padding (pd, ph, 3)) + bias [+ ReLU] on the matrix cores: x fp32
    (B,C,T,H,W) contiguous -> 16-bit channels-last (B,Do,Ho,Wo,8).  ``wpack`` from ``stem_mfma_pack_weight``."""
    _need_gpu(x, wpack, bias8)
    assert x.dtype == torch.float32 and x.is_contiguous() and wpack.dtype in HALF_TYPES and bias8.numel() == 8
    B, Cin, T, H, W = x.shape
    x4 = torch.empty(B, T, H, W + 8, 4, dtype=wpack.dtype, device=x.device)
    check(lib().kvq_pack_clip_cl4(ptr(x), C.byref((C.c_int32 * 5)(B, Cin, T, H, W)), 4, dtype_code(wpack.dtype), ptr(x4),
                                  current_stream()), "kvq_pack_clip_cl4")
    do, ho, wo = conv_out_dims((T, H, W), kernel, stride, pad)
    out = torch.empty(B, do, ho, wo, 8, dtype=wpack.dtype, device=x.device)
    check(lib().kvq_conv_stem_mfma(ptr(x4), C.byref((C.c_int32 * 4)(B, T, H, W)), ptr(wpack), ptr(bias8), C.byref(_i32x(kernel)),
                                   C.byref(_i32x(stride)), C.byref(_i32x(pad)), int(relu), dtype_code(wpack.dtype), ptr(out),
                                   current_stream()), "kvq_conv_stem_mfma")
    return out


def conv_stem_pool(x: torch.Tensor, wpack: torch.Tensor, bias8: torch.Tensor, kd: int, relu: bool = True):
    """SlowFast's fast-pathway stem in one launch (``kvq_conv_stem_pool``): Conv3d(3 -> 8, (kd,7,7), stride (1,2,2), padding
    (kd//2,3,3)) + bias [+ ReLU] + MaxPool3d((1,3,3), (1,2,2), (0,1,1)); x fp32 (B,3,T,H,W) -> 16-bit channels-last (B,T,Hp,Wp,8)."""
    _need_gpu(x, wpack, bias8)
    assert x.dtype == torch.float32 and x.is_contiguous() and wpack.dtype in HALF_TYPES and bias8.numel() == 8
    B, Cin, T, H, W = x.shape
    hp, wp_ = ((H - 1) // 2 + 1 - 1) // 2 + 1, ((W - 1) // 2 + 1 - 1) // 2 + 1
    out = torch.empty(B, T, hp, wp_, 8, dtype=wpack.dtype, device=x.device)
    check(lib().kvq_conv_stem_pool(ptr(x), C.byref((C.c_int32 * 5)(B, Cin, T, H, W)), ptr(wpack), ptr(bias8), int(kd), int(relu),
                                   dtype_code(wpack.dtype), ptr(out), current_stream()), "kvq_conv_stem_pool")
    return out


def stem64_pack_weight(w_ok: torch.Tensor, out_dtype):
    """[64][>= 147] stem weight (K ordered kh,kw,c over a 1x7x7 kernel, 3 input channels) -> the 16-bit [7][64][32] image of
    ``kvq_conv_stem64_pool``: entry [kh][o][kw * 4 + c], tap 7 and channel 3 zero."""
    assert w_ok.shape[0] == 64 and w_ok.shape[1] >= 147
    img = torch.zeros(7, 64, 8, 4, dtype=torch.float32, device=w_ok.device)
    img[:, :, :7, :3] = w_ok[:, :147].float().reshape(64, 7, 7, 3).permute(1, 0, 2, 3)
    return to_operand(img, out_dtype, img.device, (7, 64, 32))


def conv_stem64_pool(x: torch.Tensor, t_index, wimg: torch.Tensor, bias64: torch.Tensor, relu: bool = True, out=None, out_coff: int = 0):
    """SlowFast's slow-pathway stem in one launch (``kvq_conv_stem64_pool``): frames ``t_index`` of the fp32 clip x (B,3,T,H,W) ->
    Conv3d(3 -> 64, (1,7,7), (1,2,2), (0,3,3)) + bias [+ ReLU] + MaxPool3d((1,3,3), (1,2,2), (0,1,1)); 16-bit channels-last
    (B,F,Hp,Wp,64), or channels out_coff .. out_coff+63 of ``out`` (B,F,Hp,Wp,C)."""
    _need_gpu(x, wimg, bias64)
    assert x.dtype == torch.float32 and x.is_contiguous() and wimg.dtype in HALF_TYPES and bias64.numel() == 64
    B, Cin, T, H, W = x.shape
    ti = None if t_index is None else torch.as_tensor(t_index, dtype=torch.int32).to(x.device)
    F_ = T if ti is None else ti.numel()
    hp, wp_ = ((H - 1) // 2 + 1 - 1) // 2 + 1, ((W - 1) // 2 + 1 - 1) // 2 + 1
    if out is None:
        out = torch.empty(B, F_, hp, wp_, 64, dtype=wimg.dtype, device=x.device)
    assert tuple(out.shape[:4]) == (B, F_, hp, wp_) and out.is_contiguous() and out.dtype == wimg.dtype
    check(lib().kvq_conv_stem64_pool(ptr(x), C.byref((C.c_int32 * 5)(B, Cin, T, H, W)), ptr(ti) if ti is not None else None, F_, ptr(wimg),
                                     ptr(bias64), int(relu), dtype_code(wimg.dtype), ptr(out), out.shape[4], out_coff, current_stream()),
          "kvq_conv_stem64_pool")
    return out


def conv_stem_direct(x: torch.Tensor, w_kc: torch.Tensor, bias: torch.Tensor, kernel, stride, pad, relu: bool, out_dtype):
    """Direct Conv3d for few output channels: x fp32 (B,C,D,H,W), w_kc fp32 [K][Cout] (K ordered kd,kh,kw,c), -> 16-bit
    channels-last (B,Do,Ho,Wo,Cout)."""
    _need_gpu(x, w_kc, bias)
    assert x.dtype == torch.float32 and x.is_contiguous() and w_kc.dtype == torch.float32 and w_kc.is_contiguous()
    B, Cin, D, H, W = x.shape
    cout = w_kc.shape[1]
    do, ho, wo = conv_out_dims((D, H, W), kernel, stride, pad)
    out = torch.empty(B, do, ho, wo, cout, dtype=out_dtype, device=x.device)
    check(lib().kvq_conv_stem_direct(ptr(x), C.byref((C.c_int32 * 5)(B, Cin, D, H, W)), ptr(w_kc), ptr(bias), cout,
                                     C.byref(_i32x(kernel)), C.byref(_i32x(stride)), C.byref(_i32x(pad)), int(relu),
                                     dtype_code(out_dtype), ptr(out), current_stream()), "kvq_conv_stem_direct")
    return out


# ---- VQAHead training step (csrc/headtrain.hip): thin wrappers; kvq_amd/finetune.py drives them.  The forward and the backward read
# bank rows: they follow the feature bank below ----------------------------------------------------------------------------------------
def headtrain_param_count(C_in: int, hidden: int = 64) -> int:
    """length of the flat parameter vector W1 [hidden][C] | b1 [hidden] | w2 [hidden] | b2 [1] of either head (simpleVQAHead: hidden 128)"""
    return hidden * C_in + 2 * hidden + 1


def headtrain_workspace(B: int, L: int, C_in: int, hidden: int = 64, device=None) -> torch.Tensor:
    """the workspace the forward and the backward of one (B, L, C) share; raises for a shape that is not built"""
    n = int(lib().kvq_headtrain_workspace_bytes(B, L, C_in, hidden))
    if n == 0:
        raise _abi.KvqError(f"kvq_headtrain: shape B={B} L={L} C={C_in} hidden={hidden} is not built "
                            "(B >= 2, C a multiple of 64, hidden 64)")
    return torch.empty(n // 4, dtype=torch.float32, device=device if device is not None else "cuda")


def headtrain_mask(seed: int, step: int, which: int, p: float, n: int, device=None) -> torch.Tensor:
    """uint8 [n]: 1 where element i of dropout ``which`` (0: features, 1: GELU output) is kept at (seed, step)"""
    out = torch.empty(n, dtype=torch.uint8, device=device if device is not None else "cuda")
    _need_gpu(out)
    check(lib().kvq_headtrain_mask(seed & 0xFFFFFFFF, step & 0xFFFFFFFF, which, p, n, ptr(out), stream_of(out)), "kvq_headtrain_mask")
    return out


def headtrain_loss(score, label, rank_weight=0.0, out3=None, dscore=None):
    """-> (out3 = [loss, plcc_loss, rank_loss], dscore [B]) of trainer.py:337-354, one launch"""
    _need_gpu(score, label)
    assert score.dtype == label.dtype == torch.float32 and score.is_contiguous() and label.is_contiguous()
    B = score.numel()
    assert label.numel() == B
    out3 = torch.empty(3, dtype=torch.float32, device=score.device) if out3 is None else out3
    dscore = torch.empty(B, dtype=torch.float32, device=score.device) if dscore is None else dscore
    check(lib().kvq_headtrain_loss(ptr(score), ptr(label), B, float(rank_weight), ptr(out3), ptr(dscore), stream_of(score)),
          "kvq_headtrain_loss")
    return out3, dscore


def headtrain_adamw(params, grads, exp_avg, exp_avg_sq, ema, lr, wd, step):
    """torch.optim.AdamW's update of the flat vector in place (optimiser step ``step`` >= 1), then the EMA copy (``ema`` None: skipped)"""
    _need_gpu(params, grads, exp_avg, exp_avg_sq, ema)
    n = params.numel()
    for t in (grads, exp_avg, exp_avg_sq) + (() if ema is None else (ema,)):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n
    check(lib().kvq_headtrain_adamw(ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), ptr(ema), n, float(lr), float(wd), int(step),
                                    stream_of(params)), "kvq_headtrain_adamw")


# ---- simpleVQAHead training step (csrc/simple_headtrain.hip): the loss and the optimiser are headtrain_loss and headtrain_adamw above ----
def simple_headtrain_workspace(B: int, T: int, C_in: int, hidden: int = 128, device=None) -> torch.Tensor:
    """the workspace the forward and the backward of one (B, T, C) share; raises for a shape that is not built"""
    n = int(lib().kvq_simple_headtrain_workspace_bytes(B, T, C_in, hidden))
    if n == 0:
        raise _abi.KvqError(f"kvq_simple_headtrain: shape B={B} T={T} C={C_in} hidden={hidden} is not built "
                            "(2 <= B <= 1024, C a multiple of 64, hidden 128)")
    return torch.empty(n // 4, dtype=torch.float32, device=device if device is not None else "cuda")


# ---- feature bank (csrc/featbank.hip) and the two training steps on its rows: thin wrappers; kvq_amd/finetune.py drives them ------------
class FeatureBank:
    """``[n_rows][L][C]`` cached features of a frozen trunk on the device, fp32, fp16 or bf16: ``tensor`` owns the memory, ``view`` is
    the ``KvqFeatureBank`` the entries take.  ``tensor``: adopt an existing dense tensor instead of allocating one."""

    def __init__(self, n_rows: int, L: int, C_in: int, dtype=torch.float32, device=None, tensor=None):
        code = _abi.bank_dtype_code(dtype)
        if tensor is None:
            tensor = torch.empty(int(n_rows), int(L), int(C_in), dtype=_abi.bank_torch_dtype(code), device=device if device is not None else "cuda")
        assert tensor.dim() == 3 and tensor.is_contiguous() and tensor.dtype == _abi.bank_torch_dtype(code), "a bank is dense [n_rows][L][C]"
        self.tensor, self.dtype = tensor, tensor.dtype
        self.n_rows, self.L, self.C = (int(v) for v in tensor.shape)
        self.view = _abi.KvqFeatureBank(ptr(tensor), code, self.L, self.C, self.n_rows)

    @classmethod
    def of(cls, tensor):
        return cls(*tensor.shape, dtype=tensor.dtype, tensor=tensor)

    @property
    def nbytes(self) -> int:
        return self.tensor.numel() * self.tensor.element_size()


def bank_index(index, bank: "FeatureBank") -> torch.Tensor:
    """the index vector of a bank entry as int32 on the bank's device.  A CPU tensor (or a sequence) is checked here: a value outside
    ``[0, n_rows)`` raises ValueError naming it; a device tensor is not read back — the launches clamp its values into the bank."""
    if not isinstance(index, torch.Tensor):
        index = torch.as_tensor(index, dtype=torch.int64)
    if not index.is_cuda:
        index = index.reshape(-1)
        bad = ((index < 0) | (index >= bank.n_rows)).nonzero()
        if bad.numel():
            k = int(bad[0])
            raise ValueError(f"index[{k}] = {int(index[k])} is outside the bank's rows 0 .. {bank.n_rows - 1}")
        return index.to(torch.int32).to(bank.tensor.device)
    assert index.dtype == torch.int32 and index.dim() == 1 and index.is_contiguous(), "a device index is a dense int32 vector"
    return index


def feature_bank_store(feat: torch.Tensor, bank: FeatureBank, first_row: int, flag: Optional[torch.Tensor] = None):
    """rows ``first_row ..`` of the bank = the fp32 features ``feat`` [n][L][C], any sample and token strides (multiples of 4), channel
    stride 1: read where they lie, rounded to nearest even.  ``flag`` (int32 [1] on the device, never cleared here) becomes 1 when a
    NaN is stored, or a value past +-65504 into an fp16 bank (stored as +-65504)."""
    _need_gpu(feat, bank.tensor, flag)
    assert feat.dtype == torch.float32 and feat.dim() == 3 and tuple(feat.shape[1:]) == (bank.L, bank.C), "features: fp32 [n][L][C] of the bank's (L, C)"
    assert feat.stride(2) == 1 or bank.C == 1, "the channel stride of the features must be 1"
    assert flag is None or (flag.dtype == torch.int32 and flag.numel() == 1)
    check(lib().kvq_feature_bank_store(ptr(feat), feat.shape[0], feat.stride(0), feat.stride(1), C.byref(bank.view), int(first_row),
                                       ptr(flag), stream_of(feat)), "kvq_feature_bank_store")


def feature_bank_rows(bank: FeatureBank, index, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dense fp32 [B][L][C]: the bank's rows ``index`` (``bank_index``), widened"""
    idx = bank_index(index, bank)
    _need_gpu(bank.tensor, idx, out)
    if out is None:
        out = torch.empty(idx.numel(), bank.L, bank.C, dtype=torch.float32, device=bank.tensor.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (idx.numel(), bank.L, bank.C)
    check(lib().kvq_feature_bank_rows(C.byref(bank.view), ptr(idx), idx.numel(), ptr(out), stream_of(out)), "kvq_feature_bank_rows")
    return out


def _headtrain_bank_args(bank, index, params, p, seed, step, ws, hidden, score=None, dscore=None, grads=None):
    idx = bank_index(index, bank)
    _need_gpu(bank.tensor, idx, params, ws, score, dscore, grads)
    B = idx.numel()
    assert params.dtype == torch.float32 and params.is_contiguous() and params.numel() == headtrain_param_count(bank.C, hidden)
    for t in (score, dscore):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == B)
    assert grads is None or (grads.dtype == torch.float32 and grads.is_contiguous() and grads.numel() == params.numel())
    a = _abi.KvqHeadTrainBankArgs()
    a.bank, a.index, a.B, a.L, a.C, a.hidden, a.params = bank.view, ptr(idx), B, bank.L, bank.C, hidden, ptr(params)
    a.p_drop, a.seed, a.step = float(p), seed & 0xFFFFFFFF, step & 0xFFFFFFFF
    a.workspace, a.workspace_bytes = ptr(ws), ws.numel() * ws.element_size()
    a.score, a.dscore, a.grads = ptr(score), ptr(dscore), ptr(grads)
    return a, idx


def headtrain_bank_forward(bank, index, params, p, seed, step, ws, score=None):
    """train-mode scores fp32 [B] of the bank rows ``index`` (channels-last [L][C] each, read in place and widened in registers) under
    the flat parameters; the pre-activations stay in ``ws``"""
    if score is None:
        score = torch.empty(len(index), dtype=torch.float32, device=bank.tensor.device)
    a, idx = _headtrain_bank_args(bank, index, params, p, seed, step, ws, 64, score=score)
    check(lib().kvq_headtrain_bank_forward(C.byref(a), stream_of(bank.tensor)), "kvq_headtrain_bank_forward")
    return score


def headtrain_bank_backward(bank, index, params, p, seed, step, ws, dscore, grads=None):
    """the flat gradient (layout of ``params``) from ``dscore`` [B]; reads the pre-activations the forward of the same
    (seed, step, p) left in ``ws``"""
    if grads is None:
        grads = torch.empty_like(params)
    a, idx = _headtrain_bank_args(bank, index, params, p, seed, step, ws, 64, dscore=dscore, grads=grads)
    check(lib().kvq_headtrain_bank_backward(C.byref(a), stream_of(bank.tensor)), "kvq_headtrain_bank_backward")
    return grads


def simple_headtrain_bank_forward(bank, index, params, ws, score=None):
    """scores fp32 [B] of the bank rows ``index`` ([T][C] each, read in place) under the flat parameters: the mean over the T frames of
    the two Linears"""
    if score is None:
        score = torch.empty(len(index), dtype=torch.float32, device=bank.tensor.device)
    a, idx = _headtrain_bank_args(bank, index, params, 0.0, 0, 0, ws, 128, score=score)
    check(lib().kvq_simple_headtrain_bank_forward(C.byref(a), stream_of(bank.tensor)), "kvq_simple_headtrain_bank_forward")
    return score


def simple_headtrain_bank_backward(bank, index, params, ws, dscore, grads=None):
    """the flat gradient (layout of ``params``, written in full) from ``dscore`` [B]; needs no forward before it"""
    if grads is None:
        grads = torch.empty_like(params)
    a, idx = _headtrain_bank_args(bank, index, params, 0.0, 0, 0, ws, 128, dscore=dscore, grads=grads)
    check(lib().kvq_simple_headtrain_bank_backward(C.byref(a), stream_of(bank.tensor)), "kvq_simple_headtrain_bank_backward")
    return grads


# ---- the two steps on a dense fp32 batch [B][L][C]: an fp32 bank of its B rows under the index 0 .. B-1 --------------------------------
def _dense_bank(feat):
    assert feat.dtype == torch.float32 and feat.dim() == 3 and feat.is_contiguous(), "features: dense fp32 [B][L][C]"
    return FeatureBank.of(feat), torch.arange(feat.shape[0], dtype=torch.int32, device=feat.device)


def headtrain_forward(feat, params, p, seed, step, ws, score=None):
    return headtrain_bank_forward(*_dense_bank(feat), params, p, seed, step, ws, score)


def headtrain_backward(feat, params, p, seed, step, ws, dscore, grads=None):
    return headtrain_bank_backward(*_dense_bank(feat), params, p, seed, step, ws, dscore, grads)


def simple_headtrain_forward(feat, params, ws, score=None):
    return simple_headtrain_bank_forward(*_dense_bank(feat), params, ws, score)


def simple_headtrain_backward(feat, params, ws, dscore, grads=None):
    return simple_headtrain_bank_backward(*_dense_bank(feat), params, ws, dscore, grads)
