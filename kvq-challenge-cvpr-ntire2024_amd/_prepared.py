"""The one weight-preparation path of the model mirrors, which turn their parameters (and BatchNorm buffers) into kernel-ready
device tensors on the first forward and cache them: the operand cast with the fp16 clamp, the eval-mode BatchNorm fold, the K
padding, the 8-channel stem layout and the "rebuild when a tensor moved or was written" cache.  One copy, so that "fp16 operands
saturate, never inf" and "running statistics are part of the cache key" hold at every site.  Nothing here launches a kernel;
it sits beside ``_abi.py`` because ``kernels.py`` casts its packed stem images through ``to_operand`` too."""
import os

import torch

from . import _abi


def default_operand_dtype(arg=None) -> int:
    """dtype code of the 16-bit MFMA operand type: ``arg`` ("fp16" / "bf16" / a code) if given, else KVQ_OPERAND_DTYPE, else fp16."""
    return _abi.dtype_code(arg or os.environ.get("KVQ_OPERAND_DTYPE", "fp16"))


def to_f32(t, device):
    return t.detach().to(device, torch.float32).contiguous()


def to_operand(t, half, device, shape=None):
    """A GEMM / conv operand in the 16-bit type ``half``: fp32 on the device, reshaped, then cast — fp16 saturates at +-65504, never inf."""
    t = t.detach().to(device, torch.float32)
    if shape is not None:
        t = t.reshape(shape)
    if half == torch.float16:
        t = t.clamp(-65504.0, 65504.0)
    return t.to(half).contiguous()


def fold_bn(weight, gamma, beta, mean, var, eps, device=None):
    """Eval-mode BatchNorm folded into the conv / linear in front of it: scale = gamma / sqrt(var + eps) per output row ->
    (weight * scale, beta - mean * scale), both fp32 on ``device`` (default: where the weight is), the weight in its own layout."""
    device = weight.device if device is None else device
    w, g, b, mu, v = (t.detach().to(device, torch.float32) for t in (weight, gamma, beta, mean, var))
    scale = g / torch.sqrt(v + eps)
    return w * scale.view((-1,) + (1,) * (w.dim() - 1)), (b - mu * scale).contiguous()


def pad_k32(w2d):
    """[rows][K] -> [rows][K rounded up to a multiple of 32], zero filled."""
    kpad = -(-w2d.shape[1] // 32) * 32
    return w2d if kpad == w2d.shape[1] else torch.nn.functional.pad(w2d, (0, kpad - w2d.shape[1]))


def spread_stem8(w2d, taps, cin):
    """Stem weight with (tap, c < cin <= 8)-ordered columns -> the (tap, 8) columns of the channel-padded implicit conv, K padded to 32."""
    w8 = torch.zeros(w2d.shape[0], -(-taps * 8 // 32) * 32, dtype=w2d.dtype, device=w2d.device)
    w8[:, :taps * 8].view(w2d.shape[0], taps, 8)[:, :, :cin] = w2d[:, :taps * cin].reshape(w2d.shape[0], taps, cin)
    return w8


def signature(key, tensors):
    """``key`` + where every tensor lives and how often it was written in place: one host pass, no device work."""
    return (key, tuple((t.data_ptr(), t._version) for t in tensors))


class PreparedCache:
    """One prepared value per owner.  ``get`` returns the SAME objects until ``key`` changes or one of ``tensors`` (every parameter and
    buffer the build reads) moved or was written — recorded hipGraphs hold the addresses of what was returned."""

    def __init__(self):
        self._sig = self._value = None

    def get(self, key, tensors, build):
        sig = signature(key, tensors)
        if self._sig != sig:
            self._sig = None                 # a build that raises leaves no entry behind
            self._value = build()
            self._sig = sig
        return self._value
