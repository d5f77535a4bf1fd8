"""Guard-band allocations for the memory tests (tests/test_gpu_bounds.py, tests/test_guarded_cpu.py).

``with guarded() as G:`` replaces ``torch.empty`` and ``torch.empty_like`` — the only allocators kvq_amd/kernels.py uses for its
outputs and scratch — so that every tensor a wrapper allocates is the payload of one uint8 buffer

    guard | payload | pad to 16 B | guard

with the guards filled with 0xA5 and the payload with 0xFF (NaN in fp32 / fp16 / bf16, -1 in the signed integers, 255 in bytes).
A guard is max(4096 B, 32 rows of the last dimension) rounded up to 256 B and the payload starts on a 256-byte boundary, so the
alignment a kernel sees is that of a fresh allocation (alignments below 256 B are not varied here).  The registry keeps every
buffer alive until it is checked — the split-K scratch, which ``kernels.gemm`` drops right after the launch, included.

``G.wrap(t)`` copies an existing tensor into such a buffer: inputs, and outputs the caller hands in.  The guards of a wrapped
floating tensor and of a byte image are 0xFF: a value read past either end is NaN (255) and, unless it is discarded, shows in the
result.  The guards of a wrapped integer tensor of two or more bytes per element are ZERO: those are the tables a kernel turns
into addresses (scatter / gather / merge maps, token descriptors, regions, patch origins, padding rows), and an over-read of one
must form a valid address, not a wild one.  That is a blind spot, stated here on purpose: an over-read of an index table reads
index 0 and is not detected by these tests.  An over-read whose value is discarded (a clamped row) is not detected either.

Three checks:
  ``G.intact()``            every guard byte of every allocation still holds its fill (stores in front of / behind a tensor)
  ``G.payload_left(view)``  the elements of a guarded tensor that still hold the 0xFF payload (elements never written)
  ``G.untouched(view, m)``  the elements selected by ``m`` all still hold it (regions an entry point documents it leaves alone)
"""
import contextlib

import torch

GUARD_BYTE = 0xA5
PAYLOAD_BYTE = 0xFF
MIN_GUARD = 4096
ALIGN = 256

_PASS_KEYS = {"dtype", "device"}


class Report:
    """the outcome of a check: truthy when clean, and its text names what is not"""

    def __init__(self, problems):
        self.problems = list(problems)

    def __bool__(self):
        return not self.problems

    def __repr__(self):
        return "clean" if not self.problems else "; ".join(self.problems)


class _Alloc:
    __slots__ = ("buf", "start", "nbytes", "fill", "name", "view")


class Registry:
    def __init__(self, device_type, empty, payload=PAYLOAD_BYTE, max_guard=None):
        self.device_type, self._empty, self.payload, self.max_guard = device_type, empty, payload, max_guard
        self.allocs = []

    # ---------------------------------------------------------------------------------------------------------- allocation
    def alloc(self, shape, dtype, device, fill=GUARD_BYTE, name=None):
        shape = tuple(int(s) for s in shape)
        item = self._empty(0, dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * item
        padded = -(-nbytes // 16) * 16
        last = shape[-1] if shape else 1
        guard = -(-max(MIN_GUARD, 32 * last * item) // ALIGN) * ALIGN
        if self.max_guard is not None:
            guard = min(guard, -(-max(MIN_GUARD, self.max_guard) // ALIGN) * ALIGN)
        buf = self._empty(ALIGN + guard + padded + guard, dtype=torch.uint8, device=device)
        start = (-buf.data_ptr()) % ALIGN + guard
        buf.fill_(fill)
        buf[start:start + nbytes].fill_(self.payload)
        a = _Alloc()
        a.buf, a.start, a.nbytes, a.fill = buf, start, nbytes, fill
        a.name = f"#{len(self.allocs)} {name or 'empty'} {str(dtype).replace('torch.', '')} {shape}"
        a.view = buf[start:start + nbytes].view(dtype).view(shape)
        self.allocs.append(a)
        return a.view

    def wrap(self, t, poison=None, name=None):
        """``t`` copied into a guarded buffer.  ``poison``: "nan" (0xFF guards), "zero", or None = by dtype (module docstring)."""
        if poison is None:
            poison = "zero" if (not t.dtype.is_floating_point and t.element_size() >= 2) or t.dtype == torch.bool else "nan"
        fill = {"nan": 0xFF, "zero": 0x00}[poison]
        v = self.alloc(t.shape, t.dtype, t.device, fill=fill, name=f"wrap {name or ''}".strip())
        v.copy_(t)
        return v

    # -------------------------------------------------------------------------------------------------------------- checks
    def intact(self):
        """every guard of every allocation made so far; synchronises"""
        if self.device_type == "cuda":
            torch.cuda.synchronize()
        problems = []
        for a in self.allocs:
            for side, region, base in (("front", a.buf[:a.start], -a.start), ("back", a.buf[a.start + a.nbytes:], a.nbytes)):
                bad = region != a.fill
                if bool(bad.any()):
                    first = int(bad.nonzero()[0 if side == "back" else -1])
                    problems.append(f"{a.name}: {side} guard overwritten, {int(bad.sum())} bytes, nearest at byte offset {base + first} "
                                    f"of the tensor (value 0x{int(region[first]):02X})")
        return Report(problems)

    def payload_left(self, view):
        """bool tensor of ``view``'s shape: the element still holds the payload pattern (every byte)"""
        b = view.contiguous().view(-1).view(torch.uint8).view(-1, view.element_size())
        return (b == self.payload).all(1).view(view.shape)

    def untouched(self, view, mask=None):
        """the elements ``view[mask]`` (all of ``view`` without a mask) all still hold the payload pattern"""
        left = self.payload_left(view)
        sel = left if mask is None else left[mask]
        n = int((~sel).sum())
        return Report([] if n == 0 else [f"{n} of {sel.numel()} elements that should have been left alone were written"])


@contextlib.contextmanager
def guarded(device_type="cuda", payload=PAYLOAD_BYTE, max_guard=None):
    """patch ``torch.empty`` / ``torch.empty_like`` for ``device_type`` tensors; yields the registry.  Calls for another device
    type, or with keywords other than ``dtype`` / ``device``, go straight to the originals, which are put back on exit.
    ``max_guard``: an upper limit in bytes for a guard (whole-model forwards allocate flat byte buffers of many megabytes — workspaces,
    weight images — whose "32 rows" would be 32 times the buffer)."""
    orig_empty, orig_empty_like = torch.empty, torch.empty_like
    G = Registry(device_type, orig_empty, payload, max_guard)

    def _device_type(device):
        if device is None:
            device = torch.get_default_device() if hasattr(torch, "get_default_device") else "cpu"
        return torch.device(device).type

    def empty(*size, **kw):
        if set(kw) - _PASS_KEYS or _device_type(kw.get("device")) != device_type:
            return orig_empty(*size, **kw)
        shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
        if not all(isinstance(s, int) or (hasattr(s, "__index__") and not torch.is_tensor(s)) for s in shape):
            return orig_empty(*size, **kw)
        dtype = kw.get("dtype") or torch.get_default_dtype()
        return G.alloc(shape, dtype, kw.get("device") if kw.get("device") is not None else device_type)

    def empty_like(t, **kw):
        device = kw.get("device", t.device)
        if set(kw) - _PASS_KEYS or _device_type(device) != device_type or not t.is_contiguous():
            return orig_empty_like(t, **kw)
        return G.alloc(t.shape, kw.get("dtype") or t.dtype, device)

    torch.empty, torch.empty_like = empty, empty_like
    try:
        yield G
    finally:
        torch.empty, torch.empty_like = orig_empty, orig_empty_like
