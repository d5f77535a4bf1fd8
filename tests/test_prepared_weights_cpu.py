"""The shared weight preparation (``kvq_amd/_prepared.py``) on the CPU: every kernel-ready tensor the model mirrors build from
their parameters is pinned, digest by digest, to what the per-model copies produced before the helpers existed
(tests/golden/prepared_weights.json, written by tests/golden/make_prepared_golden.py at that commit), and the helpers are
checked one by one against their definitions written out here."""
import json
import os

import pytest
import torch

import kvq_amd  # noqa: F401
from kvq_amd import _abi, _prepared

import prepared_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prepared_weights.json")


@pytest.fixture(scope="module")
def digests():
    return prepared_ref.collect()


def test_prepared_tensors_match_the_recorded_digests(digests):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(digests) == sorted(want)
    bad = [k for k in want if digests[k] != want[k]]
    assert not bad, f"{len(bad)} of {len(want)} prepared tensors differ from the record, first: {bad[:8]}"


def test_recorded_inputs_exercise_the_fp16_clamp(digests):
    """The pin above would say nothing about the clamp if no folded value left the fp16 range: the ResNet stem's does."""
    from kvq_amd.models.backbones import simpleVQA_model
    net = simpleVQA_model.ResNet(layers=(1, 1, 1, 1))
    prepared_ref.fill(net)
    for dt, top in (("fp16", 65504.0), ("bf16", None)):
        net.operand_dtype = _abi.dtype_code(dt)
        w = net._weights("cpu")["stem"][0].float()
        assert torch.isfinite(w).all()
        assert w.abs().max() == top if top else w.abs().max() > 65504.0
    assert any(digests[k] != digests[k.replace("/fp16/", "/bf16/")] for k in digests if k.startswith("CONTRIQUE/fp16/"))


# ---------------------------------------------------------------------------------------------------------------- the helpers
def test_to_operand_saturates_fp16_only():
    t = torch.tensor([1e6, -1e6, 65504.0, -65504.0, 1.5])
    h = _prepared.to_operand(t, torch.float16, "cpu")
    assert h.dtype == torch.float16 and h.tolist() == [65504.0, -65504.0, 65504.0, -65504.0, 1.5]
    b = _prepared.to_operand(t, torch.bfloat16, "cpu")
    assert b.dtype == torch.bfloat16 and torch.isfinite(b).all() and b[0] == torch.tensor(1e6).to(torch.bfloat16) and b[0] > 65504
    r = _prepared.to_operand(torch.arange(6.0).reshape(1, 2, 3).requires_grad_(), torch.float16, "cpu", (2, -1))
    assert r.shape == (2, 3) and r.is_contiguous() and not r.requires_grad
    f = _prepared.to_f32(torch.arange(6, dtype=torch.float64).reshape(2, 3).t(), "cpu")
    assert f.dtype == torch.float32 and f.is_contiguous() and f.shape == (3, 2)


@pytest.mark.parametrize("shape", [(5, 3, 3, 3), (4, 3, 2, 3, 3), (6, 7)], ids=["conv2d", "conv3d", "linear"])
def test_fold_bn_is_the_written_out_formula(shape):
    n = shape[0]
    k = torch.arange(n, dtype=torch.float32)
    w = ((torch.arange(torch.Size(shape).numel()) * 7 % 23 - 11).to(torch.float32) / 8).reshape(shape)
    gamma, beta, mean, var, eps = (2 * k + 1) / 8, (k - 2) / 4, (2 * k - 5) / 16, (2 * k + 3) / 8, 1e-3
    wf, bf = _prepared.fold_bn(w, gamma, beta, mean, var, eps)
    assert wf.dtype == bf.dtype == torch.float32 and wf.shape == w.shape and bf.shape == (n,)
    for o in range(n):
        scale = gamma[o] / torch.sqrt(var[o] + eps)
        assert torch.equal(wf[o], w[o] * scale)
        assert bf[o] == beta[o] - mean[o] * scale


def test_pad_k32():
    w = torch.arange(2 * 33, dtype=torch.float32).reshape(2, 33)
    p = _prepared.pad_k32(w)
    assert p.shape == (2, 64) and torch.equal(p[:, :33], w) and not p[:, 33:].any()
    w64 = torch.ones(3, 64)
    assert _prepared.pad_k32(w64) is w64


@pytest.mark.parametrize("taps,cin", [(49, 3), (9, 3), (4, 8), (5, 1)])
def test_spread_stem8_against_a_loop(taps, cin):
    rows = 3
    w = (torch.arange(rows * (taps * cin + 5), dtype=torch.float32) + 1).reshape(rows, -1).to(torch.float16)   # columns past taps*cin: K padding
    got = _prepared.spread_stem8(w, taps, cin)
    want = torch.zeros(rows, -(-taps * 8 // 32) * 32, dtype=w.dtype)
    for r in range(rows):
        for t in range(taps):
            for c in range(cin):
                want[r, t * 8 + c] = w[r, t * cin + c]
    assert got.dtype == w.dtype and torch.equal(got, want)


class _Holder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(4))
        self.register_buffer("running_mean", torch.zeros(4))


def test_prepared_cache_rebuilds_exactly_when_something_changed():
    m, cache, calls = _Holder(), _prepared.PreparedCache(), []

    def get(key=(1, "cpu")):
        def build():
            calls.append(key)
            return [m.weight.detach() + m.running_mean]
        return cache.get(key, list(m.parameters()) + list(m.buffers()), build)

    first = get()
    assert len(calls) == 1
    again = get()
    assert again is first and again[0] is first[0] and len(calls) == 1                # a hit: the identical objects, no build
    with torch.no_grad():
        m.weight.add_(1.0)                                                            # in-place write to a parameter
    second = get()
    assert len(calls) == 2 and second is not first and second[0].tolist() == [2.0] * 4
    assert get() is second and len(calls) == 2
    m.running_mean.add_(3.0)                                                          # in-place write to a buffer (BN running mean)
    third = get()
    assert len(calls) == 3 and third[0].tolist() == [5.0] * 4
    assert get() is third and len(calls) == 3
    m.weight.data = torch.full((4,), 7.0)                                             # the parameter's storage replaced
    fourth = get()
    assert len(calls) == 4 and fourth[0].tolist() == [10.0] * 4
    assert get() is fourth and len(calls) == 4
    fifth = get((2, "cpu"))                                                           # a changed key
    assert len(calls) == 5 and fifth is not fourth
    assert get((2, "cpu")) is fifth and len(calls) == 5


def test_prepared_cache_keeps_no_entry_of_a_failed_build():
    m, cache = _Holder(), _prepared.PreparedCache()
    ok = cache.get((), m.parameters(), lambda: "ok")
    with torch.no_grad():
        m.weight.mul_(2.0)
    with pytest.raises(ZeroDivisionError):
        cache.get((), m.parameters(), lambda: 1 // 0)
    assert cache.get((), m.parameters(), lambda: "rebuilt") == "rebuilt" and ok == "ok"


def test_contrique_projector_cache_watches_the_running_statistics():
    """What the second signature inside CONTRIQUE_model.forward used to cover: a BatchNorm buffer written in place refolds."""
    from kvq_amd.models.backbones import ksvqe_modules as KM
    pj = torch.nn.Sequential(torch.nn.Linear(4, 4, bias=False), torch.nn.BatchNorm1d(4))
    mod = KM._HipModule()
    mod.projector = pj
    tensors = lambda: list(pj.parameters()) + list(pj.buffers())  # noqa: E731
    a = mod._cached("cpu", lambda: KM.CONTRIQUE_model._fold(mod, pj[0], pj[1], "cpu"), tensors=tensors())
    assert mod._cached("cpu", lambda: None, tensors=tensors()) is a
    pj[1].running_mean.add_(1.0)
    b = mod._cached("cpu", lambda: KM.CONTRIQUE_model._fold(mod, pj[0], pj[1], "cpu"), tensors=tensors())
    assert b is not a and not torch.equal(a[1], b[1])


def test_default_operand_dtype_argument_beats_environment(monkeypatch):
    monkeypatch.delenv("KVQ_OPERAND_DTYPE", raising=False)
    assert _prepared.default_operand_dtype() == _abi.dtype_code("fp16")
    monkeypatch.setenv("KVQ_OPERAND_DTYPE", "bf16")
    assert _prepared.default_operand_dtype() == _abi.dtype_code("bf16")
    assert _prepared.default_operand_dtype("fp16") == _abi.dtype_code("fp16")
    from kvq_amd.models.backbones import ksvqe_modules as KM, simpleVQA_model
    assert KM.crossattention1(64, 1).operand_dtype == _abi.dtype_code("bf16")         # evaluated at construction
    assert simpleVQA_model.ResNet(layers=(1, 1, 1, 1), operand_dtype="fp16").operand_dtype == _abi.dtype_code("fp16")
