"""simpleVQAHead training step, everything that needs no GPU: the numpy restatement (tests/simple_headtrain_ref.py) against the reference's
stored run (tests/golden/simple_headtrain.npz), the new ABI symbols and their host-side refusals, the workspace formula, the Python-side
refusals and the yml."""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest
import yaml

import kvq_amd  # noqa: F401
from kvq_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simple_headtrain_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (B, T, C, rank_weight).  e: more than 256 videos (a thread of the loss and of the sum of dscore owns two) and 1200 rows: runs longer than
# the 32-row minimum (30 runs of 40 rows), added in segments of 8, 8, 8 and 6
CASES = {"a": (4, 8, 9472, 0.0), "b": (5, 3, 9472, 0.0), "c": (7, 1, 192, 0.0), "d": (33, 8, 704, 0.0), "c_rank": (7, 1, 192, 0.3),
         "e": (300, 4, 192, 0.0)}
NEW = ["kvq_simple_headtrain_workspace_bytes"]
GONE = ["kvq_simple_headtrain_forward", "kvq_simple_headtrain_backward"]   # the dense entries: the step is the bank entries' (ABI 32)
HID = 128
SUB = (slice(3, None, 16), slice(5, None, 64))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def load_case(g, name):
    B, T, Cc, seed = (int(v) for v in g[f"{name}/meta"])
    x, y, prm = R.make_case(seed, B, T, Cc)
    return dict(B=B, T=T, C=Cc, seed=seed, rw=float(g[f"{name}/rw"]), x=x, y=y, prm=prm)


def test_fixture_holds_the_cases_of_the_issue(golden):
    g = golden("simple_headtrain.npz")
    for name, (B, T, Cc, rw) in CASES.items():
        assert tuple(int(v) for v in g[f"{name}/meta"][:3]) == (B, T, Cc) and float(g[f"{name}/rw"]) == rw
        for run in ("ref32_err", "alt32_err"):
            for k in ("dW1", "dW2"):
                assert g[f"{name}/{run}/{k}"].max() <= 5e-6
        assert np.diff(np.sort(g[f"{name}/score"][0])).min() > 1e-6 and g[f"{name}/score"][0].std() >= 0.1
        c = load_case(g, name)                     # the rebuilt inputs are the ones the reference ran on
        assert np.array_equal(c["x"].reshape(-1)[:256], g[f"{name}/x_head"]) and c["x"].astype(np.float64).sum() == g[f"{name}/x_sum"]
        assert np.array_equal(c["y"], g[f"{name}/labels"])
        nW = HID * Cc
        assert np.array_equal(c["prm"][:nW].reshape(HID, Cc)[SUB], g[f"{name}/params0_sub"])
        assert np.array_equal(c["prm"][nW:], g[f"{name}/params0_small"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "simple_headtrain.npz")) < 1 << 20


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_reference_run(golden, name):
    """every stored float64 array to 1e-10 relative (W1-shaped ones: subsample, norm and sum).  db1 and db2 are analytically zero: both
    sides hold rounding noise (<= 1e-14), and the restatement's AdamW is fed the reference's, since Adam turns that noise into a full step"""
    g = golden("simple_headtrain.npz")
    c = load_case(g, name)
    lr, wd, wu, mx = g["hyper"]
    zero = np.concatenate([g[f"{name}/db1"], g[f"{name}/db2"][:, None]], axis=1)
    steps = R.train_steps(c["x"], c["y"], c["prm"], 3, lr, wd, int(wu), int(mx), rank_weight=c["rw"], zero_grads=zero)
    nW = HID * c["C"]
    sub = lambda v: v[:nW].reshape(HID, c["C"])[SUB]               # noqa: E731
    for k, s in enumerate(steps):
        G = lambda key: g[f"{name}/{key}"][k]                      # noqa: E731
        checks = {"score": (s["score"], G("score")), "losses": (s["losses"], G("losses")), "dscore": (s["dscore"], G("dscore")),
                  "dW1_sub": (sub(s["grads"]), G("dW1_sub")), "dW1_norm": (np.linalg.norm(s["grads"][:nW]), G("dW1_norm")),
                  "dW2": (s["grads"][nW + HID:nW + 2 * HID], G("dW2")),
                  "W1_sub": (sub(s["params"]), G("W1_sub")), "W1_norm": (np.linalg.norm(s["params"][:nW]), G("W1_norm")),
                  "small": (s["params"][nW:], G("small")), "ema_W1_sub": (sub(s["ema"]), G("ema_W1_sub")),
                  "ema_W1_norm": (np.linalg.norm(s["ema"][:nW]), G("ema_W1_norm")), "ema_small": (s["ema"][nW:], G("ema_small"))}
        for key, (got, want) in checks.items():
            assert rel(got, want) <= 1e-10, (name, k, key, rel(got, want))
        assert abs(s["grads"][:nW].sum() - G("dW1_sum")) <= 1e-10 * np.abs(s["grads"][:nW]).sum()
        assert np.abs(s["grads"][nW:nW + HID]).max() <= 1e-14 and np.abs(G("db1")).max() <= 1e-14
        assert abs(s["grads"][-1]) <= 1e-14 and abs(G("db2")) <= 1e-14
    if c["rw"] > 0:
        assert steps[0]["losses"][2] > 0 and steps[0]["losses"][0] > steps[0]["losses"][1]


def test_gradients_have_the_forms_of_the_issue(golden):
    """the restatement's two-stage gradients equal the collapsed forms the kernels use: dW1 = w2 (x) g, dw2 = W1 g + b1 sum(dscore)"""
    c = load_case(golden("simple_headtrain.npz"), "c")
    W1, b1, w2, b2 = R.unflat(c["prm"], c["C"])
    score, cache = R.forward(c["x"], W1, b1, w2, b2)
    u = W1.T @ w2
    assert rel((c["x"].astype(np.float64) @ u).mean(axis=1) + w2 @ b1 + b2[0], score) <= 1e-13
    _, dscore = R.loss_and_dscore(score, c["y"])
    dW1, db1, dw2, db2 = R.backward(cache, dscore)
    g = np.einsum("b,btc->c", dscore / c["T"], c["x"].astype(np.float64))
    assert rel(np.outer(w2, g), dW1) <= 1e-13 and rel(W1 @ g + b1 * dscore.sum(), dw2) <= 1e-12


def test_symbols_declared_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "kvq_hip.h")).read()
    declared = set(re.findall(r"\b(kvq_[a-z0-9_]+)\s*\(", header))
    handle = _abi.lib()
    for name in NEW:
        assert name in declared and name in _abi.SYMBOLS and hasattr(handle, name), name
    for name in GONE:
        assert name not in declared and name not in _abi.SYMBOLS and not hasattr(handle, name), name
    assert handle.kvq_abi_version() == _abi.ABI_VERSION == 32
    assert set(re.findall(r"KvqHeadTrain\w*", header)) == {"KvqHeadTrainBankArgs"}      # one args struct, in the header and in _abi
    assert [n for n in dir(_abi) if n.startswith("KvqHeadTrain")] == ["KvqHeadTrainBankArgs"]
    assert C.sizeof(_abi.KvqHeadTrainBankArgs) == 120 and C.sizeof(_abi.KvqFeatureBank) == 32
    src = open(os.path.join(ROOT, "kvq-challenge-cvpr-ntire2024_amd", "csrc", "simple_headtrain.hip")).read()
    assert "getenv" not in src and "atomic" not in src.replace("No\n// atomics", "").replace("No atomics", "")


_HOST = (C.c_char * 4112)()


def ws_floats(B, T, Cc):
    """the documented formula (include/kvq_hip.h): u [C] | [B T][nseg] forward partials | g [C] | [nchunks][C] partial column sums"""
    N = B * T
    nseg = -(-Cc // 1024)
    ceil = lambda a, b: -(-a // b)                                 # noqa: E731
    chunk = max(32, 8 * ceil(ceil(N, 32), 8))
    nchunks = ceil(N, chunk)
    return 2 * Cc + -(-N * nseg // 4) * 4 + nchunks * Cc


def test_host_checks_refuse_before_any_launch():
    """NULL: -1; B outside 2 .. 1024, T < 1: -2 (shape); hidden != 128, C not a multiple of 64, p_drop != 0, misalignment: -3
    (unsupported); a short workspace: -4.  No GPU is touched: every pointer is one host buffer."""
    h = _abi.lib()
    P = C.c_void_p((C.addressof(_HOST) + 15) & ~15)
    off = C.c_void_p(P.value + 4)

    def args(feat=P, **kw):
        """the step on an fp32 bank of 7 rows of [8][the step's C], ``feat`` its rows, under a valid index"""
        a = _abi.KvqHeadTrainBankArgs()
        base = dict(index=P, B=4, L=8, C=9472, hidden=128, params=P, p_drop=0.0, seed=0, step=0, workspace=P, workspace_bytes=1 << 30,
                    score=P, dscore=P, grads=P)
        base.update(kw)
        a.bank = _abi.KvqFeatureBank(feat, _abi.DT_FP32, 8, base["C"], 7)
        for k, v in base.items():
            setattr(a, k, v)
        return a

    for fn, who in ((h.kvq_simple_headtrain_bank_forward, b"kvq_simple_headtrain_bank_forward"),
                    (h.kvq_simple_headtrain_bank_backward, b"kvq_simple_headtrain_bank_backward")):
        assert fn(None, None) == -1 and b"NULL" in h.kvq_last_error() and who in h.kvq_last_error()
        assert fn(C.byref(args(feat=None)), None) == -1
        assert fn(C.byref(args(params=None)), None) == -1
        assert fn(C.byref(args(workspace=None)), None) == -1
        assert fn(C.byref(args(B=1)), None) == -2 and b"B 1 " in h.kvq_last_error() and who in h.kvq_last_error()
        assert fn(C.byref(args(B=1025)), None) == -2 and b"B 1025" in h.kvq_last_error()
        assert fn(C.byref(args(L=0)), None) == -2 and b"T 0" in h.kvq_last_error()
        assert fn(C.byref(args(hidden=64)), None) == -3 and b"hidden 64" in h.kvq_last_error() and who in h.kvq_last_error()
        assert fn(C.byref(args(C=0)), None) == -3 and fn(C.byref(args(C=32)), None) == -3
        assert fn(C.byref(args(C=9480)), None) == -3 and b"C 9480" in h.kvq_last_error() and b"multiple of 64" in h.kvq_last_error()
        assert fn(C.byref(args(p_drop=0.5)), None) == -3 and b"p_drop 0.5" in h.kvq_last_error()
        for k in ("feat", "params", "workspace"):
            assert fn(C.byref(args(**{k: off})), None) == -3 and b"aligned" in h.kvq_last_error(), k
        assert fn(C.byref(args(workspace_bytes=4 * ws_floats(4, 8, 9472) - 4)), None) == -4 and b"workspace" in h.kvq_last_error()
    assert h.kvq_simple_headtrain_bank_forward(C.byref(args(score=None)), None) == -1
    assert h.kvq_simple_headtrain_bank_backward(C.byref(args(dscore=None)), None) == -1
    assert h.kvq_simple_headtrain_bank_backward(C.byref(args(grads=None)), None) == -1
    assert h.kvq_simple_headtrain_bank_backward(C.byref(args(grads=off)), None) == -3 and b"grads" in h.kvq_last_error()
    # the VQAHead entries keep their own width
    assert h.kvq_headtrain_bank_forward(C.byref(args(hidden=128, C=768)), None) == -3 and b"hidden 128" in h.kvq_last_error()


def test_workspace_bytes_equal_the_documented_formula():
    ws = _abi.lib().kvq_simple_headtrain_workspace_bytes
    # case a: 32 rows, 10 segments, one run of 32 rows;  case d: 264 rows, one segment, nine runs of 32 rows (the last holds 8)
    assert ws(4, 8, 9472, 128) == 4 * ws_floats(4, 8, 9472) == 4 * (2 * 9472 + 320 + 9472)
    assert ws(33, 8, 704, 128) == 4 * ws_floats(33, 8, 704) == 4 * (2 * 704 + 264 + 9 * 704)
    # case e: 1200 rows, 30 runs of 40 rows
    assert ws(300, 4, 192, 128) == 4 * ws_floats(300, 4, 192) == 4 * (2 * 192 + 1200 + 30 * 192)
    # 2048 rows: 32 runs of 64 rows
    assert ws(256, 8, 9472, 128) == 4 * ws_floats(256, 8, 9472) == 4 * (2 * 9472 + 20480 + 32 * 9472)
    for bad in ((1, 8, 9472, 128), (1025, 8, 9472, 128), (4, 0, 9472, 128), (4, 8, 9472, 64), (4, 8, 100, 128), (4, 8, 0, 128),
                (4, 8, 32, 128)):
        assert ws(*bad) == 0, bad


def test_python_side_refusals():
    from kvq_amd.finetune import HeadFinetuner, SimpleHeadFinetuner, finetuner_for
    from kvq_amd.models.head import VQAHead, simpleVQAHead
    kw = dict(lr=1e-3, wd=0.05, warmup_iters=2, max_iters=10)
    with pytest.raises(NotImplementedError, match="VQAHead"):
        SimpleHeadFinetuner(types.SimpleNamespace(k_head=VQAHead(768, 64)), "k", **kw)
    with pytest.raises(NotImplementedError, match="hidden_channels = 64"):
        SimpleHeadFinetuner(types.SimpleNamespace(simpleVQA_head=simpleVQAHead(in_channels=128, hidden_channels=64)), "simpleVQA", **kw)
    with pytest.raises(NotImplementedError, match="in_channels = 100"):
        SimpleHeadFinetuner(types.SimpleNamespace(simpleVQA_head=simpleVQAHead(in_channels=100, hidden_channels=128)), "simpleVQA", **kw)
    with pytest.raises(NotImplementedError, match="simpleVQAHead"):
        HeadFinetuner(types.SimpleNamespace(simpleVQA_head=simpleVQAHead(in_channels=192, hidden_channels=128)), "simpleVQA", **kw)
    with pytest.raises(KeyError):
        SimpleHeadFinetuner(types.SimpleNamespace(), "simpleVQA", **kw)
    with pytest.raises(ValueError, match="warmup_iters == 0"):
        SimpleHeadFinetuner(types.SimpleNamespace(simpleVQA_head=simpleVQAHead(192, 128)), "simpleVQA", lr=1e-3, wd=0.05, warmup_iters=0,
                            max_iters=10)
    for Cc in (192, 9472):
        head = simpleVQAHead(in_channels=Cc, hidden_channels=128)
        ft = SimpleHeadFinetuner(types.SimpleNamespace(simpleVQA_head=head), "simpleVQA", **kw)
        assert ft.params.numel() == 128 * Cc + 257 and ft.p_drop == 0.0 and ft.current_lr() == 0.0 and ft.it == 0
        assert ft.ema is not ft.params and ft.ema.equal(ft.params)
        assert ft.params[:128 * Cc].equal(head.quality[0].weight.detach().reshape(-1)) and ft.params[-1:].equal(head.quality[1].bias.detach())
        assert finetuner_for(head) is SimpleHeadFinetuner
    assert finetuner_for(VQAHead(768, 64)) is HeadFinetuner


def test_finetune_yml_loads():
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "kwai_simpleVQA_synthetic_finetune.yml")))
    for k in ("num_epochs", "l_num_epochs", "warmup_epochs", "batch_size", "ema", "save_model"):
        assert k in cfg, k
    assert cfg["optimizer"]["backbone_lr_mult"] == 0 and cfg["optimizer"]["lr"] == 1e-3 and cfg["optimizer"]["wd"] == 0.05
    assert cfg["data"]["train"]["type"] == cfg["data"]["val"]["type"] == "SyntheticSimpleVQADataset"
    assert cfg["model"]["type"] == "simpleVQA"
    assert cfg["model"]["args"]["simpleVQA"]["head"] == {"in_channels": 9472, "hidden_channels": 128}
    from kvq_amd.models import VQA_Network
    assert VQA_Network(cfg).key_names == ["simpleVQA"]
