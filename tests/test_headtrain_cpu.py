"""VQAHead training step, everything that needs no GPU: the numpy restatement (tests/headtrain_ref.py) against the reference's stored run
(tests/golden/headtrain.npz), the LR schedule, the mask hash, the new ABI symbols and their host-side refusals, the Python-side
refusals, the yml and train.py's arguments."""
import ctypes as C
import importlib.util
import os
import re
import sys
import types

import numpy as np
import pytest
import torch
import yaml

import kvq_amd  # noqa: F401
from kvq_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import headtrain_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"a": (4, 2, 3, 3, 768, 0.5, 0.0), "b": (5, 4, 7, 7, 768, 0.5, 0.0), "c": (6, 3, 7, 7, 768, 0.0, 0.0),
         "d": (7, 1, 7, 7, 768, 0.5, 0.0), "e": (4, 2, 3, 3, 128, 0.5, 0.0), "e_rank": (4, 2, 3, 3, 128, 0.5, 0.3)}
NEW = ["kvq_headtrain_workspace_bytes", "kvq_headtrain_mask", "kvq_headtrain_loss", "kvq_headtrain_adamw"]
GONE = ["kvq_headtrain_forward", "kvq_headtrain_backward"]         # the dense entries: the step is the bank entries' (ABI 32)
HID = 64


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def load_case(g, name):
    B, D, H, W, Cc, seed = (int(v) for v in g[f"{name}/meta"])
    p, rw = (float(v) for v in g[f"{name}/pw"])
    x, y, prm = R.make_case(seed, B, D * H * W, Cc)
    return dict(B=B, L=D * H * W, C=Cc, seed=seed, p=p, rw=rw, x=x, y=y, prm=prm)


def test_fixture_holds_the_cases_of_the_issue(golden):
    g = golden("headtrain.npz")
    for name, (B, D, H, W, Cc, p, rw) in CASES.items():
        assert tuple(int(v) for v in g[f"{name}/meta"][:5]) == (B, D, H, W, Cc) and tuple(g[f"{name}/pw"]) == (p, rw)
        assert B >= 3
        for k in ("dW1", "db1", "dW2"):
            assert g[f"{name}/ref32_err/{k}"].max() <= 5e-6
        assert np.diff(np.sort(g[f"{name}/score"][0])).min() > 1e-6 and g[f"{name}/score"][0].std() >= 0.1
        c = load_case(g, name)                     # the rebuilt inputs are the ones the reference ran on
        assert np.array_equal(c["x"].reshape(-1)[:256], g[f"{name}/x_head"]) and c["x"].astype(np.float64).sum() == g[f"{name}/x_sum"]
        assert np.array_equal(c["y"], g[f"{name}/labels"])
        nW = HID * Cc
        assert np.array_equal(c["prm"][:nW].reshape(HID, Cc)[:, 5::32], g[f"{name}/params0_sub"])
        assert np.array_equal(c["prm"][nW:], g[f"{name}/params0_small"])


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_reference_run(golden, name):
    """every stored float64 array to 1e-10 relative (W1-shaped ones: subsample, norm and sum).  db2 is analytically zero: both sides hold
    rounding noise (<= 1e-14), and the restatement's AdamW is fed the reference's, since Adam turns that noise into a full step"""
    g = golden("headtrain.npz")
    c = load_case(g, name)
    lr, wd, wu, mx = g["hyper"]
    steps = R.train_steps(c["x"], c["y"], c["prm"], 3, lr, wd, int(wu), int(mx), p=c["p"], seed=c["seed"], rank_weight=c["rw"],
                          db2=g[f"{name}/db2"])
    nW = HID * c["C"]
    sub = lambda v: v[:nW].reshape(HID, c["C"])[:, 5::32]          # noqa: E731
    for k, s in enumerate(steps):
        G = lambda key: g[f"{name}/{key}"][k]                      # noqa: E731
        checks = {"score": (s["score"], G("score")), "losses": (s["losses"], G("losses")), "dscore": (s["dscore"], G("dscore")),
                  "dW1_sub": (sub(s["grads"]), G("dW1_sub")), "dW1_norm": (np.linalg.norm(s["grads"][:nW]), G("dW1_norm")),
                  "db1": (s["grads"][nW:nW + HID], G("db1")), "dW2": (s["grads"][nW + HID:nW + 2 * HID], G("dW2")),
                  "W1_sub": (sub(s["params"]), G("W1_sub")), "W1_norm": (np.linalg.norm(s["params"][:nW]), G("W1_norm")),
                  "small": (s["params"][nW:], G("small")), "ema_W1_sub": (sub(s["ema"]), G("ema_W1_sub")),
                  "ema_W1_norm": (np.linalg.norm(s["ema"][:nW]), G("ema_W1_norm")), "ema_small": (s["ema"][nW:], G("ema_small"))}
        for key, (got, want) in checks.items():
            assert rel(got, want) <= 1e-10, (name, k, key, rel(got, want))
        assert abs(s["grads"][:nW].sum() - G("dW1_sum")) <= 1e-10 * np.abs(s["grads"][:nW]).sum()
        assert abs(s["grads"][-1]) <= 1e-14 and abs(G("db2")) <= 1e-14
    if c["rw"] > 0:
        assert steps[0]["losses"][2] > 0 and steps[0]["losses"][0] > steps[0]["losses"][1]


def test_lr_factors(golden):
    from kvq_amd.finetune import lr_factor
    want = golden("headtrain.npz")["lr_factors"]
    assert want.shape == (12,) and want[0] == 0.0 and want[2] == 1.0
    assert [R.lr_factor(i, 2, 10) for i in range(12)] == list(want)
    assert [lr_factor(i, 2, 10) for i in range(12)] == list(want)


@pytest.mark.parametrize("name", ["a", "c", "e"])
def test_mask_bits_and_kept_share(golden, name):
    g = golden("headtrain.npz")
    c = load_case(g, name)
    n1, n2 = c["B"] * c["L"] * c["C"], c["B"] * c["L"] * HID
    m1, m2 = R.mask(c["seed"], 0, 0, c["p"], n1), R.mask(c["seed"], 0, 1, c["p"], n2)
    assert np.array_equal(np.packbits(m1[:65536]), g[f"{name}/m1_bits"]) and np.array_equal(np.packbits(m2), g[f"{name}/m2_bits"])
    for m in (m1, m2):
        sigma = np.sqrt(c["p"] * (1 - c["p"]) / m.size)
        assert abs(m.mean() - (1 - c["p"])) <= 3 * sigma
    if c["p"] > 0:                                # the two dropouts and two steps draw different masks
        assert 0.4 < (m1[:n2] == m2).mean() < 0.6
        assert 0.4 < (m1 == R.mask(c["seed"], 1, 0, c["p"], n1)).mean() < 0.6
    for p in (0.1, 0.9):
        m = R.mask(7, 3, 0, p, 1 << 18)
        assert abs(m.mean() - (1 - np.float32(p))) <= 3 * np.sqrt(p * (1 - p) / m.size)


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
    src = open(os.path.join(ROOT, "kvq-challenge-cvpr-ntire2024_amd", "csrc", "headtrain.hip")).read()
    assert "getenv" not in src and "atomic" not in src.replace("No atomics", "")


_HOST = (C.c_char * 4112)()


def test_host_checks_refuse_before_any_launch():
    """NULL: -1; hidden != 64, C not a multiple of 64, p outside [0, 1): -3 (unsupported); B < 2, B > 1024 in the loss: -2 (shape);
    a short workspace: -4.  No GPU is touched: every pointer is one host buffer."""
    h = _abi.lib()
    P = C.c_void_p((C.addressof(_HOST) + 15) & ~15)

    def args(feat=P, **kw):
        """the step on an fp32 bank of 7 rows of the step's own (L, C), ``feat`` its rows, under a valid index"""
        a = _abi.KvqHeadTrainBankArgs()
        base = dict(index=P, B=4, L=18, C=768, hidden=64, params=P, p_drop=0.5, seed=1, step=0, workspace=P, workspace_bytes=1 << 30,
                    score=P, dscore=P, grads=P)
        base.update(kw)
        a.bank = _abi.KvqFeatureBank(feat, _abi.DT_FP32, base["L"], base["C"], 7)
        for k, v in base.items():
            setattr(a, k, v)
        return a

    for fn in (h.kvq_headtrain_bank_forward, h.kvq_headtrain_bank_backward):
        assert fn(None, None) == -1 and b"NULL" in h.kvq_last_error()
        assert fn(C.byref(args(feat=None)), None) == -1
        assert fn(C.byref(args(params=None)), None) == -1
        assert fn(C.byref(args(workspace=None)), None) == -1
        assert fn(C.byref(args(hidden=32)), None) == -3 and b"hidden 32" in h.kvq_last_error()
        assert fn(C.byref(args(C=100)), None) == -3 and b"multiple of 64" in h.kvq_last_error()
        assert fn(C.byref(args(p_drop=1.0)), None) == -3
        assert fn(C.byref(args(B=1)), None) == -2 and b"B 1" in h.kvq_last_error()
        assert fn(C.byref(args(L=0)), None) == -2
        assert fn(C.byref(args(B=1024, L=8192, C=768)), None) == -2 and b"32-bit" in h.kvq_last_error()
        assert fn(C.byref(args(feat=C.c_void_p(P.value + 4))), None) == -3 and b"aligned" in h.kvq_last_error()
        assert fn(C.byref(args(workspace_bytes=1024)), None) == -4
    assert h.kvq_headtrain_bank_forward(C.byref(args(score=None)), None) == -1
    assert h.kvq_headtrain_bank_backward(C.byref(args(dscore=None)), None) == -1
    assert h.kvq_headtrain_bank_backward(C.byref(args(grads=None)), None) == -1
    ws = h.kvq_headtrain_workspace_bytes
    assert ws(1, 18, 768, 64) == 0 and ws(4, 18, 100, 64) == 0 and ws(4, 18, 768, 32) == 0 and ws(4, 0, 768, 64) == 0
    # z and dz [72][64], 72 token scores, one chunk (80 tokens) of dW1 partials [64][768], two 64-token runs of db1 and dw2 partials
    assert ws(4, 18, 768, 64) == 4 * (2 * 72 * 64 + 72 + 64 * 768 + 2 * 2 * 64)
    # four chunks of 256 tokens, four runs each
    assert ws(5, 196, 768, 64) == 4 * (2 * 980 * 64 + 980 + 4 * 64 * 768 + 2 * 16 * 64)
    assert h.kvq_headtrain_loss(None, P, 4, 0.0, P, P, None) == -1 and h.kvq_headtrain_loss(P, P, 4, 0.0, P, None, None) == -1
    assert h.kvq_headtrain_loss(P, P, 1, 0.0, P, P, None) == -2 and h.kvq_headtrain_loss(P, P, 1025, 0.0, P, P, None) == -2
    assert h.kvq_headtrain_mask(1, 0, 0, 0.5, 16, None, None) == -1
    assert h.kvq_headtrain_mask(1, 0, 2, 0.5, 16, P, None) == -3 and h.kvq_headtrain_mask(1, 0, 0, 1.0, 16, P, None) == -3
    assert h.kvq_headtrain_mask(1, 0, 0, 0.5, 0, P, None) == -2 and h.kvq_headtrain_mask(1, 0, 0, 0.5, (1 << 32) + 1, P, None) == -2
    assert h.kvq_headtrain_adamw(None, P, P, P, None, 16, 1e-3, 0.05, 1, None) == -1
    assert h.kvq_headtrain_adamw(P, P, P, P, None, 16, 1e-3, 0.05, 0, None) == -2 and h.kvq_headtrain_adamw(P, P, P, P, None, 0, 1e-3, 0.05, 1, None) == -2


def test_python_side_refusals():
    from kvq_amd.finetune import HeadFinetuner
    from kvq_amd.models.head import VQAHead, simpleVQAHead
    from kvq_amd.trainer import Trainer
    kw = dict(lr=1e-3, wd=0.05, warmup_iters=2, max_iters=10)
    with pytest.raises(NotImplementedError, match="simpleVQAHead"):
        HeadFinetuner(types.SimpleNamespace(simpleVQA_head=simpleVQAHead(in_channels=64, hidden_channels=8)), "simpleVQA", **kw)
    with pytest.raises(NotImplementedError, match="num_class"):
        HeadFinetuner(types.SimpleNamespace(k_head=VQAHead(768, 64, num_class=5)), "k", **kw)
    with pytest.raises(NotImplementedError, match="pre_pool"):
        HeadFinetuner(types.SimpleNamespace(k_head=VQAHead(768, 64, pre_pool=True)), "k", **kw)
    with pytest.raises(NotImplementedError, match="hidden_channels 64"):
        HeadFinetuner(types.SimpleNamespace(k_head=VQAHead(768, 32)), "k", **kw)
    with pytest.raises(ValueError, match="warmup_iters == 0"):
        HeadFinetuner(types.SimpleNamespace(k_head=VQAHead(768, 64)), "k", lr=1e-3, wd=0.05, warmup_iters=0, max_iters=10)
    ft = HeadFinetuner(types.SimpleNamespace(k_head=VQAHead(768, 64)), "k", **kw)
    assert ft.params.numel() == 64 * 768 + 129 and ft.p_drop == 0.5 and ft.current_lr() == 0.0
    with pytest.raises(NotImplementedError, match="frozen"):
        Trainer.finetune_head(types.SimpleNamespace(config={"optimizer": {"lr": 1e-3, "wd": 0.05, "backbone_lr_mult": 1}}))


def test_finetune_yml_loads_and_train_py_parses_the_reference_arguments():
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "kwai_swin_grpb_synthetic_finetune.yml")))
    for k in ("num_epochs", "l_num_epochs", "warmup_epochs", "batch_size", "ema", "save_model"):
        assert k in cfg, k
    assert cfg["optimizer"]["backbone_lr_mult"] == 0 and cfg["optimizer"]["lr"] == 1e-3 and cfg["optimizer"]["wd"] == 0.05
    assert cfg["data"]["train"]["type"] == cfg["data"]["val"]["type"] == "SyntheticKVQDataset"
    from kvq_amd.models import VQA_Network
    assert VQA_Network(cfg).key_names == ["swin_tiny_grpb"]
    spec = importlib.util.spec_from_file_location("kvq_train_cli", os.path.join(ROOT, "train.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.build_parser().parse_args(["-o", "x.yml", "-t", "train", "-t1", "val-ltest", "-r", "./ck/", "--gpu_id", "0"])
    assert (a.opt, a.train_set, a.test_set, a.resume, a.gpu_id) == ("x.yml", "train", "val-ltest", "./ck/", "0")
    d = cli.build_parser().parse_args([])
    assert d.test_set == "val-ltest" and d.resume == "./checkpoint/" and d.train_set == "train"
