"""GPU: the VQAHead training step (csrc/headtrain.hip, kvq_amd/finetune.py) against the reference's float64 run
(tests/golden/headtrain.npz) through its numpy restatement (tests/headtrain_ref.py, pinned to the fixture by test_headtrain_cpu.py).

Bounds.  The fixture stores, per case, step and tensor, the relative L2 error of the reference's OWN float32 run against its float64 run
(``ref32_err``).  A gradient may miss float64 by 8 x that (the launches add up to 980 tokens in chunk order where torch adds pairwise;
8 x 5e-6 = 4e-5 still keeps any 16-bit rounding, 2^-11 = 4.9e-4, out).  Scores, losses and dscore use the same rule with a floor of
2^-23 under the stored error: a float32 result is not expected within less than a few units in the last place of float64, however
lucky the reference's float32 run was on that tensor.

The tests print every measured error beside its bound; DESIGN.md §8 keeps the figures of the run on an MI355X.
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
import yaml

import kvq_amd  # noqa: F401
from kvq_amd import kernels

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import headtrain_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["a", "b", "c", "d", "e", "e_rank"]
HID = 64
ULP = 2.0 ** -23
_cache = {}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def case(golden, name):
    """the case's inputs and its float64 run (restatement), computed once and shared"""
    if name not in _cache:
        g = golden("headtrain.npz")
        B, D, H, W, Cc, seed = (int(v) for v in g[f"{name}/meta"])
        p, rw = (float(v) for v in g[f"{name}/pw"])
        x, y, prm = R.make_case(seed, B, D * H * W, Cc)
        lr, wd, wu, mx = g["hyper"]
        steps = R.train_steps(x, y, prm, 3, lr, wd, int(wu), int(mx), p=p, seed=seed, rank_weight=rw, db2=g[f"{name}/db2"])
        err = {k: g[f"{name}/ref32_err/{k}"] for k in ("score", "losses", "dscore", "dW1", "db1", "dW2", "dp")}
        _cache[name] = types.SimpleNamespace(B=B, L=D * H * W, C=Cc, seed=seed, p=p, rw=rw, x=x, y=y, prm=prm, steps=steps, err=err,
                                             lr=float(lr), wd=float(wd), wu=int(wu), mx=int(mx), db2_32=g[f"{name}/db2_32"],
                                             adamw32=g[f"{name}/adamw32_err"], nW=HID * Cc)
    return _cache[name]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


@pytest.mark.parametrize("name,which", [("a", 0), ("a", 1), ("b", 0), ("e", 1)])
def test_mask_entry_point_is_bit_equal_to_the_restatement(golden, name, which):
    c = case(golden, name)
    n = c.B * c.L * (c.C if which == 0 else HID)
    for step, p in ((0, c.p), (2, c.p), (1, 0.0), (5, 0.25)):
        got = kernels.headtrain_mask(c.seed, step, which, p, n).cpu().numpy()
        assert np.array_equal(got, R.mask(c.seed, step, which, p, n)), (name, which, step, p)


@pytest.mark.parametrize("name", CASES)
def test_forward_loss_and_gradients_match_float64(golden, name):
    """steps 0 and 1 of the fixture (both run on the initial parameters: the scheduler's first LR is 0): train-mode scores, the loss
    triple and dscore, then dW1, db1, dW2 and db2 of the chain forward -> loss -> backward"""
    c = case(golden, name)
    x, prm, y = dev(c.x), dev(c.prm), dev(c.y)
    ws = kernels.headtrain_workspace(c.B, c.L, c.C)
    for k in (0, 1):
        want = c.steps[k]
        score = kernels.headtrain_forward(x, prm, c.p, c.seed, k, ws)
        out3, dscore = kernels.headtrain_loss(score, y, c.rw)
        grads = kernels.headtrain_backward(x, prm, c.p, c.seed, k, ws, dscore).cpu().numpy()
        got = {"score": score.cpu().numpy(), "losses": out3.cpu().numpy(), "dscore": dscore.cpu().numpy(), "dW1": grads[:c.nW],
               "db1": grads[c.nW:c.nW + HID], "dW2": grads[c.nW + HID:c.nW + 2 * HID]}
        ref = {"score": want["score"], "losses": want["losses"], "dscore": want["dscore"], "dW1": want["grads"][:c.nW],
               "db1": want["grads"][c.nW:c.nW + HID], "dW2": want["grads"][c.nW + HID:c.nW + 2 * HID]}
        errs = {t: rel(got[t], ref[t]) for t in got}
        bound = {t: 8 * (c.err[t][k] if t in ("dW1", "db1", "dW2") else max(c.err[t][k], ULP)) for t in got}
        db2_bound = max(8 * c.db2_32[k], c.B * ULP * np.abs(got["dscore"]).max())
        print(f"case {name} step {k}: " + "  ".join(f"{t} {errs[t]:.2e} ({bound[t]:.2e})" for t in errs)
              + f"  |db2| {abs(grads[-1]):.2e} ({db2_bound:.2e})")
        for t in errs:
            assert errs[t] <= bound[t], (name, k, t, errs[t], bound[t])
        assert max(bound[t] for t in ("dW1", "db1", "dW2")) <= 4e-5
        assert abs(grads[-1]) <= db2_bound
        # the backward alone, fed the float64 dscore rounded to fp32: the same bounds
        g2 = kernels.headtrain_backward(x, prm, c.p, c.seed, k, ws, dev(want["dscore"])).cpu().numpy()
        for t, sl in (("dW1", slice(0, c.nW)), ("db1", slice(c.nW, c.nW + HID)), ("dW2", slice(c.nW + HID, c.nW + 2 * HID))):
            assert rel(g2[sl], ref[t]) <= bound[t], (name, k, t, "backward alone")


@pytest.mark.parametrize("name", ["a", "b", "e_rank"])
def test_adamw_and_ema_alone(golden, name):
    """three AdamW + EMA launches fed the float64 gradients (rounded to fp32) at the schedule's learning rates: p - p0 and the EMA against
    the float64 run, within 8 x what torch's own fp32 AdamW misses it by on the same gradients"""
    c = case(golden, name)
    p, m, v = dev(c.prm), torch.zeros(c.prm.size, device="cuda"), torch.zeros(c.prm.size, device="cuda")
    ema = p.clone()
    for k in range(3):
        kernels.headtrain_adamw(p, dev(c.steps[k]["grads"]), m, v, ema, c.lr * R.lr_factor(k, c.wu, c.mx), c.wd, k + 1)
    last = c.steps[2]
    e_p, e_ema = rel(p.cpu().numpy().astype(np.float64) - c.prm, last["params"] - c.prm), rel(ema.cpu().numpy(), last["ema"])
    print(f"case {name}: p - p0 {e_p:.2e} ({8 * c.adamw32[0]:.2e})  ema {e_ema:.2e} ({8 * c.adamw32[1]:.2e})")
    assert e_p <= 8 * c.adamw32[0] and e_ema <= 8 * c.adamw32[1]
    # ema = NULL: the parameters move the same way, nothing else is written
    p2, m2, v2 = dev(c.prm), torch.zeros_like(m), torch.zeros_like(v)
    for k in range(3):
        kernels.headtrain_adamw(p2, dev(c.steps[k]["grads"]), m2, v2, None, c.lr * R.lr_factor(k, c.wu, c.mx), c.wd, k + 1)
    assert torch.equal(p2, p) and torch.equal(m2, m) and torch.equal(v2, v)


def _chain(c, n_steps):
    x, y = dev(c.x), dev(c.y)
    p, m, v = dev(c.prm), torch.zeros(c.prm.size, device="cuda"), torch.zeros(c.prm.size, device="cuda")
    ema, ws, keep = p.clone(), kernels.headtrain_workspace(c.B, c.L, c.C), []
    for k in range(n_steps):
        score = kernels.headtrain_forward(x, p, c.p, c.seed, k, ws)
        out3, dscore = kernels.headtrain_loss(score, y, c.rw)
        g = kernels.headtrain_backward(x, p, c.p, c.seed, k, ws, dscore)
        kernels.headtrain_adamw(p, g, m, v, ema, c.lr * R.lr_factor(k, c.wu, c.mx), c.wd, k + 1)
        keep += [score, out3, dscore, g.clone()]
    return [p, m, v, ema] + keep


@pytest.mark.parametrize("name", ["b", "e_rank"])
def test_whole_chain_follows_float64_and_is_deterministic(golden, name):
    """three full steps: W1 | b1 | w2 of p - p0 within 8 x the reference's own fp32 run (b2 follows the rounding noise of a zero gradient,
    in the reference as well); two runs from the same state are bit-equal in every output"""
    c = case(golden, name)
    a, b = _chain(c, 3), _chain(c, 3)
    for i, (ta, tb) in enumerate(zip(a, b)):
        assert torch.equal(ta, tb), i
    n = c.nW + 2 * HID
    e = rel(a[0].cpu().numpy().astype(np.float64)[:n] - c.prm[:n], c.steps[2]["params"][:n] - c.prm[:n])
    print(f"case {name}: chain p - p0 {e:.2e} ({8 * c.err['dp'][2]:.2e})")
    assert e <= 8 * c.err["dp"][2]


def test_p0_train_mode_scores_equal_the_inference_head(golden):
    c = case(golden, "c")
    assert c.p == 0.0
    x, prm = dev(c.x), dev(c.prm)
    score = kernels.headtrain_forward(x, prm, 0.0, c.seed, 0, kernels.headtrain_workspace(c.B, c.L, c.C))
    W1, b1, w2, b2 = (dev(t) for t in R.unflat(c.prm, c.C))
    inf = kernels.vqa_head(x.as_strided((c.B, c.C, 1, 1, c.L), (c.L * c.C, 1, c.L * c.C, c.L * c.C, c.C)), W1, b1, w2, b2).reshape(-1)
    bound = 8 * max(c.err["score"][0], ULP)
    assert rel(score.cpu().numpy(), inf.cpu().numpy()) <= bound and rel(inf.cpu().numpy(), c.steps[0]["score"]) <= bound


# ---- end to end on the smallest synthetic geometry of test_gpu_harness.py -------------------------------------------------------------
def _cfg(dropout):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "kwai_swin_grpb_synthetic_finetune.yml")))
    for split in ("train", "val"):
        cfg["data"][split]["args"].update(num_videos=3, frames=64, height=300, width=400)
        cfg["data"][split]["args"]["sample_types"]["technical"].update(clip_len=32, num_clips=2)
    cfg["model"]["args"]["swin_tiny_grpb"]["head"]["dropout_ratio"] = dropout
    return cfg


def _eval_plcc(scores_per_clip, labels):
    return R.plcc_loss(np.asarray(scores_per_clip, np.float64), np.asarray(labels, np.float64))


def test_finetuner_end_to_end(tmp_path, monkeypatch):
    from kvq_amd.finetune import HeadFinetuner
    from kvq_amd.trainer import Trainer
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    cfg = _cfg(0.0)
    tr = Trainer(types.SimpleNamespace(gpu_id="0", resume=str(tmp_path / "ck"), test_set="val"), cfg)
    trunk0 = {k: v.clone() for k, v in tr.model.state_dict().items() if "_backbone." in k}
    ft = HeadFinetuner(tr.model, "swin_tiny_grpb", lr=1e-3, wd=0.0, warmup_iters=3, max_iters=30, ema=True, seed=5)
    assert ft.cache_features(tr.val_dataset, tr) == 3
    feats, labels = ft.clip_samples()
    assert feats.shape == (6, 16 * 7 * 7, 768) and feats.is_contiguous() and labels.shape == (6,)
    x64, y64, p0 = feats.cpu().numpy().astype(np.float64), labels.cpu().numpy().astype(np.float64), ft.params.cpu().numpy().astype(np.float64)
    before = _eval_plcc(ft.predict(feats).cpu().numpy(), y64)
    log = [ft.step(feats, labels) for _ in range(30)]
    ref = R.train_steps(x64, y64, p0, 30, 1e-3, 0.0, 3, 30, p=0.0, seed=5)
    for k in range(5):                             # 4e-5 = the cap of the gradient bound, once per step taken
        d = abs(log[k]["loss"] - ref[k]["losses"][0]) / ref[k]["losses"][0]
        print(f"step {k}: loss {log[k]['loss']:.6f} float64 {ref[k]['losses'][0]:.6f} rel {d:.2e} ({(k + 1) * 4e-5:.1e})")
        assert d <= (k + 1) * 4e-5 and log[k]["lr"] == pytest.approx(1e-3 * R.lr_factor(k, 3, 30), rel=1e-12)
    after = _eval_plcc(ft.predict(feats).cpu().numpy(), y64)
    W1, b1, w2, b2 = R.unflat(ref[-1]["params"], 768)
    after64 = _eval_plcc(R.forward(x64, W1, b1, w2, b2)[0], y64)
    before64 = _eval_plcc(R.forward(x64, *R.unflat(p0, 768))[0], y64)
    print(f"eval PLCC loss {before:.5f} -> {after:.5f}; float64 {before64:.5f} -> {after64:.5f}")
    assert after < before and after64 < before64
    # write_back: the model scores with the trained head; the trunk did not move
    pred = ft.predict(feats)
    ft.write_back()
    item = tr.val_dataset[1]
    with torch.no_grad():
        s_model = tr.model(inputs=tr._model_inputs(item), reduce_scores=True).reshape(-1)
    assert rel(s_model.cpu().numpy(), pred[2:4].cpu().numpy()) <= 1e-5
    sd = tr.model.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in trunk0.items())
    assert torch.equal(sd["swin_tiny_grpb_head.fc_hid.weight"].reshape(-1), ft.params[:64 * 768])
    ft.write_back(ema=True)
    assert torch.equal(tr.model.state_dict()["swin_tiny_grpb_head.fc_last.bias"], ft.ema[-1:])


def test_finetune_head_checkpoint_round_trip(tmp_path, monkeypatch):
    from kvq_amd.trainer import Trainer
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    cfg = _cfg(0.5)
    cfg.update(num_epochs=2, batch_size=3)
    args = types.SimpleNamespace(gpu_id="0", resume=str(tmp_path / "ck"), test_set="val")
    tr = Trainer(args, cfg)
    tr._lane_graphs = "stale"
    best_n, best_s = tr.finetune_head()
    assert tr._lane_graphs is None and len(best_n) == len(best_s) == 4 and tr.finetuner.it == 4
    path = tmp_path / "ck" / "swin_tiny_grpb_synthetic_head_val_n_finetuned.pth"
    assert path.exists() and (tmp_path / "ck" / "swin_tiny_grpb_synthetic_head_val_s_finetuned.pth").exists()
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == {"state_dict", "validation_results"} and all(k.startswith("module.") for k in ck["state_dict"])
    assert "module.swin_tiny_grpb_head.fc_hid.weight" in ck["state_dict"]
    # a fresh model that loads the file scores exactly like a model holding the saved weights
    item = tr.val_dataset[0]
    tr.model.load_state_dict({k[7:]: v for k, v in ck["state_dict"].items()}, strict=False)
    with torch.no_grad():
        want = tr.model(inputs=tr._model_inputs(item), reduce_scores=True).clone()
    torch.manual_seed(1)
    tr2 = Trainer(args, cfg)
    print("load:", tr2.load_weights(str(path)))
    with torch.no_grad():
        got = tr2.model(inputs=tr2._model_inputs(tr2.val_dataset[0]), reduce_scores=True)
    assert torch.equal(got, want)


def test_train_cli_runs_one_epoch(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-o", os.path.join(ROOT, "config", "kwai_swin_grpb_synthetic_finetune.yml"),
                        "-r", str(tmp_path / "ck"), "-t1", "val", "--gpu_id", "0"], cwd=tmp_path, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "SRCC" in r.stdout and "PLCC" in r.stdout and "KRCC" in r.stdout and "RMSE" in r.stdout
    assert "the best validation accuracy of the model-n" in r.stdout
    assert (tmp_path / "ck" / "swin_tiny_grpb_synthetic_head_val_n_finetuned.pth").exists()
