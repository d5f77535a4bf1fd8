"""GPU: the simpleVQAHead training step (csrc/simple_headtrain.hip, kvq_amd/finetune.py) against the reference's float64 run
(tests/golden/simple_headtrain.npz) through its numpy restatement (tests/simple_headtrain_ref.py, pinned to the fixture by
test_simple_headtrain_cpu.py).

Bounds.  The fixture stores, per case, step and tensor, the relative L2 error against float64 of two float32 runs of the reference's own
code: as it is (``ref32_err``) and with the channels reversed (``alt32_err``: the same mathematics in another summation order).  A result
may miss float64 by 8 x the larger of the two (8 x 5e-6 = 4e-5 still keeps any 16-bit rounding, 2^-11 = 4.9e-4, out).  Scores, losses
and dscore use the same rule with a floor of 2^-23 under the stored error: a float32 result is not expected within less than a few units
in the last place of float64, however lucky the reference's float32 runs were on that tensor.

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
import simple_headtrain_ref as R  # noqa: E402
from guarded import guarded  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YML = os.path.join(ROOT, "config", "kwai_simpleVQA_synthetic_finetune.yml")
CASES = ["a", "b", "c", "d", "c_rank", "e"]
HID = 128
ULP = 2.0 ** -23
_cache = {}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def case(golden, name):
    """the case's inputs and its float64 run (restatement), computed once and shared"""
    if name not in _cache:
        g = golden("simple_headtrain.npz")
        B, T, Cc, seed = (int(v) for v in g[f"{name}/meta"])
        rw = float(g[f"{name}/rw"])
        x, y, prm = R.make_case(seed, B, T, Cc)
        lr, wd, wu, mx = g["hyper"]
        zero = np.concatenate([g[f"{name}/db1"], g[f"{name}/db2"][:, None]], axis=1)
        steps = R.train_steps(x, y, prm, 3, lr, wd, int(wu), int(mx), rank_weight=rw, zero_grads=zero)
        err = {k: np.maximum(g[f"{name}/ref32_err/{k}"], g[f"{name}/alt32_err/{k}"]) for k in ("score", "losses", "dscore", "dW1", "dW2", "dp")}
        _cache[name] = types.SimpleNamespace(B=B, T=T, C=Cc, seed=seed, rw=rw, x=x, y=y, prm=prm, steps=steps, err=err, lr=float(lr),
                                             wd=float(wd), wu=int(wu), mx=int(mx), db1_32=g[f"{name}/db1_32"].max(axis=0),
                                             db2_32=g[f"{name}/db2_32"].max(axis=0), nW=HID * Cc)
    return _cache[name]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _cut(c, flat):
    return {"dW1": flat[:c.nW], "db1": flat[c.nW:c.nW + HID], "dW2": flat[c.nW + HID:c.nW + 2 * HID], "db2": flat[-1]}


@pytest.mark.parametrize("name", CASES)
def test_forward_loss_and_gradients_match_float64(golden, name):
    """steps 0 and 1 of the fixture (both run on the initial parameters: the scheduler's first LR is 0): scores, the loss triple and
    dscore, then dW1 (the full tensor), dW2 and the analytically-zero db1 and db2 of the chain forward -> loss -> backward; then the
    backward alone, fed the float64 dscore"""
    c = case(golden, name)
    x, prm, y = dev(c.x), dev(c.prm), dev(c.y)
    ws = kernels.simple_headtrain_workspace(c.B, c.T, c.C)
    w2max = np.abs(c.prm[c.nW + HID:c.nW + 2 * HID]).max()
    for k in (0, 1):
        want = c.steps[k]
        score = kernels.simple_headtrain_forward(x, prm, ws)
        out3, dscore = kernels.headtrain_loss(score, y, c.rw)
        grads = _cut(c, kernels.simple_headtrain_backward(x, prm, ws, dscore).cpu().numpy())
        ref = _cut(c, want["grads"])
        got = {"score": score.cpu().numpy(), "losses": out3.cpu().numpy(), "dscore": dscore.cpu().numpy(), "dW1": grads["dW1"],
               "dW2": grads["dW2"]}
        ref.update(score=want["score"], losses=want["losses"], dscore=want["dscore"])
        errs = {t: rel(got[t], ref[t]) for t in got}
        bound = {t: 8 * (c.err[t][k] if t in ("dW1", "dW2") else max(c.err[t][k], ULP)) for t in got}
        dmax = np.abs(got["dscore"]).max()
        db2_bound = max(8 * c.db2_32[k], c.B * ULP * dmax)
        db1_bound = max(8 * c.db1_32[k], c.B * ULP * dmax * w2max)
        print(f"case {name} step {k}: " + "  ".join(f"{t} {errs[t]:.2e} ({bound[t]:.2e})" for t in errs)
              + f"  |db2| {abs(grads['db2']):.2e} ({db2_bound:.2e})  max|db1| {np.abs(grads['db1']).max():.2e} ({db1_bound:.2e})")
        for t in errs:
            assert errs[t] <= bound[t], (name, k, t, errs[t], bound[t])
        assert max(bound[t] for t in ("dW1", "dW2")) <= 4e-5
        assert abs(grads["db2"]) <= db2_bound and np.abs(grads["db1"]).max() <= db1_bound
        # the backward alone, fed the float64 dscore rounded to fp32: the same bounds
        d64 = dev(want["dscore"])
        g2 = _cut(c, kernels.simple_headtrain_backward(x, prm, ws, d64).cpu().numpy())
        d64max = float(d64.abs().max())
        for t in ("dW1", "dW2"):
            e = rel(g2[t], ref[t])
            print(f"    backward alone: {t} {e:.2e} ({bound[t]:.2e})")
            assert e <= bound[t], (name, k, t, "backward alone")
        assert abs(g2["db2"]) <= max(8 * c.db2_32[k], c.B * ULP * d64max)
        assert np.abs(g2["db1"]).max() <= max(8 * c.db1_32[k], c.B * ULP * d64max * w2max)


@pytest.mark.parametrize("name", CASES)
def test_dw1_is_rank_one(golden, name):
    """every row of the returned dW1, divided by its w2[j], is row 0 divided by w2[0], to 4 * 2^-23 relative"""
    c = case(golden, name)
    x, prm = dev(c.x), dev(c.prm)
    g = kernels.simple_headtrain_backward(x, prm, kernels.simple_headtrain_workspace(c.B, c.T, c.C), dev(c.steps[0]["dscore"]))
    dW1 = g[:c.nW].cpu().numpy().astype(np.float64).reshape(HID, c.C)
    w2 = prm[c.nW + HID:c.nW + 2 * HID].cpu().numpy().astype(np.float64)
    rows = dW1 / w2[:, None]
    worst = max(rel(rows[j], rows[0]) for j in range(1, HID))
    print(f"case {name}: rank-one residual {worst:.2e} ({4 * ULP:.2e})")
    assert worst <= 4 * ULP


def _chain(c, n_steps):
    x, y = dev(c.x), dev(c.y)
    p, m, v = dev(c.prm), torch.zeros(c.prm.size, device="cuda"), torch.zeros(c.prm.size, device="cuda")
    ema, ws, keep = p.clone(), kernels.simple_headtrain_workspace(c.B, c.T, c.C), []
    for k in range(n_steps):
        score = kernels.simple_headtrain_forward(x, p, ws)
        out3, dscore = kernels.headtrain_loss(score, y, c.rw)
        g = kernels.simple_headtrain_backward(x, p, ws, dscore)
        kernels.headtrain_adamw(p, g, m, v, ema, c.lr * R.lr_factor(k, c.wu, c.mx), c.wd, k + 1)
        keep += [score, out3, dscore, g.clone()]
    return [p, m, v, ema] + keep


@pytest.mark.parametrize("name", ["a", "c_rank"])
def test_whole_chain_follows_float64_and_is_deterministic(golden, name):
    """three full steps: W1 | w2 of p - p0 within 8 x the reference's own fp32 runs; two runs from the same state are bit-equal in every
    output.  b1 and b2 are left out: their gradients are analytically zero (sum_b dscore = 0 for both losses), what an implementation
    holds there is rounding noise, and Adam's normalisation turns noise into steps of +-lr, in the reference as well.  Nothing else
    depends on where they go: a common shift of b1 or of b2 moves every score by one constant, which neither loss sees."""
    c = case(golden, name)
    a, b = _chain(c, 3), _chain(c, 3)
    for i, (ta, tb) in enumerate(zip(a, b)):
        assert torch.equal(ta, tb), i
    pick = lambda v: np.concatenate([v[:c.nW], v[c.nW + HID:c.nW + 2 * HID]])          # noqa: E731
    e = rel(pick(a[0].cpu().numpy().astype(np.float64) - c.prm), pick(c.steps[2]["params"] - c.prm))
    print(f"case {name}: chain p - p0 {e:.2e} ({8 * c.err['dp'][2]:.2e})")
    assert e <= 8 * c.err["dp"][2]


@pytest.mark.parametrize("name", ["a", "c"])
def test_train_mode_scores_equal_the_inference_head(golden, name):
    c = case(golden, name)
    x, prm = dev(c.x), dev(c.prm)
    score = kernels.simple_headtrain_forward(x, prm, kernels.simple_headtrain_workspace(c.B, c.T, c.C))
    W1, b1, w2, b2 = (dev(t) for t in R.unflat(c.prm, c.C))
    inf = kernels.simple_vqa_head(x, W1, b1, w2, b2).reshape(-1)
    bound = 8 * max(c.err["score"][0], ULP)
    e_ti, e_i = rel(score.cpu().numpy(), inf.cpu().numpy()), rel(inf.cpu().numpy(), c.steps[0]["score"])
    print(f"case {name}: train vs inference {e_ti:.2e}, inference vs float64 {e_i:.2e} ({bound:.2e})")
    assert e_ti <= bound and e_i <= bound


def test_guard_bands_intact_and_outputs_fully_written(golden):
    """one full step on case b (15 rows: fewer than a 32-row run, three-row videos; ten channel segments, the last of 256) with every
    tensor in a guard-band buffer: no launch stores outside a tensor, a read outside would turn the results into NaN, and score, the loss
    triple, dscore and the flat gradient are written in full"""
    c = case(golden, "b")
    with guarded("cuda", max_guard=1 << 20) as G:      # the flat vectors are one 4.8 MB row each: 1 MiB of guard either side, not 32 rows
        x, p, y = G.wrap(dev(c.x), name="feat"), G.wrap(dev(c.prm), name="params"), G.wrap(dev(c.y), name="labels")
        m, v = G.wrap(torch.zeros_like(p), name="exp_avg"), G.wrap(torch.zeros_like(p), name="exp_avg_sq")
        ema = G.wrap(p.clone(), name="ema")
        ws = kernels.simple_headtrain_workspace(c.B, c.T, c.C)
        score = kernels.simple_headtrain_forward(x, p, ws)
        out3, dscore = kernels.headtrain_loss(score, y, c.rw)
        grads = kernels.simple_headtrain_backward(x, p, ws, dscore)
        kernels.headtrain_adamw(p, grads, m, v, ema, c.lr, c.wd, 1)
        report = G.intact()
        assert report, repr(report)
        for name, t in (("score", score), ("out3", out3), ("dscore", dscore), ("grads", grads)):
            assert not bool(G.payload_left(t).any()), name
        for t in (score, out3, dscore, grads, p, m, v, ema):
            assert bool(torch.isfinite(t).all())
    assert rel(score.cpu().numpy(), c.steps[0]["score"]) <= 8 * max(c.err["score"][0], ULP)
    assert rel(grads[:c.nW].cpu().numpy(), c.steps[0]["grads"][:c.nW]) <= 8 * c.err["dW1"][0]


# ---- end to end on the small synthetic geometry test_gpu_harness.py uses for this key ---------------------------------------------------
def _cfg(tmp_path):
    """the yml (8 training videos, 4 validation videos; the synthetic videos of the two sets are the same ones) at resize 130 / crop 112
    on videos of 80 frames, with non-zero SlowFast feature files so that their columns carry gradient"""
    cfg = yaml.safe_load(open(YML))
    g = np.random.Generator(np.random.PCG64(77))
    assert cfg["data"]["train"]["args"]["num_videos"] == 8 and cfg["data"]["val"]["args"]["num_videos"] == 4
    for i in range(8):
        d = tmp_path / "feat" / f"synthetic_{i:05d}"
        d.mkdir(parents=True, exist_ok=True)
        for k in range(8):
            np.save(str(d / f"feature_{k}_slow_feature.npy"), np.abs(g.standard_normal(2048)).astype(np.float32))
            np.save(str(d / f"feature_{k}_fast_feature.npy"), np.abs(g.standard_normal(256)).astype(np.float32))
    for split in ("train", "val"):
        cfg["data"][split]["args"].update(frames=80, height=135, width=240, data_prefix_3D=str(tmp_path / "feat"))
        cfg["data"][split]["args"]["sample_types"]["simpleVQA"].update(resize=130, crop=112)
    return cfg


def _eval_plcc(scores, labels):
    return R.plcc_loss(np.asarray(scores, np.float64), np.asarray(labels, np.float64))


def test_finetuner_end_to_end(tmp_path, monkeypatch):
    from kvq_amd.finetune import SimpleHeadFinetuner
    from kvq_amd.trainer import Trainer
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    tr = Trainer(types.SimpleNamespace(gpu_id="0", resume=str(tmp_path / "ck"), test_set="val"), _cfg(tmp_path))
    trunk0 = {k: v.clone() for k, v in tr.model.state_dict().items() if "_backbone." in k}
    ft = SimpleHeadFinetuner(tr.model, "simpleVQA", lr=1e-3, wd=0.0, warmup_iters=3, max_iters=30, ema=True, seed=5)
    assert ft.cache_features(tr.val_dataset, tr) == 4
    feats, labels = ft.clip_samples()
    assert feats.shape == (4, 8, 9472) and feats.is_contiguous() and labels.shape == (4,)
    assert float(feats[:, :, 7168:].abs().min()) > 0               # the SlowFast columns come from the files
    x64, y64, p0 = feats.cpu().numpy().astype(np.float64), labels.cpu().numpy().astype(np.float64), ft.params.cpu().numpy().astype(np.float64)
    before = _eval_plcc(ft.predict(feats).cpu().numpy(), y64)
    log = [ft.step(feats, labels) for _ in range(30)]
    assert ft.it == 30
    ref = R.train_steps(x64, y64, p0, 30, 1e-3, 0.0, 3, 30)
    for k in range(5):                             # 4e-5 = the cap of the gradient bound, once per step taken
        d = abs(log[k]["loss"] - ref[k]["losses"][0]) / ref[k]["losses"][0]
        print(f"step {k}: loss {log[k]['loss']:.6f} float64 {ref[k]['losses'][0]:.6f} rel {d:.2e} ({(k + 1) * 4e-5:.1e})")
        assert d <= (k + 1) * 4e-5 and log[k]["lr"] == pytest.approx(1e-3 * R.lr_factor(k, 3, 30), rel=1e-12)
    after = _eval_plcc(ft.predict(feats).cpu().numpy(), y64)
    after64 = _eval_plcc(R.forward(x64, *R.unflat(ref[-1]["params"], 9472))[0], y64)
    before64 = _eval_plcc(R.forward(x64, *R.unflat(p0, 9472))[0], y64)
    print(f"eval PLCC loss {before:.5f} -> {after:.5f}; float64 {before64:.5f} -> {after64:.5f}")
    assert after < before and after64 < before64
    # write_back: the model scores with the trained head; the trunk did not move
    pred = ft.predict(feats)
    tr._lane_graphs = "stale"
    ft.write_back()
    assert tr._lane_graphs is None
    item = tr.val_dataset[1]
    with torch.no_grad():
        s_model = tr.model(inputs=tr._model_inputs(item), reduce_scores=True).reshape(-1)
    assert rel(s_model.cpu().numpy(), pred[1:2].cpu().numpy()) <= 1e-5
    sd = tr.model.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in trunk0.items())
    assert torch.equal(sd["simpleVQA_head.quality.0.weight"].reshape(-1), ft.params[:128 * 9472])
    ft.write_back(ema=True)
    assert torch.equal(tr.model.state_dict()["simpleVQA_head.quality.1.bias"], ft.ema[-1:])


def test_finetune_head_checkpoint_round_trip(tmp_path, monkeypatch):
    from kvq_amd.finetune import SimpleHeadFinetuner
    from kvq_amd.trainer import Trainer
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    cfg = _cfg(tmp_path)
    assert cfg["num_epochs"] == 2 and cfg["batch_size"] == 4
    args = types.SimpleNamespace(gpu_id="0", resume=str(tmp_path / "ck"), test_set="val")
    tr = Trainer(args, cfg)
    tr._lane_graphs = "stale"
    best_n, best_s = tr.finetune_head()
    assert isinstance(tr.finetuner, SimpleHeadFinetuner)
    assert tr._lane_graphs is None and len(best_n) == len(best_s) == 4 and tr.finetuner.it == 4
    path = tmp_path / "ck" / "simpleVQA_synthetic_head_val_n_finetuned.pth"
    assert path.exists() and (tmp_path / "ck" / "simpleVQA_synthetic_head_val_s_finetuned.pth").exists()
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == {"state_dict", "validation_results"} and all(k.startswith("module.") for k in ck["state_dict"])
    assert "module.simpleVQA_head.quality.0.weight" in ck["state_dict"]
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


def test_train_cli_runs_the_yml(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-o", YML, "-r", str(tmp_path / "ck"), "-t1", "val", "--gpu_id", "0"],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "SRCC" in r.stdout and "PLCC" in r.stdout and "KRCC" in r.stdout and "RMSE" in r.stdout
    assert "the best validation accuracy of the model-n" in r.stdout
    assert (tmp_path / "ck" / "simpleVQA_synthetic_head_val_n_finetuned.pth").exists()
