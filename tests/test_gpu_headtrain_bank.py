"""GPU: the feature bank of head fine-tuning (csrc/featbank.hip, the bank entries of csrc/headtrain.hip and csrc/simple_headtrain.hip,
kvq_amd/finetune.py).  No tolerance anywhere: widening a 16-bit row is exact and the launches keep their summation orders, so every
bank path is compared bit for bit with the dense fp32 step on the widened rows (which tests/test_gpu_headtrain.py and
tests/test_gpu_simple_headtrain.py pin to float64), and the store with torch's own rounding."""
import hashlib
import os
import random
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
import simple_headtrain_ref as SR  # noqa: E402
from guarded import guarded  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def vqa_case(golden, name):
    g = golden("headtrain.npz")
    B, D, H, W, Cc, seed = (int(v) for v in g[f"{name}/meta"])
    p, rw = (float(v) for v in g[f"{name}/pw"])
    x, y, prm = R.make_case(seed, B, D * H * W, Cc)
    return types.SimpleNamespace(B=B, L=D * H * W, C=Cc, seed=seed, p=p, rw=rw, x=x, y=y, prm=prm)


def simple_case(golden, name):
    g = golden("simple_headtrain.npz")
    B, T, Cc, seed = (int(v) for v in g[f"{name}/meta"])
    x, y, prm = SR.make_case(seed, B, T, Cc)
    return types.SimpleNamespace(B=B, L=T, C=Cc, seed=seed, rw=float(g[f"{name}/rw"]), x=x, y=y, prm=prm)


def random_bank(c, dtype, seed):
    """3 B random rows of the case's (L, C) and an index of B of them, shuffled, with one row taken twice"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(3 * c.B, c.L, c.C, generator=g).to(dtype).cuda()
    idx = torch.randperm(3 * c.B, generator=g)[:c.B].clone()
    idx[-1] = idx[0]
    return kernels.FeatureBank.of(rows), idx.to(torch.int32).cuda()


# ---- the store ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
def test_store_rounds_as_torch_and_touches_only_its_rows(dtype):
    from kvq_amd.finetune import HeadFinetuner
    n, L, Cc, first, sentinel = 2, 18, 128, 3, 7.0
    g = torch.Generator().manual_seed(11)
    # magnitudes from fp16's subnormals to just under 6e4, inside a larger allocation: the features are a strided view
    big = (torch.randn(n, L + 2, Cc + 32, generator=g) * 10.0 ** (torch.rand(n, L + 2, Cc + 32, generator=g) * 12.7 - 8.0)).clamp(-5.9e4, 5.9e4)
    big = big.cuda()
    feat = big[:, 1:L + 1, 16:16 + Cc]
    assert feat.stride() == ((L + 2) * (Cc + 32), Cc + 32, 1) and float(feat.abs().max()) < 6e4
    # the trunk's output: a (n, C, D, H, W) view of channels-last storage; the finetuner's view of it is the same memory, not a copy
    feat5 = feat.permute(0, 2, 1).unflatten(2, (2, 3, 3))
    assert feat5.shape == (n, Cc, 2, 3, 3)
    view = HeadFinetuner._clip_features(None, feat5)
    assert view.data_ptr() == feat.data_ptr() and view.stride() == feat.stride() and view.shape == feat.shape
    with guarded("cuda") as G:
        rows = G.wrap(torch.full((7, L, Cc), sentinel, dtype=dtype, device="cuda"), name="bank")
        bank = kernels.FeatureBank.of(rows)
        flag = G.wrap(torch.zeros(1, dtype=torch.int32, device="cuda"), name="flag")
        kernels.feature_bank_store(view, bank, first, flag)
        assert torch.equal(bits(rows[first:first + n]), bits(feat.to(dtype)))
        keep = torch.ones(7, dtype=torch.bool)
        keep[first:first + n] = False
        assert bool((rows[keep.cuda()] == sentinel).all()) and int(flag.item()) == 0
        report = G.intact()
        assert report, repr(report)
        # a NULL flag is allowed
        kernels.feature_bank_store(view, bank, 0, None)
        assert torch.equal(bits(rows[0:n]), bits(feat.to(dtype)))
        # values fp16 cannot hold, and a NaN
        bad = feat.clone()
        bad[0, 0, 0], bad[1, 17, 127], bad[0, 5, 64] = 1e5, -1e5, float("inf")
        kernels.feature_bank_store(bad, bank, 5, flag)
        want = bad.clamp(-65504.0, 65504.0).to(dtype) if dtype == torch.float16 else bad.to(dtype)
        assert torch.equal(bits(rows[5:7]), bits(want))
        if dtype == torch.float16:
            assert rows[5, 0, 0] == 65504 and rows[6, 17, 127] == -65504 and rows[5, 5, 64] == 65504
        assert int(flag.item()) == (1 if dtype == torch.float16 else 0)
        flag.zero_()
        bad[1, 3, 5] = float("nan")
        kernels.feature_bank_store(bad, bank, 5, flag)
        assert bool(torch.isnan(rows[6, 3, 5])) and int(flag.item()) == 1
        got, ref = rows[5:7].clone(), want.clone()
        got[1, 3, 5] = ref[1, 3, 5] = 0
        assert torch.equal(bits(got), bits(ref))                   # everything but the NaN is what it was
        assert bool((rows[2] == sentinel).all())
        report = G.intact()
        assert report, repr(report)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
def test_rows_gathers_and_widens_with_the_index_clamped(dtype):
    g = torch.Generator().manual_seed(3)
    rows = torch.randn(7, 18, 128, generator=g).to(dtype).cuda()
    bank = kernels.FeatureBank.of(rows)
    idx = torch.tensor([2, 2, 9, -3, 0, 6, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32).cuda()     # a device index is clamped, not refused
    with guarded("cuda") as G:
        out = kernels.feature_bank_rows(bank, idx)
        report = G.intact()
        assert report, repr(report)
        assert not bool(G.payload_left(out).any())
    want = rows[torch.tensor([2, 2, 6, 0, 0, 6, 6, 0]).cuda()].float()
    assert out.dtype == torch.float32 and torch.equal(bits(out), bits(want))
    assert torch.equal(kernels.feature_bank_rows(bank, torch.tensor([5, 1, 5])), rows[torch.tensor([5, 1, 5]).cuda()].float())


# ---- the two steps on bank rows --------------------------------------------------------------------------------------------------------
def _vqa_step(c, prm, y, step, feats=None, bank=None, idx=None):
    ws = kernels.headtrain_workspace(c.B, c.L, c.C)
    if bank is None:
        score = kernels.headtrain_forward(feats, prm, c.p, c.seed, step, ws)
    else:
        score = kernels.headtrain_bank_forward(bank, idx, prm, c.p, c.seed, step, ws)
    _, dscore = kernels.headtrain_loss(score, y, c.rw)
    if bank is None:
        return score, kernels.headtrain_backward(feats, prm, c.p, c.seed, step, ws, dscore)
    return score, kernels.headtrain_bank_backward(bank, idx, prm, c.p, c.seed, step, ws, dscore)


def _simple_step(c, prm, y, step, feats=None, bank=None, idx=None):
    ws = kernels.simple_headtrain_workspace(c.B, c.L, c.C)
    score = kernels.simple_headtrain_forward(feats, prm, ws) if bank is None else kernels.simple_headtrain_bank_forward(bank, idx, prm, ws)
    _, dscore = kernels.headtrain_loss(score, y, c.rw)
    if bank is None:
        return score, kernels.simple_headtrain_backward(feats, prm, ws, dscore)
    return score, kernels.simple_headtrain_bank_backward(bank, idx, prm, ws, dscore)


def _bank_step_equals_dense(c, step_fn, dtype, steps):
    prm, y = dev(c.prm), dev(c.y)
    bank, idx = random_bank(c, dtype, 100 + c.B)
    dense = kernels.feature_bank_rows(bank, idx)
    assert torch.equal(dense, bank.tensor[idx.long()].float())
    for step in steps:
        s_b, g_b = step_fn(c, prm, y, step, bank=bank, idx=idx)
        s_d, g_d = step_fn(c, prm, y, step, feats=dense)
        assert torch.equal(bits(s_b), bits(s_d)), ("score", step)
        assert torch.equal(bits(g_b), bits(g_d)), ("grads", step)
        assert bool(torch.isfinite(s_b).all()) and bool(torch.isfinite(g_b).all()) and float(g_b.abs().max()) > 0
    # the fp32 bank with the identity index is the dense entry on the fixture input itself
    if dtype == torch.float32:
        x = dev(c.x)
        ident = torch.arange(c.B, dtype=torch.int32, device="cuda")
        s_b, g_b = step_fn(c, prm, y, 0, bank=kernels.FeatureBank.of(x), idx=ident)
        s_d, g_d = step_fn(c, prm, y, 0, feats=x)
        assert torch.equal(bits(s_b), bits(s_d)) and torch.equal(bits(g_b), bits(g_d))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("name", ["a", "d", "e", "b"])
def test_vqa_head_step_on_bank_rows_is_bit_equal_to_the_dense_step(golden, name, dtype):
    _bank_step_equals_dense(vqa_case(golden, name), _vqa_step, dtype, (0, 2))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("name", ["c", "d", "a"])
def test_simple_head_step_on_bank_rows_is_bit_equal_to_the_dense_step(golden, name, dtype):
    _bank_step_equals_dense(simple_case(golden, name), _simple_step, dtype, (0, 2))


@pytest.mark.parametrize("head,name,dtype", [("vqa", "a", torch.bfloat16), ("simple", "d", torch.float16)])
def test_guard_bands_intact_bank_unchanged_outputs_fully_written(golden, head, name, dtype):
    c, step_fn = (vqa_case(golden, name), _vqa_step) if head == "vqa" else (simple_case(golden, name), _simple_step)
    bank0, idx0 = random_bank(c, dtype, 9)
    with guarded("cuda", max_guard=1 << 20) as G:
        rows = G.wrap(bank0.tensor, name="bank")
        idx = G.wrap(idx0, name="index")
        prm, y = G.wrap(dev(c.prm), name="params"), G.wrap(dev(c.y), name="labels")
        before = digest(rows)
        score, grads = step_fn(c, prm, y, 1, bank=kernels.FeatureBank.of(rows), idx=idx)     # workspace, score, dscore, grads: guarded
        report = G.intact()
        assert report, repr(report)
        assert digest(rows) == before and torch.equal(idx, idx0)
        assert not bool(G.payload_left(score).any()) and not bool(G.payload_left(grads).any())
        assert bool(torch.isfinite(score).all()) and bool(torch.isfinite(grads).all())
    s_d, g_d = step_fn(c, dev(c.prm), dev(c.y), 1, feats=kernels.feature_bank_rows(bank0, idx0))
    assert torch.equal(bits(score), bits(s_d)) and torch.equal(bits(grads), bits(g_d))


# ---- the finetuner on the synthetic dataset of the new yml: 4 videos x 2 clips --------------------------------------------------------
@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from kvq_amd.datasets import SyntheticKVQDataset
    from kvq_amd.finetune import HeadFinetuner
    from kvq_amd.trainer import Trainer
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "kwai_swin_grpb_synthetic_bank_finetune.yml")))
    torch.manual_seed(0)
    tr = Trainer(types.SimpleNamespace(gpu_id="0", resume=str(tmp_path_factory.mktemp("ck")), test_set="val"), cfg)
    ds = SyntheticKVQDataset(dict(cfg["data"]["train"]["args"]), None, device=tr.device)
    new = lambda **kw: HeadFinetuner(tr.model, "swin_tiny_grpb", lr=1e-3, wd=0.05, warmup_iters=2, max_iters=12, ema=True, seed=5, **kw)  # noqa: E731
    ft = new()
    assert ft.cache_features(ds, tr, draws=2, dtype=torch.bfloat16) == 4
    return types.SimpleNamespace(tr=tr, ds=ds, new=new, ft=ft, bank=ft.bank.tensor.clone())


def _state(ft):
    return [ft.params, ft.exp_avg, ft.exp_avg_sq, ft.ema]


def _same_state(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(_state(a), _state(b)))


def test_cache_features_fills_a_two_draw_bf16_bank(env):
    ft = env.ft
    assert tuple(ft.bank.tensor.shape) == (16, 16 * 7 * 7, 768) and ft.bank.tensor.dtype == torch.bfloat16
    assert (ft.n, ft.draws, len(ft.feats), len(ft.labels)) == (8, 2, 4, 4)
    assert all(f.shape == (2, 784, 768) and f.data_ptr() == ft.bank.tensor[2 * i].data_ptr() for i, f in enumerate(ft.feats))
    one = env.new()
    assert one.cache_features(env.ds, env.tr) == 4 and one.bank.tensor.dtype == torch.float32 and tuple(one.bank.tensor.shape) == (8, 784, 768)
    assert torch.equal(bits(env.bank[:8]), bits(one.bank.tensor.to(torch.bfloat16)))          # draw 0: today's items, rounded
    assert not torch.equal(env.bank[8:], env.bank[:8])                                       # draw 1: other fragment positions
    assert env.ds.draw == 0                                                                  # the dataset is left on draw 0
    feats, labels = one.clip_samples()
    assert feats.data_ptr() == one.bank.tensor.data_ptr() and feats.is_contiguous() and labels.shape == (8,)   # a view: stored once
    wide, _ = ft.clip_samples()
    assert wide.dtype == torch.float32 and torch.equal(wide, env.bank[:8].float())
    again = env.new()
    again.cache_features(env.ds, env.tr, draws=2, dtype=torch.bfloat16)
    assert torch.equal(bits(again.bank.tensor), bits(env.bank))                              # a second run reproduces the bank
    assert torch.equal(bits(ft.predict(ft.feats[1])), bits(ft.predict(ft.feats[1].float())))  # predict widens 16-bit rows


def test_cache_features_refusals(env):
    ft = env.new()
    with pytest.raises(ValueError, match="fp32, fp16 or bf16"):
        ft.cache_features(env.ds, env.tr, dtype=torch.float64)
    with pytest.raises(ValueError, match="draws"):
        ft.cache_features(env.ds, env.tr, draws=0)
    calls = []
    real = env.tr._model_inputs
    env.tr._model_inputs = lambda item: (calls.append(1), real(item))[1]
    try:
        with pytest.raises(ValueError, match=r"bytes.*draws = 400000.*float32"):      # 400000 x 8 x 2.4 MB: before the second forward
            ft.cache_features(env.ds, env.tr, draws=400000, dtype=torch.float32)
    finally:
        del env.tr._model_inputs
    assert len(calls) == 1 and env.ds.draw == 0
    # an fp16 bank is never silently saturated
    big = env.new()
    orig = big._clip_features
    big._clip_features = lambda feat: orig(feat) * 1e5
    with pytest.raises(ValueError, match="bf16.*fp32"):
        big.cache_features(env.ds, env.tr, dtype=torch.float16)
    assert big.bank is None
    big.cache_features(env.ds, env.tr, dtype=torch.bfloat16)
    assert big.bank is not None


def test_step_indexed_equals_step_on_the_gathered_rows(env):
    a, b = env.new(), env.new()
    a.bank = b.bank = env.ft.bank
    lab = env.ft.sample_labels()
    for idx in ([0, 9, 3, 14, 9], [15, 1, 2, 8], [4, 5, 6, 7, 12, 13]):
        y = lab[torch.tensor(idx).cuda() % 8]
        ra = a.step_indexed(torch.tensor(idx), y)
        rb = b.step(kernels.feature_bank_rows(env.ft.bank, torch.tensor(idx)), y)
        assert ra == rb
    assert a.it == b.it == 3 and _same_state(a, b) and not torch.equal(a.params, env.new().params)
    with pytest.raises(ValueError, match=r"index\[1\] = 16"):
        a.step_indexed(torch.tensor([0, 16, 2]), lab[:3])
    assert a.it == 3


def test_fit_trains_on_draw_0_then_draw_1(env):
    a, b = env.new(), env.new()
    a.cache_features(env.ds, env.tr, draws=2, dtype=torch.bfloat16)
    log = a.fit(2, 4)
    lab, perm = env.ft.sample_labels(), torch.Generator().manual_seed(5)
    want = []
    for draw in (0, 1):
        order = torch.randperm(8, generator=perm)
        for s in (0, 4):
            rows = order[s:s + 4] + 8 * draw
            want.append(b.step(env.bank[rows.cuda()].float(), lab[order[s:s + 4].cuda()]))
    assert log == want and len(log) == 4 and a.epoch == 2 and _same_state(a, b)
    assert a.fit(1, 4) == [b.step(env.bank[o.cuda()].float(), lab[o.cuda()]) for o in torch.randperm(8, generator=perm).split(4)]   # epoch 2: draw 0 again


def test_fit_on_one_fp32_draw_equals_the_index_select_path(env):
    a, b = env.new(), env.new()
    a.cache_features(env.ds, env.tr)
    feats, labels = a.clip_samples()
    log = a.fit(2, 3)                                   # 8 samples: batches of 3, 3 and a dropped 2
    perm, want = torch.Generator().manual_seed(5), []
    for _ in range(2):
        order = torch.randperm(8, generator=perm)
        for s in range(0, 8, 3):
            idx = order[s:s + 3]
            if idx.numel() < 3:
                continue
            idx = idx.cuda()
            want.append(b.step(feats.index_select(0, idx), labels.index_select(0, idx)))
    assert log == want and len(log) == 4 and _same_state(a, b)


# ---- SimpleVQA's train-phase crop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("antialias", [False, True])
def test_simplevqa_train_crop_is_the_full_resize_sliced_at_the_seeded_offsets(antialias):
    from kvq_amd.datasets import fusion_datasets as fd
    g = torch.Generator().manual_seed(2)
    clip = torch.randint(0, 256, (3, 2, 270, 480), generator=g, dtype=torch.uint8).cuda()
    full = kernels.resize_bilinear(clip, 520, 520, mean=fd.SIMPLEVQA_MEAN, std=fd.SIMPLEVQA_STD, antialias=antialias)
    seen = set()
    for seed in (0, 1, 41):
        random.seed(seed)
        oy, ox = random.randrange(520 - 448), random.randrange(520 - 448)
        random.seed(seed)
        view = fd.get_resizecrop_video(clip, 520, 448, "train", mean=fd.SIMPLEVQA_MEAN, std=fd.SIMPLEVQA_STD, antialias=antialias)
        assert view.shape == (3, 2, 448, 448) and torch.equal(view, full[:, :, oy:oy + 448, ox:ox + 448])
        seen.add((oy, ox))
    assert len(seen) == 3
    test = fd.get_resizecrop_video(clip, 520, 448, "test", mean=fd.SIMPLEVQA_MEAN, std=fd.SIMPLEVQA_STD, antialias=antialias)
    assert torch.equal(test, full[:, :, 36:484, 36:484])


# ---- train.py on the two new ymls ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yml,name,key", [("kwai_swin_grpb_synthetic_bank_finetune.yml", "swin_tiny_grpb_synthetic_bank", "swin_tiny_grpb_head.fc_hid.weight"),
                                          ("kwai_simpleVQA_synthetic_bank_finetune.yml", "simpleVQA_synthetic_bank", "simpleVQA_head.quality.0.weight")])
def test_train_cli_runs_the_bank_ymls(tmp_path, yml, name, key):
    env_ = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-o", os.path.join(ROOT, "config", yml), "-r", str(tmp_path / "ck"),
                        "-t1", "val", "--gpu_id", "0"], cwd=tmp_path, env=env_, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.count("train/total_loss") == 2                     # two epochs: draw 0, then draw 1
    for word in ("SRCC", "PLCC", "KRCC", "RMSE", "the best validation accuracy of the model-n"):
        assert word in r.stdout, word
    for suffix in ("n", "s"):
        ck = torch.load(tmp_path / "ck" / f"{name}_head_val_{suffix}_finetuned.pth", map_location="cpu")
        assert set(ck) == {"state_dict", "validation_results"} and "module." + key in ck["state_dict"]
        assert bool(torch.isfinite(ck["state_dict"]["module." + key]).all())
