"""GPU: the ConvNeXt-V2 3D trunk (model key ``conv_v2_tiny``) — the GRN launches against the float64 restatement
(tests/convnextv2_ref.py) on the same 16-bit inputs, one BlockV23D against the restatement with operand rounding, the whole network
against the reference's stored outputs (tests/golden/convnextv2.npz), the (T, H, W) option, and the test.py drop-in."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import kvq_amd  # noqa: F401
from kvq_amd import _abi, kernels
from kvq_amd.utils import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnextv2_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}     # half-ulp relative rounding error
HALVES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
NS = [384, 768, 1536, 3072]
BIG = (1, 30, 30, 2)          # 900 rows per column at |x| ~ 250: the squares sum to 5.6e7


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ------------------------------------------------------------------------------------------- kvq_grn_stats / kvq_grn_apply
def _shapes(N):
    return [(2, 3, 5, 7), (1, 1, 1, 1)] + ([(2, 2, 9, 11)] if N == 3072 else []) + [BIG]


@functools.lru_cache(maxsize=None)
def _grn_case(N, shape, half):
    """16-bit input rows (as the tensor the launch reads), gamma, beta, and per axes the float64 (y, per-element bound / (EPS + 1e-4));
    computed once, shared by every test and left unchanged"""
    g = rng(N + 7 * sum(shape) + (half == torch.float16))
    x = g.standard_normal(shape + (N,))
    if shape == BIG:
        x = 250.0 * np.sign(x) * (1.0 + 0.05 * g.standard_normal(x.shape))
    x16 = torch.from_numpy(x.astype(np.float32)).to(half)
    gamma = torch.from_numpy((g.uniform(0.5, 1.5, N) * g.choice([-1.0, 1.0], N)).astype(np.float32))
    beta = torch.from_numpy((0.3 * g.standard_normal(N)).astype(np.float32))
    ref = {}
    xd, gd, bd = x16.double(), gamma.double(), beta.double()
    for axes in ("th", "thw"):
        nx, term = R.grn_parts(xd, gd, bd, axes)
        ref[axes] = (term + xd, xd.abs() * (1 + gd.abs() * nx) + bd.abs())
    return x16, gamma, beta, ref


def _grn_run(x16, gamma, beta, over, out=None):
    hid = x16.to(DEV).reshape(-1, x16.shape[-1])          # a fresh device copy: the launch works in place
    y = kernels.grn(hid, x16.shape[:4], gamma.to(DEV), beta.to(DEV), over=over, out=out)
    return y, hid


@pytest.mark.parametrize("over", ["th", "thw"])
@pytest.mark.parametrize("half", HALVES, ids=IDS)
@pytest.mark.parametrize("N", NS)
def test_grn_against_float64(N, half, over):
    for shape in _shapes(N):
        x16, gamma, beta, ref = _grn_case(N, shape, half)
        want, mag = ref[over]
        y, _ = _grn_run(x16, gamma, beta, over)
        err = (y.float().cpu().double().reshape(want.shape) - want).abs()
        worst = float((err / mag.clamp_min(1e-30)).max())
        print(f"N={N} {shape} over={over}: max |dy| / (|x| (1 + |gamma| Nx) + |beta|) = {worst:.3e} (bound {EPS[half] + 1e-4:.3e})")
        assert torch.isfinite(y.float()).all()
        assert bool((err <= (EPS[half] + 1e-4) * mag).all())
        if shape == (1, 1, 1, 1) and over == "th":         # one token: Gx = |x|
            nx = x16.double().abs().reshape(-1)
            nx = nx / (nx.mean() + 1e-6)
            assert bool(((want.reshape(-1) - (x16.double().reshape(-1) * (1 + gamma.double() * nx) + beta.double())).abs() <= 1e-12).all())


@pytest.mark.parametrize("over", ["th", "thw"])
@pytest.mark.parametrize("half", HALVES, ids=IDS)
def test_grn_statistics_do_not_mix_across_the_batch(half, over):
    for N, shape in ((384, (2, 3, 5, 7)), (3072, (2, 2, 9, 11))):
        x16, gamma, beta, _ = _grn_case(N, shape, half)
        both, _ = _grn_run(x16, gamma, beta, over)
        n = both.shape[0] // 2
        for b in range(2):
            alone, _ = _grn_run(x16[b:b + 1].contiguous(), gamma, beta, over)
            assert torch.equal(both[b * n:(b + 1) * n], alone)
        assert not torch.equal(both[:n], both[n:])


@pytest.mark.parametrize("half", HALVES, ids=IDS)
def test_grn_zero_sample_and_zero_column(half):
    N, shape = 768, (2, 3, 5, 7)
    x16, gamma, beta, _ = _grn_case(N, shape, half)
    x = x16.clone()
    x[1] = 0                      # an all-zero sample: Gx = 0 everywhere, Nx = 0 / 1e-6 = 0
    x[0, :, :, 2, 5] = 0          # an all-zero column (b = 0, w = 2, n = 5) of a live sample
    x[0, :, :, :, 9] = 0          # an all-zero channel
    b16 = beta.to(half)
    for over in ("th", "thw"):
        y, _ = _grn_run(x, gamma, beta, over)
        y = y.cpu().reshape(shape + (N,))
        assert torch.isfinite(y.float()).all()
        assert torch.equal(y[1], b16.expand(y[1].shape))
        assert torch.equal(y[0, :, :, 2, 5], b16[5].expand(3, 5)) and torch.equal(y[0, :, :, :, 9], b16[9].expand(3, 5, 7))


@pytest.mark.parametrize("half", HALVES, ids=IDS)
def test_grn_in_place_out_of_place_and_repeatable(half):
    for N, shape in ((384, (2, 3, 5, 7)), (3072, (2, 2, 9, 11)), (1536, BIG)):
        x16, gamma, beta, _ = _grn_case(N, shape, half)
        for over in ("th", "thw"):
            y1, hid1 = _grn_run(x16, gamma, beta, over)
            assert y1.data_ptr() == hid1.data_ptr()                              # in place by default
            out = torch.zeros_like(hid1)
            y2, hid2 = _grn_run(x16, gamma, beta, over, out=out)
            assert y2.data_ptr() == out.data_ptr() and torch.equal(hid2.cpu(), x16.reshape(-1, N))      # the input is left alone
            assert torch.equal(y1, y2)
            y3, _ = _grn_run(x16, gamma, beta, over)
            assert torch.equal(y1, y3)                                           # every sum has one order: two runs are bit-equal


def test_grn_unsupported_shapes_do_not_launch():
    lib = _abi.lib()
    N = 512
    x = torch.full((2 * 3 * 3, N), 7.0, dtype=torch.float16, device=DEV)
    out = torch.full((2 * 3 * 3, N), 5.0, dtype=torch.float16, device=DEV)
    vec = torch.ones(4096, device=DEV)
    ws = torch.zeros(1 << 16, device=DEV)
    a = _abi.KvqGrnArgs()
    a.x, a.y, a.gamma, a.beta, a.ws = (_abi.ptr(t) for t in (x, out, vec, vec, ws))
    a.B, a.D, a.H, a.W, a.dtype = 2, 1, 3, 3, 1
    for n in (512, 96, 400):
        a.N = n
        assert lib.kvq_grn_stats(C.byref(a), _abi.current_stream()) == -3            # KVQ_ERR_UNSUPPORTED
        assert lib.kvq_grn_apply(C.byref(a), _abi.current_stream()) == -3
    a.N, a.ws = 384, None
    assert lib.kvq_grn_apply(C.byref(a), _abi.current_stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((x == 7.0).all()) and not ws.any()
    with pytest.raises(_abi.KvqError, match="unsupported shape"):
        kernels.grn(x, (2, 1, 3, 3), vec[:N], vec[:N])
    with pytest.raises(ValueError, match="over"):
        kernels.grn(x, (2, 1, 3, 3), vec[:N], vec[:N], over="hw")
    assert bool((x == 7.0).all())


# ------------------------------------------------------------------------------------------- one block
def _block_params(g, Cc, kt):
    t = lambda *s, sc=1.0: torch.from_numpy((g.standard_normal(s) * sc).astype(np.float32))  # noqa: E731
    return {"dwconv.weight": t(Cc, 1, kt, 7, 7, sc=1.0 / np.sqrt(49 * kt)), "dwconv.bias": t(Cc, sc=0.3),
            "norm.weight": 1 + 0.2 * t(Cc), "norm.bias": 0.2 * t(Cc),
            "pwconv1.weight": t(4 * Cc, Cc, sc=0.15), "pwconv1.bias": t(4 * Cc, sc=0.3),
            "grn.gamma": torch.from_numpy((g.uniform(0.5, 1.5, (1, 1, 1, 4 * Cc)) * g.choice([-1.0, 1.0], (1, 1, 1, 4 * Cc))).astype(np.float32)),
            "grn.beta": t(1, 1, 1, 4 * Cc, sc=0.2),
            "pwconv2.weight": t(Cc, 4 * Cc, sc=0.04), "pwconv2.bias": t(Cc, sc=0.3)}


@pytest.mark.parametrize("over", ["th", "thw"])
@pytest.mark.parametrize("half", HALVES, ids=IDS)
@pytest.mark.parametrize("kt", [1, 3])
def test_one_block(kt, half, over):
    Cc, dims = 96, (2, 3, 9, 11)
    g = rng(177 + kt)
    p = _block_params(g, Cc, kt)
    x = torch.from_numpy((2.0 * g.standard_normal(dims + (Cc,))).astype(np.float32))
    with torch.no_grad():
        ref = R.block(x.double(), {k: v.double() for k, v in p.items()}, emul=half, axes=over)
    d = {k: v.to(DEV) for k, v in p.items()}
    cur = x.to(DEV).reshape(-1, Cc).clone()
    rows = kernels.dwconv3d_ln(cur.view(dims + (Cc,)), kernels.dwconv_weight_taps(d["dwconv.weight"]), d["dwconv.bias"], d["norm.weight"],
                               d["norm.bias"], eps=1e-6, out_dtype=half)
    hid = kernels.gemm(rows, d["pwconv1.weight"].to(half), d["pwconv1.bias"], _abi.EPI_GELU_BF16)
    kernels.grn(hid, dims, d["grn.gamma"].reshape(-1), d["grn.beta"].reshape(-1), over=over)
    kernels.gemm(hid, d["pwconv2.weight"].to(half), d["pwconv2.bias"], _abi.EPI_RESID_F32, out=cur)
    scale = ref.abs().max().item()
    err = (cur.cpu().double() - ref.reshape(-1, Cc)).abs().max().item()
    print(f"block kt={kt} over={over}: err {err:.3e} (gate {6 * EPS[half] * scale + 1e-4:.3e})")
    assert err <= 6 * EPS[half] * scale + 1e-4


# ------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _net(wseed, dtype, over="th"):
    from kvq_amd.models.model import VQA_Network
    net = VQA_Network({"model": {"args": {"conv_v2_tiny": {"backbone": {"operand_dtype": dtype, "grn_over": over},
                                                           "head": {"in_channels": 768, "hidden_channels": 64}}}}})
    r = net.conv_v2_tiny_backbone.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_convnextv2_weights(wseed, "stress").items()},
                                                  strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    net.conv_v2_tiny_head.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_vqa_head_weights(768, 64, wseed, "stress").items()})
    return net.to(DEV).eval()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_end_to_end_against_the_reference(golden, name, dtype):
    g = golden("convnextv2.npz")
    wseed, cseed, B, T, H, W = (int(v) for v in g[f"{name}/meta"])
    net = _net(wseed, dtype)
    x = torch.from_numpy(synth.synth_clip(cseed, T, H, W, batch=B)).to(DEV)
    with torch.no_grad():
        feat = net.conv_v2_tiny_backbone({"aesthetic": x})
        multi = net.conv_v2_tiny_backbone({"aesthetic": x}, multi=True)
        score = net(inputs={"aesthetic": x}, reduce_scores=True)
        (score_m, maps) = net(inputs={"aesthetic": x}, reduce_scores=True, return_maps=True)
    e, em = R.rel_l2(feat.cpu(), g[f"{name}/feat"]), R.rel_l2(multi.cpu(), g[f"{name}/multi"])
    ds = np.abs(score.cpu().numpy().reshape(-1) - g[f"{name}/score"]).max()
    ge, gem = float(g[f"{name}/err_emul_{dtype}"]), float(g[f"{name}/err_emul_{dtype}_multi"])
    print(f"case {name} {dtype}: rel-L2 feat {e:.3e} (emulation {ge:.3e}), multi {em:.3e} (emulation {gem:.3e}), |dscore| {ds:.3e} "
          f"(emulation {float(g[f'{name}/err_emul_{dtype}_score']):.3e})")
    assert tuple(feat.shape) == g[f"{name}/feat"].shape and tuple(multi.shape) == g[f"{name}/multi"].shape and multi.shape[1] == 672
    assert e <= 3 * ge
    assert em <= 3 * gem
    if dtype == "fp16":
        assert ds <= 1e-3                     # bf16: format-limited, reported above
    tok = maps["conv_v2_tiny"]["token_map"]
    assert tuple(tok.shape) == (B, T // 2, H // 32, W // 32) and tuple(maps["conv_v2_tiny"]["timeline"].shape) == (B, T // 2)
    assert torch.equal(score_m, score)
    assert (tok.mean((1, 2, 3)) - score.reshape(-1)).abs().max().item() <= 1e-5


def test_end_to_end_grn_over_thw(golden):
    """``grn_over="thw"`` against the float64 restatement with those axes, within 3 x the restatement's own fp16 emulation error
    (computed here), and away from the default's feat by more than that bound."""
    g = golden("convnextv2.npz")
    wseed, cseed, B, T, H, W = (int(v) for v in g["A/meta"])
    wts = synth.synth_convnextv2_weights(wseed, "stress")
    x = torch.from_numpy(synth.synth_clip(cseed, T, H, W, batch=B))
    with torch.no_grad():
        want = R.forward(wts, x, axes="thw")
        emul = R.rel_l2(R.forward(wts, x, axes="thw", emul=torch.float16), want)
        feat = _net(wseed, "fp16", "thw").conv_v2_tiny_backbone({"aesthetic": x.to(DEV)}).cpu()
        dflt = _net(wseed, "fp16").conv_v2_tiny_backbone({"aesthetic": x.to(DEV)}).cpu()
    e, gap = R.rel_l2(feat, want), R.rel_l2(dflt, want)
    print(f"grn_over=thw: rel-L2 feat {e:.3e} (emulation {emul:.3e}); the default is {gap:.3e} away")
    assert abs(R.rel_l2(want, g["A/feat"]) - float(g["A/err_thw"])) <= 1e-6       # the restatement the fixture measured
    assert e <= 3 * emul
    assert gap > 3 * emul


def test_refuses_clips_the_stem_cannot_tile():
    net = _net(34, "fp16")
    with pytest.raises(_abi.KvqError, match="stem"):
        net.conv_v2_tiny_backbone({"aesthetic": torch.zeros(1, 3, 8, 66, 64, device=DEV)})


# ------------------------------------------------------------------------------------------- harness
def test_cli_conv_v2_tiny_synthetic(tmp_path):
    """``python test.py -o config/kwai_conv_v2_tiny_synthetic_test.yml`` on two small synthetic videos: finite, distinct scores, equal to
    calling the model on the dataset's items directly (the aesthetic view draws nothing at random for 64 frames at interval 2)."""
    from kvq_amd.datasets.fusion_datasets import SyntheticKVQDataset
    from kvq_amd.models import VQA_Network
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "kwai_conv_v2_tiny_synthetic_test.yml")))
    a = cfg["data"]["val"]["args"]
    assert a["sample_types"]["aesthetic"] == dict(size_h=224, size_w=224, clip_len=32, frame_interval=2, num_clips=1)
    assert cfg["model"]["args"]["conv_v2_tiny"]["backbone"] == {"pretrained": False, "grn_over": "th"}
    a.update(num_videos=2, frames=64, height=120, width=160)
    net = VQA_Network(cfg)
    net.conv_v2_tiny_backbone.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_convnextv2_weights(3, "stress").items()})
    net.conv_v2_tiny_head.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_vqa_head_weights(768, 64, 3, "stress").items()})
    ckpt = tmp_path / "conv_v2_tiny.pth"
    torch.save({"state_dict": net.state_dict()}, str(ckpt))
    cfg["load_path"] = str(ckpt)
    yml = tmp_path / "t.yml"
    yml.write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), "-o", str(yml), "--gpu_id", "0"], cwd=tmp_path,
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = (tmp_path / "output.txt").read_text().strip().splitlines()
    assert len(lines) == 2 and all(len(l.split(",")) == 2 for l in lines)
    got = np.asarray([float(l.split(",")[1]) for l in lines])
    assert np.isfinite(got).all() and got[0] != got[1]
    ds = SyntheticKVQDataset(a, None, device=DEV)
    net = net.to(DEV).eval()
    want = []
    for i in range(2):
        item = ds[i]
        assert set(item) == {"aesthetic", "num_clips", "frame_inds", "label", "name", "video_name"}
        assert tuple(item["aesthetic"].shape) == (3, 32, 224, 224)
        with torch.no_grad():
            want.append(float(net(inputs={"aesthetic": item["aesthetic"].unsqueeze(0)}, reduce_scores=True).mean()))
    assert np.abs(got - np.asarray(want)).max() <= 1e-6
