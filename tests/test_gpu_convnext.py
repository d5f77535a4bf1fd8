"""GPU: the ConvNeXt-3D trunk (model key ``conv_tiny``) — the depthwise-conv + LayerNorm launch and the scaled-residual GEMM against
the float64 restatement (tests/convnext_ref.py), one block and one downsample layer against the restatement with operand rounding,
the whole network against the reference's stored outputs (tests/golden/convnext.npz), and the test.py drop-in."""
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
import convnext_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}     # half-ulp relative rounding error
HALVES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def rnd(t, half):
    return t.to(half).to(torch.float32)


# ------------------------------------------------------------------------------------------- kvq_dwconv3d_ln
@functools.lru_cache(maxsize=None)
def _dw_case(Cc, kt, shape):
    """inputs (fp32) and the float64 reference rows of one (C, kt, (B, T, H, W)) case; computed once, shared by every test"""
    B, T, H, W = shape
    g = rng(1000 * Cc + 10 * kt + sum(shape))
    t = lambda *s, sc=1.0: torch.from_numpy((g.standard_normal(s) * sc).astype(np.float32))  # noqa: E731
    x = t(B, T, H, W, Cc, sc=2.0)
    w = t(Cc, 1, kt, 7, 7, sc=1.0 / np.sqrt(49 * kt))
    b, lw, lb = t(Cc, sc=0.3), 1 + 0.2 * t(Cc), 0.2 * t(Cc)
    with torch.no_grad():
        ref = R.dwconv_ln(x.double(), w.double(), b.double(), lw.double(), lb.double())
    return x, w, b, lw, lb, ref


def _dw_run(x, w, b, lw, lb, out_dtype):
    return kernels.dwconv3d_ln(x.to(DEV), kernels.dwconv_weight_taps(w.to(DEV)), b.to(DEV), lw.to(DEV), lb.to(DEV), eps=1e-6,
                               out_dtype=out_dtype)


DW_SHAPES = [(2, 3, 9, 11), (1, 2, 7, 7), (2, 1, 2, 3)]      # odd sizes no tile divides; plane == window; padding only and T < kt


@pytest.mark.parametrize("half", HALVES, ids=IDS)
@pytest.mark.parametrize("kt", [1, 3])
@pytest.mark.parametrize("Cc", [96, 192, 384, 768])
def test_dwconv3d_ln(Cc, kt, half):
    for shape in DW_SHAPES:
        if shape == (2, 1, 2, 3) and kt != 3:
            continue
        x, w, b, lw, lb, ref = _dw_case(Cc, kt, shape)
        scale = ref.abs().max().item()
        out32 = _dw_run(x, w, b, lw, lb, torch.float32)
        e32 = (out32.cpu().double() - ref).abs().max().item()
        out16 = _dw_run(x, w, b, lw, lb, half)
        e16 = (out16.float().cpu().double() - ref).abs().max().item()
        print(f"C={Cc} kt={kt} {shape}: fp32 err {e32:.3e} (gate {2e-5 * max(1.0, scale):.3e}), 16-bit err {e16:.3e} "
              f"(gate {2 * EPS[half] * scale + 1e-5:.3e})")
        assert out32.shape == (int(np.prod(shape)), Cc)
        assert e32 <= 2e-5 * max(1.0, scale)
        assert e16 <= 2 * EPS[half] * scale + 1e-5
        # taps are accumulated in one fixed order: a second launch is bit-equal
        assert torch.equal(out32, _dw_run(x, w, b, lw, lb, torch.float32))
        assert torch.equal(out16, _dw_run(x, w, b, lw, lb, half))


@pytest.mark.parametrize("Cc,kt", [(96, 3), (768, 3), (192, 1)])
def test_dwconv3d_ln_no_halo_across_batch_elements(Cc, kt):
    x, w, b, lw, lb, _ = _dw_case(Cc, kt, (2, 3, 9, 11))
    x2 = x.clone()
    x2[1] *= 1e3
    both = _dw_run(x2, w, b, lw, lb, torch.float32)
    alone = _dw_run(x[:1].contiguous(), w, b, lw, lb, torch.float32)
    n = alone.shape[0]
    assert torch.equal(both[:n], alone)
    assert not torch.equal(both[n:], _dw_run(x, w, b, lw, lb, torch.float32)[n:])      # element 1 really changed


def test_dwconv3d_ln_unsupported_shapes_do_not_launch():
    lib = _abi.lib()
    x = torch.zeros(1, 2, 4, 4, 128, device=DEV)
    vec = torch.ones(147 * 128, device=DEV)
    out = torch.full((32, 128), 7.0, device=DEV)
    a = _abi.KvqDwconvLnArgs()
    a.x, a.w, a.bias, a.ln_w, a.ln_b, a.out_f32 = (_abi.ptr(t) for t in (x, vec, vec, vec, vec, out))
    a.B, a.T, a.H, a.W, a.eps = 1, 2, 4, 4, 1e-6
    for Cc, kt in ((128, 3), (100, 1), (96, 5), (96, 2)):
        a.C, a.kt = Cc, kt
        assert lib.kvq_dwconv3d_ln(C.byref(a), _abi.current_stream()) == -3          # KVQ_ERR_UNSUPPORTED
    a.C, a.kt = 96, 3
    a.out_h = _abi.ptr(out)                                                          # both outputs set
    assert lib.kvq_dwconv3d_ln(C.byref(a), _abi.current_stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(_abi.KvqError, match="unsupported shape"):
        kernels.dwconv3d_ln(x, vec.view(147, 128), vec[:128], vec[:128], vec[:128])


# ------------------------------------------------------------------------------------------- kvq_gemm_resid_scaled
@pytest.fixture(params=[-1, 1], ids=["by-shape", "wide8p"])
def tile_mode(request):
    prev = kernels.gemm_tile_mode(request.param)
    yield request.param
    kernels.gemm_tile_mode(prev)


@pytest.mark.parametrize("half", HALVES, ids=IDS)
@pytest.mark.parametrize("M,N,K", [(300, 96, 384), (77, 768, 3072)])
def test_gemm_resid_scaled(M, N, K, half, tile_mode):
    g = rng(M + N + K)
    A = rnd(torch.from_numpy(g.standard_normal((M, K)).astype(np.float32)), half)
    W = rnd(torch.from_numpy((g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)), half)
    b = torch.from_numpy(g.standard_normal(N).astype(np.float32))
    x = torch.from_numpy(g.standard_normal((M, N)).astype(np.float32))
    s = torch.from_numpy(g.uniform(0.5, 1.5, N).astype(np.float32))
    ref = A.double() @ W.double().t() + b.double()
    Ad, Wd, bd = A.to(DEV, half), W.to(DEV, half), b.to(DEV)
    if (M, N, K) == (77, 768, 3072):
        assert _abi.lib().kvq_gemm_splitk_factor(M, N, K) > 1           # this shape goes through split-K and its reduce launch
    out = x.clone().to(DEV)
    kernels.gemm(Ad, Wd, bd, _abi.EPI_RESID_F32, out=out, col_scale=s.to(DEV))
    err = (out.cpu().double() - (x.double() + s.double() * ref)).abs().max().item()
    print(f"({M},{N},{K}) scaled residual: err {err:.3e} (gate {2e-5 * np.sqrt(K):.3e})")
    assert err <= 2e-5 * np.sqrt(K)
    # scale = 1 is the plain residual epilogue to the bit
    one, plain = x.clone().to(DEV), x.clone().to(DEV)
    kernels.gemm(Ad, Wd, bd, _abi.EPI_RESID_F32, out=one, col_scale=torch.ones(N, device=DEV))
    kernels.gemm(Ad, Wd, bd, _abi.EPI_RESID_F32, out=plain)
    assert torch.equal(one, plain)
    # scale = 1e-6 (the reference's initial layer scale) on a small stream: the update is there and right.  A weight folded as
    # 1e-6 * N(0, 1/K) would have rounded to zero in fp16.  Gate: the product's error bound scaled by 1e-6, plus one fp32
    # rounding (2^-23 relative) of the sum.
    xs = (x * 1e-3).contiguous()
    tiny = xs.clone().to(DEV)
    kernels.gemm(Ad, Wd, bd, _abi.EPI_RESID_F32, out=tiny, col_scale=torch.full((N,), 1e-6, device=DEV))
    want = xs.double() + 1e-6 * ref
    assert not torch.equal(tiny.cpu(), xs)
    assert (tiny.cpu().double() - want).abs().max().item() <= 1e-6 * 2e-5 * np.sqrt(K) + 2.0 ** -23 * want.abs().max().item()
    moved = (tiny.cpu().double() - xs.double())
    assert R.rel_l2(moved, 1e-6 * ref) <= 1e-3


def test_gemm_resid_scaled_argument_checks():
    lib = _abi.lib()
    A = torch.zeros(64, 64, dtype=torch.float16, device=DEV)
    out = torch.zeros(64, 64, device=DEV)
    with pytest.raises(ValueError, match="residual epilogue"):
        kernels.gemm(A, A, None, _abi.EPI_STORE_F32, col_scale=torch.ones(64, device=DEV))
    a = _abi.KvqGemmArgs()
    a.A, a.W, a.M, a.N, a.K, a.epilogue, a.out_f32, a.dtype = _abi.ptr(A), _abi.ptr(A), 64, 64, 64, _abi.EPI_RESID_SCALE_F32, _abi.ptr(out), 1
    assert lib.kvq_gemm_bf16(C.byref(a), _abi.current_stream()) == -1       # the scale only travels through kvq_gemm_resid_scaled
    a.epilogue = _abi.EPI_STORE_F32
    assert lib.kvq_gemm_resid_scaled(C.byref(a), _abi.ptr(out), _abi.current_stream()) == -3


# ------------------------------------------------------------------------------------------- one block, one downsample layer
def _block_params(g, Cc, kt):
    t = lambda *s, sc=1.0: torch.from_numpy((g.standard_normal(s) * sc).astype(np.float32))  # noqa: E731
    return {"dwconv.weight": t(Cc, 1, kt, 7, 7, sc=1.0 / np.sqrt(49 * kt)), "dwconv.bias": t(Cc, sc=0.3),
            "norm.weight": 1 + 0.2 * t(Cc), "norm.bias": 0.2 * t(Cc),
            "pwconv1.weight": t(4 * Cc, Cc, sc=0.15), "pwconv1.bias": t(4 * Cc, sc=0.3),
            "pwconv2.weight": t(Cc, 4 * Cc, sc=0.08), "pwconv2.bias": t(Cc, sc=0.3),
            "gamma": torch.from_numpy(g.uniform(0.5, 1.5, Cc).astype(np.float32))}


@pytest.mark.parametrize("half", HALVES, ids=IDS)
@pytest.mark.parametrize("kt", [1, 3])
def test_one_block(kt, half):
    Cc, dims = 96, (1, 2, 16, 16)
    g = rng(77 + kt)
    p = _block_params(g, Cc, kt)
    x = torch.from_numpy((2.0 * g.standard_normal(dims + (Cc,))).astype(np.float32))
    with torch.no_grad():
        ref = R.block(x.double(), {k: v.double() for k, v in p.items()}, emul=half)
    d = {k: v.to(DEV) for k, v in p.items()}
    cur = x.to(DEV).reshape(-1, Cc).clone()
    rows = kernels.dwconv3d_ln(cur.view(dims + (Cc,)), kernels.dwconv_weight_taps(d["dwconv.weight"]), d["dwconv.bias"], d["norm.weight"],
                               d["norm.bias"], eps=1e-6, out_dtype=half)
    hid = kernels.gemm(rows, d["pwconv1.weight"].to(half), d["pwconv1.bias"], _abi.EPI_GELU_BF16)
    kernels.gemm(hid, d["pwconv2.weight"].to(half), d["pwconv2.bias"], _abi.EPI_RESID_F32, out=cur, col_scale=d["gamma"])
    scale = ref.abs().max().item()
    err = (cur.cpu().double() - ref.reshape(-1, Cc)).abs().max().item()
    print(f"block kt={kt}: err {err:.3e} (gate {6 * EPS[half] * scale + 1e-4:.3e})")
    assert err <= 6 * EPS[half] * scale + 1e-4


@pytest.mark.parametrize("half", HALVES, ids=IDS)
def test_one_downsample_layer(half):
    Cc, dims = 96, (1, 2, 16, 16)
    g = rng(91)
    t = lambda *s, sc=1.0: torch.from_numpy((g.standard_normal(s) * sc).astype(np.float32))  # noqa: E731
    x = t(*dims, Cc, sc=2.0)
    lw, lb, w, b = 1 + 0.2 * t(Cc), 0.2 * t(Cc), t(2 * Cc, Cc, 1, 2, 2, sc=1.0 / np.sqrt(4 * Cc)), t(2 * Cc, sc=0.3)
    with torch.no_grad():
        ref = R.downsample(x.double(), lw.double(), lb.double(), w.double(), b.double(), emul=half)
    rows = kernels.layernorm_rows(x.to(DEV).reshape(-1, Cc), lw.to(DEV), lb.to(DEV), out_dtype=half, eps=1e-6)
    w2 = w.permute(0, 2, 3, 4, 1).reshape(2 * Cc, -1).contiguous().to(DEV, half)
    out = kernels.conv_implicit(rows.view(dims + (Cc,)), w2, b.to(DEV), (1, 2, 2), (1, 2, 2), (0, 0, 0), relu=False, store_f32=True)
    scale = ref.abs().max().item()
    err = (out.cpu().double() - ref.reshape(-1, 2 * Cc)).abs().max().item()
    print(f"downsample: err {err:.3e} (gate {6 * EPS[half] * scale + 1e-4:.3e})")
    assert out.shape == (1 * 2 * 8 * 8, 2 * Cc)
    assert err <= 6 * EPS[half] * scale + 1e-4


# ------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _net(wseed, dtype):
    from kvq_amd.models.model import VQA_Network
    net = VQA_Network({"model": {"args": {"conv_tiny": {"backbone": {"pretrained": False, "operand_dtype": dtype},
                                                        "head": {"in_channels": 768, "hidden_channels": 64}}}}})
    net.conv_tiny_backbone.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_convnext_weights(wseed, "stress").items()})
    net.conv_tiny_head.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_vqa_head_weights(768, 64, wseed, "stress").items()})
    return net.to(DEV).eval()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_end_to_end_against_the_reference(golden, name, dtype):
    g = golden("convnext.npz")
    wseed, cseed, B, T, H, W = (int(v) for v in g[f"{name}/meta"])
    net = _net(wseed, dtype)
    x = torch.from_numpy(synth.synth_clip(cseed, T, H, W, batch=B)).to(DEV)
    with torch.no_grad():
        feat = net.conv_tiny_backbone({"aesthetic": x})
        assert torch.equal(feat, net.conv_tiny_backbone({"asesthetic": x}))          # the reference's spelling of the key
        multi = net.conv_tiny_backbone({"aesthetic": x}, multi=True)
        score = net(inputs={"aesthetic": x}, reduce_scores=True)
        (score_m, maps) = net(inputs={"aesthetic": x}, reduce_scores=True, return_maps=True)
    e, em = R.rel_l2(feat.cpu(), g[f"{name}/feat"]), R.rel_l2(multi.cpu(), g[f"{name}/multi"])
    ds = np.abs(score.cpu().numpy().reshape(-1) - g[f"{name}/score"]).max()
    ge, gem = float(g[f"{name}/err_emul_{dtype}"]), float(g[f"{name}/err_emul_{dtype}_multi"])
    print(f"case {name} {dtype}: rel-L2 feat {e:.3e} (emulation {ge:.3e}), multi {em:.3e} (emulation {gem:.3e}), |dscore| {ds:.3e}")
    assert tuple(feat.shape) == g[f"{name}/feat"].shape and tuple(multi.shape) == g[f"{name}/multi"].shape and multi.shape[1] == 672
    assert e <= 3 * ge
    assert em <= 3 * gem
    if dtype == "fp16":
        assert ds <= 1e-3                     # bf16: format-limited, reported above
    tok = maps["conv_tiny"]["token_map"]
    assert tuple(tok.shape) == (B, T // 2, H // 32, W // 32) and tuple(maps["conv_tiny"]["timeline"].shape) == (B, T // 2)
    assert torch.equal(score_m, score)
    assert (tok.mean((1, 2, 3)) - score.reshape(-1)).abs().max().item() <= 1e-5


def test_refuses_clips_the_stem_cannot_tile():
    net = _net(11, "fp16")
    with pytest.raises(_abi.KvqError, match="stem"):
        net.conv_tiny_backbone({"aesthetic": torch.zeros(1, 3, 8, 66, 64, device=DEV)})


# ------------------------------------------------------------------------------------------- harness
def test_cli_conv_tiny_synthetic(tmp_path):
    """``python test.py -o config/kwai_conv_tiny_synthetic_test.yml`` on two small synthetic videos: finite scores, equal to calling the
    model on the dataset's items directly (the aesthetic view draws nothing at random for 64 frames at interval 2)."""
    from kvq_amd.datasets.fusion_datasets import SyntheticKVQDataset
    from kvq_amd.models import VQA_Network
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "kwai_conv_tiny_synthetic_test.yml")))
    a = cfg["data"]["val"]["args"]
    assert a["sample_types"]["aesthetic"] == dict(size_h=224, size_w=224, clip_len=32, frame_interval=2, num_clips=1)
    assert cfg["model"]["args"]["conv_tiny"]["backbone"] == {"pretrained": False}
    a.update(num_videos=2, frames=64, height=120, width=160)
    net = VQA_Network(cfg)
    net.conv_tiny_backbone.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_convnext_weights(3, "stress").items()})
    net.conv_tiny_head.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_vqa_head_weights(768, 64, 3, "stress").items()})
    ckpt = tmp_path / "conv_tiny.pth"
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
