"""GPU: KSVQE's CLIP_tool on the HIP kernels (models/backbones/clip_visual.py) against the oracle and the reference's
stored outputs; the small ViT kernels one by one against torch."""
import numpy as np
import pytest
import torch

import kvq_amd  # noqa: F401
from kvq_amd import _abi, kernels
from kvq_amd.models.backbones.clip_visual import CLIP_extractor_addadapter_cls
from kvq_amd.utils import synth
from oracle import clip_oracle as CO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HALF = {"fp16": torch.float16, "bf16": torch.bfloat16}
EPS = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}


def _model(dtype):
    m = CLIP_extractor_addadapter_cls(CLIP_location=8, cls_use=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_clip_visual_weights(7).items()}, strict=True)
    m.operand_dtype = _abi.dtype_code(dtype)
    return m.to(DEV).eval()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("case", ["clip_112", "clip_224", "clip_96x128"])
def test_clip_tool_vs_reference_golden(golden, case, dtype):
    g = golden("clip.npz")
    B, H, W, seed = (int(v) for v in g[f"{case}/meta"])
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal((B, 3, H, W)).astype(np.float32))
    with torch.no_grad():
        outs = _model(dtype)(x.to(DEV))
    tol = {"fp16": 6e-3, "bf16": 4e-2}[dtype]                     # relative L2: 12 blocks of 16-bit-operand GEMMs
    for name, o in zip(("cls_attn", "cls_token", "pat_token"), outs):
        a = np.ascontiguousarray(o.float().cpu().numpy())
        assert tuple(g[f"{case}/{name}/shape"]) == a.shape, name
        got, ref = a.reshape(-1)[g[f"{case}/{name}/idx"]], g[f"{case}/{name}/val"]
        rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
        assert rel <= tol, (name, rel)
    # the cosine map is what the region selection ranks: absolute error
    a = outs[0].float().cpu().numpy().reshape(-1)[g[f"{case}/cls_attn/idx"]]
    assert np.abs(a - g[f"{case}/cls_attn/val"]).max() <= {"fp16": 4e-3, "bf16": 3e-2}[dtype]


def test_clip_tool_vs_oracle_no_adapter_and_errors():
    m = CLIP_extractor_addadapter_cls(CLIP_location=10, cls_use=False, layers=2, heads=12)
    wts = synth.synth_clip_visual_weights(9, layers=2, cls_use=False)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in wts.items()}, strict=True)
    m = m.to(DEV).eval()
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(1)).standard_normal((2, 3, 64, 80)).astype(np.float32))
    with torch.no_grad():
        got = m(x.to(DEV))
        ref = CO.clip_visual_extractor(x, wts, cls_use=False)
    for a, b in zip(got, ref):
        assert a.shape == b.shape
        assert (a.float().cpu() - b).norm() / b.norm() <= 3e-3
    with pytest.raises(_abi.KvqError, match="multiple"):
        m(torch.zeros(1, 3, 70, 64, device=DEV))
    with pytest.raises(_abi.KvqError, match="HIP device"):
        m(torch.zeros(1, 3, 64, 64))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("B,L,heads", [(3, 50, 12), (2, 197, 12), (1, 7, 2), (2, 300, 1)])
def test_mha_small(B, L, heads, dtype):
    g = torch.Generator().manual_seed(B * 1000 + L)
    D = heads * 64
    qkv = (torch.randn(B * L, 3 * D, generator=g) * 0.7).to(HALF[dtype])
    out = kernels.mha_small(qkv.to(DEV), B, L, heads).float().cpu()
    q, k, v = qkv.float().reshape(B, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    ref = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v).transpose(1, 2).reshape(B * L, D)
    assert (out - ref).abs().max().item() <= 2.1 * EPS[dtype] * max(1.0, ref.abs().max().item())


def test_vit_embed_ln_cls_mix_cosine_and_quickgelu():
    g = torch.Generator().manual_seed(5)
    B, G, D = 3, 49, 768
    tok, cls, pos = torch.randn(B * G, D, generator=g), torch.randn(D, generator=g), torch.randn(G + 1, D, generator=g)
    lw, lb = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    x = kernels.vit_embed_ln(tok.to(DEV), cls.to(DEV), pos.to(DEV), lw.to(DEV), lb.to(DEV), B)
    ref = torch.nn.functional.layer_norm(torch.cat([cls.expand(B, 1, D), tok.reshape(B, G, D)], 1) + pos, (D,), lw, lb)
    assert x.shape == (B, G + 1, D) and (x.cpu() - ref).abs().max().item() <= 2e-5
    cos = kernels.cosine_cls(x).cpu()
    assert (cos - torch.cosine_similarity(ref[:, :1], ref[:, 1:], dim=-1)).abs().max().item() <= 2e-6
    c16 = kernels.cls_gather(x, torch.float16)
    assert torch.equal(c16.cpu(), ref[:, 0].to(torch.float16)) or (c16.float().cpu() - ref[:, 0]).abs().max().item() <= 2.0 ** -10
    a = torch.randn(B, D, generator=g).to(torch.float16)
    before = x.clone()
    kernels.cls_mix(x, a.to(DEV), 0.5)
    assert (x[:, 0].cpu() - (0.5 * a.float() + 0.5 * before[:, 0].cpu())).abs().max().item() <= 1e-6
    assert torch.equal(x[:, 1:], before[:, 1:])
    # QuickGELU epilogue of the GEMM
    A = (torch.randn(70, 64, generator=g)).to(torch.float16)
    Wt = (torch.randn(40, 64, generator=g) / 8).to(torch.float16)
    bias = torch.randn(40, generator=g)
    y = kernels.gemm(A.to(DEV), Wt.to(DEV), bias.to(DEV), _abi.EPI_QGELU_BF16).float().cpu()
    z = A.float() @ Wt.float().t() + bias
    assert (y - z * torch.sigmoid(1.702 * z)).abs().max().item() <= 2.1 * 2.0 ** -11 * max(1.0, z.abs().max().item())


# ------------------------------------------------------------------ KSVQE CDM modules (models/backbones/ksvqe_modules.py)
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_cdm_modules_vs_reference_golden(golden, dtype):
    from kvq_amd.models.backbones import ksvqe_modules as KM
    from test_oracle_golden import _cdm_inputs
    g = golden("cdm.npz")
    w = {m: {k: torch.from_numpy(v) for k, v in sd.items()} for m, sd in synth.synth_cdm_weights(11).items()}
    x = {k: v.to(DEV) for k, v in _cdm_inputs().items()}
    mods = dict(cross=KM.crossattention1(768, 12), self=KM.Attention(768, 12), sem=KM.Semantic_Transformation2(768),
                dist=KM.Dist_Transformation3(768))
    for k, m in mods.items():
        m.load_state_dict(w[k], strict=True)
        m.operand_dtype = _abi.dtype_code(dtype)
        m.to(DEV).eval()
    with torch.no_grad():
        o, a = mods["cross"](x["Q"], x["K"])
        outs = dict(cross=o, self=mods["self"](x["xs"]), sem=mods["sem"](x["sem_x"], x["sem_in"]), dist=mods["dist"](x["dist_x"], x["dist_in"]))
    assert a is None
    tol = dict(cross=2.5, self=2.5, sem=0.02, dist=2.5)            # x the 16-bit epsilon, relative L2 (sem is fp32 end to end)
    for k, o in outs.items():
        arr = np.ascontiguousarray(o.float().cpu().numpy())
        assert tuple(g[f"{k}/shape"]) == arr.shape, k
        got, ref = arr.reshape(-1)[g[f"{k}/idx"]], g[f"{k}/val"]
        rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
        assert rel <= tol[k] * EPS[dtype], (k, rel)
    with pytest.raises(NotImplementedError):
        mods["self"](x["xs"], mask=torch.ones(98, 16, dtype=torch.bool, device=DEV))
    with pytest.raises(_abi.KvqError, match="HIP device"):
        mods["sem"](torch.zeros(1, 768, 7, 7), torch.zeros(1, 768, 7, 7))


MHA_CROSS_SHAPES = [(4, 49, 49, 12), (3, 16, 16, 12), (2, 100, 7, 3), (1, 64, 2, 2), (2, 128, 130, 1), (1, 129, 320, 1),
                    (1, 64, 320, 1),       # four key splits + the largest LDS request (K | V of 320 keys + three partial sets: 132 608 B)
                    (2, 50, 3, 2),         # four key splits over three keys: one part is empty
                    (1, 130, 9, 1)]        # just past the two-split form: a third query pass of two live rows


def _mha_cross_strided(B, Lq, Lk, heads, dtype):
    g = torch.Generator().manual_seed(Lq * 100 + Lk)
    D = heads * 64
    q = torch.randn(B * Lq, D, generator=g).to(HALF[dtype])
    kv = torch.randn(B * Lk, 2 * D + 8, generator=g).to(HALF[dtype])       # k and v interleaved in one buffer: strided rows
    kvd = kv.to(DEV)
    out = kernels.mha_cross(q.to(DEV), kvd[:, :D], kvd[:, D:2 * D], B, heads, 0.05).float().cpu()
    qh = q.float().reshape(B, Lq, heads, 64).transpose(1, 2)
    kh = kv[:, :D].float().reshape(B, Lk, heads, 64).transpose(1, 2)
    vh = kv[:, D:2 * D].float().reshape(B, Lk, heads, 64).transpose(1, 2)
    ref = (torch.softmax(qh @ kh.transpose(-1, -2) * 0.05, -1) @ vh).transpose(1, 2).reshape(B * Lq, D)
    assert (out - ref).abs().max().item() <= 2.1 * EPS[dtype] * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("B,Lq,Lk,heads", MHA_CROSS_SHAPES)
def test_mha_cross_strided(B, Lq, Lk, heads):
    _mha_cross_strided(B, Lq, Lk, heads, "fp16")


@pytest.mark.parametrize("B,Lq,Lk,heads", MHA_CROSS_SHAPES)
def test_mha_cross_strided_bf16(B, Lq, Lk, heads):
    _mha_cross_strided(B, Lq, Lk, heads, "bf16")


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("Lq", [64, 100])
def test_mha_cross_softmax_extremes(Lq, dtype):
    """A key that wins by about 90 in the logits and sits in the LAST 8-key chunk of the LAST wave's key split (Lq = 64: four
    splits of 80 keys; Lq = 100: two of 160), every other logit about -60: the wave that merges the parts holds a running
    maximum 90 below the winner's, so its own sum is scaled by exp(-90) and the part that holds the winner by 1.  Finite, and
    the float64 softmax to the output's rounding."""
    g = torch.Generator().manual_seed(900 + Lq)
    Lk, win = 320, 317
    q = (torch.randn(Lq, 64, generator=g) * 0.5).to(HALF[dtype])
    k = (torch.randn(Lk, 64, generator=g) * 0.5).to(HALF[dtype])
    v = torch.randn(Lk, 64, generator=g).to(HALF[dtype])
    q[:, 0], k[:, 0] = 8.0, -7.5                                            # every logit 8 * -7.5 = -60 (+ ~N(0, 2))
    k[win, 0] = 3.75                                                        # ... but this one: +30
    logits = q.double() @ k.double().t()
    top2 = logits.topk(2, dim=1).values
    assert (logits.argmax(1) == win).all() and float((top2[:, 0] - top2[:, 1]).min()) > 75.0
    ref = torch.softmax(logits, -1) @ v.double()
    out = kernels.mha_cross(q.to(DEV), k.to(DEV), v.to(DEV), 1, 1, 1.0).float().cpu()
    assert torch.isfinite(out).all()
    err = (out.double() - ref).abs().max().item()
    print(f"mha_cross extremes Lq={Lq} {dtype}: err {err:.3e} bound {2.1 * EPS[dtype] * max(1.0, ref.abs().max().item()):.3e}")
    assert err <= 2.1 * EPS[dtype] * max(1.0, ref.abs().max().item())


# ------------------------------------------------------------------ entry points that had no direct test
def _err_and_bound(got, ref64, ref32):
    """(max |got - ref|, bound): 8 x the error of the same expression evaluated by torch in fp32 on the CPU, floor 2^-22 max|ref| —
    the rule of test_gpu_headtrain.py (the kernel sums in another order and uses __expf; 8 x keeps any 16-bit rounding out)"""
    err = (got.double() - ref64).abs().max().item()
    bound = max(8.0 * (ref32.double() - ref64).abs().max().item(), 2.0 ** -22 * ref64.abs().max().item())
    return err, bound


@pytest.mark.parametrize("C", [64, 768, 100])
@pytest.mark.parametrize("M", [1, 98])
def test_sem_modulate_vs_float64(M, C):
    g = torch.Generator().manual_seed(M * 1000 + C)
    x, inp = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g) * 2.0
    wg, wb = torch.randn(C, generator=g) / C ** 0.5, torch.randn(C, generator=g) / C ** 0.5
    bg, bb = 0.3, -0.2
    # gate logits of +30 and -30 (the sigmoid saturates) in the first and the last row, ordinary ones between
    x[0] = x[0] + (30.0 - bg - float(wg @ x[0])) * wg / float(wg @ wg)
    if M > 1:
        x[-1] = x[-1] + (-30.0 - bg - float(wg @ x[-1])) * wg / float(wg @ wg)
    out = kernels.sem_modulate(x.to(DEV), inp.to(DEV), wg.to(DEV), bg, wb.to(DEV), bb).cpu()
    f = lambda x, inp, wg, wb: torch.sigmoid(x @ wg + bg)[:, None] * inp + (x @ wb + bb)[:, None]      # noqa: E731
    ref64 = f(x.double(), inp.double(), wg.double(), wb.double())
    assert abs(float(x[0].double() @ wg.double()) + bg - 30.0) < 1e-3
    err, bound = _err_and_bound(out, ref64, f(x, inp, wg, wb))
    print(f"sem_modulate M={M} C={C}: err {err:.3e} bound {bound:.3e}")
    assert out.shape == (M, C) and err <= bound


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("C", [64, 768, 100])
def test_dist_modulate_vs_float64(C, dtype):
    g = torch.Generator().manual_seed(C)
    B, rows = 2, 3
    inp = torch.randn(B, rows, C, generator=g) * 2.0
    gl, beta = (torch.randn(B, C, generator=g) * 2.0).to(HALF[dtype]), torch.randn(B, C, generator=g).to(HALF[dtype])
    gl[0, 0], gl[0, 1], gl[1, C - 1], gl[1, C - 2] = 30.0, -30.0, 30.0, -30.0
    out = kernels.dist_modulate(inp.to(DEV), gl.to(DEV), beta.to(DEV)).cpu()
    f = lambda inp, gl, beta: torch.sigmoid(gl)[:, None] * inp + beta[:, None]      # noqa: E731
    ref64 = f(inp.double(), gl.double(), beta.double())
    err, bound = _err_and_bound(out, ref64, f(inp, gl.float(), beta.float()))
    print(f"dist_modulate C={C} {dtype}: err {err:.3e} bound {bound:.3e}")
    assert out.shape == (B, rows, C) and err <= bound


@pytest.mark.parametrize("C", [64, 768, 100])
@pytest.mark.parametrize("M", [1, 98])
def test_axpby_vs_float64(M, C):
    g = torch.Generator().manual_seed(M + C)
    x, y = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g) * 3.0
    for a, b in ((0.2, 0.8), (0.5, -0.5)):
        out = kernels.axpby(x.to(DEV), y.to(DEV), a, b).cpu()
        a32, b32 = torch.tensor(a, dtype=torch.float32), torch.tensor(b, dtype=torch.float32)     # the kernel takes float arguments
        ref64 = a32.double() * x.double() + b32.double() * y.double()
        err, bound = _err_and_bound(out, ref64, a32 * x + b32 * y)
        print(f"axpby M={M} C={C} a={a} b={b}: err {err:.3e} bound {bound:.3e}")
        assert out.shape == (M, C) and err <= bound


CONVERT_LENGTHS = list(range(1, 10)) + [1027]


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_to_half_and_to_float_bit_exact(dtype):
    """``kvq_convert``: fp32 -> 16 bits is torch's round-to-nearest-even for finite values inside the type's range, at every tail
    length of the four-per-thread kernel (n % 4 = 0..3, n < 4, several blocks); 16 bits -> fp32 is exact."""
    g = torch.Generator().manual_seed(12)
    for n in CONVERT_LENGTHS:
        x = torch.randn(n, generator=g) * 10.0 ** torch.randint(-3, 4, (n,), generator=g).float()
        x[0] = 1.0 + 2.0 ** -11 if dtype == "fp16" else 1.0 + 2.0 ** -8            # a tie: rounds to even
        h = kernels.to_half(x.to(DEV), HALF[dtype])
        assert h.dtype == HALF[dtype] and h.shape == x.shape
        assert torch.equal(h.cpu().view(torch.int16), x.to(HALF[dtype]).view(torch.int16)), n
        f = kernels.to_float(h)
        assert f.dtype == torch.float32 and torch.equal(f.cpu(), x.to(HALF[dtype]).float()), n
    x = torch.randn(3, 343, generator=g)                                          # shape is kept
    assert kernels.to_half(x.to(DEV), HALF[dtype]).shape == (3, 343)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 2048, 100])
def test_l2_normalize_rows_vs_float64(D, dtype):
    """F.normalize(x, dim=1) in float64, every element within one 16-bit ulp (2 EPS |ref|); an all-zero row comes out as zeros
    (the 1e-12 floor of the norm), not NaN.  |x| >= 0.25 keeps every quotient inside fp16's normal range (smallest: 0.25 / ~60)."""
    g = torch.Generator().manual_seed(D)
    M = 5
    x = torch.randn(M, D, generator=g)
    x = torch.sign(x) * (0.25 + x.abs())
    x[1] *= 300.0
    x[2] *= 1e-3
    x[3] = 0.0
    out = kernels.l2_normalize_rows(x.to(DEV), HALF[dtype]).float().cpu()
    ref = x.double() / x.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    assert out.shape == (M, D) and torch.isfinite(out).all() and bool((out[3] == 0).all())
    excess = ((out.double() - ref).abs() - 2.0 * EPS[dtype] * ref.abs()).max().item()
    print(f"l2_normalize_rows D={D} {dtype}: max rel err {((out.double() - ref).abs() / ref.abs().clamp_min(1e-30)).max().item():.3e} "
          f"(bound {2.0 * EPS[dtype]:.3e})")
    assert excess <= 0.0


def test_keyframes_and_qrs_vs_reference_golden(golden):
    """Key-frame grouping (host index logic) and the QRS eval path (kvq_qrs_top_region + kvq_crop_regions): bit-exact
    against the reference's outputs — integer / copy work."""
    from kvq_amd.models.backbones import ksvqe_modules as KM
    from test_oracle_golden import _qrs_inputs
    g = golden("qrs.npz")
    x, score = _qrs_inputs()
    xd, sd = x.to(DEV), score.to(DEV)
    gid, key = KM.obtain_keyframes(xd[:, :, :, :16, :16].contiguous())
    assert np.array_equal(gid.cpu().numpy(), g["gid"])
    assert np.array_equal(key.contiguous().cpu().numpy().reshape(-1)[g["key/idx"]], g["key/val"])
    net = KM.RegionNet_CLIP(k=49, anchor_size=32, stride=1, num_samples=1).eval()
    out = net(xd, sd, 0.5, gid)
    assert out.shape == (2, 3, 16, 224, 224)
    assert np.array_equal(out.cpu().numpy().reshape(-1)[g["patches/idx"]], g["patches/val"])
    idx = kernels.qrs_top_region(sd.reshape(8, 7, 7).contiguous(), 9, 9, 7, 7).cpu().numpy().reshape(2, 4)
    assert np.array_equal(idx, g["idx"])
    # extend_by_group == the reference's .item() double loop
    per_key = torch.arange(2 * 4 * 5, dtype=torch.float32, device=DEV).reshape(2, 4, 5)
    full = KM.extend_by_group(per_key, gid).cpu()
    for i in range(2):
        for j in range(16):
            assert torch.equal(full[i, j], per_key[i, int(g["gid"][i, j])].cpu())
    # same grid as the map: no upsample; a tie keeps the first window
    flat = torch.zeros(3, 9, 9, device=DEV)
    assert kernels.qrs_top_region(flat, 9, 9, 7, 7).cpu().tolist() == [0, 0, 0]
    with pytest.raises(NotImplementedError):
        KM.RegionNet_CLIP(k=49, anchor_size=32, stride=1, sample_type="random").eval()(xd, sd, 0.5, gid)


@pytest.mark.parametrize("residual16", [True, False])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_contrique_vs_reference_golden(golden, dtype, residual16):
    """KSVQE's distortion branch on the HIP conv stack (implicit-GEMM ResNet-50 trunk on 32x32 patches, kvq_l2_normalize_rows,
    the BatchNorm-folded projector GEMMs) against the reference's stored output."""
    from kvq_amd.models.backbones import ksvqe_modules as KM
    z_ref = golden("contrique.npz")["z"]
    m = KM.CONTRIQUE_model(KM.get_network("resnet50"), 2048, residual16=residual16)     # both residual-stream widths stay pinned
    assert m.residual16 is residual16 and m._net.residual16 is residual16
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_contrique_weights(13).items()}, strict=True)
    m.operand_dtype = _abi.dtype_code(dtype)
    m = m.to(DEV).eval()
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(51)).standard_normal((1, 3, 3, 64, 96)).astype(np.float32))
    with torch.no_grad():
        z = m(x.to(DEV)).cpu().numpy()
    assert z.shape == z_ref.shape
    rel = np.linalg.norm(z - z_ref) / np.linalg.norm(z_ref)
    assert rel <= {"fp16": 1.5e-2, "bf16": 1e-1}[dtype], rel
    with pytest.raises(KeyError):
        KM.get_network("VGG16")


@pytest.mark.parametrize("dtype", ["fp16"])
def test_ksvqe_end_to_end_vs_reference_golden(golden, dtype):
    """The whole KSVQE forward on the HIP kernels (key frames -> CLIP_tool -> QRS -> CONTRIQUE / adapters -> trunk stage by
    stage with the CDM behind stages 2 and 3 -> norm) through VQA_Network, against the reference's stored features/loss."""
    from kvq_amd.models import VQA_Network
    g = golden("ksvqe.npz")
    net = VQA_Network({"model": {"args": {"KSVQE": {"backbone": dict(num_samples=1, sample_type="topkpertubation", CLIP_location=8,
                                                                       cls_use=True, tuning_stage=2, a1=1, a2=0, frozen_stages=-1),
                                                      "head": {"in_channels": 768, "hidden_channels": 64}}}}})
    bb = net.KSVQE_backbone
    missing = bb.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_ksvqe_weights(3).items()}, strict=False)
    assert not missing.unexpected_keys and all("relative_position_index" in k for k in missing.missing_keys)
    bb.operand_dtype = _abi.dtype_code(dtype)
    net = net.to(DEV).eval()
    inp = {k: torch.from_numpy(v).to(DEV) for k, v in synth.synth_ksvqe_inputs(4, b=2).items()}
    with torch.no_grad():
        (scores, feats, loss) = net(inputs=dict(inp), reduce_scores=True, return_pooled_feats=True)
        scores2, loss2 = net(inputs=dict(inp), reduce_scores=True)
    f = np.ascontiguousarray(feats["KSVQE"].float().cpu().numpy())
    assert f.shape == tuple(g["feat/shape"]) and scores.shape == (2, 1) and torch.equal(scores, scores2)
    got, ref = f.reshape(-1)[g["feat/idx"]], g["feat/val"]
    rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    assert rel <= 1e-2, rel
    assert abs(float(loss) - float(g["loss"])) <= 2e-2 and abs(float(loss2) - float(loss)) <= 1e-6
    # the head on the oracle's features vs on the HIP features: the score gate of the trunk tests
    from oracle import ksvqe_oracle as KO
    from oracle import swin3d_oracle as O
    hw = {k[len("KSVQE_head."):]: v.detach().cpu().numpy() for k, v in net.state_dict().items() if k.startswith("KSVQE_head.")}
    with torch.no_grad():
        f_or, _ = KO.ksvqe_forward({k: v.cpu() for k, v in inp.items()}, synth.synth_ksvqe_weights(3), synth.SWIN_T_GRPB)
        s_or = O.vqa_head(f_or, hw)
    assert (scores.float().cpu() - s_or).abs().max().item() <= 1e-3


def test_ksvqe_feature_taps_vs_reference_golden(golden):
    """KSVQE.forward(multi=True) / (layer=k) (KSVQE_model.py:1489-1498; no caller asks for them): feats = [behind the embedding,
    behind every stage — a tuned stage after its CDM], against the reference's stored outputs."""
    from kvq_amd.models.backbones.KSVQE_model import KSVQE
    g = golden("ksvqe.npz")
    bb = KSVQE(num_samples=1, sample_type="topkpertubation", CLIP_location=8, cls_use=True, tuning_stage=2, a1=1, a2=0, frozen_stages=-1)
    bb.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_ksvqe_weights(3).items()}, strict=False)
    bb.operand_dtype = _abi.dtype_code("fp16")
    bb = bb.to(DEV).eval()
    inp = {k: torch.from_numpy(v).to(DEV) for k, v in synth.synth_ksvqe_inputs(4, b=2).items()}
    with torch.no_grad():
        outs = {"multi": bb(dict(inp), multi=True), "layer0": bb(dict(inp), layer=0), "layer2": bb(dict(inp), layer=2),
                "layer4": bb(dict(inp), layer=4)}
        with pytest.raises(IndexError):
            bb(dict(inp), layer=5)
    for k, v in outs.items():
        f = np.ascontiguousarray(v.float().cpu().numpy())
        assert f.shape == tuple(g[f"{k}/shape"]), (k, f.shape)
        got, ref = f.reshape(-1)[g[f"{k}/idx"]], g[f"{k}/val"]
        rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
        assert rel <= (2e-3 if k == "layer0" else 1e-2), (k, rel)


def test_crop_regions_scalar_and_vector_paths():
    """kvq_crop_regions against the same gather written with slices: 6-pixel anchors (scalar kernel) and 32-pixel ones (16-byte
    kernel) — copy work, bit-exact."""
    gen = np.random.Generator(np.random.PCG64(3))
    for anchor, grid, k in ((6, 5, 3), (32, 4, 2)):
        xs = torch.from_numpy(gen.standard_normal((2, 3, 4, grid * anchor, grid * anchor)).astype(np.float32))
        nx = grid - k + 1
        reg = torch.from_numpy(gen.integers(0, nx * nx, size=8).astype(np.int32))
        got = kernels.crop_regions(xs.to(DEV), reg.to(DEV), anchor, k, k).cpu()
        assert got.shape == (2, 3, 4, k * anchor, k * anchor)
        for b in range(2):
            for t in range(4):
                ry, rx = divmod(int(reg[b * 4 + t]), nx)
                assert torch.equal(got[b, :, t], xs[b, :, t, ry * anchor:(ry + k) * anchor, rx * anchor:(rx + k) * anchor])
