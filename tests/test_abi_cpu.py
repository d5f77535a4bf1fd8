"""CPU: the C-ABI library loads and exports every symbol include/kvq_hip.h declares (no compute
calls without a GPU); host-side module logic (state_dict surface, config dispatch, error paths)."""
import ctypes
import os
import re

import pytest
import torch

import kvq_amd  # noqa: F401
from kvq_amd import _abi, _build
from kvq_amd.models import VQA_Network
from kvq_amd.utils import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_builds_and_exports_every_declared_symbol():
    _build.build()
    header = open(os.path.join(ROOT, "include", "kvq_hip.h")).read()
    declared = set(re.findall(r"\b(kvq_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 17
    handle = _abi.lib()
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in kvq_hip.h but not exported"
    assert declared == set(_abi.SYMBOLS), declared ^ set(_abi.SYMBOLS)
    assert handle.kvq_abi_version() == _abi.ABI_VERSION == 32


def test_library_reads_only_the_documented_environment_switches():
    """The library's kernel choice follows its arguments, not the process environment, except for these switches (README.md): the bench's
    latency leg, the fp32 residual-stream escape hatch, the GEMM tile mode's initial value and three probes of -DKVQ_DIAG builds."""
    names = set()
    for f in sorted(os.listdir(_build.CSRC)):
        names |= set(re.findall(r'getenv\(\s*"(KVQ_[A-Z0-9_]+)"', open(os.path.join(_build.CSRC, f)).read()))
    assert names == {"KVQ_LATENCY", "KVQ_RESID16", "KVQ_GEMM8P", "KVQ_SKIP", "KVQ_IMAGE_ONE_TYPE", "KVQ_NO_Q_STORE"}, sorted(names)


def test_struct_layouts_match_header_sizes():
    import ctypes as C
    assert C.sizeof(_abi.KvqSwinCfg) == 4 * (3 + 1 + 1 + 1 + 4 + 4 + 3 + 1 + 4 + 3)
    assert C.sizeof(_abi.KvqSwinBlockW) == 18 * 8
    assert C.sizeof(_abi.KvqBlockTailArgs) == 152          # ABI 31: + x_f16
    assert C.sizeof(_abi.KvqSwinWeights) == 5 * 8 + 8 + 3 * 4 * 8 + 2 * 8
    assert C.sizeof(_abi.KvqPatchMergeArgs) == 104         # ABI 31: + x_f16, out_f16
    assert C.sizeof(_abi.KvqPatchEmbedArgs) == 136         # ABI 31: + out_f16
    assert C.sizeof(_abi.KvqFragmentSource) == 3 * 16 * 8 + 8 + 10 * 4 + 2 * 16 + 8
    assert C.sizeof(_abi.KvqAttnDenseArgs) == 104
    assert C.sizeof(_abi.KvqGemmArgs) == 144
    assert C.sizeof(_abi.KvqConvArgs) == 160
    assert _abi.dtype_code('bf16') == 0 and _abi.dtype_code(torch.float16) == 1


def test_fragment_source_eligibility_is_host_logic():
    """kvq_patch_embed_fragments_supported decides on the host whether the embedding launch may read through the sampler
    (include/kvq_hip.h): uint8 frames, 4 x 4 patches inside the mini-patches, canvas = grid x mini-patch, source >= canvas,
    whole aligned frame groups, one clip per 32 tokens, a sane channel stride."""
    handle = _abi.lib()
    f = _abi.KvqFragmentSource()
    f.n_clips, f.src_is_u8, f.Hs, f.Ws, f.Fh, f.Fw, f.fs_h, f.fs_w, f.aligned = 4, 1, 540, 960, 7, 7, 32, 32, 8
    ok = lambda *a: handle.kvq_patch_embed_fragments_supported(f, *a)          # noqa: E731  (B, in_chans, pd, T, H, W)
    assert ok(4, 3, 2, 32, 224, 224) == 1
    assert ok(3, 3, 2, 32, 224, 224) == 0 and ok(17, 3, 2, 32, 224, 224) == 0       # batch != clips; more clips than the struct holds
    assert ok(4, 3, 2, 32, 224, 256) == 0                                            # canvas != grid x mini-patch
    assert ok(4, 3, 2, 30, 224, 224) == 0                                            # T % aligned
    assert ok(4, 5, 2, 32, 224, 224) == 0                                            # mean / std hold 4 channels
    f.chan_stride = 32 * 540 * 960 - 1
    assert ok(4, 3, 2, 32, 224, 224) == 0                                            # planes would overlap
    f.chan_stride = 256 * 540 * 960
    assert ok(4, 3, 2, 32, 224, 224) == 1                                            # clips = runs of frames of a 256-frame video
    f.src_is_u8 = 0
    assert ok(4, 3, 2, 32, 224, 224) == 0
    f.src_is_u8, f.fs_h, f.Fh = 1, 14, 16
    assert ok(4, 3, 2, 32, 224, 224) == 0                                            # patch rows would span two mini-patches
    f.fs_h, f.Fh, f.Hs = 32, 7, 200
    assert ok(4, 3, 2, 32, 224, 224) == 0                                            # source smaller than the canvas
    f.Hs, f.Fh, f.Fw = 540, 1, 1
    assert ok(4, 3, 2, 8, 32, 32) == 1                                               # 4 x 8 x 8 = 256 tokens per clip
    f.fs_h = f.fs_w = 12
    f.aligned = 2
    assert ok(4, 3, 2, 2, 12, 12) == 0                                               # 9 tokens per clip: a wave of 32 would straddle clips
    assert ok(4, 3, 2, 64, 12, 12) == 1                                              # 32 x 9 tokens
    assert handle.kvq_patch_embed_fragments_supported(None, 4, 3, 2, 32, 224, 224) == 0


def test_error_paths_without_gpu():
    handle = _abi.lib()
    rc = handle.kvq_gemm_bf16(None, None)
    assert rc == -1 and b"NULL" in handle.kvq_last_error()
    import ctypes as C
    cfg = _abi.KvqSwinCfg()
    out = C.c_void_p()
    rc = handle.kvq_swin3d_plan_create(C.byref(cfg), 1, 32, 224, 224, _abi.DT_FP16, C.byref(out))
    assert rc == -3          # num_stages == 0 -> unsupported, reported not crashed
    with pytest.raises(_abi.KvqError):
        _abi.check(rc, "plan")


_HOST_BUFFER = (ctypes.c_char * 4112)()


def _operand_guard_cases():
    """(entry, arguments, text of kvq_last_error()) for the exported entries that take an operand dtype and check it before their
    first HIP call: a valid small shape, real int32 / int64 arrays where the entry reads them on the host, one 16-byte-aligned host
    buffer for every pointer, and dtype 7.  The texts are pinned as they are: an entry that delegates answers in its delegate's name."""
    import ctypes as C
    i32 = C.c_int32
    P = C.c_void_p((C.addressof(_HOST_BUFFER) + 15) & ~15)
    BAD = 7
    dims5, dims4 = (i32 * 5)(1, 3, 2, 8, 8), (i32 * 4)(1, 2, 8, 8)
    k3, s3, p3 = (i32 * 3)(1, 7, 7), (i32 * 3)(1, 2, 2), (i32 * 3)(0, 3, 3)
    strides5 = (C.c_int64 * 5)(384, 128, 64, 8, 1)

    def struct(cls, **kw):
        a = cls()
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    attn32 = struct(_abi.KvqAttnDenseArgs, qkv=P, bias_dense=P, n_types=1, BW=1, nW=1, N=8, num_heads=1, dtype=BAD, out=P, dsplit_from=-1)
    gemm = struct(_abi.KvqGemmArgs, A=P, W=P, M=8, N=8, K=32, epilogue=_abi.EPI_RESID_F32, out_f32=P, resid_f32=P, dtype=BAD)
    conv = struct(_abi.KvqConvArgs, x=P, W=P, dims5=dims5, kernel3=k3, stride3=s3, pad3=p3, Kpad=32, N=8, epilogue=_abi.EPI_BIAS_BF16,
                  dtype=BAD, out_bf16=P)
    dw = struct(_abi.KvqDwconvLnArgs, x=P, w=P, bias=P, ln_w=P, ln_b=P, B=1, T=1, H=2, W=2, C=96, kt=1, eps=1e-6, dtype=BAD, out_h=P)
    grn = struct(_abi.KvqGrnArgs, x=P, y=P, gamma=P, beta=P, ws=P, B=1, D=1, H=2, W=2, N=384, dtype=BAD)
    tail = struct(_abi.KvqBlockTailArgs, attn=P, x=P, out_rows=32, M=32, C=96, hidden=384, pack=P, eps=1e-5, dtype=BAD)
    embed = struct(_abi.KvqPatchEmbedArgs, x=P, B=1, in_chans=3, T=2, H=32, W=32, pd=2, ph=4, pw=4, embed_dim=96, pack=P, out=P, eps=1e-5,
                   dtype=BAD)
    merge = struct(_abi.KvqPatchMergeArgs, x=P, merge_map=P, B=1, L=128, Ln=32, C=96, pack=P, out=P, eps=1e-5, dtype=BAD)
    ops, tensors, net = (_abi.KvqNetOp * 1)(), (_abi.KvqNetTensor * 2)(), C.c_void_p()
    cfg, plan = struct(_abi.KvqSwinCfg, num_stages=1), C.c_void_p()
    return [
        ("kvq_mha_cross", (P, 64, P, 64, P, 64, 1, 4, 4, 1, 64, 0.125, BAD, P, None), "kvq_mha_cross: dtype 7"),
        ("kvq_mha_small", (P, 1, 4, 1, 64, BAD, P, None), "kvq_mha_cross: dtype 7"),
        ("kvq_cls_gather", (P, 1, 2, 8, BAD, P, None), "kvq_cls_gather: dtype 7"),
        ("kvq_cls_mix", (P, P, 1, 2, 8, 0.5, BAD, None), "kvq_cls_mix: dtype 7"),
        ("kvq_convert", (P, P, 8, 1, BAD, None), "kvq_convert: dtype 7"),
        ("kvq_dist_modulate", (P, P, P, 1, 2, 8, BAD, P, None), "kvq_dist_modulate: dtype 7"),
        ("kvq_l2_normalize_rows", (P, 2, 8, BAD, P, None), "kvq_l2_normalize_rows: dtype 7"),
        ("kvq_patch_im2col", (P, 1, 3, 2, 8, 8, 2, 4, 4, BAD, P, None), "kvq_patch_im2col: dtype 7"),
        ("kvq_pack_clip_cl4", (P, dims5, 4, BAD, P, None), "kvq_pack_clip_cl4: dtype 7"),
        ("kvq_conv_stem_mfma", (P, dims4, P, P, k3, s3, p3, 1, BAD, P, None), "kvq_conv_stem_mfma: dtype 7"),
        ("kvq_conv_stem_pool", (P, dims5, P, P, 1, 1, BAD, P, None), "kvq_conv_stem_pool: dtype 7"),
        ("kvq_conv_stem64_pool", (P, dims5, None, 2, P, P, 1, BAD, P, 64, 0, None), "kvq_conv_stem64_pool: dtype 7"),
        ("kvq_im2col_nd", (P, 1, BAD, strides5, dims5, k3, s3, p3, 160, P, None), "kvq_im2col_nd: dtype 7"),
        ("kvq_pool_nd", (P, BAD, dims5, k3, s3, p3, 1, P, None), "kvq_pool_nd: dtype 7"),
        ("kvq_pool_nd_strided", (P, BAD, dims5, k3, s3, p3, 1, P, 8, 0, None), "kvq_pool_nd: dtype 7"),
        ("kvq_pack_channels_last8", (P, dims5, strides5, BAD, P, None), "kvq_pack_channels_last8: dtype 7"),
        ("kvq_mean_std_pool", (P, BAD, 2, 4, 8, P, 16, 0, 8, None), "kvq_mean_std_pool: dtype 7"),
        ("kvq_conv_stem_direct", (P, dims5, P, P, 8, k3, s3, p3, 1, BAD, P, None), "kvq_conv_stem_direct: dtype 7"),
        ("kvq_window_attention", (P, P, P, None, None, 8, 0, 1, 1, 8, 1, 0, BAD, P, None), "kvq_window_attention: dtype 7"),
        ("kvq_window_attention32", (attn32, None), "kvq_window_attention32: dtype 7"),
        ("kvq_window_attention32_ranges", (attn32, P, None), "kvq_window_attention32_ranges: dtype 7"),
        ("kvq_fast_bottleneck", (P, dims4, 8, 8, 32, 1, 1, P, BAD, P, None), "kvq_fast_bottleneck: dtype 7"),
        ("kvq_slow_bottleneck", (P, dims4, 256, 64, 256, P, BAD, P, 256, None), "kvq_slow_bottleneck: dtype 7"),
        ("kvq_layernorm_rows", (P, None, 1, 1, 2, 2, 8, P, P, 1e-5, P, BAD, None, None), "kvq_layernorm_rows: dtype 7"),
        ("kvq_dwconv3d_ln", (dw, None), "kvq_dwconv3d_ln: dtype 7"),
        ("kvq_patch_embed", (embed, None), "kvq_patch_embed: dtype 7"),
        ("kvq_patch_merge_pack", (P, P, P, 96, BAD, P, None), "kvq_patch_merge_pack: dtype 7"),
        ("kvq_patch_merge", (merge, None), "kvq_patch_merge: dtype 7"),
        ("kvq_gemm_bf16", (gemm, None), "kvq_gemm_bf16: unknown dtype 7"),
        ("kvq_gemm_resid_scaled", (gemm, P, None), "kvq_gemm_bf16: unknown dtype 7"),
        ("kvq_qkv_fill_pad", (P, P, P, 1, 1, 8, 1, 1.0, BAD, None), "kvq_qkv_fill_pad: dtype 7"),
        ("kvq_conv_implicit", (conv, None), "kvq_conv_implicit: dtype 7"),
        ("kvq_grn_stats", (grn, None), "kvq_grn_stats: dtype 7"),
        ("kvq_grn_apply", (grn, None), "kvq_grn_apply: dtype 7"),
        ("kvq_block_tail", (tail, None), "kvq_block_tail: dtype 7"),
        ("kvq_convnet_create", (ops, 1, tensors, 2, 1, 1, BAD, C.byref(net)), "kvq_convnet_create: dtype 7"),
        ("kvq_swin3d_plan_create", (C.byref(cfg), 1, 2, 32, 32, BAD, C.byref(plan)), "unknown dtype 7"),
    ]


def test_unknown_operand_dtype_is_refused_before_any_launch():
    handle = _abi.lib()
    cases = _operand_guard_cases()
    assert len({name for name, _, _ in cases}) == len(cases)
    for name, args, text in cases:
        rc = getattr(handle, name)(*args)
        assert rc == -3, (name, rc, handle.kvq_last_error())          # KVQ_ERR_UNSUPPORTED
        assert handle.kvq_last_error().decode() == text, (name, handle.kvq_last_error())


def test_state_dict_surface_matches_reference_keys():
    net = VQA_Network({"model": {"args": {"swin_tiny_grpb": {"head": {"in_channels": 768, "hidden_channels": 64}}}}})
    sd = net.state_dict()
    for k, shp in synth.swin_param_shapes(synth.SWIN_T_GRPB).items():
        assert tuple(sd["swin_tiny_grpb_backbone." + k].shape) == shp, k
    for k, shp in synth.vqa_head_param_shapes().items():
        assert tuple(sd["swin_tiny_grpb_head." + k].shape) == shp, k
    assert sd["swin_tiny_grpb_backbone.layers.0.blocks.0.attn.relative_position_index"].shape == (392, 392)
    assert "swin_tiny_grpb_backbone.layers.3.blocks.0.attn.fragment_position_bias_table" not in sd
    n = sum(p.numel() for p in net.swin_tiny_grpb_backbone.parameters())
    assert abs(n / 1e6 - 28.08) < 0.01       # 28.08 M parameters
    # DataParallel-prefixed checkpoints (trainer.py:62-74) strip to these names
    net.load_state_dict({k: v for k, v in sd.items()})


def test_model_keys_and_errors():
    tiny = VQA_Network({"model": {"args": {"swin_tiny": {"backbone": {}, "head": {}}}}})
    assert tiny.key_names == ["swin_tiny"] and not tiny.swin_tiny_backbone.frag_biases[0]
    m = VQA_Network({"model": {"args": {"swin_tiny_grpb_m": {"head": {}}}}})
    assert m.swin_tiny_grpb_m_backbone.window_size == (4, 4, 4)
    with pytest.raises(NotImplementedError):
        VQA_Network({"model": {"args": {"unknown_key": {}}}})
    with pytest.raises(NotImplementedError, match="conv_tiny"):
        VQA_Network({"model": {"args": {"conv_tiny": {}}}})
    with pytest.raises(_abi.KvqError, match="no CPU path"):
        tiny(inputs={"technical": torch.zeros(1, 3, 8, 64, 64)})


def test_relative_position_index_buffer_matches_golden(golden):
    from kvq_amd.models.backbones.swin_backbone import _rel_pos_index
    g = golden("layout.npz")
    assert torch.equal(_rel_pos_index((8, 7, 7)), torch.from_numpy(g["rpi_877"].astype("int64")))
