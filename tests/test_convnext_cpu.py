"""ConvNeXt-3D (model key ``conv_tiny``), everything that needs no GPU: the torch-CPU restatement against the reference's stored
outputs, ``inflate_weights``, the mirror's state_dict, the model-key rule, the new ABI symbols and the host query of the
depthwise-conv launch, and the synthetic dataset's ``aesthetic`` view switch."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import kvq_amd  # noqa: F401
from kvq_amd import _abi
from kvq_amd.utils import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnext_ref as R  # noqa: E402

HEAD = {"in_channels": 768, "hidden_channels": 64}
INFLATE = dict(seed=13, dims=(8, 16, 32, 64), depths=(1, 2, 1, 1))


def _case(g, name):
    wseed, cseed, B, T, H, W = (int(v) for v in g[f"{name}/meta"])
    return synth.synth_convnext_weights(wseed, "stress"), torch.from_numpy(synth.synth_clip(cseed, T, H, W, batch=B)), wseed


@pytest.mark.parametrize("name", ["A", "B"])
def test_restatement_fp32_matches_the_reference(golden, name):
    g = golden("convnext.npz")
    wts, x, wseed = _case(g, name)
    with torch.no_grad():
        feat, norms, ratios = R.forward(wts, x, dtype=torch.float32, details=True)
        multi = R.forward(wts, x, dtype=torch.float32, multi=True)
    assert tuple(feat.shape) == g[f"{name}/feat"].shape and tuple(multi.shape) == g[f"{name}/multi"].shape and multi.shape[1] == 672
    e, em = R.rel_l2(feat, g[f"{name}/feat"]), R.rel_l2(multi, g[f"{name}/multi"])
    print(f"case {name}: rel-L2 feat {e:.3e} (stored {float(g[f'{name}/err_fp32']):.3e}), multi {em:.3e}")
    assert e <= 2 * float(g[f"{name}/err_fp32"])
    assert em <= 2 * float(g[f"{name}/err_fp32_multi"])
    np.testing.assert_allclose(norms, g[f"{name}/stage_norms"], rtol=1e-4)
    assert min(ratios) >= 0.2                       # every block is visible in the fixture
    score = R.head_score(synth.synth_vqa_head_weights(768, 64, wseed, "stress"), feat)
    np.testing.assert_allclose(score.numpy().reshape(-1), g[f"{name}/score"], rtol=0, atol=1e-5)


def _mirror(**kw):
    from kvq_amd.models.backbones.conv_backbone import ConvNeXt3D
    return ConvNeXt3D(**kw)


def test_inflate_weights_is_bit_equal_to_the_reference(golden):
    g = golden("convnext.npz")
    net = _mirror(depths=INFLATE["depths"], dims=INFLATE["dims"])
    src = {k: torch.from_numpy(v) for k, v in synth.synth_convnext2d_checkpoint(INFLATE["seed"], INFLATE["depths"], INFLATE["dims"]).items()}
    net.inflate_weights(src)
    sd = net.state_dict()
    keys = [k[len("inflate/"):] for k in g.files if k.startswith("inflate/")]
    assert sorted(keys) == sorted(sd)
    for k in keys:
        assert np.array_equal(sd[k].numpy(), g["inflate/" + k]), k
    assert sd["stages.1.1.dwconv.weight"].shape == (16, 1, 3, 7, 7) and sd["stages.1.0.dwconv.weight"].shape == (16, 1, 1, 7, 7)


def test_mirror_state_dict_is_the_reference_layout():
    from kvq_amd.models.backbones.conv_backbone import convnext_3d_small, convnext_3d_tiny
    net = convnext_3d_tiny(pretrained=False)
    shapes = synth.convnext_param_shapes()
    sd = net.state_dict()
    assert list(sd) == list(shapes)
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(shapes)
    n = sum(v.numel() for v in sd.values())
    assert round(n / 1e6, 2) == 28.04
    # block j of a stage takes kt = int('131'[j % 3]); the reference's initial layer scale
    assert [sd[f"stages.2.{j}.dwconv.weight"].shape[2] for j in range(9)] == [1, 3, 1] * 3
    assert float(sd["stages.0.0.gamma"][0]) == pytest.approx(1e-6)
    assert list(convnext_3d_small().state_dict()) == list(synth.convnext_param_shapes(depths=(3, 3, 27, 3)))
    r = net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_convnext_weights(3).items()}, strict=True)
    assert not r.missing_keys and not r.unexpected_keys


def test_synth_convnext_draws():
    w = synth.synth_convnext_weights(5, "stress")
    g = w["stages.0.0.gamma"]
    assert g.min() >= 0.5 and g.max() <= 1.5
    for k in ("downsample_layers.0.1.weight", "downsample_layers.2.0.weight", "stages.1.2.norm.weight", "norm.weight"):
        assert abs(float(w[k].mean()) - 1.0) < 0.1, k               # LayerNorm weights are drawn around 1
    assert abs(float(w["downsample_layers.2.1.weight"].mean())) < 0.01      # ... the conv behind the norm is not
    wi = synth.synth_convnext_weights(5, "init")
    assert np.all(wi["stages.3.2.gamma"] == np.float32(1e-6)) and np.all(wi["downsample_layers.1.0.weight"] == 1)


def test_model_key_needs_an_explicit_pretrained_entry(tmp_path):
    from kvq_amd.models.model import VQA_Network
    net = VQA_Network({"model": {"args": {"conv_tiny": {"backbone": {"pretrained": False}, "head": HEAD}}}})
    assert net.key_names == ["conv_tiny"]
    assert type(net.conv_tiny_backbone).__name__ == "ConvNeXt3D" and type(net.conv_tiny_head).__name__ == "VQAHead"
    for bad in ({}, {"head": HEAD}, {"backbone": {}, "head": HEAD}, {"backbone": {"pretrained": True}, "head": HEAD}):
        with pytest.raises(NotImplementedError, match="conv_tiny"):
            VQA_Network({"model": {"args": {"conv_tiny": bad}}})
    # a local 2D checkpoint is inflated on load
    src = synth.synth_convnext2d_checkpoint(7)
    path = str(tmp_path / "convnext_tiny_2d.pth")
    torch.save({"model": {k: torch.from_numpy(v) for k, v in src.items()}}, path)
    net = VQA_Network({"model": {"args": {"conv_tiny": {"backbone": {"pretrained": path}, "head": HEAD}}}})
    sd = net.conv_tiny_backbone.state_dict()
    assert torch.equal(sd["stages.0.1.dwconv.weight"], torch.from_numpy(src["stages.0.1.dwconv.weight"]).unsqueeze(2).repeat(1, 1, 3, 1, 1) / 3)
    assert torch.equal(sd["downsample_layers.0.0.weight"], torch.from_numpy(src["downsample_layers.0.0.weight"]).unsqueeze(2).repeat(1, 1, 2, 1, 1) / 2)
    assert torch.equal(sd["stages.2.4.pwconv2.weight"], torch.from_numpy(src["stages.2.4.pwconv2.weight"]))
    assert torch.equal(sd["stages.2.4.gamma"], torch.from_numpy(src["stages.2.4.gamma"]))


def test_forward_refuses_what_it_cannot_mirror():
    net = _mirror(depths=(1, 1, 1, 1))
    x = torch.zeros(1, 3, 4, 32, 32)
    with pytest.raises(NotImplementedError, match="UnboundLocalError"):
        net({"aesthetic": x}, layer=1)
    with pytest.raises(_abi.KvqError, match="no CPU path"):
        net({"aesthetic": x})
    with pytest.raises(_abi.KvqError, match="no CPU path"):
        net({"asesthetic": x, "aesthetic": None})           # the reference's spelling wins when both are there


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kvq_hip.h")).read()
    lib = _abi.lib()
    for name in ("kvq_dwconv3d_ln", "kvq_dwconv3d_ln_supported", "kvq_gemm_resid_scaled"):
        assert re.search(r"\b%s\(" % name, header) and name in _abi.SYMBOLS
        assert getattr(lib, name) is not None
    assert "KVQ_EPI_RESID_SCALE_F32 = 7" in header and _abi.EPI_RESID_SCALE_F32 == 7
    assert lib.kvq_abi_version() == 32 and C.sizeof(_abi.KvqGemmArgs) == 144
    assert C.sizeof(_abi.KvqDwconvLnArgs) == 88


def test_dwconv3d_ln_supported_answers_on_the_host():
    lib = _abi.lib()
    for Cc in (96, 192, 384, 768):
        for kt in (1, 3):
            assert lib.kvq_dwconv3d_ln_supported(Cc, kt, 16, 56, 56) == 1
            assert lib.kvq_dwconv3d_ln_supported(Cc, kt, 1, 1, 1) == 1         # planes smaller than the window
    assert lib.kvq_dwconv3d_ln_supported(100, 3, 4, 8, 8) == 0
    assert lib.kvq_dwconv3d_ln_supported(96, 5, 4, 8, 8) == 0
    assert lib.kvq_dwconv3d_ln_supported(96, 3, 0, 8, 8) == 0
    # NULL arguments and shapes outside the set are refused before any launch (no device needed)
    assert lib.kvq_dwconv3d_ln(None, None) == -1
    a = _abi.KvqDwconvLnArgs()
    assert lib.kvq_dwconv3d_ln(C.byref(a), None) == -1
    assert lib.kvq_gemm_resid_scaled(None, None, None) == -1
    buf = (C.c_float * 256)()
    p = C.addressof(buf)
    a.x = a.w = a.bias = a.ln_w = a.ln_b = a.out_f32 = p        # host memory: never dereferenced, the shape is refused first
    for Cc, kt in ((100, 3), (96, 5), (128, 1)):
        a.B, a.T, a.H, a.W, a.C, a.kt = 1, 2, 4, 4, Cc, kt
        assert lib.kvq_dwconv3d_ln(C.byref(a), None) == -3
        assert b"unsupported shape" in lib.kvq_last_error()


def test_synthetic_dataset_without_an_aesthetic_entry_is_unchanged():
    from kvq_amd.datasets.fusion_datasets import SyntheticKVQDataset
    tech = dict(fragments_h=7, fragments_w=7, fsize_h=32, fsize_w=32, aligned=8, clip_len=32, frame_interval=1, num_clips=2)
    ds = SyntheticKVQDataset({"num_videos": 2, "sample_types": {"technical": tech}}, device="cpu")
    assert ds.aopt is None and ds.asampler is None and ds.sopt == tech and ds.sampler is not None
    ds2 = SyntheticKVQDataset({"num_videos": 2, "sample_types": {"aesthetic": dict(size_h=224, size_w=224, clip_len=32, frame_interval=2,
                                                                                  num_clips=1)}}, device="cpu")
    assert ds2.sopt is None and ds2.sampler is None and ds2.asampler.frame_interval == 2
    with pytest.raises(KeyError):
        SyntheticKVQDataset({"sample_types": {}}, device="cpu")
