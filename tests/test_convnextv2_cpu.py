"""ConvNeXt-V2 3D (model key ``conv_v2_tiny``), everything that needs no GPU: the torch-CPU restatement against the reference's stored
outputs and against the reference GRN module's own outputs, the mirror's state_dict, ``inflate_weights(path)``, the factories, the model
key and its yml, the new ABI symbols and the host query of the GRN launches."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch
import yaml

import kvq_amd  # noqa: F401
from kvq_amd import _abi
from kvq_amd.utils import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnextv2_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = {"in_channels": 768, "hidden_channels": 64}
INFLATE = dict(seed=33, dims=(8, 16, 32, 64), depths=(1, 2, 1, 1), num_classes=10)


def _case(g, name):
    wseed, cseed, B, T, H, W = (int(v) for v in g[f"{name}/meta"])
    return synth.synth_convnextv2_weights(wseed, "stress"), torch.from_numpy(synth.synth_clip(cseed, T, H, W, batch=B)), wseed


@pytest.mark.parametrize("name", ["A", "B"])
def test_restatement_fp32_matches_the_reference(golden, name):
    g = golden("convnextv2.npz")
    wts, x, wseed = _case(g, name)
    with torch.no_grad():
        feat, norms, ratios, terms = R.forward(wts, x, dtype=torch.float32, details=True)
        multi = R.forward(wts, x, dtype=torch.float32, multi=True)
    assert tuple(feat.shape) == g[f"{name}/feat"].shape and tuple(multi.shape) == g[f"{name}/multi"].shape and multi.shape[1] == 672
    e, em = R.rel_l2(feat, g[f"{name}/feat"]), R.rel_l2(multi, g[f"{name}/multi"])
    print(f"case {name}: rel-L2 feat {e:.3e} (stored {float(g[f'{name}/err_fp32']):.3e}), multi {em:.3e}")
    assert e <= 3 * float(g[f"{name}/err_fp32"])
    assert em <= 3 * float(g[f"{name}/err_fp32_multi"])
    np.testing.assert_allclose(norms, g[f"{name}/stage_norms"], rtol=1e-4)
    assert min(ratios) >= 0.2 and min(terms) >= 0.2          # every block, and GRN inside every block, is visible in the fixture
    # ... and the fixture tells the two GRN definitions apart
    assert float(g[f"{name}/err_thw"]) >= 10 * float(g[f"{name}/err_emul_fp16"])
    score = R.head_score(synth.synth_vqa_head_weights(768, 64, wseed, "stress"), feat)
    np.testing.assert_allclose(score.numpy().reshape(-1), g[f"{name}/score"], rtol=0, atol=1e-5)


@pytest.mark.parametrize("i", [0, 1])
def test_grn_restatement_is_the_reference_module(golden, i):
    g = golden("convnextv2.npz")
    x, gamma, beta = (torch.from_numpy(g[f"grn/{i}/{k}"]) for k in ("x", "gamma", "beta"))
    assert x.dtype == torch.float64 and x.dim() == 5
    y = R.grn(x, gamma, beta, "th")
    assert float((y - torch.from_numpy(g[f"grn/{i}/y"])).abs().max()) <= 1e-12
    if x.shape[3] > 1:                                       # (T, H, W) statistics are a different function
        assert float((R.grn(x, gamma, beta, "thw") - y).abs().max()) > 1e-3
    if i == 1:                                               # the all-zero channel: Gx = 0, y = beta
        assert torch.equal(y[..., 3], beta.reshape(-1)[3].expand(y.shape[:-1]))


def test_mirror_state_dict_is_the_reference_layout(golden):
    from kvq_amd.models.backbones.conv_backbone import ConvNeXtV23D, convnextv2_3d_tiny
    g = golden("convnextv2.npz")
    net = convnextv2_3d_tiny(pretrained=False)
    assert type(net) is ConvNeXtV23D and net.grn_over == "th"
    sd = net.state_dict()
    want = [(str(k), tuple(int(v) for v in s if v)) for k, s in zip(g["keys"], g["shapes"])]
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want
    assert list(synth.convnextv2_param_shapes().items()) == want
    assert sd["stages.2.4.grn.gamma"].shape == (1, 1, 1, 1536) and not sd["stages.2.4.grn.gamma"].any() and not sd["stages.0.0.grn.beta"].any()
    assert not any(k.endswith(".gamma") and ".grn." not in k for k in sd)        # no layer scale in V2
    assert [sd[f"stages.2.{j}.dwconv.weight"].shape[2] for j in range(9)] == [1, 3, 1] * 3
    # _init_weights: trunc_normal(0.02) on every conv / linear weight, biases 0
    assert 0.015 < float(sd["stages.1.0.pwconv1.weight"].std()) < 0.025 and 0.015 < float(sd["head.weight"].std()) < 0.025
    assert not sd["stages.1.0.pwconv1.bias"].any() and not sd["head.bias"].any()
    r = net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_convnextv2_weights(3).items()}, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    with pytest.raises(ValueError, match="grn_over"):
        ConvNeXtV23D(depths=(1, 1, 1, 1), grn_over="hw")


def test_synth_convnextv2_draws():
    w = synth.synth_convnextv2_weights(5, "stress")
    g, b = w["stages.0.0.grn.gamma"], w["stages.3.1.grn.beta"]
    assert g.shape == (1, 1, 1, 384) and 0.5 <= np.abs(g).min() and np.abs(g).max() <= 1.5 and (g < 0).any() and (g > 0).any()
    assert b.shape == (1, 1, 1, 3072) and 0.1 < b.std() < 0.3
    wi = synth.synth_convnextv2_weights(5, "init")
    assert not wi["stages.2.0.grn.gamma"].any() and not wi["stages.2.0.grn.beta"].any()
    # new prefixes: the ConvNeXt-3D streams are untouched and differ from these
    assert not np.array_equal(w["stages.0.0.pwconv1.weight"], synth.synth_convnext_weights(5, "stress")["stages.0.0.pwconv1.weight"])


def test_inflate_weights_is_bit_equal_to_the_reference(golden, tmp_path):
    from kvq_amd.models.backbones.conv_backbone import ConvNeXtV23D
    g = golden("convnextv2.npz")
    net = ConvNeXtV23D(depths=INFLATE["depths"], dims=INFLATE["dims"], num_classes=INFLATE["num_classes"])
    src = synth.synth_convnextv2_2d_checkpoint(INFLATE["seed"], INFLATE["depths"], INFLATE["dims"], INFLATE["num_classes"])
    path = str(tmp_path / "convnextv2_2d.pt")
    torch.save({"model": {k: torch.from_numpy(v) for k, v in src.items()}}, path)
    net.inflate_weights(path)
    sd = net.state_dict()
    keys = [k[len("inflate/"):] for k in g.files if k.startswith("inflate/")]
    assert sorted(keys) == sorted(sd)
    for k in keys:
        assert np.array_equal(sd[k].numpy(), g["inflate/" + k]), k
    assert sd["stages.1.1.dwconv.weight"].shape == (16, 1, 3, 7, 7) and sd["stages.1.0.dwconv.weight"].shape == (16, 1, 1, 7, 7)
    assert np.array_equal(sd["stages.1.1.grn.gamma"].numpy(), src["stages.1.1.grn.gamma"]) and sd["head.weight"].shape == (10, 64)


def test_narrow_and_wide_factories_name_the_missing_widths():
    from kvq_amd.models.backbones import conv_backbone as cb
    for name, first in (("atto", 40), ("femto", 48), ("pico", 64), ("nano", 80), ("base", 128), ("large", 192)):
        with pytest.raises(NotImplementedError, match=rf"\({first}, "):
            getattr(cb, f"convnextv2_3d_{name}")()
    with pytest.raises(NotImplementedError, match="local"):
        cb.convnextv2_3d_tiny(pretrained=True)


def test_model_key_and_yml(tmp_path):
    from kvq_amd.models.model import VQA_Network
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "kwai_conv_v2_tiny_synthetic_test.yml")))
    assert cfg["model"]["type"] == "conv_v2_tiny" and cfg["model"]["args"]["conv_v2_tiny"]["backbone"] == {"pretrained": False, "grn_over": "th"}
    net = VQA_Network(cfg)
    assert net.key_names == ["conv_v2_tiny"]
    assert type(net.conv_v2_tiny_backbone).__name__ == "ConvNeXtV23D" and type(net.conv_v2_tiny_head).__name__ == "VQAHead"
    # a missing ``pretrained`` (or a missing backbone entry) means false: the reference's V2 factories never download
    for ok in ({"head": HEAD}, {"backbone": {}, "head": HEAD}, {"backbone": {"grn_over": "thw"}, "head": HEAD}):
        n = VQA_Network({"model": {"args": {"conv_v2_tiny": ok}}})
        assert n.conv_v2_tiny_backbone.grn_over == (ok.get("backbone") or {}).get("grn_over", "th")
    # a local 2D checkpoint is inflated on load
    src = synth.synth_convnextv2_2d_checkpoint(7)
    path = str(tmp_path / "convnextv2_tiny_2d.pt")
    torch.save({"model": {k: torch.from_numpy(v) for k, v in src.items()}}, path)
    net = VQA_Network({"model": {"args": {"conv_v2_tiny": {"backbone": {"pretrained": path}, "head": HEAD}}}})
    sd = net.conv_v2_tiny_backbone.state_dict()
    assert torch.equal(sd["stages.0.1.dwconv.weight"], torch.from_numpy(src["stages.0.1.dwconv.weight"]).unsqueeze(2).repeat(1, 1, 3, 1, 1) / 3)
    assert torch.equal(sd["stages.2.4.grn.gamma"], torch.from_numpy(src["stages.2.4.grn.gamma"]))
    assert torch.equal(sd["head.weight"], torch.from_numpy(src["head.weight"]))


def test_trainer_passes_the_aesthetic_view_for_the_key():
    src = open(os.path.join(ROOT, "kvq-challenge-cvpr-ntire2024_amd", "trainer.py")).read()
    assert re.search(r'views = \("technical", "aesthetic"\) if .*"conv_v2_tiny" in self\.key_list', src)


def test_forward_refuses_what_it_cannot_mirror():
    from kvq_amd.models.backbones.conv_backbone import ConvNeXtV23D
    net = ConvNeXtV23D(depths=(1, 1, 1, 1))
    x = torch.zeros(1, 3, 4, 32, 32)
    with pytest.raises(NotImplementedError, match="UnboundLocalError"):
        net({"aesthetic": x}, layer=1)
    with pytest.raises(_abi.KvqError, match="no CPU path"):
        net({"aesthetic": x})
    with pytest.raises(KeyError):
        net({"asesthetic": x})                    # this class reads batch['aesthetic'] only (conv_backbone.py:525)


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "kvq_hip.h")).read()
    lib = _abi.lib()
    for name in ("kvq_grn_supported", "kvq_grn_workspace_bytes", "kvq_grn_stats", "kvq_grn_apply"):
        assert re.search(r"\b%s\(" % name, header) and name in _abi.SYMBOLS
        assert getattr(lib, name) is not None
    assert lib.kvq_abi_version() == 32 and "#define KVQ_ABI_VERSION 32" in header
    assert C.sizeof(_abi.KvqGrnArgs) == 5 * 8 + 7 * 4 + 4


def test_grn_supported_answers_on_the_host():
    lib = _abi.lib()
    for N in (384, 768, 1536, 3072):
        assert lib.kvq_grn_supported(N, 16, 56, 56) == 1 and lib.kvq_grn_supported(N, 1, 1, 1) == 1
        assert lib.kvq_grn_workspace_bytes(1, 16, 7, 7, N) >= 4 * 2 * 7 * N           # scale[B][W][N] and at least one chunk of partials
    for N in (96, 512, 400, 4096, 0):
        assert lib.kvq_grn_supported(N, 16, 56, 56) == 0 and lib.kvq_grn_workspace_bytes(1, 16, 56, 56, N) == 0
    assert lib.kvq_grn_supported(384, 0, 4, 4) == 0 and lib.kvq_grn_supported(384, 4, 4, 0) == 0
    # NULL arguments and shapes outside the set are refused before any launch (no device needed)
    for fn in (lib.kvq_grn_stats, lib.kvq_grn_apply):
        assert fn(None, None) == -1
        a = _abi.KvqGrnArgs()
        assert fn(C.byref(a), None) == -1
        buf = (C.c_float * 64)()
        p = (C.addressof(buf) + 15) & ~15
        a.x = a.gamma = a.beta = a.ws = p                  # host memory: never dereferenced, the shape is refused first
        a.B, a.D, a.H, a.W, a.dtype = 1, 2, 4, 4, 1
        for N in (512, 96, 3080):
            a.N = N
            assert fn(C.byref(a), None) == -3 and b"unsupported shape" in lib.kvq_last_error()
        a.N, a.B = 384, 70000
        assert fn(C.byref(a), None) == -2                  # KVQ_ERR_SHAPE: past the grid
        a.B, a.dtype = 1, 5
        assert fn(C.byref(a), None) == -3
