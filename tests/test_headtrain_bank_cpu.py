"""Feature bank of head fine-tuning, everything that needs no GPU: the new ABI symbols and structs, every host-side refusal of the
store, the gather and the four bank entries, the wrapper's check of a CPU index, ``set_draw``, the train-phase crop offsets, the
``feature_bank`` yml key and the two new configs."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import kvq_amd  # noqa: F401
from kvq_amd import _abi, kernels
from kvq_amd.datasets import fusion_datasets as fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["kvq_feature_bank_store", "kvq_feature_bank_rows", "kvq_headtrain_bank_forward", "kvq_headtrain_bank_backward",
       "kvq_simple_headtrain_bank_forward", "kvq_simple_headtrain_bank_backward"]
GONE = ["kvq_headtrain_forward", "kvq_headtrain_backward", "kvq_simple_headtrain_forward", "kvq_simple_headtrain_backward"]
NULL, SHAPE, UNSUPPORTED, WORKSPACE = -1, -2, -3, -4

_HOST = (C.c_char * 4112)()
P = C.c_void_p((C.addressof(_HOST) + 15) & ~15)      # one 16-byte aligned host buffer stands for every pointer: nothing is launched


def test_symbols_declared_bound_and_sized():
    header = open(os.path.join(ROOT, "include", "kvq_hip.h")).read()
    declared = set(re.findall(r"\b(kvq_[a-z0-9_]+)\s*\(", header))
    handle = _abi.lib()
    for name in NEW:
        assert name in declared and name in _abi.SYMBOLS and hasattr(handle, name), name
    assert "typedef struct KvqFeatureBank {" in header and "typedef struct KvqHeadTrainBankArgs {" in header
    exported = subprocess.run(["nm", "-D", "--defined-only", handle._name], capture_output=True, text=True, check=True).stdout.split()
    for name in GONE:                              # the dense entries of ABI 31 and their struct are gone from every layer
        assert name not in declared and name not in _abi.SYMBOLS and name not in exported and not hasattr(handle, name), name
    assert set(re.findall(r"KvqHeadTrain\w*", header)) == {"KvqHeadTrainBankArgs"}      # one args struct, in the header and in _abi
    assert [n for n in dir(_abi) if n.startswith("KvqHeadTrain")] == ["KvqHeadTrainBankArgs"]
    assert set(NEW) <= set(exported)
    assert handle.kvq_abi_version() == _abi.ABI_VERSION == 32
    # {void*, int32 x 3, (pad), int64}; the bank, the index pointer, int32 x 4, params, float + uint32 x 2 (+ pad), five 8-byte fields
    assert C.sizeof(_abi.KvqFeatureBank) == 32
    assert C.sizeof(_abi.KvqHeadTrainBankArgs) == 32 + 8 + 16 + 8 + 16 + 5 * 8 == 120
    assert (_abi.DT_BF16, _abi.DT_FP16, _abi.DT_FP32) == (0, 1, 2) and "KVQ_DT_FP32 = 2" in header
    assert _abi.bank_dtype_code(torch.float32) == 2 and _abi.bank_dtype_code("bf16") == 0 and _abi.bank_dtype_code(torch.float16) == 1
    with pytest.raises(ValueError, match="fp32, fp16 or bf16"):
        _abi.bank_dtype_code(torch.float64)
    for f in ("featbank.hip", "featbank.hpp"):
        src = open(os.path.join(ROOT, "kvq-challenge-cvpr-ntire2024_amd", "csrc", f)).read()
        assert "getenv" not in src and "atomic" not in src


def _bank(**kw):
    b = _abi.KvqFeatureBank(P, _abi.DT_BF16, 18, 768, 7)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def test_store_and_gather_refuse_on_the_host():
    h = _abi.lib()
    st, rows = h.kvq_feature_bank_store, h.kvq_feature_bank_rows
    L, Cc = 18, 768
    ok = dict(feat=P, n=2, sn=L * Cc, sl=Cc, bank=_bank(), first=3, flag=P)

    def store(**kw):
        a = dict(ok, **kw)
        return st(a["feat"], a["n"], a["sn"], a["sl"], None if a["bank"] is None else C.byref(a["bank"]), a["first"], a["flag"], None)

    assert store(feat=None) == NULL and b"NULL" in h.kvq_last_error()
    assert store(bank=None) == NULL and store(bank=_bank(rows=None)) == NULL
    assert store(bank=_bank(dtype=3)) == UNSUPPORTED and b"dtype 3" in h.kvq_last_error()
    assert store(bank=_bank(dtype=-1)) == UNSUPPORTED
    assert store(bank=_bank(rows=C.c_void_p(P.value + 8))) == UNSUPPORTED and b"aligned" in h.kvq_last_error()
    assert store(bank=_bank(C=770)) == UNSUPPORTED
    assert store(bank=_bank(n_rows=0)) == SHAPE and store(bank=_bank(L=0)) == SHAPE
    assert store(first=6) == SHAPE and b"bank of 7" in h.kvq_last_error()          # rows 6, 7 of 7
    assert store(first=-1) == SHAPE and store(n=0) == SHAPE and store(n=8, first=0) == SHAPE
    assert store(first=2 ** 62, n=2 ** 62) == SHAPE                                 # no overflow in first_row + n
    assert store(feat=C.c_void_p(P.value + 4)) == UNSUPPORTED
    assert store(sl=Cc + 2) == UNSUPPORTED and store(sn=L * Cc + 1) == UNSUPPORTED
    assert store(flag=C.c_void_p(P.value + 2)) == UNSUPPORTED
    assert store(sl=Cc - 4) == SHAPE and b"token stride" in h.kvq_last_error()

    def gather(bank=_bank(), index=P, B=3, out=P):
        return rows(None if bank is None else C.byref(bank), index, B, out, None)

    assert gather(bank=None) == NULL and gather(index=None) == NULL and gather(out=None) == NULL and gather(bank=_bank(rows=None)) == NULL
    assert gather(bank=_bank(dtype=5)) == UNSUPPORTED and gather(bank=_bank(n_rows=0)) == SHAPE
    assert gather(out=C.c_void_p(P.value + 8)) == UNSUPPORTED and gather(index=C.c_void_p(P.value + 2)) == UNSUPPORTED
    assert gather(B=0) == SHAPE and gather(B=2 ** 40) == SHAPE


@pytest.mark.parametrize("head", ["vqa", "simple"])
def test_bank_entries_refuse_on_the_host(head):
    """every refusal of the dense entry (tests/test_headtrain_cpu.py, test_simple_headtrain_cpu.py) with the same status, and the bank's own"""
    h = _abi.lib()
    hidden = 64 if head == "vqa" else 128
    fwd, bwd = ((h.kvq_headtrain_bank_forward, h.kvq_headtrain_bank_backward) if head == "vqa"
                else (h.kvq_simple_headtrain_bank_forward, h.kvq_simple_headtrain_bank_backward))

    def args(bank=None, **kw):
        a = _abi.KvqHeadTrainBankArgs()
        base = dict(index=P, B=4, L=18, C=768, hidden=hidden, params=P, p_drop=0.5 if head == "vqa" else 0.0, seed=1, step=0, workspace=P,
                    workspace_bytes=1 << 30, score=P, dscore=P, grads=P)
        base.update(kw)
        a.bank = _bank(**dict(dict(L=base["L"], C=base["C"]), **(bank or {})))
        for k, v in base.items():
            setattr(a, k, v)
        return a

    for fn in (fwd, bwd):
        assert fn(None, None) == NULL and b"NULL" in h.kvq_last_error()
        assert fn(C.byref(args(index=None)), None) == NULL
        assert fn(C.byref(args(bank=dict(rows=None))), None) == NULL
        assert fn(C.byref(args(params=None)), None) == NULL and fn(C.byref(args(workspace=None)), None) == NULL
        assert fn(C.byref(args(bank=dict(dtype=3))), None) == UNSUPPORTED and b"dtype 3" in h.kvq_last_error()
        for dt in (_abi.DT_FP32, _abi.DT_FP16, _abi.DT_BF16):                      # every dtype code reaches the shared checks
            assert fn(C.byref(args(bank=dict(dtype=dt), workspace_bytes=1024)), None) == WORKSPACE
        assert fn(C.byref(args(bank=dict(rows=C.c_void_p(P.value + 8)))), None) == UNSUPPORTED and b"aligned" in h.kvq_last_error()
        assert fn(C.byref(args(index=C.c_void_p(P.value + 2))), None) == UNSUPPORTED and b"index" in h.kvq_last_error()
        assert fn(C.byref(args(params=C.c_void_p(P.value + 4))), None) == UNSUPPORTED
        assert fn(C.byref(args(bank=dict(n_rows=0))), None) == SHAPE
        assert fn(C.byref(args(bank=dict(L=49))), None) == SHAPE and b"L 49" in h.kvq_last_error()
        assert fn(C.byref(args(bank=dict(C=704))), None) == SHAPE
        assert fn(C.byref(args(hidden=32)), None) == UNSUPPORTED and b"hidden 32" in h.kvq_last_error()
        assert fn(C.byref(args(C=100)), None) == UNSUPPORTED and b"multiple of 64" in h.kvq_last_error()
        assert fn(C.byref(args(B=1)), None) == SHAPE and fn(C.byref(args(L=0)), None) == SHAPE
        assert fn(C.byref(args(B=1024, L=8192, C=768)), None) == SHAPE and b"32-bit" in h.kvq_last_error()
        assert fn(C.byref(args(workspace_bytes=1024)), None) == WORKSPACE
        if head == "vqa":
            assert fn(C.byref(args(p_drop=1.0)), None) == UNSUPPORTED
        else:
            assert fn(C.byref(args(p_drop=0.5)), None) == UNSUPPORTED and fn(C.byref(args(B=1025)), None) == SHAPE
    assert fwd(C.byref(args(score=None)), None) == NULL
    assert bwd(C.byref(args(dscore=None)), None) == NULL and bwd(C.byref(args(grads=None)), None) == NULL
    assert bwd(C.byref(args(grads=C.c_void_p(P.value + 4))), None) == UNSUPPORTED and b"grads" in h.kvq_last_error()


def test_wrapper_checks_a_cpu_index_and_names_the_value():
    bank = kernels.FeatureBank.of(torch.zeros(7, 18, 128, dtype=torch.bfloat16))
    assert (bank.n_rows, bank.L, bank.C, bank.view.dtype, bank.nbytes) == (7, 18, 128, _abi.DT_BF16, 7 * 18 * 128 * 2)
    idx = kernels.bank_index(torch.tensor([6, 0, 6]), bank)
    assert idx.dtype == torch.int32 and idx.tolist() == [6, 0, 6]
    prm = torch.zeros(kernels.headtrain_param_count(128))
    for bad, shown in ((torch.tensor([0, 7, 1]), r"index\[1\] = 7"), (torch.tensor([-1, 2]), r"index\[0\] = -1"), ([3, 4, 2 ** 31], "2147483648")):
        with pytest.raises(ValueError, match=shown):
            kernels.bank_index(bad, bank)
        with pytest.raises(ValueError, match=shown):             # before anything asks for a device
            kernels.headtrain_bank_forward(bank, bad, prm, 0.5, 1, 0, torch.zeros(16))
        with pytest.raises(ValueError, match=shown):
            kernels.feature_bank_rows(bank, bad)
    with pytest.raises(_abi.KvqError, match="HIP device"):        # a valid index goes on to the launch, which needs the GPU
        kernels.feature_bank_rows(bank, torch.tensor([1, 2]))
    assert kernels.FeatureBank.of(torch.zeros(2, 4, 64)).view.dtype == _abi.DT_FP32
    assert kernels.FeatureBank.of(torch.zeros(2, 4, 64, dtype=torch.float16)).view.dtype == _abi.DT_FP16


# ---- datasets -----------------------------------------------------------------------------------------------------------------------
KVQ_OPT = dict(num_videos=3, frames=96, height=64, width=64, seed_per_item=True,
               sample_types={"technical": dict(fragments_h=2, fragments_w=2, fsize_h=8, fsize_w=8, aligned=8, clip_len=32, frame_interval=1,
                                               num_clips=2)})


def _frame_inds(ds, i, monkeypatch):
    monkeypatch.setattr(fd, "get_spatial_fragments", lambda clip, *a, **k: None)   # the host half only: the view is the GPU's
    return ds[i]["frame_inds"]


def test_set_draw_moves_the_seed_of_every_item(monkeypatch):
    ds = fd.SyntheticKVQDataset(dict(KVQ_OPT), device="cpu")
    sampler = fd.UnifiedFrameSampler(32, 2, 1)
    for i in range(3):
        np.random.seed(1234 + i)                       # today's item: its seed is 1234 + i
        today = sampler(96)
        assert np.array_equal(_frame_inds(ds, i, monkeypatch), today)
        ds.set_draw(1)
        one = _frame_inds(ds, i, monkeypatch)
        np.random.seed(1234 + i + 1000003)
        assert np.array_equal(one, sampler(96)) and not np.array_equal(one, today)
        other = fd.SyntheticKVQDataset(dict(KVQ_OPT), device="cpu")
        other.set_draw(1)
        assert np.array_equal(_frame_inds(other, i, monkeypatch), one)            # two constructions agree
        ds.set_draw(0)
        assert np.array_equal(_frame_inds(ds, i, monkeypatch), today)
    assert fd._item_seed(5, 0) == 1239 and fd._item_seed(5, 2) == 1239 + 2000006
    for cls in (fd.SyntheticSimpleVQADataset, fd.ViewDecompositionDataset_KVQ, fd.ViewDecompositionDataset_add_forSimpleVQA):
        assert callable(getattr(cls, "set_draw"))


@pytest.mark.parametrize("seed,resize,crop", [(0, 520, 448), (7, 260, 224), (123, 130, 112), (5, 9, 8)])
def test_train_crop_offsets_are_the_references_draws(seed, resize, crop):
    random.seed(seed)
    want = (random.randrange(resize - crop), random.randrange(resize - crop))      # rnd_h, then rnd_w
    random.seed(seed)
    assert fd.train_crop_offsets(resize, crop) == want
    assert 0 <= want[0] <= resize - crop - 1 and 0 <= want[1] <= resize - crop - 1


def test_train_crop_refuses_an_empty_range_as_the_reference_does():
    with pytest.raises(ValueError):
        random.randrange(0)
    with pytest.raises(ValueError, match="empty range"):
        fd.train_crop_offsets(448, 448)
    with pytest.raises(ValueError, match="empty range"):              # in front of anything that touches the frames
        fd.get_resizecrop_video(torch.zeros(3, 2, 16, 16), resize=8, crop=8, phase="train")


def test_train_phase_is_accepted_without_augment(capsys):
    st = {"simpleVQA": dict(resize=130, crop=112, clip_len=8, frame_interval=10, t_frag=8, num_clips=1)}
    infos = [dict(filename="a.y4m", label=1.0, video_name="a.y4m")]
    opt = dict(anno_file=infos, data_prefix=".", data_prefix_3D=".", feature_type="SlowFast", sample_types=st)
    ds = fd.ViewDecompositionDataset_add_forSimpleVQA(dict(opt, phase="train"), device="cpu")
    assert ds.phase == "train" and ds.draw == 0
    ds.set_draw(3)
    assert ds.draw == 3
    kt = {"technical": dict(fragments_h=7, fragments_w=7, fsize_h=32, fsize_w=32, aligned=8, clip_len=32, frame_interval=1, num_clips=2)}
    # the KVQ class keeps refusing 'train' (tests/test_host_cpu.py pins that): the reference's train phase draws its views exactly as
    # the test phase does, so phase 'test' with set_draw(k) gives the same draws
    with pytest.raises(NotImplementedError, match=r"set_draw\(k\)"):
        fd.ViewDecompositionDataset_KVQ(dict(anno_file=[dict(infos[0], dis_label=0, cls_label=0)], data_prefix=".", phase="train",
                                             sample_types=kt), device="cpu")
    kv = fd.ViewDecompositionDataset_KVQ(dict(anno_file=[dict(infos[0], dis_label=0, cls_label=0)], data_prefix=".", phase="test",
                                              sample_types=kt), device="cpu")
    kv.set_draw(2)
    assert kv.phase == "test" and kv.draw == 2
    for cls, o in ((fd.ViewDecompositionDataset_add_forSimpleVQA, dict(opt, phase="train", augment=True)),
                   (fd.ViewDecompositionDataset_KVQ, dict(anno_file=[], data_prefix=".", phase="test", sample_types=kt, augment=True))):
        with pytest.raises(NotImplementedError, match="augment"):
            cls(o, device="cpu")
    with pytest.raises(NotImplementedError, match="RandomResizedCrop"):
        fd.get_resized_video(torch.zeros(3, 2, 16, 16), random_crop=True)


# ---- yml ----------------------------------------------------------------------------------------------------------------------------
def test_feature_bank_key_is_validated():
    from kvq_amd.finetune import feature_bank_options as opt
    assert opt({}) == (1, torch.float32) and opt({"feature_bank": None}) == (1, torch.float32)
    assert opt({"feature_bank": {}}) == (1, torch.float32)
    assert opt({"feature_bank": {"draws": 4, "dtype": "bf16"}}) == (4, torch.bfloat16)
    assert opt({"feature_bank": {"dtype": "fp16"}}) == (1, torch.float16) and opt({"feature_bank": {"draws": 2}}) == (2, torch.float32)
    for bad, shown in (({"draw": 2}, "'draw'"), ({"draws": 0}, "draws"), ({"draws": 1.5}, "1.5"), ({"draws": True}, "True"),
                       ({"dtype": "fp8"}, "'fp8'"), ({"dtype": "float16"}, "'float16'"), ({"draws": 2, "spill": "host"}, "'spill'"),
                       ("bf16", "mapping")):
        with pytest.raises(ValueError, match=shown):
            opt({"feature_bank": bad})


@pytest.mark.parametrize("yml,parent,draws,dtype,name", [
    ("kwai_swin_grpb_synthetic_bank_finetune.yml", "kwai_swin_grpb_synthetic_finetune.yml", 2, torch.bfloat16, "swin_tiny_grpb_synthetic_bank"),
    ("kwai_simpleVQA_synthetic_bank_finetune.yml", "kwai_simpleVQA_synthetic_finetune.yml", 2, torch.float16, "simpleVQA_synthetic_bank")])
def test_the_bank_ymls_are_their_parents_plus_the_bank(yml, parent, draws, dtype, name):
    from kvq_amd.finetune import feature_bank_options
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", yml)))
    base = yaml.safe_load(open(os.path.join(ROOT, "config", parent)))
    assert "feature_bank" not in base and feature_bank_options(base) == (1, torch.float32)
    assert feature_bank_options(cfg) == (draws, dtype) and cfg["num_epochs"] == 2 and cfg["name"] == name
    assert cfg["data"]["train"]["args"]["phase"] == "train" and cfg["data"]["val"]["args"]["phase"] == "test"
    assert cfg["data"]["train"]["args"].get("seed_per_item") is True
    for k in ("model", "optimizer", "batch_size", "warmup_epochs", "l_num_epochs", "ema"):
        assert cfg[k] == base[k], k
    assert cfg["data"]["val"] == base["data"]["val"]
    assert cfg["data"]["train"]["args"]["sample_types"] == base["data"]["train"]["args"]["sample_types"]


# ---- the compiler's own resource remarks (tools/kres_units.py: the library's flags, device code only, no GPU) --------------------------
# vgpr + agpr and waves per SIMD of commit acb37f7, the last with a dense (float, no index) form of the four step kernels, by
# tools/kres_units.py.  DENSE: that form, the bound of every instantiation; PARENT: the indexed instantiation of each element type.
DENSE = {"headtrain_fwd_kernel": (80, 6), "headtrain_bwd_w1_kernel": (184, 2), "simple_fwd_rows_kernel": (39, 8), "simple_bwd_g_kernel": (57, 8)}
PARENT = {"headtrain_fwd_kernel": {"fp32": (80, 6), "fp16": (80, 6), "bf16": (80, 6)},
          "headtrain_bwd_w1_kernel": {"fp32": (184, 2), "fp16": (184, 2), "bf16": (184, 2)},
          "simple_fwd_rows_kernel": {"fp32": (39, 8), "fp16": (38, 8), "bf16": (38, 8)},
          "simple_bwd_g_kernel": {"fp32": (48, 8), "fp16": (46, 8), "bf16": (46, 8)}}


def _elem(name):
    """the element type of an instantiation from its (where c++filt knows the type, demangled) name"""
    return "fp32" if "<float>" in name else "bf16" if "IDF16bE" in name else "fp16" if "IDF16_E" in name else name


@pytest.mark.slow
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_no_instantiation_uses_scratch_and_none_outgrows_its_dense_form():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kres_units
    rows = kres_units.unit_rows(["headtrain.hip", "simple_headtrain.hip", "featbank.hip"])
    seen = {}
    for unit in rows.values():
        for name, vgpr, agpr, scratch, occ in unit:
            print(name, vgpr, agpr, scratch, occ)
            assert scratch == 0, name
            for stem in list(DENSE) + ["feature_bank_store_kernel", "feature_bank_rows_kernel"]:
                if stem in name:
                    seen.setdefault(stem, {})[_elem(name)] = (vgpr + agpr, occ)
    # float | _Float16 | __bf16 of the four step kernels and of the bank's own two
    assert {k: sorted(v) for k, v in seen.items()} == {k: ["bf16", "fp16", "fp32"] for k in list(DENSE) + ["feature_bank_store_kernel",
                                                                                                        "feature_bank_rows_kernel"]}
    for stem, dense in DENSE.items():
        for elem, (regs, occ) in seen[stem].items():
            assert regs <= dense[0] and occ >= dense[1], (stem, elem, regs, occ, dense)
            assert (regs, occ) == PARENT[stem][elem], (stem, elem, regs, occ, PARENT[stem][elem])     # no template parameter moved codegen
