"""Range guard of the fp16 residual stream, host side: the C entry points, the plan cache key, the yml key and the Trainer's choice
of what to score again (a stub model: no GPU)."""
import os
import re
import types

import numpy as np
import pytest
import torch

import kvq_amd  # noqa: F401
from kvq_amd import _abi, _build
from kvq_amd.models.backbones import swin_backbone as sb
from kvq_amd.trainer import Trainer

NEW = ("kvq_swin3d_set_range_flags", "kvq_swin3d_plan_set_resid16")


def test_entry_points_are_declared_and_exported():
    header = open(_build.HEADER).read()
    declared = set(re.findall(r"\b(kvq_[a-z0-9_]+)\s*\(", header))
    handle = _abi.lib()
    for name in NEW:
        assert name in declared and name in _abi.SYMBOLS
        assert hasattr(handle, name)
    assert handle.kvq_abi_version() == 32
    # NULL plan: an error code, never a crash
    assert handle.kvq_swin3d_set_range_flags(None, None) != 0
    assert handle.kvq_swin3d_plan_set_resid16(None, 0) != 0


class _FakeLib:
    """records the plan calls of SwinTransformer3D._plan; every call succeeds"""

    def __init__(self):
        self.calls = []
        self.n = 0

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "kvq_swin3d_plan_create":
                self.n += 1
                args[-1]._obj.value = 0x1000 * self.n
            return 64 if name == "kvq_swin3d_workspace_bytes" else 0
        return fn


def test_residual16_is_part_of_the_plan_cache_key(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(sb, "lib", lambda: fake)
    monkeypatch.setattr(sb, "current_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(device=torch.device("cpu"), cuda_stream=0))
    m = sb.SwinTransformer3D()
    assert m.residual16 is True
    a = m._plan(1, 16, 64, 64, "cpu")
    assert m._plan(1, 16, 64, 64, "cpu") is a
    m.residual16 = False
    b = m._plan(1, 16, 64, 64, "cpu")
    assert b is not a and m._plan(1, 16, 64, 64, "cpu") is b
    m.residual16 = True
    assert m._plan(1, 16, 64, 64, "cpu") is a
    names = [c[0] for c in fake.calls]
    assert names.count("kvq_swin3d_plan_create") == 2
    assert names.count("kvq_swin3d_set_range_flags") == 2                 # every plan gets the stream's word
    off = [c[1] for c in fake.calls if c[0] == "kvq_swin3d_plan_set_resid16"]
    assert len(off) == 1 and off[0][1] == 0                             # only the residual16 = False plan
    word = m.range_flags()
    assert word.dtype == torch.int32 and word.numel() == 1 and int(word) == 0
    assert all(c[1][1] == word.data_ptr() for c in fake.calls if c[0] == "kvq_swin3d_set_range_flags")


def _bare_trainer(config):
    t = Trainer.__new__(Trainer)
    t.config = config
    return t


@pytest.mark.parametrize("value,on", [(None, True), (True, True), (False, False), ("false", False), ("off", False), ("true", True)])
def test_range_guard_yml_key(value, on):
    cfg = {} if value is None else {"range_guard": value}
    assert _bare_trainer(cfg)._range_guard() is on


def test_config_files_parse_with_the_default_on():
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for f in os.listdir(os.path.join(root, "config")):
        cfg = yaml.safe_load(open(os.path.join(root, "config", f)))
        assert _bare_trainer(cfg)._range_guard() is True


def test_rescore_picks_exactly_the_flagged_videos(capsys):
    flags = np.array([0, 1, 0, 4, 0, 0, 5, 0], np.int32)
    assert Trainer.rescore_indices(flags) == [1, 3, 6]
    assert Trainer.rescore_indices(np.zeros(5, np.int32)) == []

    class Stub:
        residual16 = True
    swins = [Stub(), Stub()]
    seen = []
    t = _bare_trainer({})
    t.val_dataset = [f"item{i}" for i in range(20)]
    t._model_inputs = lambda item: item

    def run(inputs):
        assert all(s.residual16 is False for s in swins)
        seen.append(inputs)
        return torch.tensor([[100.0 + len(seen)]])
    t._run_model = run
    mine = list(range(0, 16, 2))                     # this shard's videos
    local = torch.arange(8, dtype=torch.float32)
    t._rescore_flagged(swins, flags, mine, local)
    assert seen == ["item2", "item6", "item12"]
    assert local.tolist() == [0.0, 101.0, 2.0, 102.0, 4.0, 5.0, 103.0, 7.0]
    assert all(s.residual16 is True for s in swins)
    err = capsys.readouterr().err
    assert "3 video(s) re-scored" in err and "stage(s) 0,2" in err
    # nothing flagged: nothing runs, nothing printed
    t._rescore_flagged(swins, np.zeros(8, np.int32), mine, local)
    assert len(seen) == 3 and capsys.readouterr().err == ""
