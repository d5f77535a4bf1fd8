"""CPU: KVQ_LATENCY is read once per process (csrc/common.cpp: latency_mode) and only the value 1 turns the mode on.  Seen from host
entry points: in the mode the C = 768 fused tail is refused (stage 3 runs as a GEMM chain) while C = 384 keeps its tail (the HC = 256
form).  tests/test_gpu_latency_mode.py runs the kernels the mode selects; its child makes the same three calls first."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _probe(value):
    env = {k: v for k, v in os.environ.items() if k != "KVQ_LATENCY"}
    env["PYTHONPATH"] = ROOT
    if value is not None:
        env["KVQ_LATENCY"] = value
    code = ("import json; import kvq_amd; from kvq_amd import _abi; h = _abi.lib(); "
            "print(json.dumps([int(h.kvq_block_tail_supported(768, 3072)), int(h.kvq_block_tail_supported(384, 1536)), "
            "int(h.kvq_block_tail_pack_bytes(768, 3072))]))")
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("value,on", [(None, False), ("0", False), ("1", True)], ids=["unset", "0", "1"])
def test_latency_switch_as_host_entry_points_see_it(value, on):
    s768, s384, bytes768 = _probe(value)
    if on:
        assert (s768, s384, bytes768) == (0, 1, 0)
    else:
        assert (s768, s384) == (1, 1) and bytes768 > 0
