"""Emit tests/golden/prepared_weights.json: one sha256 per kernel-ready tensor the model mirrors prepare (tests/prepared_ref.py
says which, and from which inputs).  The committed file was written from the commit BEFORE the weight preparation moved into
``_prepared.py``, so tests/test_prepared_weights_cpu.py pins the shared helpers to the bytes the per-model copies produced.
Needs no reference checkout and no GPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_prepared_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import prepared_ref  # noqa: E402


def main():
    d = prepared_ref.collect()
    path = os.path.join(HERE, "prepared_weights.json")
    with open(path, "w") as f:
        json.dump(d, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote prepared_weights.json: {os.path.getsize(path) / 1024:.1f} KiB, {len(d)} digests")


if __name__ == "__main__":
    main()
