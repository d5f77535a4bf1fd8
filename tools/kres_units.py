"""Register / scratch / occupancy table of named translation units, compiled exactly as the library compiles them
(_build.FLAGS + _build.EXTRA + the unit's own -D) with -Rpass-analysis=kernel-resource-usage; device code only, nothing is linked.
    python tools/kres_units.py tail.hip merge.hip [--filter SUBSTRING] [--csrc DIR]
--csrc compiles the same unit names from another source directory (e.g. a checkout of the parent commit) with this tree's flags."""
import argparse
import importlib.util
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kres  # noqa: E402


def _build_module():
    spec = importlib.util.spec_from_file_location("_kvq_build", os.path.join(ROOT, "kvq-challenge-cvpr-ntire2024_amd", "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def unit_rows(names, sub="", csrc=None):
    """{unit: [(kernel, vgpr, agpr, scratch, occupancy)]} for the units whose source file name is in `names`"""
    b = _build_module()
    cc = b._hipcc()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for src, oname, uflags in b.units():
            base = os.path.basename(src)
            if base not in names:
                continue
            if csrc:
                src = os.path.join(csrc, base)
            cmd = ([cc] + b.FLAGS + b.EXTRA.get(base, []) + uflags + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
                   + (["-x", "hip"] if src.endswith(".cpp") else []) + ["-c", src, "-o", os.path.join(tmp, oname)])
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"hipcc failed on {src}:\n{r.stderr[-4000:]}")
            out.setdefault(base, []).extend(kres.rows(r.stderr, sub))
    missing = [n for n in names if n not in out]
    if missing:
        raise SystemExit(f"not a unit of the library: {missing}")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("units", nargs="+")
    ap.add_argument("--filter", default="")
    ap.add_argument("--csrc", default=None)
    a = ap.parse_args()
    for unit, rs in unit_rows(a.units, a.filter, a.csrc).items():
        print(f"# {unit}")
        for r in sorted(rs):
            print(kres.line(r))
