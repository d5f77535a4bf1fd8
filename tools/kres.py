"""Per-kernel register / spill / occupancy table from `hipcc -Rpass-analysis=kernel-resource-usage` output:
    hipcc ... -Rpass-analysis=kernel-resource-usage -c x.hip -o x.o 2> res.txt; python tools/kres.py res.txt [substring]
(tools/kres_units.py compiles named units of the library with their own flags and prints this table)"""
import re
import subprocess
import sys

PAT = re.compile(r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", re.S)


def rows(text, sub=""):
    """[(kernel name, vgpr, agpr, scratch bytes per lane, waves per SIMD)] of the remarks in `text`, names demangled and cut at the '('"""
    found = [(m.group(1),) + tuple(int(m.group(k)) for k in range(2, 6)) for m in PAT.finditer(text)]
    if not found:
        return []
    names = subprocess.run(["c++filt"], input="\n".join(f[0] for f in found), capture_output=True, text=True).stdout.splitlines()
    out = []
    for name, f in zip(names, found):
        name = name.strip().replace("void kvq::", "").split("(")[0]
        if sub in name:
            out.append((name,) + f[1:])
    return out


def line(r):
    return f"{r[0][:100]:100s} vgpr {r[1]:>4d} agpr {r[2]:>4d} scratch {r[3]:>5d} occ {r[4]}"


if __name__ == "__main__":
    for r in rows(open(sys.argv[1]).read(), sys.argv[2] if len(sys.argv) > 2 else ""):
        print(line(r))
