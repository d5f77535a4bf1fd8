"""Device code of two trees, per kernel symbol, without a GPU (the table of profiles/launch_refactor_isa.txt):

    python tools/isa_compare.py dump <tree root> <out dir>       every unit of the tree's _build.units(), compiled with its own flags plus
                                                                 --cuda-device-only -S -Rpass-analysis=kernel-resource-usage
    python tools/isa_compare.py diff <out dir A> <out dir B>     kernel symbol sets, and each kernel's text from its label to the end of its descriptor

Ignored: comment lines and trailing remarks, .file / .loc / .ident, __hip_cuid_*, and the function's ordinal in its local labels (.LBB<n>_k ...)."""
import importlib.util
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

SKIP = re.compile(r"^\s*(;|//|\.file\b|\.loc\b|\.ident\b)")
LOCAL = re.compile(r"\.L(BB|func_begin|func_end|JTI|CPI|tmp)\d+")
RES = re.compile(r"Function Name: (\S+).*?SGPRs: (\d+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", re.S)


def dump(root, out):
    os.makedirs(out, exist_ok=True)
    spec = importlib.util.spec_from_file_location("_b", os.path.join(root, "kvq-challenge-cvpr-ntire2024_amd", "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)

    def one(u):
        src, oname, uflags = u
        base = oname[:-2]
        cmd = ([b._hipcc()] + b.FLAGS + b.EXTRA.get(os.path.basename(src), []) + uflags + (["-x", "hip"] if src.endswith(".cpp") else [])
               + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", os.path.join(out, base + ".s")])
        r = subprocess.run(cmd, capture_output=True, text=True)
        open(os.path.join(out, base + ".res"), "w").write(r.stderr)
        return base, r.returncode

    with ThreadPoolExecutor(max_workers=8) as ex:
        for base, rc in ex.map(one, b.units()):
            print(base, "ok" if rc == 0 else f"FAILED ({rc})", flush=True)


def norm(path):
    out = []
    for ln in open(path):
        if SKIP.match(ln) or "__hip_cuid_" in ln:
            continue
        ln = LOCAL.sub(r".L\1#", ln.split(" ; ")[0].rstrip())
        if ln:
            out.append(ln)
    return out


def kernels(lines):
    """symbol -> its text: from the symbol's label to the end of its .amdhsa_kernel descriptor"""
    out = {}
    for n in [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]:
        s, e = lines.index(n + ":"), lines.index("\t.amdhsa_kernel " + n)
        while not lines[e].strip().startswith(".end_amdhsa_kernel"):
            e += 1
        out[n] = lines[s:e + 1]
    return out


def instr(text):
    return sum(1 for ln in text if re.match(r"^\t[a-z]\w+", ln))


def res(path):
    return {m.group(1): m.groups()[1:] for m in RES.finditer(open(path).read())}


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: d.replace("void kvq::", "").replace("kvq::", "") for n, d in zip(names, r)}


def diff(A, B):
    units = sorted(f[:-2] for f in os.listdir(A) if f.endswith(".s"))
    assert units == sorted(f[:-2] for f in os.listdir(B) if f.endswith(".s")), "the two trees have different units"
    rows, whole, n_id, n_k = [], [], 0, 0
    for u in units:
        la, lb = norm(os.path.join(A, u + ".s")), norm(os.path.join(B, u + ".s"))
        ka, kb = kernels(la), kernels(lb)
        assert set(ka) == set(kb), (u, set(ka) ^ set(kb))
        ra, rb = res(os.path.join(A, u + ".res")), res(os.path.join(B, u + ".res"))
        dm = demangle(sorted(ka))
        same = sum(ka[n] == kb[n] for n in ka)
        n_id += same
        n_k += len(ka)
        whole.append((u, len(ka), same, sorted(la) == sorted(lb)))
        for n in sorted(ka, key=lambda n: dm[n]):
            x, y = ra.get(n, ("?",) * 5), rb.get(n, ("?",) * 5)
            cols = "  ".join(f"{p:>4s}/{q:<4s}" for p, q in zip((x[1], x[2], x[0], x[3], x[4]), (y[1], y[2], y[0], y[3], y[4])))
            rows.append(f"{u.replace('.hip', ''):11s} {'identical' if ka[n] == kb[n] else 'DIFFERENT':9s} {instr(ka[n]):6d}/{instr(kb[n]):<6d} {cols}  {dm[n][:150]}")
    print("unit        verdict     instr old/new     VGPR       AGPR       SGPR     scratch      occ     kernel")
    print("\n".join(rows))
    print("\nunit            kernels  identical  rest")
    for u, k, s, w in whole:
        print(f"{u:15s} {k:7d} {s:10d}  {'equal' if w else 'DIFFERENT'}")
    print(f"\nTotals: {n_k} kernels in {len(units)} units, {n_id} identical, {n_k - n_id} different; kernel symbol sets equal in every unit.")
    return 0 if n_id == n_k else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
