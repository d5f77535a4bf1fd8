"""Runs tests/latency_cases.py in THIS interpreter and saves what the cases compute:  python latency_mode_child.py OUTDIR

tests/test_gpu_latency_mode.py starts it once per session with KVQ_LATENCY=1 (the library reads the switch once per process, so the
mode can only be entered by a fresh one).  No comparison happens here.  The first thing it does is prove the mode from host entry
points (OUTDIR/mode.json); then the cases run in the list's order, each writing OUTDIR/<case>.npz | .txt | .json and, once the device
has synchronised, its name into OUTDIR/manifest.txt.  The first exception ends the run with a non-zero exit status: nothing is
launched after a failure."""
import json
import os
import sys
import time


def main(outdir):
    import torch

    import latency_cases as LC
    probe = LC.mode_probe()
    with open(os.path.join(outdir, "mode.json"), "w") as f:
        json.dump(probe, f)
    if probe != [0, 1, 0]:
        raise SystemExit(f"not in latency mode: {LC.MODE_PROBES} -> {probe} (KVQ_LATENCY={os.environ.get('KVQ_LATENCY')!r})")
    t_start = time.time()
    for case in LC.all_cases():
        t0 = time.time()
        case.execute(outdir)
        torch.cuda.synchronize()
        with open(os.path.join(outdir, "manifest.txt"), "a") as f:
            f.write(case.name + "\n")
        print(f"{case.name}: {time.time() - t0:.2f} s", flush=True)
    print(f"cases: {time.time() - t_start:.1f} s", flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
