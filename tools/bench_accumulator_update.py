#!/usr/bin/env python3
"""The host cost of FlowStats.update and TwoPointStats.update: frames of 8 x 9, B = 1, so that the host side is all there is; 2000
calls, then a synchronise; microseconds per call up to the last enqueue and with the synchronise.

  python tools/bench_accumulator_update.py                       one process, the package of this tree: one JSON line
  python tools/bench_accumulator_update.py --against DIR         five repetitions each of the package under DIR (another checkout's
                                                                 piv_liteflownet-pytorch_amd) and of this tree's, alternated, a process
                                                                 each; then min, median and max per package and whether the median of
                                                                 this tree lies inside the other's min-max

Either package runs on the library built in this tree.  profiles/accumulator_update_host.log is the output of the second form."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "piv_liteflownet-pytorch_amd")
CALLS, REPS = 2000, 5
KEYS = ("enqueue_us_per_call", "with_sync_us_per_call")


def one(package):
    sys.path.insert(0, package)
    import torch
    from pivlfn import _lib
    _lib.LIB_PATH = os.path.join(HERE, "pivlfn", "libpivlfn.so")
    from pivlfn.postpro import FlowStats
    from pivlfn.twopoint import TwoPointStats
    dev = torch.device("cuda", 0)
    flow = torch.randn(1, 2, 8, 9, device=dev)
    out = {}
    for name, acc in (("FlowStats", FlowStats(8, 9, 1.0, dev)), ("TwoPointStats", TwoPointStats(8, 9, max_sep=4, device=dev))):
        for _ in range(500):
            acc.update(flow)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            acc.update(flow)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        out[name] = dict(zip(KEYS, (round((t1 - t0) / CALLS * 1e6, 3), round((t2 - t0) / CALLS * 1e6, 3))))
    print(json.dumps(out))


def against(other):
    rows = {"other": [], "this": []}
    for rep in range(REPS):
        for which, package in (("other", other), ("this", HERE)):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--package", package], capture_output=True, text=True, timeout=120)
            if r.returncode != 0:
                sys.exit(f"{which}, repetition {rep}: exit {r.returncode}\n{r.stdout}{r.stderr}")
            rows[which].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(f"rep {rep} {which:5s} {json.dumps(rows[which][-1])}", flush=True)
    for cls in ("FlowStats", "TwoPointStats"):
        for key in KEYS:
            o, t = ([r[cls][key] for r in rows[k]] for k in ("other", "this"))
            med = statistics.median(t)
            print(f"{cls}.update {key}: other min {min(o)} median {statistics.median(o)} max {max(o)} | this min {min(t)} median {med} "
                  f"max {max(t)} | this median inside the other's min-max: {min(o) <= med <= max(o)}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--package", default=HERE, help="the directory that holds the pivlfn package to measure (default: this tree's)")
    ap.add_argument("--against", metavar="DIR", help="alternate this tree's package with the one under DIR")
    args = ap.parse_args()
    against(os.path.abspath(args.against)) if args.against else one(os.path.abspath(args.package))


if __name__ == "__main__":
    main()
