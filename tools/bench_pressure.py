#!/usr/bin/env python3
"""Times csrc/pressure.hip at F = 2 frames of --sizes (default 256 and 1024 squared lattices), HIP events around each call, median of
--launches after a warm-up; the flows are unit-variance noise, so every interior node is valid:

  setup:     pivlfn_pressure_setup (one launch)
  cg_iter:   one iteration of pivlfn_pressure_cg (two launches) with tol = 1e-300, which stops no frame, from a call of --iters
             iterations; every timed call starts from a fresh setup
  read:      pivlfn_pressure_read (one launch)

  python tools/bench_pressure.py [--launches 20] [--sizes 256,1024] [--iters 50]

Prints one JSON line per measurement.  tools/bench_ops.py pressure has the HBM bound of an iteration and the wall time of the class."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "piv_liteflownet-pytorch_amd"))
import torch

from pivlfn import _lib


def _time(fn, launches, warmup=3):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return t[len(t) // 2], t[len(t) // 10], t[(9 * len(t)) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    F = 2
    for S in (int(v) for v in args.sizes.split(",")):
        gen = torch.Generator().manual_seed(4)
        flows = torch.randn(F + 2, 2, S, S, generator=gen).to(dev)
        g = torch.empty(F, 2, S, S, dtype=torch.float64, device=dev)
        valid = torch.empty(F, S, S, dtype=torch.uint8, device=dev)
        nbytes = lib.pivlfn_pressure_workspace_bytes(F, S, S)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        p = torch.empty(F, S, S, dtype=torch.float64, device=dev)
        flag = torch.empty(F, S, S, dtype=torch.uint8, device=dev)
        status = torch.empty(F, 4, dtype=torch.float64, device=dev)
        _lib.check(lib.pivlfn_pressure_gradient(flows.data_ptr(), F + 2, S, S, 4.0, 0.01, g.data_ptr(), valid.data_ptr(), st), "pressure_gradient")

        def setup():
            _lib.check(lib.pivlfn_pressure_setup(g.data_ptr(), valid.data_ptr(), F, S, S, 4.0, ws.data_ptr(), nbytes, st), "pressure_setup")

        def iterate():                                       # tol = 1e-300: the stopping rule never fires, every iteration does its work
            _lib.check(lib.pivlfn_pressure_cg(ws.data_ptr(), nbytes, F, S, S, 1e-300, args.iters, st), "pressure_cg")

        def read():
            _lib.check(lib.pivlfn_pressure_read(ws.data_ptr(), nbytes, F, S, S, p.data_ptr(), flag.data_ptr(), status.data_ptr(), st), "pressure_read")
        med, p10, p90 = _time(setup, args.launches)
        print(json.dumps({"kernel": "pressure_setup", "F": F, "h": S, "w": S, "us_median": round(med, 1), "us_p10": round(p10, 1),
                          "us_p90": round(p90, 1), "workspace_MiB": round(nbytes / 2**20, 1)}), flush=True)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.launches + 1)]
        for e0, e1 in ev:                                    # every timed call starts from a fresh setup: the same iterations each time
            setup()
            e0.record()
            iterate()
            e1.record()
        read()
        torch.cuda.synchronize()
        t = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev[1:])
        print(json.dumps({"kernel": "cg_iter", "F": F, "h": S, "w": S, "launches_per_iteration": 2, "iterations_per_call": args.iters,
                          "us_per_iteration_median": round(t[len(t) // 2] / args.iters, 2), "us_per_iteration_min": round(t[0] / args.iters, 2),
                          "us_per_iteration_max": round(t[-1] / args.iters, 2), "state_after": status[:, 0].tolist(),
                          "iterations_after": status[:, 1].tolist()}), flush=True)
        med, p10, p90 = _time(read, args.launches)
        print(json.dumps({"kernel": "pressure_read", "F": F, "h": S, "w": S, "us_median": round(med, 1), "us_p10": round(p10, 1),
                          "us_p90": round(p90, 1)}), flush=True)
        del flows, g, valid, ws, p, flag
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
