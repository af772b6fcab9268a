#!/usr/bin/env python3
"""Times the post-processing kernels of csrc/postpro.hip at B frames of S x S (default 8 x 1024^2): pivlfn_flow_fields for both
kinds and both output types, and pivlfn_flow_stats_accumulate.  Each launch between its own pair of HIP events, median of
--launches launches after a warm-up, against the time the algorithmic bytes need at 8 TB/s:

  fields:  B*2*S*S*4 bytes of flow in + B*3*S*S*(4 | 8) bytes out
  stats:   B*2*S*S*4 bytes of flow in + 2 x 7*S*S*8 bytes of accumulators (read once, written once)

  python tools/bench_postpro.py [--frames 8] [--size 1024] [--launches 100]

Prints one JSON line per kernel: median / p10 / p90 microseconds, GB moved, the 8 TB/s floor and floor / median.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "piv_liteflownet-pytorch_amd"))
import torch

from pivlfn import _lib, postpro

HBM = 8e12


def _time(fn, launches, warmup=10):
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
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=100)
    a = ap.parse_args()
    if a.launches < 50:
        raise SystemExit("--launches: at least 50")
    dev = torch.device("cuda:0")
    B, S = a.frames, a.size
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(0)
    flow = torch.randn((B, 2, S, S), generator=g, device=dev) * 5
    stream = _lib.stream_ptr(dev)
    flow_bytes = B * 2 * S * S * 4
    rows = []
    for kind in postpro.KINDS:
        for dt in (torch.float32, torch.float64):
            out = torch.empty((B, 3, S, S), dtype=dt, device=dev)
            f64 = int(dt == torch.float64)

            def run(kind=kind, out=out, f64=f64):
                _lib.check(lib.pivlfn_flow_fields(flow.data_ptr(), out.data_ptr(), B, S, S, 1.0, postpro.KINDS[kind], f64, stream), kind)
            rows.append((f"flow_fields {kind} {'fp64' if f64 else 'fp32'} out", flow_bytes + out.numel() * out.element_size(), run))
    acc = torch.zeros((7, S, S), dtype=torch.float64, device=dev)

    def stats():
        _lib.check(lib.pivlfn_flow_stats_accumulate(flow.data_ptr(), acc.data_ptr(), B, S, S, 1.0, stream), "stats")
    rows.append(("flow_stats_accumulate", flow_bytes + 2 * acc.numel() * 8, stats))
    for name, nbytes, fn in rows:
        med, p10, p90 = _time(fn, a.launches)
        floor = nbytes / HBM * 1e6
        print(json.dumps({"kernel": name, "frames": B, "size": S, "launches": a.launches, "median_us": round(med, 2),
                          "p10_us": round(p10, 2), "p90_us": round(p90, 2), "mb_moved": round(nbytes / 1e6, 1),
                          "floor_us_at_8TBps": round(floor, 1), "fraction_of_floor": round(floor / med, 3)}), flush=True)


if __name__ == "__main__":
    main()
