#!/usr/bin/env python3
"""Times the picture kernels of csrc/viz.hip at B frames of S x S (default 8 x 1024^2): pivlfn_flow_maxrad, pivlfn_flow_to_color,
pivlfn_scalar_to_color, pivlfn_field_absmax and pivlfn_flow_decimate.  Each launch between its own pair of HIP events, median of
--launches launches after a warm-up, against the time the algorithmic bytes need at 8 TB/s:

  maxrad:    8 B read per pixel                        color:   8 B read + 3 B written per pixel
  absmax:    4 B read per pixel (fp32 field)           scalar:  4 B read + 3 B written per pixel (fp32 field)
  decimate:  8 B read per pixel + 12 B written per cell

  python tools/bench_viz.py [--frames 8] [--size 1024] [--launches 100] [--cell 16]

Prints one JSON line per kernel: median / p10 / p90 microseconds, MB moved, the 8 TB/s floor and floor / median.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "piv_liteflownet-pytorch_amd"))
import torch

from bench_postpro import HBM, _time
from pivlfn import _lib, viz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--cell", type=int, default=16)
    a = ap.parse_args()
    if a.launches < 50:
        raise SystemExit("--launches: at least 50")
    dev = torch.device("cuda:0")
    B, S = a.frames, a.size
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    flow = torch.randn((B, 2, S, S), generator=g, device=dev) * 5
    field = torch.randn((B, S, S), generator=g, device=dev)
    mask = (torch.rand((B, S, S), generator=g, device=dev) < 0.05).to(torch.uint8)
    norm = torch.empty(B, dtype=torch.float32, device=dev)
    amax = torch.empty(B, dtype=torch.float64, device=dev)
    out = torch.empty((B, S, S, 3), dtype=torch.uint8, device=dev)
    lut = torch.from_numpy(viz.LUTS["bwr"]).to(dev)
    cells = -(-S // a.cell)
    mean = torch.empty((B, 2, cells, cells), dtype=torch.float32, device=dev)
    count = torch.empty((B, cells, cells), dtype=torch.int32, device=dev)
    px = B * S * S
    rows = []
    for tag, m in (("", None), (" masked", mask.data_ptr())):
        extra = px if m else 0
        rows += [
            ("flow_maxrad" + tag, 8 * px + extra,
             lambda m=m: _lib.check(lib.pivlfn_flow_maxrad(flow.data_ptr(), m, norm.data_ptr(), B, S, S, st), "maxrad")),
            ("flow_to_color" + tag, 11 * px + extra,
             lambda m=m: _lib.check(lib.pivlfn_flow_to_color(flow.data_ptr(), norm.data_ptr(), m, out.data_ptr(), B, S, S, 0, 0, st), "color")),
        ]
    rows += [
        ("flow_to_color original wheel", 11 * px,
         lambda: _lib.check(lib.pivlfn_flow_to_color(flow.data_ptr(), norm.data_ptr(), None, out.data_ptr(), B, S, S, 1, 0, st), "color")),
        ("field_absmax fp32", 4 * px, lambda: _lib.check(lib.pivlfn_field_absmax(field.data_ptr(), 0, None, amax.data_ptr(), B, S, S, st), "absmax")),
        ("scalar_to_color fp32", 7 * px,
         lambda: _lib.check(lib.pivlfn_scalar_to_color(field.data_ptr(), 0, None, lut.data_ptr(), out.data_ptr(), B, S, S, -2.0, 2.0, 0, st),
                            "scalar")),
        (f"flow_decimate cell {a.cell}", 8 * px + 12 * B * cells * cells,
         lambda: _lib.check(lib.pivlfn_flow_decimate(flow.data_ptr(), None, mean.data_ptr(), count.data_ptr(), B, S, S, a.cell, st), "decimate")),
    ]
    for name, nbytes, fn in rows:
        med, p10, p90 = _time(fn, a.launches)
        floor = nbytes / HBM * 1e6
        print(json.dumps({"kernel": name, "frames": B, "size": S, "launches": a.launches, "median_us": round(med, 2),
                          "p10_us": round(p10, 2), "p90_us": round(p90, 2), "mb_moved": round(nbytes / 1e6, 1),
                          "floor_us_at_8TBps": round(floor, 1), "fraction_of_floor": round(floor / med, 3)}), flush=True)


if __name__ == "__main__":
    main()
