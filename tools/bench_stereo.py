#!/usr/bin/env python3
"""Stereo throughput: `estimate_stereo` against a plain forward of the same 2B pairs, and the 2D3C kernel on its own.

  python tools/bench_stereo.py [--size 1024] [--batches 1,4] [--iters 20]     end to end, device events after warm-up
  python tools/bench_stereo.py --kernel-only [--size 1024] [--iters 50]      the kernel alone (run it under
                                                                              rocprofv3 --kernel-trace --stats -- python ...)
Prints one JSON line.  The kernel's floor at S x S, B steps, raw flow at the output size: 16 B read + 12 B written per output
pixel over 8 TB/s of HBM.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "piv_liteflownet-pytorch_amd"))
import pivlfn  # noqa: E402
from pivlfn import stereo, synth  # noqa: E402

COEFF = {"Left": [1.0, 0, 0, 1e-4, 1e-4, 1e-4, 0, 0, 1.0, 1e-4, 1e-4, 1e-4, 0, 1.0, 0, 1e-4, 1e-4, 1e-4, 0, 0, 1.0, 1e-4, 1e-4, 1e-4],
         "calib": 0.002}
COEFF["Right"] = list(COEFF["Left"])


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3          # seconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batches", type=str, default="1,4")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    S = args.size
    tans = stereo.tangents(*stereo.angles([30.0, 40.0], [5.0]))
    res = {"size": S}
    if args.kernel_only:
        flow = torch.randn(2, 2, S, S, device=dev) * 4
        sec = timed(lambda: stereo.stereo_2d3c(flow, COEFF, tans, 15, 0.05), args.iters)
        floor_us = 28.0 * S * S / 8e12 * 1e6
        res.update({"kernel_us_events": round(sec * 1e6, 2), "floor_us_8TBps": round(floor_us, 2),
                    "note": "events include the host launch path; the rocprofv3 kernel-trace duration is the kernel's own"})
        print(json.dumps(res))
        return
    net = pivlfn.piv_liteflownet(synth.generate_weights("piv", 0)).to(dev).eval()
    for B in (int(b) for b in args.batches.split(",")):
        l1, l2 = (torch.from_numpy(x).to(dev) for x in synth.particle_batch(B, S, S, seed=1))
        r1, r2 = (torch.from_numpy(x).to(dev) for x in synth.particle_batch(B, S, S, seed=2))
        a, b = stereo.interleave(l1, r1), stereo.interleave(l2, r2)
        t_st = timed(lambda: pivlfn.estimate_stereo(net, l1, l2, r1, r2, COEFF, [30.0, 40.0], [5.0], 15, 0.05, tensor=True),
                     args.iters)
        t_fw = timed(lambda: pivlfn.estimate(net, a, b, tensor=True), args.iters)
        res[f"B{B}"] = {"stereo_steps_per_s": round(B / t_st, 2), "pairs_per_s_2B_estimate": round(2 * B / t_fw, 2),
                        "ratio_steps_to_half_pairs": round((B / t_st) / (B / t_fw), 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
