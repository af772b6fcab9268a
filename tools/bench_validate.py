#!/usr/bin/env python3
"""Times pivlfn_flow_validate (csrc/validate.hip) at S x S (default 1024^2) for radius 1 and 2, spacing 1 and 4, B = 1 and 8, the
three modes, on a smooth field with 1 % planted outliers (what a PIV flow looks like) -- and pivlfn_flow_stats_accumulate_masked
at B = 8.  Each call (one launch for flag / mask, two for replace) between its own pair of HIP events, median of --launches calls
after a warm-up, against the time the bytes the contract must move need at 8 TB/s:

  validate:      B*S*S * (2*4 bytes of flow in + 2*4 bytes of flow out + 1 byte of flag)     (flag mode: no flow out)
  masked stats:  B*S*S * (2*4 + 1) bytes in + 2 x 9*S*S*8 bytes of accumulators and counts (read once, written once)

  python tools/bench_validate.py [--size 1024] [--launches 100]

Prints one JSON line per case: median / p10 / p90 microseconds, MB moved, the 8 TB/s floor and floor / median.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "piv_liteflownet-pytorch_amd"))
import torch

from pivlfn import _lib
from pivlfn import validate as V

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


def _field(B, S, dev):
    """A vortex array of 128 px wavelength and 4 px amplitude plus 0.05 px of noise, 1 % of the vectors displaced by 1.5 px."""
    g = torch.Generator(device=dev).manual_seed(0)
    y, x = torch.meshgrid(torch.arange(S, device=dev, dtype=torch.float32), torch.arange(S, device=dev, dtype=torch.float32), indexing="ij")
    k = 2 * torch.pi / 128
    flow = torch.stack([4 * torch.sin(k * y) * torch.cos(k * x), -4 * torch.cos(k * y) * torch.sin(k * x)])[None].repeat(B, 1, 1, 1)
    flow += 0.05 * torch.randn(flow.shape, generator=g, device=dev)
    spike = torch.rand((B, 1, S, S), generator=g, device=dev) < 0.01
    return (flow + 1.5 * spike).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=100)
    a = ap.parse_args()
    if a.launches < 50:
        raise SystemExit("--launches: at least 50")
    dev = torch.device("cuda:0")
    S = a.size
    lib = _lib.load()
    stream = _lib.stream_ptr(dev)
    rows = []
    for B in (1, 8):
        flow = _field(B, S, dev)
        out, flag = torch.empty_like(flow), torch.empty((B, S, S), dtype=torch.uint8, device=dev)
        for r in (1, 2):
            for s in (1, 4):
                for mode in ("flag", "mask", "replace"):
                    def run(flow=flow, out=out, flag=flag, B=B, r=r, s=s, mode=mode):
                        _lib.check(lib.pivlfn_flow_validate(flow.data_ptr(), None if mode == "flag" else out.data_ptr(), flag.data_ptr(),
                                                            None, B, S, S, r, s, 0.1, 2.0, V.MODES[mode], stream), mode)
                    run()
                    flagged = float((flag != 0).float().mean())
                    nbytes = B * S * S * (8 + 1 + (0 if mode == "flag" else 8))
                    rows.append((f"flow_validate {mode} r={r} s={s}", B, nbytes, run, {"flagged_fraction": round(flagged, 4)}))
        if B == 8:
            acc = torch.zeros((7, S, S), dtype=torch.float64, device=dev)
            cnt = torch.zeros((2, S, S), dtype=torch.float64, device=dev)
            mflag = V.validate_flow(flow, mode="flag").flag

            def stats(flow=flow, mflag=mflag, acc=acc, cnt=cnt, B=B):
                _lib.check(lib.pivlfn_flow_stats_accumulate_masked(flow.data_ptr(), mflag.data_ptr(), acc.data_ptr(), cnt.data_ptr(), B, S, S,
                                                                   1.0, stream), "masked stats")
            rows.append(("flow_stats_accumulate_masked", B, B * S * S * 9 + 2 * 9 * S * S * 8, stats, {}))
    for name, B, nbytes, fn, extra in rows:
        med, p10, p90 = _time(fn, a.launches)
        floor = nbytes / HBM * 1e6
        print(json.dumps({"kernel": name, "frames": B, "size": S, "launches": a.launches, "median_us": round(med, 2),
                          "p10_us": round(p10, 2), "p90_us": round(p90, 2), "mb_moved": round(nbytes / 1e6, 1),
                          "floor_us_at_8TBps": round(floor, 1), "fraction_of_floor": round(floor / med, 3), **extra}), flush=True)


if __name__ == "__main__":
    main()
