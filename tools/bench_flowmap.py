#!/usr/bin/env python3
"""Times pivlfn_flowmap_advect (csrc/flowmap.hip) at S x S seeds (default 1024^2, spacing 1) through B = 8 fields in one launch, on
fields of Lamb-Oseen vortices in a drift with noise on top (pivlfn.synth.displacement_field, tiled), without and with a byte mask.
Beside it, in the same process and on the same inputs: a plain-torch fp64 formulation of the same contract (one indexed gather per
corner and component, torch.where for the frozen particles), which is what the kernel replaces.  Each call between its own pair of HIP
events, median of --launches calls after a warm-up; the state is reseeded before every call, outside the timed region.

The byte model beside each row: per particle and field 32 B of flow gathered (four corners, two components) plus 4 mask bytes where
there is a mask, counted for particles that are live at that field (a frozen lane gathers nothing), and the state read and written
once per launch (2 x 17 B per particle).  Gathered bytes are what the lanes ask for, not what the memory system moves: neighbouring
lanes share corners and lines.

  python tools/bench_flowmap.py [--size 1024] [--fields 8] [--launches 30] [--torch-launches 5] [--md FILE]

Prints one JSON line per case, then the table in Markdown (also to FILE).  The torch formulation follows the contract operation for
operation, so the line also says whether the two states are the same bits.  Also timed: pivlfn_flowmap_ftle on the final state.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "piv_liteflownet-pytorch_amd"))
import numpy as np
import torch

import pivlfn
from pivlfn import synth
from pivlfn.flowmap import LOST, OUT


def _time(fn, launches, before=lambda: None, warmup=2):
    for _ in range(warmup):
        before()
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        before()
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return t[len(t) // 2], t[len(t) // 10], t[(9 * len(t)) // 10]


def _inputs(B, S, dev):
    """B fields: a 4 x 4 array of Lamb-Oseen vortices of alternating sense (peak 4 px) in a drift, plus 0.1 px of noise per field; a
    mask with 0.1 % of the vectors rejected."""
    tile = S // 4
    y, x = np.mgrid[0:tile, 0:tile].astype(np.float64)
    u, v = synth.displacement_field(x, y, tile, tile)
    sign = np.kron(np.indices((4, 4)).sum(0) % 2 * 2.0 - 1.0, np.ones((tile, tile)))
    field = np.stack([1.5 + sign * (np.tile(u, (4, 4)) - 1.5), -0.75 + sign * (np.tile(v, (4, 4)) + 0.75)])
    rng = np.random.default_rng(0)
    flow = np.stack([field + rng.normal(0, 0.1, field.shape) for _ in range(B)]).astype(np.float32)
    mask = (rng.random((B, S, S)) < 0.001).astype(np.uint8)
    return torch.from_numpy(flow).to(dev), torch.from_numpy(mask).to(dev)


def torch_advect(flows, mask, pos, flag):
    """The forward step of the contract in plain torch, fp64: returns (pos [2,N], flag [N])."""
    B, _, H, W = flows.shape
    x, y, f = pos[0].clone(), pos[1].clone(), flag.clone()
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    lost, out, none = (torch.full((), v, dtype=torch.uint8, device=x.device) for v in (LOST, OUT, 0))
    for k in range(B):
        u, v = flows[k, 0].reshape(-1), flows[k, 1].reshape(-1)
        inside = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
        xs, ys = torch.where(inside, x, zero), torch.where(inside, y, zero)
        ix, iy = xs.floor().long().clamp_(max=W - 2), ys.floor().long().clamp_(max=H - 2)
        at = iy * W + ix
        corners = (at, at + 1, at + W, at + W + 1)
        cu, cv = [u[c].double() for c in corners], [v[c].double() for c in corners]
        known = torch.ones_like(inside)
        for c in cu + cv:
            known &= c.abs() <= 1e9
        if mask is not None:
            m = mask[k].reshape(-1)
            for c in corners:
                known &= m[c] == 0
        fx, fy = xs - ix.double(), ys - iy.double()
        gx, gy = 1.0 - fx, 1.0 - fy
        su = (gx * cu[0] + fx * cu[1]) * gy + (gx * cu[2] + fx * cu[3]) * fy
        sv = (gx * cv[0] + fx * cv[1]) * gy + (gx * cv[2] + fx * cv[3]) * fy
        g = torch.where(inside, torch.where(known, none, lost), out)
        live = f == 0
        moved = live & (g == 0)
        x, y = torch.where(moved, x + su, x), torch.where(moved, y + sv, y)
        f = torch.where(live, g, f)
    return torch.stack([x, y]), f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--fields", type=int, default=8)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--torch-launches", type=int, default=5)
    ap.add_argument("--md", type=str, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    S, B = a.size, a.fields
    flows, mask = _inputs(B, S, dev)
    rows = ["| seeds | fields | mask | live at the end | HIP median (p10 - p90) | gathered + state bytes | bytes / s | torch fp64 median | torch / HIP | same bits | ftle kernel |",
            "|---|---|---|---|---|---|---|---|---|---|---|"]
    slower = False
    for m in (None, mask):
        fm = pivlfn.FlowMap(S, S, 1, device=dev)
        hip, p10, p90 = _time(lambda: fm.update(flows, m), a.launches, before=fm.reset)
        fm.reset()
        path = fm.update(flows, m, trace=True)
        fm_steps = fm.steps
        N = fm.N
        seeds, zeros = torch.empty_like(fm.positions.reshape(2, -1)), torch.zeros(N, dtype=torch.uint8, device=dev)
        keep = (fm.positions.reshape(2, -1).clone(), fm.flag.reshape(-1).clone())
        fm.reset()
        seeds.copy_(fm.positions.reshape(2, -1))
        ref, _, _ = _time(lambda: torch_advect(flows, m, seeds, zeros), a.torch_launches, warmup=1)
        tpos, tflag = torch_advect(flows, m, seeds, zeros)
        same = bool(torch.equal(tflag, keep[1]) and torch.equal(tpos.view(torch.int64), keep[0].view(torch.int64)))
        # a particle gathers at field k if it is live before it: it moved at every earlier field (a frozen one keeps its position)
        moved = torch.cat([(path[:1].reshape(1, 2, -1) != seeds).any(1), (path[1:] != path[:-1]).reshape(B - 1, 2, -1).any(1)])
        sampled = N + int(moved[:-1].sum())                   # field 0 samples everything; field k what field k-1 moved
        nbytes = sampled * (32 + (4 if m is not None else 0)) + N * 34
        fm.steps = fm_steps
        fm._pos.copy_(keep[0])
        fm._flag.copy_(keep[1])
        ftle, _, _ = _time(fm.ftle, a.launches)
        live = float((keep[1] == 0).double().mean())
        rec = {"kernel": "flowmap_advect", "seeds": N, "size": S, "fields": B, "mask": m is not None, "launches": a.launches,
               "live_at_end": round(live, 4), "hip_median_us": round(hip, 1), "hip_p10_us": round(p10, 1), "hip_p90_us": round(p90, 1),
               "model_bytes": nbytes, "bytes_per_second": round(nbytes / (hip * 1e-6), -6), "torch_median_us": round(ref, 1),
               "torch_over_hip": round(ref / hip, 1), "same_bits_as_torch": same, "ftle_call_median_us": round(ftle, 1)}
        print(json.dumps(rec), flush=True)
        rows.append(f"| {S}² | {B} | {'yes' if m is not None else 'no'} | {100 * live:.1f} % | {hip / 1e3:.3f} ms ({p10 / 1e3:.3f} - {p90 / 1e3:.3f}) | "
                    f"{nbytes / 1e6:.0f} MB | {nbytes / (hip * 1e-6) / 1e12:.2f} TB/s | {ref / 1e3:.2f} ms | {ref / hip:.0f} x | {'yes' if same else 'no'} | "
                    f"{ftle / 1e3:.3f} ms (whole ftle() call) |")
        slower = slower or hip > ref
        del path, moved, tpos, tflag
        torch.cuda.empty_cache()
    table = "\n".join(rows)
    print(table)
    if a.md:
        with open(a.md, "w") as f:
            f.write(table + "\n")
    if slower:                  # removing the launches and temporaries of the torch formulation is why the kernel exists
        sys.exit("bench_flowmap: the kernel is slower than the plain-torch formulation")


if __name__ == "__main__":
    main()
