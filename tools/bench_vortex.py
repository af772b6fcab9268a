#!/usr/bin/env python3
"""Times pivlfn_vortex_gamma (csrc/vortex.hip) at B x S x S (default 1 and 8 x 1024^2) for radius 4, 8 and 15 at spacing 1 on a
field of Lamb-Oseen vortices in a drift with noise on top.  Beside each, on the same box and in the same process: a plain-torch fp64
formulation of the same quantities (one shifted slice of the zero-padded field per neighbour) and the network's forward at that
batch, so that the share of a forward is read off one table.  Each call between its own pair of HIP events, median of --launches
calls after a warm-up.  The operation count beside each row comes from the shapes: every vector has (2r+1)^2 - 1 Gamma2 terms, each
with one fp64 square root and one fp64 division (windows clipped by the image edge have fewer; the count is the whole-window one).

  python tools/bench_vortex.py [--size 1024] [--launches 50] [--torch-launches 3] [--md FILE]

Prints one JSON line per case, then the table in Markdown (also to FILE).  The torch formulation is not bit-comparable (its sums run
in another order); the line also reports the largest difference of Gamma2 between the two where both define it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "piv_liteflownet-pytorch_amd"))
import numpy as np
import torch
import torch.nn.functional as F

import pivlfn
from pivlfn import synth
from pivlfn.vortex import FEW, default_min_count


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


def _inputs(B, S, dev):
    """Per pair a 4 x 4 array of Lamb-Oseen vortices of alternating sense (pivlfn.synth.displacement_field, tiled) plus 0.1 px of noise."""
    tile = S // 4
    y, x = np.mgrid[0:tile, 0:tile].astype(np.float64)
    u, v = synth.displacement_field(x, y, tile, tile)
    sign = np.kron(np.indices((4, 4)).sum(0) % 2 * 2.0 - 1.0, np.ones((tile, tile)))
    field = np.stack([1.5 + sign * (np.tile(u, (4, 4)) - 1.5), -0.75 + sign * (np.tile(v, (4, 4)) + 0.75)])
    rng = np.random.default_rng(0)
    flow = np.stack([field + rng.normal(0, 0.1, field.shape) for _ in range(B)]).astype(np.float32)
    return torch.from_numpy(flow).to(dev), torch.rand(B, 3, S, S, device=dev), torch.rand(B, 3, S, S, device=dev)


def torch_gamma(flow, r):
    """The same quantities in plain torch, fp64: (Gamma1, Gamma2) [B,H,W] float32, NaN where fewer than half the neighbours are valid."""
    B, _, H, W = flow.shape
    k = ((flow.abs() <= 1e9).all(1, keepdim=True))
    uv = torch.where(k, flow.double(), torch.zeros((), dtype=torch.float64, device=flow.device))
    m = uv.pow(2).sum(1, keepdim=True).sqrt()
    unit = torch.where(m > 0, uv / m, torch.zeros_like(uv))
    kp, uvp, unitp = (F.pad(t, (r, r, r, r)) for t in (k.double(), uv, unit))

    def shifted(t, i, j):
        return t[:, :, r + j:r + j + H, r + i:r + i + W]

    n_all = F.avg_pool2d(kp, 2 * r + 1, stride=1, divisor_override=1)
    mean = F.avg_pool2d(uvp, 2 * r + 1, stride=1, divisor_override=1) / n_all
    N = n_all - k.double()
    s1, s2 = torch.zeros_like(N), torch.zeros_like(N)
    for j in range(-r, r + 1):
        for i in range(-r, r + 1):
            if i == 0 and j == 0:
                continue
            d = (i * i + j * j) ** 0.5
            px, py = i / d, j / d
            un = shifted(unitp, i, j)
            s1 = s1 + (px * un[:, 1:2] - py * un[:, 0:1])
            dd = shifted(uvp, i, j) - mean
            m2 = dd.pow(2).sum(1, keepdim=True).sqrt()
            take = (shifted(kp, i, j) > 0) & (m2 > 0)
            s2 = s2 + torch.where(take, (px * dd[:, 1:2] - py * dd[:, 0:1]) / m2, torch.zeros_like(m2))
    nan = torch.full_like(N, float("nan"))
    few = N < default_min_count(r)
    return torch.where(few, nan, s1 / N).float()[:, 0], torch.where(few, nan, s2 / N).float()[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--torch-launches", type=int, default=3)
    ap.add_argument("--md", type=str, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    S = a.size
    net = pivlfn.Network(model="piv", params=synth.generate_weights("piv", 0)).to(dev).eval()
    rows = ["| pairs | size | r | Gamma2 terms (sqrt + div each) | HIP median (p10 - p90) | terms / s | torch fp64 median | torch / HIP | forward median | share of a forward |",
            "|---|---|---|---|---|---|---|---|---|---|"]
    for B in (1, 8):
        flow, img1, img2 = _inputs(B, S, dev)
        with torch.no_grad():
            fwd, _, _ = _time(lambda: net(img1, img2), a.launches)
        for r in (4, 8, 15):
            hip, p10, p90 = _time(lambda: pivlfn.vortex_gamma(flow, r), a.launches)
            v = pivlfn.vortex_gamma(flow, r)
            ref, _, _ = _time(lambda: torch_gamma(flow, r), a.torch_launches, warmup=1)
            t1, t2 = torch_gamma(flow, r)
            both = ((v.flag & FEW) == 0) & ~torch.isnan(t2)
            terms = B * S * S * ((2 * r + 1) ** 2 - 1)
            rec = {"kernel": "vortex_gamma", "pairs": B, "size": S, "radius": r, "spacing": 1, "launches": a.launches,
                   "gamma2_terms": terms, "hip_median_us": round(hip, 1), "hip_p10_us": round(p10, 1), "hip_p90_us": round(p90, 1),
                   "terms_per_second": round(terms / (hip * 1e-6), -6), "torch_median_us": round(ref, 1), "torch_over_hip": round(ref / hip, 1),
                   "forward_median_us": round(fwd, 1), "share_of_forward": round(hip / fwd, 4),
                   "max_abs_gamma1_difference": float((v.gamma1 - t1)[both].abs().max()),
                   "max_abs_gamma2_difference": float((v.gamma2 - t2)[both].abs().max())}
            print(json.dumps(rec), flush=True)
            rows.append(f"| {B} | {S}² | {r} | {terms:.3g} | {hip / 1e3:.3f} ms ({p10 / 1e3:.3f} - {p90 / 1e3:.3f}) | {terms / (hip * 1e-6):.3g} | "
                        f"{ref / 1e3:.1f} ms | {ref / hip:.0f} x | {fwd / 1e3:.2f} ms | {100.0 * hip / fwd:.1f} % |")
            del t1, t2
            torch.cuda.empty_cache()
    table = "\n".join(rows)
    print(table)
    if a.md:
        with open(a.md, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
