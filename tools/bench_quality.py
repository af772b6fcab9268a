#!/usr/bin/env python3
"""Times pivlfn_match_quality (csrc/quality.hip) at B x S x S (default 1 and 8 x 1024^2) for radius 8 and 15 on synthetic particle
pairs with their true flow plus 0.2 px of error, three equal channels as the network gets them.  Beside each, on the same box and in
the same process: a plain-torch formulation of the same quantities (grid_sample in fp64, the 30 box sums by fp64 avg_pool2d with
divisor 1, the Gaussian fit) and the network's forward at that batch, so that the share of a forward is read off one table.  Each
call between its own pair of HIP events, median of --launches calls after a warm-up.

  python tools/bench_quality.py [--size 1024] [--launches 50] [--torch-launches 5]

Prints one JSON line per case.  The torch formulation is not bit-comparable (its sums run in another order); the line also reports
the largest difference of c between the two where both define it.
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
from pivlfn import _lib, synth
from pivlfn.quality import FEW, FLAT, default_min_count

SHIFTS = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))


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
    tile = min(S, 256)                                   # the CPU renderer is slow: one 256^2 pair per image, tiled
    reps = -(-S // tile)
    i1, i2, fl = [], [], []
    for b in range(B):
        a, c, f = synth.particle_pair(tile, tile, 100 + b)
        i1.append(np.tile(a, (reps, reps))[:S, :S])
        i2.append(np.tile(c, (reps, reps))[:S, :S])
        fl.append(np.tile(f, (1, reps, reps))[:, :S, :S])
    to = lambda x: torch.from_numpy(np.stack(x)).to(dev)          # noqa: E731
    img1 = (to(i1).float() / 255.0)[:, None].repeat(1, 3, 1, 1).contiguous()
    img2 = (to(i2).float() / 255.0)[:, None].repeat(1, 3, 1, 1).contiguous()
    return img1, img2, (to(fl) - torch.tensor([0.2, -0.15], device=dev)[None, :, None, None]).contiguous()


def torch_quality(img1, img2, flow, r, floor=1.0 / 255.0):
    """The same quantities in plain torch: c [B,H,W] float32 (NaN where few or flat) and the residual [B,2,H,W]."""
    B, _, H, W = img1.shape
    a, g2 = img1.double().mean(1, keepdim=True), img2.double().mean(1, keepdim=True)
    ys, xs = torch.meshgrid(torch.arange(H, device=flow.device, dtype=torch.float32),
                            torch.arange(W, device=flow.device, dtype=torch.float32), indexing="ij")
    xf, yf = (xs + flow[:, 0]).double(), (ys + flow[:, 1]).double()
    m = ((xf >= 0) & (xf <= W - 1) & (yf >= 0) & (yf <= H - 1))[:, None]
    grid = torch.stack([2.0 * xf / max(W - 1, 1) - 1.0, 2.0 * yf / max(H - 1, 1) - 1.0], dim=-1)
    b = torch.where(m, F.grid_sample(g2, grid, mode="bilinear", padding_mode="zeros", align_corners=True), torch.zeros_like(a))
    k, mc = 2 * r + 1, default_min_count(r)
    cs, ok = [], []
    for sx, sy in SHIFTS:
        bs = torch.roll(F.pad(b, (1, 1, 1, 1)), (-sy, -sx), (2, 3))[:, :, 1:-1, 1:-1]
        part = torch.roll(F.pad(m, (1, 1, 1, 1)), (-sy, -sx), (2, 3))[:, :, 1:-1, 1:-1].double()
        terms = torch.cat([part, a * part, a * a * part, bs * part, bs * bs * part, a * bs * part], dim=1)
        n, A, AA, Bs, BB, AB = F.avg_pool2d(terms, k, stride=1, padding=r, divisor_override=1).unbind(1)
        va, vb, cov = AA - A * A / n, BB - Bs * Bs / n, AB - A * Bs / n
        ok.append((n >= mc) & (va >= floor * floor * n) & (vb >= floor * floor * n))
        cs.append(cov / torch.sqrt(va * vb))
    c0 = cs[0]
    fit = ok[0] & ok[1] & ok[2] & ok[3] & ok[4] & (c0 > 0)
    d = []
    for cm, cp in ((cs[1], cs[2]), (cs[3], cs[4])):
        fit = fit & (cm > 0) & (cp > 0) & (c0 >= cm) & (c0 >= cp) & (2.0 * c0 - cm - cp >= 1e-6)
    l0 = torch.log(c0)
    for cm, cp in ((cs[1], cs[2]), (cs[3], cs[4])):
        lm, lp = torch.log(cm), torch.log(cp)
        d.append(torch.where(fit, 0.5 * (lm - lp) / (lm - 2.0 * l0 + lp), torch.zeros_like(c0)).float())
    return torch.where(ok[0], c0, torch.full_like(c0, float("nan"))).float(), torch.stack(d, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--torch-launches", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    S = a.size
    net = pivlfn.Network(model="piv", params=synth.generate_weights("piv", 0)).to(dev).eval()
    for B in (1, 8):
        img1, img2, flow = _inputs(B, S, dev)
        with torch.no_grad():
            fwd, _, _ = _time(lambda: net(img1, img2), a.launches)
        for r in (8, 15):
            hip, p10, p90 = _time(lambda: pivlfn.match_quality(img1, img2, flow, r), a.launches)
            q = pivlfn.match_quality(img1, img2, flow, r)
            ref, _, _ = _time(lambda: torch_quality(img1, img2, flow, r), a.torch_launches, warmup=1)
            tc, td = torch_quality(img1, img2, flow, r)
            both = ((q.flag & (FEW | FLAT)) == 0) & ~torch.isnan(tc)
            print(json.dumps({"kernel": "match_quality", "pairs": B, "size": S, "radius": r, "launches": a.launches,
                              "hip_median_us": round(hip, 1), "hip_p10_us": round(p10, 1), "hip_p90_us": round(p90, 1),
                              "torch_median_us": round(ref, 1), "torch_over_hip": round(ref / hip, 1),
                              "forward_median_us": round(fwd, 1), "share_of_forward": round(hip / fwd, 4),
                              "max_abs_c_difference": float((q.c - tc)[both].abs().max()),
                              "max_abs_d_difference": float((q.residual - td).abs().max())}), flush=True)
            del tc, td
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
