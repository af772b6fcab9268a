#!/usr/bin/env python3
"""Times pivlfn.render_particles (csrc/particles.hip) for B = 2 frames of S x S pixels (default 1024^2) at 0.05 particles per pixel
seeded with a 16 px margin, beside pivlfn.synth.ParticleSequence.frames -- the torch index_add_ renderer the package had before --
on the same device in the same process, and pivlfn.displace_particles on the same particles.

  python tools/bench_particles.py [--size 1024] [--density 0.05] [--launches 30] [--md FILE]

Every figure is the median of --launches event-timed calls after three warm-up calls.  A render_particles call is the five launches
of pivlfn_particles_render plus torch's allocation of the outputs and the workspace (from its caching allocator: no device
allocation after the warm-up).  ParticleSequence.frames(1, 2) is timed for ONE frame with the particle positions of that frame
already cached on the host, so no host advection is inside the interval; the figure is doubled for the two frames.
The two intervals are NOT alike in one respect, and the ratio is to be read with it: ParticleSequence.frames keeps its positions on the
host, so its interval holds a float32 conversion and two synchronous host-to-device copies of 55 k floats per frame (it has no other
interface); render_particles finds its inputs on the device, where displace_particles leaves them.  The line of the old renderer
carries that as "includes".
The bounds the share is taken of (MI355X: 256 CUs x 4 SIMDs, 2.4 GHz, 6.29 TB/s measured copy rate):
  exp   the exponentials the contract asks for -- one per particle and footprint pixel inside the image -- at v_exp_f32's issue rate
        of one wave instruction per 8 cycles and SIMD: 256 * 4 * 8 * 2.4e9 = 1.97e13 per second;
  HBM   the bytes that must move: 5 per pixel written (fp32 intensity, uint8 image) and 24 per particle read (x, y, diam, amp).
One JSON line per arm; --md appends them to FILE under a heading."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "piv_liteflownet-pytorch_amd"))
from pivlfn import displace_particles, render_particles, synth  # noqa: E402

EXP_PER_S, HBM_BYTES_PER_S = 256 * 4 * 8 * 2.4e9, 6.29e12


def timed(fn, launches):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    us.sort()
    return statistics.median(us), us[len(us) // 10], us[-1 - len(us) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--md", type=str, default=None)
    a = ap.parse_args()
    if a.launches < 20:
        sys.exit("bench_particles: at least 20 launches")
    dev = torch.device("cuda:0")
    S, pad, R, B = a.size, 16, 4, 2
    N = int(a.density * (S + 2 * pad) ** 2)
    rng = np.random.default_rng(7)
    pos = torch.from_numpy(rng.uniform(-pad, S + pad, (B, 2, N))).to(dev)
    diam = torch.from_numpy((1.5 + rng.random((B, N))).astype(np.float32)).to(dev)
    amp = torch.from_numpy((240.0 * np.exp(-(rng.random((B, N)) - 0.5) ** 2)).astype(np.float32)).to(dev)
    # the exponentials the contract asks for: footprint pixels inside the image
    ix, iy = np.floor(pos[:, 0].cpu().numpy()), np.floor(pos[:, 1].cpu().numpy())
    nx = np.clip(np.minimum(ix + R + 1, S - 1) - np.maximum(ix - R, 0) + 1, 0, None)
    ny = np.clip(np.minimum(iy + R + 1, S - 1) - np.maximum(iy - R, 0) + 1, 0, None)
    exps, nbytes = float((nx * ny).sum()), B * S * S * 5 + B * N * 24
    lines = []
    med, p10, p90 = timed(lambda: render_particles(pos, diam, amp, S, S, R), a.launches)
    t_exp, t_hbm = exps / EXP_PER_S * 1e6, nbytes / HBM_BYTES_PER_S * 1e6
    lines.append({"arm": "render_particles", "frames": B, "size": S, "particles_per_frame": N, "radius": R, "launches": a.launches,
                  "median_us": round(med, 1), "p10_us": round(p10, 1), "p90_us": round(p90, 1), "exps": exps, "model_bytes": nbytes,
                  "exp_bound_us": round(t_exp, 2), "hbm_bound_us": round(t_hbm, 2), "bound": "exp" if t_exp > t_hbm else "hbm",
                  "share_of_bound": round(max(t_exp, t_hbm) / med, 4)})
    seq = synth.ParticleSequence(S, S, seed=7, density=a.density, device=dev)
    seq.frames(1, 2)                                     # the positions of frame 1 are cached on the host from here on
    old, o10, o90 = timed(lambda: seq.frames(1, 2), a.launches)
    lines.append({"arm": "ParticleSequence.frames", "frames": 1, "size": S, "particles_per_frame": int(seq.z.numel()), "launches": a.launches,
                  "median_us": round(old, 1), "p10_us": round(o10, 1), "p90_us": round(o90, 1), "two_frames_us": round(2 * old, 1),
                  "over_render_particles": round(2 * old / med, 2),
                  "includes": "a host float32 conversion and two synchronous host-to-device copies of the positions per frame; "
                              "render_particles' inputs are resident on the device"})
    flow = torch.from_numpy(np.stack(synth.displacement_field(*np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64)),
                                                              S, S)).astype(np.float32)).to(dev)
    for method in ("bilinear", "cubic"):
        d, d10, d90 = timed(lambda: displace_particles(pos[0], flow, None, method), a.launches)
        lines.append({"arm": "displace_particles", "method": method, "particles": N, "size": S, "launches": a.launches,
                      "median_us": round(d, 1), "p10_us": round(d10, 1), "p90_us": round(d90, 1)})
    for ln in lines:
        print(json.dumps(ln))
    if a.md:
        with open(a.md, "a") as f:
            f.write(f"\n## `python tools/bench_particles.py --size {S} --density {a.density} --launches {a.launches}`\n\n```\n")
            f.write("\n".join(json.dumps(ln) for ln in lines) + "\n```\n")


if __name__ == "__main__":
    main()
