#!/usr/bin/env python3
"""Times csrc/smooth.hip at one flow of --sizes (default 1024 and 512 squared), HIP events around each call, median of --launches after a
warm-up:

  dct_pair:   pivlfn_dct2 forward then inverse on one fp64 plane (six launches: each call builds its tables), and the two calls on the
              2 planes of a flow; FLOP = 8 H W (H + W) per pair of planes (4 H W (H + W) per plane), as fp64 TFLOP/s -- to be read beside tools/bench_pod.py's
              tflops_fp64 for the Gram kernel, the only other user of v_mfma_f64_16x16x4_f64 here (that tool's header derives the
              78.6 TFLOP/s matrix peak it compares with)
  pcg_iter:   one iteration of pivlfn_smooth_pcg (eight launches) on a flow with 10 % random gaps and a 20 x 20 hole, with a tolerance
              no residual reaches, from a call of --iters iterations
  setup/read: pivlfn_smooth_setup (thirteen launches) and pivlfn_smooth_read
  frame:      validate_flow(mode="mask") + smooth_flow(wavelength=8) on a smooth field with noise, 5 % planted spikes and a hole, wall
              clock with the host synchronisations of sync_every=64 included, and the iterations it took; beside it the forward of
              the network on a particle pair of the same size (pivlfn.estimate), ms per pair

  python tools/bench_smooth.py [--launches 20] [--sizes 1024,512] [--iters 10] [--no-forward]

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "piv_liteflownet-pytorch_amd"))
import numpy as np
import torch

import pivlfn
from pivlfn import _lib, smooth, synth
from pivlfn.validate import validate_flow


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


def _wall(fn, launches, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(launches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    return t[len(t) // 2], out


def _field(S, seed, dev):
    """[1,2,S,S]: two long waves, 0.2 px noise, 5 % spikes of +-8 px, a 20 x 20 hole of 1e10."""
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    f = np.stack([3.0 * np.sin(2 * np.pi * ii / 97.0) * np.cos(2 * np.pi * jj / 131.0), 2.0 * np.cos(2 * np.pi * ii / 113.0 + 2 * np.pi * jj / 89.0)])
    f += 0.2 * rng.standard_normal(f.shape)
    spikes = rng.random((S, S)) < 0.05
    f[:, spikes] += 8.0 * rng.choice([-1.0, 1.0], size=(2, int(spikes.sum())))
    f[:, S // 3:S // 3 + 20, S // 2:S // 2 + 20] = 1e10
    return torch.from_numpy(f[None].astype(np.float32)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--sizes", default="1024,512")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-forward", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    for S in (int(v) for v in args.sizes.split(",")):
        H = W = S
        for P in (1, 2):
            x = torch.randn(P, H, W, dtype=torch.float64, device=dev)
            spec, back = torch.empty_like(x), torch.empty_like(x)
            nbytes = lib.pivlfn_dct2_workspace_bytes(P, H, W)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

            def pair():
                _lib.check(lib.pivlfn_dct2(x.data_ptr(), spec.data_ptr(), P, H, W, 0, ws.data_ptr(), nbytes, st), "dct2")
                _lib.check(lib.pivlfn_dct2(spec.data_ptr(), back.data_ptr(), P, H, W, 1, ws.data_ptr(), nbytes, st), "dct2")
            med, p10, p90 = _time(pair, args.launches)
            flop = 4.0 * H * W * (H + W) * P                 # four products of 2 H W K each per plane: 8 H W (H + W) per pair of planes
            print(json.dumps({"kernel": "dct_pair", "H": H, "W": W, "planes": P, "launches": 6, "us_median": round(med, 1), "us_p10": round(p10, 1),
                              "us_p90": round(p90, 1), "tflops_fp64": round(flop / med * 1e-6, 2),
                              "round_trip_max_err": float((back - x).abs().max())}), flush=True)
            del x, spec, back, ws

        flow = _field(S, 1, dev)
        rng = np.random.default_rng(2)
        mask = rng.random((1, H, W)) < 0.10
        mask[:, H // 3:H // 3 + 20, W // 2:W // 2 + 20] = True
        mask = torch.from_numpy(mask.astype(np.uint8)).to(dev)
        s = smooth.smooth_param(8.0)
        nbytes = lib.pivlfn_smooth_workspace_bytes(1, H, W)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        z = torch.empty(1, 2, H, W, dtype=torch.float64, device=dev)
        z32 = torch.empty(1, 2, H, W, dtype=torch.float32, device=dev)
        status = torch.empty(1, 2, 4, dtype=torch.float64, device=dev)

        def setup():
            _lib.check(lib.pivlfn_smooth_setup(flow.data_ptr(), None, mask.data_ptr(), 1, H, W, s, ws.data_ptr(), nbytes, st), "smooth_setup")

        def iterate():                                       # tol = 1e-300: the stopping rule never fires, every iteration does its work
            _lib.check(lib.pivlfn_smooth_pcg(ws.data_ptr(), nbytes, 1, H, W, s, 1e-300, args.iters, st), "smooth_pcg")

        def read():
            _lib.check(lib.pivlfn_smooth_read(ws.data_ptr(), nbytes, 1, H, W, z.data_ptr(), z32.data_ptr(), None, status.data_ptr(), st),
                       "smooth_read")
        med, p10, p90 = _time(setup, args.launches)
        print(json.dumps({"kernel": "smooth_setup", "H": H, "W": W, "launches": 13, "us_median": round(med, 1), "us_p10": round(p10, 1),
                          "us_p90": round(p90, 1), "workspace_MiB": round(nbytes / 2**20, 1)}), flush=True)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(max(args.launches // 4, 3) + 1)]
        for e0, e1 in ev:                                    # every timed call starts from a fresh setup: the same iterations each time
            setup()
            e0.record()
            iterate()
            e1.record()
        read()
        torch.cuda.synchronize()
        t = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev[1:])
        med, p10, p90 = t[len(t) // 2], t[0], t[-1]
        print(json.dumps({"kernel": "pcg_iter", "H": H, "W": W, "launches_per_iteration": 8, "iterations_per_call": args.iters,
                          "us_per_iteration_median": round(med / args.iters, 1), "us_per_iteration_min": round(p10 / args.iters, 1),
                          "us_per_iteration_max": round(p90 / args.iters, 1), "state_after": status[0, :, 0].tolist()}), flush=True)
        med, p10, p90 = _time(read, args.launches)
        print(json.dumps({"kernel": "smooth_read", "H": H, "W": W, "us_median": round(med, 1), "us_p10": round(p10, 1), "us_p90": round(p90, 1)}),
              flush=True)
        del ws, z, z32

        def frame():
            v = validate_flow(flow, mode="mask")
            return v, smooth.smooth_flow(flow, wavelength=8.0, mask=v.flag)
        ms_val, v = _wall(lambda: validate_flow(flow, mode="mask"), args.launches)
        ms, (v, res) = _wall(frame, max(args.launches // 4, 3))
        doc = {"kernel": "frame --validate mask --smooth 8", "H": H, "W": W, "ms_median": round(ms, 2), "ms_validate": round(ms_val, 2),
               "rejected": int((v.flag != 0).sum()), "iterations": res.iterations[0].tolist(), "converged": res.converged[0].tolist(),
               "residual": [float(r) for r in res.residual[0]]}
        if not args.no_forward:
            net = pivlfn.piv_liteflownet(synth.generate_weights("piv", 0)).to(dev).eval()
            a, b = synth.particle_batch(1, H, W, seed=5)
            a, b = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
            doc["ms_forward_per_pair"] = round(_wall(lambda: pivlfn.estimate(net, a, b, tensor=True), max(args.launches // 2, 3))[0], 2)
            del net
        print(json.dumps(doc), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
