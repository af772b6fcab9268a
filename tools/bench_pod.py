#!/usr/bin/env python3
"""Times the two snapshot-POD entry points of csrc/pod.hip: pivlfn_snapshot_gram and pivlfn_snapshot_project, each launch between
its own pair of HIP events, median of --launches launches after a warm-up, at (n, P) = (256, 2*128^2), (1250, 2*128^2),
(256, 2*1024^2) and (1250, 2*1024^2).  Beside each Gram figure, two bounds computed from the shape:

  bytes:  every 64 x 64 block of the upper triangle reads its 128 rows (64 on the diagonal) of P floats once; the sum over the blocks
          at 6.29 TB/s, the copy rate measured for the device (the rows are shared between blocks, so caches can only help)
  mfma:   blocks * 16 tiles * ceil(P / 64) * 16 matrix instructions of 16x16x4 fp64, at one per 64 cycles per SIMD (16 passes: the
          78.6 TFLOP/s fp64 matrix peak over 1024 SIMDs at 2.4 GHz is 32 FLOP per cycle per SIMD, the instruction is 2048 FLOP),
          spread over min(blocks * splits, 256) compute units of 4 SIMDs

and, as an outside yardstick, torch.matmul(X64, X64.T) on X.double(): the vendor DGEMM, which needs the fp64 copy of X that the
kernel avoids (skipped with a note where the copy does not fit).  Project is a stream of X: its bound is n*P*4 + K*P*8 bytes.

  python tools/bench_pod.py [--launches 20] [--shapes 256x32768,1250x2097152]

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "piv_liteflownet-pytorch_amd"))
import torch

from pivlfn import _lib

COPY_RATE = 6.29e12
CLOCK, SIMDS, CUS, MFMA_CYCLES = 2.4e9, 1024, 256, 64
SLAB = 2048
SHAPES = "256x32768,1250x32768,256x2097152,1250x2097152"


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
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--no-dgemm", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    for shape in args.shapes.split(","):
        n, P = (int(v) for v in shape.split("x"))
        X = torch.empty(n, P, device=dev)
        for i in range(0, n, 64):                                  # filled in pieces: no second copy of X at the large shapes
            X[i:i + 64].normal_()
        G = torch.empty(n, n, dtype=torch.float64, device=dev)
        nbytes = lib.pivlfn_snapshot_gram_workspace_bytes(n, P)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        nb = -(-n // 64)
        blocks = nb * (nb + 1) // 2
        split = nbytes > 256
        wgs = blocks * (-(-P // SLAB) if split else 1)
        read = (blocks * 128 - nb * 64) * P * 4
        mfmas = blocks * 16 * -(-P // 64) * 16
        t_bytes = read / COPY_RATE * 1e6
        t_mfma = mfmas * MFMA_CYCLES / (4 * min(wgs, CUS) * CLOCK) * 1e6

        def gram():
            _lib.check(lib.pivlfn_snapshot_gram(X.data_ptr(), n, P, P, G.data_ptr(), ws.data_ptr(), nbytes, st), "snapshot_gram")
        med, p10, p90 = _time(gram, args.launches)
        print(json.dumps({"kernel": "snapshot_gram", "n": n, "P": P, "blocks": blocks, "workgroups": wgs, "slabs_through_workspace": split,
                          "us_median": round(med, 1), "us_p10": round(p10, 1), "us_p90": round(p90, 1),
                          "us_bound_bytes": round(t_bytes, 1), "us_bound_mfma": round(t_mfma, 1),
                          "tflops_fp64": round(2.0 * mfmas * 1024 / med * 1e-6, 2)}), flush=True)
        free = torch.cuda.mem_get_info(dev)[0]
        if args.no_dgemm:
            pass
        elif n * P * 8 * 1.2 > free:
            print(json.dumps({"kernel": "dgemm", "n": n, "P": P, "note": f"skipped: the fp64 copy of X ({n * P * 8 / 2**30:.1f} GiB) does not "
                              f"fit in the {free / 2**30:.1f} GiB free"}), flush=True)
        else:
            X64 = X.double()
            med, p10, p90 = _time(lambda: torch.matmul(X64, X64.t(), out=G), args.launches)
            print(json.dumps({"kernel": "dgemm torch.matmul(X64, X64.T)", "n": n, "P": P, "us_median": round(med, 1), "us_p10": round(p10, 1),
                              "us_p90": round(p90, 1), "fp64_copy_GiB": round(n * P * 8 / 2**30, 2)}), flush=True)
            del X64
        for K in (4, 16):
            Wt = torch.randn(n, K, dtype=torch.float64, device=dev)
            out = torch.empty(K, P, dtype=torch.float64, device=dev)

            def project():
                _lib.check(lib.pivlfn_snapshot_project(X.data_ptr(), n, P, P, Wt.data_ptr(), K, out.data_ptr(), st), "snapshot_project")
            med, p10, p90 = _time(project, args.launches)
            moved = n * P * 4 + K * P * 8
            print(json.dumps({"kernel": "snapshot_project", "n": n, "P": P, "K": K, "us_median": round(med, 1), "us_p10": round(p10, 1),
                              "us_p90": round(p90, 1), "us_bound_bytes": round(moved / COPY_RATE * 1e6, 1),
                              "TBps": round(moved / med * 1e-6, 2)}), flush=True)
            del Wt, out
        del X, G, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
