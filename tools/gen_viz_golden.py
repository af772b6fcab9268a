#!/usr/bin/env python3
"""Writes tests/golden/viz_cases.npz and tests/golden/pin_report_viz.json: the reference's own `motion_to_color` on small flows, for
the tests of pivlfn_flow_to_color and of its numpy restatement (tests/viz_restatement.py).

  python tools/gen_viz_golden.py --reference DIR        (DIR: a checkout of the reference project)

The reference's src/utils_plot.py and src/utils_color.py are imported where they lie.  Two things are patched in this process only:
`np.int = int` (compute_color still uses the alias NumPy removed) and, where OpenCV is not installed, an empty stand-in module for the
`import cv2` at the top of utils_plot.py (motion_to_color never calls it).  Only inputs and the reference's outputs are stored.
Without --reference, or when DIR has no src/utils_plot.py, nothing is written and the script says so.

Every case holds a flow ([H,W,2] or [L,H,W,2] float32), a maxmotion (NaN: none) and the reference's BGR picture for both wheels.  The
inputs hold no unknown vectors: there the reference's maximum is degenerate (one 1e10 vector whitens everything) and the kernels leave
such vectors out on purpose; those cases are covered by the restatement alone.

Cases: the four signed-zero pixels; an all-zero field; 1x1, 1x9 and 9x1; widths 3, 5, 7 and 13x17 (the tails of the 4-pixel packing);
the first seeded 8x8 field (sigma 3) whose largest vector normalises to just above 1 and the first where it is exactly 1; maxmotion
below the true maximum; a [3,H,W,2] sequence whose frames differ in scale; a random 32x48 field; a 64x96 crop of
tests/golden/DNS_turbulence_out.flo.
"""
import argparse
import hashlib
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF_FILES = ("src/utils_plot.py", "src/utils_color.py")
NEAR_INTEGER = 2.0 ** -16          # original wheel: a pixel whose fk lies this close to an integer may fall on either side elsewhere
NEAR_SHARE = 1e-3


def import_reference(ref):
    np.int = int                                        # this process only
    try:
        import cv2                                      # noqa: F401
    except ImportError:
        sys.modules["cv2"] = types.ModuleType("cv2")
    sys.path.insert(0, ref)
    from src.utils_plot import motion_to_color
    return motion_to_color


def dns_crop():
    with open(os.path.join(GOLD, "DNS_turbulence_out.flo"), "rb") as f:
        assert f.read(4) == b"PIEH"
        w, h = np.frombuffer(f.read(8), np.int32)
        flow = np.frombuffer(f.read(), np.float32).reshape(h, w, 2)
    return np.ascontiguousarray(flow[:64, :96])


def seeded(seed):
    return np.random.default_rng(seed).normal(0, 3, (8, 8, 2)).astype(np.float32)


def max_pixel_rad(flow):
    """The normalised length of the longest vector, in the reference's float32 operations."""
    fx, fy = flow[..., 0], flow[..., 1]
    m = np.sqrt(fx ** 2 + fy ** 2).max()
    gx, gy = fx / m, fy / m
    return np.sqrt(gx * gx + gy * gy).max()


def first_seed(pred):
    return next(s for s in range(10000) if pred(max_pixel_rad(seeded(s))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", default=None, help="reference project checkout (has src/utils_plot.py)")
    args = ap.parse_args()
    if not args.reference or not all(os.path.isfile(os.path.join(args.reference, f)) for f in REF_FILES):
        print("gen_viz_golden: no reference checkout given (--reference DIR with src/utils_plot.py and src/utils_color.py); nothing written")
        return 0
    motion_to_color = import_reference(args.reference)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import viz_restatement as vr
    rng = np.random.default_rng(20261017)

    def rand(*shape, s=3.0):
        return rng.normal(0, s, shape + (2,)).astype(np.float32)

    above, exact = first_seed(lambda r: r > 1), first_seed(lambda r: r == 1)
    seq = rand(3, 6, 10)
    seq[1] *= np.float32(0.25)
    seq[2] *= np.float32(4.0)
    odd = rand(13, 17)
    specs = [                            # tag, flow, maxmotion
        ("signed_zeros", np.array([[[1, 0.0], [1, -0.0], [-1, 0.0], [0, 0]]], np.float32), None),
        ("zeros", np.zeros((8, 8, 2), np.float32), None),
        ("px1x1", rand(1, 1), None),
        ("row1x9", rand(1, 9), None),
        ("col9x1", rand(9, 1), None),
        ("w3", rand(5, 3), None),
        ("w5", rand(4, 5), None),
        ("w7", rand(3, 7), None),
        ("odd13x17", odd, None),
        (f"max_above_one_seed{above}", seeded(above), None),
        (f"max_exactly_one_seed{exact}", seeded(exact), None),
        ("odd13x17_maxmotion2", odd, 2.0),
        ("sequence3", seq, None),
        ("random32x48", rand(32, 48), None),
        ("random32x48_maxmotion5", rand(32, 48), 5.0),
        ("dns_crop", dns_crop(), None),
    ]
    store = {}
    report = {"numpy": np.__version__,
              "reference_sha256": {f: hashlib.sha256(open(os.path.join(args.reference, f), "rb").read()).hexdigest() for f in REF_FILES},
              "max_above_one_seed": above, "max_exactly_one_seed": exact, "cases": {}}
    for tag, flow, maxmotion in specs:
        assert flow.dtype == np.float32 and not vr.unknown(np.moveaxis(flow.reshape((-1,) + flow.shape[-3:]), -1, 1)).any()
        entry = {"shape": list(flow.shape), "maxmotion": maxmotion, "differing_values": {}}
        store[f"{tag}_flow"] = flow
        store[f"{tag}_maxmotion"] = np.float64(np.nan if maxmotion is None else maxmotion)
        for wheel, original in (("interp", False), ("original", True)):
            ref = motion_to_color(flow.copy(), maxmotion=maxmotion, original_color=original)
            assert ref.dtype == np.uint8 and ref.shape == flow.shape[:-1] + (3,)
            store[f"{tag}_bgr_{wheel}"] = ref
            entry["differing_values"][wheel] = int((vr.motion_to_color(flow, maxmotion, original) != ref).sum())
        nchw = np.moveaxis(flow.reshape((-1,) + flow.shape[-3:]), -1, 1)
        n = np.float32(maxmotion) if maxmotion is not None else vr.flow_maxrad(nchw).max()
        _, fk = vr.flow_fk(nchw, np.full(len(nchw), n, np.float32))
        near = float((np.abs(fk.astype(np.float64) - np.rint(fk.astype(np.float64))) < NEAR_INTEGER).mean())
        entry["fk_near_integer_share"] = near
        if flow.size >= 2 * 1000:
            assert near <= NEAR_SHARE, (tag, near)
        report["cases"][tag] = entry
    assert max_pixel_rad(store[f"max_above_one_seed{above}_flow"]) > 1 and max_pixel_rad(store[f"max_exactly_one_seed{exact}_flow"]) == 1
    store["cases"] = np.array([s[0] for s in specs])
    os.makedirs(GOLD, exist_ok=True)
    np.savez_compressed(os.path.join(GOLD, "viz_cases.npz"), **store)
    with open(os.path.join(GOLD, "pin_report_viz.json"), "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report, indent=1))
    print("viz_cases.npz:", os.path.getsize(os.path.join(GOLD, "viz_cases.npz")), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
