#!/usr/bin/env python3
"""Writes tests/golden/postpro_cases.npz and tests/golden/pin_report_postpro.json: the reference's own post-processing
(`calc_vorticity`, `de_vort`) on small flows, for the bit-exact tests of pivlfn_flow_fields.

  python tools/gen_postpro_golden.py --reference DIR        (DIR: a checkout of the reference project)

The reference's src/postpro.py needs only numpy and scipy; it is imported where it lies, by file path.  Only inputs and the
reference's outputs are stored.

Cases: all-zero, -0.0 and uniform flows (signs of zero); 1x1, 1x9, 9x1 and 2x2 images; odd sizes; a 64x96 crop of
tests/golden/DNS_turbulence_out.flo with the image's top-left corner; NaN and inf in the interior and on an edge; calib 1,
0.37, 2.5e-4 and a negative one.
"""
import argparse
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF_FILE = "src/postpro.py"


def import_reference(ref):
    spec = importlib.util.spec_from_file_location("reference_postpro", os.path.join(ref, REF_FILE))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.calc_vorticity, mod.de_vort


def dns_crop():
    sys.path.insert(0, os.path.join(ROOT, "piv_liteflownet-pytorch_amd"))
    from pivlfn.flo import read_flow
    return np.ascontiguousarray(read_flow(os.path.join(GOLD, "DNS_turbulence_out.flo"))[:64, :96])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="reference project checkout (has src/postpro.py)")
    args = ap.parse_args()
    calc_vorticity, de_vort = import_reference(args.reference)
    rng = np.random.default_rng(20261016)

    def rand(h, w, s=3.0):
        return rng.normal(0, s, (h, w, 2)).astype(np.float32)

    nonfinite = rand(11, 13)
    nonfinite[5, 6, 0] = np.nan          # interior, u
    nonfinite[3, 8, 1] = np.inf          # interior, v
    nonfinite[0, 4, 1] = np.nan          # top edge, v
    nonfinite[10, 0, 0] = -np.inf        # corner, u
    nonfinite[7, 12, 0] = np.inf         # right edge, u
    uniform = np.empty((7, 9, 2), np.float32)
    uniform[..., 0], uniform[..., 1] = 1.5, -2.25
    specs = [                            # tag, flow, calib
        ("zeros", np.zeros((8, 8, 2), np.float32), 1.0),
        ("negzero", np.full((8, 8, 2), -0.0, np.float32), 1.0),
        ("uniform", uniform, 0.37),
        ("px1x1", rand(1, 1), 1.0),
        ("row1x9", rand(1, 9), 0.37),
        ("col9x1", rand(9, 1), 1.0),
        ("sq2x2", rand(2, 2), 2.5e-4),
        ("odd13x17_c1", rand(13, 17), 1.0),
        ("odd13x17_c037", rand(13, 17), 0.37),
        ("odd13x17_c25em4", rand(13, 17), 2.5e-4),
        ("odd5x6_neg", rand(5, 6), -0.5),
        ("dns_crop", dns_crop(), 1.0),
        ("nonfinite", nonfinite, 1.0),
    ]
    store, report = {}, {"numpy": np.__version__, "scipy": __import__("scipy").__version__,
                         "reference_sha256": {REF_FILE: hashlib.sha256(open(os.path.join(args.reference, REF_FILE), "rb").read()).hexdigest()},
                         "cases": {}}
    for tag, flow, calib in specs:
        with np.errstate(all="ignore"):
            cv = np.stack(calc_vorticity(flow, calib))
            dv = np.stack(de_vort(flow, calib))
        assert cv.dtype == np.float64 and dv.dtype == np.float64, (cv.dtype, dv.dtype)
        store[f"{tag}_flow"], store[f"{tag}_calib"] = flow, np.float64(calib)
        store[f"{tag}_calc_vorticity"], store[f"{tag}_de_vort"] = cv, dv
        report["cases"][tag] = {"shape": list(flow.shape), "calib": calib,
                                "nan": [int(np.isnan(cv).sum()), int(np.isnan(dv).sum())],
                                "negative_zeros": [int((np.signbit(cv) & (cv == 0)).sum()), int((np.signbit(dv) & (dv == 0)).sum())]}
    store["cases"] = np.array([s[0] for s in specs])
    os.makedirs(GOLD, exist_ok=True)
    np.savez_compressed(os.path.join(GOLD, "postpro_cases.npz"), **store)
    with open(os.path.join(GOLD, "pin_report_postpro.json"), "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
