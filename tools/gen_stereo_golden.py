#!/usr/bin/env python3
"""Writes tests/golden/stereo_cases.npz and tests/golden/pin_report_stereo.json: the reference's own stereo arithmetic on
seeded flows, for the bit-exact tests of pivlfn_stereo_2d3c.

  python tools/gen_stereo_golden.py --reference DIR        (DIR: a checkout of the reference project)

The reference's `stereo.dewarp.nl_trans` and `stereo.vel3d.willert` are imported where they lie; stereo/dewarp.py imports
cv2 at module level for functions not used here, so a stub module stands in for it (as oracle/gen_golden.py stubs cupy).
stereo_run.py itself parses its command line and chdirs at import, so its two pieces used here are restated below with
their lines cited.  Only inputs and the reference's outputs are stored.

Cases (odd sizes): near-identity coefficients with small quadratic terms; asymmetric theta (30 / 40 deg) and alpha != 0;
calib absent and present; fps 1 and 15; exact zeros, negative values and |flow| up to ~50 px; a stage-1 denominator that
crosses zero (the output carries inf / NaN where numpy does).
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
REF_FILES = ("stereo/dewarp.py", "stereo/vel3d.py", "stereo_run.py")


def import_reference(ref):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, ref)
    from stereo.dewarp import nl_trans
    from stereo.vel3d import willert
    return nl_trans, willert


def angles(theta_deg, alpha_deg):
    """stereo_run.py:111-119 (_flo_process): one value for both cameras, left camera negated."""
    beta, theta = [], []
    for i in range(2):
        id = (-1) ** (i + 1)
        alpha = alpha_deg[0] if len(alpha_deg) == 1 else alpha_deg[i]
        th = theta_deg[0] if len(theta_deg) == 1 else theta_deg[i]
        beta.append(id * np.deg2rad(alpha))
        theta.append(id * np.deg2rad(th))
    return theta, beta


def stereo_cal(nl_trans, flow, A, fps, calibrate):
    """stereo_run.py:153-163 (_stereo_cal), verbatim arithmetic."""
    flow_cal = nl_trans(flow[:, :, 0], flow[:, :, 1], A)
    flow_stereo = np.dstack(flow_cal)
    if calibrate:
        flow_stereo = flow_stereo * calibrate * fps
    return flow_stereo


def near_identity(rng, quad):
    """x' ~ x, y' ~ y: A = [1,0,0,q,q,q | 0,0,1,q,q,q | 0,1,0,q,q,q | 0,0,1,q,q,q] plus small perturbations."""
    base = np.array([1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
    noise = rng.normal(0, 1e-2, 24)
    noise[[3, 4, 5, 9, 10, 11, 15, 16, 17, 21, 22, 23]] *= quad / 1e-2
    return [float(v) for v in base + noise]       # JSON numbers: Python floats


def flows(rng, h, w, peak):
    f = rng.normal(0, peak / 3, (h, w, 2)).astype(np.float32)
    f = np.clip(f, -peak, peak).astype(np.float32)
    f[0, 0] = 0.0                                   # exact zeros
    f[0, 1] = (-0.0, 0.0)
    f[1, 0] = (peak, -peak)
    return f


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="reference project checkout (has stereo/ and stereo_run.py)")
    args = ap.parse_args()
    nl_trans, willert = import_reference(args.reference)
    rng = np.random.default_rng(20261016)
    cases = []
    # tag, (h, w), peak |flow|, theta, alpha, fps, --calib, coeff calib, quadratic size
    specs = [
        ("ident", (7, 9), 5.0, [45.0], [0.0], 1, None, None, 1e-4),
        ("asym_calib", (11, 13), 50.0, [30.0, 40.0], [5.0, -3.0], 15, 0.05, 0.002, 1e-4),
        ("calib_fps1", (9, 5), 20.0, [30.0, 40.0], [2.5], 1, 0.05, 0.002, 1e-3),
        ("calib_absent", (5, 11), 50.0, [35.0], [4.0, 1.0], 15, None, 0.002, 1e-3),
        ("calib_no_coeff", (3, 7), 10.0, [25.0, 35.0], [0.0], 15, 0.05, None, 1e-4),
        ("pole", (9, 7), 8.0, [30.0, 40.0], [5.0, -3.0], 15, 0.05, 0.002, 0.0),
    ]
    store, report = {}, {"numpy": np.__version__,
                         "reference_sha256": {f: hashlib.sha256(open(os.path.join(args.reference, f), "rb").read()).hexdigest()
                                              for f in REF_FILES},
                         "cases": {}}
    for tag, (h, w), peak, th, al, fps, calib, ccal, quad in specs:
        left, right = flows(rng, h, w, peak), flows(rng, h, w, peak)
        cl, cr = near_identity(rng, quad), near_identity(rng, quad)
        if tag == "pole":
            # left x-denominator = u - 3 and right y-denominator = v + 2: a row of exact poles, 0/0 where the numerator vanishes too
            cl[6:12] = [1.0, 0.0, -3.0, 0.0, 0.0, 0.0]
            cr[18:24] = [0.0, 1.0, 2.0, 0.0, 0.0, 0.0]
            left[2, :, 0] = 3.0
            right[3, :, 1] = -2.0
            left[2, 0, :] = (3.0, 0.0)
            cl[0:6] = [1.0, 0.0, -3.0, 0.0, 0.0, 0.0]      # numerator u - 3 as well: 0/0 on that row
            left[4, :, 0] = np.linspace(2.5, 3.5, w, dtype=np.float32)   # the denominator changes sign along the row
        coeff = {"Left": cl, "Right": cr}
        if ccal is not None:
            coeff["calib"] = ccal
        # stereo_run.py:65-69: the calib rule of direct_process / _flo_process
        if "calib" in coeff.keys():
            calibrate = calib / coeff["calib"] if calib else None
        else:
            calibrate = None
        theta, beta = angles(th, al)
        with np.errstate(all="ignore"):
            fc = [stereo_cal(nl_trans, f, coeff[n], fps, calibrate) for f, n in ((left, "Left"), (right, "Right"))]
            out = willert(fc, theta, beta)
        assert fc[0].dtype == np.float32 and out.dtype == np.float64, (fc[0].dtype, out.dtype)
        out = out.astype(np.float32)                  # the .flo payload
        store[f"{tag}_left"], store[f"{tag}_right"] = left, right
        store[f"{tag}_coeff"] = np.array(cl + cr, dtype=np.float64)
        store[f"{tag}_coeff_calib"] = np.float64(np.nan if ccal is None else ccal)
        store[f"{tag}_theta"] = np.array(th, dtype=np.float64)
        store[f"{tag}_alpha"] = np.array(al, dtype=np.float64)
        store[f"{tag}_fps"] = np.int64(fps)
        store[f"{tag}_calib"] = np.float64(np.nan if calib is None else calib)
        store[f"{tag}_out"] = out
        cases.append(tag)
        fin = np.isfinite(out)
        report["cases"][tag] = {"shape": list(out.shape), "nan": int(np.isnan(out).sum()), "inf": int(np.isinf(out).sum()),
                                "max_abs_finite": float(np.abs(out[fin]).max()) if fin.any() else None,
                                "scaled": calibrate is not None, "fps": fps}
    store["cases"] = np.array(cases)
    os.makedirs(GOLD, exist_ok=True)
    np.savez_compressed(os.path.join(GOLD, "stereo_cases.npz"), **store)
    with open(os.path.join(GOLD, "pin_report_stereo.json"), "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
