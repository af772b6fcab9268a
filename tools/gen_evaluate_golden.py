#!/usr/bin/env python3
"""Writes tests/golden/evaluate_cases.npz and tests/golden/pin_report_evaluate.json: the reference's own error measures
(src/loss.py: EPE, L1, L2, MultiScale, LevelLoss through hui_loss / piv_loss) on small flows, in float32 as the reference runs them
and on .double() inputs, for the tests of pivlfn.evaluate and src.loss.

  python tools/gen_evaluate_golden.py --reference DIR        (DIR: a checkout of the reference project)

The reference's src/loss.py needs only torch and numpy; it is imported where it lies, by file path.  Only inputs and the reference's
results are stored.  Every input is rounded to float16 before the reference sees it and stored as float16 (half the bytes; the
float32 the tests rebuild from it is the very value the reference was given).

Inputs: `small_*` 64 x 96, B = 2 and `big_*` 256 x 320, B = 1 -- a truth (`*_truth` [B,2,H,W]) and one flow per pyramid level and
stage (`*_L<level>_<stage>` [B,2,H >> (level-1),W >> (level-1)], stages 0..2; the big set has stage 2 only and levels 6..2).
Results: `<case>_f32` and `<case>_f64`, each the reference's return value flattened to a float64 vector.  The case table is stored
as JSON in `cases`: name -> {fn, args, set, levels, stages, n} with n the number of pixels of the largest map the case sums over.
"""
import argparse
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF_FILE = "src/loss.py"
DEMO = ("images/demo/DNS_turbulence_out.flo", "images/demo/DNS_turbulence_flow.flo")


def import_reference(ref):
    spec = importlib.util.spec_from_file_location("reference_loss", os.path.join(ref, REF_FILE))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def half(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16)


def make_set(rng, B, H, W, levels, stages):
    """A smooth truth with noise, and per level a flow about one level-unit off div * pooled truth (div 1/5)."""
    yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    truth = np.stack([np.stack([3 * np.sin(5 * yy + b) * np.cos(4 * xx) + 1.5, 2 * np.cos(3 * yy) * np.sin(6 * xx + b) - 0.75]) for b in range(B)])
    truth = half(truth + rng.normal(0, 0.5, truth.shape))
    flows = {}
    t = torch.from_numpy(truth.astype(np.float32))
    for L in levels:
        pooled = torch.nn.functional.avg_pool2d(t, 1 << (L - 1)).numpy() * 0.2
        for s in stages:
            flows[(L, s)] = half(pooled + rng.normal(0, 0.3, pooled.shape))
    return truth, flows


def flat(res):
    """The reference's return value (a tensor, or nested lists of tensors / floats) as a float64 vector."""
    if isinstance(res, (list, tuple)):
        return np.concatenate([flat(r) for r in res])
    return np.atleast_1d(np.asarray(res.detach().cpu().numpy() if isinstance(res, torch.Tensor) else res, dtype=np.float64))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="reference project checkout (has src/loss.py)")
    args = ap.parse_args()
    ref = import_reference(args.reference)
    rng = np.random.default_rng(20261017)
    sets = {"small": make_set(rng, 2, 64, 96, range(6, 0, -1), range(3)), "big": make_set(rng, 1, 256, 320, range(6, 1, -1), (2,))}
    hw = {"small": 2 * 64 * 96, "big": 256 * 320}

    # name -> how the tests rebuild the call: fn (a name of src.loss), its keyword arguments, and which flows go in
    cases = {}

    def add(name, fn, kw, data, levels, stages, call=None):
        cases[name] = dict(fn=fn, args=kw, set=data, levels=list(levels), stages=list(stages), call=call or {},
                           n=hw[data] >> (2 * (min(levels) - 1)))

    for mean in (True, False):
        add(f"epe_mean{int(mean)}", "EPE", {}, "small", [1], [2], call=dict(mean=mean))
        add(f"l1_mean{int(mean)}", "L1", dict(mean=mean), "small", [1], [2])
        add(f"l2_mean{int(mean)}", "L2", dict(mean=mean), "small", [1], [2])
    add("l1loss", "L1Loss", dict(mul_scale=5), "small", [1], [2])
    add("l2loss", "L2Loss", dict(mul_scale=5), "small", [1], [2])
    for norm in ("L1", "L2"):
        # the evaluation branch: one flow at the lowest level
        add(f"ms_test_hui_{norm}", "hui_loss", dict(norm=norm), "small", [2], [2])
        add(f"ms_test_piv1_{norm}", "piv_loss", dict(norm=norm, version=1), "small", [1], [2])
        add(f"ms_test_piv2_{norm}", "piv_loss", dict(norm=norm, version=2), "small", [2], [2])
        # the per-level branch, every level a list (M, S, R), with both weight sets
        add(f"ms_list_hui_{norm}", "hui_loss", dict(norm=norm), "small", range(6, 1, -1), range(3))
        add(f"ms_list_piv1_{norm}", "piv_loss", dict(norm=norm, version=1), "small", range(6, 0, -1), range(3))
        add(f"ms_list_piv2_{norm}", "piv_loss", dict(norm=norm, version=2), "small", range(6, 1, -1), range(3))
        add(f"level_hui_{norm}", "hui_loss", dict(level_eval=True, norm=norm), "small", range(6, 1, -1), range(3))
        add(f"level_piv1_{norm}", "piv_loss", dict(level_eval=True, norm=norm, version=1), "small", range(6, 0, -1), range(3))
    add("level_big_hui_L1", "hui_loss", dict(level_eval=True, norm="L1"), "big", range(6, 1, -1), [2])
    # piv_loss(level_eval=True, version=2) builds six scales (64 .. 2) whatever the version: a 64 x 64 window, which the contract
    # (k <= 5) refuses -- not recorded

    store = {}
    for name, (truth, flows) in sets.items():
        store[f"{name}_truth"] = truth
        for (L, s), f in flows.items():
            store[f"{name}_L{L}_{s}"] = f

    def inputs(case, dtype):
        tr = torch.from_numpy(store[f"{case['set']}_truth"].astype(np.float32)).to(dtype)
        lv = [[torch.from_numpy(store[f"{case['set']}_L{L}_{s}"].astype(np.float32)).to(dtype) for s in case["stages"]] for L in case["levels"]]
        if len(case["levels"]) == 1:
            return lv[0][0], tr
        return [trio if len(trio) > 1 else trio[0] for trio in lv], tr

    import inspect
    names = ("EPE", "L1", "L2", "L1Loss", "L2Loss", "MultiScale", "LevelLoss", "hui_loss", "piv_loss")
    sigs = {n: str(inspect.signature(getattr(ref, n).__init__ if inspect.isclass(getattr(ref, n)) else getattr(ref, n))) for n in names}
    report = {"numpy": np.__version__, "torch": torch.__version__, "signatures": sigs,
              "reference_sha256": {REF_FILE: hashlib.sha256(open(os.path.join(args.reference, REF_FILE), "rb").read()).hexdigest()},
              "cases": {}}
    for name, case in cases.items():
        fn = getattr(ref, case["fn"])
        for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            out, tr = inputs(case, dtype)
            with torch.no_grad():
                res = fn(out, tr, **case["call"]) if case["fn"] == "EPE" else fn(**case["args"])(out, tr)
            store[f"{name}_{tag}"] = flat(res)
        a, b = store[f"{name}_f32"], store[f"{name}_f64"]
        report["cases"][name] = {"values": int(b.size), "n": case["n"], "f64": [float(x) for x in b],
                                 "f32_rel_err_max": float(np.max(np.abs(a - b) / np.abs(b)))}
    store["cases"] = np.array(json.dumps(cases))

    # the demo pair: the reference's own network output against the true field that ships next to it
    sys.path.insert(0, os.path.join(ROOT, "piv_liteflownet-pytorch_amd"))
    from pivlfn.flo import read_flow
    out_flo, true_flo = (read_flow(os.path.join(args.reference, p)) for p in DEMO)
    demo = {}
    for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        o, t = (torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))[None].to(dtype) for x in (out_flo, true_flo))
        demo[f"epe_{tag}"] = float(ref.EPE(o, t))
        demo[f"l1_{tag}"] = float(ref.L1()(o, t))
    demo["shape"] = list(true_flo.shape)
    demo["files_sha256"] = {os.path.basename(p): hashlib.sha256(open(os.path.join(args.reference, p), "rb").read()).hexdigest() for p in DEMO}
    report["demo_DNS_turbulence"] = demo

    os.makedirs(GOLD, exist_ok=True)
    np.savez_compressed(os.path.join(GOLD, "evaluate_cases.npz"), **store)
    with open(os.path.join(GOLD, "pin_report_evaluate.json"), "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in report.items() if k != "cases"}, indent=1))
    print({k: v["f32_rel_err_max"] for k, v in report["cases"].items()})
    print("npz bytes:", os.path.getsize(os.path.join(GOLD, "evaluate_cases.npz")))


if __name__ == "__main__":
    main()
