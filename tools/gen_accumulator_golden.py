#!/usr/bin/env python3
"""Writes tests/golden/accumulator_refusals.json: the refusals of the streaming accumulators' constructors and update() calls, type and
text, and the members of their save() files, as the package gives them (the cases are those of tests/accumulator_cases.py).

  python tools/gen_accumulator_golden.py [--out FILE]

Run it on a machine with a GPU, at the commit whose texts are to be kept: a pull request that moves this code records the file at its
parent and replays it on its own code (tests/test_accumulators.py, tests/test_gpu_accumulators.py).  Nothing is launched but one
update() of two 8 x 9 frames per class that has a save().
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "piv_liteflownet-pytorch_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "accumulator_refusals.json"))
    args = ap.parse_args()
    import torch
    import accumulator_cases as cases
    if not torch.cuda.is_available():
        sys.exit("gen_accumulator_golden: the update() refusals and the save() files need a GPU")
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        doc = {"constructor": cases.constructor_cases(), "update": cases.update_cases(dev), "save": cases.save_members(dev, tmp)}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
