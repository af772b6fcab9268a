"""CPU: every refusal of the analysis entry points, word for word.  tests/refusal_cases.py holds the calls, tests/golden/refusal_texts.json
what the library answered when the file was written: the return code and the whole message of every single perturbation, and per
entry point which of two messages wins when two perturbations are applied together (the order of the checks)."""
import json
import os
import re

import pytest

import refusal_cases as rc


@pytest.fixture(scope="module")
def golden():
    with open(rc.GOLDEN) as f:
        return json.load(f)


def test_the_file_covers_every_analysis_entry_point(golden):
    """The names tests/test_analysis_plans.py collects (pivlfn_stereo_2d3c up to the network's own pivlfn_create, the workspace queries
    apart) and the two uncertainty entry points at the end of the header."""
    header = open(os.path.join(os.path.dirname(rc.HERE), "include", "pivlfn.h")).read()
    names = re.findall(r"^(?:int|size_t)\s+(pivlfn_\w+)\(", header, re.M)
    first, last = names.index("pivlfn_stereo_2d3c"), names.index("pivlfn_create")
    analysis = [n for n in names[first:last] if not n.endswith("_workspace_bytes") and not n.endswith("_workspace_offset")]
    analysis += ["pivlfn_flow_uncertainty", "pivlfn_uncertainty_accumulate"]
    assert len(analysis) >= 35 and set(analysis[-2:]) <= set(names)
    assert sorted(rc.ENTRY_POINTS) == sorted(analysis)
    assert sorted(golden) == sorted(analysis)
    for name in analysis:
        assert sorted(golden[name]["cases"]) == sorted(label for label, _ in rc.ENTRY_POINTS[name][2]), name
        n = len(golden[name]["cases"])
        assert n >= 5 and len(golden[name]["order"]) == n * (n - 1) // 2, name


@pytest.mark.parametrize("name", sorted(rc.ENTRY_POINTS))
def test_every_refusal_keeps_its_code_its_text_and_its_place(name, golden):
    if rc.gpu_visible():
        pytest.skip("a GPU is visible: were a check lost, a call made of made-up pointers would reach a launch")
    from pivlfn import _lib
    got = rc.record(_lib.load(), name)
    want = golden[name]
    for label, (code, msg) in want["cases"].items():
        assert got["cases"][label] == [code, msg], f"{name} with {label}"
        assert code == 1
    labels = [label for label, _ in rc.ENTRY_POINTS[name][2]]
    pairs = [(a, b) for i, a in enumerate(labels) for b in labels[i + 1:]]
    wrong = [(a, b, w, g) for (a, b), w, g in zip(pairs, want["order"], got["order"]) if w != g]
    assert not wrong, f"{name}: with two bad arguments another check answers first (first, second, recorded, now): {wrong[:5]}"
