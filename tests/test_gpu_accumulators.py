"""GPU: what the streaming accumulators share (pivlfn/_accum.py).  The refusals of update() and the members of every save() file are those
recorded from the commit before the classes were given one base (tests/golden/accumulator_refusals.json, written by
tools/gen_accumulator_golden.py; the cases are tests/accumulator_cases.py), and an unindexed CUDA device is the current one in every class."""
import json
import os

import pytest
import torch

import accumulator_cases as cases
from conftest import GOLD

pytestmark = pytest.mark.gpu
TENSORS = {"MaskedFlowStats": ("acc", "cnt"), "FlowDistribution": ("acc", "hist"), "FrameBackground": ("min",)}     # the others: acc


def _recorded(part):
    return json.load(open(os.path.join(GOLD, "accumulator_refusals.json")))[part]


def test_update_refusals_are_those_recorded(dev):
    """Frames of 8 x 10 for accumulators of 8 x 9, a mask or a mean of another shape: type and text, on an indexed device as recorded.
    Nothing is launched."""
    want, got = _recorded("update"), cases.update_cases(dev)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key
    assert all(v is not None and v["type"] == "ValueError" for v in want.values())


def test_save_files_have_the_recorded_members(dev, tmp_path):
    """After one update() of two frames: the file name save() returns for a path without suffix, and name, dtype and shape of every
    member."""
    want, got = _recorded("save"), cases.save_members(dev, tmp_path)
    assert sorted(got) == sorted(want) == sorted(cases.SAVED)
    for key in want:
        assert got[key] == want[key], key


@pytest.mark.parametrize("name", cases.SIZED)
def test_an_unindexed_cuda_device_is_the_current_one(dev, name):
    """device="cuda" with tensors on the current indexed device.  Before the classes shared their constructor head the seven H x W
    accumulators kept the device as given, torch.device("cuda") != torch.device("cuda:0"), and this update() raised ValueError
    ("flows ... on cuda:0, accumulators ... on cuda").  Now it accumulates the bits of an object made with the indexed device."""
    with torch.cuda.device(dev):
        loose, exact = cases.make(name, device="cuda"), cases.make(name, device=dev)
        assert loose.device == exact.device == dev and loose.device.index is not None
        for acc in (loose, exact):
            acc.update(*cases.frames(name, dev, mask_w=None if name == "FlowStats" else cases.W, seed=3))
        assert loose.count == exact.count == cases.B
        for attr in TENSORS.get(name, ("acc",)):
            a, b = getattr(loose, attr), getattr(exact, attr)
            assert a.device == dev and torch.equal(a, b) and bool(a.ne(0).any()), attr
