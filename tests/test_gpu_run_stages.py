"""GPU: the files one feature of run.py writes do not depend on which other features ran beside it.  run.py makes every further
output a stage of one flat list behind a single forward (Validate, Stats, Truth, Pictures, Quality, Pod); each feature alone is
pinned against the library by its own test file, and here a run with many stages is compared, file for file, with runs that have
one group of them."""
import json
import os

import numpy as np
import pytest

from pivlfn import synth
from pivlfn.flo import write_flow

pytestmark = pytest.mark.gpu

VALIDATE = ["--validate-radius", "2", "--validate-eps", "0.01", "--validate-thresh", "0.5"]


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    """Three 64 x 64 particle pairs (64: the smallest size --truth-levels takes that still has a 2 x 2 level-6 map) and their true
    fields: (image directory, truth directory)."""
    import PIL.Image
    root = tmp_path_factory.mktemp("stages")
    seq, tr = root / "seq", root / "truth"
    seq.mkdir()
    tr.mkdir()
    for k in range(3):
        a, b, true = synth.particle_pair(64, 64, 900 + k)
        PIL.Image.fromarray(a).save(str(seq / f"p{k}_img1.png"))
        PIL.Image.fromarray(b).save(str(seq / f"p{k}_img2.png"))
        write_flow(np.ascontiguousarray(true.transpose(1, 2, 0)), str(tr / f"p{k}_flow.flo"))
    return str(seq), str(tr)


def _run(pairs, out, flags):
    """run.py -p --batch 2 (a batch of two and one of one: the per-batch records get concatenated) -> {relative path: full path}
    of every file written."""
    import run as runpy
    assert runpy.main(["--model", "piv", "-i", pairs[0], "-p", "--batch", "2", "-o", str(out)] + flags) == 3
    save = os.path.join(str(out), "piv-synthetic", "seq")
    return {os.path.relpath(os.path.join(d, f), save): os.path.join(d, f) for d, _, files in os.walk(save) for f in files}


def _same_file(a, b):
    """.npz key for key (the zip container carries a timestamp), everything else byte for byte."""
    if a.endswith(".npz"):
        x, y = np.load(a), np.load(b)
        return sorted(x.files) == sorted(y.files) and all(x[k].dtype == y[k].dtype and np.array_equal(x[k], y[k], equal_nan=x[k].dtype.kind == "f")
                                                          for k in x.files)
    with open(a, "rb") as f, open(b, "rb") as g:
        return f.read() == g.read()


def _check_subset(part, whole, expect):
    """Every file of the single-group run, args.txt apart (it lists the flags), is in the combined run and equal there."""
    names = sorted(n for n in part if n != "args.txt")
    print(len(names), "files compared:", names)
    assert set(expect) <= set(names), sorted(set(expect) - set(names))
    for n in names:
        assert n in whole, n
        assert _same_file(part[n], whole[n]), n


def _quiver():
    from pivlfn import viz
    try:
        viz._pyplot()
    except ImportError:
        return []
    return ["--quiver"]


def test_a_stage_writes_the_same_files_alone_and_beside_the_others_under_mask(pairs, tmp_path, dev):
    mask = ["--validate", "mask"] + VALIDATE
    quiver = _quiver()
    groups = {"stats": (["--stats"], ["stats.npz"]),
              "truth": (["--truth", pairs[1], "--truth-levels"], ["errors.json", "error_maps.npz"]),
              "pictures": (["--color", "--vort-image"] + quiver,
                           ["flow/color_wheel.png", "flow/p0_out.png", "flow/p2_vort.png"] + (["flow/p1_quiver.png"] if quiver else [])),
              "quality": (["--quality", "4", "--quality-image"], ["quality.json", "flow/p0_qual.flo", "flow/p2_corr.png"])}
    whole = _run(pairs, tmp_path / "all", mask + [f for flags, _ in groups.values() for f in flags])
    with open(whole["validation.json"]) as f:
        assert json.load(f)["total"]["outlier"] > 0             # the mask is not empty: the stages do see rejected vectors
    for name, (flags, expect) in groups.items():
        part = _run(pairs, tmp_path / name, mask + flags)
        _check_subset(part, whole, expect + ["validation.json"] + [f"flow/p{k}_out.flo" for k in range(3)])


def test_a_stage_writes_the_same_files_alone_and_beside_the_others_under_replace(pairs, tmp_path, dev):
    """POD joins here only: under "mask" an 8 x 8 cell may legitimately be refused as empty (test_gpu_pod.py covers that)."""
    rep = ["--validate", "replace"] + VALIDATE
    whole = _run(pairs, tmp_path / "all", rep + ["--stats", "--truth", pairs[1], "--color", "--quality", "4", "--pod", "2", "--pod-cell", "8"])
    flows = ["validation.json"] + [f"flow/p{k}_out.flo" for k in range(3)]
    part = _run(pairs, tmp_path / "pod", rep + ["--pod", "2", "--pod-cell", "8", "--color"])
    _check_subset(part, whole, flows + ["pod.npz", "pod_mode1.png", "pod_mode2.png", "flow/color_wheel.png", "flow/p1_out.png"])
    part = _run(pairs, tmp_path / "rest", rep + ["--stats", "--truth", pairs[1], "--quality", "4"])
    _check_subset(part, whole, flows + ["stats.npz", "errors.json", "error_maps.npz", "quality.json", "flow/p2_qual.flo"])
