"""GPU: the parts of tests/test_gpu_ensemble.py that use side streams, graph capture and run.py -- the stream, capture and
pointer-offset contract of pivlfn_ensemble_corr through the helpers of tests/test_gpu_op_streams.py (the sums are accumulators there:
pre-loaded, read and written), and run.py --ensemble end to end.  Not collected by name: tests/test_gpu_ensemble.py runs this file in a
pytest process of its own, for the reason tests/test_gpu_flowmap.py gives."""
import json

import numpy as np
import pytest
import torch

import ensemble_restatement as er
from test_gpu_op_streams import I32, U8, Spec, _behind_the_delay, _check, _p, _same, delay  # noqa: F401

pytestmark = pytest.mark.gpu

I64 = torch.int64
H_, W_, B_ = 24, 40, 2                                    # H*W % 4 == 0
WINDOW, STEP, SEARCH = 8, 5, 2                            # 3 x 6 windows, 25 displacements each


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _spec(seed, with_offset):
    from pivlfn import _lib
    lib = _lib.load()
    rng = np.random.default_rng(11000 + seed)
    a, b = rng.integers(0, 256, (2, B_, H_, W_), dtype=np.uint8)
    ny, nx = er.grid(H_, W_, WINDOW, STEP, SEARCH)
    P = 2 * SEARCH + 1
    offset = np.random.default_rng(5).integers(-3, 4, (2, ny, nx)).astype(np.int32) if with_offset else None      # the same for every seed
    pre = np.random.default_rng(6).integers(-2 ** 40, 2 ** 40, (ny, nx, P, P, 3))
    pre_a = np.random.default_rng(7).integers(-2 ** 40, 2 ** 40, (ny, nx, 2))

    def call(i, o, acc, ws, st):
        return lib.pivlfn_ensemble_corr(_p(i[0]), _p(i[1]), _p(i[2]) if with_offset else None, _p(acc[0]), _p(acc[1]), B_, H_, W_, WINDOW, STEP,
                                        SEARCH, st)

    def pin(outs, accs):
        want, want_a = er.ensemble_corr(a, b, WINDOW, STEP, SEARCH, offset, pre, pre_a)
        assert torch.equal(accs[0].cpu(), _t(want)) and torch.equal(accs[1].cpu(), _t(want_a))
        if with_offset:
            out = er.outside(H_, W_, WINDOW, STEP, SEARCH, offset)
            assert out.any() and not out.all() and np.array_equal(want[out], pre[out])
    ins = [_t(a), _t(b)] + ([_t(offset)] if with_offset else [])
    return Spec(ins, [], [_t(pre), _t(pre_a)], [], call, pin, (H_, W_))


SPECS = {"ensemble_corr": lambda seed: _spec(seed, False), "ensemble_corr-offset": lambda seed: _spec(seed, True)}
OPS = list(SPECS)


@pytest.fixture()
def as_an_op(monkeypatch):
    """The helpers of test_gpu_op_streams look an op up by name: the names above resolve to the specs above."""
    import test_gpu_op_streams as ops
    original = ops._get
    monkeypatch.setattr(ops, "_get", lambda op, seed, quad=False: SPECS[op](seed) if op in SPECS else original(op, seed, quad))
    return ops


@pytest.mark.parametrize("op", OPS)
def test_eager_result_is_the_restatements(op, dev, as_an_op):
    src, outs, accs, _ = as_an_op._eager(op, 31, dev)
    spec = SPECS[op](31)
    for t, s in zip(src, spec.ins):
        assert _same(t.cpu(), s), f"{op}: an input was written"
    spec.pin(outs, accs)


@pytest.mark.parametrize("op", OPS)
def test_runs_in_order_on_the_stream_it_is_given(op, dev, delay, as_an_op):        # noqa: F811
    """On a side stream behind a long-running chain of matrix products and the copies of the real frames and the real sums into
    poisoned buffers, enqueued without a host synchronisation: the eager result, bit for bit, and every guard intact."""
    still_waiting, got, ref, buffers = _behind_the_delay(op, dev, delay, lambda stream: stream.cuda_stream)
    assert still_waiting, "the delay ran out before the op was enqueued: the test would not see a launch on another stream"
    for g, want in zip(got, ref):
        assert _same(g, want), f"{op}: the result behind a delay on a side stream differs from the eager result"
    for t in buffers:
        _check(t, op)


@pytest.mark.parametrize("op", OPS)
def test_is_graph_capturable(op, dev, as_an_op):
    """Captured and replayed three times with two input sets, the sums put back to their pre-loaded values before each replay: the
    eager bits.  An allocation or a host synchronisation inside the call would be a capture error."""
    as_an_op.test_op_is_graph_capturable(op, dev)


@pytest.mark.parametrize("op", OPS)
def test_pointers_one_element_off_give_the_same_bits(op, dev, as_an_op):
    """The frames one byte, the offsets four and the sums eight bytes into their allocations."""
    as_an_op.test_pointers_one_element_off_give_the_same_bits(op, dev)


# ---- run.py --------------------------------------------------------------------------------------------------------------------------
def test_run_py_ensemble(tmp_path, dev, capsys):
    """run.py --ensemble on five 96 x 96 synthetic pairs moved by (2.3, -1.6), --batch 2: ensemble.npz holds the restatement's sums of
    the frames as they were written to disk, ensemble.flo is the displacement lattice of its result (1e10 where flagged),
    ensemble.json the summary.  A second run, on pairs moved by (6.3, 3.4) with search 2 and a uniform (6.2, 3.3) field in the form of
    a stats.npz as the predictor, pre-shifts every window by (6, 3), leaves the last window column OUTSIDE and writes the comparison.
    Without --ensemble no such file appears and args.txt does not mention it."""
    import PIL.Image
    import run as runpy
    from pivlfn import ensemble as E
    from pivlfn.flo import read_flow
    H = W = 96
    a, b = er.particle_frames(5, H, W, (2.3, -1.6), 7)
    seq = tmp_path / "seq"
    seq.mkdir()
    for k in range(5):
        PIL.Image.fromarray(a[k]).save(str(seq / f"p{k}_img1.png"))
        PIL.Image.fromarray(b[k]).save(str(seq / f"p{k}_img2.png"))
    base = ["--model", "piv", "-i", str(seq), "-p", "--batch", "2"]
    assert runpy.main(base + ["-o", str(tmp_path / "plain")]) == 5
    assert runpy.main(base + ["-o", str(tmp_path / "ens"), "--ensemble", "--ensemble-search", "4"]) == 5
    assert "Ensemble correlation of 5 pairs: 16 of 16 windows" in capsys.readouterr().out
    plain, out = (tmp_path / d / "piv-synthetic" / "seq" for d in ("plain", "ens"))
    assert not list(plain.rglob("*ensemble*")) and not [ln for ln in open(plain / "args.txt") if ln.startswith("ensemble")]
    lines = list(open(out / "args.txt"))
    assert "ensemble: 32\n" in lines and "ensemble_step: None\n" in lines and "ensemble_search: 4\n" in lines
    for f in ("ensemble.npz", "ensemble.flo", "ensemble.json"):
        assert (out / f).is_file()
    want, want_a = er.ensemble_corr(a, b, 32, 16, 4)
    res = E.EnsembleResult.load(str(out / "ensemble.npz"))
    assert np.array_equal(res.sums, want) and np.array_equal(res.sums_a, want_a)
    assert (res.frames, res.window, res.step, res.search, res.H, res.W, res.ny, res.nx) == (5, 32, 16, 4, H, W, 4, 4)
    ref = E.finalize(want, want_a, 5, 32, 16)
    assert np.array_equal(res.displacement, ref.displacement) and not res.flag.any()
    assert np.abs(res.displacement - np.array([2.3, -1.6])[:, None, None]).max() < 0.05
    lattice = read_flow(str(out / "ensemble.flo"))
    assert lattice.shape == (4, 4, 2) and np.array_equal(lattice, res.displacement.astype(np.float32).transpose(1, 2, 0))
    with open(out / "ensemble.json") as f:
        doc = json.load(f)
    assert (doc["window"], doc["step"], doc["search"], doc["predictor"], doc["rows"], doc["columns"]) == (32, 16, 4, None, 4, 4)
    assert doc["summary"] == runpy.json_strict(res.summary()) and doc["summary"]["frames"] == 5 and "comparison" not in doc

    # with a predictor
    b2 = er.particle_frames(5, H, W, (6.3, 3.4), 7)[1]
    seq2 = tmp_path / "far" / "seq"
    seq2.mkdir(parents=True)
    for k in range(5):
        PIL.Image.fromarray(a[k]).save(str(seq2 / f"p{k}_img1.png"))
        PIL.Image.fromarray(b2[k]).save(str(seq2 / f"p{k}_img2.png"))
    mean = np.empty((2, H, W))
    mean[0], mean[1] = 6.2, 3.3
    np.savez(tmp_path / "predictor.npz", mean_u=mean[0], mean_v=mean[1])
    assert runpy.main(["--model", "piv", "-i", str(seq2), "-p", "--batch", "5", "-o", str(tmp_path / "pre"), "--ensemble", "32", "--ensemble-step",
                       "28", "--ensemble-search", "2", "--ensemble-predictor", str(tmp_path / "predictor.npz")]) == 5
    out = tmp_path / "pre" / "piv-synthetic" / "seq"
    res = E.EnsembleResult.load(str(out / "ensemble.npz"))
    ny, nx = er.grid(H, W, 32, 28, 2)
    offset = np.stack([np.full((ny, nx), 6, np.int32), np.full((ny, nx), 3, np.int32)])
    assert np.array_equal(res.offset, offset)
    outside = er.outside(H, W, 32, 28, 2, offset)
    want, want_a = er.ensemble_corr(a, b2, 32, 28, 2, offset)
    assert np.array_equal(res.sums, want) and np.array_equal(res.sums_a, want_a) and np.array_equal(res.outside, outside)
    assert outside.any() and np.array_equal(res.flag, np.where(outside, E.OUTSIDE, 0))
    assert np.nanmax(np.abs(res.displacement - np.array([6.3, 3.4])[:, None, None])) < 0.05
    lattice = read_flow(str(out / "ensemble.flo"))
    assert np.array_equal(lattice, np.where(outside, 1e10, res.displacement).astype(np.float32).transpose(1, 2, 0))
    with open(out / "ensemble.json") as f:
        doc = json.load(f)
    cmp_ = res.compare(mean)
    assert doc["comparison"] == {k: cmp_[k] for k in ("windows", "bias_u", "bias_v", "rms")} and doc["comparison"]["windows"] == int((~outside).sum())
    assert abs(doc["comparison"]["bias_u"] - 0.1) < 0.05 and abs(doc["comparison"]["bias_v"] - 0.1) < 0.05
