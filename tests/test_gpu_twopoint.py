"""GPU: pivlfn_twopoint_accumulate (csrc/twopoint.hip) against the NumPy restatement of its contract (tests/twopoint_restatement.py).
Every operation of the contract is a correctly rounded fp64 operation in a fixed order, so the accumulators are compared bit for bit,
every element of them, and the counts exactly.  Shapes: rows of one pixel and images smaller than most separations, widths just over a
power of two (the tree is mostly padding) and over one 256-column pass of a wave, separations past half the row and past the edge;
the shapes of tests/analysis_plans.py with several separations a wave and with 4, 8 and 64 chunks a row.
Then how a sequence is cut into calls, the stream and capture contract as tests/test_gpu_op_streams.py holds the other entry points to
it (its helpers, imported), guarded buffers, the refusals, TwoPointStats on the DNS fixture and run.py --twopoint."""
import json
import os

import numpy as np
import pytest
import torch

import twopoint_restatement as tr
from guarded import check_guards, guarded
from test_gpu_op_streams import (F32, F64, U8, Spec, _behind_the_delay, _buf, _check, _p, _poisoned, _same, _scribble, delay)  # noqa: F401
from test_gpu_vortex import _close

pytestmark = pytest.mark.gpu


def _dev(dev, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _run(dev, flow, mask, mean, acc0, R, step, cuts=None):
    """acc0 and the frames of `flow` through the C entry point, one call per entry of `cuts` (default: one call for all): the new acc."""
    from pivlfn import _lib
    lib = _lib.load()
    B, _, H, W = flow.shape
    f, m, mu, acc = _dev(dev, flow), _dev(dev, mask), _dev(dev, mean), _dev(dev, acc0)
    assert acc.shape == (2, R + 1, 15, H) and acc.dtype == torch.float64
    at = 0
    for n in cuts or [B]:
        _lib.check(lib.pivlfn_twopoint_accumulate(f[at:].data_ptr(), m[at:].data_ptr() if m is not None else None, _p(mu), acc.data_ptr(), n, H, W,
                                                  R, step, torch.cuda.current_stream(dev).cuda_stream), "twopoint_accumulate")
        at += n
    assert at == B
    return acc.cpu().numpy()


def _compare(got, want, what):
    """Every element bit for bit; the counts are integers."""
    same = got.view(np.int64) == want.view(np.int64)
    if not same.all():
        at = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {np.count_nonzero(~same)} of {same.size} sums differ, first at [d, r, term, y] = {at}: {got[at]!r} against {want[at]!r}")


def _case(B, H, W, seed):
    """Flows with a mask, holes and a mean.  Images of fewer than 40 vectors get their invalid vectors by hand: frame 1 loses one."""
    rng = np.random.default_rng(seed)
    flow, mask, mean = tr.random_case(rng, B, H, W, holes=H * W >= 40)
    if H * W < 40:
        flow[1, 0, H // 2, W // 2] = np.nan
        mask[:] = 0
        mask[2, H - 1, W - 1] = 7
    return flow, mask, mean


SHAPES = [(1, 1, 8, 1), (1, 7, 8, 1), (7, 1, 8, 1), (5, 3, 2, 1), (37, 53, 5, 1), (37, 53, 5, 3), (70, 131, 16, 1), (33, 257, 64, 1),
          (20, 300, 255, 1), (40, 64, 4, 16)]


@pytest.mark.parametrize("with_mean", [False, True], ids=["nomean", "mean"])
@pytest.mark.parametrize("with_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("H,W,R,step", SHAPES)
def test_bits_of_the_restatement(H, W, R, step, with_mask, with_mean, dev):
    """B = 3 in one call from a non-zero acc.  1 x 1, 1 x 7, 7 x 1: most separations have no pair and leave acc as it was; 70 x 131 and
    33 x 257: one and two 256-column passes, the second all padding but one column; 20 x 300 at R = 255: separations past half the row and,
    down the column, past the image from r = 20; 40 x 64 at step 16: the partner is past the edge from r = 4 along x and r = 3 along y."""
    flow, mask, mean = _case(3, H, W, 100 * H + W + R)
    mask, mean = mask if with_mask else None, mean if with_mean else None
    acc0 = np.random.default_rng(5).normal(0, 50, (2, R + 1, 15, H))
    want = tr.accumulate(flow, mask, mean, acc0, R, step)
    got = _run(dev, flow, mask, mean, acc0, R, step)
    _compare(got, want, f"{H}x{W} R={R} step={step}")
    fresh = tr.accumulate(flow, mask, mean, np.zeros_like(acc0), R, step)              # from zeros the counts are plain integers
    assert np.array_equal(_run(dev, flow, mask, mean, np.zeros_like(acc0), R, step)[:, :, 0], fresh[:, :, 0])
    assert (fresh[:, :, 0] == np.round(fresh[:, :, 0])).all()
    assert fresh[0, 0, 0].sum() < 3 * H * W and fresh[0, 0, 0].max() > 0, "the case must exclude some pairs and keep some"
    gone = fresh[:, :, 0].sum(-1) == 0
    if gone.any():                                                          # separations without a pair: every term stays what it was
        assert np.array_equal(got[gone].view(np.int64), acc0[gone].view(np.int64))


def _plan_shapes():
    import analysis_plans as ap
    return ap.shapes(ap.TWOPOINT_CASES)


@pytest.mark.parametrize("with_mean", [False, True], ids=["nomean", "mean"])
@pytest.mark.parametrize("with_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("H,W,R,step", _plan_shapes())
def test_bits_where_the_plan_changes(H, W, R, step, with_mask, with_mean, dev):
    """B = 2 in one call from a non-zero acc, at the shapes of tests/analysis_plans.py.  66 x 300 at R = 255: two separations a wave in
    LDS; 4096 x 5: 64 of them, the largest LDS request, and one workgroup per row and direction; 1024 x 40 at R = 64: z = 4 and 5 slots
    as at 1024 x 1024; rows of 520, 1030 and 16384 columns: 4, 8 and 64 chunks of 256, joined by the counter up to its last register."""
    import analysis_plans as ap
    plan = ap.twopoint(H, W, R)
    assert plan["slots"] >= 2 or plan["chunks"] >= 4
    flow, mask, mean = _case(2, H, W, 100 * H + W + R)
    mask, mean = mask if with_mask else None, mean if with_mean else None
    acc0 = np.random.default_rng(5).normal(0, 50, (2, R + 1, 15, H))
    want = tr.accumulate(flow, mask, mean, acc0, R, step)
    got = _run(dev, flow, mask, mean, acc0, R, step)
    _compare(got, want, f"{H}x{W} R={R} step={step}")
    pairs = (want[:, :, 0] - acc0[:, :, 0]).sum(-1)                               # about the number of pairs of a separation
    assert pairs[0, 0] < 2 * H * W - 0.5 and pairs[0, min(R, (W - 1) // step)] > 0.5, "the case must exclude some pairs and keep some"
    gone = (want[:, :, 0] == acc0[:, :, 0]).all(-1)
    assert np.array_equal(got[gone].view(np.int64), acc0[gone].view(np.int64))      # separations without a pair: as they were
    if plan["slots"] >= 2:
        assert not gone[0, :min(R, (W - 1) // step) + 1].any() and not gone[1, :min(R, (H - 1) // step) + 1].any()


def test_cutting_the_sequence_changes_no_bit_with_two_slots_a_wave(dev):
    """66 x 300 at R = 255 (two separations a wave kept in LDS across the frames of a call): B = 2 in one call and in two."""
    H, W, R, step = 66, 300, 255, 1
    flow, mask, mean = _case(2, H, W, 78)
    flow[1] += np.float32(5.0)
    acc0 = np.random.default_rng(6).normal(0, 50, (2, R + 1, 15, H))
    whole = _run(dev, flow, mask, mean, acc0, R, step)
    _compare(_run(dev, flow, mask, mean, acc0, R, step, [1, 1]), whole, "cuts [1, 1]")
    _compare(whole, tr.accumulate(flow, mask, mean, acc0, R, step), "66x300 R=255")


def test_minus_zero_survives_where_the_tree_has_no_padding_to_add(dev):
    """Rows of -0.0: the root of a full tree (W = 1, 2, 4) is -0.0 in the first-order terms, one with padding (W = 3) is +0.0."""
    for W in (1, 2, 3, 4):
        flow = np.full((1, 2, 2, W), -0.0, np.float32)
        acc0 = np.full((2, 2, 15, 2), -0.0)
        want = tr.accumulate(flow, None, None, acc0, 1, 1)
        _compare(_run(dev, flow, None, None, acc0, 1, 1), want, f"-0.0, W={W}")
        assert np.signbit(want[0, 0, 1, 0]) == (W != 3)


# ---- how the sequence is cut ----------------------------------------------------------------------------------------------------------
def test_cutting_the_sequence_into_calls_changes_no_bit(dev):
    """B = 3 in one call, three calls of one frame and 2 + 1, each from the same non-zero acc (the read-modify-write); twice (run to
    run); an all-zero mask gives the bits of the NULL mask."""
    H, W, R, step = 37, 53, 5, 2
    flow, mask, mean = _case(3, H, W, 77)
    flow[1] *= 0.01
    flow[2] += np.float32(5.0)
    acc0 = np.random.default_rng(6).normal(0, 50, (2, R + 1, 15, H))
    want = tr.accumulate(flow, mask, mean, acc0, R, step)
    for cuts in ([3], [1, 1, 1], [2, 1], [3]):
        _compare(_run(dev, flow, mask, mean, acc0, R, step, cuts), want, f"cuts {cuts}")
    open_mask = _run(dev, flow, np.zeros_like(mask), mean, acc0, R, step)
    _compare(open_mask, _run(dev, flow, None, mean, acc0, R, step), "all-zero mask")
    assert not tr.same_bits(open_mask, want)


# ---- the stream and capture contract, with the helpers of tests/test_gpu_op_streams.py ------------------------------------------------
def _spec(seed, quad=False):
    """2 x 40 x 56 (H*W % 4 == 0), R = 6, step 2, with a mask and a mean, from a non-zero acc."""
    from pivlfn import _lib
    lib = _lib.load()
    B, H, W, R, step = 2, 40, 56, 6, 2
    flow, mask, mean = _case(B, H, W, 2000 + seed)
    acc0 = np.random.default_rng(3).normal(0, 50, (2, R + 1, 15, H))

    def call(i, o, a, ws, st):
        return lib.pivlfn_twopoint_accumulate(_p(i[0]), _p(i[1]), _p(i[2]), _p(a[0]), B, H, W, R, step, st)

    def pin(accs):
        assert tr.same_bits(accs[0].cpu().numpy(), tr.accumulate(flow, mask, mean, acc0, R, step))
    return Spec([torch.from_numpy(flow), torch.from_numpy(mask), torch.from_numpy(mean)], [], [torch.from_numpy(acc0)], [], call, pin, (H, W))


@pytest.fixture()
def as_an_op(monkeypatch):
    """The helpers of test_gpu_op_streams look an op up by name: "twopoint_accumulate" resolves to the spec above."""
    import test_gpu_op_streams as ops
    original = ops._get
    monkeypatch.setattr(ops, "_get", lambda op, seed, quad=False: _spec(seed, quad) if op == "twopoint_accumulate" else original(op, seed, quad))
    return ops


def test_eager_result_is_the_restatements(dev, as_an_op):
    _, _, accs, _ = as_an_op._eager("twopoint_accumulate", 31, dev)
    _spec(31).pin(accs)


def test_runs_in_order_on_the_stream_it_is_given(dev, delay, as_an_op):        # noqa: F811
    """On a side stream behind a long-running chain of matrix products and the copies of the real inputs into poisoned buffers,
    enqueued without a host synchronisation: the eager result, bit for bit, and every guard intact."""
    still_waiting, got, ref, buffers = _behind_the_delay("twopoint_accumulate", dev, delay, lambda stream: stream.cuda_stream)
    assert still_waiting, "the delay ran out before the op was enqueued: the test would not see a launch on another stream"
    for g, want in zip(got, ref):
        assert _same(g, want), "the result behind a delay on a side stream differs from the eager result"
    for t in buffers:
        _check(t, "twopoint_accumulate")


def test_is_graph_capturable(dev, as_an_op):
    as_an_op.test_op_is_graph_capturable("twopoint_accumulate", dev)


def test_pointers_one_element_off_give_the_same_bits(dev, as_an_op):
    as_an_op.test_pointers_one_element_off_give_the_same_bits("twopoint_accumulate", dev)


@pytest.mark.parametrize("W,R,step", [(46, 7, 1), (258, 3, 16)])
def test_guarded_buffers(W, R, step, dev):
    """acc between guards, guards behind flow, mask and mean (and in front of them): every guard intact, no input written, the bits of
    the unguarded call.  38 x 46: the last lanes of a pass own no column; 38 x 258 at step 16: a second pass of two columns."""
    from pivlfn import _lib
    lib = _lib.load()
    B, H = 2, 38                                       # B*H*W a multiple of 4: the byte buffer is whole 32-bit words
    flow, mask, mean = _case(B, H, W, 600 + W)
    acc0 = np.random.default_rng(7).normal(0, 50, (2, R + 1, 15, H))
    src = [torch.from_numpy(x).to(dev) for x in (flow, mask, mean, acc0)]
    bufs = [guarded(t.shape, t.dtype, dev, "nan") for t in src]
    for t, x in zip(bufs, src):
        t.copy_(x)
    _lib.check(lib.pivlfn_twopoint_accumulate(_p(bufs[0]), _p(bufs[1]), _p(bufs[2]), _p(bufs[3]), B, H, W, R, step,
                                              torch.cuda.current_stream(dev).cuda_stream), "twopoint_accumulate")
    torch.cuda.synchronize()
    _compare(bufs[3].cpu().numpy(), _run(dev, flow, mask, mean, acc0, R, step), f"guarded 38x{W}")
    _compare(bufs[3].cpu().numpy(), tr.accumulate(flow, mask, mean, acc0, R, step), f"guarded 38x{W} against the restatement")
    for t in bufs:
        check_guards(t, f"twopoint_accumulate 38x{W}")
    for t, x in zip(bufs[:3], src[:3]):
        assert torch.equal(t.view(torch.uint8), x.view(torch.uint8)), "an input was written"


def test_every_error_is_refused_before_any_launch(dev):
    """The refusals of tests/test_twopoint.py with real device buffers: acc and everything else keep every byte."""
    from pivlfn import _lib
    from test_twopoint import refusals
    lib = _lib.load()
    arena = _scribble(torch.empty(4 << 16, dtype=torch.uint8, device=dev))      # four regions 64 KiB apart: only what a case moves overlaps
    flow, mask, mean, acc = (arena.data_ptr() + (i << 16) for i in range(4))
    assert arena.data_ptr() % 8 == 0
    refusals(lib, flow, mask, mean, acc, 2, 8, 8)
    torch.cuda.synchronize()
    assert bool((arena == 0xFF).all())


# ---- the Python class ------------------------------------------------------------------------------------------------------------------
def test_twopoint_stats_on_the_dns_fixture(dev, tmp_path):
    """tests/golden/DNS_turbulence_flow.flo, 256 x 256, R = 64: acc equals the restatement's bits, rho(0) = 1 on every row with pairs,
    summary() agrees with the restatement's derived values, and save() writes what result() holds."""
    from conftest import GOLD
    from pivlfn import TwoPointStats
    flow = tr.read_flo(os.path.join(GOLD, "DNS_turbulence_flow.flo"))[None]
    assert flow.shape == (1, 2, 256, 256)
    tp = TwoPointStats(256, 256, 64, device=dev)
    tp.update(torch.from_numpy(flow).to(dev))
    assert tp.count == 1 and tp.acc.shape == (2, 65, 15, 256)
    want = tr.accumulate(flow, None, None, np.zeros((2, 65, 15, 256)), 64, 1)
    _compare(tp.acc.cpu().numpy(), want, "DNS R=64")
    res = tp.result()
    for which in ("uu", "vv"):
        for axis in ("x", "y"):
            c = res.correlation(which, axis)
            have = c.n[0] > 0
            assert have.all() and np.abs(c.rho[0][have] - 1.0).max() <= 4e-12
    got, ref = res.summary(), tr.summary(want, 1, 1)
    assert _close(got, ref), (got, ref)
    assert all(2.0 < got[k]["integral_scale"] < 64.0 and 0 < got[k]["taylor_microscale"] < 64.0 for k in ("uu_x", "uu_y", "vv_x", "vv_y")), got
    with np.load(tp.save(str(tmp_path / "tp"))) as f:
        assert tr.same_bits(f["acc"], want) and int(f["frames"]) == 1 and int(f["max_sep"]) == 64 and np.array_equal(f["sep"], np.arange(65.0))
        assert np.array_equal(f["rho_uu_x"], res.pooled("uu", "x").rho) and np.array_equal(f["d_ll_y"], res.structure(2, "L", "y", rows=slice(None)))


def test_twopoint_stats_update_mean_and_checks(dev, tmp_path):
    """Two update() calls equal one; a mask of bools; the mean as a tensor, an array and a FlowStats file give the same bits, which are
    the restatement's; wrong sizes and types are refused."""
    from pivlfn import TwoPointStats
    from pivlfn.postpro import FlowStats
    B, H, W, R, step = 4, 21, 45, 6, 2
    flow, mask, _ = _case(B, H, W, 88)
    flow = np.nan_to_num(flow, nan=0.5, posinf=1.0, neginf=-1.0)
    flow[np.abs(flow) > 1e9] = 2.0                     # FlowStats has no notion of an invalid vector
    f, m = torch.from_numpy(flow).to(dev), torch.from_numpy(mask).to(dev)
    stats = FlowStats(H, W, device=dev)
    stats.update(f)
    path = stats.save(str(tmp_path / "stats"))
    mean = np.stack([stats.result()["mean_u"], stats.result()["mean_v"]])
    want = tr.accumulate(flow, mask, mean, np.zeros((2, R + 1, 15, H)), R, step)
    for given in (path, mean, torch.from_numpy(mean), torch.from_numpy(mean).to(dev)):
        tp = TwoPointStats(H, W, R, step, mean=given, device=dev)
        tp.update(f[:3], m[:3] != 0)
        tp.update(f[3:], m[3:])
        tp.update(f[:0])
        assert tp.count == 4
        _compare(tp.acc.cpu().numpy(), want, f"mean given as {type(given).__name__}")
    with pytest.raises(ValueError, match="mean"):
        TwoPointStats(H, W, R, step, mean=mean[:, :-1], device=dev)
    with pytest.raises(ValueError, match="accumulators"):
        tp.update(f[:, :, :-1])
    with pytest.raises(TypeError):
        tp.update(f.double())
    with pytest.raises(ValueError, match="max_sep"):
        TwoPointStats(H, W, 256, device=dev)


# ---- run.py --------------------------------------------------------------------------------------------------------------------------
def test_run_py_twopoint(tmp_path, dev, capsys):
    """run.py -p --twopoint 8 on three synthetic 64 x 64 pairs, alone and with --validate flag beside --stats: twopoint.npz holds the
    accumulators of a TwoPointStats fed the written flows (with the validation flags as the mask), bit for bit; twopoint.json the
    parameters, the validation mode and summary(); stats.npz is written beside it as without --twopoint; the sharded run is refused."""
    import PIL.Image
    import run as runpy
    from pivlfn import TwoPointStats, synth
    from pivlfn import validate as V
    from pivlfn.flo import read_flow
    H = W = 64
    seq = tmp_path / "seq"
    seq.mkdir()
    names = [f"p{k}" for k in range(3)]
    for k, name in enumerate(names):
        a, b, _ = synth.particle_pair(H, W, 950 + k)
        PIL.Image.fromarray(a).save(str(seq / f"{name}_img1.png"))
        PIL.Image.fromarray(b).save(str(seq / f"{name}_img2.png"))
    base = ["--model", "piv", "-i", str(seq), "-p", "--batch", "2"]
    val = ["--validate", "flag", "--validate-radius", "2", "--validate-eps", "0.01", "--validate-thresh", "0.5"]
    assert runpy.main(base + ["-o", str(tmp_path / "alone"), "--twopoint", "8"]) == 3
    assert "integral scales in pixels uu_x" in capsys.readouterr().out
    assert runpy.main(base + val + ["-o", str(tmp_path / "both"), "--twopoint", "8", "--twopoint-step", "2", "--stats"]) == 3
    assert runpy.main(base + val + ["-o", str(tmp_path / "stats"), "--stats"]) == 3
    alone, both, stats = (tmp_path / d / "piv-synthetic" / "seq" for d in ("alone", "both", "stats"))
    assert not (stats / "twopoint.npz").exists() and not [ln for ln in open(stats / "args.txt") if ln.startswith("twopoint")]
    assert "twopoint: 8\n" in list(open(alone / "args.txt")) and "twopoint_step: 2\n" in list(open(both / "args.txt"))
    with np.load(stats / "stats.npz") as a, np.load(both / "stats.npz") as b:
        assert sorted(a.files) == sorted(b.files) and all(a[k].tobytes() == b[k].tobytes() for k in a.files)
    for out, step, mode in ((alone, 1, None), (both, 2, "flag")):
        flows = torch.stack([torch.from_numpy(read_flow(str(out / "flow" / f"{n}_out.flo"))).permute(2, 0, 1) for n in names]).contiguous().to(dev)
        flags = V.validate_flow(flows, radius=2, spacing=1, eps=0.01, thresh=0.5, mode="flag").flag if mode else None
        tp = TwoPointStats(H, W, 8, step, device=dev)
        tp.update(flows, flags)
        with np.load(out / "twopoint.npz") as f:
            _compare(f["acc"], tp.acc.cpu().numpy(), f"run.py --twopoint 8, step {step}")
            assert int(f["frames"]) == 3 and int(f["step"]) == step and (str(f["validation"]) == "flag" if mode else "validation" not in f.files)
        doc = json.load(open(out / "twopoint.json"))
        assert (doc["max_sep"], doc["step"], doc["mean"], doc["validation"]) == (8, step, None, mode)
        assert _close(doc["summary"], runpy.json_strict(tp.result().summary())), (doc["summary"], tp.result().summary())
        if mode:
            assert tp.result().acc[0, 0, 0].sum() < 3 * H * W                  # the validator did flag vectors
    os.environ["WORLD_SIZE"] = "2"
    try:
        with pytest.raises(SystemExit, match="--twopoint needs a single process"):
            runpy.main(base + ["-o", str(tmp_path / "sharded"), "--twopoint", "8"])
    finally:
        del os.environ["WORLD_SIZE"]
    assert not (tmp_path / "sharded").exists()
