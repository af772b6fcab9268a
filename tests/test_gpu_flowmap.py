"""GPU: pivlfn_flowmap_advect, pivlfn_flowmap_seed and pivlfn_flowmap_ftle (csrc/flowmap.hip) against the NumPy restatement of
their contract (tests/flowmap_restatement.py).  Every operation of the contract is a correctly rounded fp64 operation in a fixed
order, so positions, flags, traces, stretch and oflag are compared bit for bit, NaN positions included, and no particle is left out.
Shapes: the smallest image (2 x 2, every sample in the clamped last cell), 2 x 9, and 37 x 53 -- five blocks of 256 particles and a
ragged tail -- at spacings 1, 2 and 5 (5 does not divide the image).  Then particle lists, batch splitting, the FTLE, guarded and
scribbled buffers and the refusals, all on the default stream; the stream and capture contract as tests/test_gpu_op_streams.py holds
the other entry points to it (its helpers, imported) and run.py --ftle are in tests/flowmap_stream_cases.py, which the last test here
runs in a process of its own."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import flowmap_restatement as fr
from flowmap_restatement import LOST, OUT, UNDEFINED
from flowmap_stream_cases import B, _fields, _state, _t
from guarded import check_guards, guarded
from test_gpu_op_streams import _p, _same, _scribble

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 1), (2, 9, 1), (37, 53, 1), (37, 53, 2), (37, 53, 5)]


def _same_state(fm, pos, flag, what):
    got_pos, got_flag = fm.positions.reshape(2, -1).cpu().numpy(), fm.flag.reshape(-1).cpu().numpy()
    assert np.array_equal(got_flag, flag), f"{what}: {np.count_nonzero(got_flag != flag)} flag bytes differ, first at {np.argwhere(got_flag != flag)[0]}"
    same = got_pos.view(np.int64) == pos.view(np.int64)
    if not same.all():
        at = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {np.count_nonzero(~same)} coordinates differ, first {at}: {got_pos[at]!r} against {pos[at]!r}")


@pytest.mark.parametrize("holes", [False, True], ids=["plain", "holes"])
@pytest.mark.parametrize("H,W,spacing", SHAPES)
def test_bits_of_the_restatement(H, W, spacing, holes, dev):
    """Forward through B = 7 plane-wave fields in one launch: every particle's position and flag and the whole trace.  At 37 x 53 most
    particles stay live and the others go OUT (through all four sides: tests/test_flowmap.py); with a mask and NaN, -inf and 1e10
    vectors, LOST occurs too."""
    from pivlfn import FlowMap
    flows, mask = _fields(H, W, holes)
    pos0, h, w = fr.lattice(H, W, spacing)
    pos, flag, path = fr.advect(flows, mask, pos0, np.zeros(h * w, np.uint8), trace=True)
    fm = FlowMap(H, W, spacing, device=dev)
    assert (fm.h, fm.w, fm.steps) == (h, w, 0) and fm.positions.shape == (2, h, w) and fm.flag.shape == (h, w)
    _same_state(fm, pos0, np.zeros(h * w, np.uint8), "the seeds")
    got = fm.update(_t(flows, dev), _t(mask, dev), trace=True)
    assert fm.steps == B and got.shape == (B, 2, h, w) and got.dtype == torch.float64
    _same_state(fm, pos, flag, f"{H}x{W} s={spacing}")
    assert fr.same_bits(got.cpu().numpy().reshape(B, 2, -1), path), "the trace differs"
    if (H, W) == (37, 53):
        assert (flag == 0).any() and (flag == OUT).any()
        assert (flag == LOST).any() if holes else 0.8 < (flag == 0).mean() < 0.9        # a masked vector costs up to four cells, seven times over
    fm.reset()
    assert fm.steps == 0
    _same_state(fm, pos0, np.zeros(h * w, np.uint8), "the seeds after reset()")
    assert fm.update(_t(flows, dev), _t(mask, dev)) is None                      # without a trace: the same state
    _same_state(fm, pos, flag, f"{H}x{W} s={spacing} without a trace")


@pytest.mark.parametrize("iters", [1, 8])
@pytest.mark.parametrize("H,W,spacing", SHAPES)
def test_backward_bits_of_the_restatement(H, W, spacing, iters, dev):
    """backward=True, with the holes and the mask: every fixed-point iteration is a sample that may set a flag."""
    from pivlfn import FlowMap
    flows, mask = _fields(H, W, True, seed=12)
    pos0, h, w = fr.lattice(H, W, spacing)
    pos, flag, path = fr.advect(flows, mask, pos0, np.zeros(h * w, np.uint8), backward=True, iters=iters, trace=True)
    fm = FlowMap(H, W, spacing, backward=True, iters=iters, device=dev)
    got = fm.update(_t(flows, dev), _t(mask, dev), trace=True)
    _same_state(fm, pos, flag, f"backward {H}x{W} s={spacing} iters={iters}")
    assert fr.same_bits(got.cpu().numpy().reshape(B, 2, -1), path), "the trace differs"
    if (H, W) == (37, 53):
        assert (flag == 0).any() and (flag == OUT).any() and (flag == LOST).any()


def _points(n, H, W):
    """Integer nodes, the last row and column (the ix / iy clamp), the corners, a hair inside and outside every side, NaN, then
    random points in and around the image."""
    eps = 2.0 ** -40
    fixed = [(0.0, 0.0), (W - 1.0, H - 1.0), (W - 1.0, 3.0), (5.0, H - 1.0), (W - 2.0, H - 2.0), (7.0, 11.0), (W - 1.0 + eps, 4.0),
             (4.0, H - 1.0 + eps), (-eps, 4.0), (4.0, -eps), (W - 1.0 - eps, H - 1.0 - eps), (math.nan, 3.0), (3.0, math.inf), (-0.0, 2.5)]
    rng = np.random.default_rng(n)
    rest = np.stack([rng.uniform(-3, W + 2, max(n - len(fixed), 0)), rng.uniform(-3, H + 2, max(n - len(fixed), 0))], axis=1)
    return np.concatenate([np.array(fixed, np.float64).reshape(-1, 2), rest])[:n]


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("n", [0, 1, 257])
def test_particle_lists(n, backward, dev):
    from pivlfn import FlowMap
    H, W = 37, 53
    flows, mask = _fields(H, W, True, seed=13)
    pts = _points(n, H, W)
    pos, flag, path = fr.advect(flows, mask, pts.T.copy(), np.zeros(n, np.uint8), backward=backward, iters=8, trace=True)
    fm = FlowMap(H, W, points=torch.from_numpy(pts), backward=backward, device=dev)
    assert fm.positions.shape == (2, n) and fm.flag.shape == (n,)
    got = fm.update(_t(flows, dev), _t(mask, dev), trace=True)
    assert got.shape == (B, 2, n) and fm.steps == B
    _same_state(fm, pos, flag, f"{n} points")
    assert fr.same_bits(got.cpu().numpy(), path)
    if n == 257:
        if not backward:            # the nodes on the last row and column were sampled (in the clamped cell) and moved
            assert (path[0][:, 1:4] != pts.T[:, 1:4]).any(0).all()
        assert flag[6:10].tolist() == [OUT] * 4 and flag[11:13].tolist() == [OUT] * 2 and (flag == 0).any() and (flag == LOST).any()
    with pytest.raises(ValueError, match="particle list"):
        fm.ftle()


def test_a_batch_equals_its_parts(dev):
    """update(f[0:7]) == update(f[0:3]); update(f[3:7]) == seven single updates, bit for bit, with holes and a mask; an empty batch
    changes nothing."""
    from pivlfn import FlowMap
    H, W = 37, 53
    flows, mask = _fields(H, W, True, seed=14)
    f, m = _t(flows, dev), _t(mask, dev)
    whole = FlowMap(H, W, 2, device=dev)
    whole.update(f, m)
    for cuts in ((0, 3, 7), tuple(range(8)), (0, 0, 7, 7)):
        parts = FlowMap(H, W, 2, device=dev)
        for a, b in zip(cuts, cuts[1:]):
            parts.update(f[a:b], m[a:b])
        assert parts.steps == 7
        assert _same(parts.positions, whole.positions) and torch.equal(parts.flag, whole.flag), cuts


def _ulps32(a, b):
    """The distance in float32 steps between two arrays of finite float32 values of one sign pattern (NaN against NaN counts 0)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.where(np.isnan(a) & np.isnan(b), 0, np.abs(ia - ib))


@pytest.mark.parametrize("H,W,spacing", [(37, 53, 1), (37, 53, 2), (37, 53, 5), (2, 9, 1), (2, 9, 2), (9, 2, 2), (2, 2, 1), (2, 2, 3)])
def test_ftle_bits_of_the_restatement(H, W, spacing, dev):
    """stretch and oflag bit for bit, lattices of one row (2 x 9 at spacing 2), one column and one node included: all UNDEFINED.  ftle
    is log(stretch) / steps formed in float64 on the device and rounded to float32: the device's fp64 log is within an ulp or two of
    NumPy's, 2^-52 relative, and two float64 values that close round to float32 values at most one ulp apart."""
    from pivlfn import FlowMap
    flows, mask = _fields(H, W, True, seed=15)
    pos0, h, w = fr.lattice(H, W, spacing)
    pos, flag = fr.advect(flows, mask, pos0, np.zeros(h * w, np.uint8))
    stretch, oflag = fr.ftle_stretch(pos, flag, h, w, spacing)
    fm = FlowMap(H, W, spacing, device=dev)
    with pytest.raises(ValueError, match="steps == 0"):
        fm.ftle()
    fm.update(_t(flows, dev), _t(mask, dev))
    field = fm.ftle()
    assert (field.steps, field.spacing) == (B, spacing) and field.ftle.dtype == torch.float32 and field.stretch.dtype == torch.float64
    assert field.ftle.shape == field.stretch.shape == field.flag.shape == (h, w)
    assert np.array_equal(field.flag.cpu().numpy(), oflag)
    assert fr.same_bits(field.stretch.cpu().numpy(), stretch)
    with np.errstate(invalid="ignore"):
        want = (np.log(stretch) / B).astype(np.float32)
    got = field.ftle.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isnan(want), (oflag & UNDEFINED) != 0)
    assert _ulps32(got, want).max() <= 1
    if h < 2 or w < 2:
        assert (oflag & UNDEFINED).all()
    if (H, W, spacing) == (37, 53, 1):
        assert (oflag == 0).sum() > 500 and (oflag == UNDEFINED).any() and (oflag == (OUT | UNDEFINED)).any() and (oflag == (LOST | UNDEFINED)).any()
        s = field.summary()
        defined = (oflag & UNDEFINED) == 0
        assert s["defined"] == defined.sum() and s["out"] == ((oflag & OUT) != 0).mean() and s["lost"] == ((oflag & LOST) != 0).mean()
        assert s["undefined"] == (~defined).mean() and s["max_ftle"] == float(got[defined].max())
        assert abs(s["mean_ftle"] - got[defined].astype(np.float64).mean()) <= 1e-12


def test_saddle_reproduces_log1p_a(dev):
    """tests/test_flowmap.py's saddle on the device: the live positions are the closed form bit for bit, and the FTLE is log1p(1/32)
    -- to 1e-15 from the float64 stretch, to one float32 ulp in the float32 field."""
    from pivlfn import FlowMap
    steps, a = 6, 1.0 / 32
    fm = FlowMap(33, 33, device=dev)
    fm.update(_t(fr.saddle(steps, 33, a), dev))
    pos, flag = fm.positions.cpu().numpy(), fm.flag.cpu().numpy()
    x0 = np.broadcast_to(np.arange(33.0), (33, 33))
    live = flag == 0
    assert live.sum() == 27 * 33 and set(np.unique(flag)) == {0, OUT}
    assert np.array_equal(pos[0][live], 16.0 + (x0[live] - 16.0) * (33.0 / 32.0) ** steps)
    assert np.array_equal(pos[1][live], 16.0 + (x0.T[live] - 16.0) * (31.0 / 32.0) ** steps)
    field = fm.ftle()
    defined = (field.flag.cpu().numpy() & UNDEFINED) == 0
    assert defined.sum() == 25 * 33
    assert np.abs(np.log(field.stretch.cpu().numpy()[defined]) / steps - math.log1p(a)).max() <= 1e-15
    want = np.full(defined.sum(), math.log1p(a)).astype(np.float32)
    assert _ulps32(field.ftle.cpu().numpy()[defined], want).max() <= 1


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_guarded_buffers_and_a_scribbled_trace(backward, dev):
    """Inputs, state and trace between guards; the trace first holds the sentinel, then 0xFF: the same bits both times, every guard
    intact, no input written, no element of the trace left as it was."""
    from pivlfn import _lib
    lib = _lib.load()
    H, W, s = 38, 46, 1                                 # 1748 particles: B*H*W and N are multiples of 4 (whole 32-bit words)
    flows, mask = _fields(H, W, True, seed=16)
    pos0, flag0, h, w = _state(H, W, s)
    N = h * w
    pos_w, flag_w, path_w = fr.advect(flows, mask, pos0, flag0, backward=backward, iters=8, trace=True)
    src = [_t(flows, dev), _t(mask, dev)]
    ins = [guarded(t.shape, t.dtype, dev, "nan") for t in src]
    for t, x in zip(ins, src):
        t.copy_(x)
    pos, flag = guarded((2, N), torch.float64, dev, "sentinel"), guarded((N,), torch.uint8, dev, "sentinel")
    trace = guarded((B, 2, N), torch.float64, dev, "sentinel")
    st = torch.cuda.current_stream(dev).cuda_stream
    for scribble in (False, True):
        if scribble:
            _scribble(trace)
        pos.copy_(_t(pos0, dev))
        flag.copy_(_t(flag0, dev))
        _lib.check(lib.pivlfn_flowmap_advect(_p(ins[0]), _p(ins[1]), B, H, W, _p(pos), _p(flag), N, int(backward), 8, _p(trace), st), "flowmap_advect")
        torch.cuda.synchronize()
        assert fr.same_bits(pos.cpu().numpy(), pos_w) and np.array_equal(flag.cpu().numpy(), flag_w)
        assert fr.same_bits(trace.cpu().numpy(), path_w), "the trace differs, or part of it was not written"
        for t in ins + [pos, flag, trace]:
            check_guards(t, f"flowmap_advect backward={backward}")
    for t, x in zip(ins, src):
        assert torch.equal(t.view(torch.uint8), x.view(torch.uint8)), "an input was written"
    # the FTLE of that state, outputs between guards
    stretch, oflag = guarded((h, w), torch.float64, dev, "sentinel"), guarded((h, w), torch.uint8, dev, "sentinel")
    _lib.check(lib.pivlfn_flowmap_ftle(_p(pos), _p(flag), h, w, s, _p(stretch), _p(oflag), st), "flowmap_ftle")
    torch.cuda.synchronize()
    want = fr.ftle_stretch(pos_w, flag_w, h, w, s)
    assert fr.same_bits(stretch.cpu().numpy(), want[0]) and np.array_equal(oflag.cpu().numpy(), want[1])
    assert fr.same_bits(pos.cpu().numpy(), pos_w) and np.array_equal(flag.cpu().numpy(), flag_w), "an input of the FTLE was written"
    for t in (pos, flag, stretch, oflag):
        check_guards(t, "flowmap_ftle")


def test_every_error_is_refused_before_any_launch(dev):
    """The refusals of tests/test_flowmap.py with real device buffers: the state, the trace and the outputs keep every byte."""
    from pivlfn import _lib
    from test_flowmap import refusals
    lib = _lib.load()
    Bn, H, W, h, w = 3, 8, 9, 8, 9
    arena = _scribble(torch.empty(7 << 16, dtype=torch.uint8, device=dev))      # seven regions 64 KiB apart: only what a case moves overlaps
    flows, mask, pos, flag, trace, stretch, oflag = (arena.data_ptr() + (i << 16) for i in range(7))
    assert arena.data_ptr() % 8 == 0 and Bn * h * w * 16 < 1 << 16
    refusals(lib, flows, mask, pos, flag, trace, stretch, oflag, Bn, H, W, h * w, h, w)
    torch.cuda.synchronize()
    assert bool((arena == 0xFF).all())
    from pivlfn import FlowMap
    fm = FlowMap(8, 9, device=dev)
    for bad, kind in ((torch.zeros(1, 2, 8, 8, device=dev), ValueError), (torch.zeros(1, 2, 8, 9, device=dev, dtype=torch.float64), TypeError),
                      (torch.zeros(2, 8, 9, device=dev), ValueError)):
        with pytest.raises(kind):
            fm.update(bad)
    with pytest.raises(ValueError, match="mask"):
        fm.update(torch.zeros(1, 2, 8, 9, device=dev), torch.zeros(2, 8, 9, dtype=torch.uint8, device=dev))
    assert fm.steps == 0 and not bool(fm.flag.any())


# ---- side streams, graph capture and run.py: in a process of their own -----------------------------------------------------------------
def test_stream_contract_and_run_py_in_a_process_of_their_own(dev):
    """tests/flowmap_stream_cases.py -- the stream, capture and off-by-one-pointer contract of the three entry points through the
    helpers of tests/test_gpu_op_streams.py, and run.py --ftle -- in a fresh pytest process: 17 tests, all passing.  Why not in this
    process: a process has a few hardware queues for all its streams, and which side stream comes to share the default stream's queue
    follows from every stream the process has used before.  tests/test_gpu_op_streams.py::test_a_call_on_the_wrong_stream_reads_the_poison
    runs later in the suite's process and needs a side stream that does not share that queue; with the side streams of this module's
    delay, of graph capture and of run.py's network and copies used in between, it found the two on one queue and its launch on the
    wrong stream waited for the copies after all (each of those parts alone was enough to turn it, two together turned it back).
    Everything in this file runs on the default stream alone and leaves the process as it found it."""
    here = os.path.dirname(os.path.abspath(__file__))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                                                                          os.path.join(here, "flowmap_stream_cases.py")]
    r = subprocess.run(cmd, cwd=here, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and re.search(r"\b17 passed", r.stdout), r.stdout[-6000:] + r.stderr[-2000:]
