"""GPU: pivlfn_flow_moments_accumulate and pivlfn_flow_hist_accumulate (csrc/distribution.hip) against the NumPy restatement of their
contract (tests/distribution_restatement.py).  Every operation of the moments is a correctly rounded fp64 operation in a fixed order,
so acc is compared bit for bit, every element; the histograms are integer counts and are compared word by word.
Shapes: single pixels, rows and columns, 37 x 53, one vector over a 256-thread block, and each side of the steps of the launch plan
(pivlfn_flow_hist_plan: one and two workgroups of the histogram, its grid-stride loop from 2^20 vectors; the moments' grid is capped
at 4096 blocks, 2^20 pixels).  Tables: the smallest, an odd one, the default, the largest (the joint table in global memory), and both
sides of the LDS budget.  Then the inputs the contract names, how a sequence is cut into calls, the stream and capture contract with the
helpers of tests/test_gpu_op_streams.py, guarded buffers, the refusals, FlowDistribution on the DNS fixture and run.py --pdf."""
import json
import os

import numpy as np
import pytest
import torch

import distribution_restatement as dr
from guarded import check_guards, guarded
from test_distribution import plan
from test_gpu_op_streams import (F32, F64, U8, Spec, _behind_the_delay, _buf, _check, _p, _poisoned, _same, _scribble, delay)  # noqa: F401
from test_gpu_vortex import _close

pytestmark = pytest.mark.gpu
LO, HI = -2.0, 2.0                      # puts some vectors of every case outside


def _dev(dev, x):
    if x is None:
        return None
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _moments(dev, flow, mask, mean, thr, acc0, cuts=None):
    from pivlfn import _lib
    lib = _lib.load()
    B, _, H, W = flow.shape
    f, m, mu, t, acc = _dev(dev, flow), _dev(dev, mask), _dev(dev, mean), _dev(dev, thr), _dev(dev, acc0)
    at = 0
    for n in cuts or [B]:
        _lib.check(lib.pivlfn_flow_moments_accumulate(f[at:].data_ptr(), m[at:].data_ptr() if m is not None else None, _p(mu), _p(t),
                                                      acc.data_ptr(), n, H, W, _stream(dev)), "flow_moments_accumulate")
        at += n
    assert at == B
    return acc.cpu().numpy()


def _hist(dev, flow, mask, mean, scale, hist0, table, lo=LO, hi=HI, cuts=None):
    from pivlfn import _lib
    lib = _lib.load()
    B, _, H, W = flow.shape
    f, m, mu, sc, h = _dev(dev, flow), _dev(dev, mask), _dev(dev, mean), _dev(dev, scale), _dev(dev, hist0)
    at = 0
    for n in cuts or [B]:
        _lib.check(lib.pivlfn_flow_hist_accumulate(f[at:].data_ptr(), m[at:].data_ptr() if m is not None else None, _p(mu), _p(sc),
                                                   h.data_ptr(), n, H, W, lo, hi, *table, _stream(dev)), "flow_hist_accumulate")
        at += n
    assert at == B
    return h.cpu().numpy().view(np.uint64)


def _same_acc(got, want, what):
    same = got.view(np.int64) == want.view(np.int64)
    if not same.all():
        at = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {np.count_nonzero(~same)} of {same.size} sums differ, first at [term, y, x] = {at}: {got[at]!r} against {want[at]!r}")


def _same_hist(got, want, what):
    if not np.array_equal(got, want):
        at = int(np.argwhere(got != want)[0, 0])
        raise AssertionError(f"{what}: {np.count_nonzero(got != want)} of {got.size} counters differ, first at word {at}: {got[at]} against {want[at]}")


def _case(B, H, W, seed):
    """Flows with a mask, a mean, a scale and a thr, invalid vectors among them.  Images of fewer than 40 vectors get theirs by hand."""
    rng = np.random.default_rng(seed)
    flow, mask, mean, scale, thr = dr.random_case(rng, B, H, W, holes=H * W >= 40)
    if H * W < 40:
        mask[:] = 0
        flow[1, 0, H // 2, W // 2] = np.nan
        mask[2, H - 1, W - 1] = 7
    return flow, mask, mean, scale, thr


def _hist0(table, seed=5):
    return np.random.default_rng(seed).integers(0, 1 << 40, dr.hist_words(*table)).astype(np.uint64)


VARIANTS = [(False, False, False), (True, False, False), (False, True, False), (True, True, True), (False, False, True)]      # mask, mean, scale / thr
SHAPES = [(1, 1), (1, 7), (7, 1), (37, 53), (33, 257), (32, 64), (32, 65)]


@pytest.mark.parametrize("with_mask,with_mean,with_extra", VARIANTS, ids=["plain", "mask", "mean", "all", "scale-thr"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_bits_of_the_restatement(H, W, with_mask, with_mean, with_extra, dev):
    """B = 3 in one call from non-zero sums and counters, the default table over [-2, 2).  33 x 257: one vector over a 256-thread block
    of the moments; 3 x 32 x 64 and 3 x 32 x 65 vectors: three workgroups of the histogram with the last one full and a fourth with
    96 vectors."""
    flow, mask, mean, scale, thr = _case(3, H, W, 100 * H + W)
    mask, mean = mask if with_mask else None, mean if with_mean else None
    scale, thr = (scale, thr) if with_extra else (None, None)
    acc0 = np.random.default_rng(5).normal(0, 50, (21, H, W))
    table = (256, 64, 64)
    want_acc, want_hist = dr.moments(flow, mask, mean, thr, acc0), dr.hist(flow, mask, mean, scale, _hist0(table), LO, HI, *table)
    _same_acc(_moments(dev, flow, mask, mean, thr, acc0), want_acc, f"{H}x{W}")
    _same_hist(_hist(dev, flow, mask, mean, scale, _hist0(table), table), want_hist, f"{H}x{W}")
    at = dr.layout(*table)
    n, out = (int(x) for x in (want_hist - _hist0(table))[at["counted"]:at["counted"] + 2])
    assert n + out == 3 * H * W and n > 0 and out > 0, "the case must leave some vectors out and keep some"
    fresh = dr.moments(flow, mask, mean, thr, np.zeros_like(acc0))
    assert 0 < fresh[0].sum() < 3 * H * W and (not with_extra or fresh[0].sum() >= n)


def test_plan_steps_of_the_shapes():
    """What the shapes above and below are chosen for (answered on the host)."""
    assert plan(3, 32, 64, 256, 64, 64)["groups"] == 3 and plan(3, 32, 65, 256, 64, 64)["groups"] == 4
    assert plan(1, 32, 64, 1, 0, 0)["groups"] == 1 and plan(3, 37, 53, 1, 0, 0)["moment_blocks"] == 8
    assert plan(3, 33, 257, 1, 0, 0)["moment_blocks"] == 34
    below, above = plan(3, 590, 592, 256, 64, 64), plan(3, 1025, 1024, 256, 64, 64)
    assert below["groups"] == 512 and 3 * 590 * 592 < 1 << 20 and below["moment_blocks"] == 1365 < 4096
    assert above["groups"] == 512 and 3 * 1025 * 1024 > 3 << 20 and above["moment_blocks"] == 4096 < 4100


@pytest.mark.parametrize("H,W", [(590, 592), (1025, 1024)])
def test_bits_where_the_grids_are_capped(H, W, dev):
    """B = 3 with mask, mean, scale and thr.  3 x 590 x 592 = 1047840 vectors: 512 workgroups of the histogram, the last short, one
    sweep; 3 x 1025 x 1024 vectors: four sweeps of its grid-stride loop, and 4100 blocks of pixels on the moments' 4096."""
    flow, mask, mean, scale, thr = _case(3, H, W, H + W)
    acc0 = np.random.default_rng(5).normal(0, 50, (21, H, W))
    table = (256, 64, 64)
    _same_acc(_moments(dev, flow, mask, mean, thr, acc0), dr.moments(flow, mask, mean, thr, acc0), f"{H}x{W}")
    want = dr.hist(flow, mask, mean, scale, _hist0(table), LO, HI, *table)
    _same_hist(_hist(dev, flow, mask, mean, scale, _hist0(table), table), want, f"{H}x{W}")
    n, out = (int(x) for x in (want - _hist0(table))[-2:])
    assert n + out == 3 * H * W and n > 0 and out > 0


TABLES = [(1, 0, 0), (7, 3, 5), (256, 64, 64), (4096, 256, 1024), (124, 127, 0), (125, 127, 0)]


@pytest.mark.parametrize("table", TABLES, ids=lambda t: "x".join(map(str, t)))
def test_tables(table, dev):
    """3 x 37 x 53 and 3 x 32 x 65 (one and two workgroups) with everything given, over [-2, 2).  (4096, 256, 1024): the joint table is
    updated in global memory; (124, 127, 0) is exactly the 16384 counters of the LDS budget, (125, 127, 0) two over."""
    p = plan(3, 37, 53, *table)
    assert p["joint_in_lds"] == (table not in ((4096, 256, 1024), (125, 127, 0))) and p["words"] == dr.hist_words(*table)
    for H, W in ((37, 53), (32, 65)):
        flow, mask, mean, scale, _ = _case(3, H, W, 7 * H + W)
        for m, mu, sc in ((mask, mean, scale), (None, None, None)):
            want = dr.hist(flow, m, mu, sc, _hist0(table), LO, HI, *table)
            _same_hist(_hist(dev, flow, m, mu, sc, _hist0(table), table), want, f"{table} {H}x{W}")
            add = (want - _hist0(table)).astype(np.int64)
            at = dr.layout(*table)
            assert add[at["counted"]] > 0 and add[at["counted"] + 1] > 0 and add[at["joint"]:at["frac_u"]].sum() == add[at["counted"]]
            assert table[1] == 0 or add[at["outside"]] > 0


def test_edges_fractions_infinities_and_a_bad_scale(dev):
    """Values exactly on bin edges, at lo, at hi and just below it; -0.0; a tiny negative displacement (its fraction rounds to 1.0 and
    lands in the last bin); inf, NaN and 1e10; a scale plane with zeros, negatives, NaN and inf."""
    below = np.nextafter(np.float32(2.0), np.float32(0.0))
    vals = np.array([-2.0, 2.0, below, -1.0, 0.0, -0.0, 1.0, -1e-30, 0.5, -2.5, np.inf, -np.inf, np.nan, 1e10, -1e10, 1e9, 0.25, 1.75], np.float32)
    H, W = 3, len(vals)
    flow = np.zeros((2, 2, H, W), np.float32)
    flow[0, 0], flow[0, 1] = vals, vals[::-1]
    flow[1, 0], flow[1, 1] = vals[::-1], 0.5
    table = (4, 4, 4)
    got = _hist(dev, flow, None, None, None, np.zeros(dr.hist_words(*table), np.uint64), table)
    _same_hist(got, dr.hist(flow, None, None, None, np.zeros(dr.hist_words(*table), np.uint64), LO, HI, *table), "edges")
    _same_hist(got, dr.hist_loops(flow, None, None, None, np.zeros(dr.hist_words(*table), np.uint64), LO, HI, *table), "edges, the loop")
    at = dr.layout(*table)
    row = _hist(dev, flow[:1, :, :1], None, None, None, np.zeros(dr.hist_words(*table), np.uint64), table).astype(np.int64)
    # one row of frame 0: u = vals, v = vals reversed; 5 vectors are invalid in u and the same 5 in v (pairs i, 17 - i differ: 10 left out)
    assert row[at["counted"]] + row[at["counted"] + 1] == W and row[at["counted"] + 1] == 10
    fu = row[at["frac_u"]:at["frac_v"]]
    assert fu.sum() == row[at["counted"]] and fu[3] >= 1                      # 1.9999999 and 1.75; the 1.0 of -1e-30 is counted in frame 1, where v = 0.5
    scale = np.ones((2, H, W))
    scale[0, 0, 0], scale[1, 0, 4], scale[0, 1, 6], scale[1, 1, 8], scale[0, 2, 16] = 0.0, -1.0, np.nan, np.inf, -0.0
    scale[0, 2, 3] = 0.5
    acc0 = np.full((21, H, W), -0.0)
    for sc in (scale, None):
        got = _hist(dev, flow, None, None, sc, _hist0(table), table)
        _same_hist(got, dr.hist(flow, None, None, sc, _hist0(table), LO, HI, *table), "a bad scale")
    _same_acc(_moments(dev, flow, None, None, None, acc0), dr.moments(flow, None, None, None, acc0), "edges, the moments")


def test_a_constant_field_arrives_whole(dev):
    """Every lane of every wave hits one counter of each part: B x H x W must arrive in it.  Also from a workgroup's second sweep."""
    for B, H, W in ((3, 37, 53), (5, 512, 512)):
        flow = np.full((B, 2, H, W), 0.3, np.float32)
        flow[:, 1] = -1.2
        table = (256, 64, 64)
        got = _hist(dev, flow, None, None, None, np.zeros(dr.hist_words(*table), np.uint64), table).astype(np.int64)
        _same_hist(got.astype(np.uint64), dr.hist(flow, None, None, None, np.zeros(dr.hist_words(*table), np.uint64), LO, HI, *table), "constant")
        assert sorted(got[got != 0]) == [B * H * W] * 6 and got[-2] == B * H * W and got[-1] == 0


def test_a_pixel_left_out_in_every_frame_keeps_its_bits(dev):
    """Masked, NaN, 1e10 or without a finite mean in all three frames: the 21 values stay, -0.0 included; so do the quadrant terms of a
    pixel whose vectors are all inside the hole."""
    B, H, W = 3, 9, 31
    flow, mask, mean, _, thr = _case(B, H, W, 3)
    gone = [(0, 0), (4, 4), (8, 30), (2, 5)]
    mask[:, 0, 0] = 1
    flow[:, 0, 4, 4] = np.nan
    flow[:, 1, 8, 30] = 1e10
    mean[0, 2, 5] = np.inf
    thr[6, 6] = 1e30
    acc0 = np.random.default_rng(1).normal(0, 50, (21, H, W))
    acc0[::2] = -0.0
    got = _moments(dev, flow, mask, mean, thr, acc0)
    _same_acc(got, dr.moments(flow, mask, mean, thr, acc0), "left out")
    for y, x in gone:
        assert np.array_equal(got[:, y, x].view(np.int64), acc0[:, y, x].view(np.int64)), (y, x)
    assert np.array_equal(got[13:, 6, 6].view(np.int64), acc0[13:, 6, 6].view(np.int64)) and got[0, 6, 6] != acc0[0, 6, 6]
    assert np.signbit(got[14, 0, 0]) and (got.view(np.int64) != acc0.view(np.int64)).sum() > 10 * H * W


def test_cutting_the_sequence_into_calls_changes_no_bit(dev):
    """B = 6 as one call, as six calls and as 2 + 4, each from the same non-zero start, for both entry points; an all-zero mask gives the
    bits of the NULL mask."""
    B, H, W = 6, 37, 53
    flow, mask, mean, scale, thr = _case(B, H, W, 77)
    flow[1] *= 0.01
    flow[2] += np.float32(5.0)
    acc0 = np.random.default_rng(6).normal(0, 50, (21, H, W))
    table = (256, 64, 64)
    want_acc, want_hist = dr.moments(flow, mask, mean, thr, acc0), dr.hist(flow, mask, mean, scale, _hist0(table), LO, HI, *table)
    for cuts in ([6], [1] * 6, [2, 4]):
        _same_acc(_moments(dev, flow, mask, mean, thr, acc0, cuts), want_acc, f"cuts {cuts}")
        _same_hist(_hist(dev, flow, mask, mean, scale, _hist0(table), table, cuts=cuts), want_hist, f"cuts {cuts}")
    _same_acc(_moments(dev, flow, np.zeros_like(mask), mean, thr, acc0), _moments(dev, flow, None, mean, thr, acc0), "all-zero mask")
    _same_hist(_hist(dev, flow, np.zeros_like(mask), mean, scale, _hist0(table), table), _hist(dev, flow, None, mean, scale, _hist0(table), table),
               "all-zero mask")


# ---- the stream and capture contract, with the helpers of tests/test_gpu_op_streams.py ------------------------------------------------
B_, H_, W_, TABLE_ = 2, 40, 56, (64, 16, 8)                 # H*W % 4 == 0


def _inputs(seed):
    flow, mask, mean, scale, thr = _case(B_, H_, W_, 2000 + seed)
    return flow, mask, mean, scale, thr


def _spec(op, seed, quad=False):
    from pivlfn import _lib
    lib = _lib.load()
    flow, mask, mean, scale, thr = _inputs(seed)
    if op == "flow_moments_accumulate":
        acc0 = np.random.default_rng(3).normal(0, 50, (21, H_, W_))

        def call(i, o, a, ws, st):
            return lib.pivlfn_flow_moments_accumulate(_p(i[0]), _p(i[1]), _p(i[2]), _p(i[3]), _p(a[0]), B_, H_, W_, st)

        def pin(accs):
            assert dr.same_bits(accs[0].cpu().numpy(), dr.moments(flow, mask, mean, thr, acc0))
        return Spec([torch.from_numpy(x) for x in (flow, mask, mean, thr)], [], [torch.from_numpy(acc0)], [], call, pin, (H_, W_))
    h0 = _hist0(TABLE_, 3)

    def call(i, o, a, ws, st):
        return lib.pivlfn_flow_hist_accumulate(_p(i[0]), _p(i[1]), _p(i[2]), _p(i[3]), _p(a[0]), B_, H_, W_, LO, HI, *TABLE_, st)

    def pin(accs):
        assert np.array_equal(accs[0].cpu().numpy().view(np.uint64), dr.hist(flow, mask, mean, scale, h0, LO, HI, *TABLE_))
    return Spec([torch.from_numpy(x) for x in (flow, mask, mean, scale)], [], [torch.from_numpy(h0.view(np.int64))], [], call, pin, (H_, W_))


OPS = ["flow_moments_accumulate", "flow_hist_accumulate"]


@pytest.fixture()
def as_an_op(monkeypatch):
    """The helpers of test_gpu_op_streams look an op up by name: the two names resolve to the specs above."""
    import test_gpu_op_streams as ops
    original = ops._get
    monkeypatch.setattr(ops, "_get", lambda op, seed, quad=False: _spec(op, seed, quad) if op in OPS else original(op, seed, quad))
    return ops


@pytest.mark.parametrize("op", OPS)
def test_eager_result_is_the_restatements(op, dev, as_an_op):
    _, _, accs, _ = as_an_op._eager(op, 31, dev)
    _spec(op, 31).pin(accs)


@pytest.mark.parametrize("op", OPS)
def test_runs_in_order_on_the_stream_it_is_given(op, dev, delay, as_an_op):        # noqa: F811
    """On a side stream behind a long-running chain of matrix products and the copies of the real inputs into poisoned buffers,
    enqueued without a host synchronisation: the eager result, bit for bit, and every guard intact.  A launch on the default stream
    would read the poison: NaN flows, 0xFF masks and counters."""
    still_waiting, got, ref, buffers = _behind_the_delay(op, dev, delay, lambda stream: stream.cuda_stream)
    assert still_waiting, "the delay ran out before the op was enqueued: the test would not see a launch on another stream"
    for g, want in zip(got, ref):
        assert _same(g, want), "the result behind a delay on a side stream differs from the eager result"
    for t in buffers:
        _check(t, op)


@pytest.mark.parametrize("op", OPS)
def test_is_graph_capturable(op, dev, as_an_op):
    as_an_op.test_op_is_graph_capturable(op, dev)


@pytest.mark.parametrize("op", OPS)
def test_pointers_one_element_off_give_the_same_bits(op, dev, as_an_op):
    as_an_op.test_pointers_one_element_off_give_the_same_bits(op, dev)


def test_replaying_a_captured_graph_twice_doubles_the_counts(dev):
    """Both calls captured into one graph, from zeroed sums and counters: after one replay the restatement's counts, after two twice as
    many in every counter and in the count term of every pixel -- a replay adds, it does not reset."""
    from pivlfn import _lib
    lib = _lib.load()
    flow, mask, mean, scale, thr = _inputs(9)
    f, m, mu, sc, t = (_dev(dev, x) for x in (flow, mask, mean, scale, thr))
    acc = torch.zeros(21, H_, W_, dtype=F64, device=dev)
    hist = torch.zeros(dr.hist_words(*TABLE_), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = _stream(dev)
        rc = (lib.pivlfn_flow_moments_accumulate(_p(f), _p(m), _p(mu), _p(t), _p(acc), B_, H_, W_, st),
              lib.pivlfn_flow_hist_accumulate(_p(f), _p(m), _p(mu), _p(sc), _p(hist), B_, H_, W_, LO, HI, *TABLE_, st))
    assert rc == (0, 0)
    torch.cuda.synchronize()
    assert not bool(hist.any()) and not bool(acc.any()), "the capture itself ran the kernels"
    once = dr.hist(flow, mask, mean, scale, np.zeros(dr.hist_words(*TABLE_), np.uint64), LO, HI, *TABLE_)
    zero = np.zeros((21, H_, W_))
    g.replay()
    torch.cuda.synchronize()
    _same_hist(hist.cpu().numpy().view(np.uint64), once, "one replay")
    _same_acc(acc.cpu().numpy(), dr.moments(flow, mask, mean, thr, zero), "one replay")
    g.replay()
    torch.cuda.synchronize()
    _same_hist(hist.cpu().numpy().view(np.uint64), 2 * once, "two replays")
    twice = dr.moments(np.concatenate([flow, flow]), np.concatenate([mask, mask]), mean, thr, zero)
    _same_acc(acc.cpu().numpy(), twice, "two replays")
    assert np.array_equal(twice[0], 2 * dr.moments(flow, mask, mean, thr, zero)[0]) and once[-2] > 0


@pytest.mark.parametrize("W", [46, 258])
def test_guarded_buffers(W, dev):
    """acc and hist between guards, guards behind flow, mask, mean, scale and thr (and in front of them), the padding poisoned: every
    guard intact, no input written, the bits of the unguarded call."""
    from pivlfn import _lib
    lib = _lib.load()
    B, H, table = 2, 38, (64, 16, 7)                                           # B*H*W a multiple of 4: the byte buffer is whole 32-bit words
    flow, mask, mean, scale, thr = _case(B, H, W, 600 + W)
    acc0 = np.random.default_rng(7).normal(0, 50, (21, H, W))
    h0 = _hist0(table)
    src = [_dev(dev, x) for x in (flow, mask, mean, scale, thr, acc0, h0)]
    bufs = [guarded(t.shape, t.dtype, dev, "nan") for t in src]
    for t, x in zip(bufs, src):
        t.copy_(x)
    _lib.check(lib.pivlfn_flow_moments_accumulate(_p(bufs[0]), _p(bufs[1]), _p(bufs[2]), _p(bufs[4]), _p(bufs[5]), B, H, W, _stream(dev)),
               "flow_moments_accumulate")
    _lib.check(lib.pivlfn_flow_hist_accumulate(_p(bufs[0]), _p(bufs[1]), _p(bufs[2]), _p(bufs[3]), _p(bufs[6]), B, H, W, LO, HI, *table,
                                               _stream(dev)), "flow_hist_accumulate")
    torch.cuda.synchronize()
    _same_acc(bufs[5].cpu().numpy(), dr.moments(flow, mask, mean, thr, acc0), f"guarded 38x{W}")
    _same_hist(bufs[6].cpu().numpy().view(np.uint64), dr.hist(flow, mask, mean, scale, h0, LO, HI, *table), f"guarded 38x{W}")
    for t in bufs:
        check_guards(t, f"distribution 38x{W}")
    for t, x in zip(bufs[:5], src[:5]):
        assert torch.equal(t.view(torch.uint8), x.view(torch.uint8)), "an input was written"


def test_every_error_is_refused_before_any_launch(dev):
    """The refusals of tests/test_distribution.py with real device buffers: acc, hist and everything else keep every byte."""
    from pivlfn import _lib
    from test_distribution import refusals
    lib = _lib.load()
    arena = _scribble(torch.empty(6 << 16, dtype=torch.uint8, device=dev))      # six regions 64 KiB apart: only what a case moves overlaps
    flow, mask, mean, extra, acc, hist = (arena.data_ptr() + (i << 16) for i in range(6))
    assert arena.data_ptr() % 8 == 0
    refusals(lib, flow, mask, mean, extra, acc, hist, 2, 8, 8)
    torch.cuda.synchronize()
    assert bool((arena == 0xFF).all())


# ---- the Python class ------------------------------------------------------------------------------------------------------------------
def test_flow_distribution_on_the_dns_fixture(dev, tmp_path):
    """tests/golden/DNS_turbulence_flow.flo, 256 x 256: the sums and counters are the restatement's, and the result reproduces the
    numbers the feature was specified with."""
    from conftest import GOLD
    from pivlfn import DistributionResult, FlowDistribution
    flow = dr.read_flo(os.path.join(GOLD, "DNS_turbulence_flow.flo"))[None]
    wide = FlowDistribution(256, 256, bins=64, range=(-4.0, 4.0), joint_bins=16, frac_bins=16, device=dev)
    narrow = FlowDistribution(256, 256, bins=64, range=(-2.0, 2.0), joint_bins=16, frac_bins=16, device=dev)
    for fd in (wide, narrow):
        fd.update(torch.from_numpy(flow).to(dev))
        assert fd.count == 1
    _same_acc(wide.acc.cpu().numpy(), dr.moments(flow, None, None, None, np.zeros((21, 256, 256))), "DNS")
    _same_hist(wide.hist.cpu().numpy().view(np.uint64), dr.hist(flow, None, None, None, np.zeros(dr.hist_words(64, 16, 16), np.uint64), -4.0, 4.0, 64, 16, 16), "DNS")
    r = wide.result()
    assert r.counted == 65536 and r.left_out == 0 and r.outside("u") == (0.0, 0.0) and r.outside("v") == (0.0, 0.0) and r.outside_joint() == 0.0
    assert round(narrow.result().outside_joint() * 65536) == 853
    fu, fv = r.fraction("u"), r.fraction("v")
    assert (int(fu.min()), int(fu.max()), int(fv.min()), int(fv.max())) == (3701, 4719, 3643, 4423)
    assert abs(r.peak_locking("u") - 0.2157) < 5e-5 and abs(r.peak_locking("v") - 0.1764) < 5e-5
    p = r.pooled()
    assert abs(p["skewness_u"] - -0.0073) < 5e-5 and abs(p["flatness_u"] - 2.693) < 5e-4
    assert abs(p["skewness_v"] - 0.1792) < 5e-5 and abs(p["flatness_v"] - 3.046) < 5e-4
    centres, density = r.pdf("u")
    assert abs(density.sum() * (centres[1] - centres[0]) - 1.0) < 1e-14
    locked = FlowDistribution(256, 256, bins=64, range=(-4.0, 4.0), joint_bins=16, frac_bins=16, device=dev)
    locked.update(torch.from_numpy(np.rint(flow).astype(np.float32)).to(dev))
    assert locked.result().peak_locking("u") == 1.0 and locked.result().peak_locking("v") == 1.0
    back = DistributionResult.load(wide.save(str(tmp_path / "pdf")))
    assert dr.same_bits(back.acc, r.acc) and np.array_equal(back.hist, r.hist) and back.frames == 1


def test_flow_distribution_update_mean_scale_and_checks(dev, tmp_path):
    """Two update() calls equal one; a mask of bools; mean and scale as a tensor, an array and a FlowStats file give the same bits,
    which are the restatement's, with thr = hole * rms_u * rms_v; wrong sizes and types are refused."""
    from pivlfn import FlowDistribution
    from pivlfn.postpro import FlowStats
    B, H, W, hole = 4, 21, 45, 0.5
    flow, mask, _, _, _ = _case(B, H, W, 88)
    flow = np.nan_to_num(flow, nan=0.5, posinf=1.0, neginf=-1.0)
    flow[np.abs(flow) > 1e9] = 2.0                     # FlowStats has no notion of an invalid vector
    f, m = torch.from_numpy(flow).to(dev), torch.from_numpy(mask).to(dev)
    stats = FlowStats(H, W, device=dev)
    stats.update(f)
    path = stats.save(str(tmp_path / "stats"))
    res = stats.result()
    mean, rms = np.stack([res["mean_u"], res["mean_v"]]), np.stack([res["rms_u"], res["rms_v"]])
    thr = hole * rms[0] * rms[1]
    table = (32, 8, 8)
    want_acc = dr.moments(flow, mask, mean, thr, np.zeros((21, H, W)))
    want_hist = dr.hist(flow, mask, mean, rms, np.zeros(dr.hist_words(*table), np.uint64), -6.0, 6.0, *table)
    for mu, sc in ((path, path), (mean, rms), (torch.from_numpy(mean), torch.from_numpy(rms).to(dev))):
        fd = FlowDistribution(H, W, 32, (-6.0, 6.0), 8, 8, mean=mu, scale=sc, hole=hole, device=dev)
        fd.update(f[:3], m[:3] != 0)
        fd.update(f[3:], m[3:])
        fd.update(f[:0])
        assert fd.count == 4 and fd.result().normalised
        _same_acc(fd.acc.cpu().numpy(), want_acc, f"mean given as {type(mu).__name__}")
        _same_hist(fd.hist.cpu().numpy().view(np.uint64), want_hist, f"scale given as {type(sc).__name__}")
    plain = FlowDistribution(H, W, 32, (-6.0, 6.0), 8, 8, hole=hole, device=dev)
    plain.update(f, m)
    _same_acc(plain.acc.cpu().numpy(), dr.moments(flow, mask, None, np.full((H, W), hole), np.zeros((21, H, W))), "a hole without a scale")
    with pytest.raises(ValueError, match="mean"):
        FlowDistribution(H, W, mean=mean[:, :-1], device=dev)
    with pytest.raises(ValueError, match="scale"):
        FlowDistribution(H, W, scale=rms[:, :, :-1], device=dev)
    with pytest.raises(ValueError, match="accumulators"):
        fd.update(f[:, :, :-1])
    with pytest.raises(TypeError):
        fd.update(f.double())
    with pytest.raises(ValueError, match="bins"):
        FlowDistribution(H, W, bins=4097, device=dev)


# ---- run.py --------------------------------------------------------------------------------------------------------------------------
def test_run_py_pdf(tmp_path, dev, capsys):
    """run.py -p --pdf on three synthetic 64 x 64 pairs, alone and with --validate flag beside --stats, then the second pass with
    --pdf-mean / --pdf-normalise: pdf.npz holds the sums and counters of a FlowDistribution fed the written flows (with the validation
    flags as the mask), bit for bit; pdf.json the parameters, the validation mode and summary(); a run without --pdf writes none of it."""
    import PIL.Image
    import run as runpy
    from pivlfn import FlowDistribution, synth
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
    assert runpy.main(base + ["-o", str(tmp_path / "alone"), "--pdf", "--pdf-image"]) == 3
    assert "peak locking u" in capsys.readouterr().out
    assert runpy.main(base + val + ["-o", str(tmp_path / "both"), "--pdf", "32", "--pdf-range", "-2", "2", "--pdf-hole", "0.1", "--stats"]) == 3
    alone, both, second = (tmp_path / d / "piv-synthetic" / "seq" for d in ("alone", "both", "second"))
    stats = str(both / "stats.npz")
    assert runpy.main(base + val + ["-o", str(tmp_path / "second"), "--pdf", "32", "--pdf-mean", stats, "--pdf-normalise", "--pdf-hole", "1"]) == 3
    assert not (both / "pdf_joint.png").exists() and (alone / "pdf_joint.png").stat().st_size > 0
    assert "pdf: 256\n" in list(open(alone / "args.txt")) and "pdf_hole: 0.1\n" in list(open(both / "args.txt"))
    cases = ((alone, 256, (-8.0, 8.0), None, False, 0.0, None), (both, 32, (-2.0, 2.0), None, False, 0.1, "flag"),
             (second, 32, (-6.0, 6.0), stats, True, 1.0, "flag"))
    for out, bins, rng, mean, normalise, hole, mode in cases:
        flows = torch.stack([torch.from_numpy(read_flow(str(out / "flow" / f"{n}_out.flo"))).permute(2, 0, 1) for n in names]).contiguous().to(dev)
        flags = V.validate_flow(flows, radius=2, spacing=1, eps=0.01, thresh=0.5, mode="flag").flag if mode else None
        fd = FlowDistribution(H, W, bins, rng, 64, 64, mean=mean, scale=mean if normalise else None, hole=hole, device=dev)
        fd.update(flows, flags)
        with np.load(out / "pdf.npz") as f:
            _same_acc(f["acc"], fd.acc.cpu().numpy(), f"run.py --pdf {bins}")
            _same_hist(f["hist"], fd.hist.cpu().numpy().view(np.uint64), f"run.py --pdf {bins}")
            assert int(f["frames"]) == 3 and int(f["bins"]) == bins and (str(f["validation"]) == "flag" if mode else "validation" not in f.files)
        doc = json.load(open(out / "pdf.json"))
        assert (doc["bins"], doc["range"], doc["mean"], doc["normalise"], doc["hole"], doc["validation"]) == (bins, list(rng), mean, normalise, hole, mode)
        assert _close(doc["summary"], runpy.json_strict(fd.result().summary())), (doc["summary"], fd.result().summary())
        if mode:
            assert fd.result().left_out > 0                                      # the validator did flag vectors
