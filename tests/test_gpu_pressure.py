"""GPU: the pressure entry points (csrc/pressure.hip) against the NumPy restatement of their contract (tests/pressure_restatement.py).
Every operation of the contract is a correctly rounded fp64 operation in a fixed order, so g, valid, b, the adjacency (hence deg), p,
flag and the status record are compared bit for bit, every element, after 0, 1, 2, 3, 10 and 40 iterations and at convergence.
Lattices: 1 x 1 and 3 x 3 (nothing to solve), 3 x 4 and 5 x 7, 19 x 23 with a hole that splits it, 33 x 65 just over a power of two,
70 x 131 with several workgroups' leaves; and, for three iterations, the four lattices of tests/analysis_plans.py at which the plan of
the block partials changes (257 and 1025 partials, two and four chunks a workgroup).  Then a batch against its frames alone, how the iterations are cut into calls, the class, the
stream and capture contract as tests/test_gpu_op_streams.py holds the other entry points to it (its helpers, imported), guarded
buffers, the refusals and run.py --pressure."""
import json
import os

import numpy as np
import pytest
import torch

import pressure_restatement as pr
from guarded import check_guards, guarded
from test_gpu_op_streams import (F32, F64, U8, Spec, _behind_the_delay, _buf, _check, _p, _poisoned, _same, _scribble, delay)  # noqa: F401

pytestmark = pytest.mark.gpu

CONV = "convergence"
COUNTS = (0, 1, 2, 3, 10, 40, CONV)


def _dev(dev, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _popcount4(a):
    return ((a & 1) + ((a >> 1) & 1) + ((a >> 2) & 1) + ((a >> 3) & 1)).astype(np.float64)


class Device:
    """flows through pivlfn_pressure_gradient and _setup; cg() and read() as often as wanted."""

    def __init__(self, dev, flows, s, nu):
        from pivlfn import _lib
        self.lib, self.check, self.dev = _lib.load(), _lib.check, dev
        B, _, h, w = flows.shape
        self.F, self.h, self.w = B - 2, h, w
        F = self.F
        self.st = torch.cuda.current_stream(dev).cuda_stream
        self.flows = _dev(dev, flows)
        self.g = _scribble(torch.empty((F, 2, h, w), dtype=F64, device=dev))
        self.valid = _scribble(torch.empty((F, h, w), dtype=U8, device=dev))
        self.check(self.lib.pivlfn_pressure_gradient(self.flows.data_ptr(), B, h, w, s, nu, self.g.data_ptr(), self.valid.data_ptr(), self.st),
                   "gradient")
        self.nws = self.lib.pivlfn_pressure_workspace_bytes(F, h, w)
        self.s = s
        self.setup()

    def setup(self, g=None, valid=None):
        self.ws = _scribble(torch.empty(self.nws, dtype=U8, device=self.dev))          # needs no initial contents
        g, valid = self.g if g is None else g, self.valid if valid is None else valid
        self.check(self.lib.pivlfn_pressure_setup(g.data_ptr(), valid.data_ptr(), self.F, self.h, self.w, self.s, self.ws.data_ptr(), self.nws,
                                                  self.st), "setup")
        return self

    def cg(self, tol, iters):
        self.check(self.lib.pivlfn_pressure_cg(self.ws.data_ptr(), self.nws, self.F, self.h, self.w, tol, iters, self.st), "cg")
        return self

    def array(self, what, dtype):
        off = self.lib.pivlfn_pressure_workspace_offset(self.F, self.h, self.w, what)
        n = self.F * self.h * self.w * torch.empty(0, dtype=dtype).element_size()
        return self.ws[off:off + n].view(dtype).view(self.F, self.h, self.w).cpu().numpy()

    def read(self):
        """Everything that is compared, as host arrays."""
        F, h, w = self.F, self.h, self.w
        p, flag = _scribble(torch.empty((F, h, w), dtype=F64, device=self.dev)), _scribble(torch.empty((F, h, w), dtype=U8, device=self.dev))
        status = _scribble(torch.empty((F, 4), dtype=F64, device=self.dev))
        self.check(self.lib.pivlfn_pressure_read(self.ws.data_ptr(), self.nws, F, h, w, p.data_ptr(), flag.data_ptr(), status.data_ptr(), self.st),
                   "read")
        return {"g": self.g.cpu().numpy(), "valid": self.valid.cpu().numpy(), "b": self.array(0, F64), "adj": self.array(2, U8),
                "p": p.cpu().numpy(), "flag": flag.cpu().numpy(), "status": status.cpu().numpy()}


def _state(g, valid, frames):
    out = [fr.read() for fr in frames]
    return {"g": g, "valid": valid, "b": np.stack([fr.b for fr in frames]), "adj": np.stack([fr.adj for fr in frames]),
            "p": np.stack([o[0] for o in out]), "flag": np.stack([o[1] for o in out]), "status": np.stack([o[2] for o in out])}


def _compare(got, want, what):
    for key in ("g", "valid", "b", "adj", "p", "flag", "status"):
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, key, a.shape, b.shape, a.dtype, b.dtype)
        same = a.view(np.uint8).reshape(a.shape + (-1,)) == b.view(np.uint8).reshape(b.shape + (-1,))
        same = same.all(-1)
        if not same.all():
            at = tuple(np.argwhere(~same)[0])
            raise AssertionError(f"{what}: {np.count_nonzero(~same)} of {same.size} elements of {key} differ, first at {at}: "
                                 f"{a[at]!r} against {b[at]!r}")
    assert np.array_equal(_popcount4(got["adj"]), _popcount4(want["adj"]))      # deg, which the adjacency bits hold


def _flows(h, w, seed, B=3):
    """Random flows; from 5 x 7 on some vectors are unknown, and at 19 x 23 a column of the centre flow is, which splits the lattice in
    two, and one vector of the PREVIOUS flow only."""
    rng = np.random.default_rng(seed)
    flows = pr.random_flows(rng, B, h, w)
    if h * w >= 35:
        flows[1, 0, h // 2, 1] = np.nan
    if h * w >= 400:
        for k in range(h * w // 150):
            flows[rng.integers(0, B), rng.integers(0, 2), rng.integers(0, h), rng.integers(0, w)] = (np.nan, 1e10, -np.inf)[k % 3]
    if (h, w) == (19, 23):
        flows[1, :, :, 11] = 1e10
        flows[0, 1, 4, 4] = 1e10
    return flows


_cases = {}


def _reference(h, w, s, nu, tol):
    """The restatement's state after each of COUNTS iterations, made once per lattice: one Frame carried on."""
    key = (h, w, s, nu, tol)
    if key not in _cases:
        flows = _flows(h, w, 100 * h + w)
        g, valid = pr.gradient(flows, s, nu)
        fr, states, done = pr.Frame(g[0], valid[0], s), {}, 0
        cap = 10 * max(h, w) + 50
        for count in COUNTS:
            upto = cap if count == CONV else count
            fr.run(tol, upto - done)
            done = upto
            states[count] = _state(g, valid, [fr])
        assert fr.state != pr.RUNNING, "the cap must be enough for this lattice"
        _cases[key] = (flows, states, fr.iterations)
    return _cases[key]


SHAPES = [(1, 1), (3, 3), (3, 4), (5, 7), (19, 23), (33, 65), (70, 131)]


@pytest.mark.parametrize("h,w", SHAPES)
def test_bits_of_the_restatement(h, w, dev):
    """One frame, s = 2, nu* = 0.1, tol = 1e-9, from a scribbled workspace, after every count of COUNTS.  Every lattice loses nodes (the
    border) and keeps some -- but 1 x 1, which has no interior: nothing is valid there and the frame ends in BREAKDOWN with no value."""
    s, nu, tol = 2.0, 0.1, 1e-9
    flows, states, total = _reference(h, w, s, nu, tol)
    kept = int(states[0]["valid"].sum())
    assert kept < h * w and (kept > 0 or (h, w) == (1, 1)), "the case must exclude some nodes and keep some"
    if (h, w) == (3, 3):
        assert kept == 1 and states[0]["flag"][0, 1, 1] == pr.ISOLATED
    if (h, w) == (19, 23):
        fr = pr.Frame(states[0]["g"][0], states[0]["valid"][0], s)
        assert pr.components(fr)[1] == 2 and states[0]["valid"][0, 4, 4] == 0 and states[0]["valid"][0, 4, 5] == 1
    cap = 10 * max(h, w) + 50
    d = Device(dev, flows, s, nu)
    for count in COUNTS:
        d.setup().cg(tol, cap if count == CONV else count)
        _compare(d.read(), states[count], f"{h}x{w} after {count} iterations")
    final = states[CONV]["status"][0]
    assert final[0] == (pr.CONVERGED if kept > 1 else pr.BREAKDOWN) and final[1] == total
    if h * w >= 400:
        assert total > 40 and states[40]["status"][0, 0] == pr.RUNNING


# ---- where the plan of the block partials changes (tests/analysis_plans.py) -----------------------------------------------------------
LARGE_COUNTS = (0, 1, 2, 3)


def _large_reference(h, w, s, nu, tol, keep=False):
    """As _reference, for the counts of LARGE_COUNTS only: pr.tree() is the contract's full binary tree and knows nothing of chunks.
    Kept for a second test only where `keep` says so: the states of 2048 x 2049 are 300 MB."""
    key = ("large", h, w, s, nu, tol)
    if key not in _cases:
        flows = _flows(h, w, 100 * h + w)
        g, valid = pr.gradient(flows, s, nu)
        fr, states, done = pr.Frame(g[0], valid[0], s), {}, 0
        for count in LARGE_COUNTS:
            fr.run(tol, count - done)
            done = count
            states[count] = _state(g, valid, [fr])
        assert fr.state == pr.RUNNING and fr.iterations == 3
        if not keep:
            return flows, states
        _cases[key] = (flows, states)
    return _cases[key]


def _plan_holds(h, w, F=1):
    """The library's own NB, from where b lies in the workspace, is the one tests/analysis_plans.py restates and its case is named for."""
    import analysis_plans as ap
    from pivlfn import _lib
    assert _lib.load().pivlfn_pressure_workspace_offset(F, h, w, 0) == 128 * F + 24 * ap.pressure(h, w)["NB"] * F
    return ap.pressure(h, w)


def _pressure_shapes():
    import analysis_plans as ap
    return ap.shapes(ap.PRESSURE_CASES)


@pytest.mark.parametrize("h,w", _pressure_shapes())
def test_bits_where_the_partials_plan_changes(h, w, dev):
    """One frame, s, nu* and tol as test_bits_of_the_restatement, after setup and after 1, 2 and 3 iterations (no run to convergence:
    the host's share of an iteration at 2048 x 2049 is about a second).  513 x 512: 257 partials, one in the second wave of pr_finish;
    1024 x 1025: 1025, one in its second chunk; 2048 x 1025 and 2048 x 2049: two and four chunks per workgroup, PrCounter and its carry."""
    s, nu, tol = 2.0, 0.1, 1e-9
    plan = _plan_holds(h, w)
    assert plan["NB"] > 256
    flows, states = _large_reference(h, w, s, nu, tol, keep=(h, w) == (1024, 1025))
    kept = int(states[0]["valid"].sum())
    assert h * w - kept > 2 * (h + w) - 4 and kept > h * w // 2, "unknown vectors must take nodes out beside the border"
    d = Device(dev, flows, s, nu)
    for count in LARGE_COUNTS:
        d.setup().cg(tol, count)
        _compare(d.read(), states[count], f"{h}x{w} after {count} iterations")
    assert states[3]["status"][0, 0] == pr.RUNNING and states[3]["status"][0, 1] == 3


def test_cuts_and_batches_change_no_bit_with_a_second_chunk_of_partials(dev):
    """1024 x 1025 (NB = 1025): 3 iterations in one call against 1 + 2; and the frame as the second of a batch of two (its partials
    start at 1025, no multiple of anything) has the bits it has alone, as has the frame in front of it."""
    h, w, s, nu, tol = 1024, 1025, 2.0, 0.1, 1e-9
    assert _plan_holds(h, w, 2)["NB"] == 1025
    flows, states = _large_reference(h, w, s, nu, tol, keep=True)
    d = Device(dev, flows, s, nu).cg(tol, 1).cg(tol, 2)
    alone = d.read()
    _compare(alone, states[3], "cuts 1 + 2")
    del d
    before = _flows(h, w, 31)[:1]
    four = np.concatenate([before, flows])
    both = Device(dev, four, s, nu).cg(tol, 3).read()
    _compare({k: v[1:2] for k, v in both.items()}, alone, "the frame as the second of two")
    first = Device(dev, four[:3], s, nu).cg(tol, 3).read()
    _compare({k: v[0:1] for k, v in both.items()}, first, "the frame in front of it")
    assert not pr.same_bits(first["p"], alone["p"])


def test_reading_does_not_disturb_the_iteration(dev):
    """read() between two cg() calls, and twice: the same bits as without."""
    h, w, s, nu, tol = 19, 23, 2.0, 0.1, 1e-9
    flows, states, _ = _reference(h, w, s, nu, tol)
    d = Device(dev, flows, s, nu).cg(tol, 3)
    _compare(d.read(), states[3], "after 3")
    _compare(d.read(), states[3], "after 3, read again")
    d.cg(tol, 7)
    _compare(d.read(), states[10], "after 3 + 7 with a read between")


# ---- batches and cuts -------------------------------------------------------------------------------------------------------------------
def _batch_case():
    """Five flows of 19 x 23 -> three frames with different unknown vectors each; the last flow is unknown but for a small patch, so
    the third frame (the only one that reads it) has a handful of valid nodes and converges long before the others."""
    flows = _flows(19, 23, 4242, B=5)
    keep = flows[4, :, 3:8, 3:9].copy()
    flows[4] = 1e10
    flows[4, :, 3:8, 3:9] = keep
    return flows


def test_a_frame_in_a_batch_has_the_bits_it_has_alone(dev):
    s, nu, tol = 2.0, 0.1, 1e-9
    flows = _batch_case()
    g, valid = pr.gradient(flows, s, nu)
    assert len({int(v.sum()) for v in valid}) == 3 and 1 < valid[2].sum() <= 30
    for iters in (0, 1, 10, 40, 240):
        frames = [pr.Frame(g[f], valid[f], s).run(tol, iters) for f in range(3)]
        want = _state(g, valid, frames)
        got = Device(dev, flows, s, nu).cg(tol, iters).read()
        _compare(got, want, f"F = 3 after {iters}")
        for f in range(3):
            alone = Device(dev, flows[f:f + 3], s, nu).cg(tol, iters).read()
            _compare(alone, {k: v[f:f + 1] for k, v in got.items()}, f"frame {f} alone after {iters}")
    it = [fr.iterations for fr in frames]
    assert all(fr.state == pr.CONVERGED for fr in frames) and it[2] < 40 < min(it[:2]), it


def test_cutting_the_iterations_into_calls_changes_no_bit(dev):
    s, nu, tol = 2.0, 0.1, 1e-9
    flows = _batch_case()
    g, valid = pr.gradient(flows, s, nu)
    want = _state(g, valid, [pr.Frame(g[f], valid[f], s).run(tol, 40) for f in range(3)])
    for cuts in ([40], [1] * 40, [7, 33]):
        d = Device(dev, flows, s, nu)
        for n in cuts:
            d.cg(tol, n)
        _compare(d.read(), want, f"cuts {cuts[:3]}...")


# ---- the Python class -----------------------------------------------------------------------------------------------------------------
def _class_case(dev):
    """Five flows of 40 x 52 for cell = 2: smooth enough to converge, a masked block that leaves lattice cells empty, one NaN."""
    rng = np.random.default_rng(77)
    flows = pr.random_flows(rng, 5, 40, 52, sigma=0.5)
    flows[2, 0, 30, 40] = np.nan
    mask = np.zeros((5, 40, 52), np.uint8)
    mask[1, 10:16, 20:30] = 1
    mask[4, 0:8, 0:8] = 3
    return _dev(dev, flows), _dev(dev, mask)


def _result_bits(results):
    cat = lambda key: torch.cat([getattr(r, key) for r in results]).cpu().numpy()          # noqa: E731
    return {"p": cat("p_star"), "g": cat("g"), "flag": cat("flag_dev"), "status": cat("status")}


def test_pressure_field_against_the_restatement_and_however_it_is_driven(dev):
    """cell = 2: p*, g, flag and status equal the restatement fed decimate_flow's own output, bit for bit; sync_every = 64, None and 1
    and updates cut 5, 2 + 3 and 1 x 5 give the same bits; the physical values follow."""
    from pivlfn import PressureField, decimate_flow
    flows, mask = _class_case(dev)
    kw = dict(cell=2, calib=0.5, dt=0.25, rho=3.0, nu=0.02, tol=1e-9)
    dec = decimate_flow(flows, 2, mask)[0].cpu().numpy()
    assert (dec == np.float32(1e10)).any()
    nu_star = 0.02 * 0.25 / (0.5 * 0.5)
    g, valid = pr.gradient(dec, 2.0, nu_star)
    cap = 10 * 26 + 50
    p, flag, status, frames = pr.solve(g, valid, 2.0, 1e-9, cap)
    want = {"p": p, "g": g, "flag": flag, "status": status}
    assert all(fr.state == pr.CONVERGED for fr in frames) and (flag == pr.INVALID).sum() > 3 * (2 * 20 + 2 * 24)

    def drive(cuts, **more):
        pf = PressureField(40, 52, device=dev, **kw, **more)
        assert pf.max_iter == cap and (pf.ch, pf.cw) == (20, 26)
        at, out = 0, []
        for n in cuts:
            out.append(pf.update(flows[at:at + n], mask[at:at + n]))
            at += n
        assert pf.count == 3 and sum(len(r) for r in out) == 3
        return out

    first = drive([5])
    for cuts, more in (([5], {}), ([5], dict(sync_every=None)), ([5], dict(sync_every=1)), ([2, 3], {}), ([1] * 5, dict(sync_every=None))):
        got = _result_bits(drive(cuts, **more))
        for key in want:
            assert pr.same_bits(got[key], want[key]), (cuts, more, key)
    assert [len(r) for r in drive([2, 3])] == [0, 3] and [len(r) for r in drive([1] * 5)] == [0, 0, 1, 1, 1]
    res = first[0]
    assert res.converged.all() and list(res.iterations) == [fr.iterations for fr in frames] and (res.residual <= 1e-9).all()
    scale = 3.0 * (0.5 / 0.25) ** 2
    for f in range(3):
        ok = flag[f] == pr.OK
        assert np.array_equal(res.p[f][ok], scale * (p[f][ok] - p[f][ok].mean())) and np.isnan(res.p[f][~ok]).all()
    assert np.array_equal(res.grad, 3.0 * 0.5 / (0.25 * 0.25) * g)
    capped = PressureField(40, 52, device=dev, max_iter=5, **kw).update(flows, mask)
    assert not capped.converged.any() and list(capped.iterations) == [5, 5, 5] and capped.summary()["unconverged"] == 3
    with pytest.raises(ValueError, match="expected"):
        PressureField(40, 52, device=dev, **kw).update(flows[:, :, :-1])


# ---- the stream and capture contract, with the helpers of tests/test_gpu_op_streams.py ------------------------------------------------
def _spec(seed, quad=False):
    """Four flows of 20 x 28 (h*w % 4 == 0) -> two frames: gradient, setup, 12 iterations in two calls and the read-out as one op."""
    from pivlfn import _lib
    lib = _lib.load()
    B, h, w, s, nu, tol = 4, 20, 28, 2.0, 0.1, 1e-9
    F = B - 2
    flows = _flows(h, w, 3000 + seed, B=B)
    nws = lib.pivlfn_pressure_workspace_bytes(F, h, w)

    def call(i, o, a, ws, st):
        from test_gpu_op_streams import _first
        return _first(lib.pivlfn_pressure_gradient(_p(i[0]), B, h, w, s, nu, _p(o[0]), _p(o[1]), st),
                      lib.pivlfn_pressure_setup(_p(o[0]), _p(o[1]), F, h, w, s, _p(ws[0]), nws, st),
                      lib.pivlfn_pressure_cg(_p(ws[0]), nws, F, h, w, tol, 5, st), lib.pivlfn_pressure_cg(_p(ws[0]), nws, F, h, w, tol, 7, st),
                      lib.pivlfn_pressure_read(_p(ws[0]), nws, F, h, w, _p(o[2]), _p(o[3]), _p(o[4]), st))

    def pin(outs):
        g, valid = pr.gradient(flows, s, nu)
        p, flag, status, _ = pr.solve(g, valid, s, tol, 12)
        for got, want in zip(outs, (g, valid, p, flag, status)):
            assert pr.same_bits(got.cpu().numpy(), want)
        assert (status[:, 1] == 12).all()
    outs = [((F, 2, h, w), F64), ((F, h, w), U8), ((F, h, w), F64), ((F, h, w), U8), ((F, 4), F64)]
    return Spec([torch.from_numpy(flows)], outs, [], [nws], call, pin, (h, w))


@pytest.fixture()
def as_an_op(monkeypatch):
    """The helpers of test_gpu_op_streams look an op up by name: "pressure" resolves to the spec above."""
    import test_gpu_op_streams as ops
    original = ops._get
    monkeypatch.setattr(ops, "_get", lambda op, seed, quad=False: _spec(seed, quad) if op == "pressure" else original(op, seed, quad))
    return ops


def test_eager_result_is_the_restatements(dev, as_an_op):
    _, outs, _, _ = as_an_op._eager("pressure", 31, dev)
    _spec(31).pin(outs)


def test_runs_in_order_on_the_stream_it_is_given(dev, delay, as_an_op):        # noqa: F811
    """On a side stream behind a long-running chain of matrix products and the copy of the real flows into a poisoned buffer, enqueued
    without a host synchronisation: the eager result, bit for bit, and every guard intact."""
    still_waiting, got, ref, buffers = _behind_the_delay("pressure", dev, delay, lambda stream: stream.cuda_stream)
    assert still_waiting, "the delay ran out before the op was enqueued: the test would not see a launch on another stream"
    for g, want in zip(got, ref):
        assert _same(g, want), "the result behind a delay on a side stream differs from the eager result"
    for t in buffers:
        _check(t, "pressure")


def test_is_graph_capturable(dev, as_an_op):
    as_an_op.test_op_is_graph_capturable("pressure", dev)


def test_pointers_one_element_off_give_the_same_bits(dev, as_an_op):
    as_an_op.test_pointers_one_element_off_give_the_same_bits("pressure", dev)


@pytest.mark.parametrize("h,w", [(22, 46), (33, 68)])
def test_guarded_buffers(h, w, dev):
    """Every buffer between guards -- the workspace exactly as large as the query says --: every guard intact, no input written, the
    bits of the restatement.  33 x 68: 2244 nodes, three workgroups per frame, the last with 196 nodes of its 1024 leaves."""
    from pivlfn import _lib
    lib = _lib.load()
    B, s, nu, tol = 4, 2.0, 0.1, 1e-9                  # F*h*w a multiple of 4: the byte buffers are whole 32-bit words
    F = B - 2
    flows = _flows(h, w, 900 + w, B=B)
    nws = lib.pivlfn_pressure_workspace_bytes(F, h, w)
    assert nws % 4 == 0
    fl = guarded(flows.shape, F32, dev, "nan")
    fl.copy_(torch.from_numpy(flows))
    g, valid, ws = guarded((F, 2, h, w), F64, dev, "sentinel"), guarded((F, h, w), U8, dev, "sentinel"), guarded((nws,), U8, dev, "sentinel")
    p, flag, status = guarded((F, h, w), F64, dev, "sentinel"), guarded((F, h, w), U8, dev, "sentinel"), guarded((F, 4), F64, dev, "sentinel")
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.pivlfn_pressure_gradient(_p(fl), B, h, w, s, nu, _p(g), _p(valid), st), "gradient")
    _lib.check(lib.pivlfn_pressure_setup(_p(g), _p(valid), F, h, w, s, _p(ws), nws, st), "setup")
    _lib.check(lib.pivlfn_pressure_cg(_p(ws), nws, F, h, w, tol, 9, st), "cg")
    _lib.check(lib.pivlfn_pressure_read(_p(ws), nws, F, h, w, _p(p), _p(flag), _p(status), st), "read")
    torch.cuda.synchronize()
    wg, wvalid = pr.gradient(flows, s, nu)
    wp, wflag, wstatus, _ = pr.solve(wg, wvalid, s, tol, 9)
    for got, want in zip((g, valid, p, flag, status), (wg, wvalid, wp, wflag, wstatus)):
        assert pr.same_bits(got.cpu().numpy(), want)
    for t in (fl, g, valid, ws, p, flag, status):
        check_guards(t, f"pressure {h}x{w}")
    assert torch.equal(fl.view(torch.int32), torch.from_numpy(flows).to(dev).view(torch.int32)), "the flows were written"


def test_every_error_is_refused_before_any_launch(dev):
    """The refusals of tests/test_pressure.py with real device buffers: everything keeps every byte."""
    from pivlfn import _lib
    from test_pressure import refusals
    lib = _lib.load()
    arena = _scribble(torch.empty(7 << 16, dtype=torch.uint8, device=dev))      # seven regions 64 KiB apart: only what a case moves overlaps
    assert arena.data_ptr() % 8 == 0
    refusals(lib, *(arena.data_ptr() + (i << 16) for i in range(7)), 5, 8, 9)
    torch.cuda.synchronize()
    assert bool((arena == 0xFF).all())


# ---- run.py -----------------------------------------------------------------------------------------------------------------------------
def test_run_py_pressure(tmp_path, dev, capsys):
    """run.py --pressure 2 on a 7-frame 64 x 64 sequence (6 pairs, 4 centred) with --validate flag: <name>_pres.flo for every pair but the
    first and the last, with the bits of a PressureField fed the written flows and the validation flags; pressure.json; a picture with
    --pressure-image."""
    import PIL.Image
    import run as runpy
    from pivlfn import ParticleImageGen, PressureField
    from pivlfn import validate as V
    from pivlfn.flo import read_flow
    H = W = 64
    seq = tmp_path / "seq"
    seq.mkdir()
    gen = ParticleImageGen(density=0.05, seed=9, device=dev)
    x, y, z, d = gen.random_particle(H, W, pad=8)
    for k in range(7):                                 # the particles swing along x: the flow changes from pair to pair
        frame = gen.generate_image(x + 1.5 * np.sin(2 * np.pi * k / 8), y, z, d, H, W)
        PIL.Image.fromarray(frame.cpu().numpy()).save(str(seq / f"f{k:03d}.png"))
    val = ["--validate", "flag", "--validate-radius", "2", "--validate-eps", "0.01", "--validate-thresh", "0.5"]
    params = ["--pressure", "2", "--pressure-rho", "2.5", "--pressure-nu", "0.01", "--pressure-dt", "0.5", "--pressure-calib", "0.25",
              "--pressure-tol", "1e-7", "--pressure-image"]
    assert runpy.main(["--model", "piv", "-i", str(seq), "-o", str(tmp_path / "out"), "--batch", "4"] + val + params) == 6
    assert "Pressure of 4 pairs" in capsys.readouterr().out
    out = tmp_path / "out" / "piv-synthetic" / "seq"
    flos = sorted(f for f in os.listdir(out / "flow") if f.endswith("_out.flo"))
    assert len(flos) == 6
    names = [f[:-len("_out.flo")] for f in flos]
    have = sorted(f for f in os.listdir(out / "flow") if f.endswith("_pres.flo"))
    assert have == [f"{n}_pres.flo" for n in names[1:-1]]
    assert sorted(f for f in os.listdir(out / "flow") if f.endswith("_pres.png")) == [f"{n}_pres.png" for n in names[1:-1]]
    flows = torch.stack([torch.from_numpy(read_flow(str(out / "flow" / f))).permute(2, 0, 1) for f in flos]).contiguous().to(dev)
    flags = V.validate_flow(flows, radius=2, spacing=1, eps=0.01, thresh=0.5, mode="flag").flag
    pf = PressureField(H, W, 2, calib=0.25, dt=0.5, rho=2.5, nu=0.01, tol=1e-7, device=dev)
    res = pf.update(flows, flags)
    assert len(res) == 4
    doc = json.load(open(out / "pressure.json"))
    assert (doc["cell"], doc["rho"], doc["nu"], doc["dt"], doc["calib"], doc["tol"], doc["validation"]) == (2, 2.5, 0.01, 0.5, 0.25, 1e-7, "flag")
    assert doc["lattice"] == [32, 32] and doc["max_iter"] == 370 and list(doc["pairs"]) == names[1:-1]
    assert doc["unconverged"] == int((~res.converged).sum())
    summary = res.summary()["frames"]
    for f, name in enumerate(names[1:-1]):
        bands = read_flow(str(out / "flow" / f"{name}_pres.flo"))
        assert bands.shape == (32, 32, 2) and bands.dtype == np.float32
        assert pr.same_bits(np.ascontiguousarray(bands), runpy.pressure_bands(res.p[f], res.grad[f], res.flag[f]))
        ok = res.flag[f] == 0
        assert (bands[~ok] == np.float32(1e10)).all() and 0 < ok.sum() < 32 * 32 and np.isfinite(bands[ok]).all()
        assert doc["pairs"][name] == runpy.json_strict(summary[f])
        assert doc["pairs"][name]["ok"] == int(ok.sum()) and doc["pairs"][name]["iterations"] == int(res.iterations[f])
