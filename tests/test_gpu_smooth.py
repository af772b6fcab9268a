"""GPU: pivlfn.smooth -- the fp64 2-D DCT on the matrix cores against scipy.fft, and the penalised-least-squares solve against the dense
and the sparse operator of tests/smooth_restatement.py and, iteration by iteration, against its restatement of the contract (section 5b:
the frames with several workgroups a system and several blocks a matrix product).

Bounds.  Transform: elementwise (H + W + 16) 2^-52 (|C_H| |X| |C_W|^T), the forward error bound of the two chained products plus a few
ulp for the table entries (numpy's own product stays under 0.31 of it on these shapes).  Solve, from the GPU's fp64 z, with
r = W y - A z formed in numpy:  |r| <= 2 tol |W y|  (the factor 2 covers the gap between the recursively updated residual and the
recomputed one) and |z - z_direct| <= 2 |r| / lambda_min(A)."""
import json
import os

import numpy as np
import pytest
import torch
from scipy.fft import dctn, idctn

import smooth_restatement as sr
from guarded import check_guards, guarded
from pivlfn import _lib, smooth
from pivlfn.flo import read_flow

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 9), (5, 7), (63, 65), (64, 64), (65, 130), (129, 31)]       # one tile, ragged tiles, around the K chunk of 32
TOL = 1e-8


def _planes(P, H, W, seed):
    """Values spread over six decades, both signs."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((P, H, W)) * 10.0 ** rng.uniform(-3.0, 3.0, (P, H, W))


# ---- 1. the transform -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_dct2_against_scipy(H, W, dev):
    x = _planes(3, H, W, 100 * H + W)
    xd = torch.from_numpy(x).to(dev)
    fwd, inv = smooth.dct2(xd), smooth.dct2(xd, inverse=True)
    back = smooth.dct2(fwd, inverse=True)
    fb, ib = sr.dct_bound(x), sr.dct_bound(x, inverse=True)
    ef = np.abs(fwd.cpu().numpy() - dctn(x, axes=(1, 2), norm="ortho"))
    ei = np.abs(inv.cpu().numpy() - idctn(x, axes=(1, 2), norm="ortho"))
    er = np.abs(back.cpu().numpy() - x)
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"{H}x{W}: forward {np.nanmax(ef / fb):.3f}, inverse {np.nanmax(ei / ib):.3f}, round trip {np.nanmax(er / fb):.3f} of the bound")
    assert (ef <= fb).all() and (ei <= ib).all()
    assert (er <= fb).all()
    for p in range(3):                                                      # a plane alone and inside the batch
        assert torch.equal(smooth.dct2(xd[p:p + 1])[0], fwd[p]) and torch.equal(smooth.dct2(xd[p], inverse=True), inv[p])


@pytest.mark.parametrize("H,W", [(5, 7), (65, 130)])
def test_dct2_writes_nothing_outside_its_output(H, W, dev):
    lib = _lib.load()
    x = _planes(2, H, W, 7)
    want = smooth.dct2(torch.from_numpy(x).to(dev))
    xin = guarded((2, H, W), torch.float64, dev)
    out = guarded((2, H, W), torch.float64, dev)
    xin.copy_(torch.from_numpy(x))
    nbytes = lib.pivlfn_dct2_workspace_bytes(2, H, W)
    ws = guarded((nbytes // 8,), torch.float64, dev)                       # dirty: the guards' NaN pattern fills the payload too
    assert lib.pivlfn_dct2(xin.data_ptr(), out.data_ptr(), 2, H, W, 0, ws.data_ptr(), nbytes, _lib.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    for t, name in ((xin, "x"), (out, "out"), (ws, "workspace")):
        check_guards(t, name)
    assert torch.equal(xin.cpu(), torch.from_numpy(x))


# ---- 2. the solve against the dense operator ---------------------------------------------------------------------------------------------
CASES = [(24, 20, 1), (33, 17, 2)]


@pytest.fixture(scope="module")
def fields():
    return {(H, W): sr.solve_case(H, W, seed) for H, W, seed in CASES}


def _check_solve(res, flow, w, s, what, dense=True):
    """Frame 0 of a result against the operator: sr.check_solve's three assertions on each component."""
    z = res.z.cpu().numpy()
    assert res.converged.all(), (what, res.state, res.residual)
    for c in range(2):
        ref = sr.solve_reference(w, flow[c].astype(np.float64), s, TOL, dense=dense)
        sr.check_solve(z[0, c], res.iterations[0, c], ref, f"{what} c={c}")


@pytest.mark.parametrize("s", [0.05, 1.0, 50.0])
@pytest.mark.parametrize("H,W,seed", CASES)
def test_solve_against_the_dense_operator(H, W, seed, s, fields, dev):
    flow, mask = fields[(H, W)]
    res = smooth.smooth_flow(torch.from_numpy(flow[None]).to(dev), s=s, mask=torch.from_numpy(mask[None]).to(dev), tol=TOL)
    _check_solve(res, flow, sr.weights_of(flow, None, mask), s, f"{H}x{W} s={s}")
    assert torch.equal(res.filled[0].cpu(), torch.from_numpy(mask != 0))
    assert torch.equal(res.flow, res.z.to(torch.float32))


def test_solve_with_fractional_weights(fields, dev):
    flow, mask = fields[(24, 20)]
    wts = np.random.default_rng(5).uniform(0.05, 1.0, mask.shape).astype(np.float32)
    res = smooth.smooth_flow(torch.from_numpy(flow[None]).to(dev), s=1.0, weights=torch.from_numpy(wts[None]).to(dev),
                             mask=torch.from_numpy(mask[None]).to(dev), tol=TOL)
    _check_solve(res, flow, sr.weights_of(flow, wts, mask), 1.0, "24x20 fractional weights")


# ---- 3. no gaps, unit weights ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(33, 17), (70, 131)])                      # one matrix block; 3 x 2 of them: Gamma at m0, n0 > 0
def test_without_gaps_the_start_is_the_solution(H, W, fields, dev):
    flow = fields[(H, W)][0] if (H, W) in fields else sr.solve_case(H, W, 3)[0]
    s = 3.0
    res = smooth.smooth_flow(torch.from_numpy(flow[None]).to(dev), s=s, tol=TOL)
    assert (res.iterations == 0).all() and res.converged.all() and (res.state == smooth.CONVERGED).all()
    assert not res.filled.any()
    y = flow.astype(np.float64)
    spec = dctn(y, axes=(1, 2), norm="ortho")
    g = sr.gamma(H, W, s)
    want = idctn(g * spec, axes=(1, 2), norm="ortho")
    # test 1's two bounds: the inverse's own on what it is given, and the forward's carried through Gamma and the inverse's tables
    carried = np.abs(sr.dct_table(H)).T @ (g * sr.dct_bound(y)) @ np.abs(sr.dct_table(W))
    err = np.abs(res.z[0].cpu().numpy() - want)
    print(f"no gaps {H}x{W}: {float((err / (sr.dct_bound(g * spec, inverse=True) + carried)).max()):.3f} of the bound")
    assert (err <= sr.dct_bound(g * spec, inverse=True) + carried).all()


# ---- 4. gaps are data-free ---------------------------------------------------------------------------------------------------------------
def test_the_value_of_a_gap_is_never_read(fields, dev):
    flow, mask = fields[(24, 20)]
    m = torch.from_numpy(mask[None]).to(dev)
    outs = []
    for fill in (float("nan"), 1e10, 1e30, -3.0):
        f = flow.copy()
        f[:, mask != 0] = fill
        outs.append(smooth.smooth_flow(torch.from_numpy(f[None]).to(dev), s=1.0, mask=m, tol=TOL))
    for o in outs[1:]:
        assert torch.equal(o.z, outs[0].z) and torch.equal(o.status, outs[0].status)
    assert torch.isfinite(outs[0].z).all()
    # the unknown rule alone marks the first three as gaps as well
    f = flow.copy()
    f[0, mask != 0] = np.nan
    unmasked = smooth.smooth_flow(torch.from_numpy(f[None]).to(dev), s=1.0, tol=TOL)
    assert torch.equal(unmasked.z, outs[0].z) and torch.equal(unmasked.filled[0].cpu(), torch.from_numpy(mask != 0))


def test_a_constant_field_with_holes_stays_constant(fields, dev):
    _, mask = fields[(24, 20)]
    flow = np.full((2, 24, 20), -2.5, dtype=np.float32)
    res = smooth.smooth_flow(torch.from_numpy(flow[None]).to(dev), s=1.0, mask=torch.from_numpy(mask[None]).to(dev), tol=TOL)
    w = sr.weights_of(flow, None, mask)
    A, lmin = sr.operator(w, 1.0), sr.lambda_min(w, 1.0)
    for c in range(2):
        z = res.z[0, c].cpu().numpy()
        r = sr.rhs(w, flow[c].astype(np.float64)).ravel() - A @ z.ravel()
        assert np.linalg.norm(z + 2.5) <= 2.0 * np.linalg.norm(r) / lmin + 1e-300
    assert res.converged.all()


def test_an_empty_frame_reads_back_unknown_and_leaves_its_neighbours_alone(fields, dev):
    flow, mask = fields[(24, 20)]
    flows = torch.from_numpy(np.stack([flow, flow[::-1].copy(), 2.0 * flow])).to(dev)
    masks = torch.from_numpy(np.stack([mask, np.ones_like(mask), mask])).to(dev)
    res = smooth.smooth_flow(flows, s=1.0, mask=masks, tol=TOL)
    assert (res.state[1] == smooth.EMPTY).all() and (res.z[1] == 1e10).all() and (res.flow[1] == 1e10).all() and res.filled[1].all()
    assert res.converged.all()
    for k in (0, 2):
        alone = smooth.smooth_flow(flows[k:k + 1], s=1.0, mask=masks[k:k + 1], tol=TOL)
        assert torch.equal(alone.z[0], res.z[k]) and torch.equal(alone.status[0], res.status[k])


# ---- 5. independence ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch(fields):
    flow, mask = fields[(33, 17)]
    rng = np.random.default_rng(11)
    masks = np.stack([mask, (rng.random(mask.shape) < 0.3).astype(np.uint8), np.roll(mask, 5, axis=0)])
    flows = np.stack([flow, 0.5 * flow[::-1], flow + 1.0]).astype(np.float32)
    return flows, masks


def test_a_frame_does_not_depend_on_its_batch(batch, dev):
    flows, masks = torch.from_numpy(batch[0]).to(dev), torch.from_numpy(batch[1]).to(dev)
    together = smooth.smooth_flow(flows, s=0.05, mask=masks, tol=TOL)
    assert together.converged.all() and len(set(together.iterations.ravel().tolist())) > 1       # the systems do stop at different times
    for k in range(3):
        alone = smooth.smooth_flow(flows[k:k + 1], s=0.05, mask=masks[k:k + 1], tol=TOL)
        assert torch.equal(alone.z[0], together.z[k]) and torch.equal(alone.status[0], together.status[k])
        assert np.array_equal(alone.iterations[0], together.iterations[k])


def test_how_the_iterations_are_cut_changes_no_bit(batch, dev):
    flows, masks = torch.from_numpy(batch[0]).to(dev), torch.from_numpy(batch[1]).to(dev)
    want = smooth.smooth_flow(flows, s=0.05, mask=masks, tol=TOL, max_iter=60, sync_every=None)
    for every in (1, 7):
        got = smooth.smooth_flow(flows, s=0.05, mask=masks, tol=TOL, max_iter=60, sync_every=every)
        assert torch.equal(got.z, want.z) and torch.equal(got.status, want.status), every
    # the ABI: 5 + 5 + ... against one call of 60
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    B, H, W = 3, 33, 17
    nbytes = lib.pivlfn_smooth_workspace_bytes(B, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    z, status = torch.empty_like(want.z), torch.empty_like(want.status)
    assert lib.pivlfn_smooth_setup(flows.data_ptr(), None, masks.data_ptr(), B, H, W, 0.05, ws.data_ptr(), nbytes, st) == 0
    for _ in range(12):
        assert lib.pivlfn_smooth_pcg(ws.data_ptr(), nbytes, B, H, W, 0.05, TOL, 5, st) == 0
    assert lib.pivlfn_smooth_read(ws.data_ptr(), nbytes, B, H, W, z.data_ptr(), None, None, status.data_ptr(), st) == 0
    assert torch.equal(z, want.z) and torch.equal(status, want.status)


def test_u_and_v_swapped_give_swapped_outputs(batch, dev):
    flows, masks = torch.from_numpy(batch[0][:1]).to(dev), torch.from_numpy(batch[1][:1]).to(dev)
    a = smooth.smooth_flow(flows, s=1.0, mask=masks, tol=TOL)
    b = smooth.smooth_flow(flows.flip(1).contiguous(), s=1.0, mask=masks, tol=TOL)
    assert torch.equal(a.z.flip(1), b.z) and torch.equal(a.status.flip(1), b.status)


def test_a_capped_frame_is_reported_unconverged(batch, dev):
    flows, masks = torch.from_numpy(batch[0][:1]).to(dev), torch.from_numpy(batch[1][:1]).to(dev)
    res = smooth.smooth_flow(flows, s=0.05, mask=masks, tol=TOL, max_iter=2)
    assert not res.converged.any() and (res.iterations == 2).all() and (res.state == smooth.RUNNING).all()
    assert res.summary()["unconverged"] == 1


def _smooth_shapes():
    import analysis_plans as ap
    return ap.shapes(ap.SMOOTH_CASES)


@pytest.mark.parametrize("H,W", _smooth_shapes())
def test_bb_where_the_partials_plan_changes(H, W, dev):
    """One frame, unit weights, no mask, setup and the read-out with no iteration between them.  513 x 512: 257 partials, one in the
    second wave of pr_finish; 1024 x 1025: 1025, one in its second chunk; 2048 x 1025 and 2048 x 2049: two and four chunks per workgroup,
    PrCounter and its carry.  With unit weights b = y exactly and b*b rounds once, so bb = T(b*b) of a system is the restated tree over
    y^2 bit for bit: the walk of csrc/cg_shared.h, its counters and pr_finish on the smoothing side."""
    import analysis_plans as ap
    import pressure_restatement as pr
    plan = ap.pressure(H, W)
    assert plan["NB"] > 256
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    y = np.random.default_rng(1000 * H + W).standard_normal((1, 2, H, W)).astype(np.float32)
    flow = torch.from_numpy(y).to(dev)
    nbytes = lib.pivlfn_smooth_workspace_bytes(1, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    z = torch.empty(1, 2, H, W, dtype=torch.float64, device=dev)
    status = torch.empty(1, 2, 4, dtype=torch.float64, device=dev)
    assert lib.pivlfn_smooth_setup(flow.data_ptr(), None, None, 1, H, W, 1.0, ws.data_ptr(), nbytes, st) == 0, lib.pivlfn_last_error()
    assert lib.pivlfn_smooth_read(ws.data_ptr(), nbytes, 1, H, W, z.data_ptr(), None, None, status.data_ptr(), st) == 0, lib.pivlfn_last_error()
    got = status.cpu().numpy()[0]
    for c in range(2):
        want = pr.tree((y[0, c].astype(np.float64)) ** 2)
        print(f"{H}x{W} c={c}: NB = {plan['NB']}, chunks = {plan['chunks']}, bb = {got[c, 3]!r}, restated {want!r}")
        assert pr.same_bits(got[c, 3], want), (H, W, c, got[c, 3], want)
        assert got[c, 0] == smooth.RUNNING and got[c, 1] == 0


# ---- 5b. across tile seams and matrix blocks -----------------------------------------------------------------------------------------------
# The frames of analysis_plans.SMOOTH_SOLVE_CASES: several workgroups a system, several 64 x 64 blocks a matrix product.
SEAM_SEED = 3


def _solve_cases():
    import analysis_plans as ap
    return ap.shapes(ap.SMOOTH_SOLVE_CASES)


@pytest.fixture(scope="module")
def seam_fields():
    """(H, W) -> (flow, mask, fractional weights), computed once and never changed."""
    out = {}
    for H, W, _ in _solve_cases():
        flow, mask = sr.seam_case(H, W, SEAM_SEED)
        out[(H, W)] = (flow, mask, np.random.default_rng(5).uniform(0.05, 1.0, mask.shape).astype(np.float32))
    return out


SPARSE = [(H, W, s, False) for H, W, _ in _solve_cases()[:2] for s in (0.05, 1.0, 50.0)] + [(70, 131, 1.0, True)]       # no direct solve at 513 x 512
TRAJECTORY = [(H, W, iters, s, False) for H, W, iters in _solve_cases() for s in (0.05, 1.0, 50.0)] + [(70, 131, 6, 1.0, True)]


@pytest.mark.parametrize("H,W,s,fractional", SPARSE)
def test_solve_against_the_sparse_operator(H, W, s, fractional, seam_fields, dev):
    flow, mask, wts = seam_fields[(H, W)]
    wts = wts if fractional else None
    res = smooth.smooth_flow(torch.from_numpy(flow[None]).to(dev), s=s, weights=None if wts is None else torch.from_numpy(wts[None]).to(dev),
                             mask=torch.from_numpy(mask[None]).to(dev), tol=TOL)
    w = sr.weights_of(flow, wts, mask)
    _check_solve(res, flow, w, s, f"{H}x{W} s={s}{' fractional weights' if fractional else ''}", dense=False)
    assert torch.equal(res.filled[0].cpu(), torch.from_numpy(w == 0))
    assert torch.equal(res.flow, res.z.to(torch.float32))


@pytest.mark.parametrize("H,W,iters,s,fractional", TRAJECTORY)
def test_rr_follows_the_restated_iteration(H, W, iters, s, fractional, seam_fields, dev):
    """Through the ABI: setup, then alternately read and pcg(.., 1) with tol = 1e-30, so that no system stops.  status reports iteration k
    and rr_k within max(64 Y, 1e-11) of the restated iteration's (sr.check_trajectory; Y is the distance between two fp64 evaluations
    of the recurrence on the CPU), bb is the restated tree bit for bit, x after the last compared iteration lies within 64 times
    numpy's distance from the restated x, and a read changes no byte of the workspace.

    The largest share of the rr bound (and of the x bound) on the MI355X, over both components:
        s =        0.05            1.0             50.0            1.0, weights in [0.05, 1]
        37 x 61    0.036 (0.022)   0.005 (0.016)   0.012 (0.016)
        70 x 131   0.004 (0.017)   0.011 (0.021)   0.052 (0.016)   0.003 (0.021)
        513 x 512  0.003 (0.033)   0.002 (0.020)   0.039 (0.016)
    (1/64 = 0.016 of the x bound: as far from the restated x as numpy is, one or two ulp.)  A Gamma epilogue without m0, built into the
    library, misses the rr bound by 1e12 and more at 70 x 131 and 513 x 512 and passes test_solve_against_the_sparse_operator at s = 0.05."""
    import pressure_restatement as pr
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    flow, mask, wts = seam_fields[(H, W)]
    wts = wts if fractional else None
    w = sr.weights_of(flow, wts, mask)
    refs = [sr.trajectory_reference(w, flow[c].astype(np.float64), s, iters) for c in range(2)]
    bb = [pr.tree(sr.rhs(w, flow[c].astype(np.float64)) ** 2) for c in range(2)]
    fd, md = torch.from_numpy(flow[None]).to(dev), torch.from_numpy(mask[None]).to(dev)
    wd = None if wts is None else torch.from_numpy(wts[None]).to(dev)
    nbytes = lib.pivlfn_smooth_workspace_bytes(1, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    z = torch.empty(1, 2, H, W, dtype=torch.float64, device=dev)
    status = torch.empty(1, 2, 4, dtype=torch.float64, device=dev)
    assert lib.pivlfn_smooth_setup(fd.data_ptr(), None if wd is None else wd.data_ptr(), md.data_ptr(), 1, H, W, s, ws.data_ptr(), nbytes,
                                   st) == 0, lib.pivlfn_last_error()
    rr, zs = [], []
    for k in range(iters + 1):
        before = ws.clone()
        assert lib.pivlfn_smooth_read(ws.data_ptr(), nbytes, 1, H, W, z.data_ptr(), None, None, status.data_ptr(), st) == 0, lib.pivlfn_last_error()
        assert torch.equal(ws, before), f"the read-out after {k} iterations changed the workspace"
        got = status.cpu().numpy()[0]
        assert (got[:, 0] == smooth.RUNNING).all() and (got[:, 1] == k).all(), (k, got)
        rr.append(got[:, 2].copy())
        zs.append(z.cpu().numpy()[0])
        for c in range(2):
            assert pr.same_bits(got[c, 3], bb[c]), (k, c, got[c, 3], bb[c])
        if k < iters:
            assert lib.pivlfn_smooth_pcg(ws.data_ptr(), nbytes, 1, H, W, s, 1e-30, 1, st) == 0, lib.pivlfn_last_error()
    rr = np.array(rr)
    for c in range(2):
        what = f"{H}x{W} s={s}{' fractional' if fractional else ''} c={c}"
        sr.check_trajectory(rr[:, c], refs[c], what)
        sr.check_iterate(zs[refs[c]["K"]][c], refs[c], what)


@pytest.fixture(scope="module")
def seam_batch(seam_fields):
    """70 x 131, B = 3: frame 1 fully masked, frames 0 and 2 with different flows and masks."""
    flow, mask, _ = seam_fields[(70, 131)]
    rng = np.random.default_rng(11)
    masks = np.stack([mask, np.ones_like(mask), np.roll(mask, 7, axis=0) | (rng.random(mask.shape) < 0.2).astype(np.uint8)])
    flows = np.stack([flow, 0.5 * flow[::-1], flow[:, ::-1] + 1.0]).astype(np.float32)
    return flows, masks


def test_batch_cuts_and_frozen_systems(seam_batch, dev):
    B, H, W, s, cap = 3, 70, 131, 0.05, 100
    flows, masks = torch.from_numpy(seam_batch[0]).to(dev), torch.from_numpy(seam_batch[1]).to(dev)
    want = smooth.smooth_flow(flows, s=s, mask=masks, tol=TOL, max_iter=cap, sync_every=None)
    its = want.iterations
    print(f"iterations {its.tolist()}, states {want.state.tolist()}")
    assert want.converged.all() and (want.state[1] == smooth.EMPTY).all() and (want.state[[0, 2]] == smooth.CONVERGED).all()
    assert len(set(its[[0, 2]].ravel().tolist())) > 1 and its.max() < cap - 5     # the systems do stop at different iterations
    assert (want.z[1] == 1e10).all() and want.filled[1].all()
    for k in range(B):                                                      # a frame alone
        alone = smooth.smooth_flow(flows[k:k + 1], s=s, mask=masks[k:k + 1], tol=TOL, max_iter=cap)
        assert torch.equal(alone.z[0], want.z[k]) and torch.equal(alone.status[0], want.status[k]), k
    for every in (1, 7):                                                    # how the iterations are cut
        got = smooth.smooth_flow(flows, s=s, mask=masks, tol=TOL, max_iter=cap, sync_every=every)
        assert torch.equal(got.z, want.z) and torch.equal(got.status, want.status), every
    swapped = smooth.smooth_flow(flows.flip(1).contiguous(), s=s, mask=masks, tol=TOL, max_iter=cap)
    assert torch.equal(swapped.z, want.z.flip(1)) and torch.equal(swapped.status, want.status.flip(1))
    # the ABI: every system has stopped after its.max() + 1 iterations (the last one applies the stopping rule); five more move nothing
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    nbytes = lib.pivlfn_smooth_workspace_bytes(B, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    z, status = torch.empty_like(want.z), torch.empty_like(want.status)
    assert lib.pivlfn_smooth_setup(flows.data_ptr(), None, masks.data_ptr(), B, H, W, s, ws.data_ptr(), nbytes, st) == 0
    assert lib.pivlfn_smooth_pcg(ws.data_ptr(), nbytes, B, H, W, s, TOL, int(its.max()) + 1, st) == 0
    assert lib.pivlfn_smooth_read(ws.data_ptr(), nbytes, B, H, W, z.data_ptr(), None, None, status.data_ptr(), st) == 0
    assert torch.equal(z, want.z) and torch.equal(status, want.status)
    assert (status[:, :, 0] != smooth.RUNNING).all()
    z.fill_(-1.0), status.fill_(-1.0)
    assert lib.pivlfn_smooth_pcg(ws.data_ptr(), nbytes, B, H, W, s, TOL, 5, st) == 0
    assert lib.pivlfn_smooth_read(ws.data_ptr(), nbytes, B, H, W, z.data_ptr(), None, None, status.data_ptr(), st) == 0
    assert torch.equal(z, want.z) and torch.equal(status, want.status)


def _guarded_bytes(n, dev):
    """n bytes whose last lies against the back guard.  guarded() takes whole 32-bit words: the 0..3 bytes of slack in front hold 0xA5.
    Returns (the guarded buffer, the n bytes)."""
    pad = -n % 4
    g = guarded((n + pad,), torch.uint8, dev)
    g[:pad] = 0xA5
    return g, g[pad:]


@pytest.mark.parametrize("kind", ["nan", "big"])
def test_guarded_solve(kind, seam_fields, dev):
    """37 x 61, B = 2, weights and mask: every buffer of setup, pcg and read between guards, the workspace dirty."""
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    B, H, W, s = 2, 37, 61, 1.0
    flow, mask, wts = seam_fields[(H, W)]
    flows = np.stack([flow, 0.5 * flow[:, ::-1] - 1.0]).astype(np.float32)
    masks = np.stack([mask, np.roll(mask, 9, axis=1)])
    weights = np.stack([wts, wts[::-1]]).astype(np.float32)
    want = smooth.smooth_flow(torch.from_numpy(flows).to(dev), s=s, weights=torch.from_numpy(weights).to(dev), mask=torch.from_numpy(masks).to(dev),
                              tol=TOL, max_iter=60, sync_every=None)
    print(f"guarded {kind}: iterations {want.iterations.tolist()}")
    assert want.converged.all() and (want.iterations > 3).all()
    fd = guarded((B, 2, H, W), torch.float32, dev)
    wd = guarded((B, H, W), torch.float32, dev)
    mg, md = _guarded_bytes(B * H * W, dev)
    fd.copy_(torch.from_numpy(flows)), wd.copy_(torch.from_numpy(weights)), md.copy_(torch.from_numpy(masks).view(-1))
    z = guarded((B, 2, H, W), torch.float64, dev, fill="sentinel")
    z32 = guarded((B, 2, H, W), torch.float32, dev, fill="sentinel")
    fg, filled = _guarded_bytes(B * H * W, dev)
    status = guarded((B, 2, 4), torch.float64, dev, fill="sentinel")
    nbytes = lib.pivlfn_smooth_workspace_bytes(B, H, W)
    assert nbytes % 8 == 0
    ws = guarded((nbytes // 8,), torch.float64, dev, fill=kind)            # dirty: the pattern fills the payload too
    assert lib.pivlfn_smooth_setup(fd.data_ptr(), wd.data_ptr(), md.data_ptr(), B, H, W, s, ws.data_ptr(), nbytes, st) == 0, lib.pivlfn_last_error()
    for _ in range(12):
        assert lib.pivlfn_smooth_pcg(ws.data_ptr(), nbytes, B, H, W, s, TOL, 5, st) == 0, lib.pivlfn_last_error()
    assert lib.pivlfn_smooth_read(ws.data_ptr(), nbytes, B, H, W, z.data_ptr(), z32.data_ptr(), filled.data_ptr(), status.data_ptr(),
                                  st) == 0, lib.pivlfn_last_error()
    torch.cuda.synchronize()
    assert torch.equal(z, want.z) and torch.equal(status, want.status) and torch.equal(z32, want.flow)
    assert torch.equal(filled.view(B, H, W).bool(), want.filled)
    for t, name in ((fd, "flows"), (wd, "weights"), (mg, "mask"), (z, "z"), (z32, "z32"), (fg, "filled"), (status, "status"), (ws, "workspace")):
        check_guards(t, name)
    for g in (mg, fg):
        assert (g[:-B * H * W] == 0xA5).all()
    assert torch.equal(fd.cpu(), torch.from_numpy(flows)) and torch.equal(wd.cpu(), torch.from_numpy(weights))
    assert torch.equal(md.cpu(), torch.from_numpy(masks).view(-1))


# ---- 6. stream and capture ---------------------------------------------------------------------------------------------------------------
def test_a_side_stream_gives_the_same_bits(batch, dev):
    flows, masks = torch.from_numpy(batch[0]).to(dev), torch.from_numpy(batch[1]).to(dev)
    x = torch.from_numpy(_planes(2, 65, 130, 3)).to(dev)
    want, want_dct = smooth.smooth_flow(flows, s=1.0, mask=masks, tol=TOL), smooth.dct2(x)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        got, got_dct = smooth.smooth_flow(flows, s=1.0, mask=masks, tol=TOL), smooth.dct2(x)
    side.synchronize()
    assert torch.equal(got.z, want.z) and torch.equal(got.status, want.status) and torch.equal(got_dct, want_dct)


def test_dct2_and_one_pcg_call_can_be_captured(batch, dev):
    lib = _lib.load()
    flows, masks = torch.from_numpy(batch[0]).to(dev), torch.from_numpy(batch[1]).to(dev)
    B, H, W = 3, 33, 17
    x = torch.from_numpy(_planes(2, H, W, 4)).to(dev)
    want_dct = smooth.dct2(x)
    want = smooth.smooth_flow(flows, s=1.0, mask=masks, tol=TOL, max_iter=4, sync_every=None)
    nbytes, dbytes = lib.pivlfn_smooth_workspace_bytes(B, H, W), lib.pivlfn_dct2_workspace_bytes(2, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dws = torch.empty(dbytes, dtype=torch.uint8, device=dev)
    out, z, status = torch.empty_like(x), torch.empty_like(want.z), torch.empty_like(want.status)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            st = _lib.stream_ptr(dev)
            rcs = [lib.pivlfn_dct2(x.data_ptr(), out.data_ptr(), 2, H, W, 0, dws.data_ptr(), dbytes, st),
                   lib.pivlfn_smooth_pcg(ws.data_ptr(), nbytes, B, H, W, 1.0, TOL, 4, st),
                   lib.pivlfn_smooth_read(ws.data_ptr(), nbytes, B, H, W, z.data_ptr(), None, None, status.data_ptr(), st)]
        assert rcs == [0, 0, 0], lib.pivlfn_last_error()
        for _ in range(2):                                                  # the setup is eager: each replay iterates a fresh workspace
            out.zero_()
            assert lib.pivlfn_smooth_setup(flows.data_ptr(), None, masks.data_ptr(), B, H, W, 1.0, ws.data_ptr(), nbytes,
                                           _lib.stream_ptr(dev)) == 0
            graph.replay()
            side.synchronize()
            assert torch.equal(out, want_dct) and torch.equal(z, want.z) and torch.equal(status, want.status)


# ---- 7. run.py -----------------------------------------------------------------------------------------------------------------------------
VALIDATE = ["--validate-radius", "2", "--validate-eps", "0.01", "--validate-thresh", "0.5"]


def test_run_py_smooth(tmp_path, dev):
    import PIL.Image
    import pivlfn
    import run as runpy
    from pivlfn import synth
    from pivlfn import validate as V
    from pivlfn.pipeline import read_image_u8, u8_to_input
    jj, ii = torch.meshgrid(torch.arange(64.0), torch.arange(64.0), indexing="ij")
    truth = torch.stack([torch.stack([2.0 * torch.sin(jj / (8.0 + k)), 1.5 * torch.cos(ii / (9.0 + k))]) for k in range(3)]).to(dev)
    img1, img2, _ = pivlfn.ParticleImageGen(seed=40, device=dev).create_pair_from_flow(truth.contiguous())
    seq = tmp_path / "seq"
    seq.mkdir()
    for k in range(3):
        PIL.Image.fromarray(img1[k].cpu().numpy()).save(str(seq / f"p{k}_img1.png"))
        PIL.Image.fromarray(img2[k].cpu().numpy()).save(str(seq / f"p{k}_img2.png"))
    net = pivlfn.Network(model="piv", params=synth.generate_weights("piv", 0)).to(dev).eval()
    a = torch.from_numpy(np.stack([read_image_u8(str(seq / f"p{k}_img1.png")) for k in range(3)])).to(dev)
    b = torch.from_numpy(np.stack([read_image_u8(str(seq / f"p{k}_img2.png")) for k in range(3)])).to(dev)
    est = torch.cat([pivlfn.estimate(net, u8_to_input(a[lo:hi]), u8_to_input(b[lo:hi]), tensor=True) for lo, hi in ((0, 2), (2, 3))])
    params = dict(radius=2, spacing=1, eps=0.01, thresh=0.5)
    masked = V.validate_flow(est, mode="mask", **params)
    assert int((masked.flag != 0).sum()) > 0

    def run(out, flags):
        assert runpy.main(["--model", "piv", "-i", str(seq), "-p", "--batch", "2", "-o", str(out)] + flags) == 3
        save = out / "piv-synthetic" / "seq"
        return save, [read_flow(str(save / "flow" / f"p{k}_out.flo")) for k in range(3)]

    save, got = run(tmp_path / "smooth", ["--validate", "mask", "--smooth", "8"] + VALIDATE)
    want = torch.cat([smooth.smooth_flow(est[lo:hi], wavelength=8.0, mask=masked.flag[lo:hi]).flow for lo, hi in ((0, 2), (2, 3))])
    doc = json.load(open(save / "smooth.json"))
    assert doc["unconverged"] == 0 and len(doc["pairs"]) == 3 and doc["wavelength"] == 8.0 and doc["validation"] == "mask"
    filled = (masked.flag != 0).flatten(1).sum(1).tolist()
    for k, (name, row) in enumerate(doc["pairs"].items()):
        assert row["converged"] and row["filled"] == filled[k] and f"p{k}" in name, (name, row)
        assert np.abs(got[k]).max() <= 1e9
        assert np.array_equal(got[k], want[k].permute(1, 2, 0).cpu().numpy())
    assert "smooth: 8.0\n" in list(open(save / "args.txt"))

    # without --smooth: what the files were before the flag existed
    save, got = run(tmp_path / "plain", ["--validate", "mask"] + VALIDATE)
    for k in range(3):
        assert np.array_equal(got[k], masked.flow[k].permute(1, 2, 0).cpu().numpy())
    lines = list(open(save / "args.txt"))
    assert not [ln for ln in lines if ln.startswith("smooth")] and not os.path.exists(save / "smooth.json")
    ref = runpy.parser.parse_args(["--model", "piv", "-i", str(seq), "-p", "--batch", "2", "-o", str(tmp_path / "plain"), "--validate", "mask"]
                                  + VALIDATE)
    assert lines == [f"{k}: {v}\n" for k, v in sorted(vars(ref).items())
                     if k not in runpy.PREP_FLAGS + runpy.TRUTH_FLAGS + runpy.VIZ_FLAGS]
