"""CPU: the pressure contract (include/pivlfn.h, pivlfn_pressure_*) as tests/pressure_restatement.py states it -- against the decaying
Taylor-Green vortex, whose pressure is known in closed form, and against a dense least-squares solution of the edge equations on small
lattices with holes --, the properties the contract states (zero degree-weighted mean per component, the stopping and the breakdown
rule), the refusals of the four C entry points, which all come before any launch and so need no GPU, the checks of
pivlfn.pressure.PressureField and PressureResult, and the command line of run.py --pressure."""
import math

import numpy as np
import pytest
import torch

import pressure_restatement as pr

EPS = 2.0 ** -52


# ---- the restatement itself ---------------------------------------------------------------------------------------------------------
def test_the_tree_is_the_contracts():
    leaves = np.array([1e16, 1.0, -1e16, 1.0, 3.0, 1e-3, 7.0])
    want = ((leaves[0] + leaves[1]) + (leaves[2] + leaves[3])) + ((leaves[4] + leaves[5]) + (leaves[6] + 0.0))
    assert pr.tree(leaves) == want and pr.tree(leaves.reshape(7, 1)) == want
    assert pr.tree(np.array([5.0])) == 5.0 and pr.tree(np.zeros((3, 3))) == 0.0


def test_gradient_by_hand_at_one_node():
    """3 x 3, one valid node: every term of the formula written out with Python floats."""
    rng = np.random.default_rng(1)
    flows = rng.normal(0, 2, (3, 2, 3, 3)).astype(np.float32)
    s, nu = 2.0, 0.25
    g, valid = pr.gradient(flows, s, nu)
    assert valid.sum() == 1 and valid[0, 1, 1] == 1
    c = flows[1].astype(np.float64)
    uc, vc = c[0, 1, 1], c[1, 1, 1]
    for a in range(2):
        at = (float(flows[2, a, 1, 1]) - float(flows[0, a, 1, 1])) * 0.5
        ax, ay = (c[a, 1, 2] - c[a, 1, 0]) / (2.0 * s), (c[a, 2, 1] - c[a, 0, 1]) / (2.0 * s)
        lap = ((((c[a, 1, 0] + c[a, 1, 2]) + c[a, 0, 1]) + c[a, 2, 1]) - 4.0 * c[a, 1, 1]) / (s * s)
        assert g[0, a, 1, 1] == (-(at + (uc * ax + vc * ay))) + nu * lap
    assert not g[0, :, 0].any() and not g[0, :, :, 0].any()
    # an unknown vector in the previous flow only, a NaN in a neighbour, the 1e10 of an empty cell: each takes the node out
    for where, value in (((0, 1, 1, 1), 1e10), ((1, 0, 0, 1), np.nan), ((2, 0, 1, 1), -2e9), ((1, 1, 1, 2), np.inf)):
        bad = flows.copy()
        bad[where] = value
        g2, v2 = pr.gradient(bad, s, nu)
        assert v2.sum() == 0 and not g2.any() and not np.signbit(g2).any()
    edge = flows.copy()
    edge[1, 0, 0, 0] = np.nan                                  # a corner is no neighbour of the centre
    assert pr.gradient(edge, s, nu)[1].sum() == 1


def test_setup_by_hand_on_two_nodes():
    """1 x 2 valid nodes: one edge, b = -+e, deg 1, and the initial scalars."""
    g = np.zeros((2, 3, 4))
    g[0, 1, 1], g[0, 1, 2] = 0.75, -0.25
    valid = np.zeros((3, 4), np.uint8)
    valid[1, 1:3] = 1
    fr = pr.Frame(g, valid, 2.0)
    e = (0.5 * (0.75 + -0.25)) * 2.0
    assert fr.b[1, 1] == -e and fr.b[1, 2] == e and fr.deg.sum() == 2 and fr.adj[1, 1] == 16 + 2 and fr.adj[1, 2] == 16 + 1
    assert fr.rho == fr.rr == fr.bb == 2 * e * e and fr.state == pr.RUNNING and fr.iterations == 0
    fr.run(1e-12, 5)
    p, flag, status = fr.read()
    assert status[0] == pr.CONVERGED and status[1] == 1 and abs((p[1, 2] - p[1, 1]) - e) < 1e-15
    assert np.isnan(p[0]).all() and (flag[0] == pr.INVALID).all() and flag[1, 1] == pr.OK


# ---- against the analytic field ---------------------------------------------------------------------------------------------------------
_tg = {}


def _taylor_green_error(size, lam):
    """(max |err| after removing both means over the ok nodes, the bound (2ks)^2/6 max|p|, the frame) at s = 1, A = 2, nu* = 0.5,
    tol 1e-10: three flows, the pressure of the middle one."""
    if (size, lam) not in _tg:
        flows, p = pr.taylor_green(3, size, size, lam, A=2.0, nu=0.5, s=1.0)
        g, valid = pr.gradient(flows, 1.0, 0.5)
        fr = pr.Frame(g[0], valid[0], 1.0).run(1e-10, 10 * size + 50)
        got, flag, status = fr.read()
        ok = flag == pr.OK
        assert status[0] == pr.CONVERGED and ok.sum() == (size - 2) ** 2
        err = np.abs((got[ok] - got[ok].mean()) - (p[1][ok] - p[1][ok].mean())).max()
        k = 2.0 * math.pi / lam
        _tg[(size, lam)] = (err, (2.0 * k) ** 2 / 6.0 * np.abs(p[1]).max(), int(status[1]))
    return _tg[(size, lam)]


@pytest.mark.parametrize("size,lam", [(64, 32), (64, 64), (256, 64)])
def test_taylor_green_pressure_within_the_truncation_of_the_central_difference(size, lam):
    """The integration differentiates nothing twice: its error is that of the central difference that made g, whose leading term at p's
    wavenumber 2k is (2ks)^2/6 of the amplitude."""
    err, bound, iters = _taylor_green_error(size, lam)
    print(f"{size} x {size}, lambda = {lam}: max |err| = {err:.4g}, bound {bound:.4g}, {iters} iterations")
    assert err <= bound


def test_taylor_green_error_falls_with_the_square_of_the_wavelength():
    e32, e64 = _taylor_green_error(64, 32)[0], _taylor_green_error(64, 64)[0]
    print(f"64 x 64: lambda 32 -> {e32:.4g}, lambda 64 -> {e64:.4g}, ratio {e32 / e64:.3g}")
    assert e32 >= 3.0 * e64


# ---- against a dense least-squares solution ---------------------------------------------------------------------------------------------
def _holey_case(seed, h, w):
    """Random flows on a small lattice; the middle column is unknown in the centre flow, which splits the valid nodes in two (the
    column and its two neighbours lose their validity), and one more vector is unknown."""
    rng = np.random.default_rng(seed)
    flows = pr.random_flows(rng, 3, h, w)
    flows[1, :, :, w // 2] = 1e10
    flows[0, 0, 2, 2] = np.nan
    return flows


@pytest.mark.parametrize("h,w,seed", [(9, 14, 0), (8, 20, 1), (12, 16, 2)])
def test_converged_restatement_equals_dense_least_squares(h, w, seed):
    """M p = e over the active edges, by numpy.linalg.lstsq, against CG run to tol = 1e-10, both re-referenced to zero plain mean on
    every connected component.

    Tolerance.  A = M^T M is the operator and b = M^T e the right-hand side of the iteration (the normal equations), so the least-squares
    solution p* satisfies A p* = b, and with both solutions mean-free per component the error err = x - p* is orthogonal to A's null
    space (the per-component constants).  There A err = -(b - A x), hence  |err|_2 <= |b - A x|_2 / smin^2  with smin the smallest
    non-zero singular value of M, and |b|_2 = |A p*|_2 <= smax^2 |p*|_2.  CG stops at |r|_2 <= tol |b|_2, so
        |err|_2 <= tol * cond^2 * |p*|_2,   cond = smax/smin from the singular values lstsq reports (its rank tells where zero starts).
    The recurrence's r differs from b - A x by the rounding gathered over k iterations, at most about k eps |A| |x| ~ k eps smax^2 |p*|,
    which adds k eps cond^2 to tol; lstsq's own error, cond eps |p*|, is below that.  max |err| <= |err|_2."""
    tol = 1e-10
    flows = _holey_case(seed, h, w)
    g, valid = pr.gradient(flows, 1.0, 0.1)
    fr = pr.Frame(g[0], valid[0], 1.0).run(tol, 1000)
    p, flag, status = fr.read()
    lab, n = pr.components(fr)
    assert status[0] == pr.CONVERGED and n == 2 and (fr.deg > 0).sum() <= 200 and (flag == pr.INVALID).sum() > 0
    M, rhs, idx = pr.edge_system(fr, g[0], 1.0)
    sol, _, rank, sv = np.linalg.lstsq(M, rhs, rcond=None)
    assert rank == M.shape[1] - n                                          # one constant per component
    cond = sv[0] / sv[rank - 1]
    want = np.full((h, w), np.nan)
    want[idx >= 0] = sol[idx[idx >= 0]]
    err2 = 0.0
    for c in range(n):
        m = lab == c
        d = (p[m] - p[m].mean()) - (want[m] - want[m].mean())
        err2 += float((d * d).sum())
        want[m] -= want[m].mean()
    bound = (tol + status[1] * EPS * cond * cond) * cond * cond * math.sqrt(float((want[idx >= 0] ** 2).sum()))
    print(f"{h} x {w}: cond {cond:.3g}, |err|_2 = {math.sqrt(err2):.3g}, bound {bound:.3g}, {int(status[1])} iterations")
    assert math.sqrt(err2) <= bound


def test_degree_weighted_mean_is_zero_on_every_component():
    """sum deg*x over a component is zero in exact arithmetic: x gathers alpha*d, sum deg*d = sum deg*z + beta sum deg*d, sum deg*z = sum r
    and sum r = sum b - alpha sum q with sum b = sum q = 0 (every edge enters two nodes with opposite signs).  In fp64 every iteration
    forms these sums from N_c rounded values of size at most deg*|x|-ish: the bound is eps * N_c * (k + 1) * 4 max|x|."""
    flows = _holey_case(5, 19, 23)
    g, valid = pr.gradient(flows, 2.0, 0.0)
    fr = pr.Frame(g[0], valid[0], 2.0).run(1e-10, 1000)
    lab, n = pr.components(fr)
    assert n == 2 and fr.state == pr.CONVERGED
    for c in range(n):
        m = lab == c
        total, bound = float((fr.deg[m] * fr.x[m]).sum()), EPS * m.sum() * (fr.iterations + 1) * 4.0 * np.abs(fr.x[m]).max()
        print(f"component {c}: {m.sum()} nodes, sum deg*x = {total:.3g}, bound {bound:.3g}; plain mean {fr.x[m].mean():.3g}")
        assert abs(total) <= bound


# ---- the stopping rules and PressureResult ----------------------------------------------------------------------------------------------
def _result(frames, tol, g, reference=None, scale_p=1.0):
    from pivlfn.pressure import PressureResult
    out = [fr.read() for fr in frames]
    p, flag, status = (torch.from_numpy(np.stack([o[k] for o in out])) for k in range(3))
    return PressureResult(p, torch.from_numpy(np.asarray(g)), flag, status, scale_p, 1.0, tol, reference)


def test_max_iter_reached_is_reported_as_not_converged():
    flows = pr.random_flows(np.random.default_rng(3), 3, 12, 12)
    g, valid = pr.gradient(flows, 1.0, 0.0)
    short, full = pr.Frame(g[0], valid[0], 1.0).run(1e-10, 3), pr.Frame(g[0], valid[0], 1.0).run(1e-10, 500)
    res = _result([short, full], 1e-10, np.stack([g[0], g[0]]))
    assert list(res.iterations) == [3, full.iterations] and list(res.state) == [pr.RUNNING, pr.CONVERGED]
    assert list(res.converged) == [False, True] and res.residual[0] > 1e-10 >= res.residual[1]
    s = res.summary()
    assert s["unconverged"] == 1 and s["frames"][0]["converged"] is False and s["frames"][0]["ok"] == 100 and s["frames"][0]["invalid"] == 44
    ok = res.flag[1] == 0
    assert abs(res.p[1][ok].mean()) < 1e-12 and np.isnan(res.p[1][~ok]).all()
    assert s["frames"][1]["p_min"] == res.p[1][ok].min() and abs(s["frames"][1]["p_rms"] - np.sqrt((res.p[1][ok] ** 2).mean())) < 1e-15
    at = _result([full], 1e-10, g[:1], reference=(5, 6), scale_p=3.0)
    assert at.p[0][5, 6] == 0.0 and np.allclose(at.p[0][ok], 3.0 * (full.x[ok] - full.x[5, 6]), rtol=0, atol=1e-15)
    assert np.isnan(_result([full], 1e-10, g[:1], reference=(0, 0)).p).all()          # an invalid node is no reference


def test_zero_right_hand_side_breaks_down_with_zero_pressure():
    """A uniform translation: g = 0, b = 0, sigma = 0: BREAKDOWN before the first step, x = 0 -- which is the solution."""
    flows = np.ones((3, 2, 6, 7), np.float32) * np.float32(1.5)
    g, valid = pr.gradient(flows, 1.0, 0.3)
    assert valid.sum() == 20 and not g.any()
    fr = pr.Frame(g[0], valid[0], 1.0).run(1e-8, 10)
    p, flag, status = fr.read()
    assert list(status) == [pr.BREAKDOWN, 0.0, 0.0, 0.0] and (p[flag == 0] == 0).all() and np.isnan(p[flag != 0]).all()
    res = _result([fr], 1e-8, g)
    assert res.converged[0] and res.residual[0] == 0.0 and (res.p[0][flag == 0] == 0).all()
    # no valid node at all: the same end, and no value anywhere
    none = pr.Frame(np.zeros((2, 1, 1)), np.zeros((1, 1), np.uint8), 1.0).run(1e-8, 3)
    assert none.state == pr.BREAKDOWN and np.isnan(none.read()[0]).all()
    iso = pr.Frame(np.ones((2, 3, 3)), pr.gradient(np.zeros((3, 2, 3, 3), np.float32), 1.0, 0.0)[1][0], 1.0).run(1e-8, 3)
    assert iso.read()[1][1, 1] == pr.ISOLATED and np.isnan(iso.read()[0]).all() and iso.state == pr.BREAKDOWN


def test_class_refuses_bad_parameters_before_any_tensor_exists():
    from pivlfn import PressureField, pressure
    good = dict(cell=4, calib=1.0, dt=1.0, rho=1.0, nu=0.0, tol=1e-8, max_iter=None, sync_every=64)
    pressure.check_params(**good)
    pressure.check_params(**dict(good, max_iter=0, sync_every=None, nu=1e-6))
    for key, bad in (("cell", 0), ("cell", 2.0), ("cell", True), ("cell", 32769), ("calib", 0.0), ("calib", math.nan), ("dt", -1.0),
                     ("dt", math.inf), ("rho", 0), ("rho", "1"), ("nu", -1e-6), ("nu", math.nan), ("tol", 0.0), ("tol", math.inf),
                     ("max_iter", -1), ("max_iter", 2.5), ("sync_every", 0), ("sync_every", 1.5)):
        with pytest.raises(ValueError, match=key):
            pressure.check_params(**dict(good, **{key: bad}))
        with pytest.raises(ValueError, match=key):
            PressureField(64, 64, device="cpu", **dict(good, **{key: bad}))
    for H, W in ((0, 8), (8, -1), (8.0, 8)):
        with pytest.raises(ValueError, match="size"):
            PressureField(H, W, device="cpu")
    for ref in ((16, 0), (0, -1), (1,), (1.0, 2), "ab"):
        with pytest.raises(ValueError, match="reference"):
            PressureField(64, 64, cell=4, reference=ref, device="cpu")
    assert pressure.check_size(65, 64, 4) == (17, 16)
    with pytest.raises(NotImplementedError):
        PressureField(64, 64, device="cpu")


# ---- the C entry points refuse before any launch --------------------------------------------------------------------------------------
def refusals(lib, flows, g, valid, ws, p, flag, status, B, h, w):
    """Every argument error of the four entry points with the given addresses (never dereferenced: each call fails its checks before
    any launch); also called by the GPU test with real buffers, whose contents must stay."""
    F = B - 2
    need = lib.pivlfn_pressure_workspace_bytes(F, h, w)
    N = h * w

    def refused(rc, *words):
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1, (rc, msg)
        for word in words:
            assert word in msg, (word, msg)

    def grad(**kw):
        a = dict(flows=flows, B=B, h=h, w=w, s=4.0, nu=0.1, g=g, valid=valid)
        a.update(kw)
        return lib.pivlfn_pressure_gradient(a["flows"], a["B"], a["h"], a["w"], a["s"], a["nu"], a["g"], a["valid"], None)

    for kw, words in ((dict(flows=None), ("null",)), (dict(g=None), ("null",)), (dict(valid=None), ("null",)), (dict(B=2), ("B=2",)),
                      (dict(h=0), ("positive",)), (dict(w=-1), ("positive",)), (dict(B=3, h=46341, w=46341), ("2^31",)),
                      (dict(s=0.0), ("s=0",)), (dict(s=math.nan), ("s=nan",)), (dict(s=math.inf), ("s=inf",)), (dict(s=-1.0), ("s=-1",)),
                      (dict(nu=math.inf), ("nu=inf",)), (dict(nu=math.nan), ("nu=nan",)),
                      (dict(g=flows + B * 2 * N * 4 - 8), ("g overlaps flows",)), (dict(valid=flows), ("valid overlaps flows",)),
                      (dict(valid=g + F * 2 * N * 8 - 1), ("valid overlaps g",))):
        refused(grad(**kw), "pressure_gradient", *words)

    def setup(**kw):
        a = dict(g=g, valid=valid, F=F, h=h, w=w, s=4.0, ws=ws, bytes=need)
        a.update(kw)
        return lib.pivlfn_pressure_setup(a["g"], a["valid"], a["F"], a["h"], a["w"], a["s"], a["ws"], a["bytes"], None)

    for kw, words in ((dict(g=None), ("null",)), (dict(valid=None), ("null",)), (dict(ws=None), ("null",)), (dict(F=0), ("F=0",)),
                      (dict(h=0), ("positive",)), (dict(w=0), ("positive",)), (dict(F=1, h=46341, w=46341), ("2^31",)),
                      (dict(s=0.0), ("s=0",)), (dict(s=math.nan), ("s=nan",)), (dict(bytes=need - 1), ("workspace", str(need))),
                      (dict(ws=ws + 4), ("aligned",)), (dict(ws=g), ("workspace overlaps g",)),
                      (dict(ws=valid - need + 8), ("workspace overlaps valid",))):
        refused(setup(**kw), "pressure_setup", *words)

    def cg(**kw):
        a = dict(ws=ws, bytes=need, F=F, h=h, w=w, tol=1e-8, iters=3)
        a.update(kw)
        return lib.pivlfn_pressure_cg(a["ws"], a["bytes"], a["F"], a["h"], a["w"], a["tol"], a["iters"], None)

    for kw, words in ((dict(ws=None), ("null",)), (dict(F=-1), ("F=-1",)), (dict(h=0), ("positive",)), (dict(F=2, h=32768, w=32768), ("2^31",)),
                      (dict(tol=0.0), ("tol=0",)), (dict(tol=math.nan), ("tol=nan",)), (dict(tol=math.inf), ("tol=inf",)),
                      (dict(tol=-1e-8), ("tol=-1e-08",)), (dict(iters=-1), ("iters=-1",)), (dict(bytes=need - 8), ("workspace", str(need))),
                      (dict(ws=ws + 1), ("aligned",)), (dict(iters=0, ws=None), ("null",))):
        refused(cg(**kw), "pressure_cg", *words)
    assert cg(iters=0) == 0                                                 # nothing to do: no launch

    def read(**kw):
        a = dict(ws=ws, bytes=need, F=F, h=h, w=w, p=p, flag=flag, status=status)
        a.update(kw)
        return lib.pivlfn_pressure_read(a["ws"], a["bytes"], a["F"], a["h"], a["w"], a["p"], a["flag"], a["status"], None)

    for kw, words in ((dict(ws=None), ("null",)), (dict(p=None), ("null",)), (dict(flag=None), ("null",)), (dict(status=None), ("null",)),
                      (dict(F=0), ("F=0",)), (dict(w=0), ("positive",)), (dict(bytes=0), ("workspace", str(need))),
                      (dict(p=ws + need - 8), ("p overlaps the workspace",)), (dict(flag=ws), ("flag overlaps the workspace",)),
                      (dict(status=p + F * N * 8 - 8), ("p overlaps status",)), (dict(flag=status + 31), ("flag overlaps status",)),
                      (dict(flag=p), ("p overlaps flag",))):
        refused(read(**kw), "pressure_read", *words)
    assert lib.pivlfn_pressure_workspace_bytes(0, h, w) == 0 and lib.pivlfn_pressure_workspace_bytes(1, 46341, 46341) == 0
    assert lib.pivlfn_pressure_workspace_offset(F, h, w, 7) == 0 and lib.pivlfn_pressure_workspace_offset(F, 0, w, 0) == 0


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    from pivlfn import _lib
    lib = _lib.load()
    assert lib.pivlfn_abi_version() == 3
    P = 1 << 20                     # non-null, 8-byte aligned, never dereferenced
    refusals(lib, *(P + (i << 32) for i in range(7)), 5, 8, 9)
    # the workspace holds what the contract names, each array inside it and 8-byte aligned
    F, h, w = 3, 8, 9
    need = lib.pivlfn_pressure_workspace_bytes(F, h, w)
    offs = [lib.pivlfn_pressure_workspace_offset(F, h, w, k) for k in range(3)]
    assert need >= (7 * 8 + 1) * F * h * w and all(0 < o < need and o % 8 == 0 for o in offs) and len(set(offs)) == 3
    assert offs[2] + F * h * w <= need and offs[0] + 8 * F * h * w <= offs[1]


# ---- run.py -----------------------------------------------------------------------------------------------------------------------------
def test_run_py_pressure_flags_parse_and_are_checked_before_a_gpu_is_needed(tmp_path):
    import run as runpy
    plain = runpy.parser.parse_args(["-i", "x"])
    assert plain.pressure is None and plain.pressure_rho is None and plain.pressure_image is False
    assert not [ln for ln in runpy.args_lines(plain) if "pressure" in ln]
    assert runpy.parser.parse_args(["--pressure"]).pressure == 4
    full = runpy.parser.parse_args(["--pressure", "2", "--pressure-rho", "1000", "--pressure-nu", "1e-6", "--pressure-dt", "0.001",
                                    "--pressure-calib", "1e-4", "--pressure-tol", "1e-9", "--pressure-image"])
    lines = runpy.args_lines(full)
    assert "pressure: 2\n" in lines and "pressure_rho: 1000.0\n" in lines and "pressure_image: True\n" in lines
    assert runpy.pressure_params(full) == (2, 1e-4, 0.001, 1000.0, 1e-6, 1e-9)
    assert runpy.pressure_params(runpy.parser.parse_args(["--pressure"])) == (4, 1.0, 1.0, 1.0, 0.0, 1e-8)
    assert not [ln for ln in runpy.args_lines(runpy.parser.parse_args(["--spectrum"])) if "pressure" in ln]
    base = ["--model", "piv", "-i", str(tmp_path), "-o", str(tmp_path / "out")]
    for extra, word in ((["--pressure-rho", "2"], "need --pressure"), (["--pressure-image"], "need --pressure"),
                        (["--pressure-tol", "1e-6"], "need --pressure"), (["--pressure", "0"], "cell=0"),
                        (["--pressure", "--pressure-rho", "0"], "rho=0"), (["--pressure", "--pressure-nu", "-1"], "nu=-1"),
                        (["--pressure", "--pressure-dt", "nan"], "dt=nan"), (["--pressure", "--pressure-calib", "0"], "calib=0"),
                        (["--pressure", "--pressure-tol", "0"], "tol=0"), (["--pressure", "-b", "1.5"], "-b/-c"),
                        (["--pressure", "-p"], "--pressure is not available with -p")):
        with pytest.raises(SystemExit) as e:
            runpy.main(base + extra)
        assert word in str(e.value), (extra, str(e.value))


def test_run_py_pressure_is_refused_sharded(tmp_path, monkeypatch):
    import run as runpy
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        runpy.main(["--model", "piv", "-i", str(tmp_path), "-o", str(tmp_path / "out"), "--pressure", "2"])
    assert "--pressure needs a single process" in str(e.value)
