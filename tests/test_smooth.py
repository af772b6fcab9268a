"""CPU: the yardsticks of tests/smooth_restatement.py against scipy and against each other (sparse against dense, the contract-order
iteration against numpy's), three wrong variants of that iteration against the judgements the GPU tests use, the parameter arithmetic and argument checks of pivlfn.smooth, the
host-side refusals of the pivlfn_dct2 / pivlfn_smooth_* entry points, and run.py's flags.  No GPU is touched."""
import numpy as np
import pytest
import torch
from scipy.fft import dctn, idctn

import smooth_restatement as sr
from pivlfn import _lib, smooth

SHAPES = [(1, 1), (1, 9), (5, 7), (63, 65), (64, 64), (65, 130), (129, 31)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_the_table_product_is_scipys_dct(H, W):
    rng = np.random.default_rng(100 * H + W)
    x = rng.standard_normal((3, H, W)) * 10.0 ** rng.uniform(-3.0, 3.0, (3, H, W))
    assert (np.abs(sr.dct2(x) - dctn(x, axes=(1, 2), norm="ortho")) <= sr.dct_bound(x)).all()
    assert (np.abs(sr.dct2(x, inverse=True) - idctn(x, axes=(1, 2), norm="ortho")) <= sr.dct_bound(x, inverse=True)).all()
    c = sr.dct_table(W)
    assert np.abs(c @ c.T - np.eye(W)).max() <= 8 * W * 2.0 ** -52           # orthonormal


def test_the_dct_diagonalises_the_reflecting_laplacian():
    for N in (1, 2, 7, 16):
        c = sr.dct_table(N)
        assert np.abs(c @ sr.laplacian_1d(N) @ c.T + np.diag(sr.eigenvalues(N))).max() <= 64 * 2.0 ** -52
    w = np.ones((5, 6))
    y = np.random.default_rng(0).standard_normal((5, 6))
    via_dct = idctn(sr.gamma(5, 6, 0.7) * dctn(y, norm="ortho"), norm="ortho")
    assert np.abs(via_dct - sr.solve_direct(w, y, 0.7)).max() <= 1e-13
    assert np.abs(sr.lap(sr.lap(y)).ravel() - (sr.operator(w, 1.0) - np.eye(30)) @ y.ravel()).max() <= 1e-13


def test_the_restated_pcg_solves_the_dense_system():
    flow, mask = sr.solve_case(24, 20, 1)
    w = sr.weights_of(flow, None, mask)
    assert (w[mask != 0] == 0).all() and (w[mask == 0] == 1).all()
    y = flow[0].astype(np.float64)
    z, its, rr, bb = sr.pcg(w, y, 1.0, 1e-8)
    assert 0 < its < 40 and rr <= 1e-16 * bb
    r = sr.rhs(w, y).ravel() - sr.operator(w, 1.0) @ z.ravel()
    assert np.linalg.norm(z - sr.solve_direct(w, y, 1.0)) <= 2.0 * np.linalg.norm(r) / sr.lambda_min(w, 1.0)
    z0, its0, _, _ = sr.pcg(np.ones_like(w), y, 1.0, 1e-8)                   # no gaps: the start is the solution
    assert its0 == 0


@pytest.mark.parametrize("H,W,seed", [(24, 20, 1), (33, 17, 2)])
def test_the_sparse_operator_is_the_dense_one(H, W, seed):
    flow, mask = sr.solve_case(H, W, seed)
    w = sr.weights_of(flow, np.random.default_rng(seed).uniform(0.05, 1.0, mask.shape).astype(np.float32), mask)
    y = flow[0].astype(np.float64)
    for s in (0.05, 1.0, 50.0):
        dense = sr.operator(w, s)
        assert np.abs(sr.operator_sparse(w, s).toarray() - dense).max() <= 8 * 2.0 ** -52 * np.abs(dense).max()
        lmin = sr.lambda_min(w, s)
        assert abs(sr.lambda_min_sparse(w, s) - lmin) <= 1e-9 * lmin
        # two backward-stable direct solves: each within a few cond(A) ulp of the solution
        cond = np.linalg.eigvalsh(dense)[-1] / lmin
        assert np.abs(sr.solve_sparse(w, y, s) - sr.solve_direct(w, y, s)).max() <= 64 * cond * 2.0 ** -52 * np.abs(y).max()


def test_the_contract_order_restates_the_same_operator():
    a = np.random.default_rng(3).standard_normal((9, 14))
    assert np.abs(sr.lap_ordered(a) - sr.lap(a)).max() <= 8 * 2.0 ** -52 * np.abs(a).max()
    assert np.abs(sr.gamma_contract(70, 131, 0.05) - sr.gamma(70, 131, 0.05)).max() <= 2.0 ** -40       # 2 - 2 cos cancels near k = 0
    hist = []
    flow, mask = sr.solve_case(24, 20, 1)
    w, y = sr.weights_of(flow, None, mask), flow[0].astype(np.float64)
    z, its, rr, _ = sr.pcg(w, y, 1.0, 1e-8, history=hist)
    assert len(hist) == its + 1 and hist[-1] == rr
    rr_tree, x = sr.pcg_tree(w, y, 1.0, its + 5, tol=1e-8)                  # the contract's stopping rule: the same count
    assert len(rr_tree) == its + 1 and np.abs(x - z).max() <= 1e-12
    assert np.abs(np.array(rr_tree) / np.array(hist) - 1.0).max() <= 1e-9


def test_the_seam_cases_put_gaps_and_known_vectors_on_both_sides():
    for H, W in ((37, 61), (70, 131), (513, 512)):
        gap = sr.seam_case(H, W, 3)[1].reshape(-1) != 0
        assert gap[1019:1030].all() and not gap[1015:1019].any() and not gap[1030:1034].any()          # the seam 1023 | 1024
        assert not gap[2045:2051].any()                                                             # the seam 2047 | 2048 ...
        for k in (2047, 2048):
            assert gap[k - W] and gap[k + W], (H, W, k)                                             # ... and its vertical neighbours
        assert 0.05 < gap.mean() < 0.2


# ---- what the solve's judgements catch: three wrong variants of the restated iteration at 70 x 131 ----------------------------------------
MUTANT_SHAPE = (70, 131, 3)
MUTANT_ITERS = 6


@pytest.fixture(scope="module")
def mutant_case():
    H, W, seed = MUTANT_SHAPE
    flow, mask = sr.seam_case(H, W, seed)
    w, y = sr.weights_of(flow, None, mask), flow[0].astype(np.float64)
    assert H * W > 8 * sr.SEAM and H > 64 and W > 64
    return w, y, {s: sr.trajectory_reference(w, y, s, MUTANT_ITERS) for s in (0.05, 1.0, 50.0)}


def _mutants(w, s):
    """(a) a pr_finish that loses the last workgroup's partial of sigma;  (b) a tile seam: nodes 1023 and 1024, neighbours in a row,
    do not see each other;  (c) an epilogue that forgets m0: the Gamma rows of the second block of 64 are those of the first."""
    import pressure_restatement as pr
    H, W = w.shape
    last = (H * W - 1) // sr.SEAM * sr.SEAM

    def sigma_without_the_last_tile(leaves):
        l = np.array(leaves, np.float64).reshape(-1)
        l[last:] = 0.0
        return pr.tree(l)

    assert (sr.SEAM - 1) // W == sr.SEAM // W                                 # 1023 and 1024 lie in one row

    def lap_with_a_seam(a):
        l, r, u, d = (np.zeros_like(a) for _ in range(4))
        l[:, 1:] = a[:, :-1] - a[:, 1:]
        r[:, :-1] = a[:, 1:] - a[:, :-1]
        u[1:, :] = a[:-1, :] - a[1:, :]
        d[:-1, :] = a[1:, :] - a[:-1, :]
        r.reshape(-1)[sr.SEAM - 1] = 0.0
        l.reshape(-1)[sr.SEAM] = 0.0
        return ((l + r) + u) + d

    g = sr.gamma_contract(H, W, s)
    g[64:] = g[:H - 64]
    return {"a": {"sigma": sigma_without_the_last_tile}, "b": {"lap": lap_with_a_seam}, "c": {"gamma": g}}


@pytest.mark.parametrize("s", [0.05, 1.0, 50.0])
@pytest.mark.parametrize("which", ["a", "b", "c"])
def test_a_wrong_part_leaves_the_trajectory(which, s, mutant_case):
    w, y, refs = mutant_case
    ref = refs[s]
    assert sr.check_trajectory(ref["rr_pcg"], ref, f"numpy's own sums, s={s}") <= 1.0 / sr.ORDERS     # the yardstick passes its own check
    rr, _ = sr.pcg_tree(w, y, s, MUTANT_ITERS, parts=_mutants(w, s)[which])
    rel = np.abs(np.array(rr)[:ref["K"] + 1] / ref["rr_tree"][:ref["K"] + 1] - 1.0).max()
    print(f"mutant ({which}) s={s}: rr leaves the restated trajectory by {rel:.2f} of its value")
    assert rel >= 1e6 * max(sr.ORDERS * ref["Y"], sr.FLOOR)                 # far outside the bound, not a near miss
    with pytest.raises(AssertionError):
        sr.check_trajectory(rr, ref, f"mutant ({which}) s={s}")


def test_the_residual_check_sees_a_wrong_operator_and_not_a_wrong_preconditioner(mutant_case):
    """Run to the stopping rule at tol = 1e-8, s = 0.05.  Mutant (b) solves another system: its true residual fails.  Mutant (c) is still
    a symmetric positive definite preconditioner: it converges to the right answer in under twice numpy's iterations and passes all of
    check_solve, which is why the trajectory check exists."""
    w, y, _ = mutant_case
    s, tol = 0.05, 1e-8
    ref = sr.solve_reference(w, y, s, tol)
    good, x = sr.pcg_tree(w, y, s, 200, tol=tol)
    sr.check_solve(x, len(good) - 1, ref, "the restated iteration")
    assert len(good) - 1 == ref["its"]
    rr, x = sr.pcg_tree(w, y, s, 200, tol=tol, parts=_mutants(w, s)["b"])
    with pytest.raises(AssertionError):
        sr.check_solve(x, len(rr) - 1, ref, "mutant (b)")
    rr, x = sr.pcg_tree(w, y, s, 200, tol=tol, parts=_mutants(w, s)["c"])
    assert ref["its"] < len(rr) - 1 <= 2 * ref["its"]
    sr.check_solve(x, len(rr) - 1, ref, "mutant (c)")                       # passes: residual, error bound and iteration count
    _, x6 = sr.pcg_tree(w, y, s, 6, parts=_mutants(w, s)["c"])
    tref = sr.trajectory_reference(w, y, s, 6)
    with pytest.raises(AssertionError):
        sr.check_iterate(x6, tref, "mutant (c)")


def test_weights_of_applies_the_unknown_rule():
    flow = np.zeros((2, 2, 3), dtype=np.float32)
    flow[0, 0, 0], flow[1, 0, 1], flow[0, 0, 2], flow[1, 1, 0] = np.nan, 1e10, -2e9, 1e9
    wts = np.array([[1, 1, 1], [0.5, -1.0, np.inf]], dtype=np.float32)
    mask = np.zeros((2, 3), dtype=np.uint8)
    assert np.array_equal(sr.weights_of(flow, wts, mask), [[0, 0, 0], [0.5, 0, 0]])
    mask[1, 0] = 4
    assert not sr.weights_of(flow, wts, mask).any()


def test_smooth_param_and_wavelength_invert_each_other():
    for lam in (2.5, 4.0, 8.0, 11.5, 64.0, 1000.0):
        s = smooth.smooth_param(lam)
        assert abs(smooth.smooth_wavelength(s) - lam) <= 1e-9 * lam
    for lam in (4, 8, 16, 25):
        assert abs(sr.response(smooth.smooth_param(lam), lam) - 0.5) <= 1e-12
    assert smooth.smooth_param(8.0) == pytest.approx(1.0 / (2.0 - 2.0 * np.cos(np.pi / 4.0)) ** 2, rel=1e-15)
    for bad in (2.0, 0.0, -3.0, float("nan"), float("inf"), "8", None, True):
        with pytest.raises(ValueError):
            smooth.smooth_param(bad)
    for bad in (0.0, -1.0, float("nan"), 1.0 / 16.0, 0.01, "1"):
        with pytest.raises(ValueError):
            smooth.smooth_wavelength(bad)


def test_check_params():
    assert smooth.check_params() == smooth.smooth_param(8.0)
    assert smooth.check_params(s=2.5) == 2.5 and smooth.check_params(s=2.5, wavelength=None) == 2.5
    assert smooth.check_params(wavelength=12) == smooth.smooth_param(12)
    assert smooth.check_params(None, 8.0, 1e-6, 0, None) == smooth.smooth_param(8.0)
    for kw, word in ((dict(s=1.0, wavelength=12.0), "alternatives"), (dict(s=None, wavelength=None), "one of"),
                     (dict(s=0.0), "s="), (dict(s=-1.0), "s="), (dict(s=float("nan")), "s="), (dict(s=float("inf")), "s="),
                     (dict(s="1"), "s="), (dict(s=True), "s="),
                     (dict(wavelength=2.0), "wavelength="), (dict(wavelength=float("nan")), "wavelength="), (dict(wavelength="8"), "wavelength="),
                     (dict(tol=0.0), "tol="), (dict(tol=-1e-8), "tol="), (dict(tol=float("inf")), "tol="), (dict(tol=None), "tol="),
                     (dict(max_iter=-1), "max_iter="), (dict(max_iter=1.5), "max_iter="), (dict(max_iter=True), "max_iter="),
                     (dict(sync_every=0), "sync_every="), (dict(sync_every=2.0), "sync_every=")):
        with pytest.raises(ValueError) as e:
            smooth.check_params(**kw)
        assert word in str(e.value), (kw, str(e.value))


def test_smooth_flow_refuses_bad_arguments_before_any_launch():
    flow = torch.zeros(1, 2, 4, 5)
    with pytest.raises(NotImplementedError):
        smooth.smooth_flow(flow)                                            # a CPU tensor: there is no CPU path
    with pytest.raises(NotImplementedError):
        smooth.dct2(torch.zeros(4, 5, dtype=torch.float64))
    with pytest.raises(TypeError):
        smooth.smooth_flow(flow.numpy())
    with pytest.raises(TypeError):
        smooth.smooth_flow(flow.double())
    with pytest.raises(TypeError):
        smooth.dct2(torch.zeros(4, 5))
    with pytest.raises(TypeError):
        smooth.dct2(np.zeros((4, 5)))
    with pytest.raises(ValueError):
        smooth.smooth_flow(flow, s=1.0, wavelength=12.0)                    # the parameters are checked before the tensors
    with pytest.raises(ValueError):
        smooth.smooth_flow(flow, tol=0.0)
    with pytest.raises(ValueError):
        smooth.check_size(1, 4097, 8)
    with pytest.raises(ValueError):
        smooth.check_size(40000, 8, 8)
    with pytest.raises(ValueError):
        smooth.check_size(300, 2048, 2048)


def test_weights_from_uncertainty():
    from pivlfn.uncertainty import CENTRE_OUT, FEW, FlowUncertainty
    u = torch.tensor([[[[0.03, 0.4, 0.0, float("nan"), 0.06]], [[0.04, 0.3, 0.0, 0.1, 0.08]]]])       # |u| = 0.05, 0.5, 0, NaN, 0.1
    flag = torch.tensor([[[0, 0, CENTRE_OUT, 0, FEW]]], dtype=torch.uint8)
    w = smooth.weights_from_uncertainty(FlowUncertainty(u, flag), 0.1)
    assert w.dtype == torch.float32 and tuple(w.shape) == (1, 1, 5)
    assert torch.allclose(w, torch.tensor([[[1.0, 0.04, 1.0, 0.0, 0.0]]]), rtol=1e-6, atol=0)
    for bad in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            smooth.weights_from_uncertainty(FlowUncertainty(u, flag), bad)


def test_the_entry_points_refuse_bad_arguments_without_a_gpu():
    """PIVLFN_ERR_ARG and a message that names the problem, on the host before any launch (a launch on a machine without a GPU would
    return PIVLFN_ERR_HIP instead)."""
    lib = _lib.load()
    P = 4096                      # a non-null pointer that is never dereferenced: every case below fails its checks first
    Q = 1 << 40                   # another, far from P

    def refused(rc, *words):
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    big = lib.pivlfn_dct2_workspace_bytes(2, 8, 8)
    assert big == 8 * (64 + 64 + 16 + 2 * 64)
    assert lib.pivlfn_dct2_workspace_bytes(1, 4097, 8) == 0 and lib.pivlfn_dct2_workspace_bytes(0, 8, 8) == 0
    refused(lib.pivlfn_dct2(None, P, 2, 8, 8, 0, Q, big, None), "dct2", "null")
    refused(lib.pivlfn_dct2(P, P + 8192, 2, 8, 8, 0, None, big, None), "dct2", "null")
    refused(lib.pivlfn_dct2(P, P + 8192, 2, 4097, 8, 0, Q, big, None), "dct2", "H=4097", "4096")
    refused(lib.pivlfn_dct2(P, P + 8192, 2, 8, 4097, 1, Q, big, None), "W=4097")
    refused(lib.pivlfn_dct2(P, P + 8192, 2, 0, 8, 0, Q, big, None), "positive")
    refused(lib.pivlfn_dct2(P, P + 8192, 70000, 8, 8, 0, Q, big, None), "P=70000")
    refused(lib.pivlfn_dct2(P, P + 8192, 2, 8, 8, 0, Q, big - 8, None), "workspace", "too small")
    refused(lib.pivlfn_dct2(P, P + 8192, 2, 8, 8, 0, Q + 4, big, None), "workspace", "aligned")
    refused(lib.pivlfn_dct2(P, P + 512, 2, 8, 8, 0, Q, big, None), "out overlaps x")
    refused(lib.pivlfn_dct2(P, P + 8192, 2, 8, 8, 0, P + 64, big, None), "the workspace overlaps x")

    need = lib.pivlfn_smooth_workspace_bytes(2, 16, 12)
    assert need > 8 * (2 * 8 * 2 * 16 * 12) and lib.pivlfn_smooth_workspace_bytes(1, 16, 4097) == 0
    refused(lib.pivlfn_smooth_setup(None, None, None, 2, 16, 12, 1.0, Q, need, None), "smooth_setup", "null")
    refused(lib.pivlfn_smooth_setup(P, None, None, 2, 16, 12, 1.0, None, need, None), "smooth_setup", "null")
    refused(lib.pivlfn_smooth_setup(P, None, None, 2, 4097, 12, 1.0, Q, need, None), "H=4097")
    refused(lib.pivlfn_smooth_setup(P, None, None, 0, 16, 12, 1.0, Q, need, None), "F=0")
    refused(lib.pivlfn_smooth_setup(P, None, None, 2, 16, 12, 0.0, Q, need, None), "s=0", "positive")
    refused(lib.pivlfn_smooth_setup(P, None, None, 2, 16, 12, float("nan"), Q, need, None), "s=nan")
    refused(lib.pivlfn_smooth_setup(P, None, None, 2, 16, 12, 1.0, Q, need - 8, None), "workspace", "too small")
    refused(lib.pivlfn_smooth_setup(P, None, None, 2, 16, 12, 1.0, Q + 1, need, None), "aligned")
    refused(lib.pivlfn_smooth_setup(P, None, None, 2, 16, 12, 1.0, P + 8, need, None), "the workspace overlaps flows")
    refused(lib.pivlfn_smooth_setup(P, None, Q + 64, 2, 16, 12, 1.0, Q, need, None), "the workspace overlaps mask")
    refused(lib.pivlfn_smooth_pcg(None, need, 2, 16, 12, 1.0, 1e-8, 1, None), "smooth_pcg", "null")
    refused(lib.pivlfn_smooth_pcg(Q, need, 2, 16, 12, 0.0, 1e-8, 1, None), "s=0")
    refused(lib.pivlfn_smooth_pcg(Q, need, 2, 16, 12, float("nan"), 1e-8, 1, None), "s=nan")
    refused(lib.pivlfn_smooth_pcg(Q, need, 2, 16, 12, 1.0, 0.0, 1, None), "tol=0")
    refused(lib.pivlfn_smooth_pcg(Q, need, 2, 16, 12, 1.0, 1e-8, -1, None), "iters=-1")
    refused(lib.pivlfn_smooth_pcg(Q, 64, 2, 16, 12, 1.0, 1e-8, 1, None), "workspace", "too small")
    assert lib.pivlfn_smooth_pcg(Q, need, 2, 16, 12, 1.0, 1e-8, 0, None) == 0          # nothing to enqueue
    refused(lib.pivlfn_smooth_read(Q, need, 2, 16, 12, None, None, None, P, None), "smooth_read", "null")
    refused(lib.pivlfn_smooth_read(Q, need, 2, 16, 4097, P, None, None, P + (1 << 20), None), "W=4097")
    refused(lib.pivlfn_smooth_read(Q, need - 8, 2, 16, 12, P, None, None, P + (1 << 20), None), "too small")
    refused(lib.pivlfn_smooth_read(Q, need, 2, 16, 12, P, None, None, P + 64, None), "z overlaps status")
    refused(lib.pivlfn_smooth_read(Q, need, 2, 16, 12, Q + 64, None, None, P, None), "z overlaps the workspace")
    with pytest.raises(ValueError):
        _lib.check(lib.pivlfn_smooth_pcg(Q, need, 2, 16, 12, 1.0, 1e-8, -1, None), "smooth_pcg")


def test_run_py_parses_the_smooth_flags():
    import run as runpy
    plain = runpy.parser.parse_args(["-i", "x", "-o", "y"])
    assert (plain.smooth, plain.smooth_tol) == (None, None)
    assert not [ln for ln in runpy.args_lines(plain) if ln.startswith("smooth")]
    assert set(runpy.SMOOTH_FLAGS) <= set(runpy.VIZ_FLAGS)
    bare = runpy.parser.parse_args(["-i", "x", "--smooth"])
    assert (bare.smooth, bare.smooth_tol) == (8.0, None)
    full = runpy.parser.parse_args(["-i", "x", "--validate", "mask", "--smooth", "12.5", "--smooth-tol", "1e-6"])
    assert (full.smooth, full.smooth_tol) == (12.5, 1e-6)
    assert [ln for ln in runpy.args_lines(full) if ln.startswith("smooth")] == ["smooth: 12.5\n", "smooth_tol: 1e-06\n"]
    for argv, word in ((["-i", "x", "--smooth-tol", "1e-6"], "--smooth-tol needs --smooth"),
                       (["-i", "x", "--smooth", "2"], "wavelength"), (["-i", "x", "--smooth", "--smooth-tol", "0"], "tol"),
                       (["-i", "x", "--smooth", "-b", "1.0"], "-b/-c")):
        with pytest.raises(SystemExit) as e:
            runpy.main(argv)
        assert word in str(e.value), (argv, str(e.value))
    stages = runpy.make_stages(full, runpy.OutputLayout.of("out", "net", "x", 0, -1), "x", None, torch.device("cpu"), 0, 1)
    assert [type(s).__name__ for s in stages] == ["Validate", "Smooth"]
