"""CPU: the two-point contract (include/pivlfn.h, pivlfn_twopoint_accumulate) as tests/twopoint_restatement.py states it -- the loop
definition against the vectorised form bit for bit, tree order included --, the refusals of the C entry point, which all come before
any launch and so need no GPU, pivlfn.twopoint.TwoPointResult on accumulators the restatement made from sequences whose
correlation is known in closed form, and the command line of run.py --twopoint.  (TwoPointStats.merge: tests/test_accumulators.py.)"""
import math

import numpy as np
import pytest

import twopoint_restatement as tr

f64 = np.float64


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(3, 5), (4, 7)])
@pytest.mark.parametrize("step", [1, 2])
def test_loops_equal_planes_bit_for_bit(H, W, step):
    """B = 2 from a non-zero acc, with and without mask and mean: the vectorised restatement equals the triple loop, whose tree is
    written out node by node."""
    rng = np.random.default_rng(10 * H + W)
    flow, mask, mean = tr.random_case(rng, 2, H, W)
    acc0 = rng.normal(0, 50, (2, 4, 15, H))
    for m, mu in ((None, None), (mask, None), (mask, mean), (None, mean)):
        a, b = tr.accumulate(flow, m, mu, acc0, 3, step), tr.accumulate_loops(flow, m, mu, acc0, 3, step)
        assert tr.same_bits(a, b)
        n = a[:, :, 0] - acc0[:, :, 0]
        assert np.isfinite(a).all() and n.max() > 0
    assert not tr.same_bits(tr.accumulate(flow, mask, None, acc0, 3, step), tr.accumulate(flow, None, None, acc0, 3, step))


def test_the_tree_is_not_a_running_sum():
    """Seven leaves whose tree root and left-to-right sum differ in fp64, and the padding: ((a+b)+(c+d)) + ((e+f)+(g+0))."""
    leaves = np.array([1e16, 1.0, -1e16, 1.0, 3.0, 1e-3, 7.0])
    want = ((leaves[0] + leaves[1]) + (leaves[2] + leaves[3])) + ((leaves[4] + leaves[5]) + (leaves[6] + 0.0))
    assert tr.tree(leaves) == want
    running = f64(0.0)
    for x in leaves:
        running = running + x
    assert want != running
    assert tr.tree(np.array([-0.0])).tobytes() == f64(-0.0).tobytes()           # a row of one pixel is its own root
    assert tr.tree(np.array([-0.0, -0.0, -0.0])).tobytes() == f64(0.0).tobytes()   # (-0 + -0) + (-0 + +0)


def test_counts_are_exact_and_a_null_mean_leaves_exact_products():
    rng = np.random.default_rng(3)
    flow, mask, _ = tr.random_case(rng, 3, 6, 9)
    acc = tr.accumulate(flow, mask, None, np.zeros((2, 5, 15, 6)), 4, 2)
    k = np.stack([tr.valid(flow[b], mask[b]) for b in range(3)])
    assert np.array_equal(acc[0, 0, 0], k.sum((0, 2))) and np.array_equal(acc[1, 0, 0], k.sum((0, 2)))
    assert np.array_equal(acc[0, 2, 0], (k[:, :, :-4] & k[:, :, 4:]).sum((0, 2)))
    assert np.array_equal(acc[1, 1, 0, :4], (k[:, :-2] & k[:, 2:]).sum((0, 2))) and not acc[1, 1, :, 4:].any()
    assert not acc[1, 3].any() and not acc[1, 4].any()                    # 6 and 8 rows away: no pair; 8 columns away: one per row and frame
    assert np.array_equal(acc[0, 4, 0], (k[:, :, :1] & k[:, :, 8:]).sum((0, 2)))


# ---- the C entry point refuses before any launch --------------------------------------------------------------------------------------
def refusals(lib, flow, mask, mean, acc, B, H, W, R=4):
    """Every error of the contract through the C entry point with the given addresses (never dereferenced: each call fails its checks
    before any launch); also called by the GPU test with real buffers, whose contents must stay."""
    def call(**kw):
        a = dict(flow=flow, mask=mask, mean=mean, acc=acc, B=B, H=H, W=W, max_sep=R, step=1)
        a.update(kw)
        return lib.pivlfn_twopoint_accumulate(a["flow"], a["mask"], a["mean"], a["acc"], a["B"], a["H"], a["W"], a["max_sep"], a["step"], None)

    def refused(rc, *words):
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1, (rc, msg)
        for w in ("twopoint_accumulate",) + words:
            assert w in msg, (w, msg)

    refused(call(flow=None), "null")
    refused(call(acc=None), "null")
    refused(call(B=-1), "B=-1")
    refused(call(H=0), "positive")
    refused(call(W=-3), "positive")
    refused(call(H=46341, W=16384 * 4), "2^31")
    refused(call(H=2, W=16385), "W=16385")
    refused(call(max_sep=-1), "max_sep=-1")
    refused(call(max_sep=256), "max_sep=256")
    refused(call(step=0), "step=0")
    refused(call(step=17), "step=17")
    px, nacc = H * W, 2 * (R + 1) * 15 * H * 8
    refused(call(acc=flow), "acc overlaps flow")
    refused(call(acc=flow + B * px * 8 - 8), "acc overlaps flow")
    refused(call(acc=flow - nacc + 8), "acc overlaps flow")
    refused(call(acc=mask + B * px - 1), "acc overlaps mask")
    refused(call(acc=mean + px * 16 - 8), "acc overlaps mean")
    assert call(B=0, flow=None, acc=None) == 0                            # nothing to add: no pointer is read
    assert call(B=0, H=0) == 1                                            # but the sizes are still checked
    return call


def test_c_entry_point_refuses_bad_arguments_without_a_gpu():
    from pivlfn import _lib
    lib = _lib.load()
    P = 1 << 20                     # non-null, 8-byte aligned, never dereferenced
    flow, mask, mean, acc = (P + (i << 32) for i in range(4))
    call = refusals(lib, flow, mask, mean, acc, 2, 8, 8)
    with pytest.raises(ValueError, match="step=17"):
        _lib.check(call(step=17), "twopoint_accumulate")


def test_python_side_checks_its_parameters():
    from pivlfn import twopoint
    for bad in ((-1, 1), (256, 1), (4, 0), (4, 17), (True, 1), (4.0, 1)):
        with pytest.raises(ValueError):
            twopoint.check_params(*bad)
    twopoint.check_params(0, 16)
    with pytest.raises(ValueError, match="accumulators"):
        twopoint.TwoPointResult(np.zeros((2, 3, 14, 5)))
    res = twopoint.TwoPointResult(np.zeros((2, 3, 15, 5)), 2, 0)
    assert np.isnan(res.correlation("uu", "x").rho).all() and math.isnan(res.integral_scale().scale) and res.integral_scale().truncated
    for call in (lambda: res.correlation("uw"), lambda: res.correlation("uu", "z"), lambda: res.structure(2, "LLL"), lambda: res.spectrum(window="hamming"),
                 lambda: res.taylor_fit(fit=(1, 3)), lambda: res.spectrum()):
        with pytest.raises(ValueError):
            call()


# ---- TwoPointResult on a sequence with a known correlation ----------------------------------------------------------------------------
A, PERIOD, R = 2.0, 18, 24
CASES = [(0.0, False), (3.0, False), (3.0, True)]          # (c, whether the mean is handed over)
_made = {}


def _cosine(c, with_mean):
    """u = c + A*cos(2 pi x/18 + 2 pi b/8), 8 frames of 4 x 72 rounded to fp32, through the restatement; made once per case."""
    from pivlfn.twopoint import TwoPointResult
    if (c, with_mean) not in _made:
        flow = tr.cosine_sequence(c, A, 8, 4, 72, PERIOD)
        mean = np.stack([np.full((4, 72), c), np.zeros((4, 72))]) if with_mean else None
        acc = tr.accumulate(flow, None, mean, np.zeros((2, R + 1, 15, 4)), R, 1)
        _made[(c, with_mean)] = TwoPointResult(acc, 1, 8)
    return _made[(c, with_mean)]


def _bound(c):
    """Rounding u to fp32 moves it by at most 2^-24 (|c| + A); a covariance is a difference of products of two such values, so it
    moves by at most 4 * 2^-24 (|c| + A)^2 to first order, and rho = cov / (A^2/2) with both moving: a cap of 8 * 2^-24 (|c|+A)^2 / (A^2/2)."""
    return 8.0 * 2.0 ** -24 * (abs(c) + A) ** 2 / (A * A / 2.0)


@pytest.mark.parametrize("c,with_mean", CASES)
def test_rho_of_a_cosine_is_the_cosine_in_every_row(c, with_mean):
    res = _cosine(c, with_mean)
    cor = res.correlation("uu", "x")
    want = np.cos(2 * math.pi * np.arange(R + 1) / PERIOD)
    dev = np.abs(cor.rho - want[:, None]).max()
    print(f"c={c} mean={with_mean}: max |rho - cos| = {dev:.3g}, bound {_bound(c):.3g}")
    assert cor.rho.shape == (R + 1, 4) and dev <= _bound(c)
    assert np.array_equal(cor.n, np.repeat(8.0 * (72 - np.arange(R + 1)), 4).reshape(R + 1, 4))
    assert np.abs(cor.var_a - A * A / 2).max() <= _bound(c) * A * A / 2
    assert np.isnan(res.correlation("vv", "x").rho).all()                  # v = 0: no variance, no correlation
    # along y the rows are copies of each other: rho = 1 wherever the partner row exists
    down = res.correlation("uu", "y")
    have = down.n > 0
    assert np.array_equal(have, np.add.outer(np.arange(R + 1), np.arange(4)) < 4) and (down.n[have] == 8 * 72).all()
    assert np.abs(down.rho[have] - 1.0).max() <= _bound(c) and np.isnan(down.rho[~have]).all()
    # the second-order structure function of the cosine: A^2 (1 - cos)
    d2 = res.structure(2, "L", "x", rows=slice(None))
    assert np.abs(d2 - A * A * (1.0 - want)).max() <= 2 * _bound(c) * A * A
    assert np.abs(res.structure(2, "T", "x", rows=slice(None))).max() == 0 and np.abs(res.structure(3, "LLL", "x", rows=slice(None))).max() <= 1e-6


@pytest.mark.parametrize("c,with_mean", CASES)
def test_integral_scale_is_the_trapezoid_rule_to_the_interpolated_crossing(c, with_mean):
    """The zero of cos(2 pi r/18) lies at r = 4.5, between two nodes.  Against the same rule applied to the cosine in float64: the
    trapezoid weights up to the crossing add to less than 4.5 and the triangle's end moves by less than 2 b / |rho_4 - rho_5| = 5.8 b for
    a deviation b of rho, under half its height 0.17: less than 6 b in all."""
    res = _cosine(c, with_mean)
    want, truncated, crossing = tr.trapezoid_to_crossing(np.cos(2 * math.pi * np.arange(R + 1) / PERIOD), 1)
    got = res.integral_scale("uu", "x")
    assert not truncated and not got.truncated and abs(crossing - 4.5) < 1e-12 and abs(got.crossing - 4.5) <= 6 * _bound(c)
    assert abs(got.scale - want) <= 6 * _bound(c)
    assert 2.8 < want < 18 / (2 * math.pi)                                 # the exact integral is 18/(2 pi) = 2.86; the rule lies below
    # never crossing: along y rho stays 1 over the three separations that have pairs
    flat = res.integral_scale("uu", "y")
    assert flat.truncated and flat.crossing is None and abs(flat.scale - 3.0) <= 3 * _bound(c)
    assert math.isnan(res.integral_scale("vv", "x").scale)


def test_pooled_of_one_row_is_that_row_and_of_all_rows_their_weighted_mean():
    from pivlfn.twopoint import TwoPointResult
    rng = np.random.default_rng(8)
    flow, mask, mean = tr.random_case(rng, 4, 9, 40)
    res = TwoPointResult(tr.accumulate(flow, mask, None, np.zeros((2, 7, 15, 9)), 6, 3), 3, 4)
    for which in ("uu", "vv", "uv", "vu"):
        for axis in ("x", "y"):
            rows = res.correlation(which, axis)
            one = res.pooled(which, axis, rows=slice(5, 6))
            for got, want in zip(one, rows):
                assert np.allclose(got, want[:, 5], rtol=1e-14, atol=0, equal_nan=True)
            n, cov, va, vb, rho = tr.pooled(res.acc, which, "xy".index(axis))
            everything = res.pooled(which, axis)
            assert np.array_equal(everything.n, n)
            for got, want in zip(everything[1:], (cov, va, vb, rho)):
                assert np.allclose(got, want, rtol=1e-12, atol=1e-15, equal_nan=True)
            per_row = tr.row_correlation(res.acc, which, "xy".index(axis))
            for got, want in zip(rows, per_row):
                assert np.allclose(got, want, rtol=1e-13, atol=0, equal_nan=True)
    assert tr.summary(res.acc, 3, 4).keys() == res.summary().keys()


def test_spectrum_obeys_parseval_and_finds_the_wavenumber():
    res = _cosine(0.0, False)
    for window in (None, "hann"):
        k, E = res.spectrum("uu", "x", window)
        dk = k[1] - k[0]
        assert len(k) == R + 1 and abs(dk - math.pi / R) < 1e-15 and abs(k[-1] - math.pi) < 1e-12
        total = dk * (E.sum() - 0.5 * (E[0] + E[-1]))
        variance = res.pooled("uu", "x").cov[0]
        assert abs(total - variance) <= 1e-12 * variance, (window, total, variance)
        assert abs(k[np.argmax(E)] - 2 * math.pi / PERIOD) <= dk                # the line of the cosine, to the resolution
    # a 4-sample covariance by hand: M = 3, no window
    from pivlfn.twopoint import TwoPointResult
    acc = np.zeros((2, 4, 15, 1))
    acc[0, :, 0, 0] = 10.0
    acc[0, :, 9, 0] = 10.0 * np.array([4.0, 2.0, 1.0, -1.0])                   # zero means: cov = S_ab / n
    acc[0, :, 5, 0] = acc[0, :, 7, 0] = 40.0
    k, E = TwoPointResult(acc, 2, 1).spectrum("uu", "x", None)
    want = [2 / math.pi * (4 + 2 * (2 * math.cos(math.pi * m / 3) + 1 * math.cos(2 * math.pi * m / 3)) + (-1) ** m * -1.0) for m in range(4)]
    assert np.allclose(E, want, rtol=1e-14) and np.allclose(k, [math.pi * m / 6 for m in range(4)], rtol=1e-15)


def test_taylor_fit_recovers_the_noise_share_within_the_sampling_error():
    """White noise e of known variance on the cosine (8 frames of 32 x 72).  rho(r >= 1) of u = s + e is the signal's correlation times
    var_s / (var_s + var_e) plus the sample correlations of e with itself and with s at that separation.  The fit is linear in rho: its
    intercept is that factor times the intercept kappa of the same fit to the pure cosine (a cosine is not a parabola), plus the fit's
    intercept weights w_r applied to those sample terms.  Their standard error is taken from the sample: per r the standard deviation of the
    products (u_a - m)(u_b - m) over the pairs, over sqrt(pairs), relative to the variance; the bound is four times sum |w_r| se_r --
    the r treated as fully correlated, and 4 rather than 2 since pairs that share a vector are not independent."""
    from pivlfn.twopoint import TwoPointResult
    rng = np.random.default_rng(2024)
    s = tr.cosine_sequence(0.0, A, 8, 32, 72, PERIOD).astype(f64)
    e = rng.normal(0, 0.5, s[:, 0].shape)
    flow = s.copy()
    flow[:, 0] += e
    flow = flow.astype(np.float32)
    res = TwoPointResult(tr.accumulate(flow, None, None, np.zeros((2, 9, 15, 32)), 8, 1), 1, 8)
    fit = res.taylor_fit("uu", "x")
    var_s, var_e = A * A / 2, float(e.var())
    kappa = tr.parabola_fit(np.cos(2 * math.pi * np.arange(9) / PERIOD), 1)[2]
    want_c = kappa * var_s / (var_s + var_e)
    q = np.array([1.0, 4.0, 9.0, 16.0])
    w = 0.25 - (q - q.mean()) * q.mean() / ((q - q.mean()) ** 2).sum()          # the intercept of a least-squares line in q, as weights on rho
    u = flow[:, 0].astype(f64)
    dev = u - u.mean()
    se = np.array([(dev[:, :, :-r] * dev[:, :, r:]).std() / math.sqrt(dev[:, :, r:].size) / u.var() for r in (1, 2, 3, 4)])
    tol = 4.0 * float((np.abs(w) * se).sum())
    print(f"c = {fit.c:.5f}, expected {want_c:.5f}, tolerance {tol:.5f}; noise share {fit.noise:.5f}")
    assert abs(w.sum() - 1.0) < 1e-12 and tol < 0.05
    assert abs(fit.c - want_c) <= tol and fit.noise == 1.0 - fit.c and abs(fit.noise - var_e / (var_s + var_e)) <= tol + (1.0 - kappa)
    # lambda = sqrt(c) * ell is the microscale of the signal alone: that of the noise-free sequence
    clean = _cosine(0.0, False).taylor_fit("uu", "x")
    assert abs(clean.noise - (1.0 - kappa)) <= 4 * _bound(0.0) and abs(fit.microscale / clean.microscale - 1.0) <= 4 * tol
    got = tr.parabola_fit(res.pooled("uu", "x").rho, 1)
    assert np.allclose(got, fit, rtol=1e-10)


def test_run_py_twopoint_flags_parse_and_are_checked_before_a_gpu_is_needed(tmp_path):
    import run as runpy
    plain = runpy.parser.parse_args(["-i", "x"])
    assert plain.twopoint is None and plain.twopoint_step is None and plain.twopoint_mean is None
    assert not [ln for ln in runpy.args_lines(plain) if "twopoint" in ln]
    assert runpy.parser.parse_args(["--twopoint"]).twopoint == 64
    full = runpy.parser.parse_args(["--twopoint", "8", "--twopoint-step", "2", "--twopoint-mean", "stats.npz"])
    lines = runpy.args_lines(full)
    assert "twopoint: 8\n" in lines and "twopoint_step: 2\n" in lines and "twopoint_mean: stats.npz\n" in lines
    assert not [ln for ln in lines if ln.startswith(("color", "quality", "pod", "vortex"))]
    assert not [ln for ln in runpy.args_lines(runpy.parser.parse_args(["--vortex"])) if "twopoint" in ln]
    base = ["--model", "piv", "-i", str(tmp_path), "-o", str(tmp_path / "out")]
    for extra, word in ((["--twopoint-step", "2"], "need --twopoint"), (["--twopoint-mean", "x.npz"], "need --twopoint"),
                        (["--twopoint", "256"], "max_sep=256"), (["--twopoint", "--twopoint-step", "17"], "step=17"),
                        (["--twopoint", "-b", "1.5"], "-b/-c"), (["--twopoint", "--twopoint-mean", str(tmp_path / "none.npz")], "not a file")):
        with pytest.raises(SystemExit) as e:
            runpy.main(base + extra)
        assert word in str(e.value), (extra, str(e.value))


def test_run_py_twopoint_is_refused_sharded(tmp_path, monkeypatch):
    import run as runpy
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        runpy.main(["--model", "piv", "-i", str(tmp_path), "-o", str(tmp_path / "out"), "--twopoint", "8"])
    assert "--twopoint needs a single process" in str(e.value)
