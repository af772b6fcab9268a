"""CPU: the numpy restatement of pivlfn_flow_uncertainty's contract (tests/uncertainty_restatement.py) against hand-computed values, a
scalar loop over the clipped windows and the property it is meant to have on noisy particle images (the predicted uncertainty is the
scatter of the peak); the argument errors of pivlfn.uncertainty and of the C entry points, UncertaintyStats.finalize and the coverage
on planted numbers, run.py's flags -- none of which needs a GPU."""
import math

import numpy as np
import pytest
import torch

import quality_restatement as qr
import uncertainty_restatement as ur
from uncertainty_restatement import CENTRE_OUT, FEW, FLAT, NO_PEAK, NO_VARIANCE, UNUSABLE

ALL_BITS = FEW | FLAT | NO_PEAK | NO_VARIANCE | CENTRE_OUT


# ---- hand-computed values --------------------------------------------------------------------------------------------------------
def test_restatement_on_a_3x3_image_by_hand():
    """img1 = 18 at the centre of a 3 x 3 image of zeros, img2 the same plus 9 right of the centre; zero flow, r = 1, lag = 0,
    min_count 2.  The high-pass windows hold 4 (corners), 6 (edges) and 9 (centre) pixels:
      a' = [[-4.5, -3, -4.5], [-3, 16, -3], [-4.5, -3, -4.5]],  b' = [[-4.5, -4.5, -6.75], [-3, 15, 4.5], [-4.5, -4.5, -6.75]].
    The centre's window is the whole image: n0 = 9, C0 = 2 (20.25 + 13.5 + 30.375) + (9 + 240 - 13.5) = 363.75.
    x pairs (q, its right neighbour), six of them: rows 0 and 2: (t1, t2) = (20.25, 13.5) and (20.25, 20.25); row 1: (-45, -48) and
    (72, -45):  S_x = 2 (33.75 + 40.5) + (-93 + 27) = 82.5;  d = 6.75, 0, 3, 117 and with lag 0 g = d^2:
    V_x = 2 (45.5625) + 9 + 13689 = 13789.125.  y pairs: column 0: (13.5, 13.5) twice; column 1: (-45, -72) and (-72, -45); column 2:
    (-20.25, 20.25) and (20.25, -20.25):  S_y = 54 - 234 + 0 = -180,  V_y = 2 (27^2) + 2 (40.5^2) = 4738.5.
    Cm = S/2 - sqrt(V)/2 is negative on both axes: NO_PEAK, u is NaN.  With img2 = img1 every d is +-0 and V = 0: NO_VARIANCE; C0 = 4
    (20.25) + 4 (9) + 256 = 373 and S_x = S_y = 4 (27) - 2 (96) = -84: NO_PEAK as well."""
    img1 = np.zeros((1, 3, 3), np.float32)
    img1[0, 1, 1] = 18.0
    img2 = img1.copy()
    img2[0, 1, 2] = 9.0
    flow = np.zeros((2, 3, 3), np.float32)
    u, flag, parts = ur.pair_uncertainty(img1, img2, flow, 1, lag=0, min_count=2)
    assert parts["n0"][1, 1] == 9 and parts["C0"][1, 1] == 363.75
    assert parts["n"][0][1, 1] == 6 and parts["S"][0][1, 1] == 82.5 and parts["V"][0][1, 1] == 13789.125
    assert parts["n"][1][1, 1] == 6 and parts["S"][1][1, 1] == -180.0 and parts["V"][1][1, 1] == 4738.5
    assert flag[1, 1] == NO_PEAK and np.isnan(u[:, 1, 1]).all()
    # a corner's window: 4 pixels, each a pair with its right and its lower neighbour (a partner may lie outside the window); the
    # default min_count of 5 makes it FEW, the centre is not
    assert parts["n0"][0, 0] == 4 and parts["n"][0][0, 0] == 4 and parts["n"][1][0, 0] == 4
    assert parts["n0"][2, 2] == 4 and parts["n"][0][2, 2] == 2 and parts["n"][1][2, 2] == 2      # the last column / row has no partner
    _, flag5, _ = ur.pair_uncertainty(img1, img2, flow, 1, lag=0)
    assert flag5[0, 0] == FEW and flag5[1, 1] == NO_PEAK
    # the same image twice: a' = b', so t1 = t2, every d is zero and so is V
    u, flag, parts = ur.pair_uncertainty(img1, img1, flow, 1, lag=0, min_count=2)
    assert parts["V"][0][1, 1] == 0.0 and parts["V"][1][1, 1] == 0.0 and flag[1, 1] == NO_PEAK | NO_VARIANCE and np.isnan(u[:, 1, 1]).all()
    assert parts["C0"][1, 1] == 373.0 and parts["S"][0][1, 1] == parts["S"][1][1, 1] == -84.0


def test_value_of_u_from_the_sums_by_hand():
    """C0 = 100, S = 160, V = 400: sig = 20, Cm = 70, Cp = 90, u = |0.5 (ln 70 - ln 90) / (ln 70 - 2 ln 100 + ln 90)|
    = 0.5 * 0.2513144 / 0.4620355 = 0.27196...; planted through a 1 x 1 window sum by calling the per-axis arithmetic directly."""
    lm, lp, l0 = math.log(70.0), math.log(90.0), math.log(100.0)
    want = abs(0.5 * (lm - lp) / ((lm - 2.0 * l0) + lp))
    assert abs(want - 0.27196) < 1e-5
    # a pair whose sums are known: restated arithmetic on the restatement's own parts, every usable pixel
    a, c = ur.noisy_particle_pair(24, 24, (0.3, -0.2), 0.05, 3)
    flow = np.stack([np.full((24, 24), 0.3, np.float32), np.full((24, 24), -0.2, np.float32)])
    u, flag, parts = ur.pair_uncertainty(a, c, flow, 4, lag=1)
    ys, xs = np.nonzero((flag & UNUSABLE) == 0)
    assert len(ys) > 50
    for y, x in zip(ys, xs):
        for e in (0, 1):
            C0, S, V = (float(parts[k][y, x]) if k == "C0" else float(parts[k][e][y, x]) for k in ("C0", "S", "V"))
            sig = math.sqrt(V)
            lm, lp, l0 = math.log(0.5 * S - 0.5 * sig), math.log(0.5 * S + 0.5 * sig), math.log(C0)
            assert np.float32(abs(0.5 * (lm - lp) / ((lm - 2.0 * l0) + lp))) == u[e, y, x], (y, x, e)


def _scalar_pair(a, b, v, r, lag, min_count, floor):
    """The contract with plain Python floats and loops over windows clipped to the image -> (u [2,H,W] float32, flag [H,W])."""
    H, W = a.shape

    def box(term, cy, cx, R):
        tot = 0.0
        for yy in range(max(cy - R, 0), min(cy + R, H - 1) + 1):
            row = 0.0
            for xx in range(max(cx - R, 0), min(cx + R, W - 1) + 1):
                row = row + term(yy, xx)
            tot = tot + row
        return tot
    ah, bh = np.zeros((H, W)), np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            if v[y, x]:
                n1 = box(lambda yy, xx: 1.0 if v[yy, xx] else 0.0, y, x, r)
                ah[y, x] = float(a[y, x]) - box(lambda yy, xx: float(a[yy, xx]) if v[yy, xx] else 0.0, y, x, r) / n1
                bh[y, x] = float(b[y, x]) - box(lambda yy, xx: float(b[yy, xx]) if v[yy, xx] else 0.0, y, x, r) / n1
    pair, s, d = np.zeros((2, H, W), bool), np.zeros((2, H, W)), np.zeros((2, H, W))
    for e, (ex, ey) in enumerate(ur.AXES):
        for y in range(H - ey):
            for x in range(W - ex):
                if v[y, x] and v[y + ey, x + ex]:
                    t1, t2 = float(ah[y, x]) * float(bh[y + ey, x + ex]), float(ah[y + ey, x + ex]) * float(bh[y, x])
                    pair[e, y, x], s[e, y, x], d[e, y, x] = True, t1 + t2, t1 - t2
    g = np.zeros((2, H, W))
    for e in range(2):
        for y in range(H):
            for x in range(W):
                if pair[e, y, x]:
                    g[e, y, x] = float(d[e, y, x]) * box(lambda yy, xx: float(d[e, yy, xx]), y, x, lag)
    u, flag = np.full((2, H, W), np.nan, np.float32), np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            n0 = box(lambda yy, xx: 1.0 if v[yy, xx] else 0.0, y, x, r)
            C0 = box(lambda yy, xx: float(ah[yy, xx]) * float(bh[yy, xx]) if v[yy, xx] else 0.0, y, x, r)
            ne = [box(lambda yy, xx: 1.0 if pair[e, yy, xx] else 0.0, y, x, r) for e in range(2)]
            f = 0
            if n0 < min_count or ne[0] < min_count or ne[1] < min_count:
                f = FEW
            elif C0 < floor * floor * n0:
                f = FLAT
            else:
                ends = []
                for e in range(2):
                    S, V = box(lambda yy, xx: float(s[e, yy, xx]), y, x, r), box(lambda yy, xx: float(g[e, yy, xx]), y, x, r)
                    sig = math.sqrt(V) if V >= 0.0 else math.nan
                    Cm, Cp = 0.5 * S - 0.5 * sig, 0.5 * S + 0.5 * sig
                    if Cm <= 0.0 or C0 - Cp < 1e-6 * C0:
                        f |= NO_PEAK
                    if V <= 0.0 or not math.isfinite(V):
                        f |= NO_VARIANCE
                    ends.append((Cm, Cp))
                if f == 0:
                    l0 = math.log(C0)
                    for e, (Cm, Cp) in enumerate(ends):
                        lm, lp = math.log(Cm), math.log(Cp)
                        u[e, y, x] = abs(0.5 * (lm - lp) / ((lm - 2.0 * l0) + lp))
            flag[y, x] = f | (0 if v[y, x] else CENTRE_OUT)
    return u, flag


def _flagged_case(H, W, C, r, seed):
    """A noisy particle pair with its true uniform shift as the flow; one all-constant patch that holds whole windows of high-passed
    zeros, a column that warps outside, a NaN, a masked block and speckles."""
    a, c = ur.noisy_particle_pair(H, W, (0.3, -0.2), 0.05, seed)
    a, c = a[None], c[None]
    if C == 3:
        a, c = (np.concatenate([x, np.float32(0.75) * x + np.float32(0.1), x * x], axis=1) for x in (a, c))
    qr.flatten_patch(a, c, 1, 1, size=4 * r + 1)
    f = np.stack([np.full((H, W), 0.3, np.float32), np.full((H, W), -0.2, np.float32)])
    f[0, :, W - 1] = 30.0
    f[1, 3, 5] = np.nan
    return a[0], c[0], f, qr.speckle_mask(1, H, W, 3, 2 * r + 2)[0]


@pytest.mark.parametrize("C,lag", [(1, 0), (3, 2)])
def test_restatement_equals_a_scalar_loop_over_the_clipped_windows(C, lag):
    """Zero padding against clipped windows, vectorised against scalar: every pixel of a 16 x 20 image with a mask, invalid samples
    and a flat patch, r = 2, bit for bit.  Every flag bit is reached -- but NO_VARIANCE with lag 0, where V is a sum of squares."""
    H, W, r = 16, 20, 2
    a, c, f, mask = _flagged_case(H, W, C, r, 5)
    u, flag, _ = ur.pair_uncertainty(a, c, f, r, lag, mask)
    b, m = qr.warp(qr.gray(c), f)
    su, sflag = _scalar_pair(qr.gray(a), b, m & (mask == 0), r, lag, 13, 1.0 / 255.0)
    assert np.array_equal(flag, sflag)
    assert np.array_equal(u, su, equal_nan=True) and not np.signbit(u).any()          # |.| leaves no -0.0: equal values are equal bits
    assert np.array_equal(np.isnan(u[0]), (flag & UNUSABLE) != 0) and np.array_equal(np.isnan(u[0]), np.isnan(u[1]))
    seen = int(np.bitwise_or.reduce(flag, axis=None))
    assert seen == (ALL_BITS if lag else ALL_BITS & ~NO_VARIANCE), np.bincount(flag.ravel(), minlength=32)
    assert np.count_nonzero(flag == 0) >= 10


# ---- what the measure shows --------------------------------------------------------------------------------------------------------
SHIFT, SIZE, RADIUS = (0.3, -0.2), 160, 8
CENTRES = np.arange(26, SIZE - 26, 17)                   # windows of 17 x 17 every 17 px, 26 px from the borders: independent
BAND = (0.75 * 1.067, 1.25 * 1.142)


@pytest.fixture(scope="module")
def pooled():
    """sigma -> (u [2,n] of the usable sampled windows of three seeds, their peak residuals [2,n], windows sampled, windows flagged)."""
    flow = np.stack([np.full((SIZE, SIZE), SHIFT[0], np.float32), np.full((SIZE, SIZE), SHIFT[1], np.float32)])
    out = {}
    for sigma in (0.02, 0.05, 0.1):
        us, ds, sampled = [], [], 0
        for seed in (1, 2, 3):
            a, c = ur.noisy_particle_pair(SIZE, SIZE, SHIFT, sigma, seed)
            u, flag, _ = ur.pair_uncertainty(a, c, flow, RADIUS, lag=2)
            d = ur.pair_peak_residual(a, c, flow, RADIUS)
            at = np.ix_(CENTRES, CENTRES)
            ok = ((flag[at] & UNUSABLE) == 0).ravel()
            sampled += ok.size
            us.append(np.stack([u[0][at].ravel(), u[1][at].ravel()])[:, ok].astype(np.float64))
            ds.append(np.stack([d[0][at].ravel(), d[1][at].ravel()])[:, ok])
        us, ds = np.concatenate(us, axis=1), np.concatenate(ds, axis=1)
        out[sigma] = (us, ds, sampled, sampled - us.shape[1])
    return out


def test_predicted_uncertainty_is_the_scatter_of_the_peak(pooled):
    """Particle images at 0.05 ppp, 2.5 px diameter, peaks of 0.2..0.4 on an offset of 0.2, 160 x 160, a uniform shift of (0.3, -0.2)
    px, Gaussian noise; the flow is the true shift, r = 8, lag 2; 49 independent windows a pair, seeds 1, 2, 3.  The pooled RMS of u
    over the usable windows divided by the standard deviation of the peak's actual position (pair_peak_residual) over the same
    windows, measured with this restatement:
        sigma 0.05: x 1.067, y 1.088 (3 of 147 windows flagged);  sigma 0.1: x 1.101, y 1.142 (1 of 147);
        sigma 0.02: x 1.115, y 1.155 (20 of 147, all NO_VARIANCE) -- not part of the band.
    The band is the measured range 1.067 .. 1.142 widened by 25 % either side for the seed-to-seed scatter: 0.800 .. 1.4275.  (With
    lag 0 the same images give 1.09 .. 1.13 at these two noise levels and 1.30 .. 1.51 at sigma 0.02.)  u follows the noise: the RMS
    of u at sigma 0.1 is 5.6 times that at 0.02, asked to be at least 2.  Flagged windows are skipped; they are at most 15 % of the
    sampled ones at each noise level (the share grows as the noise falls: the variance estimate, a sum of covariances, comes out
    negative more often when the particle images themselves dominate the contributions; it also grows with the particles' peak
    intensity, which the issue leaves open and the test fixes at 0.2..0.4, 50 to 100 grey levels of an 8-bit frame.  The margin to
    the 15 % is small and depends on that choice.  Flagged of 147 at sigma 0.02 / 0.05 / 0.1, same seeds and windows: peaks of
    0.2..0.4: 20 / 3 / 1;  0.3..0.8: 25 / 16 / 3, so 17 % and 11 %: the bound fails at sigma 0.02;  0.1..0.2: 6 / 1 / 86: at sigma 0.1 the
    noise equals the particles and most windows have no peak)."""
    rms = {}
    for sigma, (us, ds, sampled, flagged) in pooled.items():
        rms[sigma] = np.sqrt((us ** 2).mean(axis=1))
        ratio = rms[sigma] / ds.std(axis=1)
        print(f"sigma {sigma}: rms u {rms[sigma]}, std of the peak residual {ds.std(axis=1)}, ratio {ratio}, flagged {flagged}/{sampled}")
        assert sampled == 147 and flagged <= 0.15 * sampled, (sigma, flagged, sampled)
        if sigma in (0.05, 0.1):
            assert np.all((BAND[0] <= ratio) & (ratio <= BAND[1])), (sigma, ratio)
    assert np.all(rms[0.1] >= 2.0 * rms[0.02]), (rms[0.1], rms[0.02])


# ---- host logic --------------------------------------------------------------------------------------------------------------------
def test_flow_uncertainty_argument_errors():
    import pivlfn
    from pivlfn import FlowUncertainty, flow_uncertainty
    from pivlfn import uncertainty as U
    assert (U.FEW, U.FLAT, U.NO_PEAK, U.NO_VARIANCE, U.CENTRE_OUT, U.UNUSABLE) == (FEW, FLAT, NO_PEAK, NO_VARIANCE, CENTRE_OUT, 15)
    for name in ("flow_uncertainty", "FlowUncertainty", "UncertaintyStats", "uncertainty_coverage"):
        assert getattr(pivlfn, name) is getattr(U, name) and name in pivlfn.__all__
    assert U.check_params(8, 2, 1 / 255, None) == 145 and U.check_params(1, 0, 0.0, 9) == 9 and U.check_params(15, 4, 1.0, 2) == 2
    img, flow = torch.zeros(2, 1, 8, 8), torch.zeros(2, 2, 8, 8)
    for bad in (0, 16, 2.0, True, None):
        with pytest.raises(ValueError, match="radius"):
            flow_uncertainty(img, img, flow, radius=bad)
    for bad in (-1, 5, 1.0, False, None):
        with pytest.raises(ValueError, match="lag"):
            flow_uncertainty(img, img, flow, lag=bad)
    for bad in (1, 26, 3.0, False):
        with pytest.raises(ValueError, match="min_count"):
            flow_uncertainty(img, img, flow, radius=2, min_count=bad)
    for bad in (-1e-3, math.nan, math.inf):
        with pytest.raises(ValueError, match="floor"):
            flow_uncertainty(img, img, flow, floor=bad)
    with pytest.raises(TypeError, match="img1"):
        flow_uncertainty(img.double(), img, flow)
    with pytest.raises(ValueError, match="C = 1 or 3"):
        flow_uncertainty(torch.zeros(2, 2, 8, 8), torch.zeros(2, 2, 8, 8), flow)
    with pytest.raises(ValueError, match="do not belong"):
        flow_uncertainty(img, img, torch.zeros(2, 2, 8, 9))
    with pytest.raises(TypeError, match="float32"):
        flow_uncertainty(img, img, flow.double())
    with pytest.raises(NotImplementedError, match="GPU"):            # there is no CPU path
        flow_uncertainty(img, img, flow)
    with pytest.raises(NotImplementedError, match="GPU"):
        U.UncertaintyStats(4, 4, device="cpu")
    with pytest.raises(ValueError, match="bad size"):
        U.UncertaintyStats(0, 4, device="cpu")
    empty = FlowUncertainty(torch.zeros(0, 2, 4, 4), torch.zeros(0, 4, 4, dtype=torch.uint8))
    assert empty.summary() == [] and U.uncertainty_coverage(torch.zeros(0, 2, 4, 4), torch.zeros(0, 2, 4, 4), empty) == []


def test_summary_magnitude_finalize_and_coverage_on_planted_numbers():
    from pivlfn import FlowUncertainty, UncertaintyStats, uncertainty_coverage
    nan = math.nan
    u = torch.tensor([[[[0.3, nan], [0.1, 0.5]], [[0.4, nan], [0.2, 0.5]]]])
    flag = torch.tensor([[[0, FEW | CENTRE_OUT], [CENTRE_OUT, 0]]], dtype=torch.uint8)
    unc = FlowUncertainty(u, flag)
    assert abs(float(unc.magnitude()[0, 0, 0]) - 0.5) < 1e-7 and math.isnan(float(unc.magnitude()[0, 0, 1]))
    (s,) = unc.summary()
    assert s["few"] == 0.25 and s["flat"] == s["no_peak"] == s["no_variance"] == 0.0 and s["centre_out"] == 0.5 and s["n"] == 3
    assert abs(s["mean_ux"] - 0.3) < 1e-7 and abs(s["rms_uy"] - math.sqrt((0.16 + 0.04 + 0.25) / 3)) < 1e-7
    # three usable vectors; the truth at (1, 0) is the unknown-vector value, so two are compared: errors (0.2, 0.5) at (0, 0) and
    # (0.6, 0.4) at (1, 1)
    truth = torch.zeros(1, 2, 2, 2)
    flow = torch.tensor([[[[0.2, 7.0], [0.1, 0.6]], [[-0.5, 7.0], [0.1, -0.4]]]])
    truth[0, :, 1, 0] = 1e10
    (c,) = uncertainty_coverage(flow, truth, unc)
    assert c["n_x"] == c["n_y"] == 2
    assert c["coverage_x"] == 0.5 and c["coverage_y"] == 0.5            # x: 0.2 <= 0.3, 0.6 > 0.5;  y: 0.5 > 0.4, 0.4 <= 0.5
    assert abs(c["error_over_u_x"] - math.sqrt((0.04 + 0.36) / (0.09 + 0.25))) < 1e-6
    assert abs(c["error_over_u_y"] - math.sqrt((0.25 + 0.16) / (0.16 + 0.25))) < 1e-6
    (c,) = uncertainty_coverage(flow, truth, unc, mask=torch.tensor([[[0, 0], [0, 1]]], dtype=torch.uint8))
    assert c["n_x"] == 1 and c["coverage_x"] == 1.0 and c["coverage_y"] == 0.0
    (c,) = uncertainty_coverage(flow, truth, unc, mask=torch.ones(1, 2, 2, dtype=torch.uint8))
    assert c["n_x"] == 0 and math.isnan(c["coverage_x"]) and math.isnan(c["error_over_u_y"])
    # sums of two pairs at pixel (0,0): u = 0.3, 0.5 -> sum u^2 = 0.34; one pair at (0,1); none at (1,0)
    acc = np.zeros((3, 2, 2))
    acc[:, 0, 0] = (0.34, 0.02, 2)
    acc[:, 0, 1] = (0.25, 0.0, 1)
    res = UncertaintyStats.finalize(acc, 2)
    assert res["count"] == 2 and res["n"].tolist() == [[2, 1], [0, 0]]
    assert abs(res["noise_var_u"][0, 0] - 0.17) < 1e-15 and abs(res["mean_unc_u"][0, 0] - math.sqrt(0.34) / 2) < 1e-15
    assert res["noise_var_v"][0, 0] == 0.01 and res["mean_unc_u"][0, 1] == 0.5 and res["noise_var_v"][0, 1] == 0.0
    assert np.isnan(res["noise_var_u"][1]).all() and np.isnan(res["mean_unc_v"][1]).all()
    with pytest.raises(ValueError, match=r"\[3,H,W\]"):
        UncertaintyStats.finalize(np.zeros((2, 2, 2)), 1)
    # the restatement's accumulate skips the unusable pixels
    sums = ur.accumulate(np.zeros((3, 2, 2)), u.numpy(), flag.numpy())
    assert sums[2].tolist() == [[1, 0], [1, 1]] and sums[0, 0, 1] == 0.0
    assert sums[0, 0, 0] == float(np.float32(0.3)) ** 2 and sums[1, 1, 1] == 0.25


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    """Every refusal of pivlfn_flow_uncertainty and pivlfn_uncertainty_accumulate comes from the host, before any launch, as
    PIVLFN_ERR_ARG with a message naming the problem."""
    from pivlfn import _lib
    lib = _lib.load()
    P = 1 << 20                     # non-null, 8-byte aligned, never dereferenced: every case below fails its checks first
    img1, img2, flow, mask, unc, flag, ws = (P + (i << 32) for i in range(7))
    B, H, W, r, lag = 2, 8, 8, 2, 2
    need = lib.pivlfn_flow_uncertainty_workspace_bytes(B, H, W, r, lag)
    assert need >= B * H * W * 74 and need % 256 == 0
    for bad in ((0, H, W, r, lag), (B, H, W, 16, lag), (B, H, W, 0, lag), (B, H, W, r, 5), (B, H, W, r, -1)):
        assert lib.pivlfn_flow_uncertainty_workspace_bytes(*bad) == 0

    def call(**kw):
        a = dict(img1=img1, img2=img2, C=1, flow=flow, mask=mask, unc=unc, flag=flag, B=B, H=H, W=W, radius=r, lag=lag, min_count=13,
                 floor=1 / 255, ws=ws, ws_bytes=need)
        a.update(kw)
        return lib.pivlfn_flow_uncertainty(a["img1"], a["img2"], a["C"], a["flow"], a["mask"], a["unc"], a["flag"], a["B"], a["H"],
                                           a["W"], a["radius"], a["lag"], a["min_count"], a["floor"], a["ws"], a["ws_bytes"], None)

    def refused(rc, what, *words):
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1, (rc, msg)
        for w in (what,) + words:
            assert w in msg, (w, msg)

    for name in ("img1", "img2", "flow", "unc", "flag", "ws"):
        refused(call(**{name: None}), "flow_uncertainty", "null")
    px = B * H * W
    for kw, word in ((dict(C=2), "C=2"), (dict(B=0), "positive"), (dict(H=-1), "positive"), (dict(H=46341, W=46341), "2^31"),
                     (dict(B=65536), "B=65536"), (dict(radius=0), "radius=0"), (dict(radius=16), "radius=16"), (dict(lag=-1), "lag=-1"),
                     (dict(lag=5), "lag=5"), (dict(min_count=1), "min_count=1"), (dict(min_count=26), "min_count=26"),
                     (dict(floor=-0.5), "floor"), (dict(floor=math.nan), "floor"), (dict(ws=ws + 4), "8-byte aligned"),
                     (dict(ws_bytes=need - 1), "too small"), (dict(unc=img1), "unc overlaps img1"),
                     (dict(unc=flow - px * 8 + 4), "unc overlaps flow"), (dict(unc=mask), "unc overlaps mask"),
                     (dict(unc=ws + need - 8), "unc overlaps the workspace"), (dict(flag=img2 + 3), "flag overlaps img2"),
                     (dict(flag=ws), "flag overlaps the workspace"), (dict(flag=unc + px * 8 - 1), "unc overlaps flag")):
        refused(call(**kw), "flow_uncertainty", word)
    with pytest.raises(ValueError, match="lag=5"):
        _lib.check(call(lag=5), "flow_uncertainty")
    sums = P + (7 << 32)
    acc = lib.pivlfn_uncertainty_accumulate
    refused(acc(None, flag, sums, B, H, W, None), "uncertainty_accumulate", "null")
    refused(acc(unc, flag, None, B, H, W, None), "uncertainty_accumulate", "null")
    refused(acc(unc, flag, sums, 0, H, W, None), "uncertainty_accumulate", "positive")
    refused(acc(unc, flag, sums, B, 46341, 46341, None), "uncertainty_accumulate", "2^31")
    refused(acc(unc, flag, sums + 4, B, H, W, None), "uncertainty_accumulate", "8-byte aligned")
    refused(acc(unc, flag, unc + 8, B, H, W, None), "uncertainty_accumulate", "overlaps")
    refused(acc(unc, flag, flag - 8, B, H, W, None), "uncertainty_accumulate", "overlaps")


def test_run_py_uncertainty_flags_parse_and_are_checked_before_a_gpu_is_needed(tmp_path):
    import run as runpy
    plain = runpy.parser.parse_args(["-i", "x"])
    assert plain.uncertainty is None and plain.uncertainty_lag is None and plain.uncertainty_image is False
    assert not [ln for ln in runpy.args_lines(plain) if ln.split(":")[0] in runpy.UNCERTAINTY_FLAGS]
    assert runpy.parser.parse_args(["--uncertainty"]).uncertainty == 8
    full = runpy.parser.parse_args(["--uncertainty", "4", "--uncertainty-lag", "1", "--uncertainty-image", "--uncertainty-max", "0.2"])
    assert (full.uncertainty, full.uncertainty_lag, full.uncertainty_image, full.uncertainty_max) == (4, 1, True, 0.2)
    lines = runpy.args_lines(full)
    assert "uncertainty: 4\n" in lines and "uncertainty_lag: 1\n" in lines and not [ln for ln in lines if ln.startswith("quality")]
    base = ["--model", "piv", "-i", str(tmp_path), "-o", str(tmp_path / "out")]
    for extra, word in ((["--uncertainty-image"], "need --uncertainty"), (["--uncertainty-lag", "1"], "need --uncertainty"),
                        (["--uncertainty", "16"], "radius=16"), (["--uncertainty", "--uncertainty-lag", "5"], "lag=5"),
                        (["--uncertainty", "--uncertainty-max", "1"], "needs --uncertainty-image"),
                        (["--uncertainty", "--uncertainty-image", "--uncertainty-max", "0"], "finite positive"),
                        (["--uncertainty", "-c", "1.5"], "-b/-c")):
        with pytest.raises(SystemExit, match=word):
            runpy.main(base + extra)
    assert not (tmp_path / "out").exists()
