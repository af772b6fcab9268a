"""CPU: the distribution contract (include/pivlfn.h, pivlfn_flow_moments_accumulate and pivlfn_flow_hist_accumulate) as
tests/distribution_restatement.py states it -- the plane form against the vector-by-vector loop, and on the committed DNS flow the
numbers the feature was specified with --, pivlfn.distribution.DistributionResult on synthetic sums, the launch plan and the refusals
of the C entry points, which all come before any launch and so need no GPU, and the command line of run.py --pdf."""
import ctypes
import math
import os

import numpy as np
import pytest

import distribution_restatement as dr
from conftest import GOLD

f64 = np.float64
_dns = {}


def dns():
    if "flow" not in _dns:
        _dns["flow"] = dr.read_flo(os.path.join(GOLD, "DNS_turbulence_flow.flo"))[None]
    return _dns["flow"]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_planes_equal_loops_on_5_x_7_x_3():
    """B = 3 frames of 5 x 7 with invalid vectors, from non-zero sums and counters, with and without mask, mean, scale and thr."""
    rng = np.random.default_rng(57)
    flow, mask, mean, scale, thr = dr.random_case(rng, 3, 5, 7, holes=False)
    flow[0, 0, 1, 2], flow[1, 1, 3, 3], flow[2, 0, 4, 6], flow[2, 1, 0, 0] = np.nan, 1e10, -np.inf, -0.0
    flow[1, :, 2, 2], flow[0, :, 2, 5] = (-2.0, 2.0), (1.999, -1e-30)           # on an edge, just below one, a fraction that rounds to 1
    scale[0, 0, 1], scale[1, 4, 4], scale[0, 3, 0], mean[1, 2, 6], thr[1, 1] = 0.0, -1.0, np.nan, np.inf, np.nan
    acc0 = rng.normal(0, 5, (21, 5, 7))
    nb, jb, fb = 7, 3, 5
    h0 = rng.integers(0, 9, dr.hist_words(nb, jb, fb)).astype(np.uint64)
    for m, mu, sc, t in ((None, None, None, None), (mask, None, None, None), (mask, mean, scale, thr), (None, mean, None, thr), (None, None, scale, None)):
        a, b = dr.moments(flow, m, mu, t, acc0), dr.moments_loops(flow, m, mu, t, acc0)
        assert dr.same_bits(a, b)
        g, h = dr.hist(flow, m, mu, sc, h0, -2.0, 2.0, nb, jb, fb), dr.hist_loops(flow, m, mu, sc, h0, -2.0, 2.0, nb, jb, fb)
        assert np.array_equal(g, h)
        at = dr.layout(nb, jb, fb)
        add = (g - h0).astype(np.int64)
        n, out = add[at["counted"]], add[at["counted"] + 1]
        assert n + out == 3 * 5 * 7 and 0 < out < 3 * 5 * 7
        for lo_, hi_ in ((at["u"], at["v"]), (at["v"], at["joint"]), (at["joint"], at["frac_u"]), (at["frac_u"], at["frac_v"]), (at["frac_v"], at["counted"])):
            assert add[lo_:hi_].sum() == n                                      # every vector adds to exactly one word of each part
        assert (a[0] - acc0[0]).sum() > 0
    assert not dr.same_bits(dr.moments(flow, mask, None, None, acc0), dr.moments(flow, None, None, None, acc0))


def test_edges_fractions_and_signed_zero():
    """Values on bin edges, at lo, at hi and just below it; -0.0; a tiny negative displacement, whose fraction rounds to 1.0."""
    vals = np.array([-2.0, 2.0, np.nextafter(np.float32(2.0), np.float32(0.0)), -1.0, 0.0, -0.0, 1.0, -1e-30, 0.5, -2.5], np.float32)
    flow = np.stack([vals, vals])[None, :, None, :]
    at = dr.layout(4, 4, 4)
    h = dr.hist(flow, None, None, None, np.zeros(dr.hist_words(4, 4, 4), np.uint64), -2.0, 2.0, 4, 4, 4).astype(np.int64)
    #                     under  [-2,-1) [-1,0) [0,1) [1,2)  over
    assert list(h[at["u"]:at["v"]]) == [1, 1, 1, 4, 2, 1]                      # -0.0 and -1e-30 (2 - 1e-30 rounds to 2) sit in [0, 1)
    assert list(h[at["v"]:at["joint"]]) == [1, 1, 1, 4, 2, 1]
    assert np.array_equal(h[at["joint"]:at["outside"]].reshape(4, 4), np.diag([1, 1, 4, 2])) and h[at["outside"]] == 2
    #                                              [0, .25)  ..  [.5, .75)  [.75, 1): 1.9999999 and the 1.0 of -1e-30
    assert list(h[at["frac_u"]:at["frac_v"]]) == [6, 0, 2, 2] and list(h[at["frac_v"]:at["counted"]]) == [6, 0, 2, 2]
    assert h[at["counted"]] == 10 and h[at["counted"] + 1] == 0


def test_dns_fixture_numbers():
    """tests/golden/DNS_turbulence_flow.flo, 256 x 256, in float64: the extremes, the vectors outside [-4, 4) and [-2, 2), the
    16-bin fraction histograms and the pooled skewness and flatness about the frame mean, as the feature was specified."""
    from pivlfn.distribution import DistributionResult
    flow = dns()
    assert flow.shape == (1, 2, 256, 256)
    assert abs(float(flow.min()) - -2.589) < 1e-3 and abs(float(flow.max()) - 2.751) < 1e-3
    wide = dr.hist(flow, None, None, None, np.zeros(dr.hist_words(64, 16, 16), np.uint64), -4.0, 4.0, 64, 16, 16)
    narrow = dr.hist(flow, None, None, None, np.zeros(dr.hist_words(64, 16, 16), np.uint64), -2.0, 2.0, 64, 16, 16)
    acc = dr.moments(flow, None, None, None, np.zeros((21, 256, 256)))
    r = DistributionResult(acc, wide, 64, (-4.0, 4.0), 16, 16, 1)
    assert r.counted == 65536 and r.left_out == 0 and r.outside("u") == (0.0, 0.0) and r.outside("v") == (0.0, 0.0) and r.outside_joint() == 0.0
    assert int(narrow[dr.layout(64, 16, 16)["outside"]]) == 853
    fu, fv = r.fraction("u"), r.fraction("v")
    assert (int(fu.min()), int(fu.max()), int(fv.min()), int(fv.max())) == (3701, 4719, 3643, 4423)
    assert abs(r.peak_locking("u") - 0.2157) < 5e-5 and abs(r.peak_locking("v") - 0.1764) < 5e-5
    p = r.pooled()
    u, v = flow[0, 0].astype(f64).ravel(), flow[0, 1].astype(f64).ravel()
    for c, x, skew, flat in (("u", u, -0.0073, 2.693), ("v", v, 0.1792, 3.046)):
        d = x - x.mean()
        assert abs(p[f"skewness_{c}"] - skew) < 5e-5 and abs(p[f"flatness_{c}"] - flat) < 5e-4
        assert abs(p[f"skewness_{c}"] - (d ** 3).mean() / (d ** 2).mean() ** 1.5) < 1e-10
        assert abs(p[f"flatness_{c}"] - (d ** 4).mean() / (d ** 2).mean() ** 2) < 1e-10
    # rounded to integers the same flow is completely locked
    locked = np.rint(flow).astype(np.float32)
    h = dr.hist(locked, None, None, None, np.zeros(dr.hist_words(64, 16, 16), np.uint64), -4.0, 4.0, 64, 16, 16)
    r = DistributionResult(acc, h, 64, (-4.0, 4.0), 16, 16, 1)
    assert r.peak_locking("u") == 1.0 and r.peak_locking("v") == 1.0 and int(r.fraction("u")[0]) == 65536


# ---- DistributionResult on synthetic sums ----------------------------------------------------------------------------------------------
def _sample_result(hole=0.0, n=40, H=2, W=3, lo=-0.5, hi=1.0):
    """n frames of H x W drawn from a skewed distribution, through the restatement."""
    from pivlfn.distribution import DistributionResult
    rng = np.random.default_rng(11)
    flow = (rng.gamma(2.0, 0.5, (n, 2, H, W)) - 1.0).astype(np.float32)
    flow[:, 1] = flow[:, 1] * -0.7 + 0.3 * flow[:, 0]
    thr = None if hole == 0.0 else np.full((H, W), hole)
    acc = dr.moments(flow, None, None, thr, np.zeros((21, H, W)))
    h = dr.hist(flow, None, None, None, np.zeros(dr.hist_words(16, 8, 8), np.uint64), lo, hi, 16, 8, 8)
    return flow, DistributionResult(acc, h, 16, (lo, hi), 8, 8, n, hole)


def test_pdf_integrates_to_the_share_inside_the_range():
    flow, r = _sample_result()
    for c, k in (("u", 0), ("v", 1)):
        centres, density = r.pdf(c)
        width = centres[1] - centres[0]
        under, over = r.outside(c)
        x = flow[:, k].astype(f64)
        assert abs(density.sum() * width - (1.0 - under - over)) < 1e-14
        assert under == np.mean(x < -0.5) and over == np.mean(x >= 1.0) and under > 0 and over > 0
        assert abs(centres[0] - (-0.5 + width / 2)) < 1e-15 and len(centres) == 16
    centres, density = r.joint()
    w = centres[1] - centres[0]
    assert density.shape == (8, 8) and abs(density.sum() * w * w - (1.0 - r.outside_joint())) < 1e-14
    assert r.counted == flow.shape[0] * 6 and r.left_out == 0


def test_central_moments_agree_with_numpy():
    flow, r = _sample_result()
    for c, k in (("u", 0), ("v", 1)):
        x = flow[:, k].astype(f64)
        d = x - x.mean(0)
        m2, m3, m4 = (d ** 2).mean(0), (d ** 3).mean(0), (d ** 4).mean(0)
        got = r.central(c)
        for g, want in zip(got, (m2, m3, m4)):
            assert np.abs(g - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(r.skewness(c) - m3 / m2 ** 1.5).max() <= 1e-12 and np.abs(r.flatness(c) / (m4 / m2 ** 2) - 1.0).max() <= 1e-12
    assert np.array_equal(r.count, np.full((2, 3), 40.0))
    p = r.pooled()
    x = flow[:, 0].astype(f64).ravel()
    d = x - x.mean()
    assert abs(p["skewness_u"] - (d ** 3).mean() / (d ** 2).mean() ** 1.5) <= 1e-12 and p["count"] == 240.0
    assert abs(p["cov_uv"] - np.cov(x, flow[:, 1].astype(f64).ravel(), bias=True)[0, 1]) <= 1e-13


def test_quadrant_shares_sum_to_one():
    for hole in (0.0, 0.2):
        flow, r = _sample_result(hole)
        q = r.quadrants()
        assert q["events"].shape == (4, 2, 3) and np.abs(q["events"].sum(0) - 1.0).max() < 1e-14
        U, V = flow[:, 0].astype(f64), flow[:, 1].astype(f64)
        P = U * V
        in2 = (np.abs(P) > hole) & (U < 0) & (V > 0)
        assert np.array_equal(r.acc[14], in2.sum(0)) and in2.sum() > 0
        with np.errstate(invalid="ignore"):
            assert np.allclose(q["mean"][1], (P * in2).sum(0) / in2.sum(0), rtol=1e-13, equal_nan=True)    # NaN where Q2 has no event
        if hole == 0.0:
            assert np.abs(q["stress"].sum(0) - 1.0).max() < 1e-12 and np.abs(q["hole"]).max() == 0
        else:
            assert (q["hole"] > 0).all()
        pooled = r.quadrants(pooled=True)
        assert pooled["events"].shape == (4,) and abs(pooled["events"].sum() - 1.0) < 1e-14


def test_everything_is_nan_without_vectors():
    from pivlfn.distribution import DistributionResult
    r = DistributionResult(np.zeros((21, 2, 2)), np.zeros(dr.hist_words(4, 2, 4), np.uint64), 4, (-1.0, 1.0), 2, 4)
    assert np.isnan(r.pdf("u")[1]).all() and np.isnan(r.joint()[1]).all() and all(math.isnan(x) for x in r.outside("v"))
    assert math.isnan(r.peak_locking("u")) and math.isnan(r.outside_joint())
    assert np.isnan(r.skewness("u")).all() and np.isnan(r.flatness("v")).all() and not r.count.any()
    assert all(np.isnan(v).all() for v in r.quadrants().values())
    p = r.pooled()
    assert p["count"] == 0.0 and all(math.isnan(p[k]) for k in p if k != "count")
    s = r.summary()
    assert s["counted"] == 0 and math.isnan(s["peak_locking_v"])
    # one vector a pixel: a count but no variance
    acc = np.zeros((21, 1, 1))
    acc[[0, 1, 3, 6, 10], 0, 0] = 1.0, 2.0, 4.0, 8.0, 16.0
    one = DistributionResult(acc, np.zeros(dr.hist_words(4, 0, 0), np.uint64), 4, (-1.0, 1.0), 0, 0)
    assert np.isnan(one.skewness("u")).all() and np.isnan(one.flatness("u")).all() and math.isnan(one.peak_locking("u"))
    with pytest.raises(ValueError):
        one.joint()


def test_save_load_round_trip_and_checks(tmp_path):
    from pivlfn import distribution as D
    _, r = _sample_result(0.2)
    path = r.save(str(tmp_path / "pdf"), validation="flag")
    back = D.DistributionResult.load(path)
    assert dr.same_bits(back.acc, r.acc) and np.array_equal(back.hist, r.hist) and back.hist.dtype == np.uint64
    assert (back.bins, back.lo, back.hi, back.joint_bins, back.frac_bins, back.frames, back.hole, back.normalised) == (16, -0.5, 1.0, 8, 8, 40, 0.2, False)
    assert back.summary() == r.summary()
    with np.load(path) as f:
        assert str(f["validation"]) == "flag" and np.array_equal(f["pdf_u"], r.pdf("u")[1]) and np.array_equal(f["frac_v"], r.fraction("v"))
    for bad in ((0, (-1, 1), 4, 4), (4097, (-1, 1), 4, 4), (8, (-1, 1), 257, 4), (8, (-1, 1), 4, 1025), (8, (1, 1), 4, 4), (8, (0, math.inf), 4, 4),
                (8, (0, math.nan), 4, 4), (8, 3.0, 4, 4), (8.0, (-1, 1), 4, 4), (True, (-1, 1), 4, 4), (8, (-1, 1), 4, 4, -0.5)):
        with pytest.raises(ValueError):
            D.check_params(*bad)
    D.check_params(1, (-1, 1), 0, 0)
    with pytest.raises(ValueError, match="sums"):
        D.DistributionResult(np.zeros((20, 2, 2)), np.zeros(9, np.uint64), 1, (0, 1), 0, 0)
    with pytest.raises(ValueError, match="counters"):
        D.DistributionResult(np.zeros((21, 2, 2)), np.zeros(10, np.uint64), 1, (0, 1), 0, 0)
    assert D.hist_words(256, 64, 64) == dr.hist_words(256, 64, 64) == 4743


# ---- the C entry points: names, plan and refusals, all on the host ---------------------------------------------------------------------
def test_the_new_names_are_bound():
    from pivlfn import _lib
    for name in ("pivlfn_flow_moments_accumulate", "pivlfn_flow_hist_accumulate", "pivlfn_flow_hist_plan"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert _lib.load().pivlfn_abi_version() == 3


def plan(B, H, W, nbins, jbins, fbins):
    """pivlfn_flow_hist_plan as a dict."""
    from pivlfn import _lib
    out = (ctypes.c_int * 5)()
    _lib.check(_lib.load().pivlfn_flow_hist_plan(B, H, W, nbins, jbins, fbins, out), "flow_hist_plan")
    return dict(zip(("groups", "lds_words", "joint_in_lds", "words", "moment_blocks"), out))


def test_launch_plan():
    """The table lives in LDS whole up to 16384 counters (64 KiB); above, the joint table goes to global memory.  At most 512
    workgroups of 512 threads x 4 vectors; the moments follow the frame-grid rule up to 4096 workgroups."""
    assert plan(8, 1024, 1024, 256, 64, 64) == {"groups": 512, "lds_words": 4743, "joint_in_lds": 1, "words": 4743, "moment_blocks": 4096}
    assert plan(1, 1, 1, 1, 0, 0) == {"groups": 1, "lds_words": 9, "joint_in_lds": 1, "words": 9, "moment_blocks": 1}
    big = plan(3, 37, 53, 4096, 256, 1024)
    assert big == {"groups": 3, "lds_words": 10247, "joint_in_lds": 0, "words": 75783, "moment_blocks": 8}
    fits, over = plan(3, 37, 53, 124, 127, 0), plan(3, 37, 53, 125, 127, 0)
    assert fits["words"] == 16384 and fits["joint_in_lds"] == 1 and fits["lds_words"] == 16384
    assert over["words"] == 16386 and over["joint_in_lds"] == 0 and over["lds_words"] == 16386 - 127 * 127
    assert plan(1, 32, 64, 8, 0, 0)["groups"] == 1 and plan(1, 32, 65, 8, 0, 0)["groups"] == 2           # 2048 vectors a workgroup and sweep
    assert plan(2, 512, 1024, 8, 0, 0)["groups"] == 512 and plan(1, 1023, 1024, 8, 0, 0)["groups"] == 512   # from 2^20 vectors the loop runs
    assert plan(1, 1024, 1024, 8, 0, 0)["moment_blocks"] == 4096 and plan(1, 1024, 1023, 8, 0, 0)["moment_blocks"] == 4092
    assert plan(0, 8, 8, 8, 0, 0)["groups"] == 0


def refusals(lib, flow, mask, mean, extra, acc, hist, B, H, W):
    """Every error of the contract through the two C entry points with the given addresses (never dereferenced: each call fails its
    checks before any launch); also called by the GPU test with real buffers, whose contents must stay.  `extra`: thr and scale."""
    nb, jb, fb = 8, 4, 4

    def mom(**kw):
        a = dict(flow=flow, mask=mask, mean=mean, thr=extra, acc=acc, B=B, H=H, W=W)
        a.update(kw)
        return lib.pivlfn_flow_moments_accumulate(a["flow"], a["mask"], a["mean"], a["thr"], a["acc"], a["B"], a["H"], a["W"], None)

    def his(**kw):
        a = dict(flow=flow, mask=mask, mean=mean, scale=extra, hist=hist, B=B, H=H, W=W, lo=-1.0, hi=1.0, nbins=nb, jbins=jb, fbins=fb)
        a.update(kw)
        return lib.pivlfn_flow_hist_accumulate(a["flow"], a["mask"], a["mean"], a["scale"], a["hist"], a["B"], a["H"], a["W"], a["lo"], a["hi"],
                                               a["nbins"], a["jbins"], a["fbins"], None)

    def refused(rc, op, *words):
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1, (rc, msg)
        for w in (op,) + words:
            assert w in msg, (w, msg)

    px = H * W
    for call, op, out, nout in ((mom, "flow_moments_accumulate", "acc", 21 * px * 8), (his, "flow_hist_accumulate", "hist", dr.hist_words(nb, jb, fb) * 8)):
        refused(call(H=0), op, "positive")
        refused(call(W=-3), op, "positive")
        refused(call(B=-1), op, "B=-1")
        refused(call(H=46341, W=16384 * 4), op, "2^31")
        refused(call(H=0, **{out: None}), op, "positive")                     # the shape comes first
        assert call(B=0, flow=None, **{out: None}) == 0                      # nothing to add: no pointer is read
        assert call(B=0, H=0) == 1                                           # but the sizes are still checked
        refused(call(flow=None), op, "null")
        refused(call(**{out: None}), op, "null")
        where = acc if out == "acc" else hist
        refused(call(**{out: flow}), op, f"{out} overlaps flow")
        refused(call(**{out: flow + B * px * 8 - 8}), op, f"{out} overlaps flow")
        refused(call(**{out: flow - nout + 8}), op, f"{out} overlaps flow")
        refused(call(**{out: mask + B * px - 1}), op, f"{out} overlaps mask")
        refused(call(**{out: mean + px * 16 - 8}), op, f"{out} overlaps mean")
        refused(call(**{out: extra}), op, f"{out} overlaps {'thr' if out == 'acc' else 'scale'}")
        assert where % 8 == 0
    refused(mom(acc=extra + px * 8 - 8), "flow_moments_accumulate", "acc overlaps thr")
    assert mom(B=0, acc=extra) == 0
    refused(his(hist=extra + px * 16 - 8), "flow_hist_accumulate", "hist overlaps scale")
    for kw, word in ((dict(nbins=0), "nbins=0"), (dict(nbins=4097), "nbins=4097"), (dict(jbins=-1), "jbins=-1"), (dict(jbins=257), "jbins=257"),
                     (dict(fbins=-1), "fbins=-1"), (dict(fbins=1025), "fbins=1025")):
        refused(his(**kw), "flow_hist_accumulate", word)
        refused(his(B=0, **kw), "flow_hist_accumulate", word)                 # before B == 0 succeeds
        refused(his(lo=1.0, **kw), "flow_hist_accumulate", word)              # and before the range
    for lo, hi in ((1.0, 1.0), (1.0, -1.0), (-math.inf, 1.0), (0.0, math.inf), (math.nan, 1.0), (0.0, math.nan)):
        refused(his(lo=lo, hi=hi), "flow_hist_accumulate", "range")
        refused(his(lo=lo, hi=hi, B=0), "flow_hist_accumulate", "range")
        refused(his(lo=lo, hi=hi, flow=None), "flow_hist_accumulate", "range")
    refused(his(H=0, nbins=0, lo=2.0), "flow_hist_accumulate", "positive")
    out = (ctypes.c_int * 5)()
    refused(lib.pivlfn_flow_hist_plan(1, 8, 8, 0, 0, 0, out), "flow_hist_accumulate", "nbins=0")
    refused(lib.pivlfn_flow_hist_plan(1, 0, 8, 8, 0, 0, out), "flow_hist_accumulate", "positive")
    refused(lib.pivlfn_flow_hist_plan(1, 8, 8, 8, 0, 0, None), "flow_hist_plan")
    return mom, his


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    from pivlfn import _lib
    lib = _lib.load()
    P = 1 << 20                     # non-null, 8-byte aligned, never dereferenced
    flow, mask, mean, extra, acc, hist = (P + (i << 32) for i in range(6))
    mom, his = refusals(lib, flow, mask, mean, extra, acc, hist, 2, 8, 8)
    with pytest.raises(ValueError, match="nbins=0"):
        _lib.check(his(nbins=0), "flow_hist_accumulate")


# ---- run.py ------------------------------------------------------------------------------------------------------------------------------
def test_run_py_pdf_flags_parse_and_are_checked_before_a_gpu_is_needed(tmp_path):
    import run as runpy
    plain = runpy.parser.parse_args(["-i", "x"])
    assert plain.pdf is None and plain.pdf_range is None and plain.pdf_mean is None and not plain.pdf_normalise and not plain.pdf_image
    assert not [ln for ln in runpy.args_lines(plain) if "pdf" in ln]
    assert not [ln for ln in runpy.args_lines(runpy.parser.parse_args(["--twopoint"])) if "pdf" in ln]
    assert runpy.parser.parse_args(["--pdf"]).pdf == 256
    full = runpy.parser.parse_args(["--pdf", "128", "--pdf-range", "-2", "2", "--pdf-mean", "stats.npz", "--pdf-normalise", "--pdf-hole", "1.5"])
    lines = runpy.args_lines(full)
    for want in ("pdf: 128\n", "pdf_range: [-2.0, 2.0]\n", "pdf_mean: stats.npz\n", "pdf_normalise: True\n", "pdf_hole: 1.5\n", "pdf_image: False\n"):
        assert want in lines
    assert not [ln for ln in lines if ln.startswith(("color", "quality", "pod", "vortex", "twopoint"))]
    assert runpy.pdf_params(full) == (128, (-2.0, 2.0), 64, 64, 1.5)
    assert runpy.pdf_params(runpy.parser.parse_args(["--pdf"]))[1] == (-8.0, 8.0)
    assert runpy.pdf_params(runpy.parser.parse_args(["--pdf", "--pdf-normalise"]))[1] == (-6.0, 6.0)
    base = ["--model", "piv", "-i", str(tmp_path), "-o", str(tmp_path / "out")]
    for extra, word in ((["--pdf-range", "-2", "2"], "need --pdf"), (["--pdf-mean", "x.npz"], "need --pdf"), (["--pdf-normalise"], "need --pdf"),
                        (["--pdf-hole", "1"], "need --pdf"), (["--pdf-image"], "need --pdf"),
                        (["--pdf", "-b", "1.5"], "-b/-c"), (["--pdf", "-c", "0.5"], "-b/-c"),
                        (["--pdf", "--pdf-range", "2", "2"], "hi > lo"), (["--pdf", "--pdf-range", "3", "-3"], "hi > lo"),
                        (["--pdf", "--pdf-range", "0", "inf"], "finite"), (["--pdf", "4097"], "bins=4097"), (["--pdf", "0"], "bins=0"),
                        (["--pdf", "--pdf-hole", "-1"], "hole"), (["--pdf", "--pdf-normalise"], "needs --pdf-mean"),
                        (["--pdf", "--pdf-mean", str(tmp_path / "none.npz")], "not a file")):
        with pytest.raises(SystemExit) as e:
            runpy.main(base + extra)
        assert word in str(e.value), (extra, str(e.value))
    assert not (tmp_path / "out").exists()


def test_run_py_pdf_is_refused_sharded(tmp_path, monkeypatch):
    import run as runpy
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        runpy.main(["--model", "piv", "-i", str(tmp_path), "-o", str(tmp_path / "out"), "--pdf"])
    assert "--pdf needs a single process" in str(e.value)
