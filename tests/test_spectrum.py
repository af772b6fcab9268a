"""CPU: the contract of pivlfn_spectrum_accumulate as tests/spectrum_restatement.py states it, and the host side of pivlfn.spectrum --
the basis (window, detrending, trigonometry), the normalisation against scipy.signal.welch, Parseval's sum, a planted line (peak
refinement, phase, coherence), the segment bookkeeping, every refusal and save / load.  The GPU kernel is held to the restatement's
bits in tests/test_gpu_spectrum.py."""
import numpy as np
import pytest
import torch

import spectrum_restatement as sr
from pivlfn import spectrum as S


def _result(series, L, hop, window="hann", detrend="constant", fs=1.0, K=None):
    """[n,2,N] float32 -> the TemporalSpectrumResult of the restatement's sums, vectors as a [1,N] grid."""
    B = S.basis(L, window, detrend, K)
    acc, count, launched = sr.welch_sums(series, L, hop, B)
    N = series.shape[2]
    return S.TemporalSpectrumResult(acc.reshape(-1, 4, 1, N), count.reshape(1, N), L, fs, window, detrend, L - hop, 1, series.shape[0], launched, 1, N)


def _walk(n, N, seed):
    """Random walk plus noise, rounded to float32: [n,2,N]."""
    rng = np.random.default_rng(seed)
    return (np.cumsum(rng.normal(0, 0.3, (n, 2, N)), axis=0) + rng.normal(0, 1.0, (n, 2, N))).astype(np.float32)


WELCH = [(16, 8, 64, "constant"), (64, 32, 300, "constant"), (256, 128, 1000, "constant"), (10, 10, 57, "constant"), (9, 4, 50, "constant"),
         (64, 32, 300, "linear")]


@pytest.mark.parametrize("L,hop,n,detrend", WELCH)
def test_density_is_scipy_welchs(L, hop, n, detrend):
    """Per vector the largest |psd - welch| stays within 1e-12 of the vector's largest density (measured: see DESIGN 4.17; a
    scaling, window or one-sided-weight mistake is off by tens of percent)."""
    signal = pytest.importorskip("scipy.signal")
    fs, N = 2.5, 3
    series = _walk(n, N, 10 * L + hop)
    res = _result(series, L, hop, "hann", detrend, fs)
    worst = 0.0
    for band, comp in (("uu", 0), ("vv", 1)):
        f, want = signal.welch(series[:, comp].astype(np.float64), fs=fs, window="hann", nperseg=L, noverlap=L - hop, detrend=detrend,
                               scaling="density", return_onesided=True, axis=0)
        got = res.psd(band)[:, 0]
        assert got.shape == want.shape and np.allclose(f, res.freq, rtol=1e-15, atol=0)
        ratio = np.abs(got - want).max(axis=0) / want.max(axis=0)
        worst = max(worst, float(ratio.max()))
    print(f"welch L={L} hop={hop} n={n} {detrend}: largest |psd - welch| / max density = {worst:.2e}")
    assert worst <= 1e-12
    assert (res.segments == (n - L) // hop + 1).all()


@pytest.mark.parametrize("L", [12, 9])
def test_parseval(L):
    """Boxcar, no detrending, one segment: sum_k w_k acc_k / L = sum_t x_t^2 within 8 L 2^-53 relative."""
    series = _walk(L, 4, L)
    res = _result(series, L, L, "boxcar", None)
    for band, comp in (("uu", 0), ("vv", 1)):
        energy = (res.weight[:, None] * res.acc[:, comp, 0]).sum(axis=0) / L
        want = (series[:, comp].astype(np.float64) ** 2).sum(axis=0)
        rel = np.abs(energy - want) / want
        print(f"parseval L={L} {band}: {rel.max():.2e}")
        assert rel.max() <= 8 * L * 2.0 ** -53


L0, K0 = 64, 16
OFFSETS = np.linspace(-0.49, 0.49, 15)
PHASES = np.arange(8) * (2 * np.pi / 8)


def planted_series():
    """[64, 2, 15 * 8] float32: one vector per (offset, phase)."""
    cols = [sr.planted_line(L0, L0, K0, d, phi)[:, :, 0] for d in OFFSETS for phi in PHASES]
    return np.stack(cols, axis=2)


def test_planted_line_peak():
    """u = 3 + 2 cos(2 pi (16 + d) t / 64 + phi): peak() returns 16 + d within 1e-4 bin for every offset and phase."""
    res = _result(planted_series(), L0, L0)
    f, top, share = res.peak("uu")
    want = np.repeat(K0 + OFFSETS, len(PHASES)) / L0
    err = np.abs(f[0] - want) * L0
    print(f"planted line: worst peak error {err.max():.2e} bin")
    assert err.max() <= 1e-4
    assert (share[0] > 0.4).all() and (top[0] > 0).all()
    fb, _, _ = res.peak("uu+vv", fmin=10 / L0, fmax=20 / L0)
    assert np.abs(fb[0] - want).max() * L0 <= 1e-4
    at_end = res.peak("uu", fmin=K0 / L0)[0][0]                               # the peak bin at the end of the range: not refined
    low = np.repeat(OFFSETS, len(PHASES)) < 0
    assert (at_end[low] == K0 / L0).all()


def test_planted_line_phase_and_coherence():
    """With v = 1.5 sin(the same argument) v lags u by a quarter period: at the line's bin phase() is +pi/2 within 1e-9, |Co/Qd| <
    1e-12 and the coherence within 1e-12 of 1 (measured 3.8e-15, 3.8e-15, 2.2e-16).  Held where the line sits on its bin (d = 0,
    the eight phases 2 pi j / 8): off the bin the image of the line at -(16 + d) leaks about 2 W(32 + 2d)/W(d) of its amplitude
    into Co with the sign of sin(2 phi), |Co/Qd| up to 2.1e-6 -- the data's own spectrum, not an error of the estimator, so no
    implementation can hold 1e-12 there; that figure is printed and held to 1e-3, the coherence to 1e-12 at every offset."""
    series = np.stack([sr.planted_line(L0, L0, K0, 0.0, phi)[:, :, 0] for phi in PHASES], axis=2)
    res = _result(series, L0, L0)
    f, _, _ = res.peak("uu")
    assert np.abs(f[0] * L0 - K0).max() <= 1e-4
    co, qd = res.acc[K0, S.CO, 0], res.acc[K0, S.QD, 0]
    print(f"planted line on the bin: |Co/Qd| {np.abs(co / qd).max():.2e}, phase error {np.abs(res.phase()[K0, 0] - np.pi / 2).max():.2e}, "
          f"coherence error {np.abs(res.coherence()[K0, 0] - 1).max():.2e}")
    assert (qd > 0).all() and np.abs(co / qd).max() < 1e-12
    assert np.abs(res.phase()[K0, 0] - np.pi / 2).max() <= 1e-9
    assert np.abs(res.coherence()[K0, 0] - 1.0).max() <= 1e-12
    off = _result(planted_series(), L0, L0)
    k = np.rint(off.peak("uu")[0][0] * L0).astype(int)
    leak = np.abs(off.acc[k, S.CO, 0, np.arange(k.size)] / off.acc[k, S.QD, 0, np.arange(k.size)])
    print(f"planted line off the bin: |Co/Qd| up to {leak.max():.2e}")
    assert leak.max() < 1e-3 and np.abs(off.coherence()[k, 0, np.arange(k.size)] - 1.0).max() <= 1e-12


@pytest.mark.parametrize("L,window", [(64, "hann"), (9, "hann"), (12, "boxcar")])
def test_constant_series_projects_to_rounding(L, window):
    """Under constant detrending a constant series leaves every projection below L 2^-52 |x| sum |window|."""
    x = np.float32(7.3)
    X = np.full((L, 2), x, np.float32)
    B = S.basis(L, window, "constant")
    bound = L * 2.0 ** -52 * float(x) * np.abs(S.window_values(L, window)).sum()
    for a in sr.projections(X, 0, 1, B):
        assert np.abs(a).max() <= bound
    assert np.abs(sr.projections(X, 0, 1, S.basis(L, window, None))[0][0]).max() > 1.0        # without detrending DC is there


def test_basis_detrending_is_a_projection():
    """Rows after "constant" sum to rounding; after "linear" they are also orthogonal to t; None keeps window * cos / sin; the angle
    is reduced mod L before the trigonometry."""
    L = 50
    w, t = S.window_values(L, "hann"), np.arange(L)
    raw = S.basis(L, "hann", None)
    assert raw.shape == (26, 2, L) and np.array_equal(raw[3, 0], w * np.cos(2 * np.pi * ((3 * t) % L) / L))
    assert np.array_equal(raw[0, 1], np.zeros(L)) and np.array_equal(S.basis(L, "boxcar", None, 4)[0, 0], np.ones(L))
    assert np.abs(S.basis(L, "hann", "constant").sum(axis=2)).max() < 1e-13
    lin = S.basis(L, "hann", "linear")
    assert np.abs(lin.sum(axis=2)).max() < 1e-13 and np.abs(lin @ t).max() < 1e-10
    assert S.window_values(8, "hann")[0] == 0.0 and S.window_values(8, "hann")[4] == 1.0             # periodic: the peak at L/2


# ---- the segment bookkeeping -----------------------------------------------------------------------------------------------------------
def _plan(n, L, hop, batch):
    """The launches of n frames fed in batches of `batch`: (segment, frames seen when it is launched, first), and the left-over."""
    seen, out, left = 0, [], 0
    while seen < n:
        B = min(batch, n - seen)
        launches, left = S.segment_plan(seen, B, L, hop)
        ends = [x.end for x in launches]
        assert ends == sorted(ends) and all(1 <= e <= B for e in ends)
        out += [(x.segment, seen + x.end, x.first) for x in launches]
        seen += B
    return out, left


@pytest.mark.parametrize("hop", [8, 4, 3])
def test_segment_plan(hop):
    """L = 8: segment s is launched when frame s*hop + 7 is in the ring, with first = (s*hop) % 8, whatever the batches are."""
    L, n = 8, 43
    nseg = (n - L) // hop + 1
    want = [(s, s * hop + L, (s * hop) % L) for s in range(nseg)]
    for batch in (1, 5, 20, n):
        got, left = _plan(n, L, hop, batch)
        assert got == want, (hop, batch)
        assert left == n - ((nseg - 1) * hop + L)
    assert S.segment_plan(0, 7, L, hop) == ([], 7) and S.segment_plan(3, 2, L, hop) == ([], 5)
    assert S.segment_plan(0, 8, L, hop) == ([S.Launch(0, 8, 0)], 0)
    assert [x.end for x in S.segment_plan(5, 20, L, hop)[0]] == [e for e in range(1, 21) if (5 + e - L) % hop == 0 and 5 + e >= L]


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,word", [
    (dict(segment=1), "segment"), (dict(segment=1025), "segment"), (dict(segment=8.0), "segment"), (dict(segment=True), "segment"),
    (dict(segment=8, overlap=-1), "overlap"), (dict(segment=8, overlap=8), "overlap"), (dict(segment=8, kmax=0), "kmax"),
    (dict(segment=8, kmax=5), "kmax"), (dict(segment=9, kmax=5), "kmax"), (dict(window="hamming"), "window"), (dict(detrend="quadratic"), "detrend"),
    (dict(fs=0), "fs"), (dict(fs=-1.0), "fs"), (dict(fs=float("nan")), "fs"), (dict(fs="1"), "fs"), (dict(cell=0), "cell"),
    (dict(cell=1.5), "cell")])
def test_parameters_are_refused_before_the_library_is_touched(kw, word, monkeypatch):
    from pivlfn import _lib
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    with pytest.raises(ValueError, match=word):
        S.check_params(**kw)
    with pytest.raises(ValueError, match=word):
        S.TemporalSpectrum(16, 16, **kw)


def test_sizes_and_flows_are_refused(monkeypatch):
    from pivlfn import _lib
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    for H, W in ((0, 8), (8, -1), (8.0, 8)):
        with pytest.raises(ValueError, match="size"):
            S.TemporalSpectrum(H, W)
    with pytest.raises(ValueError, match="2\\^31"):
        S.check_size(40000, 40000)
    assert S.check_size(40000, 40000, 4) == (10000, 10000) and S.check_params() == (128, 128) and S.check_params(9, 0, kmax=4) == (0, 4)
    dev = torch.device("cuda:0")
    with pytest.raises(TypeError):
        S.check_flows(np.zeros((1, 2, 4, 6), np.float32), 4, 6, dev)
    with pytest.raises(TypeError, match="float32"):
        S.check_flows(torch.zeros(1, 2, 4, 6, dtype=torch.float64), 4, 6, dev)
    for shape in ((2, 4, 6), (1, 3, 4, 6), (1, 2, 6, 4), (1, 2, 4, 7)):
        with pytest.raises(ValueError, match="shape"):
            S.check_flows(torch.zeros(shape), 4, 6, dev)
    with pytest.raises(ValueError, match="flows on cpu"):
        S.check_flows(torch.zeros(1, 2, 4, 6), 4, 6, dev)
    S.check_flows(torch.zeros(0, 2, 4, 6), 4, 6, torch.device("cpu"))


def refusals(lib, X, basis, acc, count):
    """Every error of the contract through the C entry point with the given addresses (never dereferenced: each call fails its checks
    before any launch); also called by the GPU test with real buffers, whose contents must stay."""
    def call(**kw):
        a = dict(X=X, L=8, first=0, N=10, ldx=20, basis=basis, K=5, acc=acc, count=count)
        a.update(kw)
        return lib.pivlfn_spectrum_accumulate(a["X"], a["L"], a["first"], a["N"], a["ldx"], a["basis"], a["K"], a["acc"], a["count"], None)

    def refused(rc, *words):
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1, (rc, msg)
        for w in ("spectrum_accumulate",) + words:
            assert w in msg, (w, msg)

    for name in ("X", "basis", "acc", "count"):
        refused(call(**{name: None}), "null")
    refused(call(L=1), "L=1")
    refused(call(L=1025), "L=1025")
    refused(call(first=-1), "first=-1")
    refused(call(first=8), "first=8")
    refused(call(K=0), "K=0")
    refused(call(K=514), "K=514")
    refused(call(N=0), "N=0")
    refused(call(N=-4), "N=-4")
    refused(call(N=1 << 30, ldx=1 << 31), "2^31")
    refused(call(ldx=19), "ldx=19")


def test_c_entry_point_refuses_bad_arguments_without_a_gpu():
    from pivlfn import _lib
    lib = _lib.load()
    P = 1 << 20                     # non-null, 8-byte aligned, never dereferenced
    refusals(lib, *(P + (i << 32) for i in range(4)))


# ---- save and load ---------------------------------------------------------------------------------------------------------------------
def test_save_and_load_round_trip(tmp_path):
    series = _walk(40, 6, 3)
    series[7, 0, 2] = 1e10                                     # vector 2 misses the segments that hold frame 7
    res = _result(series, 8, 3, "boxcar", "linear", fs=4.0, K=4)
    assert res.segments[0, 2] == res.launched - 3 and (np.delete(res.segments[0], 2) == res.launched).all()
    path = res.save(str(tmp_path / "spec"), validation="flag")
    assert path.endswith("spec.npz")
    back = S.TemporalSpectrumResult.load(path)
    assert sr.same_bits(back.acc, res.acc) and np.array_equal(back.segments, res.segments)
    for name in ("L", "fs", "window", "detrend", "overlap", "cell", "frames", "launched", "H", "W", "K"):
        assert getattr(back, name) == getattr(res, name), name
    assert sr.same_bits(back.psd("vv"), res.psd("vv")) and back.summary() == res.summary()
    with np.load(path) as f:
        assert str(f["validation"]) == "flag" and np.array_equal(f["freq"], np.arange(4) * 4.0 / 8) and np.array_equal(f["psd_uu"], res.pooled("uu"))
    none = _result(series, 8, 8, "hann", None)
    assert S.TemporalSpectrumResult.load(none.save(str(tmp_path / "none.npz"))).detrend is None
    s = res.summary()
    assert s["segments"] == 11 and s["frames"] == 40 and s["frames_left_over"] == 40 - (10 * 3 + 8) and s["resolution"] == 0.5
    assert s["valid_vectors"] == 6 and 0 < s["peak_share"] <= 1


def test_a_vector_without_a_segment_is_nan():
    series = _walk(16, 3, 5)
    series[:, 1, 1] = np.nan
    res = _result(series, 8, 4)
    assert res.segments[0].tolist() == [3, 0, 3]
    for a in (res.psd("uu"), res.psd("vv"), res.coherence(), res.phase(), res.cross().real):
        assert np.isnan(a[:, 0, 1]).all() and np.isfinite(a[1:, 0, 0]).all()
    f, top, share = res.peak()
    assert np.isnan(f[0, 1]) and np.isnan(top[0, 1]) and np.isfinite(f[0, [0, 2]]).all()
    assert np.isfinite(res.pooled("uu")).all() and sr.same_bits(res.acc[:, :, 0, 1], np.zeros((5, 4)))


# ---- run.py's flags --------------------------------------------------------------------------------------------------------------------
def test_run_py_spectrum_flags_parse_and_are_checked_before_a_gpu_is_needed(tmp_path, monkeypatch):
    import run as runpy
    plain = runpy.parser.parse_args(["-i", "x"])
    assert plain.spectrum is None and plain.spectrum_overlap is None and plain.spectrum_image is False and plain.spectrum_fps is None
    assert not [ln for ln in runpy.args_lines(plain) if "spectrum" in ln]
    assert runpy.parser.parse_args(["--spectrum"]).spectrum == 256
    full = runpy.parser.parse_args(["--spectrum", "64", "--spectrum-overlap", "48", "--spectrum-cell", "4", "--spectrum-fps", "1000", "--spectrum-image"])
    assert (full.spectrum, full.spectrum_overlap, full.spectrum_cell, full.spectrum_fps, full.spectrum_image) == (64, 48, 4, 1000.0, True)
    lines = runpy.args_lines(full)
    assert "spectrum: 64\n" in lines and "spectrum_overlap: 48\n" in lines and "spectrum_fps: 1000.0\n" in lines and "spectrum_image: True\n" in lines
    assert not [ln for ln in lines if ln.startswith(("color", "quality", "pod", "vortex", "ftle", "twopoint"))]
    assert not [ln for ln in runpy.args_lines(runpy.parser.parse_args(["--twopoint"])) if "spectrum" in ln]
    base = ["--model", "piv", "-i", str(tmp_path), "-o", str(tmp_path / "out")]
    for extra, word in ((["--spectrum-image"], "need --spectrum"), (["--spectrum-overlap", "3"], "need --spectrum"),
                        (["--spectrum-cell", "2"], "need --spectrum"), (["--spectrum-fps", "2"], "need --spectrum"),
                        (["--spectrum", "1"], "segment=1"), (["--spectrum", "1025"], "segment=1025"),
                        (["--spectrum", "8", "--spectrum-overlap", "8"], "overlap=8"), (["--spectrum", "8", "--spectrum-cell", "0"], "cell=0"),
                        (["--spectrum", "8", "--spectrum-fps", "0"], "fs=0"), (["--spectrum", "-p"], "not a time series"),
                        (["--spectrum", "-c", "1.5"], "-b/-c"), (["--spectrum", "-b", "0.5"], "-b/-c")):
        with pytest.raises(SystemExit, match=word):
            runpy.main(base + extra)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="single process"):
        runpy.main(base + ["--spectrum"])
    assert not (tmp_path / "out").exists()
