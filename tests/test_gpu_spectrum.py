"""GPU: pivlfn_spectrum_accumulate (csrc/spectrum.hip) against the NumPy restatement of its contract (tests/spectrum_restatement.py).
Every operation of the contract is a correctly rounded fp64 operation in a fixed order, so acc is compared bit for bit, every element of
it, and count exactly.  The basis of the bit tests is random normal, not trigonometric, so that a misplaced row or sample shows.
Shapes: segments of 2 and of 1024 samples (one staged chunk and eight), odd lengths, a ring that wraps, one vector, a few below, at and
above one wave and many tiles, K = 1 and K that is no multiple of the frequency group, row strides that are not 16-byte aligned.  Then
validity, how a sequence is cut into update() calls, guarded buffers, the stream and capture contract as tests/test_gpu_op_streams.py
holds the other entry points to it (its helpers, imported), the refusals, TemporalSpectrum end to end and run.py --spectrum."""
import json
import os

import numpy as np
import pytest
import torch

import spectrum_restatement as sr
from guarded import check_guards, guarded
from test_gpu_op_streams import (F32, F64, I32, U8, Spec, _behind_the_delay, _buf, _check, _p, _poisoned, _same, _scribble, delay)  # noqa: F401

pytestmark = pytest.mark.gpu


def _case(L, N, K, pad, seed):
    """A ring [L, 2N + pad] with NaN in the padding columns, a random normal basis [K,2,L], and a non-zero acc and count."""
    rng = np.random.default_rng(seed)
    X = np.full((L, 2 * N + pad), np.nan, np.float32)
    X[:, :2 * N] = rng.normal(0, 3, (L, 2 * N)).astype(np.float32)
    basis = rng.normal(0, 1, (K, 2, L))
    acc0 = rng.normal(0, 50, (K, 4, N))
    count0 = rng.integers(0, 9, N).astype(np.int32)
    return X, basis, acc0, count0


def _run(dev, X, first, N, basis, acc0, count0):
    """One call of the C entry point on the current stream: (acc, count) after it."""
    from pivlfn import _lib
    lib = _lib.load()
    x, b, acc, count = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (X, basis, acc0, count0))
    _lib.check(lib.pivlfn_spectrum_accumulate(x.data_ptr(), X.shape[0], first, N, X.shape[1], b.data_ptr(), basis.shape[0], acc.data_ptr(),
                                              count.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "spectrum_accumulate")
    torch.cuda.synchronize()
    assert sr.same_bits(x.cpu().numpy(), X) and sr.same_bits(b.cpu().numpy(), basis), "an input was written"
    return acc.cpu().numpy(), count.cpu().numpy()


def _compare(got, want, what):
    """Every element of acc bit for bit, every count."""
    (acc, count), (wacc, wcount) = got, want
    same = acc.view(np.int64) == wacc.view(np.int64)
    if not same.all():
        at = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {np.count_nonzero(~same)} of {same.size} sums differ, first at [k, term, p] = {at}: {acc[at]!r} against {wacc[at]!r}")
    assert np.array_equal(count, wcount), f"{what}: counts differ at {np.argwhere(count != wcount)[:4].ravel()}"


CASES = [(2, 1, 2, 0, 0), (5, 63, 3, 3, 1), (33, 65, 17, 20, 0), (64, 257, 33, 63, 2), (12, 1030, 7, 5, 3), (1024, 70, 5, 1000, 0),
         (256, 300, 129, 128, 0)]


def _corner_cases():
    """The corner of the domain, L = 1024 with K = 513, and its ragged neighbour: tests/analysis_plans.py says what each reaches."""
    import analysis_plans as ap
    return ap.shapes(ap.SPECTRUM_CASES)


@pytest.mark.parametrize("L,N,K,first,pad", CASES + _corner_cases())
def test_bits_of_the_restatement(L, N, K, first, pad, dev):
    """From a non-zero acc and count.  2 x 1: the shortest segment, one lane; 5 x 63 and 33 x 65: one lane short of a wave and one past
    it, odd lengths, strides of 127 and 130 floats; 64 x 257 at K = 33: four full frequency groups and a single, the last sample first;
    12 x 1030: 17 tiles; 1024 x 70: eight staged chunks per round; 256 x 300 at K = 129: the default segment, two chunks, three rounds;
    1024 x 65 at K = 513, the corner of the domain: 64 frequency groups and one single over 8 waves, the eight chunks staged again in
    each of the 8 rounds, a second tile of one vector; 1000 x 64 at K = 501: a last chunk of 104 samples, 62 groups (the last round
    has six) and five singles."""
    X, basis, acc0, count0 = _case(L, N, K, pad, 1000 * L + N)
    want = sr.accumulate(X, first, N, basis, acc0, count0)
    _compare(_run(dev, X, first, N, basis, acc0, count0), want, f"L={L} N={N} K={K} first={first}")
    assert np.array_equal(want[1], count0 + 1) and not sr.same_bits(want[0], acc0)
    if first:                                                   # the ring's rotation matters
        assert not sr.same_bits(sr.accumulate(X, 0, N, basis, acc0, count0)[0], want[0])


def test_validity(dev):
    """NaN, +inf, -inf, 1e10 and -2e9 in one sample of u or v: those vectors keep their acc and count bits, all others match the
    restatement; exactly 1e9f (and -1e9f) takes part.  Vector 0, vector N-1, the ring's last row, lanes 63 and 64."""
    L, N, K, first, pad = 12, 200, 9, 5, 1
    X, basis, acc0, count0 = _case(L, N, K, pad, 7)
    plant = [(0, 0, 0, np.nan), (N - 1, 1, L - 1, np.inf), (63, 0, 3, -np.inf), (64, 1, 7, 1e10), (130, 0, L - 1, -2e9), (131, 1, 0, np.nan)]
    for p, comp, row, value in plant:
        X[row, comp * N + p] = value
    X[4, 7], X[9, N + 100] = np.float32(1e9), np.float32(-1e9)
    want = sr.accumulate(X, first, N, basis, acc0, count0)
    got = _run(dev, X, first, N, basis, acc0, count0)
    _compare(got, want, "validity")
    out = [p for p, _, _, _ in plant]
    assert sr.same_bits(got[0][:, :, out], acc0[:, :, out]) and np.array_equal(got[1][out], count0[out])
    stay = np.setdiff1d(np.arange(N), out)
    assert np.array_equal(got[1][stay], count0[stay] + 1) and (got[0][:, :, [7, 100]] != acc0[:, :, [7, 100]]).all()
    assert np.isfinite(got[0][:, :, stay]).all(), "an invalid vector reached another"
    X[:, N:2 * N] = 1e10                                        # no vector takes part: nothing changes
    _compare(_run(dev, X, first, N, basis, acc0, count0), (acc0, count0), "every vector invalid")


@pytest.mark.parametrize("hop", [4, 3])
def test_cutting_the_sequence_into_batches_changes_no_bit(hop, dev):
    """40 frames of 6 x 11 with holes, L = 8, in batches of 1, 5 and 40: identical acc and segments, the restatement's applied segment
    by segment."""
    from pivlfn import TemporalSpectrum
    from pivlfn.spectrum import basis
    n, H, W, L = 40, 6, 11, 8
    rng = np.random.default_rng(40 + hop)
    flows = rng.normal(0, 2, (n, 2, H, W)).astype(np.float32)
    flows[13, 0, 2, 3], flows[30, 1, 5, 10], flows[0, 0, 0, 0] = np.nan, 1e10, np.inf
    wacc, wcount, launched = sr.welch_sums(flows.reshape(n, 2, H * W), L, hop, basis(L, "hann", "constant"))
    assert launched == (n - L) // hop + 1 and wcount.min() < launched and wcount.max() == launched
    f = torch.from_numpy(flows).to(dev)
    for batch in (1, 5, 40):
        ts = TemporalSpectrum(H, W, L, L - hop, device=dev)
        for at in range(0, n, batch):
            ts.update(f[at:at + batch])
        ts.update(f[:0])
        assert (ts.frames, ts.launched) == (n, launched)
        _compare((ts.acc.cpu().numpy(), ts.count.cpu().numpy()), (wacc, wcount), f"hop {hop}, batches of {batch}")
        res = ts.result()
        assert res.acc.shape == (L // 2 + 1, 4, H, W) and np.array_equal(res.segments.ravel(), wcount)


def test_guarded_buffers(dev):
    """X, basis, acc and count between guards, the padding columns of X NaN: every guard intact, no input written, the restatement's
    bits.  5 x 70 with 3 floats of padding: the second tile's lanes past vector 69 own nothing."""
    from pivlfn import _lib
    lib = _lib.load()
    L, N, K, first, pad = 5, 70, 3, 2, 3
    X, basis, acc0, count0 = _case(L, N, K, pad, 11)
    src = [torch.from_numpy(a).to(dev) for a in (X, basis, acc0, count0)]
    bufs = [guarded(t.shape, t.dtype, dev, "nan") for t in src]
    for t, x in zip(bufs, src):
        t.copy_(x)
    _lib.check(lib.pivlfn_spectrum_accumulate(_p(bufs[0]), L, first, N, X.shape[1], _p(bufs[1]), K, _p(bufs[2]), _p(bufs[3]),
                                              torch.cuda.current_stream(dev).cuda_stream), "spectrum_accumulate")
    torch.cuda.synchronize()
    _compare((bufs[2].cpu().numpy(), bufs[3].cpu().numpy()), sr.accumulate(X, first, N, basis, acc0, count0), "guarded 5x70")
    for t in bufs:
        check_guards(t, "spectrum_accumulate 5x70")
    for t, x in zip(bufs[:2], src[:2]):
        assert torch.equal(t.view(torch.uint8), x.view(torch.uint8)), "an input was written"


# ---- the stream and capture contract, with the helpers of tests/test_gpu_op_streams.py ------------------------------------------------
def _spec(seed, quad=False):
    """L = 12, N = 132 (three tiles), K = 9, a ring that wraps, from a non-zero acc and count (the same for every seed: the helpers
    reload them between the replays of two input sets)."""
    from pivlfn import _lib
    lib = _lib.load()
    L, N, K, first = 12, 132, 9, 7
    X, basis, _, _ = _case(L, N, K, 0, 3000 + seed)
    _, _, acc0, count0 = _case(L, N, K, 0, 3)

    def call(i, o, a, ws, st):
        return lib.pivlfn_spectrum_accumulate(_p(i[0]), L, first, N, 2 * N, _p(i[1]), K, _p(a[0]), _p(a[1]), st)

    def pin(accs):
        _compare((accs[0].cpu().numpy(), accs[1].cpu().numpy()), sr.accumulate(X, first, N, basis, acc0, count0), "the eager call")
    return Spec([torch.from_numpy(X), torch.from_numpy(basis)], [], [torch.from_numpy(acc0), torch.from_numpy(count0)], [], call, pin, (11, 12))


@pytest.fixture()
def as_an_op(monkeypatch):
    """The helpers of test_gpu_op_streams look an op up by name: "spectrum_accumulate" resolves to the spec above."""
    import test_gpu_op_streams as ops
    original = ops._get
    monkeypatch.setattr(ops, "_get", lambda op, seed, quad=False: _spec(seed, quad) if op == "spectrum_accumulate" else original(op, seed, quad))
    return ops


def test_eager_result_is_the_restatements(dev, as_an_op):
    _, _, accs, _ = as_an_op._eager("spectrum_accumulate", 31, dev)
    _spec(31).pin(accs)


def test_runs_in_order_on_the_stream_it_is_given(dev, delay, as_an_op):        # noqa: F811
    """On a side stream behind a long-running chain of matrix products and the copies of the real inputs into poisoned buffers,
    enqueued without a host synchronisation: the eager result, bit for bit, and every guard intact."""
    still_waiting, got, ref, buffers = _behind_the_delay("spectrum_accumulate", dev, delay, lambda stream: stream.cuda_stream)
    assert still_waiting, "the delay ran out before the op was enqueued: the test would not see a launch on another stream"
    for g, want in zip(got, ref):
        assert _same(g, want), "the result behind a delay on a side stream differs from the eager result"
    for t in buffers:
        _check(t, "spectrum_accumulate")


def test_is_graph_capturable(dev, as_an_op):
    as_an_op.test_op_is_graph_capturable("spectrum_accumulate", dev)


def test_pointers_one_element_off_give_the_same_bits(dev, as_an_op):
    as_an_op.test_pointers_one_element_off_give_the_same_bits("spectrum_accumulate", dev)


def test_every_error_is_refused_before_any_launch(dev):
    """The refusals of tests/test_spectrum.py with real device buffers: everything keeps every byte."""
    from pivlfn import _lib
    from test_spectrum import refusals
    lib = _lib.load()
    arena = _scribble(torch.empty(4 << 16, dtype=torch.uint8, device=dev))
    refusals(lib, *(arena.data_ptr() + (i << 16) for i in range(4)))
    torch.cuda.synchronize()
    assert bool((arena == 0xFF).all())


# ---- the Python class ------------------------------------------------------------------------------------------------------------------
def _lines(n):
    """[n, 2, 120] float32: the planted lines of tests/test_spectrum.py, one vector per (offset, phase), over n frames."""
    from test_spectrum import K0, L0, OFFSETS, PHASES
    return np.stack([sr.planted_line(L0, n, K0, d, phi)[:, :, 0] for d in OFFSETS for phi in PHASES], axis=2)


def _cpu_result(series, hop=32):
    from pivlfn.spectrum import TemporalSpectrumResult, basis
    acc, count, launched = sr.welch_sums(series, 64, hop, basis(64, "hann", "constant"))
    return TemporalSpectrumResult(acc.reshape(-1, 4, 1, series.shape[2]), count.reshape(1, -1), 64, overlap=64 - hop, frames=series.shape[0],
                                  launched=launched)


def test_temporal_spectrum_on_the_planted_line(dev):
    """128 frames of 9 x 13, every vector its own line 16 + d at its own phase, L = 64, three segments, in batches of 50; frame 40 of
    one vector masked: its segments are lower by the two that hold frame 40, nobody else's are, and the sums and the peak map are
    those of the restatement -- the CPU test's map, 16 + d within 1e-4 bin."""
    from pivlfn import TemporalSpectrum
    from test_spectrum import K0, L0, OFFSETS, PHASES
    n, H, W = 128, 9, 13
    series = _lines(n)[:, :, :H * W]
    flows = torch.from_numpy(series.reshape(n, 2, H, W)).to(dev)
    mask = torch.zeros(n, H, W, dtype=torch.uint8, device=dev)
    mask[40, 4, 6] = 1
    ts = TemporalSpectrum(H, W, L0, device=dev)
    for at in range(0, n, 50):
        ts.update(flows[at:at + 50], mask[at:at + 50])
    res = ts.result()
    holed = series.copy()
    holed[40, :, 4 * W + 6] = 1e10
    want = _cpu_result(holed)
    assert sr.same_bits(res.acc.reshape(want.acc.shape), want.acc)
    seg = np.full((H, W), 3.0)
    seg[4, 6] = 1.0
    assert np.array_equal(res.segments, seg) and (res.launched, res.frames) == (3, n)
    f = res.peak("uu")[0]
    assert np.array_equal(f.ravel(), want.peak("uu")[0].ravel())
    line = (K0 + np.repeat(OFFSETS, len(PHASES))[:H * W]) / L0
    assert np.abs(f.ravel() - line).max() * L0 <= 1e-4
    s = res.summary()
    assert abs(s["peak_frequency"] * L0 - K0) < 1.0 and s["segments"] == 3 and s["frames_left_over"] == 0 and s["valid_vectors"] == H * W


def test_temporal_spectrum_on_cell_means(dev):
    """cell = 4 on 9 x 13: 3 x 4 cells of 16, 4 and 1 vectors (sums and means of equal float32 values over a power of two are exact), every
    cell one line; the mask takes the whole corner cell out of frame 70: its segments drop by the two that hold it."""
    from pivlfn import TemporalSpectrum
    n, H, W, cell = 128, 9, 13, 4
    series = _lines(n)[:, :, 5:17]
    cells = (np.arange(H)[:, None] // cell) * 4 + np.arange(W)[None, :] // cell
    flows = torch.from_numpy(np.ascontiguousarray(series[:, :, cells])).to(dev)
    mask = torch.zeros(n, H, W, dtype=torch.bool, device=dev)
    mask[70, 8, 12] = True
    ts = TemporalSpectrum(H, W, 64, cell=cell, device=dev)
    ts.update(flows, mask)
    res = ts.result()
    holed = series.copy()
    holed[70, :, 11] = 1e10
    want = _cpu_result(holed)
    assert res.acc.shape == (33, 4, 3, 4) and sr.same_bits(res.acc.reshape(want.acc.shape), want.acc)
    assert res.segments.ravel().tolist() == [3.0] * 11 + [1.0]
    assert np.array_equal(res.peak()[0].ravel(), want.peak()[0].ravel())


def test_temporal_spectrum_checks(dev):
    from pivlfn import TemporalSpectrum
    ts = TemporalSpectrum(8, 9, 8, device=dev)
    with pytest.raises(ValueError, match="shape"):
        ts.update(torch.zeros(1, 2, 9, 8, device=dev))
    with pytest.raises(ValueError, match="flows on cpu"):
        ts.update(torch.zeros(1, 2, 8, 9))
    with pytest.raises(TypeError):
        ts.update(torch.zeros(1, 2, 8, 9, device=dev, dtype=torch.float64))
    assert ts.frames == 0 and ts.launched == 0 and not bool(ts.count.any())
    assert TemporalSpectrum.device_bytes(8, 9, 8) == 8 * 144 * 4 + 5 * 4 * 72 * 8 + 72 * 4 + 5 * 2 * 8 * 8


# ---- run.py --------------------------------------------------------------------------------------------------------------------------
def test_run_py_spectrum(tmp_path, dev, capsys):
    """run.py --spectrum 8 --spectrum-image on 17 synthetic 64 x 64 frames whose particles swing along x with a period of four frames
    (bin 2 of 8), --batch 5: spectrum.npz holds the sums of a TemporalSpectrum fed the written flows, bit for bit, spectrum.json the
    parameters and summary() with the peak within one bin of the planted one, spectrum_peak.png the map; refused with -p, -b and too
    few pairs."""
    import PIL.Image
    import run as runpy
    from pivlfn import ParticleImageGen, TemporalSpectrum
    from pivlfn.flo import read_flow
    from pivlfn.spectrum import TemporalSpectrumResult
    H = W = 64
    seq = tmp_path / "seq"
    seq.mkdir()
    gen = ParticleImageGen(density=0.05, seed=5, device=dev)
    x, y, z, d = gen.random_particle(H, W, pad=8)
    names = [f"f{k:03d}" for k in range(17)]
    for k, name in enumerate(names):
        frame = gen.generate_image(x + 1.5 * np.sin(2 * np.pi * 2 * k / 8), y, z, d, H, W)
        PIL.Image.fromarray(frame.cpu().numpy()).save(str(seq / f"{name}.png"))
    base = ["--model", "piv", "-i", str(seq), "--batch", "5"]
    assert runpy.main(base + ["-o", str(tmp_path / "out"), "--spectrum", "8", "--spectrum-image"]) == 16
    assert "pooled peak at" in capsys.readouterr().out
    out = tmp_path / "out" / "piv-synthetic" / "seq"
    lines = list(open(out / "args.txt"))
    assert "spectrum: 8\n" in lines and "spectrum_image: True\n" in lines
    flows = torch.stack([torch.from_numpy(read_flow(str(out / "flow" / f"{n}_out.flo"))).permute(2, 0, 1) for n in names[:16]]).contiguous().to(dev)
    ts = TemporalSpectrum(H, W, 8, device=dev)
    ts.update(flows)
    got = TemporalSpectrumResult.load(str(out / "spectrum.npz"))
    assert sr.same_bits(got.acc, ts.result().acc) and np.array_equal(got.segments, np.full((H, W), 3.0))
    assert (got.L, got.overlap, got.frames, got.launched, got.window, got.detrend) == (8, 4, 16, 3, "hann", "constant")
    doc = json.load(open(out / "spectrum.json"))
    assert (doc["segment"], doc["overlap"], doc["cell"], doc["fps"], doc["validation"]) == (8, 4, 1, 1.0, None)
    assert doc["summary"] == runpy.json_strict(ts.result().summary())
    print(f"run.py --spectrum: pooled peak at {doc['summary']['peak_frequency'] * 8:.3f} bins, planted 2")
    assert abs(doc["summary"]["peak_frequency"] * 8 - 2.0) <= 1.0 and doc["summary"]["segments"] == 3
    im = PIL.Image.open(out / "spectrum_peak.png")
    assert im.mode == "RGB" and im.size == (W, H)
    for extra, word in ((["-p"], "not a time series"), (["-b", "0.5"], "-b/-c"), (["--spectrum-overlap", "8"], "overlap=8")):
        with pytest.raises(SystemExit, match=word):
            runpy.main(base + ["-o", str(tmp_path / "refused"), "--spectrum", "8"] + extra)
    with pytest.raises(SystemExit, match="has 16 pairs, fewer than the 32"):
        runpy.main(base + ["-o", str(tmp_path / "refused"), "--spectrum", "32"])
    os.environ["WORLD_SIZE"] = "2"
    try:
        with pytest.raises(SystemExit, match="--spectrum needs a single process"):
            runpy.main(base + ["-o", str(tmp_path / "refused"), "--spectrum", "8"])
    finally:
        del os.environ["WORLD_SIZE"]
    assert not list((tmp_path / "refused").rglob("spectrum*"))
