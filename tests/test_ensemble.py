"""CPU: ensemble correlation without a GPU -- the NumPy restatement of pivlfn_ensemble_corr (tests/ensemble_restatement.py) against the
correlation coefficient from its definition, pivlfn.ensemble's host code (finalize, predictor_offsets, the OUTSIDE rule, save / load,
the refusals) on hand-made planes, and the accuracy of the method on rendered particle images.

Accuracy bounds: the asserted bound of each case is twice the largest error the restatement itself gave on these inputs when the
test was written (MEASURED below; DESIGN 4.23 quotes them) -- the rule DESIGN 4.19 uses for its accuracy table.  tests/
test_gpu_ensemble.py holds the device to the same sums bit for bit, so the same figures hold there.

The third case of the issue (72 x 88, window 32, step 16, search 2, offset (6, 3)) cannot have "no window flagged": by the contract's
own OUTSIDE rule the search region of its last window column ends at x = 50 + 6 + 2 + 32 = 90 > 88.  Those three windows must be
flagged OUTSIDE and nothing else; every other window of the case must be unflagged and meet the bound and the ratio."""
import ctypes
import os

import numpy as np
import pytest

import ensemble_restatement as er
from pivlfn import ensemble as E

MEASURED = (0.01599, 0.01416, 0.01820)          # px, the largest |error| of the restatement's result per accuracy case
K = 10 ** 6


def _sums_of(planes, flat_a=()):
    """Integer sums whose finalize() gives the correlation planes `planes` [ny,nx,P,P] (NaN: a flat entry) at window 8, one frame:
    sum A = sum B = 0, sum A^2 = sum B^2 = K, sum A*B = rint(c K), so corr = rint(c K) / K.  Windows in `flat_a` get sum A^2 = 0."""
    planes = np.asarray(planes, np.float64)
    ny, nx, P, _ = planes.shape
    sums, sums_a = np.zeros((ny, nx, P, P, 3), np.int64), np.zeros((ny, nx, 2), np.int64)
    sums_a[..., 1] = K
    for j, i in flat_a:
        sums_a[j, i, 1] = 0
    sums[..., 1] = np.where(np.isnan(planes), 0, K)
    sums[..., 2] = np.rint(np.where(np.isnan(planes), 0.0, planes) * K).astype(np.int64)
    return sums, sums_a


def _gauss(P, x0, y0, height=0.8, width=1.3):
    y, x = np.mgrid[0:P, 0:P].astype(np.float64)
    return height * np.exp(-((x - x0) ** 2 + (y - y0) ** 2) / width ** 2)


def test_zero_displacement_entry_is_the_correlation_coefficient():
    rng = np.random.default_rng(1)
    a, b = rng.integers(0, 256, (2, 3, 30, 34), dtype=np.uint8)
    window, step, search = 12, 5, 3
    sums, sums_a = er.ensemble_corr(a, b, window, step, search)
    res = E.finalize(sums, sums_a, 3, window, step)
    ny, nx = er.grid(30, 34, window, step, search)
    assert (res.ny, res.nx, res.P) == (ny, nx, 7) == (3, 4, 7)
    for j in range(ny):
        for i in range(nx):
            y, x = search + j * step, search + i * step
            wa = a[:, y:y + window, x:x + window].astype(np.float64).ravel()
            wb = b[:, y:y + window, x:x + window].astype(np.float64).ravel()
            da, db = wa - wa.mean(), wb - wb.mean()
            want = (da * db).sum() / np.sqrt((da * da).sum() * (db * db).sum())
            assert abs(res.corr[j, i, search, search] - want) <= 1e-12


def test_restated_sums_shift_with_the_images():
    """b = a moved by (dx, dy) = (2, -1): the entry at that displacement has sum A*B = sum A^2 and sum B = sum A, and a frame adds the
    same integers alone and in a batch."""
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (2, 26, 29), dtype=np.uint8)
    b = np.roll(a, (-1, 2), axis=(1, 2))
    sums, sums_a = er.ensemble_corr(a, b, 8, 3, 3)
    assert np.array_equal(sums[:, :, 3 - 1, 3 + 2, 2], sums_a[..., 1]) and np.array_equal(sums[:, :, 2, 5, 0], sums_a[..., 0])
    one, one_a = er.ensemble_corr(a[:1], b[:1], 8, 3, 3)
    two, two_a = er.ensemble_corr(a[1:], b[1:], 8, 3, 3, sums=one, sums_a=one_a)
    assert np.array_equal(two, sums) and np.array_equal(two_a, sums_a)


def test_finalize_reads_a_gaussian_peak():
    plane = _gauss(7, 3.3, 2.8)
    res = E.finalize(*_sums_of(plane[None, None]), 1, 8, 4, offset=np.array([[[5]], [[-2]]]))
    assert res.flag[0, 0] == 0 and tuple(res.peak[:, 0, 0]) == (3, 3)
    assert np.allclose(res.displacement[:, 0, 0], (5 + 0.3, -2 - 0.2), atol=1e-5, rtol=0)
    assert res.height[0, 0] == plane[3, 3].round(6) and res.ratio[0, 0] == np.inf          # one local maximum only
    x, y = res.centres()
    assert x.tolist() == [3 + 3.5] and y.tolist() == [3 + 3.5]


def test_finalize_on_hand_made_planes():
    P = 5
    tie = np.full((P, P), 0.1)
    tie[1, 3] = tie[3, 1] = 0.7                                         # two equal maxima: the first in row-major order
    tie[1, 2], tie[1, 4], tie[0, 3], tie[2, 3] = 0.3, 0.2, 0.25, 0.35
    rim = _gauss(P, 4.0, 2.0)                                           # the peak on the right rim
    negative = _gauss(P, 2.0, 2.0)
    negative[2, 1] = -0.05                                              # a neighbour of the peak below zero
    two = _gauss(P, 1.0, 1.0) + 0.5 * _gauss(P, 3.0, 3.0, width=0.7)    # a second local maximum of half the height
    holes = _gauss(P, 2.2, 2.1)
    holes[0, :] = np.nan                                                # flat entries away from the peak
    planes = np.stack([tie, rim, negative, two, holes, _gauss(P, 2, 2), np.full((P, P), np.nan)])[None]
    res = E.finalize(*_sums_of(planes, flat_a=[(0, 5)]), 1, 8, 4)
    assert res.flag[0].tolist() == [0, E.EDGE, E.NO_PEAK, 0, 0, E.FLAT, E.FLAT]
    assert tuple(res.peak[:, 0, 0]) == (3, 1) and res.ratio[0, 0] == 1.0
    assert tuple(res.peak[:, 0, 1]) == (4, 2) and np.isnan(res.displacement[:, 0, 1]).all() and res.height[0, 1] == 0.8
    assert np.isnan(res.displacement[:, 0, 2]).all() and res.height[0, 2] == 0.8
    second = planes[0, 3, 3, 3].round(6)
    assert res.ratio[0, 3] == planes[0, 3, 1, 1].round(6) / second and 1.9 < res.ratio[0, 3] < 2.0
    assert res.flag[0, 4] == 0 and np.isnan(res.corr[0, 4, 0]).all() and np.allclose(res.displacement[:, 0, 4], (0.2, 0.1), atol=1e-5)
    assert np.isnan(res.height[0, 5:]).all() and np.isnan(res.corr[0, 6]).all()
    doc = res.summary()
    assert (doc["windows"], doc["valid"], doc["flat"], doc["edge"], doc["no_peak"], doc["outside"]) == (7, 3, 2, 1, 1, 0)
    assert doc["median_height"] == 0.8


def test_finalize_marks_outside_windows_and_no_frames():
    planes = np.stack([_gauss(5, 2, 2)] * 3)[None]
    offset = np.array([[[0, 9, 0]], [[0, 0, -3]]])
    res = E.finalize(*_sums_of(planes), 1, 8, 4, offset=offset, H=12, W=20)                 # the grid of 12 x 20: one row of three
    assert res.outside.tolist() == [[False, True, True]] and res.flag.tolist() == [[0, E.OUTSIDE, E.OUTSIDE]]
    assert np.isnan(res.corr[0, 1:]).all() and np.isnan(res.height[0, 1:]).all()
    empty = E.finalize(np.zeros((1, 1, 3, 3, 3), np.int64), np.zeros((1, 1, 2), np.int64), 0, 8, 4)
    assert empty.flag.tolist() == [[E.FLAT]]


def test_outside_rule_is_the_restatements():
    rng = np.random.default_rng(3)
    H, W, window, step, search = 37, 53, 12, 5, 3
    ny, nx = er.grid(H, W, window, step, search)
    offset = rng.integers(-5, 6, (2, ny, nx)).astype(np.int32)
    want = er.outside(H, W, window, step, search, offset)
    assert np.array_equal(E.outside_windows(H, W, window, step, search, offset), want) and want.any() and not want.all()
    assert E.grid(H, W, window, step, search) == (ny, nx) and not E.outside_windows(H, W, window, step, search).any()


def test_predictor_offsets_round_half_to_even():
    H, W, window, step, search = 40, 44, 16, 8, 2
    ny, nx = er.grid(H, W, window, step, search)
    mean = np.empty((2, H, W))
    mean[0], mean[1] = 2.5, -1.5
    off = E.predictor_offsets(mean, window, step, search)
    assert off.dtype == np.int32 and off.shape == (2, ny, nx) and (off[0] == 2).all() and (off[1] == -2).all()
    mean[0], mean[1] = 3.5, 0.5
    mean[0, 2 + 8, 2 + 8] = np.nan                                       # inside the footprints of windows (0..1, 0..1) only
    off = E.predictor_offsets(mean, window, step, search)
    assert (off[1] == 0).all() and (off[0, :2, :2] == 0).all() and (off[0, 2:] == 4).all() and (off[0, :, 2:] == 4).all()
    ramp = np.stack([np.broadcast_to(np.arange(W, dtype=np.float64), (H, W)), np.zeros((H, W))])
    assert E.predictor_offsets(ramp, window, step, search)[0, 0].tolist() == [10, 18, 26, 34]       # 2 + 7.5 = 9.5 -> 10, 17.5 -> 18, ...
    import torch
    assert np.array_equal(E.predictor_offsets(torch.from_numpy(ramp), window, step, search), E.predictor_offsets(ramp, window, step, search))


def test_compare_takes_the_window_mean():
    plane = _gauss(7, 3.3, 2.8)
    res = E.finalize(*_sums_of(np.stack([plane, _gauss(7, 6.0, 3.0)])[None]), 1, 8, 4)       # windows at x = 3 and 7; the second: EDGE
    mean = np.zeros((2, 14, 18))
    mean[0], mean[1] = 0.1, -0.3
    doc = res.compare(mean)
    assert doc["windows"] == 1 and np.isnan(doc["difference"][:, 0, 1]).all()
    assert abs(doc["bias_u"] - 0.2) < 1e-5 and abs(doc["bias_v"] - 0.1) < 1e-5 and abs(doc["rms"] - np.hypot(0.2, 0.1)) < 1e-5
    with pytest.raises(ValueError):
        res.compare(np.zeros((2, 30, 30)))


def test_save_and_load(tmp_path):
    a, b, offset, sums, sums_a = er.accuracy_case(2)
    n, _, window, step, search, _ = er.ACCURACY[2]
    res = E.finalize(sums, sums_a, n, window, step, offset, floor=2.0, H=er.ACC_H, W=er.ACC_W)
    path = res.save(os.path.join(str(tmp_path), "ensemble"))
    assert path.endswith("ensemble.npz")
    with np.load(path) as f:
        assert f["sums"].dtype == np.int64 and np.array_equal(f["sums"], sums) and np.array_equal(f["sums_a"], sums_a)
        assert [int(f[k]) for k in ("H", "W", "window", "step", "search", "frames")] == [er.ACC_H, er.ACC_W, window, step, search, n]
        assert float(f["floor"]) == 2.0 and np.array_equal(f["offset"], offset)
    back = E.EnsembleResult.load(path)
    for k in ("displacement", "height", "ratio", "flag", "corr", "outside"):
        assert np.array_equal(getattr(back, k), getattr(res, k), equal_nan=True), k
    assert (back.frames, back.window, back.step, back.search, back.floor, back.H, back.W) == (n, window, step, search, 2.0, er.ACC_H, er.ACC_W)


def test_refusals():
    for bad in (dict(window=30), dict(window=4), dict(window=132), dict(window=32.0), dict(search=0), dict(search=33), dict(step=0),
                dict(floor=-1.0), dict(floor=float("nan"))):
        with pytest.raises(ValueError, match="EnsembleCorrelation: " + next(iter(bad))):
            E.check_params(**{**dict(window=32, step=16, search=8), **bad})
        with pytest.raises(ValueError, match="EnsembleCorrelation: " + next(iter(bad))):
            E.EnsembleCorrelation(64, 64, **bad)
    with pytest.raises(ValueError, match=r"EnsembleCorrelation: bad size 47 x 64 \(positive, at least window \+ 2\*search = 48"):
        E.EnsembleCorrelation(47, 64)
    with pytest.raises(ValueError, match="EnsembleCorrelation: bad size 64 x 0"):
        E.EnsembleCorrelation(64, 0)
    with pytest.raises(NotImplementedError, match="EnsembleCorrelation: GPU devices only"):
        E.EnsembleCorrelation(64, 64, device="cpu")
    with pytest.raises(ValueError, match=r"offset \(2, 1, 1\), expected \[2,2,2\]"):
        E.check_offset(np.zeros((2, 1, 1), np.int32), 2, 2)
    with pytest.raises(TypeError, match="offset must hold integers"):
        E.check_offset(np.zeros((2, 2, 2)), 2, 2)
    with pytest.raises(ValueError, match="expected int64 sums"):
        E.finalize(np.zeros((1, 1, 3, 3, 3)), np.zeros((1, 1, 2), np.int64), 1, 8, 4)
    import torch
    with pytest.raises(TypeError, match="expected a uint8"):
        E._as_bytes(torch.zeros(1, 8, 8, dtype=torch.float64), "a", "EnsembleCorrelation.update")
    with pytest.raises(NotImplementedError, match="GPU tensors only"):
        E._as_bytes(torch.zeros(1, 8, 8), "a", "EnsembleCorrelation.update")


@pytest.mark.parametrize("C", [0, 1, 3])
def test_float_frames_give_back_the_bytes_of_the_table(C):
    """The conversion update() applies to float32 frames, on host tensors: the pipeline's table k/255 gives back k for all 256 values,
    as [B,H,W], [B,1,H,W] and [B,3,H,W]; values outside [0, 1] are clamped, .5 goes to even."""
    import torch
    k = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16)
    f = (torch.arange(256, dtype=torch.float32) / 255.0)[k.long()]
    f = f if C == 0 else f[:, None].expand(-1, C, -1, -1)
    assert torch.equal(E._as_bytes(f, "a", "test", gpu_only=False), k)
    assert E._as_bytes(torch.tensor([[[-0.3, 1.7, 0.5, 2.5 / 255]]]), "a", "test", gpu_only=False).tolist() == [[[0, 255, 128, 2]]]
    assert E._as_bytes(k, "a", "test", gpu_only=False).data_ptr() == k.data_ptr()              # bytes are taken as they are


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    """Every PIVLFN_ERR_ARG case is answered on the host before anything is launched: pointers that are never dereferenced."""
    import pivlfn
    from pivlfn import _lib
    lib = _lib.load()
    assert "pivlfn_ensemble_corr" in _lib.SIGNATURES and hasattr(lib, "pivlfn_ensemble_corr")
    for name in ("EnsembleCorrelation", "EnsembleResult", "predictor_offsets"):
        assert getattr(pivlfn, name) is getattr(E, name) and name in pivlfn.__all__
    a, b, off, sums, sums_a = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20
    cases = er.err_arg_cases(a, b, off, sums, sums_a, 2, 37, 53, 12, 5, 3)
    assert len(cases) == 22
    for label, args, word in cases:
        rc = lib.pivlfn_ensemble_corr(*args, None)
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1 and msg.startswith("ensemble_corr: ") and word in msg, (label, rc, msg)
    assert lib.pivlfn_ensemble_corr(a, b, off, sums, sums_a, 0, 37, 53, 12, 5, 3, None) == 0          # B = 0: success, no launch
    assert lib.pivlfn_ensemble_corr(a, a, None, sums, sums_a, 0, 37, 53, 12, 5, 3, None) == 0          # a == b and no offset are fine
    assert ctypes.sizeof(ctypes.c_longlong) == 8


@pytest.mark.parametrize("k", range(3))
def test_accuracy_on_rendered_particles(k):
    n, uv, window, step, search, off = er.ACCURACY[k]
    a, b, offset, sums, sums_a = er.accuracy_case(k)
    res = E.finalize(sums, sums_a, n, window, step, offset, H=er.ACC_H, W=er.ACC_W)
    outside = er.outside(er.ACC_H, er.ACC_W, window, step, search, offset)
    err = np.abs(res.displacement - np.array(uv)[:, None, None]).max(0)
    print(f"case {k}: {res.ny} x {res.nx} windows, {int(outside.sum())} outside, largest error {np.nanmax(err):.5f} px, "
          f"smallest ratio {res.ratio[~outside].min():.2f}, smallest height {res.height[~outside].min():.3f}")
    assert np.array_equal(res.flag, np.where(outside, E.OUTSIDE, 0))          # nothing flagged but what the OUTSIDE rule itself excludes
    assert outside.sum() == (3 if k == 2 else 0)
    assert (res.ratio[~outside] >= 4.0).all()
    assert (err[~outside] <= 2.0 * MEASURED[k]).all()
    assert abs(np.nanmax(err) - MEASURED[k]) < 1e-5                          # the figure the bound was derived from still holds
