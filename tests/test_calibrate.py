"""CPU: the NumPy restatement of the stereo-calibration contracts (tests/calibrate_restatement.py) against the definitions it restates,
and the host steps of pivlfn.calibrate (gen_template, index_lattice, fit_mapping, write_coeff) on rendered targets with known truth.

Accuracy.  Four binary renderings of a cross lattice seen through a mild homography (calibrate_restatement.TARGETS).  Conditions:
every marker kept by the border rule is indexed, and with its true index; every true node at least half a template + 2 px inside the
image is found.  Bounds: a binary rendering's pixelisation error moves with the sub-pixel phase of the lattice, so each bound is twice
the maximum measured with the restatement on that target (MEASURED below: markers, centre RMS, centre max, reprojection max, px)."""
import numpy as np
import pytest
import torch

import calibrate_restatement as cr
from pivlfn import calibrate as cal
from pivlfn.stereo import read_coeff

# name: (kept markers, centre error RMS, centre error max, reprojection error max) measured with the restatement; fit residual RMS
# 0.080, 0.162, 0.101, 0.222 px
MEASURED = {"96": (16, 0.261, 0.480, 0.478), "256": (36, 0.195, 0.371, 0.303), "192x320": (24, 0.149, 0.330, 0.314),
            "512": (149, 0.228, 0.500, 0.291)}


# ---- template matching ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,th,tw", [(1, 1, 5, 5), (7, 9, 3, 5), (20, 33, 7, 5), (16, 16, 25, 25)])
def test_restated_match_is_the_definition(H, W, th, tw):
    rng = np.random.default_rng(H * W + th)
    image = rng.integers(0, 256, (H, W), dtype=np.uint8)
    templ = rng.integers(0, 256, (th, tw), dtype=np.uint8)
    got = cr.template_match(image, templ)[0]
    assert got.dtype == np.float32 and np.abs(got - cr.ccoeff_normed_direct(image, templ)).max() <= 1e-6


def test_match_is_one_where_the_image_holds_the_template_and_zero_on_flat_windows():
    templ = cal.gen_template(3, 9, 11)
    image = np.zeros((40, 50), np.uint8)
    image[12:21, 20:31] = templ
    r = cr.template_match(image, templ)[0]
    assert r[16, 25] == np.float32(1.0) and (r < 1).sum() == r.size - 1
    assert r[35, 5] == 0 and r[39, 49] == 0                                    # all-zero windows
    flat = cr.template_match(np.full((12, 12), 255, np.uint8), templ)[0]
    assert np.all(flat[4:8, 5:7] == 0)                                         # all-255 windows inside; the padded border is not flat
    assert np.all(cr.template_match(image, np.full((3, 3), 9, np.uint8)) == 0)  # a flat template


def test_gen_template_is_the_reference_cross_and_rejects_even_thickness():
    t = cal.gen_template(11, 25, 25)
    assert t.shape == (25, 25) and t.dtype == np.uint8 and set(np.unique(t)) == {0, 255}
    assert np.all(t[7:18] == 255) and np.all(t[:, 7:18] == 255) and np.all(t[:7, :7] == 0) and np.all(t[18:, 18:] == 0)
    assert np.array_equal(t, t.T) and np.array_equal(t, t[::-1, ::-1])
    for TC in (2, 4, 0):
        with pytest.raises(ValueError):
            cal.gen_template(TC, 25, 25)


# ---- marker centres --------------------------------------------------------------------------------------------------------------------------
def test_restated_centres_are_the_references_minus_half_a_pixel():
    """center_of_mass of the blurred thresholded map (stereo/matching.py:49-75) = the integer records' quotient; ours subtracts 0.5."""
    from scipy import ndimage
    image, templ, _, _, _ = cr.target("96")
    r = cr.template_match(image, templ)[0]
    res = r * (r > np.float32(0.7))
    ys = [1] + list(range(r.shape[0] - 1))
    xs = [1] + list(range(r.shape[1] - 1))
    blur = (res[ys][:, xs].astype(np.float64) + res[ys] + res[:, xs] + res) / 4.0     # cv2.blur (2, 2), default anchor, REFLECT_101
    lbl, n = ndimage.label(blur)
    ref = np.fliplr(np.array(ndimage.center_of_mass(blur, lbl, list(range(1, n + 1)))))
    pts, recs = cr.find_markers(image, templ, border=False)
    assert len(pts) == n and np.abs(pts + 0.5 - ref).max() < 1e-4 and np.all(recs[:, 3] >= 1)


@pytest.fixture(scope="module", params=list(cr.TARGETS))
def solved(request):
    image, templ, centres, index, ref4 = cr.target(request.param)
    return request.param, image, templ, centres, index, cr.calibrate_camera(image, templ, ref4)


def test_every_kept_marker_is_indexed_with_its_true_index(solved):
    name, image, templ, centres, index, res = solved
    pts, ij = res["markers"], res["ij"]
    d = np.linalg.norm(pts[:, None] - centres[None], axis=2)
    near = d.argmin(axis=1)
    assert len(pts) == MEASURED[name][0] and res["indexed"].all() and len(set(near.tolist())) == len(pts)
    assert np.array_equal(ij, index[near])
    must = cal.keep_inside(centres, image.shape[0], image.shape[1], templ.shape[0] + 4, templ.shape[1] + 4)
    assert must.sum() >= 16 and all(np.linalg.norm(pts - c, axis=1).min() < 1.0 for c in centres[must])


def test_centres_and_reprojection_stay_within_twice_the_measured_error(solved):
    name, image, templ, centres, index, res = solved
    pts, ij = res["markers"], res["ij"]
    d = np.linalg.norm(pts[:, None] - centres[None], axis=2)
    near = d.argmin(axis=1)
    err = d[np.arange(len(pts)), near]
    fx, fy = cal.nl_trans(*cal.lattice_targets(ij, res["spacing"]).T, res["A"])
    rep = np.hypot(fx + res["origin"][0] - centres[near, 0], fy + res["origin"][1] - centres[near, 1])
    print(f"{name}: centre rms {np.sqrt((err ** 2).mean()):.3f} max {err.max():.3f}  fit rms {res['rms']:.3f} max {res['max']:.3f}  "
          f"reprojection max {rep.max():.3f}")
    _, rms, worst, rep_worst = MEASURED[name]
    assert err.max() <= 2 * worst and np.sqrt((err ** 2).mean()) <= 2 * rms and rep.max() <= 2 * rep_worst


def test_index_lattice_does_not_cross_a_gap_wrongly_and_takes_marker_numbers():
    """A regular lattice with a missing node and an isolated stray point: everything connected is indexed, the stray point is not."""
    ii, jj = np.meshgrid(np.arange(-2, 4), np.arange(-1, 3), indexing="xy")
    idx = np.stack([ii.ravel(), jj.ravel()], axis=1)
    idx = idx[~((idx == (2, 1)).all(axis=1))]
    pts = np.stack([100.0 + 30.0 * idx[:, 0] + 1.5 * idx[:, 1], 80.0 + 31.0 * idx[:, 1] - 0.5 * idx[:, 0]], axis=1)
    pts = np.concatenate([pts, [[400.0, 300.0]]])
    sel = [int(np.flatnonzero((idx == c).all(axis=1))[0]) for c in ((0, 0), (1, 0), (1, 1), (0, 1))]
    ij, got_sel, (cx, cy) = cal.index_lattice(pts, sel)
    assert np.array_equal(ij[:-1], idx) and ij[-1, 0] == cal.NOT_INDEXED and got_sel.tolist() == sel
    assert cx == pytest.approx(30.0) and cy == pytest.approx(31.0)
    ij2, _, _ = cal.index_lattice(pts, pts[sel] + 3.0)                           # clicks a few pixels off snap to the same markers
    assert np.array_equal(ij2, ij)
    with pytest.raises(ValueError):
        cal.index_lattice(pts, [pts[sel[0]]] * 4)


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------------
def test_fit_mapping_recovers_a_known_first_order_mapping():
    A = np.zeros(24)
    A[0:3], A[6:9] = (1.02, -0.03, 0.4), (2e-4, -1e-4, 1.0)
    A[12:15], A[18:21] = (0.05, 0.97, -0.7), (-3e-4, 1.5e-4, 1.0)
    ii, jj = np.meshgrid(np.arange(-3, 4), np.arange(-2, 3))
    new = np.stack([40.0 * ii.ravel(), 40.0 * jj.ravel()], axis=1).astype(np.float64)
    old = np.stack(cal.nl_trans(new[:, 0], new[:, 1], A), axis=1)
    for order in (1, 2):
        got, rms, worst = cal.fit_mapping(new, old, order=order)
        assert worst < 1e-9 and rms <= worst
        fx, fy = cal.nl_trans(new[:, 0], new[:, 1], got)
        assert np.abs(fx - old[:, 0]).max() < 1e-9 and np.abs(fy - old[:, 1]).max() < 1e-9
        if order == 1:
            nz = A != 0
            assert np.all(np.abs(got[nz] - A[nz]) <= 1e-9 * np.abs(A[nz])) and np.all(got[~nz] == 0)     # each coefficient, 1e-4 .. 1
    again, _, _ = cal.fit_mapping(new, old, order=2)
    assert cr.same_bits(again, got)                                               # deterministic
    assert got[8] == 1.0 and got[20] == 1.0


def test_fit_mapping_raises_on_too_few_points():
    pts = np.random.default_rng(0).uniform(-50, 50, (10, 2))
    with pytest.raises(ValueError, match="11 unknowns"):
        cal.fit_mapping(pts, pts, order=2)
    with pytest.raises(ValueError, match="5 unknowns"):
        cal.fit_mapping(pts[:4], pts[:4], order=1)
    cal.fit_mapping(pts[:5], pts[:5], order=1)
    with pytest.raises(ValueError):
        cal.fit_mapping(pts, pts, order=3)


def test_write_coeff_reads_back_through_read_coeff(tmp_path):
    rng = np.random.default_rng(5)
    left, right = rng.standard_normal(24), rng.standard_normal(24) * 1e-5
    path = str(tmp_path / "sub" / "cal.json")
    wrote = cal.write_coeff(path, left, right, 39.25)
    got = read_coeff(path)
    assert got == wrote and got["Left"] == left.tolist() and got["Right"] == right.tolist() and got["calib"] == 39.25
    with pytest.raises(ValueError):
        cal.write_coeff(path, left[:23], right, 1.0)
    with pytest.raises(ValueError):
        cal.write_coeff(path, left, right, 0.0)


# ---- dewarp ------------------------------------------------------------------------------------------------------------------------------------
IDENTITY = np.array([1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0], dtype=np.float64)


def test_restated_dewarp_identity_returns_the_image():
    rng = np.random.default_rng(3)
    u8 = rng.integers(0, 256, (2, 9, 13), dtype=np.uint8)
    f32 = rng.standard_normal((2, 9, 13)).astype(np.float32)
    for frames in (u8, f32):
        assert cr.same_bits(cr.dewarp(frames, IDENTITY, (4.25, 3.5), "nearest", 7), frames)
        got = cr.dewarp(frames, IDENTITY, (4.0, 3.0), "bilinear", 7)
        assert cr.same_bits(got[:, :-1, :-1], frames[:, :-1, :-1]) and np.all(got[:, -1] == 7) and np.all(got[:, :, -1] == 7)


def test_restated_dewarp_is_the_references_warp_on_a_square_image_with_sources_inside():
    rng = np.random.default_rng(4)
    image = rng.integers(0, 256, (48, 48), dtype=np.uint8)
    A = IDENTITY.copy()
    A[[0, 1, 3, 5, 6, 7]] = (0.9, 0.03, 2e-4, -1e-4, 3e-4, -2e-4)
    A[[12, 13, 16, 18, 19]] = (-0.02, 0.92, 1e-4, 1e-4, 2e-4)
    origin = (23.4, 24.7)
    sx, sy = cr.source_positions(48, 48, A, origin)
    assert np.round(sx).min() >= 0 and np.round(sx).max() <= 47 and np.round(sy).min() >= 0 and np.round(sy).max() <= 47
    assert np.abs(sx - np.arange(48)[None]).max() > 1.5                              # not the identity
    assert cr.same_bits(cr.dewarp(image, A, origin)[0], cr.reference_warp_square(image, origin, A))


def test_cpu_tensors_are_refused():
    for fn in (lambda: cal.template_match(torch.zeros(4, 4, dtype=torch.uint8), cal.gen_template(1, 3, 3)),
               lambda: cal.find_markers(torch.zeros(4, 4, dtype=torch.uint8), cal.gen_template(1, 3, 3)),
               lambda: cal.target_points(torch.zeros(4, 4)),
               lambda: cal.dewarp_frames(torch.zeros(4, 4), IDENTITY, (0, 0)),
               lambda: cal.calibrate_camera(torch.zeros(4, 4, dtype=torch.uint8), cal.gen_template(1, 3, 3), [0, 1, 2, 3])):
        with pytest.raises(NotImplementedError):
            fn()


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    import ctypes
    from pivlfn import _lib
    lib = _lib.load()
    P = 4096
    A = (ctypes.c_double * 24)(*IDENTITY.tolist())

    def refused(rc, *words):
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    assert lib.pivlfn_template_match_workspace_bytes(25, 25) >= (25 * 7 + 2) * 4 and lib.pivlfn_template_match_workspace_bytes(255, 257) == 0
    refused(lib.pivlfn_template_match(None, P, P, 1, 8, 8, 5, 5, P, 1 << 20, None), "template_match", "null")
    refused(lib.pivlfn_template_match(P, P, P, 1, 8, 8, 4, 5, P, 1 << 20, None), "odd")
    refused(lib.pivlfn_template_match(P, P, P, 1, 8, 8, 257, 255, P, 1 << 20, None), "65025")
    refused(lib.pivlfn_template_match(P, P, P, 1, 8, 8, 2001, 31, P, 1 << 20, None), "160 KiB")
    refused(lib.pivlfn_template_match(P, P, P, 1, 8, 8, 5, 5, P, 8, None), "workspace")
    refused(lib.pivlfn_template_match(P, P, P, 0, 8, 8, 5, 5, P, 1 << 20, None), "B=0")
    assert lib.pivlfn_target_points_workspace_bytes(2, 10, 30) == 2 * (2 * 300 + 2) * 4
    refused(lib.pivlfn_target_points(P, 1, 8, 8, 0.7, 16, P, None, P, P, 1 << 20, None), "target_points", "null")
    refused(lib.pivlfn_target_points(P, 1, 8, 8, 0.7, 0, P, P, P, P, 1 << 20, None), "cap=0")
    refused(lib.pivlfn_target_points(P, 1, 8, 8, float("nan"), 4, P, P, P, P, 1 << 20, None), "NaN")
    refused(lib.pivlfn_target_points(P, 1, 8, 8, 0.7, 4, P, P, P, P, 16, None), "workspace")
    refused(lib.pivlfn_target_points(P, 1, 46341, 46341, 0.7, 4, P, P, P, P, 1 << 20, None), "32-bit index range")
    refused(lib.pivlfn_dewarp_frames(P, None, 0, 1, 8, 8, A, 0.0, 0.0, 0, 0.0, None), "dewarp_frames", "null")
    refused(lib.pivlfn_dewarp_frames(P, P, 0, 1, 8, 8, A, 0.0, 0.0, 0, 0.0, None), "in place")
    refused(lib.pivlfn_dewarp_frames(P, 2 * P, 0, 1, 8, 8, A, 0.0, 0.0, 2, 0.0, None), "mode=2")
    refused(lib.pivlfn_dewarp_frames(P, 2 * P, 0, 1, 8, 8, A, 0.0, 0.0, 0, 256.0, None), "fill")
    refused(lib.pivlfn_dewarp_frames(P, 2 * P, 1, 1, 8, 8, A, float("inf"), 0.0, 0, 0.0, None), "origin")
    refused(lib.pivlfn_dewarp_frames(P, 2 * P, 1, 1, 8, 8, A, 0.0, 0.0, 0, float("inf"), None), "fill", "fp32 range")
    refused(lib.pivlfn_dewarp_frames(P, 2 * P, 1, 1, 8, 8, A, 0.0, 0.0, 0, -3.5e38, None), "fill", "fp32 range")
    A[7] = float("nan")
    refused(lib.pivlfn_dewarp_frames(P, 2 * P, 1, 1, 8, 8, A, 0.0, 0.0, 0, 0.0, None), "coefficient 7")
