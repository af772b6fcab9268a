"""GPU: pivlfn_template_match, pivlfn_target_points and pivlfn_dewarp_frames (csrc/calibrate.hip) against the NumPy restatement of their
contracts (tests/calibrate_restatement.py), the Python layer on top (pivlfn.calibrate) and stereo_cal.py.

All three contracts are exact (integer sums; fp64 operations rounded one by one): everything is compared bit for bit, in guarded
buffers whose outputs hold a sentinel beforehand.  Shapes are the smallest that reach every path: images smaller than the template's
padding, one tile, tiles of 64 x 16 outputs (four per lane) straddled in both axes with a halo wider than the remainder, the 255 x 255 template whose
window sums reach the 32-bit headroom; for the labelling (blocks of 256 pixels in row-major order) components that wind across many
blocks with their smallest index far from where the merges happen.  Everything here runs on the default stream; the stream and capture
contract is in tests/calibrate_stream_cases.py, which one test runs in a process of its own."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import calibrate_restatement as cr
from pivlfn import _lib
from pivlfn import calibrate as cal
from test_gpu_op_streams import _buf, _check, _p

pytestmark = pytest.mark.gpu
F32, I32, I64, U8 = torch.float32, torch.int32, torch.int64, torch.uint8


def _in(x, dev):
    """A host array in a guarded device buffer."""
    t = torch.from_numpy(np.ascontiguousarray(x))
    g = _buf(t.shape, t.dtype, dev, "nan")
    g.copy_(t)
    return g


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ---- (a) template matching ---------------------------------------------------------------------------------------------------------------
def gpu_match(images, templ, dev, dirty=True):
    lib = _lib.load()
    B, H, W = images.shape
    th, tw = templ.shape
    need = lib.pivlfn_template_match_workspace_bytes(th, tw)
    i, t, r, ws = _in(images, dev), _in(templ, dev), _buf((B, H, W), F32, dev, "sentinel"), _buf((need,), U8, dev, "sentinel")
    if not dirty:
        ws.zero_()
    _lib.check(lib.pivlfn_template_match(_p(i), _p(t), _p(r), B, H, W, th, tw, _p(ws), need, _stream(dev)), "template_match")
    torch.cuda.synchronize()
    for b in (i, t, r, ws):
        _check(b, f"template_match {H}x{W} / {th}x{tw}")
    assert np.array_equal(i.cpu().numpy(), images) and np.array_equal(t.cpu().numpy(), templ)
    return r.cpu().numpy()


@pytest.mark.parametrize("H,W,th,tw", [(1, 1, 5, 5), (3, 2, 5, 5), (7, 9, 5, 5), (7, 9, 3, 7), (33, 65, 5, 5), (33, 65, 25, 25), (64, 129, 5, 5),
                                       (64, 129, 25, 25)])
def test_match_bits_of_the_restatement(H, W, th, tw, dev):
    """Batch 3: a random image, an all-255 image (b = 0 on every window inside) and an image that holds the template."""
    rng = np.random.default_rng(H * 1000 + W + th)
    templ = rng.integers(0, 256, (th, tw), dtype=np.uint8)
    images = np.stack([rng.integers(0, 256, (H, W), dtype=np.uint8), np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8)])
    exact = H >= th + 2 and W >= tw + 2
    if exact:
        images[2, 1:1 + th, 2:2 + tw] = templ
    want = cr.template_match(images, templ)
    got = gpu_match(images, templ, dev)
    assert cr.same_bits(got, want)
    if exact:
        assert got[2, 1 + th // 2, 2 + tw // 2] == np.float32(1.0) and np.all(got[1, th // 2:H - th // 2, tw // 2:W - tw // 2] == 0)
    assert cr.same_bits(gpu_match(images[:1], templ, dev, dirty=False)[0], want[0])        # alone, clean workspace: the same bits


def test_match_reaches_the_32_bit_headroom(dev):
    """A 255 x 255 template of 255s and 0s on a 16 x 16 checkerboard of 255s and 0s: sum(T^2) = 255^2 * 32513 and the window sums of the
    centre pixels come within a factor of 1.01 of 2^32 / 2."""
    yy, xx = np.meshgrid(np.arange(255), np.arange(255), indexing="ij")
    templ = np.where((yy + xx) % 2 == 0, 255, 0).astype(np.uint8)
    image = np.where(np.add.outer(np.arange(16), np.arange(16)) % 2 == 0, 255, 0).astype(np.uint8)
    full = np.full((255, 255), 255, np.uint8)
    full[0, 0] = 0                                                               # sum(T^2) = 255^2 * 65024: within 2e-5 of 2^32
    for t in (templ, full):
        want = cr.template_match(image[None], t)
        assert np.abs(want).max() > 0
        assert cr.same_bits(gpu_match(image[None], t, dev), want)
    assert cr.same_bits(gpu_match(np.full((1, 16, 16), 255, np.uint8), full, dev), cr.template_match(np.full((1, 16, 16), 255, np.uint8), full))


# ---- (b) marker centres ---------------------------------------------------------------------------------------------------------------------
def gpu_points(r, threshold, cap, dev, dirty=True):
    lib = _lib.load()
    B, H, W = r.shape
    need = lib.pivlfn_target_points_workspace_bytes(B, H, W)
    i = _in(r, dev)
    labels, count, rec = _buf((B, H, W), I32, dev, "sentinel"), _buf((B,), I32, dev, "sentinel"), _buf((B, cap, 4), I64, dev, "sentinel")
    ws = _buf((need,), U8, dev, "sentinel")
    if not dirty:
        ws.zero_()
    _lib.check(lib.pivlfn_target_points(_p(i), B, H, W, threshold, cap, _p(labels), _p(count), _p(rec), _p(ws), need, _stream(dev)),
               "target_points")
    torch.cuda.synchronize()
    for b in (i, labels, count, rec, ws):
        _check(b, f"target_points {H}x{W}")
    assert cr.same_bits(i.cpu().numpy(), r)
    return labels.cpu().numpy(), count.cpu().numpy(), rec.cpu().numpy()


def _same_points(got, want):
    return all(cr.same_bits(g, w) for g, w in zip(got, want))


def spiral(H, W, step=4):
    r = np.zeros((H, W), np.float32)
    top, left, bottom, right = 1, 1, H - 3, W - 3
    while right - left > step and bottom - top > step:
        r[top, left:right + 1] = 1
        r[top:bottom + 1, right] = 1
        r[bottom, left + step:right + 1] = 1
        r[top + step:bottom + 1, left + step] = 1
        top, left, bottom, right = top + step, left + step, bottom - step, right - step
        r[top, left - step:left + 1] = 1                                          # the arm that leads into the next turn
    return r


def comb(H, W):
    """Long teeth joined only along the bottom row: the smallest index is the top of the first tooth, every merge happens at the far end."""
    r = np.zeros((H, W), np.float32)
    r[1:H - 3, 2:W - 3:4] = 0.9
    r[H - 4, 2:W - 3] = 0.8
    return r


def test_points_on_hand_made_maps(dev):
    H, W = 48, 64                                                                # 12 blocks of 256 pixels
    thr = 0.7
    none = np.full((H, W), 0.5, np.float32)
    single = none.copy()
    single[20, 33] = 0.9
    equal = none.copy()
    equal[10, 10] = np.float32(thr)                                              # exactly the threshold: not kept
    equal[0, 0] = np.nextafter(np.float32(thr), np.float32(1))                   # one ulp above, in the reflected corner: kept
    diag = none.copy()
    diag[5, 5] = diag[6, 6] = 0.8                                                # touch only diagonally; their box-sums overlap
    diag[30, 30] = diag[31, 33] = 0.8                                            # box-sums one column apart: two components
    frame = none.copy()
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = 1.0               # touches all four borders
    frame[10:13, 10:13] = np.nan                                                 # NaNs are not kept
    huge = none.copy()
    huge[20:26, 8:14] = np.inf                                                   # q is clamped at 2^29: four of them do not wrap 32 bits
    huge[30:34, 40:44] = 8192.0                                                  # exactly the clamp
    huge[30:34, 50:54] = 16384.0
    huge[40, 20:23] = (3.0e38, 8191.99951171875, 65535.0)                        # the largest float below the clamp among them
    assert int(cr.box_sum(huge, thr).max()) == 1 << 31
    maps = {"none": (none, 0), "huge": (huge, 4), "single": (single, 1), "equal": (equal, 1), "diag": (diag, 3), "frame": (frame, 1), "spiral": (spiral(H, W), 1),
            "comb": (comb(H, W), 1)}
    for name, (r, n) in maps.items():
        want = cr.target_points(r[None], thr, 8)
        assert want[1][0] == n, name
        got = gpu_points(r[None], thr, 8, dev)
        assert _same_points(got, want), name
    assert (cr.box_sum(maps["spiral"][0], thr) > 0).sum() > 700 and (cr.box_sum(maps["comb"][0], thr) > 0).sum() > 1200
    # a batch of all of them: the same bits as alone; clean and dirty workspace alike
    batch = np.stack([m for m, _ in maps.values()])
    want = cr.target_points(batch, thr, 8)
    assert _same_points(gpu_points(batch, thr, 8, dev), want) and _same_points(gpu_points(batch, thr, 8, dev, dirty=False), want)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (5, 1), (17, 16), (37, 53)])
def test_points_on_random_maps_of_odd_sizes(H, W, dev):
    rng = np.random.default_rng(H * 100 + W)
    r = rng.random((2, H, W)).astype(np.float32)
    r[0] = np.where(r[0] > 0.55, r[0], 0)                                        # near the percolation threshold: winding components
    want = cr.target_points(r, 0.6, 64)
    assert _same_points(gpu_points(r, 0.6, 64, dev), want)


def test_more_components_than_cap(dev):
    rng = np.random.default_rng(11)
    r = np.zeros((2, 40, 50), np.float32)
    for b, n in ((0, 3), (1, 12)):
        for k in range(n):
            r[b, 3 + 9 * (k // 4) + int(rng.integers(0, 3)), 4 + 12 * (k % 4) + int(rng.integers(0, 3))] = 0.75 + 0.2 * rng.random()
    want = cr.target_points(r, 0.7, 5)
    got = gpu_points(r, 0.7, 5, dev)                                             # _check: the memory behind rec is untouched
    assert want[1].tolist() == [3, 12] and _same_points(got, want)
    assert np.all(got[2][0, 3:] == 0) and np.all(got[2][1, :, 3] >= 1)
    full = cr.target_points(r, 0.7, 16)
    assert cr.same_bits(got[2][1], full[2][1, :5])                               # the first cap records are the first of all


def marker_map(H, W, seed, n):
    """A quiet map with n blobs of 3 x 3 to 5 x 5 pixels above 0.7 at random places, one long thin component (a row and a column that
    cross) through many blocks of 256 pixels, and a single pixel in the last row: a component whose root lies in the last block."""
    rng = np.random.default_rng(seed)
    r = (0.5 * rng.random((H, W))).astype(np.float32)
    for _ in range(n):
        s = int(rng.integers(3, 6))
        y, x = int(rng.integers(0, H - s + 1)), int(rng.integers(0, W - s + 1))
        r[y:y + s, x:x + s] = (0.75 + 0.2 * rng.random((s, s))).astype(np.float32)
    r[H // 2, 3:W - 3] = 0.9
    r[5:H - 5, W // 3] = 0.85
    r[H - 3:, W - 10:W - 1] = 0.1
    r[H - 1, W - 6] = 0.9
    return r


def _scan_shapes():
    import analysis_plans as ap
    return ap.shapes(ap.TARGET_POINTS_CASES)


@pytest.mark.parametrize("H,W", _scan_shapes())
def test_points_where_the_scan_plan_changes(H, W, dev):
    """More than 256 blocks of 256 pixels: a thread of tp_scan_kernel sums and prefixes `per` >= 2 of them.  257 x 256: per = 2 and only
    thread 128 has a short range (the last block, which holds a root); 349 x 513: per = 3, threads from 234 on are empty; 1024 x 1280,
    the size of a camera image: per = 20.  Two maps a call (the second upside down: its single pixel lies in the first row), a few hundred components each, with
    `cap` below and above their number: the prefix decides which record a component lands in and which ones `cap` cuts off."""
    import analysis_plans as ap
    plan = ap.tp_scan(H, W)
    assert plan["per"] >= 2 and _lib.load().pivlfn_target_points_workspace_bytes(1, H, W) == (2 * H * W + plan["nblk"]) * 4
    r = np.stack([marker_map(H, W, H + W, 150 + H * W // 8000), marker_map(H, W, H + W + 1, 190 + H * W // 8000)[::-1]])
    for cap in (40, 1024):
        want = cr.target_points(r, 0.7, cap)
        n = want[1]
        assert 100 <= n.min() and n.max() < 1024 and n[0] != n[1]
        assert want[0][0].max() >= (plan["nblk"] - 1) * 256, "no root in the last block"
        big = np.bincount(want[0][0][want[0][0] >= 0]).max()
        assert big >= H + W - 20 and (cap < n[0] or want[2][0, :, 3].max() == big)        # the long component and its record
        got = gpu_points(r, 0.7, cap, dev)
        assert _same_points(got, want), f"{H}x{W} cap={cap}"
        assert np.all(got[2][:, :min(cap, n.min()), 3] >= 1)
    assert _same_points(gpu_points(r[1:], 0.7, 1024, dev, dirty=False), [w[1:] for w in want])       # alone, clean workspace


# ---- (c) dewarp --------------------------------------------------------------------------------------------------------------------------------
def gpu_dewarp(frames, A, origin, mode, fill, dev):
    lib = _lib.load()
    B, H, W = frames.shape
    f32 = frames.dtype == np.float32
    i, o = _in(frames, dev), _buf((B, H, W), F32 if f32 else U8, dev, "sentinel")
    a_c = (ctypes.c_double * 24)(*np.asarray(A, np.float64).tolist())
    _lib.check(lib.pivlfn_dewarp_frames(_p(i), _p(o), int(f32), B, H, W, a_c, origin[0], origin[1], {"nearest": 0, "bilinear": 1}[mode],
                                        fill, _stream(dev)), "dewarp_frames")
    torch.cuda.synchronize()
    _check(i, "dewarp in")
    _check(o, "dewarp out")
    return o.cpu().numpy()


IDENTITY = np.array([1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0], dtype=np.float64)


def _mappings(H, W):
    from calibrate_stream_cases import mapping
    half = IDENTITY.copy()
    half[2], half[14] = 1.5, -1.5                                                # every source exactly on .5: half to even, ax = ay = 0.5
    outside, origin = mapping(np.random.default_rng(H + W), H, W)
    mild = IDENTITY.copy()
    mild[[0, 1, 3, 5, 6, 7]] = (0.9, 0.03, 2e-4, -1e-4, 3e-4, -2e-4)
    mild[[12, 13, 16, 18, 19]] = (-0.02, 0.92, 1e-4, 1e-4, 2e-4)
    return {"identity": (IDENTITY, (0.0, 0.0)), "half": (half, (1.0, 2.0)), "outside": (outside, origin), "mild": (mild, (W / 2 - 0.3, H / 2 + 0.2))}


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("H,W", [(5, 7), (33, 65)])
def test_dewarp_bits_of_the_restatement(H, W, kind, mode, dev):
    rng = np.random.default_rng(H + 7 * W)
    frames = rng.integers(0, 256, (2, H, W), dtype=np.uint8) if kind == "u8" else (100 * rng.standard_normal((2, H, W))).astype(np.float32)
    fill = 200.0 if kind == "u8" else -7.25
    filled = {}
    for name, (A, origin) in _mappings(H, W).items():
        want = cr.dewarp(frames, A, origin, mode, fill)
        assert cr.same_bits(gpu_dewarp(frames, A, origin, mode, fill, dev), want), name
        sx, sy = cr.source_positions(H, W, A, origin)
        filled[name] = ((np.round(sx) < 0) | (np.round(sx) > W - 1) | (np.round(sy) < 0) | (np.round(sy) > H - 1)).mean()
    assert filled["identity"] == 0 and 0.05 < filled["outside"] < 0.95 and 0 < filled["half"] < 0.5
    if kind == "f32":                                                            # a NaN fill marks what fell outside
        A, origin = _mappings(H, W)["outside"]
        want = cr.dewarp(frames, A, origin, mode, float("nan"))
        assert np.isnan(want).any() and cr.same_bits(gpu_dewarp(frames, A, origin, mode, float("nan"), dev), want)
    sx, sy = cr.source_positions(H, W, *_mappings(H, W)["half"])
    assert np.all(sx % 1 == 0.5) and np.all(sy % 1 == 0.5)
    if mode == "nearest":
        want = cr.dewarp(frames, *_mappings(H, W)["half"], mode, fill)
        assert np.array_equal(want[:, 2, 1], frames[:, 0, 2]) and np.array_equal(want[:, 3, 2], frames[:, 2, 4])     # 2.5 -> 2, 0.5 -> 0, 3.5 -> 4, 1.5 -> 2


# ---- the chain ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["96", "192x320"])
def test_calibrate_camera_gives_the_restatements_records_and_coefficients(name, dev):
    image, templ, centres, index, ref4 = cr.target(name)
    want = cr.calibrate_camera(image, templ, ref4)
    got = cal.calibrate_camera(torch.from_numpy(image).to(dev), templ, ref4)
    assert cr.same_bits(got["records"], want["records"]) and cr.same_bits(got["markers"], want["markers"])
    assert np.array_equal(got["ij"], want["ij"]) and got["indexed"].all() and got["spacing"] == want["spacing"]
    assert cr.same_bits(got["A"], want["A"]) and got["rms"] == want["rms"] and got["max"] == want["max"]
    r = cal.template_match(torch.from_numpy(image).to(dev), templ)
    assert cr.same_bits(r.cpu().numpy(), cr.template_match(image, templ))
    dew = cal.dewarp_frames(torch.from_numpy(image).to(dev), got["A"], got["origin"], "nearest", 0)
    assert cr.same_bits(dew.cpu().numpy(), cr.dewarp(image, want["A"], want["origin"], "nearest", 0))


def test_find_markers_batches_and_border_rule(dev):
    image, templ, centres, index, ref4 = cr.target("96")
    other = cr.target("96", seed=7)[0]
    both = torch.from_numpy(np.stack([image, other])).to(dev)
    for border in (True, False):
        pts, recs = cal.find_markers(both, templ, border=border)
        for k, im in enumerate((image, other)):
            wp, wr = cr.find_markers(im, templ, border=border)
            assert cr.same_bits(pts[k], wp) and cr.same_bits(recs[k], wr)
    capped, _ = cal.find_markers(both, templ, cap=5, border=False)
    assert len(capped[0]) == 5 and cr.same_bits(capped[0], cr.find_markers(image, templ, border=False)[0][:5])


# ---- the command line ---------------------------------------------------------------------------------------------------------------------------
def test_stereo_cal_writes_a_coefficient_file_stereo_2d3c_accepts(tmp_path, dev):
    from pivlfn import stereo
    from pivlfn.viz import write_png_gray
    here = os.path.dirname(os.path.abspath(__file__))
    left = cr.target("192x320")
    right = cr.target("192x320", seed=9)
    root, save = tmp_path / "imgs", tmp_path / "out"
    root.mkdir()
    for cam, t in (("L", left), ("R", right)):
        write_png_gray(str(root / f"plate-{cam}.png"), np.bitwise_not(t[0]))     # dark crosses on a bright plate
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        os.path.join(os.path.dirname(here), "piv_liteflownet-pytorch_amd", "stereo_cal.py"), "--root", str(root), "--name", "plate", "--save",
        str(save), "--overlay", "--ref-left"] + [f"{v:.2f}" for v in left[4].ravel()] + ["--ref-right"] + [f"{v:.2f}" for v in right[4].ravel()]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert len(re.findall(r"(\d+) markers, \1 indexed", r.stdout)) == 2, r.stdout
    for f in ("plate-L_markers.png", "plate-R_markers.png", "plate-L_dewarped.png", "plate-R_dewarped.png"):
        assert (save / f).is_file()
    coeff = stereo.read_coeff(str(save / "plate.json"))
    for side, t in (("Left", left), ("Right", right)):
        assert cr.same_bits(np.array(coeff[side]), cr.calibrate_camera(t[0], t[1], t[4])["A"])
    assert 40 < coeff["calib"] < 56
    flow = torch.zeros(2, 2, 16, 24, device=dev)
    flow[:, 0], flow[:, 1] = 1.5, -0.75
    out = stereo.stereo_2d3c(flow, coeff, stereo.tangents(*stereo.angles(45.0, 0.0)))
    assert out.shape == (1, 16, 24, 3) and bool(torch.isfinite(out).all())


# ---- side streams and graph capture: in a process of their own ------------------------------------------------------------------------------------
def test_stream_contract_in_a_process_of_its_own(dev):
    """tests/calibrate_stream_cases.py in a fresh pytest process: 16 tests, all passing.  Why not in this process:
    tests/test_gpu_flowmap.py::test_stream_contract_and_run_py_in_a_process_of_their_own says it."""
    here = os.path.dirname(os.path.abspath(__file__))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                                                                          os.path.join(here, "calibrate_stream_cases.py")]
    r = subprocess.run(cmd, cwd=here, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and re.search(r"\b16 passed", r.stdout), r.stdout[-6000:] + r.stderr[-2000:]
