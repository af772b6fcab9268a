"""CPU: the numpy restatement of pivlfn_match_quality's contract (tests/quality_restatement.py) against hand-computed values, a scalar
loop over the clipped window and the physics it is meant to show on synthetic particle images; the argument errors of
pivlfn.quality.match_quality and the C entry point's refusals, which need no GPU."""
import math

import numpy as np
import pytest
import torch

import quality_restatement as qr
from quality_restatement import CENTRE_OUT, FEW, FLAT, NO_PEAK

INTERIOR = (slice(24, -24), slice(24, -24))
SEEDS = (7, 11, 12)
PLANTED = np.array([0.3, -0.2], np.float32)[:, None, None]


@pytest.fixture(scope="module")
def pairs():
    """seed -> (img1, img2, true flow) at 128 x 128, C = 1; computed once, never changed."""
    out = {}
    for seed in SEEDS + (107,):
        a, c, f = qr.particle_images(1, 128, 128, 1, seed)
        for t in (a, c, f):
            t.setflags(write=False)
        out[seed] = (a[0], c[0], f[0])
    return out


# ---- hand-computed values --------------------------------------------------------------------------------------------------------
def test_restatement_on_a_3x3_image_by_hand():
    """img1 = img2 = [[1,2,1],[2,4,2],[1,2,1]], zero flow, r = 1, min_count 2.  Centre, shift 0: n = 9, A = 16, AA = 36,
    va = vb = cov = 36 - 256/9, c0 = 1.  Shift (-1, 0): the six pixels of columns 1, 2 against columns 0, 1: A = Bs = 12, AA = BB = 30,
    AB = 24, va = vb = 6, cov = 24 - 144/6 = 0, c = 0: not a positive side value, NO_PEAK.  By symmetry the other shifts too."""
    img = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], np.float32)[None]
    q, flag, cs = qr.pair_quality(img, img, np.zeros((2, 3, 3), np.float32), 1, min_count=2)
    assert abs(cs[0, 1, 1] - 1.0) < 1e-15
    assert np.all(cs[1:, 1, 1] == 0.0)
    assert flag[1, 1] == NO_PEAK and q[1, 1, 1] == 0.0 and q[2, 1, 1] == 0.0
    assert abs(float(q[0, 1, 1]) - 1.0) < 1e-7
    # corner (0, 0), shift 0: the window is the 2 x 2 block 1, 2, 2, 4: n = 4, A = 9, AA = 25, va = 25 - 81/4 = 4.75, c = 1
    assert abs(cs[0, 0, 0] - 1.0) < 1e-15
    # the default min_count is 5 of 9: the corner's four pixels are too few, an edge's six are not
    _, flag5, _ = qr.pair_quality(img, img, np.zeros((2, 3, 3), np.float32), 1)
    assert flag5[0, 0] == FEW and flag5[0, 1] == NO_PEAK and flag5[1, 1] == NO_PEAK


def test_restatement_on_a_1x5_image_by_hand():
    """img1 = img2 = [0,1,0,2,0], zero flow, r = 1, min_count 2: the window of a one-row image is three pixels (two at the ends).
    Pixel 2, shift 0: values 1, 0, 2: n = 3, A = 3, AA = 5, va = 5 - 9/3 = 2, c0 = 1.  Shift (-1, 0): a = (1, 0, 2) against
    b = (0, 1, 0): A = 3, AA = 5, Bs = 1, BB = 1, AB = 0: va = 2, vb = 1 - 1/3, cov = 0 - 3/3 = -1, c = -1/sqrt(2 * 2/3) = -sqrt(3)/2.
    Both y shifts leave the image: n = 0, few.  NO_PEAK everywhere."""
    img = np.array([[0, 1, 0, 2, 0]], np.float32)[None]
    q, flag, cs = qr.pair_quality(img, img, np.zeros((2, 1, 5), np.float32), 1, min_count=2)
    assert np.allclose(cs[0, 0], 1.0, rtol=0, atol=1e-15)
    assert abs(cs[1, 0, 2] + math.sqrt(3.0) / 2.0) < 1e-15
    assert np.all(np.isnan(cs[3:]))
    assert np.all(flag == NO_PEAK) and np.all(q[1:] == 0.0)
    # the flow (0.5, 0) samples halfway: b = (0.5, 0.5, 1, 1) and the last pixel warps to x = 4.5 > W - 1: invalid
    b, m = qr.warp(img[0].astype(np.float64), np.stack([np.full((1, 5), 0.5, np.float32), np.zeros((1, 5), np.float32)]))
    assert b.tolist() == [[0.5, 0.5, 1.0, 1.0, 0.0]] and m.tolist() == [[True, True, True, True, False]]


def _scalar_pixel(a, b, m, k, y, x, r, min_count, floor):
    """The contract at one pixel with plain Python floats and a loop over the window clipped to the image."""
    H, W = a.shape
    cs, bad = [], []
    for sx, sy in qr.SHIFTS:
        tot = [0.0] * 6
        for yy in range(max(y - r, 0), min(y + r, H - 1) + 1):
            row = [0.0] * 6
            for xx in range(max(x - r, 0), min(x + r, W - 1) + 1):
                qy, qx = yy + sy, xx + sx
                if k[yy, xx] and 0 <= qy < H and 0 <= qx < W and m[qy, qx]:
                    av, bv = float(a[yy, xx]), float(b[qy, qx])
                    term = (1.0, av, av * av, bv, bv * bv, av * bv)
                else:
                    term = (0.0,) * 6
                row = [s + t for s, t in zip(row, term)]
            tot = [s + t for s, t in zip(tot, row)]
        n, A, AA, Bs, BB, AB = tot
        if n < min_count:
            cs.append(math.nan)
            bad.append(FEW)
            continue
        va, vb, cov = AA - A * A / n, BB - Bs * Bs / n, AB - A * Bs / n
        if va < floor * floor * n or vb < floor * floor * n:
            cs.append(math.nan)
            bad.append(FLAT)
            continue
        cs.append(cov / math.sqrt(va * vb))
        bad.append(0)
    flag, dx, dy = bad[0], 0.0, 0.0
    if flag == 0:
        c0 = cs[0]
        ok = not any(bad[1:]) and c0 > 0.0
        for cm, cp in ((cs[1], cs[2]), (cs[3], cs[4])):
            ok = ok and cm > 0.0 and cp > 0.0 and c0 >= cm and c0 >= cp and (2.0 * c0 - cm) - cp >= 1e-6
        if ok:
            l0 = math.log(c0)
            lm, lp = math.log(cs[1]), math.log(cs[2])
            dx = 0.5 * (lm - lp) / ((lm - 2.0 * l0) + lp)
            lm, lp = math.log(cs[3]), math.log(cs[4])
            dy = 0.5 * (lm - lp) / ((lm - 2.0 * l0) + lp)
        else:
            flag = NO_PEAK
    if not k[y, x] or not m[y, x]:
        flag |= CENTRE_OUT
    return cs[0] if not flag & 3 else math.nan, dx, dy, flag


@pytest.mark.parametrize("C", [1, 3])
def test_restatement_equals_a_scalar_loop_over_the_clipped_window(C):
    """Zero padding against the clipped window, vectorised against scalar: every pixel of a 13 x 17 image with a mask, invalid samples, a flat patch
    and all four flag bits, r = 2."""
    H, W, r = 13, 17, 2
    a, c, f = qr.particle_images(1, H, W, C, 5)
    qr.flatten_patch(a, c, 7, 1, size=5)
    f = f + np.float32(0.35)
    f[0, 0, :, 0] = -30.0
    f[0, 1, 3, 5] = np.nan
    mask = qr.speckle_mask(1, H, W, 3, 6)[0]
    q, flag, _ = qr.pair_quality(a[0], c[0], f[0], r, mask)
    ga = qr.gray(a[0])
    b, m = qr.warp(qr.gray(c[0]), f[0])
    seen = 0
    for y in range(H):
        for x in range(W):
            c0, dx, dy, fl = _scalar_pixel(ga, b, m, mask == 0, y, x, r, 13, 1.0 / 255.0)
            assert fl == flag[y, x], (y, x)
            want = np.array([c0, dx, dy]).astype(np.float32)
            assert np.array_equal(want, q[:, y, x], equal_nan=True), (y, x, want, q[:, y, x])
            seen |= fl
    assert seen == FEW | FLAT | NO_PEAK | CENTRE_OUT
    assert np.any(flag == 0)


# ---- what the measure shows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_true_flow_correlates_and_has_a_peak_everywhere(pairs, seed):
    a, c, f = pairs[seed]
    q, flag, _ = qr.pair_quality(a, c, f, 8)
    assert np.median(q[0][INTERIOR]) > 0.95
    assert not np.any(flag[INTERIOR] & NO_PEAK)
    assert not np.any(flag[INTERIOR])


@pytest.mark.parametrize("seed", SEEDS)
def test_planted_error_is_recovered_as_the_residual(pairs, seed):
    """The flow lacks (0.3, -0.2) px: the mean residual finds it to 0.05 px (measured: off by at most 0.022 px), with the sign that makes
    flow + residual the corrected vector."""
    a, c, f = pairs[seed]
    q, flag, _ = qr.pair_quality(a, c, f - PLANTED, 8)
    assert not np.any(flag[INTERIOR])
    mean = np.array([q[1][INTERIOR].mean(), q[2][INTERIOR].mean()])
    print("planted (0.3, -0.2), seed", seed, "mean residual", mean)
    assert np.all(np.abs(mean - np.array([0.3, -0.2])) < 0.05)


def test_an_error_beyond_half_a_pixel_has_no_peak_at_zero_shift(pairs):
    a, c, f = pairs[7]
    _, flag, _ = qr.pair_quality(a, c, f - 2.0 * PLANTED, 8)
    assert (flag[INTERIOR] & NO_PEAK).astype(bool).mean() > 0.5


def test_an_unrelated_second_image_does_not_correlate(pairs):
    a, _, f = pairs[7]
    q, flag, _ = qr.pair_quality(a, pairs[107][1], f, 8)
    assert np.nanmedian(q[0][INTERIOR]) < 0.2
    assert (flag[INTERIOR] & NO_PEAK).astype(bool).mean() > 0.5


def test_three_equal_channels_give_the_bits_of_one(pairs):
    a, c, f = pairs[11]
    q1, f1, _ = qr.pair_quality(a, c, f - PLANTED, 4)
    q3, f3, _ = qr.pair_quality(np.repeat(a, 3, 0), np.repeat(c, 3, 0), f - PLANTED, 4)
    assert np.array_equal(q1.view(np.int32), q3.view(np.int32)) and np.array_equal(f1, f3)


# ---- host logic --------------------------------------------------------------------------------------------------------------------
def test_match_quality_argument_errors():
    from pivlfn import FEW as few, FLAT as flat, NO_PEAK as no_peak, CENTRE_OUT as centre_out, MatchQuality, match_quality
    from pivlfn.quality import check_params, default_min_count
    assert (few, flat, no_peak, centre_out) == (FEW, FLAT, NO_PEAK, CENTRE_OUT) == (1, 2, 4, 8)
    assert default_min_count(8) == 145 and check_params(8, 1 / 255, None) == 145 and check_params(1, 0.0, 9) == 9
    img, flow = torch.zeros(2, 1, 8, 8), torch.zeros(2, 2, 8, 8)
    for bad in (0, 16, 2.0, True, None):
        with pytest.raises(ValueError, match="radius"):
            match_quality(img, img, flow, radius=bad)
    for bad in (1, 26, 3.0, False):
        with pytest.raises(ValueError, match="min_count"):
            match_quality(img, img, flow, radius=2, min_count=bad)
    for bad in (-1e-3, math.nan, math.inf):
        with pytest.raises(ValueError, match="floor"):
            match_quality(img, img, flow, floor=bad)
    with pytest.raises(TypeError, match="img1"):
        match_quality(img.double(), img, flow)
    with pytest.raises(TypeError, match="img2"):
        match_quality(img, np.zeros((2, 1, 8, 8), np.float32), flow)
    with pytest.raises(ValueError, match="C = 1 or 3"):
        match_quality(torch.zeros(2, 2, 8, 8), torch.zeros(2, 2, 8, 8), flow)
    with pytest.raises(ValueError, match="img2"):
        match_quality(img, torch.zeros(2, 1, 8, 9), flow)
    with pytest.raises(ValueError, match="do not belong"):
        match_quality(img, img, torch.zeros(2, 2, 8, 9))
    with pytest.raises(ValueError, match="do not belong"):
        match_quality(img, img, torch.zeros(1, 2, 8, 8))
    with pytest.raises(TypeError, match="float32"):
        match_quality(img, img, flow.double())
    with pytest.raises(NotImplementedError, match="GPU"):            # there is no CPU path
        match_quality(img, img, flow)
    q = MatchQuality(torch.zeros(0, 4, 4), torch.zeros(0, 2, 4, 4), torch.zeros(0, 4, 4, dtype=torch.uint8))
    assert q.summary() == []


def test_summary_and_corrected_on_known_values():
    from pivlfn import MatchQuality
    buf = torch.zeros(1, 3, 2, 2)
    buf[0, 0] = torch.tensor([[0.5, math.nan], [1.0, 0.25]])
    buf[0, 1] = torch.tensor([[0.3, 0.0], [0.0, 0.0]])
    buf[0, 2] = torch.tensor([[-0.4, 0.0], [0.0, 0.0]])
    flag = torch.tensor([[[0, FEW | CENTRE_OUT], [NO_PEAK, 0]]], dtype=torch.uint8)
    q = MatchQuality(buf[:, 0], buf[:, 1:], flag)
    (s,) = q.summary()
    assert s["few"] == 0.25 and s["flat"] == 0.0 and s["no_peak"] == 0.25 and s["centre_out"] == 0.25 and s["n_fit"] == 2
    assert abs(s["mean_c"] - (0.5 + 1.0 + 0.25) / 3) < 1e-12
    assert abs(s["rms_residual"] - math.sqrt((0.09 + 0.16) / 2)) < 1e-7
    flow = torch.ones(1, 2, 2, 2)
    assert torch.equal(q.corrected(flow), flow + buf[:, 1:])
    assert q.c.data_ptr() == buf.data_ptr() and q.residual.data_ptr() == buf[:, 1:].data_ptr()


def test_c_entry_point_refuses_bad_arguments_without_a_gpu():
    """Every refusal of pivlfn_match_quality comes from the host, before any launch, as PIVLFN_ERR_ARG with a message naming the problem
    (a launch on a machine without a GPU would return PIVLFN_ERR_HIP instead)."""
    from pivlfn import _lib
    lib = _lib.load()
    P = 1 << 20                     # non-null, 8-byte aligned, never dereferenced: every case below fails its checks first
    far = [P + (i << 32) for i in range(7)]          # seven ranges that cannot overlap at these sizes
    img1, img2, flow, mask, qual, flag, ws = far
    B, H, W, r = 2, 8, 8, 2
    need = lib.pivlfn_match_quality_workspace_bytes(B, H, W, r)
    assert need >= B * H * W * 17 and need % 256 == 0
    assert lib.pivlfn_match_quality_workspace_bytes(0, H, W, r) == 0 and lib.pivlfn_match_quality_workspace_bytes(B, H, W, 16) == 0

    def call(**kw):
        a = dict(img1=img1, img2=img2, C=1, flow=flow, mask=mask, quality=qual, flag=flag, B=B, H=H, W=W, radius=r, min_count=13,
                 floor=1 / 255, ws=ws, ws_bytes=need)
        a.update(kw)
        return lib.pivlfn_match_quality(a["img1"], a["img2"], a["C"], a["flow"], a["mask"], a["quality"], a["flag"], a["B"], a["H"],
                                        a["W"], a["radius"], a["min_count"], a["floor"], a["ws"], a["ws_bytes"], None)

    def refused(rc, *words):
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1, (rc, msg)
        for w in ("match_quality",) + words:
            assert w in msg, (w, msg)

    for name in ("img1", "img2", "flow", "quality", "flag", "ws"):
        refused(call(**{name: None}), "null")
    refused(call(C=2), "C=2")
    refused(call(C=0), "C=0")
    refused(call(B=0), "positive")
    refused(call(H=-1), "positive")
    refused(call(W=0), "positive")
    refused(call(H=46341, W=46341), "2^31")
    refused(call(B=65536), "B=65536")
    refused(call(radius=0), "radius=0")
    refused(call(radius=16), "radius=16")
    refused(call(min_count=1), "min_count=1")
    refused(call(min_count=26), "min_count=26")
    refused(call(floor=-0.5), "floor")
    refused(call(floor=math.inf), "floor")
    refused(call(floor=math.nan), "floor")
    refused(call(ws=ws + 4), "8-byte aligned")
    refused(call(ws_bytes=need - 1), "too small")
    px = B * H * W
    refused(call(quality=img1), "quality overlaps img1")
    refused(call(quality=img2 + px * 4 - 4), "quality overlaps img2")
    refused(call(quality=flow - px * 12 + 4), "quality overlaps flow")
    refused(call(quality=mask), "quality overlaps mask")
    refused(call(quality=ws + 8), "quality overlaps the workspace")
    refused(call(flag=img1 + 3), "flag overlaps img1")
    refused(call(flag=flow + px * 8 - 1), "flag overlaps flow")
    refused(call(flag=mask), "flag overlaps mask")
    refused(call(flag=qual + px * 12 - 1), "quality overlaps flag")
    with pytest.raises(ValueError, match="radius=16"):
        _lib.check(call(radius=16), "match_quality")


def test_run_py_quality_flags_parse_and_are_checked_before_a_gpu_is_needed(tmp_path):
    import run as runpy
    plain = runpy.parser.parse_args(["-i", "x"])
    assert plain.quality is None and plain.quality_image is False
    assert not [ln for ln in runpy.args_lines(plain) if ln.split(":")[0] in runpy.QUALITY_FLAGS]
    assert runpy.parser.parse_args(["--quality"]).quality == 8
    full = runpy.parser.parse_args(["--quality", "4", "--quality-image"])
    assert (full.quality, full.quality_image) == (4, True)
    lines = runpy.args_lines(full)
    assert "quality: 4\n" in lines and "quality_image: True\n" in lines and not [ln for ln in lines if ln.startswith("color")]
    base = ["--model", "piv", "-i", str(tmp_path), "-o", str(tmp_path / "out")]
    for extra, word in ((["--quality-image"], "needs --quality"), (["--quality", "16"], "radius=16"), (["--quality", "0"], "radius=0"),
                        (["--quality", "-c", "1.5"], "-b/-c")):
        with pytest.raises(SystemExit, match=word):
            runpy.main(base + extra)
    assert not (tmp_path / "out").exists()
