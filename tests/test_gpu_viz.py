"""GPU: the kernels of csrc/viz.hip (pivlfn_flow_maxrad, pivlfn_flow_to_color, pivlfn_field_absmax, pivlfn_scalar_to_color,
pivlfn_flow_decimate), pivlfn.viz and run.py's picture flags.  Maxima, cell means and the scalar colour map against the numpy
restatement of tests/viz_restatement.py bit for bit; the flow colouring against the reference's own pictures (tests/golden/
viz_cases.npz): equal where the case is exact, within one level elsewhere (the device's atan2f against NumPy's)."""
import os

import numpy as np
import pytest
import torch

import pivlfn
import viz_restatement as vr
from guarded import check_guards, guarded
from pivlfn import _lib, synth, viz
from pivlfn.flo import read_flow

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SHAPES = [(1, 1, 1), (1, 1, 9), (1, 9, 1), (1, 13, 17), (1, 67, 131), (3, 13, 17)]      # 67 x 131: nine workgroups and a ragged group


@pytest.fixture(scope="module")
def cases():
    return np.load(os.path.join(GOLD, "viz_cases.npz"))


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _nchw(flow):
    """A fixture flow [H,W,2] or [L,H,W,2] -> [L,2,H,W]."""
    return np.ascontiguousarray((flow[None] if flow.ndim == 3 else flow).transpose(0, 3, 1, 2))


def _holes(rng, B, H, W):
    """Random flows with NaN / 1e10 / inf / 2e9 vectors, and a mask with speckles (None for the first variant)."""
    flow = rng.normal(0, 3, (B, 2, H, W)).astype(np.float32)
    vals = (np.nan, 1e10, -np.inf, 2e9)
    n = max(1, H * W // 20)
    for j, (b, c, y, x) in enumerate(zip(rng.integers(0, B, n), rng.integers(0, 2, n), rng.integers(0, H, n), rng.integers(0, W, n))):
        flow[b, c, y, x] = vals[j % 4]
    mask = (rng.random((B, H, W)) < 0.1).astype(np.uint8) * 5
    return flow, mask


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_maxima_and_cell_means_match_restatement(dev, B, H, W):
    rng = np.random.default_rng(B * 100000 + H * 1000 + W)
    clean = rng.normal(0, 3, (B, 2, H, W)).astype(np.float32)
    holed, mask = _holes(rng, B, H, W)
    gone = holed.copy()
    gone[-1, 0] = np.nan                                   # an image with nothing left: maximum 0, every cell empty
    block = clean.copy()
    block[0, :, :5, :5] = 1e10                             # an empty cell at cell sizes 1, 4 and 5
    for tag, flow, m in (("clean", clean, None), ("holes", holed, None), ("holes+mask", holed, mask), ("gone", gone, mask),
                         ("block", block, None)):
        ft, mt = _t(flow, dev), None if m is None else _t(m, dev)
        got = viz.flow_maxrad(ft, mt).cpu().numpy()
        assert _same_bits(got, vr.flow_maxrad(flow, m)), (tag, got, vr.flow_maxrad(flow, m))
        if tag == "gone":
            assert got[-1] == 0 and not viz.flow_to_color(ft, mask=mt)[-1].any()
        for cell in (1, 4, 5):
            mean, count = viz.decimate_flow(ft, cell, mt)
            want_mean, want_count = vr.flow_decimate(flow, cell, m)
            assert _same_bits(count.cpu().numpy(), want_count), (tag, cell)
            assert _same_bits(mean.cpu().numpy(), want_mean), (tag, cell)
            if tag in ("gone", "block"):
                assert (want_count == 0).any() and (mean.cpu().numpy()[:, 0][want_count == 0] == np.float32(1e10)).all()
    for dtype in (np.float32, np.float64):
        field = rng.normal(0, 2, (B, H, W)).astype(dtype)
        field.reshape(-1)[::7] = (np.nan, np.inf, -np.inf, 1e30)[H % 4]
        field[0, 0, 0] = -123.5
        for m in (None, mask):
            got = viz.field_absmax(_t(field, dev), None if m is None else _t(m, dev)).cpu().numpy()
            assert _same_bits(got, vr.field_absmax(field, m)), (dtype, got)
    assert viz.field_absmax(torch.full((2, H, W), float("nan"), device=dev)).tolist() == [0.0, 0.0]
    # the batch maximum is the maximum of the per-image values, and a batch equals its images one at a time
    per = viz.flow_maxrad(_t(holed, dev))
    assert all(torch.equal(viz.flow_maxrad(_t(holed[b:b + 1], dev)), per[b:b + 1]) for b in range(B))


# ---- where the grids are capped and the kernels stride (tests/analysis_plans.py) -------------------------------------------------------
def _plan_shapes(name):
    import analysis_plans as ap
    return ap.shapes(getattr(ap, name))


def _planted(H, W, sweep):
    """Where the maximum of the LAST image is planted: its last pixel, and a pixel that only a second stride visit of a capped grid
    reaches (`sweep` pixels are one visit of the whole grid)."""
    assert sweep + 5 < H * W - 1
    return [divmod(H * W - 1, W), divmod(sweep + 5, W)]


def _speckles(rng, B, H, W):
    return (rng.random((B, H, W)) < 0.1).astype(np.uint8) * 5


@pytest.mark.parametrize("B,H,W", _plan_shapes("VIZ_ABSMAX_CASES"))
def test_field_absmax_where_the_grid_is_capped(dev, B, H, W):
    """field_absmax has at most 256 workgroups an image: 257 x 256 is one block over, 1024 x 1024 sixteen visits.  float32 and float64,
    NaN and inf among the values, with and without a mask; a larger value in pixel 0 of the last image is masked."""
    import analysis_plans as ap
    plan = ap.viz_absmax(H, W)
    assert plan["blocks"] > plan["grid"] == 256
    rng = np.random.default_rng(B * 100000 + H * 1000 + W)
    mask = _speckles(rng, B, H, W)
    for dtype in (np.float32, np.float64):
        base = rng.normal(0, 2, (B, H, W)).astype(dtype)
        base.reshape(-1)[::7], base.reshape(-1)[3::11] = np.nan, (np.inf, -np.inf)[dtype == np.float64]
        for y, x in _planted(H, W, plan["sweep"]):
            field = base.copy()
            field[-1, y, x], field[-1, 0, 0], mask[-1, y, x], mask[-1, 0, 0] = -1234.5, 5000.0, 0, 5
            for m in (None, mask):
                got = viz.field_absmax(_t(field, dev), None if m is None else _t(m, dev)).cpu().numpy()
                assert _same_bits(got, vr.field_absmax(field, m)), (dtype, y, x, got)
                assert got[-1] == (5000.0 if m is None else 1234.5) and (B == 1 or 0 < got[0] < 20)


@pytest.mark.parametrize("B,H,W", _plan_shapes("VIZ_MAXRAD_CASES"))
def test_flow_maxrad_and_its_picture_where_the_grid_is_capped(dev, B, H, W):
    """flow_maxrad has at most 256 workgroups of 4-pixel groups an image: 513 x 512 is one block over.  The maximum in the last pixel
    and in one of the second visit, unknown and masked vectors as in the small cases; the picture normalised by it within one level."""
    import analysis_plans as ap
    plan = ap.viz_maxrad(H, W)
    assert plan["blocks"] > plan["grid"] == 256
    rng = np.random.default_rng(B * 100000 + H * 1000 + W)
    holed, mask = _holes(rng, B, H, W)
    for y, x in _planted(H, W, plan["sweep"]):
        flow = holed.copy()
        flow[-1, :, y, x], flow[-1, :, 0, 0], mask[-1, y, x], mask[-1, 0, 0] = (30.0, -40.0), (300.0, 400.0), 0, 5
        for m in (None, mask):
            ft, mt = _t(flow, dev), None if m is None else _t(m, dev)
            got = viz.flow_maxrad(ft, mt).cpu().numpy()
            want = vr.flow_maxrad(flow, m)
            assert _same_bits(got, want) and got[-1] == (500.0 if m is None else 50.0), (y, x, got, want)
            pic = viz.flow_to_color(ft, mask=mt).cpu().numpy()
            assert np.abs(pic.astype(int) - vr.flow_to_color(flow, want, m).astype(int)).max() <= 1, (y, x)


@pytest.mark.parametrize("B,H,W", _plan_shapes("VIZ_COLOR_CASES"))
def test_pictures_and_cell_means_where_the_grid_is_capped(dev, B, H, W):
    """More than 4 Mi pixels over the batch: flow_to_color and scalar_to_color (groups of four pixels) and flow_decimate at cell 1 (one
    cell a thread) run on VZ_MAX_BLOCKS workgroups and stride over the rest -- five images of 1024 x 1024, and 2049 x 2048, two blocks
    over.  The largest vector of the last image lies in its last pixel, which only the second visit reaches."""
    import analysis_plans as ap
    plan = ap.viz_color(B, H, W)
    assert plan["blocks"] > plan["grid"] == ap.VZ_MAX_BLOCKS and plan["decimate_blocks"] > plan["decimate_grid"] and plan["sweep"] < B * H * W
    rng = np.random.default_rng(B * 100000 + H * 1000 + W)
    flow, mask = _holes(rng, B, H, W)
    flow[-1, :, H - 1, W - 1], mask[-1, H - 1, W - 1] = (30.0, -40.0), 0
    ft, mt = _t(flow, dev), _t(mask, dev)
    norm = vr.flow_maxrad(flow, mask)
    assert norm[-1] == 50.0 and _same_bits(viz.flow_maxrad(ft, mt).cpu().numpy(), norm)
    got = viz.flow_to_color(ft, mask=mt).cpu().numpy()
    want = vr.flow_to_color(flow, norm, mask)
    worst = max(int(np.abs(got[b].astype(np.int16) - want[b].astype(np.int16)).max()) for b in range(B))
    assert worst <= 1 and not got[mask != 0].any() and got[-1, H - 1, W - 1].any()
    del got, want
    mean, count = viz.decimate_flow(ft, 1, mt)
    want_mean, want_count = vr.flow_decimate_planes(flow, 1, mask)           # pinned to vr.flow_decimate's loops by tests/test_viz.py
    assert _same_bits(count.cpu().numpy(), want_count) and _same_bits(mean.cpu().numpy(), want_mean)
    assert (want_count == 0).any() and want_count[-1, H - 1, W - 1] == 1
    del mean, count, want_mean, want_count, ft, flow
    custom = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    for dtype in (np.float32, np.float64):
        field = rng.normal(0, 1, (B, H, W)).astype(dtype)
        field.reshape(-1)[::13] = np.nan
        field[-1, H - 1, W - 3:] = (-1.5, 9.0, 1.5 - 3 / 256)
        got = viz.scalar_to_color(_t(field, dev), -1.5, 1.5, custom, mask=mt, bad=(255, 0, 255)).cpu().numpy()
        assert np.array_equal(got, vr.scalar_to_color(field, -1.5, 1.5, custom, mask, (255, 0, 255))), dtype


def test_flow_to_color_exact_cases(dev, cases):
    """Where no rounding of the arctangent can show: equal to the reference's bytes."""
    for tag in ("signed_zeros", "zeros"):
        for wheel in ("interp", "original"):
            got = viz.flow_to_color(_t(_nchw(cases[f"{tag}_flow"]), dev), wheel=wheel, order="bgr")[0].cpu().numpy()
            assert np.array_equal(got, cases[f"{tag}_bgr_{wheel}"]), (tag, wheel, got.tolist())
    got = viz.flow_to_color(_t(_nchw(cases["signed_zeros_flow"]), dev), order="rgb")[0].cpu().numpy()
    assert got.tolist() == [[[255, 0, 0], [255, 0, 42], [0, 208, 255], [255, 255, 255]]]
    # axis-aligned and diagonal unit vectors, at full and half length
    unit = np.array([[[1, 0], [0, 1], [-1, 0], [0, -1], [0.5, 0], [0, 0.5], [-0.5, 0], [0, -0.5], [1, -0.0], [-0.0, 1]]], np.float32)
    flow = _nchw(unit)
    for wheel in ("interp", "original"):
        got = viz.flow_to_color(_t(flow, dev), maxmotion=1.0, wheel=wheel).cpu().numpy()
        assert np.array_equal(got, vr.flow_to_color(flow, [1.0], None, wheel)), (wheel, got.tolist())
    # the pixel that carries the maximum: just above 1 (darkened by 0.75) and exactly 1
    for tag in [t for t in cases["cases"] if t.startswith("max_")]:
        hw2 = cases[f"{tag}_flow"]
        at = np.unravel_index(np.argmax(hw2[..., 0] ** 2 + hw2[..., 1] ** 2), hw2.shape[:2])
        for wheel in ("interp", "original"):
            got = viz.flow_to_color(_t(_nchw(hw2), dev), wheel=wheel, order="bgr")[0].cpu().numpy()
            want = cases[f"{tag}_bgr_{wheel}"]
            assert np.array_equal(got[at], want[at]), (tag, wheel, got[at], want[at])
            assert np.abs(got.astype(int) - want.astype(int)).max() <= 1, (tag, wheel)
        assert (want[at].max() <= 191) == tag.startswith("max_above")
    # unknown and masked vectors are black and stay out of the normaliser
    flow = _nchw(cases["odd13x17_flow"]).copy()
    ref = viz.flow_to_color(_t(flow, dev)).cpu().numpy()
    flow[0, :, 3, 4], flow[0, 0, 5, 6], flow[0, 1, 0, 0], flow[0, 1, 12, 16] = 0.0, np.nan, 1e10, -np.inf
    mask = np.zeros((1, 13, 17), np.uint8)
    mask[0, 3, 4] = 2
    got = viz.flow_to_color(_t(flow, dev), mask=_t(mask, dev)).cpu().numpy()
    out = np.zeros((13, 17), bool)
    for y, x in ((3, 4), (5, 6), (0, 0), (12, 16)):
        out[y, x] = True
    assert not got[0][out].any() and np.array_equal(got[0][~out], ref[0][~out])
    assert np.abs(got.astype(int) - vr.flow_to_color(flow, vr.flow_maxrad(flow, mask), mask).astype(int)).max() <= 1


def _compare(got_bgr, want_bgr, fk, wheel, tag, share_bound=True):
    """Within one level everywhere; the share of values that differ at all at most 0.5 % (`share_bound`: not for the pictures of a
    few pixels, where one value is more than that).  Original wheel: pixels whose fk lies within 2^-16 of an integer may sit on the
    other side of it and are left out, at most 0.1 % of them."""
    assert got_bgr.shape == want_bgr.shape and got_bgr.dtype == np.uint8
    diff = np.abs(got_bgr.astype(int) - want_bgr.astype(int))
    left_out = 0.0
    if wheel == "original":
        near = np.abs(fk.astype(np.float64) - np.rint(fk.astype(np.float64))) < 2.0 ** -16
        left_out = float(near.mean())
        assert left_out <= 1e-3 or not share_bound, (tag, left_out)
        diff = diff[~near]
    share = float((diff != 0).mean()) if diff.size else 0.0
    print(f"{tag} {wheel}: {share:.5%} of {diff.size} values differ, largest difference {diff.max() if diff.size else 0}, "
          f"{left_out:.5%} of the pixels left out")
    assert diff.max() <= 1, (tag, wheel, int(diff.max()))
    assert share <= 0.005 or not share_bound, (tag, wheel, share)


def test_flow_to_color_matches_the_reference_pictures(dev, cases):
    tags = ("odd13x17", "odd13x17_maxmotion2", "random32x48", "random32x48_maxmotion5", "sequence3", "dns_crop", "w3", "w5", "w7",
            "px1x1", "row1x9", "col9x1")
    for tag in tags:
        flow = _nchw(cases[f"{tag}_flow"])
        big = flow[:, 0].size >= 180                    # the random and DNS cases: one differing value stays below the bound
        mm = float(cases[f"{tag}_maxmotion"])
        mm = None if np.isnan(mm) else mm
        n = np.float32(mm) if mm is not None else vr.flow_maxrad(flow).max()
        _, fk = vr.flow_fk(flow, np.full(len(flow), n, np.float32))
        for wheel in ("interp", "original"):
            want = cases[f"{tag}_bgr_{wheel}"].reshape((-1,) + flow.shape[2:] + (3,))
            for order in ("bgr", "rgb"):
                got = viz.flow_to_color(_t(flow, dev), mm, scope="batch", wheel=wheel, order=order).cpu().numpy()
                _compare(got if order == "bgr" else got[..., ::-1], want, fk, wheel, f"{tag} batch {order}", big)
            if len(flow) == 1:                          # one field: its own maximum is the batch's
                got = viz.flow_to_color(_t(flow, dev), mm, scope="image", wheel=wheel, order="bgr").cpu().numpy()
                _compare(got, want, fk, wheel, f"{tag} image bgr", big)
    # scope "image" inside a batch: every field as if it were alone
    pair = np.concatenate([_nchw(cases["random32x48_flow"]), _nchw(cases["random32x48_maxmotion5_flow"]) * np.float32(0.5)])
    got = viz.flow_to_color(_t(pair, dev), scope="image", order="bgr").cpu().numpy()
    _, fk = vr.flow_fk(pair[:1], vr.flow_maxrad(pair[:1]))
    _compare(got[:1], cases["random32x48_bgr_interp"][None], fk, "interp", "random32x48 image-in-batch")
    assert np.array_equal(got[1], viz.flow_to_color(_t(pair[1:], dev), order="bgr")[0].cpu().numpy())
    # the numpy drop-in: the reference's shapes and channel order
    seq = cases["sequence3_flow"]
    out = viz.motion_to_color(seq)
    assert out.shape == seq.shape[:-1] + (3,) and out.dtype == np.uint8
    assert np.array_equal(out, viz.flow_to_color(_t(_nchw(seq), dev), scope="batch", order="bgr").cpu().numpy())
    one = viz.motion_to_color(seq[1], maxmotion=2.0, original_color=True)
    assert one.shape == seq.shape[1:-1] + (3,)
    assert np.array_equal(one, viz.flow_to_color(_t(_nchw(seq[1]), dev), 2.0, wheel="original", order="bgr")[0].cpu().numpy())


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_scalar_to_color_matches_restatement(dev, B, H, W):
    rng = np.random.default_rng(B * 31 + H * 7 + W)
    custom = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    mask = (rng.random((B, H, W)) < 0.1).astype(np.uint8)
    for dtype in (np.float32, np.float64):
        field = rng.normal(0, 1, (B, H, W)).astype(dtype)
        flat = field.reshape(-1)
        ends = (-1.5, 1.5, -1.5 + 3 / 256, 1.5 - 3 / 256, np.nextafter(dtype(1.5), dtype(0)), -9.0, 9.0, np.nan, np.inf, -np.inf, 0.0, -0.0)
        for j in range(min(len(ends), flat.size)):
            flat[(j * 5) % flat.size] = ends[j]
        ft = _t(field, dev)
        for cmap, lut in (("bwr", viz.LUTS["bwr"]), ("gray", viz.LUTS["gray"]), (custom, custom)):
            got = viz.scalar_to_color(ft, -1.5, 1.5, cmap, bad=(1, 2, 3)).cpu().numpy()
            assert np.array_equal(got, vr.scalar_to_color(field, -1.5, 1.5, lut, bad=(1, 2, 3))), (dtype, H, W)
        got = viz.scalar_to_color(ft, -1.5, 1.5, custom, mask=_t(mask, dev), bad=(255, 0, 255)).cpu().numpy()
        assert np.array_equal(got, vr.scalar_to_color(field, -1.5, 1.5, custom, mask, (255, 0, 255)))
        got = viz.scalar_to_color(ft, 0.25, -0.75, "gray").cpu().numpy()                         # a reversed range
        assert np.array_equal(got, vr.scalar_to_color(field, 0.25, -0.75, viz.LUTS["gray"]))
        # symmetric: a fixed range, and every image's own largest finite magnitude
        got = viz.scalar_to_color(ft, vmax=0.5, symmetric=True).cpu().numpy()
        assert np.array_equal(got, vr.scalar_to_color(field, -0.5, 0.5, viz.LUTS["bwr"]))
        got = viz.scalar_to_color(ft, symmetric=True, mask=_t(mask, dev)).cpu().numpy()
        for b, m in enumerate(vr.field_absmax(field, mask)):
            m = m or 1.0
            assert np.array_equal(got[b], vr.scalar_to_color(field[b:b + 1], -m, m, viz.LUTS["bwr"], mask[b:b + 1])[0]), (dtype, b)
    with pytest.raises(ValueError):
        viz.scalar_to_color(ft, 1.0, 1.0)
    with pytest.raises(ValueError):
        viz.scalar_to_color(ft)


def _picture_buffer(npix, dev, flush):
    """3 * npix bytes inside a guarded buffer of whole words pre-filled with the sentinel pattern: at its start (4-byte aligned, up
    to 3 spare bytes behind it) or, `flush`, ending against the back guard (then misaligned unless 3 * npix is a multiple of 4)."""
    nbytes = 3 * npix
    whole = guarded((-(-nbytes // 4) * 4,), torch.uint8, dev, "sentinel")
    before = whole.clone()
    off = whole.numel() - nbytes if flush else 0
    return whole, before, off, whole[off:off + nbytes]


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (1, 3, 3), (1, 2, 5), (3, 3, 7), (1, 9, 1), (2, 13, 17), (4, 4, 4), (2, 5, 6), (1, 67, 131)])
def test_guarded_buffers(dev, B, H, W):
    """Every output between guards, pre-filled; the flow's last element against its back guard.  The packed-dword stores of the
    pictures write 3 * B*H*W bytes and not one more, aligned or not, and every byte of them."""
    rng = np.random.default_rng(B * 1000 + H * 10 + W)
    src, mask_h = _holes(rng, B, H, W)
    flow = guarded((B, 2, H, W), torch.float32, dev, "nan")
    flow.copy_(_t(src, dev))
    mask = _t(mask_h, dev)
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    npix = B * H * W
    norm = guarded((B,), torch.float32, dev, "sentinel")
    _lib.check(lib.pivlfn_flow_maxrad(flow.data_ptr(), mask.data_ptr(), norm.data_ptr(), B, H, W, st), "maxrad")
    torch.cuda.synchronize()
    check_guards(norm, "maxrad")
    check_guards(flow, "flow after maxrad")
    assert _same_bits(norm.cpu().numpy(), vr.flow_maxrad(src, mask_h))
    want = vr.flow_to_color(src, vr.flow_maxrad(src, mask_h), mask_h)
    field = rng.normal(0, 1, (B, H, W))
    lut = _t(viz.LUTS["bwr"], dev)
    for flush in (False, True):
        whole, before, off, out = _picture_buffer(npix, dev, flush)
        _lib.check(lib.pivlfn_flow_to_color(flow.data_ptr(), norm.data_ptr(), mask.data_ptr(), out.data_ptr(), B, H, W, 0, 0, st), "color")
        torch.cuda.synchronize()
        tag = f"flow_to_color {B}x{H}x{W} flush={flush}"
        check_guards(whole, tag)
        check_guards(flow, tag + " flow")
        spare = torch.ones(whole.numel(), dtype=torch.bool, device=dev)
        spare[off:off + 3 * npix] = False
        assert torch.equal(whole[spare], before[spare]), tag + ": a byte outside the picture changed"
        got = out.view(B, H, W, 3).cpu().numpy()
        assert np.abs(got.astype(int) - want.astype(int)).max() <= 1, tag
        for dtype in (torch.float32, torch.float64):
            fg = guarded((B, H, W), dtype, dev, "nan")
            fg.copy_(_t(field, dev).to(dtype))
            whole, before, off, out = _picture_buffer(npix, dev, flush)
            _lib.check(lib.pivlfn_scalar_to_color(fg.data_ptr(), int(dtype == torch.float64), mask.data_ptr(), lut.data_ptr(),
                                                  out.data_ptr(), B, H, W, -2.0, 2.0, 0x0A0B0C, st), "scalar")
            torch.cuda.synchronize()
            tag = f"scalar_to_color {dtype} {B}x{H}x{W} flush={flush}"
            check_guards(whole, tag)
            check_guards(fg, tag + " field")
            assert torch.equal(whole[spare], before[spare]), tag + ": a byte outside the picture changed"
            assert np.array_equal(out.view(B, H, W, 3).cpu().numpy(),
                                  vr.scalar_to_color(fg.cpu().numpy(), -2.0, 2.0, viz.LUTS["bwr"], mask_h, (10, 11, 12))), tag
            amax = guarded((B,), torch.float64, dev, "sentinel")
            _lib.check(lib.pivlfn_field_absmax(fg.data_ptr(), int(dtype == torch.float64), None, amax.data_ptr(), B, H, W, st), "absmax")
            torch.cuda.synchronize()
            check_guards(amax, "absmax")
            assert _same_bits(amax.cpu().numpy(), vr.field_absmax(fg.cpu().numpy()))
    for cell in (1, 4, 5):
        ch, cw = -(-H // cell), -(-W // cell)
        mean = guarded((B, 2, ch, cw), torch.float32, dev, "sentinel")
        count = guarded((B, ch, cw), torch.int32, dev, "sentinel")
        _lib.check(lib.pivlfn_flow_decimate(flow.data_ptr(), mask.data_ptr(), mean.data_ptr(), count.data_ptr(), B, H, W, cell, st), "decimate")
        torch.cuda.synchronize()
        check_guards(mean, f"decimate mean cell {cell}")
        check_guards(count, f"decimate count cell {cell}")
        check_guards(flow, "flow after decimate")
        want_mean, want_count = vr.flow_decimate(src, cell, mask_h)
        assert _same_bits(mean.cpu().numpy(), want_mean) and _same_bits(count.cpu().numpy(), want_count), cell


def test_vorticity_legend_and_quiver(dev, tmp_path):
    from pivlfn.postpro import flow_fields
    flow = read_flow(os.path.join(GOLD, "DNS_turbulence_out.flo"))[:64, :96]
    t = _t(_nchw(flow), dev).repeat(2, 1, 1, 1)
    t[1] *= 3.0
    vort = flow_fields(t, 0.5)[:, 0].cpu().numpy()
    got = viz.vorticity_image(t, 0.5).cpu().numpy()
    for b in range(2):
        m = float(np.abs(vort[b]).max())
        assert np.array_equal(got[b], vr.scalar_to_color(vort[b:b + 1], -m, m, viz.LUTS["bwr"])[0])
    got = viz.vorticity_image(t, 0.5, vmax=0.25, cmap="gray").cpu().numpy()
    assert np.array_equal(got, vr.scalar_to_color(vort, -0.25, 0.25, viz.LUTS["gray"]))
    wheel = viz.color_wheel_image(65, device=dev).cpu().numpy()
    assert wheel.shape == (65, 65, 3) and wheel[32, 32].tolist() == [255, 255, 255] and wheel[0, 0].tolist() == [255, 255, 255]
    assert wheel[32, 64].tolist() == [255, 0, 0] and wheel[32, 0].tolist() == [0, 208, 255]      # +x red, -x cyan-blue, full saturation
    assert not np.array_equal(wheel, viz.color_wheel_image(65, "original", device=dev).cpu().numpy())
    path = tmp_path / "q.png"
    viz.quiver_plot(flow, filename=str(path), cell=8)
    viz.quiver_plot(flow, coord=np.stack(np.meshgrid(np.arange(96.0), np.arange(64.0)), axis=-1), filename=str(path), norm=True)
    assert path.stat().st_size > 1000
    with pytest.raises(ValueError, match=".png"):
        viz.quiver_plot(flow, filename="q.jpg")


def test_run_py_pictures(tmp_path, dev):
    """run.py -p on three synthetic 64 x 96 pairs with --validate mask --color --vort-image: the .flo files are those of a run without
    the picture flags, byte for byte; every PNG decodes to exactly flow_to_color / vorticity_image of that pair's flow with its flags
    as the mask (the flags are where the .flo holds 1e10); the legend is written; the same with a fixed --color-max / --vort-max."""
    import PIL.Image
    import run as runpy
    from pivlfn import validate as V
    from pivlfn.pipeline import read_image_u8, u8_to_input
    H, W = 64, 96
    seq = tmp_path / "seq"
    seq.mkdir()
    names = [f"p{k}" for k in range(3)]
    for k, name in enumerate(names):
        a, b, _ = synth.particle_pair(H, W, 900 + k)
        PIL.Image.fromarray(a).save(str(seq / f"{name}_img1.png"))
        PIL.Image.fromarray(b).save(str(seq / f"{name}_img2.png"))
    net = pivlfn.Network(model="piv", params=synth.generate_weights("piv", 0)).to(dev).eval()
    fr = [[torch.from_numpy(np.stack([read_image_u8(str(seq / f"{n}_img{j}.png")) for n in part])).to(dev) for j in (1, 2)]
          for part in (names[:2], names[2:])]                                             # the batches of --batch 2
    est = torch.cat([pivlfn.estimate(net, u8_to_input(a), u8_to_input(b), tensor=True) for a, b in fr])
    res = V.validate_flow(est, radius=2, spacing=1, eps=0.01, thresh=0.5, mode="mask")
    assert 0.0 < float((res.flag != 0).float().mean()) < 0.9

    def png(path):
        im = PIL.Image.open(path)
        assert im.mode == "RGB"
        return np.array(im)

    base = ["--model", "piv", "-i", str(seq), "-p", "--batch", "2", "--validate", "mask", "--validate-radius", "2", "--validate-eps",
            "0.01", "--validate-thresh", "0.5"]
    assert runpy.main(base + ["-o", str(tmp_path / "plain")]) == 3
    assert runpy.main(base + ["-o", str(tmp_path / "pics"), "--color", "--vort-image"]) == 3
    assert runpy.main(base + ["-o", str(tmp_path / "fixed"), "--color", "--color-max", "4", "--vort-image", "--vort-max", "0.5",
                              "--color-wheel", "original"]) == 3
    plain, pics, fixed = (tmp_path / d / "piv-synthetic" / "seq" for d in ("plain", "pics", "fixed"))
    assert not [ln for ln in open(plain / "args.txt") if ln.split(":")[0] in runpy.VIZ_FLAGS]
    assert not list((plain / "flow").glob("*.png"))
    assert [ln for ln in open(pics / "args.txt") if ln.split(":")[0] not in runpy.VIZ_FLAGS + ("output",)] == \
        [ln for ln in open(plain / "args.txt") if not ln.startswith("output")]
    assert "color: True\n" in list(open(pics / "args.txt")) and "color_max: 4.0\n" in list(open(fixed / "args.txt"))
    for out, cmax, vmax, wheel in ((pics, None, None, "interp"), (fixed, 4.0, 0.5, "original")):
        assert (out / "flow" / "color_wheel.png").exists()
        assert np.array_equal(png(out / "flow" / "color_wheel.png"), viz.color_wheel_image(wheel=wheel, device=dev).cpu().numpy())
        assert sorted(p.name for p in (out / "flow").glob("*.png")) == sorted(
            ["color_wheel.png"] + [f"{n}_out.png" for n in names] + [f"{n}_vort.png" for n in names])
        for k, n in enumerate(names):
            data = open(out / "flow" / f"{n}_out.flo", "rb").read()
            assert data == open(plain / "flow" / f"{n}_out.flo", "rb").read(), n
            flo = _t(_nchw(read_flow(str(out / "flow" / f"{n}_out.flo"))), dev)
            flags = res.flag[k:k + 1]
            assert torch.equal(torch.from_numpy(vr.unknown(flo.cpu().numpy())).to(dev), flags != 0)
            want = viz.flow_to_color(flo, cmax, wheel=wheel, mask=flags)[0].cpu().numpy()
            got = png(out / "flow" / f"{n}_out.png")
            assert np.array_equal(got, want), n
            assert not got[(flags[0] != 0).cpu().numpy()].any() and got[(flags[0] == 0).cpu().numpy()].any()
            assert np.array_equal(want, viz.flow_to_color(est[k:k + 1], cmax, wheel=wheel, mask=flags)[0].cpu().numpy())
            # the vorticity is taken from the flow before the rejected vectors were overwritten with 1e10
            want = viz.vorticity_image(est[k:k + 1], vmax=vmax, mask=flags)[0].cpu().numpy()
            assert np.array_equal(png(out / "flow" / f"{n}_vort.png"), want), n
