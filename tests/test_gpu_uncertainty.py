"""GPU: pivlfn_flow_uncertainty and pivlfn_uncertainty_accumulate (csrc/uncertainty.hip) against the numpy restatement of their contract
(tests/uncertainty_restatement.py): the flag bytes bit for bit, NaN where and only where the restatement has it, ux and uy within
1e-6 * max(1, u).  The only operation of the contract that is not correctly rounded is the fp64 logarithm: a few ulp of it against a
denominator at or below -2e-6 is a relative error of about 1e-8 before the rounding to float32.  No pixel is left out of any
comparison.  Then batch independence, the capped pixel grids, guarded and poisoned buffers, a side stream, UncertaintyStats and
run.py --uncertainty."""
import json

import numpy as np
import pytest
import torch

import analysis_plans as ap
import quality_restatement as qr
import uncertainty_restatement as ur
from guarded import check_guards, guarded, same_bits
from uncertainty_restatement import CENTRE_OUT, FEW, FLAT, NO_PEAK, NO_VARIANCE, UNUSABLE

pytestmark = pytest.mark.gpu

ALL_BITS = FEW | FLAT | NO_PEAK | NO_VARIANCE | CENTRE_OUT
WORST = {"abs": 0.0, "rel": 0.0}


def _run(dev, img1, img2, flow, radius, lag, mask=None, **kw):
    from pivlfn import flow_uncertainty
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    unc = flow_uncertainty(t(img1), t(img2), t(flow), radius, lag, t(mask), **kw)
    assert unc.u.dtype == torch.float32 and unc.flag.dtype == torch.uint8
    assert unc.u.shape == flow.shape and unc.flag.shape == (flow.shape[0],) + flow.shape[2:]
    return unc.u.cpu().numpy(), unc.flag.cpu().numpy()


def _compare(got, want, what):
    """Every pixel: flags equal, NaN where and only where a bit of UNUSABLE is set, |u - restatement| <= 1e-6 max(1, u)."""
    u, flag = got
    wu, wflag = want
    assert np.array_equal(flag, wflag), f"{what}: {np.count_nonzero(flag != wflag)} flag bytes differ, first {np.argwhere(flag != wflag)[0]}"
    assert np.array_equal(np.isnan(u), np.isnan(wu)), what
    assert np.array_equal(np.isnan(wu), np.broadcast_to(((wflag & UNUSABLE) != 0)[:, None], wu.shape)), what
    ok = ~np.isnan(wu)
    err = np.abs(u[ok].astype(np.float64) - wu[ok].astype(np.float64))
    bound = 1e-6 * np.maximum(1.0, wu[ok].astype(np.float64))
    rel = err / np.maximum(wu[ok].astype(np.float64), 1e-300)
    if err.size:
        WORST["abs"], WORST["rel"] = max(WORST["abs"], float(err.max())), max(WORST["rel"], float(rel.max()))
    print(f"{what}: largest |u - restatement| = {err.max() if err.size else 0.0:.3g} px (relative {rel.max() if err.size else 0.0:.3g}) over "
          f"{np.count_nonzero((wflag & UNUSABLE) == 0)} usable pixels; largest so far {WORST['abs']:.3g} px, relative {WORST['rel']:.3g}")
    assert np.all(err <= bound), f"{what}: u off by {err.max():.3g} px"
    assert not np.signbit(u[ok]).any(), what


def _case(B, H, W, C, seed, r=2, kind="particles"):
    """Particle (or noise) images, a wild flow whose first pair keeps a clean left half at the true flow, one all-constant patch in both
    images that holds whole windows of high-passed zeros (up to r = 4)."""
    if kind == "noise":
        img1, img2 = qr.noise_images(B, H, W, C, seed)
        true = np.zeros((B, 2, H, W), np.float32)
    else:
        img1, img2, true = qr.particle_images(B, H, W, C, seed)
    flow = qr.wild_flow(B, H, W, seed + 1)
    half = max(W // 2, 1)
    flow[0, :, 1:, 1:half] = true[0, :, 1:, 1:half]
    if H >= 12 and W >= 12:
        qr.flatten_patch(img1, img2, 2, 2, size=min(4 * r + 1, 17))
    return img1, img2, flow


@pytest.mark.parametrize("lag", [0, 2])
@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (5, 3)])
def test_windows_larger_than_the_image(H, W, r, lag, dev):
    """Every box is clipped on every side at once; min_count 2 so that not every pixel is FEW."""
    seen = 0
    for C, kind in ((1, "noise"), (3, "particles")):
        img1, img2, flow = _case(2, H, W, C, 40 + H + W, r, kind)
        flow[1, 0], flow[1, 1] = (0.25 if W > 1 else 0.0), (0.25 if H > 1 else 0.0)
        mask = qr.speckle_mask(2, H, W, 7, 1)
        for m, mc in ((None, 2), (mask, None)):
            want = ur.batch_uncertainty(img1, img2, flow, r, lag, m, min_count=mc)
            _compare(_run(dev, img1, img2, flow, r, lag, m, min_count=mc), want, f"{H}x{W} r={r} lag={lag} C={C}")
            seen |= int(np.bitwise_or.reduce(want[1], axis=None))
    assert seen & FEW and seen & CENTRE_OUT


@pytest.mark.parametrize("lag", [0, 2, 4])
@pytest.mark.parametrize("r", [1, 4, 15])
def test_odd_sizes_against_the_restatement(r, lag, dev):
    """37 x 53, B = 3: no multiple of the tile, several tiles per image, a halo wider than the tile at r = 15.  The masked block is
    larger than the window (FEW), the constant patch holds whole windows up to r = 4 (FLAT), the wild flow has NaN, inf and 1e10
    (CENTRE_OUT), and the last pair is one image twice with a zero flow: a' = b', every d is exactly zero and so is V (NO_VARIANCE,
    at every lag and radius).  Every bit is seen in every case.  A 31 x 31 window does not fit into a flat patch of a 37 x 53 image:
    at r = 15 FLAT is reached by a second call with a floor of 0.9."""
    B, H, W = 3, 37, 53
    C = 1 if lag == 2 else 3
    img1, img2, flow = _case(B, H, W, C, 100 + r, r)
    img2[2], flow[2] = img1[2], 0.0
    mask = qr.speckle_mask(B, H, W, 9, min(2 * r + 4, 20))
    want = ur.batch_uncertainty(img1, img2, flow, r, lag, mask)
    _compare(_run(dev, img1, img2, flow, r, lag, mask), want, f"37x53 r={r} lag={lag} C={C}")
    seen = int(np.bitwise_or.reduce(want[1], axis=None))
    assert np.any((want[1] & UNUSABLE) == 0), "no usable pixel in the expected values"
    if r == 15:
        flat = ur.batch_uncertainty(img1, img2, flow, r, lag, mask, floor=0.9)
        _compare(_run(dev, img1, img2, flow, r, lag, mask, floor=0.9), flat, f"37x53 r={r} lag={lag} floor=0.9")
        seen |= int(np.bitwise_or.reduce(flat[1], axis=None))
    assert seen == ALL_BITS, f"bits seen: {seen:#x}"


def test_every_bit_in_one_call(dev):
    """r = 2, lag = 2 on noisy particle pairs at their true shift: all five bits and a good share of usable vectors in one call."""
    B, H, W, r, lag = 2, 37, 53, 2, 2
    pairs = [ur.noisy_particle_pair(H, W, (0.3, -0.2), 0.05, 20 + b) for b in range(B)]
    img1, img2 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    qr.flatten_patch(img1, img2, 2, 2, size=9)
    flow = np.zeros((B, 2, H, W), np.float32)
    flow[:, 0], flow[:, 1] = 0.3, -0.2
    flow[:, 0, :, W - 1] = 30.0
    flow[1, 1, 7, 9] = np.nan
    mask = qr.speckle_mask(B, H, W, 5, 8)
    want = ur.batch_uncertainty(img1, img2, flow, r, lag, mask)
    _compare(_run(dev, img1, img2, flow, r, lag, mask), want, "noisy pairs r=2 lag=2")
    assert int(np.bitwise_or.reduce(want[1], axis=None)) == ALL_BITS
    assert np.count_nonzero((want[1] & UNUSABLE) == 0) > 0.2 * want[1].size


def test_wide_image_largest_radius_and_lag(dev):
    B, H, W, r, lag = 1, 70, 131, 15, 4
    img1, img2, flow = _case(B, H, W, 1, 300, r)
    mask = qr.speckle_mask(B, H, W, 11, 34)
    want = ur.batch_uncertainty(img1, img2, flow, r, lag, mask)
    _compare(_run(dev, img1, img2, flow, r, lag, mask), want, "70x131 r=15 lag=4")
    assert np.any((want[1] & UNUSABLE) == 0) and np.any(want[1] & FEW)


def test_noise_images_with_terms_of_both_signs(dev):
    B, H, W, r, lag = 2, 37, 53, 4, 1
    img1, img2, flow = _case(B, H, W, 3, 400, r, "noise")
    flow[1] = 0.0
    img2[1] = img1[1] + np.float32(0.05) * img2[1]            # a pair that does correlate
    mask = qr.speckle_mask(B, H, W, 13, 12)
    for floor in (1.0 / 255.0, 0.0, 0.9):
        want = ur.batch_uncertainty(img1, img2, flow, r, lag, mask, floor=floor)
        _compare(_run(dev, img1, img2, flow, r, lag, mask, floor=floor), want, f"noise floor={floor:.3g}")
        if floor == 0.9:
            assert np.any(want[1] & FLAT)


def test_a_batch_equals_its_pairs_one_at_a_time(dev):
    from pivlfn import flow_uncertainty
    B, H, W, r, lag = 3, 37, 53, 4, 2
    img1, img2, flow = _case(B, H, W, 3, 500, r)
    mask = qr.speckle_mask(B, H, W, 15, 12)
    i1, i2, fl, mk = (torch.from_numpy(x).to(dev) for x in (img1, img2, flow, mask))
    whole = flow_uncertainty(i1, i2, fl, r, lag, mk)
    again = flow_uncertainty(i1, i2, fl, r, lag, mk)
    for b in range(B):
        one = flow_uncertainty(i1[b:b + 1], i2[b:b + 1], fl[b:b + 1], r, lag, mk[b:b + 1])
        assert same_bits(one.u, whole.u[b:b + 1]) and torch.equal(one.flag, whole.flag[b:b + 1]), b
    assert same_bits(again.u, whole.u) and torch.equal(again.flag, whole.flag)
    mag = whole.magnitude()
    assert mag.shape == whole.flag.shape and same_bits(mag, whole.u.pow(2).sum(1).sqrt())
    s = whole.summary()[0]
    ok = (whole.flag[0] & UNUSABLE) == 0
    assert s["n"] == int(ok.sum()) and abs(s["rms_ux"] - float(whole.u[0, 0][ok].double().pow(2).mean().sqrt())) < 1e-12


CAPPED_CASES = [(260, 130, 128, 2, 1)]          # (B, H, W, radius, lag): 65 blocks a frame, capped at 64


@pytest.mark.parametrize("B,H,W,r,lag", CAPPED_CASES)
def test_bits_where_the_pixel_grids_are_capped(B, H, W, r, lag, dev):
    """The warp and the fields kernel have at most max(16384 / B, 64) workgroups a pair and stride over the rest: 260 pairs of 130 x 128
    are 65 blocks of 256 pixels on a grid of 64.  Eight particle pairs, each shifted along x by another number of columns for every
    further pair.  The first, the middle and the last pair against the restatement; sixteen pairs against the same pair in a call of
    its own, whose grid is not capped."""
    from pivlfn import flow_uncertainty
    import analysis_plans as ap
    plan = ap.capped_frame_grid(H * W, B)
    assert plan["blocks"] > plan["cap"] == plan["grid"]
    base = _case(8, H, W, 1, 700, r)
    img1, img2, flow = (np.stack([np.roll(x[b % 8], b // 8, axis=-1) for b in range(B)]) for x in base)
    mask = qr.speckle_mask(B, H, W, 9, 2 * r + 4)
    i1, i2, fl, mk = (torch.from_numpy(x).to(dev) for x in (img1, img2, flow, mask))
    whole = flow_uncertainty(i1, i2, fl, r, lag, mk)
    for b in sorted({0, B // 2, B - 1}):
        want = ur.batch_uncertainty(img1[b:b + 1], img2[b:b + 1], flow[b:b + 1], r, lag, mask[b:b + 1])
        _compare((whole.u[b:b + 1].cpu().numpy(), whole.flag[b:b + 1].cpu().numpy()), want, f"pair {b} of {B} x {H}x{W} r={r} lag={lag}")
    for b in [0, 1, 2, 63, 64, 65, 127, 128, 129, 130, 191, 192, 255, 256, 258, 259]:
        one = flow_uncertainty(i1[b:b + 1], i2[b:b + 1], fl[b:b + 1], r, lag, mk[b:b + 1])
        assert same_bits(one.u, whole.u[b:b + 1]) and torch.equal(one.flag, whole.flag[b:b + 1]), b


@pytest.mark.parametrize("B,H,W,r,lag", ap.shapes(ap.UNCERTAINTY_CASES))
def test_bits_where_the_frame_grid_is_capped(B, H, W, r, lag, dev):
    """The same capped grids against the same pairs in five calls that are not capped: every uncertainty and every flag byte."""
    from pivlfn import flow_uncertainty
    base = _case(8, H, W, 1, 900, r)
    img1, img2, flow = (np.stack([np.roll(x[b % 8], b // 8, axis=-1) for b in range(B)]) for x in base)
    mask = qr.speckle_mask(B, H, W, 9, 2 * r + 4)
    i1, i2, fl, mk = (torch.from_numpy(x).to(dev) for x in (img1, img2, flow, mask))
    whole = flow_uncertainty(i1, i2, fl, r, lag, mk)
    step = ap.FRAMES_PER_UNCAPPED_CALL
    parts = [flow_uncertainty(i1[k:k + step], i2[k:k + step], fl[k:k + step], r, lag, mk[k:k + step]) for k in range(0, B, step)]
    assert same_bits(whole.u, torch.cat([p.u for p in parts])) and torch.equal(whole.flag, torch.cat([p.flag for p in parts]))
    assert 0 < int(((whole.flag & UNUSABLE) == 0).sum()) < whole.flag.numel()


def _call(lib, ins, outs, ws, B, C, H, W, r, lag, stream, ws_bytes=None):
    i1, i2, fl, mk = ins
    return lib.pivlfn_flow_uncertainty(i1.data_ptr(), i2.data_ptr(), C, fl.data_ptr(), mk.data_ptr(), outs[0].data_ptr(),
                                       outs[1].data_ptr(), B, H, W, r, lag, ((2 * r + 1) ** 2 + 1) // 2, 1.0 / 255.0, ws.data_ptr(),
                                       ws.numel() if ws_bytes is None else ws_bytes, stream)


@pytest.mark.parametrize("r,lag", [(4, 2), (15, 4)])
def test_guarded_inputs_poisoned_outputs_dirty_workspace(r, lag, dev):
    """Inputs at the end of guarded allocations (a read past either end meets NaN guards), outputs pre-filled with NaN / 0xFF, a
    workspace full of 0xFF of exactly the size asked for: the result equals the plain call's bit for bit, every guard holds, and a
    workspace one byte smaller is refused."""
    from pivlfn import _lib, flow_uncertainty
    lib = _lib.load()
    B, C, H, W = 4, 3, 19, 23                       # B*H*W a multiple of 4: the byte buffers are whole 32-bit words
    img1, img2, flow = _case(B, H, W, C, 600 + r, r)
    mask = qr.speckle_mask(B, H, W, 17, 8)
    src = [torch.from_numpy(x).to(dev) for x in (img1, img2, flow, mask)]
    ref = flow_uncertainty(*src[:3], r, lag, src[3])
    ins = [guarded(t.shape, t.dtype, dev, "nan") for t in src]
    for t, s in zip(ins, src):
        t.copy_(s)
    unc = guarded((B, 2, H, W), torch.float32, dev, "sentinel")
    flag = guarded((B, H, W), torch.uint8, dev, "sentinel")
    flag.fill_(0xFF)
    need = lib.pivlfn_flow_uncertainty_workspace_bytes(B, H, W, r, lag)
    ws = guarded((need,), torch.uint8, dev, "sentinel")
    ws.fill_(0xFF)
    st = torch.cuda.current_stream(dev).cuda_stream
    with pytest.raises(ValueError, match="too small"):
        _lib.check(_call(lib, ins, (unc, flag), ws, B, C, H, W, r, lag, st, need - 1), "flow_uncertainty")
    assert bool((flag == 0xFF).all())               # refused before anything was launched
    _lib.check(_call(lib, ins, (unc, flag), ws, B, C, H, W, r, lag, st), "flow_uncertainty")
    torch.cuda.synchronize()
    assert same_bits(unc, ref.u) and torch.equal(flag, ref.flag)
    for t in ins + [unc, flag, ws]:
        check_guards(t, f"flow_uncertainty r={r} lag={lag}")
    for t, s in zip(ins, src):
        assert torch.equal(t.view(torch.uint8), s.view(torch.uint8)), "an input was written"
    # the accumulator: guarded sums that already hold a value, guarded inputs
    sums = guarded((3, H, W), torch.float64, dev, "sentinel")
    sums.fill_(0.5)
    _lib.check(lib.pivlfn_uncertainty_accumulate(unc.data_ptr(), flag.data_ptr(), sums.data_ptr(), B, H, W, st), "uncertainty_accumulate")
    torch.cuda.synchronize()
    want = ur.accumulate(np.full((3, H, W), 0.5), ref.u.cpu().numpy(), ref.flag.cpu().numpy())
    assert np.array_equal(sums.cpu().numpy().view(np.int64), want.view(np.int64))
    for t in (unc, flag, sums):
        check_guards(t, "uncertainty_accumulate")


def test_runs_in_order_on_the_stream_it_is_given(dev):
    """On a fresh stream, behind a bounded delay (a chain of matrix products) and the copy of the real inputs into buffers that hold
    the NaN poison, both calls are enqueued without any host synchronisation; their outputs equal the eager results bit for bit.  A
    launch on another stream would read the poison or leave the sentinel."""
    from pivlfn import _lib, flow_uncertainty
    lib = _lib.load()
    B, C, H, W, r, lag = 2, 1, 40, 56, 8, 2
    img1, img2, flow = _case(B, H, W, C, 700, r)
    src = [torch.from_numpy(x).to(dev) for x in (img1, img2, flow, qr.speckle_mask(B, H, W, 19, 10))]
    ref = flow_uncertainty(*src[:3], r, lag, src[3])
    ref_sums = ur.accumulate(np.zeros((3, H, W)), ref.u.cpu().numpy(), ref.flag.cpu().numpy())
    ins = [guarded(t.shape, t.dtype, dev, "nan") for t in src]
    unc = guarded((B, 2, H, W), torch.float32, dev, "sentinel")
    flag = guarded((B, H, W), torch.uint8, dev, "sentinel")
    sums = guarded((3, H, W), torch.float64, dev, "nan")
    ws = guarded((lib.pivlfn_flow_uncertainty_workspace_bytes(B, H, W, r, lag),), torch.uint8, dev, "nan")
    n = 8192
    a, b, c = torch.randn(n, n, device=dev), torch.randn(n, n, device=dev), torch.empty(n, n, device=dev)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        torch.mm(a, b, out=c)                           # the matrix product's own set-up happens here, not in the timed part
    torch.cuda.synchronize()
    delayed = torch.cuda.Event()
    with torch.cuda.stream(stream):
        for _ in range(10):                             # >= 1.1e13 flop in fp32: some tens of milliseconds
            torch.mm(a, b, out=c)
        delayed.record(stream)
        for t, s in zip(ins, src):
            t.copy_(s, non_blocking=True)
        sums.zero_()
        rc = _call(lib, ins, (unc, flag), ws, B, C, H, W, r, lag, stream.cuda_stream)
        rc2 = lib.pivlfn_uncertainty_accumulate(unc.data_ptr(), flag.data_ptr(), sums.data_ptr(), B, H, W, stream.cuda_stream)
        still_waiting = not delayed.query()             # the calls were enqueued while the delay was still running
    _lib.check(rc, "flow_uncertainty")
    _lib.check(rc2, "uncertainty_accumulate")
    stream.synchronize()
    assert still_waiting, "the delay ran out before the calls were enqueued: the test would not see a launch on another stream"
    assert same_bits(unc, ref.u) and torch.equal(flag, ref.flag)
    assert np.array_equal(sums.cpu().numpy().view(np.int64), ref_sums.view(np.int64))
    for t in ins + [unc, flag, ws, sums]:
        check_guards(t, "flow_uncertainty on a side stream")


def test_uncertainty_stats_against_the_restatement(dev):
    """Three pairs added as 1 + 2 and as 3 at once: the sums are those of the restatement bit for bit either way, result() is
    finalize() of them, save() writes them."""
    from pivlfn import FlowUncertainty, UncertaintyStats, flow_uncertainty
    B, H, W, r, lag = 3, 37, 53, 4, 2
    img1, img2, flow = _case(B, H, W, 1, 800, r)
    flow[1:, :, 1:, 1:W // 2] = flow[0, :, 1:, 1:W // 2]        # usable vectors in every pair, where the images are pair 0's
    img1[1:], img2[1:] = img1[0] * np.float32(0.9), img2[0] * np.float32(0.9)
    mask = qr.speckle_mask(B, H, W, 21, 12)
    i1, i2, fl, mk = (torch.from_numpy(x).to(dev) for x in (img1, img2, flow, mask))
    unc = flow_uncertainty(i1, i2, fl, r, lag, mk)
    want_u, want_flag = ur.batch_uncertainty(img1, img2, flow, r, lag, mask)
    _compare((unc.u.cpu().numpy(), unc.flag.cpu().numpy()), (want_u, want_flag), "stats input")
    split, whole = UncertaintyStats(H, W, dev), UncertaintyStats(H, W, dev)
    split.update(FlowUncertainty(unc.u[:1], unc.flag[:1]))
    split.update(FlowUncertainty(unc.u[1:], unc.flag[1:]))
    whole.update(unc)
    want = ur.accumulate(np.zeros((3, H, W)), unc.u.cpu().numpy(), unc.flag.cpu().numpy())
    assert want[2].max() == 3 and want[2].min() == 0
    for stats in (split, whole):
        assert stats.count == 3
        assert np.array_equal(stats.acc.cpu().numpy().view(np.int64), want.view(np.int64))
    res = whole.result()
    ref = UncertaintyStats.finalize(want, 3)
    for key in ("n", "noise_var_u", "noise_var_v", "mean_unc_u", "mean_unc_v"):
        assert np.array_equal(res[key], ref[key], equal_nan=True), key
    assert np.isnan(res["noise_var_u"][want[2] == 0]).all() and np.isfinite(res["mean_unc_v"][want[2] > 0]).all()
    with pytest.raises(ValueError, match="accumulators"):
        whole.update(FlowUncertainty(unc.u[:, :, :-1], unc.flag[:, :-1]))


def test_run_py_uncertainty(tmp_path, dev):
    """run.py -p --uncertainty 4 --uncertainty-lag 1 --uncertainty-image --stats --truth on three synthetic 64 x 64 pairs with seeded
    weights: every <name>_unc.flo holds the two bands of flow_uncertainty on the written flow and the frames the network was given,
    1e10 where a vector has none, bit for bit; uncertainty.json is strict JSON with one entry per pair, the run's totals and the
    coverage keys (their values are not judged: seeded weights give meaningless flows); uncertainty_stats.npz holds the sums of the
    three pairs; the PNGs exist at the frames' size.  Without --uncertainty no such file appears and the .flo files are the same."""
    import PIL.Image
    import run as runpy
    import pivlfn
    from pivlfn import synth
    from pivlfn import uncertainty as U
    from pivlfn.flo import read_flow, write_flow
    from pivlfn.pipeline import read_image_u8, u8_to_input
    H = W = 64
    seq, truth = tmp_path / "seq", tmp_path / "truth"
    seq.mkdir()
    truth.mkdir()
    names = [f"p{k}" for k in range(3)]
    for k, name in enumerate(names):
        a, b, f = synth.particle_pair(H, W, 960 + k)
        PIL.Image.fromarray(a).save(str(seq / f"{name}_img1.png"))
        PIL.Image.fromarray(b).save(str(seq / f"{name}_img2.png"))
        write_flow(np.ascontiguousarray(np.asarray(f, np.float32).transpose(1, 2, 0)), str(truth / f"{name}_flow.flo"))
    base = ["--model", "piv", "-i", str(seq), "-p", "--batch", "2", "--stats", "--truth", str(truth)]
    assert runpy.main(base + ["-o", str(tmp_path / "plain")]) == 3
    assert runpy.main(base + ["-o", str(tmp_path / "unc"), "--uncertainty", "4", "--uncertainty-lag", "1", "--uncertainty-image"]) == 3
    plain, out = (tmp_path / d / "piv-synthetic" / "seq" for d in ("plain", "unc"))
    assert not list(plain.rglob("*_unc.*")) and not list(plain.rglob("uncertainty*"))
    assert not [ln for ln in open(plain / "args.txt") if ln.startswith("uncertainty")]
    lines = list(open(out / "args.txt"))
    assert "uncertainty: 4\n" in lines and "uncertainty_lag: 1\n" in lines and "uncertainty_image: True\n" in lines

    def strict(token):
        raise AssertionError(f"uncertainty.json holds {token}")
    doc = json.load(open(out / "uncertainty.json"), parse_constant=strict)
    assert doc["radius"] == 4 and doc["lag"] == 1 and doc["min_count"] == 41 and doc["mask"] is None and sorted(doc["pairs"]) == names
    total_n, acc = 0, np.zeros((3, H, W))
    for n in names:
        data = open(out / "flow" / f"{n}_out.flo", "rb").read()
        assert data == open(plain / "flow" / f"{n}_out.flo", "rb").read(), n
        i1, i2 = (u8_to_input(torch.from_numpy(read_image_u8(str(seq / f"{n}_img{j}.png"))[None]).to(dev)) for j in (1, 2))
        flo = torch.from_numpy(read_flow(str(out / "flow" / f"{n}_out.flo"))).to(dev).permute(2, 0, 1)[None].contiguous()
        want = pivlfn.flow_uncertainty(i1, i2, flo, 4, 1)
        got = torch.from_numpy(read_flow(str(out / "flow" / f"{n}_unc.flo"))).to(dev)
        assert got.shape == (H, W, 2)
        none = ((want.flag[0] & UNUSABLE) != 0)[..., None].expand(H, W, 2)
        assert same_bits(got, torch.where(none, torch.full_like(got, 1e10), want.u[0].permute(1, 2, 0))), n
        (s,) = want.summary()
        for key, val in s.items():
            have = doc["pairs"][n][key]
            # counts are exact; the float64 sums behind the means may be reduced in another order in a batch of two
            assert have == val or (have is None and val != val) or abs(have - val) <= 1e-12 * abs(val), (n, key, have, val)
        for key in ("n_x", "n_y", "coverage_x", "coverage_y", "error_over_u_x", "error_over_u_y"):
            assert key in doc["pairs"][n] and key in doc["total"], key
        tr = torch.from_numpy(read_flow(str(truth / f"{n}_flow.flo"))).to(dev).permute(2, 0, 1)[None].contiguous()
        (c,) = U.uncertainty_coverage(flo, tr, want)
        assert doc["pairs"][n]["n_x"] == c["n_x"] and doc["pairs"][n]["n_y"] == c["n_y"]
        total_n += s["n"]
        acc = ur.accumulate(acc, want.u.cpu().numpy(), want.flag.cpu().numpy())
        im = PIL.Image.open(out / "flow" / f"{n}_unc.png")
        assert im.mode == "RGB" and im.size == (W, H)
    assert doc["total"]["n"] == total_n
    saved = np.load(out / "uncertainty_stats.npz")
    assert int(saved["count"]) == 3 and int(saved["radius"]) == 4 and int(saved["lag"]) == 1
    assert np.array_equal(saved["acc"].view(np.int64), acc.view(np.int64))
    assert (out / "stats.npz").exists() and (out / "errors.json").exists()


def test_run_py_uncertainty_two_ranks(tmp_path, dev):
    """run.py --uncertainty --truth launched as two ranks (fresh child processes, RANK / WORLD_SIZE in the environment, gloo for the
    exchange): rank 0 writes one uncertainty.json with the pairs of both ranks in pair order, each pair's summary and coverage counts
    equal to a direct call on the flow that was written, and the totals are the pairs' sums."""
    import os
    import socket
    import subprocess
    import sys
    import PIL.Image
    import pivlfn
    from pivlfn import synth
    from pivlfn import uncertainty as U
    from pivlfn.flo import read_flow, write_flow
    from pivlfn.pipeline import read_image_u8, u8_to_input
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    H = W = 64
    seq, truth = tmp_path / "seq", tmp_path / "truth"
    seq.mkdir()
    truth.mkdir()
    names = [f"p{k}" for k in range(3)]
    for k, name in enumerate(names):
        a, b, f = synth.particle_pair(H, W, 970 + k)
        PIL.Image.fromarray(a).save(str(seq / f"{name}_img1.png"))
        PIL.Image.fromarray(b).save(str(seq / f"{name}_img2.png"))
        write_flow(np.ascontiguousarray(np.asarray(f, np.float32).transpose(1, 2, 0)), str(truth / f"{name}_flow.flo"))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, os.path.join(root, "piv_liteflownet-pytorch_amd", "run.py"), "-m", "piv", "-i", str(seq), "-p", "-o",
           str(tmp_path / "out"), "--batch", "2", "--truth", str(truth), "--uncertainty", "4", "--uncertainty-lag", "1"]
    procs = [subprocess.Popen(cmd, env=dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                                            MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0"),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=root) for r in range(2)]
    outs = []
    for p in procs:
        try:
            o, e = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append((p.returncode, o, e))
    for rc, o, e in outs:
        assert rc == 0, f"child failed rc={rc}\nstdout:\n{o[-2000:]}\nstderr:\n{e[-4000:]}"
    out = tmp_path / "out" / "piv-synthetic" / "seq"
    doc = json.load(open(out / "uncertainty.json"))
    assert list(doc["pairs"]) == names and doc["radius"] == 4 and doc["lag"] == 1
    total = {"n": 0, "n_x": 0, "n_y": 0}
    for n in names:
        i1, i2 = (u8_to_input(torch.from_numpy(read_image_u8(str(seq / f"{n}_img{j}.png"))[None]).to(dev)) for j in (1, 2))
        flo = torch.from_numpy(read_flow(str(out / "flow" / f"{n}_out.flo"))).to(dev).permute(2, 0, 1)[None].contiguous()
        want = pivlfn.flow_uncertainty(i1, i2, flo, 4, 1)
        got = torch.from_numpy(read_flow(str(out / "flow" / f"{n}_unc.flo"))).to(dev)
        none = ((want.flag[0] & UNUSABLE) != 0)[..., None].expand(H, W, 2)
        assert same_bits(got, torch.where(none, torch.full_like(got, 1e10), want.u[0].permute(1, 2, 0))), n
        tr = torch.from_numpy(read_flow(str(truth / f"{n}_flow.flo"))).to(dev).permute(2, 0, 1)[None].contiguous()
        record = {**want.summary()[0], **U.uncertainty_coverage(flo, tr, want)[0]}
        assert doc["pairs"][n].keys() == record.keys()
        for key, val in record.items():
            have = doc["pairs"][n][key]
            assert have == val or (have is None and val != val) or abs(have - val) <= 1e-12 * abs(val), (n, key, have, val)
        for key in total:
            total[key] += record[key]
    assert {key: doc["total"][key] for key in total} == total
