"""GPU: pivlfn_match_quality (csrc/quality.hip) against the numpy restatement of its contract (tests/quality_restatement.py): the flag
bytes and the plane c bit for bit, NaN positions included; dx and dy within 1e-6 px.  The only operation of the contract that is not
correctly rounded is the fp64 logarithm: a few ulp, against a denominator of at least 1e-6 in magnitude and |d| <= 0.5, is about 1e-8
before the rounding to float32.  No pixel is left out of any comparison.  Then batch independence, guarded and poisoned buffers, a side
stream, the planted error of tests/test_quality.py on the device and run.py --quality."""
import json

import numpy as np
import pytest
import torch

import quality_restatement as qr
from guarded import check_guards, guarded, same_bits
from quality_restatement import CENTRE_OUT, FEW, FLAT, NO_PEAK

pytestmark = pytest.mark.gpu

ALL_BITS = FEW | FLAT | NO_PEAK | CENTRE_OUT


def _run(dev, img1, img2, flow, radius, mask=None, **kw):
    from pivlfn import match_quality
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    q = match_quality(t(img1), t(img2), t(flow), radius, t(mask), **kw)
    assert q.c.dtype == torch.float32 and q.residual.dtype == torch.float32 and q.flag.dtype == torch.uint8
    assert q.c.shape == q.flag.shape == (flow.shape[0],) + flow.shape[2:] and q.residual.shape == flow.shape
    assert q.residual.data_ptr() == q.c.data_ptr() + 4 * q.c[0].numel()              # views of the one [B,3,H,W] buffer
    return q.c.cpu().numpy(), q.residual.cpu().numpy(), q.flag.cpu().numpy()


def _compare(got, want, what):
    """Every pixel: flags equal, c bit for bit (NaN where and only where the restatement has it), dx and dy within 1e-6 px."""
    c, d, flag = got
    wq, wflag = want
    assert np.array_equal(flag, wflag), f"{what}: {np.count_nonzero(flag != wflag)} flag bytes differ"
    wc = wq[:, 0]
    assert np.array_equal(np.isnan(c), np.isnan(wc)), what
    assert np.isnan(wc[(wflag & (FEW | FLAT)) != 0]).all(), what            # (floor = 0 can also give 0 / 0 without either flag)
    same = np.where(np.isnan(wc), True, c.view(np.int32) == wc.view(np.int32))
    assert same.all(), f"{what}: c differs at {np.count_nonzero(~same)} pixels, first {np.argwhere(~same)[0]}"
    err = np.abs(d.astype(np.float64) - wq[:, 1:].astype(np.float64))
    print(f"{what}: largest |d - restatement| = {err.max():.3g} px over {np.count_nonzero(wflag & 7 == 0)} fitted pixels")
    assert np.all(err <= 1e-6), f"{what}: dx/dy off by {err.max():.3g} px"
    unfit = np.broadcast_to(((wflag & 7) != 0)[:, None], d.shape)
    assert not d[unfit].any() and not np.signbit(d[unfit]).any(), what


def _case(B, H, W, C, seed, kind="particles"):
    """Particle (or noise) images, a wild flow whose first pair keeps a clean left half, a mask with a block and speckles, one
    9 x 9 all-constant patch in both images."""
    if kind == "noise":
        img1, img2 = qr.noise_images(B, H, W, C, seed)
        true = np.zeros((B, 2, H, W), np.float32)
    else:
        img1, img2, true = qr.particle_images(B, H, W, C, seed)
    flow = qr.wild_flow(B, H, W, seed + 1)
    half = max(W // 2, 1)
    flow[0, :, 1:, 1:half] = true[0, :, 1:, 1:half] - np.array([0.2, -0.15], np.float32)[:, None, None]
    if H >= 12 and W >= 12:
        qr.flatten_patch(img1, img2, 2, 2)
    return img1, img2, flow


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (5, 3)])
def test_windows_larger_than_the_image(H, W, r, dev):
    """The window is clipped on every side at once; min_count 2 so that not every pixel is FEW."""
    seen = 0
    for C, kind in ((1, "noise"), (3, "particles")):
        img1, img2, flow = _case(2, H, W, C, 40 + H + W, kind)
        flow[1, 0], flow[1, 1] = (0.25 if W > 1 else 0.0), (0.25 if H > 1 else 0.0)
        mask = qr.speckle_mask(2, H, W, 7, 1)
        for m, mc in ((None, 2), (mask, None)):
            want = qr.batch_quality(img1, img2, flow, r, m, min_count=mc)
            _compare(_run(dev, img1, img2, flow, r, m, min_count=mc), want, f"{H}x{W} r={r} C={C}")
            seen |= int(np.bitwise_or.reduce(want[1], axis=None))
    assert seen & FEW and seen & CENTRE_OUT


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("r", [1, 4, 15])
def test_odd_sizes_against_the_restatement(r, C, dev):
    """37 x 53, B = 3: no multiple of any tile, several tiles per image, a halo wider than the tile.  The masked block is larger than
    the window (FEW), the constant patch holds whole windows up to r = 4 (FLAT)."""
    B, H, W = 3, 37, 53
    img1, img2, flow = _case(B, H, W, C, 100 + r)
    mask = qr.speckle_mask(B, H, W, 9, min(2 * r + 4, 20))
    want = qr.batch_quality(img1, img2, flow, r, mask)
    _compare(_run(dev, img1, img2, flow, r, mask), want, f"37x53 r={r} C={C}")
    seen = int(np.bitwise_or.reduce(want[1], axis=None))
    assert seen & (FEW | NO_PEAK | CENTRE_OUT) == FEW | NO_PEAK | CENTRE_OUT
    assert np.any(want[1] & 7 == 0), "no fitted pixel in the expected values"
    if r <= 4:
        assert seen == ALL_BITS


def test_wide_image_largest_radius(dev):
    B, H, W, r = 1, 70, 131, 15
    img1, img2, flow = _case(B, H, W, 1, 300)
    mask = qr.speckle_mask(B, H, W, 11, 34)
    want = qr.batch_quality(img1, img2, flow, r, mask)
    _compare(_run(dev, img1, img2, flow, r, mask), want, "70x131 r=15")
    assert np.any(want[1] & 7 == 0) and np.any(want[1] & FEW) and np.any(want[1] & NO_PEAK)


def test_noise_images_with_terms_of_both_signs(dev):
    B, H, W, r = 2, 37, 53, 4
    img1, img2, flow = _case(B, H, W, 3, 400, "noise")
    flow[1] = 0.0
    img2[1] = img1[1] + np.float32(0.05) * img2[1]            # a pair that does correlate: fitted pixels
    mask = qr.speckle_mask(B, H, W, 13, 12)
    for floor in (1.0 / 255.0, 0.0, 0.9):
        want = qr.batch_quality(img1, img2, flow, r, mask, floor=floor)
        _compare(_run(dev, img1, img2, flow, r, mask, floor=floor), want, f"noise floor={floor:.3g}")
        if floor == 0.9:
            assert np.any(want[1] & FLAT)
        else:
            assert np.any(want[1] & 7 == 0) and np.nanmin(want[0][:, 0]) < 0
        if floor == 1.0 / 255.0:
            assert int(np.bitwise_or.reduce(want[1], axis=None)) == ALL_BITS


def test_a_batch_equals_its_pairs_one_at_a_time(dev):
    from pivlfn import match_quality
    B, H, W, r = 5, 37, 53, 4
    img1, img2, flow = _case(B, H, W, 3, 500)
    mask = qr.speckle_mask(B, H, W, 15, 12)
    i1, i2, fl, mk = (torch.from_numpy(x).to(dev) for x in (img1, img2, flow, mask))
    whole = match_quality(i1, i2, fl, r, mk)
    again = match_quality(i1, i2, fl, r, mk)
    for b in range(B):
        one = match_quality(i1[b:b + 1], i2[b:b + 1], fl[b:b + 1], r, mk[b:b + 1])
        assert same_bits(one.c, whole.c[b:b + 1]) and same_bits(one.residual, whole.residual[b:b + 1]), b
        assert torch.equal(one.flag, whole.flag[b:b + 1]), b
    assert same_bits(again.c, whole.c) and same_bits(again.residual, whole.residual) and torch.equal(again.flag, whole.flag)
    assert torch.equal(whole.corrected(fl)[0, :, 5, 5], (fl + whole.residual)[0, :, 5, 5])


def _capped_shapes():
    import analysis_plans as ap
    return ap.shapes(ap.QUALITY_CASES)


@pytest.mark.parametrize("B,H,W,r", _capped_shapes())
def test_bits_where_the_warp_grid_is_capped(B, H, W, r, dev):
    """quality_warp_kernel has at most max(16384 / B, 64) workgroups a pair and strides over the rest: 260 pairs of 130 x 128 are 65
    blocks of 256 pixels on a grid of 64.  Eight particle pairs, each shifted along x by another number of columns for every further
    pair (rendering 260 takes the host 12 s).  The first, the middle and the last pair against the restatement; sixteen pairs against
    the same pair in a call of its own, whose grid is not capped."""
    from pivlfn import match_quality
    import analysis_plans as ap
    plan = ap.capped_frame_grid(H * W, B)
    assert plan["blocks"] > plan["cap"] == plan["grid"]
    base = _case(8, H, W, 1, 700)
    img1, img2, flow = (np.stack([np.roll(x[b % 8], b // 8, axis=-1) for b in range(B)]) for x in base)
    mask = qr.speckle_mask(B, H, W, 9, 2 * r + 4)
    i1, i2, fl, mk = (torch.from_numpy(x).to(dev) for x in (img1, img2, flow, mask))
    whole = match_quality(i1, i2, fl, r, mk)
    seen = 0
    for b in sorted({0, B // 2, B - 1}):
        want = qr.batch_quality(img1[b:b + 1], img2[b:b + 1], flow[b:b + 1], r, mask[b:b + 1])
        got = (whole.c[b:b + 1].cpu().numpy(), whole.residual[b:b + 1].cpu().numpy(), whole.flag[b:b + 1].cpu().numpy())
        _compare(got, want, f"pair {b} of {B} x {H}x{W} r={r}")
        seen |= int(np.bitwise_or.reduce(want[1], axis=None))
        assert np.any(want[1] & 7 == 0), "no fitted pixel in the expected values"
    assert seen & (FEW | NO_PEAK | CENTRE_OUT) == FEW | NO_PEAK | CENTRE_OUT
    for b in [0, 1, 2, 63, 64, 65, 127, 128, 129, 130, 191, 192, 255, 256, 258, 259]:
        one = match_quality(i1[b:b + 1], i2[b:b + 1], fl[b:b + 1], r, mk[b:b + 1])
        assert same_bits(one.c, whole.c[b:b + 1]) and same_bits(one.residual, whole.residual[b:b + 1]), b
        assert torch.equal(one.flag, whole.flag[b:b + 1]), b


def _call(lib, ins, outs, ws, B, C, H, W, r, stream, ws_bytes=None):
    i1, i2, fl, mk = ins
    return lib.pivlfn_match_quality(i1.data_ptr(), i2.data_ptr(), C, fl.data_ptr(), mk.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                    B, H, W, r, ((2 * r + 1) ** 2 + 1) // 2, 1.0 / 255.0, ws.data_ptr(),
                                    ws.numel() if ws_bytes is None else ws_bytes, stream)


@pytest.mark.parametrize("r", [4, 15])
def test_guarded_inputs_poisoned_outputs_dirty_workspace(r, dev):
    """Inputs at the end of guarded allocations (a read past either end meets NaN guards), outputs pre-filled with NaN / 0xFF, a
    workspace full of 0xFF of exactly the size asked for: the result equals the plain call's bit for bit, every guard holds, and a
    workspace one byte smaller is refused."""
    from pivlfn import _lib, match_quality
    lib = _lib.load()
    B, C, H, W = 4, 3, 19, 23                       # B*H*W a multiple of 4: the byte buffers are whole 32-bit words
    img1, img2, flow = _case(B, H, W, C, 600 + r)
    mask = qr.speckle_mask(B, H, W, 17, 8)
    src = [torch.from_numpy(x).to(dev) for x in (img1, img2, flow, mask)]
    ref = match_quality(*src[:3], r, src[3])
    ins = [guarded(t.shape, t.dtype, dev, "nan") for t in src]
    for t, s in zip(ins, src):
        t.copy_(s)
    qual = guarded((B, 3, H, W), torch.float32, dev, "sentinel")
    flag = guarded((B, H, W), torch.uint8, dev, "sentinel")
    flag.fill_(0xFF)
    need = lib.pivlfn_match_quality_workspace_bytes(B, H, W, r)
    ws = guarded((need,), torch.uint8, dev, "sentinel")
    ws.fill_(0xFF)
    st = torch.cuda.current_stream(dev).cuda_stream
    with pytest.raises(ValueError, match="too small"):
        _lib.check(_call(lib, ins, (qual, flag), ws, B, C, H, W, r, st, need - 1), "match_quality")
    assert bool((flag == 0xFF).all())               # refused before anything was launched
    _lib.check(_call(lib, ins, (qual, flag), ws, B, C, H, W, r, st), "match_quality")
    torch.cuda.synchronize()
    assert same_bits(qual[:, 0], ref.c) and same_bits(qual[:, 1:], ref.residual) and torch.equal(flag, ref.flag)
    for t in ins + [qual, flag, ws]:
        check_guards(t, f"match_quality r={r}")
    for t, s in zip(ins, src):
        assert torch.equal(t.view(torch.uint8), s.view(torch.uint8)), "an input was written"


def test_runs_in_order_on_the_stream_it_is_given(dev):
    """On a fresh stream, behind a bounded delay (a chain of matrix products) and the copy of the real inputs into buffers that hold
    the NaN poison, the call is enqueued without any host synchronisation; its outputs equal the eager result bit for bit.  A launch
    on another stream would read the poison or leave the sentinel."""
    from pivlfn import _lib, match_quality
    lib = _lib.load()
    B, C, H, W, r = 2, 1, 40, 56, 8
    img1, img2, flow = _case(B, H, W, C, 700)
    src = [torch.from_numpy(x).to(dev) for x in (img1, img2, flow, qr.speckle_mask(B, H, W, 19, 10))]
    ref = match_quality(*src[:3], r, src[3])
    ins = [guarded(t.shape, t.dtype, dev, "nan") for t in src]
    qual = guarded((B, 3, H, W), torch.float32, dev, "sentinel")
    flag = guarded((B, H, W), torch.uint8, dev, "sentinel")
    ws = guarded((lib.pivlfn_match_quality_workspace_bytes(B, H, W, r),), torch.uint8, dev, "nan")
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
        rc = _call(lib, ins, (qual, flag), ws, B, C, H, W, r, stream.cuda_stream)
        still_waiting = not delayed.query()             # the call was enqueued while the delay was still running
    _lib.check(rc, "match_quality")
    stream.synchronize()
    assert still_waiting, "the delay ran out before the call was enqueued: the test would not see a launch on another stream"
    assert same_bits(qual[:, 0], ref.c) and same_bits(qual[:, 1:], ref.residual) and torch.equal(flag, ref.flag)
    for t in ins + [qual, flag, ws]:
        check_guards(t, "match_quality on a side stream")


@pytest.mark.parametrize("seed", [7, 11, 12])
def test_planted_error_is_recovered_on_the_device(seed, dev):
    """tests/test_quality.py's planted (0.3, -0.2) px with its bound of 0.05 px, and corrected() moves the flow towards the truth.  Its
    bound of 0.95 on the median c holds for the true flow only: with the planted error the windows are compared 0.36 px off the peak,
    so c is lower than at the true flow (0.93 against 0.98 in the float64 restatement) and is asked only to be that."""
    from pivlfn import match_quality
    img1, img2, true = qr.particle_images(1, 128, 128, 3, seed)
    img1, img2 = img1[:, [0, 0, 0]], img2[:, [0, 0, 0]]                  # the network's input: three equal channels
    flow = true - np.array([0.3, -0.2], np.float32)[:, None, None]
    i1, i2, fl, tr = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (img1, img2, flow, true))
    q = match_quality(i1, i2, fl)
    inner = (slice(None), slice(24, -24), slice(24, -24))
    assert not bool(q.flag[inner].any())
    mean = q.residual[:, :, 24:-24, 24:-24].double().mean(dim=(0, 2, 3)).cpu().numpy()
    print("planted (0.3, -0.2), seed", seed, "mean residual", mean)
    assert np.all(np.abs(mean - np.array([0.3, -0.2])) < 0.05)
    at_truth = match_quality(i1, i2, tr)
    assert not bool(at_truth.flag[inner].any()) and float(at_truth.c[inner].median()) > 0.95
    assert 0.0 < float(q.c[inner].median()) < float(at_truth.c[inner].median())       # a peak still, but 0.36 px down its flank
    fixed = q.corrected(fl)
    assert same_bits(fixed, fl + q.residual)
    before = (fl - tr)[:, :, 24:-24, 24:-24].pow(2).sum(1).sqrt().mean()
    after = (fixed - tr)[:, :, 24:-24, 24:-24].pow(2).sum(1).sqrt().mean()
    assert float(after) < 0.25 * float(before)
    (s,) = q.summary()
    assert s["few"] > 0 and s["flat"] == 0 and 0.9 < s["mean_c"] <= 1.0 and 0.2 < s["rms_residual"] < 0.5


def test_run_py_quality(tmp_path, dev):
    """run.py -p --quality 4 --quality-image --validate flag on three synthetic 64 x 64 pairs: every <name>_qual.flo holds the three bands of
    match_quality on the written flow and the frames the network was given, with the validation flags as the mask, bit for bit;
    quality.json holds one entry per pair and the run summary; the PNGs exist at the frames' size.  Without --quality no such file
    appears and the .flo files are the same bytes."""
    import PIL.Image
    import run as runpy
    import pivlfn
    from pivlfn import synth
    from pivlfn import validate as V
    from pivlfn.flo import read_flow
    from pivlfn.pipeline import read_image_u8, u8_to_input
    H = W = 64
    seq = tmp_path / "seq"
    seq.mkdir()
    names = [f"p{k}" for k in range(3)]
    for k, name in enumerate(names):
        a, b, _ = synth.particle_pair(H, W, 950 + k)
        PIL.Image.fromarray(a).save(str(seq / f"{name}_img1.png"))
        PIL.Image.fromarray(b).save(str(seq / f"{name}_img2.png"))
    base = ["--model", "piv", "-i", str(seq), "-p", "--batch", "2", "--validate", "flag", "--validate-radius", "2", "--validate-eps",
            "0.01", "--validate-thresh", "0.5"]
    assert runpy.main(base + ["-o", str(tmp_path / "plain")]) == 3
    assert runpy.main(base + ["-o", str(tmp_path / "qual"), "--quality", "4", "--quality-image"]) == 3
    plain, qual = (tmp_path / d / "piv-synthetic" / "seq" for d in ("plain", "qual"))
    assert not list(plain.rglob("*_qual.flo")) and not list(plain.rglob("*_corr.png")) and not (plain / "quality.json").exists()
    assert not [ln for ln in open(plain / "args.txt") if ln.startswith("quality")]
    assert "quality: 4\n" in list(open(qual / "args.txt")) and "quality_image: True\n" in list(open(qual / "args.txt"))
    doc = json.load(open(qual / "quality.json"))
    assert doc["radius"] == 4 and doc["min_count"] == 41 and doc["mask"] == "flag" and sorted(doc["pairs"]) == names
    total_fit = 0
    for n in names:
        data = open(qual / "flow" / f"{n}_out.flo", "rb").read()
        assert data == open(plain / "flow" / f"{n}_out.flo", "rb").read(), n
        i1, i2 = (u8_to_input(torch.from_numpy(read_image_u8(str(seq / f"{n}_img{j}.png"))[None]).to(dev)) for j in (1, 2))
        flo = torch.from_numpy(read_flow(str(qual / "flow" / f"{n}_out.flo"))).to(dev).permute(2, 0, 1)[None].contiguous()
        flags = V.validate_flow(flo, radius=2, spacing=1, eps=0.01, thresh=0.5, mode="flag").flag
        want = pivlfn.match_quality(i1, i2, flo, 4, mask=flags)
        got = torch.from_numpy(read_flow(str(qual / "flow" / f"{n}_qual.flo"), use_stereo=True)).to(dev)
        assert got.shape == (H, W, 3)
        assert same_bits(got[..., 0], want.c[0]) and same_bits(got[..., 1:], want.residual[0].permute(1, 2, 0)), n
        (s,) = want.summary()
        for key, val in s.items():
            have = doc["pairs"][n][key]
            # counts are exact; the float64 sums behind the two means may be reduced in another order in a batch of two
            assert have == val or (have is None and val != val) or abs(have - val) <= 1e-12 * abs(val), (n, key, have, val)
        total_fit += s["n_fit"]
        im = PIL.Image.open(qual / "flow" / f"{n}_corr.png")
        assert im.mode == "RGB" and im.size == (W, H)
    assert doc["total"]["n_fit"] == total_fit
    assert sorted(p.name for p in (qual / "flow").glob("*_corr.png")) == [f"{n}_corr.png" for n in names]
