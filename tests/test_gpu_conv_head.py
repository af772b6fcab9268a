"""GPU: the flow head (pivlfn_conv_head_nhwc) on every kernel its launcher can pick, one case per thing a kernel can get wrong.

HEAD_CASES (tests/test_conv_head_plan.py) holds the shapes: per (k, family) the smallest images with ragged right and bottom tiles, the
images exactly on each bound of the policy, and images thinner than a tile or than the k // 2 halo.  Every case runs
  (a) against torch's float64 convolution + residual, at the bar tests/test_gpu_conv.py holds this kernel to;
  (b) on small integers, where every fma chain and the fp32 matrix instruction are exact and any summation order must give the
      int64 result bit for bit: a wrong tap, channel, weight slot, swizzle or halo column cannot hide under a tolerance;
  (c) alone and as image 0 and image 2 of a batch of three: the same bits (the kernel choice never depends on the batch).
Then the two one-pixel kernels against each other on a column crop (d), and a NULL residual against a residual of +0.0 (e).
The two images of 2 GiB of input are made on the device and checked on bands (first and last 40 rows, first and last 70 columns of
64 middle rows); everything outside the bands must be finite."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from pivlfn import _lib
from guarded import same_bits
from test_conv_head_plan import HEAD_CASES, MFMA, NAMES, PIXEL, PIXEL_LDS, ROWS4, is_2gib, plan
from test_gpu_conv import Conv

pytestmark = pytest.mark.gpu
NAN = float("nan")
BAR = 2e-5                                   # tests/test_gpu_conv.py::test_flow_head_kernel_matches_torch: max-abs error / max(1, max|want|)
FREE_BYTES_2GIB = 4 << 30                    # x (2 GiB), res4 and out4 (256 MiB each, twice in (e)) and the bands


def _id(c):
    return f"k{c[0]}-B{c[1]}-{c[2]}x{c[3]}-{NAMES[c[4]]}"


def _seed(case, salt=0):
    k, B, H, W, fam = case
    return k * 1000003 + B * 7919 + H * 31 + W + salt


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _needs_memory(case, dev):
    if is_2gib(case) and torch.cuda.mem_get_info(dev)[0] < FREE_BYTES_2GIB:
        pytest.skip("a 2 GiB input needs about 4 GiB of free device memory")


def head(conv, xd, r4, B, H, W, dev):
    """One call on device tensors x [B,H,W,32] and res4 [B,H,W,4] (or None); out4 starts as NaN.  Lanes 2-3 must come back as +0.0."""
    assert xd.shape == (B, H, W, 32) and xd.is_contiguous() and (r4 is None or (r4.shape == (B, H, W, 4) and r4.is_contiguous()))
    out = torch.full((B, H, W, 4), NAN, device=dev)
    _lib.check(_lib.load().pivlfn_conv_head_nhwc(conv.h, xd.data_ptr(), r4.data_ptr() if r4 is not None else None, out.data_ptr(),
                                                 B, H, W, _st(dev)), "head")
    torch.cuda.synchronize(dev)
    assert bool((out[..., 2:].view(torch.int32) == 0).all()), "lanes 2-3 of out4 must be +0.0 (sign bit included)"
    return out


def res4_of(res, dev):
    """[B,H,W,2] -> res4 on the device with NaN in the lanes the kernels must not read."""
    r4 = torch.full(res.shape[:3] + (4,), NAN, device=dev)
    r4[..., :2] = res.to(dev)
    return r4


def bands(H, W):
    """(r0, r1, c0, c1) of the output regions a 2 GiB case is checked on."""
    m = H // 2 - 32
    return [(0, 40, 0, W), (H - 40, H, 0, W), (m, m + 64, 0, 70), (m, m + 64, W - 70, W)]


def band_want(x, w, b, res, band):
    """The float64 head on one band of image 0: the band is cut from x with its k // 2 halo (zero padding where the halo leaves the
    image, which is the convolution's own padding there) and the halo's outputs are dropped.  x, res: device or CPU, [1,H,W,*]."""
    r0, r1, c0, c1 = band
    P, (H, W) = w.shape[-1] // 2, x.shape[1:3]
    y0, y1, x0, x1 = max(0, r0 - P), min(H, r1 + P), max(0, c0 - P), min(W, c1 + P)
    xs = x[0, y0:y1, x0:x1].cpu().double().permute(2, 0, 1)[None]
    full = F.conv2d(xs, w.double(), b.double(), padding=P)[0]
    want = full[:, r0 - y0:r1 - y0, c0 - x0:c1 - x0].permute(1, 2, 0)
    return want + res[0, r0:r1, c0:c1].cpu().double()


def inputs(case, dev, integers):
    """conv, x [B,H,W,32] and res [B,H,W,2], seeded by the case: on the CPU, for the 2 GiB cases on the device.  integers: x in
    [-8, 8], w and b in [-4, 4], res in [-8, 8]."""
    k, B, H, W, fam = case
    g = torch.Generator().manual_seed(_seed(case, int(integers)))
    if integers:
        w = torch.randint(-4, 5, (2, 32, k, k), generator=g).float()
        b = torch.randint(-4, 5, (2,), generator=g).float()
    else:
        w = torch.randn(2, 32, k, k, generator=g) / (32 * k * k) ** 0.5
        b = torch.randn(2, generator=g) * 0.1
    on = dev if is_2gib(case) else "cpu"
    if is_2gib(case):
        g = torch.Generator(device=dev).manual_seed(_seed(case, int(integers)))
    x = torch.empty(B, H, W, 32, device=on)
    res = torch.empty(B, H, W, 2, device=on)
    if integers:
        x.random_(-8, 9, generator=g)
        res.random_(-8, 9, generator=g)
    else:
        x.normal_(generator=g)
        res.normal_(generator=g)
    return Conv(w, b), x, res


def check(case, dev, integers):
    """Runs the case and returns max|got - want| / max(1, max|want|) over what is compared; integers: asserts bit equality instead."""
    k, B, H, W, fam = case
    assert plan(k, B, H, W)[0] == fam
    conv, x, res = inputs(case, dev, integers)
    out = head(conv, x.to(dev), res4_of(res, dev), B, H, W, dev)
    if integers:
        # sum of absolute products, bias and residual: every partial sum of any summation order stays below 2^24 in magnitude,
        # so fp32 represents each of them exactly
        assert 32 * k * k * 8 * 4 + 4 + 8 < 2 ** 24
        for t, bound in ((x, 8), (res, 8), (conv.w, 4), (conv.b, 4)):
            assert -bound <= float(t.min()) and float(t.max()) <= bound
    if is_2gib(case):
        assert bool(torch.isfinite(out[..., :2]).all()), "a pixel outside the checked bands is not finite"
        pieces = [(out[0, r0:r1, c0:c1, :2].cpu(), band_want(x, conv.w, conv.b, res, (r0, r1, c0, c1))) for r0, r1, c0, c1 in bands(H, W)]
    else:
        want = F.conv2d(x.permute(0, 3, 1, 2).double(), conv.w.double(), conv.b.double(), padding=k // 2).permute(0, 2, 3, 1) + res.double()
        pieces = [(out[..., :2].cpu(), want)]
    err, scale = 0.0, 1.0
    for got, want in pieces:
        assert got.shape == want.shape
        if integers:
            want = want.to(torch.int64)                       # float64 sums of these integers are exact: this is the int64 result
            assert int(want.abs().max()) < 2 ** 24
            bad = (got.double() != want.double()).nonzero()
            assert bad.numel() == 0, f"{_id(case)}: {bad.shape[0]} of {got.numel()} outputs differ from the exact result, first at {bad[0].tolist()}"
            assert same_bits(got, want.float())
        err, scale = max(err, (got.double() - want).abs().max().item()), max(scale, want.abs().max().item())
    return err / scale


ERRORS = {}                                  # (k, family) -> worst observed error / bar's scale over the cases of (a)


@pytest.mark.parametrize("case", HEAD_CASES, ids=_id)
def test_head_matches_float64(case, dev):
    _needs_memory(case, dev)
    err = check(case, dev, integers=False)
    key = (case[0], NAMES[case[4]])
    ERRORS[key] = max(ERRORS.get(key, 0.0), err)
    print(f"\nhead k={case[0]} {NAMES[case[4]]} {case[2]}x{case[3]} B={case[1]}: max-abs error / max(1, max|want|) = {err:.3e} (bar {BAR:.0e})")
    assert err < BAR, (case, err)


def test_report_errors_per_family():
    """The worst error of (a) per (k, family); runs after the cases above and asserts only that there is something to report."""
    for (k, fam), err in sorted(ERRORS.items()):
        print(f"\nhead k={k} {fam}: worst max-abs error / max(1, max|want|) = {err:.3e} (bar {BAR:.0e})")
    assert all(e < BAR for e in ERRORS.values())


@pytest.mark.parametrize("case", HEAD_CASES, ids=_id)
def test_head_is_exact_on_small_integers(case, dev):
    _needs_memory(case, dev)
    assert check(case, dev, integers=True) == 0.0


@pytest.mark.parametrize("case", [c for c in HEAD_CASES if not is_2gib(c)], ids=_id)
def test_head_bits_do_not_depend_on_batch_mates(case, dev):
    """The case's first image alone, and as image 0 and image 2 of a batch of three whose middle image is noise."""
    k, B, H, W, fam = case
    assert plan(k, 1, H, W)[0] == fam and plan(k, 3, H, W)[0] == fam
    conv, x, res = inputs(case, dev, integers=False)
    g = torch.Generator().manual_seed(_seed(case, 2))
    xb = torch.stack([x[0], 3.0 * torch.randn(H, W, 32, generator=g), x[0]]).to(dev)
    rb = res4_of(torch.stack([res[0], torch.randn(H, W, 2, generator=g), res[0]]), dev)
    alone = head(conv, xb[:1].contiguous(), rb[:1].contiguous(), 1, H, W, dev)
    batch = head(conv, xb, rb, 3, H, W, dev)
    assert same_bits(batch[0], alone[0]), "image 0 of the batch differs from the image alone"
    assert same_bits(batch[2], alone[0]), "image 2 of the batch differs from the image alone"
    assert not same_bits(batch[1], alone[0])


@pytest.mark.parametrize("case", [c for c in HEAD_CASES if c[4] == PIXEL], ids=_id)
def test_pixel_and_pixel_lds_give_the_same_bits(case, dev):
    """conv_head.hip: the two one-pixel variants "produce the same bits as each other".  A column crop of a PIXEL image, starting at
    a column that is no multiple of the tile, is narrow enough for PIXEL_LDS; away from the crop's own left and right padding every
    output must equal the full image's."""
    k, B, H, W, fam = case
    P, c0 = k // 2, 5
    wc = 16 * min(512 // -(-H // 16), (W - c0) // 16) - 3           # the most 16 x 16 tiles PIXEL_LDS takes, the last one ragged
    if k == 7:
        wc = min(wc, (256 * 256 - 1) // H)                           # fewer than 65536 pixels, or the crop is MFMA's
    assert c0 % 16 and c0 + wc <= W and wc > 2 * P + 16
    assert plan(k, 1, H, W)[0] == PIXEL and plan(k, 1, H, wc)[0] == PIXEL_LDS
    conv, x, res = inputs(case, dev, integers=False)
    full = head(conv, x[:1].to(dev), res4_of(res[:1], dev), 1, H, W, dev)
    crop = head(conv, x[:1, :, c0:c0 + wc].contiguous().to(dev), res4_of(res[:1, :, c0:c0 + wc].contiguous(), dev), 1, H, wc, dev)
    assert same_bits(crop[:, :, P:wc - P], full[:, :, c0 + P:c0 + wc - P])


def _first_of(k, fam):
    return next(c for c in HEAD_CASES if c[0] == k and c[4] == fam and (c[2] > 1 or c[3] > 1))


@pytest.mark.parametrize("case", [_first_of(k, f) for k in (3, 5, 7) for f in (PIXEL_LDS, PIXEL, ROWS4)] + [_first_of(7, MFMA)], ids=_id)
def test_null_residual_is_a_zero_residual(case, dev):
    """res4 may be NULL (include/pivlfn.h; pivlfn_forward's coarsest level): the bits of a residual of +0.0."""
    _needs_memory(case, dev)
    k, B, H, W, fam = case
    assert plan(k, B, H, W)[0] == fam
    conv, x, res = inputs(case, dev, integers=False)
    xd = x.to(dev)
    del x, res
    none = head(conv, xd, None, B, H, W, dev)
    zero = head(conv, xd, torch.zeros(B, H, W, 4, device=dev), B, H, W, dev)
    assert bool(torch.isfinite(none).all())
    assert same_bits(none, zero)
