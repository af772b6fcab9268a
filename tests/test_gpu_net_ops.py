"""GPU: the level-pipeline kernels that run only inside pivlfn_forward, each through its per-layer entry point (include/pivlfn.h)
against a float64 restatement of the reference's operation (tests/net_ops_reference.py, cited there per op):

    pivlfn_upconv_nhwc       dwconvT_b2_kernel<14> / dwconvT_kernel<1>   upConv_M / upCorr_M          src/models.py:144-145, 151-152
    pivlfn_backwarp_nhwc     backwarp_nhwc_kernel                        Subpixel's backwarp          :214
    pivlfn_reg_prep          flow_mean_stage1 (+ stage2) + reg_prep      Regularization front         :275-277
    pivlfn_reg_tail          reg_tail_kernel<3/5/7>                      Regularization tail          :281-302
    pivlfn_prep_pyramid      prep_images + resize_nhwc4 chain            mean subtraction, pyramid    :321-323, 336-343
    pivlfn_conv1_fused_nhwc  conv_c3k7_kernel<true> (Conv1Fuse)          NetC.conv1 + NetC_ext + moduleFeat at level 1

Every output element is held to its own bound (n * 2^-24 * sum|terms| for its roundings, plus the position error times the
interpolant's slope where sample positions are computed; the docstrings of tests/net_ops_reference.py derive each), and the
maximum error to the repo's per-op bars: 1e-5 * max|out|, 2e-5 for warps.  The measured errors are printed.  Where the code states
bit identity (the fused and the stand-alone mean, the two depthwise kernels, a batch and its images alone) torch.equal is asserted.
Only the production library is called, except by the one bit-identity test of the tools build's variant kernel."""
import ctypes

import numpy as np
import pytest
import torch

import pivlfn
import pivlfn_oracle as orc
from pivlfn import _lib
import net_ops_reference as ref

pytestmark = pytest.mark.gpu
F64 = torch.float64
NAN = float("nan")
OP_BAR, WARP_BAR = 1e-5, 2e-5


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _within(got, want, bound, bar, what):
    """|got - want| <= bound element by element, and max|got - want| <= bar * max|want|."""
    got, want, bound = got.to(F64), want.to(want.device, F64), bound.to(want.device, F64)
    got = got.to(want.device)
    err = (got - want).abs()
    scale = float(want.abs().max()) if want.numel() else 0.0
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    e = float(err.max()) if err.numel() else 0.0
    print(f"{what}: max|err| {e:.2e} = {e / max(scale, 1e-300):.2e} of max|out| {scale:.3g}; worst err / bound {worst:.3f}")
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    assert bool((err <= bound).all()), f"{what}: an element exceeds its bound ({worst:.2f} x)"
    assert e <= bar * scale, f"{what}: max-abs {e:.3e} > {bar} * {scale:.3e}"


def _nhwc(t, lanes, fill=0.0):
    """NCHW [B,C,H,W] -> [B,H,W,lanes] with the lanes past C filled."""
    B, C, H, W = t.shape
    out = torch.full((B, H, W, lanes), fill, dtype=torch.float32, device=t.device)
    out[..., :C] = t.permute(0, 2, 3, 1)
    return out


# ---- upConv_M / upCorr_M -------------------------------------------------------------------------------------------------
def _upconv(x4, w, B, H, W, quads, sin, sout, dev, lib=None):
    lib = lib or _lib.load()
    out = torch.full((B, 2 * H, 2 * W, sout), NAN, device=dev)
    wc = w.float().contiguous()
    rc = lib.pivlfn_upconv_nhwc(x4.data_ptr(), wc.data_ptr(), out.data_ptr(), B, H, W, quads, sin, sout, _st(dev))
    assert rc == 0, lib.pivlfn_last_error()
    return out


def _upconv_inputs(B, H, W, quads, sin, seed, dev):
    g = torch.Generator().manual_seed(seed)
    C = 2 if quads == 1 else 49
    x = torch.randn(B, C, H, W, generator=g)
    w = 0.5 * torch.randn(C, 1, 4, 4, generator=g)
    x4 = _nhwc(x, 4 * quads)                                    # padding channels zero, as in the network
    if sin > 4 * quads:
        x4 = torch.cat([x4, torch.full((B, H, W, sin - 4 * quads), NAN)], 3)      # lanes the kernel must never read
    return x, w, x4.contiguous().to(dev)


@pytest.mark.parametrize("quads,B,H,W,sin,sout", [
    (1, 1, 1, 1, 4, 4), (14, 1, 1, 1, 56, 56),                 # one input pixel: every output has taps outside
    (1, 3, 2, 3, 4, 4), (14, 3, 3, 2, 56, 56),
    (1, 1, 7, 5, 4, 4), (14, 3, 7, 9, 56, 56),                 # odd
    (1, 1, 257, 129, 4, 4), (14, 1, 257, 129, 56, 56),         # ragged rows of the 256-item segments
    (1, 2, 9, 11, 8, 12), (14, 2, 5, 6, 60, 64),               # strides wider than cstore: NaN lanes in and out
])
def test_upconv_vs_float64(quads, B, H, W, sin, sout, dev):
    x, w, x4 = _upconv_inputs(B, H, W, quads, sin, 1000 * quads + 7 * H + W + B, dev)
    C, cs = x.shape[1], 4 * quads
    out = _upconv(x4, w, B, H, W, quads, sin, sout, dev).cpu()
    assert torch.all(out[..., C:cs] == 0), "padding lanes must be exact zeros"
    if sout > cs:
        assert torch.isnan(out[..., cs:]).all(), "lanes beyond cstore must keep their sentinel"
    want = ref.upconv(x.double(), w.double())
    _within(out[..., :C].permute(0, 3, 1, 2), want, ref.upconv_bound(x.double(), w.double()), OP_BAR,
            f"upconv q{quads} {B}x{H}x{W}")


def test_upconv_output_past_2gib(dev):
    """upCorr_M at B = 10 on a 512^2 input: 2.35 GB of output.  The last image (offsets past 2^31 floats) equals that image alone bit
    for bit, and its bottom rows match float64."""
    B, H, W, quads = 10, 512, 512, 14
    g = torch.Generator(device=dev).manual_seed(21)
    x4 = torch.zeros(B, H, W, 56, device=dev)
    x4[..., :49] = torch.randn(B, H, W, 49, device=dev, generator=g)
    w = 0.5 * torch.randn(49, 1, 4, 4)
    out = _upconv(x4, w, B, H, W, quads, 56, 56, dev)
    assert out.numel() * 4 > 2 ** 31
    for b in (0, B - 1):
        one = _upconv(x4[b:b + 1].contiguous(), w, 1, H, W, quads, 56, 56, dev)
        assert torch.equal(one[0], out[b]), b
    assert torch.all(out[..., 49:] == 0)
    # output rows 2(H-64)+1 .. 2H-1 depend on input rows H-64 .. H-1 only
    xin = x4[B - 1:B, H - 64:, :, :49].permute(0, 3, 1, 2).double().cpu()
    want = ref.upconv(xin, w.double())[:, :, 1:]
    got = out[B - 1:B, 2 * (H - 64) + 1:, :, :49].permute(0, 3, 1, 2).cpu()
    _within(got, want, ref.upconv_bound(xin, w.double())[:, :, 1:], OP_BAR, "upconv q14 B=10 512^2, last image")


def test_upconv_block_kernel_bits_equal_one_output_per_thread(dev):
    """dwconvT_b2_kernel<14> (the network's) and dwconvT_kernel<14> (selected in the tools build by knob 1 bit 8388608) give the same
    bits (ops.hip: same tap order, out-of-range taps skipped); the production library's output equals both."""
    from test_gpu_wino import _tools
    tl = _tools()
    try:
        for (B, H, W) in [(1, 1, 1), (3, 33, 17), (2, 64, 96)]:
            _, w, x4 = _upconv_inputs(B, H, W, 14, 56, 31 + H, dev)
            assert tl.pivlfn_tune(1, 0) == 0
            b2 = _upconv(x4, w, B, H, W, 14, 56, 56, dev, tl)
            assert tl.pivlfn_tune(1, 8388608) == 0
            one = _upconv(x4, w, B, H, W, 14, 56, 56, dev, tl)
            prod = _upconv(x4, w, B, H, W, 14, 56, 56, dev)
            assert torch.equal(b2, one), (B, H, W)
            assert torch.equal(prod, b2), (B, H, W)
    finally:
        tl.pivlfn_tune(1, 0)


# ---- Subpixel's backwarp ----------------------------------------------------------------------------------------------------
KINDS = ("integer", "neg_frac", "last_col", "outside", "huge", "random")


def _edge_flow(B, H, W, scale, seed):
    """A flow whose pixels each pick one of KINDS: sample exactly on integers; x in (-1, 0) (floor != truncation); x in (W-1, W)
    and y in (H-1, H) (one tap column / row out of range); entirely outside the image; +-1e4; N(0, 2) pixels.  Returns (flow
    [B,2,H,W] fp32, kind index per pixel)."""
    g = torch.Generator().manual_seed(seed)
    kind = torch.randint(0, len(KINDS), (B, H, W), generator=g)
    xs = torch.arange(W, dtype=F64).view(1, 1, W).expand(B, H, W)
    ys = torch.arange(H, dtype=F64).view(1, H, 1).expand(B, H, W)
    r = torch.rand(2, B, H, W, generator=g, dtype=F64) * 0.98 + 0.01
    tx, ty = xs + 2 * torch.randn(B, H, W, generator=g, dtype=F64), ys + 2 * torch.randn(B, H, W, generator=g, dtype=F64)
    tx = torch.where(kind == 1, -r[0], tx)
    ty = torch.where(kind == 1, -r[1], ty)
    tx = torch.where(kind == 2, W - 1 + r[0], tx)
    ty = torch.where(kind == 2, H - 1 + r[1], ty)
    side = torch.randint(0, 2, (B, H, W), generator=g).bool()
    tx = torch.where(kind == 3, torch.where(side, -1.5 - 3 * r[0], W + 0.5 + 3 * r[0]), tx)
    fl = torch.stack([(tx - xs) / scale, (ty - ys) / scale], 1).float()
    ints = 8.0 * torch.randint(-3, 4, (2, B, H, W), generator=g).float()        # x + u * scale integer for every level scale
    fl = torch.where((kind == 0)[:, None], ints.permute(1, 0, 2, 3), fl)
    huge = torch.where(torch.rand(2, B, H, W, generator=g) < 0.5, -1e4, 1e4).float().permute(1, 0, 2, 3)
    fl = torch.where((kind == 4)[:, None], huge, fl)
    return fl.contiguous(), kind


def _backwarp_nhwc(x4, fl4, scale, B, H, W, C, dev):
    out = torch.full((B, H, W, C), NAN, device=dev)
    _lib.check(_lib.load().pivlfn_backwarp_nhwc(x4.data_ptr(), fl4.data_ptr(), scale, out.data_ptr(), B, H, W, C, _st(dev)), "backwarp_nhwc")
    return out


@pytest.mark.parametrize("C,scale,shape", [
    (64, 20.0, (2, 19, 23)), (64, 10.0, (1, 130, 70)), (64, 5.0, (2, 19, 23)), (96, 2.5, (2, 17, 9)), (128, 1.25, (1, 8, 12)),
    (192, 0.625, (1, 4, 6)), (32, 20.0, (3, 16, 16)), (4, 10.0, (2, 31, 2)),
])
def test_backwarp_nhwc_vs_float64(C, scale, shape, dev):
    B, H, W = shape
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, C, H, W, generator=g)
    fl, kind = _edge_flow(B, H, W, scale, 7 * C + W)
    out = _backwarp_nhwc(_nhwc(x, C).to(dev), _nhwc(fl, 4).to(dev), scale, B, H, W, C, dev)
    got = out.permute(0, 3, 1, 2)
    xd, fd = x.double().to(dev), fl.double().to(dev)
    want, absterms = ref.backwarp(xd, fd * scale)
    bound = ref.backwarp_bound(xd, fl.to(dev), scale, absterms)
    far = ((kind == 3) | (kind == 4)).to(dev)[:, None].expand_as(got)
    assert torch.all(got[far] == 0), "samples with every tap outside the image must be exact zeros"
    _within(got, want, bound, WARP_BAR, f"backwarp_nhwc C={C} scale={scale} {B}x{H}x{W}")
    # the NCHW kernel of pivlfn.backwarp on the same data (flow * scale, rounded once): to the existing warp test's 2e-6
    fs = (fl * scale).to(dev)
    nchw = pivlfn.backwarp(tensorInput=x.to(dev), tensorFlow=fs)
    same = _backwarp_nhwc(_nhwc(x, C).to(dev), _nhwc(fs, 4), 1.0, B, H, W, C, dev).permute(0, 3, 1, 2)
    d = float((same - nchw).abs().max()) / float(nchw.abs().max())
    assert d < 2e-6, d


# ---- Regularization front -----------------------------------------------------------------------------------------------------
def _reg_prep(i1, i2, fl4, scale, B, H, W, fused, dev):
    misc = torch.full((B, H, W, 4), NAN, device=dev)
    mean = torch.full((B, 2), NAN, device=dev)
    part = torch.full((B, 128), NAN, device=dev)
    _lib.check(_lib.load().pivlfn_reg_prep(i1.data_ptr(), i2.data_ptr(), fl4.data_ptr(), scale, misc.data_ptr(), mean.data_ptr(),
                                           part.data_ptr(), B, H, W, fused, _st(dev)), "reg_prep")
    return misc, mean


@pytest.mark.parametrize("B,H,W,offset,scale", [
    (1, 1, 1, 0.0, 20.0), (3, 7, 9, 1000.0, 10.0), (1, 15, 17, 0.0, 1.25), (3, 1, 257, 0.0, 5.0),
    (1, 113, 145, 1000.0, 2.5),            # 64 * 256 + 1 pixels: one partial block holds a single pixel
    (1, 1024, 1024, 1000.0, 20.0), (2, 1024, 1024, 0.0, 20.0),
    (9000, 7, 9, 0.0, 0.625), (9000, 1, 1, 1000.0, 1.25),     # 8192 / B clamps to one workgroup per image
])
def test_reg_prep_vs_float64(B, H, W, offset, scale, dev):
    g = torch.Generator(device=dev).manual_seed(B + H + W)
    img1 = torch.rand(B, 3, H, W, device=dev, generator=g) - 0.45
    img2 = torch.rand(B, 3, H, W, device=dev, generator=g) - 0.45
    fl = offset + torch.randn(B, 2, H, W, device=dev, generator=g) * (1.0 if offset else 2.0)     # 1000 + N(0,1): the mean cancels
    i1, i2, fl4 = _nhwc(img1, 4), _nhwc(img2, 4), _nhwc(fl, 4)
    misc, mean = _reg_prep(i1, i2, fl4, scale, B, H, W, 1, dev)
    misc0, mean0 = _reg_prep(i1, i2, fl4, scale, B, H, W, 0, dev)
    assert torch.equal(mean, mean0) and torch.equal(misc, misc0), "fused and stand-alone mean must give the same bits"
    assert torch.all(misc[..., 3] == 0)
    fd = fl.double()
    m64, rm64, norm64, nb = ref.reg_prep(img1.double(), img2.double(), fd, scale)
    _within(mean, m64, ref.mean_bound(fd, H * W), OP_BAR, f"reg_prep mean {B}x{H}x{W} offset {offset}")
    rm = misc[..., 1:3].permute(0, 3, 1, 2)
    # rm = u - mean: the subtraction itself is correctly rounded around the kernel's mean; against float64 when the mean is benign
    exact_sub = fd - mean.double().view(B, 2, 1, 1)
    assert bool(((rm.double() - exact_sub).abs() <= ref.U * exact_sub.abs()).all())
    if offset == 0.0:
        _within(rm, rm64, ref.mean_bound(fd, H * W).view(B, 2, 1, 1) + ref.U * rm64.abs(), OP_BAR, "reg_prep rm")
    bar = WARP_BAR
    if max(H, W) > 256 and min(H, W) > 1:          # (the reference's grid is undefined for a size of 1)
        # Past 256 px an fp32 sample position carries up to 6e-5 px of rounding, in the kernel as in the reference's own fp32 grid_sample:
        # the repo's rule for warps there (test_gpu_ops.py::test_channels_last_kernels_vs_oracle_at_launch_sizes) -- no further from
        # float64 than twice the fp32 oracle is, and under 6e-5 of max|out|.
        w32 = orc.backwarp(img2.cpu(), (fl * scale).cpu())
        n32 = (img1.cpu() - w32).pow(2).sum(1).sqrt().double()
        e_orc = float((n32 - norm64.cpu()).abs().max()) / float(norm64.abs().max())
        e_got = float((misc[..., 0].double() - norm64).abs().max()) / float(norm64.abs().max())
        print(f"reg_prep norm {B}x{H}x{W}: |kernel - f64| {e_got:.2e}  |fp32 oracle - f64| {e_orc:.2e}")
        assert e_got <= 2.0 * e_orc + 2e-6, (e_got, e_orc)
        bar = 6e-5
    _within(misc[..., 0], norm64, nb, bar, f"reg_prep norm {B}x{H}x{W} scale {scale}")


# ---- Regularization tail -------------------------------------------------------------------------------------------------------
DSTRIDE = {3: 12, 5: 28, 7: 52}


def _dist(kind, B, KK, H, W, g):
    if kind == "normal":
        return torch.randn(B, KK, H, W, generator=g)
    if kind == "equal":
        return torch.full((B, KK, H, W), 1.7)
    if kind == "zero":
        return torch.zeros(B, KK, H, W)
    if kind == "dominant":      # one channel at 0, the rest at |d| ~ 3: e ~ 1e-4 .. 1e-5 beside 1
        d = 3.0 + 0.3 * torch.randn(B, KK, H, W, generator=g)
        c = torch.randint(0, KK, (B, 1, H, W), generator=g)
        return d.scatter(1, c, 0.0)
    # "large": |d| = 30 + 3 * rank: every channel but the minimum underflows to 0 in fp32
    rank = torch.argsort(torch.rand(B, KK, H, W, generator=g), dim=1).float()
    sign = torch.where(torch.rand(B, KK, H, W, generator=g) < 0.5, -1.0, 1.0)
    return sign * (30.0 + 3.0 * rank)


def _reg_tail(d4, dstride, fl4, wx, wy, bx, by, k, B, H, W, dev, out4=True, nchw=True, out_scale=20.0):
    o4 = torch.full((B, H, W, 4), NAN, device=dev) if out4 else None
    on = torch.full((B, 2, H, W), NAN, device=dev) if nchw else None
    _lib.check(_lib.load().pivlfn_reg_tail(d4.data_ptr(), dstride, fl4.data_ptr(), wx.data_ptr(), wy.data_ptr(), bx, by, k,
                                           o4.data_ptr() if out4 else None, on.data_ptr() if nchw else None, out_scale,
                                           B, H, W, _st(dev)), "reg_tail")
    return o4, on


@pytest.mark.parametrize("kind", ["normal", "equal", "dominant", "zero", "large"])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_reg_tail_vs_float64(k, kind, dev):
    KK, ds = k * k, DSTRIDE[k]
    g = torch.Generator().manual_seed(10 * k + len(kind))
    wx, wy = 0.3 * torch.randn(KK, generator=g), 0.3 * torch.randn(KK, generator=g)
    bx, by = 0.25, -0.125
    for (B, H, W) in [(1, 1, 1), (2, 3, 2), (3, 17, 33), (2, 40, 23)]:      # H, W = 1, < k, not multiples of 16; B > 1
        dist = _dist(kind, B, KK, H, W, g)
        fl = 2.0 * torch.randn(B, 2, H, W, generator=g)
        d4 = _nhwc(dist, ds, NAN).to(dev)           # the padding lanes are never read
        fl4 = _nhwc(fl, 4).to(dev)
        o4, on = _reg_tail(d4, ds, fl4, wx.to(dev), wy.to(dev), bx, by, k, B, H, W, dev)
        want, bound = ref.reg_tail(dist.double(), fl.double(), wx.double(), wy.double(), bx, by, k)
        assert torch.all(o4[..., 2:] == 0)
        _within(o4[..., :2].permute(0, 3, 1, 2).cpu(), want, bound, OP_BAR, f"reg_tail k={k} {kind} {B}x{H}x{W}")
        assert torch.equal(on, o4[..., :2].permute(0, 3, 1, 2) * 20.0), "out_nchw = out_scale * out4, one rounding"
        a4, _ = _reg_tail(d4, ds, fl4, wx.to(dev), wy.to(dev), bx, by, k, B, H, W, dev, nchw=False)
        _, an = _reg_tail(d4, ds, fl4, wx.to(dev), wy.to(dev), bx, by, k, B, H, W, dev, out4=False)
        assert torch.equal(a4, o4) and torch.equal(an, on)


def test_reg_tail_dist_past_2gib(dev):
    """k = 7 over 52-lane distance rows of 10 images of 1024^2: 2.18 GB of dist.  The first and the last image equal those images
    alone bit for bit; the last one matches float64."""
    B, H, W, k, ds = 10, 1024, 1024, 7, 52
    g = torch.Generator(device=dev).manual_seed(5)
    d4 = torch.randn(B, H, W, ds, device=dev, generator=g)
    assert d4.numel() * 4 > 2 ** 31
    fl4 = torch.zeros(B, H, W, 4, device=dev)
    fl4[..., :2] = 2.0 * torch.randn(B, H, W, 2, device=dev, generator=g)
    wx, wy = 0.3 * torch.randn(49, device=dev, generator=g), 0.3 * torch.randn(49, device=dev, generator=g)
    o4, _ = _reg_tail(d4, ds, fl4, wx, wy, 0.25, -0.125, k, B, H, W, dev, nchw=False)
    for b in (0, B - 1):
        one, _ = _reg_tail(d4[b:b + 1].contiguous(), ds, fl4[b:b + 1].contiguous(), wx, wy, 0.25, -0.125, k, 1, H, W, dev, nchw=False)
        assert torch.equal(one[0], o4[b]), b
    dist = d4[B - 1:, ..., :49].permute(0, 3, 1, 2).double()
    fl = fl4[B - 1:, ..., :2].permute(0, 3, 1, 2).double()
    want, bound = ref.reg_tail(dist, fl, wx.double(), wy.double(), 0.25, -0.125, k)
    del dist
    _within(o4[B - 1:, ..., :2].permute(0, 3, 1, 2), want, bound, OP_BAR, "reg_tail k=7 B=10 1024^2, last image")


# ---- mean subtraction and image pyramid ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(1, 32, 32), (2, 64, 96), (3, 160, 224), (1, 1024, 1024)])
def test_prep_pyramid_vs_float64(B, H, W, dev):
    g = torch.Generator().manual_seed(H + W + B)
    img1, img2 = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
    mean6 = [0.411618, 0.434631, 0.454253, 0.310782, 0.533645, 0.152793]      # frame 2's means differ from frame 1's
    m32 = (ctypes.c_float * 6)(*mean6)
    mean6 = [float(np.float32(m)) for m in mean6]                            # the fp32 values the kernel subtracts
    sizes = [2 * B * (H >> L) * (W >> L) * 4 for L in range(6)]
    out = torch.full((sum(sizes),), NAN, device=dev)
    d1, d2 = img1.to(dev), img2.to(dev)
    _lib.check(_lib.load().pivlfn_prep_pyramid(d1.data_ptr(), d2.data_ptr(), m32, out.data_ptr(), B, H, W, 6, _st(dev)), "prep_pyramid")
    want, bounds = ref.pyramid(img1.double(), img2.double(), mean6, 6)
    off = 0
    for L in range(1, 7):
        h, w = H >> (L - 1), W >> (L - 1)
        lv = out[off:off + sizes[L - 1]].view(2 * B, h, w, 4).cpu()
        off += sizes[L - 1]
        assert torch.all(lv[..., 3] == 0)
        _within(lv[..., :3].permute(0, 3, 1, 2), want[L - 1], bounds[L - 1], OP_BAR, f"pyramid {B}x{H}x{W} level {L}")


# ---- NetC.conv1 with level 1's NetC_ext and moduleFeat ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,B_feat,mag,fused", [
    (1, 33, 45, 1, 1.0, False),
    (2, 248, 512, 1, 1.0, False),          # 16 x 31 = 496 tiles of 8 x 32: below the fused kernel's 512
    (2, 256, 512, 1, 1.0, True),           # exactly 512 tiles
    (3, 264, 520, 2, 1.0, True),           # ragged tiles at the right and bottom
    (2, 264, 520, 1, 1e-3, True),
    (2, 264, 520, 1, 1e3, True),
])
def test_conv1_fused_vs_float64(N, H, W, B_feat, mag, fused, dev):
    g = torch.Generator().manual_seed(N * 1000 + H + W + int(np.log10(mag)))
    w1, b1 = (2.0 / 147) ** 0.5 * torch.randn(32, 3, 7, 7, generator=g), 0.1 * torch.randn(32, generator=g)
    we, be = (2.0 / 32) ** 0.5 * torch.randn(64, 32, 1, 1, generator=g), 0.1 * torch.randn(64, generator=g)
    wf, bfe = (2.0 / 32) ** 0.5 * torch.randn(128, 32, 1, 1, generator=g), 0.1 * torch.randn(128, generator=g)
    x = mag * (torch.rand(N, 3, H, W, generator=g) - 0.5)
    x4 = _nhwc(x, 4).to(dev)
    out = torch.full((N, H, W, 32), NAN, device=dev)
    ext = torch.full((N, H, W, 64), NAN, device=dev)
    feat = torch.full((N, H, W, 128), NAN, device=dev)
    ran = ctypes.c_int(-1)
    _lib.check(_lib.load().pivlfn_conv1_fused_nhwc(w1.data_ptr(), b1.data_ptr(), we.data_ptr(), be.data_ptr(), wf.data_ptr(),
                                                   bfe.data_ptr(), x4.data_ptr(), out.data_ptr(), ext.data_ptr(), feat.data_ptr(),
                                                   N, H, W, B_feat, ctypes.byref(ran), _st(dev)), "conv1_fused")
    assert ran.value == int(fused), f"fused kernel ran: {ran.value}, expected {int(fused)}"
    feat = feat.cpu()
    assert torch.isnan(feat[B_feat:]).all(), "moduleFeat rows of frame 2 must keep their sentinel"
    (a, e, f), (ba, be_, bf) = ref.conv1_fused(x.double(), w1.double(), b1.double(), we.double(), be.double(), wf.double(), bfe.double())
    tag = f"{N}x{H}x{W} |x|~{mag:g} fused={int(fused)}"
    _within(out.cpu().permute(0, 3, 1, 2), a, ba, OP_BAR, f"conv1 {tag}")
    _within(ext.cpu().permute(0, 3, 1, 2), e, be_, OP_BAR, f"NetC_ext {tag}")
    _within(feat[:B_feat].permute(0, 3, 1, 2), f[:B_feat], bf[:B_feat], OP_BAR, f"moduleFeat {tag}")
