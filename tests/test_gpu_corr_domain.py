"""GPU: the public custom ops over their whole declared domain -- correlation forward (plain and fused with the back-warp) at
strides 3 and 4 on every kernel, the backward on each of its channel groupings, backwarp at the edges of its tap rule, the bilinear
resize from one pixel to large magnification, estimate() at sizes that are no multiple of 32.

Every comparison is against the float64 restatements of tests/corr_reference.py, computed on the device.  The rule, the one
test_channels_last_kernels_vs_oracle_at_launch_sizes uses for the warp: a kernel may be no further from float64 than TWICE the pinned
fp32 oracle is, plus 2e-6 of max|out| (kernel and oracle are two valid fp32 evaluations; one contracts into fma, the other rounds
each product).  Both distances are printed per case."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pivlfn
import pivlfn_oracle as orc
from corr_reference import backwarp_f64, corr_bwd_f64, fused_f64, resize_f64
from guarded import check_guards, guarded, is_pos_zero, same_bits
from pivlfn import _lib, synth
from test_gpu_net import E2E_MAX, E2E_MEAN

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))


def _within(e_kernel, e_oracle, what):
    assert e_kernel <= 2.0 * e_oracle + 2e-6, f"{what}: |kernel - f64| {e_kernel:.2e} above 2 x |oracle - f64| {e_oracle:.2e} + 2e-6"


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


# ---- forward ---------------------------------------------------------------------------------------------------------------------
def _v6_run_length(tiles_x, tiles_y, B, cus):
    """The run length launch_wc6 (csrc/warp_corr.hip) picks for C = 64; > 1 = the sliding-window kernel."""
    slots = max(8, cus // 8 * 8)
    rl = 1
    r = 2
    while r <= tiles_y:
        n = tiles_x * -(-tiles_y // r) * B
        if n < slots:
            break
        if n % slots == 0 or n >= 4 * slots:
            rl = r
        r *= 2
    return rl


def _nhwc_kernel(B, C, H, W, s, cus):
    """Which channels-last kernel launch_warp_corr selects, and whether v3 walks in strips."""
    tx, ty = -(-(-(-W // s)) // 8), -(-(-(-H // s)) // 8)
    tiles = tx * ty * B
    if C % 64 == 0 and tiles <= cus:
        return "v7"
    if C >= 64:
        return "v6 window" if C == 64 and _v6_run_length(tx, ty, B, cus) > 1 else "v6"
    return "v3 strips" if 14 * s * W * C * 4 > (2 << 20) else "v3"


def _forward_cases(cus):
    """(name, kernel expected for the channels-last call or None for NCHW only, B, C, H, W, stride).  H % s and W % s cover 0, 1 and
    s - 1; three cases have Ho < 8.  The cases with more tiles than CUs and the sliding-window cases are sized from the CU count."""
    t = math.isqrt(cus) + 2                       # t x t tiles of 8 x 8 outputs: more than one per CU (18 x 18 at 256 CUs)
    slots = max(8, cus // 8 * 8)
    # sliding window: 8 tile columns x 2 runs per image, as many images as make the run count at a run length of 2 equal the
    # workgroup count (one per CU, a multiple of 8) -- the smallest launch for which launch_wc6 takes runs of 2.  With 3 tile rows
    # the second run of a column is a single tile; with 4 both are full.
    bw, ty3, ty4 = (slots // 16, 3, 4) if slots % 16 == 0 else (slots // 8, 2, 2)
    return [
        ("nchw32 C=20 s3", None, 2, 20, 19, 31, 3),               # Ho = 7
        ("nchw32 C=33 s4", None, 1, 33, 27, 50, 4),               # Ho = 7, H % 4 = 3
        ("v3 s3", "v3", 2, 32, 45, 64, 3),
        ("v3 s4 strips", "v3 strips", 1, 32, 270, 300, 4),        # 9 tile rows: a strip of 8 and a strip of 1
        ("v3 s4 narrow", "v3", 1, 32, 33, 120, 4),                # W = 120: off the strips walk
        ("v7 C=64 s3", "v7", 1, 64, 90, 89, 3),
        ("v7 C=128 s4", "v7", 1, 128, 61, 75, 4),
        ("v7 C=64 s4 narrow", "v7", 1, 64, 37, 120, 4),
        ("v6 C=96 s3", "v6", 1, 96, 50, 47, 3),
        ("v6 C=96 s4", "v6", 2, 96, 26, 41, 4),                   # Ho = 7
        ("v6 C=64 s3 tiles > CUs", "v6", 1, 64, 3 * (8 * t - 4), 3 * (8 * t - 4) - 1, 3),          # 420 x 419 at 256 CUs
        ("v6 C=64 s4 tiles > CUs", "v6", 1, 64, 4 * (8 * t - 6) - 2, 4 * (8 * t - 4), 4),          # 550 x 560 at 256 CUs
        ("v6 window s3", "v6 window", bw, 64, 3 * (8 * ty3 - 4) - 2, 3 * 61 - 1, 3),               # 16 x 58 x 182 at 256 CUs
        ("v6 window s4", "v6 window", bw, 64, 4 * (8 * ty4 - 3) - 3, 4 * 64 - 3, 4),               # 16 x 113 x 253 at 256 CUs
    ]


N_FORWARD = 14


def _fwd_inputs(B, C, H, W, seed):
    g = np.random.default_rng(seed)
    f1 = g.standard_normal((B, C, H, W)).astype(np.float32)
    f2 = g.standard_normal((B, C, H, W)).astype(np.float32)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    fl = np.stack([3.0 * np.sin(yy / 17.0), 2.5 * np.cos(xx / 23.0)])[None] + 0.7 * g.standard_normal((B, 2, H, W))
    fl = fl.astype(np.float32)
    fl[:, :, :3, :] += 4.0                               # the top rows point far outside
    return f1, f2, fl


def _call_nchw(t1, t2, tf, scale, s, leaky, dev):
    B, C, H, W = t1.shape
    out = torch.full((B, 49, -(-H // s), -(-W // s)), float("nan"), device=dev)
    _lib.check(_lib.load().pivlfn_warp_corr_fwd(t1.data_ptr(), t2.data_ptr(), tf.data_ptr() if tf is not None else None, scale,
                                                out.data_ptr(), B, C, H, W, s, leaky, _st(dev)), "warp_corr_fwd")
    return out


def _call_nhwc(a, b, f4, scale, s, leaky, dev):
    B, H, W, C = a.shape
    out = torch.full((B, -(-H // s), -(-W // s), 56), float("nan"), device=dev)
    _lib.check(_lib.load().pivlfn_warp_corr_nhwc(a.data_ptr(), b.data_ptr(), f4.data_ptr() if f4 is not None else None, scale,
                                                 out.data_ptr(), B, C, H, W, s, leaky, _st(dev)), "warp_corr_nhwc")
    assert bool(is_pos_zero(out[..., 49:]).all()), "the 7 padding lanes must be +0.0"
    return out


def _lrelu(x):
    return np.where(x >= 0, x, 0.1 * x)


@pytest.mark.parametrize("case", range(N_FORWARD))
def test_forward_strides_3_and_4_on_every_kernel(case, dev):
    """pivlfn_corr_fwd, pivlfn_warp_corr_fwd and pivlfn_warp_corr_nhwc at strides 3 and 4, with flow and with flow = NULL, leaky 0
    and 1, on the NCHW <64> and <32> kernels and on channels-last v3 (with and without the strips walk), v7, v6 and v6 with the sliding
    window -- the test works out which kernel the launch policy selects from the device's CU count and asserts it is the one the
    case is there for.  Flows: smooth plus noise, top rows pointing far outside, so taps leave the image on every side.  Also: the two
    layouts agree to 3e-6, the padding lanes are +0.0, image 0 of a batch equals that image alone bit for bit.

    Measured values: none recorded yet -- this test has not run on an MI355X; it prints |kernel - f64| (both layouts) and
    |oracle - f64| for every case and combination, to be copied here from its first run.  On the CPU the oracle paths were measured
    at 0.8e-7 .. 2.0e-7 (plain) and 4e-7 .. 5.5e-6 (with the warp) of max|out|."""
    cus = _cus(dev)
    cases = _forward_cases(cus)
    assert len(cases) == N_FORWARD
    name, kernel, B, C, H, W, s = cases[case]
    if kernel is not None:
        assert _nhwc_kernel(B, C, H, W, s, cus) == kernel, (name, _nhwc_kernel(B, C, H, W, s, cus))
    f1, f2, fl = _fwd_inputs(B, C, H, W, 1000 + case)
    scale = 1.25
    t1, t2, tf = (torch.from_numpy(a).to(dev) for a in (f1, f2, fl))
    if kernel is not None:
        a, b = t1.permute(0, 2, 3, 1).contiguous(), t2.permute(0, 2, 3, 1).contiguous()
        f4 = torch.zeros(B, H, W, 4, device=dev)
        f4[..., :2] = tf.permute(0, 2, 3, 1)
    for warp in (True, False):
        exact = fused_f64(f1, f2, fl if warp else None, scale, s, leaky=False, device=dev)
        want = orc.correlation_c(f1, orc.backwarp_c(f2, fl * np.float32(scale)) if warp else f2, s)
        for leaky in (1, 0):
            ex, wa = (_lrelu(exact), _lrelu(want).astype(np.float32)) if leaky else (exact, want)
            e_orc = rel(wa, ex)
            tag = f"{name} {'flow' if warp else 'no flow'} leaky {leaky}"
            nchw = _call_nchw(t1, t2, tf if warp else None, scale, s, leaky, dev)
            e_nchw = rel(nchw.cpu().numpy(), ex)
            line = f"{tag} ({B}, {C}, {H}, {W}): |NCHW kernel - f64| {e_nchw:.2e}  |oracle - f64| {e_orc:.2e}"
            if kernel is not None:
                nhwc = _call_nhwc(a, b, f4 if warp else None, scale, s, leaky, dev)
                got = nhwc[..., :49].permute(0, 3, 1, 2).contiguous()
                e_nhwc = rel(got.cpu().numpy(), ex)
                line += f"  |{kernel} kernel - f64| {e_nhwc:.2e}  |NHWC - NCHW| {rel(got.cpu().numpy(), nchw.cpu().numpy()):.2e}"
            print(line)
            _within(e_nchw, e_orc, tag + " NCHW")
            if kernel is not None:
                _within(e_nhwc, e_orc, tag + " " + kernel)
                assert rel(got.cpu().numpy(), nchw.cpu().numpy()) < 3e-6, tag
            if not warp and not leaky:           # the plain op: the same launch through pivlfn_corr_fwd
                plain = torch.full_like(nchw, float("nan"))
                _lib.check(_lib.load().pivlfn_corr_fwd(t1.data_ptr(), t2.data_ptr(), plain.data_ptr(), B, C, H, W, s, _st(dev)), "corr_fwd")
                assert same_bits(plain, nchw), tag
                assert same_bits(pivlfn.FunctionCorrelation(t1, t2, s), nchw), tag
            if warp and leaky and B > 1:         # image 0 alone (for the window cases: another kernel, v7) equals image 0 of the batch
                one = _call_nchw(t1[:1], t2[:1], tf[:1], scale, s, leaky, dev)
                assert same_bits(one[0], nchw[0]), tag + " NCHW: image 0 alone differs from image 0 of the batch"
                if kernel is not None:
                    one = _call_nhwc(a[:1], b[:1], f4[:1], scale, s, leaky, dev)
                    assert same_bits(one[0], nhwc[0]), tag + f" {kernel}: image 0 alone differs from image 0 of the batch"


def test_forward_refuses_strides_outside_1_to_4(dev):
    lib = _lib.load()
    x = torch.zeros(1, 32, 8, 8, device=dev)
    out = torch.zeros(1, 49 + 7, 8, 8, device=dev)
    for s in (0, -1, 5):
        assert lib.pivlfn_corr_fwd(x.data_ptr(), x.data_ptr(), out.data_ptr(), 1, 32, 8, 8, s, _st(dev)) == 1
        assert lib.pivlfn_warp_corr_fwd(x.data_ptr(), x.data_ptr(), None, 1.0, out.data_ptr(), 1, 32, 8, 8, s, 0, _st(dev)) == 1
        assert lib.pivlfn_warp_corr_nhwc(x.data_ptr(), x.data_ptr(), None, 1.0, out.data_ptr(), 1, 32, 8, 8, s, 0, _st(dev)) == 1
        assert lib.pivlfn_corr_bwd(x.data_ptr(), x.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), 1, 32, 8, 8, s, _st(dev)) == 1
        assert b"stride" in lib.pivlfn_last_error()
        with pytest.raises(ValueError, match="1..4"):
            pivlfn.FunctionCorrelation(x, x, s)


# ---- backward --------------------------------------------------------------------------------------------------------------------
def _cgroup(B, C, H, W, s):
    """The channel group launch_corr_bwd (csrc/corr_bwd.hip) picks: 16, halved down to 4 while tiles * cdiv(C, cgroup) * B < 2048."""
    tiles = -(-(-(-W // s)) // 16) * -(-(-(-H // s)) // 16)
    cg = 16
    while cg > 4 and tiles * -(-C // cg) * B < 2048:
        cg >>= 1
    return cg


def _grads(f1, f2, go, s, dev, need=(True, True)):
    a = torch.from_numpy(f1).to(dev).requires_grad_(need[0])
    b = torch.from_numpy(f2).to(dev).requires_grad_(need[1])
    pivlfn.FunctionCorrelation(a, b, s).backward(torch.from_numpy(go).to(dev))
    return a.grad, b.grad


def _bwd_inputs(B, C, H, W, s, seed):
    g = np.random.default_rng(seed)
    f1 = g.standard_normal((B, C, H, W)).astype(np.float32)
    f2 = g.standard_normal((B, C, H, W)).astype(np.float32)
    go = g.standard_normal((B, 49, -(-H // s), -(-W // s))).astype(np.float32)
    return f1, f2, go


@pytest.mark.parametrize("shape,cgroup", [
    ((2, 72, 256, 256, 1), 16),      # 256 tiles x 5 groups x 2 = 2560 >= 2048: groups of 16, a ragged last group of 8 channels
    ((2, 64, 256, 128, 1), 8),       # 128 tiles: 4 groups of 16 x 2 = 1024 < 2048, 8 groups of 8 x 2 = 2048: groups of 8
    ((2, 60, 256, 128, 1), 8),       # the same with a ragged last group of 4 channels
    ((1, 16, 50, 50, 3), 4),         # 2 x 2 tiles
    ((2, 33, 37, 50, 4), 4),         # one tile, a ragged last group of 1 channel
    ((2, 20, 31, 45, 2), 4),         # stride 2, 2 x 1 tiles
    ((1, 7, 1, 1, 4), 4),            # one pixel
])
def test_backward_every_channel_grouping(shape, cgroup, dev):
    """pivlfn_corr_bwd on each channel grouping of launch_corr_bwd (the grouping each shape selects is worked out beforehand and
    asserted against the library's own answer, so that a change of the policy is noticed).  First into sentinel-filled guarded
    buffers: every element written, every off-grid element an exact zero, guards intact.  Then through
    FunctionCorrelation(...).backward against corr_bwd_f64; the two calls agree bit for bit.

    Measured values: none recorded yet -- this test has not run on an MI355X; it prints both distances per shape and gradient.  On
    the CPU the oracle's gradients were measured at 2.2e-7 .. 3.5e-7 of max|grad| from float64 at strides 1..4."""
    B, C, H, W, s = shape
    assert _cgroup(*shape) == cgroup
    assert _lib.load().pivlfn_corr_bwd_channel_group(*shape) == cgroup, "launch_corr_bwd's policy changed: re-derive the shapes of this test"
    f1, f2, go = _bwd_inputs(B, C, H, W, s, 7 * C + H)
    # first into guarded buffers -- written in full, nothing outside; the guards are wide enough for a whole group of 16 channel
    # planes, so that a group running past C is seen here, before any launch into plain tensors
    lib = _lib.load()
    gb = max(1 << 20, 16 * H * W * 4)
    ins = []
    for arr in (f1, f2, go):
        t = guarded(arr.shape, torch.float32, dev, "nan", guard_bytes=gb)
        t.copy_(torch.from_numpy(arr))
        ins.append(t)
    o1 = guarded((B, C, H, W), torch.float32, dev, "sentinel", guard_bytes=gb)
    o2 = guarded((B, C, H, W), torch.float32, dev, "sentinel", guard_bytes=gb)
    _lib.check(lib.pivlfn_corr_bwd(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), o1.data_ptr(), o2.data_ptr(),
                                   B, C, H, W, s, _st(dev)), "corr_bwd")
    torch.cuda.synchronize()
    for t in ins + [o1, o2]:
        check_guards(t, f"corr_bwd {shape}")
    x1, x2 = corr_bwd_f64(f1, f2, go, s, device=dev)
    w1, w2 = orc.correlation_backward_c(f1, f2, go, s)
    g1, g2 = _grads(f1, f2, go, s, dev)
    for name, got, want, exact in (("gradFirst", g1, w1, x1.cpu().numpy()), ("gradSecond", g2, w2, x2.cpu().numpy())):
        e_k, e_o = rel(got.cpu().numpy(), exact), rel(want, exact)
        print(f"{shape} cgroup {cgroup} {name}: |kernel - f64| {e_k:.2e}  |oracle - f64| {e_o:.2e}")
        _within(e_k, e_o, f"{shape} {name}")
    assert same_bits(o1, g1) and same_bits(o2, g2)
    assert not torch.isnan(o1).any() and not torch.isnan(o2).any()
    if s > 1:
        off = torch.ones(H, W, dtype=torch.bool, device=dev)
        off[::s, ::s] = False
        assert bool((o1[:, :, off] == 0).all()) and bool((o2[:, :, off] == 0).all())


def test_backward_batch_invariance_across_channel_groupings(dev):
    """Image 0 of a batch of 8 (groups of 16 channels) equals the same image alone (groups of 4) bit for bit: a thread sums its 49
    terms per channel, the grouping only decides which workgroup handles a channel."""
    B, C, H, W, s = 8, 72, 255, 250, 2
    assert _cgroup(B, C, H, W, s) == 16 and _cgroup(1, C, H, W, s) == 4
    lib = _lib.load()
    assert lib.pivlfn_corr_bwd_channel_group(B, C, H, W, s) == 16 and lib.pivlfn_corr_bwd_channel_group(1, C, H, W, s) == 4
    f1, f2, go = _bwd_inputs(B, C, H, W, s, 5)
    g1, g2 = _grads(f1, f2, go, s, dev)
    for k in (0, B - 1):
        o1, o2 = _grads(f1[k:k + 1], f2[k:k + 1], go[k:k + 1], s, dev)
        assert same_bits(o1[0], g1[k]) and same_bits(o2[0], g2[k]), k


def test_backward_needs_input_grad_on_groups_of_16(dev):
    shape = (2, 72, 256, 256, 1)
    assert _cgroup(*shape) == 16 and _lib.load().pivlfn_corr_bwd_channel_group(*shape) == 16
    f1, f2, go = _bwd_inputs(*shape, 9)
    full1, full2 = _grads(f1, f2, go, 1, dev)
    only1, none2 = _grads(f1, f2, go, 1, dev, need=(True, False))
    none1, only2 = _grads(f1, f2, go, 1, dev, need=(False, True))
    assert none1 is None and none2 is None
    assert same_bits(only1, full1) and same_bits(only2, full2)


# ---- backwarp, NCHW --------------------------------------------------------------------------------------------------------------
def _backwarp(x, fl, dev):
    return pivlfn.backwarp(tensorInput=x.to(dev), tensorFlow=fl.to(dev))


def test_backwarp_at_the_edges_of_the_tap_rule(dev):
    """pivlfn_backwarp at a ragged 130 x 70, C = 5, B = 2 against backwarp_f64: random flows; integer flows (the shifted input, bit
    for bit); sample positions exactly at -1, -0.5, W - 1, W - 0.5 and H - 1; flows of +-1e6 and +-1e30 (all zeros); a NaN flow
    component (a zero pixel: make_taps clamps with fmaxf / fminf, which drop the NaN, so no tap is inside the image).

    Measured values: none recorded yet -- this test has not run on an MI355X; it prints both distances."""
    B, C, H, W = 2, 5, 130, 70
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, C, H, W, generator=g)
    fl = 3.0 * torch.randn(B, 2, H, W, generator=g)
    fl[:, 1, :4] -= 6.0
    fl[:, 0, :, -4:] += 6.0
    exact = backwarp_f64(x, fl, device=dev).cpu().numpy()
    want = orc.backwarp_c(x.numpy(), fl.numpy())
    got = _backwarp(x, fl, dev).cpu().numpy()
    e_k, e_o = rel(got, exact), rel(want, exact)
    print(f"backwarp {B, C, H, W}: |kernel - f64| {e_k:.2e}  |oracle - f64| {e_o:.2e}")
    _within(e_k, e_o, "backwarp")

    # integer flows: out[y, x] = in[y + v, x + u] where inside, zero elsewhere, exactly
    for u, v in [(0, 0), (1, 0), (-3, 2), (7, -5), (W - 1, H - 1), (-W, 0), (0, H)]:
        fi = torch.zeros(B, 2, H, W)
        fi[:, 0], fi[:, 1] = float(u), float(v)
        shifted = torch.zeros_like(x)
        ys, xs = slice(max(0, -v), min(H, H - v)), slice(max(0, -u), min(W, W - u))
        if ys.start < ys.stop and xs.start < xs.stop:
            shifted[:, :, ys, xs] = x[:, :, ys.start + v:ys.stop + v, xs.start + u:xs.stop + u]
        assert same_bits(_backwarp(x, fi, dev).cpu(), shifted), (u, v)

    # every pixel of a column / row samples exactly at the stated position
    xx = torch.arange(W, dtype=torch.float32).view(1, 1, W).expand(B, H, W)
    yy = torch.arange(H, dtype=torch.float32).view(1, H, 1).expand(B, H, W)
    for axis, pos in [(0, -1.0), (0, -0.5), (0, W - 1.0), (0, W - 0.5), (1, -1.0), (1, -0.5), (1, H - 1.0), (1, H - 0.5)]:
        fe = torch.zeros(B, 2, H, W)
        fe[:, axis] = pos - (xx if axis == 0 else yy)
        got = _backwarp(x, fe, dev)
        ex = backwarp_f64(x, fe, device=dev)
        assert float((got.double() - ex).abs().max()) <= 1e-7 * float(x.abs().max()), (axis, pos)      # weights 0, 0.5 and 1 are exact
        if pos == -1.0:
            assert bool((got == 0).all())

    for big in (1e6, -1e6, 1e30, -1e30):
        for comp in (0, 1):
            fb = torch.zeros(B, 2, H, W)
            fb[:, comp] = big
            assert bool((_backwarp(x, fb, dev) == 0).all()), (big, comp)

    fn = fl.clone()
    fn[0, 0, 5, 7] = float("nan")
    fn[1, 1, 100, 33] = float("nan")
    fn[1, :, 129, 69] = float("nan")
    got = _backwarp(x, fn, dev)
    ex = backwarp_f64(x, fn, device=dev)
    assert not torch.isnan(got).any()
    assert bool((got[0, :, 5, 7] == 0).all()) and bool((got[1, :, 100, 33] == 0).all()) and bool((got[1, :, 129, 69] == 0).all())
    assert rel(got.cpu().numpy(), ex.cpu().numpy()) <= 2.0 * e_o + 2e-6


# ---- resize ----------------------------------------------------------------------------------------------------------------------
def _resize(x, size, mul, dev):
    B, C, H, W = x.shape
    out = torch.full((B, C) + tuple(size), float("nan"), device=dev)
    m = (ctypes.c_float * 2)(*mul) if mul is not None else None
    _lib.check(_lib.load().pivlfn_resize_bilinear(x.data_ptr(), out.data_ptr(), B, C, H, W, size[0], size[1], m, _st(dev)), "resize")
    return out


RESIZES = [((1, 1), (64, 64)), ((37, 53), (1, 1)), ((2, 3), (100, 7)), ((1, 70), (32, 64)), ((70, 1), (64, 32)),
           ((37, 53), (37, 53)), ((32, 32), (100, 76)), ((128, 96), (100, 76)), ((3, 1000), (7, 333)), ((255, 257), (256, 256))]


@pytest.mark.parametrize("src,size", RESIZES)
def test_resize_bilinear_over_its_domain(src, size, dev):
    """pivlfn_resize_bilinear against resize_f64, with mul = (0.5, 3.0) on 4 channels and mul = NULL on 3; the oracle is torch's CPU
    fp32 interpolate.  Where torch's fp32 result is float64's exactly (1 x 1 -> 64 x 64, same size) the bound is the 2e-6 term
    alone; a same-size resize returns the input bit for bit.

    Measured values: none recorded yet for the kernel -- this test has not run on an MI355X; it prints both distances.  Torch's fp32
    resize against float64 was measured on the CPU between 0 and 6.1e-5 of max|out| on these shapes."""
    for C, mul in ((4, (0.5, 3.0)), (3, None)):
        x = torch.randn(2, C, *src, generator=torch.Generator().manual_seed(C + src[0] + size[1]))
        xd = x.to(dev)
        exact = resize_f64(xd, size, mul).cpu().numpy()
        want = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
        if mul is not None:
            want[:, 0::2] *= mul[0]
            want[:, 1::2] *= mul[1]
        got = _resize(xd, size, mul, dev)
        e_k, e_o = rel(got.cpu().numpy(), exact), rel(want.numpy(), exact)
        print(f"resize {src} -> {size} mul {mul}: |kernel - f64| {e_k:.2e}  |torch fp32 - f64| {e_o:.2e}")
        _within(e_k, e_o, f"resize {src} -> {size} mul {mul}")
        if src == size and mul is None:
            assert same_bits(got, xd)


def test_resize_multiplier_needs_an_even_channel_count(dev):
    x = torch.zeros(1, 3, 4, 4, device=dev)
    out = torch.zeros(1, 3, 8, 8, device=dev)
    mul = (ctypes.c_float * 2)(0.5, 3.0)
    assert _lib.load().pivlfn_resize_bilinear(x.data_ptr(), out.data_ptr(), 1, 3, 4, 4, 8, 8, mul, _st(dev)) == 1      # PIVLFN_ERR_ARG


# ---- estimate() ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets(dev):
    return {m: pivlfn.Network(model=m, params=synth.generate_weights(m, 0)).to(dev).eval() for m in ("piv", "hui")}


@pytest.mark.parametrize("model", ["piv", "hui"])
@pytest.mark.parametrize("H,W", [(72, 100), (33, 95), (96, 50)])
def test_estimate_at_sizes_no_multiple_of_32(model, H, W, nets, dev):
    """estimate(): resize up to a multiple of 32, forward, resize back with the flow rescaled -- against the oracle's estimate()
    on the CPU with the end-to-end tolerance of test_gpu_net.py."""
    a, b = synth.particle_batch(2, H, W, seed=H + W)
    i1, i2 = torch.from_numpy(a), torch.from_numpy(b)
    want = orc.estimate(orc.make_net(model, synth.generate_weights(model, 0), corr="c"), i1, i2, tensor=True).numpy().astype(np.float64)
    got = pivlfn.estimate(nets[model], i1.to(dev), i2.to(dev), tensor=True)
    assert tuple(got.shape) == (2, 2, H, W)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    scale = max(1.0, np.abs(want).max())
    print(f"estimate {model} {H} x {W}: max-abs {err.max():.2e}  mean-abs {err.mean():.2e}  at flow scale {scale:.2f}")
    assert err.max() <= E2E_MAX * scale and err.mean() <= E2E_MEAN * scale, (err.max(), err.mean(), scale)
