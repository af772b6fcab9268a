"""GPU: what each entry point reads and writes OUTSIDE the elements it is meant to touch (tests/guarded.py).

Every input and output of a call lives in a guarded buffer: 256-byte aligned, its last byte directly against a back guard, guards of
max(1 MiB, 32 rows) on both sides.  The lanes a contract in include/pivlfn.h says are unused are poisoned, once with a NaN and once
with a finite ~1e30 pattern (a clamp such as fminf / fmaxf would hide a NaN); lanes it requires to be finite get that finite pattern
or zero.  Outputs are pre-filled with a sentinel.  After the call each test asserts
  (a) the guards are bitwise intact,
  (b) lanes that are not stored still hold the sentinel and lanes stated to be exact zeros hold +0.0,
  (c) the result meets the existing float64 / oracle bar of that op (on the plain call of (d), which it equals),
  (d) the result is bit-identical to the same call on zero-padded, unguarded inputs, as the existing tests build them.
The whole forward runs on a workspace filled with zeros, NaN and the finite poison (including the alignment gaps between its
buffers): flows and per-level flows must be bit-identical, and the guards around the workspace, the images, flow and levels intact."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pivlfn
import pivlfn_oracle as orc
from pivlfn import _lib, synth
from pivlfn.models import LiteFlowNet2
from pivlfn.synth import MODEL_CFG
import net_ops_reference as ref
from guarded import KINDS, check_guards, check_lanes, guarded, poison, same_bits
from test_conv_head_plan import plan as head_plan
from test_gpu_conv import Conv
from test_gpu_net_ops import OP_BAR, WARP_BAR, _nhwc, _within
from test_gpu_wino import CAT_CASES
from stereo_restatement import restate
from pivlfn import stereo

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _r(n, m):
    return -(-n // m) * m


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))


# ---- convolutions ------------------------------------------------------------------------------------------------------------
def _launch(kernel, conv, x, xs, y, ys, B, H, W, s, pad, leaky, dev, res=None, terms=6, x16=0):
    lib, st = _lib.load(), _st(dev)
    if kernel == "direct":
        rc = lib.pivlfn_conv2d_nhwc(conv.h, x.data_ptr(), xs, y.data_ptr(), ys, res.data_ptr() if res is not None else None, ys,
                                    B, H, W, s, pad[0], pad[1], leaky, st)
    elif kernel == "wino":
        rc = lib.pivlfn_conv2d_nhwc_wino(conv.h, x.data_ptr(), xs, y.data_ptr(), ys, B, H, W, leaky, st)
    elif kernel == "b3":
        rc = lib.pivlfn_conv2d_nhwc_wino_b3(conv.h, x.data_ptr(), xs, y.data_ptr(), ys, B, H, W, leaky, terms, st)
    elif kernel == "split":
        rc = lib.pivlfn_conv2d_nhwc_split(conv.h, x.data_ptr(), xs, y.data_ptr(), ys, B, H, W, s, pad[0], pad[1], leaky, terms, st)
    else:
        rc = lib.pivlfn_conv2d_nhwc_f16(conv.h, x.data_ptr(), xs, x16, y.data_ptr(), ys, 0, B, H, W, s, pad[0], pad[1], leaky, st)
    _lib.check(rc, kernel)


def _conv64(x, w, b, s, pad, on):
    """torch's float64 convolution, on the CPU or -- for the cases that take the CPU many seconds -- on the device"""
    return F.conv2d(x.double().to(on), w.double().to(on), b.double().to(on), stride=s, padding=pad).cpu()


def _conv_case(kernel, case, dev, terms=6, x16=0, ref_on_device=False):
    """case: cout, cin, kh, kw, stride, pad, H, W, B, x lanes past roundup(cin), y lanes past roundup(cout, 4), residual.
    ref_on_device: the float64 reference is computed by torch on the GPU (the same torch convolution; not the library under test).
    Returns the layer, its inputs and the plain call's result for the tests that go on with them (tests/test_gpu_conv_tiles.py)."""
    co, ci, kh, kw, s, pad, H, W, B, xextra, yextra, with_res = case
    g = torch.Generator().manual_seed(co * 1000 + ci + kh * 7 + H + B + terms + 3 * x16)
    w = torch.randn(co, ci, kh, kw, generator=g) / (ci * kh * kw) ** 0.5
    b = torch.randn(co, generator=g) * 0.1
    x = torch.randn(B, ci, H, W, generator=g)
    conv = Conv(w, b)
    Ho, Wo = (H + 2 * pad[0] - kh) // s + 1, (W + 2 * pad[1] - kw) // s + 1
    res = torch.randn(B, co, Ho, Wo, generator=g) if with_res else None
    ri = _r(ci, 8 if x16 else 4)                        # lanes ci..ri must be finite; the kernel's weights there are zero
    xs, cs = ri + xextra, _r(co, 4)
    ys = cs + yextra
    xdt = torch.float16 if x16 else torch.float32
    # the split and fp16 kernels round the finite lanes to fp16: they get zeros, the fp32 kernels the finite poison
    tail_big = kernel not in ("split", "f16")
    # the 7 x 1 / 1 x 7 layers reach their streaming kernels (>= 256 x 256) only without an activation, as conv_dist_R.0 / .1
    leaky = 0 if kernel == "direct" and sorted((kh, kw)) == [1, 7] else 1

    def call(kind):
        if kind is None:                                # the existing tests' inputs: zero-padded, unguarded
            xd = torch.zeros(B, H, W, xs, dtype=xdt, device=dev)
            yd = torch.full((B, Ho, Wo, ys), NAN, device=dev)
            rd = torch.zeros(B, Ho, Wo, ys, device=dev) if with_res else None
        else:
            xd = guarded((B, H, W, xs), xdt, dev, kind)
            xd[..., ci:ri] = 0.0
            if kind == "big" and tail_big:
                poison(xd, slice(ci, ri), "big")
            poison(xd, slice(ri, xs), kind)
            yd = guarded((B, Ho, Wo, ys), torch.float32, dev, "sentinel")
            rd = None
            if with_res:                                # lanes co..cs are added into y's zero lanes: +0.0; lanes past them unread
                rd = poison(guarded((B, Ho, Wo, ys), torch.float32, dev, kind), slice(cs, ys), kind)
                rd[..., co:cs] = 0.0
        xd[..., :ci] = x.permute(0, 2, 3, 1).to(dev, xdt)
        if with_res:
            rd[..., :co] = res.permute(0, 2, 3, 1).to(dev)
        _launch(kernel, conv, xd, xs, yd, ys, B, H, W, s, pad, leaky, dev, rd, terms, x16)
        torch.cuda.synchronize()
        if kind is not None:
            tag = f"{kernel} {case} {kind}"
            for t in (xd, yd) + ((rd,) if with_res else ()):
                check_guards(t, tag)
            check_lanes(yd, slice(co, cs), "zero", tag)
            check_lanes(yd, slice(cs, ys), "sentinel", tag)
        return yd[..., :co].cpu()

    plain = call(None)
    on = dev if ref_on_device else "cpu"
    if kernel == "f16":
        assert pad == (kh // 2, kw // 2) and leaky
        want = F.leaky_relu(_conv64(x.half(), w.half(), b, s, pad, on), 0.1)      # test_gpu_f16.py::_ref; fp32 x too is rounded to fp16 when staged
        bar = 2e-5
    else:
        want = _conv64(x, w, b, s, pad, on)
        if with_res:
            want = want + res.double()
        want = F.leaky_relu(want, 0.1) if leaky else want
        bar = 2e-5 if kernel in ("direct", "split") else 1e-5
    err = (plain.permute(0, 3, 1, 2).double() - want).abs().max().item()
    assert err < bar * max(1.0, want.abs().max().item()), (kernel, case, err)
    for kind in KINDS:
        assert same_bits(call(kind), plain), f"{kernel} {case}: {kind}-poisoned, guarded call differs from the plain call"
    return SimpleNamespace(conv=conv, x=x, res=res, xs=xs, ys=ys, leaky=leaky, plain=plain)


DIRECT = [
    # cout, cin, kh, kw, stride, pad, H, W, B, x extra lanes, y extra lanes, residual
    (32, 3, 7, 7, 1, (3, 3), 261, 530, 1, 4, 0, False),       # NetC.conv1, taps packed into K
    (32, 32, 3, 3, 2, (1, 1), 262, 530, 1, 8, 4, False),      # the whole-line stride-2 kernel
    (64, 32, 3, 3, 2, (1, 1), 261, 529, 2, 0, 0, False),      # the same, odd size, B = 2, x flush against its back guard
    (49, 32, 7, 1, 1, (3, 0), 300, 261, 2, 4, 4, False),      # streaming 7 x 1 kernel
    (49, 49, 1, 7, 1, (0, 3), 261, 300, 2, 4, 0, False),      # streaming 1 x 7 kernel
    (128, 386, 3, 3, 1, (1, 1), 8, 8, 1, 8, 0, False),        # split-K on a small grid
    (9, 32, 3, 3, 1, (1, 1), 8, 8, 3, 0, 4, False),           # split-K, cout 9: lanes 9..11 zero
    (30, 32, 3, 3, 1, (1, 1), 20, 36, 1, 8, 4, True),         # residual: its lanes 30..35 poisoned, y lanes 30, 31 zero
    (2, 32, 7, 7, 1, (3, 3), 32, 48, 1, 0, 0, True),          # flow head on the matrix-core path with a residual
]


@pytest.mark.parametrize("case", DIRECT)
def test_direct_conv_guarded(case, dev):
    _conv_case("direct", case, dev)


WINO = [
    # cout, cin, H, W, B, x extra lanes, y extra lanes
    (128, 49, 33, 47, 1, 0, 4),       # partial last K step, x flush, H, W not multiples of 16
    (64, 20, 16, 16, 1, 4, 0),        # a single 16 x 16 tile
    (128, 36, 37, 29, 3, 0, 0),       # B = 3, the last image flush against the back guard
    (128, 386, 8, 8, 1, 8, 0),
    (192, 40, 100, 90, 1, 0, 4),      # cout 192
    (64, 64, 130, 70, 1, 0, 0),
    (64, 32, 300, 310, 1, 4, 0),      # 19 x 20 tiles of 16: not a multiple of the CU count
]


def _w(c):
    co, ci, H, W, B, xe, ye = c
    return (co, ci, 3, 3, 1, (1, 1), H, W, B, xe, ye, False)


@pytest.mark.parametrize("case", WINO)
def test_wino_guarded(case, dev):
    _conv_case("wino", _w(case), dev)


@pytest.mark.parametrize("case", WINO)
def test_wino_b3_guarded(case, dev):
    _conv_case("b3", _w(case), dev, terms=6)


SPLIT = [
    (128, 49, 3, 3, 1, (1, 1), 64, 64, 1, 0, 4, False),
    (64, 36, 3, 3, 1, (1, 1), 37, 45, 2, 4, 0, False),
    (64, 20, 3, 3, 1, (1, 1), 16, 16, 1, 4, 0, False),
    (128, 130, 3, 3, 1, (1, 1), 64, 64, 1, 0, 0, False),
    (49, 32, 7, 1, 1, (3, 0), 96, 96, 1, 4, 4, False),
]


@pytest.mark.parametrize("terms", [6, 3])
@pytest.mark.parametrize("case", SPLIT)
def test_split_guarded(case, terms, dev):
    _conv_case("split", case, dev, terms=terms)


F16 = [
    (64, 36, 3, 3, 1, (1, 1), 37, 45, 2, 8, 4, False),
    (128, 49, 3, 3, 1, (1, 1), 33, 47, 1, 0, 0, False),
    (64, 20, 3, 3, 2, (1, 1), 66, 50, 1, 8, 0, False),
    (32, 3, 7, 7, 1, (3, 3), 40, 72, 1, 0, 4, False),
]


@pytest.mark.parametrize("x16", [0, 1])
@pytest.mark.parametrize("case", F16)
def test_f16_guarded(case, x16, dev):
    _conv_case("f16", case, dev, x16=x16)


def test_split_k_scratch_in_the_handle(dev):
    """conv_create's own split-K scratch: after a call on 1e30-scaled input, the same handle's next call equals a fresh handle's."""
    co, ci, H, W = 128, 386, 8, 8
    g = torch.Generator().manual_seed(44)
    w = torch.randn(co, ci, 3, 3, generator=g) / (ci * 9) ** 0.5
    b = torch.randn(co, generator=g) * 0.1
    x = torch.randn(1, H, W, ci + 2, generator=g)
    x[..., ci:] = 0
    used, fresh = Conv(w, b), Conv(w, b)

    def call(conv, xin):
        xd = guarded(xin.shape, torch.float32, dev, "nan")
        xd.copy_(xin.to(dev))
        yd = guarded((1, H, W, co), torch.float32, dev, "sentinel")
        _launch("direct", conv, xd, ci + 2, yd, co, 1, H, W, 1, (1, 1), 1, dev)
        torch.cuda.synchronize()
        check_guards(xd, "split-K input")
        check_guards(yd, "split-K output")
        return yd.cpu()

    call(used, x * 1e30)
    assert same_bits(call(used, x), call(fresh, x))


def test_images_of_2_gib_and_more_per_source_b3(dev):
    """The b3 case of test_gpu_conv.py::test_images_of_2_gib_and_more_per_source: 264 x 260 pixels x 8192 lanes (2.25 GB) for 8 real
    channels, cout 64; lanes 8.. NaN-poisoned, the tensor guarded."""
    H, W, ci, co, xs = 264, 260, 8, 64, 8192
    g = torch.Generator().manual_seed(5)
    w = torch.randn(co, ci, 3, 3, generator=g) / (ci * 9) ** 0.5
    b = torch.randn(co, generator=g) * 0.1
    x = torch.randn(1, ci, H, W, generator=g)
    conv = Conv(w, b)
    xd = guarded((1, H, W, xs), torch.float32, dev, "nan")
    xd[..., :ci] = x.permute(0, 2, 3, 1).to(dev)
    assert xd.numel() * 4 >= 2 ** 31
    y = guarded((1, H, W, co), torch.float32, dev, "sentinel")
    _launch("b3", conv, xd, xs, y, co, 1, H, W, 1, (1, 1), 1, dev, terms=6)
    torch.cuda.synchronize()
    check_guards(xd, "b3 2 GiB input")
    check_guards(y, "b3 2 GiB output")
    del xd
    want = F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), padding=1), 0.1)
    got = y.cpu().permute(0, 3, 1, 2).double()
    assert (got - want).abs().max().item() < 1e-5 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("case", CAT_CASES)
def test_concatenated_sources_guarded(case, dev):
    co, chans, lanes, H, W, B = case
    lib = _lib.load()
    g = torch.Generator().manual_seed(co + sum(chans) + H + 1)
    cin = sum(chans)
    w = (torch.randn(co, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).contiguous()
    b = (torch.randn(co, generator=g) * 0.1).contiguous()
    srcs = [torch.randn(B, c, H, W, generator=g) for c in chans]
    lanes = lanes or tuple(_r(c, 4) for c in chans)
    h = ctypes.c_void_p()
    _lib.check(lib.pivlfn_conv_create_cat(w.data_ptr(), b.data_ptr(), co, len(chans), (ctypes.c_int * len(chans))(*chans), 3, 3,
                                          ctypes.byref(h)), "conv_create_cat")
    try:
        def call(kind):
            ds = []
            for s_, c, l in zip(srcs, chans, lanes):
                t = torch.zeros(B, H, W, l, device=dev) if kind is None else guarded((B, H, W, l), torch.float32, dev, kind)
                t[..., :c] = s_.permute(0, 2, 3, 1).to(dev)
                t[..., c:_r(c, 4)] = 0.0                 # the header: padding lanes zero
                if kind is not None:
                    poison(t, slice(_r(c, 4), l), kind)
                ds.append(t)
            y = torch.full((B, H, W, co), NAN, device=dev) if kind is None else guarded((B, H, W, co), torch.float32, dev, "sentinel")
            _lib.check(lib.pivlfn_conv2d_nhwc_cat(h, len(chans), (ctypes.c_void_p * len(chans))(*[t.data_ptr() for t in ds]),
                                                  (ctypes.c_int * len(chans))(*lanes), y.data_ptr(), co, B, H, W, 1, _st(dev)), "cat")
            torch.cuda.synchronize()
            if kind is not None:
                for t in ds + [y]:
                    check_guards(t, f"cat {case} {kind}")
            return y.cpu()

        plain = call(None)
        want = F.leaky_relu(F.conv2d(torch.cat(srcs, 1).double(), w.double(), b.double(), padding=1), 0.1)
        assert (plain.permute(0, 3, 1, 2).double() - want).abs().max().item() < 1e-5 * max(1.0, want.abs().max().item())
        for kind in KINDS:
            assert same_bits(call(kind), plain), (case, kind)
    finally:
        lib.pivlfn_conv_destroy(h)


@pytest.mark.parametrize("k,B,H,W", [(3, 2, 37, 53), (5, 1, 3, 70), (7, 2, 37, 53), (7, 1, 256, 300),
                                     # the other kernels of the launcher (tests/test_conv_head_plan.py): one weight per lane through the
                                     # scalar cache, four rows per lane, and the matrix-core head on images thinner than its tile and halo
                                     (3, 1, 3, 8200), (5, 1, 17, 4107), (7, 1, 7, 8195), (3, 1, 509, 517), (5, 1, 5, 52431),
                                     (7, 1, 1, 65536), (7, 1, 65537, 1), (7, 1, 5, 13109)])
def test_flow_head_guarded(k, B, H, W, dev):
    """res4 lanes 2-3 are not read (pivlfn.h); out4 lanes 2-3 are written as +0.0."""
    new = {(3, 3, 8200): 2, (5, 17, 4107): 2, (7, 7, 8195): 2, (3, 509, 517): 3, (5, 5, 52431): 3, (7, 1, 65536): 4, (7, 65537, 1): 4, (7, 5, 13109): 4}
    if (k, H, W) in new:                            # PIVLFN_HEAD_PLAN_PIXEL, _ROWS4, _MFMA
        assert head_plan(k, B, H, W)[0] == new[(k, H, W)]
    g = torch.Generator().manual_seed(k + H)
    w = torch.randn(2, 32, k, k, generator=g) / (32 * k * k) ** 0.5
    b = torch.randn(2, generator=g) * 0.1
    conv = Conv(w, b)
    x = torch.randn(B, H, W, 32, generator=g)
    res = torch.randn(B, H, W, 2, generator=g)

    def call(kind):
        if kind is None:
            xd, r4, out = x.to(dev), torch.zeros(B, H, W, 4, device=dev), torch.full((B, H, W, 4), NAN, device=dev)
        else:
            xd = guarded((B, H, W, 32), torch.float32, dev, kind)
            xd.copy_(x.to(dev))
            r4 = poison(guarded((B, H, W, 4), torch.float32, dev, kind), slice(2, 4), kind)
            out = guarded((B, H, W, 4), torch.float32, dev, "sentinel")
        r4[..., :2] = res.to(dev)
        _lib.check(_lib.load().pivlfn_conv_head_nhwc(conv.h, xd.data_ptr(), r4.data_ptr(), out.data_ptr(), B, H, W, _st(dev)), "head")
        torch.cuda.synchronize()
        if kind is not None:
            for t in (xd, r4, out):
                check_guards(t, f"head k={k} {kind}")
            check_lanes(out, slice(2, 4), "zero", f"head k={k} {kind}")
        return out.cpu()

    plain = call(None)
    want = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=k // 2) + res.permute(0, 3, 1, 2).double()
    assert (plain[..., :2].permute(0, 3, 1, 2).double() - want).abs().max().item() < 2e-5 * max(1.0, want.abs().max().item())
    for kind in KINDS:
        assert same_bits(call(kind), plain), (k, kind)


def test_flow_head_guarded_rows4_k7(dev):
    """For k = 7 the four-row kernel runs only from 2^31 bytes of input (below, the matrix-core head does): the guards, lanes and bits of
    test_flow_head_guarded on a 4096 x 4096 image that never leaves the device.  Its values against float64, on bands:
    tests/test_gpu_conv_head.py."""
    k, B, H, W = 7, 1, 4096, 4096
    assert head_plan(k, B, H, W)[0] == 3            # PIVLFN_HEAD_PLAN_ROWS4
    if torch.cuda.mem_get_info(dev)[0] < (8 << 30):
        pytest.skip("two copies of a 2 GiB input need about 8 GiB of free device memory")
    g = torch.Generator().manual_seed(k + H)
    w = torch.randn(2, 32, k, k, generator=g) / (32 * k * k) ** 0.5
    b = torch.randn(2, generator=g) * 0.1
    conv = Conv(w, b)
    gd = torch.Generator(device=dev).manual_seed(k + H)
    x = torch.empty(B, H, W, 32, device=dev).normal_(generator=gd)
    res = torch.empty(B, H, W, 2, device=dev).normal_(generator=gd)

    def call(kind):
        if kind is None:
            xd, r4, out = x, torch.zeros(B, H, W, 4, device=dev), torch.full((B, H, W, 4), NAN, device=dev)
        else:
            xd = guarded((B, H, W, 32), torch.float32, dev, kind)
            xd.copy_(x)
            r4 = poison(guarded((B, H, W, 4), torch.float32, dev, kind), slice(2, 4), kind)
            out = guarded((B, H, W, 4), torch.float32, dev, "sentinel")
        r4[..., :2] = res
        _lib.check(_lib.load().pivlfn_conv_head_nhwc(conv.h, xd.data_ptr(), r4.data_ptr(), out.data_ptr(), B, H, W, _st(dev)), "head")
        torch.cuda.synchronize()
        if kind is not None:
            for t in (xd, r4, out):
                check_guards(t, f"head k={k} {kind}")
            check_lanes(out, slice(2, 4), "zero", f"head k={k} {kind}")
        return out

    plain = call(None)
    assert bool(torch.isfinite(plain).all())
    for kind in KINDS:
        assert same_bits(call(kind), plain), (k, kind)


# ---- correlation, warps, resize, stereo: guards only ---------------------------------------------------------------------------
def _g(t, dev, kind):
    """A copy of CPU tensor t on the device: plain (kind None) or inside a guarded buffer with `kind` guards."""
    if kind is None:
        return t.contiguous().to(dev)
    d = guarded(t.shape, t.dtype, dev, kind)
    d.copy_(t.to(dev))
    return d


def _out(shape, dev, kind):
    return torch.full(shape, NAN, device=dev) if kind is None else guarded(shape, torch.float32, dev, "sentinel")


def _guards_only(fn, what):
    """fn(kind) -> (output tensors, every tensor of the call); the guarded calls equal the plain one bit for bit."""
    plain, _ = fn(None)
    for kind in KINDS:
        got, alltensors = fn(kind)
        torch.cuda.synchronize()
        for t in alltensors:
            check_guards(t, f"{what} {kind}")
        for a, p in zip(got, plain):
            assert same_bits(a.cpu(), p.cpu()), f"{what}: the guarded call ({kind}) differs from the plain call"
    return [p.cpu() for p in plain]


@pytest.mark.parametrize("B,C,H,W,s,warp", [(2, 64, 37, 29, 1, True), (1, 96, 20, 33, 2, True), (1, 32, 17, 9, 1, False)])
def test_warp_corr_guarded(B, C, H, W, s, warp, dev):
    g = np.random.default_rng(B + C + H)
    f1 = g.standard_normal((B, C, H, W)).astype(np.float32)
    f2 = g.standard_normal((B, C, H, W)).astype(np.float32)
    fl = (1.7 * g.standard_normal((B, 2, H, W))).astype(np.float32) if warp else None
    scale, Ho, Wo = 0.625, -(-H // s), -(-W // s)
    lib = _lib.load()
    f4 = None
    if warp:
        f4 = torch.zeros(B, H, W, 4)
        f4[..., :2] = torch.from_numpy(fl).permute(0, 2, 3, 1)

    def nhwc(kind):
        a = _g(torch.from_numpy(f1).permute(0, 2, 3, 1), dev, kind)
        b = _g(torch.from_numpy(f2).permute(0, 2, 3, 1), dev, kind)
        fd = _g(f4, dev, kind) if warp else None
        out = _out((B, Ho, Wo, 56), dev, kind)
        _lib.check(lib.pivlfn_warp_corr_nhwc(a.data_ptr(), b.data_ptr(), fd.data_ptr() if warp else None, scale, out.data_ptr(),
                                             B, C, H, W, s, 1, _st(dev)), "warp_corr_nhwc")
        return [out], [a, b, out] + ([fd] if warp else [])

    def nchw(kind):
        a, b = _g(torch.from_numpy(f1), dev, kind), _g(torch.from_numpy(f2), dev, kind)
        fd = _g(torch.from_numpy(fl), dev, kind) if warp else None
        out = _out((B, 49, Ho, Wo), dev, kind)
        _lib.check(lib.pivlfn_warp_corr_fwd(a.data_ptr(), b.data_ptr(), fd.data_ptr() if warp else None, scale, out.data_ptr(),
                                            B, C, H, W, s, 1, _st(dev)), "warp_corr_fwd")
        return [out], [a, b, out] + ([fd] if warp else [])

    f2w = orc.backwarp_c(f2, fl * np.float32(scale)) if warp else f2
    want = orc.correlation_c(f1, f2w, s)
    want = np.where(want >= 0, want, 0.1 * want).astype(np.float32)
    o4 = _guards_only(nhwc, "warp_corr_nhwc")[0]
    assert torch.all(o4[..., 49:] == 0)
    assert _rel(o4[..., :49].permute(0, 3, 1, 2).numpy(), want) < 2e-5
    assert _rel(_guards_only(nchw, "warp_corr_fwd")[0].numpy(), want) < 2e-5


@pytest.mark.parametrize("B,C,H,W,s", [(2, 33, 17, 23, 2), (1, 64, 32, 48, 1), (1, 7, 1, 1, 1)])
def test_corr_fwd_bwd_backwarp_guarded(B, C, H, W, s, dev):
    g = np.random.default_rng(B * 100 + C + H)
    f1 = g.standard_normal((B, C, H, W)).astype(np.float32)
    f2 = g.standard_normal((B, C, H, W)).astype(np.float32)
    Ho, Wo = -(-H // s), -(-W // s)
    go = g.standard_normal((B, 49, Ho, Wo)).astype(np.float32)
    fl = (1.7 * g.standard_normal((B, 2, H, W))).astype(np.float32)
    lib = _lib.load()
    t1, t2, tgo, tfl = (torch.from_numpy(a) for a in (f1, f2, go, fl))

    def fwd(kind):
        a, b, out = _g(t1, dev, kind), _g(t2, dev, kind), _out((B, 49, Ho, Wo), dev, kind)
        _lib.check(lib.pivlfn_corr_fwd(a.data_ptr(), b.data_ptr(), out.data_ptr(), B, C, H, W, s, _st(dev)), "corr_fwd")
        return [out], [a, b, out]

    assert _rel(_guards_only(fwd, "corr_fwd")[0].numpy(), orc.correlation_c(f1, f2, s)) < 1e-5

    w1, w2 = orc.correlation_backward_c(f1, f2, go, s)
    full = None
    for need in ((True, True), (True, False), (False, True)):
        def bwd(kind):
            a, b, gd = _g(t1, dev, kind), _g(t2, dev, kind), _g(tgo, dev, kind)
            g1 = _out((B, C, H, W), dev, kind) if need[0] else None
            g2 = _out((B, C, H, W), dev, kind) if need[1] else None
            _lib.check(lib.pivlfn_corr_bwd(a.data_ptr(), b.data_ptr(), gd.data_ptr(), g1.data_ptr() if need[0] else None,
                                           g2.data_ptr() if need[1] else None, B, C, H, W, s, _st(dev)), "corr_bwd")
            outs = [t for t in (g1, g2) if t is not None]
            return outs, [a, b, gd] + outs

        got = _guards_only(bwd, f"corr_bwd {need}")
        for t in got:
            assert torch.isfinite(t).all(), "corr_bwd must overwrite every element of its outputs"
        if full is None:
            full = got
            assert _rel(got[0].numpy(), w1) < 1e-5 and _rel(got[1].numpy(), w2) < 1e-5
        else:
            assert same_bits(got[0], full[0] if need[0] else full[1])

    def warp(kind):
        a, fd, out = _g(t1, dev, kind), _g(tfl, dev, kind), _out((B, C, H, W), dev, kind)
        _lib.check(lib.pivlfn_backwarp(a.data_ptr(), fd.data_ptr(), out.data_ptr(), B, C, H, W, _st(dev)), "backwarp")
        return [out], [a, fd, out]

    assert _rel(_guards_only(warp, "backwarp")[0].numpy(), orc.backwarp_c(f1, fl)) < 2e-6


@pytest.mark.parametrize("size", [(64, 64), (37, 53), (20, 100), (75, 107)])
def test_resize_bilinear_guarded(size, dev):
    x = torch.randn(2, 4, 37, 53, generator=torch.Generator().manual_seed(size[0]))
    mul = (ctypes.c_float * 2)(0.5, 3.0)

    def call(kind):
        xd, out = _g(x, dev, kind), _out((2, 4) + size, dev, kind)
        _lib.check(_lib.load().pivlfn_resize_bilinear(xd.data_ptr(), out.data_ptr(), 2, 4, 37, 53, size[0], size[1], mul, _st(dev)),
                   "resize")
        return [out], [xd, out]

    got = _guards_only(call, f"resize {size}")[0]
    want = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
    want[:, 0::2] *= 0.5
    want[:, 1::2] *= 3.0
    assert _rel(got.numpy(), want.numpy()) < 1e-5


@pytest.mark.parametrize("B,h,w,H,W", [(2, 37, 23, 37, 23), (3, 19, 25, 50, 31)])
def test_stereo_2d3c_guarded(B, h, w, H, W, dev):
    rng = np.random.default_rng(B + h + H)
    left = rng.normal(0, 8, (B, h, w, 2)).astype(np.float32)
    right = rng.normal(0, 8, (B, h, w, 2)).astype(np.float32)
    base = np.array([1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
    coeff = {s: [float(v) for v in base + rng.normal(0, 1e-3, 24)] for s in ("Left", "Right")}
    coeff["calib"] = 0.002
    tans = stereo.tangents(*stereo.angles([30.0, 40.0], [5.0, -3.0]))
    fl = stereo.interleave(torch.from_numpy(left).permute(0, 3, 1, 2), torch.from_numpy(right).permute(0, 3, 1, 2)).contiguous()
    c_c = (ctypes.c_float * 48)(*stereo.coeff_f32(coeff).tolist())
    t_c = (ctypes.c_double * 4)(*np.asarray(tans, np.float64).tolist())
    s = stereo.scale_factor(coeff, 0.05)
    s_c = (ctypes.c_float * 2)(s, 15.0)
    m_c = (ctypes.c_float * 2)(W / w, H / h)

    def call(kind):
        fd, out = _g(fl, dev, kind), _out((B, H, W, 3), dev, kind)
        _lib.check(_lib.load().pivlfn_stereo_2d3c(fd.data_ptr(), out.data_ptr(), B, h, w, H, W, m_c, c_c, s_c, t_c, _st(dev)), "stereo")
        return [out], [fd, out]

    got = _guards_only(call, f"stereo {B}x{h}x{w}->{H}x{W}")[0]
    if (h, w) == (H, W):
        want = restate(left, right, stereo.coeff_f32(coeff), tans, (s, 15.0))
        assert same_bits(got, torch.from_numpy(np.ascontiguousarray(want, np.float32)))
    else:
        assert torch.isfinite(got).all()


# ---- the level-pipeline ops (include/pivlfn.h, per-layer checks) --------------------------------------------------------------
@pytest.mark.parametrize("quads,B,H,W,sin,sout", [(1, 2, 9, 11, 8, 12), (14, 2, 5, 6, 60, 64), (1, 1, 257, 129, 4, 4),
                                                   (14, 3, 7, 9, 56, 56)])
def test_upconv_guarded(quads, B, H, W, sin, sout, dev):
    """The input's padding lanes C..4*quads must be finite (the finite poison); lanes past them and the guards are poisoned."""
    g = torch.Generator().manual_seed(quads * 100 + H)
    C, cs = (2 if quads == 1 else 49), 4 * quads
    x = torch.randn(B, C, H, W, generator=g)
    w = (0.5 * torch.randn(C, 1, 4, 4, generator=g)).contiguous()

    def call(kind):
        if kind is None:
            xd = torch.cat([_nhwc(x, cs), torch.full((B, H, W, sin - cs), NAN)], 3).contiguous().to(dev)
            out = torch.full((B, 2 * H, 2 * W, sout), NAN, device=dev)
        else:
            xd = guarded((B, H, W, sin), torch.float32, dev, kind)
            xd[..., C:cs] = 0.0
            if kind == "big":
                poison(xd, slice(C, cs), "big")
            poison(xd, slice(cs, sin), kind)
            out = guarded((B, 2 * H, 2 * W, sout), torch.float32, dev, "sentinel")
        xd[..., :C] = x.permute(0, 2, 3, 1).to(dev)
        _lib.check(_lib.load().pivlfn_upconv_nhwc(xd.data_ptr(), w.data_ptr(), out.data_ptr(), B, H, W, quads, sin, sout, _st(dev)),
                   "upconv")
        torch.cuda.synchronize()
        if kind is not None:
            for t in (xd, out):
                check_guards(t, f"upconv q{quads} {kind}")
            check_lanes(out, slice(C, cs), "zero", "upconv")
            check_lanes(out, slice(cs, sout), "sentinel", "upconv")
        return out[..., :cs].cpu()

    plain = call(None)
    _within(plain[..., :C].permute(0, 3, 1, 2), ref.upconv(x.double(), w.double()), ref.upconv_bound(x.double(), w.double()), OP_BAR,
            f"upconv q{quads} {B}x{H}x{W}")
    for kind in KINDS:
        assert same_bits(call(kind), plain), kind


@pytest.mark.parametrize("C,scale,B,H,W", [(64, 10.0, 2, 19, 23), (4, 2.5, 1, 31, 2), (128, 1.25, 1, 130, 70)])
def test_backwarp_nhwc_guarded(C, scale, B, H, W, dev):
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, H, W, C, generator=g)
    f4 = torch.zeros(B, H, W, 4)
    f4[..., :2] = 2.0 * torch.randn(B, H, W, 2, generator=g)

    def call(kind):
        xd, fd, out = _g(x, dev, kind), _g(f4, dev, kind), _out((B, H, W, C), dev, kind)
        _lib.check(_lib.load().pivlfn_backwarp_nhwc(xd.data_ptr(), fd.data_ptr(), scale, out.data_ptr(), B, H, W, C, _st(dev)), "bw")
        return [out], [xd, fd, out]

    got = _guards_only(call, f"backwarp_nhwc C={C}")[0]
    fl = f4[..., :2].permute(0, 3, 1, 2)
    want, absterms = ref.backwarp(x.permute(0, 3, 1, 2).double(), fl.double() * scale)
    _within(got.permute(0, 3, 1, 2), want, ref.backwarp_bound(x.permute(0, 3, 1, 2).double(), fl, scale, absterms), WARP_BAR,
            f"backwarp_nhwc C={C}")


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("B,H,W,scale", [(1, 15, 17, 1.25), (3, 7, 9, 10.0), (1, 113, 145, 2.5)])
def test_reg_prep_guarded(B, H, W, scale, fused, dev):
    """Image lane 3 is not read (poisoned); partial_ws is scratch (poisoned); misc4 lane 3 is +0.0."""
    g = torch.Generator().manual_seed(B + H + W)
    img1, img2 = torch.rand(B, 3, H, W, generator=g) - 0.45, torch.rand(B, 3, H, W, generator=g) - 0.45
    fl = torch.randn(B, 2, H, W, generator=g) * 2.0

    def call(kind):
        i1, i2, f4 = (_g(_nhwc(t, 4), dev, kind) for t in (img1, img2, fl))
        misc, mean = _out((B, H, W, 4), dev, kind), _out((B, 2), dev, kind)
        part = torch.full((B, 128), NAN, device=dev)
        if kind is not None:
            poison(i1, slice(3, 4), kind)
            poison(i2, slice(3, 4), kind)
            part = poison(guarded((B, 128), torch.float32, dev, kind), slice(0, 128), kind)
        _lib.check(_lib.load().pivlfn_reg_prep(i1.data_ptr(), i2.data_ptr(), f4.data_ptr(), scale, misc.data_ptr(), mean.data_ptr(),
                                               part.data_ptr(), B, H, W, fused, _st(dev)), "reg_prep")
        torch.cuda.synchronize()
        if kind is not None:
            check_lanes(misc, slice(3, 4), "zero", f"reg_prep {kind}")
        return [misc, mean], [i1, i2, f4, misc, mean] + ([part] if kind is not None else [])

    misc, mean = _guards_only(call, f"reg_prep {B}x{H}x{W} fused={fused}")
    fd = fl.double()
    m64, rm64, norm64, nb = ref.reg_prep(img1.double(), img2.double(), fd, scale)
    _within(mean, m64, ref.mean_bound(fd, H * W), OP_BAR, "reg_prep mean")
    _within(misc[..., 0], norm64, nb, WARP_BAR, "reg_prep norm")


@pytest.mark.parametrize("k", [3, 5, 7])
def test_reg_tail_guarded(k, dev):
    """dist lanes >= k*k are not read (poisoned); out4 lanes 2-3 are +0.0; both outputs, and each alone."""
    KK, ds = k * k, _r(k * k, 4) + 4
    g = torch.Generator().manual_seed(k)
    wx, wy = 0.3 * torch.randn(KK, generator=g), 0.3 * torch.randn(KK, generator=g)
    B, H, W = 2, 17, 33
    dist = torch.randn(B, KK, H, W, generator=g)
    fl = 2.0 * torch.randn(B, 2, H, W, generator=g)
    for o4_on, nchw_on in ((True, True), (True, False), (False, True)):
        def call(kind):
            d4 = _g(_nhwc(dist, ds), dev, kind)
            if kind is not None:
                poison(d4, slice(KK, ds), kind)
            f4, wxd, wyd = _g(_nhwc(fl, 4), dev, kind), _g(wx, dev, kind), _g(wy, dev, kind)
            o4 = _out((B, H, W, 4), dev, kind) if o4_on else None
            on = _out((B, 2, H, W), dev, kind) if nchw_on else None
            _lib.check(_lib.load().pivlfn_reg_tail(d4.data_ptr(), ds, f4.data_ptr(), wxd.data_ptr(), wyd.data_ptr(), 0.25, -0.125, k,
                                                   o4.data_ptr() if o4_on else None, on.data_ptr() if nchw_on else None, 20.0,
                                                   B, H, W, _st(dev)), "reg_tail")
            torch.cuda.synchronize()
            if kind is not None and o4_on:
                check_lanes(o4, slice(2, 4), "zero", f"reg_tail {kind}")
            outs = [t for t in (o4, on) if t is not None]
            return outs, [d4, f4, wxd, wyd] + outs

        got = _guards_only(call, f"reg_tail k={k} out4={o4_on} nchw={nchw_on}")
        want, bound = ref.reg_tail(dist.double(), fl.double(), wx.double(), wy.double(), 0.25, -0.125, k)
        if o4_on:
            _within(got[0][..., :2].permute(0, 3, 1, 2), want, bound, OP_BAR, f"reg_tail k={k}")


@pytest.mark.parametrize("B,H,W", [(1, 32, 32), (2, 64, 96)])
def test_prep_pyramid_guarded(B, H, W, dev):
    g = torch.Generator().manual_seed(H + W + B)
    img1, img2 = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
    m32 = (ctypes.c_float * 6)(0.411618, 0.434631, 0.454253, 0.310782, 0.533645, 0.152793)
    sizes = [2 * B * (H >> L) * (W >> L) * 4 for L in range(6)]

    def call(kind):
        d1, d2, out = _g(img1, dev, kind), _g(img2, dev, kind), _out((sum(sizes),), dev, kind)
        _lib.check(_lib.load().pivlfn_prep_pyramid(d1.data_ptr(), d2.data_ptr(), m32, out.data_ptr(), B, H, W, 6, _st(dev)), "pyramid")
        return [out], [d1, d2, out]

    out = _guards_only(call, f"prep_pyramid {B}x{H}x{W}")[0]
    mean6 = [float(np.float32(m)) for m in m32]
    want, bounds = ref.pyramid(img1.double(), img2.double(), mean6, 6)
    off = 0
    for L in range(1, 7):
        lv = out[off:off + sizes[L - 1]].view(2 * B, H >> (L - 1), W >> (L - 1), 4)
        off += sizes[L - 1]
        assert same_bits(lv[..., 3], torch.zeros_like(lv[..., 3]))
        _within(lv[..., :3].permute(0, 3, 1, 2), want[L - 1], bounds[L - 1], OP_BAR, f"pyramid level {L}")


@pytest.mark.parametrize("N,H,W,B_feat,fused", [(2, 33, 45, 1, False), (3, 264, 520, 2, True)])
def test_conv1_fused_guarded(N, H, W, B_feat, fused, dev):
    """x lane 3 must be finite (the finite poison); out_feat rows past B_feat keep their sentinel."""
    g = torch.Generator().manual_seed(N * 1000 + H + W)
    w1, b1 = (2.0 / 147) ** 0.5 * torch.randn(32, 3, 7, 7, generator=g), 0.1 * torch.randn(32, generator=g)
    we, be = (2.0 / 32) ** 0.5 * torch.randn(64, 32, 1, 1, generator=g), 0.1 * torch.randn(64, generator=g)
    wf, bfe = (2.0 / 32) ** 0.5 * torch.randn(128, 32, 1, 1, generator=g), 0.1 * torch.randn(128, generator=g)
    x = torch.rand(N, 3, H, W, generator=g) - 0.5

    def call(kind):
        xd = _g(_nhwc(x, 4), dev, kind)
        if kind == "big":
            poison(xd, slice(3, 4), "big")
        out, ext, feat = (_out((N, H, W, c), dev, kind) for c in (32, 64, 128))
        ran = ctypes.c_int(-1)
        _lib.check(_lib.load().pivlfn_conv1_fused_nhwc(w1.data_ptr(), b1.data_ptr(), we.data_ptr(), be.data_ptr(), wf.data_ptr(),
                                                       bfe.data_ptr(), xd.data_ptr(), out.data_ptr(), ext.data_ptr(), feat.data_ptr(),
                                                       N, H, W, B_feat, ctypes.byref(ran), _st(dev)), "conv1_fused")
        assert ran.value == int(fused)
        torch.cuda.synchronize()
        if kind is not None:
            check_lanes(feat[B_feat:], slice(0, 128), "sentinel", f"conv1 feat {kind}")
        return [out, ext, feat[:B_feat]], [xd, out, ext, feat]

    a, e, f = _guards_only(call, f"conv1_fused {N}x{H}x{W}")
    (wa, we_, wf_), (ba, be_, bf) = ref.conv1_fused(x.double(), w1.double(), b1.double(), we.double(), be.double(), wf.double(),
                                                   bfe.double())
    _within(a.permute(0, 3, 1, 2), wa, ba, OP_BAR, "conv1")
    _within(e.permute(0, 3, 1, 2), we_, be_, OP_BAR, "NetC_ext")
    _within(f.permute(0, 3, 1, 2), wf_[:B_feat], bf[:B_feat], OP_BAR, "moduleFeat")


# ---- the whole forward on a dirty workspace --------------------------------------------------------------------------------------
def _net(model, dev, precision="fp32"):
    """model: "piv", "hui", or "piv2-L<lowest level>" (LiteFlowNet2 backbone)."""
    if model.startswith("piv2"):
        L = int(model[-1])
        cfg = MODEL_CFG["piv2"]
        net = LiteFlowNet2(cfg["starting_scale"], L, cfg["rgb_mean"])
        net.load_state_dict(synth.generate_weights("piv2", 0, lowest_level=L))
    else:
        net = pivlfn.Network(model=model, params=synth.generate_weights(model, 0))
    net = net.to(dev).eval()
    net.precision = precision
    return net


def _images(B, H, W, seed):
    a, b = synth.particle_batch(B, H, W, seed=seed)
    return torch.from_numpy(a), torch.from_numpy(b)


class _Forward:
    def __init__(self, net, B, H, W, dev, seed=3):
        self.net, self.B, self.H, self.W, self.dev = net, B, H, W, dev
        self.h = net._native()
        lib = _lib.load()
        self.ws_bytes = lib.pivlfn_workspace_bytes(self.h, B, H, W)
        self.n_levels = lib.pivlfn_levels_floats(self.h, B, H, W)
        div = 2 ** (net.lowest_level - 1)
        self.flow_shape = (B, 2, H // div, W // div)
        a, b = _images(B, H, W, seed)
        self.i1, self.i2 = _g(a, dev, "nan"), _g(b, dev, "nan")

    def __call__(self, ws, levels):
        """One forward into guarded flow / levels on the workspace payload ws; returns CPU copies."""
        flow = guarded(self.flow_shape, torch.float32, self.dev, "sentinel")
        lv = guarded((self.n_levels,), torch.float32, self.dev, "sentinel") if levels else None
        _lib.check(_lib.load().pivlfn_forward(self.h, self.i1.data_ptr(), self.i2.data_ptr(), flow.data_ptr(),
                                              lv.data_ptr() if levels else None, self.B, self.H, self.W, ws.data_ptr(),
                                              self.ws_bytes, _st(self.dev)), "forward")
        torch.cuda.synchronize()
        for t in (self.i1, self.i2, flow) + ((lv,) if levels else ()):
            check_guards(t, f"forward {self.B}x{self.H}x{self.W}")
        return flow.cpu(), (lv.cpu() if levels else None)


def _dirty(ws, fill, dev):
    """Fill the whole workspace payload on the forward's stream, then wait for it."""
    with torch.cuda.stream(torch.cuda.current_stream(dev)):
        if fill == "zero":
            ws.zero_()
        else:
            poison(ws, slice(0, ws.shape[-1]), fill)
    torch.cuda.synchronize()


def _workspace(fw):
    assert fw.ws_bytes % 4 == 0
    return guarded((fw.ws_bytes // 4,), torch.float32, fw.dev, "nan")


FWD = ([("piv", p, 2, 256, 320) for p in ("fp32", "fp32_direct", "fp32_wino_mfma32", "fp16", "fp32_split", "fp32_split3")]
       + [("piv", "fp32", 1, 32, 32), ("piv", "fp32", 1, 96, 160), ("hui", "fp32", 1, 32, 32), ("hui", "fp32", 1, 96, 160),
          ("hui", "fp32", 2, 256, 320)]
       + [(f"piv2-L{L}", "fp32", B, H, W) for L in (1, 2, 3) for (B, H, W) in ((1, 32, 32), (1, 96, 160), (2, 256, 320))]
       + [("piv", "fp32", 1, 1024, 1024)])


@pytest.mark.parametrize("model,precision,B,H,W", FWD)
def test_forward_on_a_dirty_workspace(model, precision, B, H, W, dev):
    fw = _Forward(_net(model, dev, precision), B, H, W, dev)
    ws = _workspace(fw)
    for levels in (True, False):
        runs = []
        for fill in ("zero",) + KINDS:
            _dirty(ws, fill, dev)
            runs.append(fw(ws, levels))
            check_guards(ws, f"{model} {precision} workspace, {fill}")
        flow0, lv0 = runs[0]
        assert torch.isfinite(flow0).all() and (lv0 is None or torch.isfinite(lv0).all())
        for (flow, lv), fill in zip(runs[1:], KINDS):
            assert same_bits(flow, flow0), f"{model} {precision} {B}x{H}x{W}: the flow depends on the workspace's {fill} fill"
            if levels:
                assert same_bits(lv, lv0), f"{model} {precision} {B}x{H}x{W}: a level flow depends on the workspace's {fill} fill"
        if levels:
            final = flow0
        else:
            assert same_bits(flow0, final), "the flow depends on whether levels is NULL"


def test_forward_reuses_a_dirty_workspace(dev):
    """A 512 x 448 B = 2 forward, then a 96 x 160 B = 1 forward in the same (larger, still dirty) buffer without refilling it: both equal
    their results on a zeroed workspace of their own size."""
    net = _net("piv", dev)
    big, small = _Forward(net, 2, 512, 448, dev, seed=5), _Forward(net, 1, 96, 160, dev, seed=6)
    want = []
    for fw in (big, small):
        ws = _workspace(fw)
        _dirty(ws, "zero", dev)
        want.append(fw(ws, True))
        check_guards(ws, "zeroed workspace")
        del ws
    ws = _workspace(big)
    for kind in KINDS:
        _dirty(ws, kind, dev)
        for fw, (flow0, lv0) in zip((big, small), want):
            flow, lv = fw(ws, True)
            assert same_bits(flow, flow0) and same_bits(lv, lv0), f"{fw.B}x{fw.H}x{fw.W} after a {kind}-filled, reused workspace"
        check_guards(ws, f"reused workspace, {kind}")
