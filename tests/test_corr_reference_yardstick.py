"""CPU: the float64 yardsticks of tests/corr_reference.py are right and sharp.  corr_bwd_f64 is float64 autograd through the float64
forward; the pinned C oracle (forward, both gradients, strides 1..4) lies within 1e-6 of max|out| of them; and a one-defect variant
(one of the 49 terms of a gradient left out at one pixel, one resize source index off by one) is more than 100 x the bound that
tests/test_gpu_corr_domain.py asserts (twice the oracle's own distance plus 2e-6 of max|out|) away from float64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pivlfn
import pivlfn_oracle as orc
from corr_reference import backwarp_f64, corr_bwd_f64, fused_f64, resize_f64


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))


def _data(shape, s, seed):
    B, C, H, W = shape
    g = np.random.default_rng(seed)
    f1 = g.standard_normal(shape).astype(np.float32)
    f2 = g.standard_normal(shape).astype(np.float32)
    go = g.standard_normal((B, 49, -(-H // s), -(-W // s))).astype(np.float32)
    return f1, f2, go


# H = 13 and 25: H % s == 1 for s = 2, 3, 4 (the last grid row is the image's last row); H = 5 < 8; one 1 x 1 image
SHAPES = [(2, 5, 13, 10), (1, 3, 5, 7), (1, 64, 25, 19), (1, 7, 1, 1)]


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_corr_bwd_f64_is_float64_autograd(s):
    for n, shape in enumerate(SHAPES):
        f1, f2, go = _data(shape, s, 10 * s + n)
        a = torch.from_numpy(f1).double().requires_grad_(True)
        b = torch.from_numpy(f2).double().requires_grad_(True)
        out = orc.correlation_torch(a, b, s)
        assert rel(out.detach().numpy(), fused_f64(f1, f2, None, 1.0, s, leaky=False)) < 1e-12          # the float64 forward is fused_f64's
        out.backward(torch.from_numpy(go).double())
        g1, g2 = corr_bwd_f64(f1, f2, go, s)
        assert rel(g1.numpy(), a.grad.numpy()) < 1e-12 and rel(g2.numpy(), b.grad.numpy()) < 1e-12, shape
        if s > 1:
            off = np.ones(shape[2:], bool)
            off[::s, ::s] = False
            assert not g1.numpy()[:, :, off].any() and not g2.numpy()[:, :, off].any()


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_c_oracle_within_1e6_of_float64(s):
    """Measured: at most 3.5e-7 for the plain forward and both gradients."""
    for n, shape in enumerate(SHAPES):
        f1, f2, go = _data(shape, s, 100 * s + n)
        e_fwd = rel(orc.correlation_c(f1, f2, s), fused_f64(f1, f2, None, 1.0, s, leaky=False))
        w1, w2 = orc.correlation_backward_c(f1, f2, go, s)
        g1, g2 = corr_bwd_f64(f1, f2, go, s)
        e1, e2 = rel(w1, g1.numpy()), rel(w2, g2.numpy())
        print(f"{shape} stride {s}: |oracle - f64| forward {e_fwd:.2e}  gradFirst {e1:.2e}  gradSecond {e2:.2e}")
        assert e_fwd < 1e-6 and e1 < 1e-6 and e2 < 1e-6, (shape, e_fwd, e1, e2)


def test_backwarp_f64_is_the_oracles_and_drops_nan():
    """backwarp_f64 equals the oracle's grid_sample backwarp in float64 with flows that leave the image on every side; a NaN flow
    component and a flow of 1e30 give a zero pixel."""
    g = torch.Generator().manual_seed(3)
    for (B, C, H, W) in [(2, 5, 9, 13), (1, 3, 2, 2), (1, 4, 31, 7)]:
        x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
        fl = 3.0 * torch.randn(B, 2, H, W, generator=g, dtype=torch.float64)
        assert float((backwarp_f64(x, fl) - orc.backwarp(x, fl)).abs().max()) < 1e-12
    x = torch.randn(1, 2, 4, 5, generator=g)
    fl = torch.zeros(1, 2, 4, 5)
    fl[0, 0, 1, 1], fl[0, 1, 2, 2], fl[0, 0, 3, 3], fl[0, 1, 0, 4] = float("nan"), float("nan"), 1e30, -1e30
    out = backwarp_f64(x, fl)
    want = x.double().clone()
    want[0, :, 1, 1] = want[0, :, 2, 2] = want[0, :, 3, 3] = want[0, :, 0, 4] = 0
    assert torch.equal(out, want)


def test_one_gradient_term_left_out_fails_the_yardstick():
    f1, f2, go = _data((1, 8, 20, 22), 3, 7)
    s, C = 3, 8
    w1, w2 = orc.correlation_backward_c(f1, f2, go, s)
    g1, g2 = corr_bwd_f64(f1, f2, go, s)
    for want, exact, other, sign in ((w1, g1.numpy(), f2, 1), (w2, g2.numpy(), f1, -1)):
        bound = 2.0 * rel(want, exact) + 2e-6
        Y, X, dy, dx = 3, 4, 1, -2
        t = 7 * (dy + 3) + (dx + 3)
        bad = want.copy()
        if sign > 0:      # gradFirst[sY, sX] without its term t
            bad[0, :, s * Y, s * X] -= go[0, t, Y, X] * other[0, :, s * (Y + dy), s * (X + dx)] / C
        else:             # gradSecond[sY, sX] without its term t
            bad[0, :, s * Y, s * X] -= go[0, t, Y - dy, X - dx] * other[0, :, s * (Y - dy), s * (X - dx)] / C
        assert rel(bad, exact) > 100 * bound, (rel(bad, exact), bound)


def test_one_resize_source_index_off_by_one_fails_the_yardstick():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 2, 32, 32, generator=g)
    size, mul = (100, 76), (0.5, 3.0)
    exact = resize_f64(x, size, mul)
    want = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
    want[:, 0::2] *= mul[0]
    want[:, 1::2] *= mul[1]
    bound = 2.0 * rel(want.numpy(), exact.numpy()) + 2e-6
    oy, ox = 50, 40                                       # source row 32/100 * 50.5 - 0.5 = 15.66 -> rows 15, 16; column 16.55 -> 16, 17
    ly, lx = 0.32 * 50.5 - 0.5 - 15, 32 / 76 * 40.5 - 0.5 - 16
    bad = want.clone()
    for c in range(2):
        p = x[0, c].double()
        bad[0, c, oy, ox] = mul[c] * ((1 - ly) * ((1 - lx) * p[16, 16] + lx * p[16, 17]) + ly * ((1 - lx) * p[17, 16] + lx * p[17, 17]))   # rows 16, 17 for 15, 16
    assert rel(bad.numpy(), exact.numpy()) > 100 * bound
    good = want.clone()
    for c in range(2):
        p = x[0, c].double()
        good[0, c, oy, ox] = mul[c] * ((1 - ly) * ((1 - lx) * p[15, 16] + lx * p[15, 17]) + ly * ((1 - lx) * p[16, 16] + lx * p[16, 17]))
    assert rel(good.numpy(), exact.numpy()) <= bound       # the same formula with the right rows is inside


def test_resize_f64_special_sizes():
    """A same-size resize is the input exactly; a 1 x 1 source is constant; torch's own fp32 resize is exact there too."""
    x = torch.randn(2, 3, 37, 53, generator=torch.Generator().manual_seed(1))
    assert torch.equal(resize_f64(x, (37, 53)), x.double())
    one = torch.randn(1, 4, 1, 1, generator=torch.Generator().manual_seed(2))
    up = resize_f64(one, (64, 64), (0.5, 3.0))
    assert torch.equal(up, (one.double() * torch.tensor([0.5, 3.0, 0.5, 3.0], dtype=torch.float64).view(1, 4, 1, 1)).expand(1, 4, 64, 64))


@pytest.mark.parametrize("stride", [0, -1, 5])
def test_function_correlation_refuses_strides_outside_1_to_4(stride):
    a = torch.zeros(1, 8, 4, 4)
    with pytest.raises(ValueError, match="1..4"):
        pivlfn.FunctionCorrelation(a, a, stride)
    with pytest.raises(ValueError, match="1..4"):
        pivlfn.ModuleCorrelation()(a, a, stride)


def test_backward_channel_group_policy():
    """The channel grouping of pivlfn_corr_bwd for the shapes tests/test_gpu_corr_domain.py is built on, worked out by hand from
    `tiles * cdiv(C, cgroup) * B < 2048` (16 x 16 tiles of the stride grid): no GPU needed, the policy is host code."""
    from pivlfn import _lib
    lib = _lib.load()
    for shape, want in [((2, 72, 256, 256, 1), 16), ((2, 64, 256, 128, 1), 8), ((2, 60, 256, 128, 1), 8), ((1, 16, 50, 50, 3), 4),
                        ((2, 33, 37, 50, 4), 4), ((1, 7, 1, 1, 4), 4), ((8, 72, 255, 250, 2), 16), ((1, 72, 255, 250, 2), 4)]:
        assert lib.pivlfn_corr_bwd_channel_group(*shape) == want, shape
    assert lib.pivlfn_corr_bwd_channel_group(1, 8, 4, 4, 5) == 0 and lib.pivlfn_corr_bwd_channel_group(1, 8, 4, 4, 0) == 0
