"""CPU: the float64 yardsticks of tests/test_gpu_net_ops.py are sharp.  For each of the six ops a one-defect variant of the float64
result (one dropped tap, a shifted halo row, a channel missing from a sum, swapped components, a wrong mean) exceeds the per-element
bound those tests assert by at least 100x at its worst element, and exceeds the op's bar (1e-5 * max|out|, 2e-5 for warps) by 100x
as well -- a kernel with that defect could not pass.  And the pixel-unit warp of the yardstick is the oracle's grid_sample backwarp."""
import numpy as np
import torch
import torch.nn.functional as F

import net_ops_reference as ref
import pivlfn_oracle as orc

F64 = torch.float64


def _sharp(bad, want, bound, bar):
    d = (bad - want).abs()
    ratio = float((d / bound.clamp_min(1e-300)).max())
    assert ratio >= 100, f"the defect is only {ratio:.1f} x the per-element bound"
    assert float(d.max()) >= 100 * bar * float(want.abs().max()), f"the defect {float(d.max()):.2e} is not 100 x the bar"


def test_backwarp_restatement_is_the_oracles():
    """The pixel-unit four-tap form equals the oracle's grid_sample(align_corners=True) backwarp (src/models.py:20-35) in float64,
    with flows that leave the image on every side."""
    g = torch.Generator().manual_seed(3)
    for (B, C, H, W) in [(2, 5, 9, 13), (1, 3, 2, 2), (1, 4, 31, 7)]:
        x = torch.randn(B, C, H, W, generator=g, dtype=F64)
        fl = 3.0 * torch.randn(B, 2, H, W, generator=g, dtype=F64)
        fl[:, :, 0, 0] = torch.tensor([-0.25, 0.0], dtype=F64)          # x in (-1, 0)
        fl[:, :, 0, 1] = torch.tensor([W - 1.5, 0.0], dtype=F64)        # x in (W-1, W)
        want = orc.backwarp(x, fl)
        got, _ = ref.backwarp(x, fl)
        assert float((got - want).abs().max()) < 1e-12


def test_upconv_one_dropped_tap():
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(2, 49, 7, 9, generator=g, dtype=F64), 0.5 * torch.randn(49, 1, 4, 4, generator=g, dtype=F64)
    want, bound = ref.upconv(x, w), ref.upconv_bound(x, w)
    bad = want.clone()
    bad[1, 30, 5, 6] -= x[1, 30, 3, 3] * w[30, 0, 0, 1]       # output (5, 6) = 2 * 3 - 1 + ky, 2 * 3 - 1 + kx: tap (0, 1) of input (3, 3)
    _sharp(bad, want, bound, 1e-5)


def test_backwarp_one_dropped_tap():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 64, 12, 14, generator=g, dtype=F64)
    fl32 = (1.5 * torch.randn(1, 2, 12, 14, generator=g)).float()
    fl32[0, :, 6, 7] = torch.tensor([0.25, 0.25])                   # pixel (6, 7) samples at (7.3125, 6.3125): four in-range taps
    scale = 1.25
    want, absterms = ref.backwarp(x, fl32.double() * scale)
    bound = ref.backwarp_bound(x, fl32, scale, absterms)
    fx, fy = 7 + 0.25 * scale, 6 + 0.25 * scale
    ax, ay = fx - np.floor(fx), fy - np.floor(fy)
    bad = want.clone()
    bad[0, :, 6, 7] -= (1 - ax) * (1 - ay) * x[0, :, int(np.floor(fy)), int(np.floor(fx))]
    _sharp(bad, want, bound, 2e-5)


def test_reg_prep_swapped_mean_and_wrong_norm():
    g = torch.Generator().manual_seed(4)
    B, H, W = 2, 15, 17
    i1, i2 = torch.rand(B, 3, H, W, generator=g, dtype=F64), torch.rand(B, 3, H, W, generator=g, dtype=F64)
    fl = torch.randn(B, 2, H, W, generator=g).double() + torch.tensor([0.5, -0.7], dtype=F64).view(1, 2, 1, 1)
    mean, rm, norm, nb = ref.reg_prep(i1, i2, fl, 10.0)
    mb = ref.mean_bound(fl, H * W)
    _sharp(mean.flip(1), mean, mb, 1e-5)                            # u and v swapped in the mean
    _sharp(fl - mean.flip(1).view(B, 2, 1, 1), rm, mb.view(B, 2, 1, 1) + ref.U * rm.abs(), 1e-5)
    bad = norm.clone()                                              # the blue channel left out of one pixel's norm
    d = i1 - ref.backwarp(i2, fl * 10.0)[0]
    bad[1, 7, 8] = d[1, :2, 7, 8].pow(2).sum().sqrt()
    _sharp(bad, norm, nb, 2e-5)


def test_reg_tail_halo_row_shift_and_missing_channel_in_z():
    g = torch.Generator().manual_seed(5)
    k, B, H, W = 7, 1, 20, 21
    KK = k * k
    dist = torch.randn(B, KK, H, W, generator=g, dtype=F64)
    fl = 2.0 * torch.randn(B, 2, H, W, generator=g, dtype=F64)
    wx, wy = 0.3 * torch.randn(KK, generator=g, dtype=F64), 0.3 * torch.randn(KK, generator=g, dtype=F64)
    want, bound = ref.reg_tail(dist, fl, wx, wy, 0.25, -0.125, k)
    # the unfold halo shifted down by one row for the last row of the first 16 x 16 tile (row 15 reads rows 13..19 instead of 12..18)
    fl_shift = fl.clone()
    fl_shift[:, :, :-1] = fl[:, :, 1:]
    fl_shift[:, :, -1] = 0
    shifted, _ = ref.reg_tail(dist, fl_shift, wx, wy, 0.25, -0.125, k)
    bad = want.clone()
    bad[:, :, 15, :16] = shifted[:, :, 15, :16]
    _sharp(bad, want, bound, 1e-5)
    # the last softmax channel left out of Z
    negsq = -dist.pow(2)
    e = (negsq - negsq.max(1, keepdim=True)[0]).exp()
    z_bad = e[:, :KK - 1].sum(1, keepdim=True)
    un = F.unfold(fl[:, 0:1], kernel_size=k, padding=k // 2).view(B, KK, H, W)
    bad_u = ((wx.view(1, KK, 1, 1) * e * un).sum(1, keepdim=True) + 0.25) / z_bad
    _sharp(torch.cat([bad_u, want[:, 1:]], 1), want, bound, 1e-5)


def test_pyramid_wrong_frame_mean_and_corner_alignment():
    g = torch.Generator().manual_seed(6)
    B, H, W = 1, 64, 96
    i1, i2 = torch.rand(B, 3, H, W, generator=g, dtype=F64), torch.rand(B, 3, H, W, generator=g, dtype=F64)
    mean6 = [0.411618, 0.434631, 0.454253, 0.310782, 0.533645, 0.152793]
    want, bounds = ref.pyramid(i1, i2, mean6, 6)
    bad, _ = ref.pyramid(i1, i2, mean6[:3] * 2, 6)                 # frame 2 with frame 1's means
    for L in (1, 6):
        _sharp(bad[L - 1], want[L - 1], bounds[L - 1], 1e-5)
    one = F.interpolate(want[1], size=(H >> 2, W >> 2), mode="bilinear", align_corners=True)    # level 3 from level 2, wrong corners
    _sharp(one, want[2], bounds[2], 1e-5)


def test_conv1_dropped_input_channel_of_module_feat():
    g = torch.Generator().manual_seed(7)
    N, H, W = 2, 16, 40
    w1, b1 = (2.0 / 147) ** 0.5 * torch.randn(32, 3, 7, 7, generator=g, dtype=F64), 0.1 * torch.randn(32, generator=g, dtype=F64)
    we, be = (2.0 / 32) ** 0.5 * torch.randn(64, 32, 1, 1, generator=g, dtype=F64), 0.1 * torch.randn(64, generator=g, dtype=F64)
    wf, bfe = (2.0 / 32) ** 0.5 * torch.randn(128, 32, 1, 1, generator=g, dtype=F64), 0.1 * torch.randn(128, generator=g, dtype=F64)
    x = torch.rand(N, 3, H, W, generator=g, dtype=F64) - 0.5
    (a, e, f), (ba, be_, bf) = ref.conv1_fused(x, w1, b1, we, be, wf, bfe)
    wf_bad = wf.clone()
    wf_bad[:, 17] = 0                                               # moduleFeat without input channel 17
    bad = F.leaky_relu(F.conv2d(a, wf_bad, bfe), 0.1)
    _sharp(bad, f, bf, 1e-5)
    w1_bad = w1.clone()
    w1_bad[:, :, 6, 6] = 0                                          # conv1 without its last tap
    _sharp(F.leaky_relu(F.conv2d(x, w1_bad, b1, padding=3), 0.1), a, ba, 1e-5)
