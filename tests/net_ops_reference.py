"""Float64 restatements of the level-pipeline ops that run only inside pivlfn_forward, written from the reference's formulas
(the reference repository's src/models.py, cited per function; the oracle's lines where it restates them), each with a per-element bound on
what an fp32 evaluation of the same operation may differ from it.  u = 2^-24 is the unit roundoff of fp32; every bound is
n * u * sum|terms| for the n roundings an element goes through, plus, where sample positions are computed, the error of the
position times the slope of the bilinear interpolant.  Used by tests/test_gpu_net_ops.py (the kernels) and tests/test_net_ops_yardstick.py
(the bounds are sharp: one defect exceeds them by 100x).  Device-agnostic: everything runs where its inputs live."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
F64 = torch.float64


def _lrelu(x):
    return F.leaky_relu(x, negative_slope=0.1)


# ---- upConv_M / upCorr_M: src/models.py:144-145, 151-152 (oracle :224, :230) ---------------------------------------------
def upconv(x, w):
    """x NCHW [B,C,H,W], w [C,1,4,4]: depthwise ConvTranspose2d, kernel 4, stride 2, padding 1, no bias."""
    return F.conv_transpose2d(x, w, None, stride=2, padding=1, groups=x.shape[1])


def upconv_bound(x, w):
    """At most 2 x 2 taps per output, each one fma (one rounding): 4 u sum|w x|."""
    return 4 * U * upconv(x.abs(), w.abs())


# ---- backwarp: src/models.py:20-35 (oracle :144) in pixel units -------------------------------------------------------------
def backwarp(inp, flow):
    """inp NCHW [B,C,H,W], flow NCHW [B,2,H,W] in pixels.  grid_sample(align_corners=True, padding_mode='zeros') of the reference
    samples at (x + u, y + v) in pixel units: four bilinear taps, out-of-range taps contribute 0.  Returns (out, sum|w_i v_i|).
    For H, W >= 2 this equals the oracle's grid_sample form in float64 (tests/test_net_ops_yardstick.py); for a size of 1 the
    reference divides by zero (W - 1) and this is the operation it denotes."""
    B, C, H, W = inp.shape
    xs = torch.arange(W, dtype=F64, device=inp.device).view(1, 1, W) + flow[:, 0]
    ys = torch.arange(H, dtype=F64, device=inp.device).view(1, H, 1) + flow[:, 1]
    x0, y0 = torch.floor(xs), torch.floor(ys)
    ax, ay = xs - x0, ys - y0
    x0 = x0.clamp(-2, W).long()
    y0 = y0.clamp(-2, H).long()
    flat = inp.reshape(B, C, H * W)
    out = torch.zeros_like(inp)
    absterms = torch.zeros_like(inp)
    for dy, dx, wgt in ((0, 0, (1 - ax) * (1 - ay)), (0, 1, ax * (1 - ay)), (1, 0, (1 - ax) * ay), (1, 1, ax * ay)):
        xi, yi = x0 + dx, y0 + dy
        ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).view(B, 1, H * W).expand(B, C, H * W)
        v = flat.gather(2, idx).view(B, C, H, W)
        t = torch.where(ok, wgt, torch.zeros_like(wgt))[:, None] * v
        out += t
        absterms += t.abs()
    return out, absterms


def backwarp_bound(inp, flow_fp32, scale, absterms):
    """The kernel forms the position x + u * scale in fp32 (<= 2 roundings: 2 u (|x| + |u scale|) per axis), its bilinear weights
    with <= 3 roundings and sums 4 products (<= 2 roundings each): 8 u sum|w_i v_i| + slope * position error, the slope of the
    bilinear interpolant along an axis being <= 2 max|in| of the image and channel."""
    B, C, H, W = inp.shape
    us, vs = flow_fp32[:, 0].to(F64) * scale, flow_fp32[:, 1].to(F64) * scale
    xs = torch.arange(W, dtype=F64, device=inp.device).view(1, 1, W)
    ys = torch.arange(H, dtype=F64, device=inp.device).view(1, H, 1)
    dpos = 2 * U * (xs.abs() + us.abs() + ys.abs() + vs.abs())
    m = inp.abs().amax(dim=(2, 3), keepdim=True)
    return 8 * U * absterms + 2 * m * dpos[:, None]


# ---- Regularization front: src/models.py:275-277 (oracle :245-247) ------------------------------------------------------------
def reg_prep(img1, img2, flow, scale):
    """img1 / img2 NCHW [B,3,H,W], flow NCHW [B,2,H,W] (fp32 values in float64).  Returns mean [B,2] (xflow.view(B,2,-1).mean(2)),
    rm = flow - mean, norm [B,H,W] = (img1 - backwarp(img2, flow * scale)).pow(2).sum(1).sqrt(), and the norm's bound."""
    B = flow.shape[0]
    mean = flow.reshape(B, 2, -1).mean(2)
    rm = flow - mean.view(B, 2, 1, 1)
    warp, absterms = backwarp(img2, flow * scale)
    d = img1 - warp
    norm = d.pow(2).sum(1).sqrt()
    wb = backwarp_bound(img2, flow, scale, absterms)
    # |norm_k - norm| <= sum_c |d_k,c - d_c| (warp bound + one rounding of the difference) + 4 u norm (squares, two sums, sqrt)
    nb = (wb + U * d.abs()).sum(1) + 4 * U * norm
    return mean, rm, norm, nb


def mean_bound(flow, HW):
    """A deterministic two-stage sum in fp32: per thread ceil(HW / 16384) sequential adds, a 64-lane tree (6), the block's four waves
    (4), the 64 partials' tree (6) and the division (1): (ceil(HW / 16384) + 17) u mean|u| + u |mean|."""
    B = flow.shape[0]
    n = math.ceil(HW / 16384) + 17
    a = flow.reshape(B, 2, -1)
    return n * U * a.abs().mean(2) + U * a.mean(2).abs()


# ---- Regularization tail: src/models.py:281-302 (oracle :252-259) ---------------------------------------------------------------
def reg_tail(dist, flow, wx, wy, bx, by, k):
    """dist [B,k*k,H,W], flow [B,2,H,W], wx / wy [k*k]: negsq = -dist^2; e = exp(negsq - max); div = 1 / sum e; unfold (zero padding);
    moduleScaleX / Y (1 x 1 conv with bias) of e * unfold, times div.  Returns (out [B,2,H,W], per-element bound)."""
    B, KK, H, W = dist.shape
    negsq = dist.pow(2).neg()
    m = negsq.max(1, keepdim=True)[0]
    e = (negsq - m).exp()
    z = e.sum(1, keepdim=True)
    div = z.reciprocal()
    outs, bounds = [], []
    # relative error of e_c in fp32: d*d (1 rounding), - max (1), exp (<= 2 ulp): u (|d_c^2| + |max| + |arg|) + 4 u
    re = U * (dist.pow(2) + m.abs() + (negsq - m).abs() + 4)
    for ch, w, b in ((0, wx, bx), (1, wy, by)):
        un = F.unfold(flow[:, ch:ch + 1], kernel_size=k, stride=1, padding=(k - 1) // 2).view(B, KK, H, W)
        wv = w.view(1, KK, 1, 1)
        o = ((wv * e * un).sum(1, keepdim=True) + b) * div
        # d o / d e_c = (w_c u_c - o) / Z; the products e*u and w*(...) and the KK-term fma chain plus bias, 1/Z, the final product
        bnd = ((wv * un - o).abs() * e * re).sum(1, keepdim=True) * div \
            + (KK + 3) * U * ((wv * e * un).abs().sum(1, keepdim=True) + abs(b)) * div + (KK + 3) * U * o.abs()
        outs.append(o)
        bounds.append(bnd)
    return torch.cat(outs, 1), torch.cat(bounds, 1)


# ---- mean subtraction and image pyramid: src/models.py:321-323, 336-343 (oracle :274-285) -------------------------------------
def pyramid(img1, img2, mean6, levels):
    """img1 / img2 NCHW [B,3,H,W]; mean6 the 6 means (frame 1, frame 2).  Returns [level 1..levels] NCHW [2B,3,h,w] (frames 1 then
    frames 2) and their bounds.  Level 1 = img - mean (one rounding); level L = F.interpolate(level L-1, bilinear,
    align_corners=False) at H >> (L-1): on exact halvings (the sizes tested) the weights are 1/2 and exact, 3 rounded sums per value,
    and the error of level L-1 passes through the convex combination: bound_L = interp(bound_L-1) + 4 u interp(|level L-1|)."""
    B, _, H, W = img1.shape
    m1 = torch.tensor(mean6[:3], dtype=F64, device=img1.device).view(1, 3, 1, 1)
    m2 = torch.tensor(mean6[3:], dtype=F64, device=img1.device).view(1, 3, 1, 1)
    x = torch.cat([img1 - m1, img2 - m2], 0)
    outs, bounds = [x], [U * x.abs()]
    for L in range(2, levels + 1):
        size = (H >> (L - 1), W >> (L - 1))
        ip = lambda t: F.interpolate(t, size=size, mode="bilinear", align_corners=False)     # noqa: E731
        bounds.append(ip(bounds[-1]) + 4 * U * ip(outs[-1].abs()))
        outs.append(ip(outs[-1]))
    return outs, bounds


# ---- NetC.conv1 + level 1's NetC_ext + moduleFeat: src/models.py:70-72, 124, 227-232 (oracle :209, :292, :248) -----------------
def conv1_fused(x, w1, b1, we, be, wf, bfe):
    """x NCHW [N,3,H,W].  a = lrelu(conv7x7(x, pad 3)); ext = lrelu(conv1x1(a)); feat = lrelu(conv1x1(a)).  Returns
    ((a, ext, feat), (bound_a, bound_ext, bound_feat)).  conv1: 147 products and the bias (<= 149 roundings in any order);
    LeakyReLU is 1-Lipschitz, its fp32 slope 0.1f and product add <= 2 u |out|; a 1 x 1 layer: |W| bound_a carried through plus
    34 u (|W| |a| + |b|) of its own 32-term sum."""
    a = _lrelu(F.conv2d(x, w1, b1, padding=3))
    ba = 150 * U * (F.conv2d(x.abs(), w1.abs(), b1.abs(), padding=3)) + 2 * U * a.abs()
    outs, bounds = [a], [ba]
    for w, b in ((we, be), (wf, bfe)):
        y = _lrelu(F.conv2d(a, w, b))
        by = F.conv2d(ba, w.abs()) + 34 * U * F.conv2d(a.abs(), w.abs(), b.abs()) + 2 * U * y.abs()
        outs.append(y)
        bounds.append(by)
    return tuple(outs), tuple(bounds)
