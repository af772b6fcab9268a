"""Float64 restatements of the public custom ops: correlation forward (plain and fused with the back-warp) and backward, the
stand-alone back-warp and the bilinear resize.  What the fp32 kernels and the fp32 oracle are both measured against
(tests/test_gpu_corr_domain.py); tests/test_corr_reference_yardstick.py checks the restatements themselves on the CPU.
Plain torch float64 tensor operations (indexing, multiply, sum) on `device`: none of the library's kernels, not the oracle."""
import numpy as np
import torch
import torch.nn.functional as F


def _t64(a, device):
    t = torch.from_numpy(a) if isinstance(a, np.ndarray) else a
    return t.to(device).double()


def _warp64(t2, fx, fy):
    """t2 [B,C,H,W] float64 sampled bilinearly at the float64 pixel positions (fx, fy) [B,H,W]; taps outside the image contribute
    zero.  A position that is not finite (a NaN flow) has no tap inside the image: the pixel is zero."""
    B, C, H, W = t2.shape
    x0, y0 = torch.floor(fx), torch.floor(fy)
    ax, ay = fx - x0, fy - y0
    out = torch.zeros_like(t2)
    flat = t2.reshape(B, C, H * W)
    zero = torch.zeros((), dtype=torch.float64, device=t2.device)
    for dy, dx, w in ((0, 0, (1 - ax) * (1 - ay)), (0, 1, ax * (1 - ay)), (1, 0, (1 - ax) * ay), (1, 1, ax * ay)):
        xi, yi = x0 + dx, y0 + dy
        ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)               # False for NaN
        xs = torch.where(ok, xi, zero).long()
        ys = torch.where(ok, yi, zero).long()
        idx = (ys * W + xs).reshape(B, 1, H * W).expand(B, C, H * W)
        out += (torch.gather(flat, 2, idx) * torch.where(ok, w, zero).reshape(B, 1, H * W)).reshape(B, C, H, W)
    return out


def _grid(H, W, device):
    return torch.meshgrid(torch.arange(H, device=device, dtype=torch.float64), torch.arange(W, device=device, dtype=torch.float64),
                          indexing="ij")


def backwarp_f64(x, flow, device="cpu"):
    """backwarp(x, flow)  (src/models.py:20-35) in pixel units: out[b,c,y,x] = bilinear(x[b,c], x + u, y + v) with the exact sum of
    the fp32 flow and the pixel index, float64 weights and blend.  Returns a float64 tensor on `device`."""
    t, tf = _t64(x, device), _t64(flow, device)
    yy, xx = _grid(t.shape[2], t.shape[3], device)
    return _warp64(t, xx + tf[:, 0], yy + tf[:, 1])


def fused_f64(f1, f2, fl, scale, s, leaky=True, device="cpu"):
    """leaky_relu(corr(f1, backwarp(f2, flow * scale)))  (src/models.py:20-35, 171-184; src/correlation.py:36-104) in float64 and in
    pixel units: the sample position is x + u * scale with the exact product of the two fp32 numbers, the blend weights and the
    dot products are float64.  What the fp32 kernel and the fp32 oracle are both measured against.  Any stride; fl = None is the
    plain correlation."""
    t1, t2 = _t64(f1, device), _t64(f2, device)
    B, C, H, W = t1.shape
    if fl is not None:
        tf = _t64(fl, device)
        yy, xx = _grid(H, W, device)
        f2w = _warp64(t2, xx + tf[:, 0] * float(np.float32(scale)), yy + tf[:, 1] * float(np.float32(scale)))
    else:
        f2w = t2
    Ho, Wo = -(-H // s), -(-W // s)
    pad = 3 * s
    f2p = torch.zeros(B, C, H + 2 * pad, W + 2 * pad, device=device, dtype=torch.float64)
    f2p[:, :, pad:pad + H, pad:pad + W] = f2w
    a = t1[:, :, ::s, ::s]
    out = torch.empty(B, 49, Ho, Wo, device=device, dtype=torch.float64)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            sh = f2p[:, :, pad + s * dy:pad + s * dy + H:s, pad + s * dx:pad + s * dx + W:s]
            out[:, 7 * (dy + 3) + (dx + 3)] = (a * sh).sum(dim=1) / C
    if leaky:
        out = torch.where(out >= 0, out, 0.1 * out)
    return out.cpu().numpy()


def corr_bwd_f64(f1, f2, go, s, device="cpu"):
    """(gradFirst, gradSecond) of the correlation (src/correlation.py:106-234), written out from the sums rather than through
    autograd.  On the stride-s grid (Y, X) in [0,Ho) x [0,Wo), t = 7(dy+3)+(dx+3):
      gradFirst [b,c,sY,sX] = 1/C * sum_t go[b,t,Y,X]       * second[b,c,s(Y+dy),s(X+dx)]
      gradSecond[b,c,sY,sX] = 1/C * sum_t go[b,t,Y-dy,X-dx] * first [b,c,s(Y-dy),s(X-dx)]
    with terms outside the grid zero, and zero at every position off the grid.  Float64 from the fp32 inputs; two float64 tensors
    of the inputs' shape on `device`."""
    t1, t2, tg = _t64(f1, device), _t64(f2, device), _t64(go, device)
    B, C, H, W = t1.shape
    Ho, Wo = -(-H // s), -(-W // s)
    assert tuple(tg.shape) == (B, 49, Ho, Wo)
    a = F.pad(t1[:, :, ::s, ::s], (3, 3, 3, 3))                      # the operands on the grid, three zero grid steps around
    b = F.pad(t2[:, :, ::s, ::s], (3, 3, 3, 3))
    gp = F.pad(tg, (3, 3, 3, 3))
    g1 = torch.zeros(B, C, Ho, Wo, device=device, dtype=torch.float64)
    g2 = torch.zeros(B, C, Ho, Wo, device=device, dtype=torch.float64)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            t = 7 * (dy + 3) + (dx + 3)
            g1 += tg[:, t:t + 1] * b[:, :, 3 + dy:3 + dy + Ho, 3 + dx:3 + dx + Wo]
            g2 += gp[:, t:t + 1, 3 - dy:3 - dy + Ho, 3 - dx:3 - dx + Wo] * a[:, :, 3 - dy:3 - dy + Ho, 3 - dx:3 - dx + Wo]
    full1 = torch.zeros(B, C, H, W, device=device, dtype=torch.float64)
    full2 = torch.zeros(B, C, H, W, device=device, dtype=torch.float64)
    full1[:, :, ::s, ::s] = g1 / C
    full2[:, :, ::s, ::s] = g2 / C
    return full1, full2


def resize_f64(x, size, mul=None):
    """torch's bilinear resize (align_corners=False) of x [B,C,H,W] in float64 on x's device, channel c multiplied by mul[c % 2]
    (the fp32 values of mul, the product in float64) when mul is given: estimate()'s resizes, inference.py:46-49, 57-61."""
    out = F.interpolate(x.double(), size=tuple(size), mode="bilinear", align_corners=False)
    if mul is not None:
        out[:, 0::2] *= float(np.float32(mul[0]))
        out[:, 1::2] *= float(np.float32(mul[1]))
    return out
