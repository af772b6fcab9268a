"""The arithmetic contract of pivlfn_match_quality (include/pivlfn.h) restated in numpy float64, vectorised over the pixels, with an
explicit loop over the 2r + 1 offsets of a window in the contract's order; float32 only for the sampling position.  numpy rounds every
operation on its own (it never forms an fma), its divisions and square roots are correctly rounded, and np.log is the one operation
that may differ from the device's in the last bits.

The window sums run over a zero-padded term map instead of a clipped window.  That gives the same bits: a term that is absent is +0.0
here, a sum that starts at +0.0 can only become -0.0 by adding two -0.0, which never happens to a sum that holds +0.0 or a non-zero
value, and x + (+0.0) == x for every other x.  tests/test_quality.py holds this against a scalar loop over the clipped window.

Also the input builders the CPU and GPU tests share."""
import numpy as np

FEW, FLAT, NO_PEAK, CENTRE_OUT = 1, 2, 4, 8
SHIFTS = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))             # (sx, sy)


def gray(img):
    """[C,H,W] float32 -> [H,W] float64."""
    x = img.astype(np.float64)
    if x.shape[0] == 1:
        return x[0]
    assert x.shape[0] == 3
    return ((x[0] + x[1]) + x[2]) / 3.0


def warp(g2, flow):
    """b [H,W] float64 (0 where invalid) and m [H,W] bool of one pair."""
    H, W = g2.shape
    u, v = flow[0].astype(np.float32), flow[1].astype(np.float32)
    xf = np.arange(W, dtype=np.float32)[None, :] + u                # one float32 addition
    yf = np.arange(H, dtype=np.float32)[:, None] + v
    assert xf.dtype == np.float32 and yf.dtype == np.float32
    xd, yd = xf.astype(np.float64), yf.astype(np.float64)
    with np.errstate(invalid="ignore"):
        m = (xd >= 0.0) & (xd <= W - 1) & (yd >= 0.0) & (yd <= H - 1)
    x0 = np.where(m, xd, 0.0).astype(np.int64)                      # truncation
    y0 = np.where(m, yd, 0.0).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = np.where(m, xd, 0.0) - x0, np.where(m, yd, 0.0) - y0
    top = (1.0 - fx) * g2[y0, x0] + fx * g2[y0, x1]
    bot = (1.0 - fx) * g2[y1, x0] + fx * g2[y1, x1]
    b = (1.0 - fy) * top + fy * bot
    return np.where(m, b, 0.0), m


def _shifted(x, sx, sy, fill):
    """y(q) = x(q + s) where q + s lies inside, `fill` elsewhere."""
    H, W = x.shape
    out = np.full_like(x, fill)
    ys, yd = (slice(sy, H), slice(0, H - sy)) if sy >= 0 else (slice(0, H + sy), slice(-sy, H))
    xs, xd = (slice(sx, W), slice(0, W - sx)) if sx >= 0 else (slice(0, W + sx), slice(-sx, W))
    out[yd, xd] = x[ys, xs]
    return out


def window_sum(t, r):
    """Rows left to right from +0.0, then the row sums top to bottom from +0.0."""
    H, W = t.shape
    p = np.zeros((H + 2 * r, W + 2 * r))
    p[r:r + H, r:r + W] = t
    rows = np.zeros((H + 2 * r, W))
    for dx in range(-r, r + 1):
        rows = rows + p[:, r + dx:r + dx + W]
    tot = np.zeros((H, W))
    for dy in range(-r, r + 1):
        tot = tot + rows[r + dy:r + dy + H]
    return tot


def pair_quality(img1, img2, flow, radius, mask=None, floor=1.0 / 255.0, min_count=None):
    """One pair: img [C,H,W] float32, flow [2,H,W] float32, mask [H,W] or None -> (quality [3,H,W] float32, flag [H,W] uint8,
    cs [5,H,W] float64: c_s of every shift, NaN where it is few or flat)."""
    r = int(radius)
    if min_count is None:
        min_count = ((2 * r + 1) ** 2 + 1) // 2
    a = gray(img1)
    b, m = warp(gray(img2), flow)
    H, W = a.shape
    k = np.ones((H, W), bool) if mask is None else (np.asarray(mask) == 0)
    cs, bad = [], []
    with np.errstate(all="ignore"):
        for sx, sy in SHIFTS:
            part = k & _shifted(m, sx, sy, False)
            bs = _shifted(b, sx, sy, 0.0)
            term = lambda x: window_sum(np.where(part, x, 0.0), r)      # noqa: E731
            n, A, AA, Bs, BB, AB = term(np.ones((H, W))), term(a), term(a * a), term(bs), term(bs * bs), term(a * bs)
            few = n < min_count
            va, vb, cov = AA - A * A / n, BB - Bs * Bs / n, AB - A * Bs / n
            flat = (va < floor * floor * n) | (vb < floor * floor * n)
            cs.append(cov / np.sqrt(va * vb))
            bad.append(np.where(few, FEW, np.where(flat, FLAT, 0)))
        c0, cxm, cxp, cym, cyp = cs
        flag = bad[0].astype(np.uint8)
        ok = (bad[1] == 0) & (bad[2] == 0) & (bad[3] == 0) & (bad[4] == 0) & (c0 > 0.0)
        for cm, cp in ((cxm, cxp), (cym, cyp)):
            ok &= (cm > 0.0) & (cp > 0.0) & (c0 >= cm) & (c0 >= cp) & ((2.0 * c0 - cm) - cp >= 1e-6)
        fit = ok & (flag == 0)
        flag[(flag == 0) & ~ok] = NO_PEAK
        flag[~k | ~m] |= CENTRE_OUT
        l0 = np.log(c0)
        d = []
        for cm, cp in ((cxm, cxp), (cym, cyp)):
            lm, lp = np.log(cm), np.log(cp)
            d.append(np.where(fit, 0.5 * (lm - lp) / ((lm - 2.0 * l0) + lp), 0.0))
        c = np.where((flag & (FEW | FLAT)) != 0, np.nan, c0)
    quality = np.stack([c, d[0], d[1]]).astype(np.float32)
    return quality, flag, np.stack([np.where(s == 0, x, np.nan) for x, s in zip(cs, bad)])


def batch_quality(img1, img2, flow, radius, mask=None, floor=1.0 / 255.0, min_count=None):
    """[B,C,H,W], [B,2,H,W], [B,H,W] or None -> quality [B,3,H,W] float32, flag [B,H,W] uint8."""
    out = [pair_quality(img1[i], img2[i], flow[i], radius, None if mask is None else mask[i], floor, min_count)[:2]
           for i in range(len(img1))]
    return np.stack([q for q, _ in out]), np.stack([f for _, f in out])


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def particle_images(B, H, W, C, seed):
    """img1, img2 [B,C,H,W] float32 in [0,1] and the true flows [B,2,H,W] from pivlfn.synth; C = 3: three different channels."""
    from pivlfn import synth
    a, c, f = [], [], []
    for i in range(B):
        i1, i2, fl = synth.particle_pair(H, W, seed + i)
        a.append(i1.astype(np.float32) / np.float32(255.0))
        c.append(i2.astype(np.float32) / np.float32(255.0))
        f.append(fl)
    a, c = np.stack(a)[:, None], np.stack(c)[:, None]
    if C == 3:
        a, c = (np.concatenate([x, np.float32(0.75) * x + np.float32(0.1), x * x], axis=1) for x in (a, c))
    return np.ascontiguousarray(a), np.ascontiguousarray(c), np.stack(f).astype(np.float32)


def noise_images(B, H, W, C, seed):
    """Plain noise in [-1, 2]: covariances and terms of both signs."""
    g = np.random.default_rng(seed)
    return ((3.0 * g.random((B, C, H, W)) - 1.0).astype(np.float32), (3.0 * g.random((B, C, H, W)) - 1.0).astype(np.float32))


def wild_flow(B, H, W, seed):
    """Smooth plus noise of sigma 1.5 px; the top row and left column point far outside; NaN, +-inf and 1e10 sprinkled in."""
    g = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    f = np.stack([np.stack([2.0 * np.sin(0.11 * yy + i) + 0.5, 1.5 * np.cos(0.07 * xx - i) - 0.25]) for i in range(B)])
    f = (f + 1.5 * g.standard_normal(f.shape)).astype(np.float32)
    f[:, 1, 0, :] = -40.0
    f[:, 0, :, 0] = -1e4
    n = B * H * W
    for k, val in enumerate((np.nan, np.inf, -np.inf, 1e10)):
        at = g.choice(n, size=max(1, n // 97), replace=False)
        f.reshape(B, 2, -1)[at // (H * W), k % 2, at % (H * W)] = val
    return f


def speckle_mask(B, H, W, seed, block):
    """A fully masked block of `block` x `block` pixels (clipped to the image) at the lower right, and speckles."""
    g = np.random.default_rng(seed)
    m = (g.random((B, H, W)) < 0.03).astype(np.uint8) * 255
    m[:, max(H - block, 0):, max(W - block, 0):] = 1
    return m


def flatten_patch(img1, img2, y, x, size=9, value=0.25):
    """One all-constant size x size patch at (y, x) in both images, in place."""
    for img in (img1, img2):
        img[:, :, y:y + size, x:x + size] = np.float32(value)
