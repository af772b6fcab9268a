"""The arithmetic contract of pivlfn_flow_uncertainty and pivlfn_uncertainty_accumulate (include/pivlfn.h) restated in numpy float64,
vectorised over the pixels, in the style of tests/quality_restatement.py whose gray value, warp, window sum and input builders it
uses.  numpy rounds every operation on its own, its divisions and square roots are correctly rounded, and np.log is the one operation
that may differ from the device's in the last bits.

Every box sum (the high-pass means, the lag box, the window sums) runs over a zero-padded term map instead of a clipped window; that
gives the same bits, for the reason written out in quality_restatement.py."""
import numpy as np

import quality_restatement as qr

FEW, FLAT, NO_PEAK, NO_VARIANCE, CENTRE_OUT = 1, 2, 4, 8, 16
UNUSABLE = FEW | FLAT | NO_PEAK | NO_VARIANCE
AXES = ((1, 0), (0, 1))                                          # (ex, ey): x, then y


def pair_fields(img1, img2, flow, radius, lag, mask=None):
    """What the window sums are taken of.  Returns v [H,W] bool, p [H,W], and per axis (pair [H,W] bool, s, d, g)."""
    r = int(radius)
    a = qr.gray(img1)
    b, m = qr.warp(qr.gray(img2), flow)
    H, W = a.shape
    k = np.ones((H, W), bool) if mask is None else (np.asarray(mask) == 0)
    v = k & m
    with np.errstate(all="ignore"):
        n1 = qr.window_sum(np.where(v, 1.0, 0.0), r)
        A1, B1 = qr.window_sum(np.where(v, a, 0.0), r), qr.window_sum(np.where(v, b, 0.0), r)
        ah, bh = np.where(v, a - A1 / n1, 0.0), np.where(v, b - B1 / n1, 0.0)
        p = np.where(v, ah * bh, 0.0)
        axes = []
        for ex, ey in AXES:
            pair = v & qr._shifted(v, ex, ey, False)
            t1, t2 = ah * qr._shifted(bh, ex, ey, 0.0), qr._shifted(ah, ex, ey, 0.0) * bh
            s, d = np.where(pair, t1 + t2, 0.0), np.where(pair, t1 - t2, 0.0)
            D = qr.window_sum(d, int(lag))
            axes.append((pair, s, d, np.where(pair, d * D, 0.0)))
    return v, p, axes


def pair_uncertainty(img1, img2, flow, radius, lag=2, mask=None, floor=1.0 / 255.0, min_count=None):
    """One pair: img [C,H,W] float32, flow [2,H,W] float32, mask [H,W] or None -> (unc [2,H,W] float32, flag [H,W] uint8,
    parts: a dict of the float64 window sums n0, C0 and per axis n, S, V)."""
    r = int(radius)
    if min_count is None:
        min_count = ((2 * r + 1) ** 2 + 1) // 2
    v, p, axes = pair_fields(img1, img2, flow, r, lag, mask)
    n0, C0 = qr.window_sum(np.where(v, 1.0, 0.0), r), qr.window_sum(p, r)
    parts = {"n0": n0, "C0": C0, "n": [], "S": [], "V": []}
    few, no_peak, no_var, u = n0 < min_count, np.zeros(v.shape, bool), np.zeros(v.shape, bool), []
    with np.errstate(all="ignore"):
        l0 = np.log(C0)
        for pair, s, _, g in axes:
            n, S, V = qr.window_sum(np.where(pair, 1.0, 0.0), r), qr.window_sum(s, r), qr.window_sum(g, r)
            for key, val in (("n", n), ("S", S), ("V", V)):
                parts[key].append(val)
            few |= n < min_count
            sig = np.sqrt(V)
            Cpm = 0.5 * S
            Cm, Cp = Cpm - 0.5 * sig, Cpm + 0.5 * sig
            no_peak |= (Cm <= 0.0) | (C0 - Cp < 1e-6 * C0)
            no_var |= (V <= 0.0) | ~np.isfinite(V)
            lm, lp = np.log(Cm), np.log(Cp)
            u.append(np.abs(0.5 * (lm - lp) / ((lm - 2.0 * l0) + lp)))
        flat = ~few & (C0 < (floor * floor) * n0)
    rated = ~few & ~flat
    flag = (np.where(few, FEW, 0) | np.where(flat, FLAT, 0) | np.where(rated & no_peak, NO_PEAK, 0)
            | np.where(rated & no_var, NO_VARIANCE, 0) | np.where(~v, CENTRE_OUT, 0)).astype(np.uint8)
    bad = (flag & UNUSABLE) != 0
    unc = np.stack([np.where(bad, np.nan, x) for x in u]).astype(np.float32)
    return unc, flag, parts


def pair_peak_residual(img1, img2, flow, radius, mask=None):
    """[2,H,W] float64: where the peak of the correlation that pair_uncertainty rates actually sits -- the three-point Gaussian fit
    through C_minus = sum a'(q+e) b'(q), C0 and C_plus = sum a'(q) b'(q+e) of the same high-passed windows (NaN where it has none)."""
    r = int(radius)
    a = qr.gray(img1)
    b, m = qr.warp(qr.gray(img2), flow)
    v = m if mask is None else (m & (np.asarray(mask) == 0))
    out = []
    with np.errstate(all="ignore"):
        n1 = qr.window_sum(np.where(v, 1.0, 0.0), r)
        ah = np.where(v, a - qr.window_sum(np.where(v, a, 0.0), r) / n1, 0.0)
        bh = np.where(v, b - qr.window_sum(np.where(v, b, 0.0), r) / n1, 0.0)
        l0 = np.log(qr.window_sum(ah * bh, r))
        for ex, ey in AXES:
            pair = v & qr._shifted(v, ex, ey, False)
            lp = np.log(qr.window_sum(np.where(pair, ah * qr._shifted(bh, ex, ey, 0.0), 0.0), r))
            lm = np.log(qr.window_sum(np.where(pair, qr._shifted(ah, ex, ey, 0.0) * bh, 0.0), r))
            out.append(0.5 * (lm - lp) / ((lm - 2.0 * l0) + lp))
    return np.stack(out)


def batch_uncertainty(img1, img2, flow, radius, lag=2, mask=None, floor=1.0 / 255.0, min_count=None):
    """[B,C,H,W], [B,2,H,W], [B,H,W] or None -> unc [B,2,H,W] float32, flag [B,H,W] uint8."""
    out = [pair_uncertainty(img1[i], img2[i], flow[i], radius, lag, None if mask is None else mask[i], floor, min_count)[:2]
           for i in range(len(img1))]
    return np.stack([u for u, _ in out]), np.stack([f for _, f in out])


def accumulate(sums, unc, flag):
    """pivlfn_uncertainty_accumulate: sums [3,H,W] float64 (sum ux^2, sum uy^2, n) plus the pairs of unc [B,2,H,W] float32 in batch
    order, pixels with one of bits 0-3 left out.  Returns the new sums."""
    sums = np.array(sums, dtype=np.float64)
    for u, f in zip(unc, flag):
        ok = (f & UNUSABLE) == 0
        ux, uy = u[0].astype(np.float64), u[1].astype(np.float64)
        sums[0] = np.where(ok, sums[0] + ux * ux, sums[0])
        sums[1] = np.where(ok, sums[1] + uy * uy, sums[1])
        sums[2] = np.where(ok, sums[2] + 1.0, sums[2])
    return sums


def noisy_particle_pair(H, W, shift, sigma, seed, ppp=0.05, diameter=2.5, offset=0.2):
    """The property test's images: Gaussian particle images of `diameter` px (e^-2 width) at `ppp` particles per pixel, peak
    intensities uniform in 0.2..0.4 (50 to 100 grey levels of an 8-bit frame) on an offset of 0.2, the second frame's particles moved by the uniform `shift` (sx, sy) px,
    independent Gaussian noise of `sigma` on both.  -> img1, img2 [1,H,W] float32."""
    g = np.random.default_rng(seed)
    pad = 8
    n = int(round(ppp * (H + 2 * pad) * (W + 2 * pad)))
    px, py = g.uniform(-pad, W + pad, n), g.uniform(-pad, H + pad, n)
    amp = g.uniform(0.2, 0.4, n)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = []
    for sx, sy in ((0.0, 0.0), shift):
        img = np.full((H, W), offset)
        for x, y, a in zip(px + sx, py + sy, amp):
            x0, x1, y0, y1 = max(int(x) - 6, 0), min(int(x) + 8, W), max(int(y) - 6, 0), min(int(y) + 8, H)
            if x0 < x1 and y0 < y1:
                img[y0:y1, x0:x1] += a * np.exp(-8.0 * ((xx[y0:y1, x0:x1] - x) ** 2 + (yy[y0:y1, x0:x1] - y) ** 2) / diameter ** 2)
        out.append((img + sigma * g.standard_normal((H, W))).astype(np.float32)[None])
    return out[0], out[1]
