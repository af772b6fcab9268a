"""The contract of pivlfn_flow_moments_accumulate and pivlfn_flow_hist_accumulate (include/pivlfn.h) in NumPy, operation for operation:
every product, difference and quotient is one float64 operation of NumPy (correctly rounded, never fused), the frames are added in
order, and the counts are integers.  `moments` and `hist` work on whole planes; `moments_loops` and `hist_loops` read the contract
literally, vector by vector.  A helper, not a test."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
TERMS = 21


def hist_words(nbins, jbins, fbins):
    return 2 * (nbins + 2) + jbins * jbins + 1 + 2 * fbins + 2


def layout(nbins, jbins, fbins):
    """Word offsets of the parts of hist: u, v, joint, outside, frac_u, frac_v, counted (left out = counted + 1)."""
    u, v = 0, nbins + 2
    joint = 2 * (nbins + 2)
    outside = joint + jbins * jbins
    return {"u": u, "v": v, "joint": joint, "outside": outside, "frac_u": outside + 1, "frac_v": outside + 1 + fbins,
            "counted": outside + 1 + 2 * fbins}


def taken(flow, mask=None, mean=None, scale=None):
    """[H,W] bool for one frame [2,H,W]: the vectors that are NOT left out."""
    with np.errstate(invalid="ignore"):
        k = (np.abs(flow[0].astype(f64)) <= 1e9) & (np.abs(flow[1].astype(f64)) <= 1e9)          # NaN compares false
        if mask is not None:
            k &= mask == 0
        if mean is not None:
            k &= np.isfinite(mean[0]) & np.isfinite(mean[1])
        if scale is not None:
            k &= np.isfinite(scale[0]) & np.isfinite(scale[1]) & (scale[0] > 0) & (scale[1] > 0)
    return k


def values(flow, mean=None):
    U, V = flow[0].astype(f64), flow[1].astype(f64)
    if mean is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            U, V = U - mean[0], V - mean[1]
    return U, V


def moments(flow, mask, mean, thr, acc):
    """flow [B,2,H,W] float32, mask [B,H,W] or None, mean [2,H,W] or None, thr [H,W] or None, acc [21,H,W] float64: the new acc."""
    flow = np.asarray(flow)
    acc = np.array(acc, dtype=f64)
    hole = np.zeros(flow.shape[2:]) if thr is None else np.asarray(thr, f64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(flow.shape[0]):
            k = taken(flow[b], None if mask is None else mask[b], mean)
            U, V = values(flow[b], mean)
            uu, vv, P = U * U, V * V, U * V
            terms = [np.ones_like(U), U, V, uu, vv, P, uu * U, vv * V, uu * V, vv * U, uu * uu, vv * vv, uu * vv]
            for t, term in enumerate(terms):
                acc[t] = np.where(k, acc[t] + term, acc[t])
            event = k & (np.abs(P) > hole)                                        # a NaN hole admits nothing
            quads = (event & (U > 0) & (V > 0), event & (U < 0) & (V > 0), event & (U < 0) & (V < 0), event & (U > 0) & (V < 0))
            for q, inq in enumerate(quads):
                acc[13 + q] = np.where(inq, acc[13 + q] + 1.0, acc[13 + q])
                acc[17 + q] = np.where(inq, acc[17 + q] + P, acc[17 + q])
    return acc


def moments_loops(flow, mask, mean, thr, acc):
    """The same, vector by vector."""
    B, _, H, W = flow.shape
    acc = np.array(acc, dtype=f64)
    for y in range(H):
        for x in range(W):
            for b in range(B):
                u, v = f64(flow[b, 0, y, x]), f64(flow[b, 1, y, x])
                if mask is not None and mask[b, y, x] != 0:
                    continue
                if not (abs(u) <= 1e9 and abs(v) <= 1e9):
                    continue
                U, V = u, v
                if mean is not None:
                    if not (math.isfinite(mean[0, y, x]) and math.isfinite(mean[1, y, x])):
                        continue
                    U, V = u - f64(mean[0, y, x]), v - f64(mean[1, y, x])
                uu, vv, P = U * U, V * V, U * V
                for t, term in enumerate((f64(1.0), U, V, uu, vv, P, uu * U, vv * V, uu * V, vv * U, uu * uu, vv * vv, uu * vv)):
                    acc[t, y, x] = acc[t, y, x] + term
                hole = 0.0 if thr is None else thr[y, x]
                if abs(P) > hole:
                    q = 0 if U > 0 and V > 0 else 1 if U < 0 and V > 0 else 2 if U < 0 and V < 0 else 3 if U > 0 and V < 0 else None
                    if q is not None:
                        acc[13 + q, y, x] = acc[13 + q, y, x] + 1.0
                        acc[17 + q, y, x] = acc[17 + q, y, x] + P
    return acc


def _slots(X, lo, s, nbins):
    """0 under, 1 + bin, nbins + 1 over (a NaN t too)."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (X - lo) * s
        inside = (t >= 0) & (t < nbins)
        return np.where(t < 0, 0, np.where(inside, 1 + np.where(inside, t, 0).astype(np.int64), nbins + 1))


def _fraction(d, fbins):
    with np.errstate(invalid="ignore", over="ignore"):
        f = d - np.floor(d)
        return np.minimum((f * f64(fbins)).astype(np.int64), fbins - 1)


def hist(flow, mask, mean, scale, hist0, lo, hi, nbins, jbins, fbins):
    """flow [B,2,H,W] float32, mask, mean as above, scale [2,H,W] or None, hist0 [hist_words] uint64: the new hist."""
    flow = np.asarray(flow)
    out = np.array(hist0, dtype=np.uint64)
    assert out.shape == (hist_words(nbins, jbins, fbins),)
    at = layout(nbins, jbins, fbins)
    s, sj = f64(nbins) / (f64(hi) - f64(lo)), f64(jbins) / (f64(hi) - f64(lo))
    add = np.zeros(out.shape, np.int64)

    def count(words):
        add[:] += np.bincount(words, minlength=add.size)

    for b in range(flow.shape[0]):
        k = taken(flow[b], None if mask is None else mask[b], mean, scale)
        U, V = values(flow[b], mean)
        du, dv = flow[b, 0].astype(f64)[k], flow[b, 1].astype(f64)[k]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            X, Y = (U[k], V[k]) if scale is None else (U[k] / scale[0][k], V[k] / scale[1][k])
            count(at["u"] + _slots(X, lo, s, nbins))
            count(at["v"] + _slots(Y, lo, s, nbins))
            tu, tv = (X - lo) * sj, (Y - lo) * sj
            inside = (tu >= 0) & (tu < jbins) & (tv >= 0) & (tv < jbins)
            count(at["joint"] + tv[inside].astype(np.int64) * jbins + tu[inside].astype(np.int64))
            add[at["outside"]] += np.count_nonzero(~inside)
        if fbins:
            count(at["frac_u"] + _fraction(du, fbins))
            count(at["frac_v"] + _fraction(dv, fbins))
        add[at["counted"]] += np.count_nonzero(k)
        add[at["counted"] + 1] += k.size - np.count_nonzero(k)
    return out + add.astype(np.uint64)


def hist_loops(flow, mask, mean, scale, hist0, lo, hi, nbins, jbins, fbins):
    """The same, vector by vector."""
    B, _, H, W = flow.shape
    out = [int(c) for c in hist0]
    at = layout(nbins, jbins, fbins)
    s, sj = f64(nbins) / (f64(hi) - f64(lo)), f64(jbins) / (f64(hi) - f64(lo))

    def slot(x):
        t = (x - f64(lo)) * s
        return 0 if t < 0 else 1 + int(t) if t < nbins else nbins + 1

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for b in range(B):
            for y in range(H):
                for x in range(W):
                    u, v = f64(flow[b, 0, y, x]), f64(flow[b, 1, y, x])
                    left_out = (mask is not None and mask[b, y, x] != 0) or not (abs(u) <= 1e9 and abs(v) <= 1e9)
                    if mean is not None and not (math.isfinite(mean[0, y, x]) and math.isfinite(mean[1, y, x])):
                        left_out = True
                    if scale is not None:
                        su, sv = f64(scale[0, y, x]), f64(scale[1, y, x])
                        if not (math.isfinite(su) and math.isfinite(sv) and su > 0 and sv > 0):
                            left_out = True
                    if left_out:
                        out[at["counted"] + 1] += 1
                        continue
                    U, V = (u, v) if mean is None else (u - f64(mean[0, y, x]), v - f64(mean[1, y, x]))
                    X, Y = (U, V) if scale is None else (U / su, V / sv)
                    out[at["u"] + slot(X)] += 1
                    out[at["v"] + slot(Y)] += 1
                    tu, tv = (X - f64(lo)) * sj, (Y - f64(lo)) * sj
                    if 0 <= tu < jbins and 0 <= tv < jbins:
                        out[at["joint"] + int(tv) * jbins + int(tu)] += 1
                    else:
                        out[at["outside"]] += 1
                    for name, d in (("frac_u", u), ("frac_v", v)):
                        if fbins:
                            f = d - np.floor(d)
                            out[at[name] + min(int(f * f64(fbins)), fbins - 1)] += 1
                    out[at["counted"]] += 1
    return np.array(out, dtype=np.uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def random_case(rng, B, H, W, sigma=1.5, holes=True):
    """Flows [B,2,H,W] float32 with NaN, 1e10, -inf and -0.0 vectors, a speckle mask, and float64 mean [2,H,W], scale [2,H,W] (with
    a zero, a negative and a NaN where there is room) and thr [H,W]."""
    flow = rng.normal(0, sigma, (B, 2, H, W)).astype(f32)
    mask = (rng.random((B, H, W)) < 0.1).astype(np.uint8) * 5
    mean = rng.normal(0, 0.3, (2, H, W))
    scale = 0.5 + rng.random((2, H, W))
    thr = 0.3 * rng.random((H, W))
    if holes and H * W >= 40:
        for j, bad in enumerate((np.nan, 1e10, -np.inf, -0.0)):
            flow[rng.integers(0, B), j % 2, rng.integers(0, H), rng.integers(0, W)] = bad
        flat = scale.reshape(2, -1)
        flat[0, 3], flat[1, 11], flat[0, 17], flat[1, 23] = 0.0, -1.0, np.nan, np.inf
        mean.reshape(2, -1)[1, 29] = np.nan
        thr.reshape(-1)[31] = np.nan
    return flow, mask, mean, scale, thr


def read_flo(path):
    """A Middlebury .flo file as [2,H,W] float32."""
    raw = np.fromfile(path, np.uint8)
    assert raw[:4].tobytes() == b"PIEH"
    w, h = (int(x) for x in raw[4:12].view(np.int32))
    return np.ascontiguousarray(raw[12:].view(f32).reshape(h, w, 2).transpose(2, 0, 1))


# ---- what DistributionResult derives, restated for its tests ----------------------------------------------------------------------------
def central(n, s1, s2, s3, s4):
    """(m2, m3, m4) by the binomial formulas."""
    m = s1 / n
    m2 = s2 / n - m * m
    m3 = s3 / n - 3 * m * s2 / n + 2 * m ** 3
    m4 = s4 / n - 4 * m * s3 / n + 6 * m * m * s2 / n - 3 * m ** 4
    return m2, m3, m4


def peak_locking(counts):
    counts = np.asarray(counts, f64)
    return 1.0 - counts.min() / counts.max() if counts.sum() > 0 else math.nan
