"""NumPy float64 restatement of the two-point contract of include/pivlfn.h (pivlfn_twopoint_accumulate), twice: `accumulate_loops` is
the definition -- a plain loop over frames, directions, separations, rows and columns with an explicit tree -- and `accumulate` is
vectorised over the rows and columns of a frame, the tree as repeated t[0::2] + t[1::2] after padding.  Every operation is a correctly
rounded IEEE fp64 operation in both and on the device, so all three agree bit for bit.  Then the derived quantities of
pivlfn/twopoint.py (TwoPointResult), written independently of it, and the test fields.  A helper, not a test."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
NTERMS = 15


def valid(flow, mask=None):
    """k of the contract for flow [2,H,W] float32 and mask [H,W] or None."""
    with np.errstate(invalid="ignore"):
        k = (np.abs(flow[0]) <= f32(1e9)) & (np.abs(flow[1]) <= f32(1e9))          # NaN compares false
    if mask is not None:
        k = k & (np.asarray(mask) == 0)
    return k


def values(flow, mean=None):
    U, V = flow[0].astype(f64), flow[1].astype(f64)
    if mean is not None:
        with np.errstate(invalid="ignore"):
            U, V = U - mean[0], V - mean[1]
    return U, V


def tree(leaves):
    """The root of t[i] = t[2i] + t[2i+1] over the last axis, padded with +0.0 to the next power of two; one leaf is its own root."""
    W = leaves.shape[-1]
    P = 1
    while P < W:
        P *= 2
    t = np.concatenate([leaves, np.zeros(leaves.shape[:-1] + (P - W,), f64)], axis=-1)
    while t.shape[-1] > 1:
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


def pair_terms(Ua, Va, Ub, Vb, d):
    """The fifteen terms of pairs that take part, stacked on a new first axis."""
    du, dv = Ub - Ua, Vb - Va
    dL, dT = (du, dv) if d == 0 else (dv, du)
    return np.stack([np.ones_like(Ua), Ua, Va, Ub, Vb, Ua * Ua, Va * Va, Ub * Ub, Vb * Vb, Ua * Ub, Va * Vb, Ua * Vb, Va * Ub,
                     (dL * dL) * dL, (dL * dT) * dT])


def accumulate(flow, mask, mean, acc, max_sep, step):
    """flow [B,2,H,W] float32, mask [B,H,W] or None, mean [2,H,W] float64 or None, acc [2,max_sep+1,15,H] float64: returns the new acc
    (the argument is not changed)."""
    flow = np.asarray(flow)
    assert flow.dtype == f32 and flow.ndim == 4 and flow.shape[1] == 2
    B, _, H, W = flow.shape
    acc = np.array(acc, dtype=f64)
    assert acc.shape == (2, max_sep + 1, NTERMS, H)
    for b in range(B):
        k = valid(flow[b], None if mask is None else mask[b])
        U, V = values(flow[b], mean)
        for d in (0, 1):
            for r in range(max_sep + 1):
                s = r * step
                dy, dx = (0, s) if d == 0 else (s, 0)
                terms = np.zeros((NTERMS, H, W), f64)
                if dy < H and dx < W:
                    h, w = H - dy, W - dx
                    take = k[:h, :w] & k[dy:, dx:]
                    with np.errstate(invalid="ignore", over="ignore"):
                        t = pair_terms(U[:h, :w], V[:h, :w], U[dy:, dx:], V[dy:, dx:], d)
                    terms[:, :h, :w] = np.where(take, t, 0.0)                     # a pair that does not take part: +0.0 everywhere
                acc[d, r] = acc[d, r] + tree(terms)
    return acc


def accumulate_loops(flow, mask, mean, acc, max_sep, step):
    """The same by plain loops: the contract read literally."""
    B, _, H, W = flow.shape
    acc = np.array(acc, dtype=f64)
    P = 1
    while P < W:
        P *= 2
    zero = f64(0.0)
    for b in range(B):
        for d in (0, 1):
            for r in range(max_sep + 1):
                for y in range(H):
                    leaves = [[zero] * P for _ in range(NTERMS)]
                    for x in range(W):
                        yb, xb = (y, x + r * step) if d == 0 else (y + r * step, x)
                        if yb >= H or xb >= W:
                            continue
                        ok = True
                        for (yy, xx) in ((y, x), (yb, xb)):
                            u, v = flow[b, 0, yy, xx], flow[b, 1, yy, xx]
                            if mask is not None and mask[b, yy, xx] != 0:
                                ok = False
                            if not (abs(u) <= f32(1e9) and abs(v) <= f32(1e9)):
                                ok = False
                        if not ok:
                            continue
                        Ua, Va, Ub, Vb = f64(flow[b, 0, y, x]), f64(flow[b, 1, y, x]), f64(flow[b, 0, yb, xb]), f64(flow[b, 1, yb, xb])
                        if mean is not None:
                            Ua, Va, Ub, Vb = Ua - mean[0, y, x], Va - mean[1, y, x], Ub - mean[0, yb, xb], Vb - mean[1, yb, xb]
                        dL, dT = (Ub - Ua, Vb - Va) if d == 0 else (Vb - Va, Ub - Ua)
                        for i, t in enumerate((f64(1.0), Ua, Va, Ub, Vb, Ua * Ua, Va * Va, Ub * Ub, Vb * Vb, Ua * Ub, Va * Vb, Ua * Vb,
                                               Va * Ub, (dL * dL) * dL, (dL * dT) * dT)):
                            leaves[i][x] = t
                    for i in range(NTERMS):
                        t = leaves[i]
                        while len(t) > 1:
                            t = [t[2 * j] + t[2 * j + 1] for j in range(len(t) // 2)]
                        acc[d, r, i, y] = acc[d, r, i, y] + t[0]
    return acc


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- what pivlfn.twopoint.TwoPointResult derives, restated ---------------------------------------------------------------------------
# the term indices: (product, sum at a, sum at b, square at a, square at b)
PICK = {"uu": (9, 1, 3, 5, 7), "vv": (10, 2, 4, 6, 8), "uv": (11, 1, 4, 5, 8), "vu": (12, 2, 3, 6, 7)}


def row_correlation(acc, which, d):
    """Per row: (n, cov, var_a, var_b, rho), each [R+1, H]."""
    xy, xa, yb, xx, yy = PICK[which]
    R1, H = acc.shape[1], acc.shape[3]
    out = np.full((5, R1, H), np.nan)
    for r in range(R1):
        for y in range(H):
            n = acc[d, r, 0, y]
            out[0, r, y] = n
            if n == 0:
                continue
            ma, mb = acc[d, r, xa, y] / n, acc[d, r, yb, y] / n
            cov, va, vb = acc[d, r, xy, y] / n - ma * mb, acc[d, r, xx, y] / n - ma * ma, acc[d, r, yy, y] / n - mb * mb
            out[1:4, r, y] = cov, va, vb
            if n >= 2 and va > 0 and vb > 0:
                out[4, r, y] = cov / math.sqrt(va * vb)
    return out


def pooled(acc, which, d, rows=slice(None)):
    """(n, cov, var_a, var_b, rho), each [R+1]: the n-weighted means over the rows."""
    c = row_correlation(acc, which, d)[:, :, rows]
    R1 = c.shape[1]
    out = np.full((5, R1), np.nan)
    for r in range(R1):
        n = c[0, r]
        have = n > 0
        tot = n[have].sum()
        out[0, r] = tot
        if tot == 0:
            continue
        cov, va, vb = ((n[have] * c[i, r][have]).sum() / tot for i in (1, 2, 3))
        out[1:4, r] = cov, va, vb
        if tot >= 2 and va > 0 and vb > 0:
            out[4, r] = cov / math.sqrt(va * vb)
    return out


def trapezoid_to_crossing(rho, step):
    """(scale, truncated, crossing) of a correlation sampled at r*step."""
    if not np.isfinite(rho[0]):
        return math.nan, True, None
    area, r = 0.0, 1
    while r < len(rho) and np.isfinite(rho[r]) and rho[r] > 0:
        area += 0.5 * (rho[r - 1] + rho[r]) * step
        r += 1
    if r == len(rho) or not np.isfinite(rho[r]):
        return area, True, None
    frac = rho[r - 1] / (rho[r - 1] - rho[r])
    return area + 0.5 * rho[r - 1] * frac * step, False, ((r - 1) + frac) * step


def parabola_fit(rho, step, lo=1, hi=4):
    """(microscale, noise share, c, ell) of rho = c - (r*step)^2/ell^2 fitted at r = lo..hi by the normal equations."""
    q = np.array([(r * step) ** 2 for r in range(lo, hi + 1)], f64)
    y = np.asarray(rho[lo:hi + 1], f64)
    if not np.isfinite(y).all():
        return math.nan, math.nan, math.nan, math.nan
    A = np.stack([np.ones_like(q), q], axis=1)
    c, slope = np.linalg.solve(A.T @ A, A.T @ y)
    if not (slope < 0 and c > 0):
        return math.nan, 1.0 - c, c, math.nan
    ell = math.sqrt(-1.0 / slope)
    return math.sqrt(c) * ell, 1.0 - c, c, ell


def summary(acc, step, frames):
    doc = {"frames": frames, "max_sep": acc.shape[1] - 1, "step": step, "rows": acc.shape[3]}
    for which in ("uu", "vv"):
        for d, axis in enumerate("xy"):
            n, cov, va, vb, rho = pooled(acc, which, d)
            scale, truncated, crossing = trapezoid_to_crossing(rho, step)
            lam, noise = parabola_fit(rho, step)[:2] if acc.shape[1] > 4 else (math.nan, math.nan)
            doc[f"{which}_{axis}"] = {"pairs": float(n[0]), "variance": float(va[0]), "integral_scale": float(scale), "truncated": truncated,
                                      "crossing": crossing, "taylor_microscale": float(lam), "noise_share": float(noise)}
    return doc


# ---- test fields -------------------------------------------------------------------------------------------------------------------
def random_case(rng, B, H, W, holes=True, sigma=3.0):
    """Random flows [B,2,H,W] float32 with NaN, 1e10, -inf and -0.0 vectors, a speckle mask with a block, and a random float64 mean."""
    flow = rng.normal(0, sigma, (B, 2, H, W)).astype(f32)
    mask = (rng.random((B, H, W)) < 0.1).astype(np.uint8) * 5
    if holes:
        for n in range(max(2, B * H * W // 40)):
            flow[rng.integers(0, B), n % 2, rng.integers(0, H), rng.integers(0, W)] = (np.nan, 1e10, -np.inf, -0.0)[n % 4]
        mask[0, H // 3:H // 2, W // 4:W // 2] = 1
    mean = rng.normal(0, 1, (2, H, W))
    return flow, mask, mean


def cosine_sequence(c, A=2.0, frames=8, H=4, W=72, period=18):
    """u = c + A*cos(2 pi x/period + 2 pi b/frames), v = 0, rounded to float32: [frames,2,H,W]."""
    x = np.arange(W, dtype=f64)
    flow = np.zeros((frames, 2, H, W), f32)
    for b in range(frames):
        flow[b, 0] = (c + A * np.cos(2 * math.pi * x / period + 2 * math.pi * b / frames)).astype(f32)[None, :]
    return flow


def read_flo(path):
    """A Middlebury .flo file as [2,H,W] float32."""
    raw = np.fromfile(path, np.uint8)
    assert raw[:4].tobytes() == b"PIEH"
    w, h = raw[4:12].view("<i4")
    return np.ascontiguousarray(raw[12:12 + 8 * w * h].view("<f4").reshape(h, w, 2).transpose(2, 0, 1))
