"""NumPy float64 restatement of the vortex identification contract of include/pivlfn.h (pivlfn_vortex_gamma), twice: `gamma_loops` is
the definition -- plain loops over the neighbours of every vector, every operation on its own, the exclusions spelled out -- and
`gamma_planes` is vectorised over shifted slices of the zero-padded field, one accumulator per row j and then the row sums, which is
the contract's order.  Every operation is a correctly rounded IEEE fp64 operation in both and on the device, so all three agree bit for
bit.  Both work on one pair; `batch_gamma` stacks pairs into the kernel's layout.  Also the test fields.  A helper, not a test."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
FEW, CENTRE_OUT = 1, 2
CORE = 2.0 / math.pi


def default_min_count(r):
    return (2 * r + 1) ** 2 // 2


def staged(flow, mask=None):
    """k, U, V, ux, uy of the contract for flow [2,H,W] float32 and mask [H,W] or None."""
    flow = np.asarray(flow)
    assert flow.dtype == f32 and flow.ndim == 3 and flow.shape[0] == 2
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        k = (np.abs(flow[0]) <= f32(1e9)) & (np.abs(flow[1]) <= f32(1e9))          # NaN compares false
        if mask is not None:
            k &= np.asarray(mask) == 0
        U, V = np.where(k, flow[0].astype(f64), 0.0), np.where(k, flow[1].astype(f64), 0.0)
        m = np.sqrt(U * U + V * V)
        pos = m > 0
        ux, uy = np.where(pos, U / np.where(pos, m, 1.0), 0.0), np.where(pos, V / np.where(pos, m, 1.0), 0.0)
    return k, U, V, ux, uy


def directions(r):
    """px[j+r][i+r] = i / d and py = j / d with d = sqrt(i*i + j*j); the centre, which no sum uses, is 0."""
    j, i = np.mgrid[-r:r + 1, -r:r + 1]
    d = np.sqrt((i * i + j * j).astype(f64))
    d[r, r] = 1.0
    return i.astype(f64) / d, j.astype(f64) / d


def _finish(S1, S2, N, k, min_count):
    few = N < min_count
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.stack([S1 / N.astype(f64), S2 / N.astype(f64)]).astype(f32)
    g[:, few] = f32(np.nan)
    return g, (few * FEW + (~k) * CENTRE_OUT).astype(np.uint8)


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def gamma_loops(flow, r, s=1, mask=None, min_count=None):
    """One pair: flow [2,H,W] float32 -> (gamma [2,H,W] float32, flag [H,W] uint8)."""
    min_count = default_min_count(r) if min_count is None else min_count
    k, U, V, ux, uy = staged(flow, mask)
    H, W = k.shape
    px, py = directions(r)
    S1, S2, N = np.zeros((H, W), f64), np.zeros((H, W), f64), np.zeros((H, W), np.int64)
    zero = f64(0.0)
    for y in range(H):
        for x in range(W):
            n, su, sv, s1 = 0, zero, zero, zero
            for j in range(-r, r + 1):
                ru, rv, r1 = zero, zero, zero
                for i in range(-r, r + 1):
                    yy, xx = y + j * s, x + i * s
                    inside = 0 <= yy < H and 0 <= xx < W
                    ru = ru + (U[yy, xx] if inside else zero)                       # the centre is part of the mean
                    rv = rv + (V[yy, xx] if inside else zero)
                    if inside and (i, j) != (0, 0) and k[yy, xx]:
                        n += 1
                        a, b = px[j + r, i + r] * uy[yy, xx], py[j + r, i + r] * ux[yy, xx]
                        r1 = r1 + (a - b)
                    else:
                        r1 = r1 + zero
                su, sv, s1 = su + ru, sv + rv, s1 + r1
            n_all = n + int(k[y, x])
            with np.errstate(invalid="ignore", divide="ignore"):
                mx, my = su / f64(n_all), sv / f64(n_all)
            s2 = zero
            for j in range(-r, r + 1):
                r2 = zero
                for i in range(-r, r + 1):
                    yy, xx = y + j * s, x + i * s
                    term = zero
                    if 0 <= yy < H and 0 <= xx < W and (i, j) != (0, 0) and k[yy, xx]:
                        du, dv = U[yy, xx] - mx, V[yy, xx] - my
                        m2 = np.sqrt(du * du + dv * dv)
                        if m2 > 0:
                            a, b = px[j + r, i + r] * dv, py[j + r, i + r] * du
                            term = (a - b) / m2
                    r2 = r2 + term
                s2 = s2 + r2
            S1[y, x], S2[y, x], N[y, x] = s1, s2, n
    return _finish(S1, S2, N, k, min_count)


# ---- the same, vectorised ----------------------------------------------------------------------------------------------------------
def gamma_planes(flow, r, s=1, mask=None, min_count=None):
    """One pair, as gamma_loops."""
    min_count = default_min_count(r) if min_count is None else min_count
    k, U, V, ux, uy = staged(flow, mask)
    H, W = k.shape
    px, py = directions(r)
    pad = r * s
    kp, Up, Vp, xp, yp = (np.pad(a, pad) for a in (k, U, V, ux, uy))               # outside the image: k = 0 and +0.0

    def shifted(a, i, j):
        return a[pad + j * s:pad + j * s + H, pad + i * s:pad + i * s + W]

    def window(term):
        """term(i, j) -> [H,W]; rows from i = -r to +r from +0.0, then the row sums from j = -r to +r from +0.0."""
        total = np.zeros((H, W), f64)
        for j in range(-r, r + 1):
            row = np.zeros((H, W), f64)
            for i in range(-r, r + 1):
                row = row + term(i, j)
            total = total + row
        return total

    def off_centre(i, j, a):
        return a if (i, j) != (0, 0) else np.zeros((H, W), a.dtype)

    N = sum(off_centre(i, j, shifted(kp, i, j).astype(np.int64)) for j in range(-r, r + 1) for i in range(-r, r + 1))
    SU, SV = window(lambda i, j: shifted(Up, i, j)), window(lambda i, j: shifted(Vp, i, j))
    S1 = window(lambda i, j: off_centre(i, j, np.where(shifted(kp, i, j), px[j + r, i + r] * shifted(yp, i, j) - py[j + r, i + r] * shifted(xp, i, j), 0.0)))
    with np.errstate(invalid="ignore", divide="ignore"):
        n_all = (N + k).astype(f64)
        mx, my = SU / n_all, SV / n_all

        def term2(i, j):
            du, dv = shifted(Up, i, j) - mx, shifted(Vp, i, j) - my
            m2 = np.sqrt(du * du + dv * dv)
            take = shifted(kp, i, j) & (m2 > 0)
            return off_centre(i, j, np.where(take, (px[j + r, i + r] * dv - py[j + r, i + r] * du) / np.where(take, m2, 1.0), 0.0))
        S2 = window(term2)
    return _finish(S1, S2, N, k, min_count)


def batch_gamma(flow, r, s=1, mask=None, min_count=None, one=gamma_planes):
    """flow [B,2,H,W] float32, mask [B,H,W] or None -> (gamma [B,2,H,W] float32, flag [B,H,W] uint8): every pair on its own."""
    res = [one(flow[b], r, s, None if mask is None else mask[b], min_count) for b in range(len(flow))]
    return np.stack([g for g, _ in res]), np.stack([f for _, f in res])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- what pivlfn.vortex.VortexField derives, restated for one pair -----------------------------------------------------------------
def core_radius(gamma2, sign=0, threshold=CORE):
    """sqrt(area / pi) of the region gamma2 > threshold (sign > 0), < -threshold (sign < 0) or |gamma2| > threshold (0)."""
    with np.errstate(invalid="ignore"):
        region = gamma2 > threshold if sign > 0 else gamma2 < -threshold if sign < 0 else np.abs(gamma2) > threshold
    return math.sqrt(float(region.sum()) / math.pi)


# ---- test fields -------------------------------------------------------------------------------------------------------------------
def random_case(rng, B, H, W, holes=True, sigma=3.0):
    """Random flows [B,2,H,W] float32 with NaN and 1e10 vectors, and a speckle mask with a block."""
    flow = rng.normal(0, sigma, (B, 2, H, W)).astype(f32)
    mask = (rng.random((B, H, W)) < 0.1).astype(np.uint8) * 5
    if holes:
        for n in range(max(2, H * W // 40)):
            flow[rng.integers(0, B), n % 2, rng.integers(0, H), rng.integers(0, W)] = (np.nan, 1e10, -np.inf)[n % 3]
        mask[0, H // 3:H // 2, W // 4:W // 2] = 1
    return flow, mask


def lamb_oseen(H=128, W=128, peak=4.0, shift=(1.5, -0.75)):
    """The project's own Lamb-Oseen field (pivlfn.synth.displacement_field) on the pixel grid: [2,H,W] float32."""
    from pivlfn import synth
    y, x = np.mgrid[0:H, 0:W].astype(f64)
    u, v = synth.displacement_field(x, y, H, W, peak, shift)
    return np.stack([u, v]).astype(f32)


def vortex_pair(H=96, W=128, centres=((36.5, 47.5), (91.5, 47.5)), rc=10.0, peaks=(3.0, -3.0), shift=(1.5, -0.75)):
    """Two Lamb-Oseen vortices of opposite sense plus a uniform drift: [2,H,W] float32."""
    y, x = np.mgrid[0:H, 0:W].astype(f64)
    u, v = np.full((H, W), shift[0]), np.full((H, W), shift[1])
    for (cx, cy), peak in zip(centres, peaks):
        dx, dy = x - cx, y - cy
        r2 = dx * dx + dy * dy
        rad = np.sqrt(r2) + 1e-12
        vt = peak * rc / 0.6382 * (1.0 - np.exp(-r2 / (rc * rc))) / rad
        u, v = u - vt * dy / rad, v + vt * dx / rad
    return np.stack([u, v]).astype(f32)


def read_flo(path):
    """A Middlebury .flo file as [2,H,W] float32."""
    raw = np.fromfile(path, np.uint8)
    assert raw[:4].tobytes() == b"PIEH"
    w, h = raw[4:12].view("<i4")
    return np.ascontiguousarray(raw[12:12 + 8 * w * h].view("<f4").reshape(h, w, 2).transpose(2, 0, 1))
