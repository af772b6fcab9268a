"""NumPy restatement of the two contracts of the synthetic-pair section of include/pivlfn.h (csrc/particles.hip).

displace(): pivlfn_particles_displace with the contract's exact operation order -- every step a correctly rounded float64 operation,
NumPy fuses nothing -- so the kernel is compared with it bit for bit.
render(): pivlfn_particles_render as plain float64 sums over the contract's footprint: per pixel V (the value), A (the sum of amp over
the covering particles) and n (their count).  check_render() holds a float32 intensity and a uint8 image against them with the
header's bound  |intensity - V| <= 2^-21 A + n 2^-24 V  and returns the largest |err| / tol it met."""
import numpy as np

LOST, BAD = 2, 8


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64 if a.dtype == np.float64 else np.uint8),
                                                                        b.view(np.int64 if b.dtype == np.float64 else np.uint8))


def _keys(f):
    return (((-0.5 * f + 1.0) * f - 0.5) * f, ((1.5 * f - 2.5) * f) * f + 1.0, ((-1.5 * f + 2.0) * f + 0.5) * f, ((0.5 * f - 0.5) * f) * f)


def displace(pos, flow, mask=None, flag=None, method=0):
    """pos [2,N] float64, flow [2,H,W] float32, mask [H,W] uint8 or None, flag [N] uint8 or None -> (out [2,N] float64, flag [N])."""
    pos = np.asarray(pos, np.float64)
    flow = np.asarray(flow, np.float32)
    _, H, W = flow.shape
    N = pos.shape[1]
    flag = np.zeros(N, np.uint8) if flag is None else np.array(flag, np.uint8)
    x, y = pos[0], pos[1]
    out = pos.copy()
    live = flag == 0
    nan = np.isnan(x) | np.isnan(y)
    flag[live & nan] = BAD
    go = live & ~nan
    with np.errstate(all="ignore"):
        xs, ys = np.where(go, x, 0.0), np.where(go, y, 0.0)
        xc = np.where(xs < 0.0, 0.0, np.where(xs > float(W - 1), float(W - 1), xs))
        yc = np.where(ys < 0.0, 0.0, np.where(ys > float(H - 1), float(H - 1), ys))
        ix = np.minimum(np.floor(xc).astype(np.int64), W - 2)
        iy = np.minimum(np.floor(yc).astype(np.int64), H - 2)
        fx, fy = xc - ix.astype(np.float64), yc - iy.astype(np.float64)
        m = np.zeros((H, W), np.uint8) if mask is None else np.asarray(mask).astype(np.uint8)
        known = np.ones(N, bool)
        S = []
        if method == 0:
            for c in flow.astype(np.float64):
                c00, c01, c10, c11 = c[iy, ix], c[iy, ix + 1], c[iy + 1, ix], c[iy + 1, ix + 1]
                for t in (c00, c01, c10, c11):
                    known &= np.abs(t) <= 1e9
                top = (1.0 - fx) * c00 + fx * c01
                bot = (1.0 - fx) * c10 + fx * c11
                S.append(top * (1.0 - fy) + bot * fy)
            known &= (m[iy, ix] | m[iy, ix + 1] | m[iy + 1, ix] | m[iy + 1, ix + 1]) == 0
        else:
            wx, wy = _keys(fx), _keys(fy)
            cols = [np.clip(ix - 1 + k, 0, W - 1) for k in range(4)]
            rows = [np.clip(iy - 1 + r, 0, H - 1) for r in range(4)]
            for c in flow.astype(np.float64):
                row = []
                for r in range(4):
                    t = [c[rows[r], cols[k]] for k in range(4)]
                    for v in t:
                        known &= np.abs(v) <= 1e9
                    row.append(((wx[0] * t[0] + wx[1] * t[1]) + wx[2] * t[2]) + wx[3] * t[3])
                S.append(((wy[0] * row[0] + wy[1] * row[1]) + wy[2] * row[2]) + wy[3] * row[3])
            for r in range(4):
                for k in range(4):
                    known &= m[rows[r], cols[k]] == 0
        moved = go & known
        out[0] = np.where(moved, x + S[0], x)
        out[1] = np.where(moved, y + S[1], y)
    flag[go & ~known] = LOST
    return out, flag


def drawn(pos, diam, amp, flag=None):
    """Which particles the renderer draws (the contract's `particle` paragraph); s and w in float32 as the kernel forms them."""
    x, y = np.asarray(pos[0], np.float64), np.asarray(pos[1], np.float64)
    d, a = np.asarray(diam).astype(np.float32), np.asarray(amp).astype(np.float32)
    with np.errstate(all="ignore"):
        s = np.float32(0.5) * d
        w = np.float32(1.0) / (s * s)
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(d) & np.isfinite(a) & (d > 0) & (a >= 0) & np.isfinite(w)
        ok &= (np.abs(x) < 2.0 ** 30) & (np.abs(y) < 2.0 ** 30)
    if flag is not None:
        ok &= np.asarray(flag) == 0
    return ok


def render(pos, diam, amp, H, W, radius=4, flag=None):
    """One image: pos [2,N], diam [N], amp [N] -> (V, A, n), float64 [H,W] each (n as float64 counts)."""
    V, A, n = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    ok = drawn(pos, diam, amp, flag)
    xs, ys = np.asarray(pos[0], np.float64), np.asarray(pos[1], np.float64)
    ds, as_ = np.asarray(diam, np.float64), np.asarray(amp, np.float64)
    R = radius
    for p in np.flatnonzero(ok):
        x, y, d, a = xs[p], ys[p], ds[p], as_[p]
        ix, iy = int(np.floor(x)), int(np.floor(y))
        xa, xb = max(ix - R, 0), min(ix + R + 2, W)
        ya, yb = max(iy - R, 0), min(iy + R + 2, H)
        if xa >= xb or ya >= yb:
            continue
        dx = np.arange(xa, xb)[None, :] - x
        dy = np.arange(ya, yb)[:, None] - y
        s = 0.5 * d
        V[ya:yb, xa:xb] += a * np.exp(-(dx * dx + dy * dy) * (1.0 / (s * s)))
        A[ya:yb, xa:xb] += a
        n[ya:yb, xa:xb] += 1.0
    return V, A, n


def tolerance(V, A, n):
    return 2.0 ** -21 * A + n * 2.0 ** -24 * V


def check_image(image, V, A, n, what=""):
    """image == trunc(min(V, 255)), except where an integer k in 1..255 lies within the tolerance of V: there k-1 and k both pass."""
    image = np.asarray(image).astype(np.int64)
    want = np.floor(np.minimum(V, 255.0)).astype(np.int64)
    k = np.rint(V)
    edge = (k >= 1) & (k <= 255) & (np.abs(V - k) <= tolerance(V, A, n))
    ok = (image == want) | (edge & ((image == k - 1) | (image == k)))
    assert image.shape == V.shape and ok.all(), f"{what}: {np.count_nonzero(~ok)} grey levels differ, first at {tuple(np.argwhere(~ok)[0])}: " \
        f"{image[tuple(np.argwhere(~ok)[0])]} against V = {V[tuple(np.argwhere(~ok)[0])]!r}"


def check_render(intensity, image, V, A, n, what=""):
    """The header's bound on the float32 intensity and the grey-level criterion on the image; returns the largest |err| / tol."""
    intensity = np.asarray(intensity)
    assert intensity.dtype == np.float32 and intensity.shape == V.shape, what
    tol = tolerance(V, A, n)
    err = np.abs(intensity.astype(np.float64) - V)
    bad = ~(err <= tol)                                              # a NaN fails
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} pixels off by more than the bound, first at {tuple(np.argwhere(bad)[0])}: " \
        f"err {err[tuple(np.argwhere(bad)[0])]:.3e} against tol {tol[tuple(np.argwhere(bad)[0])]:.3e}"
    check_image(image, V, A, n, what)
    return float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0
