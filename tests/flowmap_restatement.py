"""NumPy float64 restatement of the flow-map contract of include/pivlfn.h (pivlfn_flowmap_advect, pivlfn_flowmap_seed,
pivlfn_flowmap_ftle), operation for operation: NumPy neither fuses nor reorders, so every line below is one correctly rounded IEEE
fp64 operation per element, as on the device, and the two agree bit for bit.  Vectorised over the particles (a step depends on the
particle's own state alone).  Also the test fields.  A helper, not a test."""
import numpy as np

f32, f64 = np.float32, np.float64
OUT, LOST, UNDEFINED = 1, 2, 4


def lattice(H, W, spacing=1):
    """(pos [2,h*w] float64, h, w): the seeds (j*spacing, i*spacing), row-major."""
    h, w = (H - 1) // spacing + 1, (W - 1) // spacing + 1
    i, j = np.mgrid[0:h, 0:w]
    return np.stack([(j * spacing).astype(f64).ravel(), (i * spacing).astype(f64).ravel()]), h, w


def sample(u, v, m, x, y):
    """S_k at the points (x, y) [N] float64 of one field (u, v [H,W] float32, m [H,W] bytes or None) -> (su, sv, flag): the flag a
    sample sets is OUT or LOST, and su, sv mean nothing there."""
    H, W = u.shape
    with np.errstate(invalid="ignore", over="ignore"):
        inside = (x >= 0.0) & (x <= f64(W - 1)) & (y >= 0.0) & (y <= f64(H - 1))          # NaN compares false
        xs, ys = np.where(inside, x, 0.0), np.where(inside, y, 0.0)
        ix = np.minimum(np.floor(xs).astype(np.int64), W - 2)
        iy = np.minimum(np.floor(ys).astype(np.int64), H - 2)
        corners = ((iy, ix), (iy, ix + 1), (iy + 1, ix), (iy + 1, ix + 1))
        cu = [u[c].astype(f64) for c in corners]
        cv = [v[c].astype(f64) for c in corners]
        known = np.ones(x.shape, bool)
        for c in cu + cv:
            known &= np.abs(c) <= 1e9
        if m is not None:
            for c in corners:
                known &= m[c] == 0
        fx, fy = xs - ix.astype(f64), ys - iy.astype(f64)
        gx, gy = 1.0 - fx, 1.0 - fy
        out = []
        for c00, c01, c10, c11 in (cu, cv):
            top = gx * c00 + fx * c01
            bot = gx * c10 + fx * c11
            out.append(top * gy + bot * fy)
    flag = np.where(inside, np.where(known, 0, LOST), OUT).astype(np.uint8)
    return out[0], out[1], flag


def advect(flows, mask, pos, flag, backward=False, iters=8, trace=False):
    """Every particle through flows [B,2,H,W] float32 (mask [B,H,W] or None) in index order.  pos [2,N] float64 and flag [N] uint8 are
    not written; returns (pos, flag) after the last field, and with `trace` also the [B,2,N] states after each field."""
    flows = np.asarray(flows)
    assert flows.dtype == f32 and flows.ndim == 4 and flows.shape[1] == 2
    x, y, f = pos[0].astype(f64).copy(), pos[1].astype(f64).copy(), np.asarray(flag, np.uint8).copy()
    path = np.empty((flows.shape[0], 2, x.size), f64)
    for k in range(flows.shape[0]):
        u, v, m = flows[k, 0], flows[k, 1], None if mask is None else mask[k]
        live = f == 0
        if not backward:
            su, sv, g = sample(u, v, m, x, y)
            with np.errstate(invalid="ignore", over="ignore"):
                nx, ny = x + su, y + sv
        else:
            nx, ny, g = x.copy(), y.copy(), np.zeros_like(f)
            for _ in range(iters):
                su, sv, gi = sample(u, v, m, nx, ny)
                g = np.where(g == 0, gi, g)                     # the first flag a sample sets ends the step
                with np.errstate(invalid="ignore", over="ignore"):
                    nx, ny = x - su, y - sv
        moved = live & (g == 0)
        x, y = np.where(moved, nx, x), np.where(moved, ny, y)
        f = np.where(live, g, f).astype(np.uint8)
        path[k, 0], path[k, 1] = x, y
    return (np.stack([x, y]), f, path) if trace else (np.stack([x, y]), f)


def ftle_stretch(pos, flag, h, w, spacing):
    """(stretch [h,w] float64, oflag [h,w] uint8) of particles seeded on the h x w lattice."""
    X, Y, F = pos[0].reshape(h, w), pos[1].reshape(h, w), np.asarray(flag, np.uint8).reshape(h, w)
    i, j = np.mgrid[0:h, 0:w]
    jl, jr, iu, id_ = np.maximum(j - 1, 0), np.minimum(j + 1, w - 1), np.maximum(i - 1, 0), np.minimum(i + 1, h - 1)
    undefined = (F != 0) | (F[i, jl] != 0) | (F[i, jr] != 0) | (F[iu, j] != 0) | (F[id_, j] != 0)
    if h < 2 or w < 2:
        undefined[:] = True
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dx, dy = ((jr - jl) * spacing).astype(f64), ((id_ - iu) * spacing).astype(f64)
        a, b = (X[i, jr] - X[i, jl]) / dx, (X[id_, j] - X[iu, j]) / dy
        c, d = (Y[i, jr] - Y[i, jl]) / dx, (Y[id_, j] - Y[iu, j]) / dy
        c11, c22, c12 = a * a + c * c, b * b + d * d, a * b + c * d
        g = 0.5 * (c11 - c22)
        lam = 0.5 * (c11 + c22) + np.sqrt(g * g + c12 * c12)
        stretch = np.where(undefined, np.nan, np.sqrt(lam))
    return stretch, (F | np.where(undefined, UNDEFINED, 0)).astype(np.uint8)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the test fields ---------------------------------------------------------------------------------------------------------------
def plane_waves(rng, B, H, W, peak=1.5, min_wavelength=40.0, waves=4):
    """[B,2,H,W] float32: per field and component the sum of `waves` plane waves of random direction, phase and wavelength
    (min_wavelength .. 3 min_wavelength pixels), amplitudes peak / waves each, drifting in phase from field to field: |c| <= peak and
    node-to-node differences of at most 2 pi peak / min_wavelength."""
    y, x = np.mgrid[0:H, 0:W].astype(f64)
    out = np.zeros((B, 2, H, W), f64)
    for c in range(2):
        for _ in range(waves):
            lam, th, ph, om = rng.uniform(min_wavelength, 3 * min_wavelength), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi), rng.uniform(-0.3, 0.3)
            kx, ky = 2 * np.pi / lam * np.cos(th), 2 * np.pi / lam * np.sin(th)
            for k in range(B):
                out[k, c] += peak / waves * np.sin(kx * x + ky * y + ph + om * k)
    return out.astype(f32)


def with_holes(rng, flows, share=0.01):
    """A copy of the flows with NaN, -inf and 1e10 in single components, and a byte mask [B,H,W] with about `share` of nonzero bytes
    (values 1 and 5) plus a small block."""
    flows = flows.copy()
    B, _, H, W = flows.shape
    for n, bad in enumerate((np.nan, -np.inf, 1e10, np.nan, 1e10, -np.inf)):
        flows[rng.integers(0, B), n % 2, rng.integers(0, H), rng.integers(0, W)] = bad
    mask = (rng.random((B, H, W)) < share).astype(np.uint8) * np.where(rng.random((B, H, W)) < 0.5, 1, 5).astype(np.uint8)
    mask[B // 2, H // 2:H // 2 + 2, W // 3:W // 3 + 2] = 1
    return flows, mask


def saddle(steps=6, size=33, a=1.0 / 32):
    """u = a (x - c), v = -a (y - c) about the centre c of a size x size image, `steps` times: stretching along x, compression along
    y.  Every value is a dyadic rational, so the float32 fields, the bilinear samples and the positions are all exact."""
    c = (size - 1) // 2
    y, x = np.mgrid[0:size, 0:size].astype(f64)
    one = np.stack([a * (x - c), -a * (y - c)]).astype(f32)
    return np.repeat(one[None], steps, 0)


def exits(pos0, path, flag, H, W):
    """Which sides OUT particles left through: the set of 'left', 'right', 'top', 'bottom', from the position each froze at."""
    out = (flag & OUT) != 0
    x, y = path[-1, 0][out], path[-1, 1][out]
    sides = {"left": (x < 0).any(), "right": (x > W - 1).any(), "top": (y < 0).any(), "bottom": (y > H - 1).any()}
    return {k for k, v in sides.items() if v}
