"""NumPy float64 restatement of the pressure contract of include/pivlfn.h (pivlfn_pressure_gradient, _setup, _cg, _read), operation for
operation: every NumPy elementwise operation is one correctly rounded fp64 operation, and they are written in the contract's order.
Also the decaying Taylor-Green vortex, an exact solution of the momentum equation in lattice units whose unsteady, convective and
viscous terms are all non-zero, and small helpers the tests share (random cases, connected components, a dense least-squares reference)."""
import math

import numpy as np

f64 = np.float64
RUNNING, CONVERGED, BREAKDOWN = 1, 2, 3
OK, INVALID, ISOLATED = 0, 1, 2


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def tree(leaves):
    """T: the root of t[i] = t[2i] + t[2i+1] over the leaves in row-major order, padded with +0.0 to the next power of two."""
    t = np.asarray(leaves, f64).reshape(-1)
    P = 1
    while P < t.size:
        P *= 2
    t = np.concatenate([t, np.zeros(P - t.size)])
    while t.size > 1:
        t = t[0::2] + t[1::2]
    return f64(t[0])


# ---- pivlfn_pressure_gradient -----------------------------------------------------------------------------------------------------------
def gradient(flows, s, nu):
    """flows [B,2,h,w] float32 -> (g [B-2,2,h,w] float64, valid [B-2,h,w] uint8)."""
    flows = np.asarray(flows)
    assert flows.dtype == np.float32 and flows.ndim == 4 and flows.shape[0] >= 3
    B, _, h, w = flows.shape
    F = B - 2
    g, valid = np.zeros((F, 2, h, w)), np.zeros((F, h, w), np.uint8)
    if h < 3 or w < 3:
        return g, valid
    s, nu = f64(s), f64(nu)
    with np.errstate(invalid="ignore", over="ignore"):
        known = (np.abs(flows) <= np.float32(1e9)).all(1)                       # [B,h,w]; NaN compares false
    for f in range(F):
        prev, cur, nxt = (flows[f + k].astype(f64) for k in range(3))
        k1 = known[f + 1]
        ok = k1[1:-1, 1:-1] & k1[1:-1, :-2] & k1[1:-1, 2:] & k1[:-2, 1:-1] & k1[2:, 1:-1] & known[f][1:-1, 1:-1] & known[f + 2][1:-1, 1:-1]
        uc, vc = cur[0, 1:-1, 1:-1], cur[1, 1:-1, 1:-1]
        with np.errstate(all="ignore"):                                          # the values of invalid nodes are formed here and dropped
            for a in range(2):
                c = cur[a]
                ac, al, ar, au, ad = c[1:-1, 1:-1], c[1:-1, :-2], c[1:-1, 2:], c[:-2, 1:-1], c[2:, 1:-1]
                at = (nxt[a, 1:-1, 1:-1] - prev[a, 1:-1, 1:-1]) * 0.5
                ax = (ar - al) / (2.0 * s)
                ay = (ad - au) / (2.0 * s)
                lap = ((((al + ar) + au) + ad) - 4.0 * ac) / (s * s)
                ga = (-(at + (uc * ax + vc * ay))) + nu * lap
                g[f, a, 1:-1, 1:-1] = np.where(ok, ga, 0.0)
        valid[f, 1:-1, 1:-1] = ok
    return g, valid


# ---- pivlfn_pressure_setup --------------------------------------------------------------------------------------------------------------
def _shift(a, dj, di):
    """a[j+dj, i+di] with +0.0 (False) outside."""
    out = np.zeros_like(a)
    h, w = a.shape
    src = a[max(dj, 0):h + min(dj, 0), max(di, 0):w + min(di, 0)]
    out[max(-dj, 0):h + min(-dj, 0), max(-di, 0):w + min(-di, 0)] = src
    return out


class Frame:
    """The state of one frame: adj (bits 0..3 = edge to the left / right / upper / lower neighbour active, bit 4 = valid), deg, b, x, r,
    z, d, rho, rr, bb, iterations, state."""

    def __init__(self, g, valid, s):
        g, v, s = np.asarray(g, f64), np.asarray(valid) != 0, f64(s)
        self.h, self.w = v.shape
        self.eL, self.eR = v & _shift(v, 0, -1), v & _shift(v, 0, 1)
        self.eU, self.eD = v & _shift(v, -1, 0), v & _shift(v, 1, 0)
        self.valid = v
        self.adj = (self.eL * 1 + self.eR * 2 + self.eU * 4 + self.eD * 8 + v * 16).astype(np.uint8)
        self.deg = (self.eL * 1 + self.eR * 1 + self.eU * 1 + self.eD * 1).astype(f64)
        gx, gy = g
        L = np.where(self.eL, (0.5 * (_shift(gx, 0, -1) + gx)) * s, 0.0)
        R = np.where(self.eR, -((0.5 * (gx + _shift(gx, 0, 1))) * s), 0.0)
        U = np.where(self.eU, (0.5 * (_shift(gy, -1, 0) + gy)) * s, 0.0)
        D = np.where(self.eD, -((0.5 * (gy + _shift(gy, 1, 0))) * s), 0.0)
        self.b = ((L + R) + U) + D
        self.x = np.zeros_like(self.b)
        self.r = self.b.copy()
        self.z = self._precondition(self.r)
        self.d = self.z.copy()
        self.rho, self.bb, self.rr = tree(self.r * self.z), tree(self.b * self.b), tree(self.r * self.r)
        self.iterations, self.state = 0, RUNNING

    def _precondition(self, r):
        with np.errstate(all="ignore"):
            return np.where(self.deg > 0, r / np.where(self.deg > 0, self.deg, 1.0), 0.0)

    def apply(self, d):
        """q = A d."""
        dl, dr = np.where(self.eL, _shift(d, 0, -1), 0.0), np.where(self.eR, _shift(d, 0, 1), 0.0)
        du, dd = np.where(self.eU, _shift(d, -1, 0), 0.0), np.where(self.eD, _shift(d, 1, 0), 0.0)
        return self.deg * d - (((dl + dr) + du) + dd)

    # ---- pivlfn_pressure_cg: one iteration ------------------------------------------------------------------------------------------
    def iterate(self, tol):
        tol = f64(tol)
        if self.state != RUNNING:
            return
        if self.bb > 0 and self.rr <= (tol * tol) * self.bb:
            self.state = CONVERGED
            return
        with np.errstate(all="ignore"):
            q = self.apply(self.d)
            sigma = tree(self.d * q)
            if not sigma > 0:
                self.state = BREAKDOWN
                return
            alpha = self.rho / sigma
            self.x = self.x + alpha * self.d
            self.r = self.r - alpha * q
            self.z = self._precondition(self.r)
            rho_new = tree(self.r * self.z)
            self.rr = tree(self.r * self.r)
            beta = rho_new / self.rho
            self.d = self.z + beta * self.d
            self.rho = rho_new
        self.iterations += 1

    def run(self, tol, iters):
        for _ in range(iters):
            if self.state != RUNNING:
                break
            self.iterate(tol)
        return self

    # ---- pivlfn_pressure_read ---------------------------------------------------------------------------------------------------------
    def read(self):
        """(p, flag, status): p is x where deg > 0 and NaN elsewhere; status = [state, iterations, rr, bb]."""
        p = np.where(self.deg > 0, self.x, np.nan)
        flag = np.where(~self.valid, INVALID, np.where(self.deg > 0, OK, ISOLATED)).astype(np.uint8)
        return p, flag, np.array([self.state, self.iterations, self.rr, self.bb], f64)


def solve(g, valid, s, tol, iters):
    """All frames: (p [F,h,w], flag [F,h,w], status [F,4], the Frame objects)."""
    frames = [Frame(g[f], valid[f], s).run(tol, iters) for f in range(len(g))]
    out = [fr.read() for fr in frames]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]), frames


# ---- the decaying Taylor-Green vortex -----------------------------------------------------------------------------------------------------
def taylor_green(B, h, w, lam, A=2.0, nu=0.5, s=1.0, n0=0):
    """Flows [B,2,h,w] float32 at the frames n0 .. n0+B-1 on a lattice of spacing s px, wavelength `lam` px:
    u = A sin kx cos ky F, v = -A cos kx sin ky F, F = exp(-2 nu k^2 n);  and p* [B,h,w] float64 = (A^2/4)(cos 2kx + cos 2ky) F^2."""
    k = 2.0 * math.pi / lam
    y, x = np.meshgrid(np.arange(h) * f64(s), np.arange(w) * f64(s), indexing="ij")
    flows, p = np.empty((B, 2, h, w), np.float32), np.empty((B, h, w))
    for n in range(B):
        F = math.exp(-2.0 * nu * k * k * (n0 + n))
        flows[n, 0] = A * np.sin(k * x) * np.cos(k * y) * F
        flows[n, 1] = -A * np.cos(k * x) * np.sin(k * y) * F
        p[n] = (A * A / 4.0) * (np.cos(2 * k * x) + np.cos(2 * k * y)) * F * F
    return flows, p


# ---- helpers of the tests -----------------------------------------------------------------------------------------------------------------
def random_flows(rng, B, h, w, sigma=2.0):
    """Smooth-ish random flows: white noise plus a shear, float32."""
    flows = rng.normal(0, sigma, (B, 2, h, w))
    flows[:, 0] += np.linspace(-1, 1, h)[None, :, None] * 3.0
    return flows.astype(np.float32)


def components(valid_edges_frame):
    """Labels [h,w] (int, -1 where deg = 0) of the connected components of a Frame's active edges."""
    fr = valid_edges_frame
    h, w = fr.h, fr.w
    lab = -np.ones((h, w), int)
    n = 0
    for j in range(h):
        for i in range(w):
            if fr.deg[j, i] > 0 and lab[j, i] < 0:
                stack, lab[j, i] = [(j, i)], n
                while stack:
                    a, b = stack.pop()
                    for bit, da, db in ((1, 0, -1), (2, 0, 1), (4, -1, 0), (8, 1, 0)):
                        if fr.adj[a, b] & bit and lab[a + da, b + db] < 0:
                            lab[a + da, b + db] = n
                            stack.append((a + da, b + db))
                n += 1
    return lab, n


def edge_system(fr, g, s):
    """The dense edge equations of a Frame: M [edges, nodes] and rhs [edges] with  p(b) - p(a) = e(a -> b)  for every active edge to the
    right and down; the nodes are those with deg > 0, numbered row-major.  Returns (M, rhs, index [h,w])."""
    idx = -np.ones((fr.h, fr.w), int)
    idx[fr.deg > 0] = np.arange(int((fr.deg > 0).sum()))
    rows, rhs = [], []
    gx, gy = np.asarray(g, f64)
    for j in range(fr.h):
        for i in range(fr.w):
            if fr.eR[j, i]:
                rows.append((idx[j, i], idx[j, i + 1]))
                rhs.append((0.5 * (gx[j, i] + gx[j, i + 1])) * s)
            if fr.eD[j, i]:
                rows.append((idx[j, i], idx[j + 1, i]))
                rhs.append((0.5 * (gy[j, i] + gy[j + 1, i])) * s)
    M = np.zeros((len(rows), int((fr.deg > 0).sum())))
    for e, (a, b) in enumerate(rows):
        M[e, a], M[e, b] = -1.0, 1.0
    return M, np.array(rhs), idx
