"""The yardsticks of pivlfn.smooth in numpy float64: the DCT tables of include/pivlfn.h, the dense operator A = W + s D^T D built from
`kron` of 1-D reflecting Laplacians, the weight rule, and the preconditioned conjugate gradients the kernels run (in numpy's own
summation order: what it shares with them is the iteration, not the bits)."""
import numpy as np


def dct_table(N):
    """C_N[k][n] = a_k cos(pi m / 2N), m = ((2n+1) k) mod 4N reduced in integers and folded into the first octant."""
    k, n = np.meshgrid(np.arange(N, dtype=np.int64), np.arange(N, dtype=np.int64), indexing="ij")
    m = ((2 * n + 1) * k) % (4 * N)
    m = np.where(m > 2 * N, 4 * N - m, m)
    neg = m > N
    m = np.where(neg, 2 * N - m, m)
    c = np.where(2 * m <= N, np.cos(np.pi * (m / (2.0 * N))), np.sin(np.pi * ((N - m) / (2.0 * N))))
    a = np.where(k == 0, np.sqrt(1.0 / N), np.sqrt(2.0 / N))
    return np.where(neg, -1.0, 1.0) * a * c


def dct2(x, inverse=False):
    """[..., H, W]: C_H x C_W^T, or C_H^T x C_W."""
    ch, cw = dct_table(x.shape[-2]), dct_table(x.shape[-1])
    return ch.T @ x @ cw if inverse else ch @ x @ cw.T


def dct_bound(x, inverse=False):
    """The elementwise forward error bound of the two chained products, (H + W + 16) 2^-52 (|C_H| |x| |C_W|^T) (transposed tables for
    the inverse): the standard bound plus a few ulp for the table entries."""
    H, W = x.shape[-2], x.shape[-1]
    ch, cw = np.abs(dct_table(H)), np.abs(dct_table(W))
    mag = ch.T @ np.abs(x) @ cw if inverse else ch @ np.abs(x) @ cw.T
    return (H + W + 16) * 2.0 ** -52 * mag


def eigenvalues(N):
    """lambda_k = 2 - 2 cos(pi k / N) of the negated 1-D reflecting Laplacian."""
    return 2.0 - 2.0 * np.cos(np.pi * np.arange(N) / N)


def gamma(H, W, s):
    e = eigenvalues(H)[:, None] + eigenvalues(W)[None, :]
    return 1.0 / (1.0 + s * e * e)


def laplacian_1d(N):
    """Rows [-1 1], [1 -2 1], ..., [1 -1]: reflecting boundaries.  Symmetric."""
    L = np.zeros((N, N))
    for i in range(N):
        if i > 0:
            L[i, i - 1] = 1.0
            L[i, i] -= 1.0
        if i + 1 < N:
            L[i, i + 1] = 1.0
            L[i, i] -= 1.0
    return L


def laplacian_2d(H, W):
    """D on row-major [H, W] fields."""
    return np.kron(laplacian_1d(H), np.eye(W)) + np.kron(np.eye(H), laplacian_1d(W))


def weights_of(flow, weights=None, mask=None):
    """[H, W] float64 weights of one frame [2, H, W]: 0 where masked, where either component is NaN or beyond 1e9, or where the weight
    is not positive and finite."""
    with np.errstate(invalid="ignore"):
        known = (np.abs(flow[0]) <= 1e9) & (np.abs(flow[1]) <= 1e9)
        w = np.ones(flow.shape[1:], dtype=np.float64) if weights is None else weights.astype(np.float64)
        ok = known & np.isfinite(w) & (w > 0)
    if mask is not None:
        ok &= mask == 0
    return np.where(ok, w, 0.0)


def operator(w, s):
    """The dense A = diag(w) + s D^T D of one frame."""
    D = laplacian_2d(*w.shape)
    return np.diag(w.ravel()) + s * (D.T @ D)


def rhs(w, y):
    """W y with the gaps' values never touched."""
    return np.where(w > 0, w * np.where(w > 0, y, 0.0), 0.0)


def solve_direct(w, y, s):
    return np.linalg.solve(operator(w, s), rhs(w, y).ravel()).reshape(w.shape)


def lambda_min(w, s):
    return float(np.linalg.eigvalsh(operator(w, s))[0])


def lap(a):
    """D a by the stencil: the sum over the neighbours that exist of (neighbour - centre)."""
    out = np.zeros_like(a)
    out[:, 1:] += a[:, :-1] - a[:, 1:]
    out[:, :-1] += a[:, 1:] - a[:, :-1]
    out[1:, :] += a[:-1, :] - a[1:, :]
    out[:-1, :] += a[1:, :] - a[:-1, :]
    return out


def pcg(w, y, s, tol=1e-8, max_iter=10000):
    """The kernels' iteration.  Returns (z, iterations, rr, bb)."""
    from scipy.fft import dctn, idctn
    g = gamma(*w.shape, s)
    minv = lambda r: idctn(g * dctn(r, norm="ortho"), norm="ortho")      # noqa: E731
    A = lambda a: w * a + s * lap(lap(a))                                  # noqa: E731
    b = rhs(w, y)
    x = minv(b)
    r = b - A(x)
    z = minv(r)
    rho, rr, bb = float((r * z).sum()), float((r * r).sum()), float((b * b).sum())
    d, it = z.copy(), 0
    while it < max_iter and not rr <= tol * tol * bb:
        q = A(d)
        sigma = float((d * q).sum())
        if not sigma > 0:
            break
        alpha = rho / sigma
        x = x + alpha * d
        r = r - alpha * q
        rr = float((r * r).sum())
        z = minv(r)
        rho_new = float((r * z).sum())
        d = z + (rho_new / rho) * d
        rho = rho_new
        it += 1
    return x, it, rr, bb


def response(s, wavelength, periods=6):
    """The share of its amplitude the gap-free smoother M^-1 = IDCT Gamma DCT leaves of a cosine of `wavelength` pixels (an integer)
    along a row of `periods` whole waves, measured by applying it."""
    N = periods * int(wavelength)
    y = np.cos(2.0 * np.pi * (np.arange(N) + 0.5) / wavelength)[None, :]
    z = dct2(gamma(1, N, s) * dct2(y), inverse=True)
    return float((z * y).sum() / (y * y).sum())


def solve_case(H, W, seed):
    """The solve tests' frame: a sine plus a cosine plus 0.3 noise, and its gaps: 10 % random weight-0 vectors plus a 5 x 5 hole."""
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    flow = np.stack([np.sin(2 * np.pi * ii / 11.0) + np.cos(2 * np.pi * jj / 7.0) + 0.3 * rng.standard_normal((H, W)),
                     np.cos(2 * np.pi * ii / 9.0) - np.sin(2 * np.pi * jj / 13.0) + 0.3 * rng.standard_normal((H, W))]).astype(np.float32)
    mask = (rng.random((H, W)) < 0.10).astype(np.uint8)
    mask[H // 3:H // 3 + 5, W // 2:W // 2 + 5] = 1
    return flow, mask

