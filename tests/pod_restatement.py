"""NumPy float64 restatement of the snapshot POD contract (include/pivlfn.h "snapshot POD", pivlfn/pod.py), written from the
contract's words and not from the code, plus the planted case the POD tests share.  No GPU, no torch."""
import numpy as np

DEGENERATE = 1e-12


def gram(X):
    """G[i][j] = sum_p (double)X[i][p] * (double)X[j][p]: a float64 product of two float32 values is exact, so only the order of the
    additions separates this from the kernel."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    return X64 @ X64.T


def gram_bound(G_ref, P):
    """|G - G_ref| <= 2 * P * 2^-53 * sqrt(G_ref[i][i] * G_ref[j][j]): each side's summation error is below P * 2^-53 * sum|ab|, and
    Cauchy-Schwarz bounds sum|ab| by the geometric mean of the two diagonal entries."""
    d = np.sqrt(np.diag(G_ref))
    return 2.0 * P * 2.0 ** -53 * np.outer(d, d)


def project(X, Wt):
    """out[k][p]: acc = +0.0; for i ascending: acc = acc + Wt[i][k] * (double)X[i][p], product and sum each rounded on its own."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    Wt = np.asarray(Wt, dtype=np.float64)
    out = np.zeros((Wt.shape[1], X64.shape[1]))
    for i in range(X64.shape[0]):
        out = out + Wt[i][:, None] * X64[i][None, :]          # elementwise: one rounding for the product, one for the sum
    return out


def solve(G, K):
    """(eigenvalues [n] descending of C = J G J, V [n,K] under the sign rule, Wt [n,K+1] = [J V diag(lambda)^-1/2 | 1]).  Raises
    ValueError for a mode whose eigenvalue is not above 1e-12 of the largest -- nor of trace(G), the scale of the centring's own
    rounding, which is all that J G J of n identical snapshots holds."""
    G = np.asarray(G, dtype=np.float64)
    n = G.shape[0]
    J = np.eye(n) - np.ones((n, n)) / n
    lam, V = np.linalg.eigh(J @ G @ J)
    order = np.argsort(-lam, kind="stable")
    lam, V = lam[order], V[:, order][:, :K].copy()
    for k in range(K):
        if not lam[k] > DEGENERATE * max(lam[0], np.trace(G)):
            raise ValueError(f"mode {k + 1} is undefined")
        col = V[:, k]
        big = np.flatnonzero(np.abs(col) == np.abs(col).max())[0]        # the first entry of largest magnitude
        if col[big] < 0:
            V[:, k] = -col
    Wt = np.concatenate([J @ V / np.sqrt(lam[:K])[None, :], np.ones((n, 1))], axis=1)
    return lam, V, Wt


def decompose(X, K, shape):
    """The whole chain on the host: dict with the fields of PODResult for snapshots X [n,P] viewed as [2,ch,cw] = shape."""
    G = gram(X)
    lam, V, Wt = solve(G, K)
    out = project(X, Wt)
    n = G.shape[0]
    return dict(modes=out[:K].reshape((K,) + tuple(shape)), mean=(out[K] / n).reshape(shape), coeff=V * np.sqrt(lam[:K]),
                energy=lam[:K] / n, fraction=lam[:K] / lam.sum(), eigenvalues=lam, gram=G)


def sign_rule(rows):
    """Rows (modes or coefficient columns, flattened) with the entry of largest magnitude of each made positive."""
    rows = np.array(rows, dtype=np.float64)
    flat = rows.reshape(rows.shape[0], -1)
    for r in flat:
        big = np.flatnonzero(np.abs(r) == np.abs(r).max())[0]
        if r[big] < 0:
            r *= -1.0
    return rows


def svd_reference(X, K):
    """numpy.linalg.svd of the centred float64 data: (eigenvalues s^2 [min(n,P)], modes [K,P] rows of Vt, coefficients [n,K] = U s)."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    Xc = X64 - X64.mean(axis=0, keepdims=True)
    U, s, Vt = np.linalg.svd(Xc, full_matrices=False)
    return s * s, Vt[:K], U[:, :K] * s[:K]


PLANTED_N, PLANTED_H, PLANTED_W = 37, 9, 13
PLANTED_AMPS = (3.0, 1.5, 0.6)


def planted_flows():
    """[37,2,9,13] float32: mean field + three orthogonal structures of unit vector length at every grid point (so each has norm^2
    = 117), amplitudes 3, 1.5 and 0.6, modulated by three orthogonal zero-mean sinusoids in time (2, 3 and 5 periods over the 37
    snapshots) + Gaussian noise of sigma = 0.01 from default_rng(7).  Eigenvalue ratios (1.5/3)^2 and (0.6/3)^2 by construction."""
    n, H, W = PLANTED_N, PLANTED_H, PLANTED_W
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ph = [2 * np.pi * x / W, 2 * np.pi * y / H, 2 * np.pi * (2 * x / W + y / H)]
    phi = [np.stack([np.sin(ph[0]), np.cos(ph[0])]), np.stack([np.cos(ph[1]), np.sin(ph[1])]), np.stack([np.sin(ph[2]), np.cos(ph[2])])]
    t = np.arange(n)
    c = [np.cos(2 * np.pi * 2 * t / n), np.sin(2 * np.pi * 3 * t / n), np.cos(2 * np.pi * 5 * t / n)]
    mean = np.stack([np.full((H, W), 0.8), np.full((H, W), -0.3)])
    flows = mean[None] + sum(a * ck[:, None, None, None] * pk[None] for a, ck, pk in zip(PLANTED_AMPS, c, phi))
    flows = flows + np.random.default_rng(7).normal(0.0, 0.01, size=flows.shape)
    return flows.astype(np.float32)
