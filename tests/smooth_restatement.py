"""The yardsticks of pivlfn.smooth in numpy float64: the DCT tables of include/pivlfn.h, the dense operator A = W + s D^T D built from
`kron` of 1-D reflecting Laplacians, the weight rule, and the preconditioned conjugate gradients the kernels run (in numpy's own
summation order: what it shares with them is the iteration, not the bits).  For frames of thousands of nodes: the same operator in
scipy.sparse, the contract's iteration once more in the kernels' own order (pcg_tree: table products, the tree sum, the ordered
Laplacian), and the judgements of a solve and of a trajectory as functions of numpy arrays, so that the same code judges the GPU's
result and a deliberately wrong restatement's."""
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


def pcg(w, y, s, tol=1e-8, max_iter=10000, history=None):
    """The kernels' iteration.  Returns (z, iterations, rr, bb).  history: a list that receives rr of the setup and of every iteration."""
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
    if history is not None:
        history.append(rr)
    while it < max_iter and not rr <= tol * tol * bb:
        q = A(d)
        sigma = float((d * q).sum())
        if not sigma > 0:
            break
        alpha = rho / sigma
        x = x + alpha * d
        r = r - alpha * q
        rr = float((r * r).sum())
        if history is not None:
            history.append(rr)
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


# ---- the sparse operator: the dense one beyond a few hundred nodes ------------------------------------------------------------------------
def operator_sparse(w, s):
    """A = diag(w) + s D^T D as a scipy.sparse CSC matrix."""
    import scipy.sparse as sp
    H, W = w.shape
    D = sp.kron(sp.csr_matrix(laplacian_1d(H)), sp.identity(W)) + sp.kron(sp.identity(H), sp.csr_matrix(laplacian_1d(W)))
    return (sp.diags(w.ravel()) + s * (D.T @ D)).tocsc()


def lambda_min_sparse(w, s):
    """The smallest eigenvalue of A, by shift-invert Lanczos about 0 (A is positive definite as soon as one weight is positive)."""
    from scipy.sparse.linalg import eigsh
    return float(eigsh(operator_sparse(w, s), k=1, sigma=0, which="LM", return_eigenvectors=False)[0])


def solve_sparse(w, y, s):
    from scipy.sparse.linalg import spsolve
    return spsolve(operator_sparse(w, s), rhs(w, y).ravel()).reshape(w.shape)


# ---- the contract's iteration in the kernels' own order ------------------------------------------------------------------------------------
def eigenvalues_contract(N):
    """lambda_N[k] = 4 sinpi(k / 2N)^2, as include/pivlfn.h forms it."""
    h = np.sin(np.pi * (np.arange(N) / (2.0 * N)))
    return 4.0 * (h * h)


def gamma_contract(H, W, s):
    """Gamma[k][l] = 1.0 / (1.0 + s*(e*e)), e = lambda_H[k] + lambda_W[l]."""
    e = eigenvalues_contract(H)[:, None] + eigenvalues_contract(W)[None, :]
    return 1.0 / (1.0 + s * (e * e))


def lap_ordered(a):
    """Lap(a) = ((l + r) + u) + d, each term (neighbour - centre) inside the frame and +0.0 outside."""
    l, r, u, d = (np.zeros_like(a) for _ in range(4))
    l[:, 1:] = a[:, :-1] - a[:, 1:]
    r[:, :-1] = a[:, 1:] - a[:, :-1]
    u[1:, :] = a[:-1, :] - a[1:, :]
    d[:-1, :] = a[1:, :] - a[:-1, :]
    return ((l + r) + u) + d


def pcg_tree(w, y, s, iters, tol=1e-30, parts=None):
    """pivlfn_smooth_setup and `iters` iterations of pivlfn_smooth_pcg for one system, step by step as include/pivlfn.h writes them:
    M^-1 by the table products dct2 with Gamma as the last step of the forward transform, every T(.) by pressure_restatement.tree, the
    Laplacian in the contract's order.  Returns (rr of the setup and of every iteration done, x).  It stops early only by the contract's
    rules, so with the default tol it does not.  parts: replacements for "lap", "gamma" (the array) and "sigma" (the tree of d*q), for
    the tests that show what a wrong part does to the trajectory."""
    from pressure_restatement import tree
    parts = parts or {}
    lap_, sigma_ = parts.get("lap", lap_ordered), parts.get("sigma", tree)
    g = parts.get("gamma", gamma_contract(*w.shape, s))
    minv = lambda a: dct2(dct2(a) * g, inverse=True)                       # noqa: E731
    A = lambda a: w * a + s * lap_(lap_(a))                                # noqa: E731
    b = rhs(w, y)
    x = minv(b)
    r = b - A(x)
    z = minv(r)
    rho, rr, bb = tree(r * z), tree(r * r), tree(b * b)
    d, history = None, [float(rr)]
    for _ in range(iters):
        if rr <= (tol * tol) * bb:
            break
        d = z if d is None else z + beta * d                               # noqa: F821
        q = A(d)
        sigma = sigma_(d * q)
        if not sigma > 0:
            break
        alpha = rho / sigma
        x = x + alpha * d
        r = r - alpha * q
        rr = tree(r * r)
        z = minv(r)
        rho_new = tree(r * z)
        beta = rho_new / rho
        rho = rho_new
        history.append(float(rr))
    return history, x


# ---- the cases and the judgements the CPU and the GPU tests share --------------------------------------------------------------------------
SEAM = 1024                       # PR_CHUNK of csrc/cg_shared.h: nodes k*1024 - 1 and k*1024 belong to different workgroups


def seam_case(H, W, seed):
    """solve_case plus holes laid across the seams between the tiles of two workgroups: nodes 1019..1029 (gaps on both sides of the seam
    at 1024, known vectors beyond them) and, where the frame reaches it, five nodes each in the rows above and below node 2048 with
    2045..2050 known (known vectors on both sides of that seam, gaps as their vertical neighbours)."""
    flow, mask = solve_case(H, W, seed)
    flat = mask.reshape(-1)
    if flat.size > 1032:
        flat[1015:1019] = flat[1030:1034] = 0
        flat[1019:1030] = 1
    if flat.size > 2 * SEAM + W + 3 and 2 * SEAM - W - 2 > 1034:
        flat[2045:2051] = 0
        flat[2 * SEAM - W - 2:2 * SEAM - W + 3] = 1
        flat[2 * SEAM + W - 2:2 * SEAM + W + 3] = 1
    return flow, mask


def solve_reference(w, y, s, tol, dense=False):
    """What check_solve compares one system with: b, the operator, its smallest eigenvalue, the direct solution, numpy's iteration count."""
    A = operator(w, s) if dense else operator_sparse(w, s)
    lmin = lambda_min(w, s) if dense else lambda_min_sparse(w, s)
    direct = solve_direct(w, y, s) if dense else solve_sparse(w, y, s)
    return {"A": A, "b": rhs(w, y).ravel(), "lmin": lmin, "direct": direct, "its": pcg(w, y, s, tol)[1], "tol": tol}


def check_solve(z, iterations, ref, what=""):
    """The solve's three assertions on one system's z [H, W] and iteration count:  |r| <= 2 tol |W y| with r = W y - A z formed here,
    |z - z_direct| <= 2 |r| / lambda_min(A), and at most twice numpy's iterations."""
    r = ref["b"] - ref["A"] @ z.ravel()
    nr, nb = np.linalg.norm(r), np.linalg.norm(ref["b"])
    err, bound = np.linalg.norm(z - ref["direct"]), 2.0 * nr / ref["lmin"]
    print(f"{what}: {int(iterations)} iterations (numpy {ref['its']}), |r|/|b| = {nr / nb:.2e}, error {err:.2e} of bound {bound:.2e}")
    assert nr <= 2.0 * ref["tol"] * nb, (what, nr / nb)
    assert err <= bound, (what, err, bound)
    assert int(iterations) <= 2 * ref["its"], (what, int(iterations), ref["its"])


KEEP = 1e-8                       # iteration k is compared while rr_k / rr_0 >= KEEP by the restated iteration
FLOOR = 1e-11                     # the least relative bound on rr
ORDERS = 64.0                     # a third summation order (the matrix instruction's) against the two of the yardstick


def trajectory_reference(w, y, s, iters):
    """The restated iteration (pcg_tree) and numpy's (pcg) over `iters` iterations of one system: two valid fp64 evaluations of the same
    recurrence in different orders.  K is the last compared iteration, Y the yardstick max over k <= K of |rr_pcg - rr_tree| / rr_tree,
    and x_tree, x_pcg are the iterates after K iterations."""
    rr_tree, x_tree = pcg_tree(w, y, s, iters)
    rr_tree = np.array(rr_tree)
    assert len(rr_tree) == iters + 1, "the restated iteration stopped early"
    below = np.nonzero(rr_tree / rr_tree[0] < KEEP)[0]
    K = int(below[0]) - 1 if len(below) else iters
    assert K >= min(3, iters), f"only iterations 0..{K} stay above {KEEP} rr_0"
    if K < iters:
        x_tree = pcg_tree(w, y, s, K)[1]
    rr_pcg = []
    x_pcg = pcg(w, y, s, 1e-30, K, history=rr_pcg)[0]
    rr_pcg = np.array(rr_pcg)
    assert len(rr_pcg) == K + 1
    Y = float((np.abs(rr_pcg - rr_tree[:K + 1]) / rr_tree[:K + 1]).max())
    return {"rr_tree": rr_tree, "rr_pcg": rr_pcg, "K": K, "Y": Y, "x_tree": x_tree, "x_pcg": x_pcg}


def check_trajectory(rr, ref, what=""):
    """rr[k], k = 0..K at least: |rr_k - rr_tree_k| <= max(64 Y, 1e-11) rr_tree_k.  Returns the largest share of the bound."""
    K, bound = ref["K"], max(ORDERS * ref["Y"], FLOOR)
    rr = np.asarray(rr, np.float64)[:K + 1]
    assert len(rr) == K + 1, (what, len(rr), K)
    rel = np.abs(rr - ref["rr_tree"][:K + 1]) / ref["rr_tree"][:K + 1]
    print(f"{what}: compared 0..{K}, Y = {ref['Y']:.2e}, bound {bound:.2e}, worst {rel.max():.2e} at k = {int(rel.argmax())}: "
          f"{rel.max() / bound:.3f} of the bound")
    assert (rel <= bound).all(), (what, rel.tolist(), bound)                # a NaN fails
    return float(rel.max() / bound)


def check_iterate(x, ref, what=""):
    """x after K iterations: max|x - x_tree| <= 64 max|x_pcg - x_tree|."""
    err, unit = float(np.abs(x - ref["x_tree"]).max()), float(np.abs(ref["x_pcg"] - ref["x_tree"]).max())
    print(f"{what}: x after {ref['K']} iterations {err:.2e} from the restated one, numpy's {unit:.2e}: {err / (ORDERS * unit):.3f} of the bound")
    assert err <= ORDERS * unit, (what, err, unit)

