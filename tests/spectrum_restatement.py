"""NumPy restatement of pivlfn_spectrum_accumulate's contract (include/pivlfn.h, "temporal spectra"): a sequential loop over the samples
of a segment, vectorised over the basis pairs and the vectors, every operation a correctly rounded float64 operation in the contract's
order -- so csrc/spectrum.hip is compared with it bit for bit.  The basis is an argument: the trigonometry, the window and the
detrending live in pivlfn.spectrum.basis alone.  Plain NumPy, no device."""
import numpy as np

LIMIT = np.float32(1e9)


def valid_vectors(X, N):
    """X [L, >= 2N] float32 -> bool [N]: every one of the vector's 2L values satisfies |x| <= 1e9f (NaN compares false)."""
    with np.errstate(invalid="ignore"):
        fine = np.abs(X[:, :2 * N]) <= LIMIT
    return (fine[:, :N] & fine[:, N:2 * N]).all(axis=0)


def projections(X, first, N, basis):
    """cu, su, cv, sv [K, N] float64: the folds over t = 0..L-1 ascending of a = a + B[t] * (double)x[(first + t) % L], from +0.0."""
    L, K = X.shape[0], basis.shape[0]
    cu, su, cv, sv = (np.zeros((K, N)) for _ in range(4))
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(L):
            row = X[(first + t) % L]
            u, v = row[None, :N].astype(np.float64), row[None, N:2 * N].astype(np.float64)
            c, s = basis[:, 0, t, None], basis[:, 1, t, None]
            cu = cu + c * u
            su = su + s * u
            cv = cv + c * v
            sv = sv + s * v
    return cu, su, cv, sv


def accumulate(X, first, N, basis, acc, count):
    """One call: (acc [K,4,N] float64, count [N] int32) after it, as new arrays.  A vector that does not take part keeps its bits."""
    ok = valid_vectors(X, N)
    cu, su, cv, sv = projections(X, first, N, basis)
    with np.errstate(invalid="ignore", over="ignore"):
        terms = np.stack([cu * cu + su * su, cv * cv + sv * sv, cu * cv + su * sv, cu * sv - su * cv], axis=1)
        new = acc + terms
    out = np.where(ok[None, None, :], new, acc)
    keep = ~ok
    out.view(np.int64)[:, :, keep] = acc.view(np.int64)[:, :, keep]          # NaN payloads and all
    return out, (count + ok.astype(np.int32)).astype(np.int32)


def welch_sums(series, L, hop, basis):
    """series [n, 2, N] float32 (u and v of N vectors over n frames) -> (acc [K,4,N], count [N], segments launched): the segments
    s*hop .. s*hop + L - 1 that fit, one accumulate() each, from zeros."""
    n, _, N = series.shape
    acc, count = np.zeros((basis.shape[0], 4, N)), np.zeros(N, np.int32)
    s = 0
    while s * hop + L <= n:
        X = np.ascontiguousarray(series[s * hop:s * hop + L].reshape(L, 2 * N))
        acc, count = accumulate(X, 0, N, basis, acc, count)
        s += 1
    return acc, count, s


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def planted_line(L, n, k0, d, phi, N=1):
    """[n,2,N] float32: u = 3 + 2 cos(2 pi (k0 + d) t / L + phi), v = 1.5 sin(the same), rounded to float32."""
    arg = 2.0 * np.pi * (k0 + d) * np.arange(n) / L + phi
    u, v = 3.0 + 2.0 * np.cos(arg), 1.5 * np.sin(arg)
    return np.repeat(np.stack([u, v], axis=1)[:, :, None], N, axis=2).astype(np.float32)
