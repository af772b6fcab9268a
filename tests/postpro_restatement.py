"""Vectorised numpy restatement of the reference's src/postpro.py (calc_vorticity :5-24, de_vort :27-50) with every rounding
spelled out, and the sequential float64 accumulation of pivlfn_flow_stats_accumulate -- the arithmetic contract of
include/pivlfn.h.  tests/golden/postpro_cases.npz pins it to the reference bit for bit (tests/test_postpro.py); the GPU tests
compare the kernels with it."""
import numpy as np

f32, f64 = np.float32, np.float64


def taps(calib):
    """(K, -K^T): K = [[1,0,-1],[2,0,-2],[1,0,-1]] / (8.0 calib), each element divided in float64."""
    K = np.array([[1, 0, -1], [2, 0, -2], [1, 0, -1]], dtype=f64) / (8.0 * float(calib))
    return K, -K.T


def conv_same_edge(x, k):
    """scipy.signal.convolve2d(x, k, 'same', boundary='symm') for a 3 x 3 k: out[i,j] = sum over the taps of k in row-major
    order of k[p,q] * xp[i+2-p, j+2-q] (xp = x with the edge repeated), from +0.0, each product rounded before it is added."""
    x = np.asarray(x, dtype=f64)
    h, w = x.shape
    xp = np.pad(x, 1, mode="edge")
    out = np.zeros((h, w), dtype=f64)
    for p in range(3):
        for q in range(3):
            out = out + k[p, q] * xp[2 - p:2 - p + h, 2 - q:2 - q + w]
    return out


def calc_vorticity(flow, calib=1.0):
    """flow [H,W,2] float32 -> (vort, shear, normal) float64."""
    K, Kt = taps(calib)
    dv = conv_same_edge(flow[:, :, 1], K)
    du = conv_same_edge(flow[:, :, 0], Kt)
    return dv - du, dv + du, -(dv + du)


def de_vort(flow, calib=1.0):
    """flow [H,W,2] float32 -> (vort, uy, vx) float64; the sums and the division in float32."""
    u = np.pad(np.asarray(flow[:, :, 0], dtype=f32), 1, mode="edge")
    v = np.pad(np.asarray(flow[:, :, 1], dtype=f32), 1, mode="edge")
    d = f32(8 * float(calib))
    two = f32(2)
    vx = (((v[2:, 2:] + two * v[1:-1, 2:]) + v[:-2, 2:]) - ((v[2:, :-2] + two * v[1:-1, :-2]) + v[:-2, :-2])) / d
    uy = (((u[:-2, :-2] + two * u[:-2, 1:-1]) + u[:-2, 2:]) - ((u[2:, :-2] + two * u[2:, 1:-1]) + u[2:, 2:])) / d
    assert vx.dtype == f32 and uy.dtype == f32
    return vx.astype(f64) - uy.astype(f64), uy.astype(f64), vx.astype(f64)


FIELDS = {"calc_vorticity": calc_vorticity, "de_vort": de_vort}


def fields(flows_b2hw, calib, kind):
    """[B,2,H,W] float32 -> [B,3,H,W] float64, the planes of pivlfn_flow_fields."""
    fn = FIELDS[kind]
    return np.stack([np.stack(fn(np.ascontiguousarray(f.transpose(1, 2, 0)), calib)) for f in np.asarray(flows_b2hw)])


def accumulate(acc, flows_b2hw, calib):
    """acc [7,H,W] float64 += u, v, u*u, v*v, u*v, w, w*w of each frame, frame by frame (w = calc_vorticity's vort)."""
    for f in np.asarray(flows_b2hw):
        u, v = f[0].astype(f64), f[1].astype(f64)
        w = calc_vorticity(np.ascontiguousarray(f.transpose(1, 2, 0)), calib)[0]
        acc[0] += u
        acc[1] += v
        acc[2] += u * u
        acc[3] += v * v
        acc[4] += u * v
        acc[5] += w
        acc[6] += w * w
    return acc


def same_bits(a, b):
    """Bit-for-bit equality of two float arrays of one dtype (signs of zero included), NaN compared by position only."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    it = np.uint64 if a.dtype == f64 else np.uint32
    return np.array_equal(a[~na].view(it), b[~nb].view(it))
