"""NumPy restatement of the stereo 2D3C arithmetic contract (include/pivlfn.h, pivlfn_stereo_2d3c) with every cast explicit,
so it does not depend on the promotion rules of the NumPy that runs it.  Shared by tests/test_stereo.py and
tests/test_gpu_stereo.py."""
import numpy as np

f32, f64 = np.float32, np.float64


def _poly(A, x, y):
    a, b, c, d, e, f = (f32(v) for v in A)
    return ((((a * x + b * y) + c) + d * (x * x)) + e * (y * y)) + (f * x) * y


def map_camera(flow_hw2, A24, scale=None):
    """stage 1: nl_trans (+ calib * fps) of one camera, float32.  A24: the 24 coefficients already rounded to float32."""
    x = np.asarray(flow_hw2[..., 0], dtype=f32)
    y = np.asarray(flow_hw2[..., 1], dtype=f32)
    with np.errstate(all="ignore"):
        xp = (_poly(A24[0:6], x, y) / _poly(A24[6:12], x, y)).astype(f32)
        yp = (_poly(A24[12:18], x, y) / _poly(A24[18:24], x, y)).astype(f32)
        if scale is not None:
            c, fps = f32(scale[0]), f32(scale[1])
            xp = ((xp * c) * fps).astype(f32)
            yp = ((yp * c) * fps).astype(f32)
    return xp, yp


def restate(left_hw2, right_hw2, coeff48_f32, tans, scale=None):
    """[..., h, w, 2] x2 -> [..., h, w, 3] float32.  tans = float64 (tan theta_L, tan theta_R, tan beta_L, tan beta_R);
    scale = (calib ratio, fps) or None."""
    A = np.asarray(coeff48_f32, dtype=f32)
    uL, vL = map_camera(left_hw2, A[:24], scale)
    uR, vR = map_camera(right_hw2, A[24:], scale)
    tL, tR, bL, bR = (f64(t) for t in tans)
    dT = f64(tL - tR)
    dB = f64(bR - bL)
    with np.errstate(all="ignore"):
        du = (uR - uL).astype(f32)
        vm = ((vL + vR) / f32(2)).astype(f32)
        U = (uR.astype(f64) * tL - uL.astype(f64) * tR) / dT
        V = vm.astype(f64) + ((du.astype(f64) * dB) / dT) / f64(2)
        W = du.astype(f64) / dT
        return np.stack([U.astype(f32), V.astype(f32), W.astype(f32)], axis=-1)


def same_bits(a, b):
    """Bit-for-bit equality of two float32 arrays, NaN compared by position only (any NaN payload)."""
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def load_case(g, tag):
    """(left, right, coeff dict, theta, alpha, fps, calib) of one case of tests/golden/stereo_cases.npz."""
    c = g[f"{tag}_coeff"].tolist()
    coeff = {"Left": c[:24], "Right": c[24:]}
    cc = float(g[f"{tag}_coeff_calib"])
    if not np.isnan(cc):
        coeff["calib"] = cc
    calib = float(g[f"{tag}_calib"])
    return (g[f"{tag}_left"], g[f"{tag}_right"], coeff, g[f"{tag}_theta"].tolist(), g[f"{tag}_alpha"].tolist(),
            int(g[f"{tag}_fps"]), None if np.isnan(calib) else calib)
