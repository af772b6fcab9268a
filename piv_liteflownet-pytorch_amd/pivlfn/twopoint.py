"""Two-point statistics of a flow sequence on the device: the spatial correlation functions R_uu(r), R_vv(r), R_uv(r) and the second-
and third-order structure functions for separations along x and along y, and what is read off them -- integral length scales, Taylor
microscales, the noise share of the variance and one-dimensional spectra.

The sums run on csrc/twopoint.hip through the C ABI (`pivlfn_twopoint_accumulate`; the arithmetic contract is written out in
include/pivlfn.h); everything derived from them is host work in float64 on a few thousand numbers:

    tp = TwoPointStats(H, W, max_sep=64)
    for flows in chunks: tp.update(flows, mask)               # enqueued on the current stream, no host synchronisation
    res = tp.result()
    res.integral_scale("uu", "x")                             # IntegralScale(scale, truncated, crossing), in pixels
    res.taylor_fit("uu", "x")                                 # TaylorFit(microscale, noise, c, ell)
    k, E = res.spectrum("uu", "x")
    tp.save("twopoint.npz")

Per row y, direction and separation index r the device keeps fifteen sums over the pairs (a, b) of the row and over the frames (TERMS):
the count, the sums of the two components at both ends, their squares, the four cross products and the two third-order increments.
Every sum is formed in an order the contract fixes, so a sequence gives the same bits however it is cut into update() calls.  GPU only,
like the rest of the package: there is no CPU path.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from . import _accum, _args, _lib

TERMS = ("n", "ua", "va", "ub", "vb", "uaua", "vava", "ubub", "vbvb", "uaub", "vavb", "uavb", "vaub", "lll", "ltt")    # acc[d, r, :, y]
T = {name: i for i, name in enumerate(TERMS)}
AXES = {"x": 0, "y": 1, 0: 0, 1: 1}
# which -> (the product, the sum at a, the sum at b, the square at a, the square at b): x is the component at a, y the one at b
WHICH = {"uu": ("uaub", "ua", "ub", "uaua", "ubub"), "vv": ("vavb", "va", "vb", "vava", "vbvb"),
         "uv": ("uavb", "ua", "vb", "uaua", "vbvb"), "vu": ("vaub", "va", "ub", "vava", "ubub")}


def check_params(max_sep, step) -> None:
    """The parameter checks of TwoPointStats (ValueError), usable before any tensor exists."""
    _args.check_int("TwoPointStats", "max_sep", max_sep, 0, 255, ", the largest separation index")
    _args.check_int("TwoPointStats", "step", step, 1, 16, ", the pixels between two separations")


def _axis(axis) -> int:
    if axis not in AXES:
        raise ValueError(f"axis={axis!r} must be 'x' (0) or 'y' (1)")
    return AXES[axis]


def _which(which):
    if which not in WHICH:
        raise ValueError(f"which={which!r} must be one of {', '.join(WHICH)}")
    return tuple(T[k] for k in WHICH[which])


class Correlation(NamedTuple):
    """n, cov, var_a, var_b, rho: [R+1, H] per row, or [R+1] pooled."""
    n: np.ndarray
    cov: np.ndarray
    var_a: np.ndarray
    var_b: np.ndarray
    rho: np.ndarray


class IntegralScale(NamedTuple):
    scale: float                  # pixels
    truncated: bool               # rho never crossed zero: the integral stops at the last separation with pairs
    crossing: Optional[float]     # the interpolated zero crossing in pixels, None where truncated


class TaylorFit(NamedTuple):
    microscale: float             # lambda = sqrt(c) * ell, pixels
    noise: float                  # 1 - c: the share of the variance that is uncorrelated from vector to vector
    c: float
    ell: float


def _rho(cov, var_a, var_b, n):
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = (n >= 2) & (var_a > 0) & (var_b > 0)
        return np.where(ok, cov / np.sqrt(np.where(ok, var_a * var_b, 1.0)), np.nan)


class TwoPointResult:
    """Everything derived from the accumulators acc [2, R+1, 15, H] (float64, TERMS order), on the host in float64.

    With S_t the sum of term t over the pairs of row y at separation r*step (direction and r fixed) and n = S_n:
        cov_xy = S_xy/n - (S_xa/n)*(S_yb/n)     x the component taken at the base point a, y the one at the partner b
        var_a  = S_xx(a)/n - (S_xa/n)^2,  var_b = S_yy(b)/n - (S_yb/n)^2
        rho    = cov / sqrt(var_a * var_b),  NaN where n < 2 or a variance is not positive.
    The mean that is taken out is therefore the one over the row's pairs and the frames, separately at the a and the b side: right for
    flows that are homogeneous along x.  For flows that are not, give TwoPointStats the per-pixel mean of a first pass (`mean=`): the
    sums are then formed from fluctuations, and what is taken out here is a remainder near zero.
    `which`: "uu", "vv", "uv" (u at a, v at b) or "vu";  `axis`: "x" / 0 (the partner r*step columns to the right) or "y" / 1 (r*step rows
    below).  Separations are in pixels: sep[r] = r*step."""

    def __init__(self, acc, step: int = 1, frames: int = 0):
        acc = np.asarray(acc, dtype=np.float64)
        if acc.ndim != 4 or acc.shape[0] != 2 or acc.shape[2] != len(TERMS):
            raise ValueError(f"TwoPointResult: expected accumulators [2,R+1,{len(TERMS)},H], got {acc.shape}")
        self.acc, self.step, self.frames = acc, int(step), int(frames)
        self.max_sep, self.H = acc.shape[1] - 1, acc.shape[3]
        self.sep = np.arange(self.max_sep + 1, dtype=np.float64) * self.step

    # ---- correlations ---------------------------------------------------------------------------------------------------------------
    def correlation(self, which: str = "uu", axis="x") -> Correlation:
        """Per row: n, cov, var_a, var_b, rho as [R+1, H] by the formulas of the class."""
        xy, xa, yb, xx, yy = _which(which)
        s = self.acc[_axis(axis)]
        n = s[:, T["n"]]
        with np.errstate(invalid="ignore", divide="ignore"):
            ma, mb = s[:, xa] / n, s[:, yb] / n
            cov, va, vb = s[:, xy] / n - ma * mb, s[:, xx] / n - ma * ma, s[:, yy] / n - mb * mb
        return Correlation(n, cov, va, vb, _rho(cov, va, vb, n))

    def pooled(self, which: str = "uu", axis="x", rows=slice(None)) -> Correlation:
        """The n-weighted mean over the rows `rows` of the per-row covariances and variances, sum_y n_y c_y / sum_y n_y (rows without
        pairs carry no weight), and rho from those: [R+1] arrays; n is the number of pairs pooled."""
        c = self.correlation(which, axis)
        n = c.n[:, rows].reshape(self.max_sep + 1, -1)
        total = n.sum(1)

        def mean(a):
            a = a[:, rows].reshape(n.shape)
            with np.errstate(invalid="ignore", divide="ignore"):
                return np.where(n > 0, n * np.where(n > 0, a, 0.0), 0.0).sum(1) / total
        cov, va, vb = mean(c.cov), mean(c.var_a), mean(c.var_b)
        return Correlation(total, cov, va, vb, _rho(cov, va, vb, total))

    # ---- structure functions -----------------------------------------------------------------------------------------------------------
    def structure(self, order: int = 2, kind: str = "L", axis="x", rows=None) -> np.ndarray:
        """Structure functions of the increment along (L) and across (T) the separation; along x the longitudinal component is u,
        along y it is v.  order 2, kind "L" or "T":  D = (S_bb - 2*S_ab + S_aa)/n of that component, the mean of (c_b - c_a)^2 from the
        stored sums.  order 3, kind "LLL": S_lll/n, the mean of dL^3;  "LTT": S_ltt/n, the mean of dL*dT^2.  rows=None: per row
        [R+1, H];  otherwise the sums are added over `rows` first: [R+1].  NaN where there is no pair."""
        d = _axis(axis)
        s = self.acc[d]
        if order == 2 and kind in ("L", "T"):
            comp = "u" if (kind == "L") == (d == 0) else "v"
            top = s[:, T[f"{comp}b{comp}b"]] - 2.0 * s[:, T[f"{comp}a{comp}b"]] + s[:, T[f"{comp}a{comp}a"]]
        elif order == 3 and kind in ("LLL", "LTT"):
            top = s[:, T[kind.lower()]]
        else:
            raise ValueError(f"structure: order={order!r}, kind={kind!r}: order 2 takes 'L' or 'T', order 3 'LLL' or 'LTT'")
        n = s[:, T["n"]]
        if rows is not None:
            top, n = top[:, rows].reshape(self.max_sep + 1, -1).sum(1), n[:, rows].reshape(self.max_sep + 1, -1).sum(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, top / n, np.nan)

    # ---- what is read off a correlation --------------------------------------------------------------------------------------------------
    def integral_scale(self, which: str = "uu", axis="x", rows=slice(None)) -> IntegralScale:
        """The trapezoid integral of the pooled rho over sep from 0 to its first zero crossing, which is interpolated linearly between
        the last positive node (i-1) and the first node with rho <= 0 (i):  x0 = sep[i-1] + rho[i-1]/(rho[i-1] - rho[i]) * step, the last
        piece being the triangle 0.5*rho[i-1]*(x0 - sep[i-1]).  If rho never crosses zero the integral runs to the last separation with
        a defined rho and truncated=True.  NaN where rho(0) is undefined."""
        rho = self.pooled(which, axis, rows).rho
        if not np.isfinite(rho[0]):
            return IntegralScale(math.nan, True, None)
        m = 1
        while m <= self.max_sep and np.isfinite(rho[m]) and rho[m] > 0:
            m += 1
        area = float(np.sum(0.5 * (rho[1:m] + rho[:m - 1]) * (self.sep[1:m] - self.sep[:m - 1])))
        if m > self.max_sep or not np.isfinite(rho[m]):
            return IntegralScale(area, True, None)
        x0 = self.sep[m - 1] + rho[m - 1] / (rho[m - 1] - rho[m]) * (self.sep[m] - self.sep[m - 1])
        return IntegralScale(area + float(0.5 * rho[m - 1] * (x0 - self.sep[m - 1])), False, float(x0))

    def taylor_fit(self, which: str = "uu", axis="x", fit=(1, 4), rows=slice(None)) -> TaylorFit:
        """The least-squares fit of rho(r) = c - (r*step)^2/ell^2 to the pooled rho at the indices fit[0] .. fit[1], both included (the
        default leaves out r = 0, where the uncorrelated noise of the vectors adds to the variance alone).  The signal's own
        correlation is rho/c = 1 - sep^2/(c*ell^2), so the Taylor microscale is lambda = sqrt(c)*ell, and 1 - c is the share of the
        variance that is noise: the usual estimate of the random error of PIV from the intercept of the correlation.  NaN where the
        parabola does not open downwards or c <= 0."""
        lo, hi = int(fit[0]), int(fit[1])
        if not 0 <= lo < hi <= self.max_sep:
            raise ValueError(f"taylor_fit: fit={fit!r} must be two indices 0 <= first < last <= {self.max_sep}")
        rho = self.pooled(which, axis, rows).rho[lo:hi + 1]
        q = self.sep[lo:hi + 1] ** 2
        if not np.isfinite(rho).all():
            return TaylorFit(math.nan, math.nan, math.nan, math.nan)
        qm, rm = q.mean(), rho.mean()
        slope = float(((q - qm) * (rho - rm)).sum() / ((q - qm) ** 2).sum())
        c = float(rm - slope * qm)
        if not (slope < 0 and c > 0):
            return TaylorFit(math.nan, 1.0 - c, c, math.nan)
        ell = math.sqrt(-1.0 / slope)
        return TaylorFit(math.sqrt(c) * ell, 1.0 - c, c, ell)

    def spectrum(self, which: str = "uu", axis="x", window: Optional[str] = "hann", rows=slice(None)):
        """(k, E): the cosine transform of the pooled covariance R(sep_j), j = 0..M, M the last separation with pairs.  R is extended
        evenly to the period 2M;  with the lag window w_j = 0.5*(1 + cos(pi*j/M)) ("hann") or w_j = 1 (None)
            k_m = pi*m/(M*step), m = 0..M  (radians per pixel),
            E_m = step/pi * (w_0 R_0 + 2*sum_{j=1}^{M-1} w_j R_j cos(pi*j*m/M) + (-1)^m w_M R_M).
        Normalisation: the one-sided density in angular wavenumber -- the trapezoid rule over k, dk*(E_0/2 + E_1 + ... + E_{M-1} + E_M/2)
        with dk = pi/(M*step), returns R_0, the variance, for either window (w_0 = 1)."""
        if window not in ("hann", None):
            raise ValueError(f"spectrum: window={window!r} must be 'hann' or None")
        p = self.pooled(which, axis, rows)
        have = np.nonzero((p.n > 0) & np.isfinite(p.cov))[0]
        M = int(have[-1]) if len(have) else 0
        if M < 1 or len(have) != M + 1:
            raise ValueError("spectrum: needs pairs at every separation up to the last one that has any, and at least two separations")
        j = np.arange(M + 1, dtype=np.float64)
        R = p.cov[:M + 1] * (0.5 * (1.0 + np.cos(math.pi * j / M)) if window == "hann" else 1.0)
        weight = np.full(M + 1, 2.0)
        weight[0] = weight[M] = 1.0
        E = self.step / math.pi * (np.cos(math.pi * np.outer(j, j) / M) @ (weight * R))
        return math.pi * j / (M * self.step), E

    def summary(self) -> Dict[str, object]:
        """The scalar results as a JSON-ready dict: the parameters, and per "uu_x", "uu_y", "vv_x", "vv_y" the pooled variance at
        separation 0, the integral scale with its flags, and the Taylor fit over the default range (NaN where max_sep < 4)."""
        doc: Dict[str, object] = {"frames": self.frames, "max_sep": self.max_sep, "step": self.step, "rows": self.H}
        for which in ("uu", "vv"):
            for axis in ("x", "y"):
                p = self.pooled(which, axis)
                scale = self.integral_scale(which, axis)
                t = self.taylor_fit(which, axis) if self.max_sep >= 4 else TaylorFit(math.nan, math.nan, math.nan, math.nan)
                doc[f"{which}_{axis}"] = {"pairs": float(p.n[0]), "variance": float(p.var_a[0]), "integral_scale": float(scale.scale),
                                          "truncated": bool(scale.truncated), "crossing": scale.crossing,
                                          "taylor_microscale": float(t.microscale), "noise_share": float(t.noise)}
        return doc


class TwoPointStats(_accum.FrameAccumulator):
    """Running two-point sums over a flow sequence of one size: acc [2, max_sep+1, 15, H] float64 on the device (TERMS order) and the
    frame count.  update() enqueues one kernel on the current stream and never synchronises the host; result() / save() do.
    `mean`: None, a [2,H,W] tensor or array (held as float64 on the device), or the path of a FlowStats file, whose mean_u and mean_v
    are taken: the second pass of a two-pass evaluation of flows that are not homogeneous along a row."""

    def __init__(self, H: int, W: int, max_sep: int = 64, step: int = 1, mean=None, device=None):
        check_params(max_sep, step)
        self.max_sep, self.step = max_sep, step
        super().__init__(H, W, device, int(W) <= 16384, " (positive, at most 16384 columns)")
        self.mean = _accum.load_planes(mean, ("mean_u", "mean_v"), "TwoPointStats: mean", self.H, self.W, self.device)
        self.acc = torch.zeros([2, max_sep + 1, len(TERMS), self.H], dtype=torch.float64, device=self.device)

    def update(self, flows: torch.Tensor, mask: Optional[torch.Tensor] = None) -> None:
        """Add the frames of `flows` [B,2,H,W] (float32, on this device), in batch order; `mask` [B,H,W]: nonzero = leave the vector out."""
        flows = _args.check_flows(flows, "TwoPointStats.update")
        self._check_mine(flows.shape[2:], flows.device, lambda: f"flows {tuple(flows.shape)} on {flows.device}",
                         "accumulators for [{H},{W}]")
        mask = _args.check_mask(mask, "TwoPointStats.update", truth=flows)
        B = flows.size(0)
        self._enqueue(B, (_lib.load().pivlfn_twopoint_accumulate, flows.data_ptr(), mask.data_ptr() if mask is not None else None,
                          self.mean.data_ptr() if self.mean is not None else None, self.acc.data_ptr(), B, self.H, self.W,
                          self.max_sep, self.step))

    def merge(self, group=None) -> None:
        """Collective over `group`: every rank ends with the accumulators of all ranks added in rank order (the same bits on every
        rank) and the summed count.  Under gloo the exchange runs on host copies, as FlowStats.merge does."""
        self.count = _accum.merge_sums([self.acc], self.count, group)

    def result(self) -> TwoPointResult:
        return TwoPointResult(self.acc.cpu().numpy(), self.step, self.count)

    def save(self, path: str, **extra) -> str:
        """An .npz with the raw accumulators (`acc`, TERMS order), the parameters (H, W, max_sep, step, frames), `sep`, and pooled over
        all rows per axis a in x, y: rho_uu_a, rho_vv_a, rho_uv_a, cov_uu_a, cov_vv_a, cov_uv_a, pairs_a, d_ll_a, d_tt_a, d_lll_a,
        d_ltt_a; and `extra`.  Returns the path written."""
        res = self.result()
        out = {"acc": res.acc, "H": np.int64(self.H), "W": np.int64(self.W), "max_sep": np.int64(self.max_sep), "step": np.int64(self.step),
               "frames": np.int64(self.count), "sep": res.sep}
        for a in ("x", "y"):
            for which in ("uu", "vv", "uv"):
                p = res.pooled(which, a)
                out[f"rho_{which}_{a}"], out[f"cov_{which}_{a}"] = p.rho, p.cov
            out[f"pairs_{a}"] = res.pooled("uu", a).n
            for name, order, kind in (("d_ll", 2, "L"), ("d_tt", 2, "T"), ("d_lll", 3, "LLL"), ("d_ltt", 3, "LTT")):
                out[f"{name}_{a}"] = res.structure(order, kind, a, rows=slice(None))
        return _accum.save_npz(path, **extra, **out)
