"""Velocity distributions of a flow sequence on the device: the probability density of u and v, their joint density, the per-pixel
skewness and flatness, the quadrant split of the Reynolds shear stress, and the histogram of the sub-pixel part of the displacement,
which shows peak locking -- the bias of a PIV estimate towards integer pixels.

The sums run on csrc/distribution.hip through the C ABI (`pivlfn_flow_moments_accumulate`, `pivlfn_flow_hist_accumulate`; the
arithmetic contract is written out in include/pivlfn.h); everything derived from them is host work in float64:

    fd = FlowDistribution(H, W, bins=256, range=(-8.0, 8.0), joint_bins=64, frac_bins=64)
    for flows in chunks: fd.update(flows, mask)               # enqueued on the current stream, no host synchronisation
    r = fd.result()
    centres, density = r.pdf("u");  r.outside("u")            # (under, over) shares
    r.peak_locking("u")                                       # 1 - N_min / N_max of the fraction histogram: 0 none, 1 complete
    r.skewness("u"), r.flatness("u"), r.count                 # [H,W] maps
    r.pooled(), r.quadrants(), r.summary();  fd.save("pdf.npz")

The per-pixel sums are kept in an order the contract fixes and the histograms are integer counts, so a sequence gives the same bits
however it is cut into update() calls.

Accuracy: the central moments follow from the raw sums S_k by the binomial formulas (DistributionResult).  Without `mean=` these
subtract large numbers from each other wherever the mean is large against the fluctuation; the two-pass form -- a first pass with
FlowStats (`run.py --stats`), then `mean="stats.npz"` -- forms the sums from fluctuations and is the accurate one.  GPU only, like the
rest of the package: there is no CPU path.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _accum, _args, _lib

TERMS = ("n", "u", "v", "uu", "vv", "uv", "uuu", "vvv", "uuv", "vvu", "uuuu", "vvvv", "uuvv", "n1", "n2", "n3", "n4", "p1", "p2", "p3",
         "p4")                                                                   # acc[:, y, x]
T = {name: i for i, name in enumerate(TERMS)}
SUMS = {"u": ("u", "uu", "uuu", "uuuu"), "v": ("v", "vv", "vvv", "vvvv")}


def hist_words(bins: int, joint_bins: int, frac_bins: int) -> int:
    """PIVLFN_HIST_WORDS of include/pivlfn.h."""
    return 2 * (bins + 2) + joint_bins * joint_bins + 1 + 2 * frac_bins + 2


def check_params(bins, range, joint_bins, frac_bins, hole=0.0) -> None:                # noqa: A002  (the keyword of FlowDistribution)
    """The parameter checks of FlowDistribution (ValueError), usable before any tensor exists."""
    _args.check_int("FlowDistribution", "bins", bins, 1, 4096, ", the bins of a marginal histogram")
    _args.check_int("FlowDistribution", "joint_bins", joint_bins, 0, 256, ", the bins per side of the joint histogram (0: none)")
    _args.check_int("FlowDistribution", "frac_bins", frac_bins, 0, 1024, ", the bins of the sub-pixel fraction (0: none)")
    try:
        lo, hi = (float(x) for x in range)
    except (TypeError, ValueError):
        raise ValueError(f"FlowDistribution: range={range!r} must be two numbers (lo, hi)") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
        raise ValueError(f"FlowDistribution: range=({lo!r}, {hi!r}) must be finite with hi > lo")
    _args.check_not_negative("FlowDistribution", "hole", hole)


def _component(c: str) -> int:
    if c not in ("u", "v"):
        raise ValueError(f"component={c!r} must be 'u' or 'v'")
    return "uv".index(c)


def _central(n, s1, s2, s3, s4):
    """(m2, m3, m4) about m = S1/n by the binomial formulas; NaN where n = 0."""
    with np.errstate(invalid="ignore", divide="ignore"):
        m = s1 / n
        m2 = s2 / n - m * m
        m3 = s3 / n - 3.0 * m * (s2 / n) + 2.0 * m * m * m
        m4 = s4 / n - 4.0 * m * (s3 / n) + 6.0 * m * m * (s2 / n) - 3.0 * m * m * m * m
    return m2, m3, m4


def _shape(n, m2, m3, m4):
    """(skewness, flatness): m3 / m2^1.5 and m4 / m2^2, NaN where n < 2 or m2 <= 0."""
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = (n >= 2) & (m2 > 0)
        safe = np.where(ok, m2, 1.0)
        return np.where(ok, m3 / safe ** 1.5, np.nan), np.where(ok, m4 / (safe * safe), np.nan)


class DistributionResult:
    """Everything derived from the raw sums acc [21,H,W] (float64, TERMS order) and the counters hist (uint64, the layout of
    include/pivlfn.h), on the host in float64.  With n = S_n and m = S1/n of a component the central moments are
        m2 = S2/n - m^2,  m3 = S3/n - 3 m S2/n + 2 m^3,  m4 = S4/n - 4 m S3/n + 6 m^2 S2/n - 3 m^4,
    skewness = m3 / m2^1.5 and flatness = m4 / m2^2, both NaN where n < 2 or m2 <= 0.  Every density, share and degree is NaN where
    nothing was counted.  `normalised`: the samples of the histograms are in units of the local rms (FlowDistribution's scale)."""

    def __init__(self, acc, hist, bins: int, range: Tuple[float, float], joint_bins: int, frac_bins: int, frames: int = 0,   # noqa: A002
                 hole: float = 0.0, normalised: bool = False):
        acc, hist = np.asarray(acc, dtype=np.float64), np.asarray(hist, dtype=np.uint64)
        if acc.ndim != 3 or acc.shape[0] != len(TERMS):
            raise ValueError(f"DistributionResult: expected sums [{len(TERMS)},H,W], got {acc.shape}")
        if hist.shape != (hist_words(bins, joint_bins, frac_bins),):
            raise ValueError(f"DistributionResult: expected {hist_words(bins, joint_bins, frac_bins)} counters for bins={bins}, "
                             f"joint_bins={joint_bins}, frac_bins={frac_bins}, got {hist.shape}")
        self.acc, self.hist = acc, hist
        self.bins, self.joint_bins, self.frac_bins = int(bins), int(joint_bins), int(frac_bins)
        self.lo, self.hi = float(range[0]), float(range[1])
        self.frames, self.hole, self.normalised = int(frames), float(hole), bool(normalised)
        j = 2 * (self.bins + 2)
        self._at = {"u": 0, "v": self.bins + 2, "joint": j, "outside": j + self.joint_bins ** 2}
        self._at["fu"] = self._at["outside"] + 1
        self._at["fv"] = self._at["fu"] + self.frac_bins
        self._at["n"] = self._at["fv"] + self.frac_bins

    # ---- the histograms ---------------------------------------------------------------------------------------------------------------
    @property
    def counted(self) -> int:
        """The vectors counted into every histogram."""
        return int(self.hist[self._at["n"]])

    @property
    def left_out(self) -> int:
        """The vectors left out: masked, invalid, or without a finite mean or a positive finite scale."""
        return int(self.hist[self._at["n"] + 1])

    def _share(self, counts):
        return np.asarray(counts, np.float64) / self.counted if self.counted else np.full(np.shape(counts), np.nan)

    def marginal(self, component: str = "u") -> np.ndarray:
        """The raw counts [bins + 2]: under, the bins, over."""
        at = self._at["uv"[_component(component)]]
        return self.hist[at:at + self.bins + 2]

    def pdf(self, component: str = "u"):
        """(centres, density): count / (vectors counted * bin width); its integral over the range is the share inside the range."""
        width = (self.hi - self.lo) / self.bins
        centres = self.lo + (np.arange(self.bins) + 0.5) * width
        return centres, self._share(self.marginal(component)[1:-1]) / width

    def outside(self, component: str = "u") -> Tuple[float, float]:
        """The shares of the vectors below lo and at or above hi."""
        m = self.marginal(component)
        under, over = self._share([m[0], m[-1]])
        return float(under), float(over)

    def joint_counts(self) -> np.ndarray:
        """The raw counts [joint_bins, joint_bins]: row = the bin of v, column = the bin of u."""
        at = self._at["joint"]
        return self.hist[at:at + self.joint_bins ** 2].reshape(self.joint_bins, self.joint_bins)

    def joint(self):
        """(centres, density [joint_bins, joint_bins]): count / (vectors counted * bin area), row = v, column = u."""
        if self.joint_bins == 0:
            raise ValueError("joint: the accumulator was made with joint_bins=0")
        width = (self.hi - self.lo) / self.joint_bins
        centres = self.lo + (np.arange(self.joint_bins) + 0.5) * width
        return centres, self._share(self.joint_counts()) / (width * width)

    def outside_joint(self) -> float:
        """The share of the vectors outside the joint range in either component."""
        return float(self._share(self.hist[self._at["outside"]]))

    def fraction(self, component: str = "u") -> np.ndarray:
        """The counts [frac_bins] of the sub-pixel part d - floor(d) of the raw displacement."""
        at = self._at["f" + "uv"[_component(component)]]
        return self.hist[at:at + self.frac_bins]

    def peak_locking(self, component: str = "u") -> float:
        """The degree of peak locking 1 - N_min / N_max of the fraction histogram: 0 for a flat histogram, 1 where a bin is empty (every
        displacement an integer).  NaN without vectors or without a fraction histogram."""
        f = self.fraction(component).astype(np.float64)
        return float(1.0 - f.min() / f.max()) if f.size and f.max() > 0 else math.nan

    # ---- the per-pixel moments -----------------------------------------------------------------------------------------------------------
    @property
    def count(self) -> np.ndarray:
        """[H,W]: the vectors that entered the sums of each pixel."""
        return self.acc[T["n"]]

    def central(self, component: str = "u"):
        """(m2, m3, m4) maps [H,W] by the formulas of the class."""
        return _central(self.count, *(self.acc[T[k]] for k in SUMS["uv"[_component(component)]]))

    def skewness(self, component: str = "u") -> np.ndarray:
        return _shape(self.count, *self.central(component))[0]

    def flatness(self, component: str = "u") -> np.ndarray:
        return _shape(self.count, *self.central(component))[1]

    def pooled(self) -> Dict[str, float]:
        """Over the frame: the sums of all pixels added (the n-weighted means of the per-pixel raw moments) and the formulas of the class
        applied to them, so the moments are about the pooled mean -- about zero where a per-pixel mean was taken out first.  Keys:
        count, mean_u, var_u, skewness_u, flatness_u, the same for v, and cov_uv."""
        s = self.acc.reshape(len(TERMS), -1).sum(1)
        n = s[T["n"]]
        out: Dict[str, float] = {"count": float(n)}
        for c in ("u", "v"):
            m2, m3, m4 = _central(n, *(s[T[k]] for k in SUMS[c]))
            skew, flat = _shape(n, m2, m3, m4)
            out[f"mean_{c}"] = float(s[T[c]] / n) if n > 0 else math.nan
            out[f"var_{c}"], out[f"skewness_{c}"], out[f"flatness_{c}"] = float(m2), float(skew), float(flat)
        out["cov_uv"] = float(s[T["uv"]] / n - (s[T["u"]] / n) * (s[T["v"]] / n)) if n > 0 else math.nan
        return out

    def quadrants(self, pooled: bool = False) -> Dict[str, np.ndarray]:
        """The quadrant analysis of P = U*V (Q1: U > 0, V > 0; Q2: U < 0, V > 0; Q3: U < 0, V < 0; Q4: U > 0, V < 0; an event needs
        |P| > the hole).  Per pixel [4,H,W], or over the frame [4] with pooled=True:  `events`: N_q / (N_1 + .. + N_4);  `stress`:
        S_q / S_uv, the share of the whole sum of U*V (the four add to 1 where the hole is 0);  `mean`: the conditional mean S_q / N_q;
        and `hole` [H,W]: the share 1 - (N_1 + .. + N_4) / n of the vectors that are no event.  NaN where the denominator is 0."""
        nq, sq, n, suv = self.acc[13:17], self.acc[17:21], self.count, self.acc[T["uv"]]
        if pooled:
            nq, sq, n, suv = nq.reshape(4, -1).sum(1), sq.reshape(4, -1).sum(1), n.sum(), suv.sum()
        with np.errstate(invalid="ignore", divide="ignore"):
            events = nq.sum(0)
            return {"events": np.where(events > 0, nq / events, np.nan), "stress": np.where(suv != 0, sq / suv, np.nan),
                    "mean": np.where(nq > 0, sq / nq, np.nan), "hole": np.where(n > 0, 1.0 - events / n, np.nan)}

    def summary(self) -> Dict[str, object]:
        """The scalar results as a JSON-ready dict."""
        q = self.quadrants(pooled=True)
        doc: Dict[str, object] = {"frames": self.frames, "bins": self.bins, "range": [self.lo, self.hi], "joint_bins": self.joint_bins,
                                  "frac_bins": self.frac_bins, "hole": self.hole, "normalised": self.normalised,
                                  "counted": self.counted, "left_out": self.left_out, "pooled": self.pooled(),
                                  "outside_joint": self.outside_joint(),
                                  "quadrants": {k: [float(x) for x in np.atleast_1d(q[k])] for k in ("events", "stress", "mean", "hole")}}
        for c in ("u", "v"):
            under, over = self.outside(c)
            doc[f"peak_locking_{c}"] = self.peak_locking(c)
            doc[f"outside_{c}"] = {"under": under, "over": over}
        return doc

    # ---- files ---------------------------------------------------------------------------------------------------------------------------
    def save(self, path: str, **extra) -> str:
        """An .npz with every raw sum and parameter: acc, hist, bins, lo, hi, joint_bins, frac_bins, frames, hole, normalised; and for
        reading without this class pdf_u, pdf_v, centres, frac_u, frac_v; and `extra`.  Returns the path written."""
        centres, pdf_u = self.pdf("u")
        out = {"acc": self.acc, "hist": self.hist, "bins": np.int64(self.bins), "lo": np.float64(self.lo), "hi": np.float64(self.hi),
               "joint_bins": np.int64(self.joint_bins), "frac_bins": np.int64(self.frac_bins), "frames": np.int64(self.frames),
               "hole": np.float64(self.hole), "normalised": np.bool_(self.normalised), "centres": centres, "pdf_u": pdf_u,
               "pdf_v": self.pdf("v")[1], "frac_u": self.fraction("u"), "frac_v": self.fraction("v")}
        return _accum.save_npz(path, **extra, **out)

    @classmethod
    def load(cls, path: str) -> "DistributionResult":
        with np.load(path) as f:
            return cls(f["acc"], f["hist"], int(f["bins"]), (float(f["lo"]), float(f["hi"])), int(f["joint_bins"]), int(f["frac_bins"]),
                       int(f["frames"]), float(f["hole"]), bool(f["normalised"]))


class FlowDistribution(_accum.FrameAccumulator):
    """Running distribution sums over a flow sequence of one size: acc [21,H,W] float64 (TERMS order) and the counters hist (int64
    holding the unsigned words of include/pivlfn.h) on the device, and the frame count.  update() enqueues two kernels on the current
    stream and never synchronises the host; result() / save() do.
    `mean`: None, a [2,H,W] tensor or array, or the path of a FlowStats file, whose mean_u and mean_v are taken out of every vector
    first: the second pass of a two-pass evaluation, and the accurate form (see the module).  `scale`: None, a [2,H,W] array, or the same
    path, whose rms_u and rms_v are taken: the histograms are then of U / scale_u and V / scale_v (`range` in those units), and a pixel
    whose scale is not positive and finite is left out of them.  `hole`: the hole size of the quadrant analysis; an event needs
    |U*V| > hole * scale_u * scale_v, or > hole where no scale is given.  The fraction histogram is of the raw displacement always."""

    def __init__(self, H: int, W: int, bins: int = 256, range=(-8.0, 8.0), joint_bins: int = 64, frac_bins: int = 64,   # noqa: A002
                 mean=None, scale=None, hole: float = 0.0, device=None):
        check_params(bins, range, joint_bins, frac_bins, hole)
        super().__init__(H, W, device, int(H) * int(W) < 1 << 31, " (positive, fewer than 2^31 vectors)")
        self.bins, self.joint_bins, self.frac_bins = bins, joint_bins, frac_bins
        self.lo, self.hi, self.hole = float(range[0]), float(range[1]), float(hole)
        self.mean = _accum.load_planes(mean, ("mean_u", "mean_v"), "FlowDistribution: mean", self.H, self.W, self.device)
        self.scale = _accum.load_planes(scale, ("rms_u", "rms_v"), "FlowDistribution: scale", self.H, self.W, self.device)
        if self.scale is not None:
            self.thr = (self.hole * self.scale[0] * self.scale[1]).contiguous()
        elif self.hole > 0.0:
            self.thr = torch.full([self.H, self.W], self.hole, dtype=torch.float64, device=self.device)
        else:
            self.thr = None
        self.acc = torch.zeros([len(TERMS), self.H, self.W], dtype=torch.float64, device=self.device)
        self.hist = torch.zeros([hist_words(bins, joint_bins, frac_bins)], dtype=torch.int64, device=self.device)

    def update(self, flows: torch.Tensor, mask: Optional[torch.Tensor] = None) -> None:
        """Add the frames of `flows` [B,2,H,W] (float32, on this device), in batch order; `mask` [B,H,W]: nonzero = leave the vector out."""
        flows = _args.check_flows(flows, "FlowDistribution.update")
        self._check_mine(flows.shape[2:], flows.device, lambda: f"flows {tuple(flows.shape)} on {flows.device}",
                         "accumulators for [{H},{W}]")
        mask = _args.check_mask(mask, "FlowDistribution.update", truth=flows)
        B = flows.size(0)
        lib = _lib.load()
        self._enqueue(B, (lib.pivlfn_flow_moments_accumulate, flows.data_ptr(), _args.ptr(mask), _args.ptr(self.mean), _args.ptr(self.thr),
                          self.acc.data_ptr(), B, self.H, self.W),
                      (lib.pivlfn_flow_hist_accumulate, flows.data_ptr(), _args.ptr(mask), _args.ptr(self.mean), _args.ptr(self.scale),
                       self.hist.data_ptr(), B, self.H, self.W, self.lo, self.hi, self.bins, self.joint_bins, self.frac_bins))

    def result(self) -> DistributionResult:
        return DistributionResult(self.acc.cpu().numpy(), self.hist.cpu().numpy().view(np.uint64), self.bins, (self.lo, self.hi),
                                  self.joint_bins, self.frac_bins, self.count, self.hole, self.scale is not None)

    def save(self, path: str, **extra) -> str:
        """DistributionResult.save of the current sums; DistributionResult.load reads the file back."""
        return self.result().save(path, **extra)
