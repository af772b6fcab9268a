"""Per-vector uncertainty of estimated flows on the device, from the image pair itself (Wieneke 2015, "PIV uncertainty quantification
from correlation statistics"): how asymmetric the correlation peak of image 1 against image 2 warped back by the flow may be, given
the pixel-wise scatter of the products it is summed from, carried through the three-point peak fit.  In pixels, per axis; needs no
truth field and no neighbouring vectors.

Runs on csrc/uncertainty.hip through the C ABI (`pivlfn_flow_uncertainty`, `pivlfn_uncertainty_accumulate`; the arithmetic contract is
written out in include/pivlfn.h):

    unc = flow_uncertainty(img1, img2, flow, radius=8)        # [B,C,H,W] images and [B,2,H,W] flows on the device
    usable = (unc.flag & UNUSABLE) == 0                       # unc.u: (ux, uy) in px, NaN elsewhere
    print(unc.summary())

    stats = UncertaintyStats(H, W, device)
    for ...: stats.update(unc)                                # enqueued on the current stream, no host synchronisation
    stats.save("uncertainty_stats.npz")                       # the noise share of the normal stresses, the uncertainty of the mean

    cov = uncertainty_coverage(flow, truth, unc)              # with a truth field: 0.68 for a calibrated estimate

Every sum is formed in float64 in an order the contract fixes: a pair gives the same bits alone, in any batch and in any run.
GPU only, like the rest of the package: there is no CPU path.
"""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import _accum, _args, _lib
from .quality import default_min_count

FEW, FLAT, NO_PEAK, NO_VARIANCE, CENTRE_OUT = 1, 2, 4, 8, 16          # the bits of a flag byte (PIVLFN_UNCERTAINTY_*)
UNUSABLE = FEW | FLAT | NO_PEAK | NO_VARIANCE                         # any of these: the vector has no uncertainty (NaN)
FLAG_NAMES = ("few", "flat", "no_peak", "no_variance", "centre_out")
SUMS = ("pixels",) + FLAG_NAMES + ("n", "sum_ux", "sum_uy", "sum_ux2", "sum_uy2")          # the columns of FlowUncertainty.sums()
STATS_SUMS = ("sum_ux2", "sum_uy2", "n")                              # the planes of UncertaintyStats.acc, in order
UNKNOWN = 1e9                                                         # |truth| above it is unknown, as in pivlfn.evaluate


def check_params(radius, lag, floor, min_count) -> int:
    """The parameter checks of flow_uncertainty (ValueError), usable before any image exists; returns the min_count in effect."""
    _args.check_int("flow_uncertainty", "radius", radius, 1, 15, " (a window of 3 x 3 to 31 x 31 pixels)")
    _args.check_int("flow_uncertainty", "lag", lag, 0, 4, " (the covariance of the contributions is summed over (2 lag + 1)^2 offsets)")
    if min_count is None:
        min_count = default_min_count(radius)
    _args.check_int("flow_uncertainty", "min_count", min_count, 2, (2 * radius + 1) ** 2, ", the pixels of the window")
    _args.check_not_negative("flow_uncertainty", "floor", floor)
    return min_count


class FlowUncertainty(NamedTuple):
    """What flow_uncertainty returns."""
    u: torch.Tensor               # [B,2,H,W] float32: (ux, uy), the standard uncertainty in pixels; NaN where a bit of UNUSABLE is set
    flag: torch.Tensor            # [B,H,W] uint8: FEW | FLAT | NO_PEAK | NO_VARIANCE | CENTRE_OUT

    def magnitude(self) -> torch.Tensor:
        """[B,H,W]: sqrt(ux^2 + uy^2)."""
        return self.u.pow(2).sum(1).sqrt()

    def sums(self) -> torch.Tensor:
        """[B,11] float64 on the device (SUMS): what summary() is formed from, additive over pairs.  No host synchronisation."""
        flat = self.flag.flatten(1)
        cols = [torch.full([flat.size(0)], float(flat.size(1)), dtype=torch.float64, device=flat.device)]
        cols += [(flat & bit).ne(0).sum(1).to(torch.float64) for bit in (FEW, FLAT, NO_PEAK, NO_VARIANCE, CENTRE_OUT)]
        ok = (flat & UNUSABLE).eq(0)
        cols.append(ok.sum(1).to(torch.float64))
        u = self.u.flatten(2).to(torch.float64)
        u = torch.where(ok.unsqueeze(1), u, torch.zeros_like(u))
        cols += [u[:, 0].sum(1), u[:, 1].sum(1), u[:, 0].pow(2).sum(1), u[:, 1].pow(2).sum(1)]
        return torch.stack(cols, dim=1)

    def summary(self) -> List[Dict[str, float]]:
        """Per pair: the shares of the five flag bits, the number of usable vectors and the mean and RMS of ux and uy over them (NaN
        where there is none).  Plain torch in float64; copies the numbers to the host."""
        if self.flag.size(0) == 0:
            return []
        return [summarize(row) for row in self.sums().cpu().tolist()]


def summarize(row) -> Dict[str, float]:
    """One row of FlowUncertainty.sums() -- or the sum of several -- as the dict summary() returns."""
    px, few, flat, no_peak, no_var, centre_out, n, sx, sy, sxx, syy = (float(x) for x in row)
    out = {name: c / px if px else math.nan for name, c in zip(FLAG_NAMES, (few, flat, no_peak, no_var, centre_out))}
    out["n"] = int(n)
    for key, s, ss in (("ux", sx, sxx), ("uy", sy, syy)):
        out["mean_" + key] = s / n if n else math.nan
        out["rms_" + key] = math.sqrt(ss / n) if n else math.nan
    return out


def flow_uncertainty(img1: torch.Tensor, img2: torch.Tensor, flow: torch.Tensor, radius: int = 8, lag: int = 2,
                     mask: Optional[torch.Tensor] = None, floor: float = 1.0 / 255.0, min_count: Optional[int] = None) -> FlowUncertainty:
    """The standard uncertainty of every vector of `flow` in pixels, per axis, from the correlation statistics of the (2*radius+1)^2
    window around it, on the device; enqueued on the current stream (no host synchronisation).

    img1, img2, flow, mask, floor, min_count: as for match_quality (image 2 is sampled at pixel + flow; masked pixels and invalid
    samples are left out).  Both images lose their mean over the window around each pixel first.  The window's correlation at zero
    shift is C0, at the two one-pixel shifts of an axis C+ and C-; the variance of C+ - C- is the sum, over the window, of the
    covariance of its pixel-wise terms over the (2*lag+1)^2 nearest offsets (the particle images make neighbouring terms dependent;
    lag 2 is enough for particle images of 2-3 px).  One standard deviation of it, put through the three-point Gaussian fit, is the
    uncertainty.  Flags: FEW -- fewer than `min_count` valid pixels or pairs; FLAT -- the high-passed windows correlate by less than
    floor^2 per pixel; NO_PEAK -- zero shift is not a positive maximum; NO_VARIANCE -- the variance estimate is not positive (the
    estimate of a sum of covariances can be); CENTRE_OUT -- the pixel itself is masked or warps outside."""
    min_count = check_params(radius, lag, floor, min_count)
    img1, img2 = _args.check_images(img1, img2, "flow_uncertainty")
    flow = _args.check_flows(flow, "flow_uncertainty", images=img1)
    mask = _args.check_mask(mask, "flow_uncertainty", truth=flow)
    B, C, H, W = img1.shape
    u = torch.empty([B, 2, H, W], dtype=torch.float32, device=flow.device)
    flag = torch.empty([B, H, W], dtype=torch.uint8, device=flow.device)
    if B > 0:
        _args.call_with_workspace("flow_uncertainty", flow.device, (B, H, W, radius, lag), img1.data_ptr(), img2.data_ptr(), C,
                                  flow.data_ptr(), _args.ptr(mask), u.data_ptr(), flag.data_ptr(), B, H, W, radius, lag, min_count,
                                  float(floor))
    return FlowUncertainty(u, flag)


class UncertaintyStats(_accum.FrameAccumulator):
    """Per-pixel running sums of the squared uncertainties over a sequence of one size: acc [3,H,W] float64 on the device
    (STATS_SUMS order; the third plane counts the pairs that had an uncertainty at the pixel).  update() enqueues one kernel on the
    current stream and never synchronises the host; result() / save() do."""

    def __init__(self, H: int, W: int, device=None):
        super().__init__(H, W, device)
        self.acc = torch.zeros([len(STATS_SUMS), self.H, self.W], dtype=torch.float64, device=self.device)

    def update(self, unc: FlowUncertainty) -> None:
        """Add the pairs of `unc` (a FlowUncertainty on this device), in batch order."""
        u, flag = unc.u, unc.flag
        if not isinstance(u, torch.Tensor) or u.dtype != torch.float32 or not isinstance(flag, torch.Tensor) or flag.dtype != torch.uint8:
            raise TypeError("UncertaintyStats.update: expected a FlowUncertainty (u float32 [B,2,H,W], flag uint8 [B,H,W])")
        self._check_mine(u.shape[2:], u.device, lambda: f"u {tuple(u.shape)} on {u.device} and flag {tuple(flag.shape)} on {flag.device}",
                         also=u.dim() == 4 and u.size(1) == 2 and tuple(flag.shape) == (u.size(0), self.H, self.W)
                         and flag.device == self.device)
        B = u.size(0)
        u, flag = u.detach().contiguous(), flag.contiguous()
        self._enqueue(B, (_lib.load().pivlfn_uncertainty_accumulate, u.data_ptr(), flag.data_ptr(), self.acc.data_ptr(), B, self.H, self.W))

    @staticmethod
    def finalize(acc, count: int) -> Dict[str, np.ndarray]:
        """From the three sums (STATS_SUMS order) of `count` pairs: `count`; `n`, the pairs that contributed at each pixel;
        noise_var_u / noise_var_v = sum u^2 / n, the mean squared uncertainty: the share of measurement noise in the measured normal
        stresses u'u' and v'v';  mean_unc_u / mean_unc_v = sqrt(sum u^2) / n, the uncertainty of the mean velocity for independent
        samples.  float64 [H,W], NaN where no pair contributed."""
        acc = np.asarray(acc, dtype=np.float64)
        if acc.ndim != 3 or acc.shape[0] != len(STATS_SUMS):
            raise ValueError(f"UncertaintyStats.finalize: expected accumulators [3,H,W], got {acc.shape}")
        n = acc[2]
        with np.errstate(divide="ignore", invalid="ignore"):
            out = {"count": np.array(count, dtype=np.int64), "n": n.astype(np.int64)}
            for key, s in (("u", acc[0]), ("v", acc[1])):
                out["noise_var_" + key] = np.where(n > 0, s / n, np.nan)
                out["mean_unc_" + key] = np.where(n > 0, np.sqrt(s) / n, np.nan)
        return out

    def result(self) -> Dict[str, np.ndarray]:
        """finalize() of the current sums."""
        return self.finalize(self.acc.cpu().numpy(), self.count)

    def save(self, path: str, **extra) -> str:
        """An .npz with result()'s arrays, the raw accumulators (`acc`, STATS_SUMS order) and `extra`; returns the path written."""
        return _accum.save_npz(path, acc=self.acc.cpu().numpy(), **extra, **self.result())


COVERAGE_SUMS = ("n_x", "n_y", "inside_x", "inside_y", "sum_err2_x", "sum_err2_y", "sum_u2_x", "sum_u2_y")


def coverage_sums(flow: torch.Tensor, truth: torch.Tensor, unc: FlowUncertainty, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B,8] float64 (COVERAGE_SUMS) on the tensors' device, additive over pairs; no host synchronisation.  Exact integer counts and
    float64 sums in plain torch."""
    u, flag = unc.u, unc.flag
    if flow.shape != truth.shape or flow.shape != u.shape or flow.dim() != 4 or flow.size(1) != 2:
        raise ValueError(f"uncertainty_coverage: flow {tuple(flow.shape)}, truth {tuple(truth.shape)} and u {tuple(u.shape)} must all "
                         "be [B,2,H,W]")
    known = (truth.abs() <= UNKNOWN).all(dim=1) & (flag & UNUSABLE).eq(0)
    if mask is not None:
        if tuple(mask.shape) != tuple(flag.shape):
            raise ValueError(f"uncertainty_coverage: mask {tuple(mask.shape)} does not belong to flags {tuple(flag.shape)}")
        known &= mask.eq(0)
    err = (flow.to(torch.float64) - truth.to(torch.float64)).abs()
    u = u.to(torch.float64)
    use = known.unsqueeze(1) & err.le(UNKNOWN)                         # a non-finite or unknown estimate is left out, per axis
    zero = torch.zeros_like(err)
    n = use.flatten(2).sum(2)
    inside = (use & err.le(u)).flatten(2).sum(2)
    e2 = torch.where(use, err * err, zero).flatten(2).sum(2)
    u2 = torch.where(use, u * u, zero).flatten(2).sum(2)
    return torch.cat([n.to(torch.float64), inside.to(torch.float64), e2, u2], dim=1)


def summarize_coverage(row) -> Dict[str, float]:
    """One row of coverage_sums() -- or the sum of several -- as a dict: per axis the number of vectors compared, the share whose
    |flow - truth| <= u (0.68 for a calibrated estimate) and RMS error / RMS u (1 for a calibrated estimate)."""
    nx, ny, ix, iy, ex, ey, ux, uy = (float(x) for x in row)
    out = {}
    for key, n, inside, e2, u2 in (("x", nx, ix, ex, ux), ("y", ny, iy, ey, uy)):
        out["n_" + key] = int(n)
        out["coverage_" + key] = inside / n if n else math.nan
        out["error_over_u_" + key] = math.sqrt(e2 / u2) if n and u2 > 0 else math.nan
    return out


def uncertainty_coverage(flow: torch.Tensor, truth: torch.Tensor, unc: FlowUncertainty,
                         mask: Optional[torch.Tensor] = None) -> List[Dict[str, float]]:
    """Per pair and axis: the share of usable vectors with known truth (|truth| <= 1e9, not masked) whose |flow - truth| <= u, and the
    ratio RMS error / RMS u over the same vectors.  Copies the numbers to the host."""
    if flow.size(0) == 0:
        return []
    return [summarize_coverage(row) for row in coverage_sums(flow, truth, unc, mask).cpu().tolist()]
