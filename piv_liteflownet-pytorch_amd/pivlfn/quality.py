"""Match quality of estimated flows on the device: how well image 2, warped back by the flow, matches image 1 inside an interrogation
window around every pixel -- the correlation peak height a classical PIV code reports beside each vector -- and, from the position of
that match's peak, what a window-deformation pass would still add to the vector.  Needs no truth field and no neighbouring vectors.

Runs on csrc/quality.hip through the C ABI (`pivlfn_match_quality`; the arithmetic contract is written out in include/pivlfn.h):

    q = match_quality(img1, img2, flow, radius=8)              # [B,C,H,W] images and [B,2,H,W] flows on the device
    good = (q.flag & (FEW | FLAT | NO_PEAK)) == 0              # q.c: peak height, q.residual: (dx, dy) in px
    better = q.corrected(flow)
    print(q.summary())

Every sum is formed in float64 in an order the contract fixes: a pair gives the same bits alone, in any batch and in any run.
GPU only, like the rest of the package: there is no CPU path.
"""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional

import torch

from . import _args

FEW, FLAT, NO_PEAK, CENTRE_OUT = 1, 2, 4, 8          # the bits of a flag byte (PIVLFN_QUALITY_*)
FLAG_NAMES = ("few", "flat", "no_peak", "centre_out")


def default_min_count(radius: int) -> int:
    """Half the window, rounded up: ((2r+1)^2 + 1) // 2."""
    return ((2 * radius + 1) ** 2 + 1) // 2


def check_params(radius, floor, min_count) -> int:
    """The parameter checks of match_quality (ValueError), usable before any image exists; returns the min_count in effect."""
    _args.check_int("match_quality", "radius", radius, 1, 15, " (a window of 3 x 3 to 31 x 31 pixels)")
    if min_count is None:
        min_count = default_min_count(radius)
    _args.check_int("match_quality", "min_count", min_count, 2, (2 * radius + 1) ** 2, ", the pixels of the window")
    _args.check_not_negative("match_quality", "floor", floor)
    return min_count


class MatchQuality(NamedTuple):
    """What match_quality returns.  `c` and `residual` are views of one [B,3,H,W] buffer (planes c, dx, dy)."""
    c: torch.Tensor               # [B,H,W] float32: the normalised correlation at zero shift; NaN where FEW or FLAT is set
    residual: torch.Tensor        # [B,2,H,W] float32: (dx, dy) in pixels, |.| <= 0.5; +0.0 where FEW, FLAT or NO_PEAK is set
    flag: torch.Tensor            # [B,H,W] uint8: FEW | FLAT | NO_PEAK | CENTRE_OUT

    def corrected(self, flow: torch.Tensor) -> torch.Tensor:
        """flow + residual: the peak sits at the error of the flow."""
        return flow + self.residual

    def sums(self) -> torch.Tensor:
        """[B,9] float64 on the device (SUMS): what summary() is formed from, additive over pairs.  No host synchronisation."""
        flat = self.flag.flatten(1)
        cols = [torch.full([flat.size(0)], float(flat.size(1)), dtype=torch.float64, device=flat.device)]
        cols += [(flat & bit).ne(0).sum(1).to(torch.float64) for bit in (FEW, FLAT, NO_PEAK, CENTRE_OUT)]
        c = self.c.flatten(1).to(torch.float64)
        has_c = (flat & (FEW | FLAT)).eq(0)
        cols += [has_c.sum(1).to(torch.float64), torch.where(has_c, c, torch.zeros_like(c)).sum(1)]
        fit = (flat & (FEW | FLAT | NO_PEAK)).eq(0)
        d2 = self.residual.to(torch.float64).pow(2).sum(1).flatten(1)
        cols += [fit.sum(1).to(torch.float64), torch.where(fit, d2, torch.zeros_like(d2)).sum(1)]
        return torch.stack(cols, dim=1)

    def summary(self) -> List[Dict[str, float]]:
        """Per pair: the shares of the four flag bits, the mean of c where it is defined (NaN where nowhere), the RMS of |residual|
        where FEW, FLAT and NO_PEAK are clear and the number of such pixels.  Plain torch in float64; copies the numbers to the
        host."""
        if self.flag.size(0) == 0:
            return []
        return [summarize(row) for row in self.sums().cpu().tolist()]


SUMS = ("pixels", "few", "flat", "no_peak", "centre_out", "n_c", "sum_c", "n_fit", "sum_d2")      # the columns of MatchQuality.sums()


def summarize(row) -> Dict[str, float]:
    """One row of MatchQuality.sums() -- or the sum of several -- as the dict summary() returns."""
    px, few, flat, no_peak, centre_out, n_c, sum_c, n_fit, sum_d2 = (float(x) for x in row)
    out = {name: n / px if px else math.nan for name, n in zip(FLAG_NAMES, (few, flat, no_peak, centre_out))}
    out["mean_c"] = sum_c / n_c if n_c else math.nan
    out["rms_residual"] = math.sqrt(sum_d2 / n_fit) if n_fit else math.nan
    out["n_fit"] = int(n_fit)
    return out


def match_quality(img1: torch.Tensor, img2: torch.Tensor, flow: torch.Tensor, radius: int = 8, mask: Optional[torch.Tensor] = None,
                  floor: float = 1.0 / 255.0, min_count: Optional[int] = None) -> MatchQuality:
    """Windowed correlation between img1 and img2 warped back by `flow`, and the sub-pixel residual of its peak, on the device;
    enqueued on the current stream (no host synchronisation).

    img1, img2: [B,C,H,W] float32 with C = 1 or 3 (the gray value is the channel mean), the tensors the network was given; flow:
    [B,2,H,W] float32 of the same H and W.  Image 2 is sampled bilinearly at pixel + flow (backwarp's position); a sample outside the
    image, and any non-finite or 1e10 flow, is invalid.  Around every pixel the (2*radius+1)^2 window, clipped to the image, gives the
    normalised correlation c0 at zero shift and the four at one-pixel shifts; pixels with a nonzero byte of `mask` [B,H,W] and
    invalid samples are left out.  Flags: FEW -- fewer than `min_count` pixels left (default: half the window); FLAT -- the gray
    values of either window vary by less than `floor` RMS (default one grey level of an 8-bit frame); NO_PEAK -- c0 is not a
    positive maximum of the five values, so the error of the vector is beyond half a pixel or the match is noise; CENTRE_OUT -- the
    pixel itself is masked or warps outside.  `residual` is the peak position by a three-point Gaussian fit per axis."""
    min_count = check_params(radius, floor, min_count)
    img1, img2 = _args.check_images(img1, img2, "match_quality")
    flow = _args.check_flows(flow, "match_quality", images=img1)
    mask = _args.check_mask(mask, "match_quality", truth=flow)
    B, C, H, W = img1.shape
    quality = torch.empty([B, 3, H, W], dtype=torch.float32, device=flow.device)
    flag = torch.empty([B, H, W], dtype=torch.uint8, device=flow.device)
    if B > 0:
        _args.call_with_workspace("match_quality", flow.device, (B, H, W, radius), img1.data_ptr(), img2.data_ptr(), C, flow.data_ptr(),
                                  _args.ptr(mask), quality.data_ptr(), flag.data_ptr(), B, H, W, radius, min_count, float(floor))
    return MatchQuality(quality[:, 0], quality[:, 1:], flag)
