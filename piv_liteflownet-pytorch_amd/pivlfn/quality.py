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

from . import _lib
from .evaluate import _check_mask
from .postpro import _check_flows

FEW, FLAT, NO_PEAK, CENTRE_OUT = 1, 2, 4, 8          # the bits of a flag byte (PIVLFN_QUALITY_*)
FLAG_NAMES = ("few", "flat", "no_peak", "centre_out")


def default_min_count(radius: int) -> int:
    """Half the window, rounded up: ((2r+1)^2 + 1) // 2."""
    return ((2 * radius + 1) ** 2 + 1) // 2


def check_params(radius, floor, min_count) -> int:
    """The parameter checks of match_quality (ValueError), usable before any image exists; returns the min_count in effect."""
    if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= 15:
        raise ValueError(f"match_quality: radius={radius!r} must be an integer 1..15 (a window of 3 x 3 to 31 x 31 pixels)")
    if min_count is None:
        min_count = default_min_count(radius)
    if isinstance(min_count, bool) or not isinstance(min_count, int) or not 2 <= min_count <= (2 * radius + 1) ** 2:
        raise ValueError(f"match_quality: min_count={min_count!r} must be an integer 2..{(2 * radius + 1) ** 2}, the pixels of the window")
    floor = float(floor)
    if not math.isfinite(floor) or floor < 0.0:
        raise ValueError(f"match_quality: floor={floor!r} must be finite and not negative")
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


def _check_images(img1, img2, what: str):
    for name, t in (("img1", img1), ("img2", img2)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"{what}: expected a float32 tensor [B,C,H,W] for {name}, got "
                            f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
    if img1.dim() != 4 or img1.size(1) not in (1, 3):
        raise ValueError(f"{what}: expected images [B,C,H,W] with C = 1 or 3, got {tuple(img1.shape)}")
    if img2.shape != img1.shape or img2.device != img1.device:
        raise ValueError(f"{what}: img2 {tuple(img2.shape)} on {img2.device} does not belong to img1 {tuple(img1.shape)} on {img1.device}")
    return img1.detach().contiguous(), img2.detach().contiguous()


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
    img1, img2 = _check_images(img1, img2, "match_quality")
    if isinstance(flow, torch.Tensor) and flow.dtype == torch.float32 and (
            flow.dim() != 4 or flow.size(1) != 2 or flow.device != img1.device or flow.size(0) != img1.size(0)
            or tuple(flow.shape[2:]) != tuple(img1.shape[2:])):
        raise ValueError(f"match_quality: flows {tuple(flow.shape)} on {flow.device} do not belong to images {tuple(img1.shape)} on "
                         f"{img1.device}")
    flow = _check_flows(flow, "match_quality")
    mask = _check_mask(mask, flow, "match_quality")
    B, C, H, W = img1.shape
    quality = torch.empty([B, 3, H, W], dtype=torch.float32, device=flow.device)
    flag = torch.empty([B, H, W], dtype=torch.uint8, device=flow.device)
    if B > 0:
        with torch.cuda.device(flow.device):
            lib = _lib.load()
            ws = torch.empty(lib.pivlfn_match_quality_workspace_bytes(B, H, W, radius), dtype=torch.uint8, device=flow.device)
            _lib.check(lib.pivlfn_match_quality(img1.data_ptr(), img2.data_ptr(), C, flow.data_ptr(),
                                                mask.data_ptr() if mask is not None else None, quality.data_ptr(), flag.data_ptr(),
                                                B, H, W, radius, min_count, float(floor), ws.data_ptr(), ws.numel(),
                                                _lib.stream_ptr(flow.device)), "match_quality")
    return MatchQuality(quality[:, 0], quality[:, 1:], flag)
