"""Vortex identification on the device: the functions Gamma1 and Gamma2 of Graftieaux, Michard and Grosjean (2001) of estimated flows.
Around every vector, over its (2*radius+1)^2 - 1 neighbours at `spacing` pixels: Gamma1 is the mean sine of the angle between the
direction to a neighbour and the neighbour's velocity -- it peaks at a vortex centre, but a drift moves the peak -- and Gamma2 is the
same about the window's own mean velocity, which makes it Galilean invariant; |Gamma2| > 2/pi is where rotation dominates shear, the
vortex core.  Vorticity cannot make that distinction: a plain shear has vorticity everywhere and |Gamma2| < 2/pi everywhere.

Runs on csrc/vortex.hip through the C ABI (`pivlfn_vortex_gamma`; the arithmetic contract is written out in include/pivlfn.h):

    v = vortex_gamma(flow, radius=4)                           # [B,2,H,W] flows on the device
    v.cores()                                                  # +1 / -1 / 0 by Gamma2 against 2/pi
    v.peaks()                                                  # per pair: the vortex centres, sub-pixel, strongest first
    print(v.summary())

Gamma is positive where dv/dx - du/dy > 0 with x the column and y the row index -- one convention throughout, unlike the mixed one of
flow_fields' "de_vort".  Every sum is formed in float64 in an order the contract fixes: a pair gives the same bits alone, in any batch
and in any run.  GPU only, like the rest of the package: there is no CPU path.
"""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional

import torch
import torch.nn.functional as F

from . import _args

FEW, CENTRE_OUT = 1, 2                # the bits of a flag byte (PIVLFN_VORTEX_*)
CORE = 2.0 / math.pi                  # |Gamma2| above it: rotation dominates shear
SUMS = ("pixels", "few", "defined", "area_pos", "area_neg", "sum_abs_gamma1", "sum_abs_gamma2")       # the columns of VortexField.sums()


def default_min_count(radius: int) -> int:
    """Half the neighbours: (2r+1)^2 // 2."""
    return (2 * radius + 1) ** 2 // 2


def check_params(radius, spacing, min_count) -> int:
    """The parameter checks of vortex_gamma (ValueError), usable before any tensor exists; returns the min_count in effect."""
    _args.check_int("vortex_gamma", "radius", radius, 1, 15, " (3 x 3 to 31 x 31 vectors)")
    _args.check_int("vortex_gamma", "spacing", spacing, 1, 16, ", the distance between neighbours in pixels")
    if min_count is None:
        min_count = default_min_count(radius)
    _args.check_int("vortex_gamma", "min_count", min_count, 1, (2 * radius + 1) ** 2 - 1, ", the neighbours of a vector")
    return min_count


def _parabola(lo: float, mid: float, hi: float) -> float:
    """The vertex of the parabola through (-1, lo), (0, mid), (1, hi), clamped to +-0.5; +0.0 where a neighbour is missing or not
    finite or the three values lie on a line."""
    if not (math.isfinite(lo) and math.isfinite(mid) and math.isfinite(hi)):
        return 0.0
    den = (lo - 2.0 * mid) + hi
    if den == 0.0:
        return 0.0
    return min(0.5, max(-0.5, 0.5 * (lo - hi) / den))


def summarize(row) -> Dict[str, float]:
    """One row of VortexField.sums() -- or the sum of several -- as the dict summary() returns."""
    px, few, defined, pos, neg, s1, s2 = (float(x) for x in row)
    share = (lambda n: n / px) if px else (lambda n: math.nan)
    return {"few": share(few), "defined": int(defined), "area_pos": int(pos), "area_neg": int(neg),
            "fraction_pos": share(pos), "fraction_neg": share(neg), "fraction_core": share(pos + neg),
            "radius_pos": math.sqrt(pos / math.pi), "radius_neg": math.sqrt(neg / math.pi),
            "mean_abs_gamma1": s1 / defined if defined else math.nan, "mean_abs_gamma2": s2 / defined if defined else math.nan}


class VortexField(NamedTuple):
    """What vortex_gamma returns.  `gamma1` and `gamma2` are views of one [B,2,H,W] buffer."""
    gamma1: torch.Tensor          # [B,H,W] float32; NaN where FEW is set
    gamma2: torch.Tensor          # [B,H,W] float32; NaN where FEW is set
    flag: torch.Tensor            # [B,H,W] uint8: FEW | CENTRE_OUT
    radius: int = 4               # the parameters the fields were formed with: peaks() takes its default distance from them
    spacing: int = 1

    def cores(self, threshold: float = CORE) -> torch.Tensor:
        """[B,H,W] int8: +1 where Gamma2 > threshold, -1 where Gamma2 < -threshold, 0 elsewhere (undefined pixels included)."""
        return (self.gamma2 > threshold).to(torch.int8) - (self.gamma2 < -threshold).to(torch.int8)

    def sums(self) -> torch.Tensor:
        """[B,7] float64 on the device (SUMS): what summary() is formed from, additive over pairs.  No host synchronisation."""
        flat = self.flag.flatten(1)
        few = (flat & FEW).ne(0)
        g1, g2 = self.gamma1.flatten(1).to(torch.float64), self.gamma2.flatten(1).to(torch.float64)
        zero = torch.zeros_like(g2)
        cols = [torch.full([flat.size(0)], float(flat.size(1)), dtype=torch.float64, device=flat.device),
                few.sum(1).to(torch.float64), (~few).sum(1).to(torch.float64),
                (g2 > CORE).sum(1).to(torch.float64), (g2 < -CORE).sum(1).to(torch.float64),
                torch.where(few, zero, g1.abs()).sum(1), torch.where(few, zero, g2.abs()).sum(1)]
        return torch.stack(cols, dim=1)

    def summary(self) -> List[Dict[str, float]]:
        """Per pair: the share of FEW pixels, the number of defined ones, the areas (pixels), area fractions and equivalent radii
        sqrt(area / pi) of the regions Gamma2 > 2/pi and Gamma2 < -2/pi, and the means of |Gamma1| and |Gamma2| over the defined
        pixels (NaN where there is none).  Plain torch in float64; copies the numbers to the host."""
        if self.flag.size(0) == 0:
            return []
        return [summarize(row) for row in self.sums().cpu().tolist()]

    def peaks(self, of: str = "gamma2", threshold: float = 0.9, distance: Optional[int] = None) -> List[List[Dict[str, float]]]:
        """Per pair the local maxima of a = |Gamma2| (or |Gamma1| with of="gamma1") that reach `threshold`, strongest first: the
        vortex centres.  Synchronises: the candidates are copied to the host.

        A candidate is a pixel with a >= threshold that equals the maximum of a over the (2*distance+1)^2 pixels around it (undefined
        pixels count as -inf); `distance` is in pixels and defaults to radius * spacing.  The candidates are sorted by (-a, linear
        index) and one is kept unless a kept one lies within Chebyshev distance `distance`.  Each kept peak is refined by a
        three-point parabola per axis (+0 where a neighbour is missing or not finite, clamped to +-0.5).  Entries: x, y (sub-pixel),
        value (signed), ix, iy."""
        if of not in ("gamma1", "gamma2"):
            raise ValueError(f"peaks: of={of!r} must be 'gamma1' or 'gamma2'")
        distance = self.radius * self.spacing if distance is None else distance
        if not _args.is_int(distance, 1):
            raise ValueError(f"peaks: distance={distance!r} must be a positive integer (pixels)")
        field = self.gamma1 if of == "gamma1" else self.gamma2
        B, H, W = field.shape
        if B == 0:
            return []
        a = torch.where(torch.isnan(field), torch.full_like(field, -math.inf), field.abs())
        k = 2 * distance + 1                                                    # the maximum over a square: along x, then along y
        top = F.max_pool2d(F.max_pool2d(a.unsqueeze(1), (1, k), stride=1, padding=(0, distance)), (k, 1), stride=1, padding=(distance, 0))
        cand = (a >= threshold) & (a == top.squeeze(1))
        b, iy, ix = cand.nonzero(as_tuple=True)
        wide = F.pad(a, (1, 1, 1, 1), value=-math.inf)                          # a missing neighbour is not finite
        taps = torch.stack([wide[b, iy + 1, ix + 1], wide[b, iy + 1, ix], wide[b, iy + 1, ix + 2], wide[b, iy, ix + 1], wide[b, iy + 2, ix + 1],
                            field[b, iy, ix]], dim=1).to(torch.float64)
        rows = torch.cat([torch.stack([b, iy, ix], dim=1).to(torch.float64), taps], dim=1).cpu().tolist()
        out: List[List[Dict[str, float]]] = [[] for _ in range(B)]
        for pb, y, x, mid, left, right, up, down, value in sorted(rows, key=lambda row: (row[0], -row[3], row[1] * W + row[2])):
            kept = out[int(pb)]
            if any(max(abs(p["ix"] - x), abs(p["iy"] - y)) <= distance for p in kept):
                continue
            kept.append({"x": x + _parabola(left, mid, right), "y": y + _parabola(up, mid, down), "value": value, "ix": int(x), "iy": int(y)})
        return out


def vortex_gamma(flow: torch.Tensor, radius: int = 4, spacing: int = 1, mask: Optional[torch.Tensor] = None,
                 min_count: Optional[int] = None) -> VortexField:
    """Gamma1 and Gamma2 of [B,2,H,W] float32 flows on the device; enqueued on the current stream (no host synchronisation).

    The neighbours of a vector are the (2*radius+1)^2 - 1 vectors at multiples of `spacing` pixels around it that lie inside the image
    (no edge replication); vectors with a nonzero byte of `mask` [B,H,W] and any non-finite or 1e10 vector are left out.  Flags: FEW --
    fewer than `min_count` neighbours left (default: half of them), both fields are NaN there; CENTRE_OUT -- the vector itself is
    masked or invalid (the values are still formed, from its neighbours)."""
    min_count = check_params(radius, spacing, min_count)
    flow = _args.check_flows(flow, "vortex_gamma")
    mask = _args.check_mask(mask, "vortex_gamma", truth=flow)
    B, _, H, W = flow.shape
    gamma = torch.empty([B, 2, H, W], dtype=torch.float32, device=flow.device)
    flag = torch.empty([B, H, W], dtype=torch.uint8, device=flow.device)
    if B > 0:
        _args.call_with_workspace("vortex_gamma", flow.device, (B, H, W, radius, spacing), flow.data_ptr(), _args.ptr(mask), gamma.data_ptr(),
                                  flag.data_ptr(), B, H, W, radius, spacing, min_count)
    return VortexField(gamma[:, 0], gamma[:, 1], flag, radius, spacing)
