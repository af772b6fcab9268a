"""Vector validation of estimated flows on the device: the normalized median test (Westerweel & Scarano, Exp. Fluids 39, 2005)
with masking or median replacement of the vectors it rejects, and flow statistics that leave the rejected vectors out.

Runs on csrc/validate.hip and csrc/postpro.hip through the C ABI (`pivlfn_flow_validate`, `pivlfn_flow_stats_accumulate_masked`;
the arithmetic contract is written out in include/pivlfn.h):

    res = validate_flow(flows)                                 # [B,2,H,W] on the device; res.flow, res.flag, res.residual
    n_outliers = int((res.flag & OUTLIER).ne(0).sum())

    stats = MaskedFlowStats(H, W, calib, device)
    for flows in chunks:
        res = validate_flow(flows, mode="flag")
        stats.update(flows, res.flag)                          # enqueued on the current stream, no host synchronisation
    stats.save("stats.npz")

GPU only, like the rest of the package: there is no CPU path.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from . import _accum, _args, _lib
from .postpro import SUMS

MODES = {"flag": 0, "mask": 1, "replace": 2}         # PIVLFN_VALIDATE_FLAG, PIVLFN_VALIDATE_MASK, PIVLFN_VALIDATE_REPLACE
OUTLIER, UNKNOWN, NOT_REPLACED = 1, 2, 4             # the bits of a flag byte
COUNTS = ("count_uv", "count_vort")                  # the planes of MaskedFlowStats.cnt, in order
MASKED_RESULT = ("count", "count_uv", "count_vort", "valid_fraction", "mean_u", "mean_v", "rms_u", "rms_v", "cov_uv", "mean_vort",
                 "rms_vort")


class Validated(NamedTuple):
    """What validate_flow returns."""
    flow: torch.Tensor                    # [B,2,H,W] float32; for mode "flag" the input tensor itself
    flag: torch.Tensor                    # [B,H,W] uint8: OUTLIER | UNKNOWN | NOT_REPLACED
    residual: Optional[torch.Tensor]      # [B,2,H,W] float32 normalized residuals (R_u, R_v), or None


def check_params(radius, spacing, eps, thresh, mode) -> None:
    """The parameter checks of validate_flow (ValueError), usable before any flow exists."""
    if mode not in MODES:
        raise ValueError(f"validate_flow: unknown mode {mode!r} (one of {', '.join(MODES)})")
    if not _args.is_int(radius, 1, 2):
        raise ValueError(f"validate_flow: radius={radius!r} must be 1 (3 x 3 neighbourhood) or 2 (5 x 5)")
    if not _args.is_int(spacing, 1) or radius * spacing >= 1 << 15:
        raise ValueError(f"validate_flow: spacing={spacing!r} must be an integer >= 1 with radius*spacing below 2^15")
    eps, thresh = float(eps), float(thresh)
    if not math.isfinite(eps) or eps < 0.0:
        raise ValueError(f"validate_flow: eps={eps!r} must be finite and not negative")
    if not math.isfinite(thresh) or thresh <= 0.0:
        raise ValueError(f"validate_flow: thresh={thresh!r} must be finite and positive")


def validate_flow(flow: torch.Tensor, radius: int = 1, spacing: int = 1, eps: float = 0.1, thresh: float = 2.0,
                  mode: str = "replace", residual: bool = False) -> Validated:
    """Normalized median test on [B,2,H,W] float32 flows on the device, enqueued on the current stream (no host synchronisation).

    Each vector is compared, per component, with the median of its (2*radius+1)^2 - 1 neighbours `spacing` pixels apart (those inside
    the image that are not unknown; no edge replication), normalised by the median of the neighbours' own distances to that
    median plus `eps`; a vector whose normalised residual exceeds `thresh` in u or v gets the OUTLIER bit of its flag byte.  A
    vector with a NaN component or one beyond 1e9 in magnitude (the reference's unknown flow) gets the UNKNOWN bit and takes no
    part in any neighbourhood.  mode "flag": nothing else (`.flow` is the input tensor itself); "mask": flagged vectors become
    1e10 in both components, the Middlebury value for an unknown vector; "replace": flagged vectors become the component-wise
    median of their unflagged neighbours (one iteration: replaced values are never used to replace others), and keep their input
    value and get the NOT_REPLACED bit when there is no such neighbour.  residual=True also returns the normalised residuals.

    The defaults eps = 0.1 px, thresh = 2 are the paper's and suit a dense field compared at `spacing` 1.  With a larger spacing the
    difference a smooth velocity gradient makes between neighbours grows past eps and clean vectors are flagged (a 4 px amplitude
    vortex of 128 px wavelength loses hundreds of clean vectors at spacing 4): raise eps with the spacing.

    pivlfn.flo needs nothing for masked flows: 1e10 round-trips through a .flo like any float, and the reference's readers treat
    anything above 1e9 as unknown."""
    check_params(radius, spacing, eps, thresh, mode)
    given, flow = flow, _args.check_flows(flow, "validate_flow")
    B, _, H, W = flow.shape
    flag = torch.empty([B, H, W], dtype=torch.uint8, device=flow.device)
    out = given if mode == "flag" else torch.empty_like(flow)
    res = torch.empty_like(flow) if residual else None
    if B > 0:
        with torch.cuda.device(flow.device):
            _lib.check(_lib.load().pivlfn_flow_validate(flow.data_ptr(), None if mode == "flag" else out.data_ptr(), flag.data_ptr(),
                                                        res.data_ptr() if residual else None, B, H, W, radius, spacing, float(eps),
                                                        float(thresh), MODES[mode], _lib.stream_ptr(flow.device)), "validate_flow")
    return Validated(out, flag, res)


def _check_flags(flag: torch.Tensor, flow: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(flag, torch.Tensor) or flag.dtype != torch.uint8:
        raise TypeError(f"{what}: expected a uint8 flag tensor [B,H,W], got "
                        f"{flag.dtype if isinstance(flag, torch.Tensor) else type(flag).__name__}")
    if flag.device != flow.device or tuple(flag.shape) != (flow.size(0), flow.size(2), flow.size(3)):
        raise ValueError(f"{what}: flags {tuple(flag.shape)} on {flag.device} do not belong to flows {tuple(flow.shape)} on {flow.device}")
    return flag.detach().contiguous()


def finalize_masked(acc: np.ndarray, cnt: np.ndarray, count: int) -> Dict[str, np.ndarray]:
    """postpro.finalize with a count per pixel: u / v statistics divide by cnt[0], vorticity statistics by cnt[1]; NaN where the
    count is 0.  Adds count_uv, count_vort (int64 [H,W]) and valid_fraction = count_uv / count."""
    acc, cnt = np.asarray(acc, dtype=np.float64), np.asarray(cnt, dtype=np.float64)
    if acc.ndim != 3 or acc.shape[0] != len(SUMS) or cnt.shape != (len(COUNTS),) + acc.shape[1:]:
        raise ValueError(f"finalize_masked: expected accumulators [7,H,W] and counts [2,H,W], got {acc.shape} and {cnt.shape}")
    if count <= 0:
        raise ValueError("finalize_masked: no frames accumulated")
    n, nw = (np.where(c > 0, c, np.nan) for c in cnt)
    mu, mv, mw = acc[0] / n, acc[1] / n, acc[5] / nw

    def rms(s2, m, k):
        return np.sqrt(np.maximum(s2 / k - m * m, 0.0))             # NaN stays NaN through maximum and sqrt
    return {"count": np.array(count, dtype=np.int64), "count_uv": cnt[0].astype(np.int64), "count_vort": cnt[1].astype(np.int64),
            "valid_fraction": cnt[0] / float(count), "mean_u": mu, "mean_v": mv, "rms_u": rms(acc[2], mu, n),
            "rms_v": rms(acc[3], mv, n), "cov_uv": acc[4] / n - mu * mv, "mean_vort": mw, "rms_vort": rms(acc[6], mw, nw)}


class MaskedFlowStats(_accum.FrameAccumulator):
    """FlowStats that leaves flagged vectors out: acc [7,H,W] float64 (postpro.SUMS order) and cnt [2,H,W] float64 (COUNTS order) on
    the device.  A frame adds its u, v sums at a pixel only where its flag is 0, and its vorticity sums only where the flags of the
    whole 3 x 3 stencil are 0.  update() enqueues one kernel on the current stream and never synchronises the host."""

    def __init__(self, H: int, W: int, calib=1.0, device=None):
        self.calib = _args.check_calib(calib)
        super().__init__(H, W, device)
        self.acc = torch.zeros([len(SUMS), self.H, self.W], dtype=torch.float64, device=self.device)
        self.cnt = torch.zeros([len(COUNTS), self.H, self.W], dtype=torch.float64, device=self.device)

    def update(self, flow: torch.Tensor, flag: torch.Tensor) -> None:
        """Add the frames of `flow` [B,2,H,W] (float32, the flows validate_flow was given) under `flag` [B,H,W], in batch order."""
        flow = _args.check_flows(flow, "MaskedFlowStats.update")
        flag = _check_flags(flag, flow, "MaskedFlowStats.update")
        self._check_mine(flow.shape[2:], flow.device, lambda: f"flows {tuple(flow.shape)} on {flow.device}")
        B = flow.size(0)
        self._enqueue(B, (_lib.load().pivlfn_flow_stats_accumulate_masked, flow.data_ptr(), flag.data_ptr(), self.acc.data_ptr(),
                          self.cnt.data_ptr(), B, self.H, self.W, self.calib))

    def merge(self, group=None) -> None:
        """Collective over `group`, as FlowStats.merge: sums and counts of all ranks added in rank order, on every rank."""
        self.count = _accum.merge_sums([self.acc, self.cnt], self.count, group)

    def result(self) -> Dict[str, np.ndarray]:
        """finalize_masked() of the current sums (MASKED_RESULT): NaN where no frame contributed."""
        return finalize_masked(self.acc.cpu().numpy(), self.cnt.cpu().numpy(), self.count)

    def save(self, path: str, **extra) -> str:
        """An .npz with result()'s arrays, the raw accumulators (`acc`, `cnt`), `calib` and `extra`; returns the path written."""
        return _accum.save_npz(path, acc=self.acc.cpu().numpy(), cnt=self.cnt.cpu().numpy(), calib=np.float64(self.calib), **extra,
                               **self.result())
