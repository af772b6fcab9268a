"""Flow smoothing and gap filling on the device: Garcia's penalised least squares (Comput. Stat. Data Anal. 54, 2010; Exp. Fluids 50,
2011 -- PIVlab's smoothn).  Per frame and component the field z that minimises

    sum w (y - z)^2 + s |Lap z|^2

with weight 0 at masked and unknown vectors, so smoothing and gap filling are one solve:  (W + s D^T D) z = W y,  D the 5-point Laplacian
with reflecting boundaries.  Solved by conjugate gradients preconditioned with the gap-free problem, which the 2-D DCT diagonalises.

The kernels are csrc/smooth.hip behind the C ABI (`pivlfn_dct2`, `pivlfn_smooth_setup`, `_pcg`, `_read`; the arithmetic contract is
written out in include/pivlfn.h):

    res = smooth_flow(flow, wavelength=8.0, mask=validate_flow(flow, mode="flag").flag)
    res.flow, res.z, res.filled                    # [B,2,H,W] float32 and float64, [B,H,W] bool: the vector had weight 0
    res.iterations, res.residual, res.converged    # [B,2], per frame and component; a frame that hit max_iter is reported, never hidden

`s` is the smoothing parameter; `wavelength` names it by the 1-D wave whose amplitude it halves: s = smooth_param(wavelength).
weights_from_uncertainty turns flow_uncertainty's output into weights.  dct2 is the transform on its own.

Limits: no automatic choice of s, no robust reweighting (validate_flow supplies the mask), no smoothing in time, sides up to 4096.
GPU only, like the rest of the package: there is no CPU path."""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from . import _args, _lib
from .uncertainty import UNUSABLE

RUNNING, CONVERGED, BREAKDOWN, EMPTY = 1, 2, 3, 4       # PIVLFN_SMOOTH_*: the state of a (frame, component) system
MAX_SIDE = 4096                                          # PIVLFN_DCT_MAX
DEFAULT_WAVELENGTH = 8.0
UNKNOWN_VALUE = 1e10                                     # what an EMPTY frame reads back as


def _is_real(x) -> bool:
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool) and math.isfinite(x)


def smooth_param(wavelength) -> float:
    """The s at which a 1-D wave of `wavelength` pixels keeps half its amplitude: 1 / (2 - 2 cos(2 pi / wavelength))^2."""
    if not _is_real(wavelength) or not wavelength > 2:
        raise ValueError(f"smooth_param: wavelength={wavelength!r} must be finite and above 2 pixels (the shortest wave a grid holds)")
    lam = 2.0 - 2.0 * math.cos(2.0 * math.pi / float(wavelength))
    return 1.0 / (lam * lam)


def smooth_wavelength(s) -> float:
    """The inverse of smooth_param: the wavelength that s halves."""
    if not _is_real(s) or not s > 0:
        raise ValueError(f"smooth_wavelength: s={s!r} must be finite and positive")
    lam = 1.0 / math.sqrt(float(s))
    if lam >= 4.0:
        raise ValueError(f"smooth_wavelength: s={s!r} halves no wave a grid holds (s must be above 1/16)")
    return 2.0 * math.pi / math.acos(1.0 - lam / 2.0)


def check_params(s=None, wavelength=DEFAULT_WAVELENGTH, tol=1e-8, max_iter=None, sync_every=64) -> float:
    """The parameter checks of smooth_flow (ValueError), usable before any tensor exists.  Returns the s in effect: `s` itself, beside
    which `wavelength` must be None or left at its default, or smooth_param(wavelength)."""
    if s is not None and wavelength is not None and wavelength != DEFAULT_WAVELENGTH:
        raise ValueError(f"smooth_flow: s={s!r} and wavelength={wavelength!r} are alternatives, give one of them")
    if s is None and wavelength is None:
        raise ValueError("smooth_flow: one of s and wavelength is required")
    if s is not None:
        if not _is_real(s) or not s > 0:
            raise ValueError(f"smooth_flow: s={s!r} must be finite and positive")
    elif not _is_real(wavelength) or not wavelength > 2:
        raise ValueError(f"smooth_flow: wavelength={wavelength!r} must be finite and above 2 pixels")
    if not _is_real(tol) or not tol > 0:
        raise ValueError(f"smooth_flow: tol={tol!r} must be finite and positive")
    if max_iter is not None and (not _args.is_integer(max_iter) or max_iter < 0):
        raise ValueError(f"smooth_flow: max_iter={max_iter!r} must be a non-negative integer or None")
    if sync_every is not None and (not _args.is_integer(sync_every) or sync_every < 1):
        raise ValueError(f"smooth_flow: sync_every={sync_every!r} must be a positive integer or None")
    return float(s) if s is not None else smooth_param(wavelength)


def check_size(B, H, W, what: str = "smooth_flow") -> None:
    if H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{what}: {H} x {W} vectors, a side must be 1..{MAX_SIDE}")
    if B < 1 or B > 32767 or 2 * B * H * W >= 1 << 31:
        raise ValueError(f"{what}: {B} frames of {H} x {W} vectors in one call, must be 1..32767 frames and stay below 2^31 values")


class Smoothed:
    """What smooth_flow returns.  The device tensors are what the kernels wrote:
        flow [B,2,H,W] float32, z [B,2,H,W] float64 (the same before rounding), filled [B,H,W] bool (the vector had weight 0: masked,
        unknown, or a weight that is not positive and finite), status [B,2,4] float64 (state, iterations, rr, bb per component).
    Derived from status on the host on first use (which synchronises):
        iterations [B,2] int;  residual [B,2] = sqrt(rr/bb), 0 where rr = 0;  state [B,2] int (RUNNING, CONVERGED, BREAKDOWN, EMPTY)
        converged  [B,2] bool: the stopping rule rr <= tol^2 bb holds, or the frame is EMPTY (nothing to solve: it reads back as 1e10);
                   False for a system that hit max_iter first."""

    def __init__(self, flow, z, filled, status, s: float, tol: float, max_iter: int):
        self.flow, self.z, self.filled, self.status = flow, z, filled, status
        self.s, self.tol, self.max_iter = s, tol, max_iter
        self._host: Dict[str, np.ndarray] = {}

    def __len__(self) -> int:
        return int(self.z.shape[0])

    def _get(self, key):
        if not self._host:
            st = self.status.cpu().numpy()
            rr, bb, state = st[..., 2], st[..., 3], st[..., 0].astype(np.int64)
            with np.errstate(invalid="ignore", divide="ignore"):
                residual = np.where(rr == 0, 0.0, np.sqrt(rr / bb))
            converged = (rr <= (self.tol * self.tol) * bb) | (state == EMPTY)
            self._host = {"state": state, "iterations": st[..., 1].astype(np.int64), "residual": residual, "converged": converged}
        return self._host[key]

    state = property(lambda self: self._get("state"))
    iterations = property(lambda self: self._get("iterations"))
    residual = property(lambda self: self._get("residual"))
    converged = property(lambda self: self._get("converged"))

    def summary(self) -> Dict[str, object]:
        """JSON-ready: the parameters, per frame summarize()'s record, and the count of unconverged frames."""
        frames = summarize(self.status.cpu().numpy(), self.filled.flatten(1).sum(1).tolist(), self.tol)
        return {"s": self.s, "tol": self.tol, "max_iter": self.max_iter, "frames": frames,
                "unconverged": int(sum(not fr["converged"] for fr in frames))}


def summarize(status: np.ndarray, filled, tol: float):
    """Per frame of a host `status` [B,2,4] and its count of filled vectors: the filled vectors, the iterations and the residual (the
    larger of u's and v's), converged (both components, as Smoothed.converged) and whether the frame was EMPTY."""
    rr, bb, state = status[..., 2], status[..., 3], status[..., 0].astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        residual = np.where(rr == 0, 0.0, np.sqrt(rr / bb))
    converged = (rr <= (tol * tol) * bb) | (state == EMPTY)
    return [{"filled": int(filled[f]), "iterations": int(status[f, :, 1].max()), "residual": float(residual[f].max()),
             "converged": bool(converged[f].all()), "empty": bool((state[f] == EMPTY).all())} for f in range(len(status))]


def smooth_flow(flow: torch.Tensor, s: Optional[float] = None, wavelength: Optional[float] = DEFAULT_WAVELENGTH, weights: Optional[torch.Tensor] = None,
                mask: Optional[torch.Tensor] = None, tol: float = 1e-8, max_iter: Optional[int] = None,
                sync_every: Optional[int] = 64) -> Smoothed:
    """Smooths `flow` [B,2,H,W] (float32, on the GPU) and fills its gaps in one solve per frame and component.

    s / wavelength: alternatives; giving both is a ValueError (a wavelength left at its default counts as not given).  The default halves waves of 8 pixels.
    weights [B,H,W] float32: the confidence of each vector, of order 1 (the preconditioner is the problem with unit weights: the
        iteration count grows as the weights leave that order; weights_from_uncertainty keeps them in (0, 1]).
    mask [B,H,W] uint8 or bool: nonzero = the vector is a gap (validate_flow's flag).
    A vector is a gap as well if either component is NaN or beyond 1e9 (the package's unknown rule, validate_flow's 1e10 included) or
    its weight is not positive and finite; the value of a gap is never read into arithmetic.  A frame that is all gaps is EMPTY and
    comes back as 1e10.

    The iterations are enqueued `sync_every` at a time and the states are read in between, which synchronises the host;
    `sync_every=None` enqueues all max_iter iterations and reads nothing.  A system that has stopped does not move again, so both ways
    give the same bits, and a frame's bits do not depend on the batch.  max_iter defaults to 10*max(H, W) + 50: a cap, not a tuning; a
    system that reaches it is reported with converged = False."""
    s = check_params(s, wavelength, tol, max_iter, sync_every)
    flow = _args.check_flows(flow, "smooth_flow")
    B, _, H, W = (int(n) for n in flow.shape)
    check_size(B, H, W)
    dev = flow.device
    mask = _args.check_mask(mask, "smooth_flow", shape=(B, H, W), device=dev)
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32:
            raise TypeError(f"smooth_flow: expected float32 weights [B,H,W], got "
                            f"{weights.dtype if isinstance(weights, torch.Tensor) else type(weights).__name__}")
        if weights.device != dev or tuple(weights.shape) != (B, H, W):
            raise ValueError(f"smooth_flow: weights {tuple(weights.shape)} on {weights.device} do not belong to flows {tuple(flow.shape)} on {dev}")
        weights = weights.detach().contiguous()
    cap = 10 * max(H, W) + 50 if max_iter is None else int(max_iter)
    z = torch.empty([B, 2, H, W], dtype=torch.float64, device=dev)
    z32 = torch.empty([B, 2, H, W], dtype=torch.float32, device=dev)
    filled = torch.empty([B, H, W], dtype=torch.uint8, device=dev)
    status = torch.empty([B, 2, 4], dtype=torch.float64, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        st = _lib.stream_ptr(dev)
        nbytes = lib.pivlfn_smooth_workspace_bytes(B, H, W)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

        def step(n):
            _lib.check(lib.pivlfn_smooth_pcg(ws.data_ptr(), nbytes, B, H, W, s, float(tol), n, st), "smooth_flow: pcg")

        def read():
            _lib.check(lib.pivlfn_smooth_read(ws.data_ptr(), nbytes, B, H, W, z.data_ptr(), z32.data_ptr(), filled.data_ptr(), status.data_ptr(),
                                              st), "smooth_flow: read")

        _lib.check(lib.pivlfn_smooth_setup(flow.data_ptr(), _args.ptr(weights), _args.ptr(mask), B, H, W, s, ws.data_ptr(), nbytes, st),
                   "smooth_flow: setup")
        _args.run_iterations(step, read, status, cap, sync_every)
    return Smoothed(z32, z, filled.bool(), status, s, float(tol), cap)


def weights_from_uncertainty(unc, floor: float) -> torch.Tensor:
    """[B,H,W] float32 weights from flow_uncertainty's result: min(1, (floor/|u|)^2) with |u| the magnitude of the uncertainty vector,
    0 where its flag says the estimate is unusable.  A vector at least as certain as `floor` (pixels) gets weight 1, so the weights stay
    of order 1, which the preconditioner of smooth_flow assumes."""
    floor = _args.check_not_negative("weights_from_uncertainty", "floor", floor)
    if floor == 0.0:
        raise ValueError("weights_from_uncertainty: floor=0.0 must be positive")
    if unc.u.dim() != 4 or unc.u.size(1) != 2:
        raise ValueError(f"weights_from_uncertainty: expected a FlowUncertainty with u [B,2,H,W], got {tuple(unc.u.shape)}")
    mag = unc.magnitude()
    usable = (unc.flag & UNUSABLE).eq(0) & torch.isfinite(mag)
    w = torch.where(mag > floor, (floor / mag) ** 2, torch.ones_like(mag))
    return torch.where(usable, w, torch.zeros_like(w)).to(torch.float32).contiguous()


def dct2(x: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """The orthonormal 2-D DCT-II (scipy.fft.dctn(norm="ortho")) of float64 planes [..., H, W] on the GPU, or its inverse: two fp64
    matrix products per plane on the matrix cores.  A plane's bits do not depend on the others."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"dct2: expected a torch tensor [..., H, W], got {type(x).__name__}")
    if x.dtype != torch.float64:
        raise TypeError(f"dct2: expected float64, got {x.dtype}")
    if not x.is_cuda:
        raise NotImplementedError("dct2: GPU tensors only")
    if x.dim() < 2:
        raise ValueError(f"dct2: expected [..., H, W], got {tuple(x.shape)}")
    H, W = int(x.shape[-2]), int(x.shape[-1])
    P = int(x.numel() // max(H * W, 1))
    if H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"dct2: {H} x {W} values, a side must be 1..{MAX_SIDE}")
    if P < 1 or P > 65535 or P * H * W >= 1 << 31:
        raise ValueError(f"dct2: {P} planes of {H} x {W} values in one call, must be 1..65535 planes and stay below 2^31 values")
    x = x.detach().contiguous()
    out = torch.empty_like(x)
    _args.call_with_workspace("dct2", x.device, (P, H, W), x.data_ptr(), out.data_ptr(), P, H, W, 1 if inverse else 0)
    return out
