"""Pressure from time-resolved planar PIV on the device: the material acceleration of three consecutive flows by central differences
(Eulerian) and the least-squares integration of the pressure gradient over the valid nodes -- the Poisson problem of the graph
Laplacian with the natural Neumann boundary on any mask shape -- by Jacobi-preconditioned conjugate gradients.

The kernels are csrc/pressure.hip behind the C ABI (`pivlfn_pressure_gradient`, `_setup`, `_cg`, `_read`; the arithmetic contract is
written out in include/pivlfn.h).  They work in lattice units (px, frame); only this layer knows units:

    pf = PressureField(H, W, cell=4, calib=1e-4, dt=1e-3, rho=1000.0, nu=1e-6)     # calib: length per pixel, dt: time per frame
    for flows in chunks:                                      # a time-resolved sequence, in order
        res = pf.update(flows, mask)                          # the frames this call completed: centred on every flow with both neighbours
        res.p, res.grad, res.flag                             # [F,ch,cw] pressure, [F,2,ch,cw] its gradient, 0 = ok / INVALID / ISOLATED
        res.iterations, res.residual, res.converged           # per frame; a frame that hit max_iter is reported, never hidden

With p* the solution in lattice units, p = rho (calib/dt)^2 p* and nu* = nu dt / calib^2; the lattice spacing is s = cell.  The solver
leaves every connected region with zero DEGREE-WEIGHTED mean; `p` is re-referenced per frame to zero plain mean over its ok nodes, or to
the value at `reference=(j, i)`.  The levels of disconnected regions are unrelated.

Limits: planar data only, the out-of-plane terms are neglected;  the Eulerian derivative amplifies noise as dt falls (a pseudo-Lagrangian
acceleration from FlowMap is the follow-up);  no multigrid and no warm start: a frame starts from x = 0, so its bits do not depend on how
the sequence is cut into update() calls.  GPU only, like the rest of the package: there is no CPU path."""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _accum, _args, _lib, viz

RUNNING, CONVERGED, BREAKDOWN = 1, 2, 3                  # PIVLFN_PRESSURE_*: the state of a frame
OK, INVALID, ISOLATED = 0, 1, 2                          # the flag of a node
WS_B, WS_X, WS_ADJ = 0, 1, 2


def _is_real(x) -> bool:
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool) and math.isfinite(x)


def check_params(cell=4, calib=1.0, dt=1.0, rho=1.0, nu=0.0, tol=1e-8, max_iter=None, sync_every=64) -> None:
    """The parameter checks of PressureField (ValueError), usable before any tensor exists."""
    if not _args.is_integer(cell) or not 1 <= cell <= 32768:
        raise ValueError(f"PressureField: cell={cell!r} must be an integer from 1 to 32768, the pixels per lattice node")
    for name, v in (("calib", calib), ("dt", dt), ("rho", rho), ("tol", tol)):
        if not _is_real(v) or not v > 0:
            raise ValueError(f"PressureField: {name}={v!r} must be finite and positive")
    if not _is_real(nu) or nu < 0:
        raise ValueError(f"PressureField: nu={nu!r} must be finite and not negative")
    if max_iter is not None and (not _args.is_integer(max_iter) or max_iter < 0):
        raise ValueError(f"PressureField: max_iter={max_iter!r} must be a non-negative integer or None")
    if sync_every is not None and (not _args.is_integer(sync_every) or sync_every < 1):
        raise ValueError(f"PressureField: sync_every={sync_every!r} must be a positive integer or None")


def check_size(H, W, cell=4) -> Tuple[int, int]:
    """(ch, cw), the lattice of an H x W flow."""
    if not _args.is_integer(H) or not _args.is_integer(W) or H < 1 or W < 1:
        raise ValueError(f"PressureField: bad flow size {H!r} x {W!r}")
    ch, cw = -(-int(H) // cell), -(-int(W) // cell)
    if ch * cw >= 1 << 31:
        raise ValueError(f"PressureField: a lattice of {ch} x {cw} nodes, must stay below 2^31")
    return ch, cw


def _check_reference(reference, ch, cw):
    if reference is None:
        return None
    if (not isinstance(reference, (tuple, list)) or len(reference) != 2 or not all(_args.is_integer(k) for k in reference)
            or not (0 <= reference[0] < ch and 0 <= reference[1] < cw)):
        raise ValueError(f"PressureField: reference={reference!r} must be a node (j, i) of the {ch} x {cw} lattice")
    return int(reference[0]), int(reference[1])


class PressureResult:
    """The frames one update() completed.  The device tensors are what the kernels wrote, in lattice units:
        p_star [F,ch,cw] float64 (NaN where the node is not ok), g [F,2,ch,cw] float64, flag [F,ch,cw] uint8, status [F,4] float64
        (state, iterations, rr, bb).
    Everything else is derived from them on the host on first use (which synchronises), frame by frame, so it does not depend on the
    batch either:
        p          [F,ch,cw] float64 = rho (calib/dt)^2 (p* - its reference), NaN where not ok;  the reference is the plain mean over
                   the frame's ok nodes, or the value at `reference` (NaN everywhere if that node is not ok)
        grad       [F,2,ch,cw] float64 = rho calib/dt^2 g: pressure per unit length, +0.0 where the node is invalid
        iterations [F] int;  residual [F] = sqrt(rr/bb), 0 where rr = 0;  state [F] int
        converged  [F] bool: the stopping rule rr <= tol^2 bb holds (a frame with b = 0 ends as BREAKDOWN with x = 0, its exact
                   solution: converged);  False for a frame that hit max_iter first."""

    def __init__(self, p_star, g, flag, status, scale_p: float, scale_g: float, tol: float, reference=None):
        self.p_star, self.g, self.flag_dev, self.status = p_star, g, flag, status
        self.scale_p, self.scale_g, self.tol, self.reference = scale_p, scale_g, tol, reference
        self._host: Dict[str, np.ndarray] = {}

    def __len__(self) -> int:
        return int(self.p_star.shape[0])

    def _get(self, key):
        if not self._host:
            st = self.status.cpu().numpy()
            ps, flag = self.p_star.cpu().numpy(), self.flag_dev.cpu().numpy()
            p = np.full_like(ps, np.nan)
            for f in range(len(ps)):
                ok = flag[f] == OK
                if self.reference is not None:
                    ref = ps[f][self.reference] if ok[self.reference] else np.nan
                else:
                    ref = ps[f][ok].mean() if ok.any() else np.nan
                p[f][ok] = self.scale_p * (ps[f][ok] - ref)
            rr, bb = st[:, 2], st[:, 3]
            with np.errstate(invalid="ignore", divide="ignore"):
                residual = np.where(rr == 0, 0.0, np.sqrt(rr / bb))
                converged = rr <= (self.tol * self.tol) * bb
            self._host = {"p": p, "flag": flag, "grad": self.scale_g * self.g.cpu().numpy(), "state": st[:, 0].astype(np.int64),
                          "iterations": st[:, 1].astype(np.int64), "residual": residual, "converged": converged}
        return self._host[key]

    p = property(lambda self: self._get("p"))
    grad = property(lambda self: self._get("grad"))
    flag = property(lambda self: self._get("flag"))
    state = property(lambda self: self._get("state"))
    iterations = property(lambda self: self._get("iterations"))
    residual = property(lambda self: self._get("residual"))
    converged = property(lambda self: self._get("converged"))

    def summary(self) -> Dict[str, object]:
        """JSON-ready: per frame the ok / invalid / isolated nodes, iterations, residual, converged and the min / max / rms of p over
        the ok nodes (None where there is none), and the count of unconverged frames."""
        frames = []
        for f in range(len(self)):
            flag, p = self.flag[f], self.p[f]
            ok = flag == OK
            v = p[ok]
            have = v.size > 0 and np.isfinite(v).all()
            frames.append({"ok": int(ok.sum()), "invalid": int((flag == INVALID).sum()), "isolated": int((flag == ISOLATED).sum()),
                           "iterations": int(self.iterations[f]), "residual": float(self.residual[f]), "converged": bool(self.converged[f]),
                           "p_min": float(v.min()) if have else None, "p_max": float(v.max()) if have else None,
                           "p_rms": float(np.sqrt(np.mean(v * v))) if have else None})
        return {"frames": frames, "unconverged": int(sum(not fr["converged"] for fr in frames))}


class PressureField:
    """Pressure fields of a time-resolved flow sequence of one size.  update() decimates the flows to cell means (viz.decimate_flow: a
    cell without a known vector is 1e10, which the gradient kernel treats as unknown), keeps the last two decimated flows as a halo and
    solves one frame for every flow that has both neighbours.  The conjugate-gradient iterations are enqueued `sync_every` at a time and
    the states are read in between, which synchronises the host; `sync_every=None` enqueues all max_iter iterations and reads nothing.  A
    frame that has stopped does not move again, so both ways give the same bits.  max_iter defaults to 10*max(ch, cw) + 50: a cap, not a
    tuning; a frame that reaches it is reported with converged = False."""

    def __init__(self, H: int, W: int, cell: int = 4, calib: float = 1.0, dt: float = 1.0, rho: float = 1.0, nu: float = 0.0, tol: float = 1e-8,
                 max_iter: Optional[int] = None, sync_every: Optional[int] = 64, device=None, reference=None):
        check_params(cell, calib, dt, rho, nu, tol, max_iter, sync_every)
        self.ch, self.cw = check_size(H, W, cell)
        self.reference = _check_reference(reference, self.ch, self.cw)
        self.H, self.W, self.cell = int(H), int(W), int(cell)
        self.calib, self.dt, self.rho, self.nu, self.tol = float(calib), float(dt), float(rho), float(nu), float(tol)
        self.max_iter = 10 * max(self.ch, self.cw) + 50 if max_iter is None else int(max_iter)
        self.sync_every = sync_every
        self.nu_star = self.nu * self.dt / (self.calib * self.calib)
        self.device = _accum.cuda_device(device, "PressureField: GPU devices only")
        self.halo = torch.empty([0, 2, self.ch, self.cw], dtype=torch.float32, device=self.device)
        self.count = 0                                    # frames solved so far

    def solve(self, seq: torch.Tensor) -> PressureResult:
        """The frames of `seq` [B,2,ch,cw] (float32 lattice flows, B >= 3 or no frame results), without touching the halo."""
        B = int(seq.shape[0])
        F, ch, cw, dev = max(B - 2, 0), self.ch, self.cw, self.device
        g = torch.empty([F, 2, ch, cw], dtype=torch.float64, device=dev)
        valid = torch.empty([F, ch, cw], dtype=torch.uint8, device=dev)
        p = torch.empty([F, ch, cw], dtype=torch.float64, device=dev)
        flag = torch.empty([F, ch, cw], dtype=torch.uint8, device=dev)
        status = torch.empty([F, 4], dtype=torch.float64, device=dev)
        if F > 0:
            if F * ch * cw >= 1 << 31:
                raise ValueError(f"PressureField: {F} frames of {ch} x {cw} nodes in one call, must stay below 2^31 nodes")
            lib = _lib.load()
            with torch.cuda.device(dev):
                st = _lib.stream_ptr(dev)
                nbytes = lib.pivlfn_pressure_workspace_bytes(F, ch, cw)
                ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                _lib.check(lib.pivlfn_pressure_gradient(seq.data_ptr(), B, ch, cw, float(self.cell), self.nu_star, g.data_ptr(), valid.data_ptr(),
                                                        st), "PressureField: gradient")
                _lib.check(lib.pivlfn_pressure_setup(g.data_ptr(), valid.data_ptr(), F, ch, cw, float(self.cell), ws.data_ptr(), nbytes, st),
                           "PressureField: setup")

                def step(n):
                    _lib.check(lib.pivlfn_pressure_cg(ws.data_ptr(), nbytes, F, ch, cw, self.tol, n, st), "PressureField: cg")

                def read():
                    _lib.check(lib.pivlfn_pressure_read(ws.data_ptr(), nbytes, F, ch, cw, p.data_ptr(), flag.data_ptr(), status.data_ptr(), st),
                               "PressureField: read")

                _args.run_iterations(step, read, status, self.max_iter, self.sync_every)
        scale_p = self.rho * (self.calib / self.dt) ** 2
        return PressureResult(p, g, flag, status, scale_p, self.rho * self.calib / (self.dt * self.dt), self.tol, self.reference)

    def update(self, flows: torch.Tensor, mask: Optional[torch.Tensor] = None) -> PressureResult:
        """The next flows of the sequence, [B,2,H,W] float32 on this device, in order; `mask` [B,H,W]: nonzero = leave the vector out.
        Returns the frames this call completed (none while fewer than three flows have been seen)."""
        if not isinstance(flows, torch.Tensor) or flows.dim() != 4 or tuple(flows.shape[1:]) != (2, self.H, self.W) or flows.device != self.device:
            shape = tuple(flows.shape) if isinstance(flows, torch.Tensor) else type(flows).__name__
            raise ValueError(f"PressureField.update: flows {shape}, expected [B,2,{self.H},{self.W}] on {self.device}")
        dec, _ = viz.decimate_flow(flows, self.cell, mask)
        seq = torch.cat([self.halo, dec]) if len(self.halo) else dec
        res = self.solve(seq.contiguous())
        self.halo = seq[-2:].clone()
        self.count += len(res)
        return res
