"""Lagrangian flow maps of a flow sequence on the device: particles carried through consecutive displacement fields (pathlines, the
flow map) and the finite-time Lyapunov exponent (FTLE) of the map, whose ridges are the Lagrangian coherent structures -- the
material lines the vortices of `vortex_gamma` sit between.  Everything else the package computes from a flow is Eulerian and per
pair; this uses the fact that flow k+1 follows flow k.

An estimated flow is a displacement field: F_k(x) is where the content at pixel x of frame k sits in frame k+1.  The flow map over an
interval is therefore x -> x + F_k(x) composed over k: one bilinear sample per particle and field, no velocities, no integrator.

Runs on csrc/flowmap.hip through the C ABI (`pivlfn_flowmap_advect`, `pivlfn_flowmap_seed`, `pivlfn_flowmap_ftle`; the arithmetic
contract is written out in include/pivlfn.h):

    fm = FlowMap(H, W, spacing=2)                              # seeds every second pixel
    for flows in batches:                                      # [B,2,H,W] float32 on the device, consecutive in time
        fm.update(flows, mask=flags)                           # one launch per batch
    field = fm.ftle()                                          # field.ftle [h,w] float32, NaN where undefined
    print(field.summary())
    paths = FlowMap(H, W, points=xy).update(flows, trace=True) # [B,2,N]: pathlines of chosen particles

A particle that leaves the image (OUT) or meets a masked or unknown vector (LOST) is frozen where it was.  `backward=True` follows
the fluid back in time (pass the fields newest first): each step solves p + F_k(p) = x by `iters` fixed-point iterations.  Every
operation is a correctly rounded float64 operation in a fixed order: a sequence gives the same bits however it is cut into batches.
GPU only, like the rest of the package: there is no CPU path.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional, Tuple

import torch

from . import _accum, _args, _lib

OUT, LOST, UNDEFINED = 1, 2, 4          # the bits of a flag byte (PIVLFN_FLOWMAP_*)


def check_params(H, W, spacing=1, iters=8) -> Tuple[int, int]:
    """The parameter checks of FlowMap (ValueError), usable before any tensor exists; H and W may be None where the frame size is not
    known yet.  Returns the lattice size (h, w) -- (None, None) without a frame size."""
    _args.check_int("FlowMap", "spacing", spacing, 1, 32768, ", the distance between seeds in pixels")
    _args.check_int("FlowMap", "iters", iters, 1, 32, ", the fixed-point iterations of a backward step")
    if H is None and W is None:
        return None, None
    for name, v in (("H", H), ("W", W)):
        if not _args.is_int(v, 2):
            raise ValueError(f"FlowMap: {name}={v!r} must be an integer >= 2 (a bilinear sample needs 2 x 2 vectors)")
    if H * W >= 1 << 31:
        raise ValueError(f"FlowMap: H*W={H * W} pixels, must stay below 2^31")
    return (H - 1) // spacing + 1, (W - 1) // spacing + 1


class FTLEField(NamedTuple):
    """What FlowMap.ftle() returns, on the seed lattice [h,w]."""
    ftle: torch.Tensor            # float32: log(stretch) / steps; NaN where UNDEFINED is set
    stretch: torch.Tensor         # float64: the largest singular value of the flow map's gradient; NaN where UNDEFINED is set
    flag: torch.Tensor            # uint8: the node's own OUT | LOST, and UNDEFINED
    steps: int                    # the fields the map spans
    spacing: int                  # the distance between seeds in pixels

    def summary(self) -> Dict[str, float]:
        """The shares of OUT, LOST and UNDEFINED nodes, the number of defined ones, and the largest and the mean FTLE over them (NaN
        where there is none).  Plain torch in float64; copies the numbers to the host."""
        n = self.flag.numel()
        defined = (self.flag & UNDEFINED).eq(0)
        f = self.ftle.to(torch.float64)
        zero = torch.zeros((), dtype=torch.float64, device=f.device)
        row = torch.stack([(self.flag & OUT).ne(0).sum().to(torch.float64), (self.flag & LOST).ne(0).sum().to(torch.float64),
                           defined.sum().to(torch.float64), torch.where(defined, f, zero).sum(),
                           torch.where(defined, f, torch.full_like(zero, -math.inf)).max() if n else zero]).cpu().tolist()
        out, lost, nd, total, top = row
        share = (lambda k: k / n) if n else (lambda k: math.nan)
        return {"out": share(out), "lost": share(lost), "undefined": share(n - nd), "defined": int(nd),
                "max_ftle": top if nd else math.nan, "mean_ftle": total / nd if nd else math.nan}


class FlowMap:
    """Particles and the flow map they trace through the flows given to update().

    Without `points`: one particle per node of the lattice (j*spacing, i*spacing), h = (H-1)//spacing + 1 rows and w likewise columns;
    `positions` is [2,h,w] (x plane, y plane) and ftle() is available.  With `points` [N,2] (x, y): those particles, `positions` is
    [2,N], and ftle() raises.  `flag` ([h,w] or [N] uint8: OUT | LOST) and `steps` (the fields passed so far) are attributes; the
    tensors are the live state, updated in place.  Everything is enqueued on the current stream; nothing synchronises the host."""

    def __init__(self, H: int, W: int, spacing: int = 1, points=None, backward: bool = False, iters: int = 8, device="cuda"):
        self.h, self.w = check_params(H, W, spacing, iters)
        self.H, self.W, self.spacing, self.backward, self.iters = H, W, spacing, bool(backward), iters
        self.device = _accum.cuda_device(device, "FlowMap: GPU only")
        self._points = None
        if points is not None:
            pts = torch.as_tensor(points)
            if pts.dim() != 2 or pts.size(1) != 2 or not (pts.is_floating_point() or pts.numel() == 0):
                raise ValueError(f"FlowMap: points must be floating point [N,2] (x, y), got {tuple(pts.shape)} of {pts.dtype}")
            self._points = pts.detach().to(self.device, torch.float64).t().contiguous()          # [2,N]
        self.N = self.h * self.w if self._points is None else self._points.size(1)
        if self.N >= 1 << 31:
            raise ValueError(f"FlowMap: {self.N} particles, must stay below 2^31")
        self._pos = torch.empty([2, self.N], dtype=torch.float64, device=self.device)
        self._flag = torch.empty([self.N], dtype=torch.uint8, device=self.device)
        self.steps = 0
        self.reset()

    @property
    def lattice(self) -> bool:
        return self._points is None

    @property
    def positions(self) -> torch.Tensor:
        return self._pos.view(2, self.h, self.w) if self.lattice else self._pos

    @property
    def flag(self) -> torch.Tensor:
        return self._flag.view(self.h, self.w) if self.lattice else self._flag

    def reset(self) -> None:
        """Back to the seeds, all flags clear, steps = 0."""
        self.steps = 0
        if not self.lattice:
            self._pos.copy_(self._points)
            self._flag.zero_()
            return
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pivlfn_flowmap_seed(self._pos.data_ptr(), self._flag.data_ptr(), self.h, self.w, self.spacing,
                                                       _lib.stream_ptr(self.device)), "FlowMap.reset")

    def update(self, flow: torch.Tensor, mask: Optional[torch.Tensor] = None, trace: bool = False) -> Optional[torch.Tensor]:
        """Carries every particle through [B,2,H,W] float32 flows that are consecutive in time -- ascending, or descending with
        `backward` -- in one launch, and adds B to `steps`.  `mask` [B,H,W] uint8 or bool: nonzero vectors are not to be used (the flag
        of validate_flow); unknown vectors (NaN, inf, 1e10) are left out by themselves.  With `trace`: returns the positions after
        every field, [B,2,h,w] or [B,2,N] float64."""
        flow = _args.check_flows(flow, "FlowMap.update")
        mask = _args.check_mask(mask, "FlowMap.update", truth=flow)
        B = flow.size(0)
        if tuple(flow.shape[2:]) != (self.H, self.W) or flow.device != self.device:
            raise ValueError(f"FlowMap.update: flows {tuple(flow.shape)} on {flow.device} do not belong to a map of {self.H} x {self.W} "
                             f"on {self.device}")
        path = torch.empty([B, 2, self.N], dtype=torch.float64, device=self.device) if trace else None
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pivlfn_flowmap_advect(flow.data_ptr(), mask.data_ptr() if mask is not None else None, B, self.H, self.W,
                                                         self._pos.data_ptr(), self._flag.data_ptr(), self.N, int(self.backward),
                                                         self.iters, path.data_ptr() if trace else None,
                                                         _lib.stream_ptr(self.device)), "FlowMap.update")
        self.steps += B
        if not trace:
            return None
        return path.view(B, 2, self.h, self.w) if self.lattice else path

    def ftle(self) -> FTLEField:
        """The FTLE of the map so far: log(stretch) / steps with the stretch of pivlfn_flowmap_ftle (float64 on the lattice), formed
        in float64 and stored as float32."""
        if not self.lattice:
            raise ValueError("FlowMap.ftle: needs the seed lattice; this map carries a particle list")
        if self.steps == 0:
            raise ValueError("FlowMap.ftle: no flow has been passed yet (steps == 0)")
        stretch = torch.empty([self.h, self.w], dtype=torch.float64, device=self.device)
        oflag = torch.empty([self.h, self.w], dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pivlfn_flowmap_ftle(self._pos.data_ptr(), self._flag.data_ptr(), self.h, self.w, self.spacing,
                                                       stretch.data_ptr(), oflag.data_ptr(), _lib.stream_ptr(self.device)), "FlowMap.ftle")
        return FTLEField((torch.log(stretch) / self.steps).to(torch.float32), stretch, oflag, self.steps, self.spacing)
