"""Post-processing of estimated flows: the reference's src/postpro.py (`calc_vorticity`, `de_vort`) and streaming statistics
of a flow sequence (mean velocity, RMS fluctuation, Reynolds stress, mean and RMS vorticity).

Both run on csrc/postpro.hip through the C ABI (`pivlfn_flow_fields`, `pivlfn_flow_stats_accumulate`; the arithmetic contract is
written out in include/pivlfn.h):

    vort, shear, normal = calc_vorticity(flow_hw2, calib)      # numpy drop-ins, bit-identical to the reference (float64 [H,W])
    vort, uy, vx = de_vort(flow_hw2, calib)
    fields = flow_fields(flows, calib, kind="de_vort")         # batched: [B,2,H,W] on the device -> [B,3,H,W]

    stats = FlowStats(H, W, calib, device)
    for flows in chunks: stats.update(flows)                   # enqueued on the current stream, no host synchronisation
    stats.merge()                                              # collective: every rank ends with the sums of all ranks
    stats.save("stats.npz")                                    # result() fields + the raw accumulators + calib

GPU only, like the rest of the package: there is no CPU path.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _accum, _args, _lib

KINDS = {"calc_vorticity": 0, "de_vort": 1}          # PIVLFN_FIELDS_CALC_VORTICITY, PIVLFN_FIELDS_DE_VORT
PLANES = {"calc_vorticity": ("vort", "shear", "normal"), "de_vort": ("vort", "uy", "vx")}
SUMS = ("sum_u", "sum_v", "sum_uu", "sum_vv", "sum_uv", "sum_w", "sum_ww")     # the planes of FlowStats.acc, in order
RESULT = ("count", "mean_u", "mean_v", "rms_u", "rms_v", "cov_uv", "mean_vort", "rms_vort")


def flow_fields(flow: torch.Tensor, calib=1.0, kind: str = "calc_vorticity", dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """[B,2,H,W] float32 flows on the device -> [B,3,H,W] of `dtype` (float32 or float64), enqueued on the current stream.
    kind "calc_vorticity": planes vort, shear, normal; "de_vort": vort, uy, vx (PLANES).  float32 output is the float64 result
    rounded once."""
    if kind not in KINDS:
        raise ValueError(f"flow_fields: unknown kind {kind!r} (one of {', '.join(KINDS)})")
    if dtype not in (torch.float32, torch.float64):
        raise TypeError(f"flow_fields: dtype must be torch.float32 or torch.float64, got {dtype}")
    flow = _args.check_flows(flow, "flow_fields")
    B, _, H, W = flow.shape
    out = torch.empty([B, 3, H, W], dtype=dtype, device=flow.device)
    if B == 0:
        return out
    with torch.cuda.device(flow.device):
        _lib.check(_lib.load().pivlfn_flow_fields(flow.data_ptr(), out.data_ptr(), B, H, W, _args.check_calib(calib), KINDS[kind],
                                                  int(dtype == torch.float64), _lib.stream_ptr(flow.device)), "flow_fields")
    return out


def _fields_hw(flow, calib, kind: str):
    """The numpy drop-ins: [H,W,C>=2] float32 (what estimate and read_flow return) -> three float64 [H,W] arrays."""
    if not isinstance(flow, np.ndarray) or flow.dtype != np.float32:
        raise TypeError(f"{kind}: expected a float32 numpy flow [H,W,2], got "
                        f"{flow.dtype if isinstance(flow, np.ndarray) else type(flow).__name__} (converting it would change the "
                        "reference's values)")
    if flow.ndim != 3 or flow.shape[2] < 2:
        raise ValueError(f"{kind}: expected a flow [H,W,2], got shape {flow.shape}")
    if not torch.cuda.is_available():
        raise NotImplementedError(f"{kind}: needs a GPU (there is no CPU path)")
    dev = _accum.cuda_device()
    t = torch.from_numpy(np.ascontiguousarray(flow[:, :, :2].transpose(2, 0, 1)))[None].to(dev)
    out = flow_fields(t, calib, kind, torch.float64)[0].cpu().numpy()
    return out[0], out[1], out[2]


def calc_vorticity(flow, calib: float = 1.0):
    """src/postpro.py:5-24: (vort, shear, normal), float64 [H,W], bit-identical to the reference; computed on the GPU."""
    return _fields_hw(flow, calib, "calc_vorticity")


def de_vort(flow, calib: float = 1.0):
    """src/postpro.py:27-50: (vort, uy, vx), float64 [H,W], bit-identical to the reference; computed on the GPU."""
    return _fields_hw(flow, calib, "de_vort")


def finalize(acc: np.ndarray, count: int) -> Dict[str, np.ndarray]:
    """Per-pixel statistics from the seven sums (SUMS order) of `count` frames: means, variances S2/N - mean^2 (ddof 0),
    rms = sqrt(max(var, 0)), cov_uv = Suv/N - mean_u*mean_v.  float64 [H,W] arrays and `count` (int64 scalar array)."""
    acc = np.asarray(acc, dtype=np.float64)
    if acc.ndim != 3 or acc.shape[0] != len(SUMS):
        raise ValueError(f"finalize: expected accumulators [7,H,W], got {acc.shape}")
    if count <= 0:
        raise ValueError("finalize: no frames accumulated")
    n = float(count)
    mu, mv, mw = acc[0] / n, acc[1] / n, acc[5] / n

    def rms(s2, m):
        return np.sqrt(np.maximum(s2 / n - m * m, 0.0))
    return {"count": np.array(count, dtype=np.int64), "mean_u": mu, "mean_v": mv, "rms_u": rms(acc[2], mu), "rms_v": rms(acc[3], mv),
            "cov_uv": acc[4] / n - mu * mv, "mean_vort": mw, "rms_vort": rms(acc[6], mw)}


class FlowStats(_accum.FrameAccumulator):
    """Per-pixel running sums over a flow sequence of one size: acc [7,H,W] float64 on the device (SUMS order) and the frame
    count.  update() enqueues one kernel on the current stream and never synchronises the host; result() / save() do."""

    def __init__(self, H: int, W: int, calib=1.0, device=None):
        self.calib = _args.check_calib(calib)
        super().__init__(H, W, device)
        self.acc = torch.zeros([len(SUMS), self.H, self.W], dtype=torch.float64, device=self.device)

    def update(self, flow: torch.Tensor) -> None:
        """Add the frames of `flow` [B,2,H,W] (float32, on this device), in batch order."""
        flow = _args.check_flows(flow, "FlowStats.update")
        self._check_mine(flow.shape[2:], flow.device, lambda: f"flows {tuple(flow.shape)} on {flow.device}")
        B = flow.size(0)
        self._enqueue(B, (_lib.load().pivlfn_flow_stats_accumulate, flow.data_ptr(), self.acc.data_ptr(), B, self.H, self.W, self.calib))

    def merge(self, group=None) -> None:
        """Collective over `group`: every rank ends with the accumulators of all ranks added in rank order (the same bits on every
        rank) and the summed count.  Under gloo the exchange runs on host copies, as dist.gather_flows does."""
        self.count = _accum.merge_sums([self.acc], self.count, group)

    def result(self) -> Dict[str, np.ndarray]:
        """finalize() of the current sums: count, mean_u, mean_v, rms_u, rms_v, cov_uv, mean_vort, rms_vort."""
        return finalize(self.acc.cpu().numpy(), self.count)

    def save(self, path: str, **extra) -> str:
        """An .npz with result()'s arrays, the raw accumulators (`acc`, SUMS order), `calib` and `extra`; returns the path written."""
        return _accum.save_npz(path, acc=self.acc.cpu().numpy(), calib=np.float64(self.calib), **extra, **self.result())
