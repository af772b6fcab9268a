"""Scoring of estimated flows against a known field on the device: average end-point error, RMSE, mean L1, bias and the largest error
per pair, the same per pyramid level and stage, and per-pixel bias / random-error maps of a sequence.

Runs on csrc/evaluate.hip through the C ABI (`pivlfn_flow_errors`, `pivlfn_level_errors`, `pivlfn_error_stats_accumulate`; the
arithmetic contract is written out in include/pivlfn.h):

    err = flow_errors(flows, truth)                            # [B,2,H,W] on the device; err.aee, err.rmse, err.bias, err.max
    flow, levels = net.forward_levels(img1, img2)
    table = level_errors(net, levels, truth, div_flow=1 / 5)   # table[i][s]: level 6 - i, stage s of (M, S, R), in level units

    stats = ErrorStats(H, W, device)
    for flows, truth in chunks: stats.update(flows, truth)     # enqueued on the current stream, no host synchronisation
    stats.save("error_maps.npz")

Every sum is formed in float64 in an order the contract fixes: a pair scores the same bits alone, in any batch and in any run.
GPU only, like the rest of the package: there is no CPU path.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import _accum, _args, _lib

FIELDS = ("n", "l1", "epe", "sq", "du", "dv", "max")         # the seven entries of a pair's sums, in order
STAGES = ("M", "S", "R")
ACC = ("count", "sum_du", "sum_dv", "sum_du2", "sum_dv2", "sum_epe")     # the planes of ErrorStats.acc, in order
RESULT = ("frames", "count", "bias_u", "bias_v", "rms_u", "rms_v", "mean_epe")


class FlowErrors(NamedTuple):
    """Per-pair float64 tensors [B] on the flows' device: the count of scored pixels, the sums over them of |du| + |dv|, the end-point
    error, its square, du and dv, and the largest end-point error (0 where nothing was scored).  `map` is [B,3,h,w] float32 (du, dv,
    epe; NaN where a pixel was left out) when it was asked for."""
    n: torch.Tensor
    l1: torch.Tensor
    epe: torch.Tensor
    sq: torch.Tensor
    du: torch.Tensor
    dv: torch.Tensor
    max: torch.Tensor
    map: Optional[torch.Tensor] = None

    @property
    def aee(self) -> torch.Tensor:
        """Average end-point error per pair (NaN where nothing was scored)."""
        return self.epe / self.n

    @property
    def rmse(self) -> torch.Tensor:
        return torch.sqrt(self.sq / self.n)

    @property
    def bias(self) -> torch.Tensor:
        """[B,2]: mean du, mean dv."""
        return torch.stack([self.du / self.n, self.dv / self.n], dim=1)

    @property
    def mean_l1(self) -> torch.Tensor:
        """The reference's L1 (mean over both components)."""
        return self.l1 / (2.0 * self.n)


def _from_sums(sums: torch.Tensor, emap: Optional[torch.Tensor] = None) -> FlowErrors:
    return FlowErrors(*(sums[:, q] for q in range(len(FIELDS))), emap)


def _pool_exponent(pool) -> int:
    if not _args.is_int(pool) or pool not in (1, 2, 4, 8, 16, 32):
        raise ValueError(f"pool={pool!r} must be a power of two from 1 to 32 (the pooled window's side)")
    return pool.bit_length() - 1


def _check_truth(truth: torch.Tensor, flow: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(truth, torch.Tensor) or truth.dtype != torch.float32:
        raise TypeError(f"{what}: expected a float32 truth tensor [B,2,H,W], got "
                        f"{truth.dtype if isinstance(truth, torch.Tensor) else type(truth).__name__}")
    if truth.device != flow.device or truth.dim() != 4 or truth.size(1) != 2 or truth.size(0) != flow.size(0):
        raise ValueError(f"{what}: truth {tuple(truth.shape)} on {truth.device} does not belong to flows {tuple(flow.shape)} on "
                         f"{flow.device}")
    return truth.detach().contiguous()


def _workspace(B: int, H: int, W: int, device) -> torch.Tensor:
    return torch.empty(_lib.load().pivlfn_flow_errors_workspace_bytes(B, H, W), dtype=torch.uint8, device=device)


def flow_errors(flow: torch.Tensor, truth: torch.Tensor, mask: Optional[torch.Tensor] = None, pool: int = 1, div_flow: float = 1.0,
                want_map: bool = False) -> FlowErrors:
    """Score [B,2,h,w] float32 flows against a [B,2,H,W] float32 truth on the device, enqueued on the current stream.

    The truth is multiplied by `div_flow` and averaged over `pool` x `pool` windows (a power of two up to 32; h = H / pool), as the
    reference's MultiScale / LevelLoss do for a pyramid level.  A pixel is left out where its truth window holds an unknown value
    (NaN or beyond 1e9 in magnitude) or a nonzero byte of `mask` [B,H,W]; a non-finite estimated flow is not left out and makes the
    sums non-finite."""
    k = _pool_exponent(pool)
    flow = _args.check_flows(flow, "flow_errors")
    truth = _check_truth(truth, flow, "flow_errors")
    mask = _args.check_mask(mask, "flow_errors", truth=truth)
    B, _, H, W = truth.shape
    if H % pool or W % pool or tuple(flow.shape[2:]) != (H // pool, W // pool):
        raise ValueError(f"flow_errors: flows {tuple(flow.shape)} are not truth {tuple(truth.shape)} pooled by {pool}")
    sums = torch.empty([B, len(FIELDS)], dtype=torch.float64, device=flow.device)
    emap = torch.empty([B, 3, H // pool, W // pool], dtype=torch.float32, device=flow.device) if want_map else None
    if B > 0:
        with torch.cuda.device(flow.device):
            ws = _workspace(B, H, W, flow.device)
            _lib.check(_lib.load().pivlfn_flow_errors(flow.data_ptr(), truth.data_ptr(), mask.data_ptr() if mask is not None else None,
                                                      B, H, W, k, float(div_flow), sums.data_ptr(),
                                                      emap.data_ptr() if want_map else None, ws.data_ptr(), ws.numel(),
                                                      _lib.stream_ptr(flow.device)), "flow_errors")
    return _from_sums(sums, emap)


def level_errors(net_or_lowest_level, levels, truth: torch.Tensor, div_flow: float, mask: Optional[torch.Tensor] = None
                 ) -> List[List[FlowErrors]]:
    """Score every flow `forward_levels` returns: [[M, S, R] per level, coarsest first] -> the same nesting of FlowErrors, level L
    against div_flow * truth averaged over 2^(L-1) windows, in one pass over the truth.  `net_or_lowest_level`: the network (its
    lowest_level is read) or the level number of the last entry.  The truth's sizes must be multiples of 32."""
    lowest = net_or_lowest_level if isinstance(net_or_lowest_level, int) else int(net_or_lowest_level.lowest_level)
    if isinstance(lowest, bool) or not 1 <= lowest <= 6:
        raise ValueError(f"level_errors: lowest_level={lowest!r} must be 1..6")
    nlev = 7 - lowest
    if not isinstance(levels, (list, tuple)) or len(levels) != nlev or any(not isinstance(t, (list, tuple)) or len(t) != 3 for t in levels):
        raise ValueError(f"level_errors: expected {nlev} levels of three flows (M, S, R), coarsest first")
    flat = [_args.check_flows(f, "level_errors") for trio in levels for f in trio]
    truth = _check_truth(truth, flat[0], "level_errors")
    mask = _args.check_mask(mask, "level_errors", truth=truth)
    B, _, H, W = truth.shape
    if H % 32 or W % 32:
        raise ValueError(f"level_errors: truth {H} x {W} must be multiples of 32 (level 6 averages 32 x 32 windows)")
    for i, f in enumerate(flat):
        k = 5 - i // 3
        if tuple(f.shape) != (B, 2, H >> k, W >> k) or f.device != truth.device:
            raise ValueError(f"level_errors: level {k + 1} flow {tuple(f.shape)} on {f.device} is not [{B},2,{H >> k},{W >> k}] on "
                             f"{truth.device}")
    # forward_levels hands out views of one packed buffer: use it as it is, pack copies otherwise
    base = flat[0].data_ptr()
    packed, at = all(f.is_contiguous() for f in flat), base
    for f in flat:
        packed = packed and f.data_ptr() == at
        at += f.numel() * 4
    buf = flat[0] if packed else torch.cat([f.reshape(-1) for f in flat])
    sums = torch.empty([B, nlev, 3, len(FIELDS)], dtype=torch.float64, device=truth.device)
    if B > 0:
        with torch.cuda.device(truth.device):
            ws = _workspace(B, H, W, truth.device)
            _lib.check(_lib.load().pivlfn_level_errors(buf.data_ptr(), lowest, truth.data_ptr(),
                                                       mask.data_ptr() if mask is not None else None, B, H, W, float(div_flow),
                                                       sums.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(truth.device)),
                       "level_errors")
    return [[_from_sums(sums[:, i, s]) for s in range(3)] for i in range(nlev)]


def finalize_errors(acc: np.ndarray, frames: int) -> Dict[str, np.ndarray]:
    """Per-pixel maps from the six sums (ACC order): bias = mean du / dv, rms = sqrt(max(mean d^2 - bias^2, 0)) (the random error),
    mean_epe; NaN where no frame was scored.  float64 [H,W] arrays, `count` int64 [H,W], `frames` an int64 scalar array."""
    acc = np.asarray(acc, dtype=np.float64)
    if acc.ndim != 3 or acc.shape[0] != len(ACC):
        raise ValueError(f"finalize_errors: expected accumulators [6,H,W], got {acc.shape}")
    if frames <= 0:
        raise ValueError("finalize_errors: no frames accumulated")
    n = np.where(acc[0] > 0, acc[0], np.nan)
    bu, bv = acc[1] / n, acc[2] / n

    def rms(s2, m):
        return np.sqrt(np.maximum(s2 / n - m * m, 0.0))             # NaN stays NaN through maximum and sqrt
    return {"frames": np.array(frames, dtype=np.int64), "count": acc[0].astype(np.int64), "bias_u": bu, "bias_v": bv,
            "rms_u": rms(acc[3], bu), "rms_v": rms(acc[4], bv), "mean_epe": acc[5] / n}


class ErrorStats(_accum.FrameAccumulator):
    """Per-pixel running error sums over a sequence of one size: acc [6,H,W] float64 on the device (ACC order) and the frame count.
    update() enqueues one kernel on the current stream and never synchronises the host; result() / save() do."""

    def __init__(self, H: int, W: int, device=None):
        super().__init__(H, W, device)
        self.acc = torch.zeros([len(ACC), self.H, self.W], dtype=torch.float64, device=self.device)

    def update(self, flow: torch.Tensor, truth: torch.Tensor, mask: Optional[torch.Tensor] = None) -> None:
        """Add the frames of `flow` against `truth` (both [B,2,H,W] float32 on this device), in batch order; `mask` as flow_errors."""
        flow = _args.check_flows(flow, "ErrorStats.update")
        truth = _check_truth(truth, flow, "ErrorStats.update")
        mask = _args.check_mask(mask, "ErrorStats.update", truth=truth)
        self._check_mine(flow.shape[2:], flow.device, lambda: f"flows {tuple(flow.shape)} and truth {tuple(truth.shape)} on {flow.device}",
                         also=truth.shape == flow.shape)
        B = flow.size(0)
        self._enqueue(B, (_lib.load().pivlfn_error_stats_accumulate, flow.data_ptr(), truth.data_ptr(),
                          mask.data_ptr() if mask is not None else None, self.acc.data_ptr(), B, self.H, self.W))

    def merge(self, group=None) -> None:
        """Collective over `group`, as FlowStats.merge: the accumulators of all ranks added in rank order, on every rank."""
        self.count = _accum.merge_sums([self.acc], self.count, group)

    def result(self) -> Dict[str, np.ndarray]:
        """finalize_errors() of the current sums (RESULT)."""
        return finalize_errors(self.acc.cpu().numpy(), self.count)

    def save(self, path: str, **extra) -> str:
        """An .npz with the raw accumulators (`acc`, float64, ACC order: what merges and what every map can be formed again from
        with finalize_errors), `frames`, result()'s maps rounded to float32 and `count` as int32 (the maps are for looking at: in
        float64 they would double the file, 101 MB for a 1024 x 1024 recording), and `extra`; returns the path written."""
        acc = self.acc.cpu().numpy()
        res = finalize_errors(acc, self.count)
        maps = {k: v.astype(np.float32) for k, v in res.items() if k not in ("frames", "count")}
        return _accum.save_npz(path, acc=acc, frames=res["frames"], count=res["count"].astype(np.int32), **extra, **maps)
