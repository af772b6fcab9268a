"""Ensemble correlation (sum of correlation, Meinhart, Wereley & Santiago 2000): the mean displacement of an image sequence read
straight from the images, without the network.  The correlation planes of fixed interrogation windows are added over all pairs of a
sequence, and one peak per window is read from the sum -- a mean displacement field that owes nothing to the weights, that still has
a peak when single pairs are too sparsely seeded to correlate, and that shows the bias of the network's mean flow window by window.

The sums run on csrc/ensemble.hip through the C ABI (`pivlfn_ensemble_corr`; the grid, the OUTSIDE rule and the sums are written out
in include/pivlfn.h); they are integers, so a sequence gives the same bits however it is cut into update() calls.  Everything derived
from them is host work in float64 on ny x nx small planes:

    ens = EnsembleCorrelation(H, W, window=32, step=16, search=8)
    for a, b in chunks: ens.update(a, b)                      # enqueued on the current stream, no host synchronisation
    res = ens.result()                                        # EnsembleResult: displacement [2,ny,nx], height, ratio, flag
    res.compare(stats_mean)                                   # the ensemble minus the window mean of a flow field, bias and rms
    ens.save("ensemble.npz");  EnsembleResult.load("ensemble.npz")

A larger displacement than `search` needs a pre-shift: `offset` [2,ny,nx] (ox, oy per window, whole pixels) moves the search region of
the second image; predictor_offsets() forms it from a mean flow field.  GPU only, like the rest of the package."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _accum, _args, _lib

OUTSIDE, FLAT, EDGE, NO_PEAK = 1, 2, 4, 8
FLAGS = {"outside": OUTSIDE, "flat": FLAT, "edge": EDGE, "no_peak": NO_PEAK}
_NEIGHBOURS = tuple((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))


def check_params(window, step, search, floor=1.0) -> None:
    """The parameter checks of EnsembleCorrelation (ValueError), usable before any tensor exists."""
    _args.check_int("EnsembleCorrelation", "window", window, 8, 128, ", the side of the interrogation window")
    if window % 4:
        raise ValueError(f"EnsembleCorrelation: window={window!r} must be a multiple of 4")
    _args.check_int("EnsembleCorrelation", "step", step, 1, 1 << 20, ", the pixels between two windows")
    _args.check_int("EnsembleCorrelation", "search", search, 1, 32, ", the largest displacement looked at")
    _args.check_not_negative("EnsembleCorrelation", "floor", floor)


def grid(H: int, W: int, window: int, step: int, search: int):
    """(ny, nx): the windows that fit with their search range; (0, 0)-sized frames are the caller's to refuse."""
    span = window + 2 * search
    return ((H - span) // step + 1 if H >= span else 0), ((W - span) // step + 1 if W >= span else 0)


def _corners(ny: int, nx: int, step: int, search: int):
    return search + step * np.arange(ny, dtype=np.int64), search + step * np.arange(nx, dtype=np.int64)


def check_offset(offset, ny: int, nx: int) -> Optional[np.ndarray]:
    """None, or the pre-shift as a host int32 [2,ny,nx] array (ox, oy)."""
    if offset is None:
        return None
    if isinstance(offset, torch.Tensor):
        offset = offset.detach().cpu().numpy()
    offset = np.asarray(offset)
    if offset.dtype.kind not in "iu":
        raise TypeError(f"EnsembleCorrelation: offset must hold integers, got {offset.dtype}")
    if offset.shape != (2, ny, nx):
        raise ValueError(f"EnsembleCorrelation: offset {offset.shape}, expected [2,{ny},{nx}]")
    wide = offset.astype(np.int64)
    if np.abs(wide).max(initial=0) >= 1 << 31:
        raise ValueError("EnsembleCorrelation: offset does not fit 32 bits")
    return np.ascontiguousarray(wide.astype(np.int32))


def outside_windows(H: int, W: int, window: int, step: int, search: int, offset=None) -> np.ndarray:
    """bool [ny,nx]: the windows whose search region in the second image, moved by `offset`, leaves the frame (the header's rule)."""
    ny, nx = grid(H, W, window, step, search)
    out = np.zeros((ny, nx), dtype=bool)
    if offset is None:
        return out
    y, x = _corners(ny, nx, step, search)
    oy, ox = np.asarray(offset[1], np.int64), np.asarray(offset[0], np.int64)
    ty, tx = y[:, None] + oy - search, x[None, :] + ox - search
    return (ty < 0) | (ty + 2 * search + window > H) | (tx < 0) | (tx + 2 * search + window > W)


def _window_mean(field, window: int, step: int, search: int) -> np.ndarray:
    """[C,H,W] -> [C,ny,nx]: the float64 mean of every plane over the footprint of each window of the first image."""
    if isinstance(field, torch.Tensor):
        field = field.detach().cpu().numpy()
    field = np.asarray(field, dtype=np.float64)
    if field.ndim != 3:
        raise ValueError(f"expected planes [C,H,W], got {field.shape}")
    ny, nx = grid(field.shape[1], field.shape[2], window, step, search)
    if ny < 1 or nx < 1:
        raise ValueError(f"planes {field.shape} hold no window of {window} + 2*{search} pixels")
    views = np.lib.stride_tricks.sliding_window_view(field, (window, window), axis=(1, 2))
    with np.errstate(invalid="ignore", over="ignore"):
        return views[:, search::step, search::step][:, :ny, :nx].mean(axis=(-2, -1))


def predictor_offsets(mean, window: int, step: int, search: int) -> np.ndarray:
    """The pre-shift a mean flow field `mean` [2,H,W] (u, v) suggests: int32 [2,ny,nx], per window the float64 mean of the field over
    the window's footprint, rounded half to even; 0 where that mean is not finite."""
    check_params(window, step, search)
    m = _window_mean(mean, window, step, search)
    if m.shape[0] != 2:
        raise ValueError(f"predictor_offsets: expected a field [2,H,W], got {m.shape[0]} planes")
    m = np.where(np.isfinite(m), m, 0.0)
    return np.rint(np.clip(m, -(2.0 ** 30), 2.0 ** 30)).astype(np.int32)


def _fit(c0, cm, cp):
    """One axis of pivlfn_match_quality's three-point Gaussian fit: the offset, or None where a condition fails (a NaN fails all)."""
    if not (cm > 0.0 and cp > 0.0 and c0 >= cm and c0 >= cp and (2.0 * c0 - cm) - cp >= 1e-6):
        return None
    lm, l0, lp = np.log(cm), np.log(c0), np.log(cp)
    return 0.5 * (lm - lp) / ((lm - 2.0 * l0) + lp)


def _ratio(plane: np.ndarray, py: int, px: int) -> float:
    """The peak over the largest OTHER local maximum (an entry >= all its in-plane neighbours; NaN entries are neither maxima nor
    neighbours); inf with no other local maximum, or a non-positive one."""
    P = plane.shape[0]
    low = np.where(np.isnan(plane), -np.inf, plane)
    pad = np.full((P + 2, P + 2), -np.inf)
    pad[1:-1, 1:-1] = low
    is_max = ~np.isnan(plane)
    for dy, dx in _NEIGHBOURS:
        is_max &= low >= pad[1 + dy:1 + dy + P, 1 + dx:1 + dx + P]
    is_max[py, px] = False
    second = low[is_max].max() if is_max.any() else -np.inf
    return float(plane[py, px] / second) if second > 0.0 else float("inf")


class EnsembleResult:
    """What the integer sums give, on the host in float64.  With N = frames * window^2 and the sums converted to float64 first:
        va = AA - A*A/N,  vb = BB - B*B/N,  cov = AB - A*B/N;  an entry is flat where va or vb < floor^2 * N;
        corr [ny,nx,P,P] = cov / sqrt(va*vb), NaN where flat (and everywhere in an OUTSIDE window).
    Peak: the largest non-NaN entry, the first in row-major order among equals.  flag [ny,nx] (uint8): OUTSIDE = 1; FLAT = 2, va is
    flat or no entry is left; EDGE = 4, the peak lies on the rim of the plane; NO_PEAK = 8, a condition of pivlfn_match_quality's fit
    fails (the centre and the four neighbours > 0, the centre >= each neighbour, (2 c0 - c_minus) - c_plus >= 1e-6 per axis).
    displacement [2,ny,nx] (x, y) = offset + integer peak + that contract's three-point Gaussian fit per axis, NaN where any flag is
    set;  height: the peak's correlation;  ratio: the peak over the largest other local maximum of the plane (an entry >= all its
    in-plane neighbours), inf where there is none or it is not positive;  frames: the pairs added.
    `outside` [ny,nx]: the OUTSIDE windows; where it is not given it follows from H, W and `offset` (none without H and W)."""

    def __init__(self, sums, sums_a, frames: int, window: int, step: int, offset=None, outside=None, floor: float = 1.0,
                 H: Optional[int] = None, W: Optional[int] = None):
        sums, sums_a = np.asarray(sums), np.asarray(sums_a)
        if sums.ndim != 5 or sums.shape[2] != sums.shape[3] or sums.shape[2] % 2 != 1 or sums.shape[4] != 3 or sums.dtype != np.int64:
            raise ValueError(f"EnsembleResult: expected int64 sums [ny,nx,P,P,3] with P odd, got {sums.dtype} {sums.shape}")
        ny, nx, P = sums.shape[:3]
        if sums_a.shape != (ny, nx, 2) or sums_a.dtype != np.int64:
            raise ValueError(f"EnsembleResult: expected int64 sums_a [{ny},{nx},2], got {sums_a.dtype} {sums_a.shape}")
        search = (P - 1) // 2
        check_params(window, step, search, floor)
        self.sums, self.sums_a, self.frames = sums, sums_a, int(frames)
        self.window, self.step, self.search, self.floor, self.H, self.W = window, step, search, float(floor), H, W
        self.ny, self.nx, self.P = ny, nx, P
        self.offset = check_offset(offset, ny, nx)
        off = np.zeros((2, ny, nx), np.int32) if self.offset is None else self.offset
        if outside is None and H is not None and W is not None:
            outside = outside_windows(H, W, window, step, search, self.offset)
        self.outside = np.zeros((ny, nx), bool) if outside is None else np.asarray(outside, dtype=bool)
        if self.outside.shape != (ny, nx):
            raise ValueError(f"EnsembleResult: outside {self.outside.shape}, expected [{ny},{nx}]")

        N = float(self.frames) * window * window
        A, AA = sums_a[..., 0].astype(np.float64)[..., None, None], sums_a[..., 1].astype(np.float64)[..., None, None]
        Bs, BB, AB = (sums[..., k].astype(np.float64) for k in range(3))
        lim = self.floor * self.floor * N
        with np.errstate(invalid="ignore", divide="ignore"):
            va, vb, cov = AA - A * A / N, BB - Bs * Bs / N, AB - A * Bs / N
            flat_a = ~(va >= lim)[..., 0, 0]                     # a NaN (no frame) is flat
            flat = ~(va >= lim) | ~(vb >= lim)
            self.corr = np.where(flat | self.outside[..., None, None], np.nan, cov / np.sqrt(np.where(flat, 1.0, va * vb)))

        self.flag = np.zeros((ny, nx), np.uint8)
        self.height = np.full((ny, nx), np.nan)
        self.ratio = np.full((ny, nx), np.nan)
        self.peak = np.full((2, ny, nx), -1, np.int64)           # (x, y) index of the peak inside the plane
        self.displacement = np.full((2, ny, nx), np.nan)
        for j in range(ny):
            for i in range(nx):
                if self.outside[j, i]:
                    self.flag[j, i] = OUTSIDE
                    continue
                c = self.corr[j, i]
                if flat_a[j, i] or np.isnan(c).all():
                    self.flag[j, i] = FLAT
                    continue
                py, px = np.unravel_index(np.nanargmax(c), c.shape)          # the first among equals
                self.peak[:, j, i] = (px, py)
                self.height[j, i], self.ratio[j, i] = c[py, px], _ratio(c, py, px)
                if py in (0, P - 1) or px in (0, P - 1):
                    self.flag[j, i] = EDGE
                    continue
                fx, fy = _fit(c[py, px], c[py, px - 1], c[py, px + 1]), _fit(c[py, px], c[py - 1, px], c[py + 1, px])
                if not c[py, px] > 0.0 or fx is None or fy is None:
                    self.flag[j, i] = NO_PEAK
                    continue
                self.displacement[:, j, i] = (off[0, j, i] + (px - search) + fx, off[1, j, i] + (py - search) + fy)

    def centres(self):
        """(x [nx], y [ny]): the centres of the windows in the first image, corner + (window - 1)/2."""
        y, x = _corners(self.ny, self.nx, self.step, self.search)
        return x + (self.window - 1) / 2.0, y + (self.window - 1) / 2.0

    def summary(self) -> Dict[str, object]:
        """The flag counts and the medians of height and ratio over the windows that have a peak, JSON-ready."""
        doc: Dict[str, object] = {"windows": int(self.flag.size), "frames": self.frames,
                                  "valid": int((self.flag == 0).sum())}
        for name, bit in FLAGS.items():
            doc[name] = int(((self.flag & bit) != 0).sum())
        have = np.isfinite(self.height)
        doc["median_height"] = float(np.median(self.height[have])) if have.any() else float("nan")
        doc["median_ratio"] = float(np.median(self.ratio[have])) if have.any() else float("nan")
        return doc

    def compare(self, mean) -> Dict[str, object]:
        """Against a flow field `mean` [2,H,W] (the mean of a FlowStats): "difference" [2,ny,nx], the ensemble displacement minus the
        mean of the field over each window's footprint (NaN where the window is flagged), and over the unflagged windows "bias_u",
        "bias_v" (its means), "rms" (the root of the mean squared length) and "windows" (their number)."""
        m = _window_mean(mean, self.window, self.step, self.search)
        if m.shape != (2, self.ny, self.nx):
            raise ValueError(f"EnsembleResult.compare: the field gives {m.shape[1:]} windows, the result has {(self.ny, self.nx)}")
        diff = self.displacement - m
        ok = (self.flag == 0) & np.isfinite(diff).all(0)
        n = int(ok.sum())
        nan = float("nan")
        return {"difference": diff, "windows": n,
                "bias_u": float(diff[0][ok].mean()) if n else nan, "bias_v": float(diff[1][ok].mean()) if n else nan,
                "rms": float(np.sqrt((diff[0][ok] ** 2 + diff[1][ok] ** 2).mean())) if n else nan}

    def save(self, path: str, **extra) -> str:
        """An .npz with the integer sums (`sums`, `sums_a`), every parameter (H, W, window, step, search, floor, frames, `offset` -- zeros
        without a pre-shift -- and `outside`), and what follows from them: x, y (the centres), displacement, height, ratio, flag; and
        `extra`.  Returns the path written."""
        x, y = self.centres()
        off = np.zeros((2, self.ny, self.nx), np.int32) if self.offset is None else self.offset
        return _accum.save_npz(path, **extra, sums=self.sums, sums_a=self.sums_a, H=np.int64(-1 if self.H is None else self.H),
                               W=np.int64(-1 if self.W is None else self.W), window=np.int64(self.window), step=np.int64(self.step),
                               search=np.int64(self.search), floor=np.float64(self.floor), frames=np.int64(self.frames), offset=off,
                               outside=self.outside, x=x, y=y, displacement=self.displacement, height=self.height, ratio=self.ratio,
                               flag=self.flag)

    @staticmethod
    def load(path: str) -> "EnsembleResult":
        """The result a save() file holds, finalised again from its integer sums."""
        with np.load(path) as f:
            H, W = int(f["H"]), int(f["W"])
            return EnsembleResult(f["sums"], f["sums_a"], int(f["frames"]), int(f["window"]), int(f["step"]), f["offset"], f["outside"],
                                  float(f["floor"]), None if H < 0 else H, None if W < 0 else W)


def finalize(sums, sums_a, frames: int, window: int, step: int, offset=None, outside=None, floor: float = 1.0, H=None, W=None):
    """Pure host code: the EnsembleResult of integer sums [ny,nx,P,P,3] and [ny,nx,2], wherever they come from."""
    return EnsembleResult(sums, sums_a, frames, window, step, offset, outside, floor, H, W)


def _as_bytes(x: torch.Tensor, name: str, what: str, gpu_only: bool = True) -> torch.Tensor:
    """uint8 [B,H,W] as it is; float32 in [0,1], [B,H,W] or [B,1|3,H,W]: gray = ((r + g) + b) / 3, then rint(255 gray) clamped to
    0..255 -- the pipeline's k/255 table gives back k."""
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"{what}: expected a uint8 [B,H,W] or float32 [B,H,W] / [B,C,H,W] tensor for {name}, got "
                        f"{x.dtype if isinstance(x, torch.Tensor) else type(x).__name__}")
    if gpu_only and not x.is_cuda:
        raise NotImplementedError(f"{what}: GPU tensors only")
    if x.dtype == torch.uint8:
        if x.dim() != 3:
            raise ValueError(f"{what}: expected uint8 frames [B,H,W] for {name}, got {tuple(x.shape)}")
        return x.detach().contiguous()
    if x.dim() == 4 and x.size(1) in (1, 3):
        x = x.detach()
        x = x[:, 0] if x.size(1) == 1 else ((x[:, 0] + x[:, 1]) + x[:, 2]) / 3
    elif x.dim() != 3:
        raise ValueError(f"{what}: expected float32 frames [B,H,W] or [B,C,H,W] with C = 1 or 3 for {name}, got {tuple(x.shape)}")
    return torch.round(255 * x.detach()).clamp_(0, 255).to(torch.uint8).contiguous()      # torch.round: half to even, rint


class EnsembleCorrelation(_accum.FrameAccumulator):
    """Running correlation sums over the pairs of an image sequence of one size: sums [ny,nx,P,P,3] and sums_a [ny,nx,2], int64 on
    the device, and the pair count.  update() enqueues one kernel on the current stream and never synchronises the host; result() /
    save() do.  `offset`: None or integers [2,ny,nx] (ox, oy), the pre-shift of each window of the second image; the windows it pushes
    out of the frame are `outside` and stay empty.  `floor`: the rms gray level below which a window counts as flat."""

    def __init__(self, H: int, W: int, window: int = 32, step: int = 16, search: int = 8, offset=None, floor: float = 1.0, device=None):
        check_params(window, step, search, floor)
        self.window, self.step, self.search, self.floor, self.P = window, step, search, float(floor), 2 * search + 1
        ny, nx = grid(int(H), int(W), window, step, search)
        super().__init__(H, W, device, ny >= 1 and nx >= 1 and int(H) * int(W) < 1 << 31,
                         f" (positive, at least window + 2*search = {window + 2 * search} pixels each way, fewer than 2^31 pixels)")
        self.ny, self.nx = ny, nx
        self.offset = check_offset(offset, ny, nx)
        self.outside = outside_windows(self.H, self.W, window, step, search, self.offset)
        self._offset = None if self.offset is None else torch.from_numpy(self.offset).to(self.device)
        self.sums = torch.zeros([ny, nx, self.P, self.P, 3], dtype=torch.int64, device=self.device)
        self.sums_a = torch.zeros([ny, nx, 2], dtype=torch.int64, device=self.device)

    def centres(self):
        """(x [nx], y [ny]): the centres of the windows in the first image."""
        y, x = _corners(self.ny, self.nx, self.step, self.search)
        return x + (self.window - 1) / 2.0, y + (self.window - 1) / 2.0

    def update(self, a: torch.Tensor, b: torch.Tensor) -> None:
        """Add the pairs (a[k], b[k]): uint8 [B,H,W], or float32 in [0,1] as [B,H,W] or [B,1|3,H,W], on this device."""
        a, b = _as_bytes(a, "a", "EnsembleCorrelation.update"), _as_bytes(b, "b", "EnsembleCorrelation.update")
        self._check_mine(a.shape[1:], a.device, lambda: f"frames {tuple(a.shape)} on {a.device}", "accumulators for [{H},{W}]")
        self._check_mine(b.shape[1:], b.device, lambda: f"second frames {tuple(b.shape)} on {b.device} beside {tuple(a.shape)}",
                         "accumulators for [{H},{W}]", also=b.size(0) == a.size(0))
        B = a.size(0)
        if B > 65535:
            raise ValueError(f"EnsembleCorrelation.update: {B} pairs, at most 65535 per call")
        self._enqueue(B, (_lib.load().pivlfn_ensemble_corr, a.data_ptr(), b.data_ptr(), _args.ptr(self._offset), self.sums.data_ptr(),
                          self.sums_a.data_ptr(), B, self.H, self.W, self.window, self.step, self.search))

    def result(self) -> EnsembleResult:
        return EnsembleResult(self.sums.cpu().numpy(), self.sums_a.cpu().numpy(), self.count, self.window, self.step, self.offset,
                              self.outside, self.floor, self.H, self.W)

    def save(self, path: str, **extra) -> str:
        """EnsembleResult.save of result(): the integer sums, every parameter and the fields.  Returns the path written."""
        return self.result().save(path, **extra)
