"""Temporal spectra of a time-resolved flow sequence on the device: Welch's power spectral density of u and v and their cross-spectrum
at every vector, and what is read off them -- the dominant frequency and its share of the energy, the coherence and the phase between
u and v.

Every vector's time series is cut into overlapping segments of L frames; a segment is detrended, windowed and projected on cosines and
sines, and the squares are averaged over the segments.  The projections and squares run on csrc/spectrum.hip through the C ABI
(`pivlfn_spectrum_accumulate`; the arithmetic contract is written out in include/pivlfn.h), one launch per completed segment; the
window, the detrending and the trigonometry are folded into the basis the kernel is handed (`basis`), and everything derived from the
sums is host work in float64:

    ts = TemporalSpectrum(H, W, segment=256, fs=1000.0)
    for flows in batches: ts.update(flows, mask)              # enqueued on the current stream, no host synchronisation
    res = ts.result()
    f, density, share = res.peak()                            # the dominant-frequency map [ch,cw]
    res.psd("uu"), res.coherence(), res.phase()               # [K,ch,cw]
    ts.save("spectrum.npz")

The frames go through viz.decimate_flow into a ring of L rows on the device; an unknown or masked vector (an empty cell) makes its
vector invalid for exactly the segments that contain the frame.  The sums of a vector are formed in an order the contract fixes, so a
sequence gives the same bits however it is cut into update() calls.  GPU only, like the rest of the package: there is no CPU path.
"""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _accum, _args, _lib

MAX_SEGMENT = 1024
WINDOWS = ("hann", "boxcar")
DETRENDS = ("constant", "linear", None)
BANDS = ("uu", "vv")
SUU, SVV, CO, QD = range(4)                    # acc[k, :, p]


class Launch(NamedTuple):
    segment: int        # index s of the segment: frames s*hop .. s*hop + L - 1
    end: int            # frames of the batch that must be in the ring before the launch (the segment's last frame is batch[end - 1])
    first: int          # ring row of the segment's sample 0


def check_params(segment=256, overlap=None, window="hann", detrend="constant", cell=1, fs=1.0, kmax=None) -> Tuple[int, int]:
    """The parameter checks of TemporalSpectrum (ValueError), usable before any tensor exists: (overlap, kmax) with the defaults filled in."""
    if not _args.is_integer(segment) or not 2 <= segment <= MAX_SEGMENT:
        raise ValueError(f"TemporalSpectrum: segment={segment!r} must be an integer 2..{MAX_SEGMENT}, the frames of a segment")
    overlap = segment // 2 if overlap is None else overlap
    if not _args.is_integer(overlap) or not 0 <= overlap <= segment - 1:
        raise ValueError(f"TemporalSpectrum: overlap={overlap!r} must be an integer 0..segment-1 = {segment - 1}")
    kmax = segment // 2 if kmax is None else kmax
    if not _args.is_integer(kmax) or not 1 <= kmax <= segment // 2:
        raise ValueError(f"TemporalSpectrum: kmax={kmax!r} must be an integer 1..segment//2 = {segment // 2}, the highest frequency index kept")
    if window not in WINDOWS:
        raise ValueError(f"TemporalSpectrum: window={window!r} must be one of {', '.join(WINDOWS)}")
    if detrend not in DETRENDS:
        raise ValueError(f"TemporalSpectrum: detrend={detrend!r} must be 'constant', 'linear' or None")
    if isinstance(fs, bool) or not isinstance(fs, (int, float, np.integer, np.floating)) or not (fs > 0 and math.isfinite(fs)):
        raise ValueError(f"TemporalSpectrum: fs={fs!r} must be a positive sampling rate")
    if not _args.is_integer(cell) or not 1 <= cell <= 32768:
        raise ValueError(f"TemporalSpectrum: cell={cell!r} must be an integer from 1 to 32768")
    return int(overlap), int(kmax)


def check_size(H, W, cell=1) -> Tuple[int, int]:
    if not _args.is_integer(H) or not _args.is_integer(W) or H < 1 or W < 1:
        raise ValueError(f"TemporalSpectrum: bad flow size {H!r} x {W!r}")
    ch, cw = -(-int(H) // cell), -(-int(W) // cell)
    if 2 * ch * cw >= 1 << 31:
        raise ValueError(f"TemporalSpectrum: {2 * ch * cw} values per snapshot, must stay below 2^31; use a larger cell")
    return ch, cw


def check_flows(flows, H: int, W: int, device) -> None:
    """The refusals of update(): a float32 tensor [B,2,H,W] on `device`."""
    if not isinstance(flows, torch.Tensor):
        raise TypeError(f"TemporalSpectrum.update: expected a torch tensor [B,2,{H},{W}], got {type(flows).__name__}")
    if flows.dtype != torch.float32:
        raise TypeError(f"TemporalSpectrum.update: expected float32 flows, got {flows.dtype}")
    if flows.dim() != 4 or tuple(flows.shape[1:]) != (2, H, W):
        raise ValueError(f"TemporalSpectrum.update: flows of shape {tuple(flows.shape)}, expected [B,2,{H},{W}]")
    if flows.device != torch.device(device):
        raise ValueError(f"TemporalSpectrum.update: flows on {flows.device}, the ring is on {device}")


def window_values(L: int, window: str) -> np.ndarray:
    if window not in WINDOWS:
        raise ValueError(f"window={window!r} must be one of {', '.join(WINDOWS)}")
    t = np.arange(L, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * t / L) if window == "hann" else np.ones(L)


def basis(L: int, window: str = "hann", detrend="constant", K: Optional[int] = None) -> np.ndarray:
    """[K,2,L] float64: row [k,0] is window * cos(2 pi k t / L), row [k,1] window * sin(2 pi k t / L), k = 0..K-1 (default L//2 + 1),
    with the detrending folded in: for a symmetric projector D, (D x) . b = x . (D b), so the kernel needs no second pass over the
    data.  "constant" takes each row's mean out, "linear" also its component along t, None nothing."""
    if detrend not in DETRENDS:
        raise ValueError(f"detrend={detrend!r} must be 'constant', 'linear' or None")
    K = L // 2 + 1 if K is None else K
    w = window_values(L, window)
    t = np.arange(L, dtype=np.int64)
    angle = 2.0 * np.pi * ((np.arange(K, dtype=np.int64)[:, None] * t[None, :]) % L).astype(np.float64) / L
    b = np.stack([w * np.cos(angle), w * np.sin(angle)], axis=1)
    if detrend is not None:
        b = b - b.mean(axis=2, keepdims=True)
    if detrend == "linear":
        tc = t.astype(np.float64) - (L - 1) / 2.0
        b = b - (b @ tc)[..., None] * tc / (tc @ tc)
    return np.ascontiguousarray(b)


def segment_plan(n_seen: int, B: int, L: int, hop: int) -> Tuple[List[Launch], int]:
    """The launches a batch of B frames completes after n_seen frames have been seen, in order, and the frames left over after the
    batch (those after the last completed segment's end; all of them while no segment is complete).  Segment s covers the frames
    s*hop .. s*hop + L - 1; frame f lives in ring row f % L, so the frames after a segment's end may only be written once it has
    been launched.  Pure host arithmetic: the plan of a sequence is the same however it is cut into batches."""
    launches = []
    s = max(0, -(-(n_seen - L + 1) // hop))
    while s * hop + L - 1 < n_seen + B:
        launches.append(Launch(s, s * hop + L - n_seen, (s * hop) % L))
        s += 1
    total = n_seen + B
    return launches, total - ((s - 1) * hop + L) if s > 0 else total


def _refine(e_prev, e_peak, e_next, window: str):
    """The offset of a line from its peak bin, in bins, from the amplitude ratio towards the larger neighbour."""
    with np.errstate(invalid="ignore", divide="ignore"):
        up = e_next >= e_prev
        alpha = np.sqrt(np.where(up, e_next, e_prev) / e_peak)
        delta = (2.0 * alpha - 1.0) / (alpha + 1.0) if window == "hann" else alpha / (1.0 + alpha)
        delta = np.where(np.isfinite(delta), np.clip(delta, 0.0, 1.0), 0.0)
    return np.where(up, delta, -delta)


class TemporalSpectrumResult:
    """Everything derived from the sums acc [K,4,ch,cw] (Suu, Svv, Co, Qd per frequency index and vector) and segments [ch,cw] (how
    many segments each vector took part in), on the host in float64.  Frequency index k stands for k*fs/L."""

    def __init__(self, acc, segments, L: int, fs: float = 1.0, window: str = "hann", detrend="constant", overlap: Optional[int] = None,
                 cell: int = 1, frames: int = 0, launched: int = 0, H: int = 0, W: int = 0):
        acc = np.asarray(acc, dtype=np.float64)
        segments = np.asarray(segments)
        if acc.ndim != 4 or acc.shape[1] != 4 or acc.shape[2:] != segments.shape:
            raise ValueError(f"TemporalSpectrumResult: expected sums [K,4,ch,cw] and segments [ch,cw], got {acc.shape} and {segments.shape}")
        self.acc, self.segments = acc, segments.astype(np.float64)
        self.L, self.fs, self.window, self.detrend = int(L), float(fs), window, detrend
        self.overlap = self.L // 2 if overlap is None else int(overlap)
        self.cell, self.frames, self.launched, self.H, self.W = int(cell), int(frames), int(launched), int(H), int(W)
        self.K = acc.shape[0]
        self.freq = np.arange(self.K, dtype=np.float64) * self.fs / self.L
        self.weight = np.where((np.arange(self.K) == 0) | ((self.L % 2 == 0) & (np.arange(self.K) == self.L // 2)), 1.0, 2.0)
        self.window_power = float((window_values(self.L, window) ** 2).sum())

    def _density(self, sums):
        """One-sided density of raw sums [K,...]: w_k * sums / (segments * fs * sum window^2), NaN where no segment."""
        with np.errstate(invalid="ignore", divide="ignore"):
            n = np.where(self.segments > 0, self.segments, np.nan)
            return self.weight.reshape((-1,) + (1,) * (sums.ndim - 1)) * sums / (n * self.fs * self.window_power)

    def _band(self, band: str) -> np.ndarray:
        if band == "uu+vv":
            return self.acc[:, SUU] + self.acc[:, SVV]
        if band not in BANDS:
            raise ValueError(f"band={band!r} must be 'uu', 'vv' or (for peak and pooled) 'uu+vv'")
        return self.acc[:, BANDS.index(band)]

    def psd(self, band: str = "uu") -> np.ndarray:
        """[K,ch,cw]: the one-sided power spectral density of u ("uu") or v ("vv"), scipy.signal.welch's scaling="density"."""
        if band not in BANDS:
            raise ValueError(f"psd: band={band!r} must be 'uu' or 'vv'")
        return self._density(self._band(band))

    def cross(self) -> np.ndarray:
        """[K,ch,cw] complex: Co + i Qd, normalised as psd."""
        return self._density(self.acc[:, CO]) + 1j * self._density(self.acc[:, QD])

    def coherence(self) -> np.ndarray:
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.abs(self.cross()) ** 2 / (self.psd("uu") * self.psd("vv"))

    def phase(self) -> np.ndarray:
        """atan2(Qd, Co): positive where v lags u.  NaN where the vector saw no segment."""
        return np.where(self.segments > 0, np.arctan2(self.acc[:, QD], self.acc[:, CO]), np.nan)

    def pooled(self, band: str = "uu+vv") -> np.ndarray:
        """[K]: the mean density over the vectors that took part in a segment."""
        d = self._density(self._band(band))
        valid = self.segments > 0
        return d[:, valid].mean(axis=1) if valid.any() else np.full(self.K, np.nan)

    def _range(self, fmin, fmax) -> Tuple[int, int]:
        lo = 0 if fmin is None else int(np.searchsorted(self.freq, fmin, "left"))
        hi = self.K - 1 if fmax is None else int(np.searchsorted(self.freq, fmax, "right")) - 1
        if not 0 <= lo <= hi <= self.K - 1:
            raise ValueError(f"peak: no frequency index between fmin={fmin!r} and fmax={fmax!r} (0 .. {self.freq[-1]!r})")
        return lo, hi

    def _peak(self, raw, density, lo, hi):
        """raw, density: [K,...] -> (frequency, density at the peak, share) over k = lo..hi; the first maximum wins."""
        d = density[lo:hi + 1]
        k = lo + np.argmax(np.where(np.isnan(d), -np.inf, d), axis=0)
        idx = np.expand_dims(k, 0)
        take = lambda a, kk: np.take_along_axis(a, np.expand_dims(np.clip(kk, 0, self.K - 1), 0), axis=0)[0]   # noqa: E731
        inner = (k > lo) & (k < hi)
        delta = np.where(inner, _refine(take(raw, k - 1), take(raw, k), take(raw, k + 1), self.window), 0.0)
        top = np.take_along_axis(density, idx, axis=0)[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            share = top / d.sum(axis=0)
        f = np.where(np.isnan(top), np.nan, (k + delta) * self.fs / self.L)
        return f, top, share

    def peak(self, band: str = "uu+vv", fmin=None, fmax=None):
        """(frequency map, density at the peak bin, its share of the band's total over the range), each [ch,cw]; NaN where the vector
        saw no segment.  The first maximum wins; away from the ends of the range the frequency is refined from the amplitude ratio to
        the larger neighbour: delta = (2a - 1)/(a + 1) for the Hann window, a/(1 + a) for boxcar, a = sqrt(E_neighbour/E_peak)."""
        lo, hi = self._range(fmin, fmax)
        raw = self._band(band)
        return self._peak(raw, self._density(raw), lo, hi)

    def summary(self) -> Dict:
        """The pooled spectrum's peak (of uu+vv, DC left out where there is another index), its share, the resolution fs/L, the
        segments launched and the frames after the last one."""
        valid = self.segments > 0
        out = {"peak_frequency": None, "peak_share": None, "resolution": self.fs / self.L, "segments": self.launched,
               "frames": self.frames, "frames_left_over": self.frames - ((self.launched - 1) * (self.L - self.overlap) + self.L)
               if self.launched > 0 else self.frames, "valid_vectors": int(valid.sum()), "vectors": int(valid.size)}
        if valid.any():
            dens = self.pooled("uu+vv")
            f, _, share = self._peak(dens / self.weight, dens, min(1, self.K - 1), self.K - 1)
            out["peak_frequency"], out["peak_share"] = float(f), float(share)
        return out

    def save(self, path: str, **extra) -> str:
        """An .npz with the raw sums (`acc`, `segments`) and every parameter, so that a file can be normalised again (`load`), beside
        `freq` and the pooled densities `psd_uu`, `psd_vv`; and `extra`.  Returns the path written."""
        out = {"acc": self.acc, "segments": self.segments.astype(np.int32), "segment": np.int64(self.L), "overlap": np.int64(self.overlap),
               "window": np.str_(self.window), "detrend": np.str_("none" if self.detrend is None else self.detrend), "fs": np.float64(self.fs),
               "cell": np.int64(self.cell), "frames": np.int64(self.frames), "launched": np.int64(self.launched), "H": np.int64(self.H),
               "W": np.int64(self.W), "freq": self.freq, "psd_uu": self.pooled("uu"), "psd_vv": self.pooled("vv")}
        return _accum.save_npz(path, **extra, **out)

    @classmethod
    def load(cls, path: str) -> "TemporalSpectrumResult":
        with np.load(path) as f:
            detrend = str(f["detrend"])
            return cls(f["acc"], f["segments"], int(f["segment"]), float(f["fs"]), str(f["window"]), None if detrend == "none" else detrend,
                       int(f["overlap"]), int(f["cell"]), int(f["frames"]), int(f["launched"]), int(f["H"]), int(f["W"]))


class TemporalSpectrum:
    """Welch sums over a flow sequence of one size: a ring of `segment` decimated frames [L, 2*ch*cw] float32, acc [K,4,ch*cw] float64
    and segments [ch*cw] int32 on the device, K = kmax + 1.  update() enqueues the copies into the ring and one kernel per completed
    segment on the current stream and never synchronises the host; result() / save() do."""

    def __init__(self, H: int, W: int, segment: int = 256, overlap: Optional[int] = None, window: str = "hann", detrend="constant",
                 cell: int = 1, fs: float = 1.0, kmax: Optional[int] = None, device=None):
        self.overlap, self.kmax = check_params(segment, overlap, window, detrend, cell, fs, kmax)
        self.ch, self.cw = check_size(H, W, cell)
        self.H, self.W, self.L, self.window, self.detrend, self.cell, self.fs = int(H), int(W), int(segment), window, detrend, int(cell), float(fs)
        self.hop, self.K, self.N = self.L - self.overlap, self.kmax + 1, self.ch * self.cw
        self.ld = -(-2 * self.N // 4) * 4
        self.device = _accum.cuda_device(device, "TemporalSpectrum: GPU devices only")
        self.ring = torch.zeros([self.L, self.ld], dtype=torch.float32, device=self.device)
        self.basis = torch.from_numpy(basis(self.L, window, detrend, self.K)).to(self.device)
        self.acc = torch.zeros([self.K, 4, self.N], dtype=torch.float64, device=self.device)
        self.count = torch.zeros([self.N], dtype=torch.int32, device=self.device)
        self.frames, self.launched = 0, 0

    @staticmethod
    def device_bytes(H: int, W: int, segment: int = 256, cell: int = 1, kmax: Optional[int] = None) -> int:
        """The bytes of the ring, the sums and the counts."""
        N = (-(-H // cell)) * (-(-W // cell))
        K = (segment // 2 if kmax is None else kmax) + 1
        return segment * (-(-2 * N // 4) * 4) * 4 + K * 4 * N * 8 + N * 4 + K * 2 * segment * 8

    def _write(self, mean: torch.Tensor, lo: int, hi: int) -> None:
        """Frames lo..hi-1 of the batch into their ring rows (frame f to row f % L)."""
        P = 2 * self.N
        while lo < hi:
            r = (self.frames + lo) % self.L
            n = min(hi - lo, self.L - r)
            self.ring[r:r + n, :P].copy_(mean[lo:lo + n].reshape(n, P))
            lo += n

    def update(self, flows: torch.Tensor, mask: Optional[torch.Tensor] = None) -> None:
        """Add the frames of `flows` [B,2,H,W] (float32, on this device), in batch order; `mask` [B,H,W]: nonzero = the vector is
        unknown in that frame, which takes it (its cell, if every vector of the cell is) out of the segments that contain the frame."""
        from .viz import decimate_flow
        check_flows(flows, self.H, self.W, self.device)
        B = flows.size(0)
        if B == 0:
            return
        mean, _ = decimate_flow(flows, self.cell, mask)
        launches, _ = segment_plan(self.frames, B, self.L, self.hop)
        lib, at = _lib.load(), 0
        with torch.cuda.device(self.device):
            for launch in launches:
                self._write(mean, at, launch.end)
                at = launch.end
                _lib.check(lib.pivlfn_spectrum_accumulate(self.ring.data_ptr(), self.L, launch.first, self.N, self.ld, self.basis.data_ptr(),
                                                          self.K, self.acc.data_ptr(), self.count.data_ptr(), _lib.stream_ptr(self.device)),
                           "TemporalSpectrum.update")
            self._write(mean, at, B)
        self.frames += B
        self.launched += len(launches)

    def result(self) -> TemporalSpectrumResult:
        return TemporalSpectrumResult(self.acc.cpu().numpy().reshape(self.K, 4, self.ch, self.cw), self.count.cpu().numpy().reshape(self.ch, self.cw),
                                      self.L, self.fs, self.window, self.detrend, self.overlap, self.cell, self.frames, self.launched, self.H, self.W)

    def save(self, path: str, **extra) -> str:
        return self.result().save(path, **extra)
