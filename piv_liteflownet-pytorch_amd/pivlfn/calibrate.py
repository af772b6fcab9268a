"""Stereo calibration: from two images of a cross target to the coefficient file `stereo_run.py -c` reads (reference: stereo_cal.py,
stereo/matching.py, stereo/dewarp.py).

Device steps (csrc/calibrate.hip, contracts in include/pivlfn.h): `template_match` (OpenCV's TM_CCOEFF_NORMED, bit-exact integer
sums), `find_markers` (threshold, 2 x 2 box-sum, 4-connected labelling, weighted centres) and `dewarp_frames` (the reference's `warp`
as a batched kernel, nearest or bilinear).  Host steps, float64 NumPy: `gen_template`, `index_lattice` (the reference's four clicks
and its `Guess` heuristics become four reference points and a neighbour search), `fit_mapping` (the 24 rational-polynomial
coefficients, in the direction `map_coeff` fits and `warp` / `pivlfn_stereo_2d3c` evaluate) and `write_coeff`.  `calibrate_camera`
chains them for one camera.  No OpenCV, SciPy or display.  GPU tensors only, like the rest of the package: CPU tensors raise
NotImplementedError."""
from __future__ import annotations

import ctypes
import json
import os
from collections import deque
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

N_COEFF = 24
NOT_INDEXED = np.iinfo(np.int64).min
MODES = {"nearest": 0, "bilinear": 1}


# ---- template ----------------------------------------------------------------------------------------------------------------------------
def gen_template(TC: int = 5, HC: int = 25, LC: int = 25) -> np.ndarray:
    """The cross template of stereo/matching.py:7-29: uint8 [HC,LC], a horizontal and a vertical bar of thickness TC (255) on 0.
    TC must be odd: the reference's even branch indexes with floats and cannot run."""
    TC, HC, LC = int(TC), int(HC), int(LC)
    if TC < 1 or TC % 2 == 0:
        raise ValueError(f"gen_template: TC={TC} must be odd and positive")
    if HC < TC or LC < TC:
        raise ValueError(f"gen_template: HC={HC} and LC={LC} must be at least TC={TC}")
    LC2, HC2, TC2 = -(-LC // 2), -(-HC // 2), TC // 2
    t = np.zeros([HC, LC], dtype=np.uint8)
    t[HC2 - TC2 - 1:HC2 + TC2, :] = 255
    t[:, LC2 - TC2 - 1:LC2 + TC2] = 255
    return t


def _images(images, what) -> torch.Tensor:
    if not isinstance(images, torch.Tensor):
        raise TypeError(f"{what}: expected a torch tensor")
    if not images.is_cuda:
        raise NotImplementedError(f"{what}: GPU tensors only")
    if images.dim() == 2:
        images = images[None]
    if images.dim() != 3 or images.numel() == 0:
        raise ValueError(f"{what}: expected [B,H,W] or [H,W], got {tuple(images.shape)}")
    return images.detach().contiguous()


def _template(template, dev) -> torch.Tensor:
    t = torch.as_tensor(template)
    if t.dtype != torch.uint8 or t.dim() != 2:
        raise ValueError("template: expected a uint8 [th,tw] array")
    th, tw = t.shape
    if th % 2 == 0 or tw % 2 == 0 or th * tw > 65025:
        raise ValueError(f"template: {th} x {tw} must have odd sides and at most 65025 taps")
    return t.to(dev).contiguous()


# ---- device steps ------------------------------------------------------------------------------------------------------------------------
def template_match(images: torch.Tensor, template) -> torch.Tensor:
    """`pivlfn_template_match`: uint8 images [B,H,W] (or [H,W]) and a uint8 template [th,tw] -> float32 r [B,H,W], the zero-mean
    normalised cross-correlation of the template centred on each pixel of the zero-padded image."""
    images = _images(images, "template_match")
    if images.dtype != torch.uint8:
        raise ValueError(f"template_match: uint8 images expected, got {images.dtype}")
    t = _template(template, images.device)
    B, H, W = images.shape
    th, tw = t.shape
    lib = _lib.load()
    need = lib.pivlfn_template_match_workspace_bytes(th, tw)
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device=images.device)
    r = torch.empty([B, H, W], dtype=torch.float32, device=images.device)
    with torch.cuda.device(images.device):
        _lib.check(lib.pivlfn_template_match(images.data_ptr(), t.data_ptr(), r.data_ptr(), B, H, W, th, tw, ws.data_ptr(), need,
                                             _lib.stream_ptr(images.device)), "template_match")
    return r


def target_points(r: torch.Tensor, threshold: float = 0.7, cap: int = 4096) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """`pivlfn_target_points` on a correlation map [B,H,W] -> (labels int32 [B,H,W], count int32 [B], rec int64 [B,cap,4]), all on
    the device; nothing is synchronised."""
    r = _images(r, "target_points")
    if r.dtype != torch.float32:
        raise ValueError(f"target_points: float32 map expected, got {r.dtype}")
    B, H, W = r.shape
    lib = _lib.load()
    need = lib.pivlfn_target_points_workspace_bytes(B, H, W)
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device=r.device)
    labels = torch.empty([B, H, W], dtype=torch.int32, device=r.device)
    count = torch.empty([B], dtype=torch.int32, device=r.device)
    rec = torch.empty([B, int(cap), 4], dtype=torch.int64, device=r.device)
    with torch.cuda.device(r.device):
        _lib.check(lib.pivlfn_target_points(r.data_ptr(), B, H, W, float(threshold), int(cap), labels.data_ptr(), count.data_ptr(),
                                            rec.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr(r.device)), "target_points")
    return labels, count, rec


def centres_from_records(rec: np.ndarray) -> np.ndarray:
    """int64 records [n,4] = (sum w, sum w*x, sum w*y, pixels) -> float64 (x, y) [n,2]: the weighted centre minus the half pixel the
    one-sided 2 x 2 window adds (the reference keeps that shift in its coordinates)."""
    rec = np.asarray(rec, dtype=np.int64).reshape(-1, 4)
    s = rec[:, 0].astype(np.float64)
    return np.stack([rec[:, 1].astype(np.float64) / s - 0.5, rec[:, 2].astype(np.float64) / s - 0.5], axis=1)


def keep_inside(centres: np.ndarray, H: int, W: int, th: int, tw: int) -> np.ndarray:
    """True for centres at least half the template away from every image edge: a cross cut by the edge still matches above 0.7,
    with a biased centre."""
    hx, hy = (tw - 1) / 2.0, (th - 1) / 2.0
    c = np.asarray(centres, dtype=np.float64).reshape(-1, 2)
    return (c[:, 0] >= hx) & (c[:, 0] <= W - 1 - hx) & (c[:, 1] >= hy) & (c[:, 1] <= H - 1 - hy)


def find_markers(images: torch.Tensor, template, threshold: float = 0.7, cap: int = 4096,
                 border: bool = True) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """Marker centres of every image: (centres, records), one float64 (x, y) array [n,2] and one int64 record array [n,4] per image,
    in ascending label order (row-major order of each component's first pixel).  With `border`, centres closer to an image edge than
    half the template are dropped (from both lists).  At most `cap` components per image are returned.  SYNCHRONISES: the number
    of components is read back before the records are."""
    images = _images(images, "find_markers")
    t = torch.as_tensor(template)
    r = template_match(images, t)
    _, count, rec = target_points(r, threshold, cap)
    count_h, rec_h = count.cpu().numpy(), rec.cpu().numpy()                  # the synchronisation
    H, W = images.shape[1:]
    centres, records = [], []
    for b in range(images.shape[0]):
        n = min(int(count_h[b]), int(cap))
        rb = rec_h[b, :n]
        cb = centres_from_records(rb)
        if border:
            keep = keep_inside(cb, H, W, t.shape[0], t.shape[1])
            cb, rb = cb[keep], rb[keep]
        centres.append(cb)
        records.append(rb)
    return centres, records


def dewarp_frames(frames: torch.Tensor, A, origin, mode: str = "nearest", fill: float = 0) -> torch.Tensor:
    """`pivlfn_dewarp_frames`: uint8 or float32 frames [B,H,W] (or [H,W]) -> frames of the same type and shape [B,H,W]; output pixel
    (x, y) takes the source at nl_trans(x - x0, y - y0; A) + (x0, y0), origin = (x0, y0).  `mode`: "nearest" (the reference's warp)
    or "bilinear"; sources outside the image give `fill`."""
    frames = _images(frames, "dewarp_frames")
    if frames.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"dewarp_frames: uint8 or float32 frames expected, got {frames.dtype}")
    if mode not in MODES:
        raise ValueError(f"dewarp_frames: mode {mode!r} (nearest or bilinear)")
    a = np.asarray(A, dtype=np.float64).reshape(-1)
    if a.shape != (N_COEFF,):
        raise ValueError(f"dewarp_frames: {N_COEFF} coefficients expected, got {a.size}")
    B, H, W = frames.shape
    out = torch.empty_like(frames)
    a_c = (ctypes.c_double * N_COEFF)(*a.tolist())
    with torch.cuda.device(frames.device):
        _lib.check(_lib.load().pivlfn_dewarp_frames(frames.data_ptr(), out.data_ptr(), int(frames.dtype == torch.float32), B, H, W, a_c,
                                                    float(origin[0]), float(origin[1]), MODES[mode], float(fill),
                                                    _lib.stream_ptr(frames.device)), "dewarp_frames")
    return out


# ---- host steps --------------------------------------------------------------------------------------------------------------------------
def index_lattice(points: np.ndarray, ref4, accept: float = 0.3) -> Tuple[np.ndarray, np.ndarray, Tuple[float, float]]:
    """Integer lattice indices of the markers.  `ref4`: four points (x, y), or four marker numbers, naming ONE lattice cell clockwise
    from top-left (top-left, top-right, bottom-right, bottom-left: the four clicks of select_ref, stereo/matching.py:78-115); each
    point is snapped to its nearest marker.  Those four get (0,0), (1,0), (1,1), (0,1); the rest are reached by a breadth-first
    neighbour search: from an indexed marker the next one along +-i / +-j is predicted with the local step (the step just behind it,
    else the parallel step of the neighbouring row or column, else the reference cell's) and the nearest marker is taken if it lies
    within `accept` of that step's length.  Gaps are simply not crossed from that side.
    Returns (ij int64 [n,2] with NOT_INDEXED rows for markers not reached, selected = the four marker numbers, (c_x, c_y) = the cell
    size by the reference's formula, matching.py:110-111)."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    n = len(pts)
    ref = np.asarray(ref4)
    if ref.shape == (4,):
        sel = [int(v) for v in ref]
        if min(sel) < 0 or max(sel) >= n:
            raise ValueError("index_lattice: a reference marker number is out of range")
    elif ref.shape == (4, 2):
        if n == 0:
            raise ValueError("index_lattice: no markers")
        sel = [int(np.argmin(np.linalg.norm(pts - np.asarray(p, dtype=np.float64), axis=1))) for p in ref]
    else:
        raise ValueError("index_lattice: ref4 must be four (x, y) points or four marker numbers")
    if len(set(sel)) != 4:
        raise ValueError(f"index_lattice: the four reference points snap to markers {sel}, which are not four different ones")
    p0, p1, p2, p3 = (pts[k] for k in sel)
    c_x = (abs(p1[0] - p0[0]) + abs(p3[0] - p2[0])) * 0.5
    c_y = (abs(p3[1] - p0[1]) + abs(p2[1] - p1[1])) * 0.5
    ex, ey = ((p1 - p0) + (p2 - p3)) * 0.5, ((p3 - p0) + (p2 - p1)) * 0.5
    ij = np.full((n, 2), NOT_INDEXED, dtype=np.int64)
    at = {}
    queue = deque()
    for k, c in zip(sel, ((0, 0), (1, 0), (1, 1), (0, 1))):
        ij[k] = c
        at[c] = k
        queue.append(k)

    def step(i, j, di, dj):
        if (i - di, j - dj) in at:
            return pts[at[(i, j)]] - pts[at[(i - di, j - dj)]]
        for s in (1, -1):                                         # the parallel edge one row / column over
            a, b = (i + s * dj, j + s * di), (i + s * dj + di, j + s * di + dj)
            if a in at and b in at:
                return pts[at[b]] - pts[at[a]]
            b = (a[0] - di, a[1] - dj)
            if a in at and b in at:
                return pts[at[a]] - pts[at[b]]
        return (ex if di else ey) * (di + dj)

    while queue:
        k = queue.popleft()
        i, j = int(ij[k, 0]), int(ij[k, 1])
        for di, dj in ((1, 0), (0, 1), (-1, 0), (0, -1)):
            c = (i + di, j + dj)
            if c in at:
                continue
            d = step(i, j, di, dj)
            dist = np.linalg.norm(pts - (pts[k] + d), axis=1)
            m = int(np.argmin(dist))
            if dist[m] <= accept * np.linalg.norm(d) and ij[m, 0] == NOT_INDEXED:
                ij[m] = c
                at[c] = m
                queue.append(m)
    return ij, np.array(sel, dtype=np.int64), (float(c_x), float(c_y))


def nl_trans(x, y, A):
    """stereo/dewarp.py:255-270 in float64."""
    A = np.asarray(A, dtype=np.float64)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)

    def P(k):
        return A[k] * x + A[k + 1] * y + A[k + 2] + A[k + 3] * np.power(x, 2) + A[k + 4] * np.power(y, 2) + A[k + 5] * x * y
    return P(0) / P(6), P(12) / P(18)


def _fit_axis(p, q, k, order):
    """One axis: k ~ N(p, q) / D(p, q), D's constant fixed at 1.  Returns the 12 coefficients (numerator, denominator)."""
    cols = [p, q, np.ones_like(p)] + ([p * p, q * q, p * q] if order == 2 else [])
    Phi = np.stack(cols, axis=1)                                  # numerator basis
    Psi = np.delete(Phi, 2, axis=1)                               # denominator basis without the constant
    nn, nd = Phi.shape[1], Psi.shape[1]
    # linear start: N - k * (D - 1) = k
    theta = np.linalg.lstsq(np.concatenate([Phi, -k[:, None] * Psi], axis=1), k, rcond=None)[0]

    def parts(th):
        return Phi @ th[:nn], Psi @ th[nn:] + 1.0

    def cost(th):
        N, D = parts(th)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = k - N / D
        c = float(r @ r)
        return c if np.isfinite(c) else np.inf

    best = cost(theta)
    for _ in range(50):                                           # damped Gauss-Newton on the true residual
        N, D = parts(theta)
        if not np.all(np.isfinite(N / D)):
            break
        J = np.concatenate([-Phi / D[:, None], (N / (D * D))[:, None] * Psi], axis=1)
        delta = np.linalg.lstsq(J, -(k - N / D), rcond=None)[0]
        lam, moved = 1.0, False
        for _ in range(12):
            c = cost(theta + lam * delta)
            if c < best:
                theta, best, moved = theta + lam * delta, c, True
                break
            lam *= 0.5
        if not moved or np.linalg.norm(lam * delta) <= 1e-15 * max(np.linalg.norm(theta), 1.0):
            break
    out = np.zeros(12)
    num, den = theta[:nn], np.insert(theta[nn:], 2, 1.0)
    out[:nn], out[6:6 + nn] = num, den
    return out


def fit_mapping(new_rel, old_rel, order: int = 2) -> Tuple[np.ndarray, float, float]:
    """The 24 coefficients A with old_rel = nl_trans(new_rel; A) in the least-squares sense: the direction map_coeff fits
    (stereo/dewarp.py:151-193) and warp / pivlfn_stereo_2d3c evaluate.  float64 NumPy, deterministic: a linear least-squares start on
    k * den = num, then damped Gauss-Newton on k - num / den, per axis.  Gauge A[8] = A[20] = 1; `order` 1 keeps the quadratic terms
    at 0.  Coordinates are scaled to unit size for the solve and the coefficients scaled back.  Fewer points than unknowns (11 per axis
    for order 2, 5 for order 1) is a ValueError.  Returns (A [24], residual RMS, residual maximum), the residuals in the units of
    old_rel (pixels), per point sqrt(dx^2 + dy^2)."""
    if order not in (1, 2):
        raise ValueError(f"fit_mapping: order={order} (1 or 2)")
    new = np.asarray(new_rel, dtype=np.float64).reshape(-1, 2)
    old = np.asarray(old_rel, dtype=np.float64).reshape(-1, 2)
    if new.shape != old.shape:
        raise ValueError("fit_mapping: new_rel and old_rel differ in length")
    unknowns = 11 if order == 2 else 5
    if len(new) < unknowns:
        raise ValueError(f"fit_mapping: {len(new)} points for {unknowns} unknowns per axis (order {order})")
    if not (np.all(np.isfinite(new)) and np.all(np.isfinite(old))):
        raise ValueError("fit_mapping: non-finite coordinates")
    s = float(np.max(np.abs(new)))
    s = s if s > 0 else 1.0
    p, q = new[:, 0] / s, new[:, 1] / s
    scale = np.array([s, s, 1.0, s * s, s * s, s * s])
    A = np.zeros(N_COEFF)
    for axis in range(2):
        c = _fit_axis(p, q, old[:, axis], order)
        A[12 * axis:12 * axis + 6] = c[:6] / scale
        A[12 * axis + 6:12 * axis + 12] = c[6:] / scale
    fx, fy = nl_trans(new[:, 0], new[:, 1], A)
    err = np.hypot(fx - old[:, 0], fy - old[:, 1])
    return A, float(np.sqrt(np.mean(err * err))), float(np.max(err))


def lattice_targets(ij: np.ndarray, spacing: Tuple[float, float]) -> np.ndarray:
    """The dewarped position of lattice node (i, j) relative to node (0, 0): (i * c_x, j * c_y)."""
    return np.asarray(ij, dtype=np.float64) * np.asarray(spacing, dtype=np.float64)


def calibrate_camera(image: torch.Tensor, template, ref4, threshold: float = 0.7, order: int = 2, cap: int = 4096,
                     border: bool = True) -> dict:
    """One camera: markers of `image` (uint8 [H,W], crosses bright) -> lattice indices from the four reference points `ref4` -> the
    mapping from the regular lattice, (i * c_x, j * c_y) about the first reference marker, to the image.  Returns a dict: "A" [24],
    "markers" [n,2], "records" [n,4], "ij" [n,2] (NOT_INDEXED rows for markers not reached), "indexed" bool [n], "selected" [4],
    "spacing" (c_x, c_y), "origin" (the first reference marker: pass it to dewarp_frames), "rms" and "max" (fit residuals, pixels).
    Synchronises (find_markers)."""
    image = _images(image, "calibrate_camera")
    if image.shape[0] != 1:
        raise ValueError("calibrate_camera: one image [H,W] expected")
    centres, records = find_markers(image, template, threshold, cap, border)
    pts = centres[0]
    if len(pts) < 4:
        raise ValueError(f"calibrate_camera: {len(pts)} markers found, at least the four reference markers are needed")
    ij, sel, spacing = index_lattice(pts, ref4)
    ok = ij[:, 0] != NOT_INDEXED
    origin = pts[sel[0]]
    A, rms, worst = fit_mapping(lattice_targets(ij[ok], spacing), pts[ok] - origin, order)
    return {"A": A, "markers": pts, "records": records[0], "ij": ij, "indexed": ok, "selected": sel, "spacing": spacing,
            "origin": (float(origin[0]), float(origin[1])), "rms": rms, "max": worst}


def write_coeff(path: str, left, right, calib: Optional[float] = None) -> dict:
    """{"Left": [24], "Right": [24], "calib": number} as pivlfn.stereo.read_coeff reads it (stereo_cal.py:55-79 wrote the same keys;
    `calib` is the mean over the cameras of c_x, stereo_cal.py:140,151).  Returns the dict written."""
    out = {}
    for side, a in (("Left", left), ("Right", right)):
        v = np.asarray(a, dtype=np.float64).reshape(-1)
        if v.shape != (N_COEFF,) or not np.all(np.isfinite(v)):
            raise ValueError(f"write_coeff: '{side}' must be {N_COEFF} finite numbers")
        out[side] = [float(x) for x in v]
    if calib is not None:
        if not np.isfinite(calib) or float(calib) == 0.0:
            raise ValueError("write_coeff: calib must be finite and non-zero")
        out["calib"] = float(calib)
    folder = os.path.dirname(os.path.abspath(path))
    os.makedirs(folder, exist_ok=True)
    with open(path, "w") as fp:
        json.dump(out, fp, indent=4)
    return out
