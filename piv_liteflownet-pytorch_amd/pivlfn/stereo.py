"""Stereoscopic PIV: two cameras' planar flows -> one 2D3C field (reference: stereo_run.py, stereo/dewarp.py, stereo/vel3d.py).

Per camera the flow is mapped through the rational-polynomial calibration (`nl_trans`, stereo/dewarp.py:255-270) and
optionally scaled to m/s (`_stereo_cal`, stereo_run.py:153-163); the two are then combined after Willert 1997 (`willert`,
stereo/vel3d.py:4-24).  All of it is one HIP kernel (`pivlfn_stereo_2d3c`, csrc/stereo.hip) that also does estimate()'s
output resize, so `estimate_stereo` runs one forward over an interleaved [L0, R0, L1, R1, ...] batch and writes the 3-band
payload directly.  The result is bit-identical to the reference's NumPy (>= 2) arithmetic cast to float32; the contract is
written out in include/pivlfn.h.  GPU only, like the rest of the package: CPU tensors raise NotImplementedError.

Host-side helpers (no GPU): `read_coeff` (the calibration JSON), `angles` / `tangents` (the degree -> radian conversion of
_flo_process, stereo_run.py:111-119), `scale_factor` (the calib rule of stereo_run.py:65-69), the left/right folder listing
and the flo-mode pairing of stereo_run.py.
"""
from __future__ import annotations

import ctypes
import json
import math
import numbers
import os
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib

N_COEFF = 24
SIDES = ("left", "right")


# ---- calibration and angles ----------------------------------------------------------------------------------------
def read_coeff(path: str) -> dict:
    """The mapping-coefficient JSON of stereo_run.py:44-58: {"Left": [24 numbers], "Right": [24 numbers], "calib": number
    (optional)}.  Returns a dict with exactly those keys (floats); anything malformed is a ValueError naming the problem."""
    if not os.path.isfile(path):
        raise ValueError(f"read_coeff: no such file: {path}")
    try:
        with open(path) as fp:
            raw = json.load(fp)
    except (json.JSONDecodeError, UnicodeDecodeError) as e:
        raise ValueError(f"read_coeff: {path} is not valid JSON ({e})") from None
    if not isinstance(raw, dict):
        raise ValueError(f"read_coeff: {path}: expected a JSON object with 'Left' and 'Right'")

    def number(v, what) -> float:
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
            raise ValueError(f"read_coeff: {path}: {what} must be a finite number, got {v!r}")
        return float(v)

    out = {}
    for side in ("Left", "Right"):
        if side not in raw:
            raise ValueError(f"read_coeff: {path}: missing '{side}' coefficients")
        vals = raw[side]
        if not isinstance(vals, list) or len(vals) != N_COEFF:
            raise ValueError(f"read_coeff: {path}: '{side}' must be a list of {N_COEFF} numbers")
        out[side] = [number(v, f"{side}[{k}]") for k, v in enumerate(vals)]
    if "calib" in raw:
        out["calib"] = number(raw["calib"], "'calib'")
        if out["calib"] == 0.0:
            raise ValueError(f"read_coeff: {path}: 'calib' must be non-zero (it divides --calib)")
    return out


def coeff_f32(coeff: dict) -> np.ndarray:
    """The 48 coefficients (left then right) as the kernel takes them: each rounded to float32, which is what NumPy does
    with a Python float multiplying a float32 array."""
    return np.array(coeff["Left"] + coeff["Right"], dtype=np.float64).astype(np.float32)


def _pair(v, what) -> Tuple[float, float]:
    vals = [v] if isinstance(v, numbers.Real) else list(v)
    if len(vals) not in (1, 2):
        raise ValueError(f"{what}: give one value (both cameras) or two (left, right), got {len(vals)}")
    return (float(vals[0]), float(vals[-1]))


def angles(theta_deg, alpha_deg) -> Tuple[List[np.float64], List[np.float64]]:
    """(theta, beta) in radians, [left, right], as _flo_process builds them (stereo_run.py:111-119): one value is used for
    both cameras, and the left camera's angles are negated."""
    th, al = _pair(theta_deg, "theta"), _pair(alpha_deg, "alpha")
    theta, beta = [], []
    for i in range(2):
        sign = (-1) ** (i + 1)
        beta.append(sign * np.deg2rad(al[i]))
        theta.append(sign * np.deg2rad(th[i]))
    return theta, beta


def tangents(theta, beta) -> np.ndarray:
    """float64 [tan theta_L, tan theta_R, tan beta_L, tan beta_R]: the np.tan scalars of willert (stereo/vel3d.py:19-23)."""
    return np.array([np.tan(theta[0]), np.tan(theta[1]), np.tan(beta[0]), np.tan(beta[1])], dtype=np.float64)


def scale_factor(coeff: dict, calib: Optional[float]) -> Optional[float]:
    """The `calibrate` argument of _stereo_cal: calib / coeff["calib"] when both are given (stereo_run.py:65-69), else None.
    _stereo_cal scales only when it is truthy (:160)."""
    if "calib" in coeff and calib:
        r = calib / coeff["calib"]
        return r if r else None
    return None


# ---- the kernel ------------------------------------------------------------------------------------------------------
def stereo_2d3c(flow: torch.Tensor, coeff: dict, tans, fps: float = 1, calib: Optional[float] = None,
                out_hw: Optional[Tuple[int, int]] = None, mul: Tuple[float, float] = (1.0, 1.0)) -> torch.Tensor:
    """`pivlfn_stereo_2d3c` over an interleaved [2B,2,h,w] flow (even entries left camera, odd right) -> [B,H,W,3] float32.
    `coeff` as read_coeff returns it; `tans` as `tangents` returns it; `fps` / `calib` as the CLI flags (`scale_factor`).
    `out_hw` (default (h, w)): when it differs from (h, w) each camera's flow is first resized exactly as estimate() does and
    multiplied by `mul` = (W/W', H/H')."""
    if not flow.is_cuda:
        raise NotImplementedError("stereo_2d3c: GPU tensors only")
    if flow.dim() != 4 or flow.size(1) != 2 or flow.size(0) % 2 or flow.size(0) == 0:
        raise ValueError(f"stereo_2d3c: expected [2B,2,h,w] (left and right interleaved), got {tuple(flow.shape)}")
    flow = flow.detach().contiguous().float()
    B, h, w = flow.size(0) // 2, flow.size(2), flow.size(3)
    H, W = out_hw if out_hw is not None else (h, w)
    out = torch.empty([B, H, W, 3], dtype=torch.float32, device=flow.device)
    c = coeff_f32(coeff)
    t = np.asarray(tans, dtype=np.float64)
    if c.shape != (2 * N_COEFF,) or t.shape != (4,):
        raise ValueError("stereo_2d3c: need 24 coefficients per camera and 4 tangents")
    s = scale_factor(coeff, calib)
    c_c = (ctypes.c_float * (2 * N_COEFF))(*c.tolist())
    t_c = (ctypes.c_double * 4)(*t.tolist())
    m_c = (ctypes.c_float * 2)(*mul)
    s_c = (ctypes.c_float * 2)(s, fps) if s is not None else None
    with torch.cuda.device(flow.device):
        _lib.check(_lib.load().pivlfn_stereo_2d3c(flow.data_ptr(), out.data_ptr(), B, h, w, H, W, m_c, c_c, s_c, t_c,
                                                  _lib.stream_ptr(flow.device)), "stereo_2d3c")
    return out


def interleave(left: torch.Tensor, right: torch.Tensor) -> torch.Tensor:
    """[B,...] x2 -> [2B,...] ordered L0, R0, L1, R1, ..."""
    if left.shape != right.shape:
        raise ValueError(f"left and right differ in shape: {tuple(left.shape)} vs {tuple(right.shape)}")
    return torch.stack([left, right], dim=1).reshape((2 * left.size(0),) + tuple(left.shape[1:]))


def estimate_interleaved(net, img1: torch.Tensor, img2: torch.Tensor, coeff: dict, tans, fps: float = 1,
                         calib: Optional[float] = None) -> torch.Tensor:
    """estimate()'s input adaptation and ONE forward of the interleaved [2B,3,H,W] pairs, then the fused kernel in place of
    the output resize -> [B,H,W,3]."""
    from .inference import _adapted_forward
    if img1.size(0) % 2:
        raise ValueError("estimate_stereo: the interleaved batch needs a left and a right pair per step")
    raw, H, W, sw, sh = _adapted_forward(net, img1, img2)
    return stereo_2d3c(raw, coeff, tans, fps, calib, out_hw=(H, W), mul=(sw, sh))


def estimate_stereo(net, l1: torch.Tensor, l2: torch.Tensor, r1: torch.Tensor, r2: torch.Tensor, coeff: dict,
                    theta_deg=45.0, alpha_deg=0.0, fps: float = 1, calib: Optional[float] = None, tensor: bool = False):
    """One stereo step per batch entry: the left pair (l1, l2) and the right pair (r1, r2), each [B,3,H,W] in [0,1] on the
    network's device -> the 2D3C field, [B,H,W,3] tensor with `tensor=True`, else numpy ([H,W,3] for B = 1, the layout
    of a 3-band .flo).  Equal to `stereo_2d3c` applied to estimate() of each camera, bit for bit."""
    theta, beta = angles(theta_deg, alpha_deg)
    out = estimate_interleaved(net, interleave(l1, r1), interleave(l2, r2), coeff, tangents(theta, beta), fps, calib)
    if tensor:
        return out
    arr = out.cpu().numpy()
    return arr[0] if arr.shape[0] == 1 else arr


# ---- folders and files -----------------------------------------------------------------------------------------------
def stereo_folders(root: str) -> Tuple[str, str]:
    """(left, right): the sub-directories of `root` named left / right in any case.  Nothing else is accepted (the reference
    takes the first two directories os.walk returns, stereo_run.py:95-98)."""
    if not os.path.isdir(root):
        raise ValueError(f"stereo input directory not found: {root}")
    found = {s: [] for s in SIDES}
    for n in sorted(os.listdir(root)):
        if n.lower() in found and os.path.isdir(os.path.join(root, n)):
            found[n.lower()].append(n)
    for s in SIDES:
        if len(found[s]) != 1:
            what = "no" if not found[s] else f"{len(found[s])} ({', '.join(found[s])})"
            raise ValueError(f"{root}: need exactly one '{s}' folder (any case), found {what}")
    return os.path.join(root, found["left"][0]), os.path.join(root, found["right"][0])


class StereoSequence:
    """The frame sequences of <root>/left and <root>/right as an interleaved pair list for pivlfn.pipeline.PairLoader:
    pairs 2k and 2k+1 are step k, (L_k, L_k+1) and (R_k, R_k+1), each called by its first frame's stem."""

    def __init__(self, root: str):
        from .datasets import image_files_from_folder
        self.left_dir, self.right_dir = stereo_folders(root)
        self.left = image_files_from_folder(self.left_dir, pair=False)
        self.right = image_files_from_folder(self.right_dir, pair=False)
        if len(self.left) != len(self.right):
            raise ValueError(f"{root}: {len(self.left)} left frames but {len(self.right)} right frames")
        if len(self.left) < 2:
            raise ValueError(f"{root}: a stereo sequence needs at least two frames per camera, found {len(self.left)}")
        self.image_list, self.name_list = [], []
        for k in range(len(self.left) - 1):
            for files in (self.left, self.right):
                self.image_list.append([files[k], files[k + 1]])
                self.name_list.append(os.path.splitext(os.path.basename(files[k]))[0])

    @property
    def steps(self) -> int:
        return len(self.left) - 1

    def camera(self, side: str) -> "_Camera":
        return _Camera(self.image_list[SIDES.index(side)::2], self.name_list[SIDES.index(side)::2])

    def direct_names(self) -> List[str]:
        """<left stem rsplit('_', 1)[0]>_2d3c.flo per step (stereo_run.py:87); two steps with one name are an error."""
        names = [self.name_list[2 * k].rsplit("_", 1)[0] + "_2d3c.flo" for k in range(self.steps)]
        seen = {}
        for k, n in enumerate(names):
            if n in seen:
                raise ValueError(f"steps {seen[n]} and {k} would both write {n} (frame names "
                                 f"{self.name_list[2 * seen[n]]!r}, {self.name_list[2 * k]!r})")
            seen[n] = k
        return names


class _Camera:
    """One camera's consecutive pairs, in the shape PairLoader reads."""

    def __init__(self, image_list, name_list):
        self.image_list, self.name_list = list(image_list), list(name_list)

    def __len__(self):
        return len(self.name_list)


def flo_pairs(save: str) -> List[Tuple[str, str, str]]:
    """(left .flo, right .flo, output .flo) of _flo_process (stereo_run.py:121-146): for every <save>/left/*.flo, sorted,
    base = name.rsplit('-', 1)[0], the right flow is <save>/right/<base>-R_out.flo and the result <save>/stereo/<base>-S_out.flo.
    Every right file is checked before anything is computed: a missing one is a FileNotFoundError listing them all."""
    import glob
    if not os.path.isdir(save):
        raise ValueError(f"flo mode: directory not found: {save}")
    lefts = sorted(glob.glob(os.path.join(glob.escape(save), "left", "*.flo")))
    if not lefts:
        raise ValueError(f"flo mode: no .flo files in {os.path.join(save, 'left')}")
    out, missing = [], []
    for lf in lefts:
        base = os.path.basename(lf).rsplit("-", 1)[0]
        rf = os.path.join(save, "right", base + "-R_out.flo")
        if not os.path.isfile(rf):
            missing.append(rf)
        out.append((lf, rf, os.path.join(save, "stereo", base + "-S_out.flo")))
    if missing:
        raise FileNotFoundError(f"flo mode: {len(missing)} right-camera flow(s) missing: " + ", ".join(missing))
    names = [o for _, _, o in out]
    if len(set(names)) != len(names):
        raise ValueError("flo mode: two left flows map to the same output name")
    return out
