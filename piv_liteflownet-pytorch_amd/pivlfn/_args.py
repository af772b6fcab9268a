"""Argument checks shared by the analysis modules: the integer range, the finite non-negative float, the flow, mask and image tensors,
the call of an entry point that wants a workspace, and the driver loop of the iterative solvers.  Private to the package; a new op calls these and keeps only what is its own."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib


def is_int(x, lo=None, hi=None) -> bool:
    """A plain int (no bool) inside [lo, hi]; None leaves a side open."""
    return not isinstance(x, bool) and isinstance(x, int) and (lo is None or lo <= x) and (hi is None or x <= hi)


def is_integer(x) -> bool:
    """An int or a NumPy integer (no bool): what sizes and seeds may be."""
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool)


def check_int(what: str, name: str, value, lo: int, hi: int, tail: str = "") -> None:
    """`tail` is what the message says after the range: ", the pixels of the window", " (3 x 3 to 31 x 31 vectors)"."""
    if not is_int(value, lo, hi):
        raise ValueError(f"{what}: {name}={value!r} must be an integer {lo}..{hi}{tail}")


def check_not_negative(what: str, name: str, value) -> float:
    value = float(value)
    if not math.isfinite(value) or value < 0.0:
        raise ValueError(f"{what}: {name}={value!r} must be finite and not negative")
    return value


def check_calib(calib) -> float:
    c = float(calib)
    if not math.isfinite(c) or c == 0.0:
        raise ValueError(f"calib={c!r} must be finite and non-zero")
    return c


def check_flows(flow, what: str, images: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B,2,H,W] float32 on the GPU, detached and contiguous; with `images` [B,C,H,W], of their batch, size and device."""
    if images is not None and isinstance(flow, torch.Tensor) and flow.dtype == torch.float32 and (
            flow.dim() != 4 or flow.size(1) != 2 or flow.device != images.device or flow.size(0) != images.size(0)
            or tuple(flow.shape[2:]) != tuple(images.shape[2:])):
        raise ValueError(f"{what}: flows {tuple(flow.shape)} on {flow.device} do not belong to images {tuple(images.shape)} on "
                         f"{images.device}")
    if not isinstance(flow, torch.Tensor):
        raise TypeError(f"{what}: expected a torch tensor [B,2,H,W], got {type(flow).__name__}")
    if flow.dtype != torch.float32:
        raise TypeError(f"{what}: expected float32 flows, got {flow.dtype}")
    if not flow.is_cuda:
        raise NotImplementedError(f"{what}: GPU tensors only")
    if flow.dim() != 4 or flow.size(1) != 2:
        raise ValueError(f"{what}: expected [B,2,H,W], got {tuple(flow.shape)}")
    return flow.detach().contiguous()


def check_mask(mask, what: str, truth: Optional[torch.Tensor] = None, shape=None, device=None) -> Optional[torch.Tensor]:
    """A uint8 or bool [B,H,W] mask (validate_flow's flag) as uint8, or None.  It belongs either to `truth` [B,2,H,W], which the
    message then names, or to a (B, H, W) `shape` on `device`."""
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool):
        raise TypeError(f"{what}: expected a uint8 or bool mask [B,H,W], got "
                        f"{mask.dtype if isinstance(mask, torch.Tensor) else type(mask).__name__}")
    if truth is not None:
        shape, device, owner = (truth.size(0), truth.size(2), truth.size(3)), truth.device, f"truth {tuple(truth.shape)}"
    else:
        owner = f"{tuple(shape)}"
    if mask.device != device or tuple(mask.shape) != tuple(shape):
        raise ValueError(f"{what}: mask {tuple(mask.shape)} on {mask.device} does not belong to {owner} on {device}")
    mask = mask.detach().contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def check_images(img1, img2, what: str):
    for name, t in (("img1", img1), ("img2", img2)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"{what}: expected a float32 tensor [B,C,H,W] for {name}, got "
                            f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
    if img1.dim() != 4 or img1.size(1) not in (1, 3):
        raise ValueError(f"{what}: expected images [B,C,H,W] with C = 1 or 3, got {tuple(img1.shape)}")
    if img2.shape != img1.shape or img2.device != img1.device:
        raise ValueError(f"{what}: img2 {tuple(img2.shape)} on {img2.device} does not belong to img1 {tuple(img1.shape)} on {img1.device}")
    return img1.detach().contiguous(), img2.detach().contiguous()


def ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def run_iterations(step, read, status: torch.Tensor, cap: int, sync_every: Optional[int]) -> None:
    """The driver loop of the iterative solvers (pressure, smooth): `step(n)` enqueues n iterations, `read()` enqueues the read-out that
    fills `status` [..., 4] (state first; 1 is RUNNING in both ABIs).  At most `cap` iterations are enqueued, `sync_every` at a time with
    a read-out in between that synchronises the host and ends the loop once no system is running; `sync_every=None` enqueues all `cap`
    at once and looks at nothing.  Either way one last read-out follows."""
    done = 0
    while done < cap:
        n = cap - done if sync_every is None else min(sync_every, cap - done)
        step(n)
        done += n
        if sync_every is not None and done < cap:
            read()
            if not bool((status[..., 0] == 1).any()):                        # synchronises
                break
    read()


def call_with_workspace(op: str, device, sizes, *args) -> None:
    """pivlfn_<op>(*args, workspace, its bytes, the current stream of `device`) with the workspace pivlfn_<op>_workspace_bytes(*sizes)
    asks for; a refusal is raised as _lib.check raises it."""
    lib = _lib.load()
    with torch.cuda.device(device):
        ws = torch.empty(getattr(lib, f"pivlfn_{op}_workspace_bytes")(*sizes), dtype=torch.uint8, device=device)
        _lib.check(getattr(lib, f"pivlfn_{op}")(*args, ws.data_ptr(), ws.numel(), _lib.stream_ptr(device)), op)
