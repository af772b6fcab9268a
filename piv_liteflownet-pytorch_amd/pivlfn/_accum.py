"""What the streaming accumulators share: the device they live on, the base of those that hold one H x W size (its check, the check that
the frames given to update() are theirs, the enqueue-and-count tail of update()), the rank-ordered merge, the .npz writer and the loader
of a [2,H,W] pair of planes.  Private to the package; a new accumulator calls these and keeps only what is its own: its tensors, its
parameter checks, its entry-point call and its result() / finalize."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib


def cuda_device(device=None, refusal: Optional[str] = None) -> torch.device:
    """The indexed CUDA device `device` stands for: None and an unindexed "cuda" are the current one.  Any other kind of device raises
    NotImplementedError(refusal); with no `refusal` it is handed back as it is, for the caller whose later steps refuse it."""
    if device is not None:
        device = torch.device(device)
        if device.type != "cuda":
            if refusal is None:
                return device
            raise NotImplementedError(refusal)
        if device.index is not None:
            return device
    return torch.device("cuda", torch.cuda.current_device())


class FrameAccumulator:
    """The base of the accumulators of one H x W size: H, W, device and the frame count."""

    def __init__(self, H, W, device=None, fits: bool = True, tail: str = ""):
        """`fits`: what else the class asks of the size; `tail`: what its refusal says after it (" (positive, at most 16384 columns)")."""
        self.H, self.W = int(H), int(W)
        if self.H <= 0 or self.W <= 0 or not fits:
            raise ValueError(f"{type(self).__name__}: bad size {H} x {W}{tail}")
        self.device = cuda_device(device, f"{type(self).__name__}: GPU devices only")
        self.count = 0

    def _check_mine(self, size, device, given, mine: str = "accumulators [{H},{W}]", also: bool = True) -> None:
        """The frames given to update(), of `size` (H, W) on `device`, are of my size and on my device (and `also` holds), or
        ValueError("<class>.update: <given()>, <mine> on <my device>"); `given` is called for its words only then."""
        if tuple(size) != (self.H, self.W) or device != self.device or not also:
            raise ValueError(f"{type(self).__name__}.update: {given()}, {mine.format(H=self.H, W=self.W)} on {self.device}")

    def _enqueue(self, B: int, *calls) -> None:
        """The tail of update() for B frames: each of `calls`, (entry point of the library, *its arguments but the last), on the current
        stream of my device, in order; then count += B.  Nothing at all for B = 0; never synchronises the host."""
        if B == 0:
            return
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            for call in calls:
                rc = call[0](*call[1:], stream)
                if rc:
                    _lib.check(rc, f"{type(self).__name__}.update")
        self.count += B


def merge_sums(tensors: Sequence[torch.Tensor], count: int, group=None) -> int:
    """Collective over `group`: every rank ends with `tensors` (float64 sums, changed in place) of all ranks added in rank order -- the
    same bits on every rank -- and gets the summed count back.  Under gloo the exchange runs on host copies, as dist.gather_flows does."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    mine = torch.cat([t.reshape(-1) for t in tensors])
    if dist.get_backend(group) != "nccl":
        mine = mine.cpu()
    cnt = torch.tensor([count], dtype=torch.int64, device=mine.device)
    sums = [torch.empty_like(mine) for _ in range(world)]
    cnts = [torch.empty_like(cnt) for _ in range(world)]
    dist.all_gather(sums, mine, group=group)
    dist.all_gather(cnts, cnt, group=group)
    total = sums[0].clone()
    for s in sums[1:]:
        total += s
    for t, part in zip(tensors, total.split([t.numel() for t in tensors])):
        t.copy_(part.view(t.shape))
    return int(sum(int(c.item()) for c in cnts))


def save_npz(path: str, /, **members) -> str:
    """np.savez of `members` under `path`, with the suffix .npz added where it is missing; returns the path written."""
    if not path.endswith(".npz"):
        path += ".npz"
    np.savez(path, **members)
    return path


def load_planes(given, keys, what: str, H: int, W: int, device) -> Optional[torch.Tensor]:
    """None, a [2,H,W] tensor or array, or the path of a FlowStats file (its arrays `keys`): float64 on the device.  `what` names the
    planes in the refusal ("TwoPointStats: mean")."""
    if given is None:
        return None
    if isinstance(given, str):
        with np.load(given) as f:
            given = np.stack([f[keys[0]], f[keys[1]]])
    t = torch.as_tensor(given).detach().to(device=device, dtype=torch.float64).contiguous()
    if tuple(t.shape) != (2, H, W):
        raise ValueError(f"{what} {tuple(t.shape)}, expected [2,{H},{W}]")
    return t
