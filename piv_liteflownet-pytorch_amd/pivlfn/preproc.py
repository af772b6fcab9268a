"""Image pre-processing of a recording on the device, in front of the network: removal of a static background (the per-pixel
minimum of the recording over time) and sliding min-max normalisation (Westerweel 1993; Adrian & Westerweel, Particle Image
Velocimetry, 2011), fused with the uint8 -> float32 conversion the network's input needs.

Runs on csrc/preproc.hip through the C ABI (`pivlfn_frames_preprocess`, `pivlfn_frames_background_min`; the arithmetic contract,
all integers up to one division, is written out in include/pivlfn.h):

    bg = FrameBackground(H, W, device)
    for frames in chunks:                                      # uint8 [n,H,W,3] on the device, what PairLoader uploads
        bg.update(frames)
    bg.save("background.png")

    x = preprocess_frames(frames, bg.image(), minmax=15)       # float32 [n,3,H,W] in [0,1], what `estimate` takes
    prep = Preprocessor(bg.image(), minmax=15)                 # the same as a callable: stream_pairs / run_sequence(prep=...)

With neither a background nor a window the result has the bits of `pipeline.u8_to_input`.  GPU only, like the rest of the package:
there is no CPU path.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _accum, _args, _lib


def check_params(minmax, floor) -> None:
    """The parameter checks of preprocess_frames (ValueError), usable before any frame exists."""
    if not (_args.is_int(minmax) and (minmax == 0 or (3 <= minmax <= 31 and minmax % 2 == 1))):
        raise ValueError(f"preprocess_frames: minmax={minmax!r} must be 0 (no normalisation) or an odd window size in 3..31")
    if not _args.is_int(floor, 1, 255):
        raise ValueError(f"preprocess_frames: floor={floor!r} must be an integer number of grey levels in 1..255")


def _check_frames(frames, what: str) -> torch.Tensor:
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
        raise TypeError(f"{what}: expected a uint8 frame tensor [n,H,W,3], got "
                        f"{frames.dtype if isinstance(frames, torch.Tensor) else type(frames).__name__}")
    if frames.device.type != "cuda":
        raise NotImplementedError(f"{what}: GPU tensors only (there is no CPU path)")
    if frames.dim() != 4 or frames.size(3) != 3 or frames.size(1) < 1 or frames.size(2) < 1:
        raise ValueError(f"{what}: expected frames [n,H,W,3] with H, W >= 1, got {tuple(frames.shape)}")
    return frames.detach().contiguous()


def _check_background(background, frames: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(background, torch.Tensor) or background.dtype != torch.uint8:
        raise TypeError(f"{what}: expected a uint8 background [H,W,3], got "
                        f"{background.dtype if isinstance(background, torch.Tensor) else type(background).__name__}")
    if background.device != frames.device or tuple(background.shape) != tuple(frames.shape[1:]):
        raise ValueError(f"{what}: background {tuple(background.shape)} on {background.device} does not belong to frames "
                         f"{tuple(frames.shape)} on {frames.device}")
    return background.detach().contiguous()


def preprocess_frames(frames_u8: torch.Tensor, background: Optional[torch.Tensor] = None, minmax: int = 0,
                      floor: int = 16) -> torch.Tensor:
    """uint8 [n,H,W,3] frames on the device -> float32 [n,3,H,W] in [0,1], one kernel enqueued on the current stream (no host
    synchronisation).  The three channels are treated independently and identically.

    `background` (uint8 [H,W,3], same device): subtracted first, clamped at 0.  `minmax` = k, an odd window size in 3..31: each pixel
    is stretched between the local minimum and maximum of its k x k neighbourhood, both smoothed by a k x k box filter, with the
    image edge replicated: (x - mean lo) / max(mean hi - mean lo, floor).  0 switches the normalisation off, and the frames are only
    divided by 255.  `floor`, in grey levels, is the smallest local contrast that is stretched to full scale: it keeps regions
    without particles from having their sensor noise amplified.  Its default of 16 grey levels is a parameter choice, not a measured
    optimum; choose it above the noise of the camera and below the dimmest particles worth keeping."""
    check_params(minmax, floor)
    frames = _check_frames(frames_u8, "preprocess_frames")
    bg = _check_background(background, frames, "preprocess_frames") if background is not None else None
    n, H, W, _ = frames.shape
    out = torch.empty([n, 3, H, W], dtype=torch.float32, device=frames.device)
    if n > 0:
        with torch.cuda.device(frames.device):
            _lib.check(_lib.load().pivlfn_frames_preprocess(frames.data_ptr(), bg.data_ptr() if bg is not None else None,
                                                            out.data_ptr(), n, H, W, minmax, floor, _lib.stream_ptr(frames.device)),
                       "preprocess_frames")
    return out


class Preprocessor:
    """preprocess_frames with its parameters bound: the `prep` callable of pipeline.stream_pairs and sequence.run_sequence."""

    def __init__(self, background: Optional[torch.Tensor] = None, minmax: int = 0, floor: int = 16):
        check_params(minmax, floor)
        self.background, self.minmax, self.floor = background, minmax, floor

    def __call__(self, frames_u8: torch.Tensor) -> torch.Tensor:
        return preprocess_frames(frames_u8, self.background, self.minmax, self.floor)


class FrameBackground(_accum.FrameAccumulator):
    """The per-pixel minimum of every frame seen: `min` uint8 [H,W,3] on the device, starting at 255, and the frame count.
    Particles are sparse and bright, so the minimum over a recording is its static background.  update() enqueues one kernel on the
    current stream and never synchronises the host."""

    def __init__(self, H: int, W: int, device=None):
        super().__init__(H, W, device)
        self.min = torch.full([self.H, self.W, 3], 255, dtype=torch.uint8, device=self.device)

    def update(self, frames_u8: torch.Tensor) -> None:
        """Take the frames of `frames_u8` [n,H,W,3] (uint8, on the accumulator's device) into the minimum."""
        frames = _check_frames(frames_u8, "FrameBackground.update")
        self._check_mine(frames.shape[1:3], frames.device, lambda: f"frames {tuple(frames.shape)} on {frames.device}",
                         "background [{H},{W},3]")
        n = frames.size(0)
        self._enqueue(n, (_lib.load().pivlfn_frames_background_min, frames.data_ptr(), self.min.data_ptr(), n, self.H, self.W))

    def image(self) -> torch.Tensor:
        """The background, uint8 [H,W,3] on the device (the accumulator itself, not a copy)."""
        return self.min

    def save(self, path: str) -> str:
        """Write the background as a lossless RGB PNG; returns the path written."""
        import PIL.Image
        PIL.Image.fromarray(self.min.cpu().numpy()).save(path, format="PNG")
        return path

    @classmethod
    def load(cls, path: str, device=None) -> "FrameBackground":
        """A background read back from an image file (as 8-bit RGB, like every frame); its frame count is unknown and set to 0."""
        from .pipeline import read_image_u8
        img = read_image_u8(path)
        bg = cls(img.shape[0], img.shape[1], device)
        bg.min.copy_(torch.from_numpy(np.ascontiguousarray(img)))
        return bg
