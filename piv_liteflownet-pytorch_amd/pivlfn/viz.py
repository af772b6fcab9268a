"""Pictures of flows and scalar fields: the reference's `motion_to_color` (src/utils_plot.py:199-256, src/utils_color.py) on the
device, a colour map for scalar fields such as the vorticity, decimated quiver plots and PNG output.

The colouring runs on csrc/viz.hip through the C ABI (`pivlfn_flow_maxrad`, `pivlfn_flow_to_color`, `pivlfn_field_absmax`,
`pivlfn_scalar_to_color`, `pivlfn_flow_decimate`; the arithmetic contract is written out in include/pivlfn.h):

    rgb = flow_to_color(flows)                                   # [B,2,H,W] on the device -> uint8 [B,H,W,3], no host synchronisation
    bgr = motion_to_color(flow_hw2)                              # numpy drop-in with the reference's shapes and channel order
    img = vorticity_image(flows, calib)                          # blue-white-red, symmetric about 0
    mean, count = decimate_flow(flows, 16)                       # cell means for arrows
    quiver_plot(flow_hw2, filename="q.png")                      # at most 64 arrows per axis (needs matplotlib)
    with PngWriter() as w: w.submit(rgb_hw3, "a.png")            # background threads, as flo.FloWriter

One deliberate difference from the reference: unknown vectors (NaN, or beyond 1e9 in a component -- what `--validate mask` writes) are
left out of the maximum that normalises a picture, as in the Middlebury color_flow.cpp.  The reference's `rad.max()` includes them, so
one such vector turns its whole picture white.  On flows without unknown vectors the two agree.

GPU only, like the rest of the package: there is no CPU path.
"""
from __future__ import annotations

import math
import queue
import threading
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import _accum, _args, _lib
from .postpro import flow_fields

WHEELS = {"interp": 0, "original": 1}          # PIVLFN_WHEEL_INTERP, PIVLFN_WHEEL_ORIGINAL
ORDERS = {"rgb": 0, "bgr": 1}                  # PIVLFN_ORDER_RGB, PIVLFN_ORDER_BGR
PNG_COMPRESS_LEVEL = 1                         # zlib level of write_png: the files are intermediate pictures, written once per pair


def _lut_bwr() -> np.ndarray:
    """Blue - white - red, 256 x 3 uint8: entry i at x = i / 255 is (min(2x, 1), 1 - |2x - 1|, min(2 - 2x, 1)), rounded to nearest."""
    x = np.arange(256, dtype=np.float64) / 255.0
    rgb = np.stack([np.minimum(2 * x, 1.0), 1.0 - np.abs(2 * x - 1.0), np.minimum(2.0 - 2 * x, 1.0)], axis=1)
    return np.floor(255.0 * rgb + 0.5).astype(np.uint8)


def _lut_gray() -> np.ndarray:
    return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)


LUTS = {"bwr": _lut_bwr(), "gray": _lut_gray()}
_DEVICE_LUTS: dict = {}


def _lut_on(cmap, device) -> torch.Tensor:
    if isinstance(cmap, str):
        if cmap not in LUTS:
            raise ValueError(f"unknown colour map {cmap!r} (one of {', '.join(LUTS)}, or a 256 x 3 uint8 table)")
        key = (cmap, str(device))
        if key not in _DEVICE_LUTS:
            _DEVICE_LUTS[key] = torch.from_numpy(LUTS[cmap]).to(device)
        return _DEVICE_LUTS[key]
    if isinstance(cmap, np.ndarray):
        cmap = torch.from_numpy(np.ascontiguousarray(cmap))
    if not isinstance(cmap, torch.Tensor) or cmap.dtype != torch.uint8 or tuple(cmap.shape) != (256, 3):
        raise TypeError("a colour map is a name or a 256 x 3 uint8 table, got "
                        f"{tuple(cmap.shape) if hasattr(cmap, 'shape') else type(cmap).__name__}"
                        f"{' of ' + str(cmap.dtype) if hasattr(cmap, 'dtype') else ''}")
    return cmap.to(device).contiguous()


def _maxmotion(maxmotion) -> float:
    m = float(maxmotion)
    if not math.isfinite(m) or m < 0.0:
        raise ValueError(f"maxmotion={m!r} must be finite and not negative (0 stands for 1, as in the reference)")
    return m


def flow_maxrad(flow: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B,2,H,W] float32 flows on the device -> float32 [B]: the largest vector length of each image over the vectors that are
    neither unknown nor masked (0 where none is left).  Enqueued on the current stream."""
    flow = _args.check_flows(flow, "flow_maxrad")
    B, _, H, W = flow.shape
    mask = _args.check_mask(mask, "flow_maxrad", shape=(B, H, W), device=flow.device)
    out = torch.empty([B], dtype=torch.float32, device=flow.device)
    if B > 0:
        with torch.cuda.device(flow.device):
            _lib.check(_lib.load().pivlfn_flow_maxrad(flow.data_ptr(), _args.ptr(mask), out.data_ptr(), B, H, W, _lib.stream_ptr(flow.device)),
                       "flow_maxrad")
    return out


def flow_to_color(flow: torch.Tensor, maxmotion=None, scope: str = "image", wheel: str = "interp", order: str = "rgb",
                  mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B,2,H,W] float32 flows on the device -> uint8 [B,H,W,3] in the Middlebury colour coding, enqueued on the current stream with
    no host synchronisation.  Every image is normalised by `maxmotion` when it is given, else by its own largest vector length
    (`scope="image"`) or the largest of the batch (`scope="batch"`); that maximum stays on the device.  `wheel`: "interp" (the
    reference's default) or "original" (`original_color=True`).  `order`: "rgb" for image files, "bgr" is what the reference returns.
    Unknown vectors and pixels with a nonzero `mask` byte ([B,H,W]; validate_flow's flag) are black and do not enter the maximum."""
    if scope not in ("image", "batch"):
        raise ValueError(f"flow_to_color: unknown scope {scope!r} (image or batch)")
    if wheel not in WHEELS:
        raise ValueError(f"flow_to_color: unknown wheel {wheel!r} (one of {', '.join(WHEELS)})")
    if order not in ORDERS:
        raise ValueError(f"flow_to_color: unknown order {order!r} (one of {', '.join(ORDERS)})")
    flow = _args.check_flows(flow, "flow_to_color")
    B, _, H, W = flow.shape
    mask = _args.check_mask(mask, "flow_to_color", shape=(B, H, W), device=flow.device)
    out = torch.empty([B, H, W, 3], dtype=torch.uint8, device=flow.device)
    if B == 0:
        return out
    if maxmotion is not None:
        norm = torch.full([B], _maxmotion(maxmotion), dtype=torch.float32, device=flow.device)
    else:
        norm = flow_maxrad(flow, mask)
        if scope == "batch":
            norm = norm.max().expand(B).contiguous()
    with torch.cuda.device(flow.device):
        _lib.check(_lib.load().pivlfn_flow_to_color(flow.data_ptr(), norm.data_ptr(), _args.ptr(mask), out.data_ptr(), B, H, W, WHEELS[wheel],
                                                    ORDERS[order], _lib.stream_ptr(flow.device)), "flow_to_color")
    return out


def _numpy_flows(flow, what: str) -> Tuple[torch.Tensor, bool]:
    """[H,W,2] or [L,H,W,2] float32 numpy -> ([L,2,H,W] on the current device, whether a single field came in)."""
    if not isinstance(flow, np.ndarray) or flow.dtype != np.float32:
        raise TypeError(f"{what}: expected a float32 numpy flow [H,W,2] or [L,H,W,2], got "
                        f"{flow.dtype if isinstance(flow, np.ndarray) else type(flow).__name__} (converting it would change the "
                        "reference's values)")
    if flow.ndim not in (3, 4) or flow.shape[-1] != 2:
        raise ValueError(f"{what}: expected a flow [H,W,2] or [L,H,W,2], got shape {flow.shape}")
    if not torch.cuda.is_available():
        raise NotImplementedError(f"{what}: needs a GPU (there is no CPU path)")
    dev = _accum.cuda_device()
    seq = flow[None] if flow.ndim == 3 else flow
    return torch.from_numpy(np.ascontiguousarray(seq.transpose(0, 3, 1, 2))).to(dev), flow.ndim == 3


def motion_to_color(flow, maxmotion=None, verbose=False, original_color: bool = False):
    """src/utils_plot.py:199-256 on the GPU: [H,W,2] -> [H,W,3], [L,H,W,2] -> [L,H,W,3] normalised over the whole sequence; uint8 in
    the reference's channel order (BGR).  `maxmotion` is taken as a float32, which is what NumPy makes of a Python float there."""
    t, single = _numpy_flows(flow, "motion_to_color")
    if verbose:
        n = _maxmotion(maxmotion) if maxmotion is not None else float(flow_maxrad(t).max()) if t.size(0) else 0.0
        print("normalizing by {}".format(n if n != 0 else 1))
    out = flow_to_color(t, maxmotion, scope="batch", wheel="original" if original_color else "interp", order="bgr").cpu().numpy()
    return out[0] if single else out


def _check_field(field, what: str) -> torch.Tensor:
    if not isinstance(field, torch.Tensor):
        raise TypeError(f"{what}: expected a torch tensor [B,H,W], got {type(field).__name__}")
    if field.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{what}: expected a float32 or float64 field, got {field.dtype}")
    if not field.is_cuda:
        raise NotImplementedError(f"{what}: GPU tensors only")
    if field.dim() != 3:
        raise ValueError(f"{what}: expected [B,H,W], got {tuple(field.shape)}")
    return field.detach().contiguous()


def field_absmax(field: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B,H,W] float32 or float64 on the device -> float64 [B]: the largest magnitude among the finite, unmasked values of each
    image (0 where none is left).  Enqueued on the current stream."""
    field = _check_field(field, "field_absmax")
    B, H, W = field.shape
    mask = _args.check_mask(mask, "field_absmax", shape=(B, H, W), device=field.device)
    out = torch.empty([B], dtype=torch.float64, device=field.device)
    if B > 0:
        with torch.cuda.device(field.device):
            _lib.check(_lib.load().pivlfn_field_absmax(field.data_ptr(), int(field.dtype == torch.float64), _args.ptr(mask), out.data_ptr(),
                                                       B, H, W, _lib.stream_ptr(field.device)), "field_absmax")
    return out


def _bad_rgb(bad) -> int:
    try:
        r, g, b = (int(c) for c in bad)
    except (TypeError, ValueError):
        raise ValueError(f"bad={bad!r} must be three byte values (r, g, b)") from None
    if not all(0 <= c <= 255 for c in (r, g, b)):
        raise ValueError(f"bad={bad!r} must be three byte values (r, g, b)")
    return (r << 16) | (g << 8) | b


def scalar_to_color(field: torch.Tensor, vmin=None, vmax=None, cmap: Union[str, np.ndarray, torch.Tensor] = "bwr",
                    symmetric: bool = False, mask: Optional[torch.Tensor] = None, bad=(0, 0, 0)) -> torch.Tensor:
    """[B,H,W] float32 or float64 on the device -> uint8 [B,H,W,3] (r, g, b) through a 256-entry colour map: "bwr" (blue - white -
    red), "gray", or a 256 x 3 uint8 table.  [vmin, vmax) is cut into 256 equal bins; values outside take the end colours, non-finite
    values and pixels with a nonzero `mask` byte take `bad`.  `symmetric`: the range is [-vmax, vmax]; without `vmax` every image
    takes its own largest magnitude (field_absmax; that reads B numbers back, the only host synchronisation here; 0 stands for 1)."""
    field = _check_field(field, "scalar_to_color")
    B, H, W = field.shape
    mask = _args.check_mask(mask, "scalar_to_color", shape=(B, H, W), device=field.device)
    lut = _lut_on(cmap, field.device)
    bad_rgb = _bad_rgb(bad)
    if symmetric:
        if vmin is not None:
            raise ValueError("scalar_to_color: symmetric=True takes vmax alone (the range is [-vmax, vmax])")
        ranges = None if vmax is None else [(-abs(float(vmax)), abs(float(vmax)))] * B
    else:
        if vmin is None or vmax is None:
            raise ValueError("scalar_to_color: give vmin and vmax, or symmetric=True")
        ranges = [(float(vmin), float(vmax))] * B
    for lo, hi in ranges or ():
        if not (math.isfinite(lo) and math.isfinite(hi)) or lo == hi:
            raise ValueError(f"scalar_to_color: the range vmin={lo!r} vmax={hi!r} must be finite and not empty")
    out = torch.empty([B, H, W, 3], dtype=torch.uint8, device=field.device)
    if B == 0:
        return out
    if ranges is None:
        ranges = [(-(m or 1.0), m or 1.0) for m in field_absmax(field, mask).tolist()]
    is_f64 = int(field.dtype == torch.float64)
    lib = _lib.load()
    with torch.cuda.device(field.device):
        st = _lib.stream_ptr(field.device)
        if all(r == ranges[0] for r in ranges):
            _lib.check(lib.pivlfn_scalar_to_color(field.data_ptr(), is_f64, _args.ptr(mask), lut.data_ptr(), out.data_ptr(), B, H, W,
                                                  ranges[0][0], ranges[0][1], bad_rgb, st), "scalar_to_color")
        else:
            for b, (lo, hi) in enumerate(ranges):
                _lib.check(lib.pivlfn_scalar_to_color(field[b].data_ptr(), is_f64, _args.ptr(mask[b]) if mask is not None else None,
                                                      lut.data_ptr(), out[b].data_ptr(), 1, H, W, lo, hi, bad_rgb, st), "scalar_to_color")
    return out


def vorticity_image(flow: torch.Tensor, calib=1.0, kind: str = "calc_vorticity", vmax=None, cmap="bwr",
                    mask: Optional[torch.Tensor] = None, bad=(0, 0, 0)) -> torch.Tensor:
    """[B,2,H,W] float32 flows on the device -> uint8 [B,H,W,3]: the vorticity plane of flow_fields(flow, calib, kind) through
    scalar_to_color, symmetric about 0 (white), `vmax` or each image's own largest magnitude at the ends."""
    vort = flow_fields(flow, calib, kind)[:, 0].contiguous()
    return scalar_to_color(vort, vmax=vmax, cmap=cmap, symmetric=True, mask=mask, bad=bad)


def decimate_flow(flow: torch.Tensor, cell: int, mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """[B,2,H,W] float32 flows on the device -> (float32 [B,2,ceil(H/cell),ceil(W/cell)] cell means, int32 [B,.,.] counts of the
    vectors averaged).  Unknown and masked vectors are left out; a cell with none is 1e10 in both components."""
    if not _args.is_int(cell, 1, 32768):
        raise ValueError(f"decimate_flow: cell={cell!r} must be an integer from 1 to 32768")
    flow = _args.check_flows(flow, "decimate_flow")
    B, _, H, W = flow.shape
    mask = _args.check_mask(mask, "decimate_flow", shape=(B, H, W), device=flow.device)
    ch, cw = -(-H // cell), -(-W // cell)
    mean = torch.empty([B, 2, ch, cw], dtype=torch.float32, device=flow.device)
    count = torch.empty([B, ch, cw], dtype=torch.int32, device=flow.device)
    if B > 0:
        with torch.cuda.device(flow.device):
            _lib.check(_lib.load().pivlfn_flow_decimate(flow.data_ptr(), _args.ptr(mask), mean.data_ptr(), count.data_ptr(), B, H, W, cell,
                                                        _lib.stream_ptr(flow.device)), "decimate_flow")
    return mean, count


def quiver_cell(H: int, W: int, arrows: int = 64) -> int:
    """The smallest cell that leaves at most `arrows` arrows along either axis."""
    return max(1, -(-max(H, W) // arrows))


def _pyplot():
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError as e:
        raise ImportError(f"quiver plots need matplotlib, which could not be imported ({e}); install it, or use flow_to_color, which "
                          "needs nothing beyond the package") from e
    return plt


def quiver_plot(flow: np.ndarray, coord: Optional[np.ndarray] = None, filename: Optional[str] = None, norm: bool = False,
                show: bool = False, cell: Optional[int] = None):
    """src/utils_plot.py:161-192 with one arrow per `cell` x `cell` block and not per pixel: the block means come from decimate_flow
    on the GPU (unknown vectors left out, empty blocks not drawn), `cell=None` picks quiver_cell().  `coord` [H,W,2] positions are
    averaged over the same blocks.  `norm`: the arrows are divided by the largest vector length (+ float32 eps), as _normalize_flow."""
    _pyplot()                                  # before anything is uploaded: a missing matplotlib is the first thing reported
    t, single = _numpy_flows(flow, "quiver_plot")
    if not single:
        raise ValueError(f"quiver_plot: expected one flow [H,W,2], got shape {flow.shape}")
    H, W = flow.shape[:2]
    if filename is not None and not (isinstance(filename, str) and filename.endswith(".png")):
        raise ValueError(f"quiver_plot: filename {filename!r} must end in .png")
    cell = quiver_cell(H, W) if cell is None else cell
    mean, count = decimate_flow(t, cell)
    mean = mean[0].cpu().numpy()
    if norm:
        mean = mean / (np.float32(float(flow_maxrad(t)[0])) + np.finfo(np.float32).eps)
    centres = None
    if coord is not None:
        if not isinstance(coord, np.ndarray) or coord.shape != (H, W, 2):
            raise ValueError(f"quiver_plot: coord must be [{H},{W},2], got {getattr(coord, 'shape', type(coord).__name__)}")
        centres = decimate_flow(_numpy_flows(np.ascontiguousarray(coord, dtype=np.float32), "quiver_plot")[0], cell)[0][0].cpu().numpy()
    draw_quiver(mean, count[0].cpu().numpy(), cell, H, W, filename, show, centres)


def draw_quiver(mean: np.ndarray, count: np.ndarray, cell: int, H: int, W: int, filename: Optional[str] = None, show: bool = False,
                centres: Optional[np.ndarray] = None) -> None:
    """The arrows of decimate_flow's (mean [2,ch,cw], count [ch,cw]) for an H x W field, at `centres` [2,ch,cw] or at the middle of
    every cell with y upwards (the reference's layout); cells without a vector are not drawn."""
    plt = _pyplot()
    u, v = mean
    drawn = count > 0
    if centres is None:
        edges_x, edges_y = np.minimum(np.arange(u.shape[1] + 1) * cell, W), np.minimum(np.arange(u.shape[0] + 1) * cell, H)
        xp, yp = np.meshgrid((edges_x[:-1] + edges_x[1:]) / 2.0, H - (edges_y[:-1] + edges_y[1:]) / 2.0)
    else:
        xp, yp = centres
    plt.quiver(xp[drawn], yp[drawn], u[drawn], v[drawn])
    plt.axis("equal")
    if show:
        plt.show()
    if filename is not None:
        plt.savefig(filename)
    plt.clf()


def color_wheel_image(size: int = 151, wheel: str = "interp", order: str = "rgb", device=None) -> torch.Tensor:
    """The legend, uint8 [size,size,3] on the device: the vectors of the unit disc (x to the right, y down, as the flows of an image)
    through the kernel that colours the flows, normalised by 1; white outside the disc."""
    if not _args.is_int(size, 1):
        raise ValueError(f"color_wheel_image: size={size!r} must be a positive integer")
    device = _accum.cuda_device(device, "color_wheel_image: GPU devices only")
    half = max(size - 1, 1) / 2.0                 # exactly 0 in the middle of an odd size and exactly -1, 1 at the ends
    ax = (torch.arange(size, dtype=torch.float32, device=device) - (size - 1) / 2.0) / half
    v, u = torch.meshgrid(ax, ax, indexing="ij")
    inside = (u * u + v * v <= 1.0).to(torch.float32)
    return flow_to_color(torch.stack([u * inside, v * inside])[None], maxmotion=1.0, wheel=wheel, order=order)[0]


def write_png(path: str, rgb: np.ndarray, compress_level: int = PNG_COMPRESS_LEVEL) -> None:
    """uint8 [H,W,3] (r, g, b) -> a PNG file."""
    import PIL.Image
    if not isinstance(rgb, np.ndarray) or rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise TypeError(f"write_png: expected a uint8 array [H,W,3], got "
                        f"{rgb.dtype if isinstance(rgb, np.ndarray) else type(rgb).__name__} {getattr(rgb, 'shape', '')}")
    PIL.Image.fromarray(np.ascontiguousarray(rgb), "RGB").save(path, format="PNG", compress_level=compress_level)


def write_png_gray(path: str, gray: np.ndarray, compress_level: int = PNG_COMPRESS_LEVEL) -> None:
    """uint8 [H,W] -> an 8-bit grey PNG file (a particle image): write_png's sibling for one channel."""
    import PIL.Image
    if not isinstance(gray, np.ndarray) or gray.dtype != np.uint8 or gray.ndim != 2:
        raise TypeError(f"write_png_gray: expected a uint8 array [H,W], got "
                        f"{gray.dtype if isinstance(gray, np.ndarray) else type(gray).__name__} {getattr(gray, 'shape', '')}")
    PIL.Image.fromarray(np.ascontiguousarray(gray), "L").save(path, format="PNG", compress_level=compress_level)


class PngWriter:
    """Background writer, as flo.FloWriter: submit(rgb_hw3, path) returns immediately; close() drains.  Errors surface on close()."""

    def __init__(self, workers: int = 4, depth: int = 64, compress_level: int = PNG_COMPRESS_LEVEL):
        self._q: "queue.Queue" = queue.Queue(maxsize=depth)
        self._err = []
        self._level = compress_level
        self._threads = [threading.Thread(target=self._run, daemon=True) for _ in range(max(1, workers))]
        for t in self._threads:
            t.start()

    def _run(self):
        while True:
            item = self._q.get()
            if item is None:
                return
            try:
                self._write(item[1], item[0])
            except Exception as e:          # noqa: BLE001
                self._err.append(e)

    def _write(self, path: str, image: np.ndarray) -> None:
        write_png(path, image, self._level)

    def submit(self, rgb: np.ndarray, filename: str) -> None:
        self._q.put((rgb, filename))

    def close(self) -> None:
        for _ in self._threads:
            self._q.put(None)
        for t in self._threads:
            t.join()
        if self._err:
            raise self._err[0]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class GrayPngWriter(PngWriter):
    """PngWriter for 8-bit grey images: submit(gray_hw, path)."""

    def _write(self, path: str, image: np.ndarray) -> None:
        write_png_gray(path, image, self._level)
