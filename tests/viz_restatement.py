"""numpy restatements of the kernels of csrc/viz.hip, in the arithmetic contract of include/pivlfn.h: flow_maxrad, flow_to_color,
field_absmax, scalar_to_color and flow_decimate.  Flows are [B,2,H,W] float32, masks [B,H,W] (nonzero = left out), pictures uint8
[B,H,W,3].  Every float32 step is one numpy float32 operation, so nothing is fused; the arctangent is numpy's float32 arctan2."""
import numpy as np

NCOLS = 55
F32 = np.float32


def wheel_table():
    """colorwheel / 255.0 of the reference's _makecolorwheel: [55,3] float64 (r, g, b)."""
    rows = []
    for seg, n in enumerate((15, 6, 4, 11, 13, 6)):
        for i in range(n):
            up = 255 * i / n
            rows.append(((255, up, 0), (255 - up, 255, 0), (0, 255, up), (0, 255 - up, 255), (up, 0, 255), (255, 0, 255 - up))[seg])
    table = np.array(rows, dtype=np.float64) / 255.0
    assert table.shape == (NCOLS, 3)
    return table


WHEEL = wheel_table()


def unknown(flow):
    """[B,2,H,W] -> bool [B,H,W]: NaN, or beyond 1e9 in a component."""
    u, v = flow[:, 0], flow[:, 1]
    with np.errstate(invalid="ignore"):
        return ~(np.fabs(u) <= F32(1e9)) | ~(np.fabs(v) <= F32(1e9))


def _left_out(flow, mask):
    out = unknown(flow)
    return out if mask is None else out | (np.asarray(mask) != 0)


def flow_maxrad(flow, mask=None):
    """float32 [B]: the largest sqrt(u*u + v*v) of each image over the vectors that stay; 0 where none does."""
    flow = np.asarray(flow, dtype=F32)
    with np.errstate(all="ignore"):
        rad = np.sqrt(flow[:, 0] * flow[:, 0] + flow[:, 1] * flow[:, 1])
    rad = np.where(_left_out(flow, mask), F32(0), rad)
    return rad.reshape(rad.shape[0], -1).max(axis=1).astype(F32) if rad[0].size else np.zeros(rad.shape[0], F32)


def flow_fk(flow, norm):
    """The float32 part of a pixel: (rad, fk) [B,H,W] for normalisers float32 [B] (0 stands for 1)."""
    flow = np.asarray(flow, dtype=F32)
    n = np.asarray(norm, dtype=F32).reshape(-1, 1, 1)
    n = np.where(n == 0, F32(1), n)
    with np.errstate(all="ignore"):
        fx, fy = flow[:, 0] / n, flow[:, 1] / n
        rad = np.sqrt(fx * fx + fy * fy)
        a = np.arctan2(-fy, -fx) / F32(np.pi)
        fk = (a + F32(1)) / F32(2) * F32(NCOLS - 1)
    assert rad.dtype == F32 and fk.dtype == F32
    return rad, fk


def flow_to_color(flow, norm, mask=None, wheel="interp", order="rgb"):
    """uint8 [B,H,W,3]."""
    flow = np.asarray(flow, dtype=F32)
    rad, fk = flow_fk(flow, norm)
    out_px = _left_out(flow, mask)
    fk = np.where(out_px, F32(0), fk)                    # left-out pixels are overwritten below; keep their index in range
    k0 = np.clip(fk.astype(np.int64), 0, NCOLS - 1)
    k1 = (k0 + 1) % NCOLS
    f = fk.astype(np.float64) - k0 if wheel == "interp" else np.zeros(fk.shape)
    radd = rad.astype(np.float64)
    img = np.zeros(fk.shape + (3,), np.uint8)
    for c in range(3):
        col = (1.0 - f) * WHEEL[k0, c] + f * WHEEL[k1, c]
        with np.errstate(invalid="ignore"):
            inside, beyond = rad <= F32(1), rad > F32(1)
            col = np.where(inside, 1.0 - radd * (1.0 - col), np.where(beyond, col * 0.75, col))
            level = 255.0 * col
            level = np.where(level >= 0, np.minimum(level, 255.0), 0.0)      # a NaN level stores 0
        img[..., c if order == "rgb" else 2 - c] = level.astype(np.int64)
    img[out_px] = 0
    return img


def field_absmax(field, mask=None):
    """float64 [B]: the largest magnitude among the finite, unmasked values of each image; 0 where none is left."""
    a = np.fabs(np.asarray(field).astype(np.float64))
    keep = np.isfinite(a) if mask is None else np.isfinite(a) & (np.asarray(mask) == 0)
    a = np.where(keep, a, 0.0)
    return a.reshape(a.shape[0], -1).max(axis=1)


def scalar_to_color(field, vmin, vmax, lut, mask=None, bad=(0, 0, 0)):
    """uint8 [B,H,W,3]: lut[clamp(floor((x - vmin) * (256 / (vmax - vmin))))], float64, the two operations rounded one by one."""
    x = np.asarray(field).astype(np.float64)
    scale = 256.0 / (float(vmax) - float(vmin))
    with np.errstate(all="ignore"):
        t = np.floor((x - float(vmin)) * scale)
    ok = np.isfinite(x) if mask is None else np.isfinite(x) & (np.asarray(mask) == 0)
    idx = np.where(t >= 0, np.minimum(t, 255.0), 0.0)
    idx = np.where(ok, idx, 0.0).astype(np.int64)
    img = np.asarray(lut, dtype=np.uint8)[idx]
    img[~ok] = np.asarray(bad, dtype=np.uint8)
    return img


def flow_decimate(flow, cell, mask=None):
    """(float32 [B,2,ch,cw] cell means, int32 [B,ch,cw] counts): float64 sums in row-major order within the cell, one division, one
    rounding to float32; 1e10 in an empty cell."""
    flow = np.asarray(flow, dtype=F32)
    B, _, H, W = flow.shape
    ch, cw = -(-H // cell), -(-W // cell)
    out_px = _left_out(flow, mask)
    mean = np.empty((B, 2, ch, cw), F32)
    count = np.empty((B, ch, cw), np.int32)
    for b in range(B):
        for i in range(ch):
            for j in range(cw):
                su, sv, n = 0.0, 0.0, 0
                for y in range(i * cell, min(H, (i + 1) * cell)):
                    for x in range(j * cell, min(W, (j + 1) * cell)):
                        if out_px[b, y, x]:
                            continue
                        su, sv, n = su + float(flow[b, 0, y, x]), sv + float(flow[b, 1, y, x]), n + 1
                mean[b, :, i, j] = (F32(su / n), F32(sv / n)) if n else F32(1e10)
                count[b, i, j] = n
    return mean, count


def flow_decimate_planes(flow, cell, mask=None):
    """flow_decimate, vectorised over the cells for images of millions of pixels: the pixels of a cell are added in the same row-major
    order, one float64 addition each, a left-out pixel as +0.0 (the sums start at +0.0 and so are never -0.0: adding +0.0 changes no
    bit).  flow_decimate stays the definition; tests/test_viz.py pins the two to each other."""
    flow = np.asarray(flow, dtype=F32)
    B, _, H, W = flow.shape
    ch, cw = -(-H // cell), -(-W // cell)
    keep = np.zeros((B, ch * cell, cw * cell), bool)
    keep[:, :H, :W] = ~_left_out(flow, mask)
    vals = np.zeros((B, 2, ch * cell, cw * cell), np.float64)
    vals[:, :, :H, :W] = flow
    vals = np.where(keep[:, None], vals, 0.0)
    s = np.zeros((B, 2, ch, cw), np.float64)
    n = np.zeros((B, ch, cw), np.int32)
    for dy in range(cell):
        for dx in range(cell):
            s = s + vals[:, :, dy::cell, dx::cell]
            n = n + keep[:, dy::cell, dx::cell]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(n[:, None] > 0, (s / n[:, None]).astype(F32), F32(1e10)).astype(F32)
    return mean, n.astype(np.int32)


def motion_to_color(flow, maxmotion=None, original_color=False):
    """The reference's entry point on the restatement: [H,W,2] or [L,H,W,2] float32 -> BGR uint8 of the same leading shape,
    normalised over the whole sequence."""
    seq = flow[None] if flow.ndim == 3 else flow
    nchw = np.ascontiguousarray(seq.transpose(0, 3, 1, 2))
    n = F32(maxmotion) if maxmotion is not None else flow_maxrad(nchw).max()
    img = flow_to_color(nchw, np.full(len(seq), n, F32), None, "original" if original_color else "interp", "bgr")
    return img[0] if flow.ndim == 3 else img
