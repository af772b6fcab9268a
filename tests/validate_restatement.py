"""NumPy restatement of the vector-validation contract of include/pivlfn.h (pivlfn_flow_validate: the normalized median test of
Westerweel & Scarano 2005 with masking / median replacement) and of pivlfn_flow_stats_accumulate_masked: plain loops over the
pixels, np.sort, np.float32 scalars, every rounding on its own.  There is no reference implementation to pin it to;
tests/test_validate.py checks it against hand-computed cases, and the GPU tests compare the kernels with it bit for bit."""
import numpy as np

from postpro_restatement import calc_vorticity

f32, f64 = np.float32, np.float64
OUTLIER, UNKNOWN, NOT_REPLACED = 1, 2, 4
MASKED = f32(1e10)
UNKNOWN_THRESH = f32(1e9)
ZERO, HALF = f32(0.0), f32(0.5)


def unknown(u, v):
    """The reference's _unknown_flow on float32 scalars."""
    return bool(np.isnan(u) or np.isnan(v) or abs(u) > UNKNOWN_THRESH or abs(v) > UNKNOWN_THRESH)


def median(values):
    """Median of n >= 1 float32 values: the middle one, or (a[n/2-1] + a[n/2]) * 0.5f."""
    a = np.sort(np.asarray(values, dtype=f32))
    n = len(a)
    if n % 2:
        return a[(n - 1) // 2]
    return f32(f32(a[n // 2 - 1] + a[n // 2]) * HALF)


def _offsets(radius, spacing):
    return [(i * spacing, j * spacing) for i in range(-radius, radius + 1) for j in range(-radius, radius + 1) if (i, j) != (0, 0)]


def detect(flow, radius=1, spacing=1, eps=0.1, thresh=2.0, rows=None):
    """Pass 1 on one frame.  flow [2,H,W] float32 -> (flag uint8 [H,W], resid float32 [2,H,W]); with `rows`, only those rows are
    computed (the others hold flag 255 / NaN)."""
    flow = np.asarray(flow)
    assert flow.dtype == f32 and flow.ndim == 3 and flow.shape[0] == 2 and radius in (1, 2) and spacing >= 1
    _, H, W = flow.shape
    eps, thresh = f32(eps), f32(thresh)
    u, v = flow[0] + ZERO, flow[1] + ZERO                       # canonicalised: -0.0 -> +0.0
    unk = np.isnan(u) | np.isnan(v) | (np.abs(u) > UNKNOWN_THRESH) | (np.abs(v) > UNKNOWN_THRESH)
    flag = np.full((H, W), 255 if rows is not None else 0, dtype=np.uint8)
    resid = np.full((2, H, W), np.nan if rows is not None else 0.0, dtype=f32)
    offs = _offsets(radius, spacing)
    with np.errstate(all="ignore"):
        for y in (range(H) if rows is None else rows):
            for x in range(W):
                if unk[y, x]:
                    flag[y, x], resid[0, y, x], resid[1, y, x] = UNKNOWN, ZERO, ZERO
                    continue
                nb = [(y + dy, x + dx) for dy, dx in offs if 0 <= y + dy < H and 0 <= x + dx < W and not unk[y + dy, x + dx]]
                if not nb:
                    flag[y, x], resid[0, y, x], resid[1, y, x] = 0, ZERO, ZERO
                    continue
                R = []
                for c in (u, v):
                    vals = np.array([c[q] for q in nb], dtype=f32)
                    m = median(vals)
                    r = median(np.abs(vals - m))
                    R.append(f32(abs(f32(c[y, x] - m)) / f32(r + eps)))
                resid[0, y, x], resid[1, y, x] = R
                flag[y, x] = OUTLIER if (R[0] > thresh or R[1] > thresh) else 0
    return flag, resid


def apply(flow, flag, radius=1, spacing=1, mode="replace"):
    """Pass 2 on one frame: (out float32 [2,H,W] or None for "flag", flag with bit 2 added where nothing could be replaced)."""
    flow = np.asarray(flow)
    _, H, W = flow.shape
    flag1 = np.asarray(flag, dtype=np.uint8)
    if mode == "flag":
        return None, flag1.copy()
    out, flag2 = flow.copy(), flag1.copy()
    if mode == "mask":
        out[:, flag1 != 0] = MASKED
        return out, flag2
    assert mode == "replace"
    u, v = flow[0] + ZERO, flow[1] + ZERO
    offs = _offsets(radius, spacing)
    for y, x in zip(*np.nonzero(flag1)):
        nb = [(y + dy, x + dx) for dy, dx in offs if 0 <= y + dy < H and 0 <= x + dx < W and flag1[y + dy, x + dx] == 0]
        if nb:
            out[0, y, x] = median([u[q] for q in nb])
            out[1, y, x] = median([v[q] for q in nb])
        else:
            flag2[y, x] |= NOT_REPLACED
    return out, flag2


def validate(flows, radius=1, spacing=1, eps=0.1, thresh=2.0, mode="replace"):
    """[B,2,H,W] float32 -> (out [B,2,H,W] or None, flag uint8 [B,H,W], resid [B,2,H,W]), frame by frame."""
    outs, flags, resids = [], [], []
    for f in np.asarray(flows):
        fl, rs = detect(f, radius, spacing, eps, thresh)
        o, fl = apply(f, fl, radius, spacing, mode)
        outs.append(o)
        flags.append(fl)
        resids.append(rs)
    B, _, H, W = np.asarray(flows).shape
    out = None if mode == "flag" else (np.stack(outs) if B else np.zeros((0, 2, H, W), f32))
    return out, np.stack(flags), np.stack(resids)


def accumulate_masked(acc, cnt, flows_b2hw, flags_bhw, calib):
    """acc [7,H,W], cnt [2,H,W] float64: frame by frame, u, v, uu, vv, uv where the frame's flag is 0, w, ww where the flags of all
    nine edge-clamped 3 x 3 neighbours are 0 (w = calc_vorticity's vort); a term left out is not added at all."""
    for f, g in zip(np.asarray(flows_b2hw), np.asarray(flags_bhw)):
        ok = g == 0
        gp = np.pad(g != 0, 1, mode="edge")
        H, W = g.shape
        bad9 = np.zeros((H, W), dtype=bool)
        for dy in range(3):
            for dx in range(3):
                bad9 |= gp[dy:dy + H, dx:dx + W]
        okw = ~bad9
        u, v = f[0].astype(f64), f[1].astype(f64)
        with np.errstate(all="ignore"):
            w = calc_vorticity(np.ascontiguousarray(f.transpose(1, 2, 0)), calib)[0]
            for k, term in enumerate((u, v, u * u, v * v, u * v)):
                acc[k][ok] = acc[k][ok] + term[ok]
            acc[5][okw] = acc[5][okw] + w[okw]
            acc[6][okw] = acc[6][okw] + (w * w)[okw]
        cnt[0][ok] += 1.0
        cnt[1][okw] += 1.0
    return acc, cnt


def same_bits32(a, b):
    """Bit-for-bit equality of two float32 arrays, NaN payloads and signs of zero included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == f32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def field_a(H=96, W=96, L=128.0):
    """A smooth vortex array: u = 4 sin(2 pi y / L) cos(2 pi x / L), v = -4 cos(2 pi y / L) sin(2 pi x / L), [2,H,W] float32."""
    y, x = np.mgrid[0:H, 0:W].astype(f64)
    k = 2.0 * np.pi / L
    return np.stack([4.0 * np.sin(k * y) * np.cos(k * x), -4.0 * np.cos(k * y) * np.sin(k * x)]).astype(f32)


def plant(flow, count, min_sep, seed):
    """A copy of flow [2,H,W] with `count` vectors displaced by 1-2 px in a random direction, every two of them at least `min_sep`
    apart in Chebyshev distance (placed by rejection), and the boolean [H,W] map of the planted positions."""
    rng = np.random.default_rng(seed)
    _, H, W = flow.shape
    assert count * min_sep * min_sep <= H * W // 2, "too many planted vectors for this separation: the rejection loop would not end"
    pts = []
    while len(pts) < count:
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        if all(max(abs(y - a), abs(x - b)) >= min_sep for a, b in pts):
            pts.append((y, x))
    out, planted = flow.copy(), np.zeros((H, W), dtype=bool)
    for y, x in pts:
        mag, ang = rng.uniform(1.0, 2.0), rng.uniform(0.0, 2.0 * np.pi)
        out[0, y, x] += f32(mag * np.cos(ang))
        out[1, y, x] += f32(mag * np.sin(ang))
        planted[y, x] = True
    return out, planted
