"""NumPy restatement of the three device contracts of stereo calibration (include/pivlfn.h, csrc/calibrate.hip) and a target renderer
for the tests.  The reference's calibration (stereo_cal.py, stereo/matching.py, stereo/dewarp.py) cannot be executed: it uses
np.int / np.issubclass_, needs cv2 and an interactive display.  What is restated, and from where:

  template_match   cv2.matchTemplate(pad_gray, template, TM_CCOEFF_NORMED) of template_matching (stereo/matching.py:43-47) from OpenCV's
                   documented formula, in exact integers: num = N sum(IT) - sum(I) sum(T), a = N sum(T^2) - sum(T)^2, b = N sum(I^2) -
                   sum(I)^2, r = float32(num / sqrt(a * b)) with one rounding per operation, 0 where a * b == 0.
  target_points    matching.py:49-75: `res > threshold`, cv2.blur(res, (2, 2)) -- its window at the default anchor (rows y-1..y, columns
                   x-1..x, BORDER_REFLECT_101), WITHOUT the division by 4 and on q = rint(r * 65536) so that every sum is an integer --
                   ndimage.label (default 4-connected structure) and the sums behind center_of_mass.  Deliberate difference: centres are
                   (sum w x / sum w - 0.5, ...): the one-sided window shifts the reference's coordinates by (+0.5, +0.5).
  dewarp           warp / nl_trans (stereo/dewarp.py:196-270).  Deliberate differences: no width / height swap on non-square images
                   (dewarp.py:214), and out-of-range sources get `fill` instead of the last pixel (dewarp.py:235-236).
                   `reference_warp_square` states the reference's index arithmetic, for the square in-range case where both agree.
SciPy is a test-only helper (ndimage.label: raster label order = ascending smallest row-major index)."""
import numpy as np

from pivlfn import calibrate as cal


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------
def window_sums(image, templ):
    """(sum I T, sum I, sum I^2) int64 [H,W] over the template's window centred on each pixel of the zero-padded image."""
    image, templ = np.asarray(image), np.asarray(templ)
    assert image.dtype == np.uint8 and templ.dtype == np.uint8
    H, W = image.shape
    th, tw = templ.shape
    ph, pw = (th - 1) // 2, (tw - 1) // 2
    pad = np.zeros((H + 2 * ph, W + 2 * pw), np.int64)
    pad[ph:ph + H, pw:pw + W] = image
    if H * W * th * tw <= 1 << 25:
        win = np.lib.stride_tricks.sliding_window_view(pad, (th, tw))
        t = templ.astype(np.int64)
        return np.einsum("yxij,ij->yx", win, t), win.sum(axis=(2, 3)), (win * win).sum(axis=(2, 3))
    sit, si, sii = (np.zeros((H, W), np.int64) for _ in range(3))
    for ty in range(th):
        for tx in range(tw):
            v = pad[ty:ty + H, tx:tx + W]
            sit += v * int(templ[ty, tx])
            si += v
            sii += v * v
    return sit, si, sii


def template_match(images, templ):
    images, templ = np.asarray(images), np.asarray(templ)
    images = images[None] if images.ndim == 2 else images
    th, tw = templ.shape
    assert th % 2 == 1 and tw % 2 == 1 and th * tw <= 65025
    N = th * tw
    t = templ.astype(np.int64)
    st, stt = int(t.sum()), int((t * t).sum())
    a = N * stt - st * st
    out = np.zeros(images.shape, np.float32)
    for k, im in enumerate(images):
        sit, si, sii = window_sums(im, templ)
        num = N * sit - si * st
        b = N * sii - si * si
        ok = (b != 0) & (a != 0)
        den = np.sqrt(np.float64(a) * b.astype(np.float64))
        with np.errstate(divide="ignore", invalid="ignore"):
            out[k] = np.where(ok, num.astype(np.float64) / den, 0.0).astype(np.float32)
    return out


def ccoeff_normed_direct(image, templ):
    """TM_CCOEFF_NORMED from its definition in float64: sum((I - mean I)(T - mean T)) / sqrt(sum((I - mean I)^2) sum((T - mean T)^2))."""
    image, templ = np.asarray(image, np.float64), np.asarray(templ, np.float64)
    H, W = image.shape
    th, tw = templ.shape
    ph, pw = (th - 1) // 2, (tw - 1) // 2
    pad = np.zeros((H + 2 * ph, W + 2 * pw))
    pad[ph:ph + H, pw:pw + W] = image
    win = np.lib.stride_tricks.sliding_window_view(pad, (th, tw))
    wz = win - win.mean(axis=(2, 3), keepdims=True)
    tz = templ - templ.mean()
    den = np.sqrt((wz * wz).sum(axis=(2, 3)) * (tz * tz).sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, (wz * tz).sum(axis=(2, 3)) / den, 0.0)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------
def box_sum(r, threshold):
    """w int64 [H,W] of one float32 map."""
    r = np.asarray(r, np.float32)
    with np.errstate(invalid="ignore"):
        keep = r > np.float32(threshold)
    q = np.where(keep, np.rint(np.minimum(np.where(keep, r, 0).astype(np.float64), 8192.0) * 65536.0), 0.0).astype(np.int64)
    H, W = q.shape
    ys = np.array([(1 if H > 1 else 0)] + list(range(H - 1)))          # index y-1, -1 reflected to +1
    xs = np.array([(1 if W > 1 else 0)] + list(range(W - 1)))
    return q[ys][:, xs] + q[ys] + q[:, xs] + q


def target_points(r, threshold, cap):
    """(labels int32 [B,H,W], count int32 [B], rec int64 [B,cap,4]) of float32 maps [B,H,W]."""
    from scipy import ndimage
    r = np.asarray(r, np.float32)
    r = r[None] if r.ndim == 2 else r
    B, H, W = r.shape
    labels = np.full((B, H, W), -1, np.int32)
    count = np.zeros(B, np.int32)
    rec = np.zeros((B, cap, 4), np.int64)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    for b in range(B):
        w = box_sum(r[b], threshold)
        lbl, n = ndimage.label(w > 0)
        count[b] = n
        flat = lbl.ravel()
        first = np.full(n + 1, H * W, np.int64)
        np.minimum.at(first, flat, np.arange(H * W))
        assert np.all(np.diff(first[1:]) > 0)                             # raster label order = ascending smallest index
        labels[b] = np.where(lbl > 0, first[lbl], -1)
        for k in range(min(n, cap)):
            m = lbl == k + 1
            rec[b, k] = (w[m].sum(), (w[m] * xx[m]).sum(), (w[m] * yy[m]).sum(), m.sum())
    return labels, count, rec


def find_markers(image, templ, threshold=0.7, cap=4096, border=True):
    """pivlfn.calibrate.find_markers of one image from the restated kernels: (centres [n,2], records [n,4])."""
    image = np.asarray(image)
    r = template_match(image, templ)
    _, count, rec = target_points(r, threshold, cap)
    rb = rec[0, :min(int(count[0]), cap)]
    cb = cal.centres_from_records(rb)
    if border:
        keep = cal.keep_inside(cb, image.shape[0], image.shape[1], templ.shape[0], templ.shape[1])
        cb, rb = cb[keep], rb[keep]
    return cb, rb


def calibrate_camera(image, templ, ref4, threshold=0.7, order=2, cap=4096, border=True):
    """pivlfn.calibrate.calibrate_camera with the restated kernels in place of the device's; the host steps are the package's."""
    pts, recs = find_markers(image, templ, threshold, cap, border)
    ij, sel, spacing = cal.index_lattice(pts, ref4)
    ok = ij[:, 0] != cal.NOT_INDEXED
    origin = pts[sel[0]]
    A, rms, worst = cal.fit_mapping(cal.lattice_targets(ij[ok], spacing), pts[ok] - origin, order)
    return {"A": A, "markers": pts, "records": recs, "ij": ij, "indexed": ok, "selected": sel, "spacing": spacing,
            "origin": (float(origin[0]), float(origin[1])), "rms": rms, "max": worst}


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------
def source_positions(H, W, A, origin):
    A = np.asarray(A, np.float64)
    x0, y0 = np.float64(origin[0]), np.float64(origin[1])
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u, v = xx - x0, yy - y0

    def P(k):
        return A[k] * u + A[k + 1] * v + A[k + 2] + A[k + 3] * (u * u) + A[k + 4] * (v * v) + A[k + 5] * u * v
    with np.errstate(divide="ignore", invalid="ignore"):
        return P(0) / P(6) + x0, P(12) / P(18) + y0


def dewarp(frames, A, origin, mode="nearest", fill=0):
    frames = np.asarray(frames)
    frames = frames[None] if frames.ndim == 2 else frames
    assert frames.dtype in (np.uint8, np.float32)
    B, H, W = frames.shape
    sx, sy = source_positions(H, W, A, origin)
    out = np.full(frames.shape, fill, frames.dtype)
    with np.errstate(invalid="ignore"):
        if mode == "nearest":
            rx, ry = np.round(sx), np.round(sy)
            ok = (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
            ix, iy = rx[ok].astype(np.int64), ry[ok].astype(np.int64)
            out[:, ok] = frames[:, iy, ix]
            return out
        fx, fy = np.floor(sx), np.floor(sy)
        ok = (fx >= 0) & (fx + 1 <= W - 1) & (fy >= 0) & (fy + 1 <= H - 1)
    ix, iy = fx[ok].astype(np.int64), fy[ok].astype(np.int64)
    ax, ay = (sx - fx)[ok], (sy - fy)[ok]
    f = frames.astype(np.float64)
    top = (1.0 - ax) * f[:, iy, ix] + ax * f[:, iy, ix + 1]
    bot = (1.0 - ax) * f[:, iy + 1, ix] + ax * f[:, iy + 1, ix + 1]
    val = (1.0 - ay) * top + ay * bot
    out[:, ok] = np.clip(np.rint(val), 0, 255).astype(np.uint8) if frames.dtype == np.uint8 else val.astype(np.float32)
    return out


def reference_warp_square(image, origin, A):
    """What warp (stereo/dewarp.py:196-252) computes for a SQUARE uint8 image, in this project's words.  The reference rounds the source
    position of every output pixel (dewarp.py:224-227), replaces a coordinate outside 0..n-1 by n-1, the last pixel (:230-236), and
    gathers from the image flattened column by column at the flat index sy + sx * n (:239-250).  `origin` stands for the first
    reference marker (old_x[pt1], old_y[pt1]).  Non-square images are left out: there the reference swaps the two sides (:214)."""
    n = image.shape[0]
    assert image.shape == (n, n)
    sx, sy = source_positions(n, n, A, origin)
    idx = []
    for s in (sx, sy):
        s = np.round(s)
        idx.append(np.where((s >= 0) & (s <= n - 1), s, n - 1).astype(np.int64))
    column_major = np.ascontiguousarray(image.T).ravel()
    return column_major[idx[1] + idx[0] * n]


# ---- the target renderer -------------------------------------------------------------------------------------------------------------------
def homography(H, W, persp, seed=0):
    """A mild plane -> image homography about the image centre: a small rotation, shear and scale and perspective terms of `persp`
    per pixel."""
    rng = np.random.default_rng(seed)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    th = np.deg2rad(rng.uniform(-2.0, 2.0))
    s = rng.uniform(0.97, 1.03)
    M = np.array([[s * np.cos(th), -s * np.sin(th) + rng.uniform(-0.02, 0.02), 0.0],
                  [s * np.sin(th), s * np.cos(th), 0.0],
                  [persp * rng.choice([-1.0, 1.0]), persp * rng.uniform(-1.0, 1.0), 1.0]])
    T = np.array([[1.0, 0.0, cx], [0.0, 1.0, cy], [0.0, 0.0, 1.0]])
    Ti = np.array([[1.0, 0.0, -cx], [0.0, 1.0, -cy], [0.0, 0.0, 1.0]])
    return T @ M @ Ti


def render_target(H, W, spacing, TC, HC, LC, M, phase=(0.0, 0.0)):
    """A binary uint8 image (crosses 255 on 0: what the calibration sees after the CLI's inversion) of crosses with bar thickness TC and
    extent HC x LC on a regular lattice of `spacing` in the target plane, seen through the homography M (plane -> image); every pixel
    is decided by mapping its centre back into the plane.  Returns (image, centres [n,2] = the true image position (x, y) of every
    lattice node whose centre falls inside the image, index [n,2] = its lattice index (i along x, j along y))."""
    Mi = np.linalg.inv(M)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = Mi[2, 0] * xx + Mi[2, 1] * yy + Mi[2, 2]
    X = (Mi[0, 0] * xx + Mi[0, 1] * yy + Mi[0, 2]) / d
    Y = (Mi[1, 0] * xx + Mi[1, 1] * yy + Mi[1, 2]) / d
    ox, oy = (W - 1 - spacing) / 2.0 + phase[0], (H - 1 - spacing) / 2.0 + phase[1]      # the cell (0,0)..(1,1) sits round the image centre
    dx = (X - ox) - np.round((X - ox) / spacing) * spacing
    dy = (Y - oy) - np.round((Y - oy) / spacing) * spacing
    cross = ((np.abs(dx) <= LC / 2.0) & (np.abs(dy) <= TC / 2.0)) | ((np.abs(dx) <= TC / 2.0) & (np.abs(dy) <= HC / 2.0))
    image = np.where(cross, 255, 0).astype(np.uint8)
    n = int(max(H, W) / spacing) + 3
    ii, jj = np.meshgrid(np.arange(-n, n + 1), np.arange(-n, n + 1), indexing="xy")
    Xn, Yn = ox + ii.ravel() * spacing, oy + jj.ravel() * spacing
    dn = M[2, 0] * Xn + M[2, 1] * Yn + M[2, 2]
    xn = (M[0, 0] * Xn + M[0, 1] * Yn + M[0, 2]) / dn
    yn = (M[1, 0] * Xn + M[1, 1] * Yn + M[1, 2]) / dn
    inside = (xn >= 0) & (xn <= W - 1) & (yn >= 0) & (yn <= H - 1)
    return image, np.stack([xn[inside], yn[inside]], axis=1), np.stack([ii.ravel()[inside], jj.ravel()[inside]], axis=1)


# the four targets of the accuracy tests: (H, W, spacing, (TC, HC, LC), perspective per pixel, seed)
TARGETS = {"96": (96, 96, 24, (3, 11, 11), 5e-4, 1), "256": (256, 256, 40, (5, 21, 21), 4e-4, 2),
           "192x320": (192, 320, 48, (11, 25, 25), 3e-4, 3), "512": (512, 512, 40, (5, 21, 21), 2e-4, 4)}


def target(name, seed=None):
    """(image, template, true centres, true indices, ref4 = the true centres of the cell (0,0), (1,0), (1,1), (0,1)).  `seed`: another
    view of the same target (the second camera of the command-line test)."""
    H, W, spacing, (TC, HC, LC), persp, own = TARGETS[name]
    seed = own if seed is None else seed
    M = homography(H, W, persp, seed)
    image, centres, index = render_target(H, W, spacing, TC, HC, LC, M, phase=(0.3, -0.2))
    ref4 = np.stack([centres[np.flatnonzero((index == c).all(axis=1))[0]] for c in ((0, 0), (1, 0), (1, 1), (0, 1))])
    return image, cal.gen_template(TC, HC, LC), centres, index, ref4


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
