"""NumPy restatement of the image pre-processing contract of include/pivlfn.h (pivlfn_frames_preprocess,
pivlfn_frames_background_min), twice: `preprocess_loops` is the definition -- plain Python loops over clamped indices, every step on
its own -- and `preprocess_plane` is a vectorised form for full-size images (window minima and maxima of the edge-padded image, box
sums from a two-dimensional cumulative sum of the edge-padded minima and maxima).  Both work on one channel of one frame, in integers
up to the one float32 division; `preprocess` stacks channels and frames into the kernel's layout.  A helper, not a test."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

f32 = np.float32


def background_min(frames, start=None):
    """min over the frames [n,...] (uint8) and, when given, the accumulator `start`; the accumulator begins at 255."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8
    acc = np.full(frames.shape[1:], 255, np.uint8) if start is None else np.asarray(start, np.uint8)
    return np.minimum(acc, frames.min(axis=0)) if len(frames) else acc.copy()


def subtract(img, bg=None):
    """Step 1: x = max(I - B, 0) as int64 (x = I without a background)."""
    x = np.asarray(img).astype(np.int64)
    if bg is not None:
        assert np.asarray(bg).shape == x.shape
        x = np.maximum(x - np.asarray(bg).astype(np.int64), 0)
    return x


def check_k(k, floor):
    assert k == 0 or (k % 2 == 1 and 3 <= k <= 31), k
    assert 1 <= floor <= 255, floor


# ---- the definition --------------------------------------------------------------------------------------------------------------
def terms_loops(x, k):
    """num and S - L of the contract at every pixel of the integer image x [H,W], by loops over clamped coordinates."""
    H, W = x.shape
    r, n = k // 2, k * k
    x = [[int(v) for v in row] for row in x]

    def cy(i):
        return min(max(i, 0), H - 1)

    def cx(j):
        return min(max(j, 0), W - 1)

    lo = [[0] * W for _ in range(H)]
    hi = [[0] * W for _ in range(H)]
    for i in range(H):
        for j in range(W):
            window = [x[cy(i + a)][cx(j + b)] for a in range(-r, r + 1) for b in range(-r, r + 1)]
            lo[i][j] = min(window)
            hi[i][j] = max(window)
    num = np.zeros((H, W), np.int64)
    span = np.zeros((H, W), np.int64)
    for i in range(H):
        for j in range(W):
            L = sum(lo[cy(i + a)][cx(j + b)] for a in range(-r, r + 1) for b in range(-r, r + 1))
            S = sum(hi[cy(i + a)][cx(j + b)] for a in range(-r, r + 1) for b in range(-r, r + 1))
            num[i, j] = n * x[i][j] - L
            span[i, j] = S - L
    return num, span


def finish(num, span, k, floor):
    """den = max(S - L, floor * n); out = float32(num) / float32(den).  Asserts 0 <= num <= den < 2^24 on every pixel."""
    den = np.maximum(span, floor * k * k)
    assert (num >= 0).all() and (num <= den).all() and den.max() < 1 << 24
    return num.astype(f32) / den.astype(f32)


def scale(x):
    """Step 3: float32(x) / 255.0f."""
    return x.astype(f32) / f32(255.0)


def preprocess_loops(img, bg=None, k=0, floor=16):
    """One channel of one frame, img and bg uint8 [H,W] -> float32 [H,W]: the definition."""
    check_k(k, floor)
    x = subtract(img, bg)
    return scale(x) if k == 0 else finish(*terms_loops(x, k), k, floor)


# ---- the same, vectorised ----------------------------------------------------------------------------------------------------------
def _window(p, k, reduce):
    return reduce(sliding_window_view(reduce(sliding_window_view(p, k, axis=1), axis=-1), k, axis=0), axis=-1)


def _box_sum(a, k):
    """Sum over the k x k window centred at every pixel of `a`, edge replicated: from the cumulative sum of the padded array."""
    r = k // 2
    c = np.pad(np.pad(a, r, mode="edge").cumsum(0).cumsum(1), ((1, 0), (1, 0)))
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


def terms_plane(x, k):
    r = k // 2
    p = np.pad(x, r, mode="edge")
    lo, hi = _window(p, k, np.min), _window(p, k, np.max)
    L, S = _box_sum(lo, k), _box_sum(hi, k)
    return k * k * x - L, S - L


def preprocess_plane(img, bg=None, k=0, floor=16):
    """One channel of one frame, as preprocess_loops."""
    check_k(k, floor)
    x = subtract(img, bg)
    return scale(x) if k == 0 else finish(*terms_plane(x, k), k, floor)


def preprocess(frames, bg=None, k=0, floor=16, plane=preprocess_plane):
    """frames uint8 [n,H,W,3], bg uint8 [H,W,3] or None -> float32 [n,3,H,W], every channel on its own."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[3] == 3
    out = np.empty((frames.shape[0], 3) + frames.shape[1:3], f32)
    for t in range(frames.shape[0]):
        for c in range(3):
            out[t, c] = plane(frames[t, :, :, c], None if bg is None else np.asarray(bg)[:, :, c], k, floor)
    return out


def same_bits32(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == f32 and b.dtype == f32 and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- test images -------------------------------------------------------------------------------------------------------------------
def smooth_background(H, W, peak=104):
    """A static background: a ramp of 0..40 grey levels along x plus a Gaussian glare spot, uint8 [H,W] with maximum `peak`."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ramp = 40.0 * x / max(W - 1, 1)
    spot = np.exp(-(((x - 0.3 * W) / (0.15 * W + 1)) ** 2 + ((y - 0.6 * H) / (0.2 * H + 1)) ** 2))
    g = ramp + spot * 100.0
    return np.floor(g * (peak / g.max())).astype(np.uint8)
