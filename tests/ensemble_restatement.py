"""NumPy restatement of pivlfn_ensemble_corr's contract (include/pivlfn.h, csrc/ensemble.hip) in int64: the window grid, the OUTSIDE rule
and three nested loops -- windows, dy, dx -- over plain slices.  A helper, not a test: tests/test_ensemble.py and
tests/test_gpu_ensemble.py compare with it bit for bit.  Written from the contract alone; it shares no code with pivlfn/ensemble.py."""
import numpy as np


def particle_frames(n, H, W, uv, seed, density=0.05, margin=12, diameter=2.2, amp=200.0):
    """n pairs of uint8 [H,W] images from tests/particles_restatement.py's render: positions uniform at `density` particles per pixel
    over the frame plus `margin` pixels each way, new ones for every pair; frame 2 is the same particles moved by the uniform (u, v).
    The grey level is trunc(min(V, 255)), the renderer's image rule."""
    import particles_restatement as pr
    rng = np.random.default_rng(seed)
    count = int(round(density * (H + 2 * margin) * (W + 2 * margin)))
    a, b = np.empty((n, H, W), np.uint8), np.empty((n, H, W), np.uint8)
    d, amps, shift = np.full(count, diameter), np.full(count, amp), np.array(uv, np.float64)[:, None]
    for k in range(n):
        pos = np.stack([rng.uniform(-margin, W + margin, count), rng.uniform(-margin, H + margin, count)])
        a[k] = np.floor(np.minimum(pr.render(pos, d, amps, H, W)[0], 255.0)).astype(np.uint8)
        b[k] = np.floor(np.minimum(pr.render(pos + shift, d, amps, H, W)[0], 255.0)).astype(np.uint8)
    return a, b


# the accuracy cases: frames, (u, v), window, step, search, uniform offset (ox, oy) or None; all at 72 x 88
ACC_H, ACC_W = 72, 88
ACCURACY = ((8, (2.3, -1.6), 32, 16, 4, None), (32, (2.3, -1.6), 16, 8, 4, None), (8, (6.3, 3.4), 32, 16, 2, (6, 3)))
_accuracy = {}


def accuracy_case(k):
    """(a, b, offset [2,ny,nx] or None, sums, sums_a) of accuracy case k: rendered and restated once per process, then shared;
    the arrays are read-only."""
    if k not in _accuracy:
        n, uv, window, step, search, off = ACCURACY[k]
        a, b = particle_frames(n, ACC_H, ACC_W, uv, 100 + k)
        ny, nx = grid(ACC_H, ACC_W, window, step, search)
        offset = None if off is None else np.stack([np.full((ny, nx), off[0], np.int32), np.full((ny, nx), off[1], np.int32)])
        got = (a, b, offset) + ensemble_corr(a, b, window, step, search, offset)
        for x in got:
            if x is not None:
                x.setflags(write=False)
        _accuracy[k] = got
    return _accuracy[k]


def err_arg_cases(a, b, offset, sums, sums_a, B, H, W, window, step, search):
    """Every PIVLFN_ERR_ARG case of the header as (label, the eleven arguments before the stream, a word of the message), made from
    one valid argument list (pointers as integers; `offset` not null)."""
    ok = [a, b, offset, sums, sums_a, B, H, W, window, step, search]

    def case(label, word, **change):
        names = ("a", "b", "offset", "sums", "sums_a", "B", "H", "W", "window", "step", "search")
        return label, tuple(change.get(n, v) for n, v in zip(names, ok)), word
    return [case("null a", "null", a=None), case("null b", "null", b=None), case("null sums", "null", sums=None),
            case("null sums_a", "null", sums_a=None),
            case("sums on a", "sums overlaps a", sums=a), case("sums on b", "sums overlaps b", sums=b),
            case("sums_a inside a", "sums_a overlaps a", sums_a=a + 8), case("sums_a on offset", "sums_a overlaps offset", sums_a=offset),
            case("sums on offset", "sums overlaps offset", sums=offset), case("sums_a inside sums", "sums overlaps sums_a", sums_a=sums + 8),
            case("window 4", "window=4", window=4), case("window 132", "window=132", window=132), case("window 30", "window=30", window=30),
            case("search 0", "search=0", search=0), case("search 33", "search=33", search=33), case("step 0", "step=0", step=0),
            case("B -1", "B=-1", B=-1), case("B 65536", "B=65536", B=65536),
            case("H short", "holds no window", H=window + 2 * search - 1), case("W short", "holds no window", W=window + 2 * search - 1),
            case("H 0", "positive", H=0), case("2^31 pixels", "2^31", H=65536, W=32768)]


def grid(H, W, window, step, search):
    assert H >= window + 2 * search and W >= window + 2 * search
    return (H - window - 2 * search) // step + 1, (W - window - 2 * search) // step + 1


def outside(H, W, window, step, search, offset=None):
    """bool [ny,nx] by the header's rule; offset [2,ny,nx] (ox, oy) or None."""
    ny, nx = grid(H, W, window, step, search)
    out = np.zeros((ny, nx), bool)
    for j in range(ny):
        for i in range(nx):
            ox, oy = (0, 0) if offset is None else (int(offset[0, j, i]), int(offset[1, j, i]))
            y, x = search + j * step + oy, search + i * step + ox
            out[j, i] = y - search < 0 or y + search + window > H or x - search < 0 or x + search + window > W
    return out


def ensemble_corr(a, b, window, step, search, offset=None, sums=None, sums_a=None):
    """a, b uint8 [B,H,W] -> (sums [ny,nx,P,P,3], sums_a [ny,nx,2]) int64, added onto `sums` / `sums_a` (copies) where given."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape and a.ndim == 3
    _, H, W = a.shape
    ny, nx = grid(H, W, window, step, search)
    P = 2 * search + 1
    sums = np.zeros((ny, nx, P, P, 3), np.int64) if sums is None else np.array(sums, np.int64)
    sums_a = np.zeros((ny, nx, 2), np.int64) if sums_a is None else np.array(sums_a, np.int64)
    out = outside(H, W, window, step, search, offset)
    A, Bq = a.astype(np.int64), b.astype(np.int64)
    with np.errstate(over="ignore"):                                  # a random pre-fill may wrap, as the device's 64-bit add does
        for j in range(ny):
            for i in range(nx):
                if out[j, i]:
                    continue
                ox, oy = (0, 0) if offset is None else (int(offset[0, j, i]), int(offset[1, j, i]))
                y, x = search + j * step, search + i * step
                wa = A[:, y:y + window, x:x + window]
                sums_a[j, i, 0] += wa.sum()
                sums_a[j, i, 1] += (wa * wa).sum()
                for dy in range(-search, search + 1):
                    for dx in range(-search, search + 1):
                        wb = Bq[:, y + oy + dy:y + oy + dy + window, x + ox + dx:x + ox + dx + window]
                        assert wb.shape == wa.shape
                        sums[j, i, dy + search, dx + search] += np.array([wb.sum(), (wb * wb).sum(), (wa * wb).sum()], np.int64)
    return sums, sums_a
