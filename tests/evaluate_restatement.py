"""The arithmetic contract of pivlfn_flow_errors / pivlfn_level_errors / pivlfn_error_stats_accumulate (include/pivlfn.h) in vectorised
numpy float64: every operation is one numpy ufunc on float64 arrays, so each is rounded on its own, and the summation order is the
contract's 2 x 2 tree.  The GPU tests compare bits with this; tests/test_evaluate.py checks it against the reference's recorded
results and hand-computed cases.  Plain numpy, no GPU."""
import numpy as np

f32, f64 = np.float32, np.float64
FIELDS = ("n", "l1", "epe", "sq", "du", "dv", "max")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def unknown(x):
    """The project's rule for an unknown fp32 value: NaN or beyond 1e9 in magnitude."""
    x = np.asarray(x, dtype=f32)
    with np.errstate(invalid="ignore"):
        return ~(np.abs(x) <= f32(1e9))


def _quad(m, op):
    """One tree step on the last two (even) axes: op(op(a, b), op(c, d)), a, b the upper row."""
    return op(op(m[..., 0::2, 0::2], m[..., 0::2, 1::2]), op(m[..., 1::2, 0::2], m[..., 1::2, 1::2]))


def _pad_even(m, value):
    ph, pw = m.shape[-2] & 1, m.shape[-1] & 1
    if not (ph or pw):
        return m
    return np.pad(m, [(0, 0)] * (m.ndim - 2) + [(0, ph), (0, pw)], constant_values=value)


def tree_sum(m):
    """Root of the 2 x 2 tree over the last two axes of a float64 map; an odd size is padded with +0.0 on the bottom / right at that
    step.  The reported root is root + 0.0."""
    m = np.asarray(m, dtype=f64)
    with np.errstate(invalid="ignore", over="ignore"):
        while m.shape[-2] > 1 or m.shape[-1] > 1:
            m = _quad(_pad_even(m, 0.0), np.add)
        return m[..., 0, 0] + 0.0


def tree_max(m):
    """The maximum over the last two axes (NaN if any entry is NaN), -inf for an empty selection."""
    m = np.asarray(m, dtype=f64)
    with np.errstate(invalid="ignore"):
        while m.shape[-2] > 1 or m.shape[-1] > 1:
            m = _quad(_pad_even(m, -np.inf), np.maximum)
    return m[..., 0, 0]


def pooled_truth(truth, mask, k, div_flow):
    """truth [B,2,H,W] fp32 -> (P [B,2,h,w] float64, excluded [B,h,w] bool)."""
    truth = np.asarray(truth)
    assert truth.dtype == f32 and truth.ndim == 4 and truth.shape[1] == 2 and 0 <= k <= 5
    B, _, H, W = truth.shape
    assert H % (1 << k) == 0 and W % (1 << k) == 0
    ex = unknown(truth[:, 0]) | unknown(truth[:, 1])
    if mask is not None:
        ex = ex | (np.asarray(mask) != 0)
    p = truth.astype(f64)
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(k):
            p = _quad(p, np.add)
            ex = _quad(ex, np.logical_or)
        p = (p / f64(4 ** k)) * f64(div_flow)
    return p, ex


def term_maps(flow, truth, mask=None, k=0, div_flow=1.0):
    """The per-pixel terms: dict of float64 [B,h,w] maps du, dv, sq, epe, l1 and the bool map `ex`."""
    flow = np.asarray(flow)
    assert flow.dtype == f32
    p, ex = pooled_truth(truth, mask, k, div_flow)
    assert flow.shape == p.shape, (flow.shape, p.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        du, dv = flow[:, 0].astype(f64) - p[:, 0], flow[:, 1].astype(f64) - p[:, 1]
        sq = du * du + dv * dv
        epe = np.sqrt(sq)
        l1 = np.abs(du) + np.abs(dv)
    return dict(du=du, dv=dv, sq=sq, epe=epe, l1=l1, ex=ex)


def flow_errors(flow, truth, mask=None, k=0, div_flow=1.0):
    """(sums [B,7] float64 in FIELDS order, err_map [B,3,h,w] fp32)."""
    t = term_maps(flow, truth, mask, k, div_flow)
    inc = ~t["ex"]
    n = inc.sum(axis=(1, 2)).astype(f64)
    cols = [n] + [tree_sum(np.where(inc, t[q], 0.0)) for q in ("l1", "epe", "sq", "du", "dv")]
    mx = tree_max(np.where(inc, t["epe"], -np.inf))
    cols.append(np.where(n == 0, 0.0, mx))
    with np.errstate(invalid="ignore", over="ignore"):
        emap = np.stack([np.where(inc, t[q], np.nan).astype(f32) for q in ("du", "dv", "epe")], axis=1)
    return np.stack(cols, axis=1), emap


def level_errors(levels, lowest_level, truth, mask=None, div_flow=1.0):
    """levels: [[M, S, R] per level, coarsest (6) first] of fp32 [B,2,h,w] -> sums [B, nlev, 3, 7]."""
    assert len(levels) == 7 - lowest_level
    out = [[flow_errors(f, truth, mask, 5 - i, div_flow)[0] for f in trio] for i, trio in enumerate(levels)]
    return np.stack([np.stack(tr, axis=1) for tr in out], axis=1)


def accumulate_errors(acc, flow, truth, mask=None):
    """acc [6,H,W] float64 += (1, du, dv, du*du, dv*dv, epe) of each frame in frame order where it is scored; returns the new acc."""
    acc = np.array(acc, dtype=f64)
    for b in range(len(flow)):
        t = term_maps(flow[b:b + 1], truth[b:b + 1], None if mask is None else mask[b:b + 1])
        inc = ~t["ex"][0]
        du, dv = t["du"][0], t["dv"][0]
        with np.errstate(invalid="ignore", over="ignore"):
            for q, v in enumerate((np.ones_like(du), du, dv, du * du, dv * dv, t["epe"][0])):
                acc[q] = np.where(inc, acc[q] + v, acc[q])
    return acc


# ---- the reference's src/loss.py in terms of the sums (what piv_liteflownet-pytorch_amd/src/loss.py computes on the device) ----------
def _seq(v):
    s = v[0]
    for x in v[1:]:
        s = s + x
    return s


def _epe(s, mean):
    return _seq(s[:, 2]) / _seq(s[:, 0]) if mean else _seq(s[:, 2]) / f64(len(s))


def _l1(s, mean):
    return _seq(s[:, 1]) / (2.0 * _seq(s[:, 0])) if mean else _seq(s[:, 1]) / f64(len(s))


def loss_value(fn, args, call, output, truth):
    """What src.loss.<fn>(**args)(output, truth) returns (EPE: src.loss.EPE(output, truth, **call)), flattened to a float64 vector
    in the order the reference returns it; plus, per entry, the number of per-pixel terms of the largest map it sums."""
    def score(f, pool=1, div=1.0):
        s = flow_errors(f, truth, None, pool.bit_length() - 1, div)[0]
        return s, int(s[:, 0].sum())

    norm = args.get("norm", "L1")
    if fn == "EPE":
        s, n = score(output)
        return np.array([_epe(s, call.get("mean", True))]), [n]
    if fn in ("L1", "L2"):
        s, n = score(output)
        return np.array([(_l1 if fn == "L1" else _epe)(s, args.get("mean", True))]), [n]
    if fn in ("L1Loss", "L2Loss"):
        s, n = score(output)
        mul = f64(float(args.get("mul_scale", 1)))
        return np.array([mul * (_l1 if fn == "L1Loss" else _epe)(s, True), mul * _epe(s, True)]), [n, n]
    version = args.get("version", 1) if fn == "piv_loss" else 2
    div = 1 / args.get("mul_scale", 5 if fn == "piv_loss" else 20)
    loss = _l1 if norm == "L1" else _epe
    if args.get("level_eval", False):
        nlev = 6 if fn == "piv_loss" else 5
        assert len(output) == nlev
        pools = [version * 2 ** sc for sc in reversed(range(nlev))]
        ls, es, ns = [], [], []
        for o, pool in zip(output, pools):
            s, n = score(o[-1] if isinstance(o, (list, tuple)) else o, pool, div)
            ls.append(loss(s, True))
            es.append(_epe(s, True))
            ns.append(n)
        return np.array(ls + es), ns + ns
    weights = {("piv_loss", 1): (0.001, 0.001, 0.001, 0.001, 0.001, 0.01), ("piv_loss", 2): (0.001, 0.001, 0.001, 0.001, 0.01),
               ("hui_loss", 2): (0.32, 0.08, 0.02, 0.01, 0.005)}[(fn, version)]
    nsc = 7 - version
    pools = [version * 2 ** sc for sc in reversed(range(nsc))]
    if not isinstance(output, (list, tuple)):
        s, n = score(output, pools[-1])
        return np.array([0.0 + loss(s, True), 0.0 + _epe(s, True)]), [n, n]
    assert len(output) == len(weights)
    lv, ev, nmax = 0.0, 0.0, 0
    for i, o in enumerate(output):
        for f in (o if isinstance(o, (list, tuple)) else [o]):
            s, n = score(f, pools[i] if i < nsc else 1, div)
            ev = ev + weights[i] * _epe(s, True)
            lv = lv + weights[i] * loss(s, True)
            nmax = max(nmax, n)
    return np.array([lv, ev]), [nmax, nmax]


def load_cases(path):
    """tests/golden/evaluate_cases.npz -> {name: dict(fn, args, call, output, truth, f32, f64)}; the stored float16 inputs widened to
    float32 (exactly the values the reference was given)."""
    import json
    z = np.load(path)
    out = {}
    for name, c in json.loads(str(z["cases"])).items():
        lv = [[z[f"{c['set']}_L{L}_{s}"].astype(f32) for s in c["stages"]] for L in c["levels"]]
        output = lv[0][0] if len(lv) == 1 else [tr if len(tr) > 1 else tr[0] for tr in lv]
        out[name] = dict(fn=c["fn"], args=c["args"], call=c["call"], output=output, truth=z[f"{c['set']}_truth"].astype(f32),
                         f32=z[f"{name}_f32"], f64=z[f"{name}_f64"])
    return out
