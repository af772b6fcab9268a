"""CPU: the C ABI of the vector-validation entry points and their host-side refusals, the Python-side argument checks, the numpy
restatement of the contract (tests/validate_restatement.py) against hand-computed cases, and the detection it promises on planted
fields.  No GPU."""
import os
import re

import numpy as np
import pytest

import validate_restatement as vr
from postpro_restatement import accumulate, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
f32 = np.float32
NEW = ("pivlfn_flow_validate", "pivlfn_flow_stats_accumulate_masked")


def _frame(u, v=None):
    u = np.array(u, dtype=f32)
    return np.stack([u, np.zeros_like(u) if v is None else np.array(v, dtype=f32)])


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_and_signatures_carry_the_new_entries():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pivlfn.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
    for k, name in enumerate(("FLAG", "MASK", "REPLACE")):
        assert re.search(rf"#define\s+PIVLFN_VALIDATE_{name}\s+{k}\b", text)
    from pivlfn import _lib
    assert set(NEW) <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW) and lib.pivlfn_abi_version() == 3


def test_entries_refuse_bad_arguments_without_a_gpu():
    """Refused on the host with PIVLFN_ERR_ARG and a message naming the problem, before anything is launched (a launch on a
    machine without a GPU would return PIVLFN_ERR_HIP instead)."""
    from pivlfn import _lib
    lib = _lib.load()
    P, Q = 4096, 8192             # non-null pointers that are never dereferenced: every case below fails its checks first

    def refused(rc, *words):
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    def val(flow=P, out=Q, flag=P, resid=None, B=1, H=4, W=4, radius=1, spacing=1, eps=0.1, thresh=2.0, mode=2):
        return lib.pivlfn_flow_validate(flow, out, flag, resid, B, H, W, radius, spacing, eps, thresh, mode, None)

    refused(val(flow=None), "flow_validate", "null")
    refused(val(flag=None), "flow_validate", "null")
    refused(val(flag=None, out=None, mode=0), "null")
    refused(val(out=None, mode=1), "null out")
    refused(val(out=None, mode=2), "null out")
    refused(val(out=P), "out == flow")
    refused(val(out=P, mode=1), "out == flow")
    refused(val(B=0), "B=0")
    refused(val(H=-1), "H=-1")
    refused(val(W=0), "W=0")
    refused(val(H=46341, W=46341), "2^31")
    refused(val(B=70000), "B=70000", "65535")
    for r in (0, 3, -1):
        refused(val(radius=r), f"radius={r}")
    refused(val(spacing=0), "spacing=0")
    refused(val(spacing=-2), "spacing=-2")
    refused(val(spacing=1 << 15), "2^15")
    refused(val(radius=2, spacing=1 << 14), "2^15")
    refused(val(eps=-0.5), "eps=-0.5")
    refused(val(eps=float("inf")), "eps=inf")
    refused(val(eps=float("nan")), "eps=nan")
    refused(val(thresh=0.0), "thresh=0")
    refused(val(thresh=-1.0), "thresh=-1")
    refused(val(thresh=float("inf")), "thresh=inf")
    refused(val(thresh=float("nan")), "thresh=nan")
    refused(val(mode=3), "mode=3")
    refused(val(mode=-1), "mode=-1")

    def msk(flow=P, flag=P, acc=P, cnt=P, B=1, H=4, W=4, calib=1.0):
        return lib.pivlfn_flow_stats_accumulate_masked(flow, flag, acc, cnt, B, H, W, calib, None)

    for name in ("flow", "flag", "acc", "cnt"):
        refused(msk(**{name: None}), "flow_stats_accumulate_masked", "null")
    refused(msk(B=0), "B=0")
    refused(msk(H=-1), "H=-1")
    refused(msk(W=0), "W=0")
    refused(msk(H=46341, W=46341), "2^31")
    for c, word in ((0.0, "calib=0"), (float("inf"), "calib=inf"), (float("nan"), "calib=nan"), (1e308, "calib=1e+308")):
        refused(msk(calib=c), word)
    with pytest.raises(ValueError):
        _lib.check(val(radius=5), "flow_validate")


# ---- Python side ---------------------------------------------------------------------------------------------------------------
def test_python_side_argument_errors():
    import torch
    import pivlfn
    from pivlfn import validate as V
    assert pivlfn.validate_flow is V.validate_flow and pivlfn.MaskedFlowStats is V.MaskedFlowStats
    import src.postpro as sp
    assert sp.validate_flow is V.validate_flow and sp.MaskedFlowStats is V.MaskedFlowStats
    assert (V.OUTLIER, V.UNKNOWN, V.NOT_REPLACED) == (1, 2, 4)
    flow = torch.zeros(1, 2, 4, 4)
    for kw in (dict(mode="fix"), dict(radius=0), dict(radius=3), dict(radius=1.0), dict(spacing=0), dict(spacing=1.5),
               dict(radius=2, spacing=1 << 14), dict(eps=-1.0), dict(eps=float("nan")), dict(thresh=0.0), dict(thresh=float("inf"))):
        with pytest.raises(ValueError):
            V.validate_flow(flow, **kw)                       # parameters are checked before the tensor and the library
    with pytest.raises(NotImplementedError):
        V.validate_flow(flow)
    with pytest.raises(TypeError):
        V.validate_flow(flow.double())
    with pytest.raises(TypeError):
        V.validate_flow(flow.numpy())
    with pytest.raises(NotImplementedError):
        V.validate_flow(torch.zeros(1, 3, 4, 4))              # a CPU tensor is refused before its shape is looked at
    with pytest.raises(NotImplementedError):
        V.MaskedFlowStats(4, 4, device="cpu")
    for c in (0.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            V.MaskedFlowStats(4, 4, calib=c, device="cuda:0")
    with pytest.raises(ValueError):
        V.MaskedFlowStats(0, 4, device="cuda:0")


def test_finalize_masked_hand_made_accumulators():
    """Pixel (0,0): two frames u = (1, 3), v = (2, -2), one vorticity sample 0.5; pixel (0,1): nothing at all."""
    from pivlfn.validate import MASKED_RESULT, finalize_masked
    acc, cnt = np.zeros((7, 1, 2)), np.zeros((2, 1, 2))
    acc[:, 0, 0] = (4.0, 0.0, 10.0, 8.0, -4.0, 0.5, 0.25)
    cnt[:, 0, 0] = (2.0, 1.0)
    r = finalize_masked(acc, cnt, 4)
    assert list(r) == list(MASKED_RESULT)
    assert r["count"] == 4 and r["count_uv"].tolist() == [[2, 0]] and r["count_vort"].tolist() == [[1, 0]]
    assert r["count_uv"].dtype == np.int64 and r["valid_fraction"].tolist() == [[0.5, 0.0]]
    want = dict(mean_u=2.0, mean_v=0.0, rms_u=1.0, rms_v=2.0, cov_uv=-2.0, mean_vort=0.5, rms_vort=0.0)
    for k, w in want.items():
        assert r[k][0, 0] == w and np.isnan(r[k][0, 1]), k
    with pytest.raises(ValueError):
        finalize_masked(acc, cnt, 0)
    with pytest.raises(ValueError):
        finalize_masked(acc, cnt[:1], 4)


def test_run_py_refuses_validate_with_modifications_or_bad_parameters(tmp_path, monkeypatch):
    import run as runpy
    base = ["--model", "piv", "-i", str(tmp_path), "-o", str(tmp_path / "out"), "--validate", "replace"]
    for extra in (["-b", "1.2"], ["-c", "0.8"]):
        with pytest.raises(SystemExit, match="-b/-c"):
            runpy.main(base + extra)
    for extra, word in ((["--validate-radius", "3"], "radius"), (["--validate-spacing", "0"], "spacing"),
                        (["--validate-eps", "-1"], "eps"), (["--validate-thresh", "0"], "thresh")):
        with pytest.raises(SystemExit, match=word):
            runpy.main(base + extra)
    with pytest.raises(SystemExit):
        runpy.main(base[:-1] + ["repair"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="single process"):
        runpy.main(base)
    assert not (tmp_path / "out").exists()
    assert runpy.parser.parse_args([]).validate is None


# ---- the restatement against hand-computed cases ------------------------------------------------------------------------------------
def test_one_spike_in_a_3x3_field():
    """u = 1 everywhere, 5 in the middle, v = 0.  Middle: 8 neighbours of 1 -> m = 1, r = 0, R_u = fl(4 / 0.1f) = 40.  A corner has
    n = 3 neighbours (1, 1, 5): m = 1, distances (0, 0, 4) -> r = 0, R = 0 / 0.1 = 0; an edge pixel has 5 (1, 1, 1, 5, 1): the same."""
    f = _frame([[1, 1, 1], [1, 5, 1], [1, 1, 1]])
    flag, resid = vr.detect(f)
    assert flag.tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]]
    want = np.zeros((2, 3, 3), f32)
    want[0, 1, 1] = 40.0
    assert f32(4.0) / f32(0.1) == f32(40.0) and vr.same_bits32(resid, want)
    out, fl = vr.apply(f, flag, mode="replace")
    assert vr.same_bits32(out, _frame(np.ones((3, 3)))) and np.array_equal(fl, flag)
    out, fl = vr.apply(f, flag, mode="mask")
    want = _frame(np.ones((3, 3)))
    want[:, 1, 1] = 1e10
    assert vr.same_bits32(out, want) and np.array_equal(fl, flag)
    out, fl = vr.apply(f, flag, mode="flag")
    assert out is None and np.array_equal(fl, flag)
    # radius 2 on a 3 x 3 image sees the same neighbours (the outer ring lies outside); spacing 2 leaves the middle none at all
    assert np.array_equal(vr.detect(f, radius=2)[0], flag)
    flag2, resid2 = vr.detect(f, spacing=2)
    assert flag2[1, 1] == 0 and resid2[0, 1, 1] == 0.0


def test_even_count_median_and_not_replaced():
    """1 x 3, u = (1, 10, 4): the middle has n = 2, m = (1 + 4) * 0.5 = 2.5, distances (1.5, 1.5) -> r = 1.5,
    R = 7.5 / fl(1.5 + 0.1f).  The end pixels have the one neighbour 10: m = 10, r = 0, R = 9 / 0.1f and 6 / 0.1f.  All three are
    outliers, so no pixel has an unflagged neighbour: nothing is replaced and every flag gets bit 2."""
    f = _frame([[1, 10, 4]])
    flag, resid = vr.detect(f)
    assert flag.tolist() == [[1, 1, 1]]
    eps = f32(0.1)
    assert resid[0, 0].tolist() == [f32(9) / eps, f32(7.5) / f32(f32(1.5) + eps), f32(6) / eps]
    assert resid[0, 0, 1] == f32(4.6875) and not resid[1].any()
    assert vr.median([4, 1]) == f32(2.5) and vr.median([3, 1, 2]) == f32(2) and vr.median([7]) == f32(7)
    assert vr.median([1, 2, 4, 8]) == f32(3) and vr.median(np.array([0.1, 0.2], f32)) == f32(f32(f32(0.1) + f32(0.2)) * f32(0.5))
    out, fl = vr.apply(f, flag, mode="replace")
    assert vr.same_bits32(out, f) and fl.tolist() == [[5, 5, 5]]
    out, fl = vr.apply(f, flag, mode="mask")
    assert np.all(out == f32(1e10)) and fl.tolist() == [[1, 1, 1]]


def test_single_pixel_and_empty_neighbourhoods():
    f = _frame([[3.5]], [[-2.0]])
    for r in (1, 2):
        flag, resid = vr.detect(f, radius=r)
        assert flag.tolist() == [[0]] and not resid.any()
        for mode in ("mask", "replace"):
            out, fl = vr.apply(f, flag, radius=r, mode=mode)
            assert vr.same_bits32(out, f) and fl.tolist() == [[0]]
    # a spacing beyond the image: n = 0 everywhere, whatever the values
    g = _frame([[1, 100, 1], [1, 1, 1]])
    flag, resid = vr.detect(g, spacing=3)
    assert not flag.any() and not resid.any()


def test_unknown_vectors_are_dropped_from_the_neighbourhood():
    """1 x 3 with eps = 1: u = (1, 2, x), x unknown.  The middle sees only the 1: m = 1, r = 0, R = 1 / (0 + 1) = 1 (no outlier);
    the unknown pixel gets bit 1, R = 0; replace gives it the median of its one valid neighbour."""
    for x in (np.nan, np.inf, -np.inf, 1e10, -1e10, 1.0000001e9):
        f = _frame([[1, 2, x]], [[5, 6, 7]])
        assert vr.unknown(f32(x), f32(0)) and vr.unknown(f32(0), f32(x))
        flag, resid = vr.detect(f, eps=1.0)
        assert flag.tolist() == [[0, 0, 2]]
        assert resid[0].tolist() == [[1.0, 1.0, 0.0]] and resid[1].tolist() == [[1.0, 1.0, 0.0]]
        out, fl = vr.apply(f, flag, mode="replace")
        assert out[:, 0].tolist() == [[1, 2, 2], [5, 6, 6]] and fl.tolist() == [[0, 0, 2]]
        out, fl = vr.apply(f, flag, mode="mask")
        assert out[:, 0].tolist() == [[1, 2, 1e10], [5, 6, 1e10]]
    assert not vr.unknown(f32(1e9), f32(-1e9))                     # the threshold itself is a valid value
    # an unknown v makes the whole vector unknown
    f = _frame([[1, 2, 3]], [[5, 6, np.nan]])
    assert vr.detect(f, eps=1.0)[0].tolist() == [[0, 0, 2]]
    # a block of unknown vectors: its middle has no valid neighbour and stays as it is, with bits 1 and 2
    f = _frame(np.ones((5, 5)))
    f[0, 1:4, 1:4] = np.nan
    flag, _ = vr.detect(f)
    out, fl = vr.apply(f, flag, mode="replace")
    assert fl[2, 2] == 6 and np.isnan(out[0, 2, 2]) and fl[1, 1] == 2 and out[0, 1, 1] == 1.0


def test_negative_zero_is_canonicalised_for_comparison_and_copied_as_it_is():
    """3 x 3 of -0.0 with a 7 in the middle, eps = 1: only the middle is an outlier (R = 7); the -0.0 around it are copied with their
    sign, the middle becomes the median of eight canonicalised zeros: +0.0."""
    f = _frame(np.full((3, 3), -0.0), np.full((3, 3), -0.0))
    f[0, 1, 1] = 7.0
    flag, resid = vr.detect(f, eps=1.0)
    assert flag.tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]] and resid[0, 1, 1] == 7.0
    assert not np.signbit(resid).any()
    out, _ = vr.apply(f, flag, mode="replace")
    sign = np.signbit(out)
    assert out[0, 1, 1] == 0.0 and not sign[:, 1, 1].any() and sign.sum() == 16
    # -0.0 and +0.0 neighbours are one value: the residuals do not depend on the signs
    g = _frame([[-0.0, 0.0, -0.0, 0.0]])
    assert not vr.detect(g)[1].any() and not np.signbit(vr.detect(g)[1]).any()


def test_two_adjacent_spikes_do_not_replace_each_other():
    """Rows (0,0,0,0), (1,9,9,1), (2,2,2,2).  Pixel (1,1): neighbours sorted (0,0,0,1,2,2,2,9), m = 1.5, distances sorted
    (.5,.5,.5,.5,1.5,1.5,1.5,7.5), r = 1, R = 7.5 / 1.1: outlier, and (1,2) by symmetry; no other pixel exceeds 2 (worked out in the
    comments below).  Replacement uses the seven unflagged neighbours (0,0,0,1,2,2,2) -> 1, not the eight with the other spike
    (which would give 1.5)."""
    f = _frame([[0, 0, 0, 0], [1, 9, 9, 1], [2, 2, 2, 2]])
    flag, resid = vr.detect(f)
    assert flag.tolist() == [[0, 0, 0, 0], [0, 1, 1, 0], [0, 0, 0, 0]]
    eps = f32(0.1)
    assert resid[0, 1, 1] == resid[0, 1, 2] == f32(7.5) / f32(f32(1) + eps)
    assert resid[0, 0, 1] == f32(1) / f32(f32(1) + eps)          # (0,1): (0,0,1,9,9) -> m = 1, distances (0,1,1,8,8) -> r = 1
    assert resid[0, 1, 0] == f32(1) / f32(f32(2) + eps)          # (1,0): (0,0,2,2,9) -> m = 2, distances (0,0,2,2,7) -> r = 2
    assert resid[0, 2, 1] == 0.0                                 # (2,1): (1,2,2,9,9) -> m = 2 = its own value
    out, fl = vr.apply(f, flag, mode="replace")
    want = f.copy()
    want[0, 1, 1] = want[0, 1, 2] = 1.0
    assert vr.same_bits32(out, want) and np.array_equal(fl, flag)


def test_validate_stacks_frames_and_masked_accumulation_reduces_to_the_plain_one():
    rng = np.random.default_rng(5)
    flows = rng.normal(0, 3, (3, 2, 7, 9)).astype(f32)
    out, flag, resid = vr.validate(flows, mode="replace")
    for b in range(3):
        fl, rs = vr.detect(flows[b])
        o, fl = vr.apply(flows[b], fl, mode="replace")
        assert np.array_equal(flag[b], fl) and vr.same_bits32(resid[b], rs) and vr.same_bits32(out[b], o)
    assert 0 < (flag != 0).sum() < flag.size
    acc, cnt = vr.accumulate_masked(np.zeros((7, 7, 9)), np.zeros((2, 7, 9)), flows, np.zeros((3, 7, 9), np.uint8), 0.37)
    assert same_bits(acc, accumulate(np.zeros((7, 7, 9)), flows, 0.37)) and np.all(cnt == 3.0)
    acc, cnt = vr.accumulate_masked(np.zeros((7, 7, 9)), np.zeros((2, 7, 9)), flows, flag, 0.37)
    assert np.array_equal(cnt[0], (flag == 0).sum(0))
    assert np.all(cnt[1] <= cnt[0]) and cnt[1].sum() < cnt[0].sum()
    y, x = np.argwhere(flag[0] != 0)[0]
    others = sum(float(flows[b, 0, y, x]) for b in range(1, 3) if flag[b, y, x] == 0)
    assert acc[0, y, x] == others
    # a NaN that is flagged stays out of every sum it would otherwise poison
    flows[1, 0, 3, 4] = np.nan
    _, flag, _ = vr.validate(flows, mode="flag")
    acc, cnt = vr.accumulate_masked(np.zeros((7, 7, 9)), np.zeros((2, 7, 9)), flows, flag, 1.0)
    assert flag[1, 3, 4] == 2 and np.isfinite(acc).all()


# ---- detection on planted fields -------------------------------------------------------------------------------------------------
def _dns_field():
    from pivlfn.flo import read_flow
    f = read_flow(os.path.join(GOLD, "DNS_turbulence_out.flo"))
    assert f.shape == (256, 256, 2) and f.dtype == f32 and np.abs(f).max() <= 2.56
    return np.ascontiguousarray(f.transpose(2, 0, 1))


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("name", ["A", "B"])
def test_planted_vectors_are_found_and_nothing_else(name, radius):
    """At the defaults (eps 0.1, thresh 2, spacing 1): nothing is flagged in the clean field, every planted vector (1-2 px off, at
    least 2*radius + 1 apart so that no neighbourhood holds two) is flagged, and no other vector is.  Field A: the smooth vortex
    array of field_a (96 x 96, 40 vectors, seed 7); field B: the reference's network output for the DNS turbulence pair (256 x 256,
    50 vectors, seed 3).  The property is one of these settings only: a larger spacing or a shorter wavelength at eps = 0.1 flags
    clean vectors of a smooth gradient (see validate_flow's docstring)."""
    field, count, seed = (vr.field_a(), 40, 7) if name == "A" else (_dns_field(), 50, 3)
    clean, _ = vr.detect(field, radius)
    assert int((clean != 0).sum()) == 0
    spiked, planted = vr.plant(field, count, 2 * radius + 1, seed)
    assert int(planted.sum()) == count
    d = np.abs(spiked - field).max(0)[planted]
    assert d.min() >= 1.0 / np.sqrt(2.0) - 1e-6 and np.hypot(*(spiked - field))[planted].max() <= 2.0 + 1e-5
    flag, _ = vr.detect(spiked, radius)
    assert int((flag[planted] == vr.OUTLIER).sum()) == count
    assert int((flag[~planted] != 0).sum()) == 0


def test_plant_refuses_an_infeasible_request():
    with pytest.raises(AssertionError):
        vr.plant(vr.field_a(), 40, 17, 7)
