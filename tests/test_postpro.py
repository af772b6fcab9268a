"""CPU: the numpy restatement of src/postpro.py against the reference's outputs, the C ABI of the post-processing entry points
and their host-side refusals, the src.postpro alias and FlowStats' finalisation.  No GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from postpro_restatement import accumulate, calc_vorticity, de_vort, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def cases():
    return np.load(os.path.join(GOLD, "postpro_cases.npz"))


def test_restatement_matches_reference_fixture(cases):
    tags = list(cases["cases"])
    assert len(tags) >= 13
    for tag in tags:
        flow, calib = cases[f"{tag}_flow"], float(cases[f"{tag}_calib"])
        assert flow.dtype == np.float32
        for name, fn in (("calc_vorticity", calc_vorticity), ("de_vort", de_vort)):
            with np.errstate(all="ignore"):
                got = np.stack(fn(flow, calib))
            assert same_bits(got, cases[f"{tag}_{name}"]), (tag, name)


def test_fixture_covers_the_edge_cases(cases):
    """Signs of zero, NaN spreading (the two functions spread it differently) and the degenerate shapes are in the fixture."""
    cv = cases["zeros_calc_vorticity"]
    assert np.signbit(cv[2]).all() and not np.signbit(cv[0]).any()          # normal = -(+0.0)
    nf_cv, nf_dv = cases["nonfinite_calc_vorticity"], cases["nonfinite_de_vort"]
    assert np.isnan(nf_cv).sum() > np.isnan(nf_dv).sum() > 0
    shapes = {tuple(cases[f"{t}_flow"].shape[:2]) for t in cases["cases"]}
    assert {(1, 1), (1, 9), (9, 1), (2, 2), (64, 96)} <= shapes
    assert {1.0, 0.37, 2.5e-4} <= {float(cases[f"{t}_calib"]) for t in cases["cases"]}


def test_sequential_accumulation_is_split_invariant():
    rng = np.random.default_rng(3)
    flows = rng.normal(0, 4, (7, 2, 9, 11)).astype(np.float32)
    one = accumulate(np.zeros((7, 9, 11)), flows, 0.37)
    parts = np.zeros((7, 9, 11))
    for a, b in ((0, 3), (3, 4), (4, 7)):
        accumulate(parts, flows[a:b], 0.37)
    assert same_bits(one, parts)
    assert same_bits(one[5], sum((calc_vorticity(f.transpose(1, 2, 0), 0.37)[0] for f in flows), np.zeros((9, 11))))


def _declared():
    text = open(os.path.join(ROOT, "include", "pivlfn.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_postpro_entries():
    text = _declared()
    for name in ("pivlfn_flow_fields", "pivlfn_flow_stats_accumulate"):
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
    assert re.search(r"#define\s+PIVLFN_FIELDS_CALC_VORTICITY\s+0\b", text)
    assert re.search(r"#define\s+PIVLFN_FIELDS_DE_VORT\s+1\b", text)
    from pivlfn import _lib
    assert {"pivlfn_flow_fields", "pivlfn_flow_stats_accumulate"} <= set(_lib.SIGNATURES)


def test_postpro_entries_refuse_bad_arguments_without_a_gpu():
    """Refused on the host with PIVLFN_ERR_ARG and a message naming the problem, before anything is launched (a launch on a
    machine without a GPU would return PIVLFN_ERR_HIP instead)."""
    from pivlfn import _lib
    lib = _lib.load()
    P = 4096                      # a non-null pointer that is never dereferenced: every case below fails its checks first

    def refused(rc, *words):
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    for what, call in (("flow_fields", lambda f, o, B, H, W, c: lib.pivlfn_flow_fields(f, o, B, H, W, c, 0, 1, None)),
                       ("flow_stats_accumulate", lambda f, o, B, H, W, c: lib.pivlfn_flow_stats_accumulate(f, o, B, H, W, c, None))):
        refused(call(None, P, 1, 4, 4, 1.0), what, "null")
        refused(call(P, None, 1, 4, 4, 1.0), what, "null")
        refused(call(P, P, 0, 4, 4, 1.0), "B=0")
        refused(call(P, P, 1, -1, 4, 1.0), "H=-1")
        refused(call(P, P, 1, 4, 0, 1.0), "W=0")
        refused(call(P, P, 1, 46341, 46341, 1.0), "2^31")
        refused(call(P, P, 1, 4, 4, 0.0), "calib=0")
        refused(call(P, P, 1, 4, 4, -0.0), "calib=-0")
        refused(call(P, P, 1, 4, 4, float("inf")), "calib=inf")
        refused(call(P, P, 1, 4, 4, float("nan")), "calib=nan")
        refused(call(P, P, 1, 4, 4, 1e308), "calib=1e+308")
    refused(lib.pivlfn_flow_fields(P, P, 70000, 4, 4, 1.0, 0, 0, None), "B=70000", "65535")
    refused(lib.pivlfn_flow_fields(P, P, 1, 4, 4, 1.0, 2, 0, None), "kind=2")
    refused(lib.pivlfn_flow_fields(P, P, 1, 4, 4, 1.0, -1, 0, None), "kind=-1")
    refused(lib.pivlfn_flow_fields(P, P, 1, 4, 4, 1.0, 1, 2, None), "out_f64=2")
    with pytest.raises(ValueError):
        _lib.check(lib.pivlfn_flow_fields(P, P, 1, 4, 4, 0.0, 0, 0, None), "flow_fields")


def test_src_postpro_alias_exports_the_reference_functions():
    import src.postpro as sp
    for name in ("calc_vorticity", "de_vort"):
        fn = getattr(sp, name)
        params = list(inspect.signature(fn).parameters.values())
        assert [p.name for p in params] == ["flow", "calib"] and params[1].default == 1.0, name


def test_numpy_dropins_refuse_other_dtypes_without_a_gpu():
    from pivlfn.postpro import calc_vorticity as cv, de_vort as dv
    for fn in (cv, dv):
        for dt in (np.float64, np.float16, np.int32):
            with pytest.raises(TypeError):
                fn(np.zeros((4, 5, 2), dtype=dt))


def test_finalize_hand_made_accumulators():
    """Two frames per pixel with known moments: u = (1, 3), v = (2, -2), w = (0.5, 1.5)."""
    from pivlfn.postpro import RESULT, finalize
    u, v, w = np.array([1.0, 3.0]), np.array([2.0, -2.0]), np.array([0.5, 1.5])
    acc = np.zeros((7, 2, 3))
    for k, s in enumerate((u.sum(), v.sum(), (u * u).sum(), (v * v).sum(), (u * v).sum(), w.sum(), (w * w).sum())):
        acc[k] = s
    acc[2, 1, 2] = acc[0, 1, 2] ** 2 / 2 - 1e-9        # a variance rounded below zero -> rms 0, not NaN
    r = finalize(acc, 2)
    assert list(r) == list(RESULT)
    assert r["count"] == 2 and r["count"].dtype == np.int64
    assert all(r[k].dtype == np.float64 and r[k].shape == (2, 3) for k in RESULT[1:])
    assert np.all(r["mean_u"] == 2.0) and np.all(r["mean_v"] == 0.0) and np.all(r["mean_vort"] == 1.0)
    assert np.all(r["rms_u"].ravel()[:-1] == 1.0) and r["rms_u"][1, 2] == 0.0
    assert np.all(r["rms_v"] == 2.0) and np.all(r["rms_vort"] == 0.5)
    assert np.all(r["cov_uv"] == -2.0)                   # mean(u v) = -2, mean_u mean_v = 0
    with pytest.raises(ValueError):
        finalize(acc, 0)
    with pytest.raises(ValueError):
        finalize(acc[:6], 2)


def test_run_py_refuses_stats_with_modifications_or_several_processes(tmp_path, monkeypatch):
    import run as runpy
    base = ["--model", "piv", "-i", str(tmp_path), "-o", str(tmp_path / "out"), "--stats"]
    for extra in (["-b", "1.2"], ["-c", "0.8"]):
        with pytest.raises(SystemExit, match="-b/-c"):
            runpy.main(base + extra)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="single process"):
        runpy.main(base)
    assert not (tmp_path / "out").exists()


def test_flowstats_refuses_a_bad_calib_before_touching_a_device():
    from pivlfn.postpro import FlowStats
    for c in (0.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            FlowStats(4, 4, calib=c, device="cuda:0")
