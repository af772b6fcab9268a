"""CPU: the C ABI of the scoring entry points and their host-side refusals, the numpy restatement of the contract
(tests/evaluate_restatement.py) against the reference's recorded results and hand-computed cases, the names and signatures of
src.loss, run.py's --truth argument handling, and ErrorStats' finalisation (its merge: tests/test_accumulators.py).  No GPU.

The tolerance against the reference's float64 results is derived, not tuned.  Reference and contract add the same N non-negative
float64 terms (end-point errors, or |du| + |dv|) in different orders.  A sum of N non-negative terms computed in any order carries a
relative error of at most (N - 1) u, u = 2^-53, to first order, so two orders differ by at most 2 N u relative; the handful of
operations around the sum (a division by the count, the weights of MultiScale, each on non-negative values) add a few u more and
the per-term roundings a few u each, all far below N u for the N used here.  The signed sums of du and dv are bounded the same way
relative to the sums of |du| and |dv|."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import evaluate_restatement as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
f32 = np.float32
U = 2.0 ** -53
NEW = ("pivlfn_flow_errors", "pivlfn_level_errors", "pivlfn_error_stats_accumulate")
CASES = er.load_cases(os.path.join(GOLD, "evaluate_cases.npz"))


def _flow(u, v=None):
    u = np.array(u, dtype=f32)
    return np.stack([u, np.zeros_like(u) if v is None else np.array(v, dtype=f32)])[None]


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_and_signatures_carry_the_new_entries():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pivlfn.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
    assert re.search(r"\bsize_t\s+pivlfn_flow_errors_workspace_bytes\s*\(", text)
    from pivlfn import _lib
    assert set(NEW) | {"pivlfn_flow_errors_workspace_bytes"} <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW) and lib.pivlfn_abi_version() == 3
    # 18 jobs x B x (tiles + 16 x 16 blocks of tiles) x 7 doubles, rounded up to 256 bytes
    assert lib.pivlfn_flow_errors_workspace_bytes(1, 32, 32) == 18 * 2 * 56 // 256 * 256 + 256
    assert lib.pivlfn_flow_errors_workspace_bytes(8, 1024, 1024) == 18 * 8 * (1024 + 4) * 56
    assert lib.pivlfn_flow_errors_workspace_bytes(0, 32, 32) == 0 and lib.pivlfn_flow_errors_workspace_bytes(1, -1, 32) == 0


def test_entries_refuse_bad_arguments_without_a_gpu():
    """Refused on the host with PIVLFN_ERR_ARG and a message naming the problem, before anything is launched (a launch on a
    machine without a GPU would return PIVLFN_ERR_HIP instead)."""
    from pivlfn import _lib
    lib = _lib.load()
    P, Q, BIG = 4096, 8192, 1 << 40        # non-null pointers that are never dereferenced: every case below fails its checks first

    def refused(rc, *words):
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    def fe(flow=P, truth=P, mask=None, B=1, H=64, W=64, k=0, div=1.0, sums=Q, emap=None, ws=P, nws=BIG):
        return lib.pivlfn_flow_errors(flow, truth, mask, B, H, W, k, div, sums, emap, ws, nws, None)

    def le(levels=P, lowest=1, truth=P, mask=None, B=1, H=64, W=64, div=0.2, sums=Q, ws=P, nws=BIG):
        return lib.pivlfn_level_errors(levels, lowest, truth, mask, B, H, W, div, sums, ws, nws, None)

    for call, what, first in ((fe, "flow_errors", "flow"), (le, "level_errors", "levels")):
        for name in (first, "truth", "sums", "ws"):
            refused(call(**{name: None}), what, "null")
        refused(call(B=0), what, "B=0")
        refused(call(H=-32), "H=-32")
        refused(call(W=0), "W=0")
        refused(call(H=46336, W=46368), "2^31")
        refused(call(B=70000), "B=70000", "65535")
        refused(call(div=float("nan")), "div_flow=nan")
        refused(call(div=float("inf")), "div_flow=inf")
        refused(call(ws=P + 4), "aligned")
        need = lib.pivlfn_flow_errors_workspace_bytes(1, 64, 64)
        refused(call(nws=need - 1), "too small", str(need))
        refused(call(nws=0), "too small")
    for k in (-1, 6):
        refused(fe(k=k), f"k={k}")
    refused(fe(H=36, k=3), "H=36", "multiples of 2^k = 8")
    refused(fe(W=65, k=1), "W=65")
    for lowest in (0, 7, -1):
        refused(le(lowest=lowest), f"lowest_level={lowest}")
    refused(le(H=48), "H=48", "multiples of 32")
    refused(le(W=100), "W=100", "multiples of 32")

    def es(flow=P, truth=P, mask=None, acc=Q, B=1, H=4, W=4):
        return lib.pivlfn_error_stats_accumulate(flow, truth, mask, acc, B, H, W, None)

    for name in ("flow", "truth", "acc"):
        refused(es(**{name: None}), "error_stats_accumulate", "null")
    refused(es(B=0), "B=0")
    refused(es(H=-1), "H=-1")
    refused(es(W=0), "W=0")
    refused(es(H=46341, W=46341), "2^31")
    with pytest.raises(ValueError):
        _lib.check(fe(k=9), "flow_errors")


# ---- the restatement against the reference's recorded results -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_against_reference_float64(name):
    c = CASES[name]
    got, ns = er.loss_value(c["fn"], c["args"], c["call"], c["output"], c["truth"])
    assert got.shape == c["f64"].shape == c["f32"].shape
    rel = np.abs(got - c["f64"]) / np.abs(c["f64"])
    bound = np.array([2 * n * U for n in ns])
    print(name, "rel", rel, "bound", bound)
    assert (rel <= bound).all(), (name, rel, bound)
    # ... and at least as close to the reference's float64 result as the reference's own float32 run is
    assert (rel <= np.abs(c["f32"] - c["f64"]) / np.abs(c["f64"])).all(), name


def test_signed_sums_against_a_sequential_float64_sum():
    """sum du, sum dv against math.fsum (exact), bounded relative to sum |du|, sum |dv| by N u; the largest error exactly."""
    import math
    c = CASES["level_piv1_L1"]
    for i, trio in enumerate(c["output"]):
        f, k = trio[2], 5 - i
        s, _ = er.flow_errors(f, c["truth"], None, k, 0.2)
        t = er.term_maps(f, c["truth"], None, k, 0.2)
        for b in range(len(f)):
            n = t["du"][b].size
            for q, key in ((4, "du"), (5, "dv")):
                exact = math.fsum(t[key][b].ravel())
                assert abs(s[b, q] - exact) <= n * U * math.fsum(np.abs(t[key][b]).ravel()), (i, b, key)
            assert s[b, 0] == n and s[b, 6] == t["epe"][b].max()


def test_demo_pair_against_the_recorded_reference_epe():
    from pivlfn.flo import read_flow
    out, true = (np.ascontiguousarray(read_flow(os.path.join(GOLD, f"DNS_turbulence_{n}.flo")).transpose(2, 0, 1))[None] for n in ("out", "flow"))
    rec = json.load(open(os.path.join(GOLD, "pin_report_evaluate.json")))["demo_DNS_turbulence"]
    assert list(out.shape[2:]) == rec["shape"][:2]
    s, _ = er.flow_errors(out, true)
    n = 256 * 256
    assert s[0, 0] == n
    assert abs(s[0, 2] / n - rec["epe_f64"]) <= 2 * n * U * rec["epe_f64"]
    assert abs(s[0, 1] / (2 * n) - rec["l1_f64"]) <= 2 * n * U * rec["l1_f64"]
    assert abs(s[0, 2] / n - rec["epe_f64"]) <= abs(rec["epe_f32"] - rec["epe_f64"])


# ---- the restatement against hand-computed cases ----------------------------------------------------------------------------------
def test_two_by_two_by_hand():
    """u = [[1,2],[3,4]], v = 0 against a zero truth: n = 4, l1 = epe = (1+2)+(3+4) = 10, sq = (1+4)+(9+16) = 30, max = 4."""
    s, m = er.flow_errors(_flow([[1, 2], [3, 4]]), _flow(np.zeros((2, 2))))
    assert s.tolist() == [[4, 10, 10, 30, 10, 0, 4]]
    assert m[0, 0].tolist() == [[1, 2], [3, 4]] and not m[0, 1].any() and m[0, 2].tolist() == [[1, 2], [3, 4]] and m.dtype == f32
    # v = (3, 4, ...) makes 3-4-5 triangles: du = 4, dv = 3 -> epe 5, l1 7, sq 25
    s, _ = er.flow_errors(_flow([[4, 4]], [[3, -3]]), _flow([[0, 0]]))
    assert s.tolist() == [[2, 14, 10, 50, 8, 0, 5]]


def test_the_tree_order_shows_where_it_matters():
    """1 x 3, du = (A, 1, -A), A = float32(1e16) > 2^53: the tree pads to 2 x 4 and adds (A + 1) + (-A + 0) = 0 -- A + 1 rounds to A.
    Left to right from the other end, or pairwise from the right, the answer would be 1."""
    A = float(f32(1e16))
    assert A + 1.0 == A
    s, _ = er.flow_errors(_flow([[A, 1, -A]]), _flow([[0, 0, 0]]))
    assert s[0, 4] == 0.0 and s[0, 0] == 3 and s[0, 6] == A
    s, _ = er.flow_errors(_flow([[1, A, -A]]), _flow([[0, 0, 0]]))      # (1 + A) + (-A + 0)
    assert s[0, 4] == 0.0
    s, _ = er.flow_errors(_flow([[A, -A, 1]]), _flow([[0, 0, 0]]))      # (A - A) + (1 + 0)
    assert s[0, 4] == 1.0
    # 3 x 3: rows are paired first -- ((a+b) + (d+e)) + ((c+0) + (f+0)) on top, ((g+h) + 0) + ((i+0) + 0) below
    a, b, c, d, e, f, g, h, i = (float(x) for x in np.random.default_rng(3).normal(0, 1, 9).astype(f32))
    s, _ = er.flow_errors(_flow([[a, b, c], [d, e, f], [g, h, i]]), _flow(np.zeros((3, 3))))
    top = ((a + b) + (d + e)) + ((c + 0.0) + (f + 0.0))
    bottom = ((g + h) + (0.0 + 0.0)) + ((i + 0.0) + (0.0 + 0.0))
    assert s[0, 4] == (top + bottom) + (0.0 + 0.0)
    assert er.tree_sum(np.array([[5.0]])) == 5.0 and er.tree_sum(np.arange(6.0).reshape(1, 6)) == 15.0


def test_unknown_truth_mask_and_all_excluded():
    flow, truth = _flow([[1, 2], [3, 4]]), _flow(np.zeros((2, 2)))
    for x in (np.nan, np.inf, -np.inf, 1e10, -1.0000001e9):
        for comp in (0, 1):
            t = truth.copy()
            t[0, comp, 0, 1] = x
            s, m = er.flow_errors(flow, t)
            assert s.tolist() == [[3, 8, 8, 26, 8, 0, 4]], x            # the pixel with u = 2 is gone
            assert np.isnan(m[0, :, 0, 1]).all() and not np.isnan(m[0, :, 1, :]).any()
    t = truth.copy()
    t[0, 0, 0, 1] = 1e9                                                 # the threshold itself is a value
    assert er.flow_errors(flow, t)[0][0, 0] == 4
    mask = np.array([[[0, 0], [9, 0]]], np.uint8)                       # leaves u = 3 out
    assert er.flow_errors(flow, truth, mask)[0].tolist() == [[3, 7, 7, 21, 7, 0, 4]]
    mask[:] = 1
    s, m = er.flow_errors(flow, truth, mask)
    assert s.tolist() == [[0, 0, 0, 0, 0, 0, 0]] and not np.signbit(s).any() and np.isnan(m).all()
    s, _ = er.flow_errors(flow, np.full_like(truth, np.nan))
    assert s.tolist() == [[0, 0, 0, 0, 0, 0, 0]]


def test_negative_zero_and_nan_in_the_flow():
    """An estimated -0.0 against a true +0.0 gives du = -0.0: the map keeps the sign, the reported sum reads +0.0.  A NaN in the
    estimated flow is not excluded: it is counted and every sum it enters is NaN (dv stays finite here)."""
    s, m = er.flow_errors(_flow(np.full((2, 2), -0.0), np.full((2, 2), -0.0)), _flow(np.zeros((2, 2))))
    assert s.tolist() == [[4, 0, 0, 0, 0, 0, 0]] and not np.signbit(s).any()
    assert np.signbit(m[0, :2]).all() and not np.signbit(m[0, 2]).any()
    s, _ = er.flow_errors(_flow([[-0.0]], [[-0.0]]), _flow([[0.0]]))     # a single pixel: no addition at all, still +0.0
    assert not np.signbit(s).any()
    s, m = er.flow_errors(_flow([[1, np.nan], [3, 4]]), _flow(np.zeros((2, 2))))
    assert s[0, 0] == 4 and np.isnan(s[0, [1, 2, 3, 4, 6]]).all() and s[0, 5] == 0.0
    assert np.isnan(m[0, 0, 0, 1]) and m[0, 1, 0, 1] == 0.0 and np.isnan(m[0, 2, 0, 1])
    s, _ = er.flow_errors(_flow([[1, np.inf], [3, 4]]), _flow(np.zeros((2, 2))))
    assert s[0, 2] == np.inf and s[0, 6] == np.inf


def test_pooled_truth_by_hand():
    """k = 1: P = ((1 + 2) + (3 + 4)) / 4 * 0.2; one unknown value or mask byte in the window excludes the pooled pixel."""
    truth = _flow([[1, 2, 5, 6], [3, 4, 7, 8]], [[0, 0, 0, 0], [0, 0, 0, 0]])
    P = (((1.0 + 2.0) + (3.0 + 4.0)) / 4.0) * 0.2, (((5.0 + 6.0) + (7.0 + 8.0)) / 4.0) * 0.2
    s, m = er.flow_errors(_flow([[1, 1]]), truth, None, 1, 0.2)
    du = (1.0 - P[0], 1.0 - P[1])
    assert s[0].tolist() == [2, abs(du[0]) + abs(du[1]), abs(du[0]) + abs(du[1]), du[0] * du[0] + du[1] * du[1], du[0] + du[1], 0,
                             max(abs(du[0]), abs(du[1]))]
    assert m[0, 0, 0].tolist() == [f32(du[0]), f32(du[1])]
    t = truth.copy()
    t[0, 1, 1, 3] = np.nan
    assert er.flow_errors(_flow([[1, 1]]), t, None, 1, 0.2)[0][0, :2].tolist() == [1, abs(du[0])]
    mask = np.zeros((1, 2, 4), np.uint8)
    mask[0, 0, 0] = 1
    assert er.flow_errors(_flow([[1, 1]]), truth, mask, 1, 0.2)[0][0, :2].tolist() == [1, abs(du[1])]
    # k = 2 on 4 x 4: the tree of trees, against numpy's own mean where the sums are exact
    t4 = np.arange(32, dtype=f32).reshape(1, 2, 4, 4)
    p, ex = er.pooled_truth(t4, None, 2, 1.0)
    assert p[0, :, 0, 0].tolist() == [7.5, 23.5] and not ex.any()
    with pytest.raises(AssertionError):
        er.pooled_truth(np.zeros((1, 2, 6, 4), f32), None, 2, 1.0)


def test_accumulate_errors_by_hand():
    flow = np.stack([_flow([[1, 2]], [[0, 2]])[0], _flow([[3, 4]], [[4, 0]])[0]])
    truth = np.zeros((2, 2, 1, 2), f32)
    truth[1, 0, 0, 1] = np.nan
    acc = er.accumulate_errors(np.zeros((6, 1, 2)), flow, truth)
    assert acc[:, 0, 0].tolist() == [2, 4, 4, 10, 16, 6] and acc[:, 0, 1].tolist() == [1, 2, 2, 4, 4, np.sqrt(8.0)]
    two = er.accumulate_errors(er.accumulate_errors(np.zeros((6, 1, 2)), flow[:1], truth[:1]), flow[1:], truth[1:])
    assert er.same_bits(acc, two)


# ---- Python side ---------------------------------------------------------------------------------------------------------------
def test_python_side_argument_errors():
    import pivlfn
    from pivlfn import evaluate as E
    assert pivlfn.flow_errors is E.flow_errors and pivlfn.level_errors is E.level_errors and pivlfn.ErrorStats is E.ErrorStats
    assert E.FIELDS == er.FIELDS == E.FlowErrors._fields[:7]
    flow = torch.zeros(1, 2, 4, 4)
    for pool in (0, 3, 64, 2.0, True):
        with pytest.raises(ValueError, match="pool"):
            E.flow_errors(flow, flow, pool=pool)
    with pytest.raises(NotImplementedError):
        E.flow_errors(flow, flow)                                  # a CPU tensor: there is no CPU path
    with pytest.raises(TypeError):
        E.flow_errors(flow.double(), flow)
    with pytest.raises(TypeError):
        E.flow_errors(flow.numpy(), flow)
    with pytest.raises(NotImplementedError):
        E.ErrorStats(4, 4, device="cpu")
    with pytest.raises(ValueError):
        E.ErrorStats(0, 4, device="cuda:0")
    with pytest.raises(ValueError, match="lowest_level"):
        E.level_errors(0, [], flow, 0.2)
    with pytest.raises(ValueError, match="6 levels"):
        E.level_errors(1, [[flow] * 3] * 5, flow, 0.2)
    e = E.FlowErrors(*(torch.tensor([v], dtype=torch.float64) for v in (4.0, 10.0, 10.0, 30.0, 10.0, -2.0, 4.0)))
    assert e.aee.item() == 2.5 and e.rmse.item() == np.sqrt(7.5) and e.bias.tolist() == [[2.5, -0.5]] and e.mean_l1.item() == 1.25
    assert e.map is None


def test_src_loss_names_and_signatures():
    """src/loss.py keeps the reference's names, signatures and defaults (recorded by tools/gen_evaluate_golden.py from the reference)."""
    import src.loss as L
    rec = json.load(open(os.path.join(GOLD, "pin_report_evaluate.json")))["signatures"]
    assert sorted(rec) == sorted(("EPE", "L1", "L2", "L1Loss", "L2Loss", "MultiScale", "LevelLoss", "hui_loss", "piv_loss"))
    for name, want in rec.items():
        obj = getattr(L, name)
        assert str(inspect.signature(obj.__init__ if inspect.isclass(obj) else obj)) == want, name
    assert L.__all__ == ['hui_loss', 'piv_loss']
    assert L.hui_loss().multiScales == [32, 16, 8, 4, 2] and L.hui_loss().div_flow == 1 / 20 and L.hui_loss().loss_weights == (0.32, 0.08, 0.02, 0.01, 0.005)
    assert L.piv_loss().multiScales == [32, 16, 8, 4, 2, 1] and L.piv_loss().loss_weights == (0.001, 0.001, 0.001, 0.001, 0.001, 0.01)
    assert L.piv_loss(version=2).multiScales == [32, 16, 8, 4, 2] and L.piv_loss(version=2).loss_weights == (0.001, 0.001, 0.001, 0.001, 0.01)
    assert isinstance(L.piv_loss(level_eval=True), L.LevelLoss) and L.piv_loss(level_eval=True).numScales == 6
    assert isinstance(L.hui_loss(level_eval=True, norm="L2").loss, L.L2) and isinstance(L.MultiScale().loss, L.L1)
    with pytest.raises(ValueError):
        L.piv_loss(version=3)
    with pytest.raises(ValueError):
        L.MultiScale(norm="L3")
    with pytest.raises(ValueError):
        L.MultiScale(l_weight=0.5)
    with pytest.raises(ValueError):
        L.LevelLoss()(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4))
    t = torch.zeros(1, 2, 96, 96)
    with pytest.raises(ValueError, match="power of two"):               # a window that is not a power of two, before any tensor check
        L.MultiScale(startScale=3)(torch.zeros(1, 2, 32, 32), t)
    with pytest.raises(ValueError, match="64"):                         # piv_loss(level_eval=True, version=2): a 64 x 64 window
        L.piv_loss(level_eval=True, version=2)([torch.zeros(1, 2, 1, 1)] * 6, t)


def test_finalize_errors_hand_made_accumulators():
    """Pixel (0,0): two frames du = (1, 3), dv = (2, -2), epe sum 6; pixel (0,1): nothing at all."""
    from pivlfn.evaluate import RESULT, finalize_errors
    acc = np.zeros((6, 1, 2))
    acc[:, 0, 0] = (2.0, 4.0, 0.0, 10.0, 8.0, 6.0)
    r = finalize_errors(acc, 3)
    assert list(r) == list(RESULT) and r["frames"] == 3 and r["count"].tolist() == [[2, 0]] and r["count"].dtype == np.int64
    want = dict(bias_u=2.0, bias_v=0.0, rms_u=1.0, rms_v=2.0, mean_epe=3.0)
    for k, w in want.items():
        assert r[k][0, 0] == w and np.isnan(r[k][0, 1]), k
    with pytest.raises(ValueError):
        finalize_errors(acc, 0)
    with pytest.raises(ValueError):
        finalize_errors(acc[:5], 3)


# ---- run.py ----------------------------------------------------------------------------------------------------------------------
def test_run_py_truth_argument_handling(tmp_path, monkeypatch):
    """Everything about --truth that can be wrong is reported before the first launch (and before a GPU is asked for): the flags'
    combinations, a missing truth file by name, a truth of another size, sizes --truth-levels cannot pool."""
    import PIL.Image
    import run as runpy
    from pivlfn.flo import write_flow
    seq, tr, out = tmp_path / "seq", tmp_path / "truth", tmp_path / "out"
    seq.mkdir()
    tr.mkdir()
    for name in ("a", "b"):
        for k in (1, 2):
            PIL.Image.fromarray(np.zeros((40, 64), np.uint8)).save(str(seq / f"{name}_img{k}.png"))
    base = ["--model", "piv", "-i", str(seq), "-o", str(out), "-p"]
    assert runpy.parser.parse_args([]).truth is None and runpy.parser.parse_args([]).truth_levels is False
    with pytest.raises(SystemExit, match="--truth-levels needs --truth"):
        runpy.main(base + ["--truth-levels"])
    with pytest.raises(SystemExit, match="-b/-c"):
        runpy.main(base + ["--truth", str(tr), "-b", "1.2"])
    with pytest.raises(SystemExit, match="not a directory"):
        runpy.main(base + ["--truth", str(tmp_path / "nowhere")])
    write_flow(np.zeros((40, 64, 2), f32), str(tr / "a_flow.flo"))
    with pytest.raises(SystemExit, match="b_flow.flo"):
        runpy.main(base + ["--truth", str(tr)])
    write_flow(np.zeros((64, 40, 2), f32), str(tr / "b_flow.flo"))
    with pytest.raises(SystemExit, match=r"b_flow.flo' is 64 x 40 .* 40 x 64"):
        runpy.main(base + ["--truth", str(tr)])
    write_flow(np.zeros((40, 64, 2), f32), str(tr / "b_flow.flo"))
    with pytest.raises(SystemExit, match="multiples of 32"):
        runpy.main(base + ["--truth", str(tr), "--truth-levels"])
    (tr / "b_flow.flo").write_bytes(b"not a flow file")
    with pytest.raises(SystemExit, match="not a .flo file"):
        runpy.main(base + ["--truth", str(tr)])
    monkeypatch.setenv("WORLD_SIZE", "2")                               # --truth itself is sharded; --validate is not
    with pytest.raises(SystemExit, match="single process"):
        runpy.main(base + ["--truth", str(tr), "--validate", "flag"])
    assert not out.exists()


def test_errors_json_keeps_a_nan_maximum_and_is_strict_json(tmp_path):
    """Pair b scored nothing (n = 0: its means are not numbers), pair c met a NaN in its flow: the run's maximum is NaN like c's, not
    the largest finite one, and every such value is written as null -- the file parses under a strict reader."""
    import run as runpy
    nan = float("nan")
    sums = torch.tensor([[4.0, 10.0, 10.0, 30.0, 10.0, -2.0, 4.0], [0.0] * 7, [2.0, nan, nan, nan, nan, 1.0, nan], [1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0]],
                        dtype=torch.float64)
    path = tmp_path / "errors.json"
    runpy.write_errors_json(str(path), ["a", "b", "c", "d"], sums, None, None, None, 0.2)

    def no_constants(name):
        raise AssertionError(f"{name} in errors.json")
    doc = json.loads(path.read_text(), parse_constant=no_constants)
    assert doc["pairs"]["a"] == {"n": 4, "aee": 2.5, "rmse": np.sqrt(7.5), "l1": 1.25, "bias_u": 2.5, "bias_v": -0.5, "max": 4.0}
    assert doc["pairs"]["b"] == {"n": 0, "aee": None, "rmse": None, "l1": None, "bias_u": None, "bias_v": None, "max": 0.0}
    assert doc["pairs"]["c"]["max"] is None and doc["pairs"]["c"]["aee"] is None and doc["pairs"]["c"]["bias_v"] == 0.5
    assert doc["total"]["n"] == 7 and doc["total"]["max"] is None and doc["total"]["aee"] is None and doc["total"]["bias_v"] == -1.0 / 7
    runpy.write_errors_json(str(path), ["a", "d"], sums[[0, 3]], torch.tensor([3, 0]), None, "mask", 0.2)
    doc = json.loads(path.read_text(), parse_constant=no_constants)
    assert doc["total"]["max"] == 4.0 and doc["excluded"] == {"pairs": {"a": 3, "d": 0}, "total": 3} and doc["validate"] == "mask"
