"""GPU: snapshot POD.  pivlfn_snapshot_gram against the float64 restatement inside the one bound its contract allows, and its
invariants bit for bit; pivlfn_snapshot_project bit for bit; both on a side stream and inside a graph; FlowPOD against the SVD of the
planted case; run.py --pod.  Everything lives in guarded buffers with NaN wherever the contract says nothing is read."""
import os

import numpy as np
import pytest
import torch

import pod_restatement as pr
from guarded import check_guards, guarded, same_bits
from pivlfn import _lib

pytestmark = pytest.mark.gpu

SLAB = 2048                     # PIVLFN_GRAM_SLAB
F32, F64, U8 = torch.float32, torch.float64, torch.uint8
TAIL = 8                        # NaN rows behind row n


def _x_buffer(dev, X, ldx, shift=0):
    """X [n,P] (host float32) as the first n rows and P columns of a [(n + TAIL), ldx] device view that starts `shift` floats into a
    guarded allocation; every other float of the view is NaN.  Returns (view, the guarded base)."""
    n, P = X.shape
    base = guarded(((n + TAIL) * ldx + 4,), F32, dev, "nan")
    view = base[shift:shift + (n + TAIL) * ldx].view(n + TAIL, ldx)
    view[:n, :P] = torch.from_numpy(X).to(dev)
    assert bool(torch.isnan(view[n:]).all()) and (ldx == P or bool(torch.isnan(view[:n, P:]).all()))
    return view, base


def _gram(dev, X, ldx=None, shift=0, stream=None):
    """pivlfn_snapshot_gram of host X in guarded buffers: G [n,n] float64 on the host."""
    lib = _lib.load()
    n, P = X.shape
    ldx = P if ldx is None else ldx
    view, base = _x_buffer(dev, X, ldx, shift)
    G = guarded((n, n), F64, dev, "sentinel")
    nbytes = lib.pivlfn_snapshot_gram_workspace_bytes(n, P)
    assert nbytes >= 8 and nbytes % 8 == 0
    ws = guarded((nbytes,), U8, dev, "sentinel")
    assert ws.data_ptr() % 8 == 0
    st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    _lib.check(lib.pivlfn_snapshot_gram(view.data_ptr(), n, P, ldx, G.data_ptr(), ws.data_ptr(), nbytes, st), "snapshot_gram")
    torch.cuda.synchronize()
    for t, what in ((base, "X"), (G, "G"), (ws, "workspace")):
        check_guards(t, f"snapshot_gram n={n} P={P} ldx={ldx}: {what}")
    assert bool(torch.isnan(view[n:]).all()), "a row behind row n was written"
    return G.cpu().clone()


def _project(dev, X, Wt, ldx=None):
    lib = _lib.load()
    n, P = X.shape
    K = Wt.shape[1]
    ldx = P if ldx is None else ldx
    view, base = _x_buffer(dev, X, ldx)
    w = guarded((n, K), F64, dev, "nan")
    w.copy_(torch.from_numpy(Wt))
    out = guarded((K, P), F64, dev, "sentinel")
    _lib.check(lib.pivlfn_snapshot_project(view.data_ptr(), n, P, ldx, w.data_ptr(), K, out.data_ptr(),
                                           torch.cuda.current_stream(dev).cuda_stream), "snapshot_project")
    torch.cuda.synchronize()
    for t, what in ((base, "X"), (w, "Wt"), (out, "out")):
        check_guards(t, f"snapshot_project n={n} K={K} P={P} ldx={ldx}: {what}")
    return out.cpu().clone()


def _data(n, P, seed):
    """float32 [n,P]: values of mixed sign and four decades of magnitude, so that a wrong order of additions shows."""
    g = np.random.default_rng(seed)
    return (g.normal(0, 1, (n, P)) * 10.0 ** g.integers(-2, 3, (n, 1))).astype(np.float32)


@pytest.fixture(scope="module")
def planted():
    flows = pr.planted_flows()
    return flows, np.ascontiguousarray(flows.reshape(pr.PLANTED_N, -1))


@pytest.fixture(scope="module")
def planted_gram(dev, planted):
    return _gram(dev, planted[1], ldx=236)


# ---- Gram: values ------------------------------------------------------------------------------------------------------------------
GRAM_SHAPES = [(1, 1), (16, 4), (17, 30), (37, 234), (65, 2 * SLAB + 6)]


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n,P", GRAM_SHAPES)
def test_gram_matches_the_restatement(n, P, pad, dev, planted):
    X = planted[1] if (n, P) == (37, 234) else _data(n, P, 100 + n)
    G = _gram(dev, X, ldx=P + pad).numpy()
    ref = pr.gram(X)
    bound = pr.gram_bound(ref, P)
    worst = float((np.abs(G - ref) / np.where(bound > 0, bound, 1.0)).max())
    print(f"gram n={n} P={P} ldx={P + pad}: worst |G - G_ref| / bound = {worst:.3g}")
    assert np.isfinite(G).all()
    assert (np.abs(G - ref) <= bound).all()


def test_gram_of_many_snapshots_adds_its_slabs_itself(dev):
    """n = 1985 is the first n with 512 blocks of 64 x 64, where one workgroup walks all slabs of its block and adds them in
    registers; below, with more than one slab, the slab sums pass through the workspace.  The same rows give the same bits either
    way: the 65 x 65 corner equals the Gram matrix of the first 65 rows alone."""
    n, P = 1985, SLAB + 5
    lib = _lib.load()
    assert lib.pivlfn_snapshot_gram_workspace_bytes(n, P) < 64 * 64 * 8 <= lib.pivlfn_snapshot_gram_workspace_bytes(65, P)
    X = _data(n, P, 77)
    G = _gram(dev, X)
    ref = pr.gram(X)
    assert (np.abs(G.numpy() - ref) <= pr.gram_bound(ref, P)).all()
    assert same_bits(G, G.t().contiguous())
    small = _gram(dev, X[:65])
    assert same_bits(small, G[:65, :65].contiguous())
    far = _gram(dev, np.ascontiguousarray(X[1900:1985]))
    assert same_bits(far, G[1900:, 1900:].contiguous())


# ---- Gram: invariants, bit for bit ---------------------------------------------------------------------------------------------------
def test_gram_is_symmetric(dev, planted_gram):
    assert same_bits(planted_gram, planted_gram.t().contiguous())
    G = _gram(dev, _data(65, 2 * SLAB + 6, 165))
    assert same_bits(G, G.t().contiguous())


def test_gram_follows_a_permutation_of_the_rows(dev, planted, planted_gram):
    perm = np.random.default_rng(3).permutation(37)
    G = _gram(dev, np.ascontiguousarray(planted[1][perm]), ldx=236)
    assert same_bits(G, planted_gram[perm][:, perm].contiguous())
    X = _data(65, 2 * SLAB + 6, 165)                    # across the two 64-blocks: rows change block and operand side
    perm = np.random.default_rng(4).permutation(65)
    assert same_bits(_gram(dev, np.ascontiguousarray(X[perm])), _gram(dev, X)[perm][:, perm].contiguous())


def test_gram_entry_does_not_depend_on_the_other_rows(dev, planted, planted_gram):
    assert same_bits(_gram(dev, np.ascontiguousarray(planted[1][:5]), ldx=236), planted_gram[:5, :5].contiguous())


def test_gram_is_the_same_from_run_to_run(dev, planted, planted_gram):
    assert same_bits(_gram(dev, planted[1], ldx=236), planted_gram)


def test_a_nan_stays_in_its_row_and_column(dev, planted, planted_gram):
    X = planted[1].copy()
    X[3, 100] = np.nan
    G = _gram(dev, X, ldx=236)
    hit = torch.zeros(37, 37, dtype=torch.bool)
    hit[3, :] = True
    hit[:, 3] = True
    assert torch.equal(torch.isnan(G), hit)
    assert same_bits(G[~hit], planted_gram[~hit])
    X[3, 100] = np.inf
    G = _gram(dev, X, ldx=236)
    assert torch.equal(~torch.isfinite(G), hit) and same_bits(G[~hit], planted_gram[~hit])


def test_rows_off_16_bytes_give_the_same_bits(dev, planted, planted_gram):
    """planted_gram took the 16-byte loads (aligned base, ldx = 236); one float into the allocation no row is aligned."""
    assert same_bits(_gram(dev, planted[1], ldx=236, shift=1), planted_gram)
    assert same_bits(_gram(dev, planted[1], ldx=234), planted_gram)          # rows alternately aligned to 8 and 16: scalar path
    X = _data(65, 2 * SLAB + 6, 165)
    assert same_bits(_gram(dev, X, ldx=2 * SLAB + 8, shift=1), _gram(dev, X, ldx=2 * SLAB + 8))


# ---- project --------------------------------------------------------------------------------------------------------------------------
def _project_cases():
    """K = 5 and K = 16: the first and the last K of project_kernel<16>, which the cases before it (K <= 4 and K >= 17) pass by."""
    import analysis_plans as ap
    return list(ap.PROJECT_CASES)


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n,K,P", [(1, 1, 1), (37, 3, 234), (5, 64, 1029), (70, 17, 300)] + _project_cases())
def test_project_equals_the_sequential_loop(n, K, P, pad, dev):
    X = _data(n, P, 200 + n)
    Wt = np.random.default_rng(300 + K).normal(0, 1, (n, K))
    out = _project(dev, X, Wt, ldx=P + pad)
    assert same_bits(out, torch.from_numpy(pr.project(X, Wt)))


# ---- stream and capture ---------------------------------------------------------------------------------------------------------------
def _stream_case(seed):
    X = _data(65, 2 * SLAB + 6, seed)                   # the Gram launch and its fold kernel, three slabs
    Wt = np.random.default_rng(seed + 1).normal(0, 1, (65, 5))
    return torch.from_numpy(X), torch.from_numpy(Wt)


def _enqueue(lib, X, Wt, G, out, ws, stream):
    n, P = X.shape
    rc = lib.pivlfn_snapshot_gram(X.data_ptr(), n, P, P, G.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    return rc or lib.pivlfn_snapshot_project(X.data_ptr(), n, P, P, Wt.data_ptr(), Wt.shape[1], out.data_ptr(), stream)


def _eager(dev, seed):
    lib = _lib.load()
    X, Wt = (t.to(dev) for t in _stream_case(seed))
    n, P = X.shape
    G = torch.full((n, n), float("nan"), dtype=F64, device=dev)
    out = torch.full((Wt.shape[1], P), float("nan"), dtype=F64, device=dev)
    ws = torch.full((lib.pivlfn_snapshot_gram_workspace_bytes(n, P),), 0xFF, dtype=U8, device=dev)
    _lib.check(_enqueue(lib, X, Wt, G, out, ws, torch.cuda.current_stream(dev).cuda_stream), "pod")
    torch.cuda.synchronize()
    return X, Wt, G, out


def test_both_entry_points_run_in_order_on_the_stream_they_are_given(dev):
    """Behind a bounded delay on a side stream (a chain of matrix products, some tens of milliseconds) the inputs are copied over NaN
    and the two calls are enqueued with no host synchronisation; outputs pre-filled with the sentinel equal the eager result.  A
    launch on another stream would read the NaN or leave the sentinel."""
    lib = _lib.load()
    X, Wt, G_ref, out_ref = _eager(dev, 31)
    n, P = X.shape
    m = 8192
    a, b, c = torch.randn(m, m, device=dev), torch.randn(m, m, device=dev), torch.empty(m, m, device=dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        torch.mm(a, b, out=c)
    Xs = guarded(tuple(X.shape), F32, dev, "nan")
    Ws = guarded(tuple(Wt.shape), F64, dev, "nan")
    G = guarded((n, n), F64, dev, "sentinel")
    out = guarded(tuple(out_ref.shape), F64, dev, "sentinel")
    ws = guarded((lib.pivlfn_snapshot_gram_workspace_bytes(n, P),), U8, dev, "sentinel")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(10):
            torch.mm(a, b, out=c)
        delayed = torch.cuda.Event()
        delayed.record(side)
        Xs.copy_(X, non_blocking=True)
        Ws.copy_(Wt, non_blocking=True)
        rc = _enqueue(lib, Xs, Ws, G, out, ws, side.cuda_stream)
        still_waiting = not delayed.query()
    _lib.check(rc, "pod")
    side.synchronize()
    torch.cuda.synchronize()
    assert still_waiting, "the delay ran out before the calls were enqueued: the test would not see a launch on another stream"
    assert same_bits(G, G_ref) and same_bits(out, out_ref)
    for t in (Xs, Ws, G, out, ws):
        check_guards(t, "pod on a side stream")


def test_both_entry_points_are_graph_capturable(dev):
    lib = _lib.load()
    first, second = _eager(dev, 41), _eager(dev, 51)
    X, Wt = torch.zeros_like(first[0]), torch.zeros_like(first[1])
    n, P = X.shape
    G, out = torch.empty_like(first[2]), torch.empty_like(first[3])
    ws = torch.empty((lib.pivlfn_snapshot_gram_workspace_bytes(n, P),), dtype=U8, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = _enqueue(lib, X, Wt, G, out, ws, torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "pod")
    for src in (first, second, first):
        X.copy_(src[0])
        Wt.copy_(src[1])
        for t in (G, out):
            t.fill_(float("nan"))
        ws.fill_(0xFF)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(G, src[2]) and same_bits(out, src[3]), "a replay differs from the eager result"


# ---- FlowPOD ----------------------------------------------------------------------------------------------------------------------------
FIELDS = ("modes", "mean", "coeff", "energy", "fraction", "eigenvalues", "gram")


def test_flowpod_on_the_planted_case(dev, planted):
    from pivlfn import FlowPOD, PODResult
    flows = torch.from_numpy(planted[0]).to(dev)
    pieces = FlowPOD(9, 13, 37, device=dev)
    assert (pieces.P, pieces.ld, tuple(pieces.store.shape)) == (234, 236, (37, 236))
    for lo, hi in ((0, 5), (5, 6), (6, 37)):
        pieces.update(flows[lo:hi])
    with pytest.raises(ValueError, match="full"):
        pieces.update(flows[:1])
    whole = FlowPOD(9, 13, 40, device=dev)
    whole.update(flows)
    a, b = pieces.solve(modes=3), whole.solve(3)
    assert isinstance(a, PODResult)
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == np.float64 and same_bits(torch.from_numpy(x), torch.from_numpy(y)), f
    assert a.modes.shape == (3, 2, 9, 13) and a.mean.shape == (2, 9, 13) and a.coeff.shape == (37, 3) and a.gram.shape == (37, 37)
    assert np.array_equal(whole.store[:37, :234].cpu().numpy(), planted[1])             # cell = 1: the flow itself

    lam_svd, modes_svd, coeff_svd = pr.svd_reference(planted[1], 3)
    l1 = lam_svd[0]
    modes = a.modes.reshape(3, -1)
    want_coeff = pr.sign_rule(coeff_svd.T).T                                            # the sign rule is stated on V's columns
    flip = np.sign(np.sum(want_coeff * coeff_svd, axis=0))
    errs = dict(eigenvalues=np.abs(a.eigenvalues[:36] - lam_svd[:36]).max() / l1,
                modes=np.abs(modes - flip[:, None] * modes_svd).max(),
                coeff=np.abs(a.coeff - want_coeff).max() / np.sqrt(l1),
                orthonormality=np.abs(modes @ modes.T - np.eye(3)).max(),
                mean=np.abs(a.mean.reshape(-1) - planted[1].astype(np.float64).mean(axis=0)).max())
    print("FlowPOD vs SVD:", errs)
    assert errs["eigenvalues"] <= 1e-9 and errs["modes"] <= 1e-9 and errs["coeff"] <= 1e-9
    assert errs["orthonormality"] <= 1e-12 and errs["mean"] <= 1e-12
    assert np.allclose(a.energy, a.eigenvalues[:3] / 37, rtol=1e-15) and np.allclose(a.fraction, [0.775, 0.194, 0.031], atol=0.002)
    for k in range(3):                                                                  # the sign rule on what came out
        col = a.coeff[:, k]
        assert col[np.flatnonzero(np.abs(col) == np.abs(col).max())[0]] > 0
    rms = np.sqrt(np.mean([(a.reconstruct(i, 3) - planted[0][i].astype(np.float64)) ** 2 for i in range(37)]))
    assert 0.0085 < rms < 0.0100
    with pytest.raises(ValueError, match="modes"):
        whole.solve(37)
    one = FlowPOD(9, 13, 2, device=dev)
    one.update(flows[:1])
    with pytest.raises(ValueError, match="at least 2"):
        one.solve(1)


def test_flowpod_cells_and_masks(dev):
    from pivlfn import FlowPOD, decimate_flow
    g = torch.Generator().manual_seed(5)
    flows = torch.randn(6, 2, 18, 26, generator=g).to(dev)
    mask = (torch.rand(6, 18, 26, generator=g) < 0.3).to(torch.uint8).to(dev)
    mask[:, ::4, ::4] = 0                                    # one vector of every 4 x 4 cell stays: no cell is empty
    pod = FlowPOD(18, 26, 6, cell=4, device=dev)
    assert (pod.ch, pod.cw, pod.P, pod.ld) == (5, 7, 70, 72)
    pod.update(flows[:2], mask[:2])
    pod.update(flows[2:], mask[2:])
    mean, count = decimate_flow(flows, 4, mask)
    assert int((count == 0).sum()) == 0
    assert same_bits(pod.store[:, :70].contiguous(), mean.view(6, 70)) and not bool(pod.store[:, 70:].any())
    res = pod.solve(2)
    assert res.modes.shape == (2, 2, 5, 7) and (res.cell, res.H, res.W) == (4, 18, 26)

    emptied = mask.clone()
    emptied[3, 4:8, 8:12] = 1                               # every vector of cell (1, 2) of frame 3
    bad = FlowPOD(18, 26, 6, cell=4, device=dev)
    bad.update(flows, emptied)
    with pytest.raises(ValueError, match=r"1 cells .* empty.*--validate replace.*larger cell"):
        bad.solve(2)


# ---- run.py ------------------------------------------------------------------------------------------------------------------------------
def test_run_py_pod(tmp_path, dev, capsys):
    """run.py -p --pod 2 --pod-cell 8 on five synthetic 64 x 64 pairs: pod.npz equals, array for array and bit for bit, a FlowPOD fed
    with the written .flo files; args.txt names the flags; --color adds the mode pictures; --validate replace runs; --validate mask
    at cell 1 runs or ends with the empty-cell message."""
    import PIL.Image
    import run as runpy
    from pivlfn import FlowPOD, synth
    from pivlfn.flo import read_flow
    H = W = 64
    seq = tmp_path / "seq"
    seq.mkdir()
    names = [f"p{k}" for k in range(5)]
    for k, name in enumerate(names):
        a, b, _ = synth.particle_pair(H, W, 950 + k)
        PIL.Image.fromarray(a).save(str(seq / f"{name}_img1.png"))
        PIL.Image.fromarray(b).save(str(seq / f"{name}_img2.png"))
    base = ["--model", "piv", "-i", str(seq), "-p", "--batch", "2"]
    assert runpy.main(base + ["-o", str(tmp_path / "plain")]) == 5
    assert runpy.main(base + ["-o", str(tmp_path / "pod"), "--pod", "2", "--pod-cell", "8", "--color"]) == 5
    said = capsys.readouterr().out
    assert "mode 1:" in said and "mode 2:" in said and "% of the fluctuation energy" in said
    plain, out = (tmp_path / d / "piv-synthetic" / "seq" for d in ("plain", "pod"))
    assert not (plain / "pod.npz").exists() and not [ln for ln in open(plain / "args.txt") if ln.startswith("pod")]
    lines = list(open(out / "args.txt"))
    assert "pod: 2\n" in lines and "pod_cell: 8\n" in lines
    pod = FlowPOD(H, W, 5, cell=8, device=dev)
    for n in names:
        data = open(out / "flow" / f"{n}_out.flo", "rb").read()
        assert data == open(plain / "flow" / f"{n}_out.flo", "rb").read(), n
        pod.update(torch.from_numpy(read_flow(str(out / "flow" / f"{n}_out.flo"))).to(dev).permute(2, 0, 1)[None].contiguous())
    want = pod.solve(2)
    z = np.load(out / "pod.npz")
    assert sorted(z.files) == sorted(FIELDS + ("cell", "H", "W"))
    for f in FIELDS:
        assert same_bits(torch.from_numpy(z[f]), torch.from_numpy(getattr(want, f))), f
    assert (int(z["cell"]), int(z["H"]), int(z["W"])) == (8, 64, 64) and z["modes"].shape == (2, 2, 8, 8)
    for k in (1, 2):
        im = PIL.Image.open(out / f"pod_mode{k}.png")
        assert im.mode == "RGB" and im.size == (8, 8)
    assert not (out / "pod_mode3.png").exists()

    val = ["--validate-radius", "2", "--validate-eps", "0.01", "--validate-thresh", "0.5"]
    assert runpy.main(base + ["-o", str(tmp_path / "rep"), "--pod", "2", "--pod-cell", "8", "--validate", "replace"] + val) == 5
    assert (tmp_path / "rep" / "piv-synthetic" / "seq" / "pod.npz").exists()
    try:
        assert runpy.main(base + ["-o", str(tmp_path / "mask"), "--pod", "2", "--validate", "mask"] + val) == 5
        assert (tmp_path / "mask" / "piv-synthetic" / "seq" / "pod.npz").exists()
    except SystemExit as e:
        assert "empty" in str(e) and "--validate replace" in str(e)
    with pytest.raises(SystemExit, match="2..4096"):
        runpy.main(base + ["-o", str(tmp_path / "few"), "--pod", "1", "--num_images", "1"])
