"""CPU: the flow-map contract of include/pivlfn.h as tests/flowmap_restatement.py states it, against closed forms -- a uniform
translation, a saddle whose every intermediate value is a dyadic rational, and the round trip forward and back -- and the host side:
check_params, the refusals of the three C entry points (made before any launch, so they need no GPU), and run.py's --ftle flags."""
import math

import numpy as np
import pytest

import flowmap_restatement as fr
from flowmap_restatement import LOST, OUT, UNDEFINED


def test_uniform_translation_is_exact_and_leaves_at_the_predicted_step():
    """(u, v) = (1.25, -0.5) on 12 x 20 for 5 fields: a particle is flagged OUT by the first sample taken outside the image, frozen
    where it was; live positions are the seeds plus k (u, v) exactly; the map's gradient is the identity, stretch == 1."""
    H, W, B, u, v = 12, 20, 5, 1.25, -0.5
    flows = np.empty((B, 2, H, W), np.float32)
    flows[:, 0], flows[:, 1] = u, v
    pos0, h, w = fr.lattice(H, W)
    pos, flag, path = fr.advect(flows, None, pos0, np.zeros(h * w, np.uint8), trace=True)
    inside = lambda x, y: (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)                       # noqa: E731
    # the step at which the sample is first taken outside: the position before field k is seed + k (u, v)
    first_out = np.full(h * w, B)
    for k in reversed(range(B)):
        first_out[~inside(pos0[0] + k * u, pos0[1] + k * v)] = k
    assert np.array_equal(flag, np.where(first_out < B, OUT, 0))
    for k in range(B):
        moved = np.minimum(first_out, k + 1)
        assert np.array_equal(path[k, 0], pos0[0] + moved * u) and np.array_equal(path[k, 1], pos0[1] + moved * v)
    assert np.array_equal(pos, path[-1]) and 0 < np.count_nonzero(flag) < flag.size
    assert (first_out[flag != 0] >= 1).all()                          # every seed lies inside: no particle is lost before field 1
    stretch, oflag = fr.ftle_stretch(pos, flag, h, w, 1)
    defined = (oflag & UNDEFINED) == 0
    assert defined.any() and (~defined).any() and (stretch[defined] == 1.0).all() and np.isnan(stretch[~defined]).all()
    assert np.array_equal(oflag & 3, flag.reshape(h, w))


def test_saddle_positions_are_the_closed_form_and_ftle_is_log1p_a():
    """u = a (x - 16), v = -a (y - 16), a = 1/32, 33 x 33, 6 fields: x - 16 grows by (1 + a) per field and y - 16 shrinks by (1 - a);
    33^6 and 31^6 fit 31 bits, so the closed forms are exact in float64 and the live positions equal them bit for bit.  The largest
    stretching is (1 + a)^6 everywhere it is defined: FTLE = log1p(a)."""
    steps, a = 6, 1.0 / 32
    flows = fr.saddle(steps, 33, a)
    pos0, h, w = fr.lattice(33, 33)
    pos, flag = fr.advect(flows, None, pos0, np.zeros(h * w, np.uint8))
    live = flag == 0
    assert np.array_equal(pos[0][live], 16.0 + (pos0[0][live] - 16.0) * (33.0 / 32.0) ** steps)
    assert np.array_equal(pos[1][live], 16.0 + (pos0[1][live] - 16.0) * (31.0 / 32.0) ** steps)
    assert set(np.unique(flag)) == {0, OUT}
    stretch, oflag = fr.ftle_stretch(pos, flag, h, w, 1)
    defined = (oflag & UNDEFINED) == 0
    # a column leaves once |x0 - 16| (33/32)^k > 16 at a sample, k <= 5: |x0 - 16| >= 14, six columns of 33; 27 stay (82 %), and the
    # 25 of them with both neighbours live are defined (76 %): flagged and unflagged nodes both exist, as do undefined live ones
    assert live.reshape(33, 33).all(0).sum() == 27 and live.sum() == 27 * 33 and defined.sum() == 25 * 33
    assert np.abs(np.log(stretch[defined]) / steps - math.log1p(a)).max() <= 1e-15
    # a node whose right neighbour left is undefined although it is live itself
    assert ((oflag == UNDEFINED).any())


def _round_trip_fields():
    return fr.plane_waves(np.random.default_rng(7), 7, 37, 53)


def test_round_trip_returns_live_particles_to_their_seeds():
    """Forward through 7 fields, then backward through the same fields newest first: p + F_k(p) = x is solved by a fixed-point
    iteration that contracts by q per pass, q = twice the largest node-to-node difference of the fields (a bilinear interpolant's
    Lipschitz bound in the 1-norm), so a step is off by at most peak q^iters / (1 - q) and 7 steps by 7 times that, the inverse map
    being an expansion by at most 1 / (1 - q) -- which the bound's last factor already grants per step for q < 1/2."""
    flows = _round_trip_fields()
    B, _, H, W = flows.shape
    pos0, h, w = fr.lattice(H, W)
    fwd, flag = fr.advect(flows, None, pos0, np.zeros(h * w, np.uint8))
    iters = 8
    back, bflag = fr.advect(flows[::-1], None, fwd, flag, backward=True, iters=iters)
    d = lambda f, ax: np.abs(np.diff(f.astype(np.float64), axis=ax)).max()                        # noqa: E731
    q = 2.0 * max(d(flows, 2), d(flows, 3))
    peak = float(np.abs(flows).max())
    assert q < 0.5 and peak <= 1.5
    tol = B * peak * q ** iters / (1.0 - q)
    live = bflag == 0
    assert live.mean() > 0.7 and (flag != 0).any()
    err = np.abs(back[:, live] - pos0[:, live]).max()
    print(f"round trip: q = {q:.4f}, tolerance {tol:.3e} px, largest error {err:.3e} px over {live.sum()} particles")
    assert err <= tol
    assert np.array_equal(back[:, flag != 0], fwd[:, flag != 0])       # what froze on the way out stays frozen on the way back
    one, _ = fr.advect(flows[::-1], None, fwd, flag, backward=True, iters=1)
    assert np.abs(one[:, live] - pos0[:, live]).max() > err            # one iteration is visibly worse: the iterations matter


def test_fields_of_the_gpu_tests_send_particles_out_through_every_side_and_keep_most():
    """What tests/test_gpu_flowmap.py relies on, established here without a GPU: on 37 x 53 the plane-wave fields keep most particles
    live and send the others OUT through all four sides; with holes and a mask, LOST occurs as well."""
    rng = np.random.default_rng(11)
    flows = fr.plane_waves(rng, 7, 37, 53)
    for spacing in (1, 2, 5):
        pos0, h, w = fr.lattice(37, 53, spacing)
        pos, flag, path = fr.advect(flows, None, pos0, np.zeros(h * w, np.uint8), trace=True)
        live = (flag == 0).mean()
        assert 0.6 < live < 0.95 and set(np.unique(flag)) == {0, OUT}, (spacing, live)
        if spacing == 1:
            assert fr.exits(pos0, path, flag, 37, 53) == {"left", "right", "top", "bottom"}
    holed, mask = fr.with_holes(rng, flows)
    pos0, h, w = fr.lattice(37, 53)
    _, flag = fr.advect(holed, mask, pos0, np.zeros(h * w, np.uint8))
    assert (flag == LOST).any() and (flag == OUT).any() and (flag == 0).any() and not (flag == (OUT | LOST)).any()


def test_a_sample_needs_all_four_corners_and_clamps_the_last_cell():
    """x = W - 1 is sampled in the last cell with fx = 1 (no read past the row); a corner of weight zero still makes the sample LOST;
    a position a hair outside is OUT; NaN is OUT."""
    H, W = 3, 4
    u = np.arange(H * W, dtype=np.float32).reshape(H, W)
    v = -u
    x = np.array([3.0, 0.0, 1.0, 3.0, np.nextafter(3.0, 4.0), -1e-300, np.nan, 1.5])
    y = np.array([2.0, 0.0, 1.0, 0.5, 1.0, 1.0, 1.0, 0.25])
    su, sv, flag = fr.sample(u, v, None, x, y)
    assert flag.tolist() == [0, 0, 0, 0, OUT, OUT, OUT, 0]
    assert su[:4].tolist() == [11.0, 0.0, 5.0, 5.0] and sv[3] == -5.0 and su[7] == 2.5
    m = np.zeros((H, W), np.uint8)
    m[2, 2] = 1                                                    # the corner (iy+1, ix+1) of the sample at (1, 1), weight zero
    assert fr.sample(u, v, m, x, y)[2].tolist() == [LOST, 0, LOST, 0, OUT, OUT, OUT, 0]
    u[0, 1] = np.inf
    assert fr.sample(u, v, None, x, y)[2].tolist() == [0, LOST, 0, 0, OUT, OUT, OUT, LOST]


def test_ftle_of_a_degenerate_lattice_is_undefined_everywhere():
    for h, w in ((1, 5), (5, 1), (1, 1)):
        pos = np.random.default_rng(0).normal(size=(2, h * w))
        stretch, oflag = fr.ftle_stretch(pos, np.zeros(h * w, np.uint8), h, w, 2)
        assert np.isnan(stretch).all() and (oflag == UNDEFINED).all()


# ---- the host side ---------------------------------------------------------------------------------------------------------------
def test_check_params():
    from pivlfn.flowmap import check_params
    assert check_params(37, 53, 1, 8) == (37, 53) and check_params(37, 53, 5) == (8, 11) and check_params(2, 2, 7) == (1, 1)
    assert check_params(None, None, 3, 32) == (None, None)
    for bad, word in (((37, 53, 0), "spacing=0"), ((37, 53, 32769), "spacing=32769"), ((37, 53, True), "spacing=True"),
                      ((37, 53, 1.0), "spacing=1.0"), ((37, 53, 1, 0), "iters=0"), ((37, 53, 1, 33), "iters=33"), ((1, 53), "H=1"),
                      ((37, 1), "W=1"), ((46341, 46341), "2^31"), ((37.0, 53), "H=37.0")):
        with pytest.raises(ValueError, match=word.replace("^", r"\^")):
            check_params(*bad)


def test_the_package_exports_the_names_and_refuses_what_needs_no_gpu():
    import pivlfn
    from pivlfn import flowmap
    assert (pivlfn.OUT, pivlfn.LOST, pivlfn.UNDEFINED) == (OUT, LOST, UNDEFINED) == (1, 2, 4)
    assert pivlfn.FlowMap is flowmap.FlowMap and pivlfn.FTLEField is flowmap.FTLEField
    with pytest.raises(ValueError, match="spacing=0"):
        pivlfn.FlowMap(8, 8, spacing=0)
    with pytest.raises(NotImplementedError, match="GPU only"):
        pivlfn.FlowMap(8, 8, device="cpu")


def test_summary_of_a_hand_made_field():
    import torch
    from pivlfn import FTLEField
    nan = math.nan
    ftle = torch.tensor([[0.5, nan, 0.25], [nan, -0.25, nan]], dtype=torch.float32)
    flag = torch.tensor([[0, OUT | UNDEFINED, 0], [LOST | UNDEFINED, 0, UNDEFINED]], dtype=torch.uint8)
    s = FTLEField(ftle, ftle.double().exp(), flag, 1, 1).summary()
    assert s == {"out": 1 / 6, "lost": 1 / 6, "undefined": 0.5, "defined": 3, "max_ftle": 0.5, "mean_ftle": 0.5 / 3}
    none = FTLEField(torch.full((1, 2), nan), torch.full((1, 2), nan, dtype=torch.float64), torch.full((1, 2), UNDEFINED, dtype=torch.uint8), 3, 2)
    s = none.summary()
    assert s["undefined"] == 1.0 and s["defined"] == 0 and math.isnan(s["max_ftle"]) and math.isnan(s["mean_ftle"])


def refusals(lib, flows, mask, pos, flag, trace, stretch, oflag, B, H, W, N, h, w):
    """Every error of the contract through the C entry points with the given addresses (never dereferenced: each call fails its checks
    before any launch); also called by the GPU test with real buffers, whose contents must stay."""
    def advect(**kw):
        a = dict(flows=flows, mask=mask, B=B, H=H, W=W, pos=pos, flag=flag, N=N, backward=0, iters=8, trace=trace)
        a.update(kw)
        return lib.pivlfn_flowmap_advect(a["flows"], a["mask"], a["B"], a["H"], a["W"], a["pos"], a["flag"], a["N"], a["backward"], a["iters"],
                                         a["trace"], None)

    def ftle(**kw):
        a = dict(pos=pos, flag=flag, h=h, w=w, spacing=1, stretch=stretch, oflag=oflag)
        a.update(kw)
        return lib.pivlfn_flowmap_ftle(a["pos"], a["flag"], a["h"], a["w"], a["spacing"], a["stretch"], a["oflag"], None)

    def seed(**kw):
        a = dict(pos=pos, flag=flag, h=h, w=w, spacing=1)
        a.update(kw)
        return lib.pivlfn_flowmap_seed(a["pos"], a["flag"], a["h"], a["w"], a["spacing"], None)

    def refused(rc, *words):
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1, (rc, msg)
        for word in words:
            assert word in msg, (word, msg)

    for name in ("flows", "pos", "flag"):
        refused(advect(**{name: None}), "flowmap_advect", "null")
    refused(advect(H=1), "H=1")
    refused(advect(W=1), "W=1")
    refused(advect(H=-3), "H=-3")
    refused(advect(H=46341, W=46341), "2^31")
    refused(advect(N=-1), "N=-1")
    refused(advect(B=-1), "B=-1")
    refused(advect(iters=0), "iters=0")
    refused(advect(iters=33), "iters=33")
    refused(advect(backward=1, iters=0), "iters=0")
    refused(advect(backward=2), "backward=2")
    refused(advect(N=0, iters=0), "iters=0")                       # the ranges are checked even where nothing would be launched
    px = B * H * W
    refused(advect(pos=flows), "pos overlaps flows")
    refused(advect(pos=flows + px * 8 - 8), "pos overlaps flows")
    refused(advect(pos=mask), "pos overlaps mask")
    refused(advect(flag=flows + px * 8 - 1), "flag overlaps flows")
    refused(advect(flag=mask + px - 1), "flag overlaps mask")
    refused(advect(trace=flows), "trace overlaps flows")
    refused(advect(trace=mask - B * N * 16 + 1), "trace overlaps mask")
    refused(advect(flag=pos + N * 16 - 1), "pos overlaps flag")
    refused(advect(trace=pos + 8), "trace overlaps pos")
    refused(advect(trace=flag - B * N * 16 + 1), "trace overlaps flag")
    for name in ("pos", "flag", "stretch", "oflag"):
        refused(ftle(**{name: None}), "flowmap_ftle", "null")
    refused(ftle(h=0), "h=0")
    refused(ftle(w=-1), "w=-1")
    refused(ftle(h=46341, w=46341), "2^31")
    refused(ftle(spacing=0), "spacing=0")
    refused(ftle(spacing=32769), "spacing=32769")
    refused(ftle(stretch=pos + 8), "stretch overlaps pos")
    refused(ftle(stretch=flag), "stretch overlaps flag")
    refused(ftle(oflag=pos + h * w * 16 - 1), "oflag overlaps pos")
    refused(ftle(oflag=flag), "oflag overlaps flag")
    refused(ftle(oflag=stretch + h * w * 8 - 1), "stretch overlaps oflag")
    for name in ("pos", "flag"):
        refused(seed(**{name: None}), "flowmap_seed", "null")
    refused(seed(h=0), "h=0")
    refused(seed(spacing=0), "spacing=0")
    refused(seed(h=46341, w=46341), "2^31")
    refused(seed(h=2, w=70000, spacing=32768), "past pixel 2^31")
    refused(seed(flag=pos + 3), "pos overlaps flag")
    return advect


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    """Every refusal comes from the host, before any launch, as PIVLFN_ERR_ARG with a message naming the problem (a launch on a machine
    without a GPU would return PIVLFN_ERR_HIP instead); N == 0 or B == 0 succeeds without a launch and without reading a pointer."""
    from pivlfn import _lib
    lib = _lib.load()
    P = 1 << 20                     # non-null, 8-byte aligned, never dereferenced
    flows, mask, pos, flag, trace, stretch, oflag = (P + (i << 32) for i in range(7))        # ranges that cannot overlap at these sizes
    advect = refusals(lib, flows, mask, pos, flag, trace, stretch, oflag, 3, 8, 9, 72, 8, 9)
    assert advect(N=0) == 0 and advect(B=0) == 0
    assert advect(N=0, flows=None, pos=None, flag=None, trace=None, mask=None) == 0
    assert advect(B=0, flows=None, mask=None, trace=None) == 0
    with pytest.raises(ValueError, match="iters=33"):
        _lib.check(advect(iters=33), "flowmap_advect")


def test_run_py_ftle_flags_parse_and_are_checked_before_a_gpu_is_needed(tmp_path, monkeypatch):
    import run as runpy
    plain = runpy.parser.parse_args(["-i", "x"])
    assert plain.ftle is None and plain.ftle_steps is None and plain.ftle_image is False and plain.ftle_max is None
    assert not [ln for ln in runpy.args_lines(plain) if "ftle" in ln]
    assert runpy.parser.parse_args(["--ftle"]).ftle == 1
    full = runpy.parser.parse_args(["--ftle", "2", "--ftle-steps", "3", "--ftle-image", "--ftle-max", "0.5"])
    assert (full.ftle, full.ftle_steps, full.ftle_image, full.ftle_max) == (2, 3, True, 0.5)
    lines = runpy.args_lines(full)
    assert "ftle: 2\n" in lines and "ftle_steps: 3\n" in lines and "ftle_image: True\n" in lines and "ftle_max: 0.5\n" in lines
    assert not [ln for ln in lines if ln.startswith(("color", "quality", "pod", "vortex"))]
    assert not [ln for ln in runpy.args_lines(runpy.parser.parse_args(["--vortex"])) if "ftle" in ln]
    base = ["--model", "piv", "-i", str(tmp_path), "-o", str(tmp_path / "out")]
    for extra, word in ((["--ftle-image"], "need --ftle"), (["--ftle-steps", "3"], "need --ftle"), (["--ftle-max", "1"], "need --ftle"),
                        (["--ftle", "--ftle-max", "1"], "--ftle-max needs --ftle-image"), (["--ftle", "0"], "spacing=0"),
                        (["--ftle", "40000"], "spacing=40000"), (["--ftle", "--ftle-steps", "0"], "--ftle-steps 0"),
                        (["--ftle", "--ftle-image", "--ftle-max", "0"], "--ftle-max 0"),
                        (["--ftle", "--ftle-image", "--ftle-max", "nan"], "--ftle-max nan"), (["--ftle", "-p"], "consecutive in time"),
                        (["--ftle", "-c", "1.5"], "-b/-c"), (["--ftle", "-b", "0.5"], "-b/-c")):
        with pytest.raises(SystemExit, match=word):
            runpy.main(base + extra)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="single process"):
        runpy.main(base + ["--ftle"])
    assert not (tmp_path / "out").exists()
