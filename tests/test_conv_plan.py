"""The direct convolution's launcher, asked on the host which kernel it picks (pivlfn_conv2d_nhwc_plan; no GPU needed).

launch_conv picks one of about thirty compiled kernels per call, from the layer geometry and from the batch: choose_conv
(csrc/conv_mfma.hip, with the dedicated kernels' choices in conv_c3k7.hip, conv_k1.hip and conv_s2.hip) names a kernel's launch function
and its plan in one statement, so a plan reported here is the kernel launched.  TILE_CASES holds one
layer and shape for every plan -- (family, rows, channels, staging class, split-K shares) -- a fixed grid of layers and shapes can
reach; tests/test_gpu_conv_tiles.py runs each against float64.  Here, on the plan function alone:
  * every case still reaches the plan it was chosen for;
  * the grid reaches exactly the plans TILE_CASES reaches: a kernel instantiation added later without a case fails here;
  * the grid reaches every compiled instantiation;
  * a geometry accepted at B = 1 is accepted at every B, and one image's split-K shares are the same at every B."""
import ctypes

import pytest

from pivlfn import _lib

V2, V1, K1, C3K7, S2, COL7, ROW7 = 1, 2, 3, 4, 5, 6, 7          # PIVLFN_CONV_PLAN_* of include/pivlfn.h
POLICY = "the launcher's policy changed: re-derive the shapes of this test"
BATCHES = (1, 2, 3, 5)


def _r(n, m):
    return -(-n // m) * m


def plan(co, ci, kh, kw, s, pad, H, W, B, res=False, leaky=1, xs=None, ys=None):
    """The five plan values, or None where pivlfn_conv2d_nhwc refuses the geometry."""
    out = (ctypes.c_int * 5)()
    rc = _lib.load().pivlfn_conv2d_nhwc_plan(co, ci, kh, kw, B, H, W, s, pad[0], pad[1], int(res), int(leaky),
                                             xs or _r(ci, 4), ys or _r(co, 4), out)
    assert rc in (0, 1), rc
    return tuple(out) if rc == 0 else None


def case_leaky(case):
    """As tests/test_gpu_guarded.py::_conv_case runs it: the 7 x 1 / 1 x 7 layers without an activation."""
    return 0 if sorted(case[2:4]) == [1, 7] else 1


def case_plan(case, B=None):
    co, ci, kh, kw, s, pad, H, W, B0, xe, ye, res = case
    return plan(co, ci, kh, kw, s, pad, H, W, B or B0, res, case_leaky(case), _r(ci, 4) + xe, _r(co, 4) + ye)


def second_batch(case):
    """A batch size whose plan differs from the single image's; where the plan never changes with B, one that differs from 1."""
    for B in (5, 3, 2):
        if case_plan(case, B) != case_plan(case, 1):
            return B
    return case[8] if case[8] != 1 else 2


# (cout, cin, kh, kw, stride, pad, H, W, B, x lanes past roundup(cin, 4), y lanes past roundup(cout, 4), residual), plan.
# The smallest shapes of the grid's kind with Wo no multiple of the tile's 32 (16) columns and Ho no multiple of its rows; cout 30, 49,
# 90, 100, 101 and 190 (no multiple of 32; all but 100 none of 4) where the plan allows; a residual on every other v2 / v1 case.
TILE_CASES = [
    ((30, 3, 5, 5, 1, (2, 2), 5, 33, 1, 4, 4, True), (1, 4, 32, 309, 1)),
    ((2, 32, 3, 3, 1, (1, 1), 5, 33, 1, 4, 4, False), (1, 4, 32, 309, 2)),
    ((49, 49, 1, 7, 1, (0, 3), 5, 33, 1, 4, 4, True), (1, 4, 32, 309, 3)),
    ((30, 64, 3, 3, 1, (1, 1), 5, 33, 1, 4, 4, True), (1, 4, 32, 309, 4)),
    ((49, 128, 3, 3, 1, (1, 1), 97, 33, 1, 4, 4, True), (1, 4, 32, 309, 5)),
    ((49, 128, 3, 3, 1, (1, 1), 37, 97, 1, 4, 4, False), (1, 4, 32, 309, 6)),
    ((49, 128, 3, 3, 1, (1, 1), 67, 33, 1, 4, 4, True), (1, 4, 32, 309, 7)),
    ((49, 128, 3, 3, 1, (1, 1), 5, 33, 1, 4, 4, False), (1, 4, 32, 309, 8)),
    ((30, 3, 5, 5, 2, (2, 2), 5, 33, 1, 4, 4, True), (1, 4, 32, 913, 1)),
    ((2, 32, 3, 3, 2, (1, 1), 5, 33, 1, 4, 4, False), (1, 4, 32, 913, 2)),
    ((49, 49, 1, 7, 2, (0, 3), 5, 33, 1, 4, 4, True), (1, 4, 32, 913, 3)),
    ((30, 64, 3, 3, 2, (1, 1), 5, 33, 1, 4, 4, True), (1, 4, 32, 913, 4)),
    ((190, 128, 3, 3, 2, (1, 1), 57, 67, 1, 4, 4, True), (1, 4, 32, 913, 5)),
    ((49, 128, 3, 3, 2, (1, 1), 301, 33, 1, 4, 4, False), (1, 4, 32, 913, 6)),
    ((49, 128, 3, 3, 2, (1, 1), 259, 33, 1, 4, 4, True), (1, 4, 32, 913, 7)),
    ((49, 128, 3, 3, 2, (1, 1), 5, 33, 1, 4, 4, False), (1, 4, 32, 913, 8)),
    ((49, 32, 1, 1, 1, (0, 0), 515, 33, 1, 4, 4, True), (1, 4, 64, 309, 1)),
    ((49, 32, 1, 1, 1, (0, 0), 41, 131, 5, 4, 4, False), (1, 4, 64, 309, 2)),
    ((100, 49, 3, 3, 1, (1, 1), 57, 33, 5, 4, 4, True), (1, 4, 64, 309, 3)),
    ((190, 128, 3, 3, 1, (1, 1), 33, 33, 5, 4, 4, False), (1, 4, 64, 309, 4)),
    ((49, 32, 1, 1, 2, (0, 0), 515, 67, 2, 4, 4, True), (1, 4, 64, 913, 1)),
    ((49, 32, 1, 1, 2, (0, 0), 41, 515, 5, 4, 4, False), (1, 4, 64, 913, 2)),
    ((100, 49, 3, 3, 2, (1, 1), 97, 67, 5, 4, 4, True), (1, 4, 64, 913, 3)),
    ((90, 32, 1, 1, 1, (0, 0), 515, 33, 1, 4, 4, False), (1, 4, 96, 309, 1)),
    ((90, 32, 1, 1, 2, (0, 0), 515, 67, 2, 4, 4, True), (1, 4, 96, 913, 1)),
    ((101, 32, 1, 1, 1, (0, 0), 515, 33, 1, 4, 4, False), (1, 4, 128, 309, 1)),
    ((100, 32, 1, 1, 2, (0, 0), 515, 67, 2, 4, 4, True), (1, 4, 128, 913, 1)),
    ((2, 32, 3, 3, 1, (1, 1), 515, 33, 5, 4, 4, False), (1, 8, 32, 309, 1)),
    ((30, 32, 7, 1, 1, (3, 0), 515, 33, 5, 4, 4, True), (1, 8, 32, 505, 1)),
    ((2, 32, 3, 3, 2, (1, 1), 301, 515, 3, 4, 4, True), (1, 8, 32, 913, 1)),
    ((49, 32, 1, 1, 1, (0, 0), 515, 33, 5, 4, 4, True), (1, 8, 64, 309, 1)),
    ((49, 32, 7, 1, 1, (3, 0), 515, 33, 5, 4, 4, False), (1, 8, 64, 505, 1)),
    ((49, 32, 1, 1, 2, (0, 0), 301, 515, 3, 4, 4, True), (1, 8, 64, 913, 1)),
    ((90, 32, 1, 1, 1, (0, 0), 515, 33, 5, 4, 4, False), (1, 8, 96, 309, 1)),
    ((100, 32, 1, 1, 1, (0, 0), 515, 33, 5, 4, 4, True), (1, 8, 128, 309, 1)),
    ((49, 32, 1, 1, 1, (0, 0), 301, 259, 3, 4, 4, False), (1, 16, 64, 505, 1)),
    ((30, 32, 9, 7, 2, (4, 3), 5, 33, 1, 4, 4, True), (2, 4, 32, 0, 1)),
    ((49, 32, 7, 7, 1, (3, 3), 515, 33, 1, 4, 4, False), (2, 4, 64, 0, 1)),
    ((90, 32, 5, 5, 1, (2, 2), 515, 33, 1, 4, 4, True), (2, 4, 96, 0, 1)),
    ((101, 32, 3, 5, 1, (1, 2), 515, 33, 1, 4, 4, False), (2, 4, 128, 0, 1)),
    ((2, 32, 5, 5, 2, (2, 2), 301, 515, 3, 4, 4, True), (2, 8, 32, 0, 1)),
    ((49, 32, 7, 1, 2, (3, 0), 301, 515, 3, 4, 0, False), (2, 8, 64, 0, 1)),
    ((190, 32, 5, 5, 1, (2, 2), 515, 33, 2, 4, 4, True), (2, 8, 96, 0, 1)),
    ((100, 32, 3, 5, 1, (1, 2), 515, 33, 5, 4, 4, False), (2, 8, 128, 0, 1)),
    ((30, 3, 5, 5, 1, (2, 2), 301, 259, 3, 4, 4, False), (3, 8, 32, 0, 1)),
    ((30, 3, 7, 7, 1, (3, 3), 259, 515, 1, 4, 4, False), (4, 8, 32, 0, 1)),
    ((2, 32, 3, 3, 2, (1, 1), 259, 515, 1, 4, 4, False), (5, 8, 32, 0, 1)),
    ((49, 32, 3, 3, 2, (1, 1), 259, 515, 1, 4, 4, False), (5, 8, 64, 0, 1)),
    ((49, 32, 7, 1, 1, (3, 0), 259, 259, 1, 4, 0, False), (6, 16, 64, 0, 1)),
    ((49, 49, 1, 7, 1, (0, 3), 259, 259, 1, 4, 0, False), (7, 16, 64, 0, 1)),
    # refused before at these batch sizes (the 64- / 128-channel tile v2 wants has too large a weight slab, and v1 takes no 4-channel
    # tail chunk / does not fit the LDS): now on v2's 32-channel tile
    ((49, 3, 7, 7, 1, (3, 3), 515, 33, 2, 4, 4, False), (1, 4, 32, 913, 1)),
    ((100, 32, 7, 7, 1, (3, 3), 259, 33, 2, 4, 4, True), (1, 4, 32, 913, 1)),
    # a 4-channel tail chunk of 55 taps: no v2 tile holds its weight slab, conv_k1 takes it at any tile count (here 4 tiles)
    ((49, 3, 5, 11, 1, (2, 5), 13, 37, 1, 4, 4, False), (3, 8, 32, 0, 1)),
    # 128 <- 128 at B = 3: eight shares of three images exceed the handle's scratch, so the batch runs image by image
    ((128, 128, 3, 3, 1, (1, 1), 45, 31, 3, 4, 4, True), (1, 4, 32, 309, 8)),
]


# ---- the grid -------------------------------------------------------------------------------------------------------------------
NET_LAYERS = [   # cout, cin, kh, kw of LiteFlowNet / LiteFlowNet2 (multi-source layers by their channel sum)
    (32, 3, 7, 7), (32, 32, 3, 3), (64, 32, 3, 3), (64, 64, 3, 3), (96, 64, 3, 3), (96, 96, 3, 3), (128, 96, 3, 3), (192, 128, 3, 3),
    (64, 32, 1, 1), (128, 32, 1, 1), (128, 64, 1, 1), (128, 96, 1, 1),
    (128, 49, 3, 3), (128, 128, 3, 3), (96, 128, 3, 3), (64, 128, 3, 3), (64, 96, 3, 3), (32, 64, 3, 3),
    (2, 32, 3, 3), (2, 32, 5, 5), (2, 32, 7, 7), (128, 130, 3, 3), (128, 386, 3, 3), (128, 131, 3, 3),
    (49, 32, 7, 1), (49, 49, 1, 7), (25, 32, 5, 1), (25, 25, 1, 5), (9, 32, 3, 3)]
WIDE_LAYERS = [(co, ci, kh, kw) for co in (32, 64, 96, 128, 192) for ci in (3, 4, 32) for (kh, kw) in ((5, 5), (3, 5), (7, 7))]
# layers outside the network: for the instantiations nothing above reaches, v2 <2,1,5,5> (a 7 x 1 layer of 32 outputs) and v1 <1,1>
# (more than 52 taps); and a 4-channel tail chunk of more than 52 taps, which conv_k1 alone takes
REST_LAYERS = [(32, 32, 7, 1), (32, 32, 9, 7), (64, 3, 5, 11)]
SIZES = (1, 2, 5, 8, 33, 41, 57, 67, 97, 130, 259, 300, 515)


def _grid():
    for (co, ci, kh, kw) in NET_LAYERS + WIDE_LAYERS + REST_LAYERS:
        # a residual or an activation changes the choice only where a kernel without them exists
        special = ci in (3, 4) or (ci == 32 and (kh, kw) == (3, 3)) or sorted((kh, kw)) == [1, 7]
        modes = ((False, 0), (False, 1), (True, 1)) if sorted((kh, kw)) == [1, 7] else ((False, 1), (True, 1)) if special else ((False, 1),)
        for s in (1, 2):
            for H in SIZES:
                for W in SIZES:
                    for res, leaky in modes:
                        yield (co, ci, kh, kw, s, (kh // 2, kw // 2), H, W), res, leaky


@pytest.fixture(scope="module")
def sweep():
    """{geometry: [plan at each of BATCHES]} over the grid."""
    return {(g, res, leaky): [plan(*g, B, res, leaky) for B in BATCHES] for g, res, leaky in _grid()}


# every kernel launch_conv can launch: (family, rows, channels, staging class).  The library's own list is the take_nt2 / take_nt4
# mappings and choose_conv1 of csrc/conv_mfma.hip and the launchers of conv_k1.hip, conv_c3k7.hip and conv_s2.hip (COL7 / ROW7: conv_layer.hip); a kernel
# added or retired there shows here as a plan the grid reaches outside this set, or no longer reaches
COMPILED = ({(V2, 16, 64, 505)}
            | {(V2, 8, 32 * nt, 309) for nt in (1, 2, 3, 4)} | {(V2, 8, 32 * nt, c) for nt in (1, 2) for c in (505, 913)}
            | {(V2, 4, 32 * nt, c) for nt in (1, 2, 3, 4) for c in (309, 913)}
            | {(V1, 4 * mt, 32 * nt, 0) for mt in (1, 2) for nt in (1, 2, 3, 4)}
            | {(K1, 8, 32, 0), (C3K7, 8, 32, 0), (S2, 8, 32, 0), (S2, 8, 64, 0), (COL7, 16, 64, 0), (ROW7, 16, 64, 0)})


@pytest.mark.parametrize("case,want", TILE_CASES, ids=lambda v: "-".join(str(x) for x in v).replace(" ", "") if isinstance(v, tuple) else None)
def test_tile_case_reaches_its_plan(case, want):
    assert case_plan(case) == want, POLICY


def test_tile_cases_have_ragged_edges_and_wide_strides():
    for case, want in TILE_CASES:
        co, ci, kh, kw, s, pad, H, W, B, xe, ye, res = case
        Ho, Wo = (H + 2 * pad[0] - kh) // s + 1, (W + 2 * pad[1] - kw) // s + 1
        cols = 16 if want[0] in (S2, COL7, ROW7) else 32
        assert Wo % cols and Ho % want[1], case
        assert xe > 0 and (ye > 0 or want[0] in (COL7, ROW7) or sorted((kh, kw)) == [1, 7]), case      # the streaming kernels: 52 lanes
    for family in (V2, V1):                                  # per N tile, a cout that leaves the last channel block (and quad) ragged
        for chans in (32, 64, 96, 128):
            assert any(w[0] == family and w[2] == chans and c[0] % 32 for c, w in TILE_CASES), (family, chans)
            assert any(w[0] == family and w[2] == chans and c[0] % 4 for c, w in TILE_CASES), (family, chans)
    assert any(c[0] == 30 and c[11] for c, w in TILE_CASES) and any(c[0] == 49 for c, w in TILE_CASES) and any(c[0] == 100 for c, w in TILE_CASES)
    assert {w[4] for c, w in TILE_CASES} == set(range(1, 9))             # every split-K factor


def test_grid_reaches_exactly_the_plans_with_a_case(sweep):
    reached = {p for plans in sweep.values() for p in plans if p is not None}
    cased = {want for _, want in TILE_CASES}
    assert reached == cased, (f"{POLICY}: plans without a case {sorted(reached - cased)}, cases whose plan the grid no longer reaches "
                              f"{sorted(cased - reached)}")


def test_grid_reaches_every_compiled_kernel(sweep):
    reached = {p[:4] for plans in sweep.values() for p in plans if p is not None}
    assert reached == COMPILED, (sorted(reached - COMPILED), sorted(COMPILED - reached))


def test_acceptance_does_not_depend_on_the_batch(sweep):
    """A geometry is accepted at every B or at none (a layer with a 4-channel tail chunk, or one whose v1 tile does not fit the LDS,
    falls to a narrower v2 tile instead of being refused at the batch sizes that want a wide one; a tail chunk of more than 52 taps
    runs on conv_k1 at any tile count, not only from 1024 tiles up)."""
    bad = [(g, plans) for g, plans in sweep.items() if len({p is None for p in plans}) > 1]
    assert not bad, bad[:5]
    for co, ci in ((64, 3), (100, 3), (160, 4), (192, 3), (256, 4)):
        assert all(plan(co, ci, 5, 11, 1, (0, 0), 1030, 64, B) is not None for B in BATCHES + (4, 8)), (co, ci)
    # wide pixel strides: beyond v2's 2 GiB descriptor range per patch, where conv_k1 and the whole-line stride-2 kernel still apply
    for g in ((32, 3, 7, 7, 1, (3, 3), 40, 3000), (32, 3, 5, 5, 1, (2, 2), 300, 3000), (64, 32, 3, 3, 2, (1, 1), 300, 2500),
              (64, 32, 3, 3, 1, (1, 1), 300, 2500)):
        assert len({plan(*g, B, xs=8192) is None for B in BATCHES + (8, 64)}) == 1, g
    assert plan(64, 3, 7, 7, 1, (3, 3), 512, 1, 1) is not None and plan(64, 3, 7, 7, 1, (3, 3), 512, 1, 2) is not None
    assert plan(128, 32, 7, 7, 1, (3, 3), 8, 8, 1) is not None and plan(128, 32, 7, 7, 1, (3, 3), 512, 1, 2) is not None


def test_split_k_shares_do_not_depend_on_the_batch(sweep):
    """One image's split-K shares, hence its summation order, are the same at every B: pivlfn_forward's factor for that image."""
    bad = [(g, plans) for g, plans in sweep.items() if len({p[4] for p in plans if p is not None}) > 1]
    assert not bad, bad[:5]
    for B in (1, 2, 3, 5, 16):                               # 128 <- 128 at 44 x 32: eight shares of three images exceed the scratch
        assert plan(128, 128, 3, 3, 1, (1, 1), 44, 32, B)[4] == 8, B


def test_plan_refuses_what_the_layer_call_refuses():
    lib = _lib.load()
    out = (ctypes.c_int * 5)()
    for args in [(32, 32, 3, 3, 1, 8, 8, 1, 1, 1, 0, 1, 30, 32),        # x_stride no multiple of 4
                 (32, 32, 3, 3, 1, 8, 8, 1, 1, 1, 0, 1, 32, 28),        # y_stride < cout
                 (32, 32, 3, 3, 1, 1, 1, 1, 0, 0, 0, 1, 32, 32),        # the kernel does not fit the padded image
                 (32, 32, 3, 3, 0, 8, 8, 1, 1, 1, 0, 1, 32, 32),        # B = 0
                 (32, 3, 9, 9, 2, 64, 64, 1, 4, 4, 0, 1, 4, 32)]:       # 81 taps on a 4-channel tail chunk: no kernel
        assert lib.pivlfn_conv2d_nhwc_plan(*args, out) == 1, args
        assert lib.pivlfn_last_error()
    assert lib.pivlfn_conv2d_nhwc_plan(32, 32, 3, 3, 1, 8, 8, 1, 1, 1, 0, 1, 32, 32, None) == 1
