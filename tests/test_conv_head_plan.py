"""The flow head's launcher, asked on the host which kernel it picks (pivlfn_conv_head_nhwc_plan; no GPU needed).

launch_head_t (csrc/conv_head.hip) picks one of four kernels for the 32 -> 2 channel k x k head, from the size of one image alone:
  PIXEL_LDS  conv_head_kernel<k, true>     at most 512 tiles of 16 x 16, and none of the rows below
  PIXEL      conv_head_kernel<k, false>    more than 512 tiles, H * W < 512 * 512
  ROWS4      conv_head4_kernel<k>          H * W >= 512 * 512 (k = 7: only where MFMA does not apply)
  MFMA       conv_head_mfma_kernel<7, 8>   k = 7, H * W >= 256 * 256, H * W * 128 bytes < 2^31
HEAD_CASES holds the shapes tests/test_gpu_conv_head.py runs against float64 and exact integers.  Here, on the plan function alone:
  * every case still reaches the family it was chosen for, and every one of the ten reachable (k, family) pairs has a case;
  * the family never depends on the batch;
  * each boundary of the policy lies where the table above says, seen from both sides;
  * which family each level of a pair of a given size runs (printed; a 2048 x 2048 pair's level 3 runs ROWS4)."""
import ctypes

import pytest

from pivlfn import _lib

PIXEL_LDS, PIXEL, ROWS4, MFMA = 1, 2, 3, 4                      # PIVLFN_HEAD_PLAN_* of include/pivlfn.h
NAMES = {PIXEL_LDS: "PIXEL_LDS", PIXEL: "PIXEL", ROWS4: "ROWS4", MFMA: "MFMA"}
TILE = {PIXEL_LDS: (16, 16), PIXEL: (16, 16), ROWS4: (32, 32), MFMA: (8, 58)}      # output rows, columns of one workgroup
POLICY = "the launcher's policy changed: re-derive the shapes of this test"
REACHABLE = {(k, f) for k in (3, 5, 7) for f in (PIXEL_LDS, PIXEL, ROWS4)} | {(7, MFMA)}
K_LEVEL = {1: 7, 2: 7, 3: 5, 4: 5, 5: 3, 6: 3}                  # the head's k at each pyramid level (csrc/net.h)
# the products of H and W, and the counts of 16 x 16 tiles, on either side of which the family changes
PIXEL_BOUNDS = (256 * 256 - 1, 256 * 256, 512 * 512 - 1, 512 * 512, 4096 * 4096 - 1, 4096 * 4096)


def plan(k, B, H, W):
    """(family, tile rows, tile columns, workgroups), or None where pivlfn_conv_head_nhwc refuses the geometry."""
    out = (ctypes.c_int * 4)()
    rc = _lib.load().pivlfn_conv_head_nhwc_plan(k, B, H, W, out)
    assert rc in (0, 1), rc
    return tuple(out) if rc == 0 else None


def family(k, B, H, W):
    return plan(k, B, H, W)[0]


def is_2gib(case):
    """The cases whose input is 2 GiB or more (one byte less for 4095 x 4097): x is made on the device, the reference on bands."""
    k, B, H, W, fam = case
    return H * W * 128 >= 2 ** 31 - 128


# (k, B, H, W, family).  The smallest shapes found that land in the family with ragged right and bottom tiles, the shapes exactly on
# each bound and their neighbours across it, and images with fewer rows or columns than a tile or than the k // 2 halo.
HEAD_CASES = (
    [(k, B, H, W, PIXEL_LDS) for k in (3, 5, 7) for (B, H, W) in ((1, 16, 16), (2, 37, 53), (1, 3, 70), (1, 1, 1), (1, 1, 17))] + [
        (5, 1, 352, 368, PIXEL_LDS),        # 506 tiles: the neighbour of 353 x 368 below
        (7, 1, 255, 257, PIXEL_LDS),        # 65535 pixels: one short of MFMA
        # PIXEL: more than 512 tiles and fewer than 512 * 512 pixels
        (3, 1, 3, 8200, PIXEL),             # 513 tiles in one tile row
        (3, 1, 368, 370, PIXEL),            # 552 tiles
        (5, 1, 17, 4107, PIXEL),            # 514 tiles in two rows, the second of one image row
        (5, 1, 353, 368, PIXEL),            # 529 tiles
        (5, 1, 511, 513, PIXEL),            # 262143 pixels: one short of ROWS4
        (7, 1, 7, 8195, PIXEL),             # k = 7 leaves PIXEL fewer than 65536 pixels: one tile row only
        # ROWS4
        (3, 1, 509, 517, ROWS4),
        (3, 1, 512, 512, ROWS4),            # exactly on the bound
        (5, 1, 5, 52431, ROWS4),            # fewer rows than one lane's four, 1639 tiles
        (5, 1, 52431, 5, ROWS4),
        (7, 1, 4096, 4096, ROWS4),          # k = 7: from 2^31 bytes of input, where MFMA's 32-bit offsets end
        # MFMA (k = 7)
        (7, 1, 1, 65536, MFMA),             # fewer rows than the 8-row tile and than the 3-row halo; exactly on the bound
        (7, 1, 65537, 1, MFMA),             # one column: every strip is halo but one lane
        (7, 1, 5, 13109, MFMA),
        (7, 3, 250, 263, MFMA),             # H % 8 == 2, W % 58 == 31
        (7, 1, 256, 256, MFMA),             # exactly on the bound
        (7, 1, 4095, 4097, MFMA),           # 16777215 pixels: the last image below the 2 GiB bound
    ])
# what tests/test_gpu_conv.py::test_flow_head_kernel_matches_torch and tests/test_gpu_guarded.py::test_flow_head_guarded ran before
# HEAD_CASES existed: PIXEL_LDS for every k and MFMA, nothing else
OLD_SHAPES = [(k, B, H, W) for k in (3, 5, 7) for (B, H, W) in ((1, 16, 16), (2, 37, 53), (1, 3, 70))] + [(7, 1, 256, 300), (7, 2, 260, 257)]


def signature(case):
    """What a case exercises: the kernel, then per axis whether the image has one tile or more, ends on a tile edge, and is one
    pixel / at most the halo / more than the halo wide; whether there is a batch; whether it sits next to a bound of the policy."""
    k, B, H, W, fam = case
    rows, cols = TILE[fam]

    def axis(n, t):
        return (min(-(-n // t), 2), n % t == 0, 0 if n == 1 else 1 if n <= k // 2 else 2)
    tiles16 = -(-H // 16) * -(-W // 16)
    return (k, fam, B > 1, axis(H, rows), axis(W, cols), H * W in PIXEL_BOUNDS or tiles16 in (512, 513))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: f"k{c[0]}-B{c[1]}-{c[2]}x{c[3]}-{NAMES[c[4]]}")
def test_case_reaches_its_family(case):
    k, B, H, W, fam = case
    p = plan(k, B, H, W)
    rows, cols = TILE[fam]
    assert p == (fam, rows, cols, -(-H // rows) * -(-W // cols) * B), POLICY


def test_cases_cover_every_reachable_family():
    covered = {(c[0], c[4]) for c in HEAD_CASES}
    print(f"\n(k, family) pairs covered by HEAD_CASES: {len(covered)}")
    assert covered == REACHABLE, (sorted(REACHABLE - covered), sorted(covered - REACHABLE))
    old = {(k, family(k, B, H, W)) for k, B, H, W in OLD_SHAPES}
    assert old == {(3, PIXEL_LDS), (5, PIXEL_LDS), (7, PIXEL_LDS), (7, MFMA)}       # what the suite launched before


def test_every_case_is_needed():
    """Without any one case, something it exercises (signature) has no case."""
    sigs = [signature(c) for c in HEAD_CASES]
    for i, c in enumerate(HEAD_CASES):
        assert sigs[i] not in sigs[:i] + sigs[i + 1:], f"the case {c} adds nothing to the others"


def test_cases_have_ragged_edges_and_ragged_grids():
    for fam in (PIXEL_LDS, PIXEL, ROWS4, MFMA):
        rows, cols = TILE[fam]
        mine = [c for c in HEAD_CASES if c[4] == fam]
        # xcd_remap's ragged branch: a workgroup count that is no multiple of the 8 XCDs
        assert any(plan(*c[:4])[3] % 8 for c in mine), NAMES[fam]
        # more than one tile along both axes and the last tile ragged on both
        assert any(H > rows and W > cols and H % rows and W % cols for (k, B, H, W, f) in mine), NAMES[fam]
    # the only images of 2 GiB: the two on either side of the bound where k = 7 leaves the matrix-core kernel
    assert [c[:4] for c in HEAD_CASES if is_2gib(c)] == [(7, 1, 4096, 4096), (7, 1, 4095, 4097)]


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------
SIZES = (1, 3, 5, 7, 15, 17, 37, 53, 70, 250, 255, 256, 257, 263, 300, 352, 353, 368, 370, 509, 511, 512, 513, 517, 1024, 2047, 2048,
         4095, 4096, 4097, 8191, 8192, 8193, 8195, 8200, 13109, 52431, 65535, 65536, 65537, 262143, 262144, 16777215, 16777216)
BATCHES = tuple(range(1, 65))


@pytest.fixture(scope="module")
def sweep():
    """{(k, H, W): [family at each of BATCHES]} over the grid; images of more than 2^25 pixels are left out (the 16777216-pixel
    bound is the last one)."""
    return {(k, H, W): [family(k, B, H, W) for B in BATCHES]
            for k in (3, 5, 7) for H in SIZES for W in SIZES if H * W <= 2 ** 25}


def test_family_does_not_depend_on_the_batch(sweep):
    bad = [(g, sorted(set(f))) for g, f in sweep.items() if len(set(f)) > 1]
    assert not bad, bad[:5]
    for k in (3, 5, 7):                              # thin shapes on either side of every bound are in the grid
        for H, W in ((1, 65535), (1, 65536), (3, 8192), (3, 8195), (262143, 1), (262144, 1), (1, 16777215), (16777216, 1), (17, 512)):
            assert (k, H, W) in sweep


def test_sweep_reaches_exactly_the_ten_reachable_families(sweep):
    reached = {(k, f[0]) for (k, H, W), f in sweep.items()}
    print(f"\n(k, family) pairs reached by the sweep: {len(reached)}")
    assert reached == REACHABLE, (sorted(REACHABLE - reached), sorted(reached - REACHABLE))
    assert len(reached) == 10


def test_boundaries_from_both_sides():
    for k in (3, 5, 7):
        # 512 against 513 tiles of 16 x 16
        assert family(k, 1, 3, 8192) == PIXEL_LDS and family(k, 1, 3, 8193) == PIXEL, POLICY
        if k != 7:                                   # two tile rows of 16 x 16 at this count: 65536 pixels and more, MFMA's for k = 7
            assert family(k, 1, 16, 8192) == PIXEL_LDS and family(k, 1, 17, 4096) == PIXEL_LDS and family(k, 1, 17, 4097) == PIXEL, POLICY
    # k = 7: H * W = 65535 against 65536
    for (H, W), (H2, W2) in (((255, 257), (256, 256)), ((1, 65535), (1, 65536)), ((65535, 1), (65536, 1)), ((3, 21845), (2, 32768))):
        assert H * W == 65535 and H2 * W2 == 65536
        assert family(7, 1, H, W) in (PIXEL_LDS, PIXEL) and family(7, 1, H2, W2) == MFMA, POLICY
        assert family(3, 1, H, W) == family(3, 1, H2, W2) and family(5, 1, H, W) == family(5, 1, H2, W2)      # no bound for k = 3, 5
    # H * W = 262143 against 262144
    for (H, W), (H2, W2) in (((511, 513), (512, 512)), ((1, 262143), (1, 262144)), ((262143, 1), (262144, 1)), ((87381, 3), (65536, 4))):
        assert H * W == 262143 and H2 * W2 == 262144
        for k in (3, 5):
            assert family(k, 1, H, W) == PIXEL and family(k, 1, H2, W2) == ROWS4, POLICY
        assert family(7, 1, H, W) == MFMA and family(7, 1, H2, W2) == MFMA, POLICY
    # k = 7: H * W = 16777215 against 16777216 (2^31 bytes of input)
    for (H, W), (H2, W2) in (((4095, 4097), (4096, 4096)), ((1, 16777215), (1, 16777216)), ((16777215, 1), (16777216, 1)), ((5, 3355443), (32, 524288))):
        assert H * W == 16777215 and H2 * W2 == 16777216
        assert family(7, 1, H, W) == MFMA and family(7, 1, H2, W2) == ROWS4, POLICY
        assert family(3, 1, H, W) == ROWS4 and family(5, 1, H2, W2) == ROWS4
    assert family(5, 1, 352, 368) == PIXEL_LDS and family(5, 1, 353, 368) == PIXEL, POLICY       # 506 against 529 tiles


def test_families_of_the_pyramid_levels():
    """Which kernel the heads of a pair of N x N pixels run: level L holds N / 2^(L-1) pixels a side; the piv model's lowest level is
    1, the others' 2 or 3 (pivlfn/synth.py MODEL_CFG), so a model runs its lowest level's column and everything right of it."""
    table = {N: [family(K_LEVEL[L], 1, N >> (L - 1), N >> (L - 1)) for L in range(1, 7)] for N in (256, 512, 1024, 2048, 4096)}
    print("\n  pair      " + "".join(f"L{L} (k={K_LEVEL[L]})".ljust(12) for L in range(1, 7)))
    for N, row in table.items():
        print(f"  {N:4d}^2    " + "".join(NAMES[f].ljust(12) for f in row))
    assert table[2048][2] == ROWS4 and K_LEVEL[3] == 5, POLICY      # no test launched ROWS4 before tests/test_gpu_conv_head.py
    assert table[2048] == [MFMA, MFMA, ROWS4, PIXEL_LDS, PIXEL_LDS, PIXEL_LDS], POLICY
    assert table[4096] == [ROWS4, MFMA, ROWS4, ROWS4, PIXEL_LDS, PIXEL_LDS], POLICY
    assert table[1024] == [MFMA, MFMA, PIXEL_LDS, PIXEL_LDS, PIXEL_LDS, PIXEL_LDS], POLICY
    # PIXEL: level 3 of pairs between about 1450 and 2048 pixels a side
    assert family(5, 1, 1456 >> 2, 1456 >> 2) == PIXEL and family(5, 1, 2044 >> 2, 2044 >> 2) == PIXEL and family(5, 1, 1408 >> 2, 1408 >> 2) == PIXEL_LDS


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_plan_refuses_what_the_entry_point_refuses():
    lib = _lib.load()
    out = (ctypes.c_int * 4)()

    def refused(args, *words):
        assert lib.pivlfn_conv_head_nhwc_plan(*args, out) == 1, args
        msg = lib.pivlfn_last_error().decode()
        for w in words:
            assert w in msg, (args, w, msg)

    for k in (-3, 0, 1, 2, 4, 6, 8, 9):
        refused((k, 1, 16, 16), "conv_head", f"k={k} unsupported")
    for B, H, W in ((0, 16, 16), (1, 0, 16), (1, 16, 0), (-1, 16, 16), (1, -16, 16), (1, 16, -16)):
        refused((7, B, H, W), "conv_head: bad arguments")
    refused((3, 2 ** 31 - 1, 4096, 4096), "conv_head", "workgroups")      # a grid of 2^31 workgroups or more
    assert lib.pivlfn_conv_head_nhwc_plan(7, 1, 16, 16, None) == 1
    assert b"conv_head_plan" in lib.pivlfn_last_error()
    assert lib.pivlfn_conv_head_nhwc_plan(7, 1, 16, 16, out) == 0 and tuple(out) == (PIXEL_LDS, 16, 16, 1)
