"""The launchers of the fp16, split, Winograd and split-bf16 Winograd convolutions, asked on the host which kernel they pick
(pivlfn_conv2d_nhwc_kernel_plan; no GPU needed).

launch_conv_h, launch_conv_x, launch_conv_w and launch_conv_wb each choose one compiled instantiation per call, from the layer geometry
and from the batch.  The *_CASES lists hold one layer and shape for every plan of theirs; tests/test_gpu_conv_kernel_tiles.py runs each
against float64 between guard pages.  Here, on the plan function alone:
  * every case still reaches the plan it was chosen for;
  * the instantiations a launcher can name are read out of its .hip text; a grid of network layers and a few outside ones reaches exactly
    those the production library can reach, and the cases reach every one of them: an instantiation added later without a case fails here;
  * the instantiations only a tools-build knob reaches are exactly TOOLS_ONLY;
  * every case has a ragged right and bottom edge, every tile width a cout that leaves the last channel block and the last quad ragged;
  * acceptance, the split-K shares and -- for split layers with a folded tail -- the choice between the big and the small kernel never
    depend on the batch;
  * conv_wino_b3_kernel's partition of the tiles over its persistent workgroups, restated, takes every tile exactly once, and its stepping
    of (channel group, tile column, tile row, image) by increments with carries arrives at the tiles the partition names.

The instantiations and the case that reaches each (cout <- cin, kh x kw, B x H x W; s2 = stride 2):

  conv_split.hip  launch_x<3,1,2,5,3,2>    49 <- 20, 3 x 3, s2, 1 x 37 x 45          stride 2, 64 channels
                  launch_x<3,1,1,5,2,2>    30 <- 20, 3 x 3, s2, 2 x 37 x 45          stride 2, 32 channels; image by image
                  launch_x<3,1,2,2,3,4>    49 <- 36, 3 x 3, 2 x 37 x 45              small grid, 64 channels; 3 shares, image by image
                                           49 <- 68, 1 x 1, 3 x 37 x 45              5 shares
                                           101 <- 130, 3 x 3, 1 x 13 x 37            8 shares, two channel blocks
                  launch_x<3,1,1,2,2,4>    30 <- 100, 3 x 3, 1 x 21 x 45             small grid, 32 channels; 7 shares
                                           30 <- 96, 3 x 3, 1 x 13 x 37              6 shares
                  launch_x<3,2,4,3,6,2>    101 <- 36, 3 x 3, 1 x 515 x 520           128-channel tiles; the small kernel's zero-padded tail chunk
                  launch_x<3,4,2,5,3,2>    49 <- 32, 3 x 3, 2 x 515 x 520            16 rows x 64 channels (one image: launch_x<3,2,2,3,3,3>)
                  launch_x<3,2,2,3,3,3>    49 <- 64, 3 x 3, 1 x 260 x 515
                  launch_x<3,2,2,5,3,2>    49 <- 32, 7 x 1, 1 x 37 x 45              tall patch, 64 channels; 2 shares
                  launch_x<3,2,2,5,7,2>    49 <- 49, 1 x 7, 1 x 37 x 45              wide rows, 64 channels; 4 shares
                  launch_x<3,2,1,3,2,3>    30 <- 32, 3 x 3, 1 x 260 x 515
                  launch_x<3,2,1,5,2,2>    25 <- 32, 7 x 1, 1 x 37 x 45              tall patch, 32 channels; 2 shares
                  launch_x<3,2,1,5,4,2>    25 <- 25, 1 x 5, 1 x 37 x 45              wide rows, 32 channels; 2 shares
                  launch_x<6,2,2,3,5,2>    49 <- 36, 3 x 3, 2 x 37 x 45              six terms never split; the handle still runs the batch
                                                                                     image by image
                  launch_x<6,2,2,5,5,2>    49 <- 32, 7 x 1, 1 x 37 x 45
                  launch_x<6,2,2,5,11,2>   49 <- 49, 1 x 7, 1 x 37 x 45
                  launch_x<6,2,1,3,3,2>    30 <- 20, 3 x 3, 1 x 37 x 45
                  launch_x<6,2,1,5,3,2>    25 <- 32, 7 x 1, 1 x 37 x 45
                  launch_x<6,2,1,5,6,2>    25 <- 25, 1 x 5, 1 x 37 x 45
                  launch_xbig<4>           101 <- 52, 3 x 3, 1 x 515 x 520           folded tail at the fewest K chunks it takes
                                           128 <- 96, 3 x 3, 1 x 515 x 520           no tail
                  launch_xbig<2>           49 <- 100, 3 x 3, 1 x 515 x 520           folded tail
                                           64 <- 96, 3 x 3, 1 x 515 x 520            no tail
  conv_f16.hip    launch_h<4,4,5,9>        101 <- 20, 3 x 3, 2 x 99 x 450            16 rows: from 192 tiles of them (one image: launch_h<2,4,5,9>)
                  launch_h<2,4,5,9>        101 <- 49, 3 x 3, 1 x 33 x 47
                  launch_h<2,2,5,9>        49 <- 36, 3 x 3, 2 x 37 x 45
                  launch_h<4,1,5,9>        30 <- 20, 3 x 3, 2 x 99 x 450             (one image: launch_h<2,1,5,9>)
                  launch_h<2,1,5,9>        30 <- 20, 1 x 1, 1 x 37 x 45
                  launch_h<2,4,9,13>       128 <- 96, 3 x 3, s2, 1 x 67 x 45         NetC's 96 -> 128 stride-2 layer
                  launch_h<2,2,9,13>       49 <- 20, 3 x 3, s2, 1 x 67 x 45
                  launch_h<2,1,9,13>       30 <- 3, 7 x 7, 1 x 37 x 45
                  launch_h<4,2,5,9>        tools build only (knob 1, bit 64)
  conv_wino.hip   launch_w<1,2>            49 <- 20, 2 x 67 x 250                    two channel blocks per wave: from 256 workgroups
                  launch_w<2,1>            30 <- 20, 2 x 259 x 250                   16 rows: from 512 tiles of them
                  launch_w<1,1>            30 <- 36, 3 x 37 x 29                     (and one image of the two above)
                  launch_w<2,2>, <1,4>     tools build only (knob 14)
  conv_wino_b3.hip  launch_b3<6>           101 <- 52, 2 x 37 x 45                    two channel groups, four K steps
                  launch_b3<8>, <9>        49 <- 20, 2 x 37 x 45
                  the persistent schedule  b3_schedule_cases, sized from the CU count (tests/test_gpu_conv_kernel_tiles.py asks the device,
                                           this file 8 ... 304)
"""
import ctypes
import os
import re

import pytest

from pivlfn import _lib
from test_conv_plan import BATCHES, NET_LAYERS, POLICY, _r

F16, SPLIT, SPLIT_BIG, WINO, WINO_B3 = 1, 2, 3, 4, 5            # PIVLFN_KERNEL_PLAN_* of include/pivlfn.h
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "piv_liteflownet-pytorch_amd", "csrc")
CUS = 256                                                       # the CU count the b3 plans of this file are asked for (an MI355X's)


def kplan(kernel, co, ci, kh, kw, s, pad, H, W, B, terms=0, x16=0, xs=None, ys=None, cus=CUS):
    """The ten plan values, or None where the entry point of that kernel refuses the geometry."""
    out = (ctypes.c_int * 10)()
    rc = _lib.load().pivlfn_conv2d_nhwc_kernel_plan(kernel, co, ci, kh, kw, B, H, W, s, pad[0], pad[1], terms, x16,
                                                    xs or _r(ci, 8 if x16 else 4), ys or _r(co, 4), cus, out)
    assert rc in (0, 1), rc
    return tuple(out) if rc == 0 else None


def inst(p):
    """The launcher instantiation a plan names, as the .hip text writes it."""
    kernel, terms, rows, chans, staging, occ = p[:6]
    if kernel == SPLIT:
        return ("launch_x", (terms, rows // 4, chans // 32, staging // 100, staging % 100, occ))
    if kernel == SPLIT_BIG:
        return ("launch_xbig", (chans // 32,))
    if kernel == F16:
        return ("launch_h", (rows // 4, chans // 32, staging // 100, staging % 100))
    if kernel == WINO:
        return ("launch_w", (rows // 8, chans // 32))
    assert kernel == WINO_B3, p
    return ("launch_b3", (terms,))


def case_plan(kernel, case, B=None, terms=0, x16=0, cus=CUS):
    """The plan of a case as tests/test_gpu_guarded.py::_conv_case runs it."""
    co, ci, kh, kw, s, pad, H, W, B0, xe, ye, _ = case
    return kplan(kernel, co, ci, kh, kw, s, pad, H, W, B or B0, terms, x16, _r(ci, 8 if x16 else 4) + xe, _r(co, 4) + ye, cus)


def second_batch(kernel, case, terms=0, x16=0, cus=CUS):
    """A batch size other than the case's whose plan differs from the single image's (in more than the workgroup count); where none
    does, any other."""
    one = case_plan(kernel, case, 1, terms, x16, cus)
    for B in (2, 3, 5):
        if B != case[8] and case_plan(kernel, case, B, terms, x16, cus)[:9] != one[:9]:
            return B
    return 2 if case[8] != 2 else 3


# ---- the instantiations, out of the sources --------------------------------------------------------------------------------------
SOURCES = {"conv_split.hip": ("launch_x", "launch_xbig"), "conv_f16.hip": ("launch_h",), "conv_wino.hip": ("launch_w",),
           "conv_wino_b3.hip": ("launch_b3",)}
# reached only through a knob of the tools build (PIV_KNOB is the constant 0 in the production library)
TOOLS_ONLY = {("launch_h", (4, 2, 5, 9)), ("launch_w", (2, 2)), ("launch_w", (1, 4))}


def instantiations(name):
    """(production, tools-only): every launch_*<...> the choice of csrc/<name> names.  Tools-only: all of its mentions stand inside an
    #ifdef PIVLFN_TOOLS block or on a line whose condition asks for a knob to be set (!(PIV_KNOB...) asks for it to be clear)."""
    prod, tools, in_tools = set(), set(), 0
    for line in open(os.path.join(CSRC, name)):
        code = line.split("//")[0]
        if re.match(r"\s*#\s*if", code):
            in_tools = in_tools + 1 if (in_tools or "PIVLFN_TOOLS" in code) else 0
        elif re.match(r"\s*#\s*endif", code) and in_tools:
            in_tools -= 1
        knob = re.search(r"(?<!!\()PIV_KNOB", code) is not None
        for fn, args in re.findall(r"\b(launch_(?:x|xbig|h|w|b3))<([0-9, ]+)>", code):
            assert fn in SOURCES[name], (name, fn)
            (tools if in_tools or knob else prod).add((fn, tuple(int(a) for a in args.split(","))))
    return prod, tools - prod


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# (cout, cin, kh, kw, stride, pad, H, W, B, x lanes past roundup(cin, 4 or 8), y lanes past roundup(cout, 4), no residual), ...
# The smallest shapes of their kind: 37 x 45 where the plan allows (two tile columns, Ho no multiple of 4, 8 or 16); the 8- and 16-row
# kernels of 3 x 3 layers only start at 512 tiles of 8 rows (the big kernels at 512, the 16-row and 128-channel tiles at 1024 of their
# own), so those run 260 x 515 or 515 x 520.  cout 25, 30, 49 and 101 leave the last channel block and the last quad ragged.
P0, P1 = (0, 0), (1, 1)
# ... terms, plan[:9]: kernel, terms, rows, channels, staging class, workgroups per CU, split-K shares, folded tail, image by image
SPLIT_CASES = [
    ((49, 20, 3, 3, 2, P1, 37, 45, 1, 4, 4, False), 3, (2, 3, 4, 64, 503, 2, 1, 0, 0)),          # stride 2
    ((30, 20, 3, 3, 2, P1, 37, 45, 2, 4, 4, False), 3, (2, 3, 4, 32, 502, 2, 1, 0, 1)),
    # small grids: 4-row tiles, split-K shares min(8, K chunks of 16 channels, 1024 / canonical tiles); a batch runs image by image.
    # 2 and 4 shares: the 7 x 1, 1 x 5 and 1 x 7 layers below
    ((49, 36, 3, 3, 1, P1, 37, 45, 2, 4, 4, False), 3, (2, 3, 4, 64, 203, 4, 3, 0, 1)),
    ((49, 68, 1, 1, 1, P0, 37, 45, 3, 4, 4, False), 3, (2, 3, 4, 64, 203, 4, 5, 0, 1)),
    ((30, 96, 3, 3, 1, P1, 13, 37, 1, 4, 4, False), 3, (2, 3, 4, 32, 202, 4, 6, 0, 0)),
    ((30, 100, 3, 3, 1, P1, 21, 45, 1, 4, 4, False), 3, (2, 3, 4, 32, 202, 4, 7, 0, 0)),
    ((101, 130, 3, 3, 1, P1, 13, 37, 1, 4, 4, False), 3, (2, 3, 4, 64, 203, 4, 8, 0, 0)),
    # 8- and 16-row tiles of the small kernel
    ((101, 36, 3, 3, 1, P1, 515, 520, 1, 4, 4, False), 3, (2, 3, 8, 128, 306, 2, 1, 0, 0)),      # its zero-padded tail chunk
    ((49, 32, 3, 3, 1, P1, 515, 520, 2, 4, 4, False), 3, (2, 3, 16, 64, 503, 2, 1, 0, 0)),
    ((49, 64, 3, 3, 1, P1, 260, 515, 1, 4, 4, False), 3, (2, 3, 8, 64, 303, 3, 1, 0, 0)),
    ((49, 32, 7, 1, 1, (3, 0), 37, 45, 1, 4, 4, False), 3, (2, 3, 8, 64, 503, 2, 2, 0, 0)),
    ((49, 49, 1, 7, 1, (0, 3), 37, 45, 1, 4, 4, False), 3, (2, 3, 8, 64, 507, 2, 4, 0, 0)),
    ((30, 32, 3, 3, 1, P1, 260, 515, 1, 4, 4, False), 3, (2, 3, 8, 32, 302, 3, 1, 0, 0)),
    ((25, 32, 7, 1, 1, (3, 0), 37, 45, 1, 4, 4, False), 3, (2, 3, 8, 32, 502, 2, 2, 0, 0)),
    ((25, 25, 1, 5, 1, (0, 2), 37, 45, 1, 4, 4, False), 3, (2, 3, 8, 32, 504, 2, 2, 0, 0)),
    # the big kernel: with the 4-lane tail folded (52 channels: the fewest K chunks it takes), and without a tail
    ((101, 52, 3, 3, 1, P1, 515, 520, 1, 4, 4, False), 3, (3, 3, 16, 128, 0, 1, 1, 1, 0)),
    ((128, 96, 3, 3, 1, P1, 515, 520, 1, 4, 4, False), 3, (3, 3, 16, 128, 0, 1, 1, 0, 0)),
    ((49, 100, 3, 3, 1, P1, 515, 520, 1, 4, 4, False), 3, (3, 3, 16, 64, 0, 1, 1, 1, 0)),
    ((64, 96, 3, 3, 1, P1, 515, 520, 1, 4, 4, False), 3, (3, 3, 16, 64, 0, 1, 1, 0, 0)),
    # six-term products: 8-row tiles at any size, no split-K
    ((49, 36, 3, 3, 1, P1, 37, 45, 2, 4, 4, False), 6, (2, 6, 8, 64, 305, 2, 1, 0, 1)),
    ((49, 32, 7, 1, 1, (3, 0), 37, 45, 1, 4, 4, False), 6, (2, 6, 8, 64, 505, 2, 1, 0, 0)),
    ((49, 49, 1, 7, 1, (0, 3), 37, 45, 1, 4, 4, False), 6, (2, 6, 8, 64, 511, 2, 1, 0, 0)),
    ((30, 20, 3, 3, 1, P1, 37, 45, 1, 4, 4, False), 6, (2, 6, 8, 32, 303, 2, 1, 0, 0)),
    ((25, 32, 7, 1, 1, (3, 0), 37, 45, 1, 4, 4, False), 6, (2, 6, 8, 32, 503, 2, 1, 0, 0)),
    ((25, 25, 1, 5, 1, (0, 2), 37, 45, 1, 4, 4, False), 6, (2, 6, 8, 32, 506, 2, 1, 0, 0)),
]
# ... plan[:6]; each case runs with fp32 and with fp16 x
F16_CASES = [
    ((101, 20, 3, 3, 1, P1, 99, 450, 2, 8, 4, False), (1, 0, 16, 128, 509, 1)),                  # 16 rows: from 192 tiles of them
    ((101, 49, 3, 3, 1, P1, 33, 47, 1, 8, 4, False), (1, 0, 8, 128, 509, 1)),
    ((49, 36, 3, 3, 1, P1, 37, 45, 2, 8, 4, False), (1, 0, 8, 64, 509, 2)),
    ((30, 20, 3, 3, 1, P1, 99, 450, 2, 8, 4, False), (1, 0, 16, 32, 509, 2)),
    ((30, 20, 1, 1, 1, P0, 37, 45, 1, 8, 4, False), (1, 0, 8, 32, 509, 2)),
    ((128, 96, 3, 3, 2, P1, 67, 45, 1, 8, 4, False), (1, 0, 8, 128, 913, 1)),                    # NetC's 96 -> 128 stride-2 layer
    ((49, 20, 3, 3, 2, P1, 67, 45, 1, 8, 4, False), (1, 0, 8, 64, 913, 1)),
    ((30, 3, 7, 7, 1, (3, 3), 37, 45, 1, 8, 4, False), (1, 0, 8, 32, 913, 2)),
]
# ... plan[:6]
WINO_CASES = [
    ((49, 20, 3, 3, 1, P1, 67, 250, 2, 4, 4, False), (4, 0, 8, 64, 0, 2)),                       # two channel blocks per wave: from 256 workgroups
    ((30, 20, 3, 3, 1, P1, 259, 250, 2, 4, 4, False), (4, 0, 16, 32, 0, 2)),                     # 16 rows: from 512 tiles of them
    ((30, 36, 3, 3, 1, P1, 37, 29, 3, 4, 4, False), (4, 0, 8, 32, 0, 2)),
]
# ... terms, plan[:6].  The schedule's cases depend on the CU count: b3_schedule_cases
B3_CASES = [
    ((101, 52, 3, 3, 1, P1, 37, 45, 2, 4, 4, False), 6, (5, 6, 16, 64, 0, 1)),                   # two channel groups, four K steps
    ((49, 20, 3, 3, 1, P1, 37, 45, 2, 4, 4, False), 8, (5, 8, 16, 64, 0, 1)),
    ((49, 20, 3, 3, 1, P1, 37, 45, 2, 4, 4, False), 9, (5, 9, 16, 64, 0, 1)),
]


def case_id(v):
    return "-".join(str(x) for x in v).replace(" ", "") if isinstance(v, tuple) else str(v)


def b3_schedule_cases(cus):
    """conv_wino_b3_kernel's persistent schedule on a device of cus compute units, as (name, case, tiles): 64 <- 16 channels so that a case
    costs nothing.  Tile counts 7, cus - 1, cus, cus + 1 and 2 cus + 7 as a single tile row (H = 11, W ragged) or a single tile column
    (W = 11, H ragged); three images of three tile columns, so that the steps carry through column, row and image; and the first count
    past cus that two and three channel groups (cout 128, 192) divide."""
    def row(n):
        return (64, 16, 3, 3, 1, P1, 11, 16 * n - 5, 1, 4, 4, False)

    def col(n, B=1):
        return (64, 16, 3, 3, 1, P1, 16 * n - 5, 11, B, 4, 4, False)
    rows = cus // 9 + 2
    cases = [("7 tiles, a row", row(7), 7), ("7 tiles, a column", col(7), 7),
             ("cus - 1 tiles, a row", row(cus - 1), cus - 1), ("cus tiles, a column", col(cus), cus),
             ("cus + 1 tiles, a row", row(cus + 1), cus + 1), ("2 cus + 7 tiles, a column", col(2 * cus + 7), 2 * cus + 7),
             ("2 x (cus + 1) / 2 tiles, columns of two images", col(-(-(cus + 1) // 2), 2), 2 * -(-(cus + 1) // 2)),
             ("3 images x 3 columns", (64, 16, 3, 3, 1, P1, 16 * rows - 5, 43, 3, 4, 4, False), 9 * rows)]
    for co in (128, 192):
        n = -(-(cus + 1) // (co // 64))
        cases.append((f"cout {co}: {co // 64} x {n} tiles", (co, 16, 3, 3, 1, P1, 11, 16 * n - 5, 1, 4, 4, False), n * (co // 64)))
    return cases


# ---- every case reaches its plan -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,terms,want", SPLIT_CASES, ids=case_id)
def test_split_case_reaches_its_plan(case, terms, want):
    assert case_plan(SPLIT, case, terms=terms)[:9] == want, POLICY


@pytest.mark.parametrize("x16", [0, 1])
@pytest.mark.parametrize("case,want", F16_CASES, ids=case_id)
def test_f16_case_reaches_its_plan(case, want, x16):
    assert case_plan(F16, case, x16=x16)[:6] == want, POLICY


@pytest.mark.parametrize("case,want", WINO_CASES, ids=case_id)
def test_wino_case_reaches_its_plan(case, want):
    assert case_plan(WINO, case)[:6] == want, POLICY


@pytest.mark.parametrize("case,terms,want", B3_CASES, ids=case_id)
def test_b3_case_reaches_its_plan(case, terms, want):
    assert case_plan(WINO_B3, case, terms=terms)[:6] == want, POLICY


@pytest.mark.parametrize("cus", [8, 64, 256, 304])
def test_b3_schedule_cases_have_their_tile_counts(cus):
    for name, case, tiles in b3_schedule_cases(cus):
        co, _, _, _, _, _, H, W, B = case[:9]
        assert B * -(-H // 16) * -(-W // 16) * (co // 64) == tiles, name
        assert case_plan(WINO_B3, case, terms=6, cus=cus) == (5, 6, 16, 64, 0, 1, 1, 0, 0, min(tiles, cus)), name
    counts = [t for _, _, t in b3_schedule_cases(cus)]
    assert {7, cus - 1, cus, cus + 1, 2 * cus + 7} <= set(counts)
    assert any(t > cus and t % 8 for t in counts) and any(t < 8 for t in counts)


def all_cases(schedule=True):
    """(kernel, case, terms, x16, plan) of every case of this file; schedule: with conv_wino_b3_kernel's schedule cases at CUS"""
    for case, terms, _ in SPLIT_CASES:
        yield SPLIT, case, terms, 0, case_plan(SPLIT, case, terms=terms)
    for case, _ in F16_CASES:
        for x16 in (0, 1):
            yield F16, case, 0, x16, case_plan(F16, case, x16=x16)
    for case, _ in WINO_CASES:
        yield WINO, case, 0, 0, case_plan(WINO, case)
    for case, terms, _ in B3_CASES:
        yield WINO_B3, case, terms, 0, case_plan(WINO_B3, case, terms=terms)
    for _, case, _ in b3_schedule_cases(CUS) if schedule else ():
        yield WINO_B3, case, 6, 0, case_plan(WINO_B3, case, terms=6)


def test_cases_have_ragged_edges_and_wide_strides():
    ragged = set()
    for kernel, case, terms, x16, p in all_cases():
        co, ci, kh, kw, s, pad, H, W, B, xe, ye, res = case
        Ho, Wo = (H + 2 * pad[0] - kh) // s + 1, (W + 2 * pad[1] - kw) // s + 1
        cols = 16 if kernel in (WINO, WINO_B3) else 32
        assert Wo % cols and Ho % p[2], case
        assert xe > 0 and ye > 0 and not res, case
        ragged |= {(p[0], p[3], "block") for _ in [0] if co % 32} | {(p[0], p[3], "quad") for _ in [0] if co % 4}
    for kernel, widths in ((SPLIT, (32, 64, 128)), (SPLIT_BIG, (64, 128)), (F16, (32, 64, 128)), (WINO, (32, 64)), (WINO_B3, (64,))):
        for chans in widths:          # per tile width, a cout that leaves the last channel block and the last quad ragged
            assert (kernel, chans, "block") in ragged and (kernel, chans, "quad") in ragged, (kernel, chans)


# ---- the grid --------------------------------------------------------------------------------------------------------------------
# layers outside the network, for the instantiations nothing in it reaches: a 7 x 1 layer of at most 32 outputs (the tall patch on a
# 32-channel tile) and one of three K chunks of 16 channels (three split-K shares)
REST_LAYERS = [(25, 32, 7, 1), (64, 36, 3, 3)]
SIZES = (5, 8, 33, 37, 45, 67, 97, 130, 259, 300, 515, 1030)


def _grid(k3_only=False):
    for (co, ci, kh, kw) in NET_LAYERS + REST_LAYERS:
        if k3_only and (kh, kw) != (3, 3):
            continue
        for H in SIZES:
            for W in SIZES:
                yield (co, ci, kh, kw), (kh // 2, kw // 2), H, W


@pytest.fixture(scope="module")
def sweeps():
    """Per family {call: [plan at each of BATCHES]} over the grid; call = (layer, stride, H, W, terms or fp16 x)."""
    split, f16, wino, b3 = {}, {}, {}, {}
    for (co, ci, kh, kw), pad, H, W in _grid():
        for s in (1, 2):
            for terms in (3, 6):
                split[(co, ci, kh, kw, s, H, W, terms)] = [kplan(SPLIT, co, ci, kh, kw, s, pad, H, W, B, terms) for B in BATCHES]
            for x16 in (0, 1):
                f16[(co, ci, kh, kw, s, H, W, x16)] = [kplan(F16, co, ci, kh, kw, s, pad, H, W, B, x16=x16) for B in BATCHES]
    for (co, ci, kh, kw), pad, H, W in _grid(k3_only=True):
        wino[(co, ci, H, W)] = [kplan(WINO, co, ci, 3, 3, 1, pad, H, W, B) for B in BATCHES]
        for terms in (6, 8, 9):
            b3[(co, ci, H, W, terms)] = [kplan(WINO_B3, co, ci, 3, 3, 1, pad, H, W, B, terms) for B in BATCHES]
    return {SPLIT: split, F16: f16, WINO: wino, WINO_B3: b3}


def _reached(sweep):
    return {p for plans in sweep.values() for p in plans if p is not None}


def test_tools_only_instantiations_are_the_listed_ones():
    tools = set()
    for name in SOURCES:
        tools |= instantiations(name)[1]
    assert tools == TOOLS_ONLY, (sorted(tools - TOOLS_ONLY), sorted(TOOLS_ONLY - tools))


@pytest.mark.parametrize("name,kernel", [("conv_split.hip", SPLIT), ("conv_f16.hip", F16), ("conv_wino.hip", WINO), ("conv_wino_b3.hip", WINO_B3)])
def test_grid_and_cases_reach_exactly_the_production_instantiations(sweeps, name, kernel):
    production = instantiations(name)[0]
    assert len(production) == {SPLIT: 20, F16: 8, WINO: 3, WINO_B3: 3}[kernel], sorted(production)
    reached = {inst(p) for p in _reached(sweeps[kernel])}
    assert reached == production, (f"{POLICY}: the grid reaches {sorted(reached - production)} that {name} does not name; it does not reach "
                                   f"{sorted(production - reached)}")
    cased = {inst(p) for k, _, _, _, p in all_cases(schedule=False) if k == kernel}
    assert cased == production, f"{POLICY}: instantiations of {name} without a case {sorted(production - cased)}"


def test_split_cases_reach_every_kind_of_plan_the_grid_reaches(sweeps):
    """Besides the instantiation: both fold states of each big kernel, every split-K factor, the image-by-image batch."""
    def kinds(plans):
        return ({(p[3], p[7]) for p in plans if p[0] == SPLIT_BIG}, {p[6] for p in plans}, {p[8] for p in plans},
                {p[7] for p in plans if p[0] == SPLIT})
    cased = kinds([p for k, _, _, _, p in all_cases() if k == SPLIT])
    assert kinds(_reached(sweeps[SPLIT])) == cased, POLICY
    assert cased == ({(64, 0), (64, 1), (128, 0), (128, 1)}, set(range(1, 9)), {0, 1}, {0})


def test_every_case_is_needed():
    """Without any one case, an instantiation, a fold state of a big kernel, a split-K factor or the image-by-image batch has no case."""
    def kinds(plans):
        return {inst(p) for p in plans} | {("fold", p[3], p[7]) for p in plans if p[0] == SPLIT_BIG} | {("shares", p[6]) for p in plans} | \
               {("image by image", p[8]) for p in plans}
    cases = [(k, c, t, p) for k, c, t, x16, p in all_cases(schedule=False) if not x16]
    for i, (k, c, t, p) in enumerate(cases):
        rest = [q for j, (_, _, _, q) in enumerate(cases) if j != i]
        assert kinds([p]) - kinds(rest), f"the case {c} (terms {t}) adds nothing to the others"


# ---- batch rules -----------------------------------------------------------------------------------------------------------------
def test_acceptance_does_not_depend_on_the_batch(sweeps):
    for kernel, sweep in sweeps.items():
        bad = [(g, plans) for g, plans in sweep.items() if len({p is None for p in plans}) > 1]
        assert not bad, (kernel, bad[:5])
    assert any(p is None for plans in sweeps[SPLIT].values() for p in plans)          # the grid has refused calls: 7 x 7, stride 2 at six terms


def test_split_k_shares_do_not_depend_on_the_batch(sweeps):
    """One image's split-K shares, hence its summation order, are the same at every B (the handle runs a batch it could split image by
    image)."""
    bad = [(g, plans) for g, plans in sweeps[SPLIT].items() if len({p[6] for p in plans if p is not None}) > 1]
    assert not bad, bad[:5]
    split_b1 = [g for g, plans in sweeps[SPLIT].items() if plans[0] is not None and plans[0][6] > 1]
    assert split_b1 and all(p[8] == 1 for g in split_b1 for p in sweeps[SPLIT][g][1:])


def test_a_folded_tail_does_not_depend_on_the_batch(sweeps):
    """The big split kernel multiplies a 4-lane tail chunk with its taps folded into K, the small one as a zero-padded chunk: other
    summation orders.  For the layers that have such a tail (staged channels = 4 mod 16), which of the two runs is decided per image."""
    tailed = {g: plans for g, plans in sweeps[SPLIT].items() if g[2:4] == (3, 3) and _r(g[1], 4) % 16 == 4 and plans[0] is not None}
    assert {g[1] for g in tailed} >= {49, 130, 386} and any(p[7] for plans in tailed.values() for p in plans)
    bad = [(g, plans) for g, plans in tailed.items() if len({(p[0], p[7]) for p in plans}) > 1]
    assert not bad, bad[:5]
    for g, plans in tailed.items():
        assert all(p[7] == (p[0] == SPLIT_BIG) for p in plans), (g, plans)
    # and without such a tail nothing is ever folded
    assert not any(p[7] for g, plans in sweeps[SPLIT].items() if g not in tailed for p in plans if p is not None)


def test_plan_refuses_what_the_entry_points_refuse():
    lib = _lib.load()
    out = (ctypes.c_int * 10)()

    def refused(args, *words):
        assert lib.pivlfn_conv2d_nhwc_kernel_plan(*args, out) == 1, args
        msg = lib.pivlfn_last_error().decode()
        for w in words:
            assert w in msg, (w, msg)
    #        kernel, cout, cin, kh, kw, B, H, W, stride, pad_y, pad_x, terms, x_is_f16, x_stride, y_stride, cus
    refused((SPLIT, 32, 32, 3, 3, 1, 8, 8, 1, 1, 1, 4, 0, 32, 32, CUS), "conv2d_split", "terms=4")
    refused((SPLIT, 32, 32, 3, 3, 1, 8, 8, 2, 1, 1, 6, 0, 32, 32, CUS), "conv2d_split", "stride 2", "6-term")
    refused((SPLIT, 32, 3, 9, 9, 1, 64, 64, 1, 4, 4, 3, 0, 4, 32, CUS), "conv2d_split", "not covered")
    refused((SPLIT, 32, 32, 3, 3, 1, 8, 8, 1, 1, 1, 3, 0, 30, 32, CUS), "conv2d_split", "x_stride=30")
    refused((SPLIT, 30, 32, 3, 3, 1, 8, 8, 1, 1, 1, 3, 0, 32, 30, CUS), "conv2d_split", "y_stride=30")
    refused((SPLIT, 32, 32, 3, 3, 1, 1, 1, 1, 0, 0, 3, 0, 32, 32, CUS), "conv2d_split", "bad geometry")
    refused((SPLIT, 32, 32, 3, 3, 0, 8, 8, 1, 1, 1, 3, 0, 32, 32, CUS), "conv_split", "empty output")
    refused((F16, 32, 32, 3, 3, 1, 8, 8, 1, 1, 1, 0, 1, 36, 32, CUS), "conv2d_f16", "multiple of 8")
    refused((F16, 32, 32, 3, 3, 1, 8, 8, 1, 1, 1, 0, 0, 32, 28, CUS), "conv2d_f16", "y_stride=28")
    refused((F16, 32, 32, 3, 3, 1, 8, 8, 0, 1, 1, 0, 0, 32, 32, CUS), "conv2d_f16", "bad geometry")
    refused((F16, 128, 32, 9, 9, 1, 64, 64, 1, 4, 4, 0, 0, 32, 128, CUS), "conv_f16", "LDS tile")
    refused((WINO, 32, 32, 5, 5, 1, 8, 8, 1, 1, 1, 0, 0, 32, 32, CUS), "conv2d_wino", "not 3 x 3")
    refused((WINO, 32, 32, 3, 3, 1, 8, 8, 2, 1, 1, 0, 0, 32, 32, CUS), "conv2d_wino", "stride 1")
    refused((WINO, 32, 32, 3, 3, 1, 8, 30000, 1, 1, 1, 0, 0, 1024, 32, CUS), "conv_wino", "exceed 2 GiB")
    refused((WINO_B3, 32, 32, 3, 3, 1, 8, 8, 1, 1, 1, 6, 0, 32, 32, CUS), "conv2d_wino_b3", "64-channel")
    refused((WINO_B3, 64, 32, 3, 3, 1, 8, 8, 1, 1, 1, 7, 0, 32, 64, CUS), "conv_wino_b3", "terms=7")
    refused((WINO_B3, 64, 32, 3, 3, 1, 8, 8, 1, 1, 1, 6, 0, 32, 64, 0), "conv_wino_b3", "compute units")
    refused((6, 64, 32, 3, 3, 1, 8, 8, 1, 1, 1, 6, 0, 32, 64, CUS), "kernel=6")
    assert lib.pivlfn_conv2d_nhwc_kernel_plan(SPLIT, 32, 32, 3, 3, 1, 8, 8, 1, 1, 1, 3, 0, 32, 32, CUS, None) == 1


# ---- conv_wino_b3_kernel's schedule, restated ------------------------------------------------------------------------------------
def b3_units_of(block, grid, units):
    """conv_wino_b3.hip, "this workgroup's tiles": the unit ids workgroup `block` of `grid` multiplies, in its order.  Every XCD (block
    mod 8) owns a contiguous band of the units, its workgroups take the band's units round-robin."""
    xcd = block & 7
    tstride = (grid - xcd + 7) >> 3
    tq, tr = units >> 3, units & 7
    uend = (xcd * (tq + 1) if xcd < tr else tr * (tq + 1) + (xcd - tr) * tq) + tq + (1 if xcd < tr else 0)
    ufirst = uend - tq - (1 if xcd < tr else 0) + (block >> 3)
    if ufirst >= uend:
        return [], tstride
    ntiles = (uend - ufirst + tstride - 1) // tstride
    return [ufirst + i * tstride for i in range(ntiles)], tstride


def b3_walk(tile0, tstride, n, NG, tiles_x, tiles_y):
    """The same file, "tile coordinates without divisions in the loop": (group, column, row, image) of n tiles from tile0 on, advanced by
    the decomposed stride with one carry each (the flat order)."""
    lng, ltx, lty, lb = tile0 % NG, (tile0 // NG) % tiles_x, (tile0 // NG // tiles_x) % tiles_y, tile0 // NG // tiles_x // tiles_y
    dsp = tstride // NG
    dng, dtx, dty, db = tstride % NG, dsp % tiles_x, (dsp // tiles_x) % tiles_y, dsp // tiles_x // tiles_y
    out = []
    for _ in range(n):
        out.append((lng, ltx, lty, lb))
        lng += dng
        if lng >= NG:
            lng -= NG
            ltx += 1
        ltx += dtx
        if ltx >= tiles_x:
            ltx -= tiles_x
            lty += 1
        lty += dty
        if lty >= tiles_y:
            lty -= tiles_y
            lb += 1
        lb += db
    return out


def test_b3_schedule_is_restated_from_the_source():
    """The lines b3_units_of restates, held to the .hip text."""
    text = open(os.path.join(CSRC, "conv_wino_b3.hip")).read()
    for line in ("const int xcd = blockIdx.x & 7;",
                 "const int tstride = ((int)gridDim.x - xcd + 7) >> 3;",
                 "const int tq = units >> 3, tr = units & 7;",
                 "const int uend = (xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq) + tq + (xcd < tr ? 1 : 0);",
                 "const int ufirst = uend - tq - (xcd < tr ? 1 : 0) + (int)(blockIdx.x >> 3);",
                 "if (ufirst >= uend) return;",
                 "const int ntiles = ((uend - ufirst + tstride - 1) / tstride) * (ginner ? NG : 1);",
                 "const int dsp = ginner ? tstride : tstride / NG;",
                 "const int dng = ginner ? 0 : tstride % NG, dtx = dsp % tiles_x, dty = (dsp / tiles_x) % tiles_y, db = dsp / tiles_x / tiles_y;",
                 "#define B3_GINNER 0"):
        assert line in text, line


def test_b3_partition_takes_every_tile_once():
    cu_counts = (8, 9, 15, 16, 63, 64, 65, 100, 104, 128, 255, 256, 257, 304)
    for cus in cu_counts:
        for units in list(range(1, 701)) + [1520, 4096, 8192, 8193] + [t for _, _, t in b3_schedule_cases(cus)]:
            grid = min(units, cus)
            taken = sorted(u for b in range(grid) for u in b3_units_of(b, grid, units)[0])
            assert taken == list(range(units)), (cus, units)


@pytest.mark.parametrize("cus", [8, 64, 104, 256, 304])
def test_b3_stepping_arrives_at_the_partitions_tiles(cus):
    for _, case, tiles in b3_schedule_cases(cus) + [("", c, 0) for c, _, _ in B3_CASES] + \
            [("", (192, 16, 3, 3, 1, P1, 16 * 7 - 5, 16 * 5 - 5, 3, 4, 4, False), 0)]:
        co, _, _, _, _, _, H, W, B = case[:9]
        NG, tiles_x, tiles_y = -(-co // 64), -(-W // 16), -(-H // 16)
        units = B * tiles_y * tiles_x * NG
        grid = min(units, cus)
        for b in range(grid):
            ids, tstride = b3_units_of(b, grid, units)
            want = [(u % NG, (u // NG) % tiles_x, (u // NG // tiles_x) % tiles_y, u // NG // tiles_x // tiles_y) for u in ids]
            assert b3_walk(ids[0], tstride, len(ids), NG, tiles_x, tiles_y) == want, (case, b)
