"""pivlfn_conv2d_nhwc_dist_b3_plan: the checks of pivlfn_conv2d_nhwc_dist_b3 (csrc/conv_dist_b3.hip) for a layer shape and a call geometry, on
the host -- what the entry point refuses is refused here with the same message and PIVLFN_ERR_ARG, without a handle and without a GPU; what
it accepts comes back with the launch it would make.  Also: pivlfn_conv2d_nhwc_plan keeps reporting the fp32-instruction streaming kernels
for these layers (the entry point behind it keeps launching them)."""
import ctypes

import pytest

from pivlfn import _lib

COL = (49, 32, 7, 1)      # cout, cin, kh, kw
ROW = (49, 49, 1, 7)


def plan(layer, B, H, W, terms, xs, ys):
    out = (ctypes.c_int * 4)()
    rc = _lib.load().pivlfn_conv2d_nhwc_dist_b3_plan(*layer, B, H, W, terms, xs, ys, out)
    return rc, tuple(out), _lib.load().pivlfn_last_error().decode()


@pytest.mark.parametrize("layer,row,occ,xs", [(COL, 0, 2, 32), (ROW, 1, 1, 52)])
def test_plan_of_accepted_calls(layer, row, occ, xs):
    for terms in (6, 8, 9):
        # one pixel; 17 x 33, two images: 2 x 3 x 2 = 12 tiles of 16 x 16, four per workgroup; five tiles: two workgroups
        for (B, H, W), wgs in (((1, 1, 1), 1), ((2, 17, 33), 3), ((1, 6, 80), 2), ((1, 1024, 1024), 1024)):
            rc, p, msg = plan(layer, B, H, W, terms, xs, 52)
            assert rc == 0, msg
            assert p == (row, terms, wgs, occ)
    assert plan(layer, 1, 8, 8, 6, 64, 56)[0] == 0      # wider tensors on both sides


def test_plan_refuses_what_the_entry_point_refuses():
    def refused(args, *words):
        rc, _, msg = plan(*args)
        assert rc == 1, (args, rc)      # PIVLFN_ERR_ARG
        for w in words:
            assert w in msg, (w, msg)
    refused((COL, 1, 8, 8, 7, 32, 52), "conv_dist_b3", "terms=7")
    refused((ROW, 1, 8, 8, 3, 52, 52), "conv_dist_b3", "terms=3")
    refused((COL, 1, 8, 8, 6, 28, 52), "conv_dist_b3", "strides 28, 52")      # fewer lanes than the layer's channels
    refused((COL, 1, 8, 8, 6, 34, 52), "conv_dist_b3", "strides 34, 52")      # not a multiple of 4
    refused((ROW, 1, 8, 8, 6, 48, 52), "conv_dist_b3", "52 staged lanes")     # the 49-channel source lives on 52 lanes
    refused((ROW, 1, 8, 8, 6, 52, 48), "conv_dist_b3", "52 stored lanes")
    refused((COL, 1, 8, 8, 6, 32, 54), "conv_dist_b3", "strides 32, 54")
    refused((COL, 1, 4096, 4096, 6, 32, 52), "conv_dist_b3", "2 GiB")         # 4096^2 x 52 lanes x 4 bytes = 3.25 GiB of offsets
    refused((ROW, 1, 3300, 3300, 6, 52, 52), "conv_dist_b3", "2 GiB")
    assert plan(ROW, 1, 3200, 3200, 6, 52, 52)[0] == 0                          # 1.98 GiB: inside
    assert plan(ROW, 8, 3200, 3200, 6, 52, 52)[0] == 0                          # the bound is per image, never per batch
    refused((COL, 0, 8, 8, 6, 32, 52), "conv_dist_b3", "bad arguments")
    refused((COL, 1, 0, 8, 6, 32, 52), "conv_dist_b3", "bad arguments")
    refused(((48, 32, 7, 1), 1, 8, 8, 6, 32, 52), "conv2d_dist_b3", "distance convolution")
    refused(((49, 32, 1, 7), 1, 8, 8, 6, 32, 52), "conv2d_dist_b3", "distance convolution")
    refused(((49, 49, 7, 1), 1, 8, 8, 6, 52, 52), "conv2d_dist_b3", "distance convolution")


def test_conv2d_nhwc_plan_keeps_the_fp32_instruction_kernels():
    out = (ctypes.c_int * 5)()
    lib = _lib.load()
    assert lib.pivlfn_conv2d_nhwc_plan(*COL, 1, 256, 272, 1, 3, 0, 0, 0, 32, 52, out) == 0 and out[0] == 6      # PIVLFN_CONV_PLAN_COL7
    assert lib.pivlfn_conv2d_nhwc_plan(*ROW, 1, 256, 272, 1, 0, 3, 0, 0, 52, 52, out) == 0 and out[0] == 7      # PIVLFN_CONV_PLAN_ROW7
