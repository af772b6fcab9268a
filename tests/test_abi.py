"""CPU: the C-ABI library loads and exports every symbol include/pivlfn.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "pivlfn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#ifdef PIVLFN_TOOLS.*?#endif", "", text, flags=re.S)      # tools-build-only declarations are not the boundary
    return sorted(set(re.findall(r"\b(pivlfn_[a-z_0-9]+)\s*\(", text)))


def test_header_declares_the_boundary():
    names = _declared()
    for must in ("pivlfn_corr_fwd", "pivlfn_backwarp", "pivlfn_warp_corr_fwd", "pivlfn_create", "pivlfn_destroy",
                 "pivlfn_workspace_bytes", "pivlfn_forward", "pivlfn_last_error", "pivlfn_resize_bilinear"):
        assert must in names


def test_library_exports_every_declared_symbol():
    from pivlfn import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared():
        assert hasattr(lib, name), f"{name} declared in include/pivlfn.h but not exported"
    assert set(_declared()) == set(_lib.SIGNATURES), "ctypes prototypes out of sync with the header"
    assert not hasattr(lib, "pivlfn_tune"), "the production library must not export the tools-only knob setter"
    loaded = _lib.load()
    assert loaded.pivlfn_abi_version() == 3
    assert loaded.pivlfn_last_error() is not None


def test_argument_errors_are_reported_without_a_gpu():
    from pivlfn import _lib
    lib = _lib.load()
    # null pointers / bad shapes are rejected on the host before any launch
    assert lib.pivlfn_corr_fwd(None, None, None, 1, 8, 4, 4, 1, None) != 0
    assert b"null" in lib.pivlfn_last_error()
    assert lib.pivlfn_workspace_bytes(None, 1, 64, 64) == 0
    with pytest.raises(ValueError):
        _lib.check(lib.pivlfn_backwarp(None, None, None, 1, 1, 1, 1, None), "backwarp")


NEW_OPS = ("pivlfn_upconv_nhwc", "pivlfn_backwarp_nhwc", "pivlfn_reg_prep", "pivlfn_reg_tail", "pivlfn_prep_pyramid",
           "pivlfn_conv1_fused_nhwc")
PLAN_OPS = ("pivlfn_conv2d_nhwc_plan", "pivlfn_conv2d_nhwc_kernel_plan", "pivlfn_conv_head_nhwc_plan")      # host only: no handle, no stream, nothing launched


def test_per_layer_entry_points_are_declared():
    names = _declared()
    for must in NEW_OPS + PLAN_OPS:
        assert must in names


def test_per_layer_entry_points_reject_bad_arguments_without_a_gpu():
    """Null pointers and shapes the kernels do not cover are refused on the host with PIVLFN_ERR_ARG and a message naming the
    problem, before anything is launched or allocated (a launch on a machine without a GPU would return PIVLFN_ERR_HIP instead)."""
    import ctypes
    from pivlfn import _lib
    lib = _lib.load()
    P = 4096                      # a non-null pointer that is never dereferenced: every case below fails its checks first
    m6 = (ctypes.c_float * 6)()
    fused = ctypes.c_int(7)

    def refused(rc, *words):
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    # upconv
    refused(lib.pivlfn_upconv_nhwc(None, P, P, 1, 4, 4, 1, 4, 4, None), "upconv", "null")
    refused(lib.pivlfn_upconv_nhwc(P, P, P, 1, 4, 4, 2, 8, 8, None), "quads=2")
    refused(lib.pivlfn_upconv_nhwc(P, P, P, 1, 4, 4, 14, 52, 56, None), "strides")
    refused(lib.pivlfn_upconv_nhwc(P, P, P, 1, 4, 4, 1, 6, 8, None), "multiples of 4")
    refused(lib.pivlfn_upconv_nhwc(P, P, P, 1, 40000, 4, 1, 4, 4, None), "80000 output rows")
    refused(lib.pivlfn_upconv_nhwc(P, P, P, 70000, 4, 4, 1, 4, 4, None), "70000 images")
    refused(lib.pivlfn_upconv_nhwc(P, P, P, 0, 4, 4, 1, 4, 4, None), "positive")
    # backwarp_nhwc
    refused(lib.pivlfn_backwarp_nhwc(P, None, 1.0, P, 1, 4, 4, 4, None), "backwarp_nhwc", "null")
    refused(lib.pivlfn_backwarp_nhwc(P, P, 1.0, P, 1, 4, 4, 6, None), "C=6", "multiple of 4")
    refused(lib.pivlfn_backwarp_nhwc(P, P, 1.0, P, 1, 32768, 32768, 8, None), "32-bit index range")
    refused(lib.pivlfn_backwarp_nhwc(P, P, 1.0, P, 1, 0, 4, 4, None), "positive")
    # reg_prep
    refused(lib.pivlfn_reg_prep(P, P, P, 1.0, P, P, None, 1, 4, 4, 1, None), "reg_prep", "null")
    refused(lib.pivlfn_reg_prep(P, P, P, 1.0, P, P, P, 70000, 4, 4, 1, None), "B=70000")
    refused(lib.pivlfn_reg_prep(P, P, P, 1.0, P, P, P, 1, 46341, 46341, 1, None), "32-bit index range")
    refused(lib.pivlfn_reg_prep(P, P, P, 1.0, P, P, P, 1, 4, 4, 2, None), "fused=2")
    # reg_tail
    refused(lib.pivlfn_reg_tail(P, 52, P, P, P, 0.0, 0.0, 7, None, None, 1.0, 1, 4, 4, None), "reg_tail", "null")
    refused(lib.pivlfn_reg_tail(P, 52, P, P, P, 0.0, 0.0, 4, P, None, 1.0, 1, 4, 4, None), "k=4")
    refused(lib.pivlfn_reg_tail(P, 48, P, P, P, 0.0, 0.0, 7, P, None, 1.0, 1, 4, 4, None), "dstride=48", ">= 49")
    refused(lib.pivlfn_reg_tail(P, 12, P, P, P, 0.0, 0.0, 3, None, P, 1.0, 1, 0, 4, None), "H=0")
    # prep_pyramid
    refused(lib.pivlfn_prep_pyramid(P, P, None, P, 1, 64, 64, 6, None), "prep_pyramid", "null")
    refused(lib.pivlfn_prep_pyramid(P, P, m6, P, 1, 64, 64, 7, None), "levels=7")
    refused(lib.pivlfn_prep_pyramid(P, P, m6, P, 1, 16, 64, 6, None), "no pixel at level 6")
    # conv1_fused
    args = [P] * 10
    refused(lib.pivlfn_conv1_fused_nhwc(*args[:6], None, *args[7:], 2, 64, 64, 1, ctypes.byref(fused), None), "conv1_fused", "null")
    refused(lib.pivlfn_conv1_fused_nhwc(*args, 2, 64, 64, 3, ctypes.byref(fused), None), "B_feat=3")
    refused(lib.pivlfn_conv1_fused_nhwc(*args, 2, 64, 64, 0, ctypes.byref(fused), None), "B_feat=0")
    refused(lib.pivlfn_conv1_fused_nhwc(*args, 70000, 40000, 64, 1, ctypes.byref(fused), None), "32-bit index range")
    with pytest.raises(ValueError):
        _lib.check(lib.pivlfn_reg_tail(P, 12, P, P, P, 0.0, 0.0, 5, P, P, 1.0, 1, 4, 4, None), "reg_tail")
    # the launchers' plans: answered on the host, refused like the entry point asked about
    plan = (ctypes.c_int * 10)()
    assert lib.pivlfn_conv2d_nhwc_kernel_plan(2, 64, 32, 3, 3, 1, 64, 64, 1, 1, 1, 3, 0, 32, 64, 256, plan) == 0 and plan[0] == 2
    refused(lib.pivlfn_conv2d_nhwc_kernel_plan(2, 64, 32, 3, 3, 1, 64, 64, 1, 1, 1, 5, 0, 32, 64, 256, plan), "conv2d_split", "terms=5")
    refused(lib.pivlfn_conv2d_nhwc_kernel_plan(0, 64, 32, 3, 3, 1, 64, 64, 1, 1, 1, 3, 0, 32, 64, 256, plan), "kernel=0")
    refused(lib.pivlfn_conv2d_nhwc_kernel_plan(2, 64, 32, 3, 3, 1, 64, 64, 1, 1, 1, 3, 0, 32, 64, 256, None), "conv2d_kernel_plan")
    assert lib.pivlfn_conv_head_nhwc_plan(7, 2, 256, 300, plan) == 0 and tuple(plan[:4]) == (4, 8, 58, 2 * 32 * 6)
    refused(lib.pivlfn_conv_head_nhwc_plan(4, 1, 64, 64, plan), "conv_head", "k=4")
    refused(lib.pivlfn_conv_head_nhwc_plan(7, 1, 0, 64, plan), "conv_head", "bad arguments")
    refused(lib.pivlfn_conv_head_nhwc_plan(7, 1, 64, 64, None), "conv_head_plan")
    # the entry point itself: the same refusals, before anything is launched
    refused(lib.pivlfn_conv_head_nhwc(None, P, P, P, 1, 64, 64, None), "conv_head")
