"""GPU: the public op entry points honour the stream they are given.  run.py, pipeline.stream_pairs and pivlfn/sequence.py call them
next to a copy stream and a producer stream; every other test calls them on the current default stream, where a launch on the wrong
stream, a helper hipMemsetAsync on stream 0, a hidden host synchronisation or a per-call allocation cannot be seen.

Covered: the six oldest ops (OPS) and every post-processing entry point added since (NEW_OPS): pivlfn_stereo_2d3c, pivlfn_flow_fields,
pivlfn_flow_stats_accumulate(_masked), pivlfn_error_stats_accumulate, pivlfn_flow_validate, pivlfn_frames_preprocess,
pivlfn_frames_background_min, pivlfn_flow_errors, pivlfn_level_errors, pivlfn_flow_maxrad -> pivlfn_flow_to_color,
pivlfn_field_absmax, pivlfn_scalar_to_color, pivlfn_flow_decimate and pivlfn_match_quality, each at the smallest shape that still
reaches every launch it makes.  Out of scope: the per-layer check entry points (pivlfn_conv2d_nhwc*, pivlfn_backwarp_nhwc,
pivlfn_reg_prep, pivlfn_reg_tail, pivlfn_prep_pyramid), which are exported for tests only, and pivlfn_upconv_nhwc /
pivlfn_conv1_fused_nhwc, which state in the header that they synchronise; the forward has its own stream tests in test_gpu_net.py.

Pinned first: the eager default-stream result of every new spec equals the CPU restatement of its op (tests/*_restatement.py), compared
as that op's own test file compares it -- bit for bit, except the one colour level flow_to_color's file grants for atan2f and the
1e-6 px match_quality's file grants its sub-pixel fit for the fp64 logarithm.  Everything below compares with that eager result, bit
for bit.
Ordering: on a side stream, behind a bounded delay (a chain of matrix products, some tens of milliseconds; its matrices are allocated
once per module) and the copy of the real inputs into buffers that hold poison (NaN, 0xFF for bytes), the op is enqueued without any
host synchronisation; its outputs, pre-filled with the sentinel, equal the eager result.  A launch on another stream reads the poison
or leaves the sentinel -- test_a_call_on_the_wrong_stream_reads_the_poison shows that the set-up does see one.
Capture: the call is captured into a graph (buffers allocated before the capture) and replayed three times with two input sets; each
replay equals the eager result -- which holds the header's "nothing here allocates per call" and the absence of a host synchronisation
(a violation is a capture error).  Host-pointer arguments are read when the call is made and are the same for both input sets.
Alignment: every device pointer one element of its own type into a guarded allocation (the workspaces stay 8-byte aligned, as the
header requires), at a shape with H*W % 4 == 0 where only the launcher's pointer test keeps the vector path away: the same bits.
Wrappers: the post-processing chain of a run.py chunk through the Python API under torch.cuda.stream(side), behind the same delay."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest
import torch

import evaluate_restatement as er
import postpro_restatement as por
import preproc_restatement as pr
import quality_restatement as qr
import stereo_restatement as sr
import validate_restatement as var
import viz_restatement as vzr
from guarded import check_guards, guarded
from pivlfn import _lib

pytestmark = pytest.mark.gpu


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _flow4(B, H, W, seed):
    f = torch.zeros(B, H, W, 4)
    f[..., :2] = 1.5 * _randn((B, H, W, 2), seed)
    return f


def _spec(op, seed):
    """(host inputs, output shapes, call(ins, outs, stream handle)) of one entry point at one small shape."""
    lib = _lib.load()
    if op == "corr_fwd":
        B, C, H, W, s = 2, 20, 19, 31, 3
        ins = [_randn((B, C, H, W), seed), _randn((B, C, H, W), seed + 1)]
        return ins, [(B, 49, 7, 11)], lambda i, o, st: lib.pivlfn_corr_fwd(i[0].data_ptr(), i[1].data_ptr(), o[0].data_ptr(), B, C, H, W, s, st)
    if op == "corr_bwd":
        B, C, H, W, s = 2, 20, 19, 31, 2
        ins = [_randn((B, C, H, W), seed), _randn((B, C, H, W), seed + 1), _randn((B, 49, 10, 16), seed + 2)]
        return ins, [(B, C, H, W), (B, C, H, W)], lambda i, o, st: lib.pivlfn_corr_bwd(
            i[0].data_ptr(), i[1].data_ptr(), i[2].data_ptr(), o[0].data_ptr(), o[1].data_ptr(), B, C, H, W, s, st)
    if op == "backwarp":
        B, C, H, W = 2, 5, 30, 22
        ins = [_randn((B, C, H, W), seed), 2.0 * _randn((B, 2, H, W), seed + 1)]
        return ins, [(B, C, H, W)], lambda i, o, st: lib.pivlfn_backwarp(i[0].data_ptr(), i[1].data_ptr(), o[0].data_ptr(), B, C, H, W, st)
    if op == "warp_corr_fwd":
        B, C, H, W, s = 1, 64, 24, 40, 2
        ins = [_randn((B, C, H, W), seed), _randn((B, C, H, W), seed + 1), 1.5 * _randn((B, 2, H, W), seed + 2)]
        return ins, [(B, 49, 12, 20)], lambda i, o, st: lib.pivlfn_warp_corr_fwd(
            i[0].data_ptr(), i[1].data_ptr(), i[2].data_ptr(), 1.25, o[0].data_ptr(), B, C, H, W, s, 1, st)
    if op == "warp_corr_nhwc":
        B, C, H, W, s = 2, 64, 24, 40, 2
        ins = [_randn((B, H, W, C), seed), _randn((B, H, W, C), seed + 1), _flow4(B, H, W, seed + 2)]
        return ins, [(B, 12, 20, 56)], lambda i, o, st: lib.pivlfn_warp_corr_nhwc(
            i[0].data_ptr(), i[1].data_ptr(), i[2].data_ptr(), 1.25, o[0].data_ptr(), B, C, H, W, s, 1, st)
    if op == "resize_bilinear":
        B, C, H, W, Ho, Wo = 2, 4, 37, 53, 50, 76
        mul = (ctypes.c_float * 2)(0.5, 3.0)
        return [_randn((B, C, H, W), seed)], [(B, C, Ho, Wo)], lambda i, o, st: lib.pivlfn_resize_bilinear(
            i[0].data_ptr(), o[0].data_ptr(), B, C, H, W, Ho, Wo, mul, st)
    raise ValueError(op)


OPS = ["corr_fwd", "corr_bwd", "backwarp", "warp_corr_fwd", "warp_corr_nhwc", "resize_bilinear"]


# ---- the entry points added since: inputs, outputs, accumulators and workspaces of any dtype --------------------------------------
# ins: host inputs;  outs: (shape, dtype) of what the call writes;  accs: host values of the buffers the call reads AND writes (acc, cnt,
# bg), pre-loaded;  ws: workspace sizes in bytes;  call(ins, outs, accs, ws, stream handle) -> return code;  pin(dev, ins, outs, accs):
# asserts the eager outputs (host tensors) against the op's CPU restatement;  hw: the image size the launchers' vector test sees.
Spec = namedtuple("Spec", "ins outs accs ws call pin hw")
F32, F64, U8, I32 = torch.float32, torch.float64, torch.uint8, torch.int32
SMALL, QUAD = (37, 53), (24, 40)                  # no multiple of anything; H*W % 4 == 0 (the vector paths)
CALIB = 0.37


def _p(t):
    return t.data_ptr() if t is not None else None


def _np(t):
    return t.cpu().numpy()


def _first(*rcs):
    """The first non-zero return code of a call sequence (every call is made, as a caller that checks afterwards would)."""
    return next((rc for rc in rcs if rc), 0)


def _assert(ok):
    assert ok


def _flows(rng, B, H, W, sigma=4.0, holes=0):
    """[B,2,H,W] float32; `holes` vectors are NaN or 1e10 in one component."""
    f = rng.normal(0, sigma, (B, 2, H, W)).astype(np.float32)
    for j in range(holes):
        f[rng.integers(0, B), j % 2, rng.integers(0, H), rng.integers(0, W)] = (np.nan, 1e10)[j // 2 % 2]
    return f


def _speckles(rng, B, H, W, value=5):
    m = (rng.random((B, H, W)) < 0.1).astype(np.uint8) * value
    m[0, H // 3:H // 2, W // 4:W // 2] = 1
    return m


def _stereo_constants():
    from pivlfn import stereo
    g = np.random.default_rng(5)
    base = np.array([1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
    coeff = {s: [float(v) for v in base + g.normal(0, 1e-3, 24)] for s in ("Left", "Right")}
    coeff["calib"] = 0.002
    return stereo.coeff_f32(coeff), stereo.tangents(*stereo.angles([30.0, 40.0], [5.0, -3.0])), (stereo.scale_factor(coeff, 0.05), 15.0)


def _spec_stereo(lib, rng, resize, quad):
    from pivlfn import stereo
    B = 2
    if resize:                                        # with mul and scale; 19 x 25 -> 50 x 31
        (h, w), (H, W) = ((12, 20), QUAD) if quad else ((19, 25), (50, 31))
    else:                                             # the input read as is, mul and scale NULL
        h, w = H, W = QUAD if quad else (37, 23)
    left, right = (rng.normal(0, 8, (B, h, w, 2)).astype(np.float32) for _ in range(2))
    flow = stereo.interleave(*(torch.from_numpy(x).permute(0, 3, 1, 2) for x in (left, right))).contiguous()
    c48, tans, scale = _stereo_constants()
    mul = (1.25, 0.8) if resize else None
    c_c, t_c = (ctypes.c_float * 48)(*c48.tolist()), (ctypes.c_double * 4)(*tans.tolist())
    m_c = (ctypes.c_float * 2)(*mul) if resize else None
    s_c = (ctypes.c_float * 2)(*scale) if resize else None

    def call(i, o, a, ws, st):
        return lib.pivlfn_stereo_2d3c(_p(i[0]), _p(o[0]), B, h, w, H, W, m_c, c_c, s_c, t_c, st)

    def pin(dev, ins, outs, accs):
        per_cam = ins[0]
        if resize:                                    # the op's own test: the restatement applied to estimate()'s resize of each camera
            from pivlfn.inference import _resize
            per_cam = _resize(ins[0].to(dev), H, W, mul=mul).cpu()
        r = _np(per_cam.permute(0, 2, 3, 1))
        assert sr.same_bits(_np(outs[0]), sr.restate(r[0::2], r[1::2], c48, tans, scale if resize else None))
    return Spec([flow], [((B, H, W, 3), F32)], [], [], call, pin, (H, W))


def _spec_fields(lib, rng, kind, f64, quad):
    from pivlfn import postpro
    B, (H, W) = 2, QUAD if quad else SMALL
    flow = _flows(rng, B, H, W)

    def call(i, o, a, ws, st):
        return lib.pivlfn_flow_fields(_p(i[0]), _p(o[0]), B, H, W, CALIB, postpro.KINDS[kind], int(f64), st)

    def pin(dev, ins, outs, accs):
        want = por.fields(flow, CALIB, kind)
        assert por.same_bits(_np(outs[0]), want if f64 else want.astype(np.float32))
    return Spec([torch.from_numpy(flow)], [((B, 3, H, W), F64 if f64 else F32)], [], [], call, pin, (H, W))


def _spec_stats(lib, rng, which, quad):
    """The three accumulating ops: acc (and cnt) hold non-zero values before the call."""
    B, (H, W) = 3, QUAD if quad else SMALL
    acc0 = np.random.default_rng(3).normal(0, 50, ({"flow": 7, "masked": 7, "error": 6}[which], H, W))
    cnt0 = np.random.default_rng(4).integers(1, 9, (2, H, W)).astype(np.float64)
    if which == "flow":
        flow = _flows(rng, B, H, W)
        return Spec([torch.from_numpy(flow)], [], [torch.from_numpy(acc0)], [],
                    lambda i, o, a, ws, st: lib.pivlfn_flow_stats_accumulate(_p(i[0]), _p(a[0]), B, H, W, CALIB, st),
                    lambda dev, ins, outs, accs: _assert(por.same_bits(_np(accs[0]), por.accumulate(acc0.copy(), flow, CALIB))), (H, W))
    if which == "masked":
        flow, flag = _flows(rng, B, H, W, holes=8), _speckles(rng, B, H, W)

        def pin(dev, ins, outs, accs):
            acc, cnt = var.accumulate_masked(acc0.copy(), cnt0.copy(), flow, flag, CALIB)
            assert por.same_bits(_np(accs[0]), acc) and np.array_equal(_np(accs[1]), cnt)
        return Spec([torch.from_numpy(flow), torch.from_numpy(flag)], [], [torch.from_numpy(acc0), torch.from_numpy(cnt0)], [],
                    lambda i, o, a, ws, st: lib.pivlfn_flow_stats_accumulate_masked(_p(i[0]), _p(i[1]), _p(a[0]), _p(a[1]), B, H, W, CALIB, st),
                    pin, (H, W))
    flow, truth, mask = _flows(rng, B, H, W, 1.0), _flows(rng, B, H, W, 3.0, holes=8), _speckles(rng, B, H, W)
    return Spec([torch.from_numpy(x) for x in (flow, truth, mask)], [], [torch.from_numpy(acc0)], [],
                lambda i, o, a, ws, st: lib.pivlfn_error_stats_accumulate(_p(i[0]), _p(i[1]), _p(i[2]), _p(a[0]), B, H, W, st),
                lambda dev, ins, outs, accs: _assert(er.same_bits(_np(accs[0]), er.accumulate_errors(acc0, flow, truth, mask))), (H, W))


def _spec_validate(lib, rng, mode, quad):
    """replace: radius 2, spacing 3, residuals -- the detect launch, then the replace launch.  flag: out and resid NULL."""
    from pivlfn import validate as V
    B, (H, W) = 2, QUAD if quad else SMALL
    flow = _flows(rng, B, H, W, 6.0, holes=12)
    r, s = (2, 3) if mode == "replace" else (1, 1)
    outs = [((B, 2, H, W), F32), ((B, H, W), U8), ((B, 2, H, W), F32)] if mode == "replace" else [((B, H, W), U8)]

    def call(i, o, a, ws, st):
        out, flag, resid = o if mode == "replace" else (None, o[0], None)
        return lib.pivlfn_flow_validate(_p(i[0]), _p(out), _p(flag), _p(resid), B, H, W, r, s, 0.1, 2.0, V.MODES[mode], st)

    def pin(dev, ins, outs, accs):
        want_out, want_flag, want_resid = var.validate(flow, r, s, 0.1, 2.0, mode)
        assert np.array_equal(_np(outs[-2] if mode == "replace" else outs[0]), want_flag)
        assert (want_flag & var.UNKNOWN).any() and (want_flag & var.OUTLIER).any()
        if mode == "replace":
            assert var.same_bits32(_np(outs[0]), want_out) and var.same_bits32(_np(outs[2]), want_resid)
    return Spec([torch.from_numpy(flow)], outs, [], [], call, pin, (H, W))


def _spec_preprocess(lib, rng, k, quad):
    """k = 7 with a background (the tiled min-max kernel) at 37 x 53; k = 0 without one at 24 x 40 (the vector path of the scale kernel)."""
    n, (H, W) = 2, QUAD if (quad or k == 0) else SMALL
    frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    bg = rng.integers(0, 160, (H, W, 3), dtype=np.uint8) if k else None
    ins = [torch.from_numpy(frames)] + ([torch.from_numpy(bg)] if k else [])
    return Spec(ins, [((n, 3, H, W), F32)], [], [],
                lambda i, o, a, ws, st: lib.pivlfn_frames_preprocess(_p(i[0]), _p(i[1]) if k else None, _p(o[0]), n, H, W, k, 16, st),
                lambda dev, ins, outs, accs: _assert(pr.same_bits32(_np(outs[0]), pr.preprocess(frames, bg, k, 16))), (H, W))


def _spec_background(lib, rng, H, W):
    n = 3
    frames = rng.integers(3, 256, (n, H, W, 3), dtype=np.uint8)
    return Spec([torch.from_numpy(frames)], [], [torch.full((H, W, 3), 255, dtype=U8)], [],
                lambda i, o, a, ws, st: lib.pivlfn_frames_background_min(_p(i[0]), _p(a[0]), n, H, W, st),
                lambda dev, ins, outs, accs: _assert(np.array_equal(_np(accs[0]), pr.background_min(frames))), (H, W))


def _spec_flow_errors(lib, rng, k, quad):
    """k = 0 at 33 x 545: 2 x 18 tiles of 32 x 32, two reduction passes over 16 x 16 node blocks, through both halves of the workspace."""
    from test_gpu_evaluate import _case
    B = 2
    H, W = (64, 96) if k else (QUAD if quad else (33, 545))
    flow, truth, mask = _case(rng, B, H, W, k)
    nws = lib.pivlfn_flow_errors_workspace_bytes(B, H, W)

    def call(i, o, a, ws, st):
        return lib.pivlfn_flow_errors(_p(i[0]), _p(i[1]), _p(i[2]), B, H, W, k, 0.2, _p(o[0]), _p(o[1]), _p(ws[0]), nws, st)

    def pin(dev, ins, outs, accs):
        want, want_map = er.flow_errors(flow, truth, mask, k, 0.2)
        assert er.same_bits(_np(outs[0]), want) and er.same_bits(_np(outs[1]), want_map)
    return Spec([torch.from_numpy(x) for x in (flow, truth, mask)], [((B, 7), F64), ((B, 3, H >> k, W >> k), F32)], [], [nws], call, pin, (H, W))


def _spec_level_errors(lib, rng):
    from test_gpu_evaluate import _case
    B, H, W = 1, 64, 96
    _, truth, mask = _case(rng, B, H, W, 0)
    levels = [[rng.normal(0, 1, (B, 2, H >> k, W >> k)).astype(np.float32) for _ in range(3)] for k in range(5, -1, -1)]
    packed = np.concatenate([f.reshape(-1) for trio in levels for f in trio])
    nws = lib.pivlfn_flow_errors_workspace_bytes(B, H, W)
    return Spec([torch.from_numpy(x) for x in (packed, truth, mask)], [((B, 6, 3, 7), F64)], [], [nws],
                lambda i, o, a, ws, st: lib.pivlfn_level_errors(_p(i[0]), 1, _p(i[1]), _p(i[2]), B, H, W, 0.2, _p(o[0]), _p(ws[0]), nws, st),
                lambda dev, ins, outs, accs: _assert(er.same_bits(_np(outs[0]), er.level_errors(levels, 1, truth, mask, 0.2))), (H, W))


def _spec_color(lib, rng, H, W):
    """pivlfn_flow_maxrad, then pivlfn_flow_to_color normalised by maxrad's device output: the chain of pivlfn/viz.py."""
    from test_gpu_viz import _holes
    B = 2
    flow, mask = _holes(rng, B, H, W)

    def call(i, o, a, ws, st):
        return _first(lib.pivlfn_flow_maxrad(_p(i[0]), _p(i[1]), _p(o[0]), B, H, W, st),
                      lib.pivlfn_flow_to_color(_p(i[0]), _p(o[0]), _p(i[1]), _p(o[1]), B, H, W, 0, 0, st))

    def pin(dev, ins, outs, accs):
        want = vzr.flow_maxrad(flow, mask)
        assert _np(outs[0]).tobytes() == want.tobytes() and want.min() > 0
        # tests/test_gpu_viz.py: the device's atan2f against NumPy's moves a byte by at most one level
        assert np.abs(_np(outs[1]).astype(int) - vzr.flow_to_color(flow, want, mask).astype(int)).max() <= 1
    return Spec([torch.from_numpy(flow), torch.from_numpy(mask)], [((B,), F32), ((B, H, W, 3), U8)], [], [], call, pin, (H, W))


def _spec_scalar(lib, rng, f64, H, W):
    """pivlfn_field_absmax and pivlfn_scalar_to_color (fixed host vmin, vmax) on one field."""
    from pivlfn import viz
    B = 2
    field = rng.normal(0, 1, (B, H, W)).astype(np.float64 if f64 else np.float32)
    field.reshape(-1)[::7] = (np.nan, np.inf, -np.inf, 1e30)[int(rng.integers(0, 4))]
    field[0, 0, 0] = -123.5
    mask, lut = (rng.random((B, H, W)) < 0.1).astype(np.uint8), viz.LUTS["bwr"]

    def call(i, o, a, ws, st):
        return _first(lib.pivlfn_field_absmax(_p(i[0]), int(f64), _p(i[1]), _p(o[0]), B, H, W, st),
                      lib.pivlfn_scalar_to_color(_p(i[0]), int(f64), _p(i[1]), _p(i[2]), _p(o[1]), B, H, W, -1.5, 1.5, 0x0A0B0C, st))

    def pin(dev, ins, outs, accs):
        assert _np(outs[0]).tobytes() == vzr.field_absmax(field, mask).tobytes()
        assert np.array_equal(_np(outs[1]), vzr.scalar_to_color(field, -1.5, 1.5, lut, mask, (10, 11, 12)))
    return Spec([torch.from_numpy(x) for x in (field, mask, lut)], [((B,), F64), ((B, H, W, 3), U8)], [], [], call, pin, (H, W))


def _spec_decimate(lib, rng, quad):
    from test_gpu_viz import _holes
    B, (H, W), cell = 2, QUAD if quad else SMALL, 5                # 37 x 53: 8 x 11 cells, the last of them ragged in both directions
    ch, cw = -(-H // cell), -(-W // cell)
    flow, mask = _holes(rng, B, H, W)

    def pin(dev, ins, outs, accs):
        want_mean, want_count = vzr.flow_decimate(flow, cell, mask)
        assert _np(outs[0]).tobytes() == want_mean.tobytes() and _np(outs[1]).tobytes() == want_count.tobytes()
    return Spec([torch.from_numpy(flow), torch.from_numpy(mask)], [((B, 2, ch, cw), F32), ((B, ch, cw), I32)], [], [],
                lambda i, o, a, ws, st: lib.pivlfn_flow_decimate(_p(i[0]), _p(i[1]), _p(o[0]), _p(o[1]), B, H, W, cell, st), pin, (H, W))


def _spec_quality(lib, seed):
    """The case of tests/test_gpu_quality.py's own stream test."""
    from test_gpu_quality import _case, _compare
    B, C, H, W, r = 2, 1, 40, 56, 8
    img1, img2, flow = _case(B, H, W, C, 700 + seed)
    mask = qr.speckle_mask(B, H, W, 19, 10)
    nws = lib.pivlfn_match_quality_workspace_bytes(B, H, W, r)

    def call(i, o, a, ws, st):
        return lib.pivlfn_match_quality(_p(i[0]), _p(i[1]), C, _p(i[2]), _p(i[3]), _p(o[0]), _p(o[1]), B, H, W, r, ((2 * r + 1) ** 2 + 1) // 2,
                                        1.0 / 255.0, _p(ws[0]), nws, st)

    def pin(dev, ins, outs, accs):
        q = _np(outs[0])
        _compare((q[:, 0], q[:, 1:], _np(outs[1])), qr.batch_quality(img1, img2, flow, r, mask), "match_quality 40x56 r=8")
    return Spec([torch.from_numpy(x) for x in (img1, img2, flow, mask)], [((B, 3, H, W), F32), ((B, H, W), U8)], [], [nws], call, pin, (H, W))


NEW_SPECS = {
    "stereo_2d3c-resize": lambda lib, rng, seed, quad: _spec_stereo(lib, rng, True, quad),
    "stereo_2d3c-same": lambda lib, rng, seed, quad: _spec_stereo(lib, rng, False, quad),
    "flow_fields-calc_vorticity-f32": lambda lib, rng, seed, quad: _spec_fields(lib, rng, "calc_vorticity", False, quad),
    "flow_fields-calc_vorticity-f64": lambda lib, rng, seed, quad: _spec_fields(lib, rng, "calc_vorticity", True, quad),
    "flow_fields-de_vort-f32": lambda lib, rng, seed, quad: _spec_fields(lib, rng, "de_vort", False, quad),
    "flow_fields-de_vort-f64": lambda lib, rng, seed, quad: _spec_fields(lib, rng, "de_vort", True, quad),
    "flow_stats_accumulate": lambda lib, rng, seed, quad: _spec_stats(lib, rng, "flow", quad),
    "flow_stats_accumulate_masked": lambda lib, rng, seed, quad: _spec_stats(lib, rng, "masked", quad),
    "error_stats_accumulate": lambda lib, rng, seed, quad: _spec_stats(lib, rng, "error", quad),
    "flow_validate-replace": lambda lib, rng, seed, quad: _spec_validate(lib, rng, "replace", quad),
    "flow_validate-flag": lambda lib, rng, seed, quad: _spec_validate(lib, rng, "flag", quad),
    "frames_preprocess-k7-bg": lambda lib, rng, seed, quad: _spec_preprocess(lib, rng, 7, quad),
    "frames_preprocess-k0": lambda lib, rng, seed, quad: _spec_preprocess(lib, rng, 0, quad),
    "frames_background_min-24x40": lambda lib, rng, seed, quad: _spec_background(lib, rng, 24, 40),
    "frames_background_min-5x3": lambda lib, rng, seed, quad: _spec_background(lib, rng, *(QUAD if quad else (5, 3))),
    "flow_errors-k0": lambda lib, rng, seed, quad: _spec_flow_errors(lib, rng, 0, quad),
    "flow_errors-k2": lambda lib, rng, seed, quad: _spec_flow_errors(lib, rng, 2, quad),
    "level_errors": lambda lib, rng, seed, quad: _spec_level_errors(lib, rng),
    "flow_maxrad+flow_to_color-37x53": lambda lib, rng, seed, quad: _spec_color(lib, rng, *(QUAD if quad else SMALL)),
    "flow_maxrad+flow_to_color-24x40": lambda lib, rng, seed, quad: _spec_color(lib, rng, *QUAD),
    "field_absmax+scalar_to_color-f32-37x53": lambda lib, rng, seed, quad: _spec_scalar(lib, rng, False, *(QUAD if quad else SMALL)),
    "field_absmax+scalar_to_color-f32-24x40": lambda lib, rng, seed, quad: _spec_scalar(lib, rng, False, *QUAD),
    "field_absmax+scalar_to_color-f64-37x53": lambda lib, rng, seed, quad: _spec_scalar(lib, rng, True, *(QUAD if quad else SMALL)),
    "field_absmax+scalar_to_color-f64-24x40": lambda lib, rng, seed, quad: _spec_scalar(lib, rng, True, *QUAD),
    "flow_decimate": lambda lib, rng, seed, quad: _spec_decimate(lib, rng, quad),
    "match_quality": lambda lib, rng, seed, quad: _spec_quality(lib, seed),
}
NEW_OPS = list(NEW_SPECS)


def _get(op, seed, quad=False):
    """The Spec of any op.  quad: the shape of the alignment test, H*W % 4 == 0 (24 x 40 where the spec's own shape is not)."""
    if op in OPS:
        ins, shapes, call = _spec(op, seed)
        return Spec(ins, [(s, F32) for s in shapes], [], [], lambda i, o, a, ws, st: call(i, o, st), None, None)
    return NEW_SPECS[op](_lib.load(), np.random.default_rng(1000 + seed), seed, quad)


# ---- buffers ------------------------------------------------------------------------------------------------------------------------
def _bytes(t):
    return t.contiguous().view(-1).view(U8)


def _same(a, b):
    """Bitwise equality of two tensors of one dtype and shape, whatever the dtype (NaNs compare by their bits)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bytes(a), _bytes(b))


def _scribble(t):
    """Every byte 0xFF: a NaN in both float types, 255, -1."""
    t.view(-1).view(U8).fill_(0xFF)
    return t


def _buf(shape, dtype, dev, fill, shift=0):
    """A `dtype` tensor `shift` elements into a guarded() allocation of whole 64-bit words, its bytes holding the guards' pattern.  The
    bytes of the allocation in front of and behind the tensor are kept for _check()."""
    es = torch.empty(0, dtype=dtype).element_size()
    nbytes, lead = es * int(np.prod(shape)), es * shift
    whole = guarded((-(-(lead + nbytes) // 8) * 8,), U8, dev, fill)
    t = whole[lead:lead + nbytes].view(dtype).view(tuple(shape))
    spare = torch.ones(whole.numel(), dtype=torch.bool, device=dev)
    spare[lead:lead + nbytes] = False
    t._guarded, t._spare = whole._guarded, (whole, spare, whole[spare].clone())
    assert t.data_ptr() % 256 == lead
    return t


def _poisoned(like, dev, shift=0):
    """An input buffer: NaN in every float element (guarded()'s words are one in float32), 0xFF in every byte of the others."""
    t = _buf(like.shape, like.dtype, dev, "nan", shift)
    if like.dtype == F64:
        t.fill_(float("nan"))
    elif like.dtype != F32:
        _scribble(t)
    return t


def _check(t, what):
    check_guards(t, what)
    whole, spare, before = t._spare
    assert torch.equal(whole[spare], before), what + ": a byte next to the tensor changed"


def _eager(op, seed, dev, quad=False):
    """The call on the current (default) stream: (device inputs, outputs, accumulators after the call, accumulators before it)."""
    spec = _get(op, seed, quad)
    d = [t.to(dev) for t in spec.ins]
    outs = [_scribble(torch.empty(s, dtype=dt, device=dev)) for s, dt in spec.outs]
    accs = [t.to(dev) for t in spec.accs]
    ws = [_scribble(torch.empty(n, dtype=U8, device=dev)) for n in spec.ws]
    _lib.check(spec.call(d, outs, accs, ws, torch.cuda.current_stream(dev).cuda_stream), op)
    torch.cuda.synchronize()
    return d, outs, accs, [t.to(dev) for t in spec.accs]


@pytest.fixture(scope="module")
def delay(dev):
    """The bounded delay: three 8192 x 8192 matrices and a side stream, once per module; the matrix product's own set-up happens here,
    not in the timed part."""
    n = 8192
    a, b, c = torch.randn(n, n, device=dev), torch.randn(n, n, device=dev), torch.empty(n, n, device=dev)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        torch.mm(a, b, out=c)
    torch.cuda.synchronize()
    return a, b, c, stream


def _start_delay(delay):
    """Inside `with torch.cuda.stream(stream)`: enqueue the chain and the event that marks its end."""
    a, b, c, stream = delay
    for _ in range(10):                                 # >= 1.1e13 flop in fp32: some tens of milliseconds
        torch.mm(a, b, out=c)
    delayed = torch.cuda.Event()
    delayed.record(stream)
    return delayed


# ---- the eager result is pinned to the CPU restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("op", NEW_OPS)
def test_eager_result_matches_the_cpu_restatement(op, dev):
    spec = _get(op, 31)
    src, outs, accs, _ = _eager(op, 31, dev)
    for t, s in zip(src, spec.ins):
        assert _same(t.cpu(), s), f"{op}: an input was written"
    spec.pin(dev, spec.ins, [t.cpu() for t in outs], [t.cpu() for t in accs])


# ---- (a) in order on the stream it is given --------------------------------------------------------------------------------------------
def _behind_the_delay(op, dev, delay, handle_of):
    """The set-up of the ordering test; handle_of(side stream) is the stream handle the call is given."""
    src, ref, ref_accs, pre = _eager(op, 31, dev)
    spec = _get(op, 31)
    ins = [_poisoned(t, dev) for t in src]
    accs = [_poisoned(t, dev) for t in pre]
    outs = [_buf(s, dt, dev, "sentinel") for s, dt in spec.outs]
    ws = [_buf((n,), U8, dev, "sentinel") for n in spec.ws]
    stream = delay[3]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        delayed = _start_delay(delay)
        for t, s in zip(ins + accs, src + pre):
            t.copy_(s, non_blocking=True)
        rc = spec.call(ins, outs, accs, ws, handle_of(stream))
        still_waiting = not delayed.query()             # the op was enqueued while the delay was still running
    _lib.check(rc, op)
    stream.synchronize()
    torch.cuda.synchronize()
    return still_waiting, outs + accs, ref + ref_accs, ins + outs + accs + ws


@pytest.mark.parametrize("op", OPS + NEW_OPS)
def test_op_runs_in_order_on_the_stream_it_is_given(op, dev, delay):
    still_waiting, got, ref, buffers = _behind_the_delay(op, dev, delay, lambda stream: stream.cuda_stream)
    assert still_waiting, "the delay ran out before the op was enqueued: the test would not see a launch on another stream"
    for g, want in zip(got, ref):
        assert _same(g, want), f"{op}: the result behind a delay on a side stream differs from the eager result"
    for t in buffers:
        _check(t, op)


def test_a_call_on_the_wrong_stream_reads_the_poison(dev, delay):
    """The same set-up with the DEFAULT stream's handle: torch's side streams do not block the default stream, so the launch does not
    wait for the copies behind the delay, reads the poison (inside its allocation) and its output differs from the eager result.  An
    ordering test that could not see a launch on another stream would pass here; this one must not."""
    op = "flow_fields-calc_vorticity-f32"
    still_waiting, got, ref, buffers = _behind_the_delay(op, dev, delay, lambda stream: torch.cuda.default_stream(dev).cuda_stream)
    assert still_waiting, "inconclusive: the delay ran out before the call was made, so the inputs may have arrived in time"
    assert not _same(got[0], ref[0]), "a call on the default stream gave the eager result: the ordering test sees no wrong stream"
    assert bool(torch.isnan(got[0]).any())
    for t in buffers:
        _check(t, op)


# ---- (b) graph capture -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS + NEW_OPS)
def test_op_is_graph_capturable(op, dev):
    first, ref_first, acc_first, pre = _eager(op, 41, dev)
    second, ref_second, acc_second, _ = _eager(op, 51, dev)
    spec = _get(op, 41)
    ins = [torch.zeros_like(t) for t in first]
    outs = [_scribble(torch.empty(s, dtype=dt, device=dev)) for s, dt in spec.outs]
    accs = [t.clone() for t in pre]
    ws = [_scribble(torch.empty(n, dtype=U8, device=dev)) for n in spec.ws]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = spec.call(ins, outs, accs, ws, torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, op)
    for src, ref in ((first, ref_first + acc_first), (second, ref_second + acc_second), (first, ref_first + acc_first)):
        for t, s in zip(ins + accs, src + pre):         # the accumulators go back to their pre-loaded values
            t.copy_(s)
        for o in outs + ws:
            _scribble(o)
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs + accs, ref):
            assert _same(got, want), f"{op}: a replay differs from the eager result"


# ---- (c) element-aligned pointers only -----------------------------------------------------------------------------------------------------
def _guarded_call(op, dev, shift):
    spec = _get(op, 61, quad=True)
    assert spec.hw[0] * spec.hw[1] % 4 == 0
    ins = [_poisoned(t, dev, shift) for t in spec.ins]
    accs = [_poisoned(t, dev, shift) for t in spec.accs]
    outs = [_buf(s, dt, dev, "sentinel", shift) for s, dt in spec.outs]
    ws = [_buf((n,), U8, dev, "sentinel") for n in spec.ws]
    for t, s in zip(ins + accs, spec.ins + spec.accs):
        t.copy_(s)
        assert t.data_ptr() % 16 == shift * t.element_size()
    _lib.check(spec.call(ins, outs, accs, ws, torch.cuda.current_stream(dev).cuda_stream), op)
    torch.cuda.synchronize()
    for t, s in zip(ins, spec.ins):
        assert _same(t.cpu(), s), f"{op}: an input was written"
    for t in ins + outs + accs + ws:
        _check(t, f"{op} shift {shift}")
    return outs + accs


@pytest.mark.parametrize("op", NEW_OPS)
def test_pointers_one_element_off_give_the_same_bits(op, dev):
    """A batch slice or a view that starts one element into an allocation: 1 byte for uint8, 4 for float32 and int32, 8 for float64."""
    want, got = _guarded_call(op, dev, 0), _guarded_call(op, dev, 1)
    for g, w in zip(got, want):
        assert _same(g, w), f"{op}: pointers one element into their allocations change the result"


# ---- the Python wrappers on a side stream ----------------------------------------------------------------------------------------------------
def _chunk_chain(frames, bg, flows, truth):
    """What run.py does to one chunk after the forward, through the Python API, all on the current stream."""
    from pivlfn import evaluate, postpro, preproc, validate, viz
    H, W = flows.shape[2:]
    x = preproc.preprocess_frames(frames, bg, 7)
    val = validate.validate_flow(flows, 2, 1, mode="replace", residual=True)
    stats = validate.MaskedFlowStats(H, W, CALIB, flows.device)
    stats.update(flows, val.flag)
    vort = postpro.flow_fields(val.flow, CALIB, "calc_vorticity", torch.float64)
    de_vort = postpro.flow_fields(val.flow, CALIB, "de_vort")
    maxrad = viz.flow_maxrad(val.flow, val.flag)
    picture = viz.flow_to_color(val.flow, mask=val.flag)
    mean, count = viz.decimate_flow(val.flow, 8, val.flag)
    err = evaluate.flow_errors(val.flow, truth, val.flag, want_map=True)
    return [x, val.flow, val.flag, val.residual, stats.acc, stats.cnt, vort, de_vort, maxrad, picture, mean, count] + list(err)


def test_wrappers_on_a_side_stream(dev, delay):
    """B = 2, 64 x 96.  The flows arrive channels-last, so the wrappers' own .contiguous() copies; their outputs and the workspace are
    allocated inside the stream context.  Every returned tensor equals the same chain run eagerly on the default stream."""
    rng = np.random.default_rng(5)
    B, H, W = 2, 64, 96
    src = [torch.from_numpy(x).to(dev) for x in (rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8), rng.integers(0, 160, (H, W, 3), dtype=np.uint8),
                                                 np.ascontiguousarray(_flows(rng, B, H, W, 3.0, holes=12).transpose(0, 2, 3, 1)),
                                                 _flows(rng, B, H, W, 3.0, holes=8))]
    want = _chunk_chain(src[0], src[1], src[2].permute(0, 3, 1, 2), src[3])
    ins = [_poisoned(t, dev) for t in src]
    stream = delay[3]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        delayed = _start_delay(delay)
        for t, s in zip(ins, src):
            t.copy_(s, non_blocking=True)
        got = _chunk_chain(ins[0], ins[1], ins[2].permute(0, 3, 1, 2), ins[3])
        still_waiting = not delayed.query()
    stream.synchronize()
    torch.cuda.synchronize()
    assert still_waiting, "the delay ran out before the chain was enqueued: the test would not see work on another stream"
    assert len(got) == len(want) == 20
    for k, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w), f"output {k} of the chain differs between a side stream and the default stream"
    assert bool((want[2] != 0).any()) and float(want[12][0]) > 0           # vectors were flagged and pixels were scored
    for t in ins:
        _check(t, "wrapper chain input")
