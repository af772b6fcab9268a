"""GPU: the stream and capture contract of pivlfn_template_match, pivlfn_target_points and pivlfn_dewarp_frames through the helpers of
tests/test_gpu_op_streams.py: launched on the stream they are given and on no other (behind a delay on a side stream, inputs arriving
late in poisoned staging), no allocation and no host synchronisation (captured into a graph and replayed with two input sets, the
workspace scribbled), pointers one element into their allocations.  Not collected by name: tests/test_gpu_calibrate.py runs this file in
a pytest process of its own, for the reason tests/test_gpu_flowmap.py gives."""
import ctypes

import numpy as np
import pytest
import torch

import calibrate_restatement as cr
from test_gpu_op_streams import (F32, I32, U8, Spec, _behind_the_delay, _check, _p, _same, delay)  # noqa: F401

pytestmark = pytest.mark.gpu

I64 = torch.int64
H_, W_, B_ = 24, 72, 2                                    # H*W % 4 == 0; two tiles along x, three along y, seven labelling blocks
CAP = 6


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def blobs(rng, B, H, W, n):
    """A correlation-like float32 map: n small blobs per image (image b gets n + 5 b of them) on a background below the threshold."""
    r = (0.5 * rng.random((B, H, W))).astype(np.float32)
    for b in range(B):
        for _ in range(n + 5 * b):
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            r[b, y:y + int(rng.integers(1, 4)), x:x + int(rng.integers(1, 4))] = np.float32(0.71 + 0.29 * rng.random())
    return r


def mapping(rng, H, W):
    """Coefficients that send part of the image outside, with all 24 terms in play."""
    A = np.zeros(24)
    A[0:6] = (1.15, 0.04, -3.0 + rng.random(), 2e-4, -1e-4, 3e-4)
    A[6:12] = (4e-4, -3e-4, 1.0, 1e-6, 2e-6, -1e-6)
    A[12:18] = (-0.05, 1.2, 2.0 + rng.random(), 1e-4, 2e-4, -2e-4)
    A[18:24] = (-2e-4, 5e-4, 1.0, -1e-6, 1e-6, 2e-6)
    return A, (W / 2.0 + 0.25, H / 2.0 - 0.5)


def _spec_match(seed):
    from pivlfn import _lib
    lib = _lib.load()
    rng = np.random.default_rng(7000 + seed)
    images = rng.integers(0, 256, (B_, H_, W_), dtype=np.uint8)
    templ = rng.integers(0, 256, (5, 7), dtype=np.uint8)
    need = lib.pivlfn_template_match_workspace_bytes(5, 7)

    def call(i, o, a, ws, st):
        return lib.pivlfn_template_match(_p(i[0]), _p(i[1]), _p(o[0]), B_, H_, W_, 5, 7, _p(ws[0]), need, st)

    def pin(outs, accs):
        assert cr.same_bits(outs[0].cpu().numpy(), cr.template_match(images, templ))
    return Spec([_t(images), _t(templ)], [((B_, H_, W_), F32)], [], [need], call, pin, (H_, W_))


def _spec_points(seed):
    from pivlfn import _lib
    lib = _lib.load()
    r = blobs(np.random.default_rng(8000 + seed), B_, H_, W_, 4)
    need = lib.pivlfn_target_points_workspace_bytes(B_, H_, W_)

    def call(i, o, a, ws, st):
        return lib.pivlfn_target_points(_p(i[0]), B_, H_, W_, 0.7, CAP, _p(o[0]), _p(o[1]), _p(o[2]), _p(ws[0]), need, st)

    def pin(outs, accs):
        labels, count, rec = cr.target_points(r, 0.7, CAP)
        assert count[0] >= 2 and count[1] > CAP                                  # one image overflows the records
        for got, want in zip(outs, (labels, count, rec)):
            assert cr.same_bits(got.cpu().numpy(), want)
    return Spec([_t(r)], [((B_, H_, W_), I32), ((B_,), I32), ((B_, CAP, 4), I64)], [], [need], call, pin, (H_, W_))


def _spec_dewarp(seed, f32, mode):
    from pivlfn import _lib
    lib = _lib.load()
    rng = np.random.default_rng(9000 + seed)
    frames = rng.standard_normal((B_, H_, W_)).astype(np.float32) if f32 else rng.integers(0, 256, (B_, H_, W_), dtype=np.uint8)
    A, origin = mapping(np.random.default_rng(0), H_, W_)       # host arguments: read when the call is made, the same for every seed
    a_c = (ctypes.c_double * 24)(*A.tolist())
    fill = -1.5 if f32 else 9.0

    def call(i, o, a, ws, st):
        return lib.pivlfn_dewarp_frames(_p(i[0]), _p(o[0]), int(f32), B_, H_, W_, a_c, origin[0], origin[1], mode, fill, st)

    def pin(outs, accs):
        want = cr.dewarp(frames, A, origin, ("nearest", "bilinear")[mode], fill)
        assert cr.same_bits(outs[0].cpu().numpy(), want)
        assert 0.1 < (want == want.dtype.type(fill)).mean() < 0.9                 # part of the image maps outside
    return Spec([_t(frames)], [((B_, H_, W_), F32 if f32 else U8)], [], [], call, pin, (H_, W_))


SPECS = {"template_match": _spec_match, "target_points": _spec_points,
         "dewarp_frames-u8-nearest": lambda seed: _spec_dewarp(seed, False, 0),
         "dewarp_frames-f32-bilinear": lambda seed: _spec_dewarp(seed, True, 1)}
OPS = list(SPECS)


@pytest.fixture()
def as_an_op(monkeypatch):
    """The helpers of test_gpu_op_streams look an op up by name: the names above resolve to the specs above."""
    import test_gpu_op_streams as ops
    original = ops._get
    monkeypatch.setattr(ops, "_get", lambda op, seed, quad=False: SPECS[op](seed) if op in SPECS else original(op, seed, quad))
    return ops


@pytest.mark.parametrize("op", OPS)
def test_eager_result_is_the_restatements(op, dev, as_an_op):
    src, outs, accs, _ = as_an_op._eager(op, 31, dev)
    spec = SPECS[op](31)
    for t, s in zip(src, spec.ins):
        assert _same(t.cpu(), s), f"{op}: an input was written"
    spec.pin(outs, accs)


@pytest.mark.parametrize("op", OPS)
def test_runs_in_order_on_the_stream_it_is_given(op, dev, delay, as_an_op):        # noqa: F811
    """On a side stream behind a long-running chain of matrix products and the copies of the real inputs into poisoned buffers,
    enqueued without a host synchronisation: the eager result, bit for bit, and every guard intact.  A launch on the default stream --
    any of target_points' six -- would read the poison or find the labels not yet written."""
    still_waiting, got, ref, buffers = _behind_the_delay(op, dev, delay, lambda stream: stream.cuda_stream)
    assert still_waiting, "the delay ran out before the op was enqueued: the test would not see a launch on another stream"
    for g, want in zip(got, ref):
        assert _same(g, want), f"{op}: the result behind a delay on a side stream differs from the eager result"
    for t in buffers:
        _check(t, op)


@pytest.mark.parametrize("op", OPS)
def test_is_graph_capturable(op, dev, as_an_op):
    """Captured and replayed three times with two input sets and a scribbled workspace: the eager bits.  An allocation or a host
    synchronisation inside the call would be a capture error."""
    as_an_op.test_op_is_graph_capturable(op, dev)


@pytest.mark.parametrize("op", OPS)
def test_pointers_one_element_off_give_the_same_bits(op, dev, as_an_op):
    as_an_op.test_pointers_one_element_off_give_the_same_bits(op, dev)
