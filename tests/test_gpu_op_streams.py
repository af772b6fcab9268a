"""GPU: the six public op entry points honour the stream they are given.  run.py and pivlfn/sequence.py call them next to a copy
stream; every other test calls them on the current default stream, where a launch on the wrong stream or a hidden host
synchronisation cannot be seen.

Ordering: on a fresh stream, behind a bounded delay (a chain of matrix products, some tens of milliseconds) and the copy of the real
inputs into buffers that hold the NaN poison, the op is enqueued without any host synchronisation; its output, pre-filled with the
sentinel, equals the eager default-stream result bit for bit.  A launch on another stream reads the poison or leaves the sentinel.
Capture: the call is captured into a graph (buffers allocated before the capture) and replayed twice with different inputs; each
replay equals the eager result bit for bit -- which holds the header's "nothing here allocates per call" and the absence of a host
synchronisation for these ops (a violation is a capture error)."""
import ctypes

import pytest
import torch

from guarded import check_guards, guarded, same_bits
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


def _eager(op, seed, dev):
    ins, shapes, call = _spec(op, seed)
    d = [t.to(dev) for t in ins]
    outs = [torch.full(s, float("nan"), device=dev) for s in shapes]
    _lib.check(call(d, outs, torch.cuda.current_stream(dev).cuda_stream), op)
    torch.cuda.synchronize()
    return d, outs


@pytest.mark.parametrize("op", OPS)
def test_op_runs_in_order_on_the_stream_it_is_given(op, dev):
    src, ref = _eager(op, 31, dev)
    _, shapes, call = _spec(op, 31)
    ins = [guarded(t.shape, torch.float32, dev, "nan") for t in src]
    outs = [guarded(s, torch.float32, dev, "sentinel") for s in shapes]
    n = 8192
    a, b, c = torch.randn(n, n, device=dev), torch.randn(n, n, device=dev), torch.empty(n, n, device=dev)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        torch.mm(a, b, out=c)                           # the matrix product's own set-up happens here, not in the timed part
    torch.cuda.synchronize()
    delayed = torch.cuda.Event()
    with torch.cuda.stream(stream):
        for _ in range(10):                             # >= 1.1e13 flop in fp32: some tens of milliseconds
            torch.mm(a, b, out=c)
        delayed.record(stream)
        for t, s in zip(ins, src):
            t.copy_(s, non_blocking=True)
        rc = call(ins, outs, stream.cuda_stream)
        still_waiting = not delayed.query()             # the op was enqueued while the delay was still running
    _lib.check(rc, op)
    stream.synchronize()
    assert still_waiting, "the delay ran out before the op was enqueued: the test would not see a launch on another stream"
    for got, want in zip(outs, ref):
        assert same_bits(got, want), f"{op}: the result behind a delay on a side stream differs from the eager result"
    for t in ins + outs:
        check_guards(t, op)


@pytest.mark.parametrize("op", OPS)
def test_op_is_graph_capturable(op, dev):
    first, ref_first = _eager(op, 41, dev)
    second, ref_second = _eager(op, 51, dev)
    _, shapes, call = _spec(op, 41)
    ins = [torch.zeros_like(t) for t in first]
    outs = [torch.full(s, float("nan"), device=dev) for s in shapes]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = call(ins, outs, torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, op)
    for src, ref in ((first, ref_first), (second, ref_second), (first, ref_first)):
        for t, s in zip(ins, src):
            t.copy_(s)
        for o in outs:
            o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, ref):
            assert same_bits(got, want), f"{op}: a replay differs from the eager result"
