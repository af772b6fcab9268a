"""GPU: pivlfn_ensemble_corr (csrc/ensemble.hip) against the NumPy restatement of its contract (tests/ensemble_restatement.py) and the
Python layer on top (pivlfn.ensemble.EnsembleCorrelation).

The contract is exact (integer sums), so everything is compared with torch.equal, in guarded buffers.  Through ctypes the sums are
pre-filled with random int64: the result is the pre-fill plus the restatement, and OUTSIDE windows keep the pre-fill.  Shapes are the
smallest that reach every path: exactly one window; a frame with a remainder; a window that is no multiple of 8 (an odd count of
dwords per row) with a search that is no multiple of 4 (every realignment shift); a step larger than the window; the largest LDS
footprint, where a window's items fill three workgroups and the last one partly; the kernels of their own that windows of 16, 32
(the accuracy cases) and 64 pixels have; displacement planes whose last group of four rows has one, two (search 1, 3) or three rows;
sums past 2^32 across frames; windows pushed out of the frame on each side.  Frames of odd width (and, in the stream cases, one byte off) reach
every alignment of a staged row.  Everything here runs on the default stream; the stream and capture contract and run.py are in
tests/ensemble_stream_cases.py, which one test runs in a process of its own."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ensemble_restatement as er
from pivlfn import _lib
from pivlfn import ensemble as E
from test_gpu_op_streams import I32, U8, _buf, _check, _p

pytestmark = pytest.mark.gpu

I64 = torch.int64


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _call(dev, a, b, window, step, search, offset=None, seed=0):
    """The entry point on guarded buffers with pre-filled sums -> (sums, sums_a, pre-fill of sums, pre-fill of sums_a), host arrays."""
    lib = _lib.load()
    B, H, W = a.shape
    ny, nx = er.grid(H, W, window, step, search)
    P = 2 * search + 1
    rng = np.random.default_rng(seed)
    pre, pre_a = rng.integers(-2 ** 40, 2 ** 40, (ny, nx, P, P, 3)), rng.integers(-2 ** 40, 2 ** 40, (ny, nx, 2))
    host = [a, b] + ([offset] if offset is not None else []) + [pre, pre_a]
    bufs = [_buf(x.shape, _t(x).dtype, dev, "nan") for x in host]
    for t, x in zip(bufs, host):
        t.copy_(_t(x))
    off = bufs[2] if offset is not None else None
    _lib.check(lib.pivlfn_ensemble_corr(_p(bufs[0]), _p(bufs[1]), _p(off), _p(bufs[-2]), _p(bufs[-1]), B, H, W, window, step, search,
                                        torch.cuda.current_stream(dev).cuda_stream), "ensemble_corr")
    torch.cuda.synchronize()
    for t in bufs:
        _check(t, f"ensemble_corr {H}x{W} window {window}")
    assert torch.equal(bufs[0].cpu(), _t(a)) and torch.equal(bufs[1].cpu(), _t(b)), "an input was written"
    return bufs[-2].cpu().numpy(), bufs[-1].cpu().numpy(), pre, pre_a


def _compare(dev, a, b, window, step, search, offset=None):
    got, got_a, pre, pre_a = _call(dev, a, b, window, step, search, offset)
    want, want_a = er.ensemble_corr(a, b, window, step, search, offset, pre, pre_a)
    assert torch.equal(_t(got), _t(want)) and torch.equal(_t(got_a), _t(want_a))
    return got, got_a, pre, pre_a


def _frames(seed, B, H, W):
    return np.random.default_rng(seed).integers(0, 256, (2, B, H, W), dtype=np.uint8)


@pytest.mark.parametrize("H,W,B,window,step,search", [
    (10, 10, 2, 8, 1, 1),             # exactly one window
    (11, 13, 2, 8, 1, 1),             # 2 x 4 windows, one pixel apart
    (37, 53, 3, 12, 5, 3),            # three dwords per row, shifts 0..3 of the realignment, a remainder both ways
    (40, 45, 2, 8, 11, 2),            # a step larger than the window: pixels between the windows belong to none
    (192, 192, 1, 128, 32, 32),       # the largest LDS footprint; 17 row groups x 65 = 1105 items in three blocks of 512, the last partly empty
    (49, 52, 2, 16, 7, 9),            # the kernel of window 16; 19 displacement rows: the last group of four has three
    (70, 75, 1, 64, 3, 2),            # the kernel of window 64
    (46, 50, 2, 20, 3, 12),           # 7 row groups x 25 = 175 items: a block of 192 lanes, the last group has one row
])
def test_sums_are_the_restatements(dev, H, W, B, window, step, search):
    a, b = _frames(H * W + window, B, H, W)
    _compare(dev, a, b, window, step, search)


def test_sums_past_32_bits_across_frames(dev):
    """Window 128, search 1 at 130 x 130, five frames of 255: every sum of squares is 5 * 255^2 * 128^2 = 5 326 848 000 > 2^32."""
    a = np.full((5, 130, 130), 255, np.uint8)
    got, got_a, pre, pre_a = _compare(dev, a, a, 128, 1, 1)
    assert ((got - pre)[..., 1:] == 5 * 255 ** 2 * 128 ** 2).all() and ((got_a - pre_a)[..., 1] == 5326848000).all()


def test_random_offsets_and_outside_windows_keep_the_prefill(dev):
    H, W, window, step, search = 37, 53, 12, 5, 3
    a, b = _frames(3, 2, H, W)
    ny, nx = er.grid(H, W, window, step, search)
    offset = np.random.default_rng(4).integers(-5, 6, (2, ny, nx)).astype(np.int32)
    offset[1, 0, 2], offset[1, -1, 3], offset[0, 1, 0], offset[0, 2, -1] = -1, 5, -1, 1             # one pixel over each side
    out = er.outside(H, W, window, step, search, offset)
    assert out[0].any() and out[-1].any() and out[:, 0].any() and out[:, -1].any() and not out[1:-1, 1:-1].any()       # each side
    got, got_a, pre, pre_a = _compare(dev, a, b, window, step, search, offset)
    assert np.array_equal(got[out], pre[out]) and np.array_equal(got_a[out], pre_a[out])
    assert (got[~out] != pre[~out]).any(-1).all()
    far = offset.copy()
    far[:, 0, 0], far[:, 1, 1] = (2 ** 31 - 1, -2 ** 31), (-2 ** 31, 2 ** 31 - 1)                  # the rule in 64 bits: no wrap-around
    _compare(dev, a, b, window, step, search, far)


def test_updates_add_up_and_a_frame_alone_is_a_frame_in_a_batch(dev):
    H, W = 37, 53
    a, b = (_t(x).to(dev) for x in _frames(5, 5, H, W))
    ny, nx = er.grid(H, W, 12, 5, 3)
    offset = np.random.default_rng(4).integers(-2, 3, (2, ny, nx)).astype(np.int32)

    def make():
        return E.EnsembleCorrelation(H, W, 12, 5, 3, offset=offset, device=dev)
    whole, parts, single = make(), make(), make()
    whole.update(a, b)
    parts.update(a[:2], b[:2])
    parts.update(a[:0], b[:0])                                          # no frame: nothing happens
    parts.update(a[2:], b[2:])
    for k in range(5):
        single.update(a[k:k + 1], b[k:k + 1])
    want, want_a = er.ensemble_corr(a.cpu().numpy(), b.cpu().numpy(), 12, 5, 3, offset)
    for acc in (whole, parts, single):
        assert acc.count == 5 and torch.equal(acc.sums.cpu(), _t(want)) and torch.equal(acc.sums_a.cpu(), _t(want_a))
    assert whole.sums.shape == (ny, nx, 7, 7, 3) and whole.sums_a.shape == (ny, nx, 2) and whole.sums.dtype == I64
    assert np.array_equal(whole.outside, er.outside(H, W, 12, 5, 3, offset)) and (whole.ny, whole.nx) == (ny, nx)
    x, y = whole.centres()
    assert x.tolist() == [3 + 5 * i + 5.5 for i in range(nx)] and y.tolist() == [3 + 5 * j + 5.5 for j in range(ny)]


@pytest.mark.parametrize("C", [0, 1, 3])
def test_float_frames_on_all_256_table_values(dev, C):
    """float32 frames holding the pipeline's table k/255 (float32, k = 0..255), as [B,H,W] (C = 0), [B,1,H,W] and [B,3,H,W]: the sums of
    the bytes k."""
    k = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    a8, b8 = np.concatenate([k, k[:, ::-1]]), np.concatenate([k.transpose(0, 2, 1), k[:, :, ::-1]])
    table = torch.arange(256, dtype=torch.float32) / 255.0

    def as_float(x):
        f = table[_t(x).long()]
        return (f if C == 0 else f[:, None].expand(-1, C, -1, -1)).to(dev)
    acc = E.EnsembleCorrelation(16, 16, 8, 2, 2, device=dev)
    acc.update(as_float(a8), as_float(b8))
    want, want_a = er.ensemble_corr(a8, b8, 8, 2, 2)
    assert torch.equal(acc.sums.cpu(), _t(want)) and torch.equal(acc.sums_a.cpu(), _t(want_a))
    assert torch.equal(E._as_bytes(as_float(a8), "a", "test").cpu(), _t(a8))
    if C == 0:                                                          # out of [0, 1]: clamped
        assert E._as_bytes(torch.tensor([[[-0.3, 1.7, 0.5]]], device=dev), "a", "test").cpu().tolist() == [[[0, 255, 128]]]


@pytest.mark.parametrize("k", [0, 1, 2])
def test_result_is_finalize_of_the_restatements_sums(dev, k):
    """The accuracy cases of tests/test_ensemble.py on the device: the same sums, so the same result bit for bit -- and with it the
    same errors, flags and ratios that file asserts."""
    n, uv, window, step, search, _ = er.ACCURACY[k]
    a, b, offset, sums, sums_a = er.accuracy_case(k)
    acc = E.EnsembleCorrelation(er.ACC_H, er.ACC_W, window, step, search, offset=offset, device=dev)
    acc.update(_t(a.copy()).to(dev), _t(b.copy()).to(dev))
    assert torch.equal(acc.sums.cpu(), _t(sums.copy())) and torch.equal(acc.sums_a.cpu(), _t(sums_a.copy()))
    got = acc.result()
    want = E.finalize(sums, sums_a, n, window, step, offset, er.outside(er.ACC_H, er.ACC_W, window, step, search, offset))
    for name in ("corr", "displacement", "height", "ratio", "flag", "outside"):
        assert np.array_equal(getattr(got, name), getattr(want, name), equal_nan=True), name
    assert got.frames == n and np.nanmax(np.abs(got.displacement - np.array(uv)[:, None, None])) < 0.04


def test_every_err_arg_case_leaves_the_sums_untouched(dev):
    lib = _lib.load()
    B, H, W, window, step, search = 2, 37, 53, 12, 5, 3
    ny, nx = er.grid(H, W, window, step, search)
    a, b = (_t(x).to(dev) for x in _frames(9, B, H, W))
    offset = torch.zeros(2, ny, nx, dtype=I32, device=dev)
    sums = torch.randint(-2 ** 40, 2 ** 40, (ny, nx, 7, 7, 3), dtype=I64, device=dev)
    sums_a = torch.randint(-2 ** 40, 2 ** 40, (ny, nx, 2), dtype=I64, device=dev)
    before, before_a = sums.clone(), sums_a.clone()
    st = torch.cuda.current_stream(dev).cuda_stream
    for label, args, word in er.err_arg_cases(_p(a), _p(b), _p(offset), _p(sums), _p(sums_a), B, H, W, window, step, search):
        rc = lib.pivlfn_ensemble_corr(*args, st)
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1 and word in msg, (label, rc, msg)
    assert lib.pivlfn_ensemble_corr(_p(a), _p(b), _p(offset), _p(sums), _p(sums_a), 0, H, W, window, step, search, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(sums, before) and torch.equal(sums_a, before_a)


def test_update_refusals(dev):
    acc = E.EnsembleCorrelation(20, 24, 8, 4, 2, device=dev)
    ok = torch.zeros(2, 20, 24, dtype=U8, device=dev)
    for bad_a, bad_b, kind, words in (
            (torch.zeros(2, 20, 25, dtype=U8, device=dev), ok, ValueError, "frames (2, 20, 25) on cuda:0, accumulators for [20,24] on cuda:0"),
            (ok, torch.zeros(3, 20, 24, dtype=U8, device=dev), ValueError, "second frames (3, 20, 24) on cuda:0 beside (2, 20, 24)"),
            (ok, torch.zeros(2, 2, 20, 24, device=dev), ValueError, "C = 1 or 3 for b, got (2, 2, 20, 24)"),
            (ok.cpu(), ok, NotImplementedError, "GPU tensors only"),
            (ok.to(torch.int32), ok, TypeError, "for a, got torch.int32"),
            (ok[0], ok, ValueError, "expected uint8 frames [B,H,W] for a, got (20, 24)")):
        with pytest.raises(kind, match=re.escape(words)):
            acc.update(bad_a, bad_b)
    assert acc.count == 0 and not bool(acc.sums.any())
    with pytest.raises(ValueError, match=re.escape("offset (2, 1, 1), expected [2,3,4]")):
        E.EnsembleCorrelation(20, 24, 8, 4, 2, offset=np.zeros((2, 1, 1), np.int32), device=dev)


# ---- side streams, graph capture and run.py: in a process of their own ----------------------------------------------------------------------------
def test_stream_contract_and_run_py_in_a_process_of_their_own(dev):
    """tests/ensemble_stream_cases.py in a fresh pytest process: 9 tests, all passing.  Why not in this process:
    tests/test_gpu_flowmap.py::test_stream_contract_and_run_py_in_a_process_of_their_own says it."""
    here = os.path.dirname(os.path.abspath(__file__))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                                                                          os.path.join(here, "ensemble_stream_cases.py")]
    r = subprocess.run(cmd, cwd=here, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and re.search(r"\b9 passed", r.stdout), r.stdout[-6000:] + r.stderr[-2000:]
