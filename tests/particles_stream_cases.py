"""GPU: the parts of tests/test_gpu_particles.py that use side streams and graph capture -- the stream and capture contract of
pivlfn_particles_displace and pivlfn_particles_render through the helpers of tests/test_gpu_op_streams.py: launched on the stream
they are given and on no other (behind a delay on a side stream, inputs arriving late), no allocation and no host synchronisation
(captured into a graph and replayed, displace followed by render included), pointers one element into their allocations.  Not
collected by name: tests/test_gpu_particles.py runs this file in a pytest process of its own, for the reason tests/test_gpu_flowmap.py
gives.  Also the inputs the two files share."""
import numpy as np
import pytest
import torch

import particles_restatement as prs
from test_gpu_op_streams import (F32, F64, U8, Spec, _behind_the_delay, _check, _first, _p, _same, delay)  # noqa: F401

pytestmark = pytest.mark.gpu


def field(H, W, seed, holes):
    """A smooth field of a few pixels; with `holes` a NaN, a -inf and a 1e10 vector and a mask with one byte set (two where there is room)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    a, b, c = rng.uniform(0.2, 0.9, 3)
    flow = np.stack([3.0 * np.sin(a * xx + b * yy) + 1.5, 2.0 * np.cos(c * xx - a * yy) - 0.75]).astype(np.float32)
    flow += (0.1 * rng.standard_normal(flow.shape)).astype(np.float32)
    if not holes:
        return flow, None
    mask = np.zeros((H, W), np.uint8)
    spots = rng.permutation(H * W)[:5]
    flow[0].flat[spots[0]] = np.nan
    flow[1].flat[spots[1 % len(spots)]] = -np.inf
    flow[:, spots[2 % len(spots)] // W, spots[2 % len(spots)] % W] = 1e10
    mask.flat[spots[3 % len(spots)]] = 1
    mask.flat[spots[4 % len(spots)]] = 255
    return flow, mask


def points(n, H, W, seed=0):
    """Integer nodes, the last row and column, the corners, a hair inside and outside every side, NaN, +-inf, -0.0, then random points
    in the image and a margin of 20 px round it."""
    eps = 2.0 ** -40
    fixed = [(0.0, 0.0), (W - 1.0, H - 1.0), (W - 1.0, 1.0), (1.0, H - 1.0), (W - 2.0, H - 2.0), (1.0, 1.0), (W - 1.0 + eps, 0.5),
             (0.5, H - 1.0 + eps), (-eps, 0.5), (0.5, -eps), (W - 1.0 - eps, H - 1.0 - eps), (np.nan, 1.0), (1.0, np.nan), (1.0, np.inf),
             (-np.inf, 0.5), (np.inf, -np.inf), (-0.0, 0.5), (0.25, -0.0), (-20.0, -20.0), (W + 19.0, H + 19.0)]
    rng = np.random.default_rng(1000 + seed)
    m = max(n - len(fixed), 0)
    rest = np.stack([rng.uniform(-20, W + 19, m), rng.uniform(-20, H + 19, m)], axis=1)
    return np.ascontiguousarray(np.concatenate([np.array(fixed, np.float64).reshape(-1, 2), rest])[:n].T)


def seeding(B, N, H, W, seed, margin=16):
    """pos [B,2,N] float64 over the image and its margin, diam [B,N] in [1.5, 2.5), amp [B,N] in [120, 240) float32."""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-margin, W + margin, (B, N)), rng.uniform(-margin, H + margin, (B, N))], axis=1)
    return pos, (1.5 + rng.random((B, N))).astype(np.float32), (120.0 + 120.0 * rng.random((B, N))).astype(np.float32)


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x))


# ---- the specs -------------------------------------------------------------------------------------------------------------------------
H_, W_, N_ = 24, 40, 700                                  # H*W % 4 == 0; 700 particles: three blocks of 256, the last one ragged


def _flag0(N):
    flag0 = np.zeros(N, np.uint8)
    flag0[[2, N // 2, N - 1]] = (prs.LOST, 1, prs.BAD)              # frozen beforehand: copied through
    return flag0


def _spec_displace(seed, method):
    from pivlfn import _lib
    lib = _lib.load()
    flow, mask = field(H_, W_, 4000 + seed, True)
    pos, flag0 = points(N_, H_, W_, seed), _flag0(N_)

    def call(i, o, a, ws, st):
        return lib.pivlfn_particles_displace(_p(i[0]), _p(i[1]), _p(i[2]), H_, W_, N_, method, _p(a[0]), _p(o[0]), st)

    def pin(outs, accs):
        out, flag = prs.displace(pos, flow, mask, flag0, method)
        assert prs.same_bits(outs[0].cpu().numpy(), out) and np.array_equal(accs[0].cpu().numpy(), flag)
        assert (flag == 0).sum() > N_ // 2 and (flag == prs.LOST).sum() > 1 and (flag == prs.BAD).sum() > 1 and flag[N_ // 2] == 1
    return Spec([_t(pos), _t(flow), _t(mask)], [((2, N_), F64)], [_t(flag0)], [], call, pin, (H_, W_))


def _render_inputs(seed):
    B = 2
    pos, diam, amp = seeding(B, N_, H_, W_, 5000 + seed)
    flag = (np.random.default_rng(seed).random((B, N_)) < 0.05).astype(np.uint8) * 7
    return B, pos, diam, amp, flag


def _pin_render(intensity, image, pos, diam, amp, flag, what):
    for b in range(pos.shape[0]):
        V, A, n = prs.render(pos[b], diam[b], amp[b], H_, W_, 4, flag[b])
        assert n.max() >= 10                                         # 0.3 ppp over image and margin: every pixel under several particles
        assert prs.check_render(intensity[b], image[b], V, A, n, f"{what} image {b}") < 1.0


def _spec_render(seed):
    from pivlfn import _lib
    lib = _lib.load()
    B, pos, diam, amp, flag = _render_inputs(seed)
    need = lib.pivlfn_particles_render_workspace_bytes(B, N_, H_, W_, 4)

    def call(i, o, a, ws, st):
        return lib.pivlfn_particles_render(_p(i[0]), _p(i[1]), _p(i[2]), _p(i[3]), B, N_, H_, W_, 4, _p(o[0]), _p(o[1]), _p(ws[0]), need, st)

    def pin(outs, accs):
        _pin_render(outs[0].cpu().numpy(), outs[1].cpu().numpy(), pos, diam, amp, flag, "render")
    return Spec([_t(pos), _t(diam), _t(amp), _t(flag)], [((B, H_, W_), F32), ((B, H_, W_), U8)], [], [need], call, pin, (H_, W_))


def _spec_chain(seed):
    """What create_pair_from_flow enqueues for a second frame: displace, then render the displaced particles with the displacer's flags."""
    from pivlfn import _lib
    lib = _lib.load()
    flow, mask = field(H_, W_, 6000 + seed, True)
    _, pos, diam, amp, _ = _render_inputs(100 + seed)
    pos, diam, amp, flag0 = pos[0], diam[0], amp[0], _flag0(N_)
    need = lib.pivlfn_particles_render_workspace_bytes(1, N_, H_, W_, 4)

    def call(i, o, a, ws, st):
        return _first(lib.pivlfn_particles_displace(_p(i[0]), _p(i[1]), _p(i[2]), H_, W_, N_, 1, _p(a[0]), _p(o[0]), st),
                      lib.pivlfn_particles_render(_p(o[0]), _p(i[3]), _p(i[4]), _p(a[0]), 1, N_, H_, W_, 4, _p(o[1]), _p(o[2]), _p(ws[0]), need, st))

    def pin(outs, accs):
        out, flag = prs.displace(pos, flow, mask, flag0, 1)
        assert prs.same_bits(outs[0].cpu().numpy(), out) and np.array_equal(accs[0].cpu().numpy(), flag) and (flag == prs.LOST).sum() > 1
        _pin_render(outs[1].cpu().numpy(), outs[2].cpu().numpy(), out[None], diam[None], amp[None], flag[None], "displace -> render")
    return Spec([_t(pos), _t(flow), _t(mask), _t(diam), _t(amp)], [((2, N_), F64), ((1, H_, W_), F32), ((1, H_, W_), U8)], [_t(flag0)], [need],
                call, pin, (H_, W_))


SPECS = {"particles_displace-bilinear": lambda seed: _spec_displace(seed, 0), "particles_displace-cubic": lambda seed: _spec_displace(seed, 1),
         "particles_render": _spec_render, "particles_displace->render": _spec_chain}
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
    """On a side stream behind a long-running chain of matrix products and the copies of the real inputs and the real flags into
    poisoned buffers, enqueued without a host synchronisation: the eager result, bit for bit, and every guard intact.  A launch on
    the default stream -- any of the renderer's five -- would read the poison or find the counters not yet cleared."""
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
