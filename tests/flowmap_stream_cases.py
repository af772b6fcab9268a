"""GPU: the parts of tests/test_gpu_flowmap.py that use side streams, graph capture and run.py -- the stream and capture contract of
pivlfn_flowmap_advect, pivlfn_flowmap_seed and pivlfn_flowmap_ftle through the helpers of tests/test_gpu_op_streams.py, and run.py
--ftle.  Not collected by name: tests/test_gpu_flowmap.py runs this file in a pytest process of its own and says why.  Also the inputs
the two files share."""
import json

import numpy as np
import pytest
import torch

import flowmap_restatement as fr
from flowmap_restatement import LOST, OUT, UNDEFINED
from test_gpu_op_streams import (F64, U8, Spec, _behind_the_delay, _buf, _check, _p, _poisoned, _same, _scribble, delay)  # noqa: F401

pytestmark = pytest.mark.gpu

B = 7


def _t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _fields(H, W, holes, seed=11):
    rng = np.random.default_rng(seed)
    flows = fr.plane_waves(rng, B, H, W)
    return fr.with_holes(rng, flows, 0.02 if H * W < 100 else 0.01) if holes else (flows, None)


# ---- the stream and capture contract, with the helpers of tests/test_gpu_op_streams.py ------------------------------------------------
def _state(H, W, spacing):
    """The in-place state the specs pre-load, the same for every seed: the seeds, three of them frozen beforehand."""
    pos0, h, w = fr.lattice(H, W, spacing)
    flag0 = np.zeros(h * w, np.uint8)
    flag0[[1, h * w // 2, h * w - 1]] = (OUT, LOST, OUT | LOST)
    return pos0, flag0, h, w


def _spec_advect(seed, backward):
    """7 x 24 x 40 (H*W % 4 == 0) with holes and a mask, spacing 1: 960 particles, a trace; pos and flag are read AND written."""
    from pivlfn import _lib
    lib = _lib.load()
    H, W = 24, 40
    flows, mask = _fields(H, W, True, seed=3000 + seed)
    pos0, flag0, h, w = _state(H, W, 1)
    N = h * w

    def call(i, o, a, ws, st):
        return lib.pivlfn_flowmap_advect(_p(i[0]), _p(i[1]), B, H, W, _p(a[0]), _p(a[1]), N, int(backward), 4, _p(o[0]), st)

    def pin(outs, accs):
        pos, flag, path = fr.advect(flows, mask, pos0, flag0, backward=backward, iters=4, trace=True)
        assert fr.same_bits(accs[0].cpu().numpy(), pos) and np.array_equal(accs[1].cpu().numpy(), flag) and fr.same_bits(outs[0].cpu().numpy(), path)
        assert (flag == 0).any() and (flag[[1, N // 2, N - 1]] == flag0[[1, N // 2, N - 1]]).all()
        assert fr.same_bits(pos[:, [1, N // 2, N - 1]], pos0[:, [1, N // 2, N - 1]])               # what was frozen stays
    return Spec([torch.from_numpy(flows), torch.from_numpy(mask)], [((B, 2, N), F64)], [torch.from_numpy(pos0), torch.from_numpy(flag0)], [],
                call, pin, (H, W))


def _spec_ftle(seed):
    """The lattice 24 x 40 at spacing 2 after seven fields: 12 x 20 nodes."""
    from pivlfn import _lib
    lib = _lib.load()
    H, W, s = 24, 40, 2
    flows, mask = _fields(H, W, True, seed=3100 + seed)
    pos0, flag0, h, w = _state(H, W, s)
    pos, flag = fr.advect(flows, mask, pos0, flag0)

    def call(i, o, a, ws, st):
        return lib.pivlfn_flowmap_ftle(_p(i[0]), _p(i[1]), h, w, s, _p(o[0]), _p(o[1]), st)

    def pin(outs, accs):
        stretch, oflag = fr.ftle_stretch(pos, flag, h, w, s)
        assert fr.same_bits(outs[0].cpu().numpy(), stretch) and np.array_equal(outs[1].cpu().numpy(), oflag)
        assert (oflag & UNDEFINED).any() and not (oflag & UNDEFINED).all()
    return Spec([torch.from_numpy(pos), torch.from_numpy(flag)], [((h, w), F64), ((h, w), U8)], [], [], call, pin, (h, w))


def _spec_seed(seed):
    from pivlfn import _lib
    lib = _lib.load()
    h, w, s = 12, 20, 3

    def call(i, o, a, ws, st):
        return lib.pivlfn_flowmap_seed(_p(o[0]), _p(o[1]), h, w, s, st)

    def pin(outs, accs):
        pos0, hh, ww = fr.lattice((h - 1) * s + 1, (w - 1) * s + 1, s)
        assert (hh, ww) == (h, w) and fr.same_bits(outs[0].cpu().numpy(), pos0) and not outs[1].any()
    return Spec([], [((2, h * w), F64), ((h * w,), U8)], [], [], call, pin, (h, w))


SPECS = {"flowmap_advect": lambda seed: _spec_advect(seed, False), "flowmap_advect-backward": lambda seed: _spec_advect(seed, True),
         "flowmap_ftle": _spec_ftle, "flowmap_seed": _spec_seed}
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
    """On a side stream behind a long-running chain of matrix products and the copies of the real inputs and the real state into
    poisoned buffers, enqueued without a host synchronisation: the eager result, bit for bit, and every guard intact."""
    still_waiting, got, ref, buffers = _behind_the_delay(op, dev, delay, lambda stream: stream.cuda_stream)
    assert still_waiting, "the delay ran out before the op was enqueued: the test would not see a launch on another stream"
    for g, want in zip(got, ref):
        assert _same(g, want), f"{op}: the result behind a delay on a side stream differs from the eager result"
    for t in buffers:
        _check(t, op)


@pytest.mark.parametrize("op", OPS)
def test_is_graph_capturable(op, dev, as_an_op):
    as_an_op.test_op_is_graph_capturable(op, dev)


@pytest.mark.parametrize("op", OPS)
def test_pointers_one_element_off_give_the_same_bits(op, dev, as_an_op):
    as_an_op.test_pointers_one_element_off_give_the_same_bits(op, dev)


# ---- run.py --------------------------------------------------------------------------------------------------------------------------
def test_run_py_ftle(tmp_path, dev):
    """run.py --ftle 2 --ftle-steps 3 --ftle-image --validate flag on a synthetic sequence of nine 64 x 64 frames, --batch 4: eight
    pairs, two windows of three -- the second batch straddles the end of the second window -- and two pairs left over.  Every
    <first pair>_ftle.flo holds the two bands of FlowMap run over the written flows with the validation flags as the mask, bit for bit;
    ftle.json holds the summaries; the PNGs have the lattice's size.  Without --ftle no such file appears, args.txt does not mention
    it, and the .flo files are the same bytes."""
    import PIL.Image
    import run as runpy
    import pivlfn
    from pivlfn import synth
    from pivlfn import validate as V
    from pivlfn.flo import read_flow
    H = W = 64
    seq = tmp_path / "seq"
    seq.mkdir()
    frames = synth.ParticleSequence(H, W, seed=77, peak=2.0, shift=(0.5, -0.25)).frames(0, 9).numpy()
    names = [f"f{k:03d}" for k in range(9)]
    for name, frame in zip(names, frames):
        PIL.Image.fromarray(frame).save(str(seq / f"{name}.png"))
    base = ["--model", "piv", "-i", str(seq), "--batch", "4", "--validate", "flag", "--validate-radius", "2", "--validate-eps", "0.01",
            "--validate-thresh", "0.5"]
    assert runpy.main(base + ["-o", str(tmp_path / "plain")]) == 8
    assert runpy.main(base + ["-o", str(tmp_path / "ftle"), "--ftle", "2", "--ftle-steps", "3", "--ftle-image"]) == 8
    plain, out = (tmp_path / d / "piv-synthetic" / "seq" for d in ("plain", "ftle"))
    assert not list(plain.rglob("*ftle*"))
    assert not [ln for ln in open(plain / "args.txt") if ln.startswith("ftle")]
    lines = list(open(out / "args.txt"))
    assert "ftle: 2\n" in lines and "ftle_steps: 3\n" in lines and "ftle_image: True\n" in lines and "ftle_max: None\n" in lines
    for n in names[:8]:
        assert open(out / "flow" / f"{n}_out.flo", "rb").read() == open(plain / "flow" / f"{n}_out.flo", "rb").read(), n
    doc = json.load(open(out / "ftle.json"))
    h = w = 32
    assert (doc["spacing"], doc["steps"], doc["mask"], doc["leftover"], doc["lattice"]) == (2, 3, "flag", 2, [h, w])
    assert list(doc["windows"]) == ["f000", "f003"]
    assert sorted(p.name for p in (out / "flow").glob("*_ftle.flo")) == ["f000_ftle.flo", "f003_ftle.flo"]
    assert sorted(p.name for p in (out / "flow").glob("*_ftle.png")) == ["f000_ftle.png", "f003_ftle.png"]
    for first in (0, 3):
        flows = torch.stack([torch.from_numpy(read_flow(str(out / "flow" / f"{n}_out.flo"))).permute(2, 0, 1) for n in names[first:first + 3]])
        flows = flows.to(dev).contiguous()
        flags = V.validate_flow(flows, radius=2, spacing=1, eps=0.01, thresh=0.5, mode="flag").flag
        fm = pivlfn.FlowMap(H, W, 2, device=dev)
        fm.update(flows, flags)
        want = fm.ftle()
        got = torch.from_numpy(read_flow(str(out / "flow" / f"{names[first]}_ftle.flo"))).to(dev)
        assert got.shape == (h, w, 2)
        assert _same(got[..., 0].contiguous(), want.ftle) and _same(got[..., 1].contiguous(), want.stretch.float()), names[first]
        assert doc["windows"][names[first]] == runpy.json_strict(want.summary())
        im = PIL.Image.open(out / "flow" / f"{names[first]}_ftle.png")
        assert im.mode == "RGB" and im.size == (w, h)
