"""GPU: pivlfn_vortex_gamma (csrc/vortex.hip) against the NumPy restatement of its contract (tests/vortex_restatement.py).  Every
operation of the contract is a correctly rounded fp64 operation in a fixed order, so both planes and the flag bytes are compared bit
for bit, NaN positions included, and no pixel is left out.  Shapes: images smaller than the window, one that is no multiple of the
16 x 32 tile, the largest halo (r = 15, the window wider than a tile), spacings that do not divide the tile and that leave most of the
window outside the image.  Then batch independence, the stream and capture contract as tests/test_gpu_op_streams.py holds the other
entry points to it (its helpers, imported), guarded and scribbled buffers, the refusals, and run.py --vortex."""
import json

import numpy as np
import pytest
import torch

import vortex_restatement as vr
from guarded import check_guards, guarded, same_bits
from test_gpu_op_streams import (F32, U8, Spec, _behind_the_delay, _buf, _check, _p, _poisoned, _same, _scribble, delay)  # noqa: F401
from vortex_restatement import CENTRE_OUT, FEW

pytestmark = pytest.mark.gpu


def _run(dev, flow, r, s=1, mask=None, min_count=None):
    from pivlfn import vortex_gamma
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    v = vortex_gamma(t(flow), r, s, t(mask), min_count)
    B, _, H, W = flow.shape
    assert v.gamma1.dtype == v.gamma2.dtype == torch.float32 and v.flag.dtype == torch.uint8 and (v.radius, v.spacing) == (r, s)
    assert v.gamma1.shape == v.gamma2.shape == v.flag.shape == (B, H, W)
    assert v.gamma2.data_ptr() == v.gamma1.data_ptr() + 4 * H * W                 # views of the one [B,2,H,W] buffer
    return v


def _compare(v, want, what):
    """Every pixel: the flag bytes equal, both planes bit for bit."""
    wg, wflag = want
    flag = v.flag.cpu().numpy()
    assert np.array_equal(flag, wflag), f"{what}: {np.count_nonzero(flag != wflag)} flag bytes differ, first {np.argwhere(flag != wflag)[0]}"
    for k, plane in enumerate((v.gamma1, v.gamma2)):
        got = plane.cpu().numpy()
        same = got.view(np.int32) == wg[:, k].view(np.int32)
        if not same.all():
            at = tuple(np.argwhere(~same)[0])
            raise AssertionError(f"{what}: Gamma{k + 1} differs at {np.count_nonzero(~same)} pixels, first {at}: {got[at]!r} against {wg[:, k][at]!r}")
    few = (wflag & FEW) != 0
    assert np.isnan(wg[:, 0][few]).all() and np.isfinite(wg[:, 0][~few]).all(), what


def test_a_single_vector_has_no_neighbours(dev):
    flow = np.ones((2, 2, 1, 1), np.float32)
    v = _run(dev, flow, 1)
    _compare(v, vr.batch_gamma(flow, 1), "1x1")
    assert bool((v.flag == FEW).all()) and bool(torch.isnan(v.gamma1).all()) and bool(torch.isnan(v.gamma2).all())


@pytest.mark.parametrize("H,W", [(1, 7), (7, 1), (5, 3)])
def test_windows_larger_than_the_image(H, W, dev):
    """r = 1 clipped on every side at once; min_count 1 so that not every pixel is FEW (for 5 x 3 also the default)."""
    flow, mask = vr.random_case(np.random.default_rng(40 + H + W), 2, H, W, holes=False)
    flow[1, 0, H // 2, W // 2] = np.nan
    for m in (None, mask):
        v = _run(dev, flow, 1, 1, m, 1)
        _compare(v, vr.batch_gamma(flow, 1, 1, m, 1), f"{H}x{W} r=1 min_count=1")
        assert not bool((v.flag & FEW).all())
    if (H, W) == (5, 3):
        _compare(_run(dev, flow, 1, 1, mask), vr.batch_gamma(flow, 1, 1, mask), "5x3 r=1")


@pytest.mark.parametrize("H,W,r,s", [(37, 53, 2, 1), (37, 53, 3, 2), (70, 131, 8, 1), (67, 90, 15, 1), (130, 140, 4, 3), (130, 140, 4, 16)])
def test_bits_of_the_restatement(H, W, r, s, dev):
    """With a mask, NaN, -inf and 1e10 vectors.  70 x 131: five by five tiles, ragged both ways; 67 x 90 at r = 15: a halo of 15 around
    16 x 32 tiles; spacing 3: the 44 x 47 vectors of a phase are no multiple of the tile; spacing 16: 256 phases of 9 x 9 vectors or
    fewer, so the 9 x 9 window is whole at one vector of a phase at the most and clipped at every other."""
    flow, mask = vr.random_case(np.random.default_rng(1000 * r + s), 1, H, W)
    v = _run(dev, flow, r, s, mask)
    want = vr.batch_gamma(flow, r, s, mask)
    _compare(v, want, f"{H}x{W} r={r} s={s}")
    assert (want[1] & FEW).any() and (want[1] & CENTRE_OUT).any() and not (want[1] & FEW).all()


def test_every_pair_of_a_batch_equals_itself_alone(dev):
    """B = 3, different content and masks per pair, 37 x 53, (r, s) = (3, 2)."""
    flow, mask = vr.random_case(np.random.default_rng(77), 3, 37, 53)
    flow[1] *= 0.01
    flow[2] += np.float32(5.0)
    both = _run(dev, flow, 3, 2, mask)
    _compare(both, vr.batch_gamma(flow, 3, 2, mask), "B=3")
    for b in range(3):
        alone = _run(dev, flow[b:b + 1], 3, 2, mask[b:b + 1])
        assert same_bits(alone.gamma1[0], both.gamma1[b]) and same_bits(alone.gamma2[0], both.gamma2[b]) and torch.equal(alone.flag[0], both.flag[b])
    again = _run(dev, flow, 3, 2, mask)
    assert same_bits(again.gamma1, both.gamma1) and same_bits(again.gamma2, both.gamma2)


def _capped_shapes():
    import analysis_plans as ap
    return ap.shapes(ap.VORTEX_CASES)


@pytest.mark.parametrize("B,H,W,r,s", _capped_shapes())
def test_bits_where_the_stage_grid_is_capped(B, H, W, r, s, dev):
    """vortex_stage_kernel has at most max(16384 / B, 64) workgroups a frame and strides over the rest: 260 frames of 130 x 128 (65
    blocks of 256 pixels on a grid of 64: block 0 comes round for the last 256 pixels) and one frame of 2049 x 2048 (16392 on 16384).
    With a mask.  The first, the middle and the last frame against the restatement; sixteen frames (or the one) against the same frame
    in a call of its own, whose grid is not capped (65 blocks under a cap of 16384) or, for the one frame, against a second run."""
    import types
    import analysis_plans as ap
    plan = ap.capped_frame_grid(H * W, B)
    assert plan["blocks"] > plan["cap"] == plan["grid"]
    flow, mask = vr.random_case(np.random.default_rng(1000 * r + B), B, H, W)
    v = _run(dev, flow, r, s, mask)
    frame = lambda b: types.SimpleNamespace(gamma1=v.gamma1[b:b + 1], gamma2=v.gamma2[b:b + 1], flag=v.flag[b:b + 1])       # noqa: E731
    seen = 0
    for b in sorted({0, B // 2, B - 1}):
        want = vr.batch_gamma(flow[b:b + 1], r, s, mask[b:b + 1])
        _compare(frame(b), want, f"frame {b} of {B} x {H}x{W} r={r} s={s}")
        seen |= int(np.bitwise_or.reduce(want[1], axis=None))
        assert not (want[1] & FEW).all()
    assert seen & FEW and seen & CENTRE_OUT
    sample = [0, 1, 2, 63, 64, 65, 127, 128, 129, 130, 191, 192, 255, 256, 258, 259] if B > 1 else [0]
    for b in sample:
        alone = _run(dev, flow[b:b + 1], r, s, mask[b:b + 1])
        assert same_bits(alone.gamma1[0], v.gamma1[b]) and same_bits(alone.gamma2[0], v.gamma2[b]) and torch.equal(alone.flag[0], v.flag[b]), b


@pytest.mark.parametrize("r,s", [(8, 1), (4, 4)])
def test_dns_turbulence_fixture(r, s, dev):
    """tests/golden/DNS_turbulence_flow.flo, 256 x 256.  At r = 8 the restatement finds 29 % of the area inside vortex cores."""
    import os
    from conftest import GOLD
    flow = vr.read_flo(os.path.join(GOLD, "DNS_turbulence_flow.flo"))[None]
    assert flow.shape == (1, 2, 256, 256)
    v = _run(dev, flow, r, s)
    want = vr.batch_gamma(flow, r, s)
    _compare(v, want, f"DNS r={r} s={s}")
    (summary,) = v.summary()
    with np.errstate(invalid="ignore"):
        share = float((np.abs(want[0][0, 1]) > vr.CORE).mean())
    assert summary["fraction_core"] == share
    if (r, s) == (8, 1):
        assert 0.28 < share < 0.31


def _close(a, b):
    """Counts, indices and peak values are exact; a float64 sum of n <= 2^14 float32 magnitudes below 2 may be reduced in another order
    on the device than on the host: each order is within n * 2^-53 relative of the exact sum, 2e-12 here."""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_close(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(_close(x, y) for x, y in zip(a, b))
    return a == b or (a != a and b != b) or (isinstance(a, float) and abs(a - b) <= 4e-12 * abs(b))


def test_lamb_oseen_peaks_and_summary_equal_the_restatements(dev):
    """The project's Lamb-Oseen field 128 x 128 with its drift, r = 4: bits, and peaks() and summary() of the device result equal
    those formed from the restatement by the same plain-torch code on the host."""
    from pivlfn import VortexField
    flow = vr.lamb_oseen()[None]
    v = _run(dev, flow, 4)
    wg, wflag = vr.batch_gamma(flow, 4)
    _compare(v, (wg, wflag), "Lamb-Oseen r=4")
    host = VortexField(torch.from_numpy(wg[:, 0]), torch.from_numpy(wg[:, 1]), torch.from_numpy(wflag), 4, 1)
    peaks = v.peaks()
    assert peaks == host.peaks() and len(peaks[0]) == 1
    assert abs(peaks[0][0]["x"] - 63.5) <= 0.5 and abs(peaks[0][0]["y"] - 63.5) <= 0.5 and peaks[0][0]["value"] > 0.99
    assert v.peaks(of="gamma1", threshold=0.5) == host.peaks(of="gamma1", threshold=0.5)
    assert _close(v.summary(), host.summary()), (v.summary(), host.summary())
    assert torch.equal(v.cores().cpu(), host.cores()) and v.summary()[0]["area_pos"] == 2120


# ---- the stream and capture contract, with the helpers of tests/test_gpu_op_streams.py ------------------------------------------------
def _spec(seed, quad=False):
    """2 x 40 x 56 (H*W % 4 == 0), (r, s) = (3, 2), with a mask."""
    from pivlfn import _lib
    lib = _lib.load()
    B, H, W, r, s = 2, 40, 56, 3, 2
    flow, mask = vr.random_case(np.random.default_rng(2000 + seed), B, H, W)
    nws = lib.pivlfn_vortex_gamma_workspace_bytes(B, H, W, r, s)

    def call(i, o, a, ws, st):
        return lib.pivlfn_vortex_gamma(_p(i[0]), _p(i[1]), _p(o[0]), _p(o[1]), B, H, W, r, s, vr.default_min_count(r), _p(ws[0]), nws, st)

    def pin(outs):
        wg, wflag = vr.batch_gamma(flow, r, s, mask)
        assert vr.same_bits(outs[0].cpu().numpy(), wg) and np.array_equal(outs[1].cpu().numpy(), wflag)
    return Spec([torch.from_numpy(flow), torch.from_numpy(mask)], [((B, 2, H, W), F32), ((B, H, W), U8)], [], [nws], call, pin, (H, W))


@pytest.fixture()
def as_an_op(monkeypatch):
    """The helpers of test_gpu_op_streams look an op up by name: "vortex_gamma" resolves to the spec above."""
    import test_gpu_op_streams as ops
    original = ops._get
    monkeypatch.setattr(ops, "_get", lambda op, seed, quad=False: _spec(seed, quad) if op == "vortex_gamma" else original(op, seed, quad))
    return ops


def test_eager_result_is_the_restatements(dev, as_an_op):
    _, outs, _, _ = as_an_op._eager("vortex_gamma", 31, dev)
    _spec(31).pin(outs)


def test_runs_in_order_on_the_stream_it_is_given(dev, delay, as_an_op):        # noqa: F811
    """On a side stream behind a long-running chain of matrix products and the copies of the real inputs into poisoned buffers,
    enqueued without a host synchronisation: the eager result, bit for bit, and every guard intact."""
    still_waiting, got, ref, buffers = _behind_the_delay("vortex_gamma", dev, delay, lambda stream: stream.cuda_stream)
    assert still_waiting, "the delay ran out before the op was enqueued: the test would not see a launch on another stream"
    for g, want in zip(got, ref):
        assert _same(g, want), "the result behind a delay on a side stream differs from the eager result"
    for t in buffers:
        _check(t, "vortex_gamma")


def test_is_graph_capturable(dev, as_an_op):
    as_an_op.test_op_is_graph_capturable("vortex_gamma", dev)


def test_pointers_one_element_off_give_the_same_bits(dev, as_an_op):
    as_an_op.test_pointers_one_element_off_give_the_same_bits("vortex_gamma", dev)


@pytest.mark.parametrize("r,s", [(2, 1), (15, 2)])
def test_guarded_buffers_scribbled_outputs_and_workspace(r, s, dev):
    """Inputs, outputs and the workspace between guards; outputs and workspace first hold the sentinel, then 0xFF: the same bits both
    times, every guard intact, no input written; a workspace one byte smaller is refused before anything is launched."""
    from pivlfn import _lib, vortex_gamma
    lib = _lib.load()
    B, H, W = 2, 38, 46                             # B*H*W a multiple of 4: the byte buffers are whole 32-bit words
    flow, mask = vr.random_case(np.random.default_rng(600 + r), B, H, W)
    src = [torch.from_numpy(x).to(dev) for x in (flow, mask)]
    ref = vortex_gamma(src[0], r, s, src[1])
    ins = [guarded(t.shape, t.dtype, dev, "nan") for t in src]
    for t, x in zip(ins, src):
        t.copy_(x)
    gamma = guarded((B, 2, H, W), torch.float32, dev, "sentinel")
    flag = guarded((B, H, W), torch.uint8, dev, "sentinel")
    need = lib.pivlfn_vortex_gamma_workspace_bytes(B, H, W, r, s)
    ws = guarded((need,), torch.uint8, dev, "sentinel")
    st = torch.cuda.current_stream(dev).cuda_stream
    mc = vr.default_min_count(r)
    flag.fill_(0xFF)
    assert lib.pivlfn_vortex_gamma(_p(ins[0]), _p(ins[1]), _p(gamma), _p(flag), B, H, W, r, s, mc, _p(ws), need - 1, st) == 1
    assert "too small" in lib.pivlfn_last_error().decode()
    torch.cuda.synchronize()
    assert bool((flag == 0xFF).all())               # refused before anything was launched
    for scribble in (False, True):
        if scribble:
            for t in (gamma, flag, ws):
                _scribble(t)
        _lib.check(lib.pivlfn_vortex_gamma(_p(ins[0]), _p(ins[1]), _p(gamma), _p(flag), B, H, W, r, s, mc, _p(ws), need, st), "vortex_gamma")
        torch.cuda.synchronize()
        assert same_bits(gamma[:, 0], ref.gamma1) and same_bits(gamma[:, 1], ref.gamma2) and torch.equal(flag, ref.flag)
        for t in ins + [gamma, flag, ws]:
            check_guards(t, f"vortex_gamma r={r} s={s}")
    for t, x in zip(ins, src):
        assert torch.equal(t.view(torch.uint8), x.view(torch.uint8)), "an input was written"


def test_every_error_is_refused_before_any_launch(dev):
    """The refusals of tests/test_vortex.py with real device buffers: the outputs and the workspace keep every byte."""
    from pivlfn import _lib
    from test_vortex import refusals
    lib = _lib.load()
    B, H, W, r = 2, 8, 8, 2
    need = lib.pivlfn_vortex_gamma_workspace_bytes(B, H, W, r, 1)
    arena = _scribble(torch.empty(5 << 16, dtype=torch.uint8, device=dev))      # five regions 64 KiB apart: only what a case moves overlaps
    flow, mask, gamma, flag, ws = (arena.data_ptr() + (i << 16) for i in range(5))
    assert arena.data_ptr() % 8 == 0 and need < 1 << 16
    refusals(lib, flow, mask, gamma, flag, ws, B, H, W, r)
    torch.cuda.synchronize()
    assert bool((arena == 0xFF).all())


# ---- run.py --------------------------------------------------------------------------------------------------------------------------
def test_run_py_vortex(tmp_path, dev):
    """run.py -p --vortex 3 --vortex-spacing 2 --vortex-image --validate flag on three synthetic 64 x 64 pairs: every <name>_gamma.flo
    holds the two bands of vortex_gamma on the written flow with the validation flags as the mask, byte for byte; vortices.json holds
    the peaks and the summary of every pair and the summary of the run; the PNGs exist at the frames' size.  Without --vortex no such
    file appears, args.txt does not mention it, and the .flo files are the same bytes."""
    import PIL.Image
    import run as runpy
    import pivlfn
    from pivlfn import synth
    from pivlfn import validate as V
    from pivlfn import vortex as VX
    from pivlfn.flo import read_flow
    H = W = 64
    seq = tmp_path / "seq"
    seq.mkdir()
    names = [f"p{k}" for k in range(3)]
    for k, name in enumerate(names):
        a, b, _ = synth.particle_pair(H, W, 950 + k)
        PIL.Image.fromarray(a).save(str(seq / f"{name}_img1.png"))
        PIL.Image.fromarray(b).save(str(seq / f"{name}_img2.png"))
    base = ["--model", "piv", "-i", str(seq), "-p", "--batch", "2", "--validate", "flag", "--validate-radius", "2", "--validate-eps",
            "0.01", "--validate-thresh", "0.5"]
    assert runpy.main(base + ["-o", str(tmp_path / "plain")]) == 3
    assert runpy.main(base + ["-o", str(tmp_path / "vort"), "--vortex", "3", "--vortex-spacing", "2", "--vortex-image"]) == 3
    plain, vort = (tmp_path / d / "piv-synthetic" / "seq" for d in ("plain", "vort"))
    assert not list(plain.rglob("*_gamma*")) and not (plain / "vortices.json").exists()
    assert not [ln for ln in open(plain / "args.txt") if ln.startswith("vortex")]
    lines = list(open(vort / "args.txt"))
    assert "vortex: 3\n" in lines and "vortex_spacing: 2\n" in lines and "vortex_image: True\n" in lines
    doc = json.load(open(vort / "vortices.json"))
    assert (doc["radius"], doc["spacing"], doc["min_count"], doc["mask"]) == (3, 2, 24, "flag") and sorted(doc["pairs"]) == names
    defined = 0
    for n in names:
        data = open(vort / "flow" / f"{n}_out.flo", "rb").read()
        assert data == open(plain / "flow" / f"{n}_out.flo", "rb").read(), n
        flo = torch.from_numpy(read_flow(str(vort / "flow" / f"{n}_out.flo"))).to(dev).permute(2, 0, 1)[None].contiguous()
        flags = V.validate_flow(flo, radius=2, spacing=1, eps=0.01, thresh=0.5, mode="flag").flag
        want = pivlfn.vortex_gamma(flo, 3, 2, mask=flags)
        got = torch.from_numpy(read_flow(str(vort / "flow" / f"{n}_gamma.flo"))).to(dev)
        assert got.shape == (H, W, 2)
        assert same_bits(got[..., 0], want.gamma1[0]) and same_bits(got[..., 1], want.gamma2[0]), n
        assert doc["pairs"][n]["peaks"] == want.peaks()[0]
        (s,) = want.summary()
        assert _close(runpy.json_strict(s), doc["pairs"][n]["summary"]), (n, s, doc["pairs"][n]["summary"])
        defined += s["defined"]
        im = PIL.Image.open(vort / "flow" / f"{n}_gamma2.png")
        assert im.mode == "RGB" and im.size == (W, H)
    pairs = [doc["pairs"][n]["summary"] for n in names]
    for key in ("defined", "area_pos", "area_neg"):                    # additive over the pairs
        assert doc["total"][key] == sum(p[key] for p in pairs), key
    assert doc["total"]["defined"] == defined
    assert abs(doc["total"]["fraction_core"] - sum(p["area_pos"] + p["area_neg"] for p in pairs) / (3.0 * H * W)) < 1e-15
    assert abs(doc["total"]["mean_abs_gamma2"] - sum(p["mean_abs_gamma2"] * p["defined"] for p in pairs) / defined) < 1e-12
    assert sorted(p.name for p in (vort / "flow").glob("*_gamma2.png")) == [f"{n}_gamma2.png" for n in names]
