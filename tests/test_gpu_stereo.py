"""GPU: pivlfn_stereo_2d3c (csrc/stereo.hip), estimate_stereo and stereo_run.py against the reference's arithmetic, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pivlfn
from pivlfn import stereo, synth
from pivlfn.inference import _resize
from stereo_restatement import load_case, restate, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "piv_liteflownet-pytorch_amd")
GOLD = os.path.join(ROOT, "tests", "golden")


def _nchw(left_hw2, right_hw2, dev):
    """[B,h,w,2] x2 (numpy) -> interleaved [2B,2,h,w] on the device."""
    l = torch.from_numpy(np.ascontiguousarray(left_hw2)).permute(0, 3, 1, 2)
    r = torch.from_numpy(np.ascontiguousarray(right_hw2)).permute(0, 3, 1, 2)
    return stereo.interleave(l, r).contiguous().to(dev)


def _want(left_hw2, right_hw2, coeff, tans, fps, calib):
    s = stereo.scale_factor(coeff, calib)
    return restate(left_hw2, right_hw2, stereo.coeff_f32(coeff), tans, None if s is None else (s, fps))


def _coeff(rng, calib=None):
    base = np.array([1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
    c = {s: [float(v) for v in base + rng.normal(0, 1e-3, 24)] for s in ("Left", "Right")}
    if calib is not None:
        c["calib"] = calib
    return c


def test_kernel_matches_reference_fixture(dev):
    g = np.load(os.path.join(GOLD, "stereo_cases.npz"))
    for tag in g["cases"]:
        left, right, coeff, th, al, fps, calib = load_case(g, tag)
        tans = stereo.tangents(*stereo.angles(th, al))
        got = stereo.stereo_2d3c(_nchw(left[None], right[None], dev), coeff, tans, fps, calib)
        assert got.shape == (1,) + left.shape[:2] + (3,)
        assert same_bits(got[0].cpu().numpy(), g[f"{tag}_out"]), tag


def _capped_shapes():
    """Where the grid of stereo_2d3c_kernel is capped at max(16384 / B, 64) workgroups a pair and strides (tests/analysis_plans.py):
    260 pairs of 130 x 128 and one of 2049 x 2048.  The 1024 x 1024 case has 4096 workgroups, below the cap."""
    import analysis_plans as ap
    return ap.shapes(ap.STEREO_CASES)


@pytest.mark.parametrize("B,h,w", [(1, 37, 23), (3, 37, 23), (3, 100, 76), (1, 1024, 1024)] + _capped_shapes())
@pytest.mark.parametrize("calib", [None, 0.05])
def test_kernel_matches_restatement_random(dev, B, h, w, calib):
    rng = np.random.default_rng(B * 1000 + h + (7 if calib else 0))
    left = rng.normal(0, 8, (B, h, w, 2)).astype(np.float32)
    right = rng.normal(0, 8, (B, h, w, 2)).astype(np.float32)
    coeff = _coeff(rng, 0.002)
    tans = stereo.tangents(*stereo.angles([30.0, 40.0], [5.0, -3.0]))
    got = stereo.stereo_2d3c(_nchw(left, right, dev), coeff, tans, 15, calib).cpu().numpy()
    assert same_bits(got, _want(left, right, coeff, tans, 15, calib))


@pytest.mark.parametrize("H,W", [(64, 64), (100, 76)])
def test_fused_resize_equals_estimate_resize(dev, H, W):
    """Raw half-resolution flows of piv v2 at the network's adapted size -> the kernel's fused resize equals the restatement
    applied to estimate()'s resized flows; in the same-size case the input passes through unchanged."""
    net = pivlfn.piv_liteflownet(synth.generate_weights("piv2", 0), version=2).to(dev).eval()
    a, b = synth.particle_batch(2, H, W, seed=H + W)
    a, b = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    raw, H_, W_, sw, sh = pivlfn.inference._adapted_forward(net, a, b)
    assert (H_, W_) == (H, W) and raw.shape[2:] != (H, W)
    resized = _resize(raw.contiguous(), H, W, mul=(sw, sh))
    assert torch.equal(resized, pivlfn.estimate(net, a, b, tensor=True))
    rng = np.random.default_rng(H)
    coeff = _coeff(rng, 0.002)
    tans = stereo.tangents(*stereo.angles([35.0], [2.0]))
    got = stereo.stereo_2d3c(raw, coeff, tans, 15, 0.05, out_hw=(H, W), mul=(sw, sh)).cpu().numpy()
    r = resized.permute(0, 2, 3, 1).cpu().numpy()
    assert same_bits(got, _want(r[0::2], r[1::2], coeff, tans, 15, 0.05))
    same = stereo.stereo_2d3c(resized, coeff, tans, 15, 0.05).cpu().numpy()        # (h, w) == (H, W): read as is
    assert same_bits(same, got)
    one = [1.0, 0, 0, 0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 0, 0, 1.0, 0, 0, 0]   # x' = u, y' = v
    ident = {"Left": one, "Right": one}
    tans1 = np.array([-1.0, 1.0, 0.0, 0.0])
    out = stereo.stereo_2d3c(raw, ident, tans1, out_hw=(H, W), mul=(sw, sh)).cpu().numpy()
    assert same_bits(out, _want(r[0::2], r[1::2], ident, tans1, 1, None))
    # U = (uR * -1 - uL * 1) / -2 = (uL + uR) / 2 exactly here, so the per-camera values went through untouched
    assert same_bits(out[..., 0], ((r[0::2, ..., 0].astype(np.float64) + r[1::2, ..., 0]) / 2).astype(np.float32))


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("B", [1, 2])
def test_estimate_stereo_is_one_interleaved_forward(dev, version, B):
    net = pivlfn.piv_liteflownet(synth.generate_weights("piv2" if version == 2 else "piv", 0), version=version).to(dev).eval()
    l1, l2 = (torch.from_numpy(x).to(dev) for x in synth.particle_batch(B, 100, 76, seed=11 + B))
    r1, r2 = (torch.from_numpy(x).to(dev) for x in synth.particle_batch(B, 100, 76, seed=21 + B))
    coeff = _coeff(np.random.default_rng(version), 0.002)
    fl = pivlfn.estimate(net, l1, l2, tensor=True)
    fr = pivlfn.estimate(net, r1, r2, tensor=True)
    raw, H, W, sw, sh = pivlfn.inference._adapted_forward(net, stereo.interleave(l1, r1), stereo.interleave(l2, r2))
    both = _resize(raw.contiguous(), H, W, mul=(sw, sh)) if raw.shape[2:] != (H, W) else raw
    assert torch.equal(both[0::2], fl) and torch.equal(both[1::2], fr)      # per camera, bit-equal to estimate()
    got = pivlfn.estimate_stereo(net, l1, l2, r1, r2, coeff, [30.0, 40.0], [5.0], fps=15, calib=0.05, tensor=True)
    tans = stereo.tangents(*stereo.angles([30.0, 40.0], [5.0]))
    want = stereo.stereo_2d3c(stereo.interleave(fl, fr), coeff, tans, 15, 0.05)
    assert got.shape == (B, 100, 76, 3) and same_bits(got.cpu().numpy(), want.cpu().numpy())
    if B == 1:
        arr = pivlfn.estimate_stereo(net, l1, l2, r1, r2, coeff, [30.0, 40.0], [5.0], fps=15, calib=0.05)
        assert isinstance(arr, np.ndarray) and arr.shape == (100, 76, 3) and same_bits(arr, want[0].cpu().numpy())


def _cli(script, args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(PKG, script)] + args, capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, f"{script} {args}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return r


def test_stereo_run_end_to_end(tmp_path, dev):
    import PIL.Image
    from pivlfn.flo import read_flow
    root = tmp_path / "SET"
    for side, tag, seed in (("left", "L", 300), ("right", "R", 500)):
        d = root / side
        d.mkdir(parents=True)
        for k in range(4):
            a, _, _ = synth.particle_pair(100, 76, seed + k)
            PIL.Image.fromarray(a).save(str(d / f"{k:04d}-{tag}.png"))
    wfile = tmp_path / "w.pt"
    torch.save(synth.generate_weights("piv", 0), str(wfile))
    coeff = tmp_path / "c.json"
    coeff.write_text(json.dumps(_coeff(np.random.default_rng(5), 0.002)))
    common = ["--coeff", str(coeff), "--theta", "30", "40", "--alpha", "5", "--fps", "15", "--calib", "0.05"]
    direct, manual = tmp_path / "direct", tmp_path / "manual"
    _cli("stereo_run.py", common + ["--root", str(root), "--save", str(direct), "--model", str(wfile),
                                    "--inference-mode", "direct", "--batch", "2"])
    _cli("stereo_run.py", common + ["--root", str(root), "--save", str(manual), "--model", str(wfile),
                                    "--inference-mode", "manual"])
    for k in range(3):
        for side, tag in (("left", "L"), ("right", "R")):
            f = read_flow(str(manual / side / f"{k:04d}-{tag}_out.flo"))
            assert f.shape == (100, 76, 2)
        d = read_flow(str(direct / "stereo" / f"{k:04d}-L_2d3c.flo"), use_stereo=True)
        m = read_flow(str(manual / "stereo" / f"{k:04d}-S_out.flo"), use_stereo=True)
        assert d.shape == (100, 76, 3) and np.isfinite(d).all() and same_bits(d, m), k
        # 3-band files: exactly header + H*W*3 float32
        assert os.path.getsize(direct / "stereo" / f"{k:04d}-L_2d3c.flo") == 12 + 100 * 76 * 3 * 4
    assert sorted(os.listdir(direct / "stereo")) == [f"{k:04d}-L_2d3c.flo" for k in range(3)]
    # run.py on both camera folders, then flo mode on its flow/ tree: the same files again
    out = tmp_path / "out"
    _cli("run.py", ["--model", "piv", "--weights", str(wfile), "-i", str(root / "left"), str(root / "right"),
                    "-o", str(out)])
    flow = out / "w" / "SET" / "flow"
    _cli("stereo_run.py", common + ["--save", str(flow)])
    for k in range(3):
        m = read_flow(str(manual / "stereo" / f"{k:04d}-S_out.flo"), use_stereo=True)
        f = read_flow(str(flow / "stereo" / f"{k:04d}-S_out.flo"), use_stereo=True)
        assert same_bits(f, m), k
