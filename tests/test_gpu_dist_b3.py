"""GPU: Regularization's (7 x 1) 49 <- 32 and (1 x 7) 49 <- 49 distance convolutions with exactly split operands on the bf16 matrix
cores (csrc/conv_dist_b3.hip, pivlfn_conv2d_nhwc_dist_b3) against a float64 convolution of the same fp32 data, next to the kernel they
replace in the default mode (pivlfn_conv2d_nhwc: the streaming fp32-instruction kernels from 256 x 256 pixels, the direct kernel below).
Replaces the two torch.nn.Conv2d of conv_dist_R at levels 1 and 2, /root/reference/src/models.py:253-261.

What this file asserts, for 6, 8 and 9 piece products per product:
  * max-abs error < 1e-5 of max(1, max |out|), and error against float64 <= 1.02 x (mean) and <= 1.25 x (max) that of the kernel
    replaced -- the bars of tests/test_gpu_wino_b3.py;
  * shapes from one pixel to the network's smallest level-1 grid: smaller than the seven taps, ragged in both directions, halos longer
    than the image, and 1, 3, 4, 5, 9 and 12 tiles (a workgroup walks four tiles and rotates the output block of each wave);
  * input lanes past the contract's hold NaN and are never read, output lanes 49..51 are exact zeros, lanes past them untouched, guards
    around both buffers keep their bits;
  * fp32's input domain, batch invariance bit for bit, and the forward in the default mode: batch invariance, graph replay, and the
    distance to the fp32_wino_mfma32 forward (which keeps the fp32-instruction kernels) within the end-to-end tolerance."""
import functools
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from guarded import check_guards, check_lanes, guarded, poison, same_bits
from pivlfn import _lib
from test_gpu_conv import Conv, run as run_fp32

pytestmark = pytest.mark.gpu

LAYERS = {"col7": (32, 7, 1, (3, 0)), "row7": (49, 1, 7, (0, 3))}      # cin, kh, kw, pad
# H, W, B
SHAPES = [(1, 1, 1), (5, 3, 1), (16, 16, 1), (17, 33, 2), (37, 45, 1), (6, 80, 1), (80, 6, 1), (16, 48, 1), (32, 32, 1), (256, 272, 1)]
STRIDES = [(52, 52), (52, 56), (64, 52), (64, 56)]                     # x stride, y stride


@functools.lru_cache(maxsize=None)
def layer(name):
    ci, kh, kw, _ = LAYERS[name]
    g = torch.Generator().manual_seed(49000 + ci + kh)
    w = torch.randn(49, ci, kh, kw, generator=g) / (ci * 7) ** 0.5
    b = torch.randn(49, generator=g) * 0.1
    return w, b, Conv(w, b)


@functools.lru_cache(maxsize=None)
def case(name, H, W, B, dev):
    """Input, float64 result and the error of the kernel replaced: computed once, shared, never modified."""
    w, b, conv = layer(name)
    ci, _, _, pad = LAYERS[name]
    g = torch.Generator().manual_seed(H * 1000 + W + B)
    x = torch.randn(B, ci, H, W, generator=g)
    want = F.conv2d(x.double(), w.double(), b.double(), padding=pad)
    e32 = (run_fp32(conv, x, 1, pad, False, dev).double() - want).abs()
    return x, want, e32


def run_b3(name, x_nchw, dev, terms=6, xs=52, ys=52, conv=None):
    """Through pivlfn_conv2d_nhwc_dist_b3 on guarded buffers: input lanes past the layer's channels NaN, output pre-filled with a sentinel."""
    conv = conv or layer(name)[2]
    B, C, H, W = x_nchw.shape
    x = guarded((B, H, W, xs), dev=dev, fill="nan")
    x[..., :C] = x_nchw.permute(0, 2, 3, 1).to(dev)
    poison(x, slice(C, xs), "nan")
    keep = x.clone()
    y = guarded((B, H, W, ys), dev=dev, fill="sentinel")
    _lib.check(_lib.load().pivlfn_conv2d_nhwc_dist_b3(conv.h, x.data_ptr(), xs, y.data_ptr(), ys, B, H, W, terms,
                                                     torch.cuda.current_stream(dev).cuda_stream), "conv2d_dist_b3")
    torch.cuda.synchronize()
    what = f"{name} {tuple(x_nchw.shape)} terms {terms} strides {xs}, {ys}"
    check_guards(x, what + " input")
    check_guards(y, what + " output")
    assert same_bits(x, keep), what + ": the input changed"
    check_lanes(y, slice(49, 52), "zero", what)
    if ys > 52:
        check_lanes(y, slice(52, ys), "sentinel", what)
    return y[..., :49].permute(0, 3, 1, 2).contiguous().cpu()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", list(LAYERS))
def test_dist_b3_matches_float64_conv(name, shape, dev):
    x, want, e32 = case(name, *shape, dev)
    scale = max(1.0, want.abs().max().item())
    first = {}
    for terms in (6, 8, 9):
        for xs, ys in STRIDES:
            got = run_b3(name, x, dev, terms, xs, ys)
            if terms in first:
                assert torch.equal(got, first[terms]), (name, shape, terms, xs, ys, "the bits depend on the strides")
                continue
            first[terms] = got
            e = (got.double() - want).abs()
            print(f"{name} {shape} terms {terms}: max {e.max().item():.3e} mean {e.mean().item():.3e}   fp32 kernel: max {e32.max().item():.3e} "
                  f"mean {e32.mean().item():.3e}")
            assert e.max().item() < 1e-5 * scale, (name, shape, terms, e.max().item())
            assert e.mean().item() <= e32.mean().item() * 1.02 + 1e-12, (name, shape, terms, e.mean().item(), e32.mean().item())
            assert e.max().item() <= e32.max().item() * 1.25 + 1e-12, (name, shape, terms, e.max().item(), e32.max().item())


def test_dist_b3_error_beside_the_fp32_kernels(dev, capsys):
    """The three piece-product counts beside the streaming fp32-instruction kernels at the network's smallest level-1 grid, printed once."""
    for name in LAYERS:
        x, want, e32 = case(name, 256, 272, 1, dev)
        rms = want.pow(2).mean().sqrt().item()
        e = {"fp32": e32}
        for t in (6, 8, 9):
            e[f"b3_{t}"] = (run_b3(name, x, dev, t).double() - want).abs()
        with capsys.disabled():
            print(f"\n{name} 256 x 272: rms(out) {rms:.3f}; error / rms  " +
                  "  ".join(f"{k}: max {v.max().item() / rms:.2e} mean {v.mean().item() / rms:.2e}" for k, v in e.items()))
        for t in (6, 8, 9):
            assert e[f"b3_{t}"].mean().item() <= e32.mean().item() * 1.02, (name, t)
            assert e[f"b3_{t}"].max().item() <= e32.max().item() * 1.25, (name, t)


@pytest.mark.parametrize("name", list(LAYERS))
def test_dist_b3_has_fp32s_input_domain(name, dev):
    """Activations scaled by 1e30 and by 1e-30 (far outside any 16-bit format with fewer exponent bits; a zero bias, so that the output
    scales with them): the error relative to max |out| stays below the 1e-5 bar and within a factor of two of the unscaled run's -- the
    maxima of three samples of one error distribution (1e30 is no power of two: every value rounds anew)."""
    x, _, _ = case(name, 37, 45, 1, dev)
    w, _, _ = layer(name)
    conv = Conv(w, torch.zeros(49))
    pad = LAYERS[name][3]
    rel = {}
    for scale in (1.0, 1e30, 1e-30):
        xs = x * scale
        want = F.conv2d(xs.double(), w.double(), padding=pad)
        got = run_b3(name, xs, dev, conv=conv)
        assert torch.isfinite(got).all()
        rel[scale] = (got.double() - want).abs().max().item() / want.abs().max().item()
    print(f"{name}: max error / max |out| at scales 1, 1e30, 1e-30: " + "  ".join(f"{v:.3e}" for v in rel.values()))
    for scale in (1e30, 1e-30):
        assert rel[scale] < 1e-5, (name, scale, rel)
        assert rel[scale] <= 2 * rel[1.0], (name, scale, rel)


@pytest.mark.parametrize("name", list(LAYERS))
def test_dist_b3_batch_invariance(name, dev):
    x, _, _ = case(name, 17, 33, 2, dev)
    full = run_b3(name, x, dev)
    for i in range(2):
        assert torch.equal(run_b3(name, x[i:i + 1], dev)[0], full[i]), (name, i)


def test_dist_b3_refuses_other_layers(dev):
    g = torch.Generator().manual_seed(6)
    conv = Conv(torch.randn(32, 32, 7, 1, generator=g), torch.zeros(32))
    x = torch.zeros(1, 8, 8, 32, device=dev)
    y = torch.zeros(1, 8, 8, 52, device=dev)
    rc = _lib.load().pivlfn_conv2d_nhwc_dist_b3(conv.h, x.data_ptr(), 32, y.data_ptr(), 52, 1, 8, 8, 6, torch.cuda.current_stream(dev).cuda_stream)
    assert rc != 0 and "distance convolution" in _lib.load().pivlfn_last_error().decode()


# ---- the forward in the default mode (level 1 of a 256 x 256 pair runs both kernels): in a process of its own ---------------------------
def test_forward_in_a_process_of_its_own(dev):
    """tests/dist_b3_forward_cases.py in a fresh pytest process: 2 tests, both passing -- batch invariance and graph replay of the default
    forward, and its distance to the fp32_wino_mfma32 forward.  Why not in this process: the networks' side streams, the capture stream and
    the graph would change which queue a later module's side stream shares with the default stream (tests/test_gpu_particles.py)."""
    here = os.path.dirname(os.path.abspath(__file__))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                                                                          os.path.join(here, "dist_b3_forward_cases.py")]
    r = subprocess.run(cmd, cwd=here, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and re.search(r"\b2 passed", r.stdout), r.stdout[-6000:] + r.stderr[-2000:]
