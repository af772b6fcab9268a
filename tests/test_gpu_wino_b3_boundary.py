"""GPU: the tile boundary of the split-operand Winograd kernel (csrc/conv_wino_b3.hip) -- the output exchange through LDS, the stores
by a row step from one offset per tile, the accumulators zeroed for the next tile, the next tile's start.

A workgroup is persistent: one per compute unit, each walking its share of the tiles.  What the boundary code can get wrong shows on a
workgroup's second and later tiles (the exchange area reused, accumulators not zeroed, a patch buffer read before it is complete or
overwritten before it is read, a store offset carried over from the tile before) and never on its first.  So every case puts two to four times as many tiles on the device as it has
compute units and compares each sample, bit for bit, with the same sample run alone: alone it has fewer tiles than the device has
compute units, every workgroup multiplies one tile and the boundary code between two tiles never runs.  The batch result also meets the
float64 bars of test_gpu_wino_b3.py::test_b3_matches_float64_conv."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv import Conv, run as run_direct
from test_gpu_wino import run_wino
from test_gpu_wino_b3 import run_b3

pytestmark = pytest.mark.gpu

CASES = [
    # cin, input lanes, cout, H, W
    (32, 32, 128, 96, 96),       # two steps: the load stream switches tiles in the first step
    (16, 16, 64, 64, 64),        # one real step and the all-zero second one
    (52, 56, 128, 96, 96),       # 52 of 56 lanes: a tail step of four channels
    (128, 128, 128, 64, 64),     # eight steps
    (64, 64, 64, 128, 128),
    (128, 128, 128, 100, 84),    # ragged edges in both directions
]
RAGGED = CASES[5]


def _batch(case, dev):
    """Samples per launch: tiles = B x ceil(H / 16) x ceil(W / 16) x (cout / 64) at least twice the compute units (and, as a sample alone has
    no more tiles than there are compute units, less than three times)."""
    ci, lanes, co, H, W = case
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    per_image = -(-H // 16) * -(-W // 16) * (co // 64)
    assert per_image <= cus, (case, per_image, cus)       # a sample alone: one tile per workgroup, the reference never crosses a tile boundary
    B = -(-2 * cus // per_image)
    assert 2 * cus <= B * per_image and (co != 128 or B * per_image <= 4 * cus), (case, B, per_image, cus)
    return B


@functools.lru_cache(maxsize=None)
def _layer(case, B):
    """Weights, bias, input and the float64 convolution of the same fp32 data: made once per case, shared by every test, never written to."""
    ci, lanes, co, H, W = case
    g = torch.Generator().manual_seed(co * 1000 + ci * 7 + H)
    w = torch.randn(co, ci, 3, 3, generator=g) / (ci * 9) ** 0.5
    b = torch.randn(co, generator=g) * 0.1
    x = torch.randn(B, ci, H, W, generator=g)
    want = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    return Conv(w, b), x, want


def _check_float64_bars(case, terms, leaky, got, conv, x, want, dev):
    """The bars of test_b3_matches_float64_conv."""
    e = (got.double() - (F.leaky_relu(want, 0.1) if leaky else want)).abs()
    scale = max(1.0, want.abs().max().item())
    assert e.max().item() < 1e-5 * scale, (case, terms, e.max().item())
    if not leaky:
        ew = (run_wino(conv, x, False, dev, x_lanes=case[1]).double() - want).abs()
        assert e.mean().item() <= ew.mean().item() * 1.02 + 1e-12, (case, terms, e.mean().item(), ew.mean().item())
        assert e.max().item() <= ew.max().item() * 1.25 + 1e-12, (case, terms, e.max().item(), ew.max().item())
        if case[3] * case[4] >= 64 * 64:
            ed = (run_direct(conv, x, 1, (1, 1), False, dev, x_lanes=case[1]).double() - want).abs()
            assert e.mean().item() <= ed.mean().item() * 1.02 + 1e-12, (case, terms, e.mean().item(), ed.mean().item())
            assert e.max().item() <= ed.max().item() * 1.25 + 1e-12, (case, terms, e.max().item(), ed.max().item())


def _check(case, terms, dev, y_lanes=None):
    B = _batch(case, dev)
    conv, x, want = _layer(case, B)
    for leaky in (False, True):
        full = run_b3(conv, x, leaky, dev, terms, x_lanes=case[1], y_lanes=y_lanes)      # run_b3: lanes past the stored ones still hold their poison
        for i in range(B):
            one = run_b3(conv, x[i:i + 1], leaky, dev, terms, x_lanes=case[1])
            assert torch.equal(one[0], full[i]), (case, terms, leaky, i, (one[0] - full[i]).abs().max().item())
        _check_float64_bars(case, terms, leaky, full, conv, x, want, dev)


@pytest.mark.parametrize("case", CASES)
def test_b3_later_tiles_equal_first_tiles(case, dev):
    """Six piece products, with and without LeakyReLU: every sample of a batch that gives each workgroup two to three tiles has the bits
    of the sample run alone, and the batch meets the float64 bars."""
    _check(case, 6, dev)


@pytest.mark.parametrize("terms", [8, 9])
def test_b3_later_tiles_equal_first_tiles_more_terms(terms, dev):
    """The eight- and nine-term instances are separate kernels with their own form of the store offsets: the ragged case on both."""
    _check(RAGGED, terms, dev)


def test_b3_boundary_leaves_lanes_past_the_stored_ones(dev):
    """Output rows of 72 lanes for 64 channels, poisoned beforehand: the stores of every tile write channels below cout_store only
    (run_b3 asserts that the lanes behind them still hold the poison), on second and later tiles as on the first."""
    _check(CASES[4], 6, dev, y_lanes=72)
