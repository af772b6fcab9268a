"""GPU: the direct convolution on every tile shape its launcher can pick, each against float64 on its own.

tests/test_conv_plan.py::TILE_CASES holds one layer and shape per plan of launch_conv (kernel family, tile rows and channels, staging
class, split-K shares), with ragged right and bottom edges, output channel counts that leave the last block and quad ragged, and
strides wider than needed.  Each case runs as tests/test_gpu_guarded.py::_conv_case runs a layer: torch.nn.functional.conv2d in
float64 (plus residual and LeakyReLU) with test_gpu_conv.py's bar, max-abs error < 2e-5 * max(1, max|want|); guarded buffers with NaN
and finite poison in the lanes that are not read; the sentinel kept in the lanes that are not stored.
Then the batch rule pivlfn_forward's guarantee rests on: the case's first image alone, in the case's own batch and in a batch whose plan
differs (the tile, the family -- NetC.conv1 moves between v2 and k1 with the batch -- or, for the handle's split-K scratch, image by
image) gives the same bits.  It holds for every family, the v1 fallback included."""
import pytest
import torch

from guarded import same_bits
from test_conv_plan import POLICY, TILE_CASES, case_plan, second_batch
from test_gpu_guarded import _conv_case, _launch

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _first_image(r, case, B, dev):
    """The case's first image as image 0 of a batch of B (the others seeded noise), through the case's own handle: its output."""
    co, ci, kh, kw, s, pad, H, W, _, _, _, with_res = case
    Ho, Wo = (H + 2 * pad[0] - kh) // s + 1, (W + 2 * pad[1] - kw) // s + 1
    g = torch.Generator().manual_seed(B)
    xd = torch.zeros(B, H, W, r.xs, device=dev)
    xd[..., :ci] = torch.randn(B, H, W, ci, generator=g).to(dev)
    xd[0, ..., :ci] = r.x[0].permute(1, 2, 0).to(dev)
    yd = torch.full((B, Ho, Wo, r.ys), NAN, device=dev)
    rd = None
    if with_res:
        rd = torch.zeros(B, Ho, Wo, r.ys, device=dev)
        rd[..., :co] = torch.randn(B, Ho, Wo, co, generator=g).to(dev)
        rd[0, ..., :co] = r.res[0].permute(1, 2, 0).to(dev)
    _launch("direct", r.conv, xd, r.xs, yd, r.ys, B, H, W, s, pad, r.leaky, dev, rd)
    torch.cuda.synchronize()
    return yd[0, ..., :co].cpu()


@pytest.mark.parametrize("case,want", TILE_CASES, ids=lambda v: "-".join(str(x) for x in v).replace(" ", "") if isinstance(v, tuple) else None)
def test_tile_against_float64_and_across_batches(case, want, dev):
    assert case_plan(case) == want, POLICY
    r = _conv_case("direct", case, dev)                      # float64 bar, guards, lanes, both poison kinds
    alone, B2 = _first_image(r, case, 1, dev), second_batch(case)
    assert same_bits(alone, r.plain[0]), f"{case}: the first image's bits differ between B = 1 ({case_plan(case, 1)}) and B = {case[8]} ({want})"
    assert same_bits(alone, _first_image(r, case, B2, dev)), \
        f"{case}: the first image's bits differ between B = 1 ({case_plan(case, 1)}) and B = {B2} ({case_plan(case, B2)})"


STREAMING = [
    # cout, cin, kh, kw, pad, H, W, family: the aspect ratios no other test gives the streaming kernels (chosen by H * W >= 256 * 256 alone)
    (49, 32, 7, 1, (3, 0), 5, 13108, 6),
    (49, 32, 7, 1, (3, 0), 32, 2048, 6),         # level 1 of a 32 x 2048 strip
    (49, 49, 1, 7, (0, 3), 13108, 5, 7),
    (49, 49, 1, 7, (0, 3), 2048, 32, 7),
]


@pytest.mark.parametrize("co,ci,kh,kw,pad,H,W,family", STREAMING)
def test_streaming_kernels_on_strips(co, ci, kh, kw, pad, H, W, family, dev):
    """No activation, 52 stored lanes; B = 2 against float64 in guarded buffers, its first image equal to the B = 1 result bit for bit."""
    case = (co, ci, kh, kw, 1, pad, H, W, 2, 4 if ci == 32 else 0, 0, False)
    for B in (1, 2):
        assert case_plan(case, B)[0] == family, POLICY
    r = _conv_case("direct", case, dev)
    assert r.ys == 52 and r.leaky == 0
    assert same_bits(_first_image(r, case, 1, dev), r.plain[0])
