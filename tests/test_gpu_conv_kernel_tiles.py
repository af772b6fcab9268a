"""GPU: the fp16, split, Winograd and split-bf16 Winograd convolutions on every kernel their launchers can pick, each against float64.

tests/test_conv_kernel_plans.py holds one layer and shape per plan of launch_conv_h, launch_conv_x, launch_conv_w and launch_conv_wb
(instantiation, split-K shares, folded tail, image-by-image batch), with ragged right and bottom edges, output channel counts that leave
the last block and quad ragged, and strides wider than needed.  Each case runs as tests/test_gpu_guarded.py::_conv_case runs a layer:
torch.nn.functional.conv2d in float64 (of the fp16-rounded operands for the fp16 kernel) with the bars of that file -- max-abs error
below 2e-5 (split, fp16) or 1e-5 (both Winograd kernels) of max(1, max|want|); guarded buffers with NaN and finite poison in the lanes
that are not read; the sentinel kept in the lanes that are not stored, zeros in the padding lanes.  The float64 convolution of the
largest layers (more than 2e9 multiply-adds: 515 x 520, 64 channels at 260 x 515) runs on the device (torch's, not the library's).
Then the batch rule the launchers promise: the case's first image alone, in the case's own batch and in a batch whose plan differs (the
tile, for the split handle image by image) gives the same bits.  For split layers with a folded tail the plan test shows that no batch
moves a layer between the big and the small kernel, whose sums differ.

conv_wino_b3_kernel's persistent schedule -- one workgroup per CU walks an XCD band of tiles round-robin, stepping (group, column, row,
image) by increments with carries -- gets cases sized from the CU count at run time (b3_schedule_cases): 7, CUs - 1, CUs, CUs + 1 and
2 CUs + 7 tiles as single tile rows and columns, three images of three tile columns, two and three channel groups.  The sentinel, the
guards and the float64 comparison together say that every output pixel is written, and nothing else."""
import pytest
import torch

from guarded import same_bits
from test_conv_kernel_plans import (B3_CASES, CUS, F16, F16_CASES, SPLIT, SPLIT_CASES, WINO, WINO_B3, WINO_CASES, b3_schedule_cases, case_id,
                                    case_plan, inst, second_batch)
from test_conv_plan import POLICY
from test_gpu_guarded import _conv_case, _launch

pytestmark = pytest.mark.gpu
NAN = float("nan")
KERNEL = {F16: "f16", SPLIT: "split", WINO: "wino", WINO_B3: "b3"}


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _first_image(kernel, r, case, B, dev, terms, x16):
    """The case's first image as image 0 of a batch of B (the others seeded noise), through the case's own handle: its output."""
    co, ci, kh, kw, s, pad, H, W = case[:8]
    Ho, Wo = (H + 2 * pad[0] - kh) // s + 1, (W + 2 * pad[1] - kw) // s + 1
    g = torch.Generator().manual_seed(B)
    xd = torch.zeros(B, H, W, r.xs, device=dev, dtype=torch.float16 if x16 else torch.float32)
    xd[..., :ci] = torch.randn(B, H, W, ci, generator=g).to(dev)
    xd[0, ..., :ci] = r.x[0].permute(1, 2, 0).to(dev)
    yd = torch.full((B, Ho, Wo, r.ys), NAN, device=dev)
    _launch(KERNEL[kernel], r.conv, xd, r.xs, yd, r.ys, B, H, W, s, pad, r.leaky, dev, None, terms, x16)
    torch.cuda.synchronize()
    return yd[0, ..., :co].cpu()


def _case_and_batches(kernel, case, dev, terms=6, x16=0, cus=CUS):
    co, ci, kh, kw, s, pad, H, W, B = case[:9]
    heavy = B * H * W * co * ci * kh * kw > 2e9              # multiply-adds of the float64 reference: seconds on the CPU from here
    r = _conv_case(KERNEL[kernel], case, dev, terms=terms, x16=x16, ref_on_device=heavy)
    plan = lambda b: case_plan(kernel, case, b, terms, x16, cus)
    alone, B2 = _first_image(kernel, r, case, 1, dev, terms, x16), second_batch(kernel, case, terms, x16, cus)
    assert same_bits(alone, r.plain[0]), f"{case}: the first image's bits differ between B = 1 ({plan(1)}) and B = {B} ({plan(B)})"
    assert same_bits(alone, _first_image(kernel, r, case, B2, dev, terms, x16)), \
        f"{case}: the first image's bits differ between B = 1 ({plan(1)}) and B = {B2} ({plan(B2)})"


@pytest.mark.parametrize("case,terms,want", SPLIT_CASES, ids=case_id)
def test_split_kernel_against_float64_and_across_batches(case, terms, want, dev):
    assert case_plan(SPLIT, case, terms=terms)[:9] == want, POLICY
    _case_and_batches(SPLIT, case, dev, terms=terms)


@pytest.mark.parametrize("x16", [0, 1])
@pytest.mark.parametrize("case,want", F16_CASES, ids=case_id)
def test_f16_kernel_against_float64_and_across_batches(case, want, x16, dev):
    """The launcher moves between 8- and 16-row tiles with the batch: the fp16 mode's batch independence rests on this."""
    assert case_plan(F16, case, x16=x16)[:6] == want, POLICY
    _case_and_batches(F16, case, dev, x16=x16)


@pytest.mark.parametrize("case,want", WINO_CASES, ids=case_id)
def test_wino_kernel_against_float64_and_across_batches(case, want, dev):
    assert case_plan(WINO, case)[:6] == want, POLICY
    _case_and_batches(WINO, case, dev)


@pytest.mark.parametrize("case,terms,want", B3_CASES, ids=case_id)
def test_b3_kernel_against_float64_and_across_batches(case, terms, want, dev):
    assert case_plan(WINO_B3, case, terms=terms, cus=_cus(dev))[:6] == want, POLICY
    _case_and_batches(WINO_B3, case, dev, terms=terms, cus=_cus(dev))


@pytest.mark.parametrize("i,name", [(i, name) for i, (name, _, _) in enumerate(b3_schedule_cases(CUS))])
def test_b3_schedule(i, name, dev):
    cus = _cus(dev)
    got_name, case, tiles = b3_schedule_cases(cus)[i]
    assert got_name == name
    p = case_plan(WINO_B3, case, terms=6, cus=cus)
    assert inst(p) == ("launch_b3", (6,)) and p[9] == min(tiles, cus), (p, POLICY)
    _case_and_batches(WINO_B3, case, dev, terms=6, cus=cus)
