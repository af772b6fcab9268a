"""CPU: the guarded-buffer checks of tests/test_gpu_guarded.py catch what they are there to catch.  On CPU tensors, each defect below
is detected: a word written one element past or before a payload, a store into a lane that is not stored, a restatement that reads
one lane past cin (with either poison kind; through an fmaxf-style clamp only `big` sees it, which is why every check runs with
both), and a two-stage pipeline whose second stage reads a workspace lane the first did not write.  The defect-free versions pass."""
import pytest
import torch

from guarded import KINDS, check_guards, check_lanes, guarded, poison, same_bits


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_guarded_layout(dtype):
    t = guarded((3, 5, 7, 8), dtype, fill="sentinel")
    r = t._guarded
    assert t.data_ptr() % 256 == 0
    assert t.data_ptr() + t.numel() * t.element_size() == r.buf.data_ptr() + r.off + r.nbytes      # flush against the back guard
    assert r.off >= 1 << 20 and r.buf.numel() - r.off - r.nbytes >= 1 << 20
    check_lanes(t, slice(0, 8), "sentinel")
    t.zero_()
    check_guards(t, "zeroed payload")


def test_guards_are_32_rows_of_a_large_tensor():
    t = guarded((1, 300, 300, 64), torch.float32, fill="nan")
    r = t._guarded
    assert r.off >= 32 * 300 * 64 * 4 and r.buf.numel() - r.off - r.nbytes >= 32 * 300 * 64 * 4


@pytest.mark.parametrize("fill", ["nan", "big", "sentinel"])
def test_one_word_past_the_payload_is_caught(fill):
    t = guarded((2, 9, 11, 4), fill=fill)
    t.fill_(1.0)
    check_guards(t)
    r = t._guarded
    w = r.buf.view(torch.int32)
    w[(r.off + r.nbytes) // 4] = 0x3F800000                     # one int32 right after the last element
    with pytest.raises(AssertionError, match="after the payload changed, first at 0 bytes after"):
        check_guards(t, "one past")


@pytest.mark.parametrize("fill", ["nan", "big", "sentinel"])
def test_one_word_before_the_payload_is_caught(fill):
    t = guarded((2, 9, 11, 4), fill=fill)
    r = t._guarded
    r.buf.view(torch.int32)[r.off // 4 - 1] = 0
    with pytest.raises(AssertionError, match="before the payload changed, first at -4 bytes before"):
        check_guards(t, "one before")


def test_a_store_into_a_lane_that_is_not_stored_is_caught():
    y = guarded((2, 5, 6, 12), fill="sentinel")
    y[..., :9] = 1.0                                             # a kernel storing cout = 9 channels ...
    y[..., 9:10] = 0.0                                           # ... and its zero lanes up to roundup(9, 4) = 12 minus two
    check_lanes(y, slice(10, 12), "sentinel")
    y[1, 4, 5, 11] = 0.0                                         # one store too many
    with pytest.raises(AssertionError, match="must hold sentinel"):
        check_lanes(y, slice(10, 12), "sentinel")
    z = guarded((1, 2, 2, 8), fill="sentinel")
    z[..., 4:] = -0.0                                            # -0.0 is not the +0.0 a zero lane must hold
    with pytest.raises(AssertionError, match="must hold zero"):
        check_lanes(z, slice(4, 8), "zero")


# ---- a restatement that reads one lane past cin --------------------------------------------------------------------------------
def _dot(x, w, cin, extra):
    """A 1 x 1 convolution over the first cin (+ extra) lanes of channels-last x, float64."""
    return (x[..., :cin + extra].double() * w[:cin + extra].double()).sum(-1)


def _tap(x, cin, extra, W):
    """A clamped sample position taken from lane cin - 1 (+ extra): fminf(fmaxf(v, 0), W - 1), which maps NaN to 0."""
    v = x[..., cin - 1 + extra]
    return torch.fmin(torch.fmax(v, torch.zeros_like(v)), torch.full_like(v, W - 1.0))


def _inputs(cin, xs, kind):
    g = torch.Generator().manual_seed(cin)
    data = torch.rand(2, 6, 7, cin, generator=g)
    plain = torch.zeros(2, 6, 7, xs)
    plain[..., :cin] = data
    bad = guarded((2, 6, 7, xs), fill=kind)
    bad[..., :cin] = data
    poison(bad, slice(cin, xs), kind)
    return plain, bad


@pytest.mark.parametrize("kind", KINDS)
def test_a_read_past_cin_is_caught_by_both_poisons(kind):
    cin, xs = 5, 8
    w = torch.randn(xs) + 2.0                                    # the weight of lane cin is not zero in the defective version
    plain, bad = _inputs(cin, xs, kind)
    assert same_bits(_dot(bad, w, cin, 0), _dot(plain, w, cin, 0))      # the right restatement: same bits on poisoned input
    assert not same_bits(_dot(bad, w, cin, 1), _dot(plain, w, cin, 1))  # one lane too many: detected


@pytest.mark.parametrize("kind", KINDS)
def test_a_read_past_cin_through_a_clamp_needs_big(kind):
    cin, xs, W = 5, 8, 7
    plain, bad = _inputs(cin, xs, kind)
    assert same_bits(_tap(bad, cin, 0, W), _tap(plain, cin, 0, W))
    caught = not same_bits(_tap(bad, cin, 1, W), _tap(plain, cin, 1, W))
    assert caught == (kind == "big"), "the clamp turns a NaN into the in-range tap 0, the value a zero lane gives"


# ---- a workspace lane that no stage writes ---------------------------------------------------------------------------------------
def _pipeline(x, ws, skip_last):
    """Stage 1 writes ws[..., :4] = 2x (all but lane 3 when skip_last); stage 2 reads ws[..., :4] and sums it."""
    n = 3 if skip_last else 4
    ws[..., :n] = 2.0 * x[..., :n]
    return ws[..., :4].sum(-1)


@pytest.mark.parametrize("skip_last", [False, True])
def test_a_workspace_lane_nobody_wrote_is_caught(skip_last):
    x = torch.rand(3, 5, 4, generator=torch.Generator().manual_seed(2))
    outs = []
    for fill in ("zero",) + KINDS:
        ws = guarded((3, 5, 4), fill="nan" if fill == "zero" else fill)
        if fill == "zero":
            ws.zero_()
        else:
            poison(ws, slice(0, 4), fill)
        outs.append(_pipeline(x, ws, skip_last))
        check_guards(ws)
    same = all(same_bits(o, outs[0]) for o in outs[1:])
    assert same != skip_last
