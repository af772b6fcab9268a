"""Guarded buffers and poisoned lanes: what a kernel reads and writes OUTSIDE the elements it is meant to touch.

guarded() places a tensor inside one flat device buffer, between a front and a back guard of known bits.  The payload starts 256-byte
aligned (pivlfn_forward's requirement) and its last byte lies directly against the back guard, so a read or write one element past
either end lands in guard memory.  Guards are max(1 MiB, 32 rows of the tensor) long: a stray tile row, halo or K step stays inside
the allocation.  check_guards() compares them bit for bit afterwards and names the first word that changed.

poison() fills lanes a contract says are unused.  Two kinds, and every check runs once with each:
  nan  a quiet NaN with a recognisable payload: caught by any arithmetic, but min / max clamps (fminf / fmaxf) drop it;
  big  finite values of mixed sign near 1e30 (about 1e38 / 300): one multiply-add with a weight of the network's size stays
       finite, clamps keep it, and it moves any sum it enters far past a tolerance.
Plain Python / torch, device-agnostic: tests/test_guarded_yardstick.py checks the helper itself on CPU tensors."""
import torch

NAN_BITS = 0x7FC0BEEF                         # quiet NaN, payload 0x40BEEF: the poison and the input-side guard fill
SENTINEL_BITS = 0x7FC5E471                    # quiet NaN of another payload: outputs are pre-filled with it
BIG_BITS = (0x71497C13, -0x0EBC5E1D)          # +0.998e30 and -0.969e30 (0xF143A1E3): a finite two-word pattern
NAN16_BITS, SENTINEL16_BITS = 0x7E5F, 0x7E71    # fp16 quiet NaNs
BIG16_BITS = (0x7A9D, -0x056C)                  # fp16 +54176 and -53888 (0xFA94)
KINDS = ("nan", "big")
ALIGN = 256


def _pattern(kind, dtype):
    if dtype == torch.float16:
        return {"nan": (NAN16_BITS,), "sentinel": (SENTINEL16_BITS,), "big": BIG16_BITS}[kind]
    if kind == "nan":
        return (NAN_BITS,)
    if kind == "sentinel":
        return (SENTINEL_BITS,)
    if kind == "big":
        return BIG_BITS
    raise ValueError(kind)


def _int_view(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _fill_bits(words, pattern):
    """words: a 1-D integer view; repeats `pattern` along it."""
    if len(pattern) == 1:
        words.fill_(pattern[0])
    else:
        for k, p in enumerate(pattern):
            words[k::len(pattern)] = p


def guard_bytes_for(shape, dtype):
    es = torch.empty(0, dtype=dtype).element_size()
    row = es * (shape[-1] * shape[-2] if len(shape) >= 2 else 0)
    g = max(1 << 20, 32 * row)
    return -(-g // ALIGN) * ALIGN


class _Record:
    def __init__(self, buf, off, nbytes, fill):
        self.buf, self.off, self.nbytes, self.fill = buf, off, nbytes, fill

    def regions(self):
        w = self.buf.view(torch.int32)
        return (("before", w[:self.off // 4], self.off // 4), ("after", w[(self.off + self.nbytes) // 4:], 0))


def guarded(shape, dtype=torch.float32, dev="cpu", fill="nan", guard_bytes=None):
    """A [shape] tensor of `dtype` inside a guarded buffer.  fill: the guards' pattern ("nan", "big" or "sentinel"); the payload is
    pre-filled with the same pattern.  Returns the payload view; the whole buffer is kept on it for check_guards()."""
    shape = tuple(int(s) for s in shape)
    es = torch.empty(0, dtype=dtype).element_size()
    n = 1
    for s in shape:
        n *= s
    nbytes = n * es
    assert nbytes % 4 == 0, "guarded(): the payload must be a whole number of 32-bit words"
    g = guard_bytes if guard_bytes is not None else guard_bytes_for(shape, dtype)
    g = -(-max(g, 4) // ALIGN) * ALIGN
    buf = torch.empty(g + nbytes + g + ALIGN, dtype=torch.uint8, device=dev)
    off = g + (-(buf.data_ptr() + g) % ALIGN)                   # payload 256-byte aligned, at least g bytes of front guard
    buf = buf[:off + nbytes + g]                                # the back guard starts at the payload's last byte + 1
    _fill_bits(buf.view(torch.int32), _pattern(fill, torch.float32))
    t = buf[off:off + nbytes].view(dtype).view(shape)
    if dtype == torch.float16:
        _fill_bits(_int_view(t).view(-1), _pattern(fill, dtype))
    t._guarded = _Record(buf, off, nbytes, fill)
    return t


def check_guards(t, what=""):
    """Assert that the guards around a guarded() tensor hold their bits.  The message names the first changed byte offset,
    counted from the payload's start (negative: before it) or from its end (after it)."""
    r = t._guarded
    pat = _pattern(r.fill, torch.float32)
    for side, words, n_before in r.regions():
        want = torch.empty_like(words)
        _fill_bits(want, pat if side == "before" or len(pat) == 1 else
                   tuple(pat[(k + (r.off + r.nbytes) // 4) % len(pat)] for k in range(len(pat))))
        if not torch.equal(words, want):
            k = int((words != want).nonzero()[0, 0])
            where = f"{(k - n_before) * 4} bytes before the payload's start" if side == "before" else \
                f"{k * 4} bytes after the payload's end"
            raise AssertionError(f"{what}: guard {side} the payload changed, first at {where}")


def poison(t, lanes, kind):
    """Fill t[..., lanes] (lanes: a slice of the last dimension) with the `kind` pattern ("nan", "big" or "sentinel")."""
    v = t[..., lanes]
    if v.numel() == 0:
        return t
    pat = _pattern(kind, t.dtype)
    if v.is_contiguous():
        _fill_bits(_int_view(v).view(-1), pat)
    elif len(pat) == 1:
        v.copy_(torch.tensor(pat[0], dtype=_int_view(t).dtype).view(t.dtype).expand_as(v))
    else:
        k = torch.arange(v.numel(), device=t.device).view(v.shape) % len(pat)
        vals = torch.tensor(pat, dtype=_int_view(t).dtype, device=t.device).view(t.dtype)
        v.copy_(vals[k])
    return t


def holds(t, kind):
    """True where t holds the `kind` pattern bit for bit (for single-word patterns: the sentinel and nan)."""
    pat = _pattern(kind, t.dtype)
    assert len(pat) == 1
    return _int_view(t) == pat[0]


def is_pos_zero(t):
    return _int_view(t) == 0


def check_lanes(t, lanes, kind, what=""):
    """Assert that every element of t[..., lanes] holds `kind` bit for bit: "sentinel" (never stored) or "zero" (+0.0)."""
    v = t[..., lanes]
    ok = is_pos_zero(v) if kind == "zero" else holds(v, kind)
    if not bool(ok.all()):
        k = (~ok).nonzero()[0].tolist()
        raise AssertionError(f"{what}: lanes {lanes.start}..{lanes.stop - 1} must hold {kind}; element {k} of them holds "
                             f"{float(v[tuple(k)])}")


def same_bits(a, b):
    """Bitwise equality of two tensors of one dtype and shape (NaNs compare by their bits)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_int_view(a.contiguous()), _int_view(b.contiguous()))
