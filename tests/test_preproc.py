"""CPU: the C ABI of the image pre-processing entry points and their host-side refusals, the Python-side argument checks, the two
NumPy restatements of the contract (tests/preproc_restatement.py) against each other and against hand-computed cases, the exact removal
of an additive background, run.py's refusals and stream_pairs' `prep` hook.  Everything is compared bit for bit.  No GPU."""
import os
import re

import numpy as np
import pytest

import preproc_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW = ("pivlfn_frames_preprocess", "pivlfn_frames_background_min")
SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (13, 17)]


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_and_signatures_carry_the_new_entries():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pivlfn.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
    from pivlfn import _lib
    assert set(NEW) <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW) and lib.pivlfn_abi_version() == 3


def test_entries_refuse_bad_arguments_without_a_gpu():
    """Refused on the host with PIVLFN_ERR_ARG and a message naming the problem, before anything is launched (a launch on a
    machine without a GPU would return PIVLFN_ERR_HIP instead)."""
    from pivlfn import _lib
    lib = _lib.load()
    P, Q, R = 1 << 20, 1 << 24, 1 << 28           # non-null pointers that are never dereferenced, far enough apart not to overlap

    def refused(rc, *words):
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    def pre(frames=P, bg=Q, out=R, n=1, H=4, W=4, k=3, floor=16):
        return lib.pivlfn_frames_preprocess(frames, bg, out, n, H, W, k, floor, None)

    refused(pre(frames=None), "frames_preprocess", "null")
    refused(pre(out=None), "frames_preprocess", "null")
    refused(pre(frames=None, bg=None), "null")
    refused(pre(n=0), "n=0")
    refused(pre(n=-3), "n=-3")
    refused(pre(H=0), "H=0")
    refused(pre(W=-1), "W=-1")
    refused(pre(H=26755, W=26755), "2^31")
    refused(pre(n=70000), "n=70000", "65535")
    for k in (1, 2, 4, 30, 33, -3, -1):
        refused(pre(k=k), f"k={k}")
        refused(pre(k=k, bg=None), f"k={k}")
    for fl in (0, 256, -16):
        refused(pre(floor=fl), f"floor={fl}")
        refused(pre(floor=fl, k=0), f"floor={fl}")
    refused(pre(out=P), "out aliases frames")
    refused(pre(out=P + 8), "out aliases frames")             # frames is 48 bytes here: out begins inside it
    refused(pre(out=P - 100, n=2), "out aliases frames")      # out is 384 bytes: it runs into frames
    refused(pre(out=Q), "out aliases bg")

    def bgm(frames=P, bg=Q, n=1, H=4, W=4):
        return lib.pivlfn_frames_background_min(frames, bg, n, H, W, None)

    refused(bgm(frames=None), "frames_background_min", "null")
    refused(bgm(bg=None), "frames_background_min", "null")
    refused(bgm(n=0), "n=0")
    refused(bgm(H=-2), "H=-2")
    refused(bgm(W=0), "W=0")
    refused(bgm(H=26755, W=26755), "2^31")
    refused(bgm(bg=P), "bg aliases frames")
    refused(bgm(bg=P + 48, n=2), "bg aliases frames")
    with pytest.raises(ValueError):
        _lib.check(pre(k=4), "frames_preprocess")


# ---- Python side ---------------------------------------------------------------------------------------------------------------
def test_python_side_argument_errors():
    import torch
    import pivlfn
    from pivlfn import preproc as P
    assert pivlfn.preprocess_frames is P.preprocess_frames and pivlfn.FrameBackground is P.FrameBackground
    P.check_params(0, 16)
    P.check_params(31, 255)
    P.check_params(3, 1)
    for minmax, floor in ((1, 16), (2, 16), (4, 16), (33, 16), (-3, 16), (3.0, 16), ("3", 16), (True, 16), (None, 16),
                          (3, 0), (3, 256), (3, -1), (3, 16.0), (0, 0), (3, None)):
        with pytest.raises(ValueError):
            P.check_params(minmax, floor)
    frames = torch.zeros(2, 4, 5, 3, dtype=torch.uint8)
    for kw in (dict(minmax=4), dict(floor=0), dict(minmax=5, floor=300)):
        with pytest.raises(ValueError):
            P.preprocess_frames(frames, **kw)                 # parameters are checked before the tensor and the library
        with pytest.raises(ValueError):
            P.Preprocessor(**kw)
    with pytest.raises(NotImplementedError):
        P.preprocess_frames(frames)
    with pytest.raises(NotImplementedError):
        P.preprocess_frames(frames, minmax=7)
    with pytest.raises(NotImplementedError):
        P.preprocess_frames(torch.zeros(2, 4, 5, dtype=torch.uint8))      # a CPU tensor is refused before its shape is looked at
    with pytest.raises(TypeError):
        P.preprocess_frames(frames.float())
    with pytest.raises(TypeError):
        P.preprocess_frames(frames.numpy())
    with pytest.raises(NotImplementedError):
        P.FrameBackground(4, 4, device="cpu")
    for H, W in ((0, 4), (4, -1)):
        with pytest.raises(ValueError):
            P.FrameBackground(H, W, device="cuda:0")
    # what the GPU side checks after the device, on stand-ins that only claim to be on one
    meta = torch.zeros(2, 4, 5, 3, dtype=torch.uint8, device="meta")
    with pytest.raises(NotImplementedError):
        P.preprocess_frames(meta)


# ---- the two restatements against each other ------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_loops_and_vectorised_restatement_agree(H, W):
    rng = np.random.default_rng(1000 * H + W)
    img = rng.integers(0, 256, (H, W), dtype=np.uint8)
    bg = rng.integers(0, 128, (H, W), dtype=np.uint8)
    for k in (3, 7, 15, 31):
        num_l, span_l = pr.terms_loops(pr.subtract(img, bg), k)
        num_v, span_v = pr.terms_plane(pr.subtract(img, bg), k)
        assert np.array_equal(num_l, num_v) and np.array_equal(span_l, span_v), (H, W, k)
        for floor in (1, 16, 255):
            want = pr.finish(num_l, span_l, k, floor)         # = preprocess_loops, with the loops run once per k
            assert pr.same_bits32(pr.preprocess_plane(img, bg, k, floor), want), (H, W, k, floor)
    for k, floor in ((3, 16), (7, 1)):                        # the whole definition, and without a background
        assert pr.same_bits32(pr.preprocess_loops(img, bg, k, floor), pr.preprocess_plane(img, bg, k, floor))
        assert pr.same_bits32(pr.preprocess_loops(img, None, k, floor), pr.preprocess_plane(img, None, k, floor))
    assert pr.same_bits32(pr.preprocess_loops(img, bg, 0), pr.preprocess_plane(img, bg, 0))


# ---- hand-computed cases -----------------------------------------------------------------------------------------------------------
def test_constant_image_gives_zero():
    """lo = hi = x everywhere, so L = n x and num = 0: the output is +0.0 whatever the value, the window and the floor."""
    for v in (0, 1, 77, 255):
        for k in (3, 15, 31):
            for plane in (pr.preprocess_loops, pr.preprocess_plane):
                out = plane(np.full((4, 6), v, np.uint8), None, k, 16)
                assert pr.same_bits32(out, np.zeros((4, 6), f32)), (v, k)


def test_single_spike_in_a_5x5_image():
    """x = 0 except x[2,2] = 255, k = 3, n = 9, floor = 16 (floor*n = 144).  lo = 0 everywhere, so L = 0.  hi = 255 on the 3 x 3 block
    around the spike (rows and columns 1..3) and 0 on the outer ring.
      spike (2,2):     S = 9 * 255 = 2295, num = 9 * 255 = 2295, den = 2295 -> 1.
      neighbour (2,1): its window covers columns 0..2, rows 1..3: the six positions in columns 1, 2 hold 255: S = 1530; num = 0 -> 0.
      corner (0,0):    clamped window = positions (0|0|1) x (0|0|1): only (1,1) holds 255, once: S = 255, num = 0, den = 255 -> 0.
    With floor = 255 nothing changes at the spike (2295 >= 255 * 9 = 2295); a spike of 254 falls below it:
      S = num = 9 * 254 = 2286, den = 2295 -> fl(2286 / 2295)."""
    img = np.zeros((5, 5), np.uint8)
    img[2, 2] = 255
    for plane in (pr.preprocess_loops, pr.preprocess_plane):
        num, span = (pr.terms_loops if plane is pr.preprocess_loops else pr.terms_plane)(pr.subtract(img), 3)
        assert num[2, 2] == 2295 and span[2, 2] == 2295 and span[2, 1] == 1530 and span[0, 0] == 255 and span[1, 1] == 4 * 255
        assert span[0, 1] == 2 * 255 and span[0, 2] == 3 * 255 and num.sum() == 2295
        out = plane(img, None, 3, 16)
        want = np.zeros((5, 5), f32)
        want[2, 2] = 1.0
        assert pr.same_bits32(out, want)
        assert pr.same_bits32(plane(img, None, 3, 255), want)
        img2 = img.copy()
        img2[2, 2] = 254
        want[2, 2] = f32(2286) / f32(2295)
        assert pr.same_bits32(plane(img2, None, 3, 255), want) and want[2, 2] < 1
        # the spike as background leaves nothing
        assert not plane(img, img, 3, 16).any()


def test_step_image_takes_the_floor_on_one_side_only():
    """1 x 8, k = 3 (n = 9; a one-row image repeats its row three times, so every sum is 3 x the 1-D one), floor = 16 (144):
         x  = 10 10 10 10 | 10 100 10 100
         lo = 10 everywhere, L = 90;  hi = 10 10 10 10 100 100 100 100,  S = 3 * (30, 30, 30, 120, 210, 300, 300, 300)
         S - L = 0 0 0 270 540 810 810 810: the three flat pixels on the left take the floor 144, the others their own span.
         num = 9 x - 90 = 0 0 0 0 0 810 0 810  ->  out = 0 0 0 0 0 1 0 1."""
    img = np.array([[10, 10, 10, 10, 10, 100, 10, 100]], np.uint8)
    for terms, plane in ((pr.terms_loops, pr.preprocess_loops), (pr.terms_plane, pr.preprocess_plane)):
        num, span = terms(pr.subtract(img), 3)
        assert num.tolist() == [[0, 0, 0, 0, 0, 810, 0, 810]] and span.tolist() == [[0, 0, 0, 270, 540, 810, 810, 810]]
        assert plane(img, None, 3, 16).tolist() == [[0, 0, 0, 0, 0, 1, 0, 1]]
        # a brighter flat side shows the floor at work: x = 12 among 10s spans 2 grey levels, far below 16
        img2 = img.copy()
        img2[0, 1] = 12
        num, span = terms(pr.subtract(img2), 3)
        assert num[0, 1] == 9 * 12 - 90 and span[0, 1] == 3 * 3 * 2 and span[0, 1] < 144
        assert plane(img2, None, 3, 16)[0, 1] == f32(18) / f32(144) and plane(img2, None, 3, 1)[0, 1] == f32(1)


# ---- properties ----------------------------------------------------------------------------------------------------------------------
def test_num_and_den_stay_ordered_and_the_plain_path_is_the_table():
    rng = np.random.default_rng(7)
    table = np.arange(256, dtype=f32) / f32(255)
    for H, W in ((9, 40), (33, 21)):
        img = rng.integers(0, 256, (H, W), dtype=np.uint8)
        bg = rng.integers(0, 256, (H, W), dtype=np.uint8)
        for k in (3, 9, 31):
            for b in (None, bg):
                num, span = pr.terms_plane(pr.subtract(img, b), k)
                for floor in (1, 16, 255):
                    den = np.maximum(span, floor * k * k)
                    assert (0 <= num).all() and (num <= den).all() and den.max() < 1 << 24
        assert pr.same_bits32(pr.preprocess_plane(img), table[img]) and pr.same_bits32(pr.preprocess_loops(img), table[img])
        frames = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
        assert pr.same_bits32(pr.preprocess(frames), table[frames].transpose(0, 3, 1, 2))
        assert pr.same_bits32(pr.preprocess(frames, frames[1])[1], np.zeros((3, H, W), f32))
    stack = rng.integers(0, 256, (5, 4, 6, 3), dtype=np.uint8)
    assert np.array_equal(pr.background_min(stack), stack.min(0))
    assert np.array_equal(pr.background_min(stack[3:], pr.background_min(stack[:3])), stack.min(0))
    assert (pr.background_min(stack[:0]) == 255).all()


def test_additive_background_is_removed_exactly():
    """F_t = P_t + G with particle images P_t <= 127 and a smooth background G <= 127: min_t F = min_t P + G, so subtracting the
    temporal minimum leaves the same integers with and without G and the outputs agree at every pixel, bit for bit.  Without the
    background subtraction G changes the result on most pixels."""
    from pivlfn import synth
    H = W = 256
    P = np.stack([synth.particle_pair(H, W, 4100 + s)[0] >> 1 for s in range(6)])
    G = pr.smooth_background(H, W)
    assert P.dtype == np.uint8 and G.dtype == np.uint8 and int(G.max()) == 104 and int(G.min()) == 0
    assert int(P.max()) <= 127 and int(G.max()) <= 127 and int(P.max()) > 60        # nothing saturates
    F = P + G[None]
    assert F.dtype == np.uint8 and np.array_equal(F.astype(np.int64), P.astype(np.int64) + G)
    bgF, bgP = pr.background_min(F), pr.background_min(P)
    assert np.array_equal(bgF.astype(np.int64), bgP.astype(np.int64) + G)
    with_bg = pr.preprocess_plane(F[0], bgF, 15)
    clean = pr.preprocess_plane(P[0], bgP, 15)
    assert pr.same_bits32(with_bg, clean)
    without = pr.preprocess_plane(F[0], None, 15)
    differ = float((without.view(np.int32) != clean.view(np.int32)).mean())
    print(f"without the background subtraction {100 * differ:.1f} % of the pixels differ")
    assert differ > 0.5
    assert float(clean.max()) > 0.5 and 0.0 <= float(clean.min())


# ---- run.py and stream_pairs ------------------------------------------------------------------------------------------------------------
def test_run_py_refuses_the_new_flags_with_modifications_or_bad_parameters(tmp_path, monkeypatch):
    import run as runpy
    base = ["--model", "piv", "-i", str(tmp_path), "-o", str(tmp_path / "out")]
    for flags in (["--background", "min"], ["--minmax", "15"], ["--minmax", "15", "--minmax-floor", "8"],
                  ["--background", str(tmp_path / "bg.png")]):
        for extra in (["-b", "1.2"], ["-c", "0.8"]):
            with pytest.raises(SystemExit, match="-b/-c"):
                runpy.main(base + flags + extra)
    for flags, word in ((["--minmax", "4"], "minmax=4"), (["--minmax", "33"], "minmax=33"),
                        (["--minmax", "7", "--minmax-floor", "0"], "floor=0"), (["--minmax-floor", "8"], "needs --minmax"),
                        (["--background", str(tmp_path / "none.png")], "neither")):
        with pytest.raises(SystemExit, match=word):
            runpy.main(base + flags)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="single process"):
        runpy.main(base + ["--background", "min"])
    with pytest.raises(SystemExit, match="single process"):
        runpy.main(base + ["--background", "min", "--minmax", "15", "--stats"])
    assert not (tmp_path / "out").exists()
    args = runpy.parser.parse_args([])
    assert args.background is None and args.minmax is None and args.minmax_floor is None


def test_stream_pairs_routes_frames_through_prep():
    """The CPU rehearsal of stream_pairs with stand-ins: `prep` is called once per frame tensor of a batch and estimate_fn gets
    exactly what it returned; without `prep` the frames go through u8_to_input as before."""
    import torch
    from pivlfn import pipeline
    rng = np.random.default_rng(3)
    batches = [([f"p{b}_{i}" for i in range(n)], torch.from_numpy(rng.integers(0, 256, (n, 4, 6, 3), dtype=np.uint8)),
                torch.from_numpy(rng.integers(0, 256, (n, 4, 6, 3), dtype=np.uint8))) for b, n in enumerate((2, 2, 1))]
    seen_by_prep, made_by_prep, seen_by_est = [], [], []

    def prep(x):
        seen_by_prep.append(x)
        y = x.permute(0, 3, 1, 2).to(torch.float32) * 0.5 + float(len(seen_by_prep))
        made_by_prep.append(y)
        return y

    def estimate_fn(net, a, b, tensor=True):
        seen_by_est.append((a, b))
        return (a[:, :2] - b[:, :2]).contiguous()

    got = []
    n = pipeline.stream_pairs(None, batches, torch.device("cpu"), lambda flow, name: got.append((name, flow.copy())),
                              estimate_fn=estimate_fn, prep=prep)
    assert n == 5 and [g[0] for g in got] == ["p0_0", "p0_1", "p1_0", "p1_1", "p2_0"]
    assert len(seen_by_prep) == 6 and len(seen_by_est) == 3
    for b, (names, a8, b8) in enumerate(batches):
        assert seen_by_prep[2 * b] is a8 and seen_by_prep[2 * b + 1] is b8
        assert seen_by_est[b][0] is made_by_prep[2 * b] and seen_by_est[b][1] is made_by_prep[2 * b + 1]
    assert np.array_equal(got[4][1], (made_by_prep[4][0, :2] - made_by_prep[5][0, :2]).permute(1, 2, 0).numpy())

    seen_by_est.clear()
    n = pipeline.stream_pairs(None, batches, torch.device("cpu"), lambda flow, name: None, estimate_fn=estimate_fn)
    assert n == 5 and len(seen_by_prep) == 6
    for b, (names, a8, b8) in enumerate(batches):
        assert torch.equal(seen_by_est[b][0], pipeline.u8_to_input(a8)) and torch.equal(seen_by_est[b][1], pipeline.u8_to_input(b8))
