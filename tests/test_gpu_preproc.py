"""GPU: pivlfn_frames_preprocess and pivlfn_frames_background_min (csrc/preproc.hip), preprocess_frames, FrameBackground, the `prep`
hooks of stream_pairs / run_sequence and run.py --background / --minmax -- against the NumPy restatement of
tests/preproc_restatement.py, bit for bit.  No tolerance appears anywhere."""
import numpy as np
import pytest
import torch

import analysis_plans as ap
import pivlfn
import preproc_restatement as pr
from guarded import check_guards, guarded, holds
from pivlfn import _lib, pipeline, synth
from pivlfn import preproc as P
from pivlfn.flo import read_flow

pytestmark = pytest.mark.gpu

f32 = np.float32
KS, FLOORS = (0, 3, 7, 15, 31), (1, 16, 255)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded_u8(shape, dev, fill="nan"):
    """guarded() for any number of bytes: the tensor ends at the back guard; when its size is not a whole number of 32-bit words the
    1..3 bytes in front of it belong to the payload, keep the fill and are returned for a check of their own.  Such a tensor starts
    at an odd address, as a slice of a larger batch would."""
    n = int(np.prod(shape))
    pad = -n % 4
    flat = guarded((n + pad,), torch.uint8, dev, fill)
    t = flat[pad:].view(*shape)
    t._guarded = flat._guarded
    t._front = (flat[:pad], flat[:pad].clone())
    return t


def _check_u8(t, what):
    check_guards(t, what)
    assert torch.equal(*t._front), what + ": a byte in front of the tensor changed"


def _call(dev, frames, bg, k, floor, fill="sentinel", what=""):
    """pivlfn_frames_preprocess on guarded copies of `frames` (uint8 [n,H,W,3] numpy) and `bg` into a guarded, pre-poisoned output:
    nothing outside any buffer changes and every output element is written.  Returns the output as numpy."""
    n, H, W, _ = frames.shape
    fr = _guarded_u8(frames.shape, dev)
    fr.copy_(torch.from_numpy(frames))
    b = None
    if bg is not None:
        b = _guarded_u8(bg.shape, dev)
        b.copy_(torch.from_numpy(bg))
    out = guarded((n, 3, H, W), torch.float32, dev, fill)
    _lib.check(_lib.load().pivlfn_frames_preprocess(fr.data_ptr(), b.data_ptr() if b is not None else None, out.data_ptr(), n, H, W, k,
                                                    floor, _lib.stream_ptr(out.device)), what)
    torch.cuda.synchronize()
    check_guards(out, what + " out")
    _check_u8(fr, what + " frames")
    assert torch.equal(fr.cpu(), torch.from_numpy(frames)), what + ": the frames changed"
    if b is not None:
        _check_u8(b, what + " bg")
        assert torch.equal(b.cpu(), torch.from_numpy(bg)), what + ": the background changed"
    if fill == "sentinel":
        assert not bool(holds(out, "sentinel").any()), what + ": an output element was not written"
    return out.cpu().numpy()


def _particles_rgb(n, H, W, seed):
    """n RGB frames [n,H,W,3] of halved particle images (three different channels: the two frames of a synthetic pair and their
    mean) on three different smooth backgrounds, and those backgrounds [H,W,3]; nothing saturates."""
    G = pr.smooth_background(H, W)
    G = np.stack([G, G[::-1, ::-1], np.ascontiguousarray(pr.smooth_background(W, H).T)], axis=-1)
    pairs = [synth.particle_pair(H, W, seed + t)[:2] for t in range(n)]
    Pt = np.stack([np.stack([a >> 1, b >> 1, (a >> 2) + (b >> 2)], axis=-1) for a, b in pairs])
    assert int(Pt.max()) <= 127 and int(G.max()) <= 127
    return Pt + G[None], G


# ---- the kernel against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (5, 3), (37, 53)])
def test_small_images_match_restatement(dev, H, W):
    """Every window, floor, with and without a background, one frame and five: images smaller than the window included."""
    rng = np.random.default_rng(100 * H + W)
    for n in (1, 5):
        frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
        bg = rng.integers(0, 160, (H, W, 3), dtype=np.uint8)
        for k in KS:
            for b in (None, bg):
                terms = None if k == 0 else [[pr.terms_plane(pr.subtract(frames[t, :, :, c], None if b is None else b[:, :, c]), k)
                                              for c in range(3)] for t in range(n)]
                for floor in FLOORS:
                    if k == 0:
                        want = pr.preprocess(frames, b, 0, floor)
                    else:
                        want = np.stack([np.stack([pr.finish(*terms[t][c], k, floor) for c in range(3)]) for t in range(n)])
                    tag = f"{H}x{W} n={n} k={k} floor={floor} bg={b is not None}"
                    got = _call(dev, frames, b, k, floor, "sentinel" if floor != 16 else "big", tag)
                    assert pr.same_bits32(got, want), tag
    if (H, W) == (5, 3):                                       # the definition itself, once
        got = _call(dev, frames, bg, 7, 16)
        assert pr.same_bits32(got, pr.preprocess(frames, bg, 7, 16, plane=pr.preprocess_loops))


def test_noise_64x64_matches_restatement(dev):
    """Uniform noise: every window has a different minimum and maximum, the worst case for the min / max passes."""
    rng = np.random.default_rng(64)
    frames = rng.integers(0, 256, (3, 64, 64, 3), dtype=np.uint8)
    bg = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    for k in KS:
        for b in (None, bg):
            for floor in (1, 16):
                tag = f"noise k={k} floor={floor} bg={b is not None}"
                assert pr.same_bits32(_call(dev, frames, b, k, floor, what=tag), pr.preprocess(frames, b, k, floor)), tag


def test_hand_computed_cases(dev):
    """The cases worked out in tests/test_preproc.py, on the device."""
    def one(img, k, floor, bg=None):
        rgb = np.repeat(np.asarray(img, np.uint8)[None, :, :, None], 3, axis=3)
        b = None if bg is None else np.repeat(np.asarray(bg, np.uint8)[:, :, None], 3, axis=2)
        out = _call(dev, rgb, b, k, floor)
        assert pr.same_bits32(out[0, 0], out[0, 1]) and pr.same_bits32(out[0, 0], out[0, 2])
        return out[0, 0]

    for v in (0, 1, 77, 255):
        for k in (3, 15, 31):
            assert pr.same_bits32(one(np.full((4, 6), v), k, 16), np.zeros((4, 6), f32)), (v, k)
    spike = np.zeros((5, 5), np.uint8)
    spike[2, 2] = 255
    want = np.zeros((5, 5), f32)
    want[2, 2] = 1.0
    assert pr.same_bits32(one(spike, 3, 16), want) and pr.same_bits32(one(spike, 3, 255), want)
    assert not one(spike, 3, 16, bg=spike).any()
    spike[2, 2] = 254
    want[2, 2] = f32(2286) / f32(2295)
    assert pr.same_bits32(one(spike, 3, 255), want)
    step = np.array([[10, 10, 10, 10, 10, 100, 10, 100]], np.uint8)
    assert one(step, 3, 16).tolist() == [[0, 0, 0, 0, 0, 1, 0, 1]]
    step[0, 1] = 12
    assert one(step, 3, 16)[0, 1] == f32(18) / f32(144) and one(step, 3, 1)[0, 1] == f32(1)


@pytest.mark.parametrize("H,W", [(1024, 1024), (1000, 1016)])
def test_megapixel_particle_frames_match_restatement(dev, H, W):
    """Full-size synthetic recordings with a background, n = 2: every tile boundary and partial tile of the kernel's tiling, against
    the vectorised restatement; and the additive background is removed exactly on the device too."""
    frames, G = _particles_rgb(2, H, W, 900 + W)
    bg = pr.background_min(frames)
    for k in (15, 31):
        tag = f"{H}x{W} k={k}"
        got = _call(dev, frames, bg, k, 16, what=tag)
        assert pr.same_bits32(got, pr.preprocess(frames, bg, k, 16)), tag
        assert 0.0 <= float(got.min()) and float(got.max()) <= 1.0 and float(got.max()) > 0.5
    clean = frames - G[None]
    got_clean = _call(dev, clean, pr.background_min(clean), 31, 16, what="clean")
    assert pr.same_bits32(got, got_clean)


def test_batch_invariance_and_python_entry(dev):
    """Five frames in one call equal the same frames one call each; preprocess_frames returns what the C entry writes; non-contiguous
    input is accepted; an empty batch gives an empty result."""
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (5, 70, 131, 3), dtype=np.uint8)
    bg = rng.integers(0, 100, (70, 131, 3), dtype=np.uint8)
    t, b = torch.from_numpy(frames).to(dev), torch.from_numpy(bg).to(dev)
    for k in KS:
        whole = P.preprocess_frames(t, b, k, 16)
        assert whole.shape == (5, 3, 70, 131) and whole.dtype == torch.float32 and whole.is_contiguous()
        for i in range(5):
            assert torch.equal(_bits(P.preprocess_frames(t[i:i + 1], b, k, 16)), _bits(whole[i:i + 1])), (k, i)
        assert pr.same_bits32(whole.cpu().numpy(), _call(dev, frames, bg, k, 16))
        assert torch.equal(_bits(P.Preprocessor(b, k, 16)(t)), _bits(whole))
    assert pr.same_bits32(P.preprocess_frames(t.permute(0, 2, 1, 3), None, 7).cpu().numpy(),
                          pr.preprocess(np.ascontiguousarray(frames.transpose(0, 2, 1, 3)), None, 7))
    empty = P.preprocess_frames(t[:0], b, 15)
    assert empty.shape == (0, 3, 70, 131) and empty.dtype == torch.float32
    with pytest.raises(ValueError):
        P.preprocess_frames(t, b[:-1])
    with pytest.raises(ValueError):
        P.preprocess_frames(t, b.cpu())
    with pytest.raises(TypeError):
        P.preprocess_frames(t, b.float())
    with pytest.raises(ValueError):
        P.preprocess_frames(t[..., :2])
    with pytest.raises(ValueError):
        P.preprocess_frames(t[0])


@pytest.mark.parametrize("n,H,W", ap.shapes(ap.PREPROC_CASES))
def test_scale_where_the_frame_grid_is_capped(dev, n, H, W):
    """minmax = 0 with more blocks a frame than the launch's cap, on the four-pixel path (H*W a multiple of 4) and the byte path: the
    kernel's grid-stride loop comes round, and the frames equal the same frames in calls that are not capped, with and without a
    background."""
    rng = np.random.default_rng(H)
    t = torch.from_numpy(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)).to(dev)
    b = torch.from_numpy(rng.integers(0, 100, (H, W, 3), dtype=np.uint8)).to(dev)
    step = ap.FRAMES_PER_UNCAPPED_CALL
    for bg in (b, None):
        whole = P.preprocess_frames(t, bg, 0)
        for k in range(0, n, step):
            assert torch.equal(_bits(P.preprocess_frames(t[k:k + step], bg, 0)), _bits(whole[k:k + step])), (k, bg is None)
    assert torch.equal(_bits(whole), _bits(pipeline.u8_to_input(t)))


def test_plain_path_equals_u8_to_input(dev):
    """minmax = 0 without a background: the bits of pipeline.u8_to_input (ToTensor's division), for every byte value, on the
    vector path (H*W a multiple of 4) and the scalar one."""
    rng = np.random.default_rng(255)
    ramp = torch.arange(256, dtype=torch.uint8).repeat(3).view(1, 16, 16, 3).to(dev)
    table = (torch.arange(256, dtype=torch.float32) / 255.0)
    assert torch.equal(_bits(P.preprocess_frames(ramp).cpu()), _bits(table.repeat(3).view(1, 16, 16, 3).permute(0, 3, 1, 2)))
    for n, H, W in ((3, 64, 64), (2, 37, 53), (1, 1, 1), (4, 1024, 1024)):
        x = torch.from_numpy(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)).to(dev)
        assert torch.equal(_bits(P.preprocess_frames(x)), _bits(pipeline.u8_to_input(x))), (n, H, W)


# ---- the background accumulator ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(24, 40), (5, 3), (1, 1)])
def test_frame_background(dev, tmp_path, H, W):
    """update() in chunks of 1, 3 and 8 over 12 frames equals the minimum over all 12 (guarded accumulator and frames); save then load
    round-trips the bytes."""
    rng = np.random.default_rng(12 + H)
    frames = rng.integers(3, 256, (12, H, W, 3), dtype=np.uint8)
    want = frames.min(0)
    assert np.array_equal(want, pr.background_min(frames)) and 3 <= int(want.min()) and int(want.max()) < 255
    acc = P.FrameBackground(H, W, dev)
    assert acc.count == 0 and bool((acc.image() == 255).all()) and acc.image().shape == (H, W, 3)
    acc.min = _guarded_u8((H, W, 3), dev, "big")
    acc.min.fill_(255)
    k = 0
    for m in (1, 3, 8):
        chunk = _guarded_u8((m, H, W, 3), dev)
        chunk.copy_(torch.from_numpy(frames[k:k + m]))
        acc.update(chunk)
        torch.cuda.synchronize()
        _check_u8(chunk, f"chunk of {m}")
        _check_u8(acc.min, f"accumulator after {m}")
        assert torch.equal(chunk.cpu(), torch.from_numpy(frames[k:k + m]))
        k += m
        assert np.array_equal(acc.image().cpu().numpy(), pr.background_min(frames[:k])), m
    assert acc.count == 12 and np.array_equal(acc.image().cpu().numpy(), want)
    acc.update(torch.from_numpy(frames[:0]).to(dev))
    assert acc.count == 12
    path = acc.save(str(tmp_path / "bg.png"))
    back = P.FrameBackground.load(path, dev)
    assert back.image().dtype == torch.uint8 and back.image().device == acc.image().device
    assert np.array_equal(back.image().cpu().numpy(), want) and (back.H, back.W, back.count) == (H, W, 0)
    with pytest.raises(ValueError):
        acc.update(torch.zeros(1, H + 1, W, 3, dtype=torch.uint8, device=dev))
    with pytest.raises(TypeError):
        acc.update(torch.zeros(1, H, W, 3, device=dev))
    with pytest.raises(NotImplementedError):
        acc.update(torch.zeros(1, H, W, 3, dtype=torch.uint8))


# ---- the paths that feed the network -------------------------------------------------------------------------------------------------
def test_run_py_background_and_minmax(tmp_path, dev):
    """run.py on a folder of 6 synthetic 256 x 256 RGB frames with a static background.  --background min --minmax 15: the .flo
    files are estimate() of the preprocessed frames, background.png is the restated minimum; --background <that png>: the same files,
    byte for byte; without the flags: other flows, and an args.txt that does not mention the flags."""
    import PIL.Image
    import run as runpy
    frames, _ = _particles_rgb(6, 256, 256, 300)
    seq = tmp_path / "seq"
    seq.mkdir()
    for k in range(6):
        PIL.Image.fromarray(frames[k]).save(str(seq / f"frame_{k:04d}.png"))
    names = [f"frame_{k:04d}" for k in range(5)]
    bg_want = pr.background_min(frames)
    net = pivlfn.Network(model="piv", params=synth.generate_weights("piv", 0)).to(dev).eval()
    t, bg = torch.from_numpy(frames).to(dev), torch.from_numpy(bg_want).to(dev)
    est = torch.cat([pivlfn.estimate(net, P.preprocess_frames(t[k:k + 2][:min(2, 5 - k)], bg, 15),
                                     P.preprocess_frames(t[k + 1:k + 3][:min(2, 5 - k)], bg, 15), tensor=True)
                     for k in (0, 2, 4)])                                              # the batches of --batch 2
    assert est.shape == (5, 2, 256, 256)

    def flo_dir(out):
        return out / "piv-synthetic" / "seq"

    base = ["--model", "piv", "-i", str(seq), "--batch", "2"]
    assert runpy.main(base + ["-o", str(tmp_path / "a"), "--background", "min", "--minmax", "15"]) == 5
    save = flo_dir(tmp_path / "a")
    for k in range(5):
        got = read_flow(str(save / "flow" / f"{names[k]}_out.flo"))
        assert pr.same_bits32(got, est[k].permute(1, 2, 0).cpu().numpy()), k
    assert np.array_equal(pipeline.read_image_u8(str(save / "background.png")), bg_want)
    lines = list(open(save / "args.txt"))
    assert "background: min\n" in lines and "minmax: 15\n" in lines and "minmax_floor: None\n" in lines

    assert runpy.main(base + ["-o", str(tmp_path / "b"), "--background", str(save / "background.png"), "--minmax", "15",
                              "--minmax-floor", "16"]) == 5
    for k in range(5):
        assert open(flo_dir(tmp_path / "b") / "flow" / f"{names[k]}_out.flo", "rb").read() == \
            open(save / "flow" / f"{names[k]}_out.flo", "rb").read(), k
    assert not (flo_dir(tmp_path / "b") / "background.png").exists()

    assert runpy.main(base + ["-o", str(tmp_path / "plain")]) == 5
    plain = flo_dir(tmp_path / "plain")
    raw = torch.cat([pivlfn.estimate(net, pipeline.u8_to_input(t[k:k + 2][:min(2, 5 - k)]),
                                     pipeline.u8_to_input(t[k + 1:k + 3][:min(2, 5 - k)]), tensor=True) for k in (0, 2, 4)])
    for k in range(5):
        got = read_flow(str(plain / "flow" / f"{names[k]}_out.flo"))
        assert pr.same_bits32(got, raw[k].permute(1, 2, 0).cpu().numpy()), k             # the default path is untouched
        assert not np.array_equal(got, read_flow(str(save / "flow" / f"{names[k]}_out.flo"))), k
    assert not [ln for ln in open(plain / "args.txt") if ln.split(":")[0] in ("background", "minmax", "minmax_floor")]
    assert not (plain / "background.png").exists()

    # an odd number of frames (-n 5): every frame is taken once
    from pivlfn.datasets import Run
    five = runpy.background_min(Run(root=str(seq), is_pair=False, n_images=5, start_at=0), dev, 2)
    assert five.count == 5 and np.array_equal(five.image().cpu().numpy(), pr.background_min(frames[:5]))
    assert not np.array_equal(bg_want, pr.background_min(frames[:5]))

    # a background of another size, and a folder of two sizes: refused with both sizes named
    PIL.Image.fromarray(bg_want[:128, :200]).save(str(tmp_path / "small.png"))
    with pytest.raises(SystemExit, match="128 x 200.*256 x 256"):
        runpy.main(base + ["-o", str(tmp_path / "c"), "--background", str(tmp_path / "small.png")])
    PIL.Image.fromarray(frames[0, :128, :200]).save(str(seq / "frame_0006.png"))
    PIL.Image.fromarray(frames[1, :128, :200]).save(str(seq / "frame_0007.png"))
    with pytest.raises(SystemExit, match="one size.*128 x 200.*256 x 256"):
        runpy.main(base + ["-o", str(tmp_path / "d"), "--background", "min"])


def test_run_sequence_with_prep(dev):
    """run_sequence(prep=...) over grey ParticleSequence frames: the flows of estimate() on the preprocessed frames, chunk by chunk;
    without prep the flows differ."""
    from pivlfn.sequence import frames_to_input, run_sequence
    H = W = 128
    seq = synth.ParticleSequence(H, W, seed=77, device=dev)
    net = pivlfn.Network(model="piv", params=synth.generate_weights("piv", 0)).to(dev).eval()
    fr = seq.frames(0, 5)
    acc = P.FrameBackground(H, W, dev)
    rgb = fr[..., None].expand(-1, -1, -1, 3).contiguous()
    acc.update(rgb)
    prep = P.Preprocessor(acc.image(), 15, 8)
    assert torch.equal(_bits(frames_to_input(fr, prep)), _bits(P.preprocess_frames(rgb, acc.image(), 15, 8)))
    assert torch.equal(_bits(frames_to_input(fr)), _bits(pipeline.u8_to_input(rgb)))
    want = []
    for f0, f1 in ((0, 3), (2, 5)):                            # chunk = 2: frames 0..2, then the halo frame 2 with 3, 4
        x = prep(rgb[f0:f1])
        want.append(pivlfn.estimate(net, x[:-1], x[1:], tensor=True))
    want = torch.cat(want).permute(0, 2, 3, 1).cpu().numpy()
    got, plain = {}, {}
    stats = run_sequence(net, seq.frames, 5, chunk=2, device=dev, sink=lambda i, flow: got.__setitem__(i, flow.copy()), prep=prep)
    assert stats["flows_emitted"] == 4 and sorted(got) == [0, 1, 2, 3]
    run_sequence(net, seq.frames, 5, chunk=2, device=dev, sink=lambda i, flow: plain.__setitem__(i, flow.copy()))
    for i in range(4):
        assert pr.same_bits32(got[i], want[i]), i
        assert not np.array_equal(got[i], plain[i]), i
