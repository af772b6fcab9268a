"""GPU: pivlfn_particles_displace and pivlfn_particles_render (csrc/particles.hip) against the NumPy restatement of their contract
(tests/particles_restatement.py), the Python layer on top (pivlfn.particles) and generate.py.

The displacer is a chain of correctly rounded fp64 operations in a fixed order: positions and flags are compared bit for bit, NaN and
inf included, no particle left out.  The renderer is held to the header's bound, per pixel
    |intensity - V| <= 2^-21 A + n 2^-24 V
(V, A, n: the float64 value, the sum of amp and the number of the covering particles; derivation in include/pivlfn.h), the image to
trunc(min(V, 255)) except where an integer lies within that bound of V, and to its own bits: twice, alone and in a batch, whatever
the workspace held.  Every case prints the largest |err| / tol it met (DESIGN records it).  Shapes are the smallest that reach every
path: one pixel, one tile, ragged tiles, lists longer than a staging chunk (0.5 ppp) and longer than the LDS (3000 particles on one
pixel).  Everything here runs on the default stream; the stream and capture contract is in tests/particles_stream_cases.py, which the
last test runs in a process of its own."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import particles_restatement as prs
from guarded import check_guards, guarded
from particles_restatement import BAD, LOST
from particles_stream_cases import field, points, seeding
from test_gpu_op_streams import _p, _scribble

pytestmark = pytest.mark.gpu


def _t(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


# ---- the displacer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["bilinear", "cubic"])
@pytest.mark.parametrize("H,W,holes", [(2, 2, False), (2, 2, True), (2, 9, False), (2, 9, True), (37, 53, False), (37, 53, True)])
def test_displacer_bits_of_the_restatement(H, W, holes, method, dev):
    """600 particles (three blocks, the last ragged): nodes, the clamped last row and column, a hair inside and outside every side, NaN,
    +-inf, -0.0 and random points up to 20 px outside.  With holes: a NaN, a -inf, a 1e10 vector and two mask bytes, so LOST occurs."""
    from pivlfn import displace_particles
    flow, mask = field(H, W, 7 * H + W, holes)
    pos = points(600, H, W, H)
    want, wflag = prs.displace(pos, flow, mask, None, 0 if method == "bilinear" else 1)
    got, flag = displace_particles(_t(pos, dev), _t(flow, dev), _t(mask, dev), method)
    assert got.shape == (2, 600) and got.dtype == torch.float64 and flag.dtype == torch.uint8
    assert np.array_equal(flag.cpu().numpy(), wflag), f"{np.count_nonzero(flag.cpu().numpy() != wflag)} flags differ"
    same = got.cpu().numpy().view(np.int64) == want.view(np.int64)
    assert same.all(), f"{np.count_nonzero(~same)} coordinates differ, first {tuple(np.argwhere(~same)[0])}"
    assert (wflag == BAD).sum() == 2 and ((wflag == LOST).any() if holes else set(np.unique(wflag)) == {0, BAD})
    if not holes:                                        # nodes, edges, margin and +-inf particles are all sampled
        assert not wflag[:11].any() and not wflag[13:20].any() and (want[:, :11] != pos[:, :11]).any(0).all()
    # flagged on entry: copied through, the others as before
    flag0 = np.zeros(600, np.uint8)
    flag0[::7] = 1 + (np.arange(0, 600, 7) % 255)
    want2, wflag2 = prs.displace(pos, flow, mask, flag0, 0 if method == "bilinear" else 1)
    got2, flag2 = displace_particles(_t(pos, dev), _t(flow, dev), _t(mask, dev), method, flag=_t(flag0, dev))
    assert np.array_equal(flag2.cpu().numpy(), wflag2) and prs.same_bits(got2.cpu().numpy(), want2)
    assert prs.same_bits(want2[:, ::7], pos[:, ::7]) and np.array_equal(wflag2[::7], flag0[::7])


def test_displacer_guarded_buffers(dev):
    """Inputs, flags and output between guards, the output first holding the sentinel, then 0xFF: the same bits, every guard intact, no
    input written.  N and H*W multiples of 4 (whole 32-bit words)."""
    from pivlfn import _lib
    lib = _lib.load()
    H, W, N = 38, 46, 600
    flow, mask = field(H, W, 3, True)
    pos = points(N, H, W, 9)
    src = [_t(pos, dev), _t(flow, dev), _t(mask, dev)]
    ins = [guarded(t.shape, t.dtype, dev, "nan") for t in src]
    for t, x in zip(ins, src):
        t.copy_(x)
    flag, out = guarded((N,), torch.uint8, dev, "sentinel"), guarded((2, N), torch.float64, dev, "sentinel")
    st = torch.cuda.current_stream(dev).cuda_stream
    for method in (0, 1):
        want, wflag = prs.displace(pos, flow, mask, None, method)
        for scribble in (False, True):
            if scribble:
                _scribble(out)
            flag.zero_()
            _lib.check(lib.pivlfn_particles_displace(_p(ins[0]), _p(ins[1]), _p(ins[2]), H, W, N, method, _p(flag), _p(out), st), "displace")
            torch.cuda.synchronize()
            assert prs.same_bits(out.cpu().numpy(), want) and np.array_equal(flag.cpu().numpy(), wflag)
            for t in ins + [flag, out]:
                check_guards(t, f"particles_displace method={method}")
    for t, x in zip(ins, src):
        assert torch.equal(t.view(torch.uint8), x.view(torch.uint8)), "an input was written"


# ---- the renderer ----------------------------------------------------------------------------------------------------------------------
def _render(dev, pos, diam, amp, H, W, R=4, flag=None, ws=None, ws_fill="sentinel"):
    """pivlfn_particles_render (B > 0) with guarded outputs and a guarded workspace; returns (intensity, image, workspace).  The image
    need not be whole 32-bit words: it lies at the END of a guarded run of whole words, and the bytes in front of it must stay too."""
    from pivlfn import _lib
    lib = _lib.load()
    B, _, N = pos.shape
    need = lib.pivlfn_particles_render_workspace_bytes(B, N, H, W, R)
    assert need > 0 and need % 8 == 0
    ins = [_t(pos, dev), _t(diam, dev), _t(amp, dev), _t(flag, dev)]
    intensity = guarded((B, H, W), torch.float32, dev, "sentinel")
    whole = guarded((-(-B * H * W // 4) * 4,), torch.uint8, dev, "sentinel")
    lead = whole.numel() - B * H * W
    image, before = whole[lead:], whole[:lead].clone()
    if ws is None:
        ws = guarded((need,), torch.uint8, dev, "nan" if ws_fill == "ff" else ws_fill)
        if ws_fill == "ff":
            _scribble(ws)
    assert ws.numel() == need and ws.data_ptr() % 8 == 0
    _lib.check(lib.pivlfn_particles_render(_p(ins[0]), _p(ins[1]), _p(ins[2]), _p(ins[3]), B, N, H, W, R, _p(intensity), _p(image), _p(ws),
                                           need, torch.cuda.current_stream(dev).cuda_stream), "particles_render")
    torch.cuda.synchronize()
    for t in (intensity, whole, ws):
        check_guards(t, "particles_render")
    assert torch.equal(whole[:lead], before), "a byte in front of the image changed"
    for t, x in zip(ins, (pos, diam, amp, flag)):
        assert x is None or np.array_equal(t.cpu().numpy().view(np.uint8), np.ascontiguousarray(x).view(np.uint8)), "an input was written"
    return intensity.cpu().numpy(), image.cpu().numpy().reshape(B, H, W), ws


def _against_the_restatement(dev, pos, diam, amp, H, W, R=4, flag=None, what=""):
    intensity, image, _ = _render(dev, pos, diam, amp, H, W, R, flag)
    worst, cover = 0.0, 0
    for b in range(pos.shape[0]):
        V, A, n = prs.render(pos[b], diam[b], amp[b], H, W, R, None if flag is None else flag[b])
        worst = max(worst, prs.check_render(intensity[b], image[b], V, A, n, f"{what} image {b}"))
        cover = max(cover, int(n.max()))
    print(f"particles_render {what}: max |err|/tol = {worst:.4f}, up to {cover} particles on a pixel")
    assert worst < 1.0
    return intensity, image


def test_one_pixel(dev):
    pos, diam, amp = np.array([[[0.3], [-0.2]]]), np.array([[2.0]], np.float32), np.array([[200.0]], np.float32)
    intensity, image = _against_the_restatement(dev, pos, diam, amp, 1, 1, what="1 x 1")
    assert 150 < intensity[0, 0, 0] < 200 and image[0, 0, 0] == int(intensity[0, 0, 0])


@pytest.mark.parametrize("R", [1, 4, 8])
def test_one_particle_in_and_round_one_tile(R, dev):
    """16 x 16, one particle an image, a batch of positions: integer, half-integer, negative, exactly on every edge, and up to R+2
    outside every side and corner -- the footprint partly, then wholly outside the image (those images are zero)."""
    xs = [5.0, 5.5, -1.5, 0.0, 15.0, 15.999, -0.001] + [-float(k) for k in range(1, R + 3)] + [15.0 + k for k in range(1, R + 3)]
    spots = [(x, 7.25) for x in xs] + [(7.25, y) for y in xs] + [(x, x) for x in xs] + [(x, 15.0 - x) for x in xs]
    pos = np.array(spots, np.float64).reshape(-1, 2, 1)
    B = len(spots)
    diam, amp = np.full((B, 1), 2.5, np.float32), np.full((B, 1), 240.0, np.float32)
    intensity, _ = _against_the_restatement(dev, pos, diam, amp, 16, 16, R, what=f"16 x 16 R={R}")
    lit = intensity.reshape(B, -1).max(1) > 0
    gone = np.array([np.floor(x) + R + 1 < 0 or np.floor(x) - R > 15 or np.floor(y) + R + 1 < 0 or np.floor(y) - R > 15 for x, y in spots])
    assert not lit[gone].any() and gone.sum() >= 8 and lit.sum() > 20


@pytest.mark.parametrize("H,W,ppp,R", [(17, 33, 0.3, 4), (37, 53, 0.05, 4), (37, 53, 0.5, 4), (37, 53, 0.2, 1), (37, 53, 0.2, 8)])
def test_seedings_against_the_restatement(H, W, ppp, R, dev):
    """Ragged tiles (17 x 33: the second tile row has one pixel row) and 37 x 53 with a 16 px margin at 0.05 and 0.5 ppp -- at 0.5 a
    tile's list has some 340 particles, more than one staging chunk -- and the smallest and the largest radius.  Two images a call."""
    N = int(ppp * (H + 32) * (W + 32))
    pos, diam, amp = seeding(2, N, H, W, 17 * H + R)
    _against_the_restatement(dev, pos, diam, amp, H, W, R, what=f"{H} x {W} {ppp} ppp R={R}")


def _tile_shapes():
    import analysis_plans as ap
    return ap.shapes(ap.PARTICLES_CASES)


@pytest.mark.parametrize("B,H,W", _tile_shapes())
def test_seedings_of_many_tiles(B, H, W, dev):
    """More tiles than one wave (65), than one workgroup (257) and than two (544 over two images) of particles_offsets_kernel, whose
    wave prefixes and atomic cursor decide where a tile's list lies; 0.05 ppp, and 2100 particles more, interleaved with the others,
    inside the middle of the LAST tile of the last image: a list longer than REN_CAP in the last workgroup's tiles.  The image does not
    depend on where a list lands (the ascending-index rule): the header's bound against the restatement, and equal bits twice."""
    import analysis_plans as ap
    plan = ap.particles_tiles(B, H, W)
    assert plan["waves"] >= 2
    extra = ap.REN_CAP + 52
    N = int(0.05 * (H + 32) * (W + 32)) + extra
    pos, diam, amp = seeding(B, N, H, W, 3 * H + W)
    rng = np.random.default_rng(W)
    here = rng.permutation(N)[:extra]
    x0, y0 = (W - 1) // 16 * 16 + 8, (H - 1) // 16 * 16 + 8                         # the footprint (R = 4) stays inside that tile
    assert x0 + 6 <= W and y0 + 6 <= H
    pos[-1, 0, here], pos[-1, 1, here] = x0 + rng.random(extra), y0 + rng.random(extra)
    intensity, image = _against_the_restatement(dev, pos, diam, amp, H, W, what=f"{B} x {H} x {W}, {plan['tiles']} tiles")
    assert image[-1, y0, x0] == 255 and intensity[-1, y0, x0] > 1e5 and (image[0] < 255).any() and (image[0, :, :16] > 0).any()
    again = _render(dev, pos, diam, amp, H, W, ws_fill="ff")
    assert np.array_equal(again[0].view(np.int32), intensity.view(np.int32)) and np.array_equal(again[1], image)


def test_thousands_of_particles_on_one_pixel(dev):
    """3000 particles inside pixel (30, 20) of 37 x 53 and 2000 spread over the image, interleaved: the lists of two tiles are longer
    than the LDS holds and are ordered window by window; the pixel saturates at 255."""
    H, W = 37, 53
    rng = np.random.default_rng(8)
    N = 5000
    pos, diam, amp = seeding(1, N, H, W, 81)
    here = rng.permutation(N)[:3000]
    pos[0, 0, here], pos[0, 1, here] = 20.0 + rng.random(3000), 30.0 + rng.random(3000)
    intensity, image = _against_the_restatement(dev, pos, diam, amp, H, W, what="3000 on one pixel")
    assert image[0, 30, 20] == 255 and intensity[0, 30, 20] > 1e5 and (image[0] < 255).any()


def test_no_particles_and_no_images(dev):
    H, W = 37, 53
    intensity, image, _ = _render(dev, np.zeros((2, 2, 0)), np.zeros((2, 0), np.float32), np.zeros((2, 0), np.float32), H, W)
    assert intensity.shape == (2, H, W) and not intensity.view(np.int32).any() and not image.any()        # +0.0f, not the sentinel
    from pivlfn import _lib
    keep = _scribble(torch.empty(4096, dtype=torch.uint8, device=dev))            # B == 0 succeeds, launches nothing, writes nothing
    assert _lib.load().pivlfn_particles_render(_p(keep), _p(keep), _p(keep), None, 0, 5, H, W, 4, _p(keep), _p(keep), _p(keep), 0,
                                               torch.cuda.current_stream(dev).cuda_stream) == 0
    torch.cuda.synchronize()
    assert bool((keep == 0xFF).all())


def test_skipped_particles(dev):
    """A flag, a NaN x, an inf diameter, a diameter of 0, a negative amp and |x| = 2^30, each in the middle of the list: the image has
    the bits of the render without them."""
    H, W, N = 37, 53, 400
    pos, diam, amp = seeding(1, N, H, W, 21)
    keep = np.ones(N, bool)
    flag = np.zeros((1, N), np.uint8)
    bad = [40, 90, 140, 190, 240, 290, 340]
    flag[0, bad[0]] = 1
    pos[0, 0, bad[1]] = np.nan
    diam[0, bad[2]] = np.inf
    diam[0, bad[3]] = 0.0
    amp[0, bad[4]] = -1.0
    pos[0, 0, bad[5]] = 2.0 ** 30
    pos[0, 1, bad[6]] = -2.0 ** 30
    keep[bad] = False
    assert not prs.drawn(pos[0], diam[0], amp[0], flag[0])[bad].any() and prs.drawn(pos[0], diam[0], amp[0], flag[0])[keep].all()
    got = _render(dev, pos, diam, amp, H, W, 4, flag)
    want = _render(dev, pos[:, :, keep], diam[:, keep], amp[:, keep], H, W)
    assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)) and np.array_equal(got[1], want[1]) and want[1].max() > 100


def test_bits_do_not_depend_on_the_call(dev):
    """The same call twice; a pair alone and inside a batch of three; a workspace of 0xFF, of zeros and with the previous call's
    contents (of another seeding): equal bits every time."""
    H, W, N = 37, 53, 2000                               # 0.4 ppp: lists of several chunks
    pos, diam, amp = seeding(3, N, H, W, 33)
    i3, m3, ws = _render(dev, pos, diam, amp, H, W)
    again = _render(dev, pos, diam, amp, H, W)
    assert np.array_equal(again[0].view(np.int32), i3.view(np.int32)) and np.array_equal(again[1], m3)
    for b in range(3):
        alone = _render(dev, pos[b:b + 1], diam[b:b + 1], amp[b:b + 1], H, W, ws_fill="ff" if b else "nan")
        assert np.array_equal(alone[0].view(np.int32), i3[b:b + 1].view(np.int32)) and np.array_equal(alone[1], m3[b:b + 1]), b
    other = seeding(3, N, H, W, 34)
    _render(dev, *other, H, W, ws=ws)                    # leaves its lists and counters behind
    reused = _render(dev, pos, diam, amp, H, W, ws=ws)
    assert np.array_equal(reused[0].view(np.int32), i3.view(np.int32)) and np.array_equal(reused[1], m3)
    ws.zero_()
    zeroed = _render(dev, pos, diam, amp, H, W, ws=ws)
    assert np.array_equal(zeroed[0].view(np.int32), i3.view(np.int32)) and np.array_equal(zeroed[1], m3)


def test_every_error_is_refused_before_any_launch(dev):
    """The refusals of tests/test_particles.py with real device buffers: every byte of them stays as it was."""
    from pivlfn import _lib
    from test_particles import refusals
    arena = _scribble(torch.empty(12 << 16, dtype=torch.uint8, device=dev))
    base = arena.data_ptr() + (1 << 16)
    assert base % 8 == 0
    refusals(_lib.load(), *(base + (i << 16) for i in range(10)))
    torch.cuda.synchronize()
    assert bool((arena == 0xFF).all())


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------
def _lamb_oseen(H, W):
    from pivlfn import synth
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack(synth.displacement_field(xx, yy, H, W)).astype(np.float32)


def test_create_pair_from_flow(dev):
    """A 64 x 64 Lamb-Oseen field, B = 2: both frames of both pairs equal the restatement fed the same particles (displaced by the
    restatement of the displacer, bit for bit), and img1 of pair 0 does not depend on the batch.  With a masked patch, LOST particles
    are in frame 1 and not in frame 2; with out_of_plane the second frame's amplitudes differ."""
    from pivlfn import ParticleImageGen
    H = W = 64
    flow = _lamb_oseen(H, W)
    flows = _t(np.stack([flow, -flow]), dev)
    gen = ParticleImageGen(density=0.05, seed=11, device=dev)
    img1, img2, truth = gen.create_pair_from_flow(flows)
    assert truth is flows and img1.shape == img2.shape == (2, H, W) and img1.dtype == img2.dtype == torch.uint8
    p = gen.pair_particles(flows)
    N = gen.count(H, W, 16)
    pos, diam, amp, flag = (t.cpu().numpy() for t in p)
    assert pos.shape == (4, 2, N) and not flag.any() and np.array_equal(amp[:2], amp[2:]) and np.array_equal(diam[:2], diam[2:])
    for b, f in enumerate((flow, -flow)):
        x, y, z, d, _ = gen._seeding(H, W, 16, 11 + b)
        assert prs.same_bits(pos[b], np.stack([x, y])) and np.array_equal(diam[b], d.astype(np.float32))
        assert np.abs(amp[b] - 240.0 * np.exp(-z * z)).max() < 1e-4
        moved, _ = prs.displace(pos[b], f, None, None, 1)
        assert prs.same_bits(pos[2 + b], moved)
        for k, img in ((b, img1[b]), (2 + b, img2[b])):
            prs.check_image(img.cpu().numpy(), *prs.render(pos[k], diam[k], amp[k], H, W), f"pair {b} frame {k // 2 + 1}")
    assert img1.max() > 150 and not torch.equal(img1[0], img2[0]) and not torch.equal(img1[0], img1[1])
    a1, a2, t1 = gen.create_pair_from_flow(flows[0])
    assert t1.shape == (2, H, W) and torch.equal(a1, img1[0]) and torch.equal(a2, img2[0])
    x, y, z, d = gen.random_particle(H, W, 16)
    assert torch.equal(gen.generate_image(x, y, z, d, H, W), img1[0])
    # a masked patch: the particles that meet it are LOST, drawn in frame 1 and left out of frame 2
    mask = torch.zeros(H, W, dtype=torch.uint8, device=dev)
    mask[20:30, 20:30] = 1
    m1, m2, _ = gen.create_pair_from_flow(flows[0], mask=mask)
    pm = gen.pair_particles(flows[:1], mask=mask[None])
    lost = pm.flag[1].cpu().numpy() == LOST
    assert torch.equal(m1, img1[0]) and lost.sum() > 3 and not pm.flag[0].any()
    prs.check_image(m2.cpu().numpy(), *prs.render(pm.pos[1].cpu().numpy(), diam[0], amp[0], H, W, 4, lost), "frame 2 with a mask")
    assert not torch.equal(m2, img2[0])
    # out of plane
    po = gen.pair_particles(flows[:1], out_of_plane=0.3)
    assert torch.equal(po.amp[0], p.amp[0]) and not torch.equal(po.amp[1], p.amp[0]) and torch.equal(po.pos, p.pos[[0, 2]])


def test_generate_py(tmp_path, dev):
    """generate.py --field lamb_oseen --size 64 64 -n 2 in a process of its own: two pairs in the layout run.py -p --truth reads, the
    truth files hold synth.displacement_field as float32 bit for bit, the PNGs what create_pair_from_flow returns for those seeds."""
    import PIL.Image
    from pivlfn import ParticleImageGen
    from pivlfn.datasets import image_files_from_folder, pair_files
    from pivlfn.flo import read_flow
    here = os.path.dirname(os.path.abspath(__file__))
    script = os.path.join(os.path.dirname(here), "piv_liteflownet-pytorch_amd", "generate.py")
    out = tmp_path / "pairs"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [script, "-o", str(out), "--field", "lamb_oseen", "--size", "64", "64",
                                                                          "-n", "2", "--seed", "5"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "2 pairs" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    pairs = pair_files(image_files_from_folder(str(out), pair=True), True)
    assert [p[2] for p in pairs] == ["lamb_oseen_0000", "lamb_oseen_0001"]
    flow = _lamb_oseen(64, 64)
    img1, img2, _ = ParticleImageGen(seed=5, device=dev).create_pair_from_flow(_t(np.stack([flow, flow]), dev))
    for k, (first, second, name) in enumerate(pairs):
        got = read_flow(str(out / f"{name}_flow.flo"))
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), np.ascontiguousarray(flow.transpose(1, 2, 0)).view(np.int32))
        for path, want in ((first, img1[k]), (second, img2[k])):
            im = PIL.Image.open(path)
            assert im.mode == "L" and np.array_equal(np.asarray(im), want.cpu().numpy()), path


# ---- side streams and graph capture: in a process of their own ---------------------------------------------------------------------------
def test_stream_contract_in_a_process_of_its_own(dev):
    """tests/particles_stream_cases.py in a fresh pytest process: 16 tests, all passing.  Why not in this process:
    tests/test_gpu_flowmap.py::test_stream_contract_and_run_py_in_a_process_of_their_own says it -- the side streams of the delay and
    of graph capture would change which queue a later module's side stream shares with the default stream."""
    here = os.path.dirname(os.path.abspath(__file__))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                                                                          os.path.join(here, "particles_stream_cases.py")]
    r = subprocess.run(cmd, cwd=here, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and re.search(r"\b16 passed", r.stdout), r.stdout[-6000:] + r.stderr[-2000:]
