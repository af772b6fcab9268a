"""CPU: the restatement of the synthetic-pair contracts (tests/particles_restatement.py) against what it restates -- synth._render,
the reference's untruncated image model, closed forms of the two interpolations -- and every parameter check of pivlfn.particles
that needs no GPU.  The kernels themselves are held to the restatement in tests/test_gpu_particles.py."""
import numpy as np
import pytest
import torch

import particles_restatement as prs
from particles_restatement import BAD, LOST


def test_renderer_restates_synth_render():
    """particle_pair's particles at 48 x 40: the same footprint and the same float64 terms as synth._render, so the uint8 image is
    identical; and the float64 image agrees to 1e-9 with synth._render's sum written out here (it returns only the clipped image)."""
    from pivlfn import synth
    H, W, m = 48, 40, 16
    g = np.random.Generator(np.random.Philox(key=[1234, 0x9E3779B9]))
    n = int(np.floor(0.05 * (H + 2 * m) * (W + 2 * m)))
    xp, yp = g.random(n) * (W + 2 * m) - m, g.random(n) * (H + 2 * m) - m
    zp, dp = g.random(n) - 0.5, 1.5 + g.random(n)
    img = synth._render(xp, yp, zp, dp, H, W)
    assert np.array_equal(img, synth.particle_pair(H, W)[0]), "these are not particle_pair's particles"
    amp = 240.0 * np.exp(-(zp ** 2))
    V, A, cnt = prs.render(np.stack([xp, yp]), dp, amp, H, W)
    assert np.array_equal(np.floor(np.minimum(V, 255.0)).astype(np.uint8), img)
    want = np.zeros((H, W))                                          # synth._render's loop: pixels ix-4 .. ix+5, the division as it writes it
    for x0, y0, a, d in zip(xp, yp, amp, dp):
        ix, iy = int(np.floor(x0)), int(np.floor(y0))
        for i in range(max(iy - 4, 0), min(iy + 6, H)):
            for j in range(max(ix - 4, 0), min(ix + 6, W)):
                want[i, j] += a * np.exp(-((j - x0) ** 2 + (i - y0) ** 2) / ((0.5 * d) ** 2))
    assert np.abs(V - want).max() <= 1e-9 and np.array_equal(np.clip(want, 0, 255).astype(np.uint8), img)
    assert cnt.max() >= 3 and (cnt == 0).any() and np.all(A >= V)


def test_footprint_loses_less_than_a_grey_level():
    """The reference's image model sums every particle over every pixel (src/particle_image_generator.py:54-56); the footprint of
    radius 4 cuts a blob off five pixels from its centre at the nearest.  32 x 32 at 0.05 ppp with the reference's diameters."""
    H = W = 32
    m = 16
    rng = np.random.default_rng(5)
    n = int(0.05 * (H + 2 * m) * (W + 2 * m))
    x, y = rng.random(n) * (W + 2 * m) - m, rng.random(n) * (H + 2 * m) - m
    d, a = 1.5 + rng.random(n), 240.0 * np.exp(-((rng.random(n) - 0.5) ** 2))
    V, _, _ = prs.render(np.stack([x, y]), d, a, H, W)
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    full = np.zeros((H, W))
    for p in range(n):
        full += a[p] * np.exp(-((jj - x[p]) ** 2 + (ii - y[p]) ** 2) / ((d[p] / 2) ** 2))
    assert V.max() > 100 and np.all(V <= full + 1e-9) and np.abs(full - V).max() < 1.0


@pytest.mark.parametrize("method", [0, 1])
def test_a_particle_moves_by_the_flow(method):
    """One particle through a uniform flow: the centroid of its image moves by that flow to < 0.01 px."""
    H = W = 32
    flow = np.empty((2, H, W), np.float32)
    flow[0], flow[1] = 2.3, -1.6
    pos = np.array([[14.3], [17.8]])
    pos2, flag = prs.displace(pos, flow, method=method)
    assert not flag.any()
    d, a = np.array([2.5]), np.array([200.0])
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    cents = []
    for p in (pos, pos2):
        V, _, _ = prs.render(p, d, a, H, W)
        cents.append((float((V * jj).sum() / V.sum()), float((V * ii).sum() / V.sum())))
    assert abs(cents[1][0] - cents[0][0] - 2.3) < 0.01 and abs(cents[1][1] - cents[0][1] + 1.6) < 0.01


def _grid(H, W):
    return np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))


def test_bilinear_reproduces_affine_fields_exactly():
    """u = 0.5 x - 0.25 y + 3, v = 0.125 x + 2 y - 1 with dyadic positions: every product and sum is exact, so is the result."""
    H, W = 9, 12
    jj, ii = _grid(H, W)
    flow = np.stack([0.5 * jj - 0.25 * ii + 3.0, 0.125 * jj + 2.0 * ii - 1.0]).astype(np.float32)
    rng = np.random.default_rng(0)
    pos = np.stack([rng.integers(0, (W - 1) * 64, 200) / 64.0, rng.integers(0, (H - 1) * 64, 200) / 64.0])
    out, flag = prs.displace(pos, flow, method=0)
    assert not flag.any()
    assert np.array_equal(out[0], pos[0] + (0.5 * pos[0] - 0.25 * pos[1] + 3.0))
    assert np.array_equal(out[1], pos[1] + (0.125 * pos[0] + 2.0 * pos[1] - 1.0))


def test_bicubic_reproduces_a_quadratic_field():
    """Catmull-Rom interpolation is exact for quadratics where no tap is clamped: cells 1 .. W-3."""
    H, W = 12, 14
    jj, ii = _grid(H, W)
    u = 0.25 * jj * jj - 0.5 * jj * ii + 0.125 * ii * ii + jj - 2.0
    v = -0.125 * jj * jj + 0.25 * ii * ii + 0.5 * ii + 1.0
    flow = np.stack([u, v]).astype(np.float32)
    assert np.array_equal(flow.astype(np.float64), np.stack([u, v]))
    rng = np.random.default_rng(1)
    x, y = rng.uniform(1.0, W - 2.0, 300), rng.uniform(1.0, H - 2.0, 300)
    out, flag = prs.displace(np.stack([x, y]), flow, method=1)
    assert not flag.any()
    assert np.abs(out[0] - (x + 0.25 * x * x - 0.5 * x * y + 0.125 * y * y + x - 2.0)).max() <= 1e-12
    assert np.abs(out[1] - (y - 0.125 * x * x + 0.25 * y * y + 0.5 * y + 1.0)).max() <= 1e-12
    lin, _ = prs.displace(np.stack([x, y]), flow, method=0)          # and the bilinear sample of the same field is not
    assert np.abs(lin[0] - out[0]).max() > 1e-3


@pytest.mark.parametrize("method", [0, 1])
def test_margin_particles_take_the_edge_value(method):
    H, W = 6, 7
    rng = np.random.default_rng(2)
    flow = rng.standard_normal((2, H, W)).astype(np.float32)
    pos = np.array([[-5.0, W + 3.0, 2.0, 3.0, -9.0, W - 1.0 + 4.0, -np.inf, 3.0],
                    [2.0, 3.0, -7.5, H + 2.0, -9.0, H - 1.0 + 0.25, 1.0, np.inf]])
    node = [(2, 0), (3, W - 1), (0, 2), (H - 1, 3), (0, 0), (H - 1, W - 1), (1, 0), (H - 1, 3)]
    out, flag = prs.displace(pos, flow, method=method)
    assert not flag.any()
    for p, (i, j) in enumerate(node):
        assert out[0, p] == pos[0, p] + float(flow[0, i, j]) and out[1, p] == pos[1, p] + float(flow[1, i, j]), p


@pytest.mark.parametrize("method", [0, 1])
def test_flags_of_the_displacer(method):
    H, W = 8, 8
    flow = np.ones((2, H, W), np.float32)
    flow[0, 2, 2], flow[1, 5, 5], flow[0, 6, 1] = np.nan, 1e10, -np.inf
    mask = np.zeros((H, W), np.uint8)
    mask[0, 6] = 1
    pos = np.array([[2.5, 5.5, 1.5, 6.5, 6.0, np.nan, 4.5, 4.5], [2.5, 5.5, 6.5, 0.5, 2.0, 1.0, np.nan, 1.5]])
    flag0 = np.zeros(8, np.uint8)
    flag0[7] = 1
    out, flag = prs.displace(pos, flow, mask, flag0, method)
    assert flag.tolist() == [LOST, LOST, LOST, LOST, 0, BAD, BAD, 1]
    assert prs.same_bits(out[:, [0, 1, 2, 3, 5, 6, 7]], pos[:, [0, 1, 2, 3, 5, 6, 7]])
    assert out[0, 4] == 7.0 and out[1, 4] == 3.0


def test_drawn_particles():
    pos = np.array([[1.0, np.nan, 1.0, 1.0, 1.0, 2.0 ** 30, 1.0, 1.0], [1.0] * 8])
    diam = np.array([2, 2, np.inf, 0, 2, 2, 2, 1e-20], np.float32)
    amp = np.array([9, 9, 9, 9, -1, 9, 9, 9], np.float32)
    flag = np.array([0, 0, 0, 0, 0, 0, 3, 0], np.uint8)
    assert prs.drawn(pos, diam, amp, flag).tolist() == [True] + [False] * 7


def test_grey_level_criterion():
    V, A, n = np.array([[3.9999999, 4.5, 300.0, 0.0]]), np.array([[200.0, 200.0, 900.0, 0.0]]), np.array([[2.0, 2.0, 4.0, 0.0]])
    prs.check_image(np.array([[3, 4, 255, 0]], np.uint8), V, A, n)
    prs.check_image(np.array([[4, 4, 255, 0]], np.uint8), V, A, n)          # 4 lies within the tolerance of V: 3 and 4 both pass
    for bad in ([[5, 4, 255, 0]], [[3, 5, 255, 0]], [[3, 4, 254, 0]], [[3, 4, 255, 1]]):
        with pytest.raises(AssertionError):
            prs.check_image(np.array(bad, np.uint8), V, A, n)
    r = prs.check_render(np.array([[4.0, 4.5, 300.0, 0.0]], np.float32), np.array([[4, 4, 255, 0]], np.uint8), V, A, n)
    assert 0.0 < r < 1.0
    with pytest.raises(AssertionError):
        prs.check_render(np.array([[4.001, 4.5, 300.0, 0.0]], np.float32), np.array([[4, 4, 255, 0]], np.uint8), V, A, n)


def refusals(lib, pos, flow, mask, flag, out, diam, amp, intensity, image, ws):
    """Every PIVLFN_ERR_ARG case of the two entry points, with ten regions at least 64 KiB apart: nothing may be launched or written
    (tests/test_gpu_particles.py runs this with real device buffers and looks at them afterwards)."""
    def refused(rc, *words):
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    H, W, N, B, R = 8, 9, 50, 2, 4
    d = lib.pivlfn_particles_displace
    refused(d(pos, flow, mask, 1, W, N, 0, flag, out, None), "particles_displace", "bad shape")
    refused(d(pos, flow, mask, H, 1, N, 0, flag, out, None), "bad shape")
    refused(d(pos, flow, mask, 1 << 16, 1 << 15, N, 0, flag, out, None), "2^31")
    refused(d(pos, flow, mask, H, W, -1, 0, flag, out, None), "N=-1")
    refused(d(pos, flow, mask, H, W, N, 2, flag, out, None), "method=2")
    refused(d(pos, flow, mask, H, W, N, -1, flag, out, None), "method=-1")
    for args in ((None, flow, mask, H, W, N, 0, flag, out), (pos, None, mask, H, W, N, 0, flag, out), (pos, flow, mask, H, W, N, 0, None, out),
                 (pos, flow, None, H, W, N, 1, flag, None)):
        refused(d(*args, None), "null")
    for args, a, b in (((pos, flow, mask, H, W, N, 0, flag, pos), "out", "pos"), ((pos, flow, mask, H, W, N, 0, flag, flow + 8), "out", "flow"),
                       ((pos, flow, mask, H, W, N, 0, flag, mask - 16 * N + 8), "out", "mask"), ((pos, flow, mask, H, W, N, 1, pos + 16 * N - 1, out), "flag", "pos"),
                       ((pos, flow, mask, H, W, N, 1, flow, out), "flag", "flow"), ((pos, flow, mask, H, W, N, 1, mask + H * W - 1, out), "flag", "mask"),
                       ((pos, flow, None, H, W, N, 0, out + 8, out), "out", "flag")):
        refused(d(*args, None), a + " overlaps " + b)
    need = lib.pivlfn_particles_render_workspace_bytes(B, N, H, W, R)
    assert 0 < need < 1 << 16
    r = lib.pivlfn_particles_render
    ok = [pos, diam, amp, flag, B, N, H, W, R, intensity, image, ws, need]

    def but(**kw):
        names = ["pos", "diam", "amp", "flag", "B", "N", "H", "W", "R", "intensity", "image", "ws", "need"]
        return [kw.get(n, v) for n, v in zip(names, ok)] + [None]
    refused(r(*but(H=0)), "particles_render", "bad shape")
    refused(r(*but(W=0)), "bad shape")
    refused(r(*but(H=1 << 16, W=1 << 15)), "2^31")
    refused(r(*but(H=1, W=(1 << 31) - 16)), "2^31 - 17")             # H*W < 2^31, but the last tile's pixel indices would pass 2^31
    refused(r(*but(H=(1 << 31) - 1, W=1)), "2^31 - 17")
    refused(r(*but(B=-1)), "B=-1")
    refused(r(*but(N=-1)), "N=-1")
    refused(r(*but(R=0)), "radius=0")
    refused(r(*but(R=9)), "radius=9")
    for name in ("pos", "diam", "amp", "intensity", "image", "ws"):
        refused(r(*but(**{name: None})), "null")
    refused(r(*but(ws=ws + 4)), "aligned")
    refused(r(*but(need=need - 1)), "needs")
    refused(r(*but(need=0)), "needs")
    for kw, a, b in ((dict(intensity=pos + 8), "intensity", "pos"), (dict(image=diam + 4 * B * N - 1), "image", "diam"), (dict(ws=amp - need + 8), "workspace", "amp"),
                     (dict(intensity=flag - 4 * B * H * W + 1), "intensity", "flag"), (dict(image=intensity), "intensity", "image"),
                     (dict(ws=image + 8), "image", "workspace"), (dict(ws=intensity + 8), "intensity", "workspace")):
        refused(r(*but(**kw)), a + " overlaps " + b)


# ---- the Python layer's parameter checks: none of them needs a GPU ----------------------------------------------------------------------
def test_generator_parameter_checks():
    from pivlfn import ParticleImageGen
    for kw in (dict(density=-0.1), dict(avg_diameter=-1.0), dict(std_diameter=-1.0), dict(laser_thickness=0), dict(density=float("nan")),
               dict(avg_diameter=0, std_diameter=0), dict(laser_thickness=float("inf"))):
        with pytest.raises(ValueError):
            ParticleImageGen(**kw)
    for kw in (dict(density="0.05"), dict(seed=1.5), dict(seed=True), dict(avg_diameter=None)):
        with pytest.raises(TypeError):
            ParticleImageGen(**kw)
    gen = ParticleImageGen(density=0.05, seed=3)
    assert (gen.p_density, gen.p_avg_d, gen.p_std_d, gen.lt) == (0.05, 1.5, 1.0, 1.0)
    assert gen.count(64, 48, 16) == int(np.floor(0.05 * 96 * 80))
    for args, kind in (((0, 8, 0), ValueError), ((8, 8, -1), ValueError), ((8, 8, 1.0), TypeError), ((8.0, 8, 0), TypeError),
                       ((1 << 16, 1 << 15, 0), ValueError)):
        with pytest.raises(kind):
            gen.count(*args)
    with pytest.raises(ValueError, match="2\\^31"):
        ParticleImageGen(density=1e6).count(1024, 1024, 0)
    # the seeding is a pure function of the seed and lies in the padded area
    x, y, z, d, z2 = gen._seeding(20, 30, 4, 3, 0.5)
    again = gen._seeding(20, 30, 4, 3, 0.5)
    assert all(np.array_equal(a, b) for a, b in zip((x, y, z, d, z2), again)) and not np.array_equal(x, gen._seeding(20, 30, 4, 4)[0])
    assert len(x) == gen.count(20, 30, 4) and x.min() >= -4 and x.max() < 34 and y.min() >= -4 and y.max() < 24
    assert d.min() >= 1.5 and d.max() < 2.5 and np.abs(z).max() <= 0.5 and not np.array_equal(z, z2)
    same = gen._seeding(20, 30, 4, 3)
    assert np.array_equal(same[2], z) and np.array_equal(same[4], z)          # without out_of_plane the depth stays
    with pytest.raises(NotImplementedError):
        ParticleImageGen(device="cpu").random_particle(8, 8)


def test_pair_parameter_checks():
    from pivlfn import ParticleImageGen
    gen = ParticleImageGen()
    flow = torch.zeros(1, 2, 8, 8)
    for kw, kind in ((dict(method="nearest"), ValueError), (dict(method=1), ValueError), (dict(out_of_plane=-1.0), ValueError),
                     (dict(out_of_plane=float("nan")), ValueError), (dict(out_of_plane="1"), TypeError), (dict(pad=-1), ValueError),
                     (dict(pad=2.0), TypeError), (dict(mask=torch.zeros(1, 8, 9, dtype=torch.uint8)), ValueError)):
        with pytest.raises(kind):
            gen.create_pair_from_flow(flow, **kw)
    with pytest.raises(TypeError):
        gen.create_pair_from_flow(flow.double())
    with pytest.raises(TypeError):
        gen.create_pair_from_flow(flow.numpy())
    with pytest.raises(ValueError):
        gen.create_pair_from_flow(torch.zeros(1, 3, 8, 8))
    with pytest.raises(NotImplementedError):
        gen.create_pair_from_flow(flow)                             # everything is in order but the device
    with pytest.raises(TypeError):
        gen.generate_image(torch.zeros(3), torch.zeros(3), torch.zeros(3), torch.zeros(2), 8, 8)


def test_displace_and_render_parameter_checks():
    from pivlfn import displace_particles, render_particles
    pos, flow = torch.zeros(2, 5, dtype=torch.float64), torch.zeros(2, 8, 8)
    for args, kw, kind in (((pos, flow), dict(method="linear"), ValueError), ((pos.float(), flow), {}, TypeError), ((pos, flow.double()), {}, TypeError),
                           ((pos.numpy(), flow), {}, TypeError), ((pos, flow), dict(mask=torch.zeros(8, 8)), TypeError),
                           ((pos, flow), dict(flag=torch.zeros(5)), TypeError), ((pos.t(), flow), {}, ValueError),
                           ((pos, flow[:, :1]), {}, ValueError), ((pos, flow[0]), {}, ValueError),
                           ((pos, flow), dict(mask=torch.zeros(8, 9, dtype=torch.uint8)), ValueError),
                           ((pos, flow), dict(flag=torch.zeros(4, dtype=torch.uint8)), ValueError), ((pos, flow), {}, NotImplementedError)):
        with pytest.raises(kind):
            displace_particles(*args, **kw)
    d, a = torch.ones(5), torch.ones(5)
    for args, kw, kind in (((pos, d, a, 0, 8), {}, ValueError), ((pos, d, a, 8, 8), dict(radius=0), ValueError), ((pos, d, a, 8, 8), dict(radius=9), ValueError),
                           ((pos, d, a, 8.0, 8), {}, TypeError), ((pos, d, a, 8, 8), dict(radius=True), TypeError),
                           ((pos, d, a, 1 << 16, 1 << 15), {}, ValueError), ((pos, d, a, 1, (1 << 31) - 16), {}, ValueError), ((pos.float(), d, a, 8, 8), {}, TypeError),
                           ((pos, d.double(), a, 8, 8), {}, TypeError), ((pos, d, a.numpy(), 8, 8), {}, TypeError),
                           ((pos, d, a, 8, 8), dict(flag=torch.zeros(5)), TypeError), ((pos.t(), d, a, 8, 8), {}, ValueError),
                           ((pos, d[:4], a, 8, 8), {}, ValueError), ((pos[None], d, a, 8, 8), {}, ValueError),
                           ((pos, d, a, 8, 8), dict(flag=torch.zeros(4, dtype=torch.uint8)), ValueError), ((pos, d, a, 8, 8), {}, NotImplementedError)):
        with pytest.raises(kind):
            render_particles(*args, **kw)


def test_new_symbols_are_bound_and_refuse_without_a_gpu():
    """The three header symbols have ctypes prototypes, and the argument errors are reported before any launch (so without a GPU)."""
    from pivlfn import _lib
    for name in ("pivlfn_particles_displace", "pivlfn_particles_render", "pivlfn_particles_render_workspace_bytes"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    base = 1 << 20                                                  # never dereferenced: every case fails its checks first
    refusals(lib, *(base + (i << 16) for i in range(10)))
    assert lib.pivlfn_particles_displace(None, None, None, 4, 4, 0, 0, None, None, None) == 0        # N == 0 reads nothing
    assert lib.pivlfn_particles_render(None, None, None, None, 0, 5, 4, 4, 4, None, None, None, 0, None) == 0     # B == 0 neither
    assert lib.pivlfn_particles_render_workspace_bytes(2, 100, 37, 53, 4) == 16 + 24 * 4 + 24 * 8 + 2 * 100 * 4 * 4
    assert lib.pivlfn_particles_render_workspace_bytes(1, 100, 16, 16, 8) == 16 + 8 + 8 + 100 * 9 * 4
    for bad in ((-1, 1, 4, 4, 4), (1, -1, 4, 4, 4), (1, 1, 0, 4, 4), (1, 1, 4, 4, 0), (1, 1, 4, 4, 9), (1, 1, 1 << 16, 1 << 15, 4), (1, 1, 1, (1 << 31) - 16, 4)):
        assert lib.pivlfn_particles_render_workspace_bytes(*bad) == 0
