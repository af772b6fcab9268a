"""CPU: the vortex identification contract (include/pivlfn.h, pivlfn_vortex_gamma) as tests/vortex_restatement.py states it -- the loop
definition against the vectorised form bit for bit -- the physics the functions are wanted for, checked on the restatement, and the
host side of pivlfn.vortex and run.py --vortex: parameter checks, cores / sums / peaks on hand-made fields, the refusals of the C entry
point, which all come before any launch and so need no GPU."""
import math

import numpy as np
import pytest
import torch

import vortex_restatement as vr
from vortex_restatement import CENTRE_OUT, CORE, FEW

RC = 0.18 * 128                     # pivlfn.synth.displacement_field's core radius at 128 x 128
R_VMAX = 1.1209                     # the radius of the largest tangential velocity of a Lamb-Oseen vortex, in core radii


def _field(gamma, flag, r, s=1):
    """A VortexField on the host from the restatement's output of one pair."""
    from pivlfn import VortexField
    return VortexField(torch.from_numpy(gamma[None, 0]), torch.from_numpy(gamma[None, 1]), torch.from_numpy(flag[None]), r, s)


@pytest.mark.parametrize("r,s", [(1, 1), (2, 1), (3, 2), (2, 5)])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (5, 3), (13, 17), (37, 53)])
def test_loops_equal_planes_bit_for_bit(H, W, r, s):
    """With a mask, NaN, -inf and 1e10 vectors; then without the mask and with min_count 1, where few pixels are FEW."""
    flow, mask = vr.random_case(np.random.default_rng(100 * H + W), 1, H, W)
    seen = 0
    for m, mc in ((mask[0], None), (None, 1)):
        a, b = vr.gamma_loops(flow[0], r, s, m, mc), vr.gamma_planes(flow[0], r, s, m, mc)
        assert vr.same_bits(a[0], b[0]) and vr.same_bits(a[1], b[1])
        assert a[0].dtype == np.float32 and a[1].dtype == np.uint8 and a[0].shape == (2, H, W)
        few = (a[1] & FEW) != 0
        assert np.isnan(a[0][:, few]).all() and np.isfinite(a[0][:, ~few]).all()
        seen |= int(a[1].max())
    if H * W > 1:
        assert seen & CENTRE_OUT
    if (H, W) == (1, 1):
        assert (a[1] & FEW).all()                  # a vector without neighbours


def test_by_hand_on_a_1x3_row():
    """u = (1, 0, -1), v = (0, 2, 0), r = 1, min_count 1.  Centre pixel: neighbours i = -1 (ux, uy) = (1, 0) and i = +1 (-1, 0); the
    directions are (-1, 0) and (1, 0); px*uy - py*ux = 0 for both: Gamma1 = 0.  The mean is (0, 2/3): du = (1, -1), dv = (-2/3, -2/3);
    px*dv - py*du = 2/3 and -2/3 over the same m2: Gamma2 = 0.  Left pixel: its one neighbour (0, 1) lies in direction (1, 0):
    Gamma1 = 1*1 - 0*0 = 1; the right pixel sees it in direction (-1, 0): Gamma1 = -1."""
    flow = np.array([[[1.0, 0.0, -1.0]], [[0.0, 2.0, 0.0]]], np.float32)
    for one in (vr.gamma_loops, vr.gamma_planes):
        g, f = one(flow, 1, 1, None, 1)
        assert not f.any()
        assert g[0, 0, 1] == 0.0 and g[1, 0, 1] == 0.0 and g[0, 0, 0] == 1.0 and g[0, 0, 2] == -1.0


def test_uniform_and_zero_flows_give_gamma2_zero_exactly():
    for u, v in ((0.0, 0.0), (1.5, -0.75)):
        flow = np.stack([np.full((9, 11), u), np.full((9, 11), v)]).astype(np.float32)
        g, f = vr.gamma_planes(flow, 2, 1, None, 1)
        assert not f.any() and not g[1].any()


def _grid(n=41):
    y, x = np.mgrid[0:n, 0:n].astype(np.float64) - n // 2
    return x, y


def test_rigid_rotation_strain_and_shear():
    """Rigid rotation: Gamma1 = 1 at its centre, Gamma2 >= 1 - 1e-12 wherever the window is whole (the mean of a whole window is the
    vector at its centre).  Pure strain: |Gamma2| < 1e-12.  The plain shear u = 0.1 y has vorticity -0.1 everywhere and
    0.60 < |Gamma2| < 2/pi: vorticity calls it a vortex, Gamma2 does not."""
    x, y = _grid()
    c = 20
    for r in (1, 3):
        inner = (slice(r, -r), slice(r, -r))
        rot, _ = vr.gamma_planes(np.stack([-y, x]).astype(np.float32), r)
        assert abs(float(rot[0, c, c]) - 1.0) < 1e-6 and float(rot[1][inner].min()) >= 1.0 - 1e-12
        strain, _ = vr.gamma_planes(np.stack([x, -y]).astype(np.float32), r)
        assert float(np.abs(strain[1][inner]).max()) < 1e-12
        shear, _ = vr.gamma_planes(np.stack([0.1 * y, 0.0 * y]).astype(np.float32), r)
        g2 = shear[1][inner]
        assert (g2 < 0).all() and 0.60 < float(np.abs(g2).min()) and float(np.abs(g2).max()) < CORE
    assert abs(float(vr.gamma_planes(np.stack([0.1 * y, 0.0 * y]).astype(np.float32), 1)[0][1, c, c]) + 0.6036) < 1e-4


@pytest.fixture(scope="module")
def lamb_oseen():
    """(drift, r) -> (gamma, flag) of the project's Lamb-Oseen field 128 x 128, peak 4 px."""
    return {(drift, r): vr.gamma_planes(vr.lamb_oseen(shift=(1.5, -0.75) if drift else (0.0, 0.0)), r)
            for drift in (True, False) for r in (2, 4)}


@pytest.mark.parametrize("r", [2, 4])
@pytest.mark.parametrize("drift", [True, False])
def test_lamb_oseen_centre_and_core(lamb_oseen, drift, r):
    """One Gamma2 peak, within 0.5 px of the true centre (63.5, 63.5) with a value above 0.99; the region |Gamma2| > 2/pi has the
    equivalent radius of the largest tangential velocity, 1.1209 rc, to 2 % (restatement: +0.6 %).  Gamma1 is not Galilean invariant:
    with the drift its maximum lies more than 4 px off."""
    gamma, flag = lamb_oseen[(drift, r)]
    v = _field(gamma, flag, r)
    (peaks,) = v.peaks()
    assert len(peaks) == 1
    (p,) = peaks
    assert math.hypot(p["x"] - 63.5, p["y"] - 63.5) <= 0.5 and p["value"] > 0.99
    radius = vr.core_radius(gamma[1])
    print(f"drift {drift} r {r}: peak ({p['x']:.3f}, {p['y']:.3f}) value {p['value']:.6f}, core radius {radius:.3f} against {R_VMAX * RC:.3f}")
    assert abs(radius / (R_VMAX * RC) - 1.0) < 0.02
    (s,) = v.summary()
    assert s["radius_pos"] == radius and s["area_neg"] == 0
    iy, ix = np.unravel_index(np.nanargmax(np.abs(gamma[0])), gamma[0].shape)
    off = math.hypot(ix - 63.5, iy - 63.5)
    assert off > 4.0 if drift else off < 1.0


def test_counter_rotating_pair():
    """96 x 128, centres (36.5, 47.5) and (91.5, 47.5), rc = 10, peaks +-3 px, drift (1.5, -0.75), r = 4: two peaks of opposite sign,
    each within 0.75 px of its centre; both core radii within 3 % of 1.1209 rc = 11.21 (restatement: +1.2 %)."""
    gamma, flag = vr.gamma_planes(vr.vortex_pair(), 4)
    (peaks,) = _field(gamma, flag, 4).peaks()
    assert len(peaks) == 2
    by_x = sorted(peaks, key=lambda p: p["x"])
    assert by_x[0]["value"] > 0.99 and by_x[1]["value"] < -0.99
    for p, (cx, cy) in zip(by_x, ((36.5, 47.5), (91.5, 47.5))):
        assert math.hypot(p["x"] - cx, p["y"] - cy) <= 0.75
    for sign in (1, -1):
        radius = vr.core_radius(gamma[1], sign)
        print(f"sign {sign}: core radius {radius:.3f}")
        assert abs(radius / 11.21 - 1.0) < 0.03


def test_gaussian_noise_has_no_core():
    noise = np.random.default_rng(3).normal(0, 1, (2, 64, 64)).astype(np.float32)
    gamma, _ = vr.gamma_planes(noise, 2, 2)
    assert float(np.nanmax(np.abs(gamma[1]))) < CORE


def test_check_params_and_argument_errors():
    from pivlfn import VortexField, vortex_gamma
    from pivlfn.vortex import CENTRE_OUT as centre_out, CORE as core, FEW as few, check_params, default_min_count
    assert (few, centre_out) == (FEW, CENTRE_OUT) == (1, 2) and core == CORE
    assert default_min_count(4) == 40 == vr.default_min_count(4) and default_min_count(1) == 4
    assert check_params(4, 1, None) == 40 and check_params(1, 16, 8) == 8 and check_params(15, 3, 1) == 1
    flow = torch.zeros(2, 2, 8, 8)
    for bad in (0, 16, 2.0, True, None):
        with pytest.raises(ValueError, match="radius"):
            vortex_gamma(flow, radius=bad)
    for bad in (0, 17, 1.0, False, None):
        with pytest.raises(ValueError, match="spacing"):
            vortex_gamma(flow, spacing=bad)
    for bad in (0, 25, 3.0, False):
        with pytest.raises(ValueError, match="min_count"):
            vortex_gamma(flow, radius=2, min_count=bad)
    with pytest.raises(TypeError, match="float32"):
        vortex_gamma(flow.double())
    with pytest.raises(TypeError, match="torch tensor"):
        vortex_gamma(np.zeros((2, 2, 8, 8), np.float32))
    with pytest.raises(NotImplementedError, match="GPU"):            # there is no CPU path
        vortex_gamma(flow)
    empty = VortexField(torch.zeros(0, 4, 4), torch.zeros(0, 4, 4), torch.zeros(0, 4, 4, dtype=torch.uint8))
    assert empty.summary() == [] and empty.peaks() == [] and (empty.radius, empty.spacing) == (4, 1)
    for kw in ({"of": "gamma3"}, {"distance": 0}, {"distance": 1.5}):
        with pytest.raises(ValueError):
            VortexField(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8)).peaks(**kw)


def test_cores_sums_and_summary_on_known_values():
    from pivlfn import VortexField
    from pivlfn.vortex import SUMS, summarize
    buf = torch.zeros(1, 2, 2, 3)
    buf[0, 0] = torch.tensor([[0.5, math.nan, -0.25], [0.0, 1.0, 0.0]])
    buf[0, 1] = torch.tensor([[0.7, math.nan, -0.9], [0.6, -0.64, 0.65]])
    flag = torch.tensor([[[0, FEW | CENTRE_OUT, 0], [0, CENTRE_OUT, 0]]], dtype=torch.uint8)
    v = VortexField(buf[:, 0], buf[:, 1], flag)
    assert v.gamma1.data_ptr() == buf.data_ptr() and v.gamma2.data_ptr() == buf[:, 1].data_ptr()
    cores = v.cores()
    assert cores.dtype == torch.int8 and cores.tolist() == [[[1, 0, -1], [0, -1, 1]]]
    assert v.cores(0.8).tolist() == [[[0, 0, -1], [0, 0, 0]]]
    sums = v.sums()
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (1, len(SUMS)) == (1, 7)
    assert sums[0, :5].tolist() == [6.0, 1.0, 5.0, 2.0, 2.0]
    g = buf.double()
    assert abs(float(sums[0, 5]) - float(g[0, 0].nan_to_num().abs().sum())) < 1e-15
    assert abs(float(sums[0, 6]) - float(g[0, 1].nan_to_num().abs().sum())) < 1e-15
    (s,) = v.summary()
    assert s == summarize(sums[0].tolist())
    assert s["few"] == 1 / 6 and s["defined"] == 5 and s["area_pos"] == 2 and s["area_neg"] == 2 and s["fraction_core"] == 4 / 6
    assert s["radius_pos"] == math.sqrt(2 / math.pi) == s["radius_neg"] and abs(s["mean_abs_gamma1"] - 1.75 / 5) < 1e-12
    both = summarize((sums[0] + sums[0]).tolist())                  # additive over pairs
    assert both["area_pos"] == 4 and both["fraction_core"] == s["fraction_core"] and abs(both["mean_abs_gamma2"] - s["mean_abs_gamma2"]) < 1e-15
    none = summarize([0.0] * 7)
    assert math.isnan(none["few"]) and math.isnan(none["mean_abs_gamma1"]) and none["radius_pos"] == 0.0


def _peaks_of(rows, **kw):
    from pivlfn import VortexField
    g2 = torch.tensor(rows, dtype=torch.float32)[None]
    return VortexField(torch.zeros_like(g2), g2, torch.zeros(g2.shape, dtype=torch.uint8), 1, 1).peaks(**kw)[0]


def test_peaks_tie_rule_and_sub_pixel_step():
    """Hand-made 5 x 7 fields, distance 1 (radius 1, spacing 1), threshold 0.9."""
    z = [0.0] * 7
    # a 2 x 2 plateau: four candidates of one value; the lowest linear index is kept, the others lie within distance 1 of it;
    # parabola through (0, 0.95, 0.95): den = 0 - 1.9 + 0.95 = -0.95, 0.5 * (0 - 0.95) / -0.95 = +0.5 on both axes
    (p,) = _peaks_of([z, [0, 0, 0.95, 0.95, 0, 0, 0], [0, 0, 0.95, 0.95, 0, 0, 0], z, z])
    assert (p["ix"], p["iy"], p["x"], p["y"]) == (2, 1, 2.5, 1.5) and abs(p["value"] - 0.95) < 1e-7
    # two equal peaks further apart than the distance: both kept, in index order; a stronger negative one comes first, signed
    got = _peaks_of([z, [0, -0.92, 0, 0, 0, 0.92, 0], z, [0, 0, 0, -0.97, 0, 0, 0], z])
    assert [(p["ix"], p["iy"]) for p in got] == [(3, 3), (1, 1), (5, 1)]
    assert got[0]["value"] < -0.96 and got[1]["value"] < 0 < got[2]["value"]
    # Chebyshev distance 2 > 1: a diagonal neighbour two steps off survives; with distance 2 it is suppressed by the stronger one
    rows = [z, [0, 0.95, 0, 0, 0, 0, 0], z, [0, 0, 0, 0.93, 0, 0, 0], z]
    assert [(p["ix"], p["iy"]) for p in _peaks_of(rows)] == [(1, 1), (3, 3)]
    assert [(p["ix"], p["iy"]) for p in _peaks_of(rows, distance=2)] == [(1, 1)]
    # below the threshold: nothing; a lower threshold finds it
    assert _peaks_of([z, [0, 0, 0.8, 0, 0, 0, 0], z, z, z]) == [] and len(_peaks_of([z, [0, 0, 0.8, 0, 0, 0, 0], z, z, z], threshold=0.5)) == 1
    # the parabola: (0.5, 1.0, 0.75) along x: den = 0.5 - 2 + 0.75 = -0.75, step 0.5 * (0.5 - 0.75) / -0.75 = 1/6; along y symmetric: 0
    (p,) = _peaks_of([z, [0, 0, 0, 0.6, 0, 0, 0], [0, 0, 0.5, 1.0, 0.75, 0, 0], [0, 0, 0, 0.6, 0, 0, 0], z])
    assert abs(p["x"] - (3 + 1 / 6)) < 1e-7 and p["y"] == 2.0
    # a missing neighbour (the image edge) and a NaN neighbour give a step of +0 on that axis; the NaN is never a candidate
    nan = math.nan
    (p,) = _peaks_of([[0.99, 0.5, 0, 0, 0, 0, 0], [0.7, 0, 0, 0, 0, 0, 0], z, z, z])
    assert (p["x"], p["y"]) == (0.0, 0.0)
    (p,) = _peaks_of([z, [0, 0, nan, 0.95, 0.5, 0, 0], z, z, z])
    assert (p["ix"], p["x"], p["y"]) == (3, 3.0, 1.0)
    # gamma1 is searched on request
    from pivlfn import VortexField
    g = torch.zeros(1, 5, 7)
    g[0, 2, 4] = -0.95
    (found,) = VortexField(g, torch.zeros_like(g), torch.zeros(g.shape, dtype=torch.uint8), 1, 1).peaks(of="gamma1")
    assert [(p["ix"], p["iy"], p["value"] < 0) for p in found] == [(4, 2, True)]


def refusals(lib, flow, mask, gamma, flag, ws, B, H, W, r):
    """Every error of the contract through the C entry point with the given addresses (never dereferenced: each call fails its checks
    before any launch); also called by the GPU test with real buffers, whose contents must stay."""
    need = lib.pivlfn_vortex_gamma_workspace_bytes(B, H, W, r, 1)
    assert need >= B * H * W * 17 and need % 256 == 0
    for bad in ((0, H, W, r, 1), (B, H, W, 16, 1), (B, H, W, 0, 1), (B, H, W, r, 0), (B, H, W, r, 17), (B, -1, W, r, 1)):
        assert lib.pivlfn_vortex_gamma_workspace_bytes(*bad) == 0

    def call(**kw):
        a = dict(flow=flow, mask=mask, gamma=gamma, flag=flag, B=B, H=H, W=W, radius=r, spacing=1, min_count=(2 * r + 1) ** 2 // 2,
                 ws=ws, ws_bytes=need)
        a.update(kw)
        return lib.pivlfn_vortex_gamma(a["flow"], a["mask"], a["gamma"], a["flag"], a["B"], a["H"], a["W"], a["radius"], a["spacing"],
                                       a["min_count"], a["ws"], a["ws_bytes"], None)

    def refused(rc, *words):
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1, (rc, msg)
        for w in ("vortex_gamma",) + words:
            assert w in msg, (w, msg)

    for name in ("flow", "gamma", "flag", "ws"):
        refused(call(**{name: None}), "null")
    refused(call(B=0), "positive")
    refused(call(H=-1), "positive")
    refused(call(W=0), "positive")
    refused(call(H=46341, W=46341), "2^31")
    refused(call(B=65536), "B=65536")
    refused(call(radius=0), "radius=0")
    refused(call(radius=16), "radius=16")
    refused(call(spacing=0), "spacing=0")
    refused(call(spacing=17), "spacing=17")
    refused(call(min_count=0), "min_count=0")
    refused(call(min_count=(2 * r + 1) ** 2), f"min_count={(2 * r + 1) ** 2}")
    refused(call(ws=ws + 4), "8-byte aligned")
    refused(call(ws_bytes=need - 1), "too small")
    refused(call(ws_bytes=0), "too small")
    px = B * H * W
    refused(call(gamma=flow), "gamma overlaps flow")
    refused(call(gamma=flow + px * 8 - 4), "gamma overlaps flow")
    refused(call(gamma=flow - px * 8 + 4), "gamma overlaps flow")
    refused(call(gamma=mask), "gamma overlaps mask")
    refused(call(gamma=ws + 8), "gamma overlaps the workspace")
    refused(call(flag=flow + px * 8 - 1), "flag overlaps flow")
    refused(call(flag=mask), "flag overlaps mask")
    refused(call(flag=ws + need - 1), "flag overlaps the workspace")
    refused(call(flag=gamma + px * 8 - 1), "gamma overlaps flag")
    return call


def test_c_entry_point_refuses_bad_arguments_without_a_gpu():
    """Every refusal of pivlfn_vortex_gamma comes from the host, before any launch, as PIVLFN_ERR_ARG with a message naming the problem
    (a launch on a machine without a GPU would return PIVLFN_ERR_HIP instead)."""
    from pivlfn import _lib
    lib = _lib.load()
    P = 1 << 20                     # non-null, 8-byte aligned, never dereferenced
    flow, mask, gamma, flag, ws = (P + (i << 32) for i in range(5))          # five ranges that cannot overlap at these sizes
    call = refusals(lib, flow, mask, gamma, flag, ws, 2, 8, 8, 2)
    with pytest.raises(ValueError, match="radius=16"):
        _lib.check(call(radius=16), "vortex_gamma")


def test_run_py_vortex_flags_parse_and_are_checked_before_a_gpu_is_needed(tmp_path):
    import run as runpy
    plain = runpy.parser.parse_args(["-i", "x"])
    assert plain.vortex is None and plain.vortex_spacing is None and plain.vortex_image is False
    assert not [ln for ln in runpy.args_lines(plain) if "vortex" in ln or "gamma" in ln]
    assert runpy.parser.parse_args(["--vortex"]).vortex == 4
    full = runpy.parser.parse_args(["--vortex", "6", "--vortex-spacing", "2", "--vortex-image"])
    assert (full.vortex, full.vortex_spacing, full.vortex_image) == (6, 2, True)
    lines = runpy.args_lines(full)
    assert "vortex: 6\n" in lines and "vortex_spacing: 2\n" in lines and "vortex_image: True\n" in lines
    assert not [ln for ln in lines if ln.startswith(("color", "quality", "pod"))]
    assert not [ln for ln in runpy.args_lines(runpy.parser.parse_args(["--quality"])) if "vortex" in ln]
    base = ["--model", "piv", "-i", str(tmp_path), "-o", str(tmp_path / "out")]
    for extra, word in ((["--vortex-image"], "need --vortex"), (["--vortex-spacing", "2"], "need --vortex"), (["--vortex", "16"], "radius=16"),
                        (["--vortex", "0"], "radius=0"), (["--vortex", "--vortex-spacing", "17"], "spacing=17"),
                        (["--vortex", "--vortex-spacing", "0"], "spacing=0"), (["--vortex", "-c", "1.5"], "-b/-c"),
                        (["--vortex", "-b", "0.5"], "-b/-c")):
        with pytest.raises(SystemExit, match=word):
            runpy.main(base + extra)
    assert not (tmp_path / "out").exists()
