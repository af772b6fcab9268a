"""CPU: the numpy restatement of the reference's motion_to_color against the reference's own pictures, the C ABI of the picture entry
points and their host-side refusals, PNG output, run.py's picture flags and the src.utils_plot alias.  No GPU."""
import builtins
import ctypes
import hashlib
import inspect
import json
import os
import re

import numpy as np
import pytest

import viz_restatement as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REFERENCE = os.environ.get("PIVLFN_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))      # a checkout beside this one


@pytest.fixture(scope="module")
def cases():
    return np.load(os.path.join(GOLD, "viz_cases.npz"))


@pytest.fixture(scope="module")
def report():
    return json.load(open(os.path.join(GOLD, "pin_report_viz.json")))


def _maxmotion(cases, tag):
    m = float(cases[f"{tag}_maxmotion"])
    return None if np.isnan(m) else m


def test_restatement_matches_reference_fixture(cases, report):
    tags = list(cases["cases"])
    assert len(tags) >= 16 and set(tags) == set(report["cases"])
    for tag in tags:
        flow = cases[f"{tag}_flow"]
        assert flow.dtype == np.float32
        for wheel in ("interp", "original"):
            got = vr.motion_to_color(flow, _maxmotion(cases, tag), wheel == "original")
            want = cases[f"{tag}_bgr_{wheel}"]
            assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (tag, wheel)
            assert report["cases"][tag]["differing_values"][wheel] == 0


def test_fixture_covers_the_edge_cases(cases, report):
    """The signed zeros, the maximum pixel above and on 1, the darkened branch, the degenerate shapes and the packing tails."""
    assert cases["signed_zeros_bgr_interp"].tolist() == [[[0, 0, 255], [42, 0, 255], [255, 208, 0], [255, 255, 255]]]
    assert (cases["zeros_bgr_interp"] == 255).all()
    tags = list(cases["cases"])
    above = [t for t in tags if t.startswith("max_above_one")][0]
    exact = [t for t in tags if t.startswith("max_exactly_one")][0]
    assert above == "max_above_one_seed9" and report["max_above_one_seed"] == 9
    for tag, check in ((above, lambda r: r > 1), (exact, lambda r: r == 1)):
        nchw = cases[f"{tag}_flow"].transpose(2, 0, 1)[None]
        rad, _ = vr.flow_fk(nchw, vr.flow_maxrad(nchw))
        assert check(rad.max()) and rad.dtype == np.float32, tag
    # the pixel above 1 takes the * 0.75 branch: no channel above 191
    flow = cases[f"{above}_flow"]
    at = np.unravel_index(np.argmax(flow[..., 0] ** 2 + flow[..., 1] ** 2), flow.shape[:2])
    assert cases[f"{above}_bgr_interp"][at].max() <= 191 and cases[f"{exact}_bgr_interp"].reshape(-1, 3).max(axis=1).min() > 191
    nchw = cases["odd13x17_flow"].transpose(2, 0, 1)[None]
    assert (vr.flow_fk(nchw, [2.0])[0] > 1).mean() > 0.3
    shapes = {tuple(cases[f"{t}_flow"].shape[:-1]) for t in tags}
    assert {(1, 1), (1, 9), (9, 1), (5, 3), (4, 5), (3, 7), (13, 17), (64, 96), (3, 6, 10)} <= shapes
    seq = cases["sequence3_flow"].transpose(0, 3, 1, 2)
    assert len(set(vr.flow_maxrad(seq).tolist())) == 3
    assert os.path.getsize(os.path.join(GOLD, "viz_cases.npz")) < 200 * 1024


def test_pin_report_names_the_reference_files(report):
    assert set(report["reference_sha256"]) == {"src/utils_plot.py", "src/utils_color.py"} and report["numpy"]
    for rel, digest in report["reference_sha256"].items():
        assert re.fullmatch(r"[0-9a-f]{64}", digest)
        path = os.path.join(REFERENCE, rel)
        if os.path.isfile(path):                       # the reference is an optional neighbour of the checkout
            assert hashlib.sha256(open(path, "rb").read()).hexdigest() == digest, rel


def test_restatement_leaves_unknown_and_masked_vectors_out():
    rng = np.random.default_rng(5)
    flow = rng.normal(0, 2, (2, 2, 6, 7)).astype(np.float32)
    flow[0, 0, 1, 2], flow[0, 1, 3, 3], flow[0, 0, 4, 4], flow[0, 1, 5, 5] = np.nan, 1e10, -np.inf, 2e9
    flow[0, 0, 0, 0] = 50.0
    mask = np.zeros((2, 6, 7), np.uint8)
    mask[0, 0, 0] = 4
    clean = flow.copy()
    for y, x in ((1, 2), (3, 3), (4, 4), (5, 5), (0, 0)):
        clean[0, :, y, x] = 0
    assert np.array_equal(vr.flow_maxrad(flow, mask), vr.flow_maxrad(clean)) and vr.flow_maxrad(flow)[0] >= np.float32(50.0)
    assert vr.flow_maxrad(flow, mask)[0] < 20 and vr.flow_maxrad(flow)[0] >= 50
    img = vr.flow_to_color(flow, vr.flow_maxrad(flow, mask), mask)
    for y, x in ((1, 2), (3, 3), (4, 4), (5, 5), (0, 0)):
        assert img[0, y, x].tolist() == [0, 0, 0]
    assert (img[1].reshape(-1, 3).max(axis=1) > 0).all()
    gone = np.full((1, 2, 3, 3), np.nan, np.float32)
    assert vr.flow_maxrad(gone)[0] == 0 and not vr.flow_to_color(gone, [0.0]).any()
    mean, count = vr.flow_decimate(flow, 4, mask)
    assert mean.shape == (2, 2, 2, 2) and count[0].tolist() == [[13, 12], [8, 4]] and count[1].tolist() == [[16, 12], [8, 6]]
    mean, count = vr.flow_decimate(gone, 2)
    assert (mean == np.float32(1e10)).all() and not count.any()


def test_the_vectorised_cell_means_are_the_loops():
    """vr.flow_decimate_planes, which the GPU tests use on images of millions of pixels, against the definition vr.flow_decimate: the
    shapes and hole patterns of tests/test_gpu_viz.py's small cases, cells 1, 4 and 5, with -0.0 and values of very different size."""
    for B, H, W in ((1, 1, 1), (1, 1, 9), (1, 9, 1), (3, 13, 17), (1, 67, 131)):
        rng = np.random.default_rng(B * 100000 + H * 1000 + W)
        flow = (rng.normal(0, 3, (B, 2, H, W)) * 10.0 ** rng.integers(-3, 4, (B, 2, H, W))).astype(np.float32)
        vals = (np.nan, 1e10, -np.inf, 2e9, -0.0)
        n = max(1, H * W // 10)
        for j, (b, c, y, x) in enumerate(zip(rng.integers(0, B, n), rng.integers(0, 2, n), rng.integers(0, H, n), rng.integers(0, W, n))):
            flow[b, c, y, x] = vals[j % 5]
        mask = (rng.random((B, H, W)) < 0.1).astype(np.uint8) * 5
        gone = flow.copy()
        gone[-1, 0, :H // 2 + 1] = np.nan
        for f, m in ((flow, None), (flow, mask), (gone, mask)):
            for cell in (1, 4, 5):
                want, got = vr.flow_decimate(f, cell, m), vr.flow_decimate_planes(f, cell, m)
                for a, b in zip(got, want):
                    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (B, H, W, cell)
        assert (vr.flow_decimate(gone, 1, mask)[1] == 0).any()


def test_restatement_scalar_map_bins():
    from pivlfn.viz import LUTS
    lut = LUTS["gray"]
    x = np.array([[[-2.0, -1.0, -1.0 + 2 / 256, 0.0, 1.0 - 1e-9, 1.0, 7.0, np.nan, np.inf]]])
    img = vr.scalar_to_color(x, -1.0, 1.0, lut, bad=(9, 8, 7))
    assert img[0, 0, :, 0].tolist() == [0, 0, 1, 128, 255, 255, 255, 9, 9] and img[0, 0, 7].tolist() == [9, 8, 7]
    assert vr.field_absmax(x)[0] == 7.0
    bwr = LUTS["bwr"]
    assert bwr.shape == (256, 3) and bwr.dtype == np.uint8
    assert bwr[0].tolist() == [0, 0, 255] and bwr[255].tolist() == [255, 0, 0] and bwr[127].tolist() == [254, 254, 255]
    assert (np.diff(bwr[:, 0].astype(int)) >= 0).all() and (np.diff(bwr[:, 2].astype(int)) <= 0).all()


def _declared():
    text = open(os.path.join(ROOT, "include", "pivlfn.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


ENTRIES = ("pivlfn_flow_maxrad", "pivlfn_flow_to_color", "pivlfn_field_absmax", "pivlfn_scalar_to_color", "pivlfn_flow_decimate")


def test_header_and_library_export_the_picture_entries():
    text = _declared()
    for name in ENTRIES:
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
    for name, value in (("PIVLFN_WHEEL_INTERP", 0), ("PIVLFN_WHEEL_ORIGINAL", 1), ("PIVLFN_ORDER_RGB", 0), ("PIVLFN_ORDER_BGR", 1)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", text), name
    from pivlfn import _lib
    assert set(ENTRIES) <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert lib.pivlfn_abi_version() == 3
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name
    import pivlfn
    from pivlfn import viz
    for name in ("flow_to_color", "motion_to_color", "scalar_to_color", "vorticity_image", "decimate_flow", "quiver_plot",
                 "color_wheel_image", "write_png", "PngWriter", "flow_maxrad", "field_absmax"):
        assert getattr(pivlfn, name) is getattr(viz, name) and name in pivlfn.__all__, name


def test_picture_entries_refuse_bad_arguments_without_a_gpu():
    """Refused on the host with PIVLFN_ERR_ARG and a message naming the problem, before anything is launched."""
    from pivlfn import _lib
    lib = _lib.load()
    P = 4096                      # a non-null pointer that is never dereferenced: every case below fails its checks first

    def refused(rc, *words):
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    shaped = (
        ("flow_maxrad", lambda B, H, W: lib.pivlfn_flow_maxrad(P, None, P, B, H, W, None)),
        ("flow_to_color", lambda B, H, W: lib.pivlfn_flow_to_color(P, P, None, P, B, H, W, 0, 0, None)),
        ("field_absmax", lambda B, H, W: lib.pivlfn_field_absmax(P, 0, None, P, B, H, W, None)),
        ("scalar_to_color", lambda B, H, W: lib.pivlfn_scalar_to_color(P, 0, None, P, P, B, H, W, -1.0, 1.0, 0, None)),
        ("flow_decimate", lambda B, H, W: lib.pivlfn_flow_decimate(P, None, P, P, B, H, W, 4, None)),
    )
    for what, call in shaped:
        refused(call(0, 4, 4), what, "B=0")
        refused(call(1, 0, 4), what, "H=0")
        refused(call(1, -3, 4), what, "H=-3")
        refused(call(1, 4, 0), what, "W=0")
        refused(call(1, 46341, 46341), what, "2^31")
        refused(call(70000, 4, 4), what, "B=70000", "65535")
    refused(lib.pivlfn_flow_maxrad(None, None, P, 1, 4, 4, None), "flow_maxrad", "null")
    refused(lib.pivlfn_flow_maxrad(P, None, None, 1, 4, 4, None), "flow_maxrad", "null")
    for args in ((None, P, None, P), (P, None, None, P), (P, P, None, None)):
        refused(lib.pivlfn_flow_to_color(*args, 1, 4, 4, 0, 0, None), "flow_to_color", "null")
    refused(lib.pivlfn_flow_to_color(P, P, None, P, 1, 4, 4, 2, 0, None), "wheel=2")
    refused(lib.pivlfn_flow_to_color(P, P, None, P, 1, 4, 4, 0, -1, None), "order=-1")
    refused(lib.pivlfn_field_absmax(None, 0, None, P, 1, 4, 4, None), "field_absmax", "null")
    refused(lib.pivlfn_field_absmax(P, 0, None, None, 1, 4, 4, None), "field_absmax", "null")
    refused(lib.pivlfn_field_absmax(P, 2, None, P, 1, 4, 4, None), "is_f64=2")
    for args in ((None, 0, None, P, P), (P, 0, None, None, P), (P, 0, None, P, None)):
        refused(lib.pivlfn_scalar_to_color(*args, 1, 4, 4, -1.0, 1.0, 0, None), "scalar_to_color", "null")
    refused(lib.pivlfn_scalar_to_color(P, 0, None, P, P, 1, 4, 4, 0.5, 0.5, 0, None), "vmax == vmin")
    refused(lib.pivlfn_scalar_to_color(P, 0, None, P, P, 1, 4, 4, float("nan"), 1.0, 0, None), "finite")
    refused(lib.pivlfn_scalar_to_color(P, 0, None, P, P, 1, 4, 4, 0.0, float("inf"), 0, None), "finite")
    refused(lib.pivlfn_scalar_to_color(P, 0, None, P, P, 1, 4, 4, 0.0, 5e-324, 0, None), "narrow")
    refused(lib.pivlfn_scalar_to_color(P, 0, None, P, P, 1, 4, 4, 0.0, 1.0, 1 << 24, None), "bad_rgb")
    refused(lib.pivlfn_scalar_to_color(P, 3, None, P, P, 1, 4, 4, 0.0, 1.0, 0, None), "is_f64=3")
    for args in ((None, None, P, P), (P, None, None, P), (P, None, P, None)):
        refused(lib.pivlfn_flow_decimate(*args, 1, 4, 4, 4, None), "flow_decimate", "null")
    refused(lib.pivlfn_flow_decimate(P, None, P, P, 1, 4, 4, 0, None), "cell=0")
    refused(lib.pivlfn_flow_decimate(P, None, P, P, 1, 4, 4, -2, None), "cell=-2")
    with pytest.raises(ValueError):
        _lib.check(lib.pivlfn_flow_decimate(P, None, P, P, 1, 4, 4, 0, None), "decimate_flow")


def test_python_entries_refuse_bad_arguments_without_a_gpu():
    import torch
    from pivlfn import viz
    cpu32 = torch.zeros(1, 2, 4, 4)
    for fn in (viz.flow_to_color, viz.flow_maxrad, lambda f: viz.decimate_flow(f, 2), viz.vorticity_image):
        with pytest.raises(TypeError, match="float64"):
            fn(cpu32.double())
        with pytest.raises(TypeError, match="ndarray"):
            fn(np.zeros((1, 2, 4, 4), np.float32))
        with pytest.raises(NotImplementedError, match="GPU tensors only"):
            fn(cpu32)
    for kw, word in ((dict(scope="frame"), "scope"), (dict(wheel="hsv"), "wheel"), (dict(order="grb"), "order")):
        with pytest.raises(ValueError, match=word):
            viz.flow_to_color(cpu32, **kw)
    with pytest.raises(TypeError, match="int32"):
        viz.scalar_to_color(torch.zeros(1, 4, 4, dtype=torch.int32), -1, 1)
    with pytest.raises(NotImplementedError):
        viz.scalar_to_color(torch.zeros(1, 4, 4), -1, 1)
    for cell in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="cell"):
            viz.decimate_flow(cpu32, cell)
    for fn in (viz.motion_to_color, viz.quiver_plot):
        with pytest.raises(TypeError, match="float64"):
            fn(np.zeros((4, 5, 2)))
        with pytest.raises(ValueError, match="shape"):
            fn(np.zeros((4, 5, 3), np.float32))
    with pytest.raises(ValueError, match="maxmotion"):
        viz._maxmotion(float("nan"))
    with pytest.raises(ValueError, match="colour map"):
        viz._lut_on("jet", "cpu")
    with pytest.raises(TypeError, match="256 x 3"):
        viz._lut_on(np.zeros((255, 3), np.uint8), "cpu")
    assert viz.quiver_cell(1024, 1024) == 16 and viz.quiver_cell(64, 96) == 2 and viz.quiver_cell(5, 64) == 1 and viz.quiver_cell(1, 65) == 2


def test_src_utils_plot_alias_has_the_reference_signatures():
    import src.utils_plot as up
    names = [p.name for p in inspect.signature(up.motion_to_color).parameters.values()]
    assert names == ["flow", "maxmotion", "verbose", "original_color"]
    q = inspect.signature(up.quiver_plot).parameters
    assert list(q) == ["flow", "coord", "filename", "norm", "show", "cell"]
    assert [q[k].default for k in q][1:] == [None, None, False, False, None]
    for name in ("read_flow", "write_flow", "flowname_modifier"):
        assert hasattr(up, name)


def test_quiver_plot_says_when_matplotlib_is_missing(monkeypatch):
    from pivlfn import viz
    real = builtins.__import__

    def no_matplotlib(name, *a, **k):
        if name == "matplotlib" or name.startswith("matplotlib."):
            raise ImportError("No module named 'matplotlib'")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_matplotlib)
    with pytest.raises(ImportError, match="quiver plots need matplotlib"):
        viz.quiver_plot(np.zeros((4, 5, 2), np.float32), filename="x.png")


def test_write_png_and_png_writer_round_trip(tmp_path):
    import PIL.Image
    from pivlfn.viz import PngWriter, write_png
    rng = np.random.default_rng(1)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((1, 1), (5, 7), (64, 96))]
    write_png(str(tmp_path / "one.png"), imgs[1])
    assert np.array_equal(np.array(PIL.Image.open(tmp_path / "one.png")), imgs[1])
    with PngWriter(workers=2) as w:
        for k, im in enumerate(imgs):
            w.submit(im, str(tmp_path / f"w{k}.png"))
    for k, im in enumerate(imgs):
        got = PIL.Image.open(tmp_path / f"w{k}.png")
        assert got.mode == "RGB" and np.array_equal(np.array(got), im)
    with pytest.raises(TypeError, match="uint8"):
        write_png(str(tmp_path / "bad.png"), imgs[1].astype(np.float32))
    w = PngWriter(workers=2)
    w.submit(imgs[0], str(tmp_path / "ok.png"))
    w.submit(imgs[0], str(tmp_path / "no_such_dir" / "x.png"))
    with pytest.raises(OSError):
        w.close()
    assert (tmp_path / "ok.png").exists()


def test_run_py_picture_flags_parse_and_stay_out_of_args_txt(tmp_path, monkeypatch):
    import run as runpy
    plain = runpy.parser.parse_args(["-i", "x", "-o", "y"])
    assert (plain.color, plain.color_max, plain.color_wheel, plain.vort_image, plain.vort_max, plain.quiver) == \
        (False, None, None, False, None, None)
    keys = [ln.split(":")[0] for ln in runpy.args_lines(plain)]
    assert not set(keys) & set(runpy.VIZ_FLAGS)
    assert keys == sorted(k for k in vars(plain) if not k.startswith("validate") and
                          k not in runpy.PREP_FLAGS + runpy.TRUTH_FLAGS + runpy.VIZ_FLAGS)
    full = runpy.parser.parse_args(["-i", "x", "--color", "--color-max", "4", "--color-wheel", "original", "--vort-image", "--vort-max",
                                    "0.5", "--quiver", "8"])
    assert (full.color, full.color_max, full.color_wheel, full.vort_image, full.vort_max, full.quiver) == \
        (True, 4.0, "original", True, 0.5, 8)
    assert runpy.parser.parse_args(["--quiver"]).quiver == 0
    lines = runpy.args_lines(full)
    assert "color: True\n" in lines and "color_max: 4.0\n" in lines and "quiver: 8\n" in lines
    assert "comparable" in runpy.parser.format_help()
    base = ["--model", "piv", "-i", str(tmp_path), "-o", str(tmp_path / "out")]
    for extra, word in ((["--color", "-b", "1.2"], "-b/-c"), (["--color-max", "3"], "need --color"), (["--color-wheel", "interp"], "need --color"),
                        (["--vort-max", "2"], "needs --vort-image"), (["--color", "--color-max", "0"], "positive"),
                        (["--vort-image", "--vort-max", "nan"], "positive"), (["--quiver", "-4"], "cell")):
        with pytest.raises(SystemExit, match=word):
            runpy.main(base + extra)
    real = builtins.__import__

    def no_matplotlib(name, *a, **k):
        if name == "matplotlib" or name.startswith("matplotlib."):
            raise ImportError("No module named 'matplotlib'")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_matplotlib)
    with pytest.raises(SystemExit, match="--quiver: quiver plots need matplotlib"):
        runpy.main(base + ["--quiver"])
    assert not (tmp_path / "out").exists()


def test_stream_pairs_hands_extras_to_the_sink():
    """The host logic of the extras path, on the CPU with a stand-in estimate."""
    import torch
    from pivlfn.pipeline import stream_pairs

    class Loader:
        def __iter__(self):
            for k in range(3):
                n = 2 if k < 2 else 1
                yield [f"p{2 * k + i}" for i in range(n)], torch.full((n, 4, 6, 3), k, dtype=torch.uint8), torch.zeros((n, 4, 6, 3), dtype=torch.uint8)

    state = {}

    def est(net, a, b, tensor=True):
        state["pic"] = (a[:, 0, :, :, None] * 255).to(torch.uint8).expand(-1, -1, -1, 3)
        return a[:, :2] * 255

    got = []
    n = stream_pairs(None, Loader(), torch.device("cpu"), lambda flow, name, extras=None: got.append((name, flow.copy(), extras)),
                     estimate_fn=est, extras=lambda: {"color": state["pic"]})
    assert n == 5 and [g[0] for g in got] == [f"p{k}" for k in range(5)]
    for k, (name, flow, extras) in enumerate(got):
        assert set(extras) == {"color"} and extras["color"].shape == (4, 6, 3) and (extras["color"] == k // 2).all()
        assert flow.shape == (4, 6, 2) and (flow == k // 2).all()
    with pytest.raises(ValueError, match="extras"):
        stream_pairs(None, Loader(), torch.device("cpu"), lambda *a, **k: None, estimate_fn=est, extras=lambda: {}, mods=[(1.0, 1.0)])
