"""CPU: the stereo 2D3C contract against the reference's fixture, and the host side of pivlfn.stereo / stereo_run.py."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from stereo_restatement import load_case, restate, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def stereo_gold():
    return np.load(os.path.join(GOLD, "stereo_cases.npz"))


def test_fixture_covers_the_cases(stereo_gold):
    tags = list(stereo_gold["cases"])
    assert len(tags) >= 5
    outs = [stereo_gold[f"{t}_out"] for t in tags]
    assert any(np.isnan(o).any() for o in outs) and any(np.isinf(o).any() for o in outs)
    assert {int(stereo_gold[f"{t}_fps"]) for t in tags} == {1, 15}
    assert all(o.shape[0] % 2 and o.shape[1] % 2 for o in outs)
    assert max(np.abs(stereo_gold[f"{t}_left"]).max() for t in tags) >= 49.0
    rep = json.load(open(os.path.join(GOLD, "pin_report_stereo.json")))
    assert rep["numpy"].split(".")[0] == "2" and len(rep["reference_sha256"]) == 3


def test_restatement_equals_reference_bit_for_bit(stereo_gold):
    from pivlfn import stereo
    for tag in stereo_gold["cases"]:
        left, right, coeff, th, al, fps, calib = load_case(stereo_gold, tag)
        theta, beta = stereo.angles(th, al)
        s = stereo.scale_factor(coeff, calib)
        got = restate(left, right, stereo.coeff_f32(coeff), stereo.tangents(theta, beta), None if s is None else (s, fps))
        assert same_bits(got, stereo_gold[f"{tag}_out"]), tag


def test_read_coeff_good_and_malformed(tmp_path):
    from pivlfn.stereo import read_coeff
    good = {"Left": list(range(24)), "Right": [0.5] * 24, "calib": 0.01}
    p = tmp_path / "c.json"
    p.write_text(json.dumps(good))
    c = read_coeff(str(p))
    assert c["Left"] == [float(v) for v in range(24)] and c["Right"] == [0.5] * 24 and c["calib"] == 0.01
    good.pop("calib")
    p.write_text(json.dumps(good))
    assert "calib" not in read_coeff(str(p))
    bad = [("{not json", "JSON"), (json.dumps([1, 2]), "object"), (json.dumps({"Left": [1.0] * 24}), "Right"),
           (json.dumps({"Left": [1.0] * 23, "Right": [1.0] * 24}), "24"),
           (json.dumps({"Left": [1.0] * 23 + ["x"], "Right": [1.0] * 24}), "Left\\[23\\]"),
           (json.dumps({"Left": [1.0] * 24, "Right": [1.0] * 23 + [True]}), "Right\\[23\\]"),
           (json.dumps({"Left": [1.0] * 24, "Right": [1.0] * 24, "calib": 0}), "calib"),
           (json.dumps({"Left": [1.0] * 24, "Right": [1.0] * 24, "calib": "a"}), "calib")]
    for text, what in bad:
        p.write_text(text)
        with pytest.raises(ValueError, match=what):
            read_coeff(str(p))
    with pytest.raises(ValueError, match="no such file"):
        read_coeff(str(tmp_path / "missing.json"))


def test_angles_broadcast_and_signs():
    from pivlfn.stereo import angles, tangents
    theta, beta = angles([30.0], [5.0])
    assert theta == [-np.deg2rad(30.0), np.deg2rad(30.0)] and beta == [-np.deg2rad(5.0), np.deg2rad(5.0)]
    theta, beta = angles(45, [2.0, -3.0])
    assert theta[0] < 0 < theta[1] and beta == [-np.deg2rad(2.0), np.deg2rad(-3.0)]
    assert all(isinstance(t, np.float64) for t in theta + beta)
    t = tangents(*angles([30.0, 40.0], [5.0]))
    assert t.dtype == np.float64 and t[0] == np.tan(-np.deg2rad(30.0)) and t[1] == np.tan(np.deg2rad(40.0))
    with pytest.raises(ValueError):
        angles([1.0, 2.0, 3.0], [0.0])


def test_scale_factor_follows_the_reference_rule():
    from pivlfn.stereo import scale_factor
    assert scale_factor({"calib": 0.002}, 0.05) == 0.05 / 0.002
    assert scale_factor({"calib": 0.002}, None) is None
    assert scale_factor({"calib": 0.002}, 0.0) is None          # `if args.calib` is falsy
    assert scale_factor({}, 0.05) is None                        # no calibration point in the file: no scaling


def _frames(d, names):
    d.mkdir(parents=True, exist_ok=True)
    for n in names:
        (d / n).write_bytes(b"")


def test_stereo_folder_listing(tmp_path):
    from pivlfn.stereo import StereoSequence, stereo_folders
    root = tmp_path / "set"
    _frames(root / "Left", [f"{k:04d}-L.png" for k in range(4)])
    _frames(root / "RIGHT", [f"{k:04d}-R.png" for k in range(4)])
    (root / "calib").mkdir()
    assert stereo_folders(str(root)) == (str(root / "Left"), str(root / "RIGHT"))
    seq = StereoSequence(str(root))
    assert seq.steps == 3 and len(seq.image_list) == 6
    assert seq.image_list[0] == [str(root / "Left" / "0000-L.png"), str(root / "Left" / "0001-L.png")]
    assert seq.image_list[1] == [str(root / "RIGHT" / "0000-R.png"), str(root / "RIGHT" / "0001-R.png")]
    assert seq.name_list[:4] == ["0000-L", "0000-R", "0001-L", "0001-R"]
    assert seq.direct_names() == ["0000-L_2d3c.flo", "0001-L_2d3c.flo", "0002-L_2d3c.flo"]
    assert seq.camera("right").image_list == seq.image_list[1::2]
    _frames(root / "RIGHT", ["0004-R.png"])
    with pytest.raises(ValueError, match="4 left frames but 5 right"):
        StereoSequence(str(root))
    other = tmp_path / "other"
    _frames(other / "cam0", ["a.png"])
    _frames(other / "cam1", ["a.png"])
    with pytest.raises(ValueError, match="'left'"):
        stereo_folders(str(other))
    _frames(other / "left", ["a.png"])
    _frames(other / "LEFT", ["a.png"])
    _frames(other / "right", ["a.png"])
    with pytest.raises(ValueError, match="exactly one 'left'"):
        stereo_folders(str(other))


@pytest.mark.parametrize("steps_per_batch", [1, 2, 3])
def test_interleaved_stream_decodes_each_frame_once_and_groups_outputs(tmp_path, steps_per_batch):
    """PairLoader(share=2) over the interleaved left / right pair list, stream_pairs(group=2) with a CPU stand-in for the
    stereo estimate: every frame is decoded once, one output per step, named after the step's left pair."""
    import PIL.Image
    from pivlfn.pipeline import PairLoader, stream_pairs
    from pivlfn.stereo import StereoSequence
    rng = np.random.default_rng(0)
    root = tmp_path / "set"
    for side, tag in (("left", "L"), ("right", "R")):
        (root / side).mkdir(parents=True)
        for k in range(5):
            PIL.Image.fromarray(rng.integers(0, 256, (6, 10), dtype=np.uint8)).save(str(root / side / f"{k:04d}-{tag}.png"))
    seq = StereoSequence(str(root))

    def fake(net, a, b, tensor=True):            # [2n,3,H,W] x2 interleaved -> [n,H,W,3]: left u, right u, their difference
        ul, ur = (b - a)[0::2].mean(1), (b - a)[1::2].mean(1)
        return torch.stack([ul, ur, ur - ul], dim=-1)

    loader = PairLoader(seq, 0, len(seq.image_list), 2 * steps_per_batch, share=2)
    seen = []
    n = stream_pairs(None, loader, torch.device("cpu"), lambda f, name: seen.append((name, f.copy())), estimate_fn=fake, group=2)
    loader.close()
    assert n == 4 and loader.decoded == 10
    assert [s[0] for s in seen] == [f"{k:04d}-L" for k in range(4)]
    from pivlfn.datasets import read_image
    for k, (_, f) in enumerate(seen):
        want_l = (read_image(seq.left[k + 1]) - read_image(seq.left[k])).mean(0)
        want_r = (read_image(seq.right[k + 1]) - read_image(seq.right[k])).mean(0)
        assert f.shape == (6, 10, 3)
        np.testing.assert_array_equal(f[..., 0], want_l.numpy())
        np.testing.assert_array_equal(f[..., 1], want_r.numpy())


def test_direct_mode_name_collisions_are_refused(tmp_path):
    from pivlfn.stereo import StereoSequence
    root = tmp_path / "set"
    _frames(root / "left", ["run_1.png", "run_2.png", "run_3.png"])
    _frames(root / "right", ["r_1.png", "r_2.png", "r_3.png"])
    with pytest.raises(ValueError, match="run_2d3c.flo"):
        StereoSequence(str(root)).direct_names()


def _flo(path):
    from pivlfn.flo import write_flow
    path.parent.mkdir(parents=True, exist_ok=True)
    write_flow(np.zeros((3, 5, 2), np.float32), str(path))


def test_flo_mode_pairing_and_names(tmp_path):
    from pivlfn.stereo import flo_pairs
    save = tmp_path / "flow"
    for k in range(3):
        _flo(save / "left" / f"{k:04d}-L_out.flo")
        _flo(save / "right" / f"{k:04d}-R_out.flo")
    got = flo_pairs(str(save))
    assert [tuple(os.path.relpath(p, save) for p in t) for t in got] == [
        (f"left/{k:04d}-L_out.flo", f"right/{k:04d}-R_out.flo", f"stereo/{k:04d}-S_out.flo") for k in range(3)]


def test_flo_mode_checks_every_right_file_before_computing(tmp_path):
    """stereo_run.py's flo mode on a tree with a missing right flow stops in the pairing step, before the GPU is needed."""
    import stereo_run
    save = tmp_path / "flow"
    for k in range(3):
        _flo(save / "left" / f"{k:04d}-L_out.flo")
    _flo(save / "right" / "0000-R_out.flo")
    coeff = tmp_path / "c.json"
    coeff.write_text(json.dumps({"Left": [1.0] * 24, "Right": [1.0] * 24}))
    with pytest.raises(FileNotFoundError) as e:
        stereo_run.main(["--coeff", str(coeff), "--save", str(save)])
    assert "0001-R_out.flo" in str(e.value) and "0002-R_out.flo" in str(e.value)
    assert not (save / "stereo").exists()


def test_stereo_run_flags():
    import stereo_run
    a = stereo_run.parser.parse_args(["-c", "c.json", "-r", "R", "-s", "S", "--theta", "30", "40", "--alpha", "5",
                                      "-ws", "1", "1", "--fps", "15", "--calib", "0.05", "--model", "m.pt",
                                      "--model-version", "2", "--inference-mode", "direct", "--batch", "3"])
    assert (a.coeff, a.root, a.save, a.theta, a.alpha, a.fps, a.calib, a.model_version, a.inference_mode, a.batch) == \
        ("c.json", "R", "S", [30.0, 40.0], [5.0], 15, 0.05, 2, "direct", 3)
    d = stereo_run.parser.parse_args([])
    assert (d.root, d.save, d.theta, d.alpha, d.inference_mode, d.model_version, d.batch) == \
        (None, "./work", [45.0, 45.0], [0.0, 0.0], "manual", 1, 2)


def test_header_declares_stereo_and_null_arguments_are_rejected():
    text = open(os.path.join(ROOT, "include", "pivlfn.h")).read()
    assert re.search(r"\bint\s+pivlfn_stereo_2d3c\s*\(", text)
    from pivlfn import _lib
    lib = _lib.load()
    assert lib.pivlfn_abi_version() == 3
    c = (ctypes.c_float * 48)()
    t = (ctypes.c_double * 4)(-1.0, 1.0, 0.0, 0.0)
    assert lib.pivlfn_stereo_2d3c(None, None, 1, 4, 4, 4, 4, None, c, None, t, None) != 0
    assert b"null" in lib.pivlfn_last_error()
    dummy = ctypes.c_void_p(16)          # never dereferenced: every check below fails on the host first
    assert lib.pivlfn_stereo_2d3c(dummy, dummy, 1, 4, 4, 4, 4, None, None, None, t, None) != 0
    assert lib.pivlfn_stereo_2d3c(dummy, dummy, 0, 4, 4, 4, 4, None, c, None, t, None) != 0
    assert b"shape" in lib.pivlfn_last_error()
    same = (ctypes.c_double * 4)(0.5, 0.5, 0.0, 0.0)
    assert lib.pivlfn_stereo_2d3c(dummy, dummy, 1, 4, 4, 4, 4, None, c, None, same, None) != 0
    assert b"tan(theta_L) == tan(theta_R)" in lib.pivlfn_last_error()
    with pytest.raises(ValueError):
        _lib.check(lib.pivlfn_stereo_2d3c(dummy, dummy, 1, 4, 4, 4, 4, None, c, None, same, None), "stereo")


def test_stereo_is_gpu_only():
    from pivlfn import stereo
    import pivlfn
    f = torch.zeros(2, 2, 4, 4)
    coeff = {"Left": [1.0] * 24, "Right": [1.0] * 24}
    with pytest.raises(NotImplementedError):
        stereo.stereo_2d3c(f, coeff, [-1.0, 1.0, 0.0, 0.0])
    net = pivlfn.piv_liteflownet().eval()
    img = torch.zeros(1, 3, 32, 32)
    with pytest.raises(NotImplementedError):
        pivlfn.estimate_stereo(net, img, img, img, img, coeff, 30.0, 0.0)
