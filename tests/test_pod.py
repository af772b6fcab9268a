"""CPU: the snapshot POD restatement against numpy.linalg.svd on the planted case, the host half of pivlfn.pod (sign rule,
reconstruct, every refusal), the ERR_ARG paths of the two entry points through ctypes, and run.py's refusals.  No GPU."""
import numpy as np
import pytest

import pod_restatement as pr


@pytest.fixture(scope="module")
def planted():
    flows = pr.planted_flows()
    X = flows.reshape(pr.PLANTED_N, -1)
    return flows, X, pr.decompose(X, 3, (2, pr.PLANTED_H, pr.PLANTED_W)), pr.svd_reference(X, 3)


def test_planted_case_is_what_it_claims(planted):
    flows, X, res, _ = planted
    assert flows.shape == (37, 2, 9, 13) and flows.dtype == np.float32 and X.shape == (37, 234)
    lam = res["eigenvalues"]
    print("ratios", lam[1] / lam[0], lam[2] / lam[0], lam[3] / lam[0], "fractions", res["fraction"])
    assert abs(lam[1] / lam[0] - 0.25) < 0.005 and abs(lam[2] / lam[0] - 0.040) < 0.002
    assert 1e-7 < lam[3] / lam[0] < 1e-5                         # the noise floor, far from the third structure
    assert np.allclose(res["fraction"], [0.775, 0.194, 0.031], atol=0.002)
    assert np.allclose(res["energy"], lam[:3] / 37)
    assert abs(np.abs(res["mean"][0]).mean() - 0.8) < 0.01 and abs(np.abs(res["mean"][1]).mean() - 0.3) < 0.01


def test_restatement_agrees_with_the_svd(planted):
    _, X, res, (lam_svd, modes_svd, coeff_svd) = planted
    lam = res["eigenvalues"]
    l1 = lam[0]
    err_lam = np.abs(lam[:36] - lam_svd[:36]).max() / l1
    modes = res["modes"].reshape(3, -1)
    # the SVD's signs are arbitrary: bring both to the sign of the coefficient column's largest entry
    s = np.sign(np.sum(res["coeff"] * coeff_svd, axis=0))
    err_modes = np.abs(modes - s[:, None] * modes_svd).max()
    err_coeff = np.abs(res["coeff"] - s[None, :] * coeff_svd).max() / np.sqrt(l1)
    err_orth = np.abs(modes @ modes.T - np.eye(3)).max()
    print("vs svd: eigenvalues", err_lam, "modes", err_modes, "coeff", err_coeff, "orthonormality", err_orth)
    assert err_lam < 1e-12 and err_modes < 1e-12 and err_coeff < 1e-12 and err_orth < 1e-12
    assert abs(lam[36]) / l1 < 1e-12                              # centring leaves n - 1 directions


def test_sign_rule_and_reconstruct(planted):
    from pivlfn.pod import PODResult, solve_gram
    flows, X, res, _ = planted
    lam, V, Wt = solve_gram(res["gram"], 3)
    lam_r, V_r, Wt_r = pr.solve(res["gram"], 3)
    assert np.allclose(lam, lam_r, rtol=0, atol=1e-12 * lam[0]) and np.allclose(V, V_r, atol=1e-12) and np.allclose(Wt, Wt_r, atol=1e-12)
    for k in range(3):
        big = np.flatnonzero(np.abs(V[:, k]) == np.abs(V[:, k]).max())[0]
        assert V[big, k] > 0
    assert np.array_equal(Wt[:, 3], np.ones(37))
    from pivlfn.pod import sign_rule
    tie = np.array([[-0.5, 0.5, 0.1], [0.5, -0.5, -0.7], [0.5, 0.5, 0.7], [-0.5, 0.5, 0.0]])    # a tie goes to the first such entry
    assert np.array_equal(sign_rule(tie), tie * np.array([-1.0, 1.0, -1.0]))
    assert np.array_equal(pr.sign_rule(tie.T).T, sign_rule(tie))
    out = pr.project(X, Wt)
    r = PODResult(modes=out[:3].reshape(3, 2, 9, 13), mean=(out[3] / 37).reshape(2, 9, 13), coeff=V * np.sqrt(lam[:3]),
                  energy=lam[:3] / 37, fraction=lam[:3] / lam.sum(), eigenvalues=lam, gram=res["gram"], cell=1, H=9, W=13)
    rms = np.sqrt(np.mean([(r.reconstruct(i, 3) - flows[i].astype(np.float64)) ** 2 for i in range(37)]))
    print("rank-3 reconstruction rms", rms)
    assert 0.0085 < rms < 0.0100                                  # the noise of sigma 0.01 less what 4 of 37 directions absorb
    assert np.array_equal(r.reconstruct(5), r.reconstruct(5, 3)) and np.array_equal(r.reconstruct(5, 0), r.mean)
    assert np.allclose(r.reconstruct(5, 2), r.mean + r.coeff[5, 0] * r.modes[0] + r.coeff[5, 1] * r.modes[1], atol=1e-15)
    rms2 = np.sqrt(np.mean([(r.reconstruct(i, 2) - flows[i].astype(np.float64)) ** 2 for i in range(37)]))
    assert 0.25 < rms2 < 0.35                                     # without the third structure: 0.6 / sqrt 2 / sqrt 2
    with pytest.raises(ValueError):
        r.reconstruct(0, 4)
    with pytest.raises(IndexError):
        r.reconstruct(37, 1)


def test_result_saves_every_field(planted, tmp_path):
    from pivlfn.pod import PODResult
    _, _, res, _ = planted
    r = PODResult(cell=2, H=18, W=26, **res)
    z = np.load(r.save(str(tmp_path / "pod.npz")))
    assert sorted(z.files) == sorted(["modes", "mean", "coeff", "energy", "fraction", "eigenvalues", "gram", "cell", "H", "W"])
    for k in res:
        assert np.array_equal(z[k], res[k])
    assert (int(z["cell"]), int(z["H"]), int(z["W"])) == (2, 18, 26)


def test_host_side_refusals():
    from pivlfn.pod import FlowPOD, check_solve, solve_gram
    for cap in (1, 0, -3, 4097, 2.0, True):
        with pytest.raises(ValueError, match="capacity"):
            FlowPOD(8, 8, cap)                                    # before any device is touched
    with pytest.raises(ValueError, match="cell"):
        FlowPOD(8, 8, 4, cell=0)
    assert check_solve(37, 3, 0) == 3 and check_solve(2, 1, 0) == 1 and check_solve(100, 64, 0) == 64
    for n, K in ((37, 0), (37, 37), (37, 65), (100, 65), (3, 3), (37, 2.0), (37, True)):
        with pytest.raises(ValueError, match="modes"):
            check_solve(n, K, 0)
    for n in (0, 1):
        with pytest.raises(ValueError, match="at least 2"):
            check_solve(n, 1, 0)
    with pytest.raises(ValueError, match=r"--validate replace.*larger cell"):
        check_solve(37, 3, 5)
    same = np.tile(np.linspace(-1, 1, 50, dtype=np.float32), (6, 1))        # n identical snapshots: no fluctuation at all
    with pytest.raises(ValueError, match="mode 1 is undefined"):
        solve_gram(pr.gram(same), 1)
    with pytest.raises(ValueError, match="undefined"):
        pr.solve(pr.gram(same), 1)
    two = same.copy()
    two[0, 0] += 1.0                                              # one direction only: mode 1 exists, mode 2 does not
    solve_gram(pr.gram(two), 1)
    with pytest.raises(ValueError, match="mode 2 is undefined"):
        solve_gram(pr.gram(two), 2)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from pivlfn import _lib
    lib = _lib.load()
    A = 4096                       # a non-null, 8-byte aligned pointer that is never dereferenced: every case fails its checks first
    big = 1 << 40

    def refused(rc, *words):
        msg = lib.pivlfn_last_error().decode()
        assert rc == 1, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    q = lib.pivlfn_snapshot_gram_workspace_bytes
    assert q(37, 234) > 0 and q(4096, 2 * 1024 * 1024) > 0 and q(1, 1) > 0
    assert q(0, 10) == 0 and q(4097, 10) == 0 and q(4, 0) == 0 and q(4, 1 << 31) == 0
    slab = 2048                                                  # PIVLFN_GRAM_SLAB
    assert q(65, 2 * slab + 6) >= 3 * 3 * 64 * 64 * 8            # three slab sums of three 64 x 64 blocks pass through the workspace
    gram = lib.pivlfn_snapshot_gram
    refused(gram(None, 4, 10, 10, A, A, big, None), "snapshot_gram", "null")
    refused(gram(A, 4, 10, 10, None, A, big, None), "null")
    refused(gram(A, 4, 10, 10, A, None, big, None), "null")
    refused(gram(A, 0, 10, 10, A, A, big, None), "n=0")
    refused(gram(A, 4097, 10, 10, A, A, big, None), "n=4097", "4096")
    refused(gram(A, 4, 0, 10, A, A, big, None), "P=0")
    refused(gram(A, 4, 1 << 31, 1 << 31, A, A, big, None), "P=2147483648")
    refused(gram(A, 4, 10, 9, A, A, big, None), "ldx=9")
    refused(gram(A, 4, 10, 10, A, A + 4, big, None), "8-byte aligned")
    refused(gram(A, 65, 2 * slab + 6, 2 * slab + 6, A, A, q(65, 2 * slab + 6) - 1, None), "too small")
    refused(gram(A, 4, 10, 10, A, A, q(4, 10) - 1, None), "too small")
    proj = lib.pivlfn_snapshot_project
    refused(proj(None, 4, 10, 10, A, 2, A, None), "snapshot_project", "null")
    refused(proj(A, 4, 10, 10, None, 2, A, None), "null")
    refused(proj(A, 4, 10, 10, A, 2, None, None), "null")
    refused(proj(A, 0, 10, 10, A, 2, A, None), "n=0")
    refused(proj(A, 4097, 10, 10, A, 2, A, None), "n=4097")
    refused(proj(A, 4, 0, 10, A, 2, A, None), "P=0")
    refused(proj(A, 4, 1 << 31, 1 << 31, A, 2, A, None), "P=2147483648")
    refused(proj(A, 4, 10, 9, A, 2, A, None), "ldx=9")
    refused(proj(A, 4, 10, 10, A, 0, A, None), "K=0")
    refused(proj(A, 4, 10, 10, A, 65, A, None), "K=65")
    with pytest.raises(ValueError):
        _lib.check(proj(A, 4, 10, 10, A, 65, A, None), "snapshot_project")


def test_header_constants_match_the_package():
    import os
    import re
    from pivlfn import pod
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pivlfn.h")).read()
    assert int(re.search(r"#define PIVLFN_POD_MAX_SNAPSHOTS\s+(\d+)", text).group(1)) == pod.MAX_SNAPSHOTS == 4096
    assert int(re.search(r"#define PIVLFN_GRAM_SLAB\s+(\d+)", text).group(1)) == 2048


def test_run_py_refusals(tmp_path, monkeypatch):
    import run as runpy
    base = ["--model", "piv", "-i", str(tmp_path), "-o", str(tmp_path / "out")]
    for k in ("0", "65", "-1"):
        with pytest.raises(SystemExit, match="1..64"):
            runpy.main(base + ["--pod", k])
    with pytest.raises(SystemExit, match="--pod-cell needs --pod"):
        runpy.main(base + ["--pod-cell", "4"])
    with pytest.raises(SystemExit, match="cell must be"):
        runpy.main(base + ["--pod", "2", "--pod-cell", "0"])
    for extra in (["-b", "1.2"], ["-c", "0.8"]):
        with pytest.raises(SystemExit, match="-b/-c"):
            runpy.main(base + ["--pod", "2"] + extra)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="single process"):
        runpy.main(base + ["--pod", "2"])
    assert not (tmp_path / "out").exists()


def test_args_txt_lists_the_pod_flags_only_when_used():
    import run as runpy
    a = runpy.parser.parse_args(["--model", "piv", "-i", "x"])
    assert not any(line.startswith("pod") for line in runpy.args_lines(a))
    a = runpy.parser.parse_args(["--model", "piv", "-i", "x", "--pod", "2", "--pod-cell", "8"])
    lines = runpy.args_lines(a)
    assert "pod: 2\n" in lines and "pod_cell: 8\n" in lines
