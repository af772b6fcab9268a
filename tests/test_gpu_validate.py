"""GPU: pivlfn_flow_validate (csrc/validate.hip) and pivlfn_flow_stats_accumulate_masked (csrc/postpro.hip), validate_flow,
MaskedFlowStats and run.py --validate -- against the numpy restatement of tests/validate_restatement.py, bit for bit: flags,
residuals and flows.  No tolerance appears anywhere."""
import json
import os

import numpy as np
import pytest
import torch

import analysis_plans as ap
import pivlfn
import validate_restatement as vr
from guarded import check_guards, guarded, holds
from pivlfn import _lib, postpro, synth
from pivlfn import validate as V
from pivlfn.flo import read_flow
from postpro_restatement import same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MODES = ("flag", "mask", "replace")
RADII, SPACINGS = (1, 2), (1, 3, 8)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _check_against_restatement(dev, flows, what, configs=None, expect=None):
    """Every radius x spacing x mode x residual on/off against the restatement (pass 1 restated once per radius and spacing)."""
    flows = np.ascontiguousarray(flows, dtype=np.float32)
    t = torch.from_numpy(flows).to(dev)
    for r, s in (configs or [(r, s) for r in RADII for s in SPACINGS]):
        det = [vr.detect(f, r, s) for f in flows]
        flag1 = np.stack([d[0] for d in det])
        resid = np.stack([d[1] for d in det])
        for mode in MODES:
            pass2 = [vr.apply(f, g, r, s, mode) for f, g in zip(flows, flag1)]
            want_flag = np.stack([p[1] for p in pass2])
            for with_resid in (False, True):
                got = V.validate_flow(t, r, s, mode=mode, residual=with_resid)
                tag = (what, r, s, mode, with_resid)
                assert np.array_equal(got.flag.cpu().numpy(), want_flag), tag
                if mode == "flag":
                    assert got.flow is t, tag
                else:
                    assert got.flow is not t and vr.same_bits32(got.flow.cpu().numpy(), np.stack([p[0] for p in pass2])), tag
                if with_resid:
                    assert vr.same_bits32(got.residual.cpu().numpy(), resid), tag
                else:
                    assert got.residual is None
        if expect is not None:
            expect(r, s, flag1, want_flag)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (5, 3)])
def test_small_images_match_restatement(dev, H, W):
    rng = np.random.default_rng(100 * H + W)

    def expect(r, s, flag1, flag2):
        if s >= max(H, W):                      # a spacing beyond the image: no pixel has a neighbour, nothing is flagged
            assert not flag2.any()
    _check_against_restatement(dev, rng.normal(0, 6, (2, 2, H, W)), f"{H}x{W}", expect=expect)


def test_noise_batch_matches_restatement(dev):
    """37 x 53, B = 5, Gaussian sigma = 6 px: many flags, many flagged pixels whose neighbours are flagged too."""
    rng = np.random.default_rng(37)

    def expect(r, s, flag1, flag2):
        assert 0.1 < (flag1 != 0).mean() < 0.9
        if r == 1:
            assert (flag2 & vr.NOT_REPLACED).any()       # with 8 neighbours some outliers have only outliers around them
    _check_against_restatement(dev, rng.normal(0, 6, (5, 2, 37, 53)), "noise", expect=expect)


def test_non_finite_and_signed_zero_inputs_match_restatement(dev):
    """64 x 64 with NaN, +-inf, 1e10 and -0.0 sprinkled in, a fully unknown 5 x 5 block (NOT_REPLACED occurs) and a patch of zeros
    of both signs."""
    rng = np.random.default_rng(64)
    f = rng.normal(0, 2, (1, 2, 64, 64)).astype(np.float32)
    vals = [np.nan, np.inf, -np.inf, 1e10, -0.0]
    for k, (y, x) in enumerate(rng.integers(0, 64, (60, 2))):
        f[0, k % 2, y, x] = vals[k % 5]
    f[0, :, 20:25, 30:35] = np.nan
    f[0, 0, 40:44, 40:44] = -0.0
    f[0, 1, 40:44, 40:44] = 0.0

    def expect(r, s, flag1, flag2):
        assert (flag1 & vr.UNKNOWN).sum() >= 25 + 30
        if s == 1:
            assert flag2[0, 22, 32] == (vr.UNKNOWN | vr.NOT_REPLACED)
    _check_against_restatement(dev, f, "special", expect=expect)
    # what is copied is copied bit for bit: the NaN payloads and the signs of zero of unflagged or unreplaceable pixels
    t = torch.from_numpy(f).to(dev)
    got = V.validate_flow(t, mode="replace")
    keep = (got.flag == 0) | ((got.flag & V.NOT_REPLACED) != 0)
    assert torch.equal(_bits(got.flow)[:, 0][keep], _bits(t)[:, 0][keep])


def _dns_planted(radius):
    f = np.ascontiguousarray(read_flow(os.path.join(GOLD, "DNS_turbulence_out.flo")).transpose(2, 0, 1))
    return vr.plant(f, 50, 2 * radius + 1, 3)


@pytest.mark.parametrize("radius", RADII)
def test_reference_network_output_with_planted_spikes(dev, radius):
    """The reference's own network output (256 x 256) with the 50 planted vectors of tests/test_validate.py: equal to the restatement
    at every spacing, and at spacing 1 exactly the 50 are flagged."""
    spiked, planted = _dns_planted(radius)

    def expect(r, s, flag1, flag2):
        if s == 1:
            assert np.array_equal(flag2[0] != 0, planted) and int(planted.sum()) == 50
    _check_against_restatement(dev, spiked[None], "dns", configs=[(radius, s) for s in SPACINGS], expect=expect)


def test_megapixel_estimate_output_and_batch_invariance(dev):
    """1024 x 1024, B = 3: a real estimate() output of the seeded network with planted spikes (twice, different spikes) and a noise
    frame.  Pass 1 against the restatement on every 41st row; pass 2 in full against the restatement's pass 2 run on the flags the
    GPU returned; and the batch against its frames one at a time, everything bit for bit."""
    S = 1024
    net = pivlfn.piv_liteflownet(synth.generate_weights("piv", 0)).to(dev).eval()
    a, b = synth.particle_batch(1, S, S, seed=5)
    est = pivlfn.estimate(net, torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), tensor=True)[0].cpu().numpy()
    assert np.abs(est).max() > 0.5
    rng = np.random.default_rng(1024)
    flows = np.stack([vr.plant(est, 300, 5, 11)[0], vr.plant(est, 300, 5, 12)[0], rng.normal(0, 6, (2, S, S)).astype(np.float32)])
    t = torch.from_numpy(flows).to(dev)
    rows = range(0, S, 41)
    for r, s in ((1, 1), (2, 1), (1, 3), (2, 8)):
        res = {m: V.validate_flow(t, r, s, mode=m, residual=True) for m in MODES}
        flag1 = res["flag"].flag.cpu().numpy()
        resid = res["flag"].residual.cpu().numpy()
        for k in (0, 2) if (r, s) == (1, 1) else (1,):
            want_flag, want_resid = vr.detect(flows[k], r, s, rows=rows)
            assert np.array_equal(flag1[k][rows], want_flag[rows]), (r, s, k)
            assert vr.same_bits32(resid[k][:, rows], want_resid[:, rows]), (r, s, k)
        assert np.array_equal(res["mask"].flag.cpu().numpy(), flag1)
        for k in (0, 1) if (r, s) == (1, 1) else (0,):    # pass 2 of the estimate frames (the noise frame: in the batch check)
            for m in ("mask", "replace"):
                want_out, want_flag2 = vr.apply(flows[k], flag1[k], r, s, m)
                assert vr.same_bits32(res[m].flow[k].cpu().numpy(), want_out), (r, s, k, m)
                assert np.array_equal(res[m].flag[k].cpu().numpy(), want_flag2), (r, s, k, m)
        for m in MODES:
            for k in range(3):
                one = V.validate_flow(t[k:k + 1], r, s, mode=m, residual=True)
                assert torch.equal(one.flag[0], res[m].flag[k]), (r, s, m, k)
                assert torch.equal(_bits(one.residual[0]), _bits(res[m].residual[k])), (r, s, m, k)
                if m != "flag":
                    assert torch.equal(_bits(one.flow[0]), _bits(res[m].flow[k])), (r, s, m, k)
    empty = V.validate_flow(t[:0], residual=True)
    assert empty.flow.shape == (0, 2, S, S) and empty.flag.shape == (0, S, S) and empty.flag.dtype == torch.uint8
    assert empty.residual.shape == (0, 2, S, S)


@pytest.mark.parametrize("B,H,W", ap.shapes(ap.VALIDATE_CASES))
def test_bits_where_the_frame_grid_is_capped(dev, B, H, W):
    """More blocks a frame than the cap of both launches (detect and replace), so their grid-stride loops come round: a smooth flow
    with planted outliers in every frame gives the bits of the same frames in calls that are not capped."""
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([np.sin(xx / 17.0) + 0.01 * yy, np.cos(yy / 13.0) - 0.01 * xx]).astype(np.float32)
    frames, planted = zip(*(vr.plant(base, 20, 3, 1000 + b) for b in range(B)))
    t = torch.from_numpy(np.stack(frames)).to(dev)
    whole = V.validate_flow(t, 1, 1, mode="replace", residual=True)
    flagged = whole.flag.cpu().numpy() != 0
    assert np.array_equal(flagged, np.stack(planted)) and not torch.equal(_bits(whole.flow), _bits(t))
    step = ap.FRAMES_PER_UNCAPPED_CALL
    parts = [V.validate_flow(t[k:k + step], 1, 1, mode="replace", residual=True) for k in range(0, B, step)]
    assert torch.equal(whole.flag, torch.cat([p.flag for p in parts]))
    assert torch.equal(_bits(whole.flow), _bits(torch.cat([p.flow for p in parts])))
    assert torch.equal(_bits(whole.residual), _bits(torch.cat([p.residual for p in parts])))


@pytest.mark.parametrize("B,H,W", ap.shapes(ap.ACCUMULATOR_CASES))
def test_masked_stats_where_the_grid_is_capped(dev, B, H, W):
    """More blocks than the flat cap of the masked accumulator's launch: the restatement's sums, bit for bit, and its exact counts."""
    rng = np.random.default_rng(H + W)
    host = rng.normal(0, 5, (B, 2, H, W)).astype(np.float32)
    fh = (rng.random((B, H, W)) < 0.1).astype(np.uint8) * rng.integers(1, 8, (B, H, W), dtype=np.uint8)
    st = V.MaskedFlowStats(H, W, 0.37, dev)
    st.update(torch.from_numpy(host).to(dev), torch.from_numpy(fh).to(dev))
    want_acc, want_cnt = vr.accumulate_masked(np.zeros((7, H, W)), np.zeros((2, H, W)), host, fh, 0.37)
    assert same_bits(st.acc.cpu().numpy(), want_acc)
    assert np.array_equal(st.cnt.cpu().numpy(), want_cnt) and want_cnt[0].min() < want_cnt[0].max() == B


def _lib_validate(flow, out, flag, resid, r, s, mode):
    B, _, H, W = flow.shape
    _lib.check(_lib.load().pivlfn_flow_validate(flow.data_ptr(), out.data_ptr() if out is not None else None, flag.data_ptr(),
                                                resid.data_ptr() if resid is not None else None, B, H, W, r, s, 0.1, 2.0,
                                                V.MODES[mode], _lib.stream_ptr(flow.device)), mode)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 77), (77, 1), (3, 1025), (1024, 1024)])
def test_guarded_buffers(dev, H, W):
    """The flow's last byte against the back guard, every output pre-filled: every element of out, flag and resid written, nothing
    outside any buffer touched, and what the outputs held before the call does not change the result."""
    B = 4                                                  # B*H*W bytes of flags: a whole number of 32-bit words for guarded()
    rng = np.random.default_rng(H * 7 + W)
    src = torch.from_numpy(rng.normal(0, 4, (B, 2, H, W)).astype(np.float32)).to(dev)
    src[0, 0].view(-1)[::5] = float("nan")                 # unknown vectors, so that every flag bit occurs where the size allows
    fl = guarded((B, 2, H, W), torch.float32, dev, "nan")
    fl.copy_(src)
    for r, s in ((1, 1), (2, 1), (2, 8)):
        for mode in MODES:
            want = V.validate_flow(src, r, s, mode=mode, residual=True)
            for fill in ("sentinel", "big"):
                out = guarded((B, 2, H, W), torch.float32, dev, fill) if mode != "flag" else None
                flag = guarded((B, H, W), torch.uint8, dev, fill)
                resid = guarded((B, 2, H, W), torch.float32, dev, fill)
                assert bool((flag > 7).all())              # no byte of either fill is a value a flag can take
                _lib_validate(fl, out, flag, resid, r, s, mode)
                torch.cuda.synchronize()
                tag = f"{mode} r={r} s={s} {H}x{W} {fill}"
                check_guards(fl, tag + " flow")
                check_guards(flag, tag + " flag")
                check_guards(resid, tag + " resid")
                assert bool((flag <= 7).all()), tag + ": a flag byte was not written"
                assert torch.equal(flag, want.flag), tag
                assert torch.equal(_bits(resid), _bits(want.residual)), tag
                if fill == "sentinel":
                    assert not bool(holds(resid, "sentinel").any()), tag + ": a residual was not written"
                if out is not None:
                    check_guards(out, tag + " out")
                    assert torch.equal(_bits(out), _bits(want.flow)), tag
                    if fill == "sentinel":
                        assert not bool(holds(out, "sentinel").any()), tag + ": an output element was not written"
    # the masked accumulation: flows and flags against their back guards, acc and cnt guarded
    flags = V.validate_flow(src, mode="flag").flag
    gflag = guarded((B, H, W), torch.uint8, dev, "nan")
    gflag.copy_(flags)
    st = V.MaskedFlowStats(H, W, device=dev)
    st.acc = guarded((7, H, W), torch.float64, dev, "sentinel")
    st.cnt = guarded((2, H, W), torch.float64, dev, "sentinel")
    st.acc.zero_()
    st.cnt.zero_()
    st.update(fl, gflag)
    torch.cuda.synchronize()
    for g, name in ((fl, "flow"), (gflag, "flag"), (st.acc, "acc"), (st.cnt, "cnt")):
        check_guards(g, "masked stats " + name)
    acc, cnt = vr.accumulate_masked(np.zeros((7, H, W)), np.zeros((2, H, W)), src.cpu().numpy(), flags.cpu().numpy(), 1.0)
    assert same_bits(st.acc.cpu().numpy(), acc) and np.array_equal(st.cnt.cpu().numpy(), cnt)


def test_masked_stats(dev):
    """All-zero flags: the sums of FlowStats, bit for bit.  Flags of validate_flow on noisy frames with unknown vectors: the
    restatement's masked sums and exact counts, for any split of the frames into calls; result() is NaN exactly where a count is 0."""
    rng = np.random.default_rng(13)
    H, W, calib, n = 96, 131, 0.37, 13
    host = (rng.normal(0, 5, (n, 2, H, W)) + rng.normal(1, 0.5, (2, 1, 1))).astype(np.float32)
    host[:, 0, 40, 50] = np.nan                            # a pixel that is unknown in every frame: count 0
    host[::2, 1, 10, 10] = np.inf
    flows = torch.from_numpy(host).to(dev)
    zero = torch.zeros([n, H, W], dtype=torch.uint8, device=dev)
    plain, masked = postpro.FlowStats(H, W, calib, dev), V.MaskedFlowStats(H, W, calib, dev)
    plain.update(flows)
    masked.update(flows, zero)
    assert torch.equal(masked.acc.view(torch.int64), plain.acc.view(torch.int64))
    assert bool((masked.cnt == float(n)).all()) and masked.count == n
    flags = V.validate_flow(flows, mode="flag").flag
    fh = flags.cpu().numpy()
    assert np.array_equal(fh, vr.validate(host, mode="flag")[1])
    assert (fh[:, 40, 50] == vr.UNKNOWN).all() and 0.05 < (fh != 0).mean() < 0.95
    want_acc, want_cnt = vr.accumulate_masked(np.zeros((7, H, W)), np.zeros((2, H, W)), host, fh, calib)
    runs = []
    for splits in ([n], [1] * n, [4, 4, 5]):
        st = V.MaskedFlowStats(H, W, calib, dev)
        k = 0
        for m in splits:
            st.update(flows[k:k + m], flags[k:k + m])
            k += m
        assert st.count == n
        assert same_bits(st.acc.cpu().numpy(), want_acc), splits
        assert np.array_equal(st.cnt.cpu().numpy(), want_cnt), splits
        runs.append(st)
    assert np.isfinite(want_acc).all()                     # every NaN and inf of the input was flagged and left out
    assert want_cnt[0, 40, 50] == 0 and want_cnt[1, 40, 50] == 0 and want_cnt[1, 39, 49] == 0
    r = runs[2].result()
    assert list(r) == list(V.MASKED_RESULT)
    for k in ("mean_u", "mean_v", "rms_u", "rms_v", "cov_uv"):
        assert np.array_equal(np.isnan(r[k]), want_cnt[0] == 0), k
    for k in ("mean_vort", "rms_vort"):
        assert np.array_equal(np.isnan(r[k]), want_cnt[1] == 0), k
    assert (want_cnt[1] == 0).sum() > (want_cnt[0] == 0).sum() >= 1
    assert np.array_equal(r["count_uv"], want_cnt[0].astype(np.int64)) and np.array_equal(r["valid_fraction"], want_cnt[0] / n)
    ok = fh[:, 7, 9] == 0
    assert ok.any() and abs(r["mean_u"][7, 9] - host[ok, 0, 7, 9].astype(np.float64).mean()) < 1e-12
    with pytest.raises(TypeError):
        masked.update(flows, flags.to(torch.int32))
    with pytest.raises(ValueError):
        masked.update(flows, flags[:, :-1])


def test_run_py_validate(tmp_path, dev):
    """run.py on a small PNG sequence.  Without --validate: the .flo files are estimate()'s outputs, byte for byte, and args.txt
    does not mention validation.  --validate replace --stats: the .flo files are validate_flow(estimate(...)), validation.json
    holds the flags' popcounts, stats.npz is FlowStats over the replaced flows.  --validate flag --stats: the flows unchanged,
    stats.npz is MaskedFlowStats over (flow, flag)."""
    import PIL.Image
    import run as runpy
    from pivlfn.pipeline import read_image_u8, u8_to_input
    seq = tmp_path / "seq"
    seq.mkdir()
    for k in range(6):
        a, _, _ = synth.particle_pair(64, 96, 700 + k)
        PIL.Image.fromarray(a).save(str(seq / f"frame_{k:04d}.png"))
    names = [f"frame_{k:04d}" for k in range(5)]
    net = pivlfn.Network(model="piv", params=synth.generate_weights("piv", 0)).to(dev).eval()
    frames = torch.from_numpy(np.stack([read_image_u8(str(seq / f"frame_{k:04d}.png")) for k in range(6)])).to(dev)
    est = torch.cat([pivlfn.estimate(net, u8_to_input(frames[k:k + 2][:min(2, 5 - k)]), u8_to_input(frames[k + 1:k + 3][:min(2, 5 - k)]),
                                     tensor=True) for k in (0, 2, 4)])                    # the batches of --batch 2
    assert est.shape == (5, 2, 64, 96)

    def flos(out):
        save = out / "piv-synthetic" / "seq"
        return save, [read_flow(str(save / "flow" / f"{n}_out.flo")) for n in names]

    base = ["--model", "piv", "-i", str(seq), "--batch", "2"]
    assert runpy.main(base + ["-o", str(tmp_path / "plain")]) == 5
    save, got = flos(tmp_path / "plain")
    for k in range(5):
        assert vr.same_bits32(got[k], est[k].permute(1, 2, 0).cpu().numpy()), k
    assert not [ln for ln in open(save / "args.txt") if ln.startswith("validate")] and not (save / "validation.json").exists()

    params = dict(radius=2, spacing=1, eps=0.01, thresh=0.5)
    flags_cli = ["--validate-radius", "2", "--validate-eps", "0.01", "--validate-thresh", "0.5"]
    want = V.validate_flow(est, mode="replace", **params)
    assert int((want.flag != 0).sum()) > 0
    assert runpy.main(base + ["-o", str(tmp_path / "rep"), "--validate", "replace", "--stats"] + flags_cli) == 5
    save, got = flos(tmp_path / "rep")
    for k in range(5):
        assert vr.same_bits32(got[k], want.flow[k].permute(1, 2, 0).cpu().numpy()), k
    doc = json.load(open(save / "validation.json"))
    assert doc["mode"] == "replace" and {k: doc[k] for k in params} == params and list(doc["pairs"]) == names
    wf = want.flag.cpu().numpy()
    for k, n in enumerate(names):
        assert doc["pairs"][n] == {"outlier": int((wf[k] & 1 != 0).sum()), "unknown": int((wf[k] & 2 != 0).sum()),
                                   "not_replaced": int((wf[k] & 4 != 0).sum())}
    assert doc["total"] == {key: sum(doc["pairs"][n][key] for n in names) for key in ("outlier", "unknown", "not_replaced")}
    st = postpro.FlowStats(64, 96, device=dev)
    st.update(want.flow)
    npz = np.load(save / "stats.npz")
    assert str(npz["validation"]) == "replace" and int(npz["count"]) == 5 and same_bits(npz["acc"], st.acc.cpu().numpy())
    assert "validate: replace\n" in list(open(save / "args.txt")) and "validate_radius: 2\n" in list(open(save / "args.txt"))

    assert runpy.main(base + ["-o", str(tmp_path / "flag"), "--validate", "flag", "--stats"] + flags_cli) == 5
    save, got = flos(tmp_path / "flag")
    for k in range(5):
        assert open(save / "flow" / f"{names[k]}_out.flo", "rb").read() == \
            open(tmp_path / "plain" / "piv-synthetic" / "seq" / "flow" / f"{names[k]}_out.flo", "rb").read()
    ms = V.MaskedFlowStats(64, 96, device=dev)
    fl = V.validate_flow(est, mode="flag", **params)
    ms.update(est, fl.flag)
    npz = np.load(save / "stats.npz")
    assert str(npz["validation"]) == "flag" and same_bits(npz["acc"], ms.acc.cpu().numpy())
    assert np.array_equal(npz["cnt"], ms.cnt.cpu().numpy()) and np.array_equal(npz["count_uv"], ms.cnt[0].cpu().numpy().astype(np.int64))
    assert json.load(open(save / "validation.json"))["total"]["not_replaced"] == 0

    assert runpy.main(base + ["-o", str(tmp_path / "mask"), "--validate", "mask"] + flags_cli) == 5
    save, got = flos(tmp_path / "mask")
    wm = V.validate_flow(est, mode="mask", **params)
    for k in range(5):
        assert vr.same_bits32(got[k], wm.flow[k].permute(1, 2, 0).cpu().numpy()), k
    assert (np.stack(got) == np.float32(1e10)).any() and not (save / "stats.npz").exists()
