"""GPU: pivlfn_flow_fields / pivlfn_flow_stats_accumulate (csrc/postpro.hip), the numpy drop-ins of src/postpro.py, FlowStats
and its use in run_sequence, tools/sequence_run.py --stats and run.py --stats -- against the reference's outputs and the
restatement of tests/postpro_restatement.py, bit for bit."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import analysis_plans as ap
import pivlfn
from pivlfn import postpro, synth
from pivlfn.flo import read_flow
from guarded import check_guards, guarded, holds
from postpro_restatement import accumulate, fields, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
KINDS = ("calc_vorticity", "de_vort")


def _dev_flows(flow_hw2, dev):
    return torch.from_numpy(np.ascontiguousarray(flow_hw2.transpose(2, 0, 1)))[None].to(dev)


def test_fields_match_reference_fixture(dev):
    g = np.load(os.path.join(GOLD, "postpro_cases.npz"))
    for tag in g["cases"]:
        flow, calib = g[f"{tag}_flow"], float(g[f"{tag}_calib"])
        f = _dev_flows(flow, dev)
        for kind in KINDS:
            want = g[f"{tag}_{kind}"]
            got64 = postpro.flow_fields(f, calib, kind, torch.float64)[0].cpu().numpy()
            assert same_bits(got64, want), (tag, kind)
            got32 = postpro.flow_fields(f, calib, kind, torch.float32)[0].cpu().numpy()
            assert same_bits(got32, want.astype(np.float32)), (tag, kind, "fp32")
        # the numpy drop-ins return the reference's arrays exactly
        for kind, fn in (("calc_vorticity", postpro.calc_vorticity), ("de_vort", postpro.de_vort)):
            out = fn(flow, calib)
            assert len(out) == 3 and all(o.dtype == np.float64 and o.shape == flow.shape[:2] for o in out)
            assert same_bits(np.stack(out), g[f"{tag}_{kind}"]), (tag, kind, "drop-in")
    with pytest.raises(TypeError):
        postpro.calc_vorticity(g["odd13x17_c1_flow"].astype(np.float64))
    with pytest.raises(TypeError):
        postpro.de_vort(g["odd13x17_c1_flow"].astype(np.float64))
    import src.postpro as sp
    assert same_bits(np.stack(sp.de_vort(g["dns_crop_flow"])), g["dns_crop_de_vort"])


def test_large_and_batched_inputs_match_restatement(dev):
    """1024^2, B = 3: random flows and a real estimate() output; a batch of 5 equals the same frames one at a time."""
    rng = np.random.default_rng(11)
    S = 1024
    net = pivlfn.piv_liteflownet(synth.generate_weights("piv", 0)).to(dev).eval()
    a, b = synth.particle_batch(1, S, S, seed=5)
    est = pivlfn.estimate(net, torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), tensor=True)
    flows = torch.cat([torch.from_numpy(rng.normal(0, 6, (2, 2, S, S)).astype(np.float32)).to(dev), est])
    host = flows.cpu().numpy()
    assert np.abs(host[2]).max() > 0.5
    for kind, calib in (("calc_vorticity", 0.37), ("de_vort", 2.5e-4)):
        want = fields(host, calib, kind)
        assert same_bits(postpro.flow_fields(flows, calib, kind, torch.float64).cpu().numpy(), want), kind
        assert same_bits(postpro.flow_fields(flows, calib, kind).cpu().numpy(), want.astype(np.float32)), kind
    five = torch.from_numpy(rng.normal(0, 6, (5, 2, 37, 53)).astype(np.float32)).to(dev)
    for kind in KINDS:
        for dt in (torch.float32, torch.float64):
            batched = postpro.flow_fields(five, 1.0, kind, dt)
            single = torch.cat([postpro.flow_fields(five[k:k + 1], 1.0, kind, dt) for k in range(5)])
            assert same_bits(batched.cpu().numpy(), single.cpu().numpy()), (kind, dt)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 77), (77, 1), (3, 1025), (1024, 1024)])
def test_guarded_buffers(dev, H, W):
    """The flow's last byte against the back guard, the output pre-filled with a sentinel: every output element written, nothing
    outside either buffer touched; the accumulators likewise."""
    B = 2
    rng = np.random.default_rng(H * 7 + W)
    src = torch.from_numpy(rng.normal(0, 4, (B, 2, H, W)).astype(np.float32)).to(dev)
    fl = guarded((B, 2, H, W), torch.float32, dev, "nan")
    fl.copy_(src)
    for kind in KINDS:
        for dt in (torch.float32, torch.float64):
            out = guarded((B, 3, H, W), dt, dev, "sentinel")
            _lib_fields(fl, out, kind)
            torch.cuda.synchronize()
            check_guards(fl, f"{kind} flow {H}x{W}")
            check_guards(out, f"{kind} out {H}x{W} {dt}")
            assert not bool(holds(out, "sentinel").any()), f"{kind} {dt}: an output element was not written"
            assert same_bits(out.cpu().numpy(), postpro.flow_fields(src, 1.0, kind, dt).cpu().numpy())
    acc = guarded((7, H, W), torch.float64, dev, "sentinel")
    acc.zero_()
    st = postpro.FlowStats(H, W, device=dev)
    st.acc = acc
    st.update(fl)
    torch.cuda.synchronize()
    check_guards(fl, "stats flow")
    check_guards(acc, "stats acc")
    assert same_bits(acc.cpu().numpy(), accumulate(np.zeros((7, H, W)), src.cpu().numpy(), 1.0))


@pytest.mark.parametrize("B,H,W", ap.shapes(ap.FIELDS_CASES))
def test_fields_where_the_frame_grid_is_capped(dev, B, H, W):
    """More blocks a frame than the launch's cap, so the kernel's grid-stride loop comes round: the bits of the same frames in calls
    that are not capped."""
    gen = torch.Generator(device=dev).manual_seed(B + H)
    flows = torch.randn([B, 2, H, W], generator=gen, device=dev) * 6
    step = ap.FRAMES_PER_UNCAPPED_CALL
    for kind in KINDS:
        whole = postpro.flow_fields(flows, 0.37, kind)
        parts = torch.cat([postpro.flow_fields(flows[k:k + step], 0.37, kind) for k in range(0, B, step)])
        assert torch.equal(whole, parts), kind


@pytest.mark.parametrize("B,H,W", ap.shapes(ap.ACCUMULATOR_CASES))
def test_stats_where_the_grid_is_capped(dev, B, H, W):
    """More blocks than the flat cap of the accumulator's launch: the sequential numpy loop, bit for bit."""
    host = np.random.default_rng(H + W).normal(0, 5, (B, 2, H, W)).astype(np.float32)
    st = postpro.FlowStats(H, W, 0.37, dev)
    st.update(torch.from_numpy(host).to(dev))
    assert same_bits(st.acc.cpu().numpy(), accumulate(np.zeros((7, H, W)), host, 0.37))


def _lib_fields(flow, out, kind):
    from pivlfn import _lib
    B, _, H, W = flow.shape
    _lib.check(_lib.load().pivlfn_flow_fields(flow.data_ptr(), out.data_ptr(), B, H, W, 1.0, postpro.KINDS[kind],
                                              int(out.dtype == torch.float64), _lib.stream_ptr(flow.device)), kind)


def test_flowstats_accumulation_split_invariant(dev):
    """13 flows as one call, as 13 calls and as 4 + 4 + 5: identical accumulators, identical to the sequential numpy loop; the
    vorticity sums are the frame-ordered sum of flow_fields' float64 vort; result() agrees with two-pass float64 statistics."""
    rng = np.random.default_rng(13)
    H, W, calib = 96, 131, 0.37
    host = (rng.normal(0, 5, (13, 2, H, W)) + rng.normal(1, 0.5, (2, 1, 1))).astype(np.float32)
    flows = torch.from_numpy(host).to(dev)
    runs = []
    for splits in ([13], [1] * 13, [4, 4, 5]):
        st = postpro.FlowStats(H, W, calib, dev)
        k = 0
        for n in splits:
            st.update(flows[k:k + n])
            k += n
        assert st.count == 13
        runs.append(st)
    accs = [r.acc.cpu().numpy() for r in runs]
    assert same_bits(accs[0], accs[1]) and same_bits(accs[0], accs[2])
    assert same_bits(accs[0], accumulate(np.zeros((7, H, W)), host, calib))
    vort = postpro.flow_fields(flows, calib, "calc_vorticity", torch.float64)[:, 0].cpu().numpy()
    s5, s6 = np.zeros((H, W)), np.zeros((H, W))
    for v in vort:
        s5 = s5 + v
        s6 = s6 + v * v
    assert same_bits(accs[0][5], s5) and same_bits(accs[0][6], s6)
    r = runs[2].result()
    u, v = host[:, 0].astype(np.float64), host[:, 1].astype(np.float64)
    want = {"mean_u": u.mean(0), "mean_v": v.mean(0), "rms_u": u.std(0), "rms_v": v.std(0),
            "cov_uv": ((u - u.mean(0)) * (v - v.mean(0))).mean(0), "mean_vort": vort.mean(0), "rms_vort": vort.std(0)}
    assert int(r["count"]) == 13
    for k, w in want.items():
        assert np.abs(r[k] - w).max() <= 1e-9, (k, np.abs(r[k] - w).max())


def _sequence_flows(dev, n_frames, S, seed):
    from pivlfn.sequence import frames_to_input
    net = pivlfn.piv_liteflownet(synth.generate_weights("piv", 0)).to(dev).eval()
    x = frames_to_input(synth.ParticleSequence(S, S, seed=seed, device=dev).frames(0, n_frames))
    return net, [pivlfn.estimate(net, x[k:k + 1], x[k + 1:k + 2], tensor=True) for k in range(n_frames - 1)]


@pytest.mark.parametrize("chunk", [3, 4])
def test_run_sequence_stats_one_rank(dev, chunk):
    """Chunks of 3 and 4 over 7 pairs (a short last chunk): the accumulators equal FlowStats fed estimate() pair by pair."""
    from pivlfn.sequence import run_sequence
    n_frames, S = 8, 256
    net, per_pair = _sequence_flows(dev, n_frames, S, seed=21)
    want = postpro.FlowStats(S, S, device=dev)
    for f in per_pair:
        want.update(f)
    st = postpro.FlowStats(S, S, device=dev)
    out = run_sequence(net, synth.ParticleSequence(S, S, seed=21, device=dev).frames, n_frames, chunk, dev,
                       sink=lambda gi, flow: None, stats=st)
    assert out["pairs_total"] == 7 and st.count == 7
    assert torch.equal(st.acc.view(torch.int64), want.acc.view(torch.int64))


def test_sequence_run_stats_two_ranks(tmp_path, dev):
    """tools/sequence_run.py --stats with 2 gloo ranks on one GPU: merged count = n_pairs, every accumulator within 1e-12 of
    sum |terms| of the one-rank sums at each pixel, and only rank 0 writes the file."""
    from test_gpu_configs import _run_children
    n_frames, S = 8, 256
    path = tmp_path / "stats.npz"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "sequence_run.py"), "--frames", str(n_frames), "--size", str(S), "--chunk", "3",
           "--null-sink", "--seed", "7", "--stats", str(path)]
    outs = _run_children(lambda r: cmd, 2, {"PIVLFN_BENCH_BACKEND": "gloo"})
    line = json.loads([ln for ln in outs[0][1].splitlines() if ln.startswith("{")][-1])
    assert line["stats_file"] == str(path)
    assert not [ln for ln in outs[1][1].splitlines() if ln.startswith("{")]
    assert sorted(os.listdir(tmp_path)) == ["stats.npz"]
    got = np.load(path)
    assert int(got["count"]) == n_frames - 1 and float(got["calib"]) == 1.0
    _, per_pair = _sequence_flows(dev, n_frames, S, seed=7)
    host = torch.cat(per_pair).cpu().numpy()
    want = accumulate(np.zeros((7, S, S)), host, 1.0)
    absw = np.zeros((7, S, S))
    ab = np.abs(host.astype(np.float64))
    vort = np.abs(fields(host, 1.0, "calc_vorticity")[:, 0])
    for t, term in enumerate((ab[:, 0], ab[:, 1], ab[:, 0] ** 2, ab[:, 1] ** 2, ab[:, 0] * ab[:, 1], vort, vort ** 2)):
        absw[t] = term.sum(0)
    assert np.all(np.abs(got["acc"] - want) <= 1e-12 * absw)
    for k in postpro.RESULT[1:]:
        assert got[k].shape == (S, S)


def test_run_py_stats(tmp_path, dev):
    """run.py --stats on a small PNG sequence: stats.npz equals FlowStats over the .flo files the run wrote, read back."""
    import PIL.Image
    import run as runpy
    seq = tmp_path / "seq"
    seq.mkdir()
    for k in range(6):
        a, _, _ = synth.particle_pair(64, 96, 700 + k)
        PIL.Image.fromarray(a).save(str(seq / f"frame_{k:04d}.png"))
    out = tmp_path / "out"
    assert runpy.main(["--model", "piv", "-i", str(seq), "-o", str(out), "--batch", "2", "--stats"]) == 5
    save = out / "piv-synthetic" / "seq"
    got = np.load(save / "stats.npz")
    want = postpro.FlowStats(64, 96, device=dev)
    for k in range(5):
        f = read_flow(str(save / "flow" / f"frame_{k:04d}_out.flo"))
        want.update(torch.from_numpy(np.ascontiguousarray(f.transpose(2, 0, 1)))[None].to(dev))
    assert int(got["count"]) == 5 and same_bits(got["acc"], want.acc.cpu().numpy())
    with pytest.raises(SystemExit):
        runpy.main(["--model", "piv", "-i", str(seq), "-o", str(tmp_path / "o2"), "--stats", "-b", "1.1"])
    env = os.environ.get("WORLD_SIZE")
    os.environ["WORLD_SIZE"] = "2"
    try:
        with pytest.raises(SystemExit):
            runpy.main(["--model", "piv", "-i", str(seq), "-o", str(tmp_path / "o3"), "--stats"])
    finally:
        if env is None:
            del os.environ["WORLD_SIZE"]
        else:
            os.environ["WORLD_SIZE"] = env
