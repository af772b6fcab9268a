"""GPU: pivlfn_flow_errors, pivlfn_level_errors and pivlfn_error_stats_accumulate (csrc/evaluate.hip), flow_errors, level_errors,
ErrorStats, src.loss and run.py --truth -- the sums against the numpy restatement of tests/evaluate_restatement.py bit for bit, the
reference's recorded float64 results within the bound derived in tests/test_evaluate.py."""
import json
import os

import numpy as np
import pytest
import torch

import analysis_plans as ap
import evaluate_restatement as er
import pivlfn
from guarded import KINDS, check_guards, guarded, poison, same_bits
from pivlfn import _lib, synth
from pivlfn import evaluate as E
from pivlfn.flo import read_flow, write_flow

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _sums(err):
    return torch.stack([getattr(err, q) for q in E.FIELDS], dim=1)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _case(rng, B, H, W, k, holes=True):
    """Flows a pixel or so off a smooth-plus-noise truth; some truth values unknown and a mask with a block and speckles."""
    truth = (rng.normal(0, 3, (B, 2, H, W)) + rng.normal(0, 2, (B, 2, 1, 1))).astype(np.float32)
    flow = rng.normal(0, 1, (B, 2, H >> k, W >> k)).astype(np.float32)
    mask = None
    if holes:
        n = max(1, H * W // 50)
        vals = (np.nan, 1e10, -np.inf, 2e9)
        for j, (b, c, y, x) in enumerate(zip(rng.integers(0, B, n), rng.integers(0, 2, n), rng.integers(0, H, n), rng.integers(0, W, n))):
            truth[b, c, y, x] = vals[j % 4]
        mask = (rng.random((B, H, W)) < 0.02).astype(np.uint8) * 7
        mask[0, H // 3:H // 2, W // 4:W // 2] = 1
    return flow, truth, mask


def _check(dev, flow, truth, mask, k, div_flow, tag):
    want, want_map = er.flow_errors(flow, truth, mask, k, div_flow)
    got = E.flow_errors(_t(flow, dev), _t(truth, dev), None if mask is None else _t(mask, dev), pool=1 << k, div_flow=div_flow,
                        want_map=True)
    assert same_bits(_sums(got).cpu(), torch.from_numpy(want)), (tag, _sums(got).cpu().numpy(), want)
    assert same_bits(got.map.cpu(), torch.from_numpy(want_map)), tag           # NaN where excluded: the canonical quiet NaN in both
    return got


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (37, 53), (33, 64), (64, 96), (32, 8224)])
def test_full_resolution_matches_restatement(dev, H, W):
    """Odd sizes (scalar loads, partial tiles), tile multiples (16-byte loads), and 1 x 257 tiles: three passes of the second kernel."""
    rng = np.random.default_rng(H * 1000 + W)
    for holes in (False, True):
        flow, truth, mask = _case(rng, 3, H, W, 0, holes)
        got = _check(dev, flow, truth, mask, 0, 0.2 if holes else 1.0, (H, W, holes))
        assert bool(torch.isfinite(_sums(got)).all())
        if not holes:
            assert got.n.tolist() == [H * W] * 3


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 5])
def test_every_pool_exponent_matches_restatement(dev, k):
    """Sizes that are multiples of 2^k but not of 32 where that is possible (partial tiles below the pooled level), and 96 x 160:
    a 3 x 5 tile grid, padded to the contract's tree in the second kernel."""
    rng = np.random.default_rng(50 + k)
    for H, W in ((3 << k, 5 << k), (96, 160)):
        flow, truth, mask = _case(rng, 2, H, W, k)
        _check(dev, flow, truth, mask, k, 1.0 / 5, (k, H, W))


def test_batch_of_five_equals_five_single_calls(dev):
    rng = np.random.default_rng(5)
    flow, truth, mask = _case(rng, 5, 70, 131, 0)
    f, t, m = _t(flow, dev), _t(truth, dev), _t(mask, dev)
    whole = E.flow_errors(f, t, m, want_map=True)
    again = E.flow_errors(f, t, m)
    assert same_bits(_sums(whole), _sums(again))
    for b in range(5):
        one = E.flow_errors(f[b:b + 1], t[b:b + 1], m[b:b + 1], want_map=True)
        assert same_bits(_sums(one)[0], _sums(whole)[b]) and same_bits(one.map[0], whole.map[b]), b
    empty = E.flow_errors(f[:0], t[:0])
    assert empty.n.shape == (0,) and empty.aee.shape == (0,)


def test_unaligned_pointers_take_the_scalar_path(dev):
    """Flow and truth that start 4 bytes off a 16-byte boundary: the same bits as the aligned copies."""
    rng = np.random.default_rng(16)
    flow, truth, mask = _case(rng, 2, 64, 96, 0)
    f, t, m = _t(flow, dev), _t(truth, dev), _t(mask, dev)
    off = [torch.empty(x.numel() + 1, device=dev)[1:].view(x.shape).copy_(x) for x in (f, t)]
    assert all(x.data_ptr() % 16 == 4 and x.is_contiguous() for x in off)
    want = E.flow_errors(f, t, m, want_map=True)
    for ff, tt in ((off[0], t), (f, off[1]), (off[0], off[1])):
        got = E.flow_errors(ff, tt, m, want_map=True)
        assert same_bits(_sums(got), _sums(want)) and same_bits(got.map, want.map)
    st, st2 = E.ErrorStats(64, 96, dev), E.ErrorStats(64, 96, dev)
    st.update(f, t, m)
    st2.update(off[0], off[1], m)
    assert torch.equal(st.acc.view(torch.int64), st2.acc.view(torch.int64))


def test_special_values(dev):
    """An all-excluded pair reports zeros (max 0, not -inf) and a NaN AEE; a NaN in the estimated flow is not excluded; -0.0 sums
    read +0.0."""
    truth = np.zeros((3, 2, 8, 8), np.float32)
    flow = np.zeros((3, 2, 8, 8), np.float32)
    truth[0] = np.nan
    flow[1, 0, 3, 3] = np.nan
    flow[2] = -0.0
    got = E.flow_errors(_t(flow, dev), _t(truth, dev))
    s = _sums(got).cpu().numpy()
    assert s[0].tolist() == [0.0] * 7 and not np.signbit(s[0]).any() and np.isnan(got.aee[0].item())
    assert s[1, 0] == 64 and np.isnan(s[1, [1, 2, 3, 4, 6]]).all() and s[1, 5] == 0.0       # dv is 0 everywhere
    assert s[2].tolist() == [64.0, 0, 0, 0, 0, 0, 0] and not np.signbit(s[2]).any()
    want, _ = er.flow_errors(flow[[0, 2]], truth[[0, 2]])
    assert er.same_bits(s[[0, 2]], want)


@pytest.fixture(scope="module")
def megapixel(dev):
    """1024 x 1024, B = 3, 32 x 32 tiles: a real estimate() output of the seeded network for one particle pair, the same with noise
    added and with its sign turned; a real forward_levels() output for the pair three times; three different truths (the pair's true
    field, the same with noise, its negative) with some unknown values, and a mask."""
    S = 1024
    net = pivlfn.piv_liteflownet(synth.generate_weights("piv", 0)).to(dev).eval()
    i1, i2, true = synth.particle_pair(S, S, 40)
    a, b = _t(synth.to_input(i1)[None], dev), _t(synth.to_input(i2)[None], dev)
    est = pivlfn.estimate(net, a, b, tensor=True)
    rng = np.random.default_rng(40)
    noise = torch.from_numpy(rng.normal(0, 0.3, (1, 2, S, S)).astype(np.float32)).to(dev)
    est = torch.cat([est, est + noise, -est]).contiguous()
    _, levels = net.forward_levels(a.expand(3, -1, -1, -1).contiguous(), b.expand(3, -1, -1, -1).contiguous())
    truth = np.stack([true, true + rng.normal(0, 0.2, true.shape).astype(np.float32), -true])
    truth[1, 0, 100:103, 700:900] = np.nan
    truth[2, 1, 1023, 1023] = 1e10
    mask = np.zeros((3, S, S), np.uint8)
    mask[0, 500:540, 33:600] = 1
    mask[2, ::97, ::89] = 200
    return dict(net=net, est=est, levels=levels, truth=truth, mask=mask)


def test_megapixel_estimate_output(dev, megapixel):
    est, truth = megapixel["est"], megapixel["truth"]
    for mask in (None, megapixel["mask"]):
        want = er.flow_errors(est.cpu().numpy(), truth, mask)[0]
        got = E.flow_errors(est, _t(truth, dev), None if mask is None else _t(mask, dev))
        assert same_bits(_sums(got).cpu(), torch.from_numpy(want))
        assert bool((got.max >= got.aee).all()) and bool((got.rmse >= got.aee).all())
    assert got.n.tolist() == want[:, 0].tolist() and got.n[0].item() == 1024 * 1024 - 40 * 567
    one = E.flow_errors(est[1:2], _t(truth[1:2], dev), _t(mask[1:2], dev))
    assert same_bits(_sums(one)[0], _sums(got)[1])


def test_megapixel_level_errors(dev, megapixel):
    """forward_levels at 1024 x 1024, B = 3: a 32 x 32 tile grid, so the second kernel runs twice with 18 jobs per tile.  The one
    pass gives the bits of the 18 separate calls and of the restatement."""
    net, levels, truth, mask = (megapixel[k] for k in ("net", "levels", "truth", "mask"))
    t, m = _t(truth, dev), _t(mask, dev)
    table = E.level_errors(net, levels, t, 0.2, m)
    assert len(table) == 6
    for i, trio in enumerate(levels):
        for s, f in enumerate(trio):
            one = E.flow_errors(f, t, m, pool=1 << (5 - i), div_flow=0.2)
            assert same_bits(_sums(table[i][s]), _sums(one)), (i, s)
    want = er.level_errors([[f.cpu().numpy() for f in trio] for trio in levels], 1, truth, mask, 0.2)
    got = torch.stack([torch.stack([_sums(e) for e in row], dim=1) for row in table], dim=1)
    assert same_bits(got.cpu(), torch.from_numpy(want))
    assert bool(torch.isfinite(got).all()) and got[1, 5, 2, 0].item() == 1024 * 1024 - 3 * 200
    alone = E.level_errors(net, [[f[2:3] for f in trio] for trio in levels], t[2:3], 0.2, m[2:3])      # a pair alone: copies, not the packed buffer
    assert all(same_bits(_sums(alone[i][s])[0], _sums(table[i][s])[2]) for i in range(6) for s in range(3))


def test_megapixel_error_stats(dev, megapixel):
    est, truth, mask = megapixel["est"], megapixel["truth"], megapixel["mask"]
    want = er.accumulate_errors(np.zeros((6, 1024, 1024)), est.cpu().numpy(), truth, mask)
    for splits in ([3], [1, 2]):
        st, k = E.ErrorStats(1024, 1024, dev), 0
        for c in splits:
            st.update(est[k:k + c], _t(truth[k:k + c], dev), _t(mask[k:k + c], dev))
            k += c
        assert st.count == 3 and er.same_bits(st.acc.cpu().numpy(), want), splits


@pytest.mark.parametrize("B,H,W", ap.shapes(ap.ACCUMULATOR_CASES))
def test_error_stats_where_the_grid_is_capped(dev, B, H, W):
    """More blocks than the flat cap of the accumulator's launch, with unknown truth and a mask: the restatement's sums, bit for bit."""
    flow, truth, mask = _case(np.random.default_rng(H + W), B, H, W, 0)
    st = E.ErrorStats(H, W, dev)
    st.update(_t(flow, dev), _t(truth, dev), _t(mask, dev))
    assert st.count == B and er.same_bits(st.acc.cpu().numpy(), er.accumulate_errors(np.zeros((6, H, W)), flow, truth, mask))


MODELS = [("piv", 1), ("hui", 1), ("hui", 2)]


@pytest.mark.parametrize("model,version", MODELS)
def test_level_errors_equal_per_level_flow_errors(dev, model, version):
    """A real forward_levels output at 64 x 96 and 128 x 160, B = 2, with unknown truth and a mask: one pass over the truth gives the bits
    of nlev * 3 separate calls, which give the restatement's."""
    name = model + ("2" if version == 2 else "")
    net = pivlfn.Network(model=model, params=synth.generate_weights(name, 0), version=version).to(dev).eval()
    div = 1.0 / (5 if model == "piv" else 20)
    for H, W in ((64, 96), (128, 160)):
        pairs = [synth.particle_pair(H, W, 60 + b) for b in range(2)]
        a = _t(np.stack([synth.to_input(p[0]) for p in pairs]), dev)
        b = _t(np.stack([synth.to_input(p[1]) for p in pairs]), dev)
        _, levels = net.forward_levels(a, b)
        truth = np.stack([p[2] for p in pairs])
        truth[0, 1, 5, 7] = np.nan
        mask = np.zeros((2, H, W), np.uint8)
        mask[1, 20:30, 40:70] = 255
        t, m = _t(truth, dev), _t(mask, dev)
        assert len(levels) == 7 - net.lowest_level
        table = E.level_errors(net, levels, t, div, m)
        for i, trio in enumerate(levels):
            for s, f in enumerate(trio):
                one = E.flow_errors(f, t, m, pool=1 << (5 - i), div_flow=div)
                assert same_bits(_sums(table[i][s]), _sums(one)), (model, version, H, i, s)
        want = er.level_errors([[f.cpu().numpy() for f in trio] for trio in levels], net.lowest_level, truth, mask, div)
        got = torch.stack([torch.stack([_sums(e) for e in row], dim=1) for row in table], dim=1)
        assert same_bits(got.cpu(), torch.from_numpy(want))
        # copies that are not one packed buffer give the same
        again = E.level_errors(net.lowest_level, [[f.clone() for f in trio] for trio in levels], t, div, m)
        assert all(same_bits(_sums(x), _sums(y)) for r1, r2 in zip(table, again) for x, y in zip(r1, r2))


def test_error_stats_any_split(dev):
    rng = np.random.default_rng(21)
    H, W, n = 37, 53, 9
    flow, truth, mask = _case(rng, n, H, W, 0)
    truth[:, 0, 4, 4] = np.nan                                  # never scored: count 0
    f, t, m = _t(flow, dev), _t(truth, dev), _t(mask, dev)
    want = er.accumulate_errors(np.zeros((6, H, W)), flow, truth, mask)
    for splits in ([n], [1] * n, [2, 3, 4]):
        st = E.ErrorStats(H, W, dev)
        k = 0
        for c in splits:
            st.update(f[k:k + c], t[k:k + c], m[k:k + c])
            k += c
        assert st.count == n and er.same_bits(st.acc.cpu().numpy(), want), splits
    r = st.result()
    assert list(r) == list(E.RESULT) and r["count"][4, 4] == 0 and np.isnan(r["bias_u"][4, 4]) and int(r["frames"]) == n
    inc = ~(er.unknown(truth[:, 0, 7, 9]) | er.unknown(truth[:, 1, 7, 9]) | (mask[:, 7, 9] != 0))
    d = flow[inc, 0, 7, 9].astype(np.float64) - truth[inc, 0, 7, 9].astype(np.float64)
    assert abs(r["bias_u"][7, 9] - d.mean()) < 1e-12 and abs(r["rms_u"][7, 9] - d.std()) < 1e-9
    plain = E.ErrorStats(H, W, dev)
    plain.update(f, t)
    assert er.same_bits(plain.acc.cpu().numpy(), er.accumulate_errors(np.zeros((6, H, W)), flow, truth))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W,k", [(37, 53, 0), (64, 96, 0), (64, 96, 2), (24, 40, 3)])
def test_guarded_buffers_and_poisoned_workspace(dev, kind, H, W, k):
    """Every buffer's last byte against its back guard, the workspace and the outputs pre-filled with poison: guards intact, the
    result is that of a clean call, every element of sums and err_map written."""
    rng = np.random.default_rng(H + W + k)
    B = 2
    flow, truth, mask = _case(rng, B, H, W, k)
    want = E.flow_errors(_t(flow, dev), _t(truth, dev), _t(mask, dev), pool=1 << k, div_flow=0.2, want_map=True)
    h, w = H >> k, W >> k
    gf, gt = guarded((B, 2, h, w), torch.float32, dev, kind), guarded((B, 2, H, W), torch.float32, dev, kind)
    gf.copy_(_t(flow, dev))
    gt.copy_(_t(truth, dev))
    sums = guarded((B, 7), torch.float64, dev, kind)
    emap = guarded((B, 3, h, w), torch.float32, dev, "sentinel")
    lib = _lib.load()
    nws = lib.pivlfn_flow_errors_workspace_bytes(B, H, W)
    ws = guarded((nws // 4,), torch.float32, dev, kind)
    poison(ws, slice(0, nws // 4), kind)
    _lib.check(lib.pivlfn_flow_errors(gf.data_ptr(), gt.data_ptr(), _t(mask, dev).data_ptr(), B, H, W, k, 0.2, sums.data_ptr(),
                                      emap.data_ptr(), ws.data_ptr(), nws, _lib.stream_ptr(dev)), "flow_errors")
    torch.cuda.synchronize()
    for g, name in ((gf, "flow"), (gt, "truth"), (sums, "sums"), (emap, "err_map"), (ws, "workspace")):
        check_guards(g, f"{name} {H}x{W} k={k} {kind}")
    assert same_bits(sums, _sums(want)) and same_bits(emap, want.map)
    if H % 32 == 0 and W % 32 == 0:
        lv = [[torch.randn(B, 2, H >> j, W >> j, device=dev) for _ in range(3)] for j in range(5, -1, -1)]
        buf = guarded((sum(f.numel() for tr in lv for f in tr),), torch.float32, dev, kind)
        buf.copy_(torch.cat([f.reshape(-1) for tr in lv for f in tr]))
        lsums = guarded((B, 6, 3, 7), torch.float64, dev, kind)
        poison(ws, slice(0, nws // 4), kind)
        _lib.check(lib.pivlfn_level_errors(buf.data_ptr(), 1, gt.data_ptr(), None, B, H, W, 0.2, lsums.data_ptr(), ws.data_ptr(), nws,
                                           _lib.stream_ptr(dev)), "level_errors")
        torch.cuda.synchronize()
        for g, name in ((buf, "levels"), (gt, "truth"), (lsums, "sums"), (ws, "workspace")):
            check_guards(g, f"level_errors {name} {kind}")
        for i, tr in enumerate(lv):
            for s, f in enumerate(tr):
                one = E.flow_errors(f, gt, pool=1 << (5 - i), div_flow=0.2)
                assert same_bits(lsums[:, i, s], _sums(one)), (i, s)
    st = E.ErrorStats(H, W, dev)
    if k == 0:
        st.acc = guarded((6, H, W), torch.float64, dev, kind)
        st.acc.zero_()
        st.update(gf, gt)
        torch.cuda.synchronize()
        for g, name in ((gf, "flow"), (gt, "truth"), (st.acc, "acc")):
            check_guards(g, f"error stats {name} {kind}")
        assert er.same_bits(st.acc.cpu().numpy(), er.accumulate_errors(np.zeros((6, H, W)), flow, truth))


# ---- src.loss against the reference's recorded float64 results -------------------------------------------------------------------
U = 2.0 ** -53
CASES = er.load_cases(os.path.join(GOLD, "evaluate_cases.npz"))


def _flat(res):
    if isinstance(res, (list, tuple)):
        return torch.cat([_flat(r) for r in res])
    assert res.dtype == torch.float64 and res.dim() == 0 and res.is_cuda and not res.requires_grad
    return res.reshape(1)


@pytest.mark.parametrize("name", list(CASES))
def test_src_loss_against_reference_float64(dev, name):
    """Every recorded case through src.loss on the device: within 2 N u of the reference's float64 result (the bound derived in
    tests/test_evaluate.py), and the very bits of the restatement (the batch means are formed the same way)."""
    import src.loss as L
    c = CASES[name]
    out = _t(c["output"], dev) if isinstance(c["output"], np.ndarray) else \
        [[_t(f, dev) for f in o] if isinstance(o, list) else _t(o, dev) for o in c["output"]]
    truth = _t(c["truth"], dev)
    res = L.EPE(out, truth, **c["call"]) if c["fn"] == "EPE" else getattr(L, c["fn"])(**c["args"])(out, truth)
    got = _flat(res).cpu().numpy()
    want, ns = er.loss_value(c["fn"], c["args"], c["call"], c["output"], c["truth"])
    rel = np.abs(got - c["f64"]) / np.abs(c["f64"])
    print(name, "rel", rel)
    assert (rel <= np.array([2 * n * U for n in ns])).all(), (name, rel)
    assert er.same_bits(got, want), name


def test_demo_pair_reproduces_the_recorded_reference_epe(dev):
    """The reference's own network output for its demo pair against the true field that ships next to it."""
    rec = json.load(open(os.path.join(GOLD, "pin_report_evaluate.json")))["demo_DNS_turbulence"]
    out, true = (_t(read_flow(os.path.join(GOLD, f"DNS_turbulence_{n}.flo")).transpose(2, 0, 1)[None], dev) for n in ("out", "flow"))
    e = E.flow_errors(out, true)
    n = 256 * 256
    assert e.n.item() == n
    print("aee", e.aee.item(), "recorded", rec["epe_f64"], "l1", e.mean_l1.item(), rec["l1_f64"])
    assert abs(e.aee.item() - rec["epe_f64"]) <= 2 * n * U * rec["epe_f64"]
    assert abs(e.mean_l1.item() - rec["l1_f64"]) <= 2 * n * U * rec["l1_f64"]
    import src.loss as L
    assert abs(L.EPE(out, true).item() - rec["epe_f64"]) <= 2 * n * U * rec["epe_f64"]


# ---- run.py --truth ------------------------------------------------------------------------------------------------------------------
def test_run_py_truth(tmp_path, dev):
    """run.py -p on three synthetic particle pairs (PNG pair plus the true field as <name>_flow.flo).  errors.json equals
    flow_errors(estimate(...), truth) exactly; the .flo files and args.txt equal those of a run without --truth, byte for byte;
    error_maps.npz is ErrorStats over the same flows.  With --validate mask the flags are the mask and the excluded vectors are
    counted; with --truth-levels the level x stage table is level_errors' on the same forward."""
    import PIL.Image
    import run as runpy
    from pivlfn import validate as V
    from pivlfn.pipeline import read_image_u8, u8_to_input
    H, W = 64, 96
    seq, tr = tmp_path / "seq", tmp_path / "truth"
    seq.mkdir()
    tr.mkdir()
    names = [f"p{k}" for k in range(3)]
    truths = []
    for k, name in enumerate(names):
        a, b, true = synth.particle_pair(H, W, 900 + k)
        PIL.Image.fromarray(a).save(str(seq / f"{name}_img1.png"))
        PIL.Image.fromarray(b).save(str(seq / f"{name}_img2.png"))
        write_flow(np.ascontiguousarray(true.transpose(1, 2, 0)), str(tr / f"{name}_flow.flo"))
        truths.append(true)
    truth = _t(np.stack(truths), dev)
    net = pivlfn.Network(model="piv", params=synth.generate_weights("piv", 0)).to(dev).eval()
    fr = [[torch.from_numpy(np.stack([read_image_u8(str(seq / f"{n}_img{j}.png")) for n in part])).to(dev) for j in (1, 2)]
          for part in (names[:2], names[2:])]                                             # the batches of --batch 2
    est = torch.cat([pivlfn.estimate(net, u8_to_input(a), u8_to_input(b), tensor=True) for a, b in fr])

    def check_records(doc, err, names):
        for k, n in enumerate(names):
            cnt = err.n[k].item()
            want = {"n": int(cnt), "aee": err.epe[k].item() / cnt, "rmse": float(np.sqrt(err.sq[k].item() / cnt)),
                    "l1": err.l1[k].item() / cnt / 2.0, "bias_u": err.du[k].item() / cnt, "bias_v": err.dv[k].item() / cnt,
                    "max": err.max[k].item()}
            assert doc["pairs"][n] == want, (n, doc["pairs"][n], want)
        tot = doc["total"]
        assert tot["n"] == int(err.n.sum().item()) and tot["max"] == err.max.max().item()
        s = 0.0
        for v in err.epe.tolist():
            s += v
        assert tot["aee"] == s / tot["n"]

    base = ["--model", "piv", "-i", str(seq), "-p", "--batch", "2"]
    assert runpy.main(base + ["-o", str(tmp_path / "plain")]) == 3
    assert runpy.main(base + ["-o", str(tmp_path / "scored"), "--truth", str(tr)]) == 3
    plain, scored = (tmp_path / d / "piv-synthetic" / "seq" for d in ("plain", "scored"))
    for n in names:
        data = open(scored / "flow" / f"{n}_out.flo", "rb").read()
        assert data == open(plain / "flow" / f"{n}_out.flo", "rb").read()
    assert vr_same(read_flow(str(scored / "flow" / "p1_out.flo")), est[1].permute(1, 2, 0).cpu().numpy())
    assert not (plain / "errors.json").exists() and not (plain / "error_maps.npz").exists()
    assert not [ln for ln in open(plain / "args.txt") if ln.startswith("truth")]
    assert [ln for ln in open(scored / "args.txt") if not ln.startswith(("truth", "output"))] == \
        [ln for ln in open(plain / "args.txt") if not ln.startswith("output")]
    err = E.flow_errors(est, truth)
    doc = json.load(open(scored / "errors.json"))
    assert list(doc["pairs"]) == names and "levels" not in doc and "excluded" not in doc
    check_records(doc, err, names)
    assert 0.0 < doc["total"]["aee"] < 50.0
    st = E.ErrorStats(H, W, dev)
    st.update(est, truth)
    npz = np.load(scored / "error_maps.npz")
    assert er.same_bits(npz["acc"], st.acc.cpu().numpy()) and int(npz["frames"]) == 3 and npz["bias_u"].shape == (H, W)
    assert npz["bias_u"].dtype == np.float32 and npz["count"].dtype == np.int32 and int(npz["count"].max()) == 3
    assert np.array_equal(npz["bias_u"], st.result()["bias_u"].astype(np.float32), equal_nan=True)

    # --validate mask: the raw flows scored with the flags as the mask
    params = dict(radius=2, spacing=1, eps=0.01, thresh=0.5)
    cli = ["--validate-radius", "2", "--validate-eps", "0.01", "--validate-thresh", "0.5"]
    assert runpy.main(base + ["-o", str(tmp_path / "masked"), "--truth", str(tr), "--validate", "mask"] + cli) == 3
    masked = tmp_path / "masked" / "piv-synthetic" / "seq"
    val = V.validate_flow(est, mode="mask", **params)
    assert int((val.flag != 0).sum()) > 0
    doc = json.load(open(masked / "errors.json"))
    check_records(doc, E.flow_errors(est, truth, val.flag), names)
    assert doc["validate"] == "mask" and doc["excluded"]["pairs"] == {n: int((val.flag[k] != 0).sum()) for k, n in enumerate(names)}
    assert doc["excluded"]["total"] == int((val.flag != 0).sum()) and doc["total"]["n"] == 3 * H * W - doc["excluded"]["total"]
    assert vr_same(read_flow(str(masked / "flow" / "p0_out.flo")), val.flow[0].permute(1, 2, 0).cpu().numpy())
    # --validate replace: the replaced flow is what is scored
    assert runpy.main(base + ["-o", str(tmp_path / "rep"), "--truth", str(tr), "--validate", "replace"] + cli) == 3
    rep = V.validate_flow(est, mode="replace", **params)
    doc = json.load(open(tmp_path / "rep" / "piv-synthetic" / "seq" / "errors.json"))
    check_records(doc, E.flow_errors(rep.flow, truth), names)
    assert "excluded" not in doc

    # --truth-levels: the table of the same forward, the flows unchanged
    assert runpy.main(base + ["-o", str(tmp_path / "lv"), "--truth", str(tr), "--truth-levels"]) == 3
    lv = tmp_path / "lv" / "piv-synthetic" / "seq"
    for n in names:
        assert open(lv / "flow" / f"{n}_out.flo", "rb").read() == open(plain / "flow" / f"{n}_out.flo", "rb").read()
    doc = json.load(open(lv / "errors.json"))
    check_records(doc, err, names)
    tot = None
    for a, b in fr:
        _, levels = net.forward_levels(u8_to_input(a), u8_to_input(b))
        table = E.level_errors(net, levels, truth[:a.size(0)] if tot is None else truth[2:], 0.2)
        for bsum in torch.stack([torch.stack([_sums(e) for e in row], dim=1) for row in table], dim=1):
            tot = bsum.clone() if tot is None else tot + bsum
    want = (tot[:, :, 2] / tot[:, :, 0]).tolist()
    assert doc["levels"]["levels"] == [6, 5, 4, 3, 2, 1] and doc["levels"]["stages"] == ["M", "S", "R"] and doc["levels"]["div_flow"] == 0.2
    assert doc["levels"]["aee_level_units"] == want and doc["levels"]["aee_px"] == [[v / 0.2 for v in row] for row in want]
    # the finest level's last stage is the flow itself, in level units
    assert abs(doc["levels"]["aee_px"][5][2] - doc["total"]["aee"]) < 1e-5 * doc["total"]["aee"]


def vr_same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_run_py_truth_two_ranks(tmp_path, dev):
    """run.py --truth launched as two ranks (fresh child processes, RANK / WORLD_SIZE in the environment, gloo for the exchange): the
    same errors.json as one process, byte for byte, and the same accumulators in error_maps.npz."""
    import socket
    import subprocess
    import sys
    import PIL.Image
    seq, tr = tmp_path / "seq", tmp_path / "truth"
    seq.mkdir()
    tr.mkdir()
    for k in range(6):
        a, _, true = synth.particle_pair(64, 64, 700 + k)
        PIL.Image.fromarray(a).save(str(seq / f"f_{k:03d}.png"))
        if k < 5:
            write_flow(np.ascontiguousarray(true.transpose(1, 2, 0)), str(tr / f"f_{k:03d}_flow.flo"))
    run_py = os.path.join(ROOT, "piv_liteflownet-pytorch_amd", "run.py")

    def launch(out, world):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        cmd = [sys.executable, run_py, "-m", "piv", "-i", str(seq), "-o", str(out), "--batch", "2", "--truth", str(tr), "--truth-levels"]
        procs = [subprocess.Popen(cmd, env=dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                                                MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0"),
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT) for r in range(world)]
        outs = []
        for p in procs:
            try:
                o, e = p.communicate(timeout=300)
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                raise
            outs.append((p.returncode, o, e))
        for rc, o, e in outs:
            assert rc == 0, f"child failed rc={rc}\nstdout:\n{o[-2000:]}\nstderr:\n{e[-4000:]}"
        return out / "piv-synthetic" / "seq"

    one, two = launch(tmp_path / "one", 1), launch(tmp_path / "two", 2)
    doc = json.load(open(one / "errors.json"))
    assert list(doc["pairs"]) == [f"f_{k:03d}" for k in range(5)] and len(doc["levels"]["aee_px"]) == 6
    assert open(one / "errors.json", "rb").read() == open(two / "errors.json", "rb").read()
    a, b = np.load(one / "error_maps.npz"), np.load(two / "error_maps.npz")
    assert int(a["frames"]) == int(b["frames"]) == 5
    # per pixel the two ranks' sums are added once more (rank order) where one process adds frame by frame: the counts are equal,
    # the sums agree to rounding
    assert np.array_equal(a["count"], b["count"]) and np.allclose(a["acc"], b["acc"], rtol=1e-14, atol=0)
