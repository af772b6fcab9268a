"""GPU: every workload of BASELINE.json `configs` at its own size (or, for the 8-GPU ones, the per-GPU share and a miniature
of the multi-rank control flow), checked against the oracle / against size-independent properties.

  configs[0]  run.py --model hui on two 256x256 particle images                    -> test_config0_*
  configs[1]  PIV forward, batch 1, 1024x1024 fp32                                 -> tests/test_gpu_net.py::test_full_size_1024_properties, bench.py
  configs[2]  batch 32 x 512x512                                                   -> test_config2_*
  configs[3]  10 000-frame 1024x1024 sequence sharded over 8 GPUs                  -> test_config3_* (9 frames, 1 rank + 2-rank gloo rehearsal)
  configs[4]  fp16 activations / fp32 accumulate, batch 64 x 1024x1024 over 8 GPUs -> test_config4_* (the per-GPU share: 8 x 1024x1024)
"""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import pivlfn
import pivlfn_oracle as orc
from pivlfn import synth
from pivlfn.flo import read_flow

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
E2E_MAX, E2E_MEAN = 1e-4, 1e-5          # fp32 end-to-end tolerance, relative to max(1, max|flow|)


def _check(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(1.0, np.abs(want).max())
    err = np.abs(got - want)
    assert err.max() <= E2E_MAX * scale, f"{what}: max-abs {err.max():.3e} at flow scale {scale:.2f}"
    assert err.mean() <= E2E_MEAN * scale, f"{what}: mean-abs {err.mean():.3e}"


# ---- configs[0] ---------------------------------------------------------------------------------------------------
def test_config0_run_py_hui_256_pair(tmp_path, dev):
    """`run.py --model hui -p` on 256x256 pairs: one synthetic particle pair and the reference's own demo pair
    (tests/golden/DNS_turbulence_img{1,2}.tif, grey TIFFs) -> .flo files against the oracle's estimate() on the CPU."""
    import PIL.Image
    import run as runpy
    d = tmp_path / "pairs"
    d.mkdir()
    a, b, _ = synth.particle_pair(256, 256, 4242)
    PIL.Image.fromarray(a).save(str(d / "synthetic_img1.png"))
    PIL.Image.fromarray(b).save(str(d / "synthetic_img2.png"))
    for k in (1, 2):
        with open(os.path.join(GOLDEN, f"DNS_turbulence_img{k}.tif"), "rb") as src, open(str(d / f"DNS_turbulence_img{k}.tif"), "wb") as dst:
            dst.write(src.read())
    out = tmp_path / "out"
    assert runpy.main(["--model", "hui", "-p", "-i", str(d), "-o", str(out), "--batch", "1"]) == 2
    flodir = out / "hui-synthetic" / "pairs" / "flow"
    assert sorted(os.listdir(flodir)) == ["DNS_turbulence_out.flo", "synthetic_out.flo"]
    onet = orc.make_net("hui", synth.generate_weights("hui", 0), corr="c")
    for name, ext in (("synthetic", "png"), ("DNS_turbulence", "tif")):
        ims = [np.asarray(PIL.Image.open(str(d / f"{name}_img{k}.{ext}")).convert("RGB"), dtype=np.uint8) for k in (1, 2)]
        x = [torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1))).float().div_(255.0)[None] for im in ims]
        with torch.no_grad():
            want = orc.estimate(onet, x[0], x[1], tensor=False)
        got = read_flow(str(flodir / f"{name}_out.flo"))
        assert got.shape == (256, 256, 2)
        _check(got, want, f"run.py hui {name}")
        assert np.abs(want).max() > 0.5                             # the pair does carry a flow


def test_config0_run_py_brightness_contrast(tmp_path, dev):
    """`run.py -b 1.0 1.5 -c 0.75` (reference main(), run.py:100-134): one .flo per consecutive pair and combination, named
    <prefix>_<BBB>_<CCC>_<suffix>_out.flo, equal to Inference.parser on PIL images enhanced the way the reference does."""
    import PIL.Image
    import PIL.ImageEnhance
    import run as runpy
    seq = tmp_path / "seq"
    seq.mkdir()
    frames = []
    for k in range(3):
        a, _, _ = synth.particle_pair(64, 96, 900 + k)
        frames.append(a)
        PIL.Image.fromarray(a).save(str(seq / f"cam_{k:04d}.png"))
    out = tmp_path / "out"
    n = runpy.main(["-m", "piv", "-i", str(seq), "-o", str(out), "-b", "1.0", "1.5", "-c", "0.75", "--batch", "2"])
    assert n == 2 * 2
    flodir = out / "piv-synthetic" / "seq" / "flow"
    assert sorted(os.listdir(flodir)) == ["cam_100_075_0000_out.flo", "cam_100_075_0001_out.flo",
                                          "cam_150_075_0000_out.flo", "cam_150_075_0001_out.flo"]
    net = pivlfn.piv_liteflownet(synth.generate_weights("piv", 0)).to(dev).eval()

    def enhanced(arr, b, c):
        im = PIL.Image.fromarray(arr).convert("RGB")
        return PIL.ImageEnhance.Contrast(PIL.ImageEnhance.Brightness(im).enhance(b)).enhance(c)
    for b in (1.0, 1.5):
        for k in range(2):
            want = pivlfn.Inference.parser(net, enhanced(frames[k], b, 0.75), enhanced(frames[k + 1], b, 0.75), device=dev)
            got = read_flow(str(flodir / f"cam_{int(b * 100):03d}_075_{k:04d}_out.flo"))
            assert np.array_equal(got, want), (b, k)


# ---- configs[2] ---------------------------------------------------------------------------------------------------
def test_config2_batch32_512(dev):
    """32 pairs of 512x512 in one forward: every pair equals its single-pair flow bit for bit (nothing in the path may depend
    on the batch mates: per-image split-K rule, one summation order in both warp+correlation kernels), and two of them are
    checked against the oracle on the CPU."""
    B, S = 32, 512
    a, b = synth.particle_batch(B, S, S, seed=2024)
    i1, i2 = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    net = pivlfn.piv_liteflownet(synth.generate_weights("piv", 0)).to(dev).eval()
    lib_bytes = pivlfn._lib.load().pivlfn_workspace_bytes(net._native(), B, S, S)
    full = net(i1, i2)
    assert net._ws.numel() == lib_bytes                           # the workspace query is what the forward was given
    assert tuple(full.shape) == (B, 2, S, S) and torch.isfinite(full).all()
    for k in range(B):
        one = net(i1[k:k + 1], i2[k:k + 1])
        assert torch.equal(one[0], full[k]), f"pair {k} depends on its batch mates"
    onet = orc.make_net("piv", synth.generate_weights("piv", 0), corr="c")
    for k in (0, 17):
        with torch.no_grad():
            want = onet.forward(torch.from_numpy(a[k:k + 1]), torch.from_numpy(b[k:k + 1])).numpy()
        _check(full[k:k + 1].cpu().numpy(), want, f"batch-32 pair {k}")


# ---- configs[3] ---------------------------------------------------------------------------------------------------
def _sequence_reference(dev, n_frames, S, seed):
    """estimate() pair by pair on the frames run_sequence renders."""
    net = pivlfn.piv_liteflownet(synth.generate_weights("piv", 0)).to(dev).eval()
    fr = synth.ParticleSequence(S, S, seed=seed, device=dev).frames(0, n_frames)
    from pivlfn.sequence import frames_to_input
    x = frames_to_input(fr)          # the LUT conversion of run.py's input path (bit-identical to ToTensor)
    return net, [pivlfn.estimate(net, x[k:k + 1], x[k + 1:k + 2], tensor=False) for k in range(n_frames - 1)]


def test_config3_sequence_miniature_one_rank(tmp_path, dev):
    """9 frames of 1024x1024, chunks of 4 pairs, one rank: 8 .flo files, bit-equal to estimate() on each pair."""
    from pivlfn.sequence import flow_file_name, run_sequence
    n_frames, S = 9, 1024
    net, want = _sequence_reference(dev, n_frames, S, seed=99)
    seq = synth.ParticleSequence(S, S, seed=99, device=dev)
    st = run_sequence(net, seq.frames, n_frames, 4, dev, write_dir=str(tmp_path / "flow"))
    assert st["pairs_total"] == 8 and st["flows_emitted"] == 8
    assert sorted(os.listdir(tmp_path / "flow")) == [flow_file_name(k) for k in range(8)]
    for k in range(8):
        got = read_flow(str(tmp_path / "flow" / flow_file_name(k)))
        assert got.shape == (S, S, 2) and np.array_equal(got, want[k]), f"pair {k}"
    assert np.abs(want[0]).max() > 1.0


def _run_children(cmd_for_rank, world, env_extra, timeout=900):
    """Fresh child processes, one per rank (never an exec of this GPU-initialised process)."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", **env_extra)
        procs.append(subprocess.Popen(cmd_for_rank(r), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT))
    outs = []
    for p in procs:
        try:
            o, e = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append((p.returncode, o, e))
    for rc, o, e in outs:
        assert rc == 0, f"child failed rc={rc}\nstdout:\n{o[-2000:]}\nstderr:\n{e[-4000:]}"
    return outs


def test_config3_sequence_two_rank_rehearsal(tmp_path, dev):
    """The 2-rank control flow of config #4 on one GPU (gloo instead of RCCL, both ranks on device 0): contiguous shards, halo
    frame, per-chunk all-gather, rank 0 writes -- the same .flo set, bit for bit, as estimate() pair by pair, and the pairs at the
    shard boundary within the end-to-end tolerance of the CPU oracle."""
    from pivlfn.sequence import flow_file_name
    n_frames, S = 8, 512                                            # 7 pairs: shards of 4 and 3, chunk 3 -> a short last chunk
    outdir = tmp_path / "flow2"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "sequence_run.py"), "--frames", str(n_frames), "--size", str(S), "--chunk", "3",
           "--write", str(outdir), "--seed", "7"]
    outs = _run_children(lambda r: cmd, 2, {"PIVLFN_BENCH_BACKEND": "gloo"})
    line = json.loads([ln for ln in outs[0][1].splitlines() if ln.startswith("{")][-1])
    assert line["flo_files_written"] == 7
    _, want = _sequence_reference(dev, n_frames, S, seed=7)
    assert sorted(os.listdir(outdir)) == [flow_file_name(k) for k in range(7)]
    for k in range(7):
        assert np.array_equal(read_flow(str(outdir / flow_file_name(k))), want[k]), f"pair {k}"
    # ... and not only equal to the library's own estimate(): the two pairs either side of the shard boundary (pair 3 is rank 0's
    # last, pair 4 is rank 1's first and starts at its halo frame) against the oracle's estimate() on the CPU, from the same frames
    from pivlfn.sequence import frames_to_input
    x = frames_to_input(synth.ParticleSequence(S, S, seed=7, device=dev).frames(3, 6)).cpu()
    onet = orc.make_net("piv", synth.generate_weights("piv", 0), corr="c")
    for j, k in enumerate((3, 4)):
        with torch.no_grad():
            ow = orc.estimate(onet, x[j:j + 1], x[j + 1:j + 2], tensor=False)
        _check(read_flow(str(outdir / flow_file_name(k))), ow, f"2-rank sequence pair {k} vs oracle")


def test_bench_py_two_rank_rehearsal(dev):
    """bench.py's N>1 path (barrier, max over ranks, async gather, one JSON line from rank 0) rehearsed with gloo as two fresh
    child processes on this one GPU, at a small size."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--size", "256", "--no-cpu-baseline"]
    outs = _run_children(lambda r: cmd, 2, {"PIVLFN_BENCH_BACKEND": "gloo"})
    lines = [ln for ln in outs[0][1].splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and not [ln for ln in outs[1][1].splitlines() if ln.startswith("{")]      # rank 0 only
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["steps"] == 3 and j["scaling"] == "weak" and j["unit"] == "image-pairs/s"
    assert j["value"] > 0 and len(j["per_rank"]) == 2
    assert abs(j["value"] - 2 * 3 / (j["ms_per_step"] * 3e-3)) / j["value"] < 0.01                  # value = all ranks' pairs / max time


def test_bench_py_dumps_what_the_timed_path_computed(dev, tmp_path):
    """A plain `bench.py --dump-outputs DIR` run: one JSON line with the headline fields and none of the --full extras, and
    DIR/flow.npy holds the last timed step's flows bit for bit -- the same forward run here on the same seeded inputs."""
    S = 256
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--size", str(S),
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    j = lines[0]
    assert j["steps"] == 3 and j["ms_per_step"] > 0 and j["unit"] == "image-pairs/s" and j["higher_is_better"] is True
    assert j["cpu_baseline"] is None and not {"arithmetic", "roofline_batch8", "roofline_conv", "roofline_level1"} & set(j)
    assert os.listdir(tmp_path / "out") == ["flow.npy"]
    got = np.load(tmp_path / "out" / "flow.npy")
    a, b = synth.particle_batch(1, S, S, seed=1234)
    net = pivlfn.Network(model="piv", params=synth.generate_weights("piv", 0)).to(dev).eval()
    want = net(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (1, 2, S, S) and np.array_equal(got, want)
    assert np.abs(want).max() > 0.5


def test_config3_one_ranks_share_at_length(dev):
    """A whole per-rank share of BASELINE configs[3] on one GPU: 1 251 frames of 1024 x 1024 (1 250 pairs, 157 chunks of 8) through
    run_sequence with a sink that drops the flows -- the pinned ring, the producer thread and the sink thread over a long run: every
    pair reaches the sink exactly once and in order per chunk, host memory stays flat, and the loop runs at the forward's rate (the
    frames of the next chunk are rendered while the current one is estimated)."""
    import resource
    from pivlfn.sequence import run_sequence
    S, n_frames, chunk = 1024, 1251, 8
    net = pivlfn.piv_liteflownet(synth.generate_weights("piv", 0)).to(dev).eval()
    seq = synth.ParticleSequence(S, S, seed=7, device=dev)
    got = []
    rss = []

    def sink(gi, flow):
        got.append(gi)
        assert flow.shape == (S, S, 2)
        if gi % 200 == 0:
            rss.append(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss)
    st = run_sequence(net, seq.frames, n_frames, chunk, dev, sink=sink)
    assert got == list(range(n_frames - 1)) and st["flows_emitted"] == n_frames - 1
    assert rss[-1] - rss[1] < 200 * 1024, rss          # KiB: no growth with the number of chunks once the ring is allocated
    rate = (n_frames - 1) / st["seconds"]
    est = (n_frames - 1) / st["seconds_estimation"]
    print(f"1250 pairs: {rate:.1f} pairs/s whole loop, {est:.1f} pairs/s in the estimation")
    assert rate > 0.8 * est, (rate, est)


def test_bench_py_starts_its_own_ranks(dev):
    """The plain command `python bench.py --gpus 2` with no outer launcher and no RANK / WORLD_SIZE in the environment: the parent
    starts two fresh ranks itself (gloo here: one GPU) and relays rank 0's single JSON line; asking for more devices than are
    visible with the RCCL backend is refused before anything is started."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--size", "256", "--no-cpu-baseline",
           "--no-arithmetic", "--lean"]
    r = subprocess.run(cmd, env=dict(env, PIVLFN_BENCH_BACKEND="gloo"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{") and "metric" in ln]
    assert len(lines) == 1
    j = lines[0]
    assert j["n_gpus"] == 2 and len(j["per_rank"]) == 2 and j["value"] > 0
    # what the backend saw, and where every rank ran
    assert j["backend_world_size"] == 2
    assert all("device_index" in e and e["device_name"] for e in j["per_rank"])
    if torch.cuda.device_count() < 2:
        r = subprocess.run(cmd, env=dict(env, PIVLFN_BENCH_BACKEND="nccl"), capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "device(s) visible" in r.stderr and not r.stdout.strip()


def test_bench_py_supervises_its_ranks(dev):
    """A rank that dies before the rendezvous (PIVLFN_BENCH_FAIL_RANK=1: rank 1 exits 3) does not leave rank 0 sitting in
    init_process_group: the parent notices, stops the other rank, names the dead one with its stderr and returns non-zero within
    seconds -- no JSON line, no retry."""
    import time
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--size", "256", "--no-cpu-baseline",
           "--no-arithmetic", "--lean"]
    t0 = time.monotonic()
    r = subprocess.run(cmd, env=dict(env, PIVLFN_BENCH_BACKEND="gloo", PIVLFN_BENCH_FAIL_RANK="1"), capture_output=True, text=True, timeout=120)
    took = time.monotonic() - t0
    assert r.returncode != 0
    assert took < 30, took
    assert "rank 1 exited with code 3" in r.stderr and "exits 3 on request" in r.stderr, r.stderr[-1500:]
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{") and "metric" in ln]


def test_rccl_branch_executes_on_one_rank(dev, tmp_path):
    """The `nccl` (= RCCL) code paths, which the gloo rehearsals replace, executed for real in a fresh child with a process group
    of one rank on this one GPU: bench.py's init_process_group("nccl", device_id=...) + asynchronous all_gather_into_tensor +
    barrier + all_reduce(MAX), and pivlfn.dist.gather_flows on device tensors (synchronous and asynchronous)."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--size", "256", "--no-cpu-baseline",
           "--no-arithmetic"]
    outs = _run_children(lambda r: cmd, 1, {"PIVLFN_BENCH_FORCE_DIST": "1", "PIVLFN_BENCH_BACKEND": "nccl"})
    lines = [json.loads(ln) for ln in outs[0][1].splitlines() if ln.startswith("{")]
    main = [j for j in lines if "metric" in j]
    forced = [j for j in lines if j.get("forced_dist")]
    assert len(main) == 1 and len(forced) == 1
    assert forced[0]["backend"] == "nccl" and forced[0]["gathered_equals_flow"] is True
    j = main[0]
    assert j["n_gpus"] == 1 and j["value"] > 0 and len(j["per_rank"]) == 1
    # the rank's own rate is timed after its stream has drained: the same thing as `value` on one rank (not the host's enqueue rate)
    assert abs(j["per_rank"][0]["pairs_per_s"] - j["value"]) / j["value"] < 0.2, (j["per_rank"], j["value"])
    script = tmp_path / "gather_nccl.py"
    script.write_text(
        "import os, sys, torch, torch.distributed as dist\n"
        f"sys.path.insert(0, {os.path.join(ROOT, 'piv_liteflownet-pytorch_amd')!r})\n"
        "from pivlfn.dist import gather_flows\n"
        "torch.cuda.set_device(0)\n"
        "dev = torch.device('cuda', 0)\n"
        "dist.init_process_group('nccl', device_id=dev)\n"
        "x = torch.randn(3, 2, 64, 96, device=dev)\n"
        "full = gather_flows(x, 3)\n"
        "work, finish = gather_flows(x * 2, 3, async_op=True)\n"
        "y = finish()\n"
        "torch.cuda.synchronize()\n"
        "ok = torch.equal(full, x) and torch.equal(y, x * 2) and full.is_cuda and dist.get_backend() == 'nccl'\n"
        "dist.destroy_process_group()\n"
        "print('GATHER_OK' if ok else 'GATHER_BAD')\n")
    outs = _run_children(lambda r: [sys.executable, str(script)], 1, {})
    assert "GATHER_OK" in outs[0][1], outs[0]


def test_real_weights_file_through_run_py(tmp_path, dev):
    """run.py --weights on a state-dict FILE (reference: run.py:71-83 `get_weights` = torch.load of a .paramOnly, :217-226): a seeded
    state dict is written with torch.save under the reference's file name, run.py loads it and estimates the reference's own demo
    pair; the .flo equals estimate() with the same weights loaded in memory.  Also records the largest activation magnitude of
    every layer on that pair (from the CPU oracle): the head-room of the opt-in split modes, whose inputs must stay below 65504."""
    import shutil
    wts = synth.generate_weights("piv", 0)
    wfile = tmp_path / "PIV-LiteFlowNet-en.paramOnly"
    torch.save(wts, str(wfile))
    indir = tmp_path / "demo"
    indir.mkdir()
    for k in (1, 2):
        shutil.copy(os.path.join(ROOT, "tests", "golden", f"DNS_turbulence_img{k}.tif"), indir / f"DNS_turbulence_img{k}.tif")
    outdir = tmp_path / "out"
    rc = subprocess.run([sys.executable, os.path.join(ROOT, "piv_liteflownet-pytorch_amd", "run.py"), "--model", "piv", "-p", "-i", str(indir),
                         "-o", str(outdir), "--weights", str(wfile)], capture_output=True, text=True, cwd=ROOT)
    assert rc.returncode == 0, rc.stderr[-3000:]
    flos = [os.path.join(d, f) for d, _, fs in os.walk(outdir) for f in fs if f.endswith(".flo")]
    assert len(flos) == 1
    got = read_flow(flos[0])
    from pivlfn.pipeline import read_image_u8 as _rd, u8_to_input
    a = torch.from_numpy(_rd(str(indir / "DNS_turbulence_img1.tif")))[None]
    b = torch.from_numpy(_rd(str(indir / "DNS_turbulence_img2.tif")))[None]
    net = pivlfn.piv_liteflownet(torch.load(str(wfile))).to(dev).eval()
    want = pivlfn.estimate(net, u8_to_input(a.to(dev)), u8_to_input(b.to(dev)), tensor=False)
    assert got.shape == (256, 256, 2) and np.array_equal(got, want)
    # per-layer activation range on this pair (oracle = CPU restatement of the reference's forward, test infrastructure)
    from unittest import mock
    onet = orc.make_net("piv", wts, corr="c")
    peaks = []
    real_conv2d = orc.F.conv2d

    def spy(x, *a, **k):
        peaks.append(float(x.abs().max()))           # what a convolution layer is fed
        return real_conv2d(x, *a, **k)
    with mock.patch.object(orc.F, "conv2d", spy), torch.no_grad():
        onet.forward(u8_to_input(a), u8_to_input(b))
    top = max(peaks) if peaks else 0.0
    print(f"largest |input| over {len(peaks)} convolution calls on the demo pair: {top:.3g} (fp16 range of the split modes' leading piece: 65504)")
    assert peaks and top < 65504 / 64, "seeded weights leave less than 6 binades of head-room for the opt-in split modes"


# ---- configs[4] ---------------------------------------------------------------------------------------------------
def test_config4_fp16_batch8_1024(dev):
    """The per-GPU share of config #5 (64 x 1024x1024 over 8 GPUs = 8 per GPU) in the fp16-multiplicand mode: finite, the
    workspace query is honoured, and every pair stays within the stated end-point-error bound of the fp32 mode."""
    B, S = 8, 1024
    a, b = synth.particle_batch(B, S, S, seed=5150)
    i1, i2 = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    net = pivlfn.piv_liteflownet(synth.generate_weights("piv", 0)).to(dev).eval()
    f32 = net(i1, i2)
    net.precision = "fp16"
    need = pivlfn._lib.load().pivlfn_workspace_bytes(net._native(), B, S, S)
    f16 = net(i1, i2)
    assert net._ws.numel() >= need and torch.isfinite(f16).all() and tuple(f16.shape) == (B, 2, S, S)
    epe = torch.sqrt(((f16 - f32) ** 2).sum(1))                    # [B,H,W]
    per_pair = epe.flatten(1).mean(1).cpu().numpy()
    print("fp16 mode, 8 x 1024x1024: mean EPE per pair vs fp32 mode:", np.round(per_pair, 5), "max", float(epe.max()))
    assert (per_pair <= 0.05).all() and float(epe.max()) <= 0.5
    assert not torch.equal(f16, f32)
    one = net(i1[3:4], i2[3:4])
    assert torch.equal(one[0], f16[3])                              # batch-independent in this mode too
    # a workspace that is too small is refused, not overrun
    lib = pivlfn._lib.load()
    small = torch.empty(1024, dtype=torch.uint8, device=dev)
    out = torch.empty(B, 2, S, S, device=dev)
    rc = lib.pivlfn_forward(net._native(), i1.data_ptr(), i2.data_ptr(), out.data_ptr(), None, B, S, S, small.data_ptr(), small.numel(),
                            torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 3 and b"workspace" in lib.pivlfn_last_error()


# ---- boundary: re-entrancy ------------------------------------------------------------------------------------------
def test_two_nets_two_threads_two_streams(dev):
    """The library keeps no process-global mutable state: two handles driven from two threads on two streams give the flows a
    single-threaded run gives, bit for bit (include/pivlfn.h; SURVEY.md section 8(b) 'Threading / streams')."""
    wts = synth.generate_weights("piv", 0)
    nets = [pivlfn.piv_liteflownet(wts).to(dev).eval() for _ in range(2)]
    pairs = []
    for t in range(2):
        a, b = synth.particle_batch(1, 256, 320, seed=60 + t)
        pairs.append((torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)))
    want = [nets[0](*pairs[t]).clone() for t in range(2)]
    torch.cuda.synchronize()
    got = [None, None]
    errs = []

    def work(t):
        try:
            s = torch.cuda.Stream(dev)
            with torch.cuda.stream(s):
                for _ in range(6):
                    f = nets[t](*pairs[t])
                s.synchronize()
            got[t] = f
        except Exception as e:          # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    for t in range(2):
        assert torch.equal(got[t], want[t])


# ---- run.py sharded over ranks, Inference.images_parsing -----------------------------------------------------------------
def test_run_py_two_ranks_write_disjoint_shards(tmp_path, dev):
    """`torch.distributed.run`-style launch of run.py (RANK / WORLD_SIZE in the environment): every rank estimates and writes
    its contiguous shard of the folder's pairs; together the files are exactly the single-process result."""
    import PIL.Image
    seq = tmp_path / "seq"
    seq.mkdir()
    for k in range(6):
        a, _, _ = synth.particle_pair(64, 64, 700 + k)
        PIL.Image.fromarray(a).save(str(seq / f"f_{k:03d}.png"))
    run_py = os.path.join(ROOT, "piv_liteflownet-pytorch_amd", "run.py")
    one = tmp_path / "one"
    two = tmp_path / "two"
    _run_children(lambda r: [sys.executable, run_py, "-m", "piv", "-i", str(seq), "-o", str(one), "--batch", "2"], 1, {})
    outs = _run_children(lambda r: [sys.executable, run_py, "-m", "piv", "-i", str(seq), "-o", str(two), "--batch", "2"], 2, {})
    assert "Processing 3 of 5 pairs" in outs[0][1] and "Processing 2 of 5 pairs" in outs[1][1]
    d1, d2 = one / "piv-synthetic" / "seq" / "flow", two / "piv-synthetic" / "seq" / "flow"
    names = sorted(os.listdir(d1))
    assert names == [f"f_{k:03d}_out.flo" for k in range(5)] and sorted(os.listdir(d2)) == names
    for n in names:
        assert open(d1 / n, "rb").read() == open(d2 / n, "rb").read()


def test_inference_images_parsing(tmp_path, dev):
    """`Inference(net, ...).images_parsing(dir, pair)` (inference.py:120-171): paired folder -> <out>/<net>/<dir>_parse/*.flo."""
    import PIL.Image
    d = tmp_path / "shots"
    d.mkdir()
    a, b, _ = synth.particle_pair(64, 96, 811)
    PIL.Image.fromarray(a).save(str(d / "s0_img1.png"))
    PIL.Image.fromarray(b).save(str(d / "s0_img2.png"))
    PIL.Image.fromarray(a).save(str(d / "lonely_img1.png"))          # no partner: skipped
    net = pivlfn.piv_liteflownet(synth.generate_weights("piv", 0)).to(dev).eval()
    inf = pivlfn.Inference(net, netname="weights/PIV-x.paramOnly", output_dir=str(tmp_path / "out"), device=dev)
    flows = inf.images_parsing(str(d), pair=True)
    assert len(flows) == 1 and flows[0].shape == (64, 96, 2)
    got = read_flow(str(tmp_path / "out" / "PIV-x" / "shots_parse" / "s0_out.flo"))
    want = pivlfn.estimate(net, torch.from_numpy(synth.to_input(a))[None].to(dev), torch.from_numpy(synth.to_input(b))[None].to(dev))
    assert np.array_equal(got, want) and np.array_equal(flows[0], want)
