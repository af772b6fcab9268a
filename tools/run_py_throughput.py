#!/usr/bin/env python3
"""End-to-end rate of run.py on a folder of PNG frames (decode -> H2D -> estimate -> D2H -> .flo): N2/N1 of SURVEY section 8(f).
  python tools/run_py_throughput.py [frames] [size] [--truth] [--color] [--vort-image]
--color / --vort-image: every pair also gets its picture (main_dl's `viz`: coloured on the device, written as PNG on background
threads); their cost is the difference to a run without them.
--truth: every pair also has a truth file (<frame>_flow.flo, 8 bytes per pixel) that run.py reads and scores on the device
(main_dl's `truth`): the cost of --truth is the difference to a run without it; the part of it spent after the last pair, on
errors.json and error_maps.npz (run.py's finish_truth), is timed and printed beside the rate."""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "piv_liteflownet-pytorch_amd"))
import PIL.Image
import torch

import run as runpy
from pivlfn import synth

with_truth = "--truth" in sys.argv
pictures = [a for a in ("--color", "--vort-image") if a in sys.argv]
argv = [a for a in sys.argv[1:] if a not in ("--truth", "--color", "--vort-image")]
n = int(argv[0]) if len(argv) > 0 else 33
S = int(argv[1]) if len(argv) > 1 else 1024
d = tempfile.mkdtemp(prefix="seq_")
fr = synth.ParticleSequence(S, S, seed=3, device="cuda:0").frames(0, n).cpu().numpy()
for k in range(n):
    PIL.Image.fromarray(fr[k]).save(os.path.join(d, f"frame_{k:05d}.png"))
out = tempfile.mkdtemp(prefix="flo_")
truth = None
if with_truth:
    from pivlfn.flo import write_flow
    tdir = tempfile.mkdtemp(prefix="truth_")
    field = torch.randn(S, S, 2, generator=torch.Generator().manual_seed(3)).numpy()
    for k in range(n - 1):
        write_flow(field, os.path.join(tdir, f"frame_{k:05d}_flow.flo"))
    truth = (tdir, False, os.path.join(out, "errors.json"), os.path.join(out, "error_maps.npz"))
kw = dict(truth=truth) if with_truth else {}
if pictures:
    kw["viz"] = dict(color="--color" in pictures, color_max=None, color_wheel=None, vort_image="--vort-image" in pictures, vort_max=None,
                     quiver=None)
finish_s = [0.0]
if with_truth:
    _finish = runpy.finish_truth

    def timed_finish(*a, **k):
        t = time.perf_counter()
        _finish(*a, **k)
        finish_s[0] = time.perf_counter() - t
    runpy.finish_truth = timed_finish
dev = torch.device("cuda:0")
net = runpy.Network(model="piv", params=synth.generate_weights("piv", 0)).to(dev).eval()
for precision in ("fp32", "fp16"):
    net.precision = precision
    for batch in (1, 4):
        runpy.main_dl(net, d, out, False, 0, 5, dev, batch, **kw)               # warm-up (workspace, caches)
        t0 = time.perf_counter()
        pairs = runpy.main_dl(net, d, out, False, 0, -1, dev, batch, **kw)      # run.py's per-directory loop (run.py:137-168)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"run.py main_dl{' --truth' if with_truth else ''}{''.join(' ' + p for p in pictures)} {S}x{S} PNG sequence, {pairs} pairs, --batch {batch}, {precision}: {dt:.2f} s = {pairs / dt:.1f} pairs/s "
              f"end to end (PNG decode -> H2D -> estimate -> D2H -> .flo{' and .png' if pictures else ''} files closed)"
              + (f"; of it {finish_s[0]:.3f} s after the last pair (errors.json, error_maps.npz)" if with_truth else ""), flush=True)
