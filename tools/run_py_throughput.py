#!/usr/bin/env python3
"""End-to-end rate of run.py on a folder of PNG frames (decode -> H2D -> estimate -> D2H -> .flo): N2/N1 of SURVEY section 8(f).
  python tools/run_py_throughput.py [frames] [size] [--truth] [--color] [--vort-image]
--color / --vort-image: every pair also gets its picture (run.py's Pictures stage: coloured on the device, written as PNG on
background threads); their cost is the difference to a run without them.
--truth: every pair also has a truth file (<frame>_flow.flo, 8 bytes per pixel) that run.py reads and scores on the device
(run.py's Truth stage): the cost of --truth is the difference to a run without it; the part of it spent after the last pair, on
errors.json and error_maps.npz (the stage's finish), is timed and printed beside the rate."""
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
tdir = None
if with_truth:
    from pivlfn.flo import write_flow
    tdir = tempfile.mkdtemp(prefix="truth_")
    field = torch.randn(S, S, 2, generator=torch.Generator().manual_seed(3)).numpy()
    for k in range(n - 1):
        write_flow(field, os.path.join(tdir, f"frame_{k:05d}_flow.flo"))
lay = runpy.OutputLayout(save=out, flow=out, args_file=os.path.join(out, "args.txt"))
finish_s = [0.0]


class TimedTruth(runpy.Truth):
    def finish(self, names, ctx):
        t = time.perf_counter()
        super().finish(names, ctx)
        finish_s[0] = time.perf_counter() - t


def stages(frames):
    """The stages of one main_dl call over the first `frames` frames (-1: all of them)."""
    made = []
    if with_truth:
        paths = runpy.truth_files(runpy.Run(root=d, is_pair=False, n_images=frames, start_at=0), tdir)
        made.append(TimedTruth(net, paths, False, lay.sibling("errors.json"), lay.sibling("error_maps.npz"), pin=True))
    if pictures:
        made.append(runpy.Pictures("--color" in pictures, None, None, "--vort-image" in pictures, None, None))
    return made


dev = torch.device("cuda:0")
net = runpy.Network(model="piv", params=synth.generate_weights("piv", 0)).to(dev).eval()
for precision in ("fp32", "fp16"):
    net.precision = precision
    for batch in (1, 4):
        runpy.main_dl(net, d, lay, False, 0, 5, dev, batch, stages=stages(5))               # warm-up (workspace, caches)
        t0 = time.perf_counter()
        pairs = runpy.main_dl(net, d, lay, False, 0, -1, dev, batch, stages=stages(-1))      # run.py's per-directory loop (run.py:137-168)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"run.py main_dl{' --truth' if with_truth else ''}{''.join(' ' + p for p in pictures)} {S}x{S} PNG sequence, {pairs} pairs, --batch {batch}, {precision}: {dt:.2f} s = {pairs / dt:.1f} pairs/s "
              f"end to end (PNG decode -> H2D -> estimate -> D2H -> .flo{' and .png' if pictures else ''} files closed)"
              + (f"; of it {finish_s[0]:.3f} s after the last pair (errors.json, error_maps.npz)" if with_truth else ""), flush=True)
