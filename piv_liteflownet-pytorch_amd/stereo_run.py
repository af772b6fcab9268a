#!/usr/bin/env python3
"""Counterpart of the reference's stereo_run.py on the HIP path: stereoscopic PIV, two cameras -> one 2D3C (U, V, W) field.

  python stereo_run.py --coeff C.json [--root SET] [--save DIR] [--theta T [T]] [--alpha A [A]] [--fps N] [--calib M]
                       [--model FILE] [--model-version 1|2] [--inference-mode manual|direct] [--precision P] [--batch S]

Flags of the reference (stereo_run.py:21-38), with its defaults.  Three modes:
  * no --root (flo mode, _flo_process :106-146): every <save>/left/*.flo, sorted, with base = name.rsplit('-', 1)[0], is
    combined with <save>/right/<base>-R_out.flo into <save>/stereo/<base>-S_out.flo.  The layout `run.py -i SET/left -i
    SET/right` writes under OUT/<net>/SET/flow.
  * --root SET, manual (:91-103): every consecutive frame pair of SET/left and SET/right through `estimate`, written to
    <save>/left/<stem>_out.flo and <save>/right/<stem>_out.flo (run.py's sequence naming), then flo mode.  With frames named
    <n>-L.<ext> / <n>-R.<ext> this is the layout flo mode reads.
  * --root SET, direct (:60-88): per batch of `--batch` stereo steps ONE forward of the interleaved left / right pairs,
    the 2D3C kernel in place of estimate()'s output resize, <save>/stereo/<left stem rsplit('_', 1)[0]>_2d3c.flo.
All three produce the same numbers: direct's fused kernel equals the kernel applied to estimate()'s flows bit for bit.
--window-size is accepted and unused, as in the reference.  Relative paths resolve against the working directory.

Differences, all deliberate:
  * direct mode converts --theta / --alpha to radians and negates the left camera's angles as flo mode does (the reference
    hands the degrees to willert unconverted and unsigned: with the default [45, 45] every output is inf / NaN);
  * the right camera's step k is (R_k, R_k+1) (the reference estimates (L_k+1, R_k), stereo_run.py:79);
  * `--inference-mode` is compared with == (the reference's `is "manual"`, :193, selects direct for a mode given on the
    command line); manual mode writes its flows where flo mode looks for them;
  * no file is dropped for having `test` in its path (src/datasets.py:370), and there is no CenterCrop (which swaps width and
    height on non-square frames, :404-425): estimate()'s own size adaptation, so the output grid is the input grid the
    calibration refers to;
  * .flo payloads are float32 (the reference writes willert's float64 array, which its own read_flow cannot read back);
  * the input folders are exactly <root>/left and <root>/right, in any case (the reference takes the first two directories
    os.walk returns); the two cameras must have the same number of frames;
  * the reference chdirs into its own folder at import; here nothing changes the working directory;
  * --model is a state-dict file that must exist, loaded with map_location='cpu'; there is no CPU path.
"""
import argparse
import os
import sys
from typing import List, Optional

import numpy as np
import torch

HERE = os.path.dirname(os.path.realpath(__file__))
sys.path.insert(0, HERE)

from pivlfn import stereo                                # noqa: E402
from pivlfn.flo import FloWriter, flowname_modifier, read_flow, write_flow     # noqa: E402
from pivlfn.pipeline import PairLoader, stream_pairs     # noqa: E402

parser = argparse.ArgumentParser(description="Stereoscopic PIV image processing (MI355X-native path)")
parser.add_argument("--coeff", "-c", type=str, help="mapping coefficient json file path.")
parser.add_argument("--root", "-r", default=None, type=str, help="root directory for series of images (left/ and right/)")
parser.add_argument("--save", "-s", default="./work", type=str, help="directory for saving")
parser.add_argument("--theta", default=[45.0, 45.0], type=float, nargs="+", help="object plane angle (degrees)")
parser.add_argument("--alpha", default=[0.0, 0.0], type=float, nargs="+",
                    help="scheimpflug criterion, image plane angle (degrees)")
parser.add_argument("--window-size", "-ws", default=[1.0, 1.0], type=float, nargs="+",
                    help="Window size in the real length (accepted, unused, as in the reference)")
parser.add_argument("--fps", default=1, type=int, help="camera frame rate (FPS).")
parser.add_argument("--calib", default=None, type=float, help="real length calibration in meters (m).")
parser.add_argument("--model", default="./models/pretrain_torch/PIV-LiteFlowNet-en.paramOnly", type=str,
                    help="model weight parameters to use (state-dict file)")
parser.add_argument("--model-version", default=1, type=int, choices=[1, 2],
                    help="choose which base model version to use, LiteFlowNet or LiteFlowNet2")
parser.add_argument("--inference-mode", default="manual", type=str, choices=["manual", "direct"],
                    help="choose which inference method to use")
parser.add_argument("--precision", type=str, default=None,
                    choices=["fp32", "fp32_wino_mfma32", "fp32_direct", "fp32_split", "fp32_split3", "fp16"],
                    help="how the large convolutions multiply (not a reference flag; see Network.precision)")
parser.add_argument("--batch", type=int, default=2, help="stereo steps per forward (two pairs each; not a reference flag)")


def _require_gpu() -> torch.device:
    if not torch.cuda.is_available():
        raise SystemExit("stereo_run.py: this build has no CPU path; a GPU is required")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    return dev


def _setup(args):
    coeff = stereo.read_coeff(args.coeff) if args.coeff else None
    if coeff is None:
        raise ValueError("stereo_run.py: --coeff is required")
    theta, beta = stereo.angles(args.theta, args.alpha)
    return coeff, stereo.tangents(theta, beta)


def flo_process(args) -> int:
    """_flo_process (stereo_run.py:106-146): stored left / right flows -> <save>/stereo/<base>-S_out.flo."""
    coeff, tans = _setup(args)
    pairs = stereo.flo_pairs(args.save)              # every right file checked before anything is computed
    dev = _require_gpu()
    os.makedirs(os.path.join(args.save, "stereo"), exist_ok=True)
    for lf, rf, out in pairs:
        left, right = read_flow(lf), read_flow(rf)
        if left.shape != right.shape:
            raise ValueError(f"{lf} and {rf} differ in size: {left.shape} vs {right.shape}")
        flow = torch.from_numpy(np.stack([left, right]).transpose(0, 3, 1, 2).copy()).to(dev)     # [2,2,H,W]
        field = stereo.stereo_2d3c(flow, coeff, tans, args.fps, args.calib)
        write_flow(field[0].cpu().numpy(), out)
    print(f"Wrote {len(pairs)} stereo flow fields to {os.path.join(args.save, 'stereo')}")
    return len(pairs)


def _net(args, dev):
    from pivlfn import Network
    if not os.path.isfile(args.model):
        raise ValueError(f"Unknown model params input ({args.model})!")
    params = torch.load(args.model, map_location="cpu")
    net = Network(model="piv", params=params, version=args.model_version).to(dev).eval()
    if args.precision is not None:
        net.precision = args.precision
    return net


def manual_process(args, net, dev, seq: stereo.StereoSequence) -> int:
    """manual_process (stereo_run.py:91-103): each camera's flows to <save>/<side>/<stem>_out.flo, then flo mode."""
    for side in stereo.SIDES:
        cam = seq.camera(side)
        outdir = os.path.join(args.save, side)
        os.makedirs(outdir, exist_ok=True)
        loader = PairLoader(cam, 0, len(cam), 2 * args.batch, depth=2, pin=True)
        try:
            with FloWriter() as writer:
                n = stream_pairs(net, loader, dev,
                                 lambda flow, name, d=outdir: writer.submit(flow, flowname_modifier(name, d, pair=False)))
        finally:
            loader.close()
        assert n == len(cam)
    return flo_process(args)


def direct_process(args, net, dev, seq: stereo.StereoSequence) -> int:
    """direct_process (stereo_run.py:60-88): interleaved forwards, fused 2D3C kernel, <save>/stereo/<name>_2d3c.flo."""
    coeff, tans = _setup(args)
    names = seq.direct_names()                       # a name collision is refused before anything is computed
    outdir = os.path.join(args.save, "stereo")
    os.makedirs(outdir, exist_ok=True)
    step = {seq.name_list[2 * k]: n for k, n in enumerate(names)}

    def est(net_, a, b, tensor=True):
        return stereo.estimate_interleaved(net_, a, b, coeff, tans, args.fps, args.calib)

    loader = PairLoader(seq, 0, len(seq.image_list), 2 * args.batch, depth=2, pin=True, share=2)
    try:
        with FloWriter() as writer:
            n = stream_pairs(net, loader, dev, lambda field, name: writer.submit(field, os.path.join(outdir, step[name])),
                             estimate_fn=est, group=2)
    finally:
        loader.close()
    assert n == seq.steps
    print(f"Wrote {n} stereo flow fields to {outdir}")
    return n


def main(argv: Optional[List[str]] = None) -> int:
    args = parser.parse_args(argv)
    if args.batch < 1:
        raise ValueError("--batch must be >= 1")
    if args.root is None:
        return flo_process(args)
    _setup(args)                                     # a bad --coeff / angle is reported before the network is built
    seq = stereo.StereoSequence(args.root)
    if args.inference_mode == "direct":
        seq.direct_names()
    dev = _require_gpu()
    net = _net(args, dev)
    if args.inference_mode == "manual":
        return manual_process(args, net, dev, seq)
    return direct_process(args, net, dev, seq)


if __name__ == "__main__":
    main()
