"""Synthetic PIV pairs from a known flow, written in the layout run.py -p --truth reads.

Usage:
    generate.py -o OUT (--flow A.flo [B.flo ...] | --field lamb_oseen|uniform|shear --size H W) [-n PAIRS] [--density PPP]
                [--diameter AVG STD] [--laser-thickness LT] [--pad PX] [--method cubic|bilinear] [--out-of-plane SIGMA] [--seed S]

For every flow -- a Middlebury .flo file (a DNS field, the output of an earlier run) or an analytic field of the given size -- and
every one of PAIRS seedings it writes
    OUT/<name>_img1.png, OUT/<name>_img2.png    8-bit grey particle images
    OUT/<name>_flow.flo                         the true displacement of img1 -> img2: the flow itself
with <name> the .flo file's stem or the field's name, followed by _0000, _0001, ... where PAIRS > 1.  Then
    python run.py -i OUT -p --truth OUT ...
estimates the pairs and scores every estimate against its truth.  The particles are seeded on the host (pivlfn.particles: seeding k
of flow f uses seed S + f * PAIRS + k), moved and drawn on the GPU (pivlfn.ParticleImageGen.create_pair_from_flow, one render launch
for all pairs of a flow); only finished uint8 images are copied back, and background threads write the files.

The fields (pixel centres at integers, x the column, y the row, displacements in pixels):
    lamb_oseen   pivlfn.synth.displacement_field: a Lamb-Oseen vortex of peak displacement 4 px plus the shift (1.5, -0.75)
    uniform      (1.5, -0.75) everywhere
    shear        u = 0.05 * (y - (H-1)/2), v = 0
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.realpath(__file__))
sys.path.insert(0, HERE)

from pivlfn import synth                                 # noqa: E402
from pivlfn.flo import FloWriter, read_flow              # noqa: E402
from pivlfn.particles import METHODS, ParticleImageGen   # noqa: E402
from pivlfn.viz import GrayPngWriter                     # noqa: E402

FIELDS = ("lamb_oseen", "uniform", "shear")
CHUNK = 8                                                # pairs per render launch

parser = argparse.ArgumentParser(description="Synthetic PIV image pairs from a known flow (MI355X-native path)")
parser.add_argument("--output", "-o", type=str, required=True, help="Output directory (created if missing).")
src = parser.add_mutually_exclusive_group(required=True)
src.add_argument("--flow", type=str, nargs="+", metavar="FLO", help="Middlebury .flo files: each is the true displacement of its pairs.")
src.add_argument("--field", type=str, choices=FIELDS, help="An analytic field of --size.")
parser.add_argument("--size", type=int, nargs=2, metavar=("H", "W"), default=None, help="Frame size of --field.")
parser.add_argument("--pairs", "-n", type=int, default=1, help="Seedings per flow.")
parser.add_argument("--density", type=float, default=0.05, help="Particles per pixel.")
parser.add_argument("--diameter", type=float, nargs=2, metavar=("AVG", "STD"), default=(1.5, 1.0), help="d = AVG + STD * U[0,1) pixels.")
parser.add_argument("--laser-thickness", type=float, default=1.0, help="Light-sheet thickness: I = 240 exp(-z^2 / LT^2).")
parser.add_argument("--pad", type=int, default=16, help="Seeding margin round the image in pixels.")
parser.add_argument("--method", type=str, default="cubic", choices=sorted(METHODS), help="Interpolation of the flow at a particle.")
parser.add_argument("--out-of-plane", type=float, default=0.0, help="Std of the depth change between the frames (0: none).")
parser.add_argument("--seed", type=int, default=0, help="Seed of the first seeding.")


def analytic_field(kind: str, H: int, W: int) -> np.ndarray:
    """float32 [2,H,W] (u, v)."""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    if kind == "lamb_oseen":
        u, v = synth.displacement_field(xx, yy, H, W)
    elif kind == "uniform":
        u, v = np.full((H, W), 1.5), np.full((H, W), -0.75)
    else:
        u, v = 0.05 * (yy - 0.5 * (H - 1)), np.zeros((H, W))
    return np.stack([u, v]).astype(np.float32)


def main(argv=None) -> int:
    """Returns the number of pairs written."""
    args = parser.parse_args(argv)
    if args.pairs < 1:
        raise SystemExit(f"generate.py: -n {args.pairs}: at least one pair per flow")
    if args.field and (args.size is None or min(args.size) < 2):
        raise SystemExit("generate.py: --field needs --size H W with H, W >= 2")
    if args.flow and args.size is not None:
        raise SystemExit("generate.py: --size belongs to --field; a .flo file has its own size")
    try:                                                 # every parameter check before any file or tensor is touched
        ParticleImageGen(args.density, args.diameter[0], args.diameter[1], args.laser_thickness, args.seed)
    except (ValueError, TypeError) as e:
        raise SystemExit(f"generate.py: {e}")
    if args.pad < 0 or args.out_of_plane < 0 or not np.isfinite(args.out_of_plane):
        raise SystemExit("generate.py: --pad and --out-of-plane must not be negative")
    if args.flow:
        for path in args.flow:
            if not os.path.isfile(path):
                raise SystemExit(f"generate.py: --flow: no file '{path}'")
        sources = [(os.path.splitext(os.path.basename(p))[0], p) for p in args.flow]
        if len({s[0] for s in sources}) != len(sources):
            raise SystemExit("generate.py: --flow: two files of the same name would overwrite each other's pairs")
    else:
        sources = [(args.field, None)]
    if not torch.cuda.is_available():
        raise SystemExit("generate.py: no GPU: the particles are moved and drawn on the device, there is no CPU path")
    device = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(args.output, exist_ok=True)
    written = 0
    with GrayPngWriter() as png, FloWriter() as flo:
        for f, (stem, path) in enumerate(sources):
            if path is None:
                field = analytic_field(args.field, *args.size)
            else:
                field = np.ascontiguousarray(read_flow(path)[..., :2].transpose(2, 0, 1), dtype=np.float32)
            truth = np.ascontiguousarray(field.transpose(1, 2, 0))          # [H,W,2], what write_flow takes
            flow = torch.from_numpy(field).to(device)
            for k0 in range(0, args.pairs, CHUNK):
                n = min(CHUNK, args.pairs - k0)
                gen = ParticleImageGen(args.density, args.diameter[0], args.diameter[1], args.laser_thickness,
                                       args.seed + f * args.pairs + k0, device=device)
                img1, img2, _ = gen.create_pair_from_flow(flow[None].expand(n, -1, -1, -1), args.pad, args.method, None, args.out_of_plane)
                img1, img2 = img1.cpu().numpy(), img2.cpu().numpy()
                for k in range(n):
                    name = stem if args.pairs == 1 else f"{stem}_{k0 + k:04d}"
                    png.submit(img1[k], os.path.join(args.output, f"{name}_img1.png"))
                    png.submit(img2[k], os.path.join(args.output, f"{name}_img2.png"))
                    flo.submit(truth, os.path.join(args.output, f"{name}_flow.flo"))
                    written += 1
    print(f"generate.py: {written} pairs in {args.output}")
    return written


if __name__ == "__main__":
    main()
