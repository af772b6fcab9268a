#!/usr/bin/env python3
"""Counterpart of the reference's stereo_cal.py on the HIP path: two images of a cross target -> the mapping-coefficient file
`stereo_run.py --coeff` reads.  No window is opened; the four mouse clicks per camera become flags.

  python stereo_cal.py --root DIR --name NAME --save DIR --ref-left x y x y x y x y --ref-right x y x y x y x y
                       [--template TC HC LC] [--threshold T] [--order 1|2] [--no-invert] [--overlay]

Flags of the reference (stereo_cal.py:17-20): --root, --name, --save; the images are <root>/<name>-L.<ext> and <root>/<name>-R.<ext>
with the reference's extension list (:38).  --ref-left / --ref-right: four points (pixels, x then y) naming one lattice cell of that
camera clockwise from top-left (select_ref's L-R-D-L clicks, stereo/matching.py:78-115); each is snapped to its nearest marker.
--template: the cross template, default 11 25 25 (what the reference calls gen_template with, :99).  --threshold: the correlation
threshold, default 0.7 (:111).  --order: 2 fits all 24 coefficients, 1 keeps the quadratic ones at 0.  By default the image is
inverted (bitwise_not, :110: dark crosses on a bright plate); --no-invert for bright crosses.  --overlay writes
<save>/<name>-L_markers.png, <name>-R_markers.png (markers drawn on the image: indexed ones white-in-black, others black) and
<name>-L_dewarped.png, <name>-R_dewarped.png (pivlfn_dewarp_frames of the image, nearest).
Prints, per camera, the markers found and indexed and the fit residuals; writes <save>/<name>.json = {"Left", "Right", "calib"},
calib = the mean over the cameras of the cell width c_x (:140,151).

Differences, all deliberate: grey conversion is PIL's "L" (the reference: cv2's BGR2GRAY); marker centres are free of the half-pixel
shift of the reference's one-sided blur window; lattice indexing is a neighbour search from the reference cell instead of `Guess`; the
fit is a least-squares Gauss-Newton instead of Nelder-Mead; nothing changes the working directory."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.realpath(__file__))
sys.path.insert(0, HERE)

from pivlfn import calibrate as cal                       # noqa: E402
from pivlfn.viz import write_png_gray                      # noqa: E402

EXTS = [".jpg", ".jpeg", ".png", ".bmp", ".tif", ".ppm"]

parser = argparse.ArgumentParser(description="Stereoscopic PIV calibration (MI355X-native path)")
parser.add_argument("--root", "-r", default="./imgs", type=str, help="root directory for the input images")
parser.add_argument("--name", "-n", default="30-5_0", type=str, help="stereo image input names")
parser.add_argument("--save", "-s", default="./work", type=str, help="directory for saving")
parser.add_argument("--ref-left", type=float, nargs=8, required=True, metavar="V",
                    help="one lattice cell of the left image, clockwise from top-left: x y x y x y x y")
parser.add_argument("--ref-right", type=float, nargs=8, required=True, metavar="V", help="the same for the right image")
parser.add_argument("--template", type=int, nargs=3, default=[11, 25, 25], metavar=("TC", "HC", "LC"), help="cross thickness, height, width")
parser.add_argument("--threshold", type=float, default=0.7, help="correlation threshold")
parser.add_argument("--order", type=int, default=2, choices=[1, 2], help="order of the rational mapping")
parser.add_argument("--no-invert", action="store_true", help="the crosses are bright on dark: do not invert the image")
parser.add_argument("--overlay", action="store_true", help="write the marker overlays and the dewarped images")


def read_images(root: str, name: str):
    if not os.path.isdir(root):
        raise SystemExit(f"stereo_cal.py: --root {root} is not a directory")
    for ext in EXTS:
        names = [os.path.join(root, f"{name}{cam}{ext}") for cam in ("-L", "-R")]
        if all(os.path.isfile(n) for n in names):
            return names
    raise SystemExit(f"stereo_cal.py: no pair {name}-L.<ext> / {name}-R.<ext> in {root} (extensions {', '.join(EXTS)})")


def read_gray(path: str, invert: bool) -> np.ndarray:
    import PIL.Image
    with PIL.Image.open(path) as im:
        g = np.array(im.convert("L"), dtype=np.uint8)
    return np.bitwise_not(g) if invert else g


def draw_markers(gray: np.ndarray, markers: np.ndarray, indexed: np.ndarray) -> np.ndarray:
    out = gray.copy()
    H, W = out.shape
    for (x, y), ok in zip(markers, indexed):
        cx, cy = int(round(x)), int(round(y))
        out[max(cy - 2, 0):cy + 3, max(cx - 2, 0):cx + 3] = 0
        if ok and 0 <= cy < H and 0 <= cx < W:
            out[max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2] = 255
    return out


def main(argv=None) -> int:
    args = parser.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("stereo_cal.py: this build has no CPU path; a GPU is required")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    try:
        template = cal.gen_template(*args.template)
    except ValueError as e:
        raise SystemExit(f"stereo_cal.py: {e}")
    names = read_images(args.root, args.name)
    os.makedirs(args.save, exist_ok=True)
    coeff, c_x = {}, []
    for side, cam, path, ref in (("Left", "-L", names[0], args.ref_left), ("Right", "-R", names[1], args.ref_right)):
        gray = read_gray(path, not args.no_invert)
        image = torch.from_numpy(gray).to(dev)
        try:
            res = cal.calibrate_camera(image, template, np.asarray(ref, dtype=np.float64).reshape(4, 2), args.threshold, args.order)
        except ValueError as e:
            raise SystemExit(f"stereo_cal.py: {side.lower()} camera ({path}): {e}")
        print(f"{side}: {path}: {len(res['markers'])} markers, {int(res['indexed'].sum())} indexed, cell {res['spacing'][0]:.3f} x "
              f"{res['spacing'][1]:.3f} px, fit residual rms {res['rms']:.4f} px, max {res['max']:.4f} px")
        coeff[side] = res["A"]
        c_x.append(res["spacing"][0])
        if args.overlay:
            write_png_gray(os.path.join(args.save, f"{args.name}{cam}_markers.png"), draw_markers(gray, res["markers"], res["indexed"]))
            dew = cal.dewarp_frames(image, res["A"], res["origin"], "nearest", 0)
            write_png_gray(os.path.join(args.save, f"{args.name}{cam}_dewarped.png"), dew[0].cpu().numpy())
    out = os.path.join(args.save, f"{args.name}.json")
    cal.write_coeff(out, coeff["Left"], coeff["Right"], float(np.mean(c_x)))
    print(f"wrote {out} (calib {float(np.mean(c_x)):.4f} px per cell)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
