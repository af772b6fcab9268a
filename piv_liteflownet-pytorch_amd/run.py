#!/usr/bin/env python3
"""Counterpart of the reference's run.py on the HIP path: same flags, same output tree.

  python run.py --model piv -i DIR [-i DIR2 ...] -o OUT [-p] [-s N] [-n N] [-b F ...] [-c F ...] [-v 1|2]
                [--weights FILE] [--batch B] [--stats] [--validate flag|mask|replace]
                [--background min|FILE] [--minmax K] [--minmax-floor N] [--truth DIR [--truth-levels]]
                [--color [--color-max X] [--color-wheel interp|original]] [--vort-image [--vort-max X]] [--quiver [CELL]]
                [--quality [R] [--quality-image]] [--uncertainty [R] [--uncertainty-lag L] [--uncertainty-image [--uncertainty-max X]]]
                [--vortex [R] [--vortex-spacing S] [--vortex-image]] [--pod K [--pod-cell C]]
                [--ftle [SPACING] [--ftle-steps T] [--ftle-image [--ftle-max X]]]
                [--twopoint [R] [--twopoint-step S] [--twopoint-mean FILE]]
                [--pdf [BINS] [--pdf-range LO HI] [--pdf-mean FILE [--pdf-normalise]] [--pdf-hole H] [--pdf-image]]
                [--spectrum [L] [--spectrum-overlap O] [--spectrum-cell C] [--spectrum-fps F] [--spectrum-image]]
                [--pressure [CELL] [--pressure-rho R] [--pressure-nu NU] [--pressure-dt DT] [--pressure-calib C] [--pressure-tol T]
                 [--pressure-image]]
                [--smooth [WAVELENGTH] [--smooth-tol T]]
                [--ensemble [WINDOW] [--ensemble-step S] [--ensemble-search R] [--ensemble-predictor STATS.npz]]

Flags of the reference (run.py:24-42): --start/-s, --num_images/-n, --is_pair/-p, --brightness/-b, --contrast/-c,
--model/-m, --version/-v, --input/-i, --output/-o, --no_cuda.  Output tree (run.py:232-266):
OUT/<netname>/<input-basename>[-<start>_<count|end>]/flow[/left|right]/<name>_out.flo plus args[_left|_right].txt.
Without -b/-c every pair of the folder goes through `estimate` (reference main_dl, run.py:137-168); with -b and/or -c the
folder is read as a frame sequence and every consecutive pair is estimated once per (brightness, contrast) combination on
frames modified like the reference's `image_mod` (run.py:88-134), each flow named <prefix>_<BBB>_<CCC>_<suffix>_out.flo.

Differences, all deliberate:
  * `--weights FILE` names the state dict (the reference hard-codes models/pretrain_torch/*.paramOnly, which are not
    shipped, .MISSING_LARGE_BLOBS); without it the seeded generator of pivlfn.synth stands in and the net is called
    <model>-synthetic;  `--model` defaults to piv (the reference has no default and then fails on a None model);
  * `--no_cuda` (or no GPU) is an error: there is no CPU path, as in src/correlation.py:339-340;
  * pairs of equal size are batched (`--batch`), frames are decoded once on a prefetch thread, staged in pinned memory and
    converted on the device; flows return on a copy stream and a background writer closes the .flo files while the next
    batch computes (pivlfn.pipeline); under torch.distributed.run the pairs are sharded over the ranks
    (pivlfn.dist.shard_bounds);
  * `--background min|FILE`, `--minmax K`, `--minmax-floor N` pre-process every frame on the device before it is estimated
    (pivlfn.preproc: background subtraction, sliding min-max normalisation); without them the frames are only divided by 255, as
    in the reference;
  * `--truth DIR` scores every flow against the known field DIR/<name>_flow.flo on the device before it is copied back
    (pivlfn.evaluate: AEE, RMSE, L1, bias and the largest error per pair in <save>/errors.json, per-pixel bias and random-error
    maps in <save>/error_maps.npz); `--truth-levels` adds the table of pyramid level x stage errors;
  * `--color`, `--vort-image` and `--quiver` write pictures beside every .flo: <name>_out.png (the Middlebury colour coding of the
    reference's motion_to_color, with color_wheel.png as the legend), <name>_vort.png (vorticity, blue - white - red) and
    <name>_quiver.png (one arrow per cell).  They are coloured / averaged on the device before the copy back (pivlfn.viz) and written
    on background threads; with --validate flag|mask the rejected vectors are black and left out of the normaliser and the arrows;
  * `--quality [R]` writes a per-vector quality measure beside every .flo, computed on the device from the two frames the network was
    given and the flow that is written (pivlfn.quality.match_quality: the correlation of frame 1 with frame 2 warped back by the
    flow inside (2R+1)^2 windows, and the sub-pixel residual of its peak): <name>_qual.flo with the three bands c, dx, dy, the
    summaries in <save>/quality.json, and with `--quality-image` <name>_corr.png (c on 0..1 in gray, undefined pixels red); with
    --validate flag|mask the rejected vectors are left out of the windows;
  * `--uncertainty [R]` writes the standard uncertainty of every vector in pixels beside every .flo, computed on the device from the two
    frames the network was given and the flow that is written (pivlfn.uncertainty.flow_uncertainty: the correlation statistics of
    (2R+1)^2 windows, the covariance of the contributions summed over `--uncertainty-lag L` pixels, default 2): <name>_unc.flo with the
    bands ux, uy (1e10 where a vector has none), the parameters and summaries in <save>/uncertainty.json -- with `--truth` also the
    coverage, the share of vectors whose error is within their uncertainty (0.68 for a calibrated estimate), and RMS error / RMS u --
    with `--stats` <save>/uncertainty_stats.npz (the noise share of the normal stresses and the uncertainty of the mean, per pixel), and
    with `--uncertainty-image` <name>_unc.png (|u| in gray on 0..X of `--uncertainty-max`, default 0.5 px; vectors without a value red);
    with --validate flag|mask the rejected vectors are left out of the windows;
  * `--vortex [R]` writes the vortex identification functions of the flow that is written beside every .flo, computed on the device
    (pivlfn.vortex.vortex_gamma: Gamma1 and Gamma2 over the (2R+1)^2 vectors at `--vortex-spacing S` pixels around each one):
    <name>_gamma.flo with the two bands, the vortex centres and core areas of every pair and the summary of the run in
    <save>/vortices.json, and with `--vortex-image` <name>_gamma2.png (Gamma2 on -1..1 in blue - white - red, undefined pixels
    black); with --validate flag|mask the rejected vectors are left out;
  * `--twopoint [R]` accumulates the two-point statistics of the flows of every input directory on the device
    (pivlfn.twopoint.TwoPointStats: per row the sums behind R_uu, R_vv, R_uv and the structure functions at the separations
    0..R times `--twopoint-step S` pixels along x and along y; with --validate flag|mask the rejected vectors are left out) and
    writes <save>/twopoint.npz and <save>/twopoint.json with the integral scales, Taylor microscales and noise shares;
    `--twopoint-mean FILE` takes the per-pixel mean of a --stats run out first (flows that are not homogeneous along a row);
  * `--pdf [BINS]` accumulates the velocity distributions of the flows of every input directory on the device
    (pivlfn.distribution.FlowDistribution: the histograms of u and v over `--pdf-range LO HI`, their joint histogram, the histogram
    of the sub-pixel fraction of the displacement, and per pixel the sums up to the fourth order with the quadrant split of u'v' at
    the hole `--pdf-hole H`; with --validate flag|mask the rejected vectors are left out) and writes <save>/pdf.npz and
    <save>/pdf.json with the peak-locking degree, the pooled skewness and flatness and the shares outside the range;
    `--pdf-mean FILE` takes the per-pixel mean of a --stats run out first, `--pdf-normalise` also divides by its rms;
    `--pdf-image` adds <save>/pdf_joint.png, the joint density on a logarithmic gray scale over four decades, empty bins red;
  * `--spectrum [L]` estimates the temporal spectra of the flows of every input directory, which must be a time-resolved frame
    sequence (not -p), on the device (pivlfn.spectrum.TemporalSpectrum, Welch's method: Hann-windowed segments of L pairs that
    overlap by `--spectrum-overlap O` (default L/2), mean removed; `--spectrum-cell C` analyses the means over C x C blocks of
    vectors; `--spectrum-fps F` the pairs per time unit, default 1: frequencies in cycles per pair) and writes <save>/spectrum.npz
    (the raw sums and every parameter) and <save>/spectrum.json (the pooled peak frequency and its share, the resolution, the
    segments and the pairs left over); with `--spectrum-image` <save>/spectrum_peak.png, the dominant-frequency map in gray on
    0..the highest frequency kept, vectors without a segment red; with --validate flag|mask a rejected vector drops the segments
    it sits in;
  * `--pressure [CELL]` integrates the pressure field of every flow of an input directory that has both neighbours in time; the
    directory must be a time-resolved frame sequence (not -p).  On the device (pivlfn.pressure.PressureField): the flows are averaged
    over CELL x CELL blocks (default 4), the material acceleration is taken by central differences over three consecutive flows and
    the pressure gradient is integrated in the least-squares sense by conjugate gradients.  `--pressure-rho R`, `--pressure-nu NU`,
    `--pressure-dt DT` (time per pair) and `--pressure-calib C` (length per pixel) give the units, all default to lattice units (1, 0, 1,
    1); `--pressure-tol T` is the relative residual to reach (default 1e-8).  Per centred pair <name>_pres.flo with the bands p and
    |grad p| on the lattice (1e10 where a node has no value; the first and the last pair of a directory get none), the parameters and
    per-pair summaries in <save>/pressure.json, with `--pressure-image` <name>_pres.png (blue - white - red on a symmetric range);
    with --validate flag|mask the rejected vectors are left out of the block means.  A single process, not with -b/-c;
  * `--smooth [WAVELENGTH]` smooths every flow and fills its gaps in one solve, on the device (pivlfn.smooth.smooth_flow: penalised
    least squares, conjugate gradients preconditioned in the DCT basis), directly after --validate: under flag|mask the rejected
    vectors are the gaps, under replace only those the median step could not replace, and unknown vectors always are.  Waves of
    WAVELENGTH pixels (default 8) keep half their amplitude; `--smooth-tol T` is the relative residual to reach (default 1e-8).  The
    .flo files and every later stage get the smoothed, complete flow; the parameters and per pair the filled vectors, iterations,
    residual and converged go to <save>/smooth.json.  A single process, not with -b/-c;
  * `--ensemble [WINDOW]` measures the mean displacement of every input directory a second way, straight from the frames the
    network was given (after any pre-processing) and without the weights: ensemble correlation on the device
    (pivlfn.ensemble.EnsembleCorrelation: the correlation planes of WINDOW x WINDOW interrogation windows, default 32, every
    `--ensemble-step S` pixels, default half the window, at the displacements -R..R of `--ensemble-search R`, default 8, added over all
    pairs; one peak per window is read from the sum).  `--ensemble-predictor STATS.npz` names the per-pixel mean of an earlier --stats
    run: it supplies a whole-pixel pre-shift per window, for displacements beyond R, and is the field the result is compared with.
    Writes <save>/ensemble.npz (the integer sums and every parameter), <save>/ensemble.flo (two bands on the window lattice, 1e10
    where a window is flagged) and <save>/ensemble.json (the parameters, the pairs, the flag counts, the median peak height and peak
    ratio, and with a predictor the bias and rms of the difference).  A single process, not with -b/-c;
  * `--pod K` decomposes the flows of every input directory after it has been processed (pivlfn.pod.FlowPOD, snapshot POD: the
    Gram matrix of the flows in float64 on the device, its eigenvectors on the host): the first K modes, the mean, the coefficients
    and the energy fractions go to <save>/pod.npz, one line per mode is printed, and with --color the modes are drawn as
    <save>/pod_mode<k>.png; `--pod-cell C` decomposes the means over C x C blocks of vectors.  2..4096 pairs per directory, a
    single process, not with -b/-c; a rejected vector that leaves a cell empty is refused (use --validate replace or a larger cell);
  * `--ftle [SPACING]` follows fluid through the flows of every input directory, which must be a time-resolved frame sequence (not
    -p), on the device (pivlfn.flowmap.FlowMap: particles seeded every SPACING pixels, carried through consecutive flows by one
    bilinear sample per flow): the finite-time Lyapunov exponent over windows of `--ftle-steps T` pairs (default: the whole
    directory), <first pair of the window>_ftle.flo with the bands ftle and stretch on the seed lattice, the summaries in
    <save>/ftle.json, and with `--ftle-image` <name>_ftle.png (gray on 0..X of `--ftle-max`, else the window's own maximum; undefined
    nodes red).  A trailing incomplete window is dropped and counted; with --validate flag|mask a particle that meets a rejected
    vector is LOST.  A single process, not with -b/-c;
  * a trailing slash on an input directory is ignored (the reference would name the output directory '');
  * with -b/-c a frame whose file name has no '_' gets the tag appended (<stem>_<BBB>_<CCC>_out.flo) -- the reference splits
    the whole path at its last '_' and then either fails or lets the combinations overwrite each other.
"""
import argparse
import json
import math
import os
import struct
import sys
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from types import SimpleNamespace
from itertools import product
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

HERE = os.path.dirname(os.path.realpath(__file__))
sys.path.insert(0, HERE)

from pivlfn import Network                               # noqa: E402
from pivlfn import flowmap, quality, synth, uncertainty, viz, vortex  # noqa: E402
from pivlfn.datasets import Run, image_files_from_folder, pair_files     # noqa: E402
from pivlfn.dist import shard_bounds                     # noqa: E402
from pivlfn import _accum, ensemble                     # noqa: E402
from pivlfn.evaluate import ErrorStats, flow_errors, level_errors        # noqa: E402
from pivlfn.flo import FloWriter, flowname_modifier, write_flow     # noqa: E402
from pivlfn.imagemod import mod_name                     # noqa: E402
from pivlfn.inference import estimate                    # noqa: E402
from pivlfn.pipeline import PairLoader, stream_pairs     # noqa: E402
from pivlfn.pod import FlowPOD                           # noqa: E402
from pivlfn.pressure import PressureField                # noqa: E402
from pivlfn.pressure import check_params as check_pressure               # noqa: E402
from pivlfn.smooth import check_params as check_smooth, smooth_flow, summarize as summarize_smooth      # noqa: E402
from pivlfn.postpro import FlowStats                     # noqa: E402
from pivlfn.preproc import FrameBackground, Preprocessor                 # noqa: E402
from pivlfn.distribution import FlowDistribution         # noqa: E402
from pivlfn.distribution import check_params as check_pdf                # noqa: E402
from pivlfn.spectrum import TemporalSpectrum             # noqa: E402
from pivlfn.spectrum import check_params as check_spectrum               # noqa: E402
from pivlfn.twopoint import TwoPointStats                # noqa: E402
from pivlfn.twopoint import check_params as check_twopoint               # noqa: E402
from pivlfn.preproc import check_params as check_prep    # noqa: E402
from pivlfn.validate import NOT_REPLACED, OUTLIER, UNKNOWN, MaskedFlowStats, validate_flow      # noqa: E402
from pivlfn.validate import check_params as check_validate               # noqa: E402

parser = argparse.ArgumentParser(description="Inferencing script for LiteFlowNet (MI355X-native path)")
parser.add_argument("--start", "-s", type=int, default=0, help="Input image starting index.")
parser.add_argument("--num_images", "-n", type=int, default=-1, help="Number of image(s) to process from the directory.")
parser.add_argument("--is_pair", "-p", action="store_true", help="To check if the input image format is in pair.")
parser.add_argument("--brightness", "-b", default=None, type=float, nargs="+",
                    help="Add brightness factor to modify all the input images (optional).")
parser.add_argument("--contrast", "-c", default=None, type=float, nargs="+",
                    help="Add contrast factor to modify all the input images (optional).")
parser.add_argument("--model", "-m", type=str, choices=["hui", "piv"], default="piv", help="Select which model to solve the problem!")
parser.add_argument("--version", "-v", type=int, choices=[1, 2], default=1,
                    help="Select the LiteFlowNet model backbone version (i.e., LiteFlowNet or LiteFlowNet2)!")
parser.add_argument("--input", "-i", default=["./images/demo"], type=str, nargs="+", help="Input images directory(ies).")
parser.add_argument("--output", "-o", default="./results", type=str, help="Main output directory.")
parser.add_argument("--no_cuda", action="store_true")
parser.add_argument("--weights", type=str, default=None, help="state dict file (torch.load); default: seeded synthetic weights")
parser.add_argument("--synthetic_weights", action="store_true")
parser.add_argument("--batch", type=int, default=4, help="pairs per forward")
parser.add_argument("--precision", type=str, default=None, choices=["fp32", "fp32_wino_mfma32", "fp32_direct", "fp32_split", "fp32_split3", "fp16"],
                    help="how the large convolutions multiply (not a reference flag; default: the library's, fp32 -- "
                         "see Network.precision)")
parser.add_argument("--stats", action="store_true",
                    help="also write per-pixel statistics of each input directory's flows (mean, RMS, Reynolds stress, vorticity; "
                         "pivlfn.postpro.FlowStats) to <save>/stats.npz (not a reference flag; not with -b/-c, single process only)")
parser.add_argument("--validate", type=str, default=None, choices=["flag", "mask", "replace"],
                    help="normalized median test on every flow, on the device (pivlfn.validate.validate_flow; not a reference flag; "
                         "not with -b/-c, single process only): 'flag' writes the flows unchanged, 'mask' writes 1e10 for rejected "
                         "vectors, 'replace' the median of their neighbours; all write <save>/validation.json")
parser.add_argument("--validate-radius", type=int, default=1, help="neighbourhood radius of --validate: 1 (3 x 3) or 2 (5 x 5)")
parser.add_argument("--validate-spacing", type=int, default=1, help="distance in pixels between the neighbours of --validate")
parser.add_argument("--validate-eps", type=float, default=0.1, help="noise level of --validate in pixels (raise it with the spacing)")
parser.add_argument("--validate-thresh", type=float, default=2.0, help="normalized residual above which --validate rejects a vector")
parser.add_argument("--background", type=str, default=None, metavar="min|FILE",
                    help="subtract a static background from every frame on the device before it is estimated "
                         "(pivlfn.preproc; not a reference flag; not with -b/-c): 'min' takes the per-pixel minimum over the frames "
                         "of each input directory first and writes it to <save>/background.png (single process only); FILE is such "
                         "an image")
parser.add_argument("--minmax", type=int, default=None, metavar="K",
                    help="sliding min-max normalisation of every frame over K x K windows, K odd in 3..31, after the background "
                         "(pivlfn.preproc.preprocess_frames; not with -b/-c)")
parser.add_argument("--minmax-floor", type=int, default=None, metavar="N",
                    help="smallest local contrast, in grey levels 1..255, that --minmax stretches to full scale (default 16)")
parser.add_argument("--truth", type=str, default=None, metavar="DIR",
                    help="score every flow against the known field DIR/<name>_flow.flo (<name>: what the flow file is called without "
                         "_out.flo) on the device (pivlfn.evaluate; not a reference flag; not with -b/-c; sharded over ranks like the "
                         "flows, the records meeting on rank 0): writes <save>/errors.json (a value that is not finite, such as the AEE of "
                         "a pair with nothing to score, is written as null) and <save>/error_maps.npz; with --validate flag|mask the "
                         "rejected vectors are left out, with --validate replace the replaced flow is scored (--validate itself is "
                         "single process only)")
parser.add_argument("--truth-levels", action="store_true",
                    help="with --truth: also the average end-point error of every pyramid level and stage (M, S, R) in errors.json; "
                         "the frame sizes must be multiples of 32")
parser.add_argument("--color", action="store_true",
                    help="also write <name>_out.png beside every .flo: the flow in the Middlebury colour coding (pivlfn.viz.flow_to_color; "
                         "not a reference flag; not with -b/-c), coloured on the device after --validate (rejected vectors are black "
                         "under flag and mask), and color_wheel.png, the legend, once per output directory")
parser.add_argument("--color-max", type=float, default=None, metavar="X",
                    help="with --color: the vector length in pixels that gets full saturation.  Without it every pair is normalised by "
                         "its own longest vector, as the reference does for a single field, so the pictures of a sequence are only "
                         "comparable with a fixed normaliser")
parser.add_argument("--color-wheel", type=str, default=None, choices=["interp", "original"],
                    help="with --color: the interpolated colour wheel (default, the reference's) or the original Middlebury one")
parser.add_argument("--vort-image", action="store_true",
                    help="also write <name>_vort.png beside every .flo: the vorticity (pivlfn.postpro.flow_fields) in blue - white - red, "
                         "symmetric about 0 (pivlfn.viz.vorticity_image; not a reference flag; not with -b/-c)")
parser.add_argument("--vort-max", type=float, default=None, metavar="X",
                    help="with --vort-image: the vorticity magnitude at the ends of the colour map; without it every pair takes its own "
                         "largest magnitude")
parser.add_argument("--quiver", type=int, nargs="?", const=0, default=None, metavar="CELL",
                    help="also write <name>_quiver.png beside every .flo: one arrow per CELL x CELL block of vectors, averaged on the "
                         "device (pivlfn.viz.decimate_flow); without CELL the smallest block that leaves at most 64 arrows per axis.  "
                         "Needs matplotlib (not a reference flag; not with -b/-c)")
parser.add_argument("--quality", type=int, nargs="?", const=8, default=None, metavar="R",
                    help="also write <name>_qual.flo beside every .flo: the match quality of the written flow (pivlfn.quality."
                         "match_quality; not a reference flag; not with -b/-c): bands c, the correlation of frame 1 with frame 2 warped "
                         "back by the flow inside (2R+1) x (2R+1) windows (R = 1..15, default 8), and dx, dy, the sub-pixel residual of "
                         "its peak; the summaries go to <save>/quality.json.  With --validate flag|mask the rejected vectors are left out "
                         "of the windows, with --validate replace the replaced flow is rated")
parser.add_argument("--quality-image", action="store_true",
                    help="with --quality: also <name>_corr.png, c on 0..1 in gray, pixels without a value in red")
parser.add_argument("--uncertainty", type=int, nargs="?", const=8, default=None, metavar="R",
                    help="also write <name>_unc.flo beside every .flo: the standard uncertainty of the written flow in pixels, bands ux "
                         "and uy, from the correlation statistics of (2R+1) x (2R+1) windows (pivlfn.uncertainty.flow_uncertainty; R = "
                         "1..15, default 8; not a reference flag; not with -b/-c); 1e10 where a vector has none; the summaries go to "
                         "<save>/uncertainty.json, with --truth also the coverage, with --stats the per-pixel sums to "
                         "<save>/uncertainty_stats.npz.  With --validate flag|mask the rejected vectors are left out of the windows, "
                         "with --validate replace the replaced flow is rated")
parser.add_argument("--uncertainty-lag", type=int, default=None, metavar="L",
                    help="with --uncertainty: the covariance of the pixel-wise contributions is summed over (2L+1) x (2L+1) offsets, "
                         "L = 0..4 (default 2)")
parser.add_argument("--uncertainty-image", action="store_true",
                    help="with --uncertainty: also <name>_unc.png, |u| in gray on 0..X, vectors without a value in red")
parser.add_argument("--uncertainty-max", type=float, default=None, metavar="X",
                    help="with --uncertainty-image: the |u| in pixels that is drawn white (default 0.5)")
parser.add_argument("--vortex", type=int, nargs="?", const=4, default=None, metavar="R",
                    help="also write <name>_gamma.flo beside every .flo: the vortex identification functions Gamma1 and Gamma2 of the "
                         "written flow (pivlfn.vortex.vortex_gamma; not a reference flag; not with -b/-c) over the (2R+1) x (2R+1) "
                         "vectors around each one (R = 1..15, default 4); the vortex centres (peaks of |Gamma2|) and the core areas "
                         "(|Gamma2| > 2/pi) go to <save>/vortices.json.  With --validate flag|mask the rejected vectors are left out, "
                         "with --validate replace the replaced flow is rated")
parser.add_argument("--vortex-spacing", type=int, default=None, metavar="S",
                    help="with --vortex: the distance in pixels between the neighbours, 1..16 (default 1)")
parser.add_argument("--vortex-image", action="store_true",
                    help="with --vortex: also <name>_gamma2.png, Gamma2 in blue - white - red on the fixed range -1..1 (the pictures of a "
                         "sequence are comparable), pixels without a value in black")
parser.add_argument("--pod", type=int, default=None, metavar="K",
                    help="after each input directory, write the first K POD modes of its flows (method of snapshots, pivlfn.pod.FlowPOD: "
                         "mean, modes, coefficients, energies) to <save>/pod.npz and print their energy fractions; with --color also "
                         "<save>/pod_mode<k>.png (not a reference flag; not with -b/-c, single process only, at most 4096 pairs)")
parser.add_argument("--pod-cell", type=int, default=None, metavar="C",
                    help="with --pod: decompose the means over C x C blocks of vectors (default 1: every vector)")
parser.add_argument("--ftle", type=int, nargs="?", const=1, default=None, metavar="SPACING",
                    help="follow fluid through the consecutive flows of each input directory (pivlfn.flowmap.FlowMap; not a reference "
                         "flag; not with -p or -b/-c, single process only): particles seeded every SPACING pixels (default 1), the "
                         "finite-time Lyapunov exponent of their flow map in <first pair of the window>_ftle.flo (bands ftle and "
                         "stretch, on the seed lattice) and the summaries in <save>/ftle.json.  With --validate flag|mask a particle "
                         "that meets a rejected vector is lost, with --validate replace the replaced flow carries it")
parser.add_argument("--ftle-steps", type=int, default=None, metavar="T",
                    help="with --ftle: the pairs per window (default: all pairs of the directory, one window); the map is reseeded after "
                         "each window and a trailing incomplete window is dropped")
parser.add_argument("--ftle-image", action="store_true",
                    help="with --ftle: also <name>_ftle.png, the exponent in gray on 0..X, nodes without a value in red")
parser.add_argument("--ftle-max", type=float, default=None, metavar="X",
                    help="with --ftle-image: the exponent (per pair interval) that is drawn white; without it every window takes its own "
                         "maximum")
parser.add_argument("--twopoint", type=int, nargs="?", const=64, default=None, metavar="R",
                    help="accumulate the two-point statistics of the flows of each input directory on the device "
                         "(pivlfn.twopoint.TwoPointStats; not a reference flag; not with -b/-c, single process only): correlations and "
                         "structure functions at the separations 0..R (0..255, default 64) along x and y, written to "
                         "<save>/twopoint.npz, the integral scales, Taylor microscales and noise shares to <save>/twopoint.json")
parser.add_argument("--twopoint-step", type=int, default=None, metavar="S",
                    help="with --twopoint: the pixels between two separations, 1..16 (default 1)")
parser.add_argument("--twopoint-mean", type=str, default=None, metavar="FILE",
                    help="with --twopoint: a stats.npz of an earlier --stats run over the same frames; its mean_u and mean_v are taken "
                         "out of every vector before the sums are formed")
parser.add_argument("--pdf", type=int, nargs="?", const=256, default=None, metavar="BINS",
                    help="accumulate the velocity distributions of the flows of each input directory on the device "
                         "(pivlfn.distribution.FlowDistribution; not a reference flag; not with -b/-c, single process only): the "
                         "histograms of u and v with BINS bins (1..4096, default 256), their joint histogram, the histogram of the "
                         "sub-pixel fraction (peak locking) and the per-pixel sums up to the fourth order with the quadrant split, "
                         "written to <save>/pdf.npz, the scalar results to <save>/pdf.json")
parser.add_argument("--pdf-range", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="with --pdf: the range of the histograms in pixels (default -8 8), with --pdf-normalise in units of the local "
                         "rms (default -6 6)")
parser.add_argument("--pdf-mean", type=str, default=None, metavar="FILE",
                    help="with --pdf: a stats.npz of an earlier --stats run over the same frames; its mean_u and mean_v are taken out "
                         "of every vector first (the accurate form of the higher moments)")
parser.add_argument("--pdf-normalise", action="store_true",
                    help="with --pdf and --pdf-mean: the samples of the histograms are divided by rms_u and rms_v of that file, and "
                         "the hole is in units of rms_u * rms_v")
parser.add_argument("--pdf-hole", type=float, default=None, metavar="H",
                    help="with --pdf: the hole size of the quadrant analysis, an event needs |U*V| > H (default 0)")
parser.add_argument("--pdf-image", action="store_true",
                    help="with --pdf: also <save>/pdf_joint.png, the joint density of (u, v) in gray on a logarithmic scale")
PDF_FLAGS = ("pdf", "pdf_range", "pdf_mean", "pdf_normalise", "pdf_hole", "pdf_image")
parser.add_argument("--spectrum", type=int, nargs="?", const=256, default=None, metavar="L",
                    help="estimate the temporal spectra of the flows of each input directory, read as a frame sequence, on the device "
                         "(pivlfn.spectrum.TemporalSpectrum, Welch's method; not a reference flag; not with -p or -b/-c, single process "
                         "only): segments of L pairs (2..1024, default 256), the sums in <save>/spectrum.npz, the pooled peak frequency "
                         "and its share in <save>/spectrum.json")
parser.add_argument("--spectrum-overlap", type=int, default=None, metavar="O",
                    help="with --spectrum: the pairs two consecutive segments share, 0..L-1 (default L/2)")
parser.add_argument("--spectrum-cell", type=int, default=None, metavar="C",
                    help="with --spectrum: analyse the means over C x C blocks of vectors (default 1: every vector)")
parser.add_argument("--spectrum-fps", type=float, default=None, metavar="F",
                    help="with --spectrum: the pairs per time unit (default 1: frequencies in cycles per pair)")
parser.add_argument("--spectrum-image", action="store_true",
                    help="with --spectrum: also <save>/spectrum_peak.png, the dominant-frequency map in gray, vectors without a segment in red")
PREP_FLAGS = ("background", "minmax", "minmax_floor")
parser.add_argument("--pressure", type=int, nargs="?", const=4, default=None, metavar="CELL",
                    help="integrate the pressure field of every flow that has both neighbours in time (pivlfn.pressure.PressureField; not a "
                         "reference flag; not with -p or -b/-c, single process only) on the means over CELL x CELL blocks of vectors "
                         "(default 4): <name>_pres.flo with the bands p and |grad p|, the summaries in <save>/pressure.json")
parser.add_argument("--pressure-rho", type=float, default=None, metavar="R", help="with --pressure: the density (default 1)")
parser.add_argument("--pressure-nu", type=float, default=None, metavar="NU", help="with --pressure: the kinematic viscosity (default 0)")
parser.add_argument("--pressure-dt", type=float, default=None, metavar="DT", help="with --pressure: the time between two pairs (default 1)")
parser.add_argument("--pressure-calib", type=float, default=None, metavar="C", help="with --pressure: the length of a pixel (default 1)")
parser.add_argument("--pressure-tol", type=float, default=None, metavar="T",
                    help="with --pressure: the relative residual at which the conjugate gradients stop (default 1e-8)")
parser.add_argument("--pressure-image", action="store_true",
                    help="with --pressure: also <name>_pres.png, p in blue - white - red on a symmetric range, nodes without a value black")
parser.add_argument("--smooth", type=float, nargs="?", const=8.0, default=None, metavar="WAVELENGTH",
                    help="smooth every flow and fill its gaps by penalised least squares (pivlfn.smooth.smooth_flow), directly after "
                         "--validate, whose rejected vectors are the gaps: waves of WAVELENGTH pixels (default 8) keep half their "
                         "amplitude; the .flo files and every later stage get the smoothed flow, the summaries go to <save>/smooth.json")
parser.add_argument("--smooth-tol", type=float, default=None, metavar="T",
                    help="with --smooth: the relative residual at which the conjugate gradients stop (default 1e-8)")
parser.add_argument("--ensemble", type=int, nargs="?", const=32, default=None, metavar="WINDOW",
                    help="ensemble correlation of the frames of every input directory on the device (pivlfn.ensemble.EnsembleCorrelation; "
                         "not a reference flag; not with -b/-c, single process only): the correlation planes of WINDOW x WINDOW "
                         "interrogation windows (a multiple of 4 in 8..128, default 32) added over all pairs, one displacement per "
                         "window to <save>/ensemble.flo, the sums to <save>/ensemble.npz, the summary to <save>/ensemble.json")
parser.add_argument("--ensemble-step", type=int, default=None, metavar="S",
                    help="with --ensemble: the pixels between two windows (default half the window)")
parser.add_argument("--ensemble-search", type=int, default=None, metavar="R",
                    help="with --ensemble: the largest displacement looked at around the pre-shift, 1..32 pixels (default 8)")
parser.add_argument("--ensemble-predictor", type=str, default=None, metavar="FILE",
                    help="with --ensemble: a stats.npz of an earlier --stats run over the same frames; its mean_u and mean_v, averaged "
                         "over each window and rounded, pre-shift the window of the second frame, and the result is compared with them")
SMOOTH_FLAGS = ("smooth", "smooth_tol")
ENSEMBLE_FLAGS = ("ensemble", "ensemble_step", "ensemble_search", "ensemble_predictor")
PRESSURE_FLAGS = ("pressure", "pressure_rho", "pressure_nu", "pressure_dt", "pressure_calib", "pressure_tol", "pressure_image")
SPECTRUM_FLAGS = ("spectrum", "spectrum_overlap", "spectrum_cell", "spectrum_fps", "spectrum_image")
TWOPOINT_FLAGS = ("twopoint", "twopoint_step", "twopoint_mean")
POD_FLAGS = ("pod", "pod_cell")
QUALITY_FLAGS = ("quality", "quality_image")
QUALITY_BAD_RGB = (255, 0, 0)
UNCERTAINTY_FLAGS = ("uncertainty", "uncertainty_lag", "uncertainty_image", "uncertainty_max")
VORTEX_FLAGS = ("vortex", "vortex_spacing", "vortex_image")
PICTURE_FLAGS = ("color", "color_max", "color_wheel", "vort_image", "vort_max", "quiver")
FTLE_FLAGS = ("ftle", "ftle_steps", "ftle_image", "ftle_max")
VIZ_FLAGS = PICTURE_FLAGS + QUALITY_FLAGS + UNCERTAINTY_FLAGS + VORTEX_FLAGS + POD_FLAGS + FTLE_FLAGS + TWOPOINT_FLAGS + PDF_FLAGS + SPECTRUM_FLAGS + PRESSURE_FLAGS + SMOOTH_FLAGS + ENSEMBLE_FLAGS      # every flag of a further output beside the .flo: absent from args.txt unless used
TRUTH_FLAGS = ("truth", "truth_levels")


def _used(args, flags) -> bool:
    """Whether the command line sets any flag of the group."""
    return any(getattr(args, k) is not None and getattr(args, k) is not False for k in flags)


@dataclass(frozen=True)
class OutputLayout:
    """Where the results of one input directory go."""
    save: str          # OUT/<netname>/<label>
    flow: str          # <save>/flow[/left|right]
    args_file: str     # <save>/args[_left|_right].txt

    @staticmethod
    def of(out_root: str, netname: str, input_dir: str, start: int, num_images: int) -> "OutputLayout":
        parts = os.path.normpath(input_dir).split(os.sep)
        side = parts[-1].lower() if parts[-1].lower() in ("left", "right") else None      # stereo halves share one parent label
        label = parts[-2] if side and len(parts) > 1 else parts[-1]
        if start != 0 or num_images >= 0:                                                  # a slice of the folder says so in its name
            label += f"-{start}_{'end' if num_images < 0 else num_images}"
        save = os.path.join(out_root, netname, label)
        return OutputLayout(save=save,
                            flow=os.path.join(save, "flow", side) if side else os.path.join(save, "flow"),
                            args_file=os.path.join(save, f"args_{side}.txt" if side else "args.txt"))

    def sibling(self, name: str) -> str:
        """A file beside args[_left|_right].txt: "stats.npz" -> <save>/stats.npz (stats_left / stats_right.npz for the halves of a
        stereo set)."""
        stem, ext = os.path.splitext(name)
        return os.path.join(self.save, stem + os.path.basename(self.args_file)[len("args"):-len(".txt")] + ext)


class _FrameSequence:
    """Consecutive frames of a folder as pairs, each called by the PATH of its first frame (the -b/-c path names its
    outputs from that path, run.py:126-129).  Listing as the reference's getpair (run.py:48-70): lower-case extensions."""

    def __init__(self, folder: str, n_images: int, start_at: int):
        if not os.path.isdir(folder):
            raise ValueError(f"Input image directory is NOT found! '{folder}'")
        if n_images == 1:
            raise ValueError("--num_images 1 leaves no pair to process")
        files = image_files_from_folder(folder, pair=False, upper=False, n_images=n_images, start_at=start_at)
        pairs = pair_files(files, is_pair=False)
        self.image_list = [[a, b] for a, b, _ in pairs]
        self.name_list = [a for a, _, _ in pairs]

    def __len__(self):
        return len(self.name_list)


def mod_flow_name(first_frame: str, savedir: str, mod: Tuple[float, float]) -> str:
    """<savedir>/<prefix>_<BBB>_<CCC>_<suffix>_out.flo, prefix/suffix = the frame's file name split at its last '_'."""
    stem = os.path.splitext(os.path.basename(first_frame))[0]
    prefix, sep, suffix = stem.rpartition("_")
    tagged = f"{prefix}_{mod_name(*mod)}_{suffix}" if sep else f"{stem}_{mod_name(*mod)}"
    return flowname_modifier(tagged, savedir, pair=False)


def checked(prefix, check, *params):
    """check(*params), its ValueError turned into the SystemExit of a refused command line."""
    try:
        return check(*params)
    except ValueError as e:
        raise SystemExit(f"run.py: {prefix}{e}")


def json_strict(x):
    """JSON has no NaN or Infinity: null stands for every value that is not finite."""
    if isinstance(x, dict):
        return {k: json_strict(v) for k, v in x.items()}
    if isinstance(x, list):
        return [json_strict(v) for v in x]
    return None if isinstance(x, float) and not math.isfinite(x) else x


def write_json(path, doc, **kw):
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, **kw)
        f.write("\n")


def gather_rows(names, rows, world):
    """(the names of all ranks, [every rank's `rows`]), both in rank order -- the shards are contiguous, so that is pair order.
    Sharded runs (world > 1) need a process group."""
    if world == 1:
        return names, [rows]
    import torch.distributed as dist
    parts = [None] * world
    dist.all_gather_object(parts, (names, rows))
    return [n for p in parts for n in p[0]], [p[1] for p in parts]


def _cat(parts):
    """The per-batch records of a stage, kept on the device until now, as one host tensor in pair order (None without a batch)."""
    return torch.cat(parts).cpu() if parts else None


# ---- one forward, then the stages ----------------------------------------------------------------------------------------------------
@dataclass
class Batch:
    """What one forward produced, all on the device."""
    img1: torch.Tensor                      # the tensors the network was given
    img2: torch.Tensor
    raw: torch.Tensor                       # the network's flow
    flow: torch.Tensor                      # what the .flo files get: `raw` unless validation masks or replaces
    flag: Optional[torch.Tensor] = None     # the validator's flags
    mode: Optional[str] = None              # the validation mode
    levels: Optional[list] = None           # the per-level flows of the same forward, if a stage asked for them
    truth: Optional[torch.Tensor] = None    # the known flows [n,2,H,W], once the Truth stage has run
    extras: dict = field(default_factory=dict)      # name -> tensor [n, ...] that returns to the host with the flows

    def masked(self):
        """(flow, mask) for what looks at the vectors that passed: under "flag" and "mask" the raw flow with the flags as the mask,
        otherwise (no validation, or "replace") the written flow and no mask."""
        return (self.raw, self.flag) if self.mode in ("flag", "mask") else (self.flow, None)


class Stage:
    """One further output of run.py.  The Estimator calls begin() before every forward and the stage itself after it, in the order of
    its list; the stage enqueues on the current stream and never synchronises the host.  main_dl calls finish() after the directory
    (`names`: the pairs of this rank in order; `ctx`: rank, world, device) and close() whatever happened."""
    levels = False          # wants Batch.levels
    extras = False          # puts per-pair outputs into Batch.extras

    def begin(self, n, device):
        pass

    def __call__(self, batch):
        pass

    def finish(self, names, ctx):
        pass

    def close(self):
        pass


class _LevelsNet:
    """Stands in for the network inside estimate(): the same forward, with the per-level flows of the last call kept."""

    def __init__(self, net):
        self.net, self.training, self.levels = net, False, None

    def eval(self):
        return self

    def __call__(self, a, b):
        out, self.levels = self.net.forward_levels(a, b)
        return out


class Estimator:
    """stream_pairs' estimate_fn: one forward per batch, then every stage on its Batch; extras() is stream_pairs' hook of that name."""

    def __init__(self, stages, estimate=estimate):
        self.stages, self.estimate = list(stages), estimate
        self.levels = any(s.levels for s in self.stages)
        self.batch = None

    def __call__(self, net, img1, img2, tensor=True):
        for stage in self.stages:
            stage.begin(img1.size(0), img1.device)
        run_net = _LevelsNet(net) if self.levels else net          # estimate()'s resize logic stays the single code path
        raw = self.estimate(run_net, img1, img2, tensor=True)
        self.batch = Batch(img1, img2, raw, raw, levels=run_net.levels if self.levels else None)
        for stage in self.stages:
            stage(self.batch)
        return self.batch.flow

    def extras(self):
        return self.batch.extras


class Validate(Stage):
    """validate_flow on the device: sets what the .flo files get -- the flow itself for "flag", the masked / replaced flow otherwise.
    The per-pair counts of the three flag bits are reduced on the device and stay there until finish() copies them once."""

    def __init__(self, mode, radius, spacing, eps, thresh, file):
        self.mode, self.params, self.file = mode, dict(radius=radius, spacing=spacing, eps=eps, thresh=thresh), file
        self._counts = []

    def __call__(self, batch):
        res = validate_flow(batch.raw, mode=self.mode, **self.params)
        batch.flow, batch.flag, batch.mode = res.flow, res.flag, self.mode
        flat = res.flag.flatten(1)
        self._counts.append(torch.stack([(flat & bit).ne(0).sum(1) for bit in (OUTLIER, UNKNOWN, NOT_REPLACED)], dim=1))

    def finish(self, names, ctx):
        """<save>/validation.json: the parameters, per pair name the counts of outlier / unknown / not-replaced vectors, the totals."""
        rows = _cat(self._counts).tolist() if self._counts else []
        assert len(rows) == len(names)
        keys = ("outlier", "unknown", "not_replaced")
        write_json(self.file, {"mode": self.mode, **self.params,
                               "pairs": {name: dict(zip(keys, row)) for name, row in zip(names, rows)},
                               "total": {k: sum(row[i] for row in rows) for i, k in enumerate(keys)}})


class Smooth(Stage):
    """smooth_flow on the device, directly after validation: under "flag" and "mask" the raw flow with the validator's flags as the gaps,
    under "replace" the replaced flow with only the NOT_REPLACED vectors as gaps, without validation the flow as it is (unknown vectors
    are gaps by themselves).  Sets what the .flo files and every later stage get to the smoothed flow -- complete, so the flags and the
    mode are cleared.  The iterations are driven as the Pressure stage drives its own: in chunks, the states read in between.  The
    per-pair records stay on the device until finish() copies them once."""

    def __init__(self, wavelength, tol, file):
        self.wavelength, self.tol, self.file = wavelength, tol, file
        self.mode, self.s, self.max_iter, self._rows = None, None, None, []

    def __call__(self, batch):
        if batch.mode in ("flag", "mask"):
            flow, gaps = batch.raw, batch.flag
        elif batch.mode == "replace":
            flow, gaps = batch.flow, batch.flag & NOT_REPLACED
        else:
            flow, gaps = batch.flow, None
        try:
            res = smooth_flow(flow, wavelength=self.wavelength, mask=gaps, tol=self.tol)
        except ValueError as e:
            raise SystemExit(f"run.py: --smooth: {e}")
        if not self._rows:
            self.mode, self.s, self.max_iter = batch.mode, res.s, res.max_iter
        self._rows.append((res.filled.flatten(1).sum(1), res.status))
        batch.flow, batch.flag, batch.mode = res.flow, None, None

    def finish(self, names, ctx):
        """<save>/smooth.json: the parameters, per pair name the filled vectors, iterations, residual and converged, and the count of
        unconverged pairs."""
        filled = _cat([f for f, _ in self._rows])
        status = _cat([st for _, st in self._rows])
        frames = summarize_smooth(status.numpy(), filled.tolist(), self.tol) if self._rows else []
        assert len(frames) == len(names)
        doc = {"wavelength": self.wavelength, "s": self.s, "tol": self.tol, "max_iter": self.max_iter, "validation": self.mode,
               "pairs": dict(zip(names, frames)), "unconverged": int(sum(not fr["converged"] for fr in frames))}
        write_json(self.file, json_strict(doc), allow_nan=False)
        print(f"Smoothed {len(frames)} pairs at {self.wavelength} px: {sum(fr['filled'] for fr in frames)} vectors filled, "
              f"{doc['unconverged']} pairs not converged -> '{self.file}'")


class Stats(Stage):
    """Adds every batch of flows to a FlowStats, created at the first batch's size; after "flag" and "mask" (raw flow, flag) go to a
    MaskedFlowStats instead, after "replace" the FlowStats gets the replaced flow.  The file says which validation the flows went
    through."""

    def __init__(self, file):
        self.file, self.stats, self.extra = file, None, {}

    def __call__(self, batch):
        flow, flag = batch.masked()
        if self.stats is None:
            kind = FlowStats if flag is None else MaskedFlowStats
            self.stats = kind(flow.size(2), flow.size(3), device=flow.device)
            self.extra = {} if batch.mode is None else {"validation": batch.mode}
        self.stats.update(*((flow,) if flag is None else (flow, flag)))

    def finish(self, names, ctx):
        if self.stats is not None:
            self.stats.save(self.file, **self.extra)


class TwoPoint(Stage):
    """Adds every batch of flows to a TwoPointStats, created at the first batch's size and fed like Stats: after "flag" and "mask" the
    raw flow with the flags as the mask, otherwise the written flow.  finish() writes the sums and what follows from them."""

    def __init__(self, max_sep, step, mean, file, json_file):
        self.max_sep, self.step, self.mean, self.file, self.json_file = max_sep, step, mean, file, json_file
        self.stats, self.mode = None, None

    def __call__(self, batch):
        flow, flag = batch.masked()
        if self.stats is None:
            try:
                self.stats = TwoPointStats(flow.size(2), flow.size(3), self.max_sep, self.step, self.mean, flow.device)
            except ValueError as e:
                raise SystemExit(f"run.py: --twopoint: {e}")
            self.mode = batch.mode
        self.stats.update(flow, flag)

    def finish(self, names, ctx):
        """<save>/twopoint.npz (TwoPointStats.save) and <save>/twopoint.json: the parameters, the validation the flows went through and
        TwoPointResult.summary(); one line with the four integral scales."""
        if self.stats is None:
            return
        extra = {} if self.mode is None else {"validation": self.mode}
        self.stats.save(self.file, **extra)
        summary = self.stats.result().summary()
        write_json(self.json_file, json_strict({"max_sep": self.max_sep, "step": self.step, "mean": self.mean, "validation": self.mode,
                                                "summary": summary}))
        scales = ", ".join(f"{key} {summary[key]['integral_scale']:.2f}{'+' if summary[key]['truncated'] else ''}"
                           for key in ("uu_x", "uu_y", "vv_x", "vv_y"))
        print(f"Two-point statistics of {self.stats.count} flows: integral scales in pixels {scales} ('+': the correlation did not reach zero)")


class Ensemble(Stage):
    """Adds the frames of every batch -- the tensors the network was given -- to an EnsembleCorrelation, created at the first batch's
    size; with a predictor file its window means are the pre-shift and the field the result is compared with.  finish() writes the
    sums, the displacement lattice and the summary."""

    def __init__(self, window, step, search, predictor, file, flo_file, json_file):
        self.window, self.step, self.search, self.predictor = window, step, search, predictor
        self.file, self.flo_file, self.json_file = file, flo_file, json_file
        self.acc, self.mean = None, None

    def __call__(self, batch):
        if self.acc is None:
            H, W = batch.img1.shape[2:]
            try:
                offset = None
                if self.predictor is not None:
                    self.mean = _accum.load_planes(self.predictor, ("mean_u", "mean_v"), "EnsembleCorrelation: predictor", H, W, "cpu").numpy()
                    offset = ensemble.predictor_offsets(self.mean, self.window, self.step, self.search)
                self.acc = ensemble.EnsembleCorrelation(H, W, self.window, self.step, self.search, offset, device=batch.img1.device)
            except ValueError as e:
                raise SystemExit(f"run.py: --ensemble: {e}")
        self.acc.update(batch.img1, batch.img2)

    def finish(self, names, ctx):
        """<save>/ensemble.npz (EnsembleResult.save), <save>/ensemble.flo (the displacement on the window lattice, 1e10 where a window
        is flagged) and <save>/ensemble.json (the parameters, EnsembleResult.summary() and, with a predictor, the comparison); one
        line with the counts."""
        if self.acc is None:
            return
        res = self.acc.result()
        res.save(self.file)
        lattice = np.where(res.flag[None] != 0, 1e10, res.displacement).astype(np.float32)
        write_flow(np.ascontiguousarray(lattice.transpose(1, 2, 0)), self.flo_file)
        summary = res.summary()
        doc = {"window": self.window, "step": self.step, "search": self.search, "predictor": self.predictor, "rows": res.ny,
               "columns": res.nx, "summary": summary}
        if self.mean is not None:
            doc["comparison"] = {k: v for k, v in res.compare(self.mean).items() if k != "difference"}
        write_json(self.json_file, json_strict(doc), allow_nan=False)
        print(f"Ensemble correlation of {res.frames} pairs: {summary['valid']} of {summary['windows']} windows of {self.window} px give a "
              f"displacement, median peak height {summary['median_height']:.3f}, median peak ratio {summary['median_ratio']:.1f} "
              f"-> '{self.flo_file}'")


def pdf_params(args):
    """(bins, range, joint_bins, frac_bins, hole) of the --pdf flags with the defaults filled in."""
    rng = tuple(args.pdf_range) if args.pdf_range is not None else ((-6.0, 6.0) if args.pdf_normalise else (-8.0, 8.0))
    return args.pdf, rng, 64, 64, 0.0 if args.pdf_hole is None else args.pdf_hole


class Distribution(Stage):
    """Adds every batch of flows to a FlowDistribution, created at the first batch's size and fed like Stats: after "flag" and "mask" the
    raw flow with the flags as the mask, otherwise the written flow.  finish() writes the sums and what follows from them."""

    def __init__(self, params, mean, normalise, image, file, json_file, image_file):
        self.params, self.mean, self.normalise, self.image = params, mean, normalise, image
        self.file, self.json_file, self.image_file = file, json_file, image_file
        self.dist, self.mode = None, None

    def __call__(self, batch):
        flow, flag = batch.masked()
        if self.dist is None:
            bins, rng, joint_bins, frac_bins, hole = self.params
            try:
                self.dist = FlowDistribution(flow.size(2), flow.size(3), bins, rng, joint_bins, frac_bins, mean=self.mean,
                                             scale=self.mean if self.normalise else None, hole=hole, device=flow.device)
            except (ValueError, KeyError) as e:
                raise SystemExit(f"run.py: --pdf: {e}")
            self.mode = batch.mode
        self.dist.update(flow, flag)

    def finish(self, names, ctx):
        """<save>/pdf.npz (DistributionResult.save) and <save>/pdf.json: the parameters, the validation the flows went through and
        DistributionResult.summary(); one line with the peak-locking degrees, the pooled skewness and flatness and the share outside
        the range; with `image` <save>/pdf_joint.png."""
        if self.dist is None:
            return
        res = self.dist.result()
        res.save(self.file, **({} if self.mode is None else {"validation": self.mode}))
        summary = res.summary()
        bins, rng, joint_bins, frac_bins, hole = self.params
        write_json(self.json_file, json_strict({"bins": bins, "range": list(rng), "joint_bins": joint_bins, "frac_bins": frac_bins,
                                                "hole": hole, "mean": self.mean, "normalise": bool(self.normalise),
                                                "validation": self.mode, "summary": summary}))
        pooled = summary["pooled"]
        out = max(sum(summary[f"outside_{c}"].values()) for c in "uv")
        print(f"Velocity distributions of {res.frames} flows ({res.counted} vectors, {res.left_out} left out): peak locking u "
              f"{summary['peak_locking_u']:.3f}, v {summary['peak_locking_v']:.3f}; skewness u {pooled['skewness_u']:.3f}, v "
              f"{pooled['skewness_v']:.3f}; flatness u {pooled['flatness_u']:.3f}, v {pooled['flatness_v']:.3f}; "
              f"{100.0 * out:.2f} % outside [{rng[0]:g}, {rng[1]:g})")
        if self.image:
            _, density = res.joint()
            with np.errstate(divide="ignore", invalid="ignore"):
                logd = np.where(density > 0, np.log10(density), np.nan)            # empty bins and a histogram without vectors: bad
            top = float(np.nanmax(logd)) if np.isfinite(logd).any() else 0.0
            rgb = viz.scalar_to_color(torch.from_numpy(logd[None]).to(self.dist.device), top - 4.0, top, cmap="gray", bad=QUALITY_BAD_RGB)
            viz.write_png(self.image_file, rgb[0].cpu().numpy())


class Spectrum(Stage):
    """Feeds every batch of flows to a TemporalSpectrum, created at the first batch's size and fed like Stats: after "flag" and "mask"
    the raw flow with the flags as the mask (a rejected vector drops the segments it sits in), otherwise the written flow.  finish()
    writes the sums, the summary and with `image` the dominant-frequency map."""

    def __init__(self, segment, overlap, cell, fs, image, file, json_file, image_file):
        self.segment, self.overlap, self.cell, self.fs, self.image = segment, overlap, cell, fs, image
        self.file, self.json_file, self.image_file = file, json_file, image_file
        self.spectrum, self.mode = None, None

    def __call__(self, batch):
        flow, flag = batch.masked()
        if self.spectrum is None:
            H, W = flow.size(2), flow.size(3)
            need, free = TemporalSpectrum.device_bytes(H, W, self.segment, self.cell), torch.cuda.mem_get_info(flow.device)[0]
            if need > free // 2:
                raise SystemExit(f"run.py: --spectrum: the ring of {self.segment} flows of {H} x {W} and the sums take {need / 2**30:.1f} GiB, "
                                 f"more than half of the {free / 2**30:.1f} GiB free on the device; analyse block means with --spectrum-cell C")
            try:
                self.spectrum = TemporalSpectrum(H, W, self.segment, self.overlap, cell=self.cell, fs=self.fs, device=flow.device)
            except ValueError as e:
                raise SystemExit(f"run.py: --spectrum: {e}")
            self.mode = batch.mode
        self.spectrum.update(flow, flag)

    def finish(self, names, ctx):
        """<save>/spectrum.npz (TemporalSpectrumResult.save), <save>/spectrum.json (the parameters, the validation the flows went
        through and summary()), one line with the pooled peak, and with `image` <save>/spectrum_peak.png."""
        if self.spectrum is None:
            return
        res = self.spectrum.result()
        res.save(self.file, **({} if self.mode is None else {"validation": self.mode}))
        summary = res.summary()
        write_json(self.json_file, json_strict({"segment": self.segment, "overlap": res.overlap, "cell": self.cell, "fps": self.fs,
                                                "window": res.window, "detrend": res.detrend, "validation": self.mode, "summary": summary}))
        if summary["peak_frequency"] is None:
            print(f"Temporal spectra of {res.frames} flows: no vector is known throughout a segment")
        else:
            print(f"Temporal spectra of {res.frames} flows in {summary['segments']} segments of {self.segment}: pooled peak at "
                  f"{summary['peak_frequency']:.6g} cycles per {'pair' if self.fs == 1.0 else 'time unit'} (resolution "
                  f"{summary['resolution']:.3g}), {100.0 * summary['peak_share']:.1f} % of the fluctuation energy")
        if self.image:
            f, _, _ = res.peak()
            rgb = viz.scalar_to_color(torch.from_numpy(f[None]).to(self.spectrum.device), 0.0, float(res.freq[-1]), cmap="gray",
                                      bad=QUALITY_BAD_RGB)
            viz.write_png(self.image_file, rgb[0].cpu().numpy())


def pressure_params(args):
    """(cell, calib, dt, rho, nu, tol) of the --pressure flags with the defaults filled in."""
    pick = lambda v, d: d if v is None else v            # noqa: E731
    return (args.pressure, pick(args.pressure_calib, 1.0), pick(args.pressure_dt, 1.0), pick(args.pressure_rho, 1.0),
            pick(args.pressure_nu, 0.0), pick(args.pressure_tol, 1e-8))


class Pressure(Stage):
    """Feeds every batch of flows to a PressureField, created at the first batch's size and fed like Stats: after "flag" and "mask"
    the raw flow with the flags as the mask, otherwise the written flow.  A frame is centred on every pair that has both neighbours, so
    the results of a batch belong to pairs one earlier; they stay on the device until finish() writes the files."""

    def __init__(self, params, image, flowdir, file):
        self.params, self.image, self.flowdir, self.file = params, image, flowdir, file
        self.field, self.mode, self.results = None, None, []

    def __call__(self, batch):
        flow, flag = batch.masked()
        if self.field is None:
            cell, calib, dt, rho, nu, tol = self.params
            try:
                self.field = PressureField(flow.size(2), flow.size(3), cell, calib, dt, rho, nu, tol, device=flow.device)
            except ValueError as e:
                raise SystemExit(f"run.py: --pressure: {e}")
            self.mode = batch.mode
        self.results.append(self.field.update(flow, flag))

    def finish(self, names, ctx):
        """<flow dir>/<name>_pres.flo (bands p and |grad p| on the lattice, float32, 1e10 where the node is not ok) for every pair
        but the first and the last, with `image` the picture beside it, and <save>/pressure.json."""
        cell, calib, dt, rho, nu, tol = self.params
        doc = {"cell": cell, "calib": calib, "dt": dt, "rho": rho, "nu": nu, "tol": tol, "validation": self.mode,
               "max_iter": None if self.field is None else self.field.max_iter,
               "lattice": None if self.field is None else [self.field.ch, self.field.cw], "pairs": {}, "unconverged": 0}
        centred = names[1:-1]
        assert sum(len(r) for r in self.results) == len(centred)
        at = 0
        with FloWriter() as writer, viz.PngWriter() as pictures:
            for res in self.results:
                if len(res) == 0:
                    continue
                summary = res.summary()
                doc["unconverged"] += summary["unconverged"]
                for f in range(len(res)):
                    name = centred[at]
                    at += 1
                    doc["pairs"][os.path.basename(flowname_modifier(name, self.flowdir, ext="", pair=False))] = summary["frames"][f]
                    writer.submit(pressure_bands(res.p[f], res.grad[f], res.flag[f]), flowname_modifier(name, self.flowdir, ext="_pres.flo", pair=False))
                    if self.image:
                        top = max(abs(summary["frames"][f]["p_min"] or 0.0), abs(summary["frames"][f]["p_max"] or 0.0)) or 1.0
                        p = torch.from_numpy(np.ascontiguousarray(res.p[f][None])).to(res.p_star.device)
                        rgb = viz.scalar_to_color(p, -top, top, cmap="bwr")
                        pictures.submit(rgb[0].cpu().numpy(), flowname_modifier(name, self.flowdir, ext="_pres.png", pair=False))
        write_json(self.file, json_strict(doc), allow_nan=False)
        print(f"Pressure of {len(centred)} pairs on {doc['lattice']} nodes: {doc['unconverged']} not converged -> '{self.file}'")


def pressure_bands(p, grad, flag):
    """[ch,cw,2] float32: p and |grad p|, 1e10 where the node is not ok."""
    ok = flag == 0
    mag = np.sqrt(grad[0] * grad[0] + grad[1] * grad[1])
    return np.stack([np.where(ok, p, 1e10), np.where(ok, mag, 1e10)], axis=2).astype(np.float32)


def check_pressure_pairs(pairs, inputdir):
    if pairs < 3:
        raise SystemExit(f"run.py: --pressure: '{inputdir}' has {pairs} pairs, fewer than the 3 a pressure field is centred in")


def check_spectrum_pairs(pairs, segment, inputdir):
    if pairs < segment:
        raise SystemExit(f"run.py: --spectrum: '{inputdir}' has {pairs} pairs, fewer than the {segment} of one segment")


def truth_files(ds, truth_dir, levels=False):
    """The truth file of every pair of `ds` (a Run), DIR/<stem>_flow.flo with the stem flowname_modifier gives the flow file.  Every
    file must exist and have the size of the pair's first frame (a multiple of 32 both ways for `levels`): checked here, from the
    headers alone, before anything is launched."""
    import PIL.Image
    paths = []
    for name, pair in zip(ds.name_list, ds.image_list):
        path = flowname_modifier(name, truth_dir, ext="_flow.flo", pair=False)
        if not os.path.isfile(path):
            raise SystemExit(f"run.py: --truth: no truth file '{path}' for pair '{name}'")
        with open(path, "rb") as f:
            head = f.read(12)
        if len(head) != 12 or head[:4] != b"PIEH":
            raise SystemExit(f"run.py: --truth: '{path}' is not a .flo file")
        w, h = struct.unpack("<ii", head[4:])
        with PIL.Image.open(pair[0]) as im:
            fw, fh = im.size
        if (w, h) != (fw, fh):
            raise SystemExit(f"run.py: --truth: '{path}' is {h} x {w} (H x W) but the frames of pair '{name}' are {fh} x {fw}")
        if levels and (fw % 32 or fh % 32):
            raise SystemExit(f"run.py: --truth-levels needs frame sizes that are multiples of 32, pair '{name}' is {fh} x {fw} (H x W)")
        paths.append(path)
    return paths


class _TruthPrefetch:
    """Reads the truth files of the pairs in order on a few threads, `depth` files ahead, each straight from the file into a pinned
    [H,W,2] float32 tensor (the .flo payload as it is; the headers were checked by truth_files).  A 1024 x 1024 field is 8 MB: one
    thread going through read_flow, a host transpose and pin_memory() -- four passes over it -- held the fp16 loop back."""

    def __init__(self, paths, pin, depth=8, workers=4):
        self.paths, self.pin, self.depth, self.at = list(paths), pin, depth, 0
        self.pool = ThreadPoolExecutor(max_workers=workers)
        self.pending = deque()
        self._fill()

    def _read(self, path):
        with open(path, "rb") as f:
            w, h = struct.unpack("<ii", f.read(12)[4:])
            buf = torch.empty([h, w, 2], dtype=torch.float32, pin_memory=self.pin)
            got = f.readinto(buf.numpy().reshape(-1).view(np.uint8))      # little-endian float32, the layout of the file
        if got != buf.numel() * 4:
            raise SystemExit(f"run.py: --truth: '{path}' holds {got} of {buf.numel() * 4} payload bytes")
        return buf

    def _fill(self):
        while len(self.pending) < self.depth and self.at < len(self.paths):
            self.pending.append(self.pool.submit(self._read, self.paths[self.at]))
            self.at += 1

    def take(self, n):
        out = []
        for _ in range(n):
            out.append(self.pending.popleft().result())
            self._fill()
        return out

    def close(self):
        for f in self.pending:
            f.cancel()
        self.pool.shutdown(wait=True)


class Truth(Stage):
    """Scores every flow against the next truth field (`paths`: the truth_files() of this rank's pairs) on the device: per-pair sums
    (pivlfn.evaluate.flow_errors) stay there until finish() copies them once, and an ErrorStats collects the per-pixel maps.  After
    "flag" and "mask" the raw flow is scored with the flags as the mask, after "replace" the replaced flow.  `levels`: also
    level_errors on the per-level flows of the same forward; as Stage.levels it is also what makes the Estimator keep them."""

    def __init__(self, net, paths, levels, errors_file, maps_file, pin):
        self.net, self.levels, self.errors_file, self.maps_file = net, levels, errors_file, maps_file
        self.div_flow = 1.0 / (5.0 if net.starting_scale == 10 else 20.0)
        self.prefetch = _TruthPrefetch(paths, pin)
        self.copy = None                                        # the truth goes up on its own stream, under the forward
        self.stats, self.mode = None, None
        self._sums, self._excluded, self._level_sums = [], [], []

    def begin(self, n, device):
        if self.copy is None:
            self.copy = torch.cuda.Stream(device)
        with torch.cuda.stream(self.copy):
            self.raw = torch.stack([t.to(device, non_blocking=True) for t in self.prefetch.take(n)])        # [n,H,W,2]

    def __call__(self, batch):
        main = torch.cuda.current_stream(batch.raw.device)
        main.wait_stream(self.copy)
        self.raw.record_stream(main)
        truth = batch.truth = self.raw.permute(0, 3, 1, 2).contiguous()
        scored, mask = batch.masked()
        self.mode = batch.mode
        if mask is not None:
            self._excluded.append(mask.flatten(1).ne(0).sum(1))
        err = flow_errors(scored, truth, mask)
        self._sums.append(torch.stack(list(err[:7]), dim=1))
        if self.stats is None:
            self.stats = ErrorStats(scored.size(2), scored.size(3), device=scored.device)
        self.stats.update(scored, truth, mask)
        if self.levels:
            table = level_errors(self.net, batch.levels, truth, self.div_flow, mask)
            self._level_sums.append(torch.stack([torch.stack([torch.stack(list(e[:7]), dim=1) for e in row], dim=1) for row in table],
                                                dim=1))

    def close(self):
        self.prefetch.close()

    def finish(self, names, ctx):
        """Writes errors.json and error_maps.npz.  Sharded runs: the per-pair records of all ranks are gathered (gather_rows), the
        maps are merged (ErrorStats.merge), and rank 0 writes."""
        size = None if self.stats is None else (self.stats.H, self.stats.W)
        names, parts = gather_rows(names, (_cat(self._sums), _cat(self._excluded), _cat(self._level_sums), size), ctx.world)
        sums, excluded, levels = (torch.cat([p[i] for p in parts if p[i] is not None]) if any(p[i] is not None for p in parts) else None
                                  for i in (0, 1, 2))
        size = next((p[3] for p in parts if p[3] is not None), None)
        if ctx.world > 1 and size is not None:
            if self.stats is None:                              # a rank without pairs still takes part in the merge
                self.stats = ErrorStats(size[0], size[1], device=ctx.device)
            self.stats.merge()
        if ctx.rank == 0:
            write_errors_json(self.errors_file, names, sums, excluded, levels, self.mode, self.div_flow)      # validation: one process
            if self.stats is not None and self.stats.count > 0:
                self.stats.save(self.maps_file)


def write_errors_json(path, names, sums, excluded, levels, mode, div_flow):
    """<save>/errors.json: per pair name n, aee, rmse, l1, bias_u, bias_v, max (pixels; null where the value is not finite: nothing
    scored, or a non-finite estimated flow); the totals over the run, formed from the per-pair sums in pair order; with --validate flag|mask the vectors left out; with --truth-levels the level x stage AEE tables.
    sums [pairs,7], excluded [pairs] or None, levels [pairs,nlev,3,7] or None: host tensors (Truth.finish)."""
    rows = sums.tolist() if sums is not None else []
    assert len(rows) == len(names)

    def record(s):
        n = s[0]
        div = (lambda x: x / n) if n else (lambda x: float("nan"))
        return {"n": int(n), "aee": div(s[2]), "rmse": math.sqrt(div(s[3])) if n else float("nan"), "l1": div(s[1]) / 2.0,
                "bias_u": div(s[4]), "bias_v": div(s[5]), "max": s[6]}
    total = [0.0] * 7
    for s in rows:                  # the largest error of the run is NaN if a pair's is (Python's max would drop it)
        total = [a + b for a, b in zip(total[:6], s[:6])] + [s[6] if s[6] != s[6] or s[6] > total[6] else total[6]]
    doc = {"pairs": {name: record(s) for name, s in zip(names, rows)}, "total": record(total)}
    if excluded is not None:
        ex = excluded.tolist()
        doc["validate"] = mode
        doc["excluded"] = {"pairs": dict(zip(names, ex)), "total": sum(ex)}
    if levels is not None:
        tot = levels[0].clone()
        for s in levels[1:]:
            tot += s                                            # the pairs' sums in pair order
        aee = (tot[:, :, 2] / tot[:, :, 0]).tolist()            # [nlev][3] in level units (flow * div_flow at that level's resolution)
        doc["levels"] = {"div_flow": div_flow, "stages": ["M", "S", "R"], "levels": [6 - i for i in range(len(aee))],
                         "aee_level_units": aee, "aee_px": [[v / div_flow for v in row] for row in aee]}
    write_json(path, json_strict(doc), allow_nan=False)


class Pictures(Stage):
    """Makes the pictures of every batch on the device, right after the flows and on the same stream; they go back to the host with
    the flows.  After "flag" and "mask" the pictures show the raw flow with the flags as the mask (what is rejected is black, stays
    out of the normalisers and out of the arrows), after "replace" the replaced flow."""
    extras = True

    def __init__(self, color, color_max, color_wheel, vort_image, vort_max, quiver):
        self.color, self.color_max, self.color_wheel = color, color_max, color_wheel or "interp"
        self.vort_image, self.vort_max, self.quiver = vort_image, vort_max, quiver

    def cell(self, H, W):
        return self.quiver or viz.quiver_cell(H, W)

    def __call__(self, batch):
        shown, mask = batch.masked()
        if self.color:
            batch.extras["color"] = viz.flow_to_color(shown, self.color_max, wheel=self.color_wheel, mask=mask)
        if self.vort_image:
            batch.extras["vort"] = viz.vorticity_image(shown, vmax=self.vort_max, mask=mask)
        if self.quiver is not None:
            batch.extras["quiver_mean"], batch.extras["quiver_count"] = viz.decimate_flow(shown, self.cell(*shown.shape[2:]), mask)


class Quality(Stage):
    """Rates every batch of flows on the device, right after them and on the same stream: match_quality of the frames the network
    was given and the flow that is written, with the flags of "flag" or "mask" as the mask.  The three bands -- and the picture of
    c, with `image` -- go back to the host with the flows; the per-pair sums (pivlfn.quality.SUMS) stay on the device until finish()
    copies them once."""
    extras = True

    def __init__(self, radius, image, file, mask=None):
        self.radius, self.image, self.file, self.mask = radius, image, file, mask      # mask: "flag", "mask" or None, for quality.json
        self.floor = 1.0 / 255.0
        self.min_count = quality.check_params(radius, self.floor, None)
        self._sums = []

    def __call__(self, batch):
        q = quality.match_quality(batch.img1, batch.img2, batch.flow, self.radius, batch.masked()[1], self.floor, self.min_count)
        self._sums.append(q.sums())
        batch.extras["qual"] = torch.cat([q.c.unsqueeze(1), q.residual], dim=1).permute(0, 2, 3, 1)      # the .flo layout
        if self.image:
            batch.extras["corr"] = viz.scalar_to_color(q.c.contiguous(), 0.0, 1.0, cmap="gray", bad=QUALITY_BAD_RGB)

    def finish(self, names, ctx):
        """<save>/quality.json: the parameters, per pair name the summary of MatchQuality.summary(), and the same over the run, formed
        from the per-pair sums in pair order.  Sharded runs: the records of all ranks are gathered (gather_rows) and rank 0 writes.
        A value that is not finite is written as null."""
        rows = _cat(self._sums).tolist() if self._sums else []
        assert len(rows) == len(names)
        names, parts = gather_rows(names, rows, ctx.world)
        if ctx.rank != 0:
            return
        rows = [row for part in parts for row in part]
        total = [0.0] * 9
        for row in rows:
            total = [a + b for a, b in zip(total, row)]
        doc = {"radius": self.radius, "floor": self.floor, "min_count": self.min_count, "mask": self.mask,
               "pairs": {name: quality.summarize(row) for name, row in zip(names, rows)}, "total": quality.summarize(total)}
        write_json(self.file, json_strict(doc), allow_nan=False)


class Uncertainty(Stage):
    """Puts an uncertainty on every batch of flows on the device, right after them and on the same stream: flow_uncertainty of the
    frames the network was given and the flow that is written, with the flags of "flag" or "mask" as the mask.  The two bands -- and
    the picture of |u|, with `image` -- go back to the host with the flows; the per-pair sums (pivlfn.uncertainty.SUMS and, after a
    Truth stage, COVERAGE_SUMS) stay on the device until finish() copies them once.  `stats`: the file of the per-pixel sums, or
    None."""
    extras = True

    def __init__(self, radius, lag, image, vmax, file, stats, mask=None):
        self.radius, self.lag, self.image, self.vmax, self.file, self.mask = radius, lag, image, vmax, file, mask
        self.floor = 1.0 / 255.0
        self.min_count = uncertainty.check_params(radius, lag, self.floor, None)
        self.stats_file, self.stats = stats, None
        self._sums, self._coverage = [], []

    def __call__(self, batch):
        mask = batch.masked()[1]
        unc = uncertainty.flow_uncertainty(batch.img1, batch.img2, batch.flow, self.radius, self.lag, mask, self.floor, self.min_count)
        self._sums.append(unc.sums())
        if batch.truth is not None:
            self._coverage.append(uncertainty.coverage_sums(batch.flow, batch.truth, unc, mask))
        if self.stats_file is not None:
            if self.stats is None:
                self.stats = uncertainty.UncertaintyStats(unc.u.size(2), unc.u.size(3), device=unc.u.device)
            self.stats.update(unc)
        none = (unc.flag & uncertainty.UNUSABLE).ne(0).unsqueeze(1)
        batch.extras["unc"] = torch.where(none, torch.full_like(unc.u, 1e10), unc.u).permute(0, 2, 3, 1)      # the .flo layout
        if self.image:
            batch.extras["unc_image"] = viz.scalar_to_color(unc.magnitude(), 0.0, self.vmax, cmap="gray", bad=QUALITY_BAD_RGB)

    def finish(self, names, ctx):
        """<save>/uncertainty.json: the parameters, per pair name the summary of FlowUncertainty.summary() -- after a Truth stage with
        the coverage and RMS error / RMS u of uncertainty_coverage() -- and the same over the run, formed from the per-pair sums in pair
        order.  Sharded runs: the records of all ranks are gathered (gather_rows) and rank 0 writes.  A value that is not finite is
        written as null.  With `stats` <save>/uncertainty_stats.npz (a single process)."""
        rows = _cat(self._sums).tolist() if self._sums else []
        cover = _cat(self._coverage).tolist() if self._coverage else None
        assert len(rows) == len(names) and (cover is None or len(cover) == len(names))
        if self.stats is not None:
            self.stats.save(self.stats_file, radius=self.radius, lag=self.lag)
        names, parts = gather_rows(names, (rows, cover), ctx.world)
        if ctx.rank != 0:
            return
        rows = [row for part in parts for row in part[0]]
        cover = [row for part in parts for row in part[1] or []]

        def record(row, cov):
            return {**uncertainty.summarize(row), **(uncertainty.summarize_coverage(cov) if cov is not None else {})}

        def total(table, width):
            tot = [0.0] * width
            for row in table:
                tot = [a + b for a, b in zip(tot, row)]
            return tot
        scored = len(cover) == len(rows) and len(rows) > 0
        doc = {"radius": self.radius, "lag": self.lag, "floor": self.floor, "min_count": self.min_count, "mask": self.mask,
               "pairs": {name: record(row, cover[i] if scored else None) for i, (name, row) in enumerate(zip(names, rows))},
               "total": record(total(rows, len(uncertainty.SUMS)),
                               total(cover, len(uncertainty.COVERAGE_SUMS)) if scored else None)}
        write_json(self.file, json_strict(doc), allow_nan=False)


class Vortex(Stage):
    """Rates every batch of flows on the device, right after them and on the same stream: vortex_gamma of the flow that is written,
    with the flags of "flag" or "mask" as the mask.  The two bands -- and the picture of Gamma2, with `image` -- go back to the host
    with the flows, where pair() finds the peaks of each pair from its bands; the per-pair sums (pivlfn.vortex.SUMS) stay on the device
    until finish() copies them once."""
    extras = True

    def __init__(self, radius, spacing, image, file, mask=None):
        self.radius, self.spacing, self.image, self.file, self.mask = radius, spacing, image, file, mask      # mask: for vortices.json
        self.min_count = vortex.check_params(radius, spacing, None)
        self._sums, self._peaks = [], []

    def __call__(self, batch):
        v = vortex.vortex_gamma(batch.flow, self.radius, self.spacing, batch.masked()[1], self.min_count)
        self._sums.append(v.sums())
        batch.extras["gamma"] = torch.stack([v.gamma1, v.gamma2], dim=3)      # the .flo layout
        if self.image:          # red is the colour of Gamma2 = 1 in this map: what has no value is black, as in the vorticity pictures
            batch.extras["gamma2"] = viz.scalar_to_color(v.gamma2.contiguous(), -1.0, 1.0, cmap="bwr")

    def pair(self, gamma):
        """The peaks of one pair from its bands on the host ([H,W,2]): VortexField.peaks is plain torch."""
        g = torch.from_numpy(np.ascontiguousarray(gamma)).permute(2, 0, 1).unsqueeze(1)
        flag = torch.zeros(g.shape[1:], dtype=torch.uint8)
        self._peaks.append(vortex.VortexField(g[0], g[1], flag, self.radius, self.spacing).peaks()[0])

    def finish(self, names, ctx):
        """<save>/vortices.json: the parameters, per pair name the peaks of |Gamma2| (VortexField.peaks) and the summary
        (VortexField.summary), and the summary over the run, formed from the per-pair sums in pair order.  Sharded runs: the records of
        all ranks are gathered (gather_rows) and rank 0 writes.  A value that is not finite is written as null."""
        rows = _cat(self._sums).tolist() if self._sums else []
        assert len(rows) == len(names) == len(self._peaks)
        names, parts = gather_rows(names, (rows, self._peaks), ctx.world)
        if ctx.rank != 0:
            return
        rows, peaks = [row for part in parts for row in part[0]], [p for part in parts for p in part[1]]
        total = [0.0] * len(vortex.SUMS)
        for row in rows:
            total = [a + b for a, b in zip(total, row)]
        doc = {"radius": self.radius, "spacing": self.spacing, "min_count": self.min_count, "mask": self.mask, "threshold": vortex.CORE,
               "pairs": {name: {"peaks": p, "summary": vortex.summarize(row)} for name, p, row in zip(names, peaks, rows)},
               "total": vortex.summarize(total)}
        write_json(self.file, json_strict(doc), allow_nan=False)


class Pod(Stage):
    """Stores every batch of flows in a FlowPOD, created at the first batch's size -- what the .flo files get after "replace", the raw
    flow with the flags as the mask after "flag" and "mask" -- and decomposes them after the directory.  `pairs`: how many pairs
the directory has (check_pod_pairs); `wheel`: the name of the colour wheel the modes are drawn with, or None for no pictures."""

    def __init__(self, modes, cell, pairs, file, wheel):
        self.modes, self.cell, self.capacity, self.file, self.wheel = modes, cell, pairs, file, wheel
        self.pod = None

    def __call__(self, batch):
        if self.pod is None:
            H, W = batch.flow.size(2), batch.flow.size(3)
            need, free = FlowPOD.store_bytes(H, W, self.capacity, self.cell), torch.cuda.mem_get_info(batch.flow.device)[0]
            if need > free // 2:
                raise SystemExit(f"run.py: --pod: the store of {self.capacity} snapshots of {H} x {W} takes {need / 2**30:.1f} GiB, more "
                                 f"than half of the {free / 2**30:.1f} GiB free on the device; decompose block means with --pod-cell C")
            self.pod = FlowPOD(H, W, self.capacity, self.cell, device=batch.flow.device)
        self.pod.update(*batch.masked())

    def finish(self, names, ctx):
        """<save>/pod.npz, one line per mode, and with a wheel the modes as pod_mode<k>.png beside it."""
        res = checked("--pod: ", self.pod.solve, self.modes)
        print(f"POD of {self.pod.n} flows -> '{res.save(self.file)}'")
        for k in range(self.modes):
            print(f"  mode {k + 1}: {100.0 * res.fraction[k]:6.2f} % of the fluctuation energy")
        if self.wheel is not None:
            pics = viz.flow_to_color(torch.from_numpy(res.modes.astype("float32")).to(self.pod.device), None, wheel=self.wheel).cpu().numpy()
            with viz.PngWriter() as pictures:
                for k in range(self.modes):
                    pictures.submit(pics[k], self.file[:-4] + f"_mode{k + 1}.png")


class Ftle(Stage):
    """Carries a FlowMap through the directory's flows in time order, batch by batch and on the same stream -- the raw flow with the
    flags as the mask after "flag" and "mask", the written flow otherwise.  The directory's `pairs` pairs are cut into windows of
    `steps`: a batch that straddles a window end is split there, the window's FTLEField stays on the device and the map is reseeded;
    what is left after the last whole window is counted and not followed.  finish() writes the files."""

    def __init__(self, spacing, steps, pairs, image, vmax, flowdir, file, mask=None):
        self.spacing, self.steps, self.image, self.vmax, self.flowdir, self.file, self.mask = spacing, steps, image, vmax, flowdir, file, mask
        self.windows, self.leftover = pairs // steps, pairs % steps
        self.map, self.fields, self.skipped = None, [], 0

    def __call__(self, batch):
        flow, mask = batch.masked()
        if self.map is None:
            self.map = flowmap.FlowMap(flow.size(2), flow.size(3), self.spacing, device=flow.device)
        at, n = 0, flow.size(0)
        while at < n and len(self.fields) < self.windows:
            take = min(n - at, self.steps - self.map.steps)
            self.map.update(flow[at:at + take], None if mask is None else mask[at:at + take])
            at += take
            if self.map.steps == self.steps:
                self.fields.append(self.map.ftle())
                self.map.reset()
        self.skipped += n - at

    def finish(self, names, ctx):
        """<flow dir>/<first pair of the window>_ftle.flo (bands ftle and stretch, float32), with `image` the picture beside it, and
        <save>/ftle.json: the parameters, per window FTLEField.summary(), and the pairs left over.  A value that is not finite is
        written as null."""
        assert len(self.fields) == self.windows and self.skipped == self.leftover and len(names) == self.windows * self.steps + self.leftover
        doc = {"spacing": self.spacing, "steps": self.steps, "iters": None if self.map is None else self.map.iters, "mask": self.mask,
               "lattice": None if self.map is None else [self.map.h, self.map.w], "windows": {}, "leftover": self.leftover}
        with FloWriter() as writer, viz.PngWriter() as pictures:
            for k, field in enumerate(self.fields):
                first = names[k * self.steps]
                summary = field.summary()
                doc["windows"][os.path.basename(flowname_modifier(first, self.flowdir, ext="", pair=False))] = summary
                bands = torch.stack([field.ftle, field.stretch.to(torch.float32)], dim=2)
                writer.submit(bands.cpu().numpy(), flowname_modifier(first, self.flowdir, ext="_ftle.flo", pair=False))
                if self.image:
                    top = self.vmax if self.vmax is not None else summary["max_ftle"]
                    top = top if math.isfinite(top) and top > 0.0 else 1.0            # nothing defined, or nothing stretched
                    rgb = viz.scalar_to_color(field.ftle[None].contiguous(), 0.0, top, cmap="gray", bad=QUALITY_BAD_RGB)
                    pictures.submit(rgb[0].cpu().numpy(), flowname_modifier(first, self.flowdir, ext="_ftle.png", pair=False))
        write_json(self.file, json_strict(doc), allow_nan=False)
        print(f"FTLE over {self.windows} window(s) of {self.steps} pairs ({self.leftover} pairs left over) -> '{self.file}'")


def check_ftle_pairs(pairs, steps, inputdir):
    """The pairs per window in effect (`steps` None: the whole directory)."""
    steps = pairs if steps is None else steps
    if pairs < 1 or steps > pairs:
        raise SystemExit(f"run.py: --ftle: '{inputdir}' has {pairs} pairs, fewer than the {steps} of one window")
    return steps


def check_pod_pairs(pairs, modes, inputdir):
    if not 2 <= pairs <= 4096:
        raise SystemExit(f"run.py: --pod: '{inputdir}' has {pairs} pairs; the method of snapshots here takes 2..4096 (decompose a "
                         "part of the recording with --start / --num_images)")
    if modes > pairs - 1:
        raise SystemExit(f"run.py: --pod {modes}: '{inputdir}' has {pairs} pairs, which carry at most {pairs - 1} modes")


def make_stages(args, layout, inputdir, net, device, rank, world, truth_paths=None):
    """The stages the command line asks for, for one input directory, in their fixed order: what validation sets is what every later
    stage sees.  `truth_paths`: the truth_files() of the whole directory."""
    stages = []
    if args.pod is not None:                # refused before anything is launched
        pairs = len(Run(root=inputdir, is_pair=args.is_pair, n_images=args.num_images, start_at=args.start))
        check_pod_pairs(pairs, args.pod, inputdir)
    if args.ftle is not None:
        ftle_pairs = len(Run(root=inputdir, is_pair=args.is_pair, n_images=args.num_images, start_at=args.start))
        ftle_steps = check_ftle_pairs(ftle_pairs, args.ftle_steps, inputdir)
    if args.spectrum is not None:
        check_spectrum_pairs(len(Run(root=inputdir, is_pair=args.is_pair, n_images=args.num_images, start_at=args.start)), args.spectrum,
                             inputdir)
    if args.pressure is not None:
        check_pressure_pairs(len(Run(root=inputdir, is_pair=args.is_pair, n_images=args.num_images, start_at=args.start)), inputdir)
    if args.validate is not None:
        stages.append(Validate(args.validate, args.validate_radius, args.validate_spacing, args.validate_eps, args.validate_thresh,
                               layout.sibling("validation.json")))
    if args.smooth is not None:
        stages.append(Smooth(args.smooth, 1e-8 if args.smooth_tol is None else args.smooth_tol, layout.sibling("smooth.json")))
    if args.stats:
        stages.append(Stats(layout.sibling("stats.npz")))
    if args.twopoint is not None:
        stages.append(TwoPoint(args.twopoint, args.twopoint_step or 1, args.twopoint_mean, layout.sibling("twopoint.npz"),
                               layout.sibling("twopoint.json")))
    if args.ensemble is not None:
        stages.append(Ensemble(args.ensemble, args.ensemble_step or args.ensemble // 2, 8 if args.ensemble_search is None else args.ensemble_search,
                               args.ensemble_predictor, layout.sibling("ensemble.npz"), layout.sibling("ensemble.flo"),
                               layout.sibling("ensemble.json")))
    if args.pdf is not None:
        stages.append(Distribution(pdf_params(args), args.pdf_mean, args.pdf_normalise, args.pdf_image, layout.sibling("pdf.npz"),
                                   layout.sibling("pdf.json"), layout.sibling("pdf_joint.png")))
    if args.spectrum is not None:
        stages.append(Spectrum(args.spectrum, args.spectrum_overlap, args.spectrum_cell or 1, 1.0 if args.spectrum_fps is None else args.spectrum_fps,
                               args.spectrum_image, layout.sibling("spectrum.npz"), layout.sibling("spectrum.json"),
                               layout.sibling("spectrum_peak.png")))
    if args.pressure is not None:
        stages.append(Pressure(pressure_params(args), args.pressure_image, layout.flow, layout.sibling("pressure.json")))
    if args.truth is not None:
        lo, hi = shard_bounds(len(truth_paths), rank, world)
        stages.append(Truth(net, truth_paths[lo:hi], args.truth_levels, layout.sibling("errors.json"), layout.sibling("error_maps.npz"),
                            pin=device.type == "cuda"))
    if _used(args, PICTURE_FLAGS):
        stages.append(Pictures(args.color, args.color_max, args.color_wheel, args.vort_image, args.vort_max, args.quiver))
    if args.quality is not None:
        stages.append(Quality(args.quality, args.quality_image, layout.sibling("quality.json"),
                              args.validate if args.validate in ("flag", "mask") else None))
    if args.uncertainty is not None:
        stages.append(Uncertainty(args.uncertainty, 2 if args.uncertainty_lag is None else args.uncertainty_lag, args.uncertainty_image,
                                  0.5 if args.uncertainty_max is None else args.uncertainty_max, layout.sibling("uncertainty.json"),
                                  layout.sibling("uncertainty_stats.npz") if args.stats else None,
                                  args.validate if args.validate in ("flag", "mask") else None))
    if args.vortex is not None:
        stages.append(Vortex(args.vortex, args.vortex_spacing or 1, args.vortex_image, layout.sibling("vortices.json"),
                             args.validate if args.validate in ("flag", "mask") else None))
    if args.ftle is not None:
        stages.append(Ftle(args.ftle, ftle_steps, ftle_pairs, args.ftle_image, args.ftle_max, layout.flow, layout.sibling("ftle.json"),
                           args.validate if args.validate in ("flag", "mask") else None))
    if args.pod is not None:
        stages.append(Pod(args.pod, args.pod_cell or 1, pairs, layout.sibling("pod.npz"), (args.color_wheel or "interp") if args.color else None))
    return stages


@dataclass(frozen=True)
class Prep:
    """--background / --minmax / --minmax-floor, checked."""
    background: object      # None, "min" (main_dl takes the minimum over the folder first) or the image, uint8 [H,W,3] on the device
    minmax: int
    floor: int


class _SizedPrep:
    """pivlfn.preproc.Preprocessor that checks the background's size against the first batch and names both sizes if they differ."""

    def __init__(self, background, minmax, floor):
        self.prep, self.checked = Preprocessor(background, minmax, floor), background is None

    def __call__(self, frames):
        if not self.checked:
            have, want = tuple(self.prep.background.shape[:2]), tuple(frames.shape[1:3])
            if have != want:
                raise SystemExit(f"run.py: --background is {have[0]} x {have[1]} (H x W) but the frames are {want[0]} x {want[1]}")
            self.checked = True
        return self.prep(frames)


def background_min(ds, device, batch):
    """The per-pixel minimum over every distinct frame of `ds` (a Run), each decoded once on PairLoader's threads: a
    pivlfn.preproc.FrameBackground.  All frames must have one size."""
    paths = list(dict.fromkeys(p for pair in ds.image_list for p in pair))
    odd = len(paths) % 2
    twos = SimpleNamespace(image_list=[[paths[i], paths[min(i + 1, len(paths) - 1)]] for i in range(0, len(paths), 2)])
    twos.name_list = [a for a, _ in twos.image_list]
    loader = PairLoader(twos, 0, len(twos.image_list), batch, depth=2, pin=device.type == "cuda", share=1)
    bg, seen = None, 0
    try:
        for names, a8, b8 in loader:
            seen += len(names)
            if odd and seen == len(twos.image_list):
                b8 = b8[:-1]                        # the last frame of an odd count stands in both places of its pair
            if bg is None:
                bg = FrameBackground(a8.size(1), a8.size(2), device)
            if tuple(a8.shape[1:3]) != (bg.H, bg.W):
                raise SystemExit(f"run.py: --background min needs frames of one size: '{names[0]}' is {a8.size(1)} x {a8.size(2)} "
                                 f"(H x W), the frames before it are {bg.H} x {bg.W}")
            for t in (a8, b8):
                if t.size(0):
                    bg.update(t.to(device, non_blocking=True))
            torch.cuda.current_stream(device).synchronize()      # the loader refills its pinned staging once a batch is consumed
    except ValueError as e:                         # PairLoader: the two frames of one pair differ in size
        raise SystemExit(f"run.py: --background min needs frames of one size: {e}")
    finally:
        loader.close()
    assert bg is not None and bg.count == len(paths)
    return bg


def main_dl(net, inputdir, layout, is_pair, start_id, num_images, device, batch, rank=0, world=1, stages=(), prep=None):
    """Every pair of the folder through `estimate` (reference main_dl, run.py:137-168) and then through `stages` (make_stages), whose
    files are written after the last pair.  `prep` (a Prep): the frames go through pivlfn.preproc.preprocess_frames; a background of
    "min" is computed from the folder first and written beside args.txt."""
    try:
        savedir = layout.flow
        os.makedirs(savedir, exist_ok=True)
        ds = Run(root=inputdir, is_pair=is_pair, n_images=num_images, start_at=start_id)
        if prep is not None:
            background = prep.background
            if isinstance(background, str):
                bg = background_min(ds, device, batch)
                print(f"Background: minimum over {bg.count} frames -> '{bg.save(layout.sibling('background.png'))}'")
                background = bg.image()
            prep = _SizedPrep(background, prep.minmax, prep.floor)
        lo, hi = shard_bounds(len(ds), rank, world)
        print(f"Processing {hi - lo} of {len(ds)} pairs of images (rank {rank}/{world})...")
        loader = PairLoader(ds, lo, hi, batch, depth=2, pin=device.type == "cuda")
        est = Estimator(stages)
        painter = next((s for s in stages if isinstance(s, Pictures)), None)
        vortices = next((s for s in stages if isinstance(s, Vortex)), None)
        if painter is not None and painter.color and rank == 0:
            viz.write_png(os.path.join(savedir, "color_wheel.png"), viz.color_wheel_image(wheel=painter.color_wheel, device=device).cpu().numpy())
        seen = []

        def sink(flow, name, extras=None):
            seen.append(name)
            writer.submit(flow, flowname_modifier(name, savedir, pair=False))
            if extras and "qual" in extras:
                writer.submit(extras["qual"], flowname_modifier(name, savedir, ext="_qual.flo", pair=False))
            if extras and "unc" in extras:
                writer.submit(extras["unc"], flowname_modifier(name, savedir, ext="_unc.flo", pair=False))
            if extras and "gamma" in extras:
                writer.submit(extras["gamma"], flowname_modifier(name, savedir, ext="_gamma.flo", pair=False))
                vortices.pair(extras["gamma"])
            for key, ext in (("color", "_out.png"), ("vort", "_vort.png"), ("corr", "_corr.png"), ("unc_image", "_unc.png"),
                             ("gamma2", "_gamma2.png")):
                if extras and key in extras:
                    pictures.submit(extras[key], flowname_modifier(name, savedir, ext=ext, pair=False))
            if extras and "quiver_mean" in extras:          # pyplot is not thread-safe: the arrows are drawn here
                viz.draw_quiver(extras["quiver_mean"], extras["quiver_count"], painter.cell(*flow.shape[:2]), *flow.shape[:2],
                                flowname_modifier(name, savedir, ext="_quiver.png", pair=False))
        try:
            with FloWriter() as writer:
                if not any(s.extras for s in stages):
                    n = stream_pairs(net, loader, device, sink, estimate_fn=est, prep=prep)
                else:
                    with viz.PngWriter() as pictures:
                        n = stream_pairs(net, loader, device, sink, estimate_fn=est, prep=prep, extras=est.extras)
        finally:
            loader.close()
        assert n == hi - lo
        ctx = SimpleNamespace(rank=rank, world=world, device=device)
        for stage in stages:
            stage.finish(seen, ctx)
        return hi - lo
    finally:                                # whatever failed, and where: a stage may hold threads
        for stage in stages:
            stage.close()


def main_mod(net, inputdir, savedir, start_id, num_images, device, mod_factors: Sequence[Tuple[float, float]], batch,
             rank=0, world=1):
    """Consecutive frames x (brightness, contrast) combinations (reference main, run.py:100-134)."""
    os.makedirs(savedir, exist_ok=True)
    ds = _FrameSequence(inputdir, num_images, start_id)
    lo, hi = shard_bounds(len(ds), rank, world)
    print(f"Processing {hi - lo} of {len(ds)} pairs of images x {len(mod_factors)} modifications (rank {rank}/{world})...")
    loader = PairLoader(ds, lo, hi, batch, depth=2, pin=device.type == "cuda")
    try:
        with FloWriter() as writer:
            n = stream_pairs(net, loader, device,
                             lambda flow, first, mod: writer.submit(flow, mod_flow_name(first, savedir, mod)),
                             mods=list(mod_factors))
    finally:
        loader.close()
    assert n == (hi - lo) * len(mod_factors)
    return n


def args_lines(args) -> List[str]:
    """The lines of args.txt.  The flags of validation, pre-processing, scoring, pictures, quality, vortices and flow maps appear only in runs that use them:
    without them the file is what it was before they existed."""
    prep, pictures = _used(args, PREP_FLAGS), _used(args, PICTURE_FLAGS)
    return [f"{k}: {v}\n" for k, v in sorted(vars(args).items())
            if not ((args.validate is None and k.startswith("validate")) or (not prep and k in PREP_FLAGS) or
                    (args.truth is None and k in TRUTH_FLAGS) or (not pictures and k in PICTURE_FLAGS) or
                    (args.quality is None and k in QUALITY_FLAGS) or (args.vortex is None and k in VORTEX_FLAGS) or
                    (args.uncertainty is None and k in UNCERTAINTY_FLAGS) or
                    (args.pod is None and k in POD_FLAGS) or (args.ftle is None and k in FTLE_FLAGS) or
                    (args.pdf is None and k in PDF_FLAGS) or
                    (args.twopoint is None and k in TWOPOINT_FLAGS) or (args.spectrum is None and k in SPECTRUM_FLAGS) or
                    (args.pressure is None and k in PRESSURE_FLAGS) or (args.smooth is None and k in SMOOTH_FLAGS) or
                    (args.ensemble is None and k in ENSEMBLE_FLAGS))]


def load_weights(args) -> Tuple[dict, str]:
    if args.weights and not args.synthetic_weights:
        if not os.path.isfile(args.weights):
            raise ValueError("Unknown params input!")
        return torch.load(args.weights, map_location="cpu"), os.path.splitext(os.path.basename(args.weights))[0]
    tag = args.model + ("2" if args.version == 2 else "")
    return synth.generate_weights(tag, 0), f"{tag}-synthetic"


def refuse_mods(args, what):
    """`what`: the flags and their verb, "--stats is"."""
    if args.brightness is not None or args.contrast is not None:
        raise SystemExit(f"run.py: {what} not available with -b/-c (every combination is a different experiment)")


def refuse_sharded(flag, reason):
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(f"run.py: {flag} needs a single process ({reason})")


def main(argv: Optional[List[str]] = None) -> int:
    args = parser.parse_args(argv)
    if args.stats:
        refuse_mods(args, "--stats is")
        refuse_sharded("--stats", "run.py has no process group to merge the statistics; the sharded path for statistics is "
                                  "pivlfn.sequence.run_sequence")
    if (args.twopoint_step is not None or args.twopoint_mean is not None) and args.twopoint is None:
        raise SystemExit("run.py: --twopoint-step and --twopoint-mean need --twopoint")
    if args.twopoint is not None:
        refuse_mods(args, "--twopoint is")
        refuse_sharded("--twopoint", "run.py has no process group to merge the sums of the ranks")
        checked("--twopoint: ", check_twopoint, args.twopoint, 1 if args.twopoint_step is None else args.twopoint_step)
        if args.twopoint_mean is not None and not os.path.isfile(args.twopoint_mean):
            raise SystemExit(f"run.py: --twopoint-mean '{args.twopoint_mean}' is not a file")
    if _used(args, ENSEMBLE_FLAGS[1:]) and args.ensemble is None:
        raise SystemExit("run.py: --ensemble-step, --ensemble-search and --ensemble-predictor need --ensemble")
    if args.ensemble is not None:
        refuse_mods(args, "--ensemble is")
        refuse_sharded("--ensemble", "run.py has no process group to merge the sums of the ranks")
        checked("--ensemble: ", ensemble.check_params, args.ensemble, args.ensemble // 2 if args.ensemble_step is None else args.ensemble_step,
                8 if args.ensemble_search is None else args.ensemble_search)
        if args.ensemble_predictor is not None and not os.path.isfile(args.ensemble_predictor):
            raise SystemExit(f"run.py: --ensemble-predictor '{args.ensemble_predictor}' is not a file")
    if _used(args, PDF_FLAGS[1:]) and args.pdf is None:
        raise SystemExit("run.py: --pdf-range, --pdf-mean, --pdf-normalise, --pdf-hole and --pdf-image need --pdf")
    if args.pdf is not None:
        refuse_mods(args, "--pdf is")
        refuse_sharded("--pdf", "run.py has no process group to merge the sums of the ranks")
        if args.pdf_normalise and args.pdf_mean is None:
            raise SystemExit("run.py: --pdf-normalise needs --pdf-mean (the rms of a --stats run)")
        checked("--pdf: ", check_pdf, *pdf_params(args))
        if args.pdf_mean is not None and not os.path.isfile(args.pdf_mean):
            raise SystemExit(f"run.py: --pdf-mean '{args.pdf_mean}' is not a file")
    if _used(args, SPECTRUM_FLAGS[1:]) and args.spectrum is None:
        raise SystemExit("run.py: --spectrum-overlap, --spectrum-cell, --spectrum-fps and --spectrum-image need --spectrum")
    if args.spectrum is not None:
        refuse_mods(args, "--spectrum is")
        if args.is_pair:
            raise SystemExit("run.py: --spectrum is not available with -p (the pairs of a pair folder are not a time series)")
        refuse_sharded("--spectrum", "a spectrum follows the pairs of a directory in order, on one device")
        checked("--spectrum: ", check_spectrum, args.spectrum, args.spectrum_overlap, "hann", "constant",
                1 if args.spectrum_cell is None else args.spectrum_cell, 1.0 if args.spectrum_fps is None else args.spectrum_fps)
    if _used(args, PRESSURE_FLAGS[1:]) and args.pressure is None:
        raise SystemExit("run.py: --pressure-rho, --pressure-nu, --pressure-dt, --pressure-calib, --pressure-tol and --pressure-image need "
                         "--pressure")
    if args.pressure is not None:
        refuse_mods(args, "--pressure is")
        if args.is_pair:
            raise SystemExit("run.py: --pressure is not available with -p (the pairs of a pair folder are not a time series)")
        refuse_sharded("--pressure", "a pressure field follows the pairs of a directory in order, on one device")
        checked("--pressure: ", check_pressure, *pressure_params(args))
    if args.smooth_tol is not None and args.smooth is None:
        raise SystemExit("run.py: --smooth-tol needs --smooth")
    if args.smooth is not None:
        refuse_mods(args, "--smooth is")
        refuse_sharded("--smooth", "smooth.json lists the pairs of one process")
        checked("--smooth: ", check_smooth, None, args.smooth, 1e-8 if args.smooth_tol is None else args.smooth_tol)
    if args.pod_cell is not None and args.pod is None:
        raise SystemExit("run.py: --pod-cell needs --pod")
    if args.pod is not None:
        refuse_mods(args, "--pod is")
        refuse_sharded("--pod", "the snapshots of one decomposition live on one device")
        if not 1 <= args.pod <= 64:
            raise SystemExit(f"run.py: --pod {args.pod}: the number of modes must be 1..64")
        if args.pod_cell is not None and not 1 <= args.pod_cell <= 32768:
            raise SystemExit(f"run.py: --pod-cell {args.pod_cell}: the cell must be 1..32768")
    if args.validate is not None:
        refuse_mods(args, "--validate is")
        refuse_sharded("--validate", "validation.json lists the pairs of one process")
        checked("", check_validate, args.validate_radius, args.validate_spacing, args.validate_eps, args.validate_thresh, args.validate)
    if args.truth_levels and args.truth is None:
        raise SystemExit("run.py: --truth-levels needs --truth")
    truth_paths = {}
    if args.truth is not None:
        refuse_mods(args, "--truth is")
        if not os.path.isdir(args.truth):
            raise SystemExit(f"run.py: --truth '{args.truth}' is not a directory")
        # every truth file of every directory, before the first forward
        truth_paths = {imdir: truth_files(Run(root=imdir, is_pair=args.is_pair, n_images=args.num_images, start_at=args.start),
                                          args.truth, args.truth_levels) for imdir in args.input}
    prep = None
    if _used(args, PREP_FLAGS):
        refuse_mods(args, "--background / --minmax are")
        if args.background == "min":
            refuse_sharded("--background min", "run.py has no process group to merge the minima of the ranks; compute the background "
                                               "once and pass --background FILE")
        if args.minmax_floor is not None and args.minmax is None:
            raise SystemExit("run.py: --minmax-floor needs --minmax")
        if args.background not in (None, "min") and not os.path.isfile(args.background):
            raise SystemExit(f"run.py: --background '{args.background}' is neither 'min' nor an image file")
        prep = Prep(args.background, 0 if args.minmax is None else args.minmax, 16 if args.minmax_floor is None else args.minmax_floor)
        checked("", check_prep, prep.minmax, prep.floor)
    if _used(args, PICTURE_FLAGS):
        refuse_mods(args, "--color / --vort-image / --quiver are")
        if (args.color_max is not None or args.color_wheel is not None) and not args.color:
            raise SystemExit("run.py: --color-max and --color-wheel need --color")
        if args.vort_max is not None and not args.vort_image:
            raise SystemExit("run.py: --vort-max needs --vort-image")
        for flag, x in (("--color-max", args.color_max), ("--vort-max", args.vort_max)):
            if x is not None and not (math.isfinite(x) and x > 0):
                raise SystemExit(f"run.py: {flag} {x} must be a finite positive number")
        if args.quiver is not None:
            if not 0 <= args.quiver <= 32768:
                raise SystemExit(f"run.py: --quiver {args.quiver}: the cell must be 1..32768")
            try:
                viz._pyplot()                       # once, here, and not at the first pair
            except ImportError as e:
                raise SystemExit(f"run.py: --quiver: {e}")
    if args.quality_image and args.quality is None:
        raise SystemExit("run.py: --quality-image needs --quality")
    if args.quality is not None:
        refuse_mods(args, "--quality is")
        checked("--quality: ", quality.check_params, args.quality, 1.0 / 255.0, None)
    if _used(args, UNCERTAINTY_FLAGS[1:]) and args.uncertainty is None:
        raise SystemExit("run.py: --uncertainty-lag, --uncertainty-image and --uncertainty-max need --uncertainty")
    if args.uncertainty is not None:
        refuse_mods(args, "--uncertainty is")
        checked("--uncertainty: ", uncertainty.check_params, args.uncertainty, 2 if args.uncertainty_lag is None else args.uncertainty_lag,
                1.0 / 255.0, None)
        if args.uncertainty_max is not None and not args.uncertainty_image:
            raise SystemExit("run.py: --uncertainty-max needs --uncertainty-image")
        if args.uncertainty_max is not None and not (math.isfinite(args.uncertainty_max) and args.uncertainty_max > 0):
            raise SystemExit(f"run.py: --uncertainty-max {args.uncertainty_max} must be a finite positive number")
    if (args.vortex_image or args.vortex_spacing is not None) and args.vortex is None:
        raise SystemExit("run.py: --vortex-spacing and --vortex-image need --vortex")
    if args.vortex is not None:
        refuse_mods(args, "--vortex is")
        checked("--vortex: ", vortex.check_params, args.vortex, 1 if args.vortex_spacing is None else args.vortex_spacing, None)
    if (args.ftle_steps is not None or args.ftle_image or args.ftle_max is not None) and args.ftle is None:
        raise SystemExit("run.py: --ftle-steps, --ftle-image and --ftle-max need --ftle")
    if args.ftle is not None:
        refuse_mods(args, "--ftle is")
        if args.is_pair:
            raise SystemExit("run.py: --ftle is not available with -p (the pairs of a pair folder are not consecutive in time)")
        refuse_sharded("--ftle", "a flow map follows the pairs of a directory in order, on one device")
        checked("--ftle: ", flowmap.check_params, None, None, args.ftle)
        if args.ftle_steps is not None and args.ftle_steps < 1:
            raise SystemExit(f"run.py: --ftle-steps {args.ftle_steps}: a window has at least 1 pair")
        if args.ftle_max is not None and not args.ftle_image:
            raise SystemExit("run.py: --ftle-max needs --ftle-image")
        if args.ftle_max is not None and not (math.isfinite(args.ftle_max) and args.ftle_max > 0):
            raise SystemExit(f"run.py: --ftle-max {args.ftle_max} must be a finite positive number")
    if args.no_cuda or not torch.cuda.is_available():
        raise SystemExit("run.py: this build has no CPU path (the reference's correlation has none either, "
                         "src/correlation.py:339-340); a GPU is required")
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())   # ranks may share a card
    torch.cuda.set_device(device)
    if (args.truth is not None or args.quality is not None or args.vortex is not None or args.uncertainty is not None) and world > 1:        # the ranks' records and maps meet on rank 0: a small host-side exchange
        import torch.distributed as dist
        if not dist.is_initialized():
            dist.init_process_group("gloo", rank=rank, world_size=world)
    weights, netname = load_weights(args)
    net = Network(model=args.model, params=weights, version=args.version).to(device).eval()
    if args.precision is not None:
        net.precision = args.precision
    if prep is not None and prep.background not in (None, "min"):
        prep = Prep(FrameBackground.load(prep.background, device).image(), prep.minmax, prep.floor)
    mods = None
    if args.brightness is not None or args.contrast is not None:
        mods = list(product(tuple(args.brightness or (1.0,)), tuple(args.contrast or (1.0,))))
    total = 0
    for i, imdir in enumerate(args.input):
        print(f"---------- Processing images from directory #{str(i).zfill(2)}: '{imdir}'")
        lay = OutputLayout.of(args.output, netname, imdir, args.start, args.num_images)
        os.makedirs(lay.save, exist_ok=True)
        if rank == 0:
            with open(lay.args_file, "w") as f:
                f.writelines(args_lines(args))
        if mods is None:
            total += main_dl(net, imdir, lay, args.is_pair, args.start, args.num_images, device, args.batch, rank, world,
                             make_stages(args, lay, imdir, net, device, rank, world, truth_paths.get(imdir)), prep)
        else:
            total += main_mod(net, imdir, lay.flow, args.start, args.num_images, device, mods, args.batch, rank, world)
    if (args.truth is not None or args.quality is not None or args.vortex is not None or args.uncertainty is not None) and world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    print(f"Finish processing {total} flow fields")
    return total


if __name__ == "__main__":
    main()
