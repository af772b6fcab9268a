/*
 * pivlfn.h -- C ABI of libpivlfn.so: the MI355X (gfx950) PIV-LiteFlowNet inference hot path.
 *
 * This is the drop-in boundary for the reference's src/models.py + src/correlation.py.  Every entry
 * point takes plain device pointers, sizes and a hipStream_t (passed as void*); nothing here
 * allocates per call (outputs and the workspace are the caller's), every function returns 0 on
 * success or a non-zero code, and pivlfn_last_error() gives the thread-local message.
 * All tensors are fp32.  "NCHW" tensors are contiguous, exactly what the reference's Python passes.
 * Citations are into /root/reference/.
 */
#ifndef PIVLFN_H
#define PIVLFN_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PIVLFN_OK            0
#define PIVLFN_ERR_ARG       1   /* bad shape / null pointer / unsupported configuration */
#define PIVLFN_ERR_HIP       2   /* a HIP runtime call failed (message has the hipError string) */
#define PIVLFN_ERR_WORKSPACE 3   /* workspace too small */
#define PIVLFN_ERR_WEIGHTS   4   /* state dict does not match the network layout */

typedef struct pivlfn_net pivlfn_net;   /* opaque: packed weights of one network on one device */

/* One entry of a state dict (host memory, fp32, contiguous).  Same names and shapes as
 * LiteFlowNet.state_dict() in src/models.py:305-317 (key pattern in SURVEY.md section 8 a10). */
typedef struct {
    const char  *name;
    const float *data;
    int          ndim;
    int          shape[4];
} pivlfn_tensor;

const char *pivlfn_last_error(void);
/* ABI version.  3 (round 6): + pivlfn_conv2d_nhwc_wino_b3, PIVLFN_PRECISION_F32_WINO_MFMA32; - pivlfn_conv2d_nhwc_wino4 (now exported by the tools build only).  2 (round 4): + pivlfn_warp_corr_nhwc_timed, pivlfn_conv2d_nhwc_wino4, pivlfn_conv_create_cat, pivlfn_conv2d_nhwc_cat; since 1 also pivlfn_conv2d_nhwc_wino and PIVLFN_PRECISION_F32_DIRECT
 * (added in round 3 without a bump); since 3 also the host-only pivlfn_conv2d_nhwc_plan, pivlfn_conv2d_nhwc_kernel_plan and pivlfn_conv_head_nhwc_plan, and
 * pivlfn_conv2d_nhwc_dist_b3 with its host-only pivlfn_conv2d_nhwc_dist_b3_plan.  No entry point of version 1 changed its signature or meaning. */
int         pivlfn_abi_version(void);

/* The library keeps no process-global mutable state: entry points may be called concurrently from several threads, on
 * several devices and streams (one pivlfn_net / pivlfn_conv handle per device; a handle is used by one thread at a time).
 * Kernel-variant knobs for in-process A/B timing exist only in the separate tools build (libpivlfn_tools.so, compiled with
 * -DPIVLFN_TOOLS and loaded by tools/ alone); libpivlfn.so does not export pivlfn_tune. */
#ifdef PIVLFN_TOOLS
int         pivlfn_tune(int knob, int value);
#endif

/* ---- custom op: replaces _FunctionCorrelation.forward, src/correlation.py:287-344 (+ kernels :9-104)
 * first, second: NCHW [B,C,H,W]; out: NCHW [B,49,ceil(H/stride),ceil(W/stride)];
 * out[b,7(dy+3)+(dx+3),y,x] = (1/C) sum_c first[b,c,s*y,s*x] * second[b,c,s*(y+dy),s*(x+dx)], zeros outside.
 * 1 <= stride <= 4, PIVLFN_ERR_ARG otherwise: one range for this entry point, pivlfn_corr_bwd and the two fused ones. */
int pivlfn_corr_fwd(const float *first, const float *second, float *out,
                    int B, int C, int H, int W, int stride, void *stream);

/* ---- backward of the custom op: replaces _FunctionCorrelation.backward, src/correlation.py:348-405 (+ kernels :106-234).
 * grad_out: NCHW [B,49,ceil(H/stride),ceil(W/stride)]; grad_first / grad_second: NCHW [B,C,H,W], every element written
 * (exact zeros off the stride grid); either may be NULL (needs_input_grad false, :353-356).
 * 1 <= stride <= 4 as for the forward, PIVLFN_ERR_ARG otherwise. */
int pivlfn_corr_bwd(const float *first, const float *second, const float *grad_out, float *grad_first, float *grad_second,
                    int B, int C, int H, int W, int stride, void *stream);

/* Channels per workgroup (16, 8 or 4) of the pivlfn_corr_bwd launch of this size: the launch policy, a function of the size
 * alone, exported so that tests can tell which grouping a shape runs on (the gradients' bits do not depend on it).  No launch,
 * no GPU needed; 0 for a shape or stride pivlfn_corr_bwd refuses.  Added without an ABI bump (additive). */
int pivlfn_corr_bwd_channel_group(int B, int C, int H, int W, int stride);

/* ---- replaces backwarp(), src/models.py:20-35.  in: NCHW [B,C,H,W]; flow: NCHW [B,2,H,W] (pixels);
 * out[b,c,y,x] = bilinear(in[b,c], x + flow[b,0,y,x], y + flow[b,1,y,x]), zeros outside.
 * A flow of any finite size is in range (a sample far outside gives zero); a NaN flow component gives a zero output pixel:
 * the tap positions are clamped with fmaxf / fminf, which drop a NaN, so no tap of that pixel lies inside the image. */
int pivlfn_backwarp(const float *in, const float *flow, float *out,
                    int B, int C, int H, int W, void *stream);

/* ---- fused Matching front end: backwarp(second, flow*flow_scale) then correlation, then optional
 * LeakyReLU(0.1): src/models.py:171-184.  NCHW in / NCHW out, flow may be NULL (level 6).
 * 1 <= stride <= 4, PIVLFN_ERR_ARG otherwise. */
int pivlfn_warp_corr_fwd(const float *first, const float *second, const float *flow, float flow_scale,
                         float *out, int B, int C, int H, int W, int stride, int leaky, void *stream);

/* ---- the same kernel on the network's internal channels-last layout (what pivlfn_forward launches;
 * exported for benchmarks and roofline measurement).  first/second: [B,H,W,C]; flow: [B,H,W,4] (u,v,0,0)
 * or NULL; out: [B,Ho,Wo,56] (49 displacements + 7 zero lanes). C must be a multiple of 32.
 * 1 <= stride <= 4, PIVLFN_ERR_ARG otherwise. */
int pivlfn_warp_corr_nhwc(const float *first, const float *second, const float *flow, float flow_scale,
                          float *out, int B, int C, int H, int W, int stride, int leaky, void *stream);

/* ---- measurement hook: `launches` (1..256) back-to-back launches of pivlfn_warp_corr_nhwc on `stream`, each dispatch carrying
 * its own start / stop events (hipExtLaunchKernelGGL: the dispatch's begin / end timestamps, the figure rocprofv3 reports per
 * kernel -- no inter-kernel gap, no marker packets).  Synchronises the stream; *us_dispatch = mean microseconds per dispatch. */
int pivlfn_warp_corr_nhwc_timed(const float *first, const float *second, const float *flow, float flow_scale,
                                float *out, int B, int C, int H, int W, int stride, int leaky, int launches,
                                double *us_dispatch, void *stream);

/* ---- bilinear resize, align_corners=False, NCHW -> NCHW, with a per-channel multiplier
 * (mul[c % 2] when mul != NULL, host pointer to 2 floats): the two interpolate calls and the flow
 * rescale of estimate(), inference.py:46-49 and :57-61. */
int pivlfn_resize_bilinear(const float *in, float *out, int B, int C, int H, int W, int Ho, int Wo,
                           const float *mul, void *stream);

/* ---- stereoscopic 2D3C reconstruction: stereo_run.py:153-163 (_stereo_cal) with stereo/dewarp.py:255-270 (nl_trans) per
 * camera, then stereo/vel3d.py:4-24 (willert), fused with estimate()'s output resize.  Added without an ABI bump (additive).
 * flow: NCHW [2B,2,h,w], batch entry 2b = left camera, 2b+1 = right camera of step b (the raw network output of an interleaved
 * batch, or flows already at H x W);  out: [B,H,W,3] fp32, the band order of a 3-band .flo (U, V, W interleaved).
 * When (h,w) != (H,W) each camera's u, v is resampled exactly as pivlfn_resize_bilinear does and multiplied by mul[0] (u) /
 * mul[1] (v) (host pointer to 2 floats, NULL = 1): the per-camera values equal estimate(..., tensor=True) bit for bit.  When
 * (h,w) == (H,W) the input is read as is and mul is not used (estimate() skips its identity resize).
 * coeff: host pointer to 48 floats, the 24 coefficients A of the left camera then the right one, rounded to fp32.
 * scale: host pointer to 2 floats (calib, fps), or NULL for no m/s scaling.
 * tangents: host pointer to 4 doubles tan(theta_L), tan(theta_R), tan(beta_L), tan(beta_R) (radians, left angles negated).
 * Arithmetic contract, every operation rounded on its own (no fma), correctly rounded divisions; x = u, y = v of one camera:
 *   stage 1, fp32:  P(a..f) = ((((a*x + b*y) + c) + d*(x*x)) + e*(y*y)) + (f*x)*y
 *                   x' = P(A0..A5) / P(A6..A11),  y' = P(A12..A17) / P(A18..A23);  with scale: x' = (x' * calib) * fps, same for y'
 *   stage 2, fp64:  dT = tL - tR;  dB = bR - bL;  du = (uR' - uL') in fp32
 *                   U = ((double)uR' * tL - (double)uL' * tR) / dT
 *                   V = (double)((vL' + vR') / 2 in fp32) + (((double)du * dB) / dT) / 2
 *                   W = (double)du / dT;     out = (float)U, (float)V, (float)W
 * which is what the reference computes under NumPy >= 2 promotion.  A zero denominator in stage 1 gives inf / NaN where numpy
 * does.  Errors (PIVLFN_ERR_ARG): null flow / out / coeff / tangents, a non-positive size, a non-finite tangent, dT == 0. */
int pivlfn_stereo_2d3c(const float *flow, float *out, int B, int h, int w, int H, int W, const float *mul,
                       const float *coeff, const float *scale, const double *tangents, void *stream);

/* ---- derived fields of a flow batch: src/postpro.py, calc_vorticity (:5-24) and de_vort (:27-50).  Added without an ABI bump
 * (additive).  flow: NCHW [B,2,H,W] fp32 (u, v; what estimate(..., tensor=True) returns); out: NCHW [B,3,H,W], fp64 when out_f64 = 1,
 * else fp32 (each plane the fp64 result below rounded once).  Planes: CALC_VORTICITY -> vort, shear, normal; DE_VORT -> vort, uy, vx.
 * Arithmetic contract, every operation rounded on its own (no fma), x[i,j] read with the edge pixel repeated outside the image:
 *   CALC_VORTICITY, fp64:  d = 8.0 * calib;  K = [[1,0,-1],[2,0,-2],[1,0,-1]] / d, each element divided in fp64;
 *                   conv(x, k)[i,j] = sum over the taps of k in row-major order of k[p,q] * (double)x[i+1-p, j+1-q], from +0.0
 *                   (zero taps included: a NaN or inf reaches all 3 x 3 neighbours);  dv = conv(v, K);  du = conv(u, -K^T)
 *                   (K^T negated elementwise: its zero taps are -0.0 for d > 0);  vort = dv - du, shear = dv + du, normal = -(dv + du)
 *                   = scipy.signal.convolve2d(x, k, 'same', boundary='symm') as the reference calls it.
 *   DE_VORT, fp32:  vx = (((v[i+1,j+1] + 2 v[i,j+1]) + v[i-1,j+1]) - ((v[i+1,j-1] + 2 v[i,j-1]) + v[i-1,j-1])) / float32(8 calib)
 *                   uy = (((u[i-1,j-1] + 2 u[i-1,j]) + u[i-1,j+1]) - ((u[i+1,j-1] + 2 u[i+1,j]) + u[i+1,j+1])) / float32(8 calib)
 *                   vort = (double)vx - (double)uy in fp64  (NumPy >= 2 with a Python-float calib).
 * Errors (PIVLFN_ERR_ARG): null flow / out, a non-positive size, H*W >= 2^31, B > 65535, an unknown kind, out_f64 not 0 / 1, a zero or
 * non-finite calib (the reference returns inf / NaN there). */
#define PIVLFN_FIELDS_CALC_VORTICITY 0   /* -> vort, shear, normal */
#define PIVLFN_FIELDS_DE_VORT        1   /* -> vort, uy, vx */
int pivlfn_flow_fields(const float *flow, void *out, int B, int H, int W, double calib, int kind, int out_f64, void *stream);

/* ---- streaming statistics of a flow sequence: acc [7,H,W] fp64 += the per-pixel sums, in this order, of u, v, u*u, v*v, u*v, w,
 * w*w over the B frames of flow (NCHW [B,2,H,W] fp32), w = the vort plane of PIVLFN_FIELDS_CALC_VORTICITY with this calib.  u, v are
 * widened to fp64 exactly, products are rounded in fp64 (no fma), and each pixel adds the frames in frame order to the value acc held
 * before the call (acc is read and written once per call): any split of a sequence into calls gives the same bits, and so does a
 * sequential fp64 loop (acc += u*u, ...).  Errors (PIVLFN_ERR_ARG): null flow / acc, a non-positive size, H*W >= 2^31, a zero or
 * non-finite calib. */
int pivlfn_flow_stats_accumulate(const float *flow, double *acc, int B, int H, int W, double calib, void *stream);

/* ---- vector validation: the normalized median test (Westerweel & Scarano, Exp. Fluids 39, 2005) with masking or median
 * replacement of the rejected vectors.  Added without an ABI bump (additive).
 * flow: NCHW [B,2,H,W] fp32;  flag: [B,H,W] bytes, required in every mode;  out: NCHW [B,2,H,W] (NULL allowed for FLAG only), must
 * not overlap flow;  resid: NCHW [B,2,H,W] or NULL.  At most two launches on `stream`, no allocation, no host synchronisation; a batch
 * equals its frames one at a time, bit for bit.  No output depends on what flag / out / resid held before the call.
 * Arithmetic contract, all fp32, every operation rounded on its own (no fma), the division correctly rounded:
 *   unknown(p) = isnan(u) | isnan(v) | fabs(u) > 1e9f | fabs(v) > 1e9f   (the reference's _unknown_flow, src/utils_plot.py:23, 299-306)
 *   A loaded component is canonicalised by x + 0.0f (-0.0 becomes +0.0) before it is compared or subtracted, so equal values are
 *   indistinguishable and every sorting / selection method gives the same bits; medians are medians of canonicalised values.
 *   Values copied to the output are copied bit for bit.
 *   N(p), p = (y, x): the pixels (y + i*spacing, x + j*spacing), i, j in [-radius, radius], (i, j) != (0, 0), that lie inside the
 *   image and are not unknown; n = |N(p)| is 0..8 (radius 1) or 0..24 (radius 2).  No edge replication.
 *   median of n >= 1 values sorted ascending a[0..n-1]:  n odd -> a[(n-1)/2];  n even -> (a[n/2-1] + a[n/2]) * 0.5f
 *   pass 1, per component c:  m_c = median{U_c(q)},  r_c = median{fabs(U_c(q) - m_c)}  over q in N(p);
 *                   R_c = fabs(U_c(p) - m_c) / (r_c + eps);   flag(p) bit 0 (outlier) = R_u > thresh || R_v > thresh,
 *                   bit 1 = unknown(p).  n = 0 -> R_c = 0, bit 0 clear;  unknown(p) -> R_c = 0, bit 0 clear, bit 1 set.
 *                   resid = R_u, R_v.
 *   pass 2:  FLAG     no flow output.
 *            MASK     flag != 0 -> both components 1e10f (the Middlebury "unknown" value), else copied.
 *            REPLACE  for flag(p) != 0: V(p) = the in-image neighbours (same radius, spacing) with flag(q) == 0 after pass 1 (one
 *                     iteration, a replaced value is never used to replace another);  |V| >= 1 -> out_c = median{U_c(q), q in V(p)};
 *                     |V| = 0 -> the input copied and bit 2 (not replaced) set in flag(p).  flag(p) == 0 -> copied.
 * Errors (PIVLFN_ERR_ARG, before any launch): null flow / flag, null out outside FLAG, out == flow, a non-positive size,
 * H*W >= 2^31, B > 65535, radius not 1 or 2, spacing < 1 or radius*spacing >= 2^15, eps negative or non-finite, thresh non-finite
 * or <= 0, an unknown mode. */
#define PIVLFN_VALIDATE_FLAG    0
#define PIVLFN_VALIDATE_MASK    1
#define PIVLFN_VALIDATE_REPLACE 2
int pivlfn_flow_validate(const float *flow, float *out, unsigned char *flag, float *resid, int B, int H, int W,
                         int radius, int spacing, float eps, float thresh, int mode, void *stream);

/* ---- pivlfn_flow_stats_accumulate with a flag byte per frame and pixel (pivlfn_flow_validate's [B,H,W]): the same acc [7,H,W] fp64,
 * order, fp64 arithmetic and frame order, but frame b adds to u, v, u*u, v*v, u*v at p only if flag[b,p] == 0, and to w, w*w only if
 * all nine edge-clamped 3 x 3 neighbours of p have flag == 0.  cnt [2,H,W] fp64 += the number of additions of either kind (exact
 * integers).  With an all-zero flag the seven sums are bit-identical to pivlfn_flow_stats_accumulate's.  Added without an ABI bump.
 * Errors (PIVLFN_ERR_ARG): as pivlfn_flow_stats_accumulate, and null flag / cnt. */
int pivlfn_flow_stats_accumulate_masked(const float *flow, const unsigned char *flag, double *acc, double *cnt,
                                        int B, int H, int W, double calib, void *stream);

/* ---- image pre-processing in front of the network: background removal and sliding min-max normalisation (Westerweel 1993;
 * Adrian & Westerweel, Particle Image Velocimetry, 2011) of uint8 frames.  The reference has no such step.  Added without an ABI bump
 * (additive).  frames I: [n,H,W,3] bytes;  bg B: [H,W,3] bytes or NULL;  out: NCHW [n,3,H,W] fp32 in [0,1], must not overlap frames or
 * bg.  One launch on `stream`, no allocation, no workspace, no host synchronisation; the channels are treated independently and
 * identically, a batch equals its frames one at a time, and out does not depend on what it held before the call.
 * Arithmetic contract, per frame and channel, integers up to the one division:
 *   1. x = max(I - B, 0) with a background, x = I without: an integer 0..255.
 *   2. k != 0 (k odd, 3 <= k <= 31, r = k/2, n = k*k; 1 <= floor <= 255).  Every coordinate is clamped to the image (edge
 *      replication), in both passes:
 *        lo(p) = min, hi(p) = max of x over the k x k window centred at p;
 *        L(p) = sum of lo, S(p) = sum of hi over the k x k window centred at p (lo and hi taken at the clamped positions);
 *        num = n*x(p) - L(p);  den = max(S(p) - L(p), floor*n);  out = (float)num / (float)den, one correctly rounded division.
 *      num and den stay below 255*31*31 < 2^24, so both conversions are exact, and 0 <= num <= den: every window that contains p has
 *      lo <= x(p) <= hi, and clamping only moves a window position nearer to p.  No clamp of out is needed or applied.
 *   3. k == 0:  out = (float)x / 255.0f, correctly rounded.  With NULL bg these are the bits of ToTensor's byte -> float -> div(255).
 * Errors (PIVLFN_ERR_ARG, before any launch): null frames / out, n, H or W < 1, H*W*3 >= 2^31, n > 65535, k not 0 or odd in 3..31,
 * floor outside 1..255 (whatever k is), out overlapping frames or bg. */
int pivlfn_frames_preprocess(const unsigned char *frames, const unsigned char *bg, float *out, int n, int H, int W,
                             int k, int floor, void *stream);

/* ---- background accumulator of a recording: bg [H,W,3] bytes = min(bg, the minimum over the n frames [n,H,W,3]), in place, byte by
 * byte; start it at 255.  One launch, no temporaries.  Errors (PIVLFN_ERR_ARG): null frames / bg, n, H or W < 1, H*W*3 >= 2^31, bg
 * overlapping frames. */
int pivlfn_frames_background_min(const unsigned char *frames, unsigned char *bg, int n, int H, int W, void *stream);

/* ---- scoring of flows against a known field: the sums behind the reference's src/loss.py (EPE :12-21, L1 :24-38, L2 :41-55, the
 * evaluation branch of MultiScale :144-148, LevelLoss :151-190), per pair.  Added without an ABI bump (additive).
 * flow: NCHW [B,2,h,w] fp32;  truth: NCHW [B,2,H,W] fp32;  mask: [B,H,W] bytes or NULL, nonzero = leave out;  k: pool exponent 0..5,
 * h = H >> k, w = W >> k, H and W multiples of 2^k;  sums: [B,7] fp64;  err_map: NCHW [B,3,h,w] fp32 or NULL;  workspace: 8-byte
 * aligned, at least pivlfn_flow_errors_workspace_bytes(B,H,W) bytes, needs no initial contents.  Launches only on `stream`, no
 * allocation, no host synchronisation, no floating-point atomics.
 * Arithmetic contract, all fp64, every operation rounded on its own (no fma):
 *   pooled truth:  k steps of a 2 x 2 tree on the fp32 values widened to fp64; one step is (a + b) + (c + d), a, b the upper row and
 *                  c, d the lower row of the window;  P = (tree / 4^k) * div_flow  (nn.AvgPool2d(2^k) of div_flow * truth up to rounding).
 *   per pixel:     du = (double)flow_u - P_u, dv likewise;  sq = du*du + dv*dv;  epe = sqrt(sq);  l1 = fabs(du) + fabs(dv).
 *   excluded:      a pixel whose 2^k x 2^k truth window holds an unknown value (NaN or fabs(x) > 1e9f, in u or v: the rule of
 *                  pivlfn_flow_validate) or a nonzero mask byte.  It is +0.0 in every sum and absent from the count and the maximum;
 *                  its terms do not enter a sum (no 0 * NaN).  A non-finite *estimated* flow is not excluded: the sums turn non-finite.
 *   sums[b] = (n, sum l1, sum epe, sum sq, sum du, sum dv, max epe).  Each sum is the root of the same 2 x 2 tree continued over the
 *                  h x w term map until 1 x 1; a map with an odd size is padded with +0.0 on the bottom / right at that step; the
 *                  root + 0.0 is reported (a sum of -0.0 reads +0.0, so further zero padding never shows).  The order is fixed by
 *                  this contract and not by the launch geometry: a pair gives the same bits alone or inside any batch, and from
 *                  run to run.  n is exact.  The maximum is 0 when n = 0 and NaN when an included epe is NaN.
 *   err_map:       planes du, dv, epe, each rounded once from fp64; NaN in all three where the pixel is excluded.
 * Errors (PIVLFN_ERR_ARG, before any launch): null flow / truth / sums / workspace, a non-positive size, k outside 0..5, H or W not
 * a multiple of 2^k, H*W >= 2^31, B > 65535, a non-finite div_flow, a misaligned or too-small workspace. */
size_t pivlfn_flow_errors_workspace_bytes(int B, int H, int W);
int pivlfn_flow_errors(const float *flow, const float *truth, const unsigned char *mask, int B, int H, int W, int k,
                       double div_flow, double *sums, float *err_map, void *workspace, size_t workspace_bytes, void *stream);

/* ---- pivlfn_flow_errors for every flow pivlfn_forward writes into `levels` (coarsest level first, M, S, R per level, packed back to
 * back), in one pass over the truth: sums [B, nlev, 3, 7] fp64, nlev = 7 - lowest_level, entry [b, i, s] = the sums of stage s of
 * level L = 6 - i scored with k = L - 1.  Bit-identical to nlev * 3 calls of pivlfn_flow_errors.  H and W must be multiples of 32.
 * Errors: as pivlfn_flow_errors, and lowest_level outside 1..6. */
int pivlfn_level_errors(const float *levels, int lowest_level, const float *truth, const unsigned char *mask, int B, int H, int W,
                        double div_flow, double *sums, void *workspace, size_t workspace_bytes, void *stream);

/* ---- streaming per-pixel error statistics of a sequence: acc [6,H,W] fp64 += the per-pixel sums, in this order, of 1, du, dv, du*du,
 * dv*dv, epe over the B frames of flow against truth (both NCHW [B,2,H,W] fp32; k = 0, div_flow = 1; du, dv, epe as above), a frame
 * left out at a pixel where its truth is unknown or its mask byte (mask [B,H,W] or NULL) is nonzero.  Each pixel adds the frames in
 * frame order to the value acc held before the call (acc is read and written once per call): any split of a sequence into calls
 * gives the same bits.  Errors (PIVLFN_ERR_ARG): null flow / truth / acc, a non-positive size, H*W >= 2^31. */
int pivlfn_error_stats_accumulate(const float *flow, const float *truth, const unsigned char *mask, double *acc, int B, int H, int W,
                                  void *stream);

/* ---- pictures of flows and scalar fields: the reference's motion_to_color (src/utils_plot.py:199-256) with compute_color
 * (src/utils_color.py:23-93), a colour map for scalar fields, the maxima that normalise both, and cell means for quiver plots.  Added
 * without an ABI bump (additive).  flow: NCHW [B,2,H,W] fp32;  mask: [B,H,W] bytes or NULL, nonzero = leave out (the flag of
 * pivlfn_flow_validate);  pictures: packed bytes [B,H,W,3].  Launches only on `stream`, no allocation, no host synchronisation, no
 * floating-point atomics; no output depends on what it held before the call, and a batch equals its images one at a time.
 *   unknown(p) = isnan(u) | isnan(v) | fabs(u) > 1e9f | fabs(v) > 1e9f      (the reference's _unknown_flow, as pivlfn_flow_validate)
 *
 * pivlfn_flow_maxrad: maxrad[b] (fp32 [B]) = the largest sqrtf(u*u + v*v) over the pixels of image b that are neither unknown nor
 *   masked, each operation rounded on its own in fp32 (no fma); 0 where nothing is left.  A maximum does not depend on the order it is
 *   formed in.  The maximum of a batch is the maximum of its entries.
 *   Deliberate divergence: the reference takes rad.max() over everything, so one 1e10 vector of a masked flow normalises the whole
 *   picture to white; the Middlebury color_flow.cpp it was adapted from leaves unknown flow out, and so does this.  Without unknown
 *   vectors the two agree bit for bit.
 *
 * pivlfn_flow_to_color: norm: fp32 [B] on the device, one normaliser per image (an entry of maxrad, the batch maximum or a fixed
 *   value); n = (norm[b] == 0 ? 1 : norm[b]).  Per pixel, in the types NumPy uses in the reference for float32 flows:
 *     fp32, every operation rounded on its own, both divisions IEEE (no reciprocal):
 *       fx = u / n;  fy = v / n;  rad = sqrtf(fx*fx + fy*fy);  a = atan2f(-fy, -fx) / (float)pi;  fk = (a + 1) / 2 * 54
 *       k0 = (int)fk (truncated, 0..54);  k1 = (k0 + 1) % 55
 *     fp64:  f = (double)fk - k0 (WHEEL_INTERP) or 0 (WHEEL_ORIGINAL);  per channel c of the 55-entry wheel T = colorwheel / 255.0:
 *       col = (1 - f) * T[k0][c] + f * T[k1][c];   rad <= 1: col = 1 - (double)rad * (1 - col);   rad > 1: col = col * 0.75
 *       byte = (int)(255.0 * col), truncated.
 *   ORDER_BGR stores the wheel's (r, g, b) as the reference does (colim[..., 2 - c]); ORDER_RGB stores r, g, b.  Unknown and masked
 *   pixels are 0, 0, 0.  atan2f is the device library's: its last-bit differences from another libm move a byte by at most one
 *   level; signed zeros are honoured (a = -1 for (1, +0.0) is wheel entry 0, a = +1 for (1, -0.0) is entry 54).
 *
 * pivlfn_field_absmax: absmax[b] (fp64 [B]) = the largest fabs(x) over the finite, unmasked values of image b of field ([B,H,W] fp32,
 *   or fp64 with is_f64 = 1), exact; 0 where nothing is left.
 *
 * pivlfn_scalar_to_color: field as above;  lut: 256 x 3 bytes (r, g, b) on the device;  scale = 256.0 / (vmax - vmin), formed once
 *   on the host;  idx = floor(((double)x - vmin) * scale) in fp64, two operations each rounded on its own, clamped to 0..255;  the
 *   pixel is lut[idx].  A non-finite x or a masked pixel is bad_rgb (0xRRGGBB).  vmax < vmin reverses the map.
 *
 * pivlfn_flow_decimate: mean: NCHW [B,2,ch,cw] fp32, count: [B,ch,cw] int32, ch = ceil(H / cell), cw = ceil(W / cell).  Cell (i, j)
 *   covers rows i*cell .. min(H, (i+1)*cell) - 1 and the columns likewise (a ragged last cell averages what it has).  The vectors of
 *   a cell that are neither unknown nor masked are added in row-major order in fp64, from +0.0;  mean = (float)(sum / (double)count);
 *   an empty cell is 1e10f in both components with count 0.
 *
 * Errors (PIVLFN_ERR_ARG, before any launch): a null pointer other than mask, a non-positive size, H*W >= 2^31, B > 65535, an unknown
 * wheel or order, is_f64 not 0 / 1, non-finite or equal vmin and vmax (or a range so narrow that scale overflows), bad_rgb outside
 * 0..0xFFFFFF, cell outside 1..32768. */
#define PIVLFN_WHEEL_INTERP   0
#define PIVLFN_WHEEL_ORIGINAL 1
#define PIVLFN_ORDER_RGB      0
#define PIVLFN_ORDER_BGR      1
int pivlfn_flow_maxrad(const float *flow, const unsigned char *mask, float *maxrad, int B, int H, int W, void *stream);
int pivlfn_flow_to_color(const float *flow, const float *norm, const unsigned char *mask, unsigned char *out, int B, int H, int W,
                         int wheel, int order, void *stream);
int pivlfn_field_absmax(const void *field, int is_f64, const unsigned char *mask, double *absmax, int B, int H, int W, void *stream);
int pivlfn_scalar_to_color(const void *field, int is_f64, const unsigned char *mask, const unsigned char *lut, unsigned char *out,
                           int B, int H, int W, double vmin, double vmax, int bad_rgb, void *stream);
int pivlfn_flow_decimate(const float *flow, const unsigned char *mask, float *mean, int *count, int B, int H, int W, int cell,
                         void *stream);

/* ---- match quality of an estimated flow: the normalised correlation between image 1 and image 2 warped back by the flow inside a
 * (2*radius+1)^2 window around every pixel, at zero shift and at the four one-pixel shifts, and the sub-pixel position of its peak
 * (three-point Gaussian fit) -- the correlation peak height of a classical PIV evaluation and what a window-deformation pass would
 * still add to the vector.  Added without an ABI bump (additive).
 * img1, img2: NCHW [B,C,H,W] fp32, C = 1 or 3;  flow: NCHW [B,2,H,W] fp32;  mask: [B,H,W] bytes or NULL, nonzero = leave the pixel
 * out;  quality: NCHW [B,3,H,W] fp32, planes c, dx, dy;  flag: [B,H,W] bytes;  workspace: 8-byte aligned, at least
 * pivlfn_match_quality_workspace_bytes(B,H,W,radius) bytes, needs no initial contents.  Launches only on `stream`, no allocation, no
 * host synchronisation, no floating-point atomics; no output depends on what quality, flag or the workspace held before the call; a
 * pair gives the same bits alone, inside any batch and from run to run.
 * Arithmetic contract, all fp64 unless stated, every operation rounded on its own (no fma), divisions and square roots correctly
 * rounded:
 *   gray value:  C = 1: g(q) = (double)x;  C = 3: g(q) = (((double)r + (double)g) + (double)b) / 3.0 (three equal channels give the
 *                bits of C = 1).  a = g of img1, g2 = g of img2.
 *   warp:        xf = (float)x + u(p), yf = (float)y + v(p), one fp32 addition each;  m(p) = 1 iff 0 <= xf <= W-1 && 0 <= yf <= H-1
 *                (NaN and inf compare false: the 1e10 of a masked flow is invalid by itself).  Where m = 1: x0 = (int)xf,
 *                x1 = min(x0+1, W-1), fx = (double)xf - x0 (exact), the same in y;
 *                top = (1.0-fx)*g2(y0,x0) + fx*g2(y0,x1), bot likewise on row y1;  b(p) = (1.0-fy)*top + fy*bot.
 *                This is pivlfn_backwarp's sampling position (align_corners=True: pixel x + u).
 *   exclusion:   k(q) = 1 iff mask is NULL or mask(q) == 0.
 *   shifts:      s = (sx, sy) in {(0,0), (-1,0), (+1,0), (0,-1), (0,+1)}, in this order.  Pixel q takes part in shift s iff k(q) = 1,
 *                q+s lies inside the image and m(q+s) = 1.  Its six terms are 1, a(q), a(q)^2, b(q+s), b(q+s)^2, a(q)*b(q+s); a pixel
 *                that does not take part is +0.0 in all six.
 *   window sums: over the (2*radius+1)^2 window centred at p, clipped to the image (no edge replication): per row the terms are added
 *                left to right from +0.0, then the row sums top to bottom from +0.0.  The order is fixed by this contract and not by
 *                the launch geometry.  Results per shift: n (an exact count), A, AA, Bs, BB, AB.
 *   per shift:   few = n < min_count;  va = AA - A*A/n, vb = BB - Bs*Bs/n, cov = AB - A*Bs/n;
 *                flat = va < floor*floor*n || vb < floor*floor*n;  c_s = cov / sqrt(va*vb) where neither few nor flat.
 *   flag byte:   bit 0 (1) FEW: shift 0 is few;  bit 1 (2) FLAT: shift 0 is flat and not few;  bit 2 (4) NO_PEAK: FEW and FLAT are
 *                clear and a fit condition fails;  bit 3 (8) CENTRE_OUT: k(p) = 0 or m(p) = 0 (informational: the values are still
 *                formed).  Fit conditions, on the c values as computed: the four other shifts are neither few nor flat; c0 > 0; each
 *                side value > 0; c0 >= each side value; (2*c0 - c_minus) - c_plus >= 1e-6 in x and in y.
 *   outputs:     c = (float)c0, NaN where FEW or FLAT is set.  Where bits 0-2 are clear, with l = ln (the device library's fp64
 *                logarithm, the one operation here that is not correctly rounded):
 *                dx = 0.5*(l(c_minus) - l(c_plus)) / ((l(c_minus) - 2.0*l(c0)) + l(c_plus)) over the x shifts, dy over the y shifts,
 *                each rounded once to fp32; the conditions keep the denominator below -1e-6 and |dx|, |dy| <= 0.5.  dx = dy = +0.0f
 *                wherever one of bits 0-2 is set.  The peak sits at the error of the flow: flow + (dx, dy) is the corrected vector.
 * Errors (PIVLFN_ERR_ARG, before any launch): null img1 / img2 / flow / quality / flag / workspace, quality or flag overlapping an
 * input, the workspace or each other, C not 1 or 3, a non-positive size, H*W >= 2^31, B > 65535, radius outside 1..15, min_count < 2
 * or > (2*radius+1)^2, floor negative or non-finite, a misaligned or too-small workspace. */
#define PIVLFN_QUALITY_FEW        1
#define PIVLFN_QUALITY_FLAT       2
#define PIVLFN_QUALITY_NO_PEAK    4
#define PIVLFN_QUALITY_CENTRE_OUT 8
size_t pivlfn_match_quality_workspace_bytes(int B, int H, int W, int radius);
int pivlfn_match_quality(const float *img1, const float *img2, int C, const float *flow, const unsigned char *mask, float *quality,
                         unsigned char *flag, int B, int H, int W, int radius, int min_count, double floor, void *workspace,
                         size_t workspace_bytes, void *stream);

/* ---- vortex identification: the functions Gamma1 and Gamma2 of Graftieaux, Michard and Grosjean (2001) of a flow field over the
 * (2*radius+1)^2 - 1 neighbours at distance `spacing` pixels around every vector.  Gamma1 peaks at a vortex centre but is not Galilean
 * invariant; Gamma2 is formed about the window's own mean velocity, is Galilean invariant, and |Gamma2| > 2/pi marks the region where
 * rotation dominates shear (the vortex core).  Added without an ABI bump (additive).
 * flow: NCHW [B,2,H,W] fp32;  mask: [B,H,W] bytes or NULL, nonzero = leave the vector out;  gamma: NCHW [B,2,H,W] fp32, planes Gamma1
 * and Gamma2;  flag: [B,H,W] bytes;  workspace: 8-byte aligned, at least pivlfn_vortex_gamma_workspace_bytes(B,H,W,radius,spacing)
 * bytes (0 for arguments out of range), needs no initial contents.  Launches only on `stream`, no allocation, no host
 * synchronisation, no floating-point atomics; no output depends on what gamma, flag or the workspace held before the call; a pair
 * gives the same bits alone, inside any batch and from run to run.
 * Arithmetic contract, all fp64, every operation rounded on its own (no fma), divisions and square roots correctly rounded; x is the
 * column index, y the row index, r = radius, s = spacing:
 *   validity:    k(q) = 1 iff (mask is NULL or mask(q) == 0) and |u(q)| <= 1e9 && |v(q)| <= 1e9 (NaN compares false; the 1e10 of a
 *                masked flow is invalid by itself).
 *   vectors:     U = (double)u, V = (double)v where k = 1, else +0.0 for both;  m = sqrt(U*U + V*V);  ux = U/m, uy = V/m where m > 0,
 *                else +0.0.
 *   neighbours:  of P = (x, y): M = (x + i*s, y + j*s) with |i|, |j| <= r, (i, j) != (0, 0), M inside the image (no edge
 *                replication).  M takes part iff k(M) = 1.
 *   directions:  d = sqrt((double)(i*i + j*j)), px = i/d, py = j/d.  The table does not depend on s.
 *   window sums: per row j the terms are added from i = -r to +r starting at +0.0, then the row sums from j = -r to +r starting at
 *                +0.0.  A neighbour that does not take part is +0.0, and the centre is +0.0 where it is excluded.  The order is fixed
 *                by this contract and not by the launch geometry.
 *   counts:      N = the number of neighbours taking part (exact);  n_all = N + k(P).
 *   Gamma1:      the sum of px*uy(M) - py*ux(M), divided by N.
 *   window mean: SU, SV = the sums of U and V over the window, centre included, in the same order;  Mx = SU / n_all, My = SV / n_all.
 *   Gamma2:      du = U(M) - Mx, dv = V(M) - My, m2 = sqrt(du*du + dv*dv);  the term is (px*dv - py*du) / m2 where m2 > 0, else +0.0;
 *                Gamma2 = the sum divided by N.
 *   outputs:     both values rounded once to fp32.  Flag bit 0 (PIVLFN_VORTEX_FEW): N < min_count; both planes are NaN there.  Bit 1
 *                (PIVLFN_VORTEX_CENTRE_OUT): k(P) = 0 (informational: the values are still formed).
 *   sign:        Gamma is positive where dv/dx - du/dy > 0 with x the column index and y the row index: a rotation that turns the x
 *                axis towards the y axis, which is clockwise in a picture drawn with the row index growing downwards.  It does not
 *                follow the mixed convention of the de_vort kind of pivlfn_flow_fields.
 * Errors (PIVLFN_ERR_ARG, before any launch): null flow / gamma / flag / workspace, gamma or flag overlapping an input, the workspace
 * or each other, a non-positive size, H*W >= 2^31, B > 65535, radius outside 1..15, spacing outside 1..16, min_count outside
 * 1..(2*radius+1)^2 - 1, a misaligned or too-small workspace. */
#define PIVLFN_VORTEX_FEW        1
#define PIVLFN_VORTEX_CENTRE_OUT 2
size_t pivlfn_vortex_gamma_workspace_bytes(int B, int H, int W, int radius, int spacing);
int pivlfn_vortex_gamma(const float *flow, const unsigned char *mask, float *gamma, unsigned char *flag, int B, int H, int W, int radius,
                        int spacing, int min_count, void *workspace, size_t workspace_bytes, void *stream);

/* ---- Lagrangian flow maps of a flow SEQUENCE: particles carried through consecutive displacement fields (pathlines, the flow map)
 * and the largest stretching of the map, whose logarithm over the interval is the finite-time Lyapunov exponent (FTLE).  An estimated
 * flow is a displacement field: F_k(x) is where the content at pixel x of frame k sits in frame k+1, so the flow map over an interval
 * is x -> x + F_k(x) composed over k -- one bilinear sample per particle and field, no velocities and no integrator.  Added without
 * an ABI bump (additive).
 * State: N particles, pos planar [2,N] fp64 (the x plane, then the y plane; x is the column index, y the row index, pixel centres at
 * integers) and flag [N] bytes.  A particle with a nonzero flag byte is frozen: no call changes its position or its flag again.
 * Flag bits: PIVLFN_FLOWMAP_OUT -- the particle left the image; PIVLFN_FLOWMAP_LOST -- it met a masked or unknown vector;
 * PIVLFN_FLOWMAP_UNDEFINED -- only in the oflag of pivlfn_flowmap_ftle.
 * All three entry points launch only on `stream` (one launch each), never synchronise the host, allocate nothing, need no workspace
 * and can be captured into a graph.  No result depends on the launch geometry, on N, or on how a sequence is cut into calls: B fields
 * in one call give the bits of B calls of one field.
 * Arithmetic contract, all fp64, every operation a correctly rounded fp64 operation in the stated order (no fma; (double) of a float
 * is exact):
 *
 * pivlfn_flowmap_advect -- every particle through the B fields flows[0..B-1] in index order ([B,2,H,W] fp32 NCHW; mask [B,H,W] bytes
 * or NULL, nonzero = the vector is not to be used).  A step depends on the particle's own state alone.
 *   sample S_k(x, y) of field k:
 *     1. if not (0 <= x <= W-1 and 0 <= y <= H-1): the sample sets OUT (a NaN coordinate fails the test).
 *     2. ix = min((int)floor(x), W-2), fx = x - (double)ix;  iy = min((int)floor(y), H-2), fy = y - (double)iy  (so x = W-1 is
 *        sampled with ix = W-2 and fx = 1).
 *     3. the four corners (iy + {0,1}, ix + {0,1}) are all required whatever their weights: if any has a nonzero mask byte or a
 *        component c that fails |c| <= 1e9 (NaN, +-inf, the 1e10 of a masked flow), the sample sets LOST.
 *     4. per component, with c00 = (iy, ix), c01 = (iy, ix+1), c10 = (iy+1, ix), c11 = (iy+1, ix+1) as (double):
 *        top = (1 - fx)*c00 + fx*c01;  bot = (1 - fx)*c10 + fx*c11;  S = top*(1 - fy) + bot*fy.
 *   forward step (backward = 0): (u, v) = S_k(x, y);  x = x + u, y = y + v.  A sample that sets a flag leaves (x, y) as it is.  A
 *     particle is not flagged for where a step puts it, only by the next sample taken there.
 *   backward step (backward = 1; the caller passes the fields newest first): solves p + F_k(p) = (x, y) by exactly `iters` fixed-point
 *     iterations, 1..32:  p_0 = (x, y);  p_i = (x, y) - S_k(p_(i-1));  the new position is p_iters.  A sample that sets a flag ends
 *     the step with the particle frozen at (x, y).
 *   trace: NULL, or [B,2,N] fp64 that receives the state of every particle, frozen ones included, after each field (pathlines).
 *   Errors (PIVLFN_ERR_ARG, before any launch): H < 2 or W < 2, H*W >= 2^31, B < 0, N < 0, backward not 0 or 1, iters outside 1..32
 *   (also where backward = 0);  then N == 0 or B == 0 succeeds, launches nothing and reads no pointer;  otherwise null flows / pos /
 *   flag, and pos, flag or trace overlapping flows, mask or each other.
 *
 * pivlfn_flowmap_seed -- the h x w lattice at `spacing` pixels, row-major, n = i*w + j:  pos = ((double)(j*spacing),
 * (double)(i*spacing)), flag = 0.
 *
 * pivlfn_flowmap_ftle -- for particles seeded on that lattice; X and Y are the planes of pos.  At node (i, j):
 *     jl = max(j-1, 0), jr = min(j+1, w-1), iu = max(i-1, 0), id = min(i+1, h-1)  (central inside, one-sided at the border);
 *     dx = (double)((jr - jl)*spacing), dy = (double)((id - iu)*spacing);
 *     a = (X[i][jr] - X[i][jl]) / dx;  b = (X[id][j] - X[iu][j]) / dy;  c = (Y[i][jr] - Y[i][jl]) / dx;  d = (Y[id][j] - Y[iu][j]) / dy;
 *     c11 = a*a + c*c;  c22 = b*b + d*d;  c12 = a*b + c*d;  g = 0.5*(c11 - c22);  lam = 0.5*(c11 + c22) + sqrt(g*g + c12*c12);
 *     stretch = sqrt(lam)  [h,w] fp64: the largest singular value of the map's gradient.
 *   UNDEFINED is set and stretch is NaN where the node's own flag or the flag of one of the four particles used is nonzero, and
 *   everywhere if h < 2 or w < 2.  oflag [h,w] bytes = the node's own flag | UNDEFINED.
 *   The logarithm is not part of the contract (the device's log is not correctly rounded): FTLE = log(stretch) / steps is the caller's.
 *   Errors of seed and ftle (PIVLFN_ERR_ARG, before any launch): h < 1 or w < 1, h*w >= 2^31, spacing outside 1..32768, a lattice that
 *   reaches past pixel 2^31, a null pointer, outputs overlapping an input or each other. */
#define PIVLFN_FLOWMAP_OUT       1
#define PIVLFN_FLOWMAP_LOST      2
#define PIVLFN_FLOWMAP_UNDEFINED 4
int pivlfn_flowmap_advect(const float *flows, const unsigned char *mask, int B, int H, int W, double *pos, unsigned char *flag, int N,
                          int backward, int iters, double *trace, void *stream);
int pivlfn_flowmap_seed(double *pos, unsigned char *flag, int h, int w, int spacing, void *stream);
int pivlfn_flowmap_ftle(const double *pos, const unsigned char *flag, int h, int w, int spacing, double *stretch, unsigned char *oflag,
                        void *stream);

/* ---- synthetic PIV pairs from a known flow: N particles carried through ONE displacement field (pivlfn_particles_displace) and
 * particle images rendered as sums of Gaussian blobs (pivlfn_particles_render): rendering a seeding before and after the displacement
 * gives an image pair whose true displacement is the field.  Added without an ABI bump (additive).
 * Coordinates as in the flow-map section: x is the column, y the row, pixel centres at integers.  Both entry points launch only on
 * `stream`, never synchronise the host, allocate nothing and can be captured into a graph as one linear chain of kernels.
 *
 * pivlfn_particles_displace -- pos [2,N] fp64 planar (x plane, y plane);  flow [2,H,W] fp32 (u, v);  mask [H,W] bytes or NULL, nonzero =
 * the vector is not to be used;  flag [N] bytes, read and written;  out [2,N] fp64.  One launch.  All fp64, every operation a correctly
 * rounded fp64 operation in the stated order (no fma; (double) of a float is exact):
 *   0. a particle whose flag byte is nonzero on entry is copied through: out = pos, the flag as it was.
 *   1. a NaN coordinate sets PIVLFN_PARTICLES_BAD; out = pos.
 *   2. clamp to the image:  xc = 0.0 if x < 0, (double)(W-1) if x > W-1, else x (so -0.0 and +-inf are defined);  yc likewise with H.
 *      A particle in the seeding margin round the image takes the displacement of the edge.
 *   3. the cell, as the flow-map sampler: ix = min((int)floor(xc), W-2), fx = xc - (double)ix;  iy and fy likewise.
 *   4. method 0, bilinear: the four corners c00 = (iy, ix), c01 = (iy, ix+1), c10 = (iy+1, ix), c11 = (iy+1, ix+1) as (double), per
 *      component:  top = (1 - fx)*c00 + fx*c01;  bot = (1 - fx)*c10 + fx*c11;  S = top*(1 - fy) + bot*fy.
 *      method 1, Catmull-Rom bicubic (Keys, a = -0.5): 16 taps at rows iy-1 .. iy+2 and columns ix-1 .. ix+2, every tap index clamped to
 *      the image.  Weights of the taps -1, 0, 1, 2 as polynomials in f (f = fx along x, fy along y), evaluated as written:
 *        w0 = ((-0.5*f + 1.0)*f - 0.5)*f;   w1 = ((1.5*f - 2.5)*f)*f + 1.0;   w2 = ((-1.5*f + 2.0)*f + 0.5)*f;   w3 = ((0.5*f - 0.5)*f)*f.
 *      Along x first, per row r = 0..3 and component:  row_r = ((w0*c_r0 + w1*c_r1) + w2*c_r2) + w3*c_r3 with the weights of fx;
 *      then along y:  S = ((w0*row_0 + w1*row_1) + w2*row_2) + w3*row_3 with the weights of fy.
 *   5. every tap of the method is required whatever its weight: one with a nonzero mask byte or a component c that fails |c| <= 1e9
 *      (NaN, +-inf, the 1e10 of a masked flow) sets PIVLFN_PARTICLES_LOST; out = pos.
 *   6. otherwise out = (x + Su, y + Sv), of the unclamped position, and the flag stays 0.
 *   Errors (PIVLFN_ERR_ARG, before any launch): H < 2 or W < 2, H*W >= 2^31, N < 0, method not 0 or 1;  then N == 0 succeeds, launches
 *   nothing and reads no pointer;  otherwise null pos / flow / flag / out, and out or flag overlapping pos, flow, mask or each other.
 *
 * pivlfn_particles_render -- B images of N particles each.  pos [B,2,N] fp64;  diam [B,N] fp32, the diameter in pixels;  amp [B,N] fp32,
 * the peak grey level;  flag [B,N] bytes or NULL;  intensity [B,H,W] fp32 and image [B,H,W] bytes, both written completely;  radius R in
 * 1..8;  workspace: 8-byte aligned, at least pivlfn_particles_render_workspace_bytes(B,N,H,W,radius) bytes (0 for arguments out of
 * range), needs no initial contents.  Five launches in a chain (three where N == 0: nothing to bin); integer atomics only.
 *   particle:  left out if its flag byte is nonzero, if x, y, diam or amp is not finite, if diam <= 0 or amp < 0, if |x| >= 2^30 or
 *              |y| >= 2^30, or if w below is not finite (a diameter under 4e-19).  Otherwise ix = (int)floor(x), iy = (int)floor(y)
 *              (floor, not truncation: the margin has negative coordinates);  its footprint is the pixels j in [ix-R, ix+R+1],
 *              i in [iy-R, iy+R+1] that lie inside the image;  in fp32, once:  s = 0.5f*diam;  w = 1.0f/(s*s)  (a correctly rounded division).
 *   term:      per pixel (i, j) of the footprint, fp32, every operation rounded on its own (no fma):
 *              dx = (float)((double)j - x);  dy = (float)((double)i - y);  q = (dx*dx + dy*dy)*w;  t = amp*expf(-q),  expf within one ulp.
 *   pixel:     intensity[i][j] = the fp32 sum of the t of all particles whose footprint holds the pixel, added in ASCENDING PARTICLE
 *              INDEX starting from +0.0f;  image[i][j] = (unsigned char)min(intensity, 255.0f), truncating.
 *   The order of the sum is fixed by this contract and not by the launch geometry, by how the particles were binned or by the batch: an
 *   image has the same bits alone, inside any batch, whatever the workspace held, and from run to run.
 *   Against a sum V of the same terms in exact arithmetic, with A = the sum of amp and n = the number of the covering particles and
 *   u = 2^-24:  dx and dy carry one rounding each (the fp64 difference adds less than 2^-52 of it), so q is off by at most 7u relative
 *   (3u in each square -- two from dx, one of its own --, one more in their sum, two in w -- s*s and the division --, one in the
 *   product);  d(e^-q) = q e^-q dq/q and q e^-q <= 1/e, so the exponential is off by at most 7u/e + 2u (its own ulp is up to 2u
 *   relative) and the product with amp by one more rounding: a term is off by at most about 5.6u*amp, and 8u*amp leaves margin;
 *   all terms are >= 0, so each of the n additions rounds a partial sum <= V:
 *       |intensity - V| <= 2^-21*A + n*2^-24*V.
 *   Errors (PIVLFN_ERR_ARG, before any launch): H < 1 or W < 1, H or W > 2^31 - 17, H*W >= 2^31, B < 0 or N < 0, radius outside 1..8;  then B == 0 succeeds,
 *   launches nothing and reads no pointer;  otherwise B*ceil(H/16)*ceil(W/16) >= 2^31 tiles, B*N >= 2^39, null intensity / image /
 *   workspace, null pos / diam / amp where N > 0, a misaligned or too-small workspace, and intensity, image or the workspace overlapping
 *   an input or each other.  N == 0 with B > 0 writes images of zeros. */
#define PIVLFN_PARTICLES_LOST 2
#define PIVLFN_PARTICLES_BAD  8
int pivlfn_particles_displace(const double *pos, const float *flow, const unsigned char *mask, int H, int W, int N, int method,
                              unsigned char *flag, double *out, void *stream);
size_t pivlfn_particles_render_workspace_bytes(int B, int N, int H, int W, int radius);
int pivlfn_particles_render(const double *pos, const float *diam, const float *amp, const unsigned char *flag, int B, int N, int H, int W,
                            int radius, float *intensity, unsigned char *image, void *workspace, size_t workspace_bytes, void *stream);

/* ---- snapshot POD of a flow sequence: the two device steps of proper orthogonal decomposition by the method of snapshots.  The
 * eigenproblem of the n x n matrix stays a host job.  Added without an ABI bump (additive).
 * X: n rows (snapshots) of P fp32 values, row stride ldx >= P floats.  Nothing beyond column P of a row and nothing beyond row n is
 * read.  Both entry points launch only on `stream`, allocate nothing, never synchronise the host and can be captured into a graph; no
 * output depends on what G, out or the workspace held before the call.
 *
 * pivlfn_snapshot_gram: G ([n,n] fp64, row-major, written completely) with G[i][j] = sum over p of (double)X[i][p] * (double)X[j][p].
 *   Every product of two fp32 values is exact in fp64, so the only rounding is the summation, done in fp64 by the matrix instruction
 *   v_mfma_f64_16x16x4_f64 in an order that depends on P alone: P is cut into slabs of PIVLFN_GRAM_SLAB floats; a slab is summed in
 *   ascending p by one chain of matrix instructions (four consecutive p per instruction) into an accumulator that starts at +0.0;
 *   G[i][j] = ((+0.0 + S_0) + S_1) + ... over the slab sums in slab order, plain fp64 additions.  Tile padding (rows past n, columns
 *   past P) is +0.0 in both operands.  Consequences: G[i][j] has the same bits whatever n is, wherever rows i and j sit in X, whatever
 *   the other rows hold and from run to run;  G[j][i] is G[i][j] bit for bit (the upper triangle is computed and mirrored);  a NaN or
 *   inf in row i reaches row i and column i of G and nothing else.
 *   workspace: 8-byte aligned, at least pivlfn_snapshot_gram_workspace_bytes(n, P) bytes (0 for arguments out of range), needs no
 *   initial contents.  Where G has few 64 x 64 blocks, the slab sums of a block are formed by different workgroups and pass through
 *   it; the values do not depend on that choice.
 *   Errors (PIVLFN_ERR_ARG, before any launch): null X / G / workspace, n outside 1..PIVLFN_POD_MAX_SNAPSHOTS, P < 1, P >= 2^31,
 *   ldx < P, a misaligned or too-small workspace.
 *
 * pivlfn_snapshot_project: Wt: [n,K] fp64 row-major on the device;  out: [K,P] fp64;  out[k][p] = the fold over i = 0 .. n-1,
 *   ascending, of acc = acc + Wt[i][k] * (double)X[i][p] from +0.0, the multiplication and the addition each rounded on its own (no
 *   fma): a sequential fp64 loop gives the same bits.  X is read once.
 *   Errors (PIVLFN_ERR_ARG, before any launch): null X / Wt / out, n, P and ldx as above, K outside 1..64. */
#define PIVLFN_GRAM_SLAB         2048
#define PIVLFN_POD_MAX_SNAPSHOTS 4096
size_t pivlfn_snapshot_gram_workspace_bytes(int n, long P);
int pivlfn_snapshot_gram(const float *X, int n, long P, long ldx, double *G, void *ws, size_t ws_bytes, void *stream);
int pivlfn_snapshot_project(const float *X, int n, long P, long ldx, const double *Wt, int K, double *out, void *stream);

/* ---- two-point statistics of a flow SEQUENCE: the sums from which the spatial correlation functions R_uu(r), R_vv(r), R_uv(r) and the
 * second- and third-order structure functions follow, per image row, for separations along a row and down a column.  Added without an
 * ABI bump (additive).
 * flow: NCHW [B,2,H,W] fp32;  mask: [B,H,W] bytes or NULL, nonzero = leave the vector out;  mean: [2,H,W] fp64 (the planes of u and v)
 * or NULL;  acc: [2, max_sep+1, PIVLFN_TWOPOINT_TERMS, H] fp64, read and written once per call: direction d (0: the partner lies r*step
 * columns to the right, 1: r*step rows below), separation index r = 0..max_sep, term, base row y.  One launch, only on `stream`; no
 * allocation, no workspace, no host synchronisation, no floating-point atomics; can be captured into a graph.  No value depends on the
 * launch geometry or on how a sequence is cut into calls: B frames in one call give the bits of B calls of one frame.
 * Arithmetic contract, all fp64, every operation rounded on its own (no fma; (double) of a float is exact):
 *   validity:     k(p) = 1 iff (mask is NULL or mask(p) == 0) and |u(p)| <= 1e9 && |v(p)| <= 1e9 (the rule of pivlfn_vortex_gamma: NaN
 *                 compares false; the 1e10 of a masked flow is invalid by itself).
 *   values:       U(p) = (double)u(p) - mean_u(p), V(p) = (double)v(p) - mean_v(p);  with a NULL mean U = (double)u, V = (double)v.
 *   pair:         base point a = (y, x);  partner b = (y, x + r*step) for d = 0 and (y + r*step, x) for d = 1.  The pair takes part iff
 *                 b lies inside the image and k(a) = k(b) = 1.  A pair that does not take part is +0.0 in every term, the count
 *                 included; its products are not formed (no 0 * NaN).
 *   increments:   dL along the separation, dT across it:  d = 0: dL = Ub - Ua, dT = Vb - Va;  d = 1: dL = Vb - Va, dT = Ub - Ua.
 *   terms:        0: 1 (the count);  1..4: Ua, Va, Ub, Vb;  5..8: Ua*Ua, Va*Va, Ub*Ub, Vb*Vb;  9..12: Ua*Ub, Va*Vb, Ua*Vb, Va*Ub;
 *                 13: (dL*dL)*dL;  14: (dL*dT)*dT.
 *   row sum:      for every (frame, d, r, term, row y) the sum over x = 0..W-1 is the root of the binary tree t[i] = t[2i] + t[2i+1]
 *                 whose leaves are the terms at x = 0..W-1 padded with +0.0 to the next power of two >= W (a row of one pixel is its
 *                 own root): the 1-D analogue of the tree of pivlfn_flow_errors.
 *   accumulation: acc[d][r][term][y] = ((acc_before + rowsum(frame 0)) + rowsum(frame 1)) + ..., in frame order.
 *   exactness:    the counts are exact integers;  with a NULL mean every product of two values is exact in fp64 (24 x 24 bits), so
 *                 only the additions round.
 * Errors (PIVLFN_ERR_ARG, before any launch): H < 1 or W < 1, B < 0, H*W >= 2^31, W > 16384, max_sep outside 0..255, step outside
 * 1..16;  then B == 0 succeeds, launches nothing and reads no pointer;  otherwise null flow or acc, and acc overlapping flow, mask or
 * mean. */
#define PIVLFN_TWOPOINT_TERMS 15
int pivlfn_twopoint_accumulate(const float *flow, const unsigned char *mask, const double *mean, double *acc, int B, int H, int W,
                               int max_sep, int step, void *stream);

/* ---- temporal spectra of a flow SEQUENCE: one segment of Welch's method.  Every vector's L samples of u and v are projected on K pairs of
 * basis rows (the caller's windowed, detrended cosines and sines) and the power and cross-spectrum terms are added to running sums.
 * Added without an ABI bump (additive).
 * X: a ring of exactly L rows, one snapshot per row, row stride ldx >= 2N floats; a row is [2,N] fp32, the plane of u then the plane of
 * v (the row layout of pivlfn_snapshot_gram); nothing past column 2N is read.  Sample t = 0..L-1 of the segment is row (first + t) % L.
 * basis: [K,2,L] fp64, C_k[t] = basis[k][0][t], S_k[t] = basis[k][1][t]; the kernel gives them no meaning.  acc: [K,4,N] fp64 and
 * count: [N] int32, both read and written once per call.  One launch, only on `stream`; no allocation, no workspace, no host
 * synchronisation, no atomics; can be captured into a graph.  Nothing about one vector reaches another, and no value depends on the
 * launch geometry.
 * Arithmetic contract, all fp64, every operation rounded on its own (no fma; (double) of a float is exact):
 *   validity:     vector p takes part iff all 2L of its values satisfy |x| <= 1e9f (the rule of pivlfn_vortex_gamma: NaN compares
 *                 false; the 1e10 of pivlfn_flow_decimate's empty cell and of a masked flow is invalid by itself).  For a vector that
 *                 does not take part acc[.][.][p] and count[p] keep their bits.
 *   projections:  for each k, cu = the fold over t = 0..L-1 ascending of a = a + C_k[t] * (double)u[t][p] from a = +0.0;  su with S_k;
 *                 cv and sv the same of v.
 *   terms:        Suu = cu*cu + su*su;  Svv = cv*cv + sv*sv;  Co = cu*cv + su*sv;  Qd = cu*sv - su*cv  (with X = c - i s this is
 *                 Im(U conj V): positive where v lags u).
 *   accumulation: acc[k][j][p] = acc[k][j][p] + term_j, j = 0..3 in the order Suu, Svv, Co, Qd;  count[p] += 1.
 * Errors (PIVLFN_ERR_ARG, before any launch): null X, basis, acc or count;  L outside 2..1024;  first outside 0..L-1;  K outside
 * 1..513;  N < 1;  2N >= 2^31;  ldx < 2N.  acc is indexed with 64 bits (K*4*N passes 2^31 at full size). */
int pivlfn_spectrum_accumulate(const float *X, int L, int first, long N, long ldx, const double *basis, int K, double *acc, int *count,
                               void *stream);

/* ---- pressure from a time-resolved planar flow SEQUENCE: the pressure gradient of the in-plane incompressible momentum equation in
 * lattice units (px, frame),  grad p* = g = -(du/dt + u du/dx + v du/dy) + nu* lap u,  from three consecutive flows, and its least-squares
 * integration over the valid nodes: the graph-Laplacian Poisson problem with the natural Neumann boundary on any mask shape, solved by
 * Jacobi-preconditioned conjugate gradients.  Units (p = rho (calib/dt)^2 p*, nu* = nu dt/calib^2) are the caller's.  Added without an ABI
 * bump (additive).
 * Every entry point launches only on `stream`, allocates nothing, never synchronises the host, uses no atomics and can be captured into a
 * graph as one linear chain of kernels.  There is no grid-wide barrier, no persistent kernel, no spin wait and no cooperative launch: a
 * seam between two phases is a kernel boundary, and every loop of a kernel has a bound known at launch.
 * All arithmetic is fp64, every operation rounded on its own (no fma; (double) of a float is exact; divisions are IEEE).  A node is
 * (j, i) = (row, column) of an h x w lattice, node index j*w + i; "left / right" are columns i-1 / i+1, "up / down" rows j-1 / j+1.
 *
 * T(.), the sum over a frame: the root of the binary tree t[i] = t[2i] + t[2i+1] whose leaves are the N = h*w per-node values in
 *   row-major order, padded with +0.0 to the next power of two >= N: the tree of pivlfn_twopoint_accumulate's row sum, taken over the
 *   whole lattice of one frame.  No value depends on how workgroups cut the tree.
 *
 * pivlfn_pressure_gradient -- flows [B,2,h,w] fp32, B >= 3 consecutive flows;  s: lattice spacing, px per node;  nu: nu*;  g [B-2,2,h,w]
 *   fp64 and valid [B-2,h,w] bytes, both written completely.  Output frame f uses flows f, f+1 and f+2.  One launch.
 *   validity: node (j,i) of frame f is valid iff 1 <= j <= h-2 and 1 <= i <= w-2 and both components of all seven vectors -- the centre and
 *     its four neighbours in flow f+1, the centre in flows f and f+2 -- satisfy |x| <= 1e9f (the rule of pivlfn_vortex_gamma: NaN is
 *     invalid, and so is the 1e10 of an unknown vector).
 *   per component a in {u, v}, c the centre, l, r, u, d the neighbours in flow f+1, prev / next the centre in flows f / f+2:
 *     at  = (a_next - a_prev) * 0.5
 *     ax  = (a_r - a_l) / (2.0*s);   ay = (a_d - a_u) / (2.0*s)
 *     lap = ((((a_l + a_r) + a_u) + a_d) - 4.0*a_c) / (s*s)
 *     g_a = (-(at + (u_c*ax + v_c*ay))) + nu*lap
 *   An invalid node gets g = +0.0 in both components and valid = 0; its products are not formed.
 *
 * pivlfn_pressure_setup -- g [F,2,h,w], valid [F,h,w] (nonzero = valid), s as above;  fills the workspace: 8-byte aligned, at least
 *   pivlfn_pressure_workspace_bytes(F,h,w) bytes (0 for arguments out of range), needs no initial contents.  One launch.
 *   The edge between 4-neighbours a and b is active iff both are valid;  deg(a) = the number of active edges at a.
 *   For the edge a -> right neighbour b:  e = (0.5*(gx(a) + gx(b))) * s;  for a -> lower neighbour the same with gy.
 *   b(a) = ((L + R) + U) + D  with  L = +e(left -> a), R = -e(a -> right), U = +e(up -> a), D = -e(a -> down);  an inactive edge is +0.0.
 *   Initial state: x = +0.0, r = b, z = r/deg (+0.0 where deg = 0), d = z, rho = T(r*z), bb = T(b*b), rr = T(r*r), iterations = 0,
 *   state = PIVLFN_PRESSURE_RUNNING.
 *   pivlfn_pressure_workspace_offset(F,h,w,what) gives the byte offset of three arrays a caller may read (0 for arguments out of range):
 *   PIVLFN_PRESSURE_WS_B: b [F,h,w] fp64;  PIVLFN_PRESSURE_WS_X: x [F,h,w] fp64;  PIVLFN_PRESSURE_WS_ADJ: [F,h,w] bytes, bit 0 / 1 / 2 / 3 =
 *   the edge to the left / right / upper / lower neighbour is active (deg = the number of these bits), bit 4 = the node is valid.  The
 *   rest of the layout is the library's.
 *
 * pivlfn_pressure_cg -- enqueues `iters` iterations for all F frames in the same launches, two launches per iteration (the frame is a
 *   grid dimension).  Every frame has its own scalars: a frame's bits are the same alone, in any batch, and however `iters` is cut into
 *   calls.  One iteration of one frame:
 *     1. if state != RUNNING, do nothing.
 *     2. if rr <= (tol*tol)*bb and bb > 0, set state = CONVERGED and change nothing else.  (With bb = 0, that is b = 0, rule 4 decides.)
 *     3. q(a) = deg(a)*d(a) - (((d_l + d_r) + d_u) + d_d), an inactive edge contributing +0.0;  sigma = T(d*q).
 *     4. if !(sigma > 0), set state = BREAKDOWN and change nothing else (b = 0, where x = 0 is the solution, ends here; so does a NaN).
 *     5. alpha = rho/sigma;  x = x + alpha*d;  r = r - alpha*q;  z = r/deg (+0.0 where deg = 0);  rho' = T(r*z);  rr = T(r*r);
 *        beta = rho'/rho;  d = z + beta*d;  rho = rho';  iterations += 1.
 *   All nodes take part in every formula, the invalid ones with deg = 0 and b = +0.0.  Every workgroup derives the frozen-or-running
 *   decision from the same reduced scalars; no flag is written by one workgroup and read by another within a launch.
 *   Because z = r/deg, x has zero DEGREE-WEIGHTED mean on every connected component of the valid nodes, exactly in exact arithmetic and
 *   to rounding here:  sum over the component of deg*x = 0.  The plain mean is not zero, and the levels of disconnected components are
 *   unrelated; re-reference p as the application needs.
 *   iters == 0 succeeds and launches nothing.
 *
 * pivlfn_pressure_read -- p [F,h,w] fp64: x where deg > 0, a quiet NaN elsewhere;  flag [F,h,w] bytes: 0 = ok, PIVLFN_PRESSURE_INVALID,
 *   PIVLFN_PRESSURE_ISOLATED (valid with deg = 0);  status [F,4] fp64: state, iterations, rr, bb of each frame.  One launch.  The workspace
 *   is not changed: iterating can go on afterwards.
 *
 * Errors (PIVLFN_ERR_ARG, before any launch, the message names the problem): a null pointer;  B < 3;  F < 1;  h or w < 1;  F*h*w >= 2^31
 * (F = B-2 for the gradient);  s or tol not finite and positive;  nu not finite;  iters < 0;  a workspace that is misaligned or smaller
 * than the query;  gradient: g or valid overlapping flows or each other;  setup: the workspace overlapping g or valid;  read: p, flag or
 * status overlapping the workspace or each other. */
#define PIVLFN_PRESSURE_RUNNING   1
#define PIVLFN_PRESSURE_CONVERGED 2
#define PIVLFN_PRESSURE_BREAKDOWN 3
#define PIVLFN_PRESSURE_INVALID   1
#define PIVLFN_PRESSURE_ISOLATED  2
#define PIVLFN_PRESSURE_WS_B      0
#define PIVLFN_PRESSURE_WS_X      1
#define PIVLFN_PRESSURE_WS_ADJ    2
int pivlfn_pressure_gradient(const float *flows, int B, int h, int w, double s, double nu, double *g, unsigned char *valid, void *stream);
size_t pivlfn_pressure_workspace_bytes(int F, int h, int w);
size_t pivlfn_pressure_workspace_offset(int F, int h, int w, int what);
int pivlfn_pressure_setup(const double *g, const unsigned char *valid, int F, int h, int w, double s, void *workspace,
                          size_t workspace_bytes, void *stream);
int pivlfn_pressure_cg(void *workspace, size_t workspace_bytes, int F, int h, int w, double tol, int iters, void *stream);
int pivlfn_pressure_read(const void *workspace, size_t workspace_bytes, int F, int h, int w, double *p, unsigned char *flag,
                         double *status, void *stream);

/* ---- stereo calibration: what produces the coefficients pivlfn_stereo_2d3c reads.  Template matching of a calibration target
 * (stereo/matching.py:32-56, OpenCV's TM_CCOEFF_NORMED), marker centres from the correlation map (matching.py:49-75: threshold,
 * cv2.blur (2, 2), ndimage.label, centre of mass) and the image dewarp (stereo/dewarp.py:196-270, warp / nl_trans).  The fit of the
 * coefficients themselves is host code (pivlfn/calibrate.py).  Added without an ABI bump (additive).  Every entry point launches on
 * `stream` only, allocates nothing, does not synchronise and can be captured into a graph; the workspaces need no initial contents.
 *
 * pivlfn_template_match -- images [B,H,W] bytes, templ [th,tw] bytes (th and tw odd, th*tw <= 65025), r [B,H,W] fp32.  The template is
 *   centred on each pixel of the image zero-padded by (th-1)/2 rows and (tw-1)/2 columns (template_matching's pad_gray).  With the sums
 *   over the window, N = th*tw:
 *       num = N*sum(I*T) - sum(I)*sum(T);   a = N*sum(T*T) - sum(T)^2;   b = N*sum(I*I) - sum(I)^2          (integers, exact)
 *       r = (float)((double)num / sqrt((double)a * (double)b)),   r = +0.0 where a == 0 or b == 0 (flat template or flat window).
 *   The window sums fit 32 bits unsigned (255^2 * 65025 < 2^32), num, a and b are below 2^53 in magnitude: the conversions are exact
 *   and the product, the root and the quotient are each rounded once (no fma).  The result does not depend on the tiling or on B.
 *   workspace: 4-byte aligned, pivlfn_template_match_workspace_bytes(th, tw) bytes (0 for arguments out of range).  Two launches.
 *   A workgroup stages (15 + th) rows of 64 + 4*ceil(tw/4) bytes: a template for which that exceeds 160 KiB (255 x 255 fits) is refused.
 *
 * pivlfn_target_points -- r [B,H,W] fp32 -> labels [B,H,W] int32, count [B] int32, rec [B,cap,4] int64.
 *   1. q = (integer) rint(min((double)r, 8192.0) * 65536.0) where r > threshold (strict, compared in fp32; a NaN is not kept), else 0.
 *      q <= 2^29 whatever r holds (+inf included), so the sum of four below is at most 2^31.
 *   2. w(y,x) = q(y-1,x-1) + q(y-1,x) + q(y,x-1) + q(y,x), index -1 reflected to +1 (to 0 on an axis of length 1): the window of
 *      cv2.blur(res, (2, 2)) at its default anchor (BORDER_REFLECT_101) without the division by 4.  An exact 32-bit integer.
 *   3. labels: the 4-connected components of w > 0 (ndimage.label's default structure); a pixel's label is the smallest row-major
 *      index y*W + x of its component, -1 where w == 0.
 *   4. count[b] = the number of components, whatever cap is.  rec[b][k] for k < min(count[b], cap) belongs to the component with the
 *      k-th smallest label: (sum w, sum w*x, sum w*y, number of pixels) as 64-bit integers (sums modulo 2^64; r <= 1 stays far from
 *      that).  rec[b][k] for count[b] <= k < cap is zero.  Integer atomics: the bits do not depend on the order of arrival.
 *   The centre of mass of findLocalMax is (rec[1]/rec[0], rec[2]/rec[0]); it carries the (+0.5, +0.5) of the one-sided window.
 *   workspace: 4-byte aligned, pivlfn_target_points_workspace_bytes(B, H, W) bytes;  rec 8-byte aligned;  1 <= cap <= 2^24.  Six launches.
 *
 * pivlfn_dewarp_frames -- frames, out [B,H,W] bytes (is_f32 = 0) or fp32 (is_f32 = 1); A: HOST, 24 doubles, read during the call.
 *   For output pixel (x, y), u = x - x0, v = y - y0, all in fp64, each operation rounded on its own, in numpy's order for nl_trans:
 *       P(k) = ((((A[k]*u + A[k+1]*v) + A[k+2]) + A[k+3]*(u*u)) + A[k+4]*(v*v)) + (A[k+5]*u)*v
 *       sx = P(0)/P(6) + x0;   sy = P(12)/P(18) + y0.
 *   PIVLFN_DEWARP_NEAREST: (rx, ry) = rint of each (half to even, np.round); out = frames[ry][rx] if 0 <= rx <= W-1 and 0 <= ry <= H-1,
 *   else fill.  PIVLFN_DEWARP_BILINEAR: fx = floor(sx), fy = floor(sy), ax = sx - fx, ay = sy - fy; if the four taps (fx, fy) ..
 *   (fx+1, fy+1) all lie inside the image,
 *       top = (1-ax)*I[fy][fx] + ax*I[fy][fx+1];  bot = (1-ax)*I[fy+1][fx] + ax*I[fy+1][fx+1];  val = (1-ay)*top + ay*bot
 *   (fp64), stored as (float)val or as rint(val) clamped to 0..255; else fill.  A non-finite source position gives fill.
 *   fill: (float)fill, finite and within the fp32 range or a NaN; for bytes an integer 0..255.  One launch.  out must not be frames.
 *   On a square image whose sources all fall inside, NEAREST is the reference's warp (dewarp.py:196-252).  Two deliberate differences:
 *   the reference swaps width and height on non-square images (`width, height = gray_img.shape`), and it maps out-of-range sources to
 *   the LAST pixel (dewarp.py:235-236) although its comment says they are painted black; here they get `fill`.
 *
 * Errors (PIVLFN_ERR_ARG, before any launch): a null pointer;  B outside 1..65535;  H or W < 1;  H*W >= 2^31 - 256;  an even or
 * oversized template;  cap out of range;  a NaN threshold;  a misaligned or short workspace;  a non-finite coefficient or origin;  a
 * fill that the frame type cannot hold;  an unknown mode. */
#define PIVLFN_DEWARP_NEAREST  0
#define PIVLFN_DEWARP_BILINEAR 1
size_t pivlfn_template_match_workspace_bytes(int th, int tw);
int pivlfn_template_match(const unsigned char *images, const unsigned char *templ, float *r, int B, int H, int W, int th, int tw,
                          void *workspace, size_t workspace_bytes, void *stream);
size_t pivlfn_target_points_workspace_bytes(int B, int H, int W);
int pivlfn_target_points(const float *r, int B, int H, int W, float threshold, int cap, int *labels, int *count, long long *rec,
                         void *workspace, size_t workspace_bytes, void *stream);
int pivlfn_dewarp_frames(const void *frames, void *out, int is_f32, int B, int H, int W, const double *A, double x0, double y0,
                         int mode, double fill, void *stream);

/* ---- network: replaces LiteFlowNet.__init__ + load_state_dict (src/models.py:39-317, 736-738, 762-764).
 * Uploads and repacks the weights once (this is the only call that allocates device memory).
 * starting_scale / lowest_level / rgb_mean as in the factories src/models.py:729-730, 754-755. */
int pivlfn_create(const pivlfn_tensor *tensors, int n_tensors, float starting_scale, int lowest_level,
                  const float rgb_mean[6], pivlfn_net **out);
int pivlfn_destroy(pivlfn_net *net);

/* Bytes of scratch pivlfn_forward needs for a [B,3,H,W] pair batch (H, W multiples of 32) in the precision mode set at the time of
 * the query: ask again after pivlfn_set_precision (a forward whose mode needs more than it is given returns PIVLFN_ERR_WORKSPACE).
 * In the fp32 Winograd modes (PIVLFN_PRECISION_F32 and _F32_WINO_MFMA32): 5604 MiB per pair at 1024 x 1024 with lowest_level 1
 * (1788 MiB with lowest_level 2); of that, 672 MiB (160 MiB) hold the flow-independent partial sums of Regularization's first
 * layer at the levels of at least 256 x 256 pixels.  The other modes do without them: 4932 MiB (1628 MiB). */
size_t pivlfn_workspace_bytes(const pivlfn_net *net, int B, int H, int W);

/* ---- replaces LiteFlowNet.forward in eval mode, src/models.py:319-370.
 * img1, img2: NCHW [B,3,H,W] in [0,1] (NOT modified: the reference's in-place mean subtraction
 * :321-323 happens on an internal copy).  flow: NCHW [B,2,H/2^(lowest_level-1),W/2^(lowest_level-1)],
 * already multiplied by SCALEFACTOR[1] (:370).
 * levels (optional, may be NULL): receives the per-level [M,S,R] flows of the training-mode return
 * (:363-367), coarsest level first, each NCHW [B,2,h,w], packed back to back.
 * The workspace needs no initial contents: flow and levels do not depend on what it holds before the call (alignment gaps included),
 * and nothing outside workspace[0, workspace_bytes), flow and levels is written. */
int pivlfn_forward(pivlfn_net *net, const float *img1, const float *img2, float *flow, float *levels,
                   int B, int H, int W, void *workspace, size_t workspace_bytes, void *stream);

/* Precision of the conv stacks inside pivlfn_forward.
 * PIVLFN_PRECISION_F32 (the library's default, the mode every fp32 parity statement and the headline benchmark refer to):
 * fp32 operands, fp32 products and fp32 accumulation on the fp32 matrix-core instruction v_mfma_f32_32x32x2_f32 (exact fma
 * chains).  The 3 x 3 / stride 1 layers with an output grid of at least 64 x 64 per image are computed by Winograd's minimal
 * filtering F(2x2, 3x3) (csrc/conv_wino.hip; the algorithm cuDNN / MIOpen choose for fp32 3 x 3 layers: 2.25 x fewer multiplies,
 * all of them fp32 x fp32 on 24-bit operands; tests/test_gpu_wino.py measures the error against float64 next to the direct
 * kernel's); every other layer by direct convolution.  PIVLFN_PRECISION_F32_DIRECT: direct convolution for every layer.
 * PIVLFN_PRECISION_F16 (BASELINE config #5): operands rounded to fp16 while they are staged, fp32 accumulation, activations
 * still fp32 in HBM; flows agree with the fp32 mode to an end-point error stated in tests/test_gpu_f16.py.
 * Everything that is not a convolution (correlation, warps, flow heads, regularisation tail) is fp32 in all modes. */
#define PIVLFN_PRECISION_F32 0
#define PIVLFN_PRECISION_F16 1
#define PIVLFN_PRECISION_F32_DIRECT 4
/* PIVLFN_PRECISION_F32_WINO_MFMA32: the default of rounds 3-5 -- as PIVLFN_PRECISION_F32, but every Winograd layer on the fp32 matrix
 * instruction (csrc/conv_wino.hip).  Since round 6 PIVLFN_PRECISION_F32 runs the Winograd layers with whole 64-channel output groups
 * and >= 48 staged input channels on csrc/conv_wino_b3.hip: the same algorithm and the same fp32 U = G g G^T, each fp32 operand split
 * EXACTLY into three bf16 pieces (8 + 8 + 8 significand bits, fp32's exponent range: no narrower input domain) and each product
 * formed from six exact bf16 x bf16 products accumulated in fp32 on v_mfma_f32_32x32x16_bf16 -- what is dropped (ml + lm + ll) is
 * about 2^-25 of a product under round-to-nearest pieces: of the order of the rounding an fp32 fma commits on the same product (at
 * most 2^-24 of it), not below every such rounding; measured against float64 the layer error is at or below both
 * fp32-instruction kernels' (tests/test_gpu_wino_b3.py).  Regularization's (7 x 1) 49 <- 32 and (1 x 7) 49 <- 49 distance layers of
 * levels 1 and 2 (>= 256 x 256 pixels per image) multiply the same way on v_mfma_f32_16x16x32_bf16 (csrc/conv_dist_b3.hip,
 * tests/test_gpu_dist_b3.py; their output channel 48 is an fp32 fma chain); under F32_WINO_MFMA32 they stay on v_mfma_f32_16x16x4_f32. */
#define PIVLFN_PRECISION_F32_WINO_MFMA32 5
/* PIVLFN_PRECISION_F32_SPLIT: fp32 results from the fp16 matrix cores.  Every fp32 operand is split exactly into three fp16
 * pieces (11 + 11 + 2 significand bits at scales 1, 2^-11, 2^-22) and each product is formed from six exact fp16 x fp16
 * products accumulated in fp32; what is dropped is below 2^-32 of a product, 256 x under the rounding of an fp32 fma
 * (csrc/conv_split.hip; tests/test_gpu_split.py measures the error against float64 next to the fp32 instruction's).
 * Applies to the residual-free stride-1 convolutions with an output grid of at least 256 x 256 per image; everything else runs
 * as in F32.  Inputs of those layers must stay below 65504 in magnitude (fp16 range of the leading piece; beyond it the
 * result is NaN, not a silently saturated value); inputs below 2^-14 in magnitude are represented to an absolute 2^-37
 * (2^-26 in SPLIT3) instead of exactly. */
#define PIVLFN_PRECISION_F32_SPLIT 2
/* PIVLFN_PRECISION_F32_SPLIT3: the same with two pieces per operand and the three leading partial products (h.h, h.m, m.h):
 * a product carries a relative error of at most 2^-21 (typically 2^-23.5, about one fp32 ulp on each operand); measured against
 * float64 the layer outputs' mean error stays within 2 x the fp32 instruction's (what tests/test_gpu_split.py asserts; on the layers
 * measured there it was lower: the fp16 instruction rounds once per 16 products), at half the matrix work of SPLIT.  Applies to the residual-free convolutions with an output grid of at least 64 x 64 per
 * image: stride 1 (4-row tiles and split-K on the small grids) and 3 x 3 stride 2.  Opt-in (not the default): the multiplicands
 * are 22-23 bits wide, one fewer than fp32's. */
#define PIVLFN_PRECISION_F32_SPLIT3 3
int pivlfn_set_precision(pivlfn_net *net, int precision);

/* Number of floats `levels` must hold for pivlfn_forward. */
size_t pivlfn_levels_floats(const pivlfn_net *net, int B, int H, int W);

/* ---- one convolution layer on the network's channels-last layout (what pivlfn_forward launches for every
 * torch.nn.Conv2d of src/models.py:70-106, 124, 154-163, 197-207, 229-272); exported so the kernel can be checked and
 * timed on its own.  weight: host, OIHW [cout,cin,kh,kw]; bias: host [cout].
 * x: [B,H,W,x_stride] (first cin lanes used, x_stride % 4 == 0, lanes cin..roundup(cin,4) must be finite, lanes past them are
 * not read);  y: [B,Ho,Wo,y_stride], lanes cout..min(roundup(cout,4), y_stride) are written as exact zeros, lanes past them untouched;
 * res (optional): same grid as y, added before the activation; its lanes cout..roundup(cout,4) are added into y's zero lanes, so they
 * must be +0.0 (pivlfn_forward's residuals, upConv_M's flow and the previous flow head's output, hold +0.0 there), and lanes past
 * them are not read; leaky: LeakyReLU(0.1) on the result.
 * Dispatch = the PIVLFN_PRECISION_F32_WINO_MFMA32 network's for the shape, except Winograd (own entry points below; the split-bf16
 * distance kernels of PIVLFN_PRECISION_F32 have theirs too, pivlfn_conv2d_nhwc_dist_b3): the direct kernel
 * everywhere, but a 7 x 1 layer (pad 3, 0; no residual, no activation) on an image of >= 256 x 256 pixels runs on the streaming
 * matrix-core kernel pivlfn_forward uses for conv_dist_R.0 there -- not bit-comparable with the F32_DIRECT network's layer.
 * The handle's split-K scratch holds one image's shares: a batch it is too small for runs image by image, so a sample's split factor
 * -- pivlfn_forward's for that image -- and its bits do not depend on B. */
typedef struct pivlfn_conv pivlfn_conv;
int pivlfn_conv_create(const float *weight, const float *bias, int cout, int cin, int kh, int kw, pivlfn_conv **out);
int pivlfn_conv_destroy(pivlfn_conv *conv);
int pivlfn_conv2d_nhwc(const pivlfn_conv *conv, const float *x, int x_stride, float *y, int y_stride,
                       const float *res, int res_stride, int B, int H, int W, int stride, int pad_y, int pad_x,
                       int leaky, void *stream);
/* Which kernel pivlfn_conv2d_nhwc runs for a layer of this shape (as pivlfn_conv_create packs it) and a call of this geometry: the
 * launcher's own decision, made on the host -- nothing is launched, no handle and no GPU is needed.  has_res: a residual is passed.
 * plan[0] the kernel family, plan[1] / plan[2] the output rows / output channels of one workgroup's tile, plan[3] the v2 kernel's
 * staging class as 100 * PMAX + WMAX (309, 505 or 913; 0 for the other families), plan[4] the split-K shares (1 = not split).
 * A batch whose split-K shares exceed the handle's scratch runs image by image: the plan is then one image's.
 * Returns PIVLFN_ERR_ARG, with a message, for everything pivlfn_conv2d_nhwc refuses for that geometry (its pointers apart).
 * Whether a geometry is accepted, and the split-K shares, never depend on B; family and tile do, the bits of a sample do not
 * (tests/test_conv_plan.py, tests/test_gpu_conv_tiles.py). */
#define PIVLFN_CONV_PLAN_V2   1   /* conv_mfma2_kernel<rows / 4, channels / 32, PMAX, WMAX>, register-prefetched */
#define PIVLFN_CONV_PLAN_V1   2   /* conv_mfma_kernel<rows / 4, channels / 32>: what v2's staging classes do not cover */
#define PIVLFN_CONV_PLAN_K1   3   /* one 4-channel K chunk, >= 16 taps: weights resident, persistent workgroups (from 1024 tiles; at any
                                   * count where no other kernel takes the layer) */
#define PIVLFN_CONV_PLAN_C3K7 4   /* 7 x 7 from 3 channels to 32, taps packed into K */
#define PIVLFN_CONV_PLAN_S2   5   /* 3 x 3 stride 2 from 32 channels, whole lines */
#define PIVLFN_CONV_PLAN_COL7 6   /* streaming 7 x 1 */
#define PIVLFN_CONV_PLAN_ROW7 7   /* streaming 1 x 7 */
int pivlfn_conv2d_nhwc_plan(int cout, int cin, int kh, int kw, int B, int H, int W, int stride, int pad_y, int pad_x,
                            int has_res, int leaky, int x_stride, int y_stride, int plan[5]);

/* The same layer in the optional reduced-precision mode (BASELINE config #5: fp16 multiplicands, fp32 accumulation, on
 * v_mfma_f32_32x32x16_f16): x is fp32 or fp16 elements (x_is_f16; stride granularity 4 / 8 elements), y is stored as fp32
 * or fp16 (y_is_f16); with fp16 x, lanes cin..roundup(cin,8) must be finite and lanes past them are not read.  No residual input. */
int pivlfn_conv2d_nhwc_f16(const pivlfn_conv *conv, const void *x, int x_stride, int x_is_f16, void *y, int y_stride,
                           int y_is_f16, int B, int H, int W, int stride, int pad_y, int pad_x, int leaky, void *stream);

/* The same layer (stride 1, no residual) on the split-operand kernel of PIVLFN_PRECISION_F32_SPLIT (terms = 6) or
 * PIVLFN_PRECISION_F32_SPLIT3 (terms = 3): fp32 x, fp32 y. */
int pivlfn_conv2d_nhwc_split(const pivlfn_conv *conv, const float *x, int x_stride, float *y, int y_stride,
                             int B, int H, int W, int stride, int pad_y, int pad_x, int leaky, int terms, void *stream);

/* The same layer (3 x 3, stride 1, pad 1, no residual) on the Winograd F(2x2, 3x3) kernel PIVLFN_PRECISION_F32 uses: fp32 x,
 * fp32 y, output grid = input grid. */
int pivlfn_conv2d_nhwc_wino(const pivlfn_conv *conv, const float *x, int x_stride, float *y, int y_stride,
                            int B, int H, int W, int leaky, void *stream);
/* The same layer (3 x 3, stride 1, pad 1, no residual; cout rounded up to 32 a multiple of 64) by Winograd F(2x2, 3x3) with every
 * fp32 operand split exactly into three bf16 pieces (8 + 8 + 8 significand bits, fp32's exponent range) and the products formed
 * on v_mfma_f32_32x32x16_bf16 (csrc/conv_wino_b3.hip): terms = 6 (dropped piece products about 2^-25 of a product), 8
 * (<= 2^-32) or 9 (the exact product of the two fp32 operands).  fp32 x, fp32 y. */
int pivlfn_conv2d_nhwc_wino_b3(const pivlfn_conv *conv, const float *x, int x_stride, float *y, int y_stride,
                               int B, int H, int W, int leaky, int terms, void *stream);
/* Regularization's two 49-channel distance layers -- (7 x 1) from 32 channels (pad 3, 0) and (1 x 7) from 49 channels on 52 staged lanes
 * (pad 0, 3); stride 1, no residual, no activation, output grid = input grid -- on the streaming kernel PIVLFN_PRECISION_F32 uses for them
 * on images of >= 256 x 256 pixels (csrc/conv_dist_b3.hip): the structure of the fp32-instruction kernels behind pivlfn_conv2d_nhwc, every
 * fp32 operand split exactly into three bf16 pieces and the products formed on v_mfma_f32_16x16x32_bf16; terms = 6, 8 or 9 as above.
 * Output channel 48 is an fp32 fma chain on the vector unit.  Any H, W >= 1.  x: x_stride % 4 == 0 and >= 32 (7 x 1) or >= 52 (1 x 7;
 * lanes 49..51 are not read); y: y_stride % 4 == 0 and >= 52, lanes 49..51 are written as exact zeros, lanes past them untouched.
 * One image's loads and stores use 32-bit byte offsets: H * W * max(x_stride, y_stride) * 4 < 2^31.  Other layers are refused. */
int pivlfn_conv2d_nhwc_dist_b3(const pivlfn_conv *conv, const float *x, int x_stride, float *y, int y_stride,
                               int B, int H, int W, int terms, void *stream);
/* What pivlfn_conv2d_nhwc_dist_b3 launches for a layer of this shape and a call of this geometry, from its own checks: nothing is launched,
 * no handle and no GPU is needed.  plan[0] 0 = the (7 x 1) layer (a wave walks rows), 1 = the (1 x 7) layer (columns); plan[1] terms;
 * plan[2] the workgroups (four 16 x 16-pixel tiles each); plan[3] the workgroups per CU the kernel is compiled for.
 * Returns PIVLFN_ERR_ARG, with the same message, for everything the entry point refuses for that geometry (its pointers apart). */
int pivlfn_conv2d_nhwc_dist_b3_plan(int cout, int cin, int kh, int kw, int B, int H, int W, int terms, int x_stride, int y_stride,
                                    int plan[4]);
/* Which kernel pivlfn_conv2d_nhwc_f16 / _split / _wino / _wino_b3 runs for a layer of this shape (as pivlfn_conv_create packs it) and a
 * call of this geometry: the entry point's own checks and the launcher's own decision, made on the host -- nothing is launched, no handle
 * and no GPU is needed.  kernel: PIVLFN_KERNEL_PLAN_F16, _SPLIT, _WINO or _WINO_B3, the entry point asked about.  terms: the split entry
 * point's (3 or 6) and the wino_b3 one's (6, 8 or 9), ignored by the others; x_is_f16: the f16 entry point's, ignored by the others; the
 * two Winograd entry points take stride 1 and padding 1 only.  cus: the compute units the wino_b3 kernel's persistent grid is sized for
 * (the library asks the device; here the caller says, so that the function needs none), >= 1, ignored by the others.
 *   plan[0]  the kernel, PIVLFN_KERNEL_PLAN_*: for the split entry point _SPLIT (conv_split_kernel) or _SPLIT_BIG (conv_split_big_kernel)
 *   plan[1]  piece products per product, the kernel's TERMS (split: 3 or 6, 3 for the big kernel; wino_b3: 6, 8 or 9; else 0)
 *   plan[2]  output rows of one workgroup's tile     (f16, split: 4 * MT; wino: 8 * MB; big, wino_b3: 16)
 *   plan[3]  output channels of one workgroup's tile (f16, split, big: 32 * NT; wino: 32 * NBW; wino_b3: 64)
 *   plan[4]  the staging class as 100 * PM + WM (f16, split; else 0)
 *   plan[5]  the workgroups per CU the kernel is compiled for (its launch bound)
 *   plan[6]  the split-K shares (1 = not split; only the three-term split kernel splits)
 *   plan[7]  1 when the big split kernel multiplies the layer's 4-lane tail chunk with its taps folded into K
 *   plan[8]  1 when the handle runs the batch image by image (split: a batch on a grid small enough for split-K, since the handle's
 *            scratch holds one image's shares); plan[] is then one image's
 *   plan[9]  the workgroups of the launch (per image where plan[8] is set; the split-K reduction's launch not counted)
 * Returns PIVLFN_ERR_ARG, with the same message, for everything the entry point refuses for that geometry (its pointers apart).
 * Whether a geometry is accepted and the split-K shares never depend on B, nor does the choice between the big and the small split kernel
 * for a layer with a folded tail; the tile otherwise does, the bits of a sample do not (tests/test_conv_kernel_plans.py,
 * tests/test_gpu_conv_kernel_tiles.py). */
#define PIVLFN_KERNEL_PLAN_F16       1   /* conv_f16_kernel<rows / 4, channels / 32, PM, WM> */
#define PIVLFN_KERNEL_PLAN_SPLIT     2   /* conv_split_kernel<terms, rows / 4, channels / 32, PM, WM, workgroups per CU> */
#define PIVLFN_KERNEL_PLAN_SPLIT_BIG 3   /* conv_split_big_kernel<channels / 32>: 16 rows, one workgroup per CU, three-term products */
#define PIVLFN_KERNEL_PLAN_WINO      4   /* conv_wino_kernel<rows / 8, channels / 32> */
#define PIVLFN_KERNEL_PLAN_WINO_B3   5   /* conv_wino_b3_kernel<terms>: min(tiles, cus) persistent workgroups */
int pivlfn_conv2d_nhwc_kernel_plan(int kernel, int cout, int cin, int kh, int kw, int B, int H, int W, int stride, int pad_y, int pad_x,
                                   int terms, int x_is_f16, int x_stride, int y_stride, int cus, int plan[10]);
#ifdef PIVLFN_TOOLS
/* Tools build only (tools/libpivlfn_tools.so; the kernel lives in tools/kernels/conv_wino4.hip since round 6): the same layer on the
 * Winograd F(4x4, 3x3) kernel (6 x 6 transforms; relative error ~1e-5 against ~1.4e-6 of F(2x2)).  Measured 0.98x of F(2x2) on
 * 128->128 at 1024 x 1024 and slower below: no user path launches it. */
int pivlfn_conv2d_nhwc_wino4(const pivlfn_conv *conv, const float *x, int x_stride, float *y, int y_stride,
                             int B, int H, int W, int leaky, void *stream);
#endif

/* One Conv2d (odd k, stride 1, "same" padding, + bias, optional LeakyReLU(0.1)) over the channel concatenation of 1-3 sources --
 * torch.cat + Conv2d of the front layers of Matching / Subpixel / Regularization (src/models.py:171-187, 209-217, 280) -- through
 * the dispatch of PIVLFN_PRECISION_F32: the multi-source staging of the direct and the Winograd kernel, for per-layer checks.
 * weight is OIHW over the concatenated channels; channels[i] = real channels of source i; x[i] is [B,H,W,x_stride[i]] with
 * x_stride[i] a multiple of 4 and >= channels[i] rounded up to 4 (padding lanes zero, lanes past them not read); only the last source
 * may have a channel count that is 4 (mod 8) after rounding. */
int pivlfn_conv_create_cat(const float *weight, const float *bias, int cout, int nsrc, const int *channels, int kh, int kw,
                           pivlfn_conv **out);
int pivlfn_conv2d_nhwc_cat(const pivlfn_conv *conv, int nsrc, const float *const *x, const int *x_stride, float *y, int y_stride,
                           int B, int H, int W, int leaky, void *stream);

/* The 32 -> 2 channel k x k flow head (conv_M.6 / conv_S.6) on its dedicated kernel: x [B,H,W,32], res4/out4 [B,H,W,4].  Lanes 2-3
 * of res4 are not read (pivlfn_forward's flow4 holds zeros there); lanes 2-3 of out4 are written as +0.0.  res4 may be NULL: no
 * residual is added (pivlfn_forward's coarsest level, which has no flow to refine); the bits are those of a residual of +0.0. */
int pivlfn_conv_head_nhwc(const pivlfn_conv *conv, const float *x, const float *res4, float *out4, int B, int H, int W,
                          void *stream);
/* Which kernel pivlfn_conv_head_nhwc runs for a k x k head (k = 3, 5, 7) on B images of H x W: the launcher's own decision, made on
 * the host -- nothing is launched, no handle and no GPU is needed.  plan[0] the kernel family, plan[1] / plan[2] the output rows /
 * columns of one workgroup's tile (16 x 16, 16 x 16, 32 x 32, 8 x 58), plan[3] the workgroups of the launch.
 * Returns PIVLFN_ERR_ARG, with the same message, for everything pivlfn_conv_head_nhwc refuses for that geometry (its pointers apart).
 * The family depends on the size of one image alone, never on B: the families sum in different orders, and a pair's flow must not
 * depend on its batch mates (tests/test_conv_head_plan.py, tests/test_gpu_conv_head.py).  Added without an ABI bump (additive). */
#define PIVLFN_HEAD_PLAN_PIXEL_LDS 1   /* conv_head_kernel<k, true>: one pixel per lane, weights in LDS; at most 512 tiles of 16 x 16 per image */
#define PIVLFN_HEAD_PLAN_PIXEL     2   /* conv_head_kernel<k, false>: the same with the weights through the scalar cache; same bits */
#define PIVLFN_HEAD_PLAN_ROWS4     3   /* conv_head4_kernel<k>: four rows per lane; images of >= 512 x 512 pixels that MFMA does not take */
#define PIVLFN_HEAD_PLAN_MFMA      4   /* conv_head_mfma_kernel<7, 8>: k = 7, images of >= 256 x 256 pixels and < 2^31 bytes of input */
int pivlfn_conv_head_nhwc_plan(int k, int B, int H, int W, int plan[4]);

/* ---- per-layer checks: the level-pipeline ops that otherwise run only inside pivlfn_forward, each on the kernel and with the
 * weight packing pivlfn_forward uses, exported so that every kernel can be checked on its own (tests/test_gpu_net_ops.py).  Not a
 * hot path: the two entry points that take host weights pack and upload them per call and synchronise `stream` before returning.
 * Added without an ABI bump (additive).  Layouts are the network's channels-last ones; "flow4" is [B,H,W,4] = (u, v, 0, 0).
 *
 * upConv_M / upCorr_M, src/models.py:144-145, 151-152 (depthwise ConvTranspose2d k4 s2 p1, no bias).  quads = 1: the flow, 2
 * channels on 4 lanes; quads = 14: the correlation, 49 channels on 56 lanes.  w16: host, OIHW [C,1,4,4] (C = 2 or 49).  in:
 * [B,H,W,stride_in]; out: [B,2H,2W,stride_out], lanes 0..4*quads-1 written (padding lanes as exact zeros: the input's padding
 * lanes must be finite), the rest untouched.  Strides are multiples of 4 and >= 4*quads; 2H <= 65535, B <= 65535. */
int pivlfn_upconv_nhwc(const float *in, const float *w16, float *out, int B, int H, int W, int quads, int stride_in,
                       int stride_out, void *stream);
/* Subpixel's backwarp(feat2, flow * scale), src/models.py:214: in / out [B,H,W,C] (C % 4 == 0), flow4 [B,H,W,4]; fewer than
 * 2^31 (pixel, channel quad) work items. */
int pivlfn_backwarp_nhwc(const float *in, const float *flow4, float scale, float *out, int B, int H, int W, int C, void *stream);
/* Regularization front, src/models.py:275-277: mean_out [B,2] = per-image mean of (u, v); misc4 [B,H,W,4] = (||img1 - backwarp(img2,
 * flow * scale)||_2 over the 3 colour lanes, u - mean_u, v - mean_v, 0).  img1_4 / img2_4 [B,H,W,4]; partial_ws: device scratch
 * of 128 * B floats, no initial contents needed.  Lane 3 of img1_4 / img2_4 is not read; misc4 lane 3 is written as +0.0.
 * fused = 1: pivlfn_forward's path (partial sums, the mean formed inside the reg_prep kernel); fused = 0: the one-wave mean kernel,
 * then reg_prep reads mean_out.  Both give the same bits.  1 <= B <= 65535. */
int pivlfn_reg_prep(const float *img1_4, const float *img2_4, const float *flow4, float scale, float *misc4, float *mean_out,
                    float *partial_ws, int B, int H, int W, int fused, void *stream);
/* Regularization tail, src/models.py:281-302: softmax(-dist^2) over the k*k channels, the k x k unfold of (u, v) with zero padding,
 * moduleScaleX / Y (wx, wy: DEVICE pointers to k*k floats; bx, by their biases), divided by the softmax sum.  dist [B,H,W,dstride]
 * (first k*k lanes used, dstride >= k*k), flow4 [B,H,W,4], k in {3, 5, 7}.  out4 [B,H,W,4] = (u', v', 0, 0) and / or out_nchw
 * [B,2,H,W] = out_scale * (u', v'); either may be NULL, not both. */
int pivlfn_reg_tail(const float *dist, int dstride, const float *flow4, const float *wx, const float *wy, float bx, float by,
                    int k, float *out4, float *out_nchw, float out_scale, int B, int H, int W, void *stream);
/* Mean subtraction and image pyramid, src/models.py:321-323, 336-343: img1 / img2 NCHW [B,3,H,W]; mean6 host, 6 floats (frame 1's
 * RGB means, then frame 2's).  out_levels receives levels 1..levels (1..6) back to back, level L = [2B, H>>(L-1), W>>(L-1), 4]
 * (frames 1 then frames 2, lane 3 zero), each level the bilinear (align_corners=False) resize of the one before. */
int pivlfn_prep_pyramid(const float *img1, const float *img2, const float *mean6, float *out_levels, int B, int H, int W,
                        int levels, void *stream);
/* NetC.conv1 (7 x 7, 3 -> 32, LeakyReLU) with level 1's NetC_ext (1 x 1, 32 -> 64, LeakyReLU) and moduleFeat (1 x 1, 32 -> 128,
 * LeakyReLU) on top: src/models.py:70-72, 124, 227-232.  Weights host, OIHW, with their biases.  x [N,H,W,4] (lane 3 finite);
 * out [N,H,W,32], out_ext [N,H,W,64] for every image, out_feat [B_feat,H,W,128] for the first B_feat (1..N) images only.  Where the
 * image has >= 512 tiles of 8 x 32 pixels, the three layers run in conv1's kernel as in pivlfn_forward and *fused = 1; below, the
 * three layers run on their own kernels and *fused = 0 (fused may be NULL). */
int pivlfn_conv1_fused_nhwc(const float *w1, const float *b1, const float *w_ext, const float *b_ext, const float *w_feat,
                            const float *b_feat, const float *x, float *out, float *out_ext, float *out_feat, int N, int H, int W,
                            int B_feat, int *fused, void *stream);

/* ---- measurement hooks.  With profiling on, pivlfn_forward times the level-`level` warp+correlation launch
 * with HIP events on `stream` in two ways: start/stop events attached to the dispatch itself
 * (hipExtLaunchKernelGGL: the dispatch's own begin/end timestamps) and a plain hipEventRecord pair around it
 * (which also contains the marker packets' own cost).  pivlfn_profile_read() synchronises those events and
 * returns both accumulated times in milliseconds and the launch count since the last reset. */
int pivlfn_profile_enable(pivlfn_net *net, int level);   /* level 1..6, 0 = off */
int pivlfn_profile_read(pivlfn_net *net, double *ms_dispatch, double *ms_event_pair, long *launches, int reset);

/* ---- uncertainty of an estimated flow from correlation statistics (Wieneke 2015, "PIV uncertainty quantification from correlation
 * statistics"): per vector and axis, the standard uncertainty in pixels that follows from how asymmetric the correlation peak of image 1
 * against image 2 warped back by the flow may be, given the pixel-wise scatter of the products the peak is summed from, carried
 * through the three-point Gaussian peak fit.  Needs no truth field.  Added without an ABI bump (additive).
 * img1, img2, flow, mask: as for pivlfn_match_quality;  unc: NCHW [B,2,H,W] fp32, planes ux, uy in pixels;  flag: [B,H,W] bytes;
 * workspace: 8-byte aligned, at least pivlfn_flow_uncertainty_workspace_bytes(B,H,W,radius,lag) bytes (74 bytes per pixel and pair:
 * nine fp64 planes and two bytes; 0 for arguments out of range), needs no initial contents.  Launches only on `stream`, no
 * allocation, no host synchronisation, no floating-point atomics; no output depends on what unc, flag or the workspace held before
 * the call; a pair gives the same bits alone, inside any batch and from run to run.
 * Arithmetic contract, all fp64, every operation rounded on its own (no fma), divisions and square roots correctly rounded; r =
 * radius:
 *   a, b, m, k:  the gray value a of img1, the warped gray value b of img2, the validity m of the sample and the exclusion k, word for
 *                word those of pivlfn_match_quality (the same kernel forms them).  Pixel q is valid, v(q) = 1, iff k(q) = 1 && m(q) = 1.
 *   box sums:    every sum below over a (2*R+1)^2 box around a pixel is taken over the box clipped to the image, in
 *                pivlfn_match_quality's order: per row the terms left to right from +0.0, then the row sums top to bottom from
 *                +0.0; a term that is not defined is +0.0.  The order is fixed by this contract and not by the launch geometry.
 *   high-pass:   n1(q), A1(q), B1(q) = the box sums of radius r of v, of a where v = 1 and of b where v = 1.  Where v(q) = 1:
 *                a'(q) = a(q) - A1(q)/n1(q), b'(q) = b(q) - B1(q)/n1(q) (the local background would flatten the peak).
 *   fields:      p(q) = a'(q)*b'(q) where v(q) = 1.  For the axis e in {(1,0), (0,1)} (x, then y), where q+e lies inside the image and
 *                v(q) = v(q+e) = 1 (q is a pair of e): t1 = a'(q)*b'(q+e), t2 = a'(q+e)*b'(q), s_e(q) = t1 + t2, d_e(q) = t1 - t2
 *                (the terms of C+ + C- and of C+ - C-);  D_e(q) = the box sum of radius `lag` of d_e;  g_e(q) = d_e(q)*D_e(q) where q
 *                is a pair of e: its window sum is the autocovariance of the terms of C+ - C- summed over the lags |delta| <= lag,
 *                the variance of C+ - C-.
 *   window sums: box sums of radius r around p:  n0 of v, C0 of p, and per axis n_e of the pairs, S_e of s_e, V_e of g_e (the counts
 *                are exact).
 *   per axis:    sig = sqrt(V_e);  Cpm = 0.5*S_e;  Cm = Cpm - 0.5*sig;  Cp = Cpm + 0.5*sig.
 *   flag byte:   bit 0 (1) FEW: n0 < min_count || n_x < min_count || n_y < min_count;  bit 1 (2) FLAT: FEW is clear and
 *                C0 < floor*floor*n0;  where FEW and FLAT are clear: bit 2 (4) NO_PEAK: on either axis Cm <= 0 || C0 - Cp < 1e-6*C0
 *                (free of logarithms, so the flags are bit-exact; a NaN compares false);  bit 3 (8) NO_VARIANCE: on either axis
 *                V_e <= 0 or V_e is not finite;  bit 4 (16) CENTRE_OUT: v(p) = 0 (informational: the values are still formed).
 *   outputs:     where bits 0-3 are clear, with l = ln (the device library's fp64 logarithm, the one operation here that is not
 *                correctly rounded): u_e = | 0.5*(l(Cm) - l(Cp)) / ((l(Cm) - 2.0*l(C0)) + l(Cp)) |, rounded once to fp32; the
 *                conditions keep the denominator at or below about -2e-6.  Elsewhere both planes are NaN.
 * Errors (PIVLFN_ERR_ARG, before any launch): those of pivlfn_match_quality (with unc in the place of quality), and lag outside 0..4.
 *
 * pivlfn_uncertainty_accumulate adds the pairs of unc / flag, in batch order, to sums [3,H,W] fp64 (8-byte aligned; planes: the sum of
 * ux^2, the sum of uy^2, the number of pairs): one thread per pixel, sum = sum + (double)u*(double)u and n = n + 1.0 for every pair
 * whose flag has bits 0-3 clear, the others are skipped.  Only on `stream`, no atomics.  Errors: a null pointer, a non-positive size,
 * H*W >= 2^31, misaligned sums, sums overlapping an input. */
#define PIVLFN_UNCERTAINTY_FEW         1
#define PIVLFN_UNCERTAINTY_FLAT        2
#define PIVLFN_UNCERTAINTY_NO_PEAK     4
#define PIVLFN_UNCERTAINTY_NO_VARIANCE 8
#define PIVLFN_UNCERTAINTY_CENTRE_OUT 16
size_t pivlfn_flow_uncertainty_workspace_bytes(int B, int H, int W, int radius, int lag);
int pivlfn_flow_uncertainty(const float *img1, const float *img2, int C, const float *flow, const unsigned char *mask,
                            float *unc /* [B,2,H,W]: ux, uy in px */, unsigned char *flag /* [B,H,W] */, int B, int H, int W, int radius,
                            int lag, int min_count, double floor, void *workspace, size_t workspace_bytes, void *stream);
int pivlfn_uncertainty_accumulate(const float *unc, const unsigned char *flag, double *sums /* [3,H,W]: sum ux^2, sum uy^2, n */, int B,
                                  int H, int W, void *stream);

/* ---- velocity distributions of a flow SEQUENCE: per-pixel sums up to the fourth order with the quadrant split of U*V, and pooled
 * histograms (marginal, joint, and of the sub-pixel fraction of the raw displacement: peak locking).  Added without an ABI bump
 * (additive).
 * Common to both entry points.  flow: NCHW [B,2,H,W] fp32;  mask: [B,H,W] bytes or NULL, nonzero = leave the vector out;  mean: [2,H,W]
 * fp64 (the planes of u and v) or NULL.  One launch, only on `stream`; no allocation, no workspace, no host synchronisation, no
 * floating-point atomics; can be captured into a graph.  A vector at pixel p is LEFT OUT iff its mask byte is nonzero, or
 * !(|u| <= 1e9 && |v| <= 1e9) (NaN compares false; the 1e10 of a masked flow is invalid by itself), or a given mean or scale value at p
 * is not finite, or a scale is given and !(scale_u(p) > 0 && scale_v(p) > 0).  All arithmetic is fp64, every operation rounded on its
 * own (no fma; (double) of a float is exact):
 *   U = (double)u - mean_u(p), V = (double)v - mean_v(p);  with a NULL mean U = (double)u, V = (double)v.
 *
 * pivlfn_flow_moments_accumulate.  acc: [PIVLFN_MOMENT_TERMS, H, W] fp64, read once and written once per call;  thr: [H,W] fp64 or NULL
 * (0.0), the hole of the quadrant analysis.  Per pixel, frame by frame in frame order, acc[t][p] = acc[t][p] + term_t:
 *   0: 1 (the count);  1, 2: U, V;  3..5: U*U, V*V, U*V;  6..9: (U*U)*U, (V*V)*V, (U*U)*V, (V*V)*U;
 *   10..12: (U*U)*(U*U), (V*V)*(V*V), (U*U)*(V*V);  13..16: 1 for the quadrant of the vector;  17..20: P = U*V for that quadrant.
 *   Quadrants: Q1 U > 0 && V > 0, Q2 U < 0 && V > 0, Q3 U < 0 && V < 0, Q4 U > 0 && V < 0.  A vector takes part in its quadrant iff
 *   fabs(P) > thr(p) (a NaN thr admits nothing); the terms of the other quadrants, and all eight where it takes part in none, are not
 *   added to (no + 0.0).  A vector that is left out is skipped: its pixel's 21 values keep their bits.
 *   B frames in one call give the bits of B calls of one frame; no value depends on the launch geometry.
 *
 * pivlfn_flow_hist_accumulate.  scale: [2,H,W] fp64 or NULL;  hist: PIVLFN_HIST_WORDS(nbins, jbins, fbins) unsigned 64-bit counters, added
 * to with integer atomics and never reset, so the result has the same bits whatever the launch geometry, the arrival order or the
 * cutting of the sequence.  nbins 1..4096, jbins 0..256 (0: no joint histogram), fbins 0..1024 (0: none), hi > lo, both finite.
 *   s = (double)nbins / (hi - lo) and sj = (double)jbins / (hi - lo), each formed once on the host.
 *   samples:   X = U / scale_u(p), Y = V / scale_v(p);  with a NULL scale X = U, Y = V.
 *   marginal:  t = (X - lo) * s;  t < 0: the underflow slot;  t >= nbins: the overflow slot;  otherwise slot (int)t.  (A NaN t, which
 *              needs an s or a difference beyond the range of a double, counts as overflow.)
 *   layout:    1. u marginal, nbins + 2 words (under, the bins, over);  2. v marginal, the same;  3. joint, jbins * jbins words, row = the
 *              bin of Y, column = the bin of X, binned like a marginal with sj;  4. one word: the vectors outside the joint range in
 *              either component (with jbins = 0: every vector counted);  5. the fraction histogram of u, then of v, fbins words each;
 *              6. two words: the vectors counted, the vectors left out.
 *   fraction:  of the RAW displacement -- mean and scale do not enter:  d = (double)u;  f = d - floor(d);
 *              k = min((int)(f * (double)fbins), fbins - 1)  (a tiny negative d has f = 1.0 and lands in the last bin).
 *   Every vector adds 1 to exactly one word of each of the parts 1, 2, 3 + 4, 5u, 5v and to the first word of 6, or, if it is left out,
 *   to the last word alone.
 * pivlfn_flow_hist_plan (host only, nothing launched): what the launcher picks for such a call -- plan[0] the persistent workgroups of
 * the histogram launch, plan[1] the 32-bit counters of a workgroup's private table in LDS, plan[2] 1 if the joint table is part of it
 * and 0 if the joint histogram is updated in global memory directly, plan[3] PIVLFN_HIST_WORDS, plan[4] the workgroups of
 * pivlfn_flow_moments_accumulate at the same H and W.  It refuses what pivlfn_flow_hist_accumulate refuses before its pointers.
 * Errors (PIVLFN_ERR_ARG, before any launch), in this order: H < 1, W < 1, B < 0 or H*W >= 2^31;  (hist) nbins, jbins or fbins out of
 * range;  (hist) hi <= lo or either not finite;  then B == 0 succeeds, launches nothing and reads no pointer;  otherwise null flow, acc
 * or hist;  acc or hist overlapping flow, mask, mean, thr or scale. */
#define PIVLFN_MOMENT_TERMS 21
#define PIVLFN_HIST_WORDS(nbins, jbins, fbins) (2 * ((size_t)(nbins) + 2) + (size_t)(jbins) * (size_t)(jbins) + 1 + 2 * (size_t)(fbins) + 2)
int pivlfn_flow_moments_accumulate(const float *flow, const unsigned char *mask, const double *mean, const double *thr, double *acc,
                                   int B, int H, int W, void *stream);
int pivlfn_flow_hist_accumulate(const float *flow, const unsigned char *mask, const double *mean, const double *scale,
                                unsigned long long *hist, int B, int H, int W, double lo, double hi, int nbins, int jbins, int fbins,
                                void *stream);
int pivlfn_flow_hist_plan(int B, int H, int W, int nbins, int jbins, int fbins, int plan[5]);

/* ---- flow smoothing and gap filling: the orthonormal 2-D DCT-II of fp64 planes, and Garcia's penalised least squares (Comput. Stat. Data
 * Anal. 54, 2010; Exp. Fluids 50, 2011): per frame f and component c the field z that minimises  sum w (y - z)^2 + s |D z|^2,  that is
 *   A z = W y,   A = W + s D^T D,
 * W the diagonal of the weights (0 at masked and unknown vectors, so smoothing and gap filling are one solve), D the 5-point Laplacian
 * with reflecting boundaries.  Solved by conjugate gradients preconditioned with M = I + s D^T D, which the DCT diagonalises.  Added
 * without an ABI bump (additive).
 * Every entry point launches only on `stream`, allocates nothing, never synchronises the host, copies nothing from the host, uses no
 * atomics and can be captured into a graph as one linear chain of kernels; workspaces are 8-byte aligned and need no initial contents.
 * All arithmetic is fp64, every operation rounded on its own (no fma outside the matrix instruction; (double) of a float is exact).
 *
 * Tables, built on the device:  C_N[k][n] = a_k cos(pi m / 2N),  m = ((2n+1) k) mod 4N  reduced in integers and folded into [0, N/2] by
 *   the symmetries of the cosine (cospi(m/2N), or sinpi((N-m)/2N) past N/2),  a_0 = sqrt(1/N), a_k = sqrt(2/N): the orthonormal DCT-II
 *   of scipy.fft.dctn(norm="ortho").  lambda_N[k] = 4 sinpi(k/2N)^2 = 2 - 2 cos(pi k/N), the eigenvalues of the negated 1-D Laplacian.
 *
 * pivlfn_dct2 -- x, out [P,H,W] fp64;  forward (inverse = 0): out = C_H x C_W^T;  inverse: out = C_H^T x C_W.  Three launches: the
 *   tables, the product along the rows into the workspace, the product along the columns.  Each product is v_mfma_f64_16x16x4_f64 over
 *   k in ascending order, four k per instruction, into accumulators that start at +0.0; operands past an edge are +0.0.  An output value
 *   depends on its own plane alone: not on P, not on the other planes.  1 <= H, W <= PIVLFN_DCT_MAX, 1 <= P <= 65535, P*H*W < 2^31.
 *   workspace: pivlfn_dct2_workspace_bytes(P,H,W) bytes (0 for arguments out of range).
 *
 * T(.) is the tree sum of pivlfn_pressure_*, over the N = H*W nodes of one system (f, c) in row-major order.
 * Lap(a)(j,i) = ((l + r) + u) + d,  each term (neighbour - centre) for a neighbour inside the frame and +0.0 for one outside.
 * A a = w*a + s*Lap(Lap(a)).   M^-1 a = IDCT(Gamma o DCT(a)),  Gamma[k][l] = 1.0 / (1.0 + s*(e*e)),  e = lambda_H[k] + lambda_W[l],
 *   the product with Gamma being the last step of the forward transform.
 *
 * pivlfn_smooth_setup -- flows [F,2,H,W] fp32;  weights [F,H,W] fp32 or NULL (all 1);  mask [F,H,W] bytes or NULL.  Thirteen launches.
 *   w = (double)weight where the vector takes part, else +0.0.  A vector takes part iff its mask byte is zero (or mask is NULL), both its
 *   components satisfy |x| <= 1e9f (NaN fails: the unknown rule of pivlfn_vortex_gamma) and its weight is positive and finite.  The
 *   components of a vector that does not take part enter no arithmetic: b = w*(double)y where it takes part, else +0.0.
 *   x = M^-1 b;  r = b - A x;  z = M^-1 r;  rho = T(r*z);  rr = T(r*r);  bb = T(b*b);  iterations = 0;  state = PIVLFN_SMOOTH_RUNNING,
 *   or PIVLFN_SMOOTH_EMPTY where !(T(w) > 0): such a frame takes no further part.
 *
 * pivlfn_smooth_pcg -- enqueues `iters` iterations for all 2F systems in the same launches, eight launches per iteration.  s must be the
 *   s of the setup.  Every system has its own scalars and state: a frame's bits are the same alone, in any batch, and however `iters` is
 *   cut into calls; u and v of a frame share nothing but w.  One iteration of one system:
 *     1. if state != RUNNING, do nothing (the matrix products skip its planes).
 *     2. if rr <= (tol*tol)*bb, set state = CONVERGED and change nothing else.
 *     3. d = z (first iteration) or z + beta*d;  q = A d;  sigma = T(d*q).
 *     4. if !(sigma > 0), set state = BREAKDOWN and change nothing else (a NaN ends here).
 *     5. alpha = rho/sigma;  x = x + alpha*d;  r = r - alpha*q;  rr = T(r*r);  z = M^-1 r;  rho' = T(r*z);  beta = rho'/rho;  rho = rho';
 *        iterations += 1.
 *   With unit weights and no gap A = M, x from the setup is the solution and the system converges with 0 iterations.  M^-1 assumes
 *   weights of order 1: the iteration count grows as they leave it.
 *   iters == 0 succeeds and launches nothing.
 *
 * pivlfn_smooth_read -- z [F,2,H,W] fp64: x, or 1e10 in an EMPTY frame;  z32 (may be NULL): the same rounded to fp32;  filled (may be
 *   NULL) [F,H,W] bytes: 1 where w = 0;  status [F,2,4] fp64: state, iterations, rr, bb of each system.  One launch.  The workspace is not
 *   changed: iterating can go on afterwards.
 *
 * Errors (PIVLFN_ERR_ARG, on the host before any launch, the message names the problem): a null pointer;  H or W outside
 * 1..PIVLFN_DCT_MAX;  P outside 1..65535;  F outside 1..32767;  P*H*W or 2*F*H*W >= 2^31;  s or tol not finite and positive;  iters < 0;
 * a workspace that is misaligned or smaller than the query;  dct2: out overlapping x, the workspace overlapping either;  setup: the
 * workspace overlapping an input;  read: an output overlapping the workspace or another output. */
#define PIVLFN_DCT_MAX          4096
#define PIVLFN_SMOOTH_RUNNING   1
#define PIVLFN_SMOOTH_CONVERGED 2
#define PIVLFN_SMOOTH_BREAKDOWN 3
#define PIVLFN_SMOOTH_EMPTY     4
size_t pivlfn_dct2_workspace_bytes(int P, int H, int W);
int pivlfn_dct2(const double *x, double *out, int P, int H, int W, int inverse, void *workspace, size_t workspace_bytes, void *stream);
size_t pivlfn_smooth_workspace_bytes(int F, int H, int W);
int pivlfn_smooth_setup(const float *flows, const float *weights, const unsigned char *mask, int F, int H, int W, double s,
                        void *workspace, size_t workspace_bytes, void *stream);
int pivlfn_smooth_pcg(void *workspace, size_t workspace_bytes, int F, int H, int W, double s, double tol, int iters, void *stream);
int pivlfn_smooth_read(const void *workspace, size_t workspace_bytes, int F, int H, int W, double *z, float *z32, unsigned char *filled,
                       double *status, void *stream);

/* ---- ensemble correlation: the window sums of sum-of-correlation PIV (Meinhart, Wereley & Santiago 2000), the displacement read
 * straight from the images and averaged over a sequence.  Added without an ABI bump (additive).  Launches only on `stream`, no
 * allocation, no host synchronisation, capturable into a graph.  One launch; B = 0 returns success without one.
 *
 * a, b: [B,H,W] bytes, any address;  offset: [2,ny,nx] int32, plane 0 ox and plane 1 oy, or NULL for no pre-shift;
 * sums: [ny,nx,P,P,3] int64, sums_a: [ny,nx,2] int64, with P = 2*search + 1.
 * Grid: window (j, i) of a has its top-left pixel at y_j = search + j*step, x_i = search + i*step;
 *   ny = (H - window - 2*search)/step + 1 (integer division), nx likewise from W; both are at least 1.
 *   Window (j, i) of b for displacement (dy, dx), each in -search..search, has its top-left pixel at (y_j + oy + dy, x_i + ox + dx).
 * A window is OUTSIDE when  y_j + oy - search < 0  or  y_j + oy + search + window > H,  or the same in x with ox and W: it adds nothing,
 *   in this call or any other.  Every other window adds, over its window^2 pixels and the B frames, as exact integers:
 *       sums_a[j][i][0..1]                       += sum A, sum A^2
 *       sums[j][i][dy+search][dx+search][0..2]   += sum B, sum B^2, sum A*B
 *   The call ADDS to what sums and sums_a hold (the caller zeroes them once): a plain 64-bit load, add and store by the one lane that
 *   owns the entry, no atomics; the stream orders successive calls.  A per-frame window sum fits 32 bits (255^2 * 128^2 = 1 065 369 600)
 *   and is widened to 64 bits before the frames are added, so a frame adds the same integers alone and inside any batch.
 * Ranges: window a multiple of 4 in 8..128;  search 1..32;  step >= 1;  H*W < 2^31;  B <= 65535.
 * Errors (PIVLFN_ERR_ARG, before any launch): a null a, b, sums or sums_a;  an output that overlaps an input or the other output;  a
 * value out of the ranges above;  H or W smaller than window + 2*search.
 * Launch plan: a lane owns four vertically adjacent displacements of one window, so a window has items = ceil(P / 4) * P of them;
 * ny*nx x ceil(items / T) workgroups of T threads, T = items rounded up to whole waves and kept within 128..512 (one block up to
 * search 21, three at search 32).  Windows of 16, 32 and 64 pixels have a kernel of their own, every other window shares one.  The
 * workgroup stages (window + 6) * window + (window + 2*search) * (window + 2*search rounded up to 4, + 4) bytes: at most 54784, no
 * opt-in. */
int pivlfn_ensemble_corr(const unsigned char *a, const unsigned char *b, const int *offset, long long *sums, long long *sums_a,
                         int B, int H, int W, int window, int step, int search, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIVLFN_H */
