// Shared declarations for the gfx950 kernels of libpivlfn.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include "../../include/pivlfn.h"

namespace pivlfn {

void set_error(const char *fmt, ...);

// Tuning knobs for in-process A/B measurements exist only in the tools build (libpivlfn_tools.so, -DPIVLFN_TOOLS, loaded
// by tools/ alone): 0 = warp_corr variant, 1 = conv variant bits, 2/3/7 = ablation masks, 5/6 = stamp buffer address.
// In the production library every knob is the compile-time constant 0: no process-global mutable state.
#ifdef PIVLFN_TOOLS
extern int g_knob[16];
#define PIV_KNOB(i) (pivlfn::g_knob[i])
#define PIV_DBG(p) ((p).dbg)            // a kernel's ablation mask (timing runs of the tools): a field of its parameter block
#define PIV_SET_DBG(p, v) ((p).dbg = (v))
#else
#define PIV_KNOB(i) 0
#define PIV_DBG(p) 0                    // production: the constant 0 -- no field in the parameter blocks, no test in the kernels
#define PIV_SET_DBG(p, v) ((void)0)
#endif

// Opt-in to > 64 KiB of dynamic LDS for kernel `fn`, once per (call site, device); thread-safe.  `slot` is a zero-initialised
// static at the call site.
struct LdsAttr { int bytes[64]; };
int ensure_dyn_lds(LdsAttr &slot, const void *fn, int bytes);

#define PIV_CHECK_HIP(expr)                                                                  \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            pivlfn::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return PIVLFN_ERR_HIP;                                                           \
        }                                                                                    \
    } while (0)

// say: leave the refusal's message as the last error (false for a choice's speculative attempts, conv_mfma.hip)
#define PIV_REQUIRE_IF(say, cond, ...)                                                       \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            if (say) pivlfn::set_error(__VA_ARGS__);                                         \
            return PIVLFN_ERR_ARG;                                                           \
        }                                                                                    \
    } while (0)
#define PIV_REQUIRE(cond, ...) PIV_REQUIRE_IF(true, cond, __VA_ARGS__)

int device_cus();      // compute units of the current device (cached per device; 256 when the query fails)

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// Blocks b and b+8 share an XCD (round-robin dispatch over the 8 XCDs); give every XCD a contiguous
// run of logical tile ids so neighbouring tiles (shared halos) hit the same L2.  Bijective for any n.
__device__ __forceinline__ int xcd_remap(int bid, int n)
{
    const int q = n >> 3, r = n & 7;
    const int xcd = bid & 7, k = bid >> 3;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + k;
}

__device__ __forceinline__ float lrelu01(float v) { return v >= 0.f ? v : 0.1f * v; }

// Bilinear taps of a back-warp sample at (fx, fy): pixel indices (y*W+x) of the four neighbours, -1 when the
// neighbour lies outside the image (padding_mode='zeros', align_corners=True: src/models.py:32-35).
struct Taps { int o00, o01, o10, o11; float w00, w01, w10, w11; };
__device__ __forceinline__ Taps make_taps(float fx, float fy, int H, int W)
{
    Taps t;
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float ax = fx - x0f, ay = fy - y0f;
    // clamp before the int conversion so wild flows cannot overflow; anything clamped is out of range anyway
    const int x0 = (int)fminf(fmaxf(x0f, -2.f), (float)W);
    const int y0 = (int)fminf(fmaxf(y0f, -2.f), (float)H);
    const bool xa = x0 >= 0 && x0 < W, xb = x0 + 1 >= 0 && x0 + 1 < W;
    const bool ya = y0 >= 0 && y0 < H, yb = y0 + 1 >= 0 && y0 + 1 < H;
    t.o00 = (xa && ya) ? y0 * W + x0 : -1;
    t.o01 = (xb && ya) ? y0 * W + x0 + 1 : -1;
    t.o10 = (xa && yb) ? (y0 + 1) * W + x0 : -1;
    t.o11 = (xb && yb) ? (y0 + 1) * W + x0 + 1 : -1;
    t.w00 = (1.f - ax) * (1.f - ay);
    t.w01 = ax * (1.f - ay);
    t.w10 = (1.f - ax) * ay;
    t.w11 = ax * ay;
    return t;
}

// ---- convolution (conv_mfma.hip, conv_k1.hip, conv_c3k7.hip, conv_s2.hip; conv_direct.h) -----------
struct ConvSeg {
    const float *ptr;   // NHWC base, channel offset already applied
    int cload;          // channels staged from this source, multiple of 4 (zero-weight lanes allowed)
    int stride;         // floats between consecutive pixels
};

struct ConvParams {
    ConvSeg seg[3];
    int nseg;
    const float *wpk;   // [nchunk][KH*KW][2][cout_pad][4]
    const float *bias;  // [cout_pad]
    float *out;         // NHWC, channel offset applied
    int out_stride;     // floats per output pixel
    int cout_store;     // channels written per pixel (>= real Cout; the extra ones are exact zeros)
    int cout_pad;       // multiple of 32, >= cout_store
    const float *res;   // optional residual added before the activation (same pixel grid as out)
    int res_stride;
    int B, H, W;        // input
    int Ho, Wo;         // output
    int KH, KW, S, padY, padX;
    int nchunk;         // K chunks of 8 input channels over all segments (the last one may be a 4-channel tail)
    int tail;           // 1 when the last chunk is a 4-channel tail (last source has cload % 8 == 4)
    int cin_real;       // real input channels of the layer (the weights of padding lanes are zero); 0 = not stated
    int lrelu;
    // split-K for layers with too few tiles to fill the chip (the coarse pyramid levels): gridDim.z workgroups share a tile,
    // each contracts a contiguous range of K chunks into scratch[z][pixel][cout_pad]; conv_splitk_reduce_kernel adds the
    // partial sums in z order (deterministic), then bias / residual / activation.  scratch == nullptr: never split.
    float *scratch;
    size_t scratch_floats;
    int ksplit;         // number of K shares (set by the launcher; 0/1 = no split)
    unsigned long long *stamps;   // tools only: per-workgroup phase times (s_memtime ticks), 8 per workgroup; nullptr in production
#ifdef PIVLFN_TOOLS
    int dbg;            // tools only (-DPIVLFN_STAMPS builds): ablation mask, 1 no MFMAs, 2 no global loads, 4 no epilogue stores
#endif
};

// What launch_conv runs for a call (pivlfn_conv2d_nhwc_plan): kernel family (PIVLFN_CONV_PLAN_*), output rows and channels of a
// workgroup's tile, v2's staging class as 100 * PMAX + WMAX (0 elsewhere), split-K shares.
struct ConvPlan { int family, rows, chans, staging, ksplit; };
// The launcher's decision from the geometry alone (no pointer read, no device call); scratch_floats == 0 stands for "no scratch".
int choose_conv(const ConvParams &p, ConvPlan &pl);
int launch_conv(const ConvParams &p, hipStream_t st);
// NetC.conv1 with the two 1 x 1 layers that read its output at level 1 -- NetC_ext (32 -> 64, both frames) and Regularization's
// moduleFeat (32 -> 128, first frame) -- computed from the activated accumulators in the same kernel (conv_c3k7.hip).
struct Conv1Fuse {
    const float *w11;   // [6 blocks: 2 of NetC_ext, 4 of moduleFeat][4 groups][64 lanes][4]: W[32 blk + (lane & 31)][8 g + 4 (lane >> 5) + e]
    const float *b11;   // [64 + 128]
    float *out_ext;     // [images][H][W][64]
    float *out_feat;    // [first B_feat images][H][W][128]
    int B_feat;
};
int launch_conv1_fused(const ConvParams &p, const Conv1Fuse &f, hipStream_t st);     // -1: the layer / size is not covered
int launch_touch(const float *p, size_t floats, float *sink, hipStream_t st);     // read-only prefetch pass (ops.hip)
int launch_splitk_reduce(const ConvParams &p, int nz, hipStream_t st);     // second pass of a split-K layer (also used by conv_split.hip)

// What launch_conv_h / _x / _w / _wb run for a call (pivlfn_conv2d_nhwc_kernel_plan; the fields are plan[0..9] there): the kernel
// (PIVLFN_KERNEL_PLAN_*) and its template arguments -- piece products per product (split, b3; 0 elsewhere), output rows and channels
// of a workgroup's tile, the staging class as 100 * PM + WM (f16, split; 0 elsewhere), the workgroups per CU it is compiled for --
// then the split-K shares, whether the folded 4-lane tail is used, whether the handle runs the batch image by image (set by the
// entry point's side, conv_layer.hip's conv_call_x; the plan is then one image's), and the workgroups of the launch.
struct ConvKernelPlan { int kernel, terms, rows, chans, staging, occ, ksplit, fold, per_image, blocks; };
// Each of those launchers is a choice and a launch.  The choice (choose_conv_*) reads the geometry alone -- no pointer is followed,
// no device is touched -- and names the instantiation by its launch function and its plan in one statement; launch_conv_* makes the
// choice and launches what it named.  What the choice cannot see of the caller's pointers it is told: has_scratch, has_wtail.
template <class P>
struct ConvChoice {
    int (*run)(const P &, hipStream_t);
    ConvKernelPlan pl;
};
// L = one instantiation's launcher: L::plan holds its own bounds and its grid, L::run launches it (C: also conv_direct.h's ConvChoiceD)
template <class L, class P, class C, class... A>
static inline int conv_take(const P &p, C &ch, A... more)
{
    ch.run = &L::run;
    return L::plan(p, ch.pl, more...);
}

// ---- fp16-multiplicand variant (conv_f16.hip): optional reduced-precision mode, K chunks of 16 channels ----------------
struct ConvSegH {
    const void *ptr;    // NHWC base (fp32 or fp16 elements), channel offset already applied
    int cload;          // channels staged from this source: multiple of 4 (fp32) or 8 (fp16); zero-weight lanes allowed
    int stride;         // elements between consecutive pixels
    int f16;            // element type of this source: 0 = fp32 (converted while staging), 1 = fp16
};
struct ConvParamsH {
    ConvSegH seg[3];
    int nseg;
    const void *wpk;    // fp16 [nchunk][KH*KW][2][cout_pad][8]
    const float *bias;  // [cout_pad]
    void *out;          // NHWC fp32 or fp16
    int out_stride, cout_store, cout_pad, out_f16;
    int B, H, W, Ho, Wo;
    int KH, KW, S, padY, padX;
    int nchunk, lrelu;
#ifdef PIVLFN_TOOLS
    int dbg;            // ablation mask for tools/bench_ops.py (0 in production): 1 no MFMAs, 2 no global loads, 4 no LDS commit
#endif
    unsigned long long *stamps;   // tools only: per-workgroup phase times (s_memtime ticks), 8 per workgroup; nullptr in production
};
int choose_conv_h(const ConvParamsH &p, ConvChoice<ConvParamsH> &ch);
int launch_conv_h(const ConvParamsH &p, hipStream_t st);
// ---- fp32 by exact fp16 operand splitting (conv_split.hip): fp32 sources and output, K chunks of 16 channels ------------
struct ConvParamsX {
    ConvSeg seg[3];
    int nseg;
    const void *wpk;    // fp16 pieces [nchunk][KH*KW][3][2][cout_pad][8]
    const void *wtail;  // 3 x 3 layers whose staged channels end in a 4-lane tail: that chunk with taps folded into K,
                        // [step 3][piece 2][k-half 2][cout_pad][8 = 2 taps x 4 channels]; nullptr otherwise (conv_split_big_kernel)
    int tail;           // set by the launcher: the kernel uses wtail for the last chunk
    const float *bias;  // [cout_pad]
    float *out;         // NHWC fp32
    int out_stride, cout_store, cout_pad;
    float out_scale;    // 2^-k: undoes the power-of-two scale of the packed weights
    int terms;          // partial products per product: 6 (exact to 2^-32) or 3 (h.h, h.m, m.h: 2^-21)
    float *scratch;     // split-K scratch [z][pixel][cout_pad] (nullptr: never split); the policy is in launch_conv_x
    size_t scratch_floats;
    int ksplit;         // set by the launcher
    int B, H, W, Ho, Wo;
    int KH, KW, S, padY, padX;
    int nchunk, lrelu;
#ifdef PIVLFN_TOOLS
    int dbg;            // ablation mask for tools/bench_ops.py (0 in production): 1 no MFMAs, 2 no global loads, 4 no LDS commit
#endif
};
// ch.pl.terms / .ksplit / .fold: what launch_conv_x sets in the parameter block (terms only differ from p.terms under a tools knob)
int choose_conv_x(const ConvParamsX &p, bool has_scratch, bool has_wtail, ConvChoice<ConvParamsX> &ch);
int launch_conv_x(const ConvParamsX &p, hipStream_t st);
bool conv_split_supports(int KH, int KW, int S, int cout_pad, int terms);
// ---- 3x3 stride-1 layers by Winograd F(2x2, 3x3) on the fp32 matrix cores (conv_wino.hip): fp32 everywhere, K chunks of 8 channels ----
struct ConvParamsW {
    ConvSeg seg[3];
    int nseg;
    const float *wpk;   // Winograd-domain weights, [nchunk][cout_pad/32][4][4][64][4] (pack_conv_w)
    const float *bias;  // [cout_pad]
    float *out;         // NHWC fp32, channel offset applied
    int out_stride, cout_store, cout_pad;
    int B, H, W;        // output grid = input grid (3x3, stride 1, pad 1)
    int nchunk, lrelu;
    unsigned long long *stamps;   // tools build (-DPIVLFN_STAMPS) only: per-workgroup phase times of wave 0 (s_memtime ticks), 8 per workgroup; nullptr in production
#ifdef PIVLFN_TOOLS
    int dbg;            // tools build only: ablation mask of conv_wino_ws.hip (timing runs, wrong results)
#endif
    const void *wpk_b;  // conv_wino_b3.hip: the same U split into three bf16 pieces, [nchunk][cout_pad/64][4][4][2][3][64][8] (pack_conv_wb); nchunk = K steps of 16 channels
    int terms;          // conv_wino_b3.hip: piece products per product, 6 (default), 8 or 9
};
int choose_conv_w(const ConvParamsW &p, ConvChoice<ConvParamsW> &ch);
// conv_wino_b3.hip's grid is sized by the device: its choice takes the CU count, its launch the workgroups the choice planned
struct ConvChoiceB3 {
    int (*run)(const ConvParamsW &, int blocks, hipStream_t);
    ConvKernelPlan pl;
};
int choose_conv_wb(const ConvParamsW &p, int cus, ConvChoiceB3 &ch);
int launch_conv_w(const ConvParamsW &p, hipStream_t st);
int launch_conv_wb(const ConvParamsW &p, hipStream_t st);      // the same layers with exactly split operands on the bf16 matrix cores (conv_wino_b3.hip)
int launch_conv_wb(const ConvParamsW &p, int cus, hipStream_t st);      // ... on at most `cus` compute units (0 = the device's): the same bits on any grid
bool conv_wino_b3_supports(int cout_pad);
int launch_conv_w_ws(const ConvParamsW &p, hipStream_t st);   // the same layers on persistent workgroups with producer / consumer waves (conv_wino_ws.hip); bit-identical
long conv_wino_ws_items(const ConvParamsW &p);                // work items such a launch would have (0: not covered)
int launch_conv_w4(const ConvParamsW &p, hipStream_t st);      // F(4x4, 3x3): wpk = [nchunk][cout_pad/32][6][6][64][4] (pack_conv_w4)
bool conv_wino_supports(int KH, int KW, int S, int padY, int padX);
// 32 -> 2 channel k x k flow head on the VALU (conv_head.hip); w = [k*k][8][2][4] on the device
// (7 x 1) convolution from 32 channels to up to 64 on v_mfma_f32_16x16x4_f32, operands from global memory (conv_head.hip)
int launch_conv_col7(const float *x, int x_stride, const float *wf, const float *bias, float *out, int out_stride, int cout_store,
                     int single48, int B, int H, int W, hipStream_t st);
// (1 x 7) convolution 49 -> 49 channels (52 stored lanes), the same way along x (conv_head.hip)
int launch_conv_row7(const float *x, int x_stride, const float *wf, const float *wf12, const float *bias, float *out, int out_stride,
                     int B, int H, int W, hipStream_t st);
int check_conv_col7(int x_stride, int out_stride, int cout_store, int single48, int B, int H, int W);   // their argument checks,
int check_conv_row7(int x_stride, int out_stride, int B, int H, int W);                                  // pointers apart
// The two 49-channel distance layers with exactly split operands on v_mfma_f32_16x16x32_bf16 (conv_dist_b3.hip): row = 0 the (7 x 1)
// 49 <- 32 layer, 1 the (1 x 7) 49 <- 49 one; wb = pack_conv_dist_b3's fragments, wf / wf12 = the fp32 kernels' (output channel 48 stays
// an fp32 fmaf chain); terms = 6, 8 or 9 piece products per product; any H, W >= 1
int launch_conv_dist_b3(int row, const float *x, int x_stride, const void *wb, const float *wf, const float *wf12, const float *bias,
                        float *out, int out_stride, int terms, int B, int H, int W, hipStream_t st);
int check_conv_dist_b3(int row, int x_stride, int out_stride, int terms, int B, int H, int W);           // its argument checks, pointers apart
long conv_dist_b3_tiles(int row, int B, int H, int W);      // tiles of a call (a workgroup walks four) and the workgroups per CU the
int conv_dist_b3_occupancy(int row);                        // kernel is compiled for
int launch_conv_head(const float *x, const float *w, float b0, float b1, const float *res4, float *out4, int B, int H, int W,
                     int k, hipStream_t st);
// What launch_conv_head runs for a call (pivlfn_conv_head_nhwc_plan): kernel family (PIVLFN_HEAD_PLAN_*), output rows and columns of a
// workgroup's tile, workgroups of the launch.  The launcher's decision from the geometry alone; exclude = 0: the shipped policy.
struct HeadPlan { int family, rows, cols, blocks; };
int choose_conv_head(int k, int B, int H, int W, unsigned exclude, HeadPlan &pl);

// ---- warp + correlation (warp_corr.hip) ------------------------------------------------------------
int launch_warp_corr(const float *f1, const float *f2, const float *flow, float flow_scale, float *out,
                     int B, int C, int H, int W, int stride, int leaky, bool nhwc, hipStream_t st);
void warp_corr_time_next(hipEvent_t start, hipEvent_t stop);   // attach start/stop events to the next channels-last launch
int launch_backwarp_nchw(const float *in, const float *flow, float *out, int B, int C, int H, int W, hipStream_t st);
int launch_corr_bwd(const float *first, const float *second, const float *gout, float *gfirst, float *gsecond,
                    int B, int C, int H, int W, int s, hipStream_t st);
int corr_bwd_cgroup(int B, int C, int H, int W, int s);        // channels per workgroup of that launch (16, 8 or 4)

// ---- small ops (ops.hip); NHWC unless noted ----------------------------------------------------------
int launch_prep_images(const float *img1, const float *img2, float *out, int B, int H, int W,
                       const float mean[6], hipStream_t st);                       // NCHW x2 -> [2B,H,W,4]
int launch_resize_nhwc4(const float *in, float *out, int N, int H, int W, int Ho, int Wo, hipStream_t st);
int launch_resize_nchw(const float *in, float *out, int B, int C, int H, int W, int Ho, int Wo,
                       float m0, float m1, int use_mul, hipStream_t st);
int launch_dwconvT(const float *in, const float *w, float *out, int B, int H, int W, int C, int stride_in,
                   int stride_out, int cstore, hipStream_t st);                    // k4 s2 p1 depthwise
int launch_backwarp_nhwc(const float *in, const float *flow4, float scale, float *out, int B, int H, int W,
                         int C, hipStream_t st);
int launch_flow_mean(const float *flow4, float *partial, float *mean, int B, int HW, hipStream_t st);
int launch_reg_prep(const float *img1, const float *img2, const float *flow4, float *mean, const float *partial, float scale,
                    float *misc4, int B, int H, int W, hipStream_t st);
// conv_R.0's three flow-dependent channels + bias + the precomputed partial sum of its feature channels + LeakyReLU (ops.hip)
bool reg_r0_tail_supports(int B, int H, int W);
int launch_reg_r0_tail(const float *misc4, const float *w, const float *bias, const float *part, float *out, int B, int H, int W,
                       hipStream_t st);
int launch_reg_tail(const float *dist, int dstride, const float *flow4, const float *wx, const float *wy,
                    float bx, float by, int k, float *out4, float *out_nchw, float out_scale,
                    int B, int H, int W, hipStream_t st);
int launch_flow4_to_nchw(const float *flow4, float *out, int B, int H, int W, hipStream_t st);

// ---- stereo 2D3C reconstruction (stereo.hip): [2B,2,h,w] NCHW interleaved cameras -> [B,H,W,3] ------------------------
int launch_stereo_2d3c(const float *flow, float *out, int B, int h, int w, int H, int W, const float *mul,
                       const float *coeff, const float *scale, const double *tan4, hipStream_t st);
int flow_mean_partials(int HW);

// ---- derived fields and streaming statistics (postpro.hip): [B,2,H,W] NCHW flows ----------------------------------------------
int launch_flow_fields(const float *flow, void *out, int B, int H, int W, double calib, int kind, int out_f64, hipStream_t st);
int launch_flow_stats(const float *flow, double *acc, int B, int H, int W, double calib, hipStream_t st);
int launch_flow_stats_masked(const float *flow, const unsigned char *flag, double *acc, double *cnt, int B, int H, int W, double calib,
                             hipStream_t st);

// ---- vector validation (validate.hip): normalized median test on [B,2,H,W] NCHW flows, flag [B,H,W] bytes ------------------------
int launch_flow_validate(const float *flow, float *out, unsigned char *flag, float *resid, int B, int H, int W, int radius,
                         int spacing, float eps, float thresh, int mode, hipStream_t st);

// ---- scoring against a known field (evaluate.hip): [B,2,h,w] NCHW flows, [B,2,H,W] truth, mask [B,H,W] bytes or nullptr ------------
size_t flow_errors_workspace_bytes(int B, int H, int W);
int launch_flow_errors(const float *flow, const float *truth, const unsigned char *mask, int B, int H, int W, int k, double div_flow,
                       double *sums, float *err_map, void *ws, size_t ws_bytes, hipStream_t st);
int launch_level_errors(const float *levels, int lowest_level, const float *truth, const unsigned char *mask, int B, int H, int W,
                        double div_flow, double *sums, void *ws, size_t ws_bytes, hipStream_t st);
int launch_error_stats(const float *flow, const float *truth, const unsigned char *mask, double *acc, int B, int H, int W, hipStream_t st);

// ---- pictures (viz.hip): [B,2,H,W] NCHW flows or [B,H,W] fields -> packed bytes [B,H,W,3]; mask [B,H,W] bytes or nullptr ------------
int launch_flow_maxrad(const float *flow, const unsigned char *mask, float *maxrad, int B, int H, int W, hipStream_t st);
int launch_flow_to_color(const float *flow, const float *norm, const unsigned char *mask, unsigned char *out, int B, int H, int W,
                         int wheel, int order, hipStream_t st);
int launch_field_absmax(const void *field, int is_f64, const unsigned char *mask, double *absmax, int B, int H, int W, hipStream_t st);
int launch_scalar_to_color(const void *field, int is_f64, const unsigned char *mask, const unsigned char *lut, unsigned char *out, int B,
                           int H, int W, double vmin, double vmax, int bad_rgb, hipStream_t st);
int launch_flow_decimate(const float *flow, const unsigned char *mask, float *mean, int *count, int B, int H, int W, int cell,
                         hipStream_t st);

// ---- match quality (quality.hip): windowed correlation of img1 with img2 warped by the flow, and the sub-pixel residual of its peak ----
size_t match_quality_workspace_bytes(int B, int H, int W, int radius);
int launch_match_quality(const float *img1, const float *img2, int C, const float *flow, const unsigned char *mask, float *quality,
                         unsigned char *flag, int B, int H, int W, int radius, int min_count, double floor, void *ws, size_t ws_bytes,
                         hipStream_t st);

// the warp kernel of match_quality alone: a, b [B,H,W] fp64 and the byte of m (bit 0) and k (bit 1); arguments checked by the caller
int launch_quality_warp(const float *img1, const float *img2, int C, const float *flow, const unsigned char *mask, double *wa, double *wb,
                        unsigned char *wf, int B, int H, int W, hipStream_t st);

// ---- flow uncertainty (uncertainty.hip): per-vector uncertainty from correlation statistics, and its per-pixel sums over a sequence ----
size_t flow_uncertainty_workspace_bytes(int B, int H, int W, int radius, int lag);
int launch_flow_uncertainty(const float *img1, const float *img2, int C, const float *flow, const unsigned char *mask, float *unc,
                            unsigned char *flag, int B, int H, int W, int radius, int lag, int min_count, double floor, void *ws,
                            size_t ws_bytes, hipStream_t st);
int launch_uncertainty_accumulate(const float *unc, const unsigned char *flag, double *sums, int B, int H, int W, hipStream_t st);

// ---- vortex identification (vortex.hip): Gamma1 and Gamma2 of a flow over the (2r+1)^2 neighbours at spacing s -----------------------
size_t vortex_gamma_workspace_bytes(int B, int H, int W, int radius, int spacing);
int launch_vortex_gamma(const float *flow, const unsigned char *mask, float *gamma, unsigned char *flag, int B, int H, int W, int radius,
                        int spacing, int min_count, void *ws, size_t ws_bytes, hipStream_t st);

// ---- Lagrangian flow maps (flowmap.hip): particles through consecutive displacement fields, the stretching of the map they trace ------
int launch_flowmap_advect(const float *flows, const unsigned char *mask, int B, int H, int W, double *pos, unsigned char *flag, int N,
                          int backward, int iters, double *trace, hipStream_t st);
int launch_flowmap_seed(double *pos, unsigned char *flag, int h, int w, int spacing, hipStream_t st);
int launch_flowmap_ftle(const double *pos, const unsigned char *flag, int h, int w, int spacing, double *stretch, unsigned char *oflag,
                        hipStream_t st);

// ---- synthetic PIV pairs (particles.hip): particles through one displacement field, particle images as ordered sums of Gaussian blobs --
int launch_particles_displace(const double *pos, const float *flow, const unsigned char *mask, int H, int W, int N, int method,
                              unsigned char *flag, double *out, hipStream_t st);
size_t particles_render_workspace_bytes(int B, int N, int H, int W, int radius);
int launch_particles_render(const double *pos, const float *diam, const float *amp, const unsigned char *flag, int B, int N, int H, int W,
                            int radius, float *intensity, unsigned char *image, void *workspace, size_t workspace_bytes, hipStream_t st);

// ---- snapshot POD (pod.hip): fp64 Gram matrix of n fp32 snapshots on the fp64 matrix instruction, fp64 weighted sums of snapshots -----
size_t snapshot_gram_workspace_bytes(int n, long P);
int launch_snapshot_gram(const float *X, int n, long P, long ldx, double *G, void *ws, size_t ws_bytes, hipStream_t st);
int launch_snapshot_project(const float *X, int n, long P, long ldx, const double *Wt, int K, double *out, hipStream_t st);

// ---- two-point statistics (twopoint.hip): per-row sums of pair terms at separations along x and y, accumulated over a sequence ----------
int launch_twopoint_accumulate(const float *flow, const unsigned char *mask, const double *mean, double *acc, int B, int H, int W,
                               int max_sep, int step, hipStream_t st);

// ---- velocity distributions (distribution.hip): per-pixel sums up to the fourth order with the quadrant split; pooled histograms ---------
// What launch_flow_hist runs for a call (pivlfn_flow_hist_plan): the launcher's decision from the sizes alone.
struct HistPlan { int groups, lds_words, joint_in_lds; size_t words; int moment_blocks; };
int choose_flow_hist(int B, int H, int W, int nbins, int jbins, int fbins, HistPlan &pl);
int launch_flow_moments(const float *flow, const unsigned char *mask, const double *mean, const double *thr, double *acc, int B, int H,
                        int W, hipStream_t st);
int launch_flow_hist(const float *flow, const unsigned char *mask, const double *mean, const double *scale, unsigned long long *hist,
                     int B, int H, int W, double lo, double hi, int nbins, int jbins, int fbins, hipStream_t st);

// ---- temporal spectra (spectrum.hip): one Welch segment of every vector's time series projected on K basis pairs, quadratic forms summed --
int launch_spectrum_accumulate(const float *X, int L, int first, long N, long ldx, const double *basis, int K, double *acc, int *count,
                               hipStream_t st);

// ---- pressure from PIV (pressure.hip): material acceleration of three consecutive flows, least-squares integration by Jacobi-CG ----------
int launch_pressure_gradient(const float *flows, int B, int h, int w, double s, double nu, double *g, unsigned char *valid, hipStream_t st);
size_t pressure_workspace_bytes(int F, int h, int w);
size_t pressure_workspace_offset(int F, int h, int w, int what);
int launch_pressure_setup(const double *g, const unsigned char *valid, int F, int h, int w, double s, void *ws, size_t ws_bytes, hipStream_t st);
int launch_pressure_cg(void *ws, size_t ws_bytes, int F, int h, int w, double tol, int iters, hipStream_t st);
int launch_pressure_read(const void *ws, size_t ws_bytes, int F, int h, int w, double *p, unsigned char *flag, double *status, hipStream_t st);

// ---- smoothing and gap filling (smooth.hip): the fp64 2-D DCT on the matrix cores, penalised least squares by DCT-preconditioned CG ------
size_t dct2_workspace_bytes(int P, int H, int W);
int launch_dct2(const double *x, double *out, int P, int H, int W, int inverse, void *ws, size_t ws_bytes, hipStream_t st);
size_t smooth_workspace_bytes(int F, int H, int W);
int launch_smooth_setup(const float *flows, const float *weights, const unsigned char *mask, int F, int H, int W, double s, void *ws,
                        size_t ws_bytes, hipStream_t st);
int launch_smooth_pcg(void *ws, size_t ws_bytes, int F, int H, int W, double s, double tol, int iters, hipStream_t st);
int launch_smooth_read(const void *ws, size_t ws_bytes, int F, int H, int W, double *z, float *z32, unsigned char *filled, double *status,
                       hipStream_t st);

// ---- stereo calibration (calibrate.hip): template matching, marker centres of the correlation map, image dewarp -------------------------
size_t template_match_workspace_bytes(int th, int tw);
int launch_template_match(const unsigned char *images, const unsigned char *templ, float *r, int B, int H, int W, int th, int tw,
                          void *ws, size_t ws_bytes, hipStream_t st);
size_t target_points_workspace_bytes(int B, int H, int W);
int launch_target_points(const float *r, int B, int H, int W, float threshold, int cap, int *labels, int *count, long long *rec,
                         void *ws, size_t ws_bytes, hipStream_t st);
int launch_dewarp_frames(const void *frames, void *out, int is_f32, int B, int H, int W, const double *A, double x0, double y0, int mode,
                         double fill, hipStream_t st);

// ---- ensemble correlation (ensemble.hip): the integer window sums of sum-of-correlation PIV, added over frames and calls -----------------
int launch_ensemble_corr(const unsigned char *a, const unsigned char *b, const int *offset, long long *sums, long long *sums_a, int B,
                         int H, int W, int window, int step, int search, hipStream_t st);

// ---- image pre-processing (preproc.hip): [n,H,W,3] uint8 frames -> background minimum [H,W,3], network input [n,3,H,W] fp32 --------
int launch_frames_background_min(const unsigned char *frames, unsigned char *bg, int n, int H, int W, hipStream_t st);
int launch_frames_preprocess(const unsigned char *frames, const unsigned char *bg, float *out, int n, int H, int W, int k, int floor,
                             hipStream_t st);

}  // namespace pivlfn
