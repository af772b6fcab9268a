// One convolution layer call: the parameter block of every kernel family from a packed layer (ConvW) and a call description
// (ConvCall), the network's per-layer kernel choice and launch (conv), and the stand-alone layer handles behind the pivlfn_conv*
// entry points, which run one chosen family each with their own argument checks.
#include <algorithm>
#include <vector>
#include "net.h"

namespace pivlfn {

// ---- parameter blocks: each is filled here and nowhere else; the split-K scratch is the caller's to add ----------------------------
static inline void out_grid(const ConvW &cw, const ConvCall &c, int &Ho, int &Wo)
{
    Ho = (c.H + 2 * c.padY - cw.KH) / c.S + 1;
    Wo = (c.W + 2 * c.padX - cw.KW) / c.S + 1;
}

ConvParams conv_params(const ConvW &cw, const ConvCall &c)
{
    ConvParams p;
    memset(&p, 0, sizeof(p));
    for (int i = 0; i < c.nsrc; ++i) p.seg[i] = c.src[i];
    p.nseg = c.nsrc;
    p.wpk = cw.wpk; p.bias = cw.bias; p.out = c.out; p.out_stride = c.out_stride; p.cout_store = c.cout_store;
    p.cout_pad = cw.cout_pad; p.res = c.res; p.res_stride = c.res_stride;
    p.B = c.B; p.H = c.H; p.W = c.W;
    p.KH = cw.KH; p.KW = cw.KW; p.S = c.S; p.padY = c.padY; p.padX = c.padX;
    out_grid(cw, c, p.Ho, p.Wo);
    p.nchunk = cw.nchunk; p.tail = cw.tail; p.lrelu = c.lrelu; p.cin_real = cw.cin;
    return p;
}

static ConvParamsH conv_params_h(const ConvW &cw, const ConvCall &c)
{
    ConvParamsH q;
    memset(&q, 0, sizeof(q));
    for (int i = 0; i < c.nsrc; ++i) q.seg[i] = ConvSegH{c.src[i].ptr, c.src[i].cload, c.src[i].stride, (c.in16 >> i) & 1};
    q.nseg = c.nsrc;
    q.wpk = cw.wpk_h; q.bias = cw.bias; q.out = c.out; q.out_stride = c.out_stride; q.cout_store = c.cout_store;
    q.cout_pad = cw.cout_pad; q.out_f16 = c.out16;
    q.B = c.B; q.H = c.H; q.W = c.W;
    q.KH = cw.KH; q.KW = cw.KW; q.S = c.S; q.padY = c.padY; q.padX = c.padX;
    out_grid(cw, c, q.Ho, q.Wo);
    q.nchunk = cw.nchunk_h; q.lrelu = c.lrelu;
    return q;
}

static ConvParamsX conv_params_x(const ConvW &cw, const ConvCall &c, int terms)
{
    ConvParamsX q;
    memset(&q, 0, sizeof(q));
    for (int i = 0; i < c.nsrc; ++i) q.seg[i] = c.src[i];
    q.nseg = c.nsrc;
    q.wpk = cw.wpk_x; q.wtail = cw.wtail_x; q.bias = cw.bias; q.out = c.out; q.out_stride = c.out_stride; q.cout_store = c.cout_store;
    q.cout_pad = cw.cout_pad; q.out_scale = cw.scale_x; q.terms = terms;
    q.B = c.B; q.H = c.H; q.W = c.W;
    q.KH = cw.KH; q.KW = cw.KW; q.S = c.S; q.padY = c.padY; q.padX = c.padX;
    out_grid(cw, c, q.Ho, q.Wo);
    q.nchunk = cw.nchunk_x; q.lrelu = c.lrelu;
    return q;
}

// The three Winograd packings of a 3 x 3 layer: F(2x2) on the fp32 instruction, F(4x4) (tools build), F(2x2) in three bf16 pieces
enum WinoPack { WINO_F2, WINO_F4, WINO_B3 };
static ConvParamsW conv_params_w(const ConvW &cw, const ConvCall &c, WinoPack pack, int terms = 0)
{
    ConvParamsW q;
    memset(&q, 0, sizeof(q));
    for (int i = 0; i < c.nsrc; ++i) q.seg[i] = c.src[i];
    q.nseg = c.nsrc;
    if (pack == WINO_B3) { q.wpk_b = cw.wpk_wb; q.nchunk = cw.nstep_wb; q.terms = terms; }
    else if (pack == WINO_F4) { q.wpk = cw.wpk_w4; q.nchunk = cw.nchunk_w4; }
    else { q.wpk = cw.wpk_w; q.nchunk = cw.nchunk_w; }
    q.bias = cw.bias; q.out = c.out; q.out_stride = c.out_stride; q.cout_store = c.cout_store;
    q.cout_pad = cw.cout_pad;
    q.B = c.B; q.H = c.H; q.W = c.W; q.lrelu = c.lrelu;
    return q;
}

// ---- the streaming kernels' calls: one statement each, for the network's choice and for pivlfn_conv2d_nhwc (and its _plan) ---------
// The call's side only: the layer must carry the packing (wpk_c / wpk_r, made where packs_col7 / packs_row7 hold: that fixes KH, KW,
// the channel counts and cout_pad <= 64), and the tools knob that turns the kernels off is tested where they are chosen.
// The (7 x 1) distance convolution on >= 256 x 256 images (output grid = input grid at this geometry)
static bool calls_col7(const ConvCall &c)
{
    return !c.res && !c.lrelu && c.S == 1 && c.padY == 3 && c.padX == 0 && c.nsrc == 1 && c.src[0].cload == 32 &&
           (long)c.H * c.W >= 256 * 256 && c.cout_store % 4 == 0 && (long)c.H * c.W * std::max(c.src[0].stride, c.out_stride) * 4 < (1L << 31);
}
// The (1 x 7) 49 -> 49 one: 52 staged and 52 stored lanes
static bool calls_row7(const ConvCall &c)
{
    return !c.res && !c.lrelu && c.S == 1 && c.padY == 0 && c.padX == 3 && c.nsrc == 1 && c.src[0].cload == 52 && c.src[0].stride >= 52 &&
           c.out_stride >= 52 && c.cout_store == 52 && (long)c.H * c.W >= 256 * 256 &&
           (long)c.H * c.W * std::max(c.src[0].stride, c.out_stride) * 4 < (1L << 31);
}

// ---- the network's per-layer kernel choice ----------------------------------------------------------------------------------------
enum ConvFamily {
    CONV_DIRECT, CONV_F16, CONV_SPLIT, CONV_COL7_B3, CONV_ROW7_B3, CONV_COL7, CONV_ROW7, CONV_WINO, CONV_WINO_B3,
#ifdef PIVLFN_TOOLS
    CONV_WINO4,
#endif
};

// Which family runs a call: from the mode, the layer's packings and the call's geometry, no pointer into device memory is followed
static ConvFamily conv_family(const ConvCtx &ctx, const ConvW &cw, const ConvCall &c)
{
    int Ho, Wo;
    out_grid(cw, c, Ho, Wo);
    // fp16 mode: every residual-free conv whose output grid is at least 64x64 (smaller levels are launch-latency-bound and
    // stay on the fp32 kernel); activations stay fp32 in HBM, operands are rounded to fp16 while they are staged.
    if (ctx.precision == 1 && !c.res && (long)Ho * Wo >= 64 * 64) return CONV_F16;
    // split modes: every residual-free conv the split kernel covers, with an output grid of at least 64x64 per image (the three-term
    // kernel has 4-row tiles and split-K for the small grids; below 64x64 the layers are a dependent chain of ~12 us launches on
    // either kernel).  The six-term kernel has neither and keeps the 256x256 bound.  Per image: the choice never depends on the
    // batch (tools/split_threshold.py: 1024^2, 512^2 and 256^2 inputs).
    if ((ctx.precision == 2 || ctx.precision == 3) && !c.res && cw.wpk_x && conv_split_supports(cw.KH, cw.KW, c.S, cw.cout_pad, ctx.precision == 3 ? 3 : 6) &&
        (long)Ho * Wo >= (PIV_KNOB(11) ? PIV_KNOB(11) : (ctx.precision == 3 ? 64 * 64 : 256 * 256)))
        return CONV_SPLIT;
    // Default fp32 mode: the two 49-channel distance convolutions of levels 1 and 2 with every operand split exactly into three bf16
    // pieces on the 16-bit matrix cores (conv_dist_b3.hip: the streaming kernels' structure, six piece products per product; error
    // against float64 below the fp32 instruction's: tests/test_gpu_dist_b3.py) -- 1.15-1.5 x the speed of the kernels below at 256^2 ...
    // 1024^2, so the same per-image bound.  PIVLFN_PRECISION_F32_WINO_MFMA32 keeps the fp32 instruction; tools knob bit 2^30 as well.
    if (ctx.precision == 0 && !ctx.no_b3 && !(PIV_KNOB(1) & 1073741824)) {
        if (cw.wpk_cb && cw.wpk_c && calls_col7(c) && c.cout_store == 52 && c.out_stride >= 52) return CONV_COL7_B3;
        if (cw.wpk_rb && cw.wpk_r && calls_row7(c)) return CONV_ROW7_B3;
    }
    // fp32 mode: the (7 x 1) distance convolution of levels 1 and 2 on its streaming matrix-core kernel (per image: >= 256 x 256)
    if (ctx.precision == 0 && cw.wpk_c && calls_col7(c)) return CONV_COL7;
    if (ctx.precision == 0 && cw.wpk_r && calls_row7(c) && !(PIV_KNOB(1) & 65536)) return CONV_ROW7;
    // fp32 mode: the 3 x 3 / stride 1 layers by Winograd F(2x2, 3x3) on the fp32 matrix instruction (conv_wino.hip) from a
    // 64 x 64 grid per image up (a 32 x 32 grid is 32 workgroups with the whole K loop each: the split-K direct kernel is faster);
    // the bound is per image, never a function of the batch
    if (ctx.precision == 0 && !c.res && cw.wpk_w && conv_wino_supports(cw.KH, cw.KW, c.S, c.padY, c.padX) &&
        (long)Ho * Wo >= (PIV_KNOB(12) ? PIV_KNOB(12) : 64 * 64) && c.cout_store % 4 == 0) {
        int cl = 0;
        for (int i = 0; i < c.nsrc; ++i) cl += c.src[i].cload;
        // Default fp32 mode: layers with whole 64-channel output groups and at least 48 staged input channels run the same Winograd
        // algorithm with every operand split exactly into three bf16 pieces on the 16-bit matrix cores (conv_wino_b3.hip; all 24
        // significand bits, error against float64 at or below the fp32 instruction's: tests/test_gpu_wino_b3.py) -- 1.08-1.3 x the
        // speed of the fp32-instruction kernel on those layers at 256^2 ... 1024^2 (conv_M.0's 49 channels, four K steps: 1.08-1.16);
        // 32-channel inputs (two steps per tile: the tile's fixed cost decides, 1.0 x) and the 32- and 96-channel outputs stay on
        // conv_wino.hip.  Per layer shape, never per batch.  PIVLFN_PRECISION_F32_WINO_MFMA32 keeps
        // every layer on the fp32 instruction.
        // From 256 x 256 outputs per image: its persistent workgroups (one per CU, 16 x 16 pixels x 64 channels per tile) need at least a
        // tile per CU; the 128 x 128 layers of level 4 took 23-64 us on it against 12-25 us on conv_wino.hip.
        if (!ctx.no_b3 && cw.wpk_wb && conv_wino_b3_supports(cw.cout_pad) && cl >= 48 && (long)Ho * Wo >= 256 * 256 && !(PIV_KNOB(1) & 2097152) &&
            (long)16 * c.W * c.out_stride * 4 < (1L << 31))
            return CONV_WINO_B3;
        // F(4x4, 3x3) is not used by pivlfn_forward: 1.78x fewer matrix instructions, but its 6x6 transforms, 106 KB of LDS (one
        // workgroup per CU) and lockstep of 12 waves leave it at 0.98x of F(2x2) on 128->128 and 0.68x on 32->32 at 1024 x 1024
        // (DESIGN.md 4.2c).  The tools build can switch it in from knob 13 output pixels per image up, for A/B runs of the forward.
#ifdef PIVLFN_TOOLS
        if (cw.wpk_w4 && PIV_KNOB(13) > 0 && (long)Ho * Wo >= PIV_KNOB(13)) return CONV_WINO4;
#endif
        return CONV_WINO;
    }
    return CONV_DIRECT;
}

int conv(const ConvCtx &ctx, const ConvW &cw, const ConvCall &c, hipStream_t st)
{
    const ConvFamily fam = conv_family(ctx, cw, c);
    if (fam != CONV_F16) PIV_REQUIRE(!c.in16 && !c.out16, "internal: fp16 activations routed to the fp32 conv kernel");
    float *const scratch = (ctx.side && st == ctx.side) ? nullptr : ctx.scratch;      // one scratch area: the side stream never splits
    switch (fam) {
        case CONV_F16: return launch_conv_h(conv_params_h(cw, c), st);
        case CONV_SPLIT: {
            ConvParamsX q = conv_params_x(cw, c, ctx.precision == 3 ? 3 : 6);
            q.scratch = scratch;
            q.scratch_floats = KSPLIT_FLOATS * c.B;
            return launch_conv_x(q, st);
        }
        case CONV_COL7_B3:
            return launch_conv_dist_b3(0, c.src[0].ptr, c.src[0].stride, cw.wpk_cb, cw.wpk_c, nullptr, cw.bias, c.out, c.out_stride, 6, c.B, c.H, c.W, st);
        case CONV_ROW7_B3:
            return launch_conv_dist_b3(1, c.src[0].ptr, c.src[0].stride, cw.wpk_rb, cw.wpk_r, cw.wpk_r12, cw.bias, c.out, c.out_stride, 6, c.B, c.H, c.W, st);
        case CONV_COL7:
            return launch_conv_col7(c.src[0].ptr, c.src[0].stride, cw.wpk_c, cw.bias, c.out, c.out_stride, c.cout_store, cw.cout == 49, c.B, c.H, c.W, st);
        case CONV_ROW7: return launch_conv_row7(c.src[0].ptr, c.src[0].stride, cw.wpk_r, cw.wpk_r12, cw.bias, c.out, c.out_stride, c.B, c.H, c.W, st);
        // persistent workgroups: on the side stream they leave the CUs free that the main stream's small kernels need meanwhile
        case CONV_WINO_B3: return launch_conv_wb(conv_params_w(cw, c, WINO_B3, 6), (ctx.side && st == ctx.side) ? ctx.side_cus : 0, st);
#ifdef PIVLFN_TOOLS
        case CONV_WINO4: return launch_conv_w4(conv_params_w(cw, c, WINO_F4), st);
#endif
        case CONV_WINO: return launch_conv_w(conv_params_w(cw, c, WINO_F2), st);
        case CONV_DIRECT: break;
    }
    ConvParams p = conv_params(cw, c);
    p.scratch = scratch;
    p.scratch_floats = KSPLIT_FLOATS * c.B;
    return launch_conv(p, st);
}

// ---- stand-alone convolution layer (tests, micro-benchmarks) ---------------------------------------------------------
// What conv_create and conv_create_cat share: a handle that owns its device allocations, the layer packed from its sources
static int conv_create_packed(const float *weight, const float *bias, int cout, int cin, int kh, int kw, const std::vector<SegDef> &segs,
                              pivlfn_conv **out)
{
    pivlfn_conv *c = new pivlfn_conv();
    c->owner = new pivlfn_net();
    c->cin = cin;
    const int rc = pack_conv(c->owner, "c", weight, bias, cout, cin, kh, kw, segs, &c->cw);
    if (rc) { conv_destroy(c); return rc; }
    *out = c;
    return PIVLFN_OK;
}

int conv_create(const float *weight, const float *bias, int cout, int cin, int kh, int kw, pivlfn_conv **out)
{
    PIV_REQUIRE(weight && bias && out && cout > 0 && cin > 0 && kh > 0 && kw > 0, "conv_create: bad arguments");
    pivlfn_conv *c = nullptr;
    int rc = conv_create_packed(weight, bias, cout, cin, kh, kw, {{cin, rup(cin, 4)}}, &c);
    if (rc) return rc;
    {   // pivlfn_conv2d_nhwc_plan and pivlfn_conv2d_nhwc_kernel_plan derive these from the shape alone
        const ConvShape sh = conv_shape(cout, cin, kh, kw);
        const ConvW &cw = c->cw;
        if (sh.cout_pad != cw.cout_pad || sh.nchunk != cw.nchunk || sh.tail != cw.tail || sh.col7 != (cw.wpk_c != nullptr) ||
            sh.row7 != (cw.wpk_r != nullptr) || sh.nchunk_h != cw.nchunk_h || sh.split != (cw.wpk_x != nullptr) ||
            (sh.split && sh.nchunk_x != cw.nchunk_x) || sh.split_tail != (cw.wtail_x != nullptr) || sh.wino != (cw.wpk_w != nullptr) ||
            (sh.wino && sh.nchunk_w != cw.nchunk_w) || sh.wino_b3 != (cw.wpk_wb != nullptr) || (sh.wino_b3 && sh.nstep_wb != cw.nstep_wb)) {
            set_error("internal: conv_shape disagrees with pack_conv for %d<-%d %dx%d", cout, cin, kh, kw);
            rc = PIVLFN_ERR_WEIGHTS;
        }
    }
    if (!rc && cout == 2 && cin == 32 && kh == kw && (kh == 3 || kh == 5 || kh == 7)) rc = pack_head(c->owner, weight, bias, kh, &c->head, c->hb);
    if (!rc) {
        void *d = nullptr;
        if (hipMalloc(&d, KSPLIT_FLOATS * sizeof(float)) != hipSuccess) { set_error("conv_create: scratch allocation failed"); rc = PIVLFN_ERR_HIP; }
        else { c->owner->allocs.push_back(d); c->scratch = (float *)d; }
    }
    if (rc) { conv_destroy(c); return rc; }
    *out = c;
    return PIVLFN_OK;
}

int conv_destroy(pivlfn_conv *c)
{
    if (!c) return PIVLFN_OK;
    net_destroy(c->owner);
    delete c;
    return PIVLFN_OK;
}

// The call of a single-source handle's layer: the source staged in whole groups of g channels (4, or 8 for fp16 elements), every
// channel quad of the output stored that the output's stride has room for
static ConvCall single_call(int cout, int cin, int g, const void *x, int x_stride, void *y, int y_stride, const float *res, int res_stride,
                            int leaky, int B, int H, int W, int stride, int pad_y, int pad_x)
{
    const ConvSeg sx{(const float *)x, rup(cin, g), x_stride};
    return conv_call(&sx, 1, (float *)y, y_stride, std::min(rup(cout, 4), y_stride), res, res_stride, leaky, B, H, W, stride, pad_y, pad_x);
}

// The kernel choice of pivlfn_conv2d_nhwc from the layer's shape and the call's geometry: its argument checks, the streaming kernels'
// conditions and launch_conv's own choice.  No pointer is read (res only says whether there is a residual): pivlfn_conv2d_nhwc and
// pivlfn_conv2d_nhwc_plan both come through here.  p receives everything but the pointers.  per_image: the handle's split-K scratch
// holds one image's shares, so a batch it is too small for runs image by image (pl is then one image's plan) -- the split factor,
// hence the summation order and the bits of a sample, is pivlfn_forward's at any B.
int conv_forward_choose(const ConvShape &c, int x_stride, int y_stride, const float *res, int B, int H, int W, int stride, int pad_y,
                        int pad_x, int leaky, ConvParams &p, ConvPlan &pl, bool &per_image)
{
    PIV_REQUIRE(x_stride % 4 == 0 && x_stride >= rup(c.cin, 4), "conv2d: x_stride=%d must be a multiple of 4 and >= %d", x_stride, rup(c.cin, 4));
    PIV_REQUIRE(y_stride >= c.cout, "conv2d: y_stride=%d < cout=%d", y_stride, c.cout);
    PIV_REQUIRE(stride >= 1 && pad_y >= 0 && pad_x >= 0 && H + 2 * pad_y >= c.KH && W + 2 * pad_x >= c.KW, "conv2d: bad geometry");
    ConvW cw;       // the shape without a packing
    cw.cout = c.cout; cw.cout_pad = c.cout_pad; cw.cin = c.cin; cw.KH = c.KH; cw.KW = c.KW; cw.nchunk = c.nchunk; cw.tail = c.tail;
    const ConvCall call = single_call(c.cout, c.cin, 4, nullptr, x_stride, nullptr, y_stride, res, 0, leaky, B, H, W, stride, pad_y, pad_x);
    p = conv_params(cw, call);
    p.scratch_floats = KSPLIT_FLOATS;
    per_image = false;
    // the (7 x 1) distance convolution on >= 256 x 256 images: the kernel pivlfn_forward uses for it in the fp32 mode
    if (c.col7 && calls_col7(call) && !(PIV_KNOB(1) & 65536)) {
        pl = ConvPlan{PIVLFN_CONV_PLAN_COL7, 16, 64, 0, 1};
        return check_conv_col7(x_stride, y_stride, p.cout_store, c.cout == 49, B, H, W);
    }
    if (c.row7 && calls_row7(call) && !(PIV_KNOB(1) & 65536)) {
        pl = ConvPlan{PIVLFN_CONV_PLAN_ROW7, 16, 64, 0, 1};
        return check_conv_row7(x_stride, y_stride, B, H, W);
    }
    if (int rc = choose_conv(p, pl)) return rc;
    if (B > 1) {
        ConvParams p1 = p;
        ConvPlan pl1;
        p1.B = 1;
        if (choose_conv(p1, pl1) == PIVLFN_OK && pl1.ksplit != pl.ksplit) { pl = pl1; per_image = true; }
    }
    return PIVLFN_OK;
}

ConvShape conv_shape(int cout, int cin, int kh, int kw)
{
    const int cload = rup(cin, 4);
    const int cp = rup(cout, 32), nchunk16 = (cload + 15) / 16;
    const bool split = conv_split_supports(kh, kw, 1, cp, 6), wino = kh == 3 && kw == 3;
    return ConvShape{cout, cp, cin, kh, kw, seg_chunks(cload), seg_tail(cload), packs_col7(cout, cin, kh, kw, 1, cload),
                     packs_row7(cout, cin, kh, kw, 1, cload), nchunk16, nchunk16, seg_chunks(cload), std::max(nchunk16, 2),
                     split, split && wino && cload % 16 == 4, wino, wino && conv_wino_b3_supports(cp)};
}

// The layer a shape stands for, for the choices made without a handle: where pack_conv would make a packing, a pointer that is
// never followed
static ConvW shape_layer(const ConvShape &sh)
{
    static float packed = 0.f;
    ConvW cw;
    cw.cout = sh.cout; cw.cout_pad = sh.cout_pad; cw.cin = sh.cin; cw.KH = sh.KH; cw.KW = sh.KW; cw.nchunk = sh.nchunk; cw.tail = sh.tail;
    cw.wpk_h = &packed; cw.nchunk_h = sh.nchunk_h;
    if (sh.split) { cw.wpk_x = &packed; cw.nchunk_x = sh.nchunk_x; }
    if (sh.split_tail) cw.wtail_x = &packed;
    if (sh.wino) { cw.wpk_w = &packed; cw.nchunk_w = sh.nchunk_w; }
    if (sh.wino_b3) { cw.wpk_wb = &packed; cw.nstep_wb = sh.nstep_wb; }
    return cw;
}

int conv_forward(const pivlfn_conv *c, const float *x, int x_stride, float *y, int y_stride, const float *res, int res_stride,
                 int B, int H, int W, int stride, int pad_y, int pad_x, int leaky, hipStream_t st)
{
    PIV_REQUIRE(c && x && y, "conv2d: null argument");
    const ConvShape sh{c->cw.cout, c->cw.cout_pad, c->cin, c->cw.KH, c->cw.KW, c->cw.nchunk, c->cw.tail, c->cw.wpk_c != nullptr, c->cw.wpk_r != nullptr};
    ConvParams p;
    ConvPlan pl;
    bool per_image;
    if (int rc = conv_forward_choose(sh, x_stride, y_stride, res, B, H, W, stride, pad_y, pad_x, leaky, p, pl, per_image)) return rc;
    if (pl.family == PIVLFN_CONV_PLAN_COL7)
        return launch_conv_col7(x, x_stride, c->cw.wpk_c, c->cw.bias, y, y_stride, p.cout_store, c->cw.cout == 49, B, H, W, st);
    if (pl.family == PIVLFN_CONV_PLAN_ROW7)
        return launch_conv_row7(x, x_stride, c->cw.wpk_r, c->cw.wpk_r12, c->cw.bias, y, y_stride, B, H, W, st);
    p.seg[0].ptr = x;
    p.wpk = c->cw.wpk; p.bias = c->cw.bias; p.out = y; p.res_stride = res_stride;
    p.scratch = c->scratch;
    if (!per_image) return launch_conv(p, st);
    p.B = 1;
    for (int b = 0; b < B; ++b) {
        p.seg[0].ptr = x + (size_t)b * H * W * x_stride;
        p.out = y + (size_t)b * p.Ho * p.Wo * y_stride;
        if (res) p.res = res + (size_t)b * p.Ho * p.Wo * res_stride;
        if (int rc = launch_conv(p, st)) return rc;
    }
    return PIVLFN_OK;
}

// One Conv2d over the channel concatenation of up to three sources (torch.cat + Conv2d, src/models.py:165-187, 209-217, 280: the
// front layers of Matching / Subpixel / Regularization), through the same dispatch as pivlfn_forward's fp32 mode: multi-source
// staging of the direct and the Winograd kernel for per-layer checks.
int conv_create_cat(const float *weight, const float *bias, int cout, int nsrc, const int *channels, int kh, int kw, pivlfn_conv **out)
{
    PIV_REQUIRE(weight && bias && out && channels && cout > 0 && nsrc >= 1 && nsrc <= 3 && kh > 0 && kw > 0, "conv_create_cat: bad arguments");
    int cin = 0;
    std::vector<SegDef> segs;
    for (int i = 0; i < nsrc; ++i) {
        PIV_REQUIRE(channels[i] > 0, "conv_create_cat: source %d has %d channels", i, channels[i]);
        segs.push_back(SegDef{channels[i], rup(channels[i], 4)});
        cin += channels[i];
    }
    pivlfn_conv *c = nullptr;
    if (int rc = conv_create_packed(weight, bias, cout, cin, kh, kw, segs, &c)) return rc;
    c->nsrc = nsrc;
    for (int i = 0; i < nsrc; ++i) c->src_real[i] = channels[i];
    *out = c;
    return PIVLFN_OK;
}

int conv_head_forward(const pivlfn_conv *c, const float *x, const float *res4, float *out4, int B, int H, int W, hipStream_t st)
{
    PIV_REQUIRE(c && c->head, "conv_head: the layer is not a 32->2 kxk flow head");
    return launch_conv_head(x, c->head, c->hb[0], c->hb[1], res4, out4, B, H, W, c->cw.KH, st);
}

// ---- the stand-alone entry points of the other four families: conv_call_* holds an entry point's checks, its parameter block and the
// launcher's choice for a layer cw of cin channels -- a handle's, or a shape's stand-in with null x and y (conv_kernel_plan): nothing in
// them follows a pointer
static int conv_call_h(const ConvW &cw, int cin, const void *x, int x_stride, int x_f16, void *y, int y_stride, int y_f16,
                       int B, int H, int W, int stride, int pad_y, int pad_x, int leaky, ConvParamsH &q, ConvKernelPlan &pl)
{
    const int g = x_f16 ? 8 : 4;
    PIV_REQUIRE(x_stride % g == 0 && x_stride >= rup(cin, g), "conv2d_f16: x_stride=%d must be a multiple of %d and >= %d", x_stride, g, rup(cin, g));
    PIV_REQUIRE(y_stride % 4 == 0 && y_stride >= cw.cout, "conv2d_f16: y_stride=%d must be a multiple of 4 and >= cout=%d", y_stride, cw.cout);
    PIV_REQUIRE(stride >= 1 && pad_y >= 0 && pad_x >= 0 && H + 2 * pad_y >= cw.KH && W + 2 * pad_x >= cw.KW, "conv2d_f16: bad geometry");
    ConvCall call = single_call(cw.cout, cin, g, x, x_stride, y, y_stride, nullptr, 0, leaky, B, H, W, stride, pad_y, pad_x);
    call.in16 = x_f16 ? 1 : 0;
    call.out16 = y_f16;
    q = conv_params_h(cw, call);
    ConvChoice<ConvParamsH> ch;
    const int rc = choose_conv_h(q, ch);
    pl = ch.pl;
    return rc;
}

// Standalone layer in the fp16 mode (tests, tools): x / y element types chosen per call.
int conv_forward_h(const pivlfn_conv *c, const void *x, int x_stride, int x_f16, void *y, int y_stride, int y_f16,
                   int B, int H, int W, int stride, int pad_y, int pad_x, int leaky, hipStream_t st)
{
    PIV_REQUIRE(c && x && y, "conv2d_f16: null argument");
    ConvParamsH q;
    ConvKernelPlan pl;
    if (int rc = conv_call_h(c->cw, c->cin, x, x_stride, x_f16, y, y_stride, y_f16, B, H, W, stride, pad_y, pad_x, leaky, q, pl)) return rc;
    return launch_conv_h(q, st);
}

// pl.per_image: the handle has one image's worth of split-K scratch, so a batch of a grid launch_conv_x may split runs image by image
// (pl is then one image's plan): the split factor -- hence the summation order and the bits of a sample -- is the same whatever the
// batch (the invariant launch_conv_x states for the network's own calls)
static int conv_call_x(const ConvW &cw, int cin, bool has_scratch, const float *x, int x_stride, float *y, int y_stride, int B, int H, int W,
                       int stride, int pad_y, int pad_x, int leaky, int terms, ConvParamsX &q, ConvKernelPlan &pl)
{
    PIV_REQUIRE(terms == 6 || terms == 3, "conv2d_split: terms=%d (6 or 3 partial products per product)", terms);
    PIV_REQUIRE(cw.wpk_x && conv_split_supports(cw.KH, cw.KW, stride, cw.cout_pad, terms),
                "conv2d_split: this layer's geometry (k=%dx%d, stride %d, %d-term products) is not covered by the split kernel", cw.KH, cw.KW, stride, terms);
    PIV_REQUIRE(x_stride % 4 == 0 && x_stride >= rup(cin, 4), "conv2d_split: x_stride=%d must be a multiple of 4 and >= %d", x_stride, rup(cin, 4));
    PIV_REQUIRE(y_stride % 4 == 0 && y_stride >= cw.cout, "conv2d_split: y_stride=%d must be a multiple of 4 and >= cout=%d", y_stride, cw.cout);
    PIV_REQUIRE(pad_y >= 0 && pad_x >= 0 && H + 2 * pad_y >= cw.KH && W + 2 * pad_x >= cw.KW, "conv2d_split: bad geometry");
    q = conv_params_x(cw, single_call(cw.cout, cin, 4, x, x_stride, y, y_stride, nullptr, 0, leaky, B, H, W, stride, pad_y, pad_x), terms);
    q.scratch_floats = KSPLIT_FLOATS;
    const bool per_image = B > 1 && (long)cdiv(q.Wo, 32) * cdiv(q.Ho, 4) * (q.cout_pad / 32) <= 256;      // the grids launch_conv_x may split
    ConvParamsX q1 = q;
    if (per_image) q1.B = 1;
    ConvChoice<ConvParamsX> ch;
    const int rc = choose_conv_x(q1, has_scratch, cw.wtail_x != nullptr, ch);
    pl = ch.pl;
    pl.per_image = per_image;
    return rc;
}

// Standalone layer on the split-operand kernel (tests, tools): fp32 in, fp32 out.
int conv_forward_x(const pivlfn_conv *c, const float *x, int x_stride, float *y, int y_stride,
                   int B, int H, int W, int stride, int pad_y, int pad_x, int leaky, int terms, hipStream_t st)
{
    PIV_REQUIRE(c && x && y, "conv2d_split: null argument");
    ConvParamsX q;
    ConvKernelPlan pl;
    if (int rc = conv_call_x(c->cw, c->cin, c->scratch != nullptr, x, x_stride, y, y_stride, B, H, W, stride, pad_y, pad_x, leaky, terms, q, pl))
        return rc;
    q.scratch = c->scratch;
    if (pl.per_image) {
        for (int b = 0; b < B; ++b) {
            ConvParamsX qb = q;
            qb.B = 1;
            qb.seg[0].ptr = x + (size_t)b * H * W * x_stride;
            qb.out = y + (size_t)b * q.Ho * q.Wo * y_stride;
            if (int rc = launch_conv_x(qb, st)) return rc;
        }
        return PIVLFN_OK;
    }
    return launch_conv_x(q, st);
}

// The handle's layer through the network's dispatch in the fp32 mode, on one stream
int conv_forward_cat(const pivlfn_conv *c, int nsrc, const float *const *x, const int *x_stride, float *y, int y_stride,
                     int B, int H, int W, int leaky, hipStream_t st)
{
    PIV_REQUIRE(c && x && x_stride && y && nsrc == c->nsrc, "conv2d_cat: the layer was created for %d sources", c ? c->nsrc : 0);
    PIV_REQUIRE(B > 0 && H > 0 && W > 0 && c->cw.KH % 2 == 1 && c->cw.KW % 2 == 1, "conv2d_cat: bad shape");
    PIV_REQUIRE(y_stride % 4 == 0 && y_stride >= c->cw.cout, "conv2d_cat: y_stride=%d must be a multiple of 4 and >= cout=%d", y_stride, c->cw.cout);
    ConvSeg sg[3];
    for (int i = 0; i < nsrc; ++i) {
        PIV_REQUIRE(x[i] && x_stride[i] % 4 == 0 && x_stride[i] >= rup(c->src_real[i], 4), "conv2d_cat: source %d: stride %d for %d channels", i, x_stride[i], c->src_real[i]);
        sg[i] = ConvSeg{x[i], rup(c->src_real[i], 4), x_stride[i]};
    }
    const ConvCtx ctx{0, false, nullptr, nullptr};          // never split: the handle has no per-batch scratch
    const int cs = std::min(rup(c->cw.cout, 4), y_stride);
    return conv(ctx, c->cw, conv_call(sg, nsrc, y, y_stride, cs, nullptr, 0, leaky, B, H, W, 1, c->cw.KH / 2, c->cw.KW / 2), st);
}

static int conv_call_w(const ConvW &cw, int cin, const float *x, int x_stride, float *y, int y_stride, int B, int H, int W, int leaky,
                       ConvCall &call)
{
    PIV_REQUIRE(cw.wpk_w, "conv2d_wino: the layer is not 3 x 3 (k=%dx%d)", cw.KH, cw.KW);
    PIV_REQUIRE(x_stride % 4 == 0 && x_stride >= rup(cin, 4), "conv2d_wino: x_stride=%d must be a multiple of 4 and >= %d", x_stride, rup(cin, 4));
    PIV_REQUIRE(y_stride % 4 == 0 && y_stride >= cw.cout, "conv2d_wino: y_stride=%d must be a multiple of 4 and >= cout=%d", y_stride, cw.cout);
    call = single_call(cw.cout, cin, 4, x, x_stride, y, y_stride, nullptr, 0, leaky, B, H, W, 1, 1, 1);
    return PIVLFN_OK;
}

static int conv_call_wb(const ConvW &cw, int cin, const float *x, int x_stride, float *y, int y_stride, int B, int H, int W, int leaky,
                        int terms, ConvParamsW &q)
{
    PIV_REQUIRE(cw.wpk_wb, "conv2d_wino_b3: the layer is not 3 x 3 with whole 64-channel output groups (k=%dx%d, cout_pad=%d)", cw.KH, cw.KW, cw.cout_pad);
    PIV_REQUIRE(x_stride % 4 == 0 && x_stride >= rup(cin, 4), "conv2d_wino_b3: x_stride=%d must be a multiple of 4 and >= %d", x_stride, rup(cin, 4));
    PIV_REQUIRE(y_stride % 4 == 0 && y_stride >= cw.cout, "conv2d_wino_b3: y_stride=%d must be a multiple of 4 and >= cout=%d", y_stride, cw.cout);
    q = conv_params_w(cw, single_call(cw.cout, cin, 4, x, x_stride, y, y_stride, nullptr, 0, leaky, B, H, W, 1, 1, 1), WINO_B3, terms);
    return PIVLFN_OK;
}

// Standalone 3 x 3 / stride 1 / pad 1 layer on the Winograd kernels (tests, tools): fp32 in, fp32 out.  tile = 2: F(2x2, 3x3), 4: F(4x4, 3x3).
int conv_forward_w(const pivlfn_conv *c, const float *x, int x_stride, float *y, int y_stride, int B, int H, int W, int leaky,
                   hipStream_t st, int tile)
{
    PIV_REQUIRE(tile == 2 || tile == 4, "conv2d_wino: tile=%d (2 or 4)", tile);
    PIV_REQUIRE(c && x && y, "conv2d_wino: null argument");
    ConvCall call;
    if (int rc = conv_call_w(c->cw, c->cin, x, x_stride, y, y_stride, B, H, W, leaky, call)) return rc;
    if (tile == 4) {
#ifdef PIVLFN_TOOLS
        PIV_REQUIRE(c->cw.wpk_w4, "conv2d_wino4: the layer object carries no F(4x4) weights");
        return launch_conv_w4(conv_params_w(c->cw, call, WINO_F4), st);
#else
        PIV_REQUIRE(false, "conv2d_wino: the F(4x4) kernel is part of the tools build only");
#endif
    }
    return launch_conv_w(conv_params_w(c->cw, call, WINO_F2), st);
}

// Standalone 3 x 3 / stride 1 / pad 1 layer on the split-operand Winograd kernel (conv_wino_b3.hip): fp32 in, fp32 out; terms = 6, 8 or 9.
int conv_forward_wb(const pivlfn_conv *c, const float *x, int x_stride, float *y, int y_stride, int B, int H, int W, int leaky,
                    int terms, hipStream_t st)
{
    PIV_REQUIRE(c && x && y, "conv2d_wino_b3: null argument");
    ConvParamsW q;
    if (int rc = conv_call_wb(c->cw, c->cin, x, x_stride, y, y_stride, B, H, W, leaky, terms, q)) return rc;
    return launch_conv_wb(q, st);
}

// Standalone (7 x 1) 49 <- 32 / (1 x 7) 49 <- 49 layer on the split-operand streaming kernel (conv_dist_b3.hip): fp32 in, fp32 out, 52
// stored lanes, output grid = input grid, any H, W >= 1; terms = 6, 8 or 9.  conv_dist_b3_call holds the entry point's checks for a
// layer shape -- a handle's, or the arguments of pivlfn_conv2d_nhwc_dist_b3_plan: no pointer is followed.
static int conv_dist_b3_call(int cout, int cin, int kh, int kw, int x_stride, int y_stride, int terms, int B, int H, int W, int &row)
{
    const int cload = rup(cin, 4);
    PIV_REQUIRE(packs_dist_b3(cout, cin, kh, kw, 1, cload),
                "conv2d_dist_b3: the layer is neither the (7 x 1) 49 <- 32 nor the (1 x 7) 49 <- 49 distance convolution (%d <- %d, k=%dx%d)", cout, cin, kh, kw);
    row = kw == 7;
    return check_conv_dist_b3(row, x_stride, y_stride, terms, B, H, W);
}

int conv_forward_dist_b3(const pivlfn_conv *c, const float *x, int x_stride, float *y, int y_stride, int B, int H, int W, int terms,
                         hipStream_t st)
{
    PIV_REQUIRE(c && x && y, "conv2d_dist_b3: null argument");
    int row = 0;
    if (int rc = conv_dist_b3_call(c->cw.cout, c->cin, c->cw.KH, c->cw.KW, x_stride, y_stride, terms, B, H, W, row)) return rc;
    const ConvW &cw = c->cw;
    PIV_REQUIRE(c->nsrc == 1 && (row ? cw.wpk_rb && cw.wpk_r : cw.wpk_cb && cw.wpk_c), "conv2d_dist_b3: the layer object carries no split-bf16 fragments");
    return launch_conv_dist_b3(row, x, x_stride, row ? cw.wpk_rb : cw.wpk_cb, row ? cw.wpk_r : cw.wpk_c, cw.wpk_r12, cw.bias, y, y_stride, terms, B, H, W, st);
}

// pivlfn_conv2d_nhwc_dist_b3_plan: plan = {0 walks rows (7 x 1) | 1 walks columns (1 x 7), terms, workgroups, workgroups per CU}
int conv_dist_b3_plan(int cout, int cin, int kh, int kw, int B, int H, int W, int terms, int x_stride, int y_stride, int plan[4])
{
    PIV_REQUIRE(plan, "conv2d_dist_b3_plan: null argument");
    int row = 0;
    if (int rc = conv_dist_b3_call(cout, cin, kh, kw, x_stride, y_stride, terms, B, H, W, row)) return rc;
    plan[0] = row; plan[1] = terms; plan[2] = (int)((conv_dist_b3_tiles(row, B, H, W) + 3) / 4); plan[3] = conv_dist_b3_occupancy(row);
    return PIVLFN_OK;
}

// pivlfn_conv2d_nhwc_kernel_plan: what pivlfn_conv2d_nhwc_f16 / _split / _wino / _wino_b3 would launch for a layer of this shape, as
// pivlfn_conv_create packs it, and a call of this geometry -- through the entry points' own checks and the launchers' own choices.
int conv_kernel_plan(int kernel, int cout, int cin, int kh, int kw, int B, int H, int W, int stride, int pad_y, int pad_x, int terms,
                     int x_f16, int x_stride, int y_stride, int cus, ConvKernelPlan &pl)
{
    const ConvW cw = shape_layer(conv_shape(cout, cin, kh, kw));
    switch (kernel) {
        case PIVLFN_KERNEL_PLAN_F16: {
            ConvParamsH q;
            return conv_call_h(cw, cin, nullptr, x_stride, x_f16, nullptr, y_stride, 0, B, H, W, stride, pad_y, pad_x, 1, q, pl);
        }
        case PIVLFN_KERNEL_PLAN_SPLIT: {
            ConvParamsX q;
            return conv_call_x(cw, cin, true, nullptr, x_stride, nullptr, y_stride, B, H, W, stride, pad_y, pad_x, 1, terms, q, pl);
        }
        case PIVLFN_KERNEL_PLAN_WINO: {
            PIV_REQUIRE(stride == 1 && pad_y == 1 && pad_x == 1, "conv2d_wino: stride 1 and padding 1 only (stride %d, padding %d, %d)", stride, pad_y, pad_x);
            ConvCall call;
            if (int rc = conv_call_w(cw, cin, nullptr, x_stride, nullptr, y_stride, B, H, W, 1, call)) return rc;
            ConvChoice<ConvParamsW> ch;
            const int rc = choose_conv_w(conv_params_w(cw, call, WINO_F2), ch);
            pl = ch.pl;
            return rc;
        }
        case PIVLFN_KERNEL_PLAN_WINO_B3: {
            PIV_REQUIRE(stride == 1 && pad_y == 1 && pad_x == 1, "conv2d_wino_b3: stride 1 and padding 1 only (stride %d, padding %d, %d)", stride, pad_y, pad_x);
            ConvParamsW q;
            if (int rc = conv_call_wb(cw, cin, nullptr, x_stride, nullptr, y_stride, B, H, W, 1, terms, q)) return rc;
            ConvChoiceB3 ch;
            const int rc = choose_conv_wb(q, cus, ch);
            pl = ch.pl;
            return rc;
        }
        default: PIV_REQUIRE(false, "conv2d_kernel_plan: kernel=%d (PIVLFN_KERNEL_PLAN_F16, _SPLIT, _WINO or _WINO_B3)", kernel);
    }
    return PIVLFN_OK;
}

}  // namespace pivlfn
