// Internal declarations shared by net_weights.hip (weight packing, the network object), conv_layer.hip (one layer call: kernel
// choice, parameter blocks, the stand-alone layer handles), net.hip (workspace plan, forward) and api.hip.
#pragma once
#include <vector>
#include "common.h"

namespace pivlfn {

static const int K_LEVEL[7] = {0, 7, 7, 5, 5, 3, 3};            // src/models.py:161,205,225
static const int C_FEAT[7] = {0, 32, 32, 64, 96, 128, 192};     // src/models.py:70-106
static const int C_MATCH[7] = {0, 64, 64, 64, 96, 128, 192};    // NetC_ext: src/models.py:124,353-357

static inline int rup(int a, int b) { return (a + b - 1) / b * b; }

// Split-K scratch (conv_mfma.hip): a layer is split only when one image has <= 128 workgroups of 128 px x 32 channels, i.e. at
// most 128*128*32 partial sums per share and image, and into at most 8 shares.
static const size_t KSPLIT_FLOATS = (size_t)8 * 128 * 128 * 32;
// The reduction of the shares is a kernel of its own (16 launches of 6.7 us at 1024^2).  Round 6 let the share that arrives last at a
// tile do it (arrival counter, agent-scope release / acquire fences; same order, same bits): the forward got 0.42 ms SLOWER
// (profiles/r06_item5_net_ab.log) -- a release at agent scope writes back the XCD's whole L2 (eight L2s that are not coherent with
// each other), ~500 workgroups x 16 layers of it while the side stream keeps 1.4 GB of dirty lines going.  Not adopted.

void pack_conv_h(const float *w, int cout, int cin, int taps, const int *creal, const int *cload, const int *coff, int nseg,
                 std::vector<unsigned short> &pk, int *nchunk_out);      // conv_f16.hip
void pack_conv_x(const float *w, int cout, int cin, int taps, const int *creal, const int *cload, const int *coff, int nseg,
                 std::vector<unsigned short> &pk, int *nchunk_out, float *out_scale);      // conv_split.hip
void pack_conv_x_tail(const float *w, int cout, int cin, int c_first, int c_real, float scale_inv, std::vector<unsigned short> &pk);
void pack_conv_w(const float *w, int cout, int cin, const int *creal, const int *cload, const int *coff, int nseg,
                 std::vector<float> &pk, int *nchunk_out);
#ifdef PIVLFN_TOOLS
void pack_conv_w4(const float *w, int cout, int cin, const int *creal, const int *cload, const int *coff, int nseg,
                 std::vector<float> &pk, int *nchunk_out);      // tools/kernels/conv_wino4.hip
#endif
void pack_conv_wb(const float *w, int cout, int cin, const int *creal, const int *cload, const int *coff, int nseg,
                  std::vector<unsigned short> &pk, int *nstep_out);      // conv_wino_b3.hip
void pack_conv_dist_b3(const float *w, int cin, std::vector<unsigned short> &pk);      // conv_dist_b3.hip: w = OIHW [49][cin = 32 | 49][7 taps]

struct ConvW {
    float *wpk = nullptr, *bias = nullptr;
    int cout = 0, cout_pad = 0, KH = 0, KW = 0, nchunk = 0, tail = 0, cin = 0;
    void *wpk_h = nullptr;         // fp16 packing for conv_f16.hip (K chunks of 16 channels)
    int nchunk_h = 0;
    void *wpk_x = nullptr;         // three-piece fp16 packing for conv_split.hip (fp32 by exact splitting); nullptr = unsupported geometry
    int nchunk_x = 0;
    float scale_x = 1.f;           // 2^-k undoing the weight scale of wpk_x
    void *wtail_x = nullptr;       // 3 x 3 layers whose staged channels end in a 4-lane tail: that chunk with taps folded into K
    float *wpk_c = nullptr;        // (7 x 1) layers from 32 channels: A fragments of conv_col7_kernel, [4][7][2][64][4]
    float *wpk_r = nullptr, *wpk_r12 = nullptr;   // the (1 x 7) 49 -> 49 layer: A fragments of conv_row7_kernel, [4][7][3][64][4] and [4][7][64]
    void *wpk_cb = nullptr, *wpk_rb = nullptr;    // the 49-channel ones of those once more as three bf16 pieces per weight: A fragments of
                                                  // conv_dist_b3_kernel, [3][7][steps 1 | 2][3][64][8] (made where packs_dist_b3 holds)
    float *wpk_w = nullptr;        // 3 x 3 layers: Winograd-domain weights G g G^T in fragment order (conv_wino.hip)
    float *wpk_w4 = nullptr;       // the same for F(4x4, 3x3): 36 planes (conv_wino4.hip)
    int nchunk_w = 0, nchunk_w4 = 0;
    void *wpk_wb = nullptr;        // 3 x 3 layers with whole 64-channel groups: the Winograd-domain weights as three bf16 pieces each (conv_wino_b3.hip)
    int nstep_wb = 0;
};

struct LevelW {
    float *upconv = nullptr, *upcorr = nullptr;    // depthwise k4 weights [16 taps][C4]
    ConvW M[6], S[6], R[6], feat, dist0, dist1;   // M/S: nstack hidden 3x3 layers, then the k x k head at index nstack
    // conv_R.0 once more as two layers (levels < 5): R0a = its 128 moduleFeat input channels, zero bias (flow-independent: net_forward
    // computes it on the side stream); R0b = its three [difference, flow - mean] channels with the layer's bias, which adds R0a's output
    ConvW R0a, R0b;
    float *r0t = nullptr;          // R0b's weights once more as [9 taps][3 channels][128 outputs] for reg_r0_tail_kernel (ops.hip)
    float *headM = nullptr, *headS = nullptr;      // VALU flow-head weights [k*k][8][4][2]
    float hbM[2] = {0.f, 0.f}, hbS[2] = {0.f, 0.f};
    float *wx = nullptr, *wy = nullptr;
    float bx = 0.f, by = 0.f;
};

}  // namespace pivlfn

struct pivlfn_net;
struct pivlfn_conv {
    pivlfn::ConvW cw;
    int cin = 0;
    int nsrc = 1;              // sources of the layer (pivlfn_conv_create_cat: a convolution over a channel concatenation)
    int src_real[3] = {0, 0, 0};
    float *scratch = nullptr;  // split-K scratch (KSPLIT_FLOATS), allocated by conv_create
    float *head = nullptr;     // set when the layer is a 32->2 kxk flow head
    float hb[2] = {0.f, 0.f};
    pivlfn_net *owner = nullptr;   // holds the device allocations
};

struct pivlfn_net {
    float scale[7];
    int lowest;
    int nstack = 3;                // hidden conv_M / conv_S layers: 3 = LiteFlowNet (src/models.py:154-163), 5 = LiteFlowNet2 (:487-500)
    int width[5] = {128, 64, 32, 0, 0};
    float mean[6];
    int precision = 0;             // PIVLFN_PRECISION_*: 0 fp32 instruction (default; 3x3 stride-1 layers by Winograd), 1 fp16 multiplicands,
                                   // 2 / 3 fp32 by operand splitting, 4 fp32 instruction with direct convolution everywhere
    pivlfn::ConvW netc[10];
    pivlfn::ConvW ext[3];          // index by level (1,2)
    pivlfn::LevelW lv[7];
    std::vector<void *> allocs;
    // side stream for the flow-independent 1x1 convs (NetC_ext, moduleFeat): they overlap the latency-bound coarse levels
    hipStream_t side = nullptr;
    float *fuse1_w = nullptr, *fuse1_b = nullptr;      // level 1: NetC_ext + moduleFeat as 1 x 1 layers inside NetC.conv1's kernel (Conv1Fuse)
    hipEvent_t ev_fork[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, ev_join[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // the flow-independent part of conv_R.0 (R0a) on the side stream: a join per level; one fork, for level 1 behind conv1's fused kernel
    hipEvent_t ev_pfork = nullptr, ev_pjoin[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // measurement hooks
    int prof_level = 0;
    std::vector<hipEvent_t> ev;
    size_t ev_used = 0;
    long ev_dropped = 0;
};

namespace pivlfn {

// ---- weight packing and the network object (net_weights.hip) --------------------------------------------------------------------
// A host array to the device, freed with the net; P is T, or void for the packings the kernels take as untyped 16-bit data
template <typename T, typename P>
static int upload(pivlfn_net *net, const std::vector<T> &h, P **dev)
{
    void *d = nullptr;
    PIV_CHECK_HIP(hipMalloc(&d, h.size() * sizeof(T)));
    net->allocs.push_back(d);
    PIV_CHECK_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *dev = (P *)d;
    return PIVLFN_OK;
}

// What pack_conv makes of a layer's shape, for the callers that have the shape and no packed layer (pivlfn_conv2d_nhwc_plan):
// K chunks of 8 staged channels per source, the last one a 4-channel tail chunk when cload = 4 mod 8; the streaming kernels' packings
static inline int seg_chunks(int cload) { return (cload + 7) / 8; }
static inline int seg_tail(int cload) { return cload % 8 != 0 && cload % 8 <= 4; }
static inline bool packs_col7(int cout, int cin, int kh, int kw, size_t nseg, int cload0) { return kh == 7 && kw == 1 && cin == 32 && cout <= 64 && nseg == 1 && cload0 == 32; }
static inline bool packs_row7(int cout, int cin, int kh, int kw, size_t nseg, int cload0) { return kh == 1 && kw == 7 && cin == 49 && cout == 49 && nseg == 1 && cload0 == 52; }
// the split-bf16 packing of the two: where the streaming packing is made and the layer has 49 output channels
static inline bool packs_dist_b3(int cout, int cin, int kh, int kw, size_t nseg, int cload0)
{
    return cout == 49 && (packs_col7(cout, cin, kh, kw, nseg, cload0) || packs_row7(cout, cin, kh, kw, nseg, cload0));
}

struct SegDef { int creal, cload; int coff = -1; };   // coff: first input channel of this source in the OIHW weight (-1 = running offset)

// w: OIHW [cout, cin, kh, kw], b: [cout], on the host; name only words the messages
int pack_conv(pivlfn_net *net, const char *name, const float *w, const float *b, int cout, int cin, int kh, int kw,
              const std::vector<SegDef> &segs, ConvW *out);
int pack_head(pivlfn_net *net, const float *w, const float *b, int k, float **dev, float bias[2]);     // w: OIHW [2, 32, k, k], b: [2]
void pack_dw_host(const float *w, int C, int cpad, std::vector<float> &h);
void pack_conv1_fuse(const float *we, const float *be, const float *wf, const float *bfe, std::vector<float> &w11, std::vector<float> &b11);

int net_create(const pivlfn_tensor *tensors, int n, float starting_scale, int lowest, const float mean[6], pivlfn_net **out);
int net_destroy(pivlfn_net *net);
int net_profile_enable(pivlfn_net *net, int level);
int net_profile_read(pivlfn_net *net, double *ms, double *ms_empty, long *launches, int reset);
int net_set_precision(pivlfn_net *net, int precision);

// ---- one layer call (conv_layer.hip) ---------------------------------------------------------------------------------------------
// What the kernel choice depends on besides the layer and the call: set by the caller for each of its calls, nothing is remembered.
struct ConvCtx {
    int precision;         // PIVLFN_PRECISION_* 0 ... 4 (5 is precision 0 with no_b3)
    bool no_b3;            // PIVLFN_PRECISION_F32_WINO_MFMA32: precision 0 with every Winograd layer on the fp32 instruction
    float *scratch;        // split-K scratch of the forward in progress, KSPLIT_FLOATS per image (main stream only); nullptr: never split
    hipStream_t side;      // the caller's side stream (it never splits: there is one scratch area), or nullptr
    int side_cus = 0;      // compute units a persistent kernel may take when it is launched on `side` (0 = all): the rest stay free for
                           // the main stream's kernels, which cannot share a CU with a workgroup that holds its whole register file
};

// This layer, called like this.  Every kernel family's parameter block is made from a ConvW and one of these.
struct ConvCall {
    ConvSeg src[3];
    int nsrc;
    float *out;            // fp16 elements when out16
    int out_stride, cout_store;
    const float *res;      // optional residual (direct kernels only)
    int res_stride;
    int lrelu;
    int B, H, W, S, padY, padX;
    // in16: bit i set = source i holds fp16 elements; out16: the output is stored as fp16.  Both are only ever non-zero for layers
    // that run on the fp16 kernel (net_forward's `h16` uses the same size test as the choice).
    int in16, out16;
};

static inline ConvCall conv_call(const ConvSeg *segs, int nseg, float *out, int out_stride, int cout_store, const float *res,
                                 int res_stride, int lrelu, int B, int H, int W, int S, int padY, int padX, int in16 = 0, int out16 = 0)
{
    ConvCall c{{}, nseg, out, out_stride, cout_store, res, res_stride, lrelu, B, H, W, S, padY, padX, in16, out16};
    for (int i = 0; i < nseg; ++i) c.src[i] = segs[i];
    return c;
}

// The network's per-layer dispatch: chooses the kernel family from ctx, the layer and the call, fills its parameter block, launches.
int conv(const ConvCtx &ctx, const ConvW &cw, const ConvCall &c, hipStream_t st);
// The ConvParams of a call: everything but the split-K scratch, which is the caller's (also for launch_conv1_fused)
ConvParams conv_params(const ConvW &cw, const ConvCall &c);

// A single-source layer's shape as pivlfn_conv_create packs it, and pivlfn_conv2d_nhwc's kernel choice for a call of it
// nchunk_h / _x / _w, nstep_wb: the K chunks of the fp16, split and Winograd packings; split, split_tail, wino, wino_b3: whether the layer
// gets the split packing, its folded 4-lane tail, the Winograd packing, its three-piece bf16 form
struct ConvShape {
    int cout, cout_pad, cin, KH, KW, nchunk, tail;
    bool col7, row7;
    int nchunk_h, nchunk_x, nchunk_w, nstep_wb;
    bool split, split_tail, wino, wino_b3;
};
ConvShape conv_shape(int cout, int cin, int kh, int kw);
int conv_kernel_plan(int kernel, int cout, int cin, int kh, int kw, int B, int H, int W, int stride, int pad_y, int pad_x, int terms,
                     int x_f16, int x_stride, int y_stride, int cus, ConvKernelPlan &pl);
int conv_forward_choose(const ConvShape &c, int x_stride, int y_stride, const float *res, int B, int H, int W, int stride, int pad_y,
                        int pad_x, int leaky, ConvParams &p, ConvPlan &pl, bool &per_image);

int conv_create(const float *weight, const float *bias, int cout, int cin, int kh, int kw, pivlfn_conv **out);
int conv_create_cat(const float *weight, const float *bias, int cout, int nsrc, const int *channels, int kh, int kw, pivlfn_conv **out);
int conv_destroy(pivlfn_conv *c);
int conv_forward(const pivlfn_conv *c, const float *x, int x_stride, float *y, int y_stride, const float *res, int res_stride,
                 int B, int H, int W, int stride, int pad_y, int pad_x, int leaky, hipStream_t st);
int conv_forward_h(const pivlfn_conv *c, const void *x, int x_stride, int x_f16, void *y, int y_stride, int y_f16,
                   int B, int H, int W, int stride, int pad_y, int pad_x, int leaky, hipStream_t st);
int conv_forward_x(const pivlfn_conv *c, const float *x, int x_stride, float *y, int y_stride,
                   int B, int H, int W, int stride, int pad_y, int pad_x, int leaky, int terms, hipStream_t st);
int conv_forward_cat(const pivlfn_conv *c, int nsrc, const float *const *x, const int *x_stride, float *y, int y_stride,
                     int B, int H, int W, int leaky, hipStream_t st);
int conv_forward_w(const pivlfn_conv *c, const float *x, int x_stride, float *y, int y_stride, int B, int H, int W, int leaky,
                   hipStream_t st, int tile);
int conv_forward_wb(const pivlfn_conv *c, const float *x, int x_stride, float *y, int y_stride, int B, int H, int W, int leaky,
                    int terms, hipStream_t st);
int conv_forward_dist_b3(const pivlfn_conv *c, const float *x, int x_stride, float *y, int y_stride, int B, int H, int W, int terms,
                         hipStream_t st);
int conv_dist_b3_plan(int cout, int cin, int kh, int kw, int B, int H, int W, int terms, int x_stride, int y_stride, int plan[4]);
int conv_head_forward(const pivlfn_conv *c, const float *x, const float *res4, float *out4, int B, int H, int W, hipStream_t st);

// ---- workspace plan, forward, per-layer checks of the level pipeline (net.hip) ---------------------------------------------------
size_t net_workspace_bytes(const pivlfn_net *net, int B, int H, int W);
size_t net_levels_floats(const pivlfn_net *net, int B, int H, int W);
int net_forward(pivlfn_net *net, const float *img1, const float *img2, float *flow, float *levels, int B, int H, int W,
                void *ws, size_t ws_bytes, hipStream_t st);
int upconv_forward(const float *in, const float *w, float *out, int B, int H, int W, int quads, int stride_in, int stride_out,
                   hipStream_t st);
int conv1_fused_forward(const float *w1, const float *b1, const float *we, const float *be, const float *wf, const float *bfe,
                        const float *x, float *out, float *out_ext, float *out_feat, int N, int H, int W, int B_feat, int *fused,
                        hipStream_t st);

}  // namespace pivlfn
