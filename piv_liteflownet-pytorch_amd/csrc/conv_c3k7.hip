// Direct fp32 convolution, NetC.conv1 (7 x 7, 3 -> 32) with the taps packed into K.
// conv_k1 (conv_k1.hip) contracts the 4-lane padded pixel per tap: two MFMAs (k = 2 each) of which the second carries one real channel -- 98
// MFMAs per 32 pixels for 147 real products per output.  Here the patch is stored in LDS with 3 floats per pixel, so the 21
// (tap, channel) slots of one kernel row are 21 consecutive floats: K runs over (row ky, slot pair j) and a lane half reads slot
// 2 j + hh with one immediate offset -- 7 x 11 = 77 MFMAs (the 22nd slot of a row reads the next pixel's first channel against a zero
// weight).  The 77 weight fragments stay in registers for the life of the persistent workgroup (no LDS reads for them), the patch is
// 6.5 KB: three workgroups per CU.  K order: rows, then slot pairs (conv_k1: taps, then channel pairs).
#include "conv_direct.h"

namespace pivlfn {

constexpr int C3_PW = 38, C3_PITCH = 116, C3_PH = 14;         // patch of an 8 x 32 tile, floats per patch row (38 x 3 + the pad slot)

// FUSE: the level-1 1 x 1 layers on top (Conv1Fuse): the accumulator layout of the 32 x 32 x 2 instruction is already its B-operand
// layout -- lane (pixel, hh) holds channels 8 g + 4 hh + e in register 4 g + e, and k-slot hh of the MFMA (g, e) wants exactly that
// channel -- so the activated accumulators feed the next MFMAs without a transpose: 16 MFMAs per 32 output channels.
// Round 6, where the fused kernel's 450 us go (tools/c3k7_ablate.sh, profiles/r06_c3k7_ablation.log): stores alone 248 us (1.34 GB at
// 5.4 TB/s), matrix work + loads alone 362 us, loads alone 95 us -- the phases overlap only partly.  Two ways of overlapping them more
// were built and are SLOWER on the same box: the next patch written to a second LDS buffer before the tile's stores are issued (so that
// no wait has stores in front of it; 470 vs 448 us), and the 1 x 1 blocks software-pipelined over two accumulator sets (MFMAs of block
// k + 1 between the activation / stores of block k; 522 vs 462 us; tools/kernels/conv_c3k7_pipelined_blocks.hip.txt).
template <bool FUSE, int ABL = 0>
__global__ __launch_bounds__(256, FUSE ? 2 : 3) void conv_c3k7_kernel(const ConvParams p, const Conv1Fuse f)
{
    __shared__ __attribute__((aligned(16))) float patch[C3_PH * C3_PITCH + 4];
    __shared__ __attribute__((aligned(16))) float w11s[FUSE ? 6 * 4 * 64 * 4 : 4];
    if (FUSE) {
        for (int i = threadIdx.x; i < 6 * 4 * 64; i += 256) reinterpret_cast<f32x4 *>(w11s)[i] = reinterpret_cast<const f32x4 *>(f.w11)[i];
    }
    constexpr int TH = 8;
    const int tiles_x = (p.Wo + 31) >> 5, tiles_y = (p.Ho + TH - 1) / TH;
    const int ntiles = tiles_x * tiles_y * p.B;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = lane & 31, hh = lane >> 5;
    if ((int)blockIdx.x >= ntiles) return;
    // weight fragments: slot s = 3 kx + c of row ky is wpk[((ky * 7 + kx) * 2 + (c >> 1)) * cout_pad + n][c & 1] (net_weights.hip pack_conv,
    // 4-channel tail layout); slot 21 is the pad
    float wq[7][11];
#pragma unroll
    for (int ky = 0; ky < 7; ++ky)
#pragma unroll
        for (int j = 0; j < 11; ++j) {
            const int s_ = 2 * j + hh;
            const int kx = s_ / 3, c = s_ - 3 * kx;
            wq[ky][j] = s_ < 21 ? p.wpk[(((size_t)(ky * 7 + kx) * 2 + (c >> 1)) * p.cout_pad + row) * 4 + (c & 1)] : 0.f;
        }
    for (int i = tid; i < C3_PH; i += 256) { patch[i * C3_PITCH + 114] = 0.f; patch[i * C3_PITCH + 115] = 0.f; }     // pad slots: finite
    const f32x4 bias4[4] = {*reinterpret_cast<const f32x4 *>(p.bias + 4 * hh), *reinterpret_cast<const f32x4 *>(p.bias + 8 + 4 * hh),
                            *reinterpret_cast<const f32x4 *>(p.bias + 16 + 4 * hh), *reinterpret_cast<const f32x4 *>(p.bias + 24 + 4 * hh)};
    const float *sp = p.seg[0].ptr;
    const int sst = p.seg[0].stride;
    int abase[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) abase[m] = (wave * 2 + m) * C3_PITCH + row * 3 + hh;
    f32x4 pr[3];
#define C3_LOAD(T)                                                                                \
    do {                                                                                          \
        int t_ = (T);                                                                             \
        const int tx_ = t_ % tiles_x;                                                             \
        t_ /= tiles_x;                                                                            \
        const int b_ = t_ / tiles_y;                                                              \
        const int ix0_ = tx_ * 32 - 3, iy0_ = (t_ - b_ * tiles_y) * TH - 3;                       \
        _Pragma("unroll") for (int i = 0; i < 3; ++i) {                                           \
            const int pix_ = tid + 256 * i;                                                       \
            const int py_ = pix_ / C3_PW, px_ = pix_ - py_ * C3_PW;                               \
            const int iy_ = iy0_ + py_, ix_ = ix0_ + px_;                                         \
            f32x4 v = {0.f, 0.f, 0.f, 0.f};                                                       \
            if (pix_ < C3_PH * C3_PW && iy_ >= 0 && iy_ < p.H && ix_ >= 0 && ix_ < p.W)           \
                v = *reinterpret_cast<const f32x4 *>(sp + ((size_t)(b_ * p.H + iy_) * p.W + ix_) * sst); \
            pr[i] = v;                                                                            \
        }                                                                                         \
    } while (0)

    // ABL != 0: instances of the tools build for timing runs (tools/c3k7_ablate.sh): 1 no stores of the fused 1 x 1 layers, 2 no conv1
    // stores, 4 no MFMAs of the fused layers, 8 no conv1 MFMAs, 16 no patch loads after the first
    constexpr int abl = ABL;
    C3_LOAD(blockIdx.x);
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        __syncthreads();          // the previous tile's operand reads are done
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int pix = tid + 256 * i;
            if (pix < C3_PH * C3_PW) {
                const int py = pix / C3_PW, px = pix - py * C3_PW;
                float *d = patch + py * C3_PITCH + px * 3;
                d[0] = pr[i][0]; d[1] = pr[i][1]; d[2] = pr[i][2];
            }
        }
        __syncthreads();
        if (tile + (int)gridDim.x < ntiles && !(abl & 16)) C3_LOAD(tile + gridDim.x);
        f32x16 acc[2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
#pragma unroll
        for (int ky = 0; ky < 7; ++ky)
#pragma unroll
            for (int j = 0; j < 11; ++j) {
                float a[2];
#pragma unroll
                for (int m = 0; m < 2; ++m) a[m] = patch[abase[m] + ky * C3_PITCH + 2 * j];
#pragma unroll
                for (int m = 0; m < 2; ++m)
                    if (!(abl & 8)) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(wq[ky][j], a[m], acc[m], 0, 0, 0);
                    else acc[m][j & 15] += a[m];
            }
        int t_ = tile;
        const int tx = t_ % tiles_x;
        t_ /= tiles_x;
        const int b = t_ / tiles_y;
        const int x0 = tx * 32, y0 = (t_ - b * tiles_y) * TH;
        const int ox = x0 + row;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int oy = y0 + wave * 2 + m;
            const bool ok = oy < p.Ho && ox < p.Wo;
            float *orow = p.out + ((size_t)(b * p.Ho + (ok ? oy : 0)) * p.Wo + (ok ? ox : 0)) * p.out_stride;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v = {acc[m][4 * g + 0], acc[m][4 * g + 1], acc[m][4 * g + 2], acc[m][4 * g + 3]};
                v += bias4[g];
                if (p.lrelu) {
                    v[0] = lrelu01(v[0]); v[1] = lrelu01(v[1]); v[2] = lrelu01(v[2]); v[3] = lrelu01(v[3]);
                }
                if (ok && 8 * g + 4 * hh < p.cout_store && !(abl & 2)) *reinterpret_cast<f32x4 *>(orow + 8 * g + 4 * hh) = v;
                if (FUSE) { acc[m][4 * g + 0] = v[0]; acc[m][4 * g + 1] = v[1]; acc[m][4 * g + 2] = v[2]; acc[m][4 * g + 3] = v[3]; }
            }
        }
        if (FUSE) {
            // blocks 0, 1: NetC_ext (64 channels, every image); blocks 2..5: moduleFeat (128 channels, the first B_feat images)
            const int nblk = b < f.B_feat ? 6 : 2;
#pragma unroll 1
            for (int blk = 0; blk < nblk; ++blk) {
                f32x16 a2[2];
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) a2[m][r] = 0.f;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 wv = reinterpret_cast<const f32x4 *>(w11s)[(blk * 4 + g) * 64 + lane];
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int m = 0; m < 2; ++m)
                            if (!(abl & 4)) a2[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[e], acc[m][4 * g + e], a2[m], 0, 0, 0);
                            else a2[m][4 * g + e] += wv[e] * acc[m][4 * g + e];
                }
                const bool ext = blk < 2;
                const int cb = ext ? 32 * blk : 32 * (blk - 2), cs = ext ? 64 : 128;
                const float *bsrc = f.b11 + (ext ? 0 : 64) + cb + 4 * hh;
                float *obase = ext ? f.out_ext : f.out_feat;
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const int oy = y0 + wave * 2 + m;
                    if (oy >= p.Ho || ox >= p.Wo) continue;
                    float *orow = obase + ((size_t)(b * p.Ho + oy) * p.Wo + ox) * cs + cb + 4 * hh;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        f32x4 v = {a2[m][4 * g + 0], a2[m][4 * g + 1], a2[m][4 * g + 2], a2[m][4 * g + 3]};
                        v += *reinterpret_cast<const f32x4 *>(bsrc + 8 * g);
                        v[0] = lrelu01(v[0]); v[1] = lrelu01(v[1]); v[2] = lrelu01(v[2]); v[3] = lrelu01(v[3]);
                        if (!(abl & 1) || v[0] == 1.2345e38f) *reinterpret_cast<f32x4 *>(orow + 8 * g) = v;
                    }
                }
            }
        }
    }
#undef C3_LOAD
}

// Applies to: 7 x 7, stride 1, pad 3, one source of 3 real channels on 4 lanes, 32 output channels, no residual, >= 512 tiles
static bool c3k7_applies(const ConvParams &p)
{
    if (p.KH != 7 || p.KW != 7 || p.S != 1 || p.padY != 3 || p.padX != 3 || p.nseg != 1 || p.seg[0].cload != 4 || p.nchunk != 1 || !p.tail ||
        p.res || p.cout_pad != 32 || p.cin_real != 3)
        return false;
    return (long)cdiv(p.Wo, 32) * cdiv(p.Ho, 8) >= 512;             // per image: never a function of the batch
}

// The plain instantiation (static LDS: no bound of its own); grid: persistent workgroups, per CU the launch bound's 3 (2 with the fused layers)
struct launch_c3k7 {
    static dim3 grid(const ConvParams &p, long per_cu) { return dim3((unsigned)std::min<long>((long)cdiv(p.Wo, 32) * cdiv(p.Ho, 8) * p.B, per_cu * device_cus())); }
    static int plan(const ConvParams &, ConvPlan &pl) { pl = ConvPlan{PIVLFN_CONV_PLAN_C3K7, 8, 32, 0, 1}; return PIVLFN_OK; }
    static int run(const ConvParams &p, hipStream_t st)
    {
        hipLaunchKernelGGL((conv_c3k7_kernel<false>), grid(p, 3), dim3(256), 0, st, p, Conv1Fuse{});
        PIV_CHECK_HIP(hipGetLastError());
        return PIVLFN_OK;
    }
};

bool choose_conv_c3k7(const ConvParams &p, ConvChoiceD &ch)
{
    if (!c3k7_applies(p) || (PIV_KNOB(1) & 134217728)) return false;
    return conv_take<launch_c3k7>(p, ch) == PIVLFN_OK;
}

// conv1 + NetC_ext + moduleFeat of level 1 in one launch (same applicability as choose_conv_c3k7; cout_store 32, LeakyReLU on)
int launch_conv1_fused(const ConvParams &p, const Conv1Fuse &f, hipStream_t st)
{
    if (!c3k7_applies(p) || p.cout_store != 32 || !p.lrelu || !f.w11 || !f.b11 || !f.out_ext || !f.out_feat) return -1;
    const dim3 grid = launch_c3k7::grid(p, 2);
    switch (PIV_KNOB(7)) {
#ifdef PIVLFN_TOOLS
#define C3_ABL(M) case M: hipLaunchKernelGGL((conv_c3k7_kernel<true, M>), grid, dim3(256), 0, st, p, f); break;
        C3_ABL(1) C3_ABL(2) C3_ABL(3) C3_ABL(4) C3_ABL(5) C3_ABL(12) C3_ABL(15) C3_ABL(28) C3_ABL(31)
#undef C3_ABL
#endif
        default: hipLaunchKernelGGL((conv_c3k7_kernel<true>), grid, dim3(256), 0, st, p, f);
    }
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
