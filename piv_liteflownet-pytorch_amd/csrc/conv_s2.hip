// Direct fp32 convolution, 3 x 3 / stride 2 from 32 channels (NetC.conv2.0 32 -> 32 at 1024^2, NetC.conv3.0 32 -> 64 at 512^2).
// The v2 kernel (conv_mfma.hip) stages 8 channels of its patch per K chunk: 32 of a pixel's 128 bytes, four times over a workgroup's life, and with
// ~100 patches of 90-270 KB in flight per XCD the line has left that L2 before the next chunk asks for it -- the layer fetched its
// input 3.3 times (FETCH_SIZE, round 3) and ran at the HBM bound of that traffic.  Here a pixel is fetched once, as one whole line:
// the patch holds all 32 channels (17 x 33 pixels for an 8 x 16 output tile: 2 rows x 16 columns per wave), the weights of the whole
// layer stay in LDS for the workgroup's life, a workgroup walks tiles blockIdx.x, + gridDim.x, ... with the next tile's patch
// prefetched into registers under the current tile's MFMAs (one workgroup per CU: the patch and the weights take 118-155 KB).
// K order per output: the four 8-channel groups outer, taps inner, as in the v2 kernel.
// (Measured and dropped: the weight fragments straight from global memory, ten steps ahead of their use, so that the patch alone
// is in LDS and two workgroups fit a CU -- 291 us against 119 on 32 -> 32 at 1024^2: the fragment loads queue behind the next
// patch's HBM loads in the in-order wait counter, and 36 KB of fragments per tile and wave do not stay in L1.)
#include "conv_direct.h"

namespace pivlfn {

constexpr int S2_PIXP = 36, S2_PH = 17, S2_PW = 33, S2_NPIX = S2_PH * S2_PW, S2_PMAX = 18;     // 561 x 8 quads <= 256 x 18

template <int NT>
__global__ __launch_bounds__(256) void conv_s2c32_kernel(const ConvParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int BN = 32 * NT;
    float *patch = smem;
    float *wts = smem + S2_NPIX * S2_PIXP;
    const int tiles_x = (p.Wo + 15) >> 4, tiles_y = (p.Ho + 7) >> 3;
    const int ntiles = tiles_x * tiles_y * p.B;
    const int n0 = blockIdx.y * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = lane & 31, hh = lane >> 5, prow = (lane >> 4) & 1, pcol = lane & 15;
    if ((int)blockIdx.x >= ntiles) return;
    {   // the layer's weights for this block of output channels -> LDS, once: [group][tap][half][BN][4]
        const f32x4 *wsrc = reinterpret_cast<const f32x4 *>(p.wpk) + n0;
        for (int idx = tid; idx < 4 * 9 * 2 * BN; idx += 256)
            reinterpret_cast<f32x4 *>(wts)[idx] = wsrc[(idx / BN) * p.cout_pad + (idx % BN)];
    }
    const int abase = ((2 * (wave * 2 + prow)) * S2_PW + 2 * pcol) * S2_PIXP + hh * 4;
    const int bbase = (hh * BN + row) * 4;
    const float *sp = p.seg[0].ptr;
    const int sst = p.seg[0].stride;
    const int q = tid & 7, pix0 = tid >> 3;             // staging slot i: quad q of patch pixel pix0 + 32 i
    f32x4 bias4[NT][4];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int g = 0; g < 4; ++g) bias4[n][g] = *reinterpret_cast<const f32x4 *>(p.bias + n0 + n * 32 + 8 * g + 4 * hh);
    // patch coordinates of this thread's slots (the same for every tile): py << 8 | px, 0xffff = past the patch
    unsigned pyx[S2_PMAX];
#pragma unroll
    for (int i = 0; i < S2_PMAX; ++i) {
        const int pix = pix0 + 32 * i;
        const int py = pix / S2_PW, px = pix - py * S2_PW;
        pyx[i] = pix < S2_NPIX ? (unsigned)(py << 8 | px) : 0xffffu;
    }

    f32x4 pr[S2_PMAX];
    // Buffer loads through a descriptor that starts at the first image row of the tile's patch: zero padding and slots past the patch
    // carry an out-of-range offset (no branch around a load), and one image may be of any size.
#define S2_LOAD(T)                                                                                \
    do {                                                                                          \
        int t_ = (T);                                                                             \
        const int tx_ = t_ % tiles_x;                                                             \
        t_ /= tiles_x;                                                                            \
        const int b_ = t_ / tiles_y;                                                              \
        const int ix0_ = tx_ * 32 - 1, iy0_ = (t_ - b_ * tiles_y) * 16 - 1;                       \
        const int row0_ = min(max(iy0_, 0), p.H - 1);                                             \
        const size_t left_ = (size_t)(p.H - row0_) * p.W - 1;                                     \
        const __amdgpu_buffer_rsrc_t rs_ = __builtin_amdgcn_make_buffer_rsrc(                     \
            const_cast<float *>(sp + ((size_t)b_ * p.H * p.W + (size_t)row0_ * p.W) * sst), 0,    \
            (unsigned)min((left_ * sst + 32) * 4, (size_t)0x7fffffff), 0x00020000);               \
        _Pragma("unroll") for (int i = 0; i < S2_PMAX; ++i) {                                     \
            const int iy_ = iy0_ + (int)(pyx[i] >> 8), ix_ = ix0_ + (int)(pyx[i] & 255u);         \
            const bool ok_ = (pyx[i] != 0xffffu) & (iy_ >= 0) & (iy_ < p.H) & (ix_ >= 0) & (ix_ < p.W); \
            const unsigned off_ = ok_ ? (unsigned)((iy_ - row0_) * p.W + ix_) * (unsigned)(sst * 4) + 16u * q : C2OOB; \
            pr[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_, (int)off_, 0, 0)); \
        }                                                                                         \
    } while (0)

#ifndef S2_ABL_CT
#define S2_ABL_CT 0               // timing-only ablations (tools/ab_variant.sh): 1 no MFMAs, 2 no patch loads after the first, 4 no stores, 8 no LDS commit, 16 no barriers
#endif
    S2_LOAD(blockIdx.x);
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (!(S2_ABL_CT & 16)) __syncthreads();          // the previous tile's operand reads are done (first pass: the weights are written)
#pragma unroll
        for (int i = 0; i < S2_PMAX; ++i)
            if (pyx[i] != 0xffffu && (!(S2_ABL_CT & 8) || tile == (int)blockIdx.x)) *reinterpret_cast<f32x4 *>(patch + (pix0 + 32 * i) * S2_PIXP + 4 * q) = pr[i];
        if (!(S2_ABL_CT & 16)) __syncthreads();
        if (tile + (int)gridDim.x < ntiles && !(S2_ABL_CT & 2)) S2_LOAD(tile + gridDim.x);
        f32x16 acc[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
        // 36 steps (group c, tap): one 16-byte read of either operand feeds four MFMAs.  The reads run S2_D steps ahead of their
        // MFMAs, pinned by scheduling fences: with one wave per SIMD nothing else covers an LDS round trip (left to the compiler the
        // reads sit right in front of their use).  Measured: the same 120 us on 32 -> 32 at 1024^2 either way -- a tile takes
        // 17.8 k cycles for 9.2 k of matrix work.  Compile-time ablations (S2_ABL_CT, tools/ab_variant.sh; us per launch): whole
        // 121.7, without the MFMAs 70.9, without the next patch's loads 96.9, without the stores 109.0, without the LDS commit
        // 116.8, without the barriers 122.1, with none of the first four 22.5 -- the pieces ADD (51 + 25 + 13 + 5 + 22): one wave per
        // SIMD runs them in order and nothing else is there to overlap them.  Two workgroups per CU need the weights out of LDS
        // (patch 80.8 KB): from global memory that was 291 us (header), in registers 144 + 72 staging registers do not fit 256.
        constexpr int S2_D = 3;
        f32x4 av[36], bv[36][NT];
#define S2_READ(S)                                                                                \
        do {                                                                                      \
            const int c_ = (S) / 9, tap_ = (S) % 9, ky_ = tap_ / 3, kx_ = tap_ % 3;               \
            av[S] = *reinterpret_cast<const f32x4 *>(patch + abase + (ky_ * S2_PW + kx_) * S2_PIXP + 8 * c_); \
            _Pragma("unroll") for (int n = 0; n < NT; ++n)                                        \
                bv[S][n] = *reinterpret_cast<const f32x4 *>(wts + ((c_ * 9 + tap_) * 2 * BN) * 4 + bbase + n * 128); \
        } while (0)
#pragma unroll
        for (int s_ = 0; s_ < S2_D; ++s_) S2_READ(s_);
#pragma unroll
        for (int s_ = 0; s_ < 36; ++s_) {
            if (s_ + S2_D < 36) S2_READ(s_ + S2_D);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    if (S2_ABL_CT & 1) acc[n][(s_ + j) & 15] += bv[s_][n][j] * av[s_][j];
                    else acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[s_][n][j], av[s_][j], acc[n], 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
#undef S2_READ
        // epilogue: lane & 31 = pixel (2 rows x 16 columns of the wave), registers 4 g .. 4 g + 3 = channels 8 g + 4 hh + {0..3}
        int t_ = tile;
        const int tx = t_ % tiles_x;
        t_ /= tiles_x;
        const int b = t_ / tiles_y;
        const int oy = (t_ - b * tiles_y) * 8 + wave * 2 + prow, ox = tx * 16 + pcol;
        if (oy < p.Ho && ox < p.Wo && (!(S2_ABL_CT & 4) || acc[0][0] == 12345.f)) {
            float *orow = p.out + ((size_t)(b * p.Ho + oy) * p.Wo + ox) * p.out_stride + n0;
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (n0 + n * 32 + 8 * g + 4 * hh >= p.cout_store) continue;
                    f32x4 v = {acc[n][4 * g + 0], acc[n][4 * g + 1], acc[n][4 * g + 2], acc[n][4 * g + 3]};
                    v += bias4[n][g];
                    if (p.lrelu) {
                        v[0] = lrelu01(v[0]); v[1] = lrelu01(v[1]); v[2] = lrelu01(v[2]); v[3] = lrelu01(v[3]);
                    }
                    *reinterpret_cast<f32x4 *>(orow + n * 32 + 8 * g + 4 * hh) = v;
                }
        }
    }
#undef S2_LOAD
}

// One instantiation (32 NT output channels, the layer's): plan = its descriptor bound (-1: beyond it), run = one persistent workgroup per CU
template <int NT>
struct launch_s2 {
    static size_t lds_bytes(const ConvParams &) { return ((size_t)S2_NPIX * S2_PIXP + (size_t)4 * 9 * 2 * 32 * NT * 4) * sizeof(float); }
    static dim3 grid(const ConvParams &p) { return dim3((unsigned)std::min<long>((long)cdiv(p.Wo, 16) * cdiv(p.Ho, 8) * p.B, device_cus()), 1); }
    static int plan(const ConvParams &p, ConvPlan &pl)
    {
        if ((size_t)S2_PH * p.W * p.seg[0].stride * 4 >= 0x7fffffffull) return -1;       // one patch inside a descriptor's 2 GiB
        pl = ConvPlan{PIVLFN_CONV_PLAN_S2, 8, 32 * NT, 0, 1};
        return PIVLFN_OK;
    }
    static int run(const ConvParams &p, hipStream_t st) { return conv_run_d<launch_s2>(conv_s2c32_kernel<NT>, 160 * 1024, p, st); }
};

// Applies to: 3 x 3, stride 2, pad 1, one source of exactly 32 channels, 32 or 64 output channels, no residual, and (per image, never
// a function of the batch) at least 256 tiles of 8 x 16 outputs.
bool choose_conv_s2(const ConvParams &p, ConvChoiceD &ch)
{
    if (p.KH != 3 || p.KW != 3 || p.S != 2 || p.padY != 1 || p.padX != 1 || p.nseg != 1 || p.seg[0].cload != 32 || p.nchunk != 4 || p.tail ||
        p.res || (p.cout_pad != 32 && p.cout_pad != 64) || (PIV_KNOB(1) & 4194304))
        return false;
    if ((long)cdiv(p.Wo, 16) * cdiv(p.Ho, 8) < 256) return false;
    return (p.cout_pad == 32 ? conv_take<launch_s2<1>>(p, ch) : conv_take<launch_s2<2>>(p, ch)) == PIVLFN_OK;
}

}  // namespace pivlfn
