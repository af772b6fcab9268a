// Regularization's separable distance convolution of levels 1 and 2 -- (7 x 1) from 32 to 49 channels and (1 x 7) from 49 to 49 on 52
// stored lanes (conv_dist_R.0 / .1, /root/reference/src/models.py:253-261) -- with every fp32 operand split EXACTLY into three bf16
// pieces and the products formed on v_mfma_f32_16x16x32_bf16 (a K-32 step in ~16 cycles where v_mfma_f32_16x16x4_f32 needs 8 x 32).
//
// Structure: conv_col7_kernel / conv_row7_kernel of conv_head.hip, unchanged.  No LDS and no barrier; a wave owns 16 pixels across
// the walked axis (16 columns of a row for the 7 x 1 layer, 16 rows of a column for the 1 x 7 layer) and one 16-channel output block,
// walks 16 + 6 lines along the other axis, loads every line once through a buffer descriptor (out-of-range offsets read zeros: the
// padding) and feeds it to the seven outputs it belongs to -- the shift of a tap is a different accumulator, never a different lane.
// An accumulator starts from the bias and is stored, 16 bytes per lane, as soon as its seventh tap is in.  A workgroup walks four
// consecutive tiles and wave w takes block (w + i) & 3 of the i-th: block 3 is output channel 48 alone, an fp32 fmaf chain on the
// vector unit from the fp32 fragments of the fp32-instruction kernels (the same instructions in the same order as there).
//
// Arithmetic of blocks 0-2.  x = h + m + l exactly (bf16_split.h), once per loaded activation (5.5 instructions per value, reused by
// seven taps and 16 output channels per MFMA); the weights are split the same way at pack time.  A bf16 x bf16 product is exact in the
// fp32 the matrix core accumulates in, so u . v is the sum over piece pairs, of which the kernel forms TERMS, smallest products first:
//     6: lh, mm, hl, mh, hm, hh (weight piece, activation piece)   -- dropped: ml + lm + ll, about 2^-25 |u v| under RNE pieces
//     8: + lm, ml                                                  -- dropped: ll <= 2^-32 |u v|
//     9: all                                                       -- the exact product of the two fp32 numbers
// Operand layout of the instruction: lane l holds k = 8 (l >> 4) + j, j = 0..7, of column l & 15 (B, activations) or row l & 15 (A,
// weights); the accumulator is the 16x16x4 instruction's (lane holds channels 16 blk + 4 (l >> 4) .. + 3 of pixel l & 15).  K order,
// with kq = l >> 4, chosen so that a lane's eight values are the two 16-byte quads the fp32 kernels load:
//     step 0: j < 4 -> channel 4 kq + j, j >= 4 -> channel 16 + 4 kq + (j - 4)                      (both layers: channels 0..31)
//     step 1: j < 4 -> channel 32 + 4 kq + j, (kq, j) = (0, 4) -> channel 48, every other slot zero   (1 x 7 layer only)
// Lanes 49..51 of the 52-lane source are not defined by contract and are never loaded (a zero weight times NaN would be NaN); the empty
// slots of step 1 are constants in the kernel and zeros in the packed weights.
// Summation order per output: lines ascending (taps descending); per line the piece pairs in the order above, per pair step 0 then
// step 1; the hh products accumulate on the bias, all other pairs in a second accumulator that is added once, before the store (see
// there); the matrix core adds an instruction's 32 products in its own fixed order.  Independent of grid, tile phase and batch.
//
// Registers.  7 x 1: 7 taps x 3 pieces x 4 = 84 weight registers, two workgroups per CU as conv_col7_kernel.  1 x 7: 7 x 2 steps x 3 x 4
// = 168 weight registers + 64 of live accumulators + 39 of lines in flight + 48 of pieces (two lines: the next line is split under the
// current one's MFMAs) do not fit the 256 of two waves per SIMD: that instance is compiled for one workgroup per CU (512 registers).
#include <algorithm>
#include <vector>
#include "common.h"
#include "bf16_split.h"

namespace pivlfn {

struct DistB3Params {
    const float *x;
    const void *wb;         // pack_conv_dist_b3: [3 blocks][7 taps][steps][3 pieces][64 lanes][8] bf16
    const float *wf;        // the fp32 kernels' fragments (wpk_c / wpk_r): block 3 = output channel 48 replicated over the slots
    const float *wf12;      // 1 x 7: input channel 48's fragment (wpk_r12)
    const float *bias;
    float *out;
    int x_stride, out_stride, B, H, W;
};

// Measured at 1024 x 1024 (tools/bench_dist.py --b3 6, same box): the shipped values 188 / 279 us (7 x 1 / 1 x 7).
//   * 7 x 1 at one workgroup per CU with eight lines in flight, 1 x 7 with six: 184 / 285 -- the loads are not waited for;
//   * 32-line tiles (less halo, fewer tile starts): 175 / 270 at 1024^2, but 62 / 108 against 39 / 66 at 512^2 (too few workgroups);
//   * five / four lines in flight at two workgroups per CU: 180 / 279; a barrier in front of every tile (the four waves on the same
//     lines): 175 / 288; an MFMA-VALU-MFMA order asked of the scheduler in the one-wave 1 x 7 instance: 275-284;
//   * timing builds: no activation loads 97 / 237, no stores 120 / 233, neither 86 / 206.
#ifdef DIST_ABL_NOLOAD       // timing builds: every activation load / every store out of range (no memory access)
#define DIST_ABL_LOADCOND && H < 0
#else
#define DIST_ABL_LOADCOND
#endif
#ifdef DIST_ABL_NOSTORE
#define DIST_ABL_STORECOND && H < 0
#else
#define DIST_ABL_STORECOND
#endif
#ifndef DIST_T
#define DIST_T 16            // output lines of a tile along the walked axis
#endif
#ifndef DIST_COL_OCC
#define DIST_COL_OCC 2       // workgroups per CU the 7 x 1 instances are compiled for
#endif
#ifndef DIST_COL_AHEAD
#define DIST_COL_AHEAD 3     // lines loaded in front of their MFMAs
#endif
#ifndef DIST_ROW_AHEAD
#define DIST_ROW_AHEAD 2     // with three the 1 x 7 instances spill a register or two
#endif

template <bool ROW, int TERMS>
__global__ __launch_bounds__(256, ROW ? 1 : DIST_COL_OCC) void conv_dist_b3_kernel(const DistB3Params p)
{
    constexpr int K = 7, P = 3, T = DIST_T, NL = T + 2 * P, AHEAD = ROW ? DIST_ROW_AHEAD : DIST_COL_AHEAD;
    constexpr int NSTEP = ROW ? 2 : 1, NQ = ROW ? 3 : 2;      // K-32 steps; 16-byte quads a lane loads per line
    const int H = p.H, W = p.W, x_stride = p.x_stride, out_stride = p.out_stride;
    const int tiles_x = (W + (ROW ? T : 16) - 1) / (ROW ? T : 16), tiles_y = (H + (ROW ? 16 : T) - 1) / (ROW ? 16 : T);
    const int ntiles = tiles_x * tiles_y * p.B;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n16 = lane & 15, kq = lane >> 4;
#pragma unroll 1
    for (int ph = 0; ph < 4; ++ph) {
    int bid = xcd_remap(blockIdx.x, gridDim.x) * 4 + ph;
    if (bid >= ntiles) break;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int b = bid / tiles_y;
    const int blk = (wave + ph) & 3;                                 // 16-channel output block of this wave in this tile
    // lp: this lane's position on the axis the 16 pixels lie along (x for 7 x 1, y for 1 x 7); w0: first output line of the tile on the walked axis
    const int lp = (ROW ? ty : tx) * 16 + n16, w0 = (ROW ? tx : ty) * T;
    const int NW = ROW ? W : H;                                      // lines of the walked axis
    const bool lin = lp < (ROW ? H : W);
    const size_t img = (size_t)H * W;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.x + (size_t)b * img * x_stride), 0,
                                                                          (unsigned)(((img - 1) * x_stride + (ROW ? 52 : 32)) * sizeof(float)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rso = __builtin_amdgcn_make_buffer_rsrc(p.out + (size_t)b * img * out_stride, 0,
                                                                           (unsigned)(((img - 1) * out_stride + 52) * sizeof(float)), 0x00020000);
    const int ch = 16 * blk + 4 * kq;
    const bool chin = lin && ch < 52;
    f32x4 b4 = *reinterpret_cast<const f32x4 *>(p.bias + ch);
    if (blk == 3 && kq != 0) b4 = f32x4{0.f, 0.f, 0.f, 0.f};        // the vector path adds its four lane groups at the end: the bias once
    f32x4 acc[T];           // acc[i] is live from line i (its first tap) to line i + 6 (its store): seven or eight at a time
    f32x4 Bq[NL][NQ];
    float B12[NL];
    // out-of-range lines and pixels read zeros (offsets past the descriptor); channel 48 of the source is loaded by lane group kq = 0 only
#define DIST_LOAD(LI)                                                                             \
    do {                                                                                          \
        const int w_ = w0 - P + (LI);                                                             \
        const bool in_ = lin & (w_ >= 0) & (w_ < NW);                                             \
        const unsigned pix_ = (unsigned)((ROW ? lp * W + w_ : w_ * W + lp) * x_stride) * 4u;      \
        const unsigned off_ = (in_ DIST_ABL_LOADCOND) ? pix_ + 16u * kq : WOOB;                   \
        _Pragma("unroll") for (int g = 0; g < NQ; ++g)                                            \
            Bq[LI][g] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off_, 64 * g, 0)); \
        if (ROW) {                                                                                \
            const unsigned o12_ = (in_ & (kq == 0)) ? pix_ + 192u : WOOB;                         \
            B12[LI] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)o12_, 0, 0)); \
        }                                                                                         \
    } while (0)
#define DIST_STORE(XO)                                                                            \
    do {                                                                                          \
        const int wo_ = w0 + (XO);                                                                \
        const unsigned off = (chin && wo_ < NW DIST_ABL_STORECOND) ? (unsigned)((ROW ? lp * W + wo_ : wo_ * W + lp) * out_stride + ch) * 4u : WOOB; \
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[XO]), rso, (int)off, 0, 0); \
    } while (0)
    if (blk == 3) {
        // Output channel 48 on the vector unit: a fourth MFMA block would spend 15 of its 16 rows on padding.  The fragment registers hold
        // that channel's fp32 weights (replicated over the slots at pack time), every lane multiplies its channels of the line, the four
        // channel groups of a pixel are added across lanes at the end.
        f32x4 A[K][NQ];
        float A12[K];
#pragma unroll
        for (int t = 0; t < K; ++t) {
#pragma unroll
            for (int g = 0; g < NQ; ++g) A[t][g] = *reinterpret_cast<const f32x4 *>(p.wf + (((3 * K + t) * NQ + g) * 64 + lane) * 4);
            if (ROW) A12[t] = p.wf12[(3 * K + t) * 64 + lane];
        }
#pragma unroll
        for (int li = 0; li < AHEAD; ++li) DIST_LOAD(li);
#pragma unroll
        for (int li = 0; li < NL; ++li) {
            if (li + AHEAD < NL) DIST_LOAD(li + AHEAD);
            if (li < T) acc[li] = b4;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < K; ++t) {
                const int xo = li - t;
                if (xo < 0 || xo >= T) continue;
                float e = acc[xo][0];
#pragma unroll
                for (int g = 0; g < NQ; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) e = fmaf(A[t][g][j], Bq[li][g][j], e);
                if (ROW) e = fmaf(A12[t], B12[li], e);
                acc[xo][0] = e;
            }
            if (li >= K - 1) {                     // output line li - 6 is complete
                const int xo = li - (K - 1);
                float e = acc[xo][0];              // channel groups kq = 0..3 of a pixel live in lanes l, l+16, l+32, l+48: add them (fixed order)
                e = e + __shfl_xor(e, 16);
                e = e + __shfl_xor(e, 32);
                acc[xo] = f32x4{e, 0.f, 0.f, 0.f};
                DIST_STORE(xo);
            }
        }
    } else {
        u32x4 A[K][NSTEP][3];
#pragma unroll
        for (int t = 0; t < K; ++t)
#pragma unroll
            for (int s = 0; s < NSTEP; ++s)
#pragma unroll
                for (int pc = 0; pc < 3; ++pc)
                    A[t][s][pc] = *reinterpret_cast<const u32x4 *>(static_cast<const char *>(p.wb) + (size_t)(((((blk * K + t) * NSTEP + s) * 3 + pc) * 64 + lane) * 16));
        // Two accumulators per output.  What limits the accuracy is the fp32 rounding of the accumulator behind every MFMA, not the
        // products (exact) or the dropped pairs: one chain of 42 (84) instructions per output rounds as often as the fp32 instruction's
        // chain of 56 (91) and measured the same error against float64.  Only the hh products are of the output's magnitude; every
        // other pair is 2^-8 of it or less and goes to an accumulator of its own, whose roundings are 2^-8 of the output's ulp; the
        // main chain is 7 (14) instructions and one addition at the end.
        f32x4 accs[T];
        u32x4 X[2][NSTEP][3];       // [line parity][step][piece]: the next line is split under the current line's MFMAs
#define DIST_SPLIT(LI)                                                                            \
    do {                                                                                          \
        {                                                                                         \
            const float v_[8] = {Bq[LI][0][0], Bq[LI][0][1], Bq[LI][0][2], Bq[LI][0][3], Bq[LI][1][0], Bq[LI][1][1], Bq[LI][1][2], Bq[LI][1][3]}; \
            split8(v_, X[(LI)&1][0][0], X[(LI)&1][0][1], X[(LI)&1][0][2]);                        \
        }                                                                                         \
        if (ROW) {                                                                                \
            const float v_[8] = {Bq[LI][NQ - 1][0], Bq[LI][NQ - 1][1], Bq[LI][NQ - 1][2], Bq[LI][NQ - 1][3], B12[LI], 0.f, 0.f, 0.f}; \
            split8(v_, X[(LI)&1][NSTEP - 1][0], X[(LI)&1][NSTEP - 1][1], X[(LI)&1][NSTEP - 1][2]); \
        }                                                                                         \
    } while (0)
// one piece pair of a line: consecutive MFMAs target different accumulators
#define DIST_PAIR(ACC, LI, WP, XP)                                                                \
    _Pragma("unroll") for (int s = 0; s < NSTEP; ++s) _Pragma("unroll") for (int t = 0; t < K; ++t) { \
        const int xo = (LI) - t;                                                                  \
        if (xo < 0 || xo >= T) continue;                                                          \
        ACC[xo] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, A[t][s][WP]), __builtin_bit_cast(bf16x8, X[(LI)&1][s][XP]), ACC[xo], 0, 0, 0); \
    }
#pragma unroll
        for (int li = 0; li < AHEAD; ++li) DIST_LOAD(li);
        DIST_SPLIT(0);
#pragma unroll
        for (int li = 0; li < NL; ++li) {
            if (li + AHEAD < NL) DIST_LOAD(li + AHEAD);
            if (li < T) { acc[li] = b4; accs[li] = f32x4{0.f, 0.f, 0.f, 0.f}; }
            __builtin_amdgcn_sched_barrier(0);
            if (li + 1 < NL) DIST_SPLIT(li + 1);
            // (weight piece, activation piece), smallest products first; everything but hh goes to the second accumulator
            if (TERMS >= 9) { DIST_PAIR(accs, li, 2, 2); }
            if (TERMS >= 8) { DIST_PAIR(accs, li, 2, 1); DIST_PAIR(accs, li, 1, 2); }
            DIST_PAIR(accs, li, 2, 0); DIST_PAIR(accs, li, 1, 1); DIST_PAIR(accs, li, 0, 2);
            DIST_PAIR(accs, li, 1, 0); DIST_PAIR(accs, li, 0, 1); DIST_PAIR(acc, li, 0, 0);
            if (li >= K - 1) {                              // output line li - 6 is complete
                acc[li - (K - 1)] += accs[li - (K - 1)];
                DIST_STORE(li - (K - 1));
            }
        }
#undef DIST_SPLIT
#undef DIST_PAIR
    }
#undef DIST_LOAD
#undef DIST_STORE
    }       // tiles of the workgroup
}

// OIHW [49][cin][7 taps] (cin = 32: the 7 x 1 layer, one K-32 step; cin = 49: the 1 x 7 layer, two) -> the A fragments of blocks 0-2, each
// weight split into three bf16 pieces: [3 blocks][7 taps][steps][3 pieces][64 lanes][8], slot order as in the header
void pack_conv_dist_b3(const float *w, int cin, std::vector<unsigned short> &pk)
{
    const int nstep = cin == 32 ? 1 : 2;
    pk.assign((size_t)3 * 7 * nstep * 3 * 64 * 8, 0);
    for (int blk = 0; blk < 3; ++blk)
        for (int t = 0; t < 7; ++t)
            for (int s = 0; s < nstep; ++s)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int o = 16 * blk + (lane & 15), kq = lane >> 4;
                        int c;
                        if (s == 0) c = j < 4 ? 4 * kq + j : 16 + 4 * kq + (j - 4);
                        else c = j < 4 ? 32 + 4 * kq + j : (kq == 0 && j == 4 ? 48 : -1);
                        if (c < 0 || c >= cin) continue;
                        unsigned short pc[3];
                        bf16_split3(w[((size_t)o * cin + c) * 7 + t], pc);
                        for (int q = 0; q < 3; ++q) pk[((((((size_t)blk * 7 + t) * nstep + s) * 3 + q) * 64 + lane) * 8) + j] = pc[q];
                    }
}

// Tiles of a call: 16 pixels across the walked axis x DIST_T lines along it; a workgroup takes four
long conv_dist_b3_tiles(int row, int B, int H, int W) { return (long)cdiv(W, row ? DIST_T : 16) * cdiv(H, row ? 16 : DIST_T) * B; }
int conv_dist_b3_occupancy(int row) { return row ? 1 : DIST_COL_OCC; }

// What launch_conv_dist_b3 accepts, apart from its pointers: row = 0 the (7 x 1) 49 <- 32 layer, 1 the (1 x 7) 49 <- 49 one
int check_conv_dist_b3(int row, int x_stride, int out_stride, int terms, int B, int H, int W)
{
    PIV_REQUIRE(B > 0 && H > 0 && W > 0, "conv_dist_b3: bad arguments");
    PIV_REQUIRE(terms == 6 || terms == 8 || terms == 9, "conv_dist_b3: terms=%d (6, 8 or 9)", terms);
    PIV_REQUIRE(x_stride % 4 == 0 && x_stride >= (row ? 52 : 32) && out_stride % 4 == 0 && out_stride >= 52,
                "conv_dist_b3: %d staged lanes in and 52 stored lanes out (strides %d, %d)", row ? 52 : 32, x_stride, out_stride);
    PIV_REQUIRE((long)H * W * std::max(x_stride, out_stride) * 4 < (1L << 31), "conv_dist_b3: image exceeds 2 GiB (32-bit buffer offsets for the loads and the stores)");
    PIV_REQUIRE(conv_dist_b3_tiles(row, B, H, W) < (1L << 31), "conv_dist_b3: too many tiles");
    return PIVLFN_OK;
}

template <bool ROW>
static int launch_dist_t(const DistB3Params &p, int terms, hipStream_t st)
{
    const dim3 grid((unsigned)((conv_dist_b3_tiles(ROW, p.B, p.H, p.W) + 3) / 4));
    switch (terms) {
        case 6: hipLaunchKernelGGL((conv_dist_b3_kernel<ROW, 6>), grid, dim3(256), 0, st, p); break;
        case 8: hipLaunchKernelGGL((conv_dist_b3_kernel<ROW, 8>), grid, dim3(256), 0, st, p); break;
        default: hipLaunchKernelGGL((conv_dist_b3_kernel<ROW, 9>), grid, dim3(256), 0, st, p);
    }
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

// wb: pack_conv_dist_b3's fragments; wf (wf12): the fp32 kernels' (block 3 of them is read); bias: [64]
int launch_conv_dist_b3(int row, const float *x, int x_stride, const void *wb, const float *wf, const float *wf12, const float *bias,
                        float *out, int out_stride, int terms, int B, int H, int W, hipStream_t st)
{
    PIV_REQUIRE(x && wb && wf && (wf12 || !row) && bias && out, "conv_dist_b3: bad arguments");
    if (int rc = check_conv_dist_b3(row, x_stride, out_stride, terms, B, H, W)) return rc;
    const DistB3Params p{x, wb, wf, wf12, bias, out, x_stride, out_stride, B, H, W};
    return row ? launch_dist_t<true>(p, terms, st) : launch_dist_t<false>(p, terms, st);
}

}  // namespace pivlfn
