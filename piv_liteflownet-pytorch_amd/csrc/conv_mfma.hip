// Direct (im2col-free) NHWC fp32 convolution on the gfx950 fp32 matrix cores.
//
// Covers every dense conv on the LiteFlowNet path (reference: torch.nn.Conv2d call sites in
// /root/reference/src/models.py:70-106, 124, 154-163, 197-207, 229-272): 3x3 s1/s2, 1x1, 7x7, kxk flow
// heads, (kx1)/(1xk) separable pairs; bias, optional LeakyReLU(0.1) and optional residual fused in the
// epilogue; up to three input sources so the concatenations of src/models.py:216 and :280 never
// materialise.
//
// Formulation: implicit GEMM  D[pixel][cout] = sum_{tap, cin} X[pixel+tap][cin] * W[cout][cin][tap]
//   * one workgroup = 4 waves = a TH x 32 output-pixel tile (TH = 4*MT rows) x BN = 32*NT channels;
//   * K is walked in chunks of 8 input channels: the (TH*S+KH-1) x (32*S+KW-1) x 8 input patch is staged
//     ONCE per chunk into LDS and reused by all KH*KW taps (this is what makes it im2col-free), together
//     with the chunk's [tap][8][BN] weight slab;
//   * v_mfma_f32_32x32x2_f32: A = 32 consecutive output pixels of one row, B = 32 output channels.
//     Each lane fetches 4 consecutive k with one ds_read_b128 and feeds them to 4 MFMAs, so MFMA j of a
//     chunk contracts input channels {j, 4+j}: a permutation of the k order inside a chunk, exact fp32
//     fma chains (the matrix core rounds once per product like fmaf).
//   * LDS pixel pitch is 12 floats (8 + 4 pad): the 16-lane groups of ds_read_b128 hit 16 distinct
//     16-byte slots, conflict-free at stride 1.
//   * accumulator layout (32x32): lane&31 = channel, so every epilogue store instruction writes two
//     full 128-byte channel runs.
#include "conv_direct.h"

namespace pivlfn {

template <int MT, int NT>
__global__ __launch_bounds__(256, 2) void conv_mfma_kernel(const ConvParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int BN = NT * 32;
    constexpr int TH = 4 * MT;
    const int taps = p.KH * p.KW;
    const int PH = (TH - 1) * p.S + p.KH;
    const int PW = 31 * p.S + p.KW;
    float *patch = smem;
    float *wts = smem + PH * PW * PIXP;

    const int tiles_x = (p.Wo + 31) >> 5;
    const int tiles_y = (p.Ho + TH - 1) / TH;
    int bid = blockIdx.x;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int b = bid / tiles_y;
    const int n0 = blockIdx.y * BN;
    const int x0 = tx * 32, y0 = ty * TH;
    const int ix0 = x0 * p.S - p.padX, iy0 = y0 * p.S - p.padY;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int row = lane & 31, hh = lane >> 5;

    f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

    int abase[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) abase[m] = ((wave * MT + m) * p.S * PW + row * p.S) * PIXP + hh * 4;
    const int bbase = (hh * BN + row) * 4;

    const int npix = PH * PW;
    const f32x4 *wsrc = reinterpret_cast<const f32x4 *>(p.wpk);
    int chunk = 0;
    for (int s = 0; s < p.nseg; ++s) {
        const float *sp = p.seg[s].ptr;
        const int scl = p.seg[s].cload, sst = p.seg[s].stride;
        for (int c0 = 0; c0 < scl; c0 += 8, ++chunk) {
            if (chunk) __syncthreads();
            for (int idx = tid; idx < npix * 2; idx += 256) {
                const int pix = idx >> 1, q = idx & 1;
                const int py = pix / PW, px = pix - py * PW;
                const int iy = iy0 + py, ix = ix0 + px, c = c0 + q * 4;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W && c < scl)
                    v = *reinterpret_cast<const f32x4 *>(sp + (size_t)((b * p.H + iy) * p.W + ix) * sst + c);
                *reinterpret_cast<f32x4 *>(patch + pix * PIXP + q * 4) = v;
            }
            const f32x4 *wc = wsrc + (size_t)chunk * taps * 2 * p.cout_pad + n0;
            for (int idx = tid; idx < taps * 2 * BN; idx += 256) {
                const int th = idx / BN, n = idx - th * BN;
                reinterpret_cast<f32x4 *>(wts)[idx] = wc[(size_t)th * p.cout_pad + n];
            }
            __syncthreads();
            int tap = 0;
            for (int ky = 0; ky < p.KH; ++ky) {
                for (int kx = 0; kx < p.KW; ++kx, ++tap) {
                    const int toff = (ky * PW + kx) * PIXP;
                    f32x4 a[MT], bq[NT];
#pragma unroll
                    for (int m = 0; m < MT; ++m) a[m] = *reinterpret_cast<const f32x4 *>(patch + abase[m] + toff);
#pragma unroll
                    for (int n = 0; n < NT; ++n)
                        bq[n] = *reinterpret_cast<const f32x4 *>(wts + tap * 2 * BN * 4 + bbase + n * 128);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int m = 0; m < MT; ++m)
#pragma unroll
                            for (int n = 0; n < NT; ++n)
                                acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][j], bq[n][j], acc[m][n], 0, 0, 0);
                }
            }
        }
    }

    // epilogue: bias, residual, activation, masked NHWC store
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int ch = n0 + n * 32 + row;
        if (ch >= p.cout_store) continue;
        const float bias = p.bias[ch];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int oy = y0 + wave * MT + m;
            if (oy >= p.Ho) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ox = x0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                if (ox >= p.Wo) continue;
                const size_t pix = (size_t)(b * p.Ho + oy) * p.Wo + ox;
                float v = acc[m][n][r] + bias;
                if (p.res) v += p.res[pix * p.res_stride + ch];
                if (p.lrelu) v = lrelu01(v);
                p.out[pix * p.out_stride + ch] = v;
            }
        }
    }
}

// ---- v2: same tiling, plus register prefetch ------------------------------------------------------------------------
// The next K-chunk's input patch and weight slab are loaded global -> registers BEFORE the current chunk's MFMAs and
// written to LDS after them, so the global/L2 latency hides behind the matrix work even with one workgroup per CU
// (the small pyramid levels, where v1 spent >90% of its time waiting on exposed staging).
// PMAX / WMAX = compile-time bounds on the 16-byte loads per thread for the patch / the weight slab.
// (64-accumulator tiles with the small staging class fit 168 VGPRs: three workgroups per CU)
template <int MT, int NT, int PMAX, int WMAX>
__global__ __launch_bounds__(256, (MT * NT <= 4 && NT <= 2 && PMAX <= 5) ? 3 : 2) void conv_mfma2_kernel(const ConvParams p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int BN = NT * 32;
    constexpr int TH = 4 * MT;
    const int taps = p.KH * p.KW;
    const int PH = (TH - 1) * p.S + p.KH;
    const int PW = 31 * p.S + p.KW;
    float *patch = smem;
    float *wts = smem + PH * PW * PIXP;

    const int tiles_x = (p.Wo + 31) >> 5;
    const int tiles_y = (p.Ho + TH - 1) / TH;
    int bid = blockIdx.x;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int b = bid / tiles_y;
    const int n0 = blockIdx.y * BN;
    const int x0 = tx * 32, y0 = ty * TH;
    const int ix0 = x0 * p.S - p.padX, iy0 = y0 * p.S - p.padY;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int row = lane & 31, hh = lane >> 5;

    f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

    int abase[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) abase[m] = ((wave * MT + m) * p.S * PW + row * p.S) * PIXP + hh * 4;
    const int bbase = (hh * BN + row) * 4;

    // this thread's staging slots: patch slot i covers (pixel, quad) = (idx>>1, idx&1), idx = tid + 256*i
    const int npix2 = PH * PW * 2;
    const int nw4 = taps * 2 * BN;
    // Staging loads are buffer loads through per-source, per-image descriptors: a slot outside the image (the zero padding) or past
    // the patch carries an out-of-range offset and the hardware's range check returns zeros -- no divergent branch around any load
    // (the predicated form cost an exec-mask save / branch / restore per load and turned the counted waits into vmcnt(0): on the
    // short K loops of NetC's stride-2 layers a quarter of a workgroup's time went into issuing them).
    // The descriptors start at the first image row of this workgroup's patch (64-bit scalar arithmetic): the 32-bit per-lane
    // offsets only span the patch rows, so one image of a source may be of any size (round 3: < 2 GiB).
    const int row0 = min(max(iy0, 0), p.H - 1);
    unsigned ppix[PMAX];       // index of the pixel relative to (row0, 0) of its image, C2OOB = zero
    int plds[PMAX];            // LDS float offset
#pragma unroll
    for (int i = 0; i < PMAX; ++i) {
        const int idx = tid + 256 * i;
        const int pix = idx >> 1, q = idx & 1;
        const int py = pix / PW, px = pix - py * PW;
        const int iy = iy0 + py, ix = ix0 + px;
        const bool ok = idx < npix2 && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        ppix[i] = ok ? (unsigned)((iy - row0) * p.W + ix) : C2OOB;      // relative to the descriptor's first row
        plds[i] = idx < npix2 ? pix * PIXP + q * 4 : -1;
    }
    const int q4 = (tid & 1) * 4;
    unsigned woff[WMAX];       // byte offset inside the chunk's slab, C2OOB = none
#pragma unroll
    for (int i = 0; i < WMAX; ++i) {
        const int idx = tid + 256 * i;
        const int th = idx / BN, n = idx - th * BN;
        woff[i] = idx < nw4 ? (unsigned)(th * p.cout_pad + n0 + n) * 16u : C2OOB;
    }
    const unsigned wchunk_bytes = (unsigned)taps * 2u * (unsigned)p.cout_pad * 16u;
    const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.wpk), 0, (unsigned)p.nchunk * wchunk_bytes, 0x00020000);

    f32x4 pr[PMAX], wr[WMAX];
    // this workgroup's K range: all chunks, or with split-K (gridDim.z > 1) an even share of the full chunks; the 4-channel
    // tail chunk, if any, goes to the last share
    const int nfull = p.nchunk - p.tail;
    const int nz = gridDim.z, kz = blockIdx.z;
    const int per = (nfull + nz - 1) / nz;
    const int kc0 = min(nfull, kz * per), kc1 = min(nfull, kc0 + per);
    const bool has_tail = p.tail && kz == nz - 1;
    const int kend = kc1 + (has_tail ? 1 : 0);
    int seg = 0, c0 = kc0 * 8;
    while (seg + 1 < p.nseg && c0 >= p.seg[seg].cload) { c0 -= (p.seg[seg].cload + 7) / 8 * 8; ++seg; }
    int scl = p.seg[seg].cload, sst = p.seg[seg].stride;
    const size_t img_px = (size_t)p.H * p.W;
    const size_t px_left = (size_t)(p.H - row0) * p.W - 1;          // pixels from the base to the last one of the image
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.seg[seg].ptr + ((size_t)b * img_px + (size_t)row0 * p.W) * sst), 0,
                                                                  (unsigned)min((px_left * sst + scl) * 4, (size_t)0x7fffffff), 0x00020000);
    unsigned pvo[PMAX];        // byte offset of the slot's 16 bytes inside the current source's image (pixel record + quad), C2OOB = zero
#pragma unroll
    for (int i = 0; i < PMAX; ++i) pvo[i] = ppix[i] != C2OOB ? ppix[i] * (unsigned)(sst * 4) + (unsigned)q4 * 4u : C2OOB;

#ifdef PIVLFN_STAMPS
#define CONV2_ABL(BIT) (PIV_DBG(p) & (BIT))
#else
#define CONV2_ABL(BIT) false
#endif
#define CONV2_LOAD(CH)                                                                            \
    do {                                                                                          \
        if (CONV2_ABL(2)) break;                                                                  \
        const unsigned back_ = (scl - c0 <= 4) ? (unsigned)q4 * 4u : 0u;      /* 4-channel tail: both quads fetch the same 16 bytes (an out-of-range offset stays out of range) */ \
        _Pragma("unroll") for (int i = 0; i < PMAX; ++i)                                          \
            pr[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(pvo[i] - back_), c0 * 4, 0)); \
        _Pragma("unroll") for (int i = 0; i < WMAX; ++i)                                          \
            wr[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsw, (int)woff[i], (int)((unsigned)(CH)*wchunk_bytes), 0)); \
    } while (0)

    // K loop.  A source whose channel count is 4 (mod 8) ends in a half chunk; the packer only allows that for the LAST
    // source, so the tail is peeled: the hot loop below stays branch-free, and the tail contracts its 4 channels with two
    // MFMAs per tap (k = {j, 2+j}; staged as [c0 c1 c2 c3 | c2 c3 0 0] so both lane halves read their pair at j = 0, 1).
    // phase stamps (tools/bench_ops.py conv_stamps --tune3 -1; only in a -DPIVLFN_STAMPS build: the accumulators cost
    // registers the shipped <2,4> and <2,2> tiles do not have)
#ifdef PIVLFN_STAMPS
    const bool stamp = p.stamps != nullptr && wave == 0 && blockIdx.y == 0 && blockIdx.z == 0;
    unsigned long long tk = 0, d_commit = 0, d_bar1 = 0, d_issue = 0, d_taps = 0, d_bar2 = 0, t_begin = 0;
#define STAMP(ACC)                                                                                \
    do {                                                                                          \
        if (stamp) {                                                                              \
            const unsigned long long now_ = __builtin_readcyclecounter();                         \
            ACC += now_ - tk;                                                                     \
            tk = now_;                                                                            \
        }                                                                                         \
    } while (0)
    if (stamp) t_begin = tk = __builtin_readcyclecounter();
#else
#define STAMP(ACC) do { } while (0)
#endif
    if (kc0 < kend) CONV2_LOAD(kc0);
    for (int chunk = kc0; chunk < kc1; ++chunk) {
        // registers -> LDS (waits for the loads of this chunk)
#pragma unroll
        for (int i = 0; i < PMAX; ++i)
            if (plds[i] >= 0) *reinterpret_cast<f32x4 *>(patch + plds[i]) = pr[i];
#pragma unroll
        for (int i = 0; i < WMAX; ++i)
            if (woff[i] != C2OOB) reinterpret_cast<f32x4 *>(wts)[tid + 256 * i] = wr[i];
        STAMP(d_commit);
        __syncthreads();
        STAMP(d_bar1);
        // advance to the next chunk's source and put its loads in flight
        if (chunk + 1 < kend) {
            c0 += 8;
            if (c0 >= scl) {
                ++seg;
                c0 = 0;
                scl = p.seg[seg].cload; sst = p.seg[seg].stride;
                rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.seg[seg].ptr + ((size_t)b * img_px + (size_t)row0 * p.W) * sst), 0,
                                                       (unsigned)min((px_left * sst + scl) * 4, (size_t)0x7fffffff), 0x00020000);
#pragma unroll
                for (int i = 0; i < PMAX; ++i) pvo[i] = ppix[i] != C2OOB ? ppix[i] * (unsigned)(sst * 4) + (unsigned)q4 * 4u : C2OOB;
            }
            CONV2_LOAD(chunk + 1);
        }
        STAMP(d_issue);
        int tap = 0;
        for (int ky = 0; ky < (CONV2_ABL(1) ? 0 : p.KH); ++ky) {
            for (int kx = 0; kx < p.KW; ++kx, ++tap) {
                const int toff = (ky * PW + kx) * PIXP;
                f32x4 a[MT], bq[NT];
#pragma unroll
                for (int m = 0; m < MT; ++m) a[m] = *reinterpret_cast<const f32x4 *>(patch + abase[m] + toff);
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    bq[n] = *reinterpret_cast<const f32x4 *>(wts + tap * 2 * BN * 4 + bbase + n * 128);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int n = 0; n < NT; ++n)
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[n][j], a[m][j], acc[m][n], 0, 0, 0);   // A = channels, B = pixels
            }
        }
        STAMP(d_taps);
        __syncthreads();       // all waves done with this chunk's LDS image before it is overwritten
        STAMP(d_bar2);
    }
#ifdef PIVLFN_STAMPS
    unsigned long long t_loop_end = 0;
    if (stamp) t_loop_end = __builtin_readcyclecounter();
#endif
    if (has_tail) {
#pragma unroll
        for (int i = 0; i < PMAX; ++i)
            if (plds[i] >= 0) {
                f32x4 v = pr[i];
                if (q4) v = f32x4{v[2], v[3], 0.f, 0.f};
                *reinterpret_cast<f32x4 *>(patch + plds[i]) = v;
            }
#pragma unroll
        for (int i = 0; i < WMAX; ++i)
            if (woff[i] != C2OOB) reinterpret_cast<f32x4 *>(wts)[tid + 256 * i] = wr[i];
        __syncthreads();
        int tap = 0;
        for (int ky = 0; ky < p.KH; ++ky) {
            for (int kx = 0; kx < p.KW; ++kx, ++tap) {
                const int toff = (ky * PW + kx) * PIXP;
                f32x2 a[MT], bq[NT];
#pragma unroll
                for (int m = 0; m < MT; ++m) a[m] = *reinterpret_cast<const f32x2 *>(patch + abase[m] + toff);
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    bq[n] = *reinterpret_cast<const f32x2 *>(wts + tap * 2 * BN * 4 + bbase + n * 128);
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int n = 0; n < NT; ++n)
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[n][j], a[m][j], acc[m][n], 0, 0, 0);
            }
        }
    }
#undef CONV2_LOAD

    // Epilogue.  With A = weights and B = pixels the accumulator tile is D[channel][pixel]: lane&31 = pixel, and registers
    // 4g..4g+3 hold channels 8g + 4*hh + {0,1,2,3} -- four consecutive channels per lane, so bias / residual / output move
    // as 16-byte vectors: 32 stores per thread for a 64x128 wave tile instead of 128, and a quarter of the address math.
    if (nz > 1) {       // split-K: raw partial sums, every channel of the padded N block, to scratch[kz][pixel][cout_pad]
        const int ox = x0 + row;
        const size_t npix = (size_t)p.B * p.Ho * p.Wo;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int oy = y0 + wave * MT + m;
            if (oy >= p.Ho || ox >= p.Wo) continue;
            float *prow = p.scratch + ((size_t)kz * npix + (size_t)(b * p.Ho + oy) * p.Wo + ox) * p.cout_pad + n0;
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<f32x4 *>(prow + n * 32 + 8 * g + 4 * hh) =
                        f32x4{acc[m][n][4 * g + 0], acc[m][n][4 * g + 1], acc[m][n][4 * g + 2], acc[m][n][4 * g + 3]};
        }
    } else {
        const int ox = x0 + row;
        const bool interior = x0 + 32 <= p.Wo && y0 + TH <= p.Ho && n0 + BN <= p.cout_store;   // workgroup-uniform fast path
        // all bias vectors of this lane first (the staging registers are dead by now): a load between two stores would wait for
        // the store in front of it -- vmcnt counts loads and stores in one order -- and serialise the whole epilogue
        f32x4 bias4[NT][4];
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int g = 0; g < 4; ++g) bias4[n][g] = *reinterpret_cast<const f32x4 *>(p.bias + n0 + n * 32 + 8 * g + 4 * hh);   // bias is padded to cout_pad
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int oy = y0 + wave * MT + m;
            const bool pix_ok = interior || (oy < p.Ho && ox < p.Wo);
            const size_t pix = (size_t)(b * p.Ho + (oy < p.Ho ? oy : 0)) * p.Wo + (ox < p.Wo ? ox : 0);
            float *orow = p.out + pix * p.out_stride;
            const float *rrow = p.res ? p.res + pix * p.res_stride : nullptr;
#pragma unroll
            for (int n = 0; n < NT; ++n) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ch = n0 + n * 32 + 8 * g + 4 * hh;
                    if (!pix_ok || (!interior && ch >= p.cout_store)) continue;
                    if (CONV2_ABL(4) && acc[m][n][0] != 12345.f) continue;
                    f32x4 v = {acc[m][n][4 * g + 0], acc[m][n][4 * g + 1], acc[m][n][4 * g + 2], acc[m][n][4 * g + 3]};
                    v += bias4[n][g];
                    if (rrow) v += *reinterpret_cast<const f32x4 *>(rrow + ch);
                    if (p.lrelu) {
                        v[0] = lrelu01(v[0]); v[1] = lrelu01(v[1]); v[2] = lrelu01(v[2]); v[3] = lrelu01(v[3]);
                    }
                    *reinterpret_cast<f32x4 *>(orow + ch) = v;
                }
            }
        }
    }
#ifdef PIVLFN_STAMPS
    if (stamp && lane == 0) {
        const unsigned long long t_end = __builtin_readcyclecounter();
        unsigned long long *o = p.stamps + (size_t)blockIdx.x * 8;
        o[0] = d_commit; o[1] = d_bar1; o[2] = d_issue; o[3] = d_taps; o[4] = d_bar2;
        o[5] = t_end - t_loop_end;       // (tail chunk +) epilogue
        o[6] = t_end - t_begin;
        o[7] = t_begin;
    }
#endif
#undef STAMP
}

// Second pass of a split-K layer: out = act(bias + residual + sum_z scratch[z]), z ascending (deterministic), 4 channels per thread.
__global__ __launch_bounds__(256) void conv_splitk_reduce_kernel(const ConvParams p, int nz)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int cq = p.cout_pad / 4;
    const long npix = (long)p.B * p.Ho * p.Wo;
    if (idx >= npix * cq) return;
    const long pix = idx / cq;
    const int ch = (int)(idx - pix * cq) * 4;
    if (ch >= p.cout_store) return;
    f32x4 v = *reinterpret_cast<const f32x4 *>(p.scratch + (size_t)pix * p.cout_pad + ch);
    for (int z = 1; z < nz; ++z) v += *reinterpret_cast<const f32x4 *>(p.scratch + ((size_t)z * npix + pix) * p.cout_pad + ch);
    v += *reinterpret_cast<const f32x4 *>(p.bias + ch);
    if (p.res) v += *reinterpret_cast<const f32x4 *>(p.res + (size_t)pix * p.res_stride + ch);
    if (p.lrelu) {
        v[0] = lrelu01(v[0]); v[1] = lrelu01(v[1]); v[2] = lrelu01(v[2]); v[3] = lrelu01(v[3]);
    }
    *reinterpret_cast<f32x4 *>(p.out + (size_t)pix * p.out_stride + ch) = v;
}

int launch_splitk_reduce(const ConvParams &p, int nz, hipStream_t st)
{
    const long items = (long)p.B * p.Ho * p.Wo * (p.cout_pad / 4);
    hipLaunchKernelGGL(conv_splitk_reduce_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, p, nz);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

// What one v1 / v2 workgroup needs for the input patch of a th x 32 tile and one K chunk's weight slab for bn channels: the LDS bytes,
// and v2's staging loads per thread (16 bytes each), pm for the patch and wm for the slab
struct TileNeeds { size_t lds; int pm, wm; };
static TileNeeds tile_needs(const ConvParams &p, int th, int bn)
{
    const int PH = (th - 1) * p.S + p.KH, PW = 31 * p.S + p.KW, taps = p.KH * p.KW;
    return {((size_t)PH * PW * PIXP + (size_t)taps * 2 * bn * 4) * sizeof(float), cdiv(PH * PW * 2, 256), cdiv(taps * 2 * bn, 256)};
}

// One v2 / v1 instantiation: plan = its LDS and staging bounds, run = the launch and, with split-K shares (p.ksplit, the plan's), the reduce pass
template <int MT, int NT, int PM, int WM>
struct launch_d2 {
    static constexpr int TH = 4 * MT, BN = NT * 32;
    static size_t lds_bytes(const ConvParams &p) { return tile_needs(p, TH, BN).lds; }
    static dim3 grid(const ConvParams &p) { return dim3(cdiv(p.Wo, 32) * cdiv(p.Ho, TH) * p.B, p.cout_pad / BN, std::max(p.ksplit, 1)); }
    static int plan(const ConvParams &p, ConvPlan &pl, int ksplit, bool say)
    {
        const TileNeeds n = tile_needs(p, TH, BN);
        PIV_REQUIRE_IF(say, n.lds <= 160 * 1024, "conv: LDS tile of %zu bytes exceeds 160 KiB (k=%dx%d s=%d)", n.lds, p.KH, p.KW, p.S);
        PIV_REQUIRE_IF(say, n.pm <= PM && n.wm <= WM, "conv: internal staging bound exceeded");
        pl = ConvPlan{PIVLFN_CONV_PLAN_V2, TH, BN, 100 * PM + WM, ksplit};
        return PIVLFN_OK;
    }
    static int run(const ConvParams &p, hipStream_t st)
    {
        if (int rc = conv_run_d<launch_d2>(conv_mfma2_kernel<MT, NT, PM, WM>, 160 * 1024, p, st)) return rc;
        return p.ksplit > 1 ? launch_splitk_reduce(p, p.ksplit, st) : PIVLFN_OK;
    }
};
template <int MT, int NT>
struct launch_d1 {
    static constexpr int TH = 4 * MT, BN = NT * 32;
    static size_t lds_bytes(const ConvParams &p) { return tile_needs(p, TH, BN).lds; }
    static dim3 grid(const ConvParams &p) { return dim3(cdiv(p.Wo, 32) * cdiv(p.Ho, TH) * p.B, p.cout_pad / BN); }
    static int plan(const ConvParams &p, ConvPlan &pl, bool say)
    {
        const size_t lds = lds_bytes(p);
        PIV_REQUIRE_IF(say, lds <= 160 * 1024, "conv: LDS tile of %zu bytes exceeds 160 KiB (k=%dx%d s=%d)", lds, p.KH, p.KW, p.S);
        pl = ConvPlan{PIVLFN_CONV_PLAN_V1, TH, BN, 0, 1};
        return PIVLFN_OK;
    }
    static int run(const ConvParams &p, hipStream_t st) { return conv_run_d<launch_d1>(conv_mfma_kernel<MT, NT>, 160 * 1024, p, st); }
};

// The compiled v2 instantiations of a row count and staging class by the policy's N tile: all four, or the two narrow ones.  What is not
// compiled is "not covered" (-1): no plan without a kernel.  (v1's eight: choose_conv1.  All of them: tests/test_conv_plan.py::COMPILED.)
template <int MT, int PM, int WM, class T>
static int take_nt2(int nt, T take) { return nt == 1 ? take(launch_d2<MT, 1, PM, WM>()) : nt == 2 ? take(launch_d2<MT, 2, PM, WM>()) : -1; }
template <int MT, int PM, int WM, class T>
static int take_nt4(int nt, T take) { return nt == 3 ? take(launch_d2<MT, 3, PM, WM>()) : nt == 4 ? take(launch_d2<MT, 4, PM, WM>()) : take_nt2<MT, PM, WM>(nt, take); }

// (Measured and dropped in round 2: a dedicated streaming kernel for the HBM-bound 1x1 layers -- NetC_ext 32 -> 64, moduleFeat
// 32 -> 128 -- with the whole weight matrix resident in LDS, operands read straight from global memory one pixel run ahead and no
// barriers: 193.7 vs 195.8 us (moduleFeat, level 1) and 216.7 vs 235.3 us (NetC_ext) against this kernel's 16-row tiles, and no
// change of the step time.  Both run at ~3.5 TB/s of a 4:1 write-heavy stream; tools/bench_ops.py conv --filter 1x1.)

// Tile choice for v2.  Staging loads per thread: patch = PH*PW*2/256, slab = taps*2*BN/256 (16-byte each).
// nt_cap / mt_cap bound the tile (4 / 4: the shipped policy).  Returns PIVLFN_OK with the plan, -1 when v2 does not cover the layer
// with that tile (the caller falls back to v1), or PIVLFN_ERR_ARG.
static int choose_conv2(const ConvParams &p, int nt_cap, int mt_cap, ConvChoiceD &ch, bool say)
{
    for (int s = 0; s < p.nseg; ++s)      // 32-bit byte offsets inside the rows of one patch (the descriptors are rebased per workgroup)
        PIV_REQUIRE_IF(say, (size_t)(15 * p.S + p.KH) * p.W * p.seg[s].stride * 4 < 0x7fffffffull, "conv: one patch (%d rows x %d x %d floats) of source %d exceeds the 2 GiB buffer-descriptor range", 15 * p.S + p.KH, p.W, p.seg[s].stride, s);
    // Split-K when one image has too few tiles for the chip and the K loop is long enough to be worth sharing.  Decided from
    // the per-image count of canonical (4 rows x 32 px x 32 channels) tiles only -- never from the batch size or from the tile
    // shape picked below (which does depend on it): a pair's flow must not depend on its batch mates, bit for bit.
    int ksplit = 1;
    {
        const int nfull = p.nchunk - p.tail;
        const long blocks1 = (long)cdiv(p.Wo, 32) * cdiv(p.Ho, 4) * (p.cout_pad / 32);
        if (p.scratch_floats && blocks1 <= 128 && nfull >= 4 && !(PIV_KNOB(1) & 128)) {
            ksplit = (int)std::min<long>(std::min(8, nfull / 2), std::max<long>(1, 512 / blocks1));
            if ((size_t)p.B * p.Ho * p.Wo * p.cout_pad * ksplit > p.scratch_floats) ksplit = 1;   // a scratch smaller than the batch needs
        }
    }
    const long px_blocks1 = (long)cdiv(p.Wo, 32) * cdiv(p.Ho, 4) * p.B;     // workgroups with MT = 1 per N block
    // widest N tile (32*nt channels) that still leaves >= 256 workgroups; with fewer the tile is narrowed so more CUs get
    // work (the input patch is then re-staged once per N block, which is cheap at the small levels where this happens)
    int nt = 1;
    for (int cand = std::min(4, nt_cap); cand >= 1; --cand) {
        if (p.cout_pad % (cand * 32)) continue;
        if (px_blocks1 * (p.cout_pad / (cand * 32)) >= 256 || cand == 1) { nt = cand; break; }
    }
    if ((PIV_KNOB(1) & 8) && nt == 4) nt = 2;              // A/B: 64-channel N tiles (three workgroups per CU) for 128-channel layers
    int mt = (px_blocks1 / 2) * (p.cout_pad / (nt * 32)) >= 512 && mt_cap >= 2 ? 2 : 1;
    const auto need = [&](int mt_, int nt_, int &pm, int &wm) { const TileNeeds n = tile_needs(p, 4 * mt_, 32 * nt_); pm = n.pm; wm = n.wm; };
    const auto take = [&](auto l) { return conv_take<decltype(l)>(p, ch, ksplit, say); };
    int pm, wm;
    // 16-row tiles for the 64-channel layers of the fine levels: the weight slab and the patch halo a workgroup restages per
    // K chunk are amortised over twice the pixels (same accumulator budget as the 8-row x 128-channel tile).  Measured at level 1:
    // 128->64 113 -> 129 TFLOP/s, 64->64 104 -> 119; the 32-channel layers LOSE with 16 rows (116 -> 96) and keep 8.
    if (nt == 2 && mt == 2 && mt_cap >= 4 && (px_blocks1 / 4) * (p.cout_pad / 64) >= 512 && !(PIV_KNOB(1) & 16)) {
        need(4, nt, pm, wm);
        if (pm <= 5 && wm <= 5) return take(launch_d2<4, 2, 5, 5>());
    }
    need(mt, nt, pm, wm);
    if ((pm > 3 || wm > 9) && mt == 2 && nt >= 3) { mt = 1; need(mt, nt, pm, wm); }   // keep the big-staging class under 256 VGPRs
    if (pm > 9 || wm > 13) return -1;      // not covered: caller falls back to v1
    const bool small = pm <= 3 && wm <= 9;
    // a middle staging class (<= 5 patch loads, <= 5 slab loads per thread) for the k x 1 layers of conv_dist_R (7 x 1: a 14-row
    // patch, 4 + 4 loads): 168 instead of 240 registers, three workgroups per CU instead of two
    const bool mid = !small && pm <= 5 && wm <= 5 && !(PIV_KNOB(1) & 4);
    if (mt == 2 && nt >= 3 && !small) return -1;
    if (small) return mt == 2 ? take_nt4<2, 3, 9>(nt, take) : take_nt4<1, 3, 9>(nt, take);
    if (mt == 2 && mid) return take_nt2<2, 5, 5>(nt, take);
    return mt == 2 ? take_nt2<2, 9, 13>(nt, take) : take_nt4<1, 9, 13>(nt, take);
}

// Tile choice for v1, the fallback for what v2's staging classes do not cover
static int choose_conv1(const ConvParams &p, ConvChoiceD &ch, bool say)
{
    PIV_REQUIRE_IF(say, !p.tail, "conv: this layer's weights are packed with a 4-channel tail chunk, which only the v2 kernel understands");
    const auto take = [&](auto l) { return conv_take<decltype(l)>(p, ch, say); };
    // Two output rows per wave (l2) when that still leaves a full chip's worth of workgroups, one (l1) otherwise
    const auto rows = [&](auto l2, auto l1) {
        constexpr int bn = decltype(l2)::BN;
        const long blocks2 = (long)cdiv(p.Wo, 32) * cdiv(p.Ho, 8) * p.B * (p.cout_pad / bn);
        const bool big = blocks2 >= 512 && (p.KH * p.KW <= 25 || bn == 32);
        return big && l2.lds_bytes(p) <= 160 * 1024 ? take(l2) : take(l1);      // a refusal must not depend on the batch
    };
    if (p.cout_pad % 128 == 0) return rows(launch_d1<2, 4>(), launch_d1<1, 4>());
    if (p.cout_pad % 96 == 0) return rows(launch_d1<2, 3>(), launch_d1<1, 3>());
    if (p.cout_pad % 64 == 0) return rows(launch_d1<2, 2>(), launch_d1<1, 2>());
    return rows(launch_d1<2, 1>(), launch_d1<1, 1>());
}

// Which kernel a call runs, from its geometry alone: no pointer is read and no device is touched.  A take names the launch function and
// its plan at once: pivlfn_conv2d_nhwc_plan reports what launch_conv launches.  p.scratch_floats > 0: a split-K scratch of that size exists.
static int choose_conv_d(const ConvParams &p, ConvChoiceD &ch)
{
    PIV_REQUIRE(p.nseg >= 1 && p.nseg <= 3, "conv: nseg=%d", p.nseg);
    PIV_REQUIRE(p.cout_pad % 32 == 0 && p.cout_store <= p.cout_pad, "conv: cout_pad=%d cout_store=%d", p.cout_pad, p.cout_store);
    PIV_REQUIRE(p.B > 0 && p.H > 0 && p.W > 0 && p.Ho > 0 && p.Wo > 0, "conv: empty shape");
    for (int s = 0; s < p.nseg; ++s)
        PIV_REQUIRE(p.seg[s].cload % 4 == 0 && p.seg[s].stride % 4 == 0, "conv: segment %d misaligned", s);
    if (!(PIV_KNOB(1) & 2)) {               // shipped path: v2 (register prefetch); knob bit 1 forces v1 for A/B
        if (choose_conv_c3k7(p, ch) || choose_conv_k1(p, false, ch) || choose_conv_s2(p, ch)) return PIVLFN_OK;
        const int rc = choose_conv2(p, 4, 4, ch, false);
        if (rc == PIVLFN_OK) return rc;
        if (rc == -1) {
            if (choose_conv1(p, ch, false) == PIVLFN_OK) return PIVLFN_OK;
            // Neither the tile v2 wants at this batch nor v1 (no 4-channel tail chunks, one LDS tile) takes the layer: a v2 tile of
            // fewer rows and channels may.  Same bits: the K order of an output does not depend on the tile.
            for (int cap = 4; cap >= 1; --cap)
                if (choose_conv2(p, cap, 1, ch, false) == PIVLFN_OK) return PIVLFN_OK;
        }
        // conv_k1 at any tile count before a refusal: it alone takes a 4-channel tail chunk of more than 52 taps, and an image row
        // beyond v2's descriptor range.  With these two steps every condition of a refusal is one of the geometry of a single image:
        // whether a call is accepted never depends on the batch.
        if (choose_conv_k1(p, true, ch)) return PIVLFN_OK;
        return rc == -1 ? choose_conv1(p, ch, true) : choose_conv2(p, 4, 4, ch, true);
    }
    return choose_conv1(p, ch, true);
}

int choose_conv(const ConvParams &p, ConvPlan &pl)
{
    ConvChoiceD ch;
    const int rc = choose_conv_d(p, ch);
    if (rc == PIVLFN_OK) pl = ch.pl;
    return rc;
}

int launch_conv(const ConvParams &p, hipStream_t st)
{
    ConvChoiceD ch;
    ConvParams q = p;
    if (!q.scratch) q.scratch_floats = 0;
    if (int rc = choose_conv_d(q, ch)) return rc;
    for (int s = 0; s < p.nseg; ++s) PIV_REQUIRE(p.seg[s].ptr, "conv: segment %d has no data", s);
    q.ksplit = ch.pl.ksplit;
    q.stamps = reinterpret_cast<unsigned long long *>(((unsigned long long)(unsigned)PIV_KNOB(6) << 32) | (unsigned)PIV_KNOB(5));   // tools only
    PIV_SET_DBG(q, PIV_KNOB(7));
    return ch.run(q, st);
}

}  // namespace pivlfn
