// Stereo calibration on the device (gfx950): template matching of a calibration target, marker centres from the correlation map and
// the image dewarp.  Reference: stereo/matching.py:32-75 (template_matching, findLocalMax), stereo/dewarp.py:196-270 (warp, nl_trans).
// Arithmetic contracts: include/pivlfn.h.  Every sum here is an integer (order-independent) and every floating-point operation is
// fp64, rounded on its own: the results do not depend on the tiling, the batch or the order the atomics arrive in.
#include <cmath>
#include "common.h"

namespace pivlfn {

// ---- (a) zero-mean normalised cross-correlation ---------------------------------------------------------------------------------------
// A workgroup of 256 computes TM_TX x TM_TY outputs from one staged tile (outputs + halo, zero outside the image).  The tile is kept
// as bytes in rows of `pitch` bytes.  A lane owns TM_R vertically adjacent outputs and walks the th + TM_R - 1 tile rows under them
// once: four taps at a time, dword (x >> 2) + k of the row realigned by x & 3 with v_alignbyte, then v_dot4_u32_u8 against the
// template row each of its outputs sees in that tile row (I.T), and I.I and I.1 once per row for all of them.  A wave is 64
// consecutive x: its 64 dword reads of a row are 16-17 consecutive dwords, each broadcast to four lanes -- no bank conflict.  The
// template arrives packed the same way, four taps per dword with zero padding, TM_R - 1 zero rows above and below it (a tile row outside
// an output's window meets a zero row), through wave-uniform indices: scalar loads.
constexpr int TM_TX = 64, TM_R = 4, TM_TY = 4 * TM_R;

static inline int tm_nk(int tw) { return (tw + 3) / 4; }
static inline int tm_pitch(int tw) { return TM_TX + 4 * tm_nk(tw); }                 // bytes: 16 + nk dwords, the last one read by k = nk - 1 only
static inline size_t tm_lds(int th, int tw) { return (size_t)(TM_TY + th - 1) * tm_pitch(tw); }

size_t template_match_workspace_bytes(int th, int tw)
{
    if (th <= 0 || tw <= 0 || (long)th * tw > 65025) return 0;
    return ((size_t)(th + 2 * (TM_R - 1)) * tm_nk(tw) + 2) * sizeof(unsigned);
}

// tp[TM_R - 1 + th + TM_R - 1][nk] packed taps (zero rows first and last), then sum T and sum T^2.  One workgroup.
__global__ __launch_bounds__(256) void template_pack_kernel(const unsigned char *__restrict__ t, unsigned *__restrict__ tp, int th, int tw, int nk)
{
    __shared__ unsigned tot[2];
    if (threadIdx.x < 2) tot[threadIdx.x] = 0u;
    __syncthreads();
    unsigned s = 0u, ss = 0u;
    const int rows = th + 2 * (TM_R - 1);
    for (int i = threadIdx.x; i < rows * nk; i += 256) {
        const int ry = i / nk, k = i - ry * nk, ty = ry - (TM_R - 1);
        unsigned v = 0u;
        if (ty >= 0 && ty < th)
            for (int j = 0; j < 4; ++j) {
                const int x = 4 * k + j;
                if (x < tw) {
                    const unsigned b = t[(size_t)ty * tw + x];
                    v |= b << (8 * j);
                    s += b;
                    ss += b * b;
                }
            }
        tp[i] = v;
    }
    atomicAdd(&tot[0], s);
    atomicAdd(&tot[1], ss);
    __syncthreads();
    if (threadIdx.x < 2) tp[rows * nk + threadIdx.x] = tot[threadIdx.x];
}

__device__ __forceinline__ unsigned dot4(unsigned a, unsigned b, unsigned c)
{
#if __has_builtin(__builtin_amdgcn_udot4)
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    return c + (a & 255u) * (b & 255u) + ((a >> 8) & 255u) * ((b >> 8) & 255u) + ((a >> 16) & 255u) * ((b >> 16) & 255u) + (a >> 24) * (b >> 24);
#endif
}

struct TmParams { int H, W, th, tw, nk, pitch, rows; };

__global__ __launch_bounds__(256) void template_match_kernel(const unsigned char *__restrict__ images, const unsigned *__restrict__ tp,
                                                             float *__restrict__ rout, const TmParams p)
{
    extern __shared__ unsigned tm_tile[];
    unsigned char *tb = reinterpret_cast<unsigned char *>(tm_tile);
    const int ph = (p.th - 1) / 2, pw = (p.tw - 1) / 2;
    const int bx0 = (int)blockIdx.x * TM_TX - pw, by0 = (int)blockIdx.y * TM_TY - ph;
    const unsigned char *img = images + (size_t)blockIdx.z * p.H * p.W;
    const int used = TM_TX + p.tw - 1;
    for (int i = threadIdx.x; i < p.rows * p.pitch; i += 256) {
        const int ry = i / p.pitch, c = i - ry * p.pitch;
        const int gy = by0 + ry, gx = bx0 + c;
        unsigned char v = 0;
        if (c < used && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) v = img[(size_t)gy * p.W + gx];
        tb[i] = v;
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, ly0 = (int)(threadIdx.x >> 6) * TM_R;        // ly0: wave-uniform
    const int ox = (int)blockIdx.x * TM_TX + lx, oy0 = (int)blockIdx.y * TM_TY + ly0;
    if (oy0 >= p.H) return;
    const unsigned sh = (unsigned)lx & 3u;
    const int pitch4 = p.pitch >> 2, nk = p.nk;
    const unsigned tail = (p.tw & 3) ? ((1u << (8 * (p.tw & 3))) - 1u) : 0xFFFFFFFFu;
    const int trows = p.th + 2 * (TM_R - 1);
    const unsigned ST = tp[trows * nk], STT = tp[trows * nk + 1];
    unsigned sI[TM_R], sII[TM_R], sIT[TM_R];
#pragma unroll
    for (int o = 0; o < TM_R; ++o) sI[o] = sII[o] = sIT[o] = 0u;
    for (int ry = 0; ry < p.th + TM_R - 1; ++ry) {                                 // tile row ly0 + ry is template row ry - o of output o
        const unsigned *row = tm_tile + (ly0 + ry) * pitch4 + (lx >> 2);
        const unsigned *trow = tp + (ry + TM_R - 1) * nk;                         // output o reads the packed row ry - o + (TM_R - 1)
        unsigned lo = row[0], rI = 0u, rII = 0u;
        for (int k = 0; k < nk; ++k) {
            const unsigned hi = row[k + 1];
            unsigned v = __builtin_amdgcn_alignbyte(hi, lo, sh);
            lo = hi;
            if (k == nk - 1) v &= tail;
            rII = dot4(v, v, rII);
            rI = dot4(v, 0x01010101u, rI);
#pragma unroll
            for (int o = 0; o < TM_R; ++o) sIT[o] = dot4(v, trow[k - o * nk], sIT[o]);
        }
#pragma unroll
        for (int o = 0; o < TM_R; ++o)
            if (ry >= o && ry - o < p.th) { sI[o] += rI; sII[o] += rII; }
    }
    if (ox >= p.W) return;
    // integers below 2^53 in magnitude: the conversions to double are exact; product, root and quotient rounded once each
    const long long N = (long long)p.th * p.tw;
    const long long a = N * (long long)STT - (long long)ST * (long long)ST;
#pragma unroll
    for (int o = 0; o < TM_R; ++o) {
        if (oy0 + o >= p.H) break;
        const long long num = N * (long long)sIT[o] - (long long)sI[o] * (long long)ST;
        const long long b = N * (long long)sII[o] - (long long)sI[o] * (long long)sI[o];
        float r = 0.f;
        if (a != 0 && b != 0) {
            const double prod = (double)a * (double)b;
            r = (float)((double)num / sqrt(prod));
        }
        rout[(size_t)blockIdx.z * p.H * p.W + (size_t)(oy0 + o) * p.W + ox] = r;
    }
}

int launch_template_match(const unsigned char *images, const unsigned char *templ, float *r, int B, int H, int W, int th, int tw,
                          void *ws, size_t ws_bytes, hipStream_t st)
{
    PIV_REQUIRE(images && templ && r && ws, "template_match: null pointer");
    PIV_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "template_match: bad shape B=%d (1..65535) H=%d W=%d", B, H, W);
    PIV_REQUIRE((size_t)H * W < ((size_t)1 << 31) - 256 && cdiv(H, TM_TY) <= 65535,
                "template_match: H=%d x W=%d pixels exceed the 32-bit index range (H*W < 2^31 - 256, H <= %d)", H, W, 65535 * TM_TY);
    PIV_REQUIRE(th > 0 && tw > 0 && (th & 1) && (tw & 1), "template_match: template %d x %d must have odd sides", th, tw);
    PIV_REQUIRE((long)th * tw <= 65025, "template_match: template %d x %d has more than 65025 taps (32-bit window sums)", th, tw);
    const size_t lds = tm_lds(th, tw);
    PIV_REQUIRE(lds <= 160 * 1024, "template_match: template %d x %d needs a %zu-byte tile, more than the 160 KiB of local memory", th, tw, lds);
    PIV_REQUIRE(((uintptr_t)ws & 3) == 0 && ws_bytes >= template_match_workspace_bytes(th, tw),
                "template_match: workspace of %zu bytes, 4-byte aligned, needed (got %zu)", template_match_workspace_bytes(th, tw), ws_bytes);
    unsigned *tp = static_cast<unsigned *>(ws);
    hipLaunchKernelGGL(template_pack_kernel, dim3(1), dim3(256), 0, st, templ, tp, th, tw, tm_nk(tw));
    PIV_CHECK_HIP(hipGetLastError());
    static LdsAttr attr;
    if (lds > 64 * 1024)
        if (int rc = ensure_dyn_lds(attr, reinterpret_cast<const void *>(template_match_kernel), (int)lds)) return rc;
    const TmParams p{H, W, th, tw, tm_nk(tw), tm_pitch(tw), TM_TY + th - 1};
    hipLaunchKernelGGL(template_match_kernel, dim3(cdiv(W, TM_TX), cdiv(H, TM_TY), B), dim3(256), lds, st, images, tp, r, p);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

// ---- (b) marker centres: threshold, 2 x 2 box-sum, 4-connected labelling, per-component integer sums -------------------------------------
// Labelling is a union-find over the whole image in global memory (Playne & Hawick 2018 / Allegretti et al. 2019): every foreground
// pixel starts as its own root, the merge pass unites it with its left and upper neighbour by atomicMin on the larger root, the
// compress pass replaces every label by its root.  A root is always the smallest row-major index of its tree, so the final label is
// the smallest index of the component whatever the order of the merges.  Ranks of the roots (ascending) come from a three-step prefix
// count; the sums are 64-bit integer atomics.  Six launches, whatever the image holds.
constexpr int TP_BLOCK = 256;          // pixels per workgroup of every pass

struct TpWs { unsigned *w; int *slot; int *bcount; int nblk; };

size_t target_points_workspace_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0 || (size_t)H * W >= ((size_t)1 << 31)) return 0;
    const size_t hw = (size_t)H * W, nblk = (hw + TP_BLOCK - 1) / TP_BLOCK;
    return (size_t)B * (2 * hw + nblk) * 4;
}

static TpWs tp_carve(void *ws, int B, int H, int W)
{
    const size_t hw = (size_t)H * W, nblk = (hw + TP_BLOCK - 1) / TP_BLOCK;
    TpWs t;
    t.w = static_cast<unsigned *>(ws);
    t.slot = reinterpret_cast<int *>(t.w + (size_t)B * hw);
    t.bcount = t.slot + (size_t)B * hw;
    t.nblk = (int)nblk;
    return t;
}

__device__ __forceinline__ unsigned tp_q(const float *__restrict__ r, int y, int x, int W, float thr)
{
#pragma clang fp contract(off)
    const float v = r[(size_t)y * W + x];
    if (!(v > thr)) return 0u;                                    // NaN is not kept
    const double s = fmin((double)v, 8192.0) * 65536.0;           // q <= 2^29: the box-sum of four is at most 2^31
    return s > 0.0 ? (unsigned)(long long)rint(s) : 0u;
}

// w, labels = own index or -1, rec = 0 (first cap*4 words of every image), grid (nblk, B)
__global__ __launch_bounds__(TP_BLOCK) void tp_boxsum_kernel(const float *__restrict__ r, unsigned *__restrict__ w, int *__restrict__ lab,
                                                             long long *__restrict__ rec, int H, int W, float thr, int cap)
{
    const unsigned hw = (unsigned)H * (unsigned)W;
    const unsigned pix = blockIdx.x * TP_BLOCK + threadIdx.x;
    const size_t img = (size_t)blockIdx.y * hw;
    for (size_t i = (size_t)blockIdx.x * TP_BLOCK + threadIdx.x; i < (size_t)cap * 4; i += (size_t)gridDim.x * TP_BLOCK)
        rec[(size_t)blockIdx.y * cap * 4 + i] = 0;
    if (pix >= hw) return;
    const int y = (int)(pix / (unsigned)W), x = (int)(pix - (unsigned)y * (unsigned)W);
    const int ym = y > 0 ? y - 1 : (H > 1 ? 1 : 0), xm = x > 0 ? x - 1 : (W > 1 ? 1 : 0);      // index -1 reflected to +1
    const float *ri = r + img;
    const unsigned s = tp_q(ri, ym, xm, W, thr) + tp_q(ri, ym, x, W, thr) + tp_q(ri, y, xm, W, thr) + tp_q(ri, y, x, W, thr);
    w[img + pix] = s;
    lab[img + pix] = s ? (int)pix : -1;
}

__device__ __forceinline__ int tp_find(int *lab, int a)
{
    for (;;) {
        const int up = __atomic_load_n(lab + a, __ATOMIC_RELAXED);         // up <= a always: the walk ends at a root
        if (up == a) return a;
        a = up;
    }
}

__device__ __forceinline__ void tp_union(int *lab, int a, int b)
{
    for (;;) {
        a = tp_find(lab, a);
        b = tp_find(lab, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(lab + b, a);                              // b was a root when read: hang it under the smaller root
        if (old == b) return;
        b = old;                                                            // someone else re-rooted b first: unite with that root
    }
}

__global__ __launch_bounds__(TP_BLOCK) void tp_merge_kernel(int *__restrict__ lab, int H, int W)
{
    const unsigned hw = (unsigned)H * (unsigned)W;
    const unsigned pix = blockIdx.x * TP_BLOCK + threadIdx.x;
    if (pix >= hw) return;
    int *l = lab + (size_t)blockIdx.y * hw;
    if (__atomic_load_n(l + pix, __ATOMIC_RELAXED) < 0) return;
    const int y = (int)(pix / (unsigned)W), x = (int)(pix - (unsigned)y * (unsigned)W);
    if (x > 0 && __atomic_load_n(l + pix - 1, __ATOMIC_RELAXED) >= 0) tp_union(l, (int)pix, (int)pix - 1);
    if (y > 0 && __atomic_load_n(l + pix - W, __ATOMIC_RELAXED) >= 0) tp_union(l, (int)pix, (int)pix - W);
}

// labels -> roots; bcount[b][blk] = roots among this workgroup's pixels.  A root's label is already final, every other pixel writes
// only its own word: no pixel reads a word another one is writing a DIFFERENT final value to (the walk passes through labels that may
// be compressed meanwhile, and a compressed label still lies on the path to the same root).
__global__ __launch_bounds__(TP_BLOCK) void tp_compress_kernel(int *__restrict__ lab, int *__restrict__ bcount, int H, int W, int nblk)
{
    __shared__ int n;
    if (threadIdx.x == 0) n = 0;
    __syncthreads();
    const unsigned hw = (unsigned)H * (unsigned)W;
    const unsigned pix = blockIdx.x * TP_BLOCK + threadIdx.x;
    if (pix < hw) {
        int *l = lab + (size_t)blockIdx.y * hw;
        const int own = __atomic_load_n(l + pix, __ATOMIC_RELAXED);
        if (own == (int)pix) atomicAdd(&n, 1);
        else if (own >= 0) __atomic_store_n(l + pix, tp_find(l, own), __ATOMIC_RELAXED);
    }
    __syncthreads();
    if (threadIdx.x == 0) bcount[(size_t)blockIdx.y * nblk + blockIdx.x] = n;
}

// one workgroup per image: bcount -> exclusive prefix in place, count[b] = total
__global__ __launch_bounds__(256) void tp_scan_kernel(int *__restrict__ bcount, int *__restrict__ count, int nblk)
{
    __shared__ int part[256];
    int *bc = bcount + (size_t)blockIdx.x * nblk;
    const int per = (nblk + 255) / 256;
    const int lo = min((int)threadIdx.x * per, nblk), hi = min(lo + per, nblk);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += bc[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) { const int v = part[i]; part[i] = run; run += v; }
        count[blockIdx.x] = run;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int i = lo; i < hi; ++i) { const int v = bc[i]; bc[i] = run; run += v; }
}

// slot[root pixel] = its rank among the image's roots
__global__ __launch_bounds__(TP_BLOCK) void tp_slot_kernel(const int *__restrict__ lab, const int *__restrict__ bcount, int *__restrict__ slot,
                                                           int H, int W, int nblk)
{
    __shared__ int wave_n[TP_BLOCK / 64];
    const unsigned hw = (unsigned)H * (unsigned)W;
    const unsigned pix = blockIdx.x * TP_BLOCK + threadIdx.x;
    const size_t img = (size_t)blockIdx.y * hw;
    const bool root = pix < hw && lab[img + pix] == (int)pix;
    const unsigned long long vote = __ballot(root);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) wave_n[wv] = __popcll(vote);
    __syncthreads();
    if (!root) return;
    int rank = bcount[(size_t)blockIdx.y * nblk + blockIdx.x] + __popcll(vote & ((1ull << lane) - 1ull));
    for (int i = 0; i < wv; ++i) rank += wave_n[i];
    slot[img + pix] = rank;
}

__global__ __launch_bounds__(TP_BLOCK) void tp_sum_kernel(const int *__restrict__ lab, const unsigned *__restrict__ w, const int *__restrict__ slot,
                                                          long long *__restrict__ rec, int H, int W, int cap)
{
    const unsigned hw = (unsigned)H * (unsigned)W;
    const unsigned pix = blockIdx.x * TP_BLOCK + threadIdx.x;
    if (pix >= hw) return;
    const size_t img = (size_t)blockIdx.y * hw;
    const int root = lab[img + pix];
    if (root < 0) return;
    const int s = slot[img + root];
    if (s >= cap) return;
    const int y = (int)(pix / (unsigned)W), x = (int)(pix - (unsigned)y * (unsigned)W);
    unsigned long long *o = reinterpret_cast<unsigned long long *>(rec) + ((size_t)blockIdx.y * cap + s) * 4;
    const unsigned long long wv = w[img + pix];
    atomicAdd(o + 0, wv);
    atomicAdd(o + 1, wv * (unsigned long long)x);
    atomicAdd(o + 2, wv * (unsigned long long)y);
    atomicAdd(o + 3, 1ull);
}

int launch_target_points(const float *r, int B, int H, int W, float threshold, int cap, int *labels, int *count, long long *rec,
                         void *ws, size_t ws_bytes, hipStream_t st)
{
    PIV_REQUIRE(r && labels && count && rec && ws, "target_points: null pointer");
    PIV_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "target_points: bad shape B=%d (1..65535) H=%d W=%d", B, H, W);
    PIV_REQUIRE((size_t)H * W < ((size_t)1 << 31) - TP_BLOCK, "target_points: H=%d x W=%d pixels exceed the 32-bit index range", H, W);
    PIV_REQUIRE(cap > 0 && cap <= (1 << 24), "target_points: cap=%d must be 1..2^24", cap);
    PIV_REQUIRE(threshold == threshold, "target_points: threshold is NaN");
    PIV_REQUIRE(((uintptr_t)ws & 3) == 0 && ((uintptr_t)rec & 7) == 0 && ws_bytes >= target_points_workspace_bytes(B, H, W),
                "target_points: workspace of %zu bytes, 4-byte aligned, and an 8-byte aligned rec needed (got %zu bytes)",
                target_points_workspace_bytes(B, H, W), ws_bytes);
    const TpWs t = tp_carve(ws, B, H, W);
    const dim3 grid((unsigned)t.nblk, (unsigned)B), blk(TP_BLOCK);
    hipLaunchKernelGGL(tp_boxsum_kernel, grid, blk, 0, st, r, t.w, labels, rec, H, W, threshold, cap);
    hipLaunchKernelGGL(tp_merge_kernel, grid, blk, 0, st, labels, H, W);
    hipLaunchKernelGGL(tp_compress_kernel, grid, blk, 0, st, labels, t.bcount, H, W, t.nblk);
    hipLaunchKernelGGL(tp_scan_kernel, dim3((unsigned)B), dim3(256), 0, st, t.bcount, count, t.nblk);
    hipLaunchKernelGGL(tp_slot_kernel, grid, blk, 0, st, labels, t.bcount, t.slot, H, W, t.nblk);
    hipLaunchKernelGGL(tp_sum_kernel, grid, blk, 0, st, labels, t.w, t.slot, rec, H, W, cap);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

// ---- (c) dewarp ------------------------------------------------------------------------------------------------------------------------
struct DwParams {
    double A[24];
    double x0, y0, fill;
    int H, W, mode;
};

// nl_trans's numerators and denominators in numpy's evaluation order (stereo/dewarp.py:263-268; poly6 of stereo.hip in fp64)
__device__ __forceinline__ double poly6d(const double *A, double x, double y)
{
#pragma clang fp contract(off)
    return ((((A[0] * x + A[1] * y) + A[2]) + A[3] * (x * x)) + A[4] * (y * y)) + (A[5] * x) * y;
}

template <typename T> __device__ __forceinline__ T dw_cast(double v);
template <> __device__ __forceinline__ float dw_cast<float>(double v) { return (float)v; }
template <> __device__ __forceinline__ unsigned char dw_cast<unsigned char>(double v)
{
    const double r = rint(v);
    return (unsigned char)(r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r));         // a NaN compares false twice and converts to 0
}

template <typename T>
__global__ __launch_bounds__(256) void dewarp_kernel(const T *__restrict__ in, T *__restrict__ out, const DwParams p)
{
#pragma clang fp contract(off)
    const unsigned hw = (unsigned)p.H * (unsigned)p.W;
    const unsigned pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    const int y = (int)(pix / (unsigned)p.W), x = (int)(pix - (unsigned)y * (unsigned)p.W);
    const T *src = in + (size_t)blockIdx.y * hw;
    const double u = (double)x - p.x0, v = (double)y - p.y0;
    const double sx = poly6d(p.A, u, v) / poly6d(p.A + 6, u, v) + p.x0;
    const double sy = poly6d(p.A + 12, u, v) / poly6d(p.A + 18, u, v) + p.y0;
    T val = dw_cast<T>(p.fill);
    if (p.mode == PIVLFN_DEWARP_NEAREST) {
        const double rx = rint(sx), ry = rint(sy);                            // half to even, as np.round
        if (rx >= 0.0 && rx <= (double)(p.W - 1) && ry >= 0.0 && ry <= (double)(p.H - 1)) val = src[(size_t)(int)ry * p.W + (int)rx];
    } else {
        const double fx0 = floor(sx), fy0 = floor(sy);
        if (fx0 >= 0.0 && fx0 + 1.0 <= (double)(p.W - 1) && fy0 >= 0.0 && fy0 + 1.0 <= (double)(p.H - 1)) {
            const int ix = (int)fx0, iy = (int)fy0;
            const double ax = sx - fx0, ay = sy - fy0;
            const T *q = src + (size_t)iy * p.W + ix;
            const double top = (1.0 - ax) * (double)q[0] + ax * (double)q[1];
            const double bot = (1.0 - ax) * (double)q[p.W] + ax * (double)q[p.W + 1];
            val = dw_cast<T>((1.0 - ay) * top + ay * bot);
        }
    }
    out[(size_t)blockIdx.y * hw + pix] = val;
}

int launch_dewarp_frames(const void *frames, void *out, int is_f32, int B, int H, int W, const double *A, double x0, double y0, int mode,
                         double fill, hipStream_t st)
{
    PIV_REQUIRE(frames && out && A, "dewarp_frames: null pointer");
    PIV_REQUIRE(frames != out, "dewarp_frames: in place is not supported");
    PIV_REQUIRE(is_f32 == 0 || is_f32 == 1, "dewarp_frames: is_f32=%d (0 = uint8, 1 = float32)", is_f32);
    PIV_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "dewarp_frames: bad shape B=%d (1..65535) H=%d W=%d", B, H, W);
    PIV_REQUIRE((size_t)H * W < ((size_t)1 << 31) - 256, "dewarp_frames: H=%d x W=%d pixels exceed the 32-bit index range", H, W);
    PIV_REQUIRE(mode == PIVLFN_DEWARP_NEAREST || mode == PIVLFN_DEWARP_BILINEAR, "dewarp_frames: mode=%d (0 nearest, 1 bilinear)", mode);
    PIV_REQUIRE(std::isfinite(x0) && std::isfinite(y0), "dewarp_frames: the origin must be finite");
    for (int k = 0; k < 24; ++k) PIV_REQUIRE(std::isfinite(A[k]), "dewarp_frames: coefficient %d is not finite", k);
    if (is_f32) PIV_REQUIRE(fill != fill || std::fabs(fill) <= 3.4028234663852886e38, "dewarp_frames: fill=%g is beyond the fp32 range (a NaN is allowed)", fill);
    else PIV_REQUIRE(fill >= 0.0 && fill <= 255.0 && fill == std::floor(fill), "dewarp_frames: fill=%g must be an integer 0..255 for uint8 frames", fill);
    DwParams p;
    for (int k = 0; k < 24; ++k) p.A[k] = A[k];
    p.x0 = x0; p.y0 = y0; p.fill = fill; p.H = H; p.W = W; p.mode = mode;
    const dim3 grid((unsigned)(((size_t)H * W + 255) / 256), (unsigned)B);
    if (is_f32) hipLaunchKernelGGL(dewarp_kernel<float>, grid, dim3(256), 0, st, (const float *)frames, (float *)out, p);
    else hipLaunchKernelGGL(dewarp_kernel<unsigned char>, grid, dim3(256), 0, st, (const unsigned char *)frames, (unsigned char *)out, p);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
