// Snapshot POD of a flow sequence (include/pivlfn.h "snapshot POD"): the fp64 Gram matrix of n fp32 snapshots on the fp64 matrix
// instruction v_mfma_f64_16x16x4_f64, and fp64 weighted sums of the snapshots (mean and spatial modes).
//
// Gram.  A workgroup of 4 waves owns one 64 x 64 block (bi <= bj) of G; wave w owns the 32 x 32 quarter (w >> 1, w & 1) as 2 x 2 MFMA
// tiles, so 4 independent accumulator chains cover the instruction's dependent latency.  P is walked in chunks of GR_KC = 64 floats:
// the 64 rows of block bi and the 64 of block bj are staged in LDS as fp32 (rows of GR_LD = 68 floats: a lane's read of row l & 15,
// column 4t + (l >> 4) then touches bank 4*row + k, all 64 different), the next chunk is already on its way to registers while the
// current one feeds 16 k-steps of 4 MFMAs per wave, and a value is widened to fp64 as it leaves LDS.  A slab is
// PIVLFN_GRAM_SLAB / GR_KC chunks chained into accumulators that start at +0.0; the slab sums are then added in slab order, by the
// workgroup itself (direct) or, where G has too few blocks to fill the device and the workspace may hold every slab sum, by
// gram_fold_kernel.  Either way G[i][j] = (((+0.0 + S_0) + S_1) + ...) with S_s the MFMA chain of slab s: the bits depend on P alone.
#include "launch_checks.h"

namespace pivlfn {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int GR_BLK = 64;                       // a workgroup's block of G is GR_BLK x GR_BLK
constexpr int GR_KC = 64;                        // floats of a row staged per chunk
constexpr int GR_LD = GR_KC + 4;                 // LDS row stride in floats: == 4 (mod 64), see above
constexpr int GR_THREADS = 256;
constexpr int GR_TILE = GR_BLK * GR_BLK;         // doubles of one block's slab sum in the workspace
constexpr int GR_CHUNKS = PIVLFN_GRAM_SLAB / GR_KC;
constexpr size_t GR_WS_CAP = (size_t)512 << 20;  // the slab sums go through the workspace only where they fit in this many bytes
constexpr int GR_SPLIT_BLOCKS = 512;             // ... and G has fewer blocks than this (two per CU)
static_assert(PIVLFN_GRAM_SLAB % GR_KC == 0, "a slab is a whole number of chunks");

struct GramParams {
    const float *X;
    double *G, *ws;
    long P, ldx;
    int n, nb, ntri, nslab, slabs_per_wg, direct, vec;
};

__device__ __forceinline__ void tri_block(int b, int nb, int &bi, int &bj)      // b-th block of the upper triangle, row by row
{
    bi = 0;
    while (b >= nb - bi) { b -= nb - bi; ++bi; }
    bj = bi + b;
}

// element (tile, reg) of lane `lane` of wave `wave`: row and column inside the 64 x 64 block (C/D map of the fp64 instruction:
// col = lane & 15, row = (lane >> 4) + 4 * reg)
__device__ __forceinline__ void frag_pos(int wave, int lane, int tile, int reg, int &r, int &c)
{
    r = (wave >> 1) * 32 + (tile >> 1) * 16 + (lane >> 4) + 4 * reg;
    c = (wave & 1) * 32 + (tile & 1) * 16 + (lane & 15);
}

__device__ __forceinline__ void write_mirrored(double *__restrict__ G, int n, int gi, int gj, double v)
{
    if (gi < n && gj < n && gi <= gj) {                    // the diagonal blocks' lower halves are not written from here: they are mirrored
        G[(size_t)gi * n + gj] = v;
        if (gi != gj) G[(size_t)gj * n + gi] = v;
    }
}

__global__ __launch_bounds__(GR_THREADS) void gram_kernel(const GramParams p)
{
    __shared__ __align__(16) float tile[2 * GR_BLK * GR_LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int bi, bj;
    tri_block(blockIdx.x, p.nb, bi, bj);
    const bool diag = bi == bj;
    const int nload = diag ? 4 : 8;                        // a diagonal block stages its 64 rows once and reads them as A and as B
    const int lc = t & 15, lr = t >> 4;                    // this thread loads floats 4*lc .. 4*lc+3 of rows lr, lr+16, ...

    // staged row r of the block pair -> row of X, or -1 for a row past n (staged as +0.0, never read)
    auto xrow = [&](int r) { const int g = (r < GR_BLK ? bi : bj) * GR_BLK + (r & (GR_BLK - 1)); return g < p.n ? g : -1; };

    float4 pre[8];
    auto fetch = [&](long p0) {
        const long c0 = p0 + 4 * lc;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            const int g = xrow(lr + 16 * i);
            if (i < nload && g >= 0 && c0 < p.P) {
                const float *src = p.X + (size_t)g * p.ldx + c0;
                if (p.vec && c0 + 3 < p.P) {
                    v = *reinterpret_cast<const float4 *>(src);
                } else {                                   // unaligned rows, and the ragged end of a row: nothing past column P is read
                    v.x = src[0];
                    if (c0 + 1 < p.P) v.y = src[1];
                    if (c0 + 2 < p.P) v.z = src[2];
                    if (c0 + 3 < p.P) v.w = src[3];
                }
            }
            pre[i] = v;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i < nload) *reinterpret_cast<float4 *>(&tile[(lr + 16 * i) * GR_LD + 4 * lc]) = pre[i];
    };

    const float *la0 = tile + ((wave >> 1) * 32 + (lane & 15)) * GR_LD + (lane >> 4);
    const float *lb0 = tile + ((diag ? 0 : GR_BLK) + (wave & 1) * 32 + (lane & 15)) * GR_LD + (lane >> 4);

    const d4 zero = {0.0, 0.0, 0.0, 0.0};
    d4 total[4] = {zero, zero, zero, zero};
    const int s_begin = blockIdx.y * p.slabs_per_wg;
    const int s_end = s_begin + p.slabs_per_wg < p.nslab ? s_begin + p.slabs_per_wg : p.nslab;
    for (int s = s_begin; s < s_end; ++s) {
        const long p_lo = (long)s * PIVLFN_GRAM_SLAB;
        const long left = p.P - p_lo;
        const int chunks = left >= PIVLFN_GRAM_SLAB ? GR_CHUNKS : (int)((left + GR_KC - 1) / GR_KC);
        d4 acc[4] = {zero, zero, zero, zero};
        fetch(p_lo);
        for (int c = 0; c < chunks; ++c) {
            __syncthreads();                               // the previous chunk has been read by every wave
            stage();
            __syncthreads();
            if (c + 1 < chunks) fetch(p_lo + (long)(c + 1) * GR_KC);
#pragma unroll 4
            for (int k = 0; k < GR_KC / 4; ++k) {          // ascending p: k-step k is columns 4k .. 4k+3 of the chunk
                const double a0 = (double)la0[4 * k], a1 = (double)la0[16 * GR_LD + 4 * k];
                const double b0 = (double)lb0[4 * k], b1 = (double)lb0[16 * GR_LD + 4 * k];
                acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[3], 0, 0, 0);
            }
        }
        if (p.direct) {
#pragma unroll
            for (int q = 0; q < 4; ++q) total[q] = total[q] + acc[q];
        } else {                                           // fragment order: coalesced here and in gram_fold_kernel
            double *dst = p.ws + ((size_t)s * p.ntri + blockIdx.x) * GR_TILE + wave * 1024 + lane;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) dst[(q * 4 + r) * 64] = acc[q][r];
        }
    }
    if (p.direct) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int br, bc;
                frag_pos(wave, lane, q, r, br, bc);
                write_mirrored(p.G, p.n, bi * GR_BLK + br, bj * GR_BLK + bc, total[q][r]);
            }
    }
}

__global__ __launch_bounds__(GR_THREADS) void gram_fold_kernel(const GramParams p)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int bi, bj;
    tri_block(blockIdx.x, p.nb, bi, bj);
    {
        const int e = blockIdx.y;                          // one of the 16 fragment elements per workgroup: 16 x the blocks in flight
        const double *src = p.ws + (size_t)blockIdx.x * GR_TILE + wave * 1024 + e * 64 + lane;
        double sum = 0.0;
        for (int s = 0; s < p.nslab; ++s) sum = sum + src[(size_t)s * p.ntri * GR_TILE];
        int br, bc;
        frag_pos(wave, lane, e >> 2, e & 3, br, bc);
        write_mirrored(p.G, p.n, bi * GR_BLK + br, bj * GR_BLK + bc, sum);
    }
}

// the launch plan is a function of (n, P) alone, so that the workspace query and the launch agree without a device
struct GramPlan { int nb, ntri, nslab; bool split; size_t ws_bytes; };

static bool gram_plan(int n, long P, GramPlan &g)
{
    if (n < 1 || n > PIVLFN_POD_MAX_SNAPSHOTS || P < 1 || P >= (1L << 31)) return false;
    g.nb = cdiv(n, GR_BLK);
    g.ntri = g.nb * (g.nb + 1) / 2;
    g.nslab = (int)((P + PIVLFN_GRAM_SLAB - 1) / PIVLFN_GRAM_SLAB);
    const size_t all = (size_t)g.nslab * g.ntri * GR_TILE * sizeof(double);
    g.split = g.nslab > 1 && g.ntri < GR_SPLIT_BLOCKS && all <= GR_WS_CAP;
    g.ws_bytes = g.split ? all : 256;
    return true;
}

size_t snapshot_gram_workspace_bytes(int n, long P)
{
    GramPlan g;
    return gram_plan(n, P, g) ? g.ws_bytes : 0;
}

int launch_snapshot_gram(const float *X, int n, long P, long ldx, double *G, void *ws, size_t ws_bytes, hipStream_t st)
{
    PIV_REQUIRE(X && G && ws, "snapshot_gram: null pointer (X, G and the workspace are required)");
    PIV_REQUIRE(n >= 1 && n <= PIVLFN_POD_MAX_SNAPSHOTS, "snapshot_gram: n=%d snapshots, must be 1..%d", n, PIVLFN_POD_MAX_SNAPSHOTS);
    PIV_REQUIRE(P >= 1 && P < (1L << 31), "snapshot_gram: P=%ld values per snapshot, must be 1..2^31-1", P);
    PIV_REQUIRE(ldx >= P, "snapshot_gram: row stride ldx=%ld is smaller than P=%ld", ldx, P);
    GramPlan g;
    gram_plan(n, P, g);
    if (int rc = check_workspace("snapshot_gram", ws, ws_bytes, g.ws_bytes, "n=%d P=%ld", n, P)) return rc;
    GramParams p;
    p.X = X; p.G = G; p.ws = (double *)ws; p.P = P; p.ldx = ldx; p.n = n;
    p.nb = g.nb; p.ntri = g.ntri; p.nslab = g.nslab;
    p.direct = g.split ? 0 : 1;
    p.slabs_per_wg = g.split ? 1 : g.nslab;
    p.vec = ((size_t)X & 15) == 0 && (ldx & 3) == 0;
    hipLaunchKernelGGL(gram_kernel, dim3((unsigned)g.ntri, (unsigned)(g.split ? g.nslab : 1)), dim3(GR_THREADS), 0, st, p);
    PIV_CHECK_HIP(hipGetLastError());
    if (g.split) {
        hipLaunchKernelGGL(gram_fold_kernel, dim3((unsigned)g.ntri, 16), dim3(GR_THREADS), 0, st, p);
        PIV_CHECK_HIP(hipGetLastError());
    }
    return PIVLFN_OK;
}

// ---- weighted sums: one lane per p with KT accumulators, X streamed once.  The weights of PJ_ROWS snapshots are staged in LDS, padded
// with zeros to KT columns, so the inner loop has no branch and every lane reads the same address (a broadcast).
constexpr int PJ_THREADS = 256;
constexpr int PJ_ROWS = 32;

template <int KT>
__global__ __launch_bounds__(PJ_THREADS) void project_kernel(const float *__restrict__ X, const double *__restrict__ Wt,
                                                             double *__restrict__ out, int n, long P, long ldx, int K)
{
#pragma clang fp contract(off)
    __shared__ __align__(16) double lw[PJ_ROWS * KT];
    const long col = (long)blockIdx.x * PJ_THREADS + threadIdx.x;
    const bool live = col < P;
    const float *x = X + (live ? col : 0);
    double acc[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) acc[k] = 0.0;
    for (int i0 = 0; i0 < n; i0 += PJ_ROWS) {
        __syncthreads();
        for (int e = threadIdx.x; e < PJ_ROWS * KT; e += PJ_THREADS) {
            const int r = i0 + e / KT, k = e % KT;
            lw[e] = (r < n && k < K) ? Wt[(size_t)r * K + k] : 0.0;
        }
        __syncthreads();
        if (!live) continue;
        const int rows = n - i0 < PJ_ROWS ? n - i0 : PJ_ROWS;
        int j = 0;
        for (; j + 4 <= rows; j += 4) {                    // four rows in flight per lane
            float xv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) xv[u] = x[(size_t)(i0 + j + u) * ldx];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double xd = (double)xv[u];
#pragma unroll
                for (int k = 0; k < KT; ++k) acc[k] = acc[k] + lw[(j + u) * KT + k] * xd;
            }
        }
        for (; j < rows; ++j) {
            const double xd = (double)x[(size_t)(i0 + j) * ldx];
#pragma unroll
            for (int k = 0; k < KT; ++k) acc[k] = acc[k] + lw[j * KT + k] * xd;
        }
    }
    if (live) {
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k < K) out[(size_t)k * P + col] = acc[k];
    }
}

int launch_snapshot_project(const float *X, int n, long P, long ldx, const double *Wt, int K, double *out, hipStream_t st)
{
    PIV_REQUIRE(X && Wt && out, "snapshot_project: null pointer (X, Wt and out are required)");
    PIV_REQUIRE(n >= 1 && n <= PIVLFN_POD_MAX_SNAPSHOTS, "snapshot_project: n=%d snapshots, must be 1..%d", n, PIVLFN_POD_MAX_SNAPSHOTS);
    PIV_REQUIRE(P >= 1 && P < (1L << 31), "snapshot_project: P=%ld values per snapshot, must be 1..2^31-1", P);
    PIV_REQUIRE(ldx >= P, "snapshot_project: row stride ldx=%ld is smaller than P=%ld", ldx, P);
    PIV_REQUIRE(K >= 1 && K <= 64, "snapshot_project: K=%d weight columns, must be 1..64", K);
    const dim3 grid((unsigned)((P + PJ_THREADS - 1) / PJ_THREADS));
    if (K <= 4)
        hipLaunchKernelGGL(project_kernel<4>, grid, dim3(PJ_THREADS), 0, st, X, Wt, out, n, P, ldx, K);
    else if (K <= 16)
        hipLaunchKernelGGL(project_kernel<16>, grid, dim3(PJ_THREADS), 0, st, X, Wt, out, n, P, ldx, K);
    else
        hipLaunchKernelGGL(project_kernel<64>, grid, dim3(PJ_THREADS), 0, st, X, Wt, out, n, P, ldx, K);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
