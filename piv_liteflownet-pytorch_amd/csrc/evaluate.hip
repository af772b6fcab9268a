// Scoring of flow batches against a known field (gfx950): the sums behind AEE, RMSE, mean L1 and bias of the reference's src/loss.py
// (EPE :12-21, L1 :24-38, L2 :41-55, MultiScale :86-148, LevelLoss :151-190), per pair and per pyramid level, and per-pixel error
// statistics of a sequence.  Reads [B,2,h,w] NCHW flows -- what estimate(..., tensor=True) returns, or the packed per-level buffer
// of pivlfn_forward -- and a [B,2,H,W] truth.  Arithmetic contract: include/pivlfn.h.
//
// Every sum is the root of one fixed 2 x 2 tree over the term map, so its bits depend on neither the launch geometry nor the batch.
// A workgroup owns one aligned 32 x 32 truth tile, which is a subtree at every pool exponent: it pools the truth once (fp64, the
// contract's order), scores every (level, stage) job on the pooled values, and leaves one 7-tuple per job; eval_finish_kernel
// continues the same tree over the tile grid, 16 x 16 nodes (four steps) per pass.
#include <cmath>
#include "launch_checks.h"

namespace pivlfn {

constexpr int EV_THREADS = 128;       // a 2 x 4 truth patch per thread: two 2 x 2 blocks, 16-byte loads along x
constexpr int EV_NSUM = 7;            // n, sum l1, sum epe, sum sq, sum du, sum dv, max epe
constexpr int EV_MAX_JOBS = 18;       // levels 6..1 x (M, S, R)
constexpr int EV_POOL = 256 + 64 + 16 + 4 + 1;      // pooled nodes of a tile at k = 1..5

struct EvalJob {
    const float *flow;      // [B,2,H >> k,W >> k]
    int k;
    int vec;                // k = 0 only: rows of this flow may be read 16 bytes at a time
};

struct EvalParams {
    const float *truth;             // [B,2,H,W]
    const unsigned char *mask;      // [B,H,W] or nullptr
    float *err_map;                 // [B,3,h,w] or nullptr (single job only)
    double *part;                   // [B][njobs][TY*TX][7]
    double div_flow;
    int H, W, TY, TX, njobs, kmax, vec;
    EvalJob job[EV_MAX_JOBS];
};

__device__ __forceinline__ bool unknown_truth(float x) { return !(fabsf(x) <= 1e9f); }      // NaN fails the comparison

__device__ __forceinline__ double nan_max(double a, double b)       // a NaN on either side stays
{
    return a != a ? a : (b != b ? b : (a > b ? a : b));
}

__device__ __forceinline__ int pool_offset(int s)      // first node of level s = 1..5 in the tile's pooled arrays
{
    return s == 1 ? 0 : s == 2 ? 256 : s == 3 ? 320 : s == 4 ? 336 : 340;
}

// The seven terms of one pixel.  pu, pv: the pooled truth, already scaled.  An excluded pixel is +0.0 in every sum and -inf in the max.
__device__ __forceinline__ void pixel_terms(float fu, float fv, double pu, double pv, bool ex, double t[EV_NSUM])
{
#pragma clang fp contract(off)
    const double du = (double)fu - pu, dv = (double)fv - pv;
    const double sq = du * du + dv * dv;
    const double epe = sqrt(sq);
    t[0] = ex ? 0.0 : 1.0;
    t[1] = ex ? 0.0 : fabs(du) + fabs(dv);
    t[2] = ex ? 0.0 : epe;
    t[3] = ex ? 0.0 : sq;
    t[4] = ex ? 0.0 : du;
    t[5] = ex ? 0.0 : dv;
    t[6] = ex ? -__builtin_inf() : epe;
}

__device__ __forceinline__ void store_err(float *e, size_t plane, size_t at, const double t[EV_NSUM], bool ex)
{
    const float nanf_ = __builtin_nanf("");
    e[at] = ex ? nanf_ : (float)t[4];
    e[plane + at] = ex ? nanf_ : (float)t[5];
    e[2 * plane + at] = ex ? nanf_ : (float)t[2];
}

// One node from its four children, (a + b) + (c + d) with a, b the upper row; slot 6 is the maximum.
__device__ __forceinline__ double tree_node(int q, double a, double b, double c, double d)
{
#pragma clang fp contract(off)
    return q == 6 ? nan_max(nan_max(a, b), nan_max(c, d)) : (a + b) + (c + d);
}

// red0 holds [7][side*side] terms; continues the tree to 1 x 1 between red0 and red1 and returns the buffer holding the [7] roots.
// All threads of the workgroup call it; it ends with a barrier.
__device__ __forceinline__ const double *tile_tree(double *red0, double *red1, int side)
{
    double *src = red0, *dst = red1;
    __syncthreads();
    while (side > 1) {
        const int m = side >> 1, mm = m * m, ss = side * side;
        for (int i = threadIdx.x; i < EV_NSUM * mm; i += EV_THREADS) {
            const int q = i / mm, r = i - q * mm, y = r / m, x = r - y * m;
            const double *s = src + q * ss + (2 * y) * side + 2 * x;
            dst[i] = tree_node(q, s[0], s[1], s[side], s[side + 1]);
        }
        __syncthreads();
        double *t = src;
        src = dst;
        dst = t;
        side = m;
    }
    return src;
}

__global__ __launch_bounds__(EV_THREADS) void eval_tiles_kernel(const EvalParams p)
{
#pragma clang fp contract(off)
    __shared__ double pool_u[EV_POOL], pool_v[EV_POOL];
    __shared__ unsigned char pool_x[EV_POOL];
    __shared__ double red0[EV_NSUM * 256], red1[EV_NSUM * 64];

    const int t = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    const int ty = tile / p.TX, tx = tile - ty * p.TX;
    const int py = t >> 3, px = t & 7;
    const int y0 = ty * 32 + 2 * py, x0 = tx * 32 + 4 * px;
    const unsigned HW = (unsigned)p.H * (unsigned)p.W;
    const float *tu_p = p.truth + (size_t)b * 2 * HW, *tv_p = tu_p + HW;
    const unsigned char *mk = p.mask ? p.mask + (size_t)b * HW : nullptr;

    // the thread's 2 x 4 truth patch; a pixel outside the image counts as excluded
    float tu[2][4], tv[2][4];
    bool ex[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int y = y0 + r;
        const unsigned row = (unsigned)y * (unsigned)p.W + (unsigned)x0;
        if (y < p.H && p.vec && x0 + 3 < p.W) {
            const float4 a = *reinterpret_cast<const float4 *>(tu_p + row), c = *reinterpret_cast<const float4 *>(tv_p + row);
            tu[r][0] = a.x; tu[r][1] = a.y; tu[r][2] = a.z; tu[r][3] = a.w;
            tv[r][0] = c.x; tv[r][1] = c.y; tv[r][2] = c.z; tv[r][3] = c.w;
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) ex[r][c4] = false;
        } else {
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                const bool in = y < p.H && x0 + c4 < p.W;
                tu[r][c4] = in ? tu_p[row + c4] : 0.0f;
                tv[r][c4] = in ? tv_p[row + c4] : 0.0f;
                ex[r][c4] = !in;
            }
        }
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) {
            const bool in = !ex[r][c4];
            const bool m = in && mk && mk[row + c4] != 0;
            ex[r][c4] = !in || m || unknown_truth(tu[r][c4]) || unknown_truth(tv[r][c4]);
        }
    }

    // pooled truth of the tile for k = 1..kmax: step 1 from registers, the others from the level below
    if (p.kmax >= 1) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int at = py * 16 + 2 * px + j;
            pool_u[at] = ((double)tu[0][2 * j] + (double)tu[0][2 * j + 1]) + ((double)tu[1][2 * j] + (double)tu[1][2 * j + 1]);
            pool_v[at] = ((double)tv[0][2 * j] + (double)tv[0][2 * j + 1]) + ((double)tv[1][2 * j] + (double)tv[1][2 * j + 1]);
            pool_x[at] = ex[0][2 * j] || ex[0][2 * j + 1] || ex[1][2 * j] || ex[1][2 * j + 1];
        }
        for (int s = 2; s <= p.kmax; ++s) {
            __syncthreads();
            const int m = 32 >> s, n = 2 * m, src = pool_offset(s - 1), dst = pool_offset(s);
            for (int i = t; i < m * m; i += EV_THREADS) {
                const int y = i / m, x = i - y * m, a = src + (2 * y) * n + 2 * x;
                pool_u[dst + i] = (pool_u[a] + pool_u[a + 1]) + (pool_u[a + n] + pool_u[a + n + 1]);
                pool_v[dst + i] = (pool_v[a] + pool_v[a + 1]) + (pool_v[a + n] + pool_v[a + n + 1]);
                pool_x[dst + i] = pool_x[a] | pool_x[a + 1] | pool_x[a + n] | pool_x[a + n + 1];
            }
        }
    }

    for (int j = 0; j < p.njobs; ++j) {
        const EvalJob job = p.job[j];
        const int k = job.k, h = p.H >> k, w = p.W >> k;
        const unsigned hw = (unsigned)h * (unsigned)w;
        const float *fu_p = job.flow + (size_t)b * 2 * hw, *fv_p = fu_p + hw;
        float *em = p.err_map ? p.err_map + (size_t)b * 3 * hw : nullptr;
        int side;
        if (k == 0) {
            // terms of the 2 x 4 patch, then the first tree step in registers: two nodes of the tile's 16 x 16 map
            double node[2][EV_NSUM];
            double tm[2][4][EV_NSUM];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int y = y0 + r;
                const unsigned row = (unsigned)y * (unsigned)p.W + (unsigned)x0;
                float fu[4], fv[4];
                if (y < p.H && job.vec && x0 + 3 < p.W) {
                    const float4 a = *reinterpret_cast<const float4 *>(fu_p + row), c = *reinterpret_cast<const float4 *>(fv_p + row);
                    fu[0] = a.x; fu[1] = a.y; fu[2] = a.z; fu[3] = a.w;
                    fv[0] = c.x; fv[1] = c.y; fv[2] = c.z; fv[3] = c.w;
                } else {
#pragma unroll
                    for (int c4 = 0; c4 < 4; ++c4) {
                        const bool in = y < p.H && x0 + c4 < p.W;
                        fu[c4] = in ? fu_p[row + c4] : 0.0f;
                        fv[c4] = in ? fv_p[row + c4] : 0.0f;
                    }
                }
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) {
                    pixel_terms(fu[c4], fv[c4], (double)tu[r][c4] * p.div_flow, (double)tv[r][c4] * p.div_flow, ex[r][c4], tm[r][c4]);
                    if (em && y < p.H && x0 + c4 < p.W) store_err(em, hw, row + c4, tm[r][c4], ex[r][c4]);
                }
            }
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int q = 0; q < EV_NSUM; ++q)
                    node[jj][q] = tree_node(q, tm[0][2 * jj][q], tm[0][2 * jj + 1][q], tm[1][2 * jj][q], tm[1][2 * jj + 1][q]);
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int q = 0; q < EV_NSUM; ++q) red0[q * 256 + py * 16 + 2 * px + jj] = node[jj][q];
            side = 16;
        } else {
            const int ts = 32 >> k, off = pool_offset(k);
            const double inv = 1.0 / (double)(1 << (2 * k));        // a power of two: the division by 4^k, exact
            __syncthreads();                                        // the pooled arrays are complete
            for (int i = t; i < ts * ts; i += EV_THREADS) {
                const int y = i / ts, x = i - y * ts, gy = ty * ts + y, gx = tx * ts + x;
                const bool in = gy < h && gx < w;
                const unsigned at = in ? (unsigned)gy * (unsigned)w + (unsigned)gx : 0u;
                const bool exc = !in || pool_x[off + i] != 0;
                double tm[EV_NSUM];
                pixel_terms(fu_p[at], fv_p[at], (pool_u[off + i] * inv) * p.div_flow, (pool_v[off + i] * inv) * p.div_flow, exc, tm);
                if (em && in) store_err(em, hw, at, tm, exc);
#pragma unroll
                for (int q = 0; q < EV_NSUM; ++q) red0[q * ts * ts + i] = tm[q];
            }
            side = ts;
        }
        const double *root = tile_tree(red0, red1, side);
        if (t < EV_NSUM) p.part[(((size_t)b * p.njobs + j) * ((size_t)p.TY * p.TX) + tile) * EV_NSUM + t] = root[t];
        __syncthreads();            // the roots are read before the next job writes red0 / red1
    }
}

// One pass over a node grid src [nb][gy][gx][7]: every workgroup continues the tree over one aligned 16 x 16 block of nodes (absent
// nodes: +0.0, -inf for the maximum) and writes dst [nb][oy][ox][7].  The last pass (oy = ox = 1) writes the reported tuple:
// every sum + 0.0 (a -0.0 becomes +0.0), the maximum 0 when nothing was counted.
__global__ __launch_bounds__(EV_THREADS) void eval_finish_kernel(const double *__restrict__ src, double *__restrict__ dst, int gy, int gx,
                                                                 int oy, int ox, int last)
{
#pragma clang fp contract(off)
    __shared__ double red0[EV_NSUM * 256], red1[EV_NSUM * 64];
    const unsigned nodes = (unsigned)oy * (unsigned)ox;
    const unsigned jb = blockIdx.x / nodes, node = blockIdx.x - jb * nodes;
    const int ny = (int)(node / (unsigned)ox), nx = (int)(node - (unsigned)ny * (unsigned)ox);
    const double *s = src + (size_t)jb * gy * gx * EV_NSUM;
    for (int i = threadIdx.x; i < 256; i += EV_THREADS) {
        const int y = ny * 16 + (i >> 4), x = nx * 16 + (i & 15);
        const bool in = y < gy && x < gx;
        const double *e = s + ((size_t)(in ? y : 0) * gx + (in ? x : 0)) * EV_NSUM;
#pragma unroll
        for (int q = 0; q < EV_NSUM; ++q) red0[q * 256 + i] = in ? e[q] : (q == 6 ? -__builtin_inf() : 0.0);
    }
    const double *root = tile_tree(red0, red1, 16);
    if (threadIdx.x < EV_NSUM) {
        const int q = threadIdx.x;
        double v = root[q];
        if (last) v = q == 6 ? (root[0] == 0.0 ? 0.0 : v) : v + 0.0;
        dst[(size_t)blockIdx.x * EV_NSUM + q] = v;
    }
}

// acc [6,H,W] fp64 += (1, du, dv, du*du, dv*dv, epe) of frames 0..B-1 in frame order where the truth is known and the mask is 0
// (k = 0, div_flow = 1).  acc is read and written once per call, so any split of a sequence into calls gives the same bits.
__global__ __launch_bounds__(256) void error_stats_kernel(const float *__restrict__ flow, const float *__restrict__ truth,
                                                          const unsigned char *__restrict__ mask, double *__restrict__ acc, int B,
                                                          unsigned HW)
{
#pragma clang fp contract(off)
    for (unsigned pix = blockIdx.x * 256 + threadIdx.x; pix < HW; pix += gridDim.x * 256) {
        double s[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] = acc[(size_t)k * HW + pix];
        for (int b = 0; b < B; ++b) {
            const size_t at = (size_t)b * 2 * HW + pix;
            const float tu = truth[at], tv = truth[at + HW];
            if (unknown_truth(tu) || unknown_truth(tv) || (mask && mask[(size_t)b * HW + pix] != 0)) continue;
            const double du = (double)flow[at] - (double)tu, dv = (double)flow[at + HW] - (double)tv;
            s[0] = s[0] + 1.0;
            s[1] = s[1] + du;
            s[2] = s[2] + dv;
            s[3] = s[3] + du * du;
            s[4] = s[4] + dv * dv;
            s[5] = s[5] + sqrt(du * du + dv * dv);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[(size_t)k * HW + pix] = s[k];
    }
}

static size_t eval_tiles(int H, int W) { return (size_t)cdiv(H, 32) * (size_t)cdiv(W, 32); }
static size_t eval_tiles2(int H, int W) { return (size_t)cdiv(cdiv(H, 32), 16) * (size_t)cdiv(cdiv(W, 32), 16); }

size_t flow_errors_workspace_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const size_t bytes = (size_t)EV_MAX_JOBS * (size_t)B * (eval_tiles(H, W) + eval_tiles2(H, W)) * EV_NSUM * sizeof(double);
    return (bytes + 255) / 256 * 256;
}

// Host-side checks shared by the two scoring entry points.
static int eval_check(const char *what, const void *truth, const void *sums, const void *ws, size_t ws_bytes, int B, int H, int W,
                      double div_flow)
{
    PIV_REQUIRE(truth && sums && ws, "%s: null pointer (flows, truth, sums and the workspace are required)", what);
    if (int rc = check_shape(what, B, H, W, "pairs")) return rc;
    PIV_REQUIRE((size_t)B * EV_MAX_JOBS * eval_tiles(H, W) < ((size_t)1 << 31), "%s: B=%d pairs of %d x %d are too many tiles for one call",
                what, B, H, W);
    PIV_REQUIRE(std::isfinite(div_flow), "%s: div_flow=%g must be finite", what, div_flow);
    return check_workspace(what, ws, ws_bytes, flow_errors_workspace_bytes(B, H, W), "B=%d H=%d W=%d", B, H, W);
}

static bool aligned16(const void *p, int w) { return ((size_t)p & 15) == 0 && (w & 3) == 0; }

static int eval_launch(EvalParams &p, int B, double *sums, void *ws, hipStream_t st)
{
    p.TY = cdiv(p.H, 32);
    p.TX = cdiv(p.W, 32);
    p.vec = aligned16(p.truth, p.W);
    double *bufA = (double *)ws, *bufB = bufA + (size_t)EV_MAX_JOBS * B * eval_tiles(p.H, p.W) * EV_NSUM;
    p.part = bufA;
    hipLaunchKernelGGL(eval_tiles_kernel, dim3((unsigned)(p.TY * p.TX), (unsigned)B), dim3(EV_THREADS), 0, st, p);
    PIV_CHECK_HIP(hipGetLastError());
    const unsigned nb = (unsigned)B * (unsigned)p.njobs;
    int gy = p.TY, gx = p.TX;
    const double *src = bufA;
    while (true) {
        const int oy = cdiv(gy, 16), ox = cdiv(gx, 16), last = oy == 1 && ox == 1;
        double *dst = last ? sums : (src == bufA ? bufB : bufA);
        hipLaunchKernelGGL(eval_finish_kernel, dim3(nb * (unsigned)oy * (unsigned)ox), dim3(EV_THREADS), 0, st, src, dst, gy, gx, oy, ox, last);
        PIV_CHECK_HIP(hipGetLastError());
        if (last) break;
        src = dst;
        gy = oy;
        gx = ox;
    }
    return PIVLFN_OK;
}

int launch_flow_errors(const float *flow, const float *truth, const unsigned char *mask, int B, int H, int W, int k, double div_flow,
                       double *sums, float *err_map, void *ws, size_t ws_bytes, hipStream_t st)
{
    PIV_REQUIRE(flow, "flow_errors: null pointer (flow, truth, sums and the workspace are required)");
    const int rc = eval_check("flow_errors", truth, sums, ws, ws_bytes, B, H, W, div_flow);
    if (rc != PIVLFN_OK) return rc;
    PIV_REQUIRE(k >= 0 && k <= 5, "flow_errors: pool exponent k=%d must be 0..5", k);
    PIV_REQUIRE(H % (1 << k) == 0 && W % (1 << k) == 0, "flow_errors: H=%d W=%d must be multiples of 2^k = %d", H, W, 1 << k);
    EvalParams p = {};
    p.truth = truth;
    p.mask = mask;
    p.err_map = err_map;
    p.div_flow = div_flow;
    p.H = H;
    p.W = W;
    p.njobs = 1;
    p.kmax = k;
    p.job[0] = {flow, k, k == 0 && aligned16(flow, W)};
    return eval_launch(p, B, sums, ws, st);
}

int launch_level_errors(const float *levels, int lowest_level, const float *truth, const unsigned char *mask, int B, int H, int W,
                        double div_flow, double *sums, void *ws, size_t ws_bytes, hipStream_t st)
{
    PIV_REQUIRE(levels, "level_errors: null pointer (levels, truth, sums and the workspace are required)");
    const int rc = eval_check("level_errors", truth, sums, ws, ws_bytes, B, H, W, div_flow);
    if (rc != PIVLFN_OK) return rc;
    PIV_REQUIRE(lowest_level >= 1 && lowest_level <= 6, "level_errors: lowest_level=%d must be 1..6", lowest_level);
    PIV_REQUIRE(H % 32 == 0 && W % 32 == 0, "level_errors: H=%d W=%d must be multiples of 32 (level 6 pools 32 x 32 windows)", H, W);
    EvalParams p = {};
    p.truth = truth;
    p.mask = mask;
    p.div_flow = div_flow;
    p.H = H;
    p.W = W;
    p.kmax = 5;
    const float *at = levels;
    for (int L = 6; L >= lowest_level; --L) {
        const int k = L - 1;
        const size_t n = (size_t)B * 2 * (size_t)(H >> k) * (size_t)(W >> k);
        for (int s = 0; s < 3; ++s) {
            p.job[p.njobs++] = {at, k, k == 0 && aligned16(at, W)};
            at += n;
        }
    }
    return eval_launch(p, B, sums, ws, st);
}

int launch_error_stats(const float *flow, const float *truth, const unsigned char *mask, double *acc, int B, int H, int W, hipStream_t st)
{
    PIV_REQUIRE(flow && truth && acc, "error_stats_accumulate: null pointer (flow, truth and acc are required)");
    if (int rc = check_shape("error_stats_accumulate", B, H, W, "frames", false)) return rc;
    hipLaunchKernelGGL(error_stats_kernel, dim3(frame_grid((size_t)H * W, 1)), dim3(256), 0, st, flow, truth, mask, acc, B,
                       (unsigned)H * (unsigned)W);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
