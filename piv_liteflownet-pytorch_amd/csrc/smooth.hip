// Flow smoothing and gap filling (gfx950): the orthonormal 2-D DCT-II of fp64 planes as two dense matrix products on the fp64 matrix
// instruction v_mfma_f64_16x16x4_f64 (dct_tables_kernel, dct_mm_kernel), and Garcia's penalised least squares  (W + s D^T D) z = W y  by
// conjugate gradients preconditioned with the gap-free solve in the DCT basis.  Arithmetic contract: include/pivlfn.h.
//
// The matrix kernel is pod.hip's gram_kernel with two operands: a workgroup of 4 waves owns a 64 x 64 block of the product, wave w the
// 32 x 32 quarter (w >> 1, w & 1) as 2 x 2 MFMA tiles (4 independent accumulator chains), K is walked in ascending chunks of DC_KC = 32
// into accumulators that start at +0.0, both operands are staged in LDS as [output index][k] (rows of DC_LD = 34 doubles: the 32 lanes of
// half a wave read row l & 15, column 4t + (l >> 4), that is dword banks 4*row + 2*k + {0, 1}, all 64 different), and the next chunk is on
// its way to registers while the current one feeds 8 k-steps of 4 MFMAs per wave.  An operand is addressed by strides, so C, C^T, a
// plane and its transpose are the same kernel; the loader walks whichever index is contiguous in memory fastest.  Rows, columns and k
// past the edge are staged as +0.0.  A value depends on its plane and its (row, column) alone, never on the batch or the grid.
//
// The solver follows pressure.hip: no grid-wide barrier, a seam between two phases is a kernel boundary, every scalar of the recurrence
// is derived by EVERY workgroup of a system from the same block partials and the same record of the launch before, the record of a
// system ping-pongs between two copies, and so does the search direction.  A system is one component of one frame, 2f + c.  One
// iteration is eight launches: direction and first Laplacian (recA -> recB), second Laplacian and d*q, the x / r update (recB -> recA),
// the four matrix products of the preconditioner (skipped plane by plane for a system that is not running) and r*z.
//
// The tree T(.) of the contract, the walk of a workgroup over its tile of nodes and the record of a system are cg_shared.h, shared with
// pressure.hip.
#include <cmath>
#include "launch_checks.h"
#include "cg_shared.h"

namespace pivlfn {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int DC_BLK = 64, DC_KC = 32, DC_LD = DC_KC + 2, DC_THREADS = 256;

// ---- the DCT tables -----------------------------------------------------------------------------------------------------------------------
struct DctTables { double *ch, *cw, *lh, *lw; };           // C_H [H][H], C_W [W][W], lambda_H [H], lambda_W [W]

static size_t dct_table_doubles(int H, int W) { return (size_t)H * H + (size_t)W * W + H + W; }

static DctTables dct_tables_at(double *base, int H, int W)
{
    DctTables t;
    t.ch = base;
    t.cw = t.ch + (size_t)H * H;
    t.lh = t.cw + (size_t)W * W;
    t.lw = t.lh + H;
    return t;
}

// a_k cos(pi m / 2N), m = ((2n+1) k) mod 4N folded in integers into the first octant, where cospi and sinpi keep their relative accuracy
__device__ __forceinline__ double dct_entry(int k, int n, int N)
{
#pragma clang fp contract(off)
    long m = ((long)(2 * n + 1) * k) % (4L * N);
    if (m > 2L * N) m = 4L * N - m;
    const bool neg = m > N;
    if (neg) m = 2L * N - m;
    const double c = 2 * m <= N ? cospi((double)m / (double)(2L * N)) : sinpi((double)(N - m) / (double)(2L * N));
    const double v = sqrt((k == 0 ? 1.0 : 2.0) / (double)N) * c;
    return neg ? -v : v;
}

__device__ __forceinline__ double dct_lambda(int k, int N)
{
#pragma clang fp contract(off)
    const double h = sinpi((double)k / (double)(2L * N));
    return 4.0 * (h * h);
}

__global__ __launch_bounds__(256) void dct_tables_kernel(const DctTables t, int H, int W)
{
    const size_t nh = (size_t)H * H, nw = (size_t)W * W;
    size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < nh) { t.ch[e] = dct_entry((int)(e / H), (int)(e % H), H); return; }
    e -= nh;
    if (e < nw) { t.cw[e] = dct_entry((int)(e / W), (int)(e % W), W); return; }
    e -= nw;
    if (e < (size_t)H) { t.lh[e] = dct_lambda((int)e, H); return; }
    e -= H;
    if (e < (size_t)W) t.lw[e] = dct_lambda((int)e, W);
}

// ---- the matrix product -------------------------------------------------------------------------------------------------------------------
// D[p][m][n] = sum over k of A[p*spa + m*sam + k*sak] * B[p*spb + k*sbk + n*sbn], D row-major [P][M][N]
struct MmParams {
    const double *A, *B;
    double *D;
    long spa, sam, sak, spb, sbk, sbn;
    int M, N, K;
    int a_kfast, b_kfast;                      // k is the operand's contiguous index in memory
    const double *lamM, *lamN;                 // not null: D *= 1 / (1 + s (lamM[m] + lamN[n])^2)
    double s;
    const CgRec *rec;                          // not null: plane p is skipped unless rec[p] is running
};

__global__ __launch_bounds__(DC_THREADS) void dct_mm_kernel(const MmParams p)
{
#pragma clang fp contract(off)
    __shared__ __align__(16) double tile[2 * DC_BLK * DC_LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int pl = blockIdx.z;
    if (p.rec && p.rec[pl].state != PIVLFN_SMOOTH_RUNNING) return;
    const int m0 = blockIdx.y * DC_BLK, n0 = blockIdx.x * DC_BLK;
    const double *A = p.A + (size_t)pl * p.spa, *B = p.B + (size_t)pl * p.spb;

    // element e = t + 256 i of a staged 64 x 32 operand tile: (output index, k)
    auto pos = [&](int e, int kfast, int &idx, int &k) {
        if (kfast) { k = e & (DC_KC - 1); idx = e >> 5; }
        else       { idx = e & (DC_BLK - 1); k = e >> 6; }
    };
    double pa[8], pb[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int idx, k;
            pos(t + DC_THREADS * i, p.a_kfast, idx, k);
            pa[i] = (m0 + idx < p.M && k0 + k < p.K) ? A[(size_t)(m0 + idx) * p.sam + (size_t)(k0 + k) * p.sak] : 0.0;
            pos(t + DC_THREADS * i, p.b_kfast, idx, k);
            pb[i] = (n0 + idx < p.N && k0 + k < p.K) ? B[(size_t)(k0 + k) * p.sbk + (size_t)(n0 + idx) * p.sbn] : 0.0;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int idx, k;
            pos(t + DC_THREADS * i, p.a_kfast, idx, k);
            tile[idx * DC_LD + k] = pa[i];
            pos(t + DC_THREADS * i, p.b_kfast, idx, k);
            tile[(DC_BLK + idx) * DC_LD + k] = pb[i];
        }
    };

    const double *la0 = tile + ((wave >> 1) * 32 + (lane & 15)) * DC_LD + (lane >> 4);
    const double *lb0 = tile + (DC_BLK + (wave & 1) * 32 + (lane & 15)) * DC_LD + (lane >> 4);
    const d4 zero = {0.0, 0.0, 0.0, 0.0};
    d4 acc[4] = {zero, zero, zero, zero};
    const int chunks = (p.K + DC_KC - 1) / DC_KC;
    fetch(0);
    for (int c = 0; c < chunks; ++c) {
        __syncthreads();                                   // the previous chunk has been read by every wave
        stage();
        __syncthreads();
        if (c + 1 < chunks) fetch((c + 1) * DC_KC);
#pragma unroll
        for (int k = 0; k < DC_KC / 4; ++k) {              // ascending k: k-step k is columns 4k .. 4k+3 of the chunk
            const double a0 = la0[4 * k], a1 = la0[16 * DC_LD + 4 * k];
            const double b0 = lb0[4 * k], b1 = lb0[16 * DC_LD + 4 * k];
            acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[3], 0, 0, 0);
        }
    }
    double *D = p.D + (size_t)pl * p.M * p.N;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) {                      // C/D map of the instruction: col = lane & 15, row = (lane >> 4) + 4 * reg
            const int row = m0 + (wave >> 1) * 32 + (q >> 1) * 16 + (lane >> 4) + 4 * r;
            const int col = n0 + (wave & 1) * 32 + (q & 1) * 16 + (lane & 15);
            if (row < p.M && col < p.N) {
                double v = acc[q][r];
                if (p.lamM) {
                    const double e = p.lamM[row] + p.lamN[col];
                    v = v * (1.0 / (1.0 + p.s * (e * e)));
                }
                D[(size_t)row * p.N + col] = v;
            }
        }
}

// The transform of P planes: in -> tmp -> out.  gamma: the forward transform's result is multiplied by Gamma (s is then read).
static void dct_enqueue(const DctTables &tb, const double *in, double *tmp, double *out, int P, int H, int W, bool inverse, bool gamma, double s,
                        const CgRec *rec, hipStream_t st)
{
    const long HW = (long)H * W;
    const dim3 grid((unsigned)cdiv(W, DC_BLK), (unsigned)cdiv(H, DC_BLK), (unsigned)P), block(DC_THREADS);
    MmParams a = {}, b = {};
    a.M = b.M = H, a.N = b.N = W, a.rec = b.rec = rec, a.s = b.s = s;
    // rows: tmp[h][n] = sum over k of in[h][k] * (forward: C_W[n][k], inverse: C_W[k][n])
    a.A = in, a.spa = HW, a.sam = W, a.sak = 1, a.a_kfast = 1;
    a.B = tb.cw, a.spb = 0, a.sbk = inverse ? W : 1, a.sbn = inverse ? 1 : W, a.b_kfast = inverse ? 0 : 1;
    a.D = tmp, a.K = W;
    // columns: out[m][w] = sum over k of (forward: C_H[m][k], inverse: C_H[k][m]) * tmp[k][w]
    b.A = tb.ch, b.spa = 0, b.sam = inverse ? 1 : H, b.sak = inverse ? H : 1, b.a_kfast = inverse ? 0 : 1;
    b.B = tmp, b.spb = HW, b.sbk = W, b.sbn = 1, b.b_kfast = 0;
    b.D = out, b.K = H;
    if (gamma) b.lamM = tb.lh, b.lamN = tb.lw;
    hipLaunchKernelGGL(dct_mm_kernel, grid, block, 0, st, a);
    hipLaunchKernelGGL(dct_mm_kernel, grid, block, 0, st, b);
}

static bool dct_shape_ok(int P, int H, int W)
{
    return P >= 1 && P <= 65535 && H >= 1 && H <= PIVLFN_DCT_MAX && W >= 1 && W <= PIVLFN_DCT_MAX && (size_t)P * H * W < ((size_t)1 << 31);
}

size_t dct2_workspace_bytes(int P, int H, int W)
{
    return dct_shape_ok(P, H, W) ? 8 * (dct_table_doubles(H, W) + (size_t)P * H * W) : 0;
}

#define DC_SIZE(fn, H, W)                                                                                                        \
    PIV_REQUIRE(H >= 1 && W >= 1, fn ": bad size H=%d W=%d (both must be positive)", H, W);                                       \
    PIV_REQUIRE(H <= PIVLFN_DCT_MAX && W <= PIVLFN_DCT_MAX, fn ": H=%d W=%d, a side may be at most %d", H, W, PIVLFN_DCT_MAX)

int launch_dct2(const double *x, double *out, int P, int H, int W, int inverse, void *ws, size_t ws_bytes, hipStream_t st)
{
    PIV_REQUIRE(x && out && ws, "dct2: null pointer (x, out and the workspace are required)");
    DC_SIZE("dct2", H, W);
    PIV_REQUIRE(P >= 1 && P <= 65535, "dct2: P=%d planes, must be 1..65535 (grid z dimension)", P);
    PIV_REQUIRE((size_t)P * H * W < ((size_t)1 << 31), "dct2: P*H*W=%zu values, must stay below 2^31", (size_t)P * H * W);
    const size_t need = dct2_workspace_bytes(P, H, W), bytes = (size_t)P * H * W * 8;
    if (int rc = check_workspace("dct2", ws, ws_bytes, need, "P=%d H=%d W=%d", P, H, W)) return rc;
    const Span in = {x, bytes, "x"}, o = {out, bytes, "out"}, w = {ws, need, "the workspace"};
    if (int rc = check_apart("dct2", o, in)) return rc;
    if (int rc = check_apart("dct2", w, in)) return rc;
    if (int rc = check_apart("dct2", w, o)) return rc;
    const DctTables tb = dct_tables_at(static_cast<double *>(ws), H, W);
    double *tmp = static_cast<double *>(ws) + dct_table_doubles(H, W);
    hipLaunchKernelGGL(dct_tables_kernel, dim3((unsigned)((dct_table_doubles(H, W) + 255) / 256)), dim3(256), 0, st, tb, H, W);
    dct_enqueue(tb, x, tmp, out, P, H, W, inverse != 0, false, 0.0, nullptr, st);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

// ---- the solver's workspace -------------------------------------------------------------------------------------------------------------
struct SmWs {
    CgRec *recA, *recB;                        // [S], S = 2F systems
    double *prz, *prr, *pdq, *pbb, *pw;        // [S][NB] block partials of r*z, r*r, d*q, b*b;  [F][NB] of the weights
    DctTables tb;
    double *w;                                 // [F][N]
    double *b, *x, *r, *z, *d[2], *t, *q;      // [S][N]; t and q are also the transforms' intermediate planes
    unsigned N;
    int H, W, chunks, NB;
};

struct SmLayout { SmWs ws; size_t bytes; };

static SmLayout sm_layout(void *base, int F, int H, int W)
{
    SmLayout L;
    const size_t N = (size_t)H * W, S = 2 * (size_t)F;
    const PrPlan plan = pr_plan(N);
    const size_t NB = plan.NB;
    WsCarver cv = {static_cast<unsigned char *>(base)};
    L.ws.recA = cv.take<CgRec>(S);
    L.ws.recB = cv.take<CgRec>(S);
    L.ws.prz = cv.take<double>(NB * S);
    L.ws.prr = cv.take<double>(NB * S);
    L.ws.pdq = cv.take<double>(NB * S);
    L.ws.pbb = cv.take<double>(NB * S);
    L.ws.pw = cv.take<double>(NB * F);
    L.ws.tb = dct_tables_at(cv.take<double>(dct_table_doubles(H, W)), H, W);
    L.ws.w = cv.take<double>(N * F);
    L.ws.b = cv.take<double>(N * S);
    L.ws.x = cv.take<double>(N * S);
    L.ws.r = cv.take<double>(N * S);
    L.ws.z = cv.take<double>(N * S);
    L.ws.d[0] = cv.take<double>(N * S);
    L.ws.d[1] = cv.take<double>(N * S);
    L.ws.t = cv.take<double>(N * S);
    L.ws.q = cv.take<double>(N * S);
    L.ws.N = (unsigned)N;
    L.ws.H = H;
    L.ws.W = W;
    L.ws.chunks = plan.chunks;
    L.ws.NB = plan.NB;
    L.bytes = cv.at;
    return L;
}

static bool sm_shape_ok(int F, int H, int W)
{
    return F >= 1 && F <= 32767 && H >= 1 && H <= PIVLFN_DCT_MAX && W >= 1 && W <= PIVLFN_DCT_MAX && 2 * (size_t)F * H * W < ((size_t)1 << 31);
}

size_t smooth_workspace_bytes(int F, int H, int W) { return sm_shape_ok(F, H, W) ? sm_layout(nullptr, F, H, W).bytes : 0; }

// ---- the Laplacian with reflecting boundaries: the sum over the neighbours that exist of (neighbour - centre) --------------------------
template <typename V>
__device__ __forceinline__ double sm_lap(const V &val, unsigned i, int H, int W)
{
#pragma clang fp contract(off)
    const int y = (int)(i / (unsigned)W), x = (int)(i - (unsigned)y * (unsigned)W);
    const double c = val(i);
    const double l = x > 0 ? val(i - 1) - c : 0.0, r = x + 1 < W ? val(i + 1) - c : 0.0;
    const double u = y > 0 ? val(i - (unsigned)W) - c : 0.0, d = y + 1 < H ? val(i + (unsigned)W) - c : 0.0;
    return ((l + r) + u) + d;
}

__device__ __forceinline__ bool sm_known(float a, float b) { return fabsf(a) <= 1e9f && fabsf(b) <= 1e9f; }      // NaN fails

// ---- setup --------------------------------------------------------------------------------------------------------------------------------
// blockIdx.x = frame * NB + the workgroup's tile of the frame: the weights, b = w*y of both components, the partials of w and b*b
__global__ __launch_bounds__(PR_THREADS) void smooth_prep_kernel(const float *flows, const float *weights, const unsigned char *mask, const SmWs ws)
{
#pragma clang fp contract(off)
    __shared__ double sw[3][4];
    const unsigned N = ws.N, f = blockIdx.x / (unsigned)ws.NB, blk = blockIdx.x - f * (unsigned)ws.NB;
    const int tid = threadIdx.x;
    const size_t fo = (size_t)f * N;
    const float *fu = flows + 2 * fo, *fv = fu + N;
    double root[3];                                                            // w, b*b of u, b*b of v
    pr_tile_roots<3>(ws.chunks, N, blk, sw, root, [&](unsigned i, double (&l)[3]) {
        const float u = fu[i], v = fv[i];
        const float wf = weights ? weights[fo + i] : 1.0f;
        const bool pos = sm_known(u, v) && !(mask && mask[fo + i]) && wf > 0.0f && wf <= 3.402823466e38f;
        const double wd = pos ? (double)wf : 0.0;
        const double bu = pos ? wd * (double)u : 0.0, bv = pos ? wd * (double)v : 0.0;             // a weight-0 value enters no product
        ws.w[fo + i] = wd;
        ws.b[2 * fo + i] = bu;
        ws.b[2 * fo + N + i] = bv;
        l[0] = wd;
        l[1] = bu * bu;
        l[2] = bv * bv;
    });
    if (tid == 0) {
        ws.pw[(size_t)f * ws.NB + blk] = root[0];
        ws.pbb[(size_t)(2 * f) * ws.NB + blk] = root[1];
        ws.pbb[(size_t)(2 * f + 1) * ws.NB + blk] = root[2];
    }
}

// blockIdx.x = system * NB + tile, here and below.  t = D x
__global__ __launch_bounds__(PR_THREADS) void smooth_lap_kernel(const SmWs ws)
{
    const unsigned N = ws.N, sys = blockIdx.x / (unsigned)ws.NB, blk = blockIdx.x - sys * (unsigned)ws.NB;
    const double *x = ws.x + (size_t)sys * N;
    double *t = ws.t + (size_t)sys * N;
    auto val = [&](unsigned k) { return x[k]; };
    pr_tile_for_each(ws.chunks, N, blk, [&](size_t i) { t[i] = sm_lap(val, (unsigned)i, ws.H, ws.W); });
}

// r = b - (w*x + s*(D t)), the partials of r*r, and the first record of the system
__global__ __launch_bounds__(PR_THREADS) void smooth_resid_kernel(const SmWs ws, double s)
{
#pragma clang fp contract(off)
    __shared__ double sw[2][4];
    const unsigned N = ws.N, sys = blockIdx.x / (unsigned)ws.NB, blk = blockIdx.x - sys * (unsigned)ws.NB;
    const int tid = threadIdx.x;
    const size_t so = (size_t)sys * N, fo = (size_t)(sys >> 1) * N;
    const double *t = ws.t + so;
    auto val = [&](unsigned k) { return t[k]; };
    double root[1];                                                            // r*r
    pr_tile_roots<1>(ws.chunks, N, blk, sw, root, [&](unsigned i, double (&l)[1]) {
        const double rn = ws.b[so + i] - (ws.w[fo + i] * ws.x[so + i] + s * sm_lap(val, i, ws.H, ws.W));
        ws.r[so + i] = rn;
        l[0] = rn * rn;
    });
    if (tid == 0) ws.prr[(size_t)sys * ws.NB + blk] = root[0];
    if (blk == 0) {                                                            // the whole workgroup: pr_finish synchronises it
        const double *const parts[2] = {ws.pw + (size_t)(sys >> 1) * ws.NB, ws.pbb + (size_t)sys * ws.NB};
        double top[2];
        pr_finish<2>(parts, ws.NB, sw, top);
        if (tid == 0) {
            CgRec rec = {0.0, 0.0, top[1], top[0] > 0.0 ? PIVLFN_SMOOTH_RUNNING : PIVLFN_SMOOTH_EMPTY, 0, CG_FRESH, 0, {0.0, 0.0, 0.0}};
            cg_store(ws.recA + sys, rec);
        }
    }
}

// the partials of r*z of a running system (recA is only read)
__global__ __launch_bounds__(PR_THREADS) void smooth_rz_kernel(const SmWs ws)
{
#pragma clang fp contract(off)
    __shared__ double sw[1][4];
    const unsigned N = ws.N, sys = blockIdx.x / (unsigned)ws.NB, blk = blockIdx.x - sys * (unsigned)ws.NB;
    const int tid = threadIdx.x;
    if (ws.recA[sys].state != PIVLFN_SMOOTH_RUNNING) return;
    const double *r = ws.r + (size_t)sys * N, *z = ws.z + (size_t)sys * N;
    double root[1];
    pr_tile_roots<1>(ws.chunks, N, blk, sw, root, [&](size_t i, double (&l)[1]) { l[0] = r[i] * z[i]; });
    if (tid == 0) ws.prz[(size_t)sys * ws.NB + blk] = root[0];
}

// ---- one iteration ------------------------------------------------------------------------------------------------------------------------
// finish rho' and rr, apply the stopping rule, d = z + beta d, t = D d.  recA -> recB.
__global__ __launch_bounds__(PR_THREADS) void smooth_pcg_dir_kernel(const SmWs ws, double tol)
{
#pragma clang fp contract(off)
    __shared__ double sw[2][4];
    const unsigned N = ws.N, sys = blockIdx.x / (unsigned)ws.NB, blk = blockIdx.x - sys * (unsigned)ws.NB;
    const int tid = threadIdx.x;
    const CgRec in = cg_load(ws.recA + sys);
    const bool writer = blk == 0 && tid == 0;
    if (cg_frozen(in, ws.recB + sys, writer)) return;
    const double *const parts[2] = {ws.prz + (size_t)sys * ws.NB, ws.prr + (size_t)sys * ws.NB};
    double top[2];
    pr_finish<2>(parts, ws.NB, sw, top);
    CgRec out = in;
    const bool fresh = in.phase == CG_FRESH;
    double beta = 0.0;
    out.rho = top[0];
    out.rr = top[1];
    if (!fresh) {
        beta = top[0] / in.rho;
        out.iters = in.iters + 1;
    }
    out.phase = CG_MID;
    if (out.rr <= (tol * tol) * out.bb) {
        out.state = PIVLFN_SMOOTH_CONVERGED;
        if (writer) cg_store(ws.recB + sys, out);
        return;
    }
    const size_t so = (size_t)sys * N;
    const bool odd = (in.dsel & 1) != 0;                                       // a select, not an index: the arguments stay in registers
    const double *z = ws.z + so, *dold = (odd ? ws.d[1] : ws.d[0]) + so;
    double *dnew = (odd ? ws.d[0] : ws.d[1]) + so, *t = ws.t + so;
    out.dsel = (in.dsel & 1) ^ 1;
    auto val = [&](unsigned k) { return fresh ? z[k] : z[k] + beta * dold[k]; };
    pr_tile_for_each(ws.chunks, N, blk, [&](unsigned i) {
        dnew[i] = val(i);
        t[i] = sm_lap(val, i, ws.H, ws.W);
    });
    if (writer) cg_store(ws.recB + sys, out);
}

// q = w*d + s*(D t), the partials of d*q.  recB is only read.
__global__ __launch_bounds__(PR_THREADS) void smooth_pcg_q_kernel(const SmWs ws, double s)
{
#pragma clang fp contract(off)
    __shared__ double sw[1][4];
    const unsigned N = ws.N, sys = blockIdx.x / (unsigned)ws.NB, blk = blockIdx.x - sys * (unsigned)ws.NB;
    const int tid = threadIdx.x;
    const CgRec in = cg_load(ws.recB + sys);
    if (in.state != PIVLFN_SMOOTH_RUNNING) return;
    const size_t so = (size_t)sys * N, fo = (size_t)(sys >> 1) * N;
    const double *d = ((in.dsel & 1) ? ws.d[1] : ws.d[0]) + so, *t = ws.t + so, *w = ws.w + fo;
    double *q = ws.q + so;
    auto val = [&](unsigned k) { return t[k]; };
    double root[1];                                                            // d*q
    pr_tile_roots<1>(ws.chunks, N, blk, sw, root, [&](unsigned i, double (&l)[1]) {
        const double dc = d[i], qv = w[i] * dc + s * sm_lap(val, i, ws.H, ws.W);
        q[i] = qv;
        l[0] = dc * qv;
    });
    if (tid == 0) ws.pdq[(size_t)sys * ws.NB + blk] = root[0];
}

// finish sigma, the breakdown rule, x and r, the partials of r*r.  recB -> recA.
__global__ __launch_bounds__(PR_THREADS) void smooth_pcg_xr_kernel(const SmWs ws)
{
#pragma clang fp contract(off)
    __shared__ double sw[1][4];
    const unsigned N = ws.N, sys = blockIdx.x / (unsigned)ws.NB, blk = blockIdx.x - sys * (unsigned)ws.NB;
    const int tid = threadIdx.x;
    const CgRec in = cg_load(ws.recB + sys);
    const bool writer = blk == 0 && tid == 0;
    double alpha;
    if (cg_frozen(in, ws.recA + sys, writer) || !cg_alpha(in, ws.recA + sys, writer, ws.pdq + (size_t)sys * ws.NB, ws.NB, sw, alpha)) return;
    const size_t so = (size_t)sys * N;
    const double *d = ((in.dsel & 1) ? ws.d[1] : ws.d[0]) + so, *q = ws.q + so;
    double *x = ws.x + so, *r = ws.r + so;
    double root[1];                                                            // r*r
    pr_tile_roots<1>(ws.chunks, N, blk, sw, root, [&](unsigned i, double (&l)[1]) {
        x[i] = x[i] + alpha * d[i];
        const double rn = r[i] - alpha * q[i];
        r[i] = rn;
        l[0] = rn * rn;
    });
    CgRec out = in;
    out.phase = CG_PENDING;
    if (tid == 0) {
        ws.prr[(size_t)sys * ws.NB + blk] = root[0];
        if (blk == 0) cg_store(ws.recA + sys, out);
    }
}

// ---- read-out -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PR_THREADS) void smooth_read_kernel(const SmWs ws, double *z, float *z32, unsigned char *filled, double *status)
{
#pragma clang fp contract(off)
    __shared__ double sw[1][4];
    const unsigned N = ws.N, sys = blockIdx.x / (unsigned)ws.NB, blk = blockIdx.x - sys * (unsigned)ws.NB;
    const int tid = threadIdx.x;
    const size_t so = (size_t)sys * N, fo = (size_t)(sys >> 1) * N;
    CgRec rec = cg_load(ws.recA + sys);
    if (blk == 0) {                                                            // the whole workgroup: pr_finish synchronises it
        if (rec.state == PIVLFN_SMOOTH_RUNNING) {
            const double *const parts[1] = {ws.prr + (size_t)sys * ws.NB};
            double top[1];
            pr_finish<1>(parts, ws.NB, sw, top);
            rec.rr = top[0];
            if (rec.phase != CG_FRESH) rec.iters += 1;
        }
        if (tid == 0) cg_write_status(status + 4 * (size_t)sys, rec);
    }
    const bool empty = rec.state == PIVLFN_SMOOTH_EMPTY;
    pr_tile_for_each(ws.chunks, N, blk, [&](size_t i) {
        const double v = empty ? 1e10 : ws.x[so + i];
        z[so + i] = v;
        if (z32) z32[so + i] = (float)v;
        if (filled && !(sys & 1)) filled[fo + i] = ws.w[fo + i] > 0.0 ? 0 : 1;
    });
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
#define SM_SHAPE(fn, F, H, W)                                                                                                    \
    PIV_REQUIRE(F >= 1 && F <= 32767, fn ": F=%d frames, must be 1..32767 (two planes each in the grid z dimension)", F);        \
    DC_SIZE(fn, H, W);                                                                                                           \
    PIV_REQUIRE(2 * (size_t)(F) * H * W < ((size_t)1 << 31), fn ": 2*F*H*W=%zu values, must stay below 2^31", 2 * (size_t)(F) * H * W)

#define SM_WORKSPACE(fn, F, H, W, ws, ws_bytes)                                                                                  \
    PIV_REQUIRE(ws != nullptr, fn ": null pointer (the workspace is required)");                                                 \
    if (int rc = check_workspace(fn, ws, ws_bytes, smooth_workspace_bytes(F, H, W), "F=%d H=%d W=%d", F, H, W)) return rc

// z = M^-1 r for the planes of running systems (rec not null) or of all
static void sm_precondition(const SmWs &ws, const double *in, double *out, int S, double s, const CgRec *rec, hipStream_t st)
{
    dct_enqueue(ws.tb, in, ws.t, ws.q, S, ws.H, ws.W, false, true, s, rec, st);
    dct_enqueue(ws.tb, ws.q, ws.t, out, S, ws.H, ws.W, true, false, 0.0, rec, st);
}

int launch_smooth_setup(const float *flows, const float *weights, const unsigned char *mask, int F, int H, int W, double s, void *ws,
                        size_t ws_bytes, hipStream_t st)
{
    SM_SHAPE("smooth_setup", F, H, W);
    PIV_REQUIRE(std::isfinite(s) && s > 0.0, "smooth_setup: s=%g must be finite and positive", s);
    PIV_REQUIRE(flows != nullptr, "smooth_setup: null pointer (flows is required)");
    SM_WORKSPACE("smooth_setup", F, H, W, ws, ws_bytes);
    const size_t N = (size_t)H * W, need = smooth_workspace_bytes(F, H, W);
    if (int rc = check_alias_by_input("smooth_setup", {{ws, need, "the workspace"}},
                                      {{flows, (size_t)F * 2 * N * 4, "flows"}, {weights, (size_t)F * N * 4, "weights"}, {mask, (size_t)F * N, "mask"}}, ""))
        return rc;
    const SmLayout L = sm_layout(ws, F, H, W);
    const int S = 2 * F;
    const dim3 block(PR_THREADS), per_frame((unsigned)F * (unsigned)L.ws.NB), per_sys((unsigned)S * (unsigned)L.ws.NB);
    hipLaunchKernelGGL(dct_tables_kernel, dim3((unsigned)((dct_table_doubles(H, W) + 255) / 256)), dim3(256), 0, st, L.ws.tb, H, W);
    hipLaunchKernelGGL(smooth_prep_kernel, per_frame, block, 0, st, flows, weights, mask, L.ws);
    sm_precondition(L.ws, L.ws.b, L.ws.x, S, s, nullptr, st);                  // x0 = M^-1 W y
    hipLaunchKernelGGL(smooth_lap_kernel, per_sys, block, 0, st, L.ws);
    hipLaunchKernelGGL(smooth_resid_kernel, per_sys, block, 0, st, L.ws, s);
    sm_precondition(L.ws, L.ws.r, L.ws.z, S, s, L.ws.recA, st);
    hipLaunchKernelGGL(smooth_rz_kernel, per_sys, block, 0, st, L.ws);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

int launch_smooth_pcg(void *ws, size_t ws_bytes, int F, int H, int W, double s, double tol, int iters, hipStream_t st)
{
    SM_SHAPE("smooth_pcg", F, H, W);
    PIV_REQUIRE(std::isfinite(s) && s > 0.0, "smooth_pcg: s=%g must be finite and positive", s);
    PIV_REQUIRE(std::isfinite(tol) && tol > 0.0, "smooth_pcg: tol=%g must be finite and positive", tol);
    PIV_REQUIRE(iters >= 0, "smooth_pcg: iters=%d must not be negative", iters);
    SM_WORKSPACE("smooth_pcg", F, H, W, ws, ws_bytes);
    if (iters == 0) return PIVLFN_OK;                                          // nothing to enqueue
    const SmLayout L = sm_layout(ws, F, H, W);
    const int S = 2 * F;
    const dim3 grid((unsigned)S * (unsigned)L.ws.NB), block(PR_THREADS);
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(smooth_pcg_dir_kernel, grid, block, 0, st, L.ws, tol);
        hipLaunchKernelGGL(smooth_pcg_q_kernel, grid, block, 0, st, L.ws, s);
        hipLaunchKernelGGL(smooth_pcg_xr_kernel, grid, block, 0, st, L.ws);
        sm_precondition(L.ws, L.ws.r, L.ws.z, S, s, L.ws.recA, st);
        hipLaunchKernelGGL(smooth_rz_kernel, grid, block, 0, st, L.ws);
    }
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

int launch_smooth_read(const void *ws, size_t ws_bytes, int F, int H, int W, double *z, float *z32, unsigned char *filled, double *status,
                       hipStream_t st)
{
    SM_SHAPE("smooth_read", F, H, W);
    PIV_REQUIRE(z && status, "smooth_read: null pointer (z and status are required)");
    SM_WORKSPACE("smooth_read", F, H, W, ws, ws_bytes);
    const size_t N = (size_t)H * W, need = smooth_workspace_bytes(F, H, W);
    const Span outs[] = {{z, (size_t)F * 2 * N * 8, "z"}, {z32, (size_t)F * 2 * N * 4, "z32"}, {filled, (size_t)F * N, "filled"},
                         {status, (size_t)F * 64, "status"}};
    for (int a = 0; a < 4; ++a) {
        if (int rc = check_apart("smooth_read", outs[a], {ws, need, "the workspace"})) return rc;
        for (int b = a + 1; b < 4; ++b)
            if (int rc = check_apart("smooth_read", outs[a], outs[b])) return rc;
    }
    const SmLayout L = sm_layout(const_cast<void *>(ws), F, H, W);
    hipLaunchKernelGGL(smooth_read_kernel, dim3(2u * (unsigned)F * (unsigned)L.ws.NB), dim3(PR_THREADS), 0, st, L.ws, z, z32, filled, status);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
