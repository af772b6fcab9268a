// Pressure from time-resolved planar PIV (gfx950): the pressure gradient g of the momentum equation from three consecutive flows
// (pressure_gradient_kernel), its least-squares integration over the valid nodes -- the graph-Laplacian Poisson problem with the natural
// Neumann boundary -- by Jacobi-preconditioned conjugate gradients (pressure_setup_kernel, two kernels per iteration), and the read-out.
// Arithmetic contract: include/pivlfn.h.
//
// No grid-wide barrier, no persistent kernel, no flag that one workgroup writes and another reads in the same launch: the seam between two
// phases of an iteration is a kernel boundary, and every scalar of the recurrence (rho, sigma, rr, alpha, beta, the state) is derived by
// EVERY workgroup of a frame from the same block partials and the same record of the launch before, so all of them take the same
// frozen-or-running decision.  The record of a frame ping-pongs between two copies (recA is read by the first kernel of an iteration, which
// writes recB; the second reads recB and writes recA; one thread of the frame's first workgroup writes), and so does the search direction
// d, whose new value a neighbouring workgroup needs while the old one is still being read.
//
// The tree T(.) of the contract, the walk of a workgroup over its tile of nodes and the record of a frame are cg_shared.h, shared with
// smooth.hip.
//
// What an iteration moves per node: the first kernel reads z and d (the four neighbours of each from cache) and the adjacency byte and
// writes d and q; the second reads d, q, x, r and the byte and writes x, r, z: 11 doubles and 2 bytes, 90 bytes.
//
// Step 5 of the contract's iteration is split over the boundary: the second kernel of iteration k leaves x, r, z and the partials of
// r*z and r*r (phase PENDING); beta, d, rho = rho' and the iteration count are completed by the first kernel of iteration k + 1, which
// may belong to a later call, or -- the count and rr -- by the read-out.  d is no output, so where the stopping rule fires first the
// last d is never formed.
#include <cmath>
#include "launch_checks.h"
#include "cg_shared.h"

namespace pivlfn {

struct PrWs {
    CgRec *recA, *recB;                        // [F]
    double *prz, *prr, *pdq;                   // [F][NB] block partials of r*z, r*r, d*q
    double *b, *x, *r, *z, *d[2], *q;          // [F][N]
    unsigned char *adj;                        // [F][N]: bit 0 left, 1 right, 2 up, 3 down edge active; bit 4 the node is valid
    unsigned N;
    int w, chunks, NB;                         // chunks per workgroup, partials per frame
};

struct PrLayout {
    PrWs ws;
    size_t off_b, off_x, off_adj, bytes;
};

// N >= 1.  Offsets are multiples of 8 from an 8-byte aligned base; adj comes last.
static PrLayout pr_layout(void *base, int F, int h, int w)
{
    PrLayout L;
    const size_t N = (size_t)h * w;
    const PrPlan plan = pr_plan(N);
    const size_t NB = plan.NB;
    WsCarver cv = {static_cast<unsigned char *>(base)};
    L.ws.recA = cv.take<CgRec>(F);
    L.ws.recB = cv.take<CgRec>(F);
    L.ws.prz = cv.take<double>(NB * F);
    L.ws.prr = cv.take<double>(NB * F);
    L.ws.pdq = cv.take<double>(NB * F);
    L.off_b = cv.at;
    L.ws.b = cv.take<double>(N * F);
    L.off_x = cv.at;
    L.ws.x = cv.take<double>(N * F);
    L.ws.r = cv.take<double>(N * F);
    L.ws.z = cv.take<double>(N * F);
    L.ws.d[0] = cv.take<double>(N * F);
    L.ws.d[1] = cv.take<double>(N * F);
    L.ws.q = cv.take<double>(N * F);
    L.off_adj = cv.at;
    L.ws.adj = cv.take<unsigned char>(N * F);
    L.ws.N = (unsigned)N;
    L.ws.w = w;
    L.ws.chunks = plan.chunks;
    L.ws.NB = plan.NB;
    L.bytes = cv.at;
    return L;
}

static bool pr_shape_ok(int F, int h, int w) { return F >= 1 && h >= 1 && w >= 1 && (size_t)F * h * w < ((size_t)1 << 31); }

size_t pressure_workspace_bytes(int F, int h, int w) { return pr_shape_ok(F, h, w) ? pr_layout(nullptr, F, h, w).bytes : 0; }

size_t pressure_workspace_offset(int F, int h, int w, int what)
{
    if (!pr_shape_ok(F, h, w)) return 0;
    const PrLayout L = pr_layout(nullptr, F, h, w);
    return what == PIVLFN_PRESSURE_WS_B ? L.off_b : what == PIVLFN_PRESSURE_WS_X ? L.off_x : what == PIVLFN_PRESSURE_WS_ADJ ? L.off_adj : 0;
}

__device__ __forceinline__ double pr_deg(unsigned a) { return (double)__popc(a & 15u); }

// ---- the gradient -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool pr_known(float a, float b) { return fabsf(a) <= 1e9f && fabsf(b) <= 1e9f; }      // NaN fails

// one thread per node of an output frame; 32-bit node index over all frames (the host checks (B-2)*h*w < 2^31)
__global__ __launch_bounds__(PR_THREADS) void pressure_gradient_kernel(const float *flows, int F, int h, int w, double s, double nu, double *g,
                                                                       unsigned char *valid)
{
#pragma clang fp contract(off)
    const unsigned N = (unsigned)h * (unsigned)w, total = (unsigned)F * N;
    const unsigned t = blockIdx.x * (unsigned)PR_THREADS + threadIdx.x;
    if (t >= total) return;
    const unsigned f = t / N, i = t - f * N;
    const int y = (int)(i / (unsigned)w), x = (int)(i - (unsigned)y * (unsigned)w);
    const float *prev = flows + (size_t)f * 2 * N, *cur = prev + 2 * (size_t)N, *next = cur + 2 * (size_t)N;
    double gx = 0.0, gy = 0.0;
    bool ok = y >= 1 && y <= h - 2 && x >= 1 && x <= w - 2;
    if (ok)
        ok = pr_known(cur[i], cur[N + i]) && pr_known(cur[i - 1], cur[N + i - 1]) && pr_known(cur[i + 1], cur[N + i + 1]) &&
             pr_known(cur[i - w], cur[N + i - w]) && pr_known(cur[i + w], cur[N + i + w]) && pr_known(prev[i], prev[N + i]) &&
             pr_known(next[i], next[N + i]);
    if (ok) {
        const double uc = (double)cur[i], vc = (double)cur[N + i];
        double out[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const float *cp = cur + (size_t)a * N;
            const double ac = (double)cp[i], al = (double)cp[i - 1], ar = (double)cp[i + 1], au = (double)cp[i - w], ad = (double)cp[i + w];
            const double at = ((double)next[(size_t)a * N + i] - (double)prev[(size_t)a * N + i]) * 0.5;
            const double ax = (ar - al) / (2.0 * s), ay = (ad - au) / (2.0 * s);
            const double lap = ((((al + ar) + au) + ad) - 4.0 * ac) / (s * s);
            out[a] = (-(at + (uc * ax + vc * ay))) + nu * lap;
        }
        gx = out[0];
        gy = out[1];
    }
    g[(size_t)f * 2 * N + i] = gx;
    g[(size_t)f * 2 * N + N + i] = gy;
    valid[t] = ok ? 1 : 0;
}

// ---- setup ------------------------------------------------------------------------------------------------------------------------------
// blockIdx.x = frame * NB + the workgroup's tile of the frame.  At most four waves a SIMD: the kernel's 96 registers would admit a fifth,
// and with five workgroups a CU 2 x 1024 x 1024 nodes take 108 us instead of 102 (measured).
__global__ __launch_bounds__(PR_THREADS) __attribute__((amdgpu_waves_per_eu(1, 4))) void pressure_setup_kernel(const double *g, const unsigned char *valid, double s, const PrWs ws)
{
#pragma clang fp contract(off)
    __shared__ double sw[2][4];
    const unsigned N = ws.N, f = blockIdx.x / (unsigned)ws.NB, blk = blockIdx.x - f * (unsigned)ws.NB;
    const int tid = threadIdx.x, w = ws.w;
    const size_t fo = (size_t)f * N;
    const double *gx = g + 2 * fo, *gy = gx + N;
    const unsigned char *va = valid + fo;
    double root[2];                                                            // r*z, r*r
    pr_tile_roots<2>(ws.chunks, N, blk, sw, root, [&](unsigned i, double (&l)[2]) {
        const unsigned col = i % (unsigned)w;
        const bool me = va[i] != 0;
        const bool eL = me && col > 0 && va[i - 1] != 0, eR = me && col + 1 < (unsigned)w && va[i + 1] != 0;
        const bool eU = me && i >= (unsigned)w && va[i - w] != 0, eD = me && i + (unsigned)w < N && va[i + w] != 0;
        const unsigned a = (eL ? 1u : 0u) | (eR ? 2u : 0u) | (eU ? 4u : 0u) | (eD ? 8u : 0u);
        const double L = eL ? (0.5 * (gx[i - 1] + gx[i])) * s : 0.0;
        const double R = eR ? -((0.5 * (gx[i] + gx[i + 1])) * s) : 0.0;
        const double U = eU ? (0.5 * (gy[i - w] + gy[i])) * s : 0.0;
        const double D = eD ? -((0.5 * (gy[i] + gy[i + w])) * s) : 0.0;
        const double b = ((L + R) + U) + D;
        const double z = a ? b / pr_deg(a) : 0.0;
        ws.adj[fo + i] = (unsigned char)(a | (me ? 16u : 0u));
        ws.b[fo + i] = b;
        ws.x[fo + i] = 0.0;
        ws.r[fo + i] = b;
        ws.z[fo + i] = z;
        l[0] = b * z;
        l[1] = b * b;
    });
    if (tid == 0) {
        ws.prz[(size_t)f * ws.NB + blk] = root[0];
        ws.prr[(size_t)f * ws.NB + blk] = root[1];
        if (blk == 0) {
            CgRec rec = {0.0, 0.0, 0.0, PIVLFN_PRESSURE_RUNNING, 0, CG_FRESH, 0, {0.0, 0.0, 0.0}};
            cg_store(ws.recA + f, rec);
        }
    }
}

// ---- one iteration: two kernels -----------------------------------------------------------------------------------------------------------
// First kernel: finish rho' and rr, apply the stopping rule, d = z + beta d, q = A d, the partials of d*q.  recA -> recB.
__global__ __launch_bounds__(PR_THREADS) void pressure_cg_dq_kernel(const PrWs ws, double tol)
{
#pragma clang fp contract(off)
    __shared__ double sw[2][4];
    const unsigned N = ws.N, f = blockIdx.x / (unsigned)ws.NB, blk = blockIdx.x - f * (unsigned)ws.NB;
    const int tid = threadIdx.x, w = ws.w;
    const CgRec in = cg_load(ws.recA + f);
    const bool writer = blk == 0 && tid == 0;
    if (cg_frozen(in, ws.recB + f, writer)) return;
    const double *const parts[2] = {ws.prz + (size_t)f * ws.NB, ws.prr + (size_t)f * ws.NB};
    double top[2];
    pr_finish<2>(parts, ws.NB, sw, top);
    CgRec out = in;
    const bool fresh = in.phase == CG_FRESH;
    double beta = 0.0;
    out.rho = top[0];
    out.rr = top[1];
    if (fresh) {
        out.bb = top[1];                                                       // r = b: T(b*b) is T(r*r)
    } else {
        beta = top[0] / in.rho;
        out.iters = in.iters + 1;
    }
    out.phase = CG_MID;
    if (out.bb > 0.0 && out.rr <= (tol * tol) * out.bb) {                      // b = 0 is left to the breakdown rule
        out.state = PIVLFN_PRESSURE_CONVERGED;
        if (writer) cg_store(ws.recB + f, out);
        return;
    }
    const size_t fo = (size_t)f * N;
    const bool odd = (in.dsel & 1) != 0;                                       // a select, not an index: the arguments stay in registers
    const double *z = ws.z + fo, *dold = (odd ? ws.d[1] : ws.d[0]) + fo;
    double *dnew = (odd ? ws.d[0] : ws.d[1]) + fo, *q = ws.q + fo;
    const unsigned char *adj = ws.adj + fo;
    out.dsel = (in.dsel & 1) ^ 1;
    double root[1];                                                            // d*q
    pr_tile_roots<1>(ws.chunks, N, blk, sw, root, [&](unsigned i, double (&l)[1]) {
        const unsigned a = adj[i];
        // the direction of a node, its own or a neighbour's: an edge is active only where the neighbour exists
#define PR_D(k) (fresh ? z[k] : z[k] + beta * dold[k])
        const double dc = PR_D(i);
        // (the bounds hold for every byte setup writes; they keep a workspace that never saw setup inside itself)
        const double dl = ((a & 1u) && i > 0) ? PR_D(i - 1) : 0.0, dr = ((a & 2u) && i + 1 < N) ? PR_D(i + 1) : 0.0;
        const double du = ((a & 4u) && i >= (unsigned)w) ? PR_D(i - w) : 0.0, dd = ((a & 8u) && i + (unsigned)w < N) ? PR_D(i + w) : 0.0;
#undef PR_D
        const double qv = pr_deg(a) * dc - (((dl + dr) + du) + dd);
        dnew[i] = dc;
        q[i] = qv;
        l[0] = dc * qv;
    });
    if (tid == 0) {
        ws.pdq[(size_t)f * ws.NB + blk] = root[0];
        if (blk == 0) cg_store(ws.recB + f, out);
    }
}

// Second kernel: finish sigma, the breakdown rule, x, r, z and the partials of r*z and r*r.  recB -> recA.
__global__ __launch_bounds__(PR_THREADS) void pressure_cg_xr_kernel(const PrWs ws)
{
#pragma clang fp contract(off)
    __shared__ double sw[2][4];
    const unsigned N = ws.N, f = blockIdx.x / (unsigned)ws.NB, blk = blockIdx.x - f * (unsigned)ws.NB;
    const int tid = threadIdx.x;
    const CgRec in = cg_load(ws.recB + f);
    const bool writer = blk == 0 && tid == 0;
    double alpha;
    if (cg_frozen(in, ws.recA + f, writer) || !cg_alpha(in, ws.recA + f, writer, ws.pdq + (size_t)f * ws.NB, ws.NB, sw, alpha)) return;
    const size_t fo = (size_t)f * N;
    const double *d = ((in.dsel & 1) ? ws.d[1] : ws.d[0]) + fo, *q = ws.q + fo;
    double *x = ws.x + fo, *r = ws.r + fo, *z = ws.z + fo;
    const unsigned char *adj = ws.adj + fo;
    double root[2];                                                            // r*z, r*r
    pr_tile_roots<2>(ws.chunks, N, blk, sw, root, [&](unsigned i, double (&l)[2]) {
        const unsigned a = adj[i] & 15u;
        x[i] = x[i] + alpha * d[i];
        const double rn = r[i] - alpha * q[i];
        const double zn = a ? rn / pr_deg(a) : 0.0;
        r[i] = rn;
        z[i] = zn;
        l[0] = rn * zn;
        l[1] = rn * rn;
    });
    CgRec out = in;
    out.phase = CG_PENDING;
    if (tid == 0) {
        ws.prz[(size_t)f * ws.NB + blk] = root[0];
        ws.prr[(size_t)f * ws.NB + blk] = root[1];
        if (blk == 0) cg_store(ws.recA + f, out);
    }
}

// ---- read-out ---------------------------------------------------------------------------------------------------------------------------
// p, flag and the status record; a running frame's rr (and, behind a finished iteration, its count) is completed from the partials.
__global__ __launch_bounds__(PR_THREADS) void pressure_read_kernel(const PrWs ws, double *p, unsigned char *flag, double *status)
{
#pragma clang fp contract(off)
    __shared__ double sw[1][4];
    const unsigned N = ws.N, f = blockIdx.x / (unsigned)ws.NB, blk = blockIdx.x - f * (unsigned)ws.NB;
    const int tid = threadIdx.x;
    const size_t fo = (size_t)f * N;
    if (blk == 0) {                                                            // the whole workgroup: pr_finish synchronises it
        CgRec rec = cg_load(ws.recA + f);
        if (rec.state == PIVLFN_PRESSURE_RUNNING) {
            const double *const parts[1] = {ws.prr + (size_t)f * ws.NB};
            double top[1];
            pr_finish<1>(parts, ws.NB, sw, top);
            rec.rr = top[0];
            if (rec.phase == CG_FRESH) rec.bb = top[0];
            else rec.iters += 1;
        }
        if (tid == 0) cg_write_status(status + 4 * (size_t)f, rec);
    }
    pr_tile_for_each(ws.chunks, N, blk, [&](size_t node) {
        const size_t i = fo + node;
        const unsigned a = ws.adj[i];
        p[i] = (a & 15u) ? ws.x[i] : __longlong_as_double(0x7ff8000000000000LL);
        flag[i] = !(a & 16u) ? PIVLFN_PRESSURE_INVALID : !(a & 15u) ? PIVLFN_PRESSURE_ISOLATED : 0;
    });
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
#define PR_SHAPE(fn, F, h, w)                                                                                                   \
    PIV_REQUIRE(h >= 1 && w >= 1, fn ": bad lattice h=%d w=%d (both must be positive)", h, w);                                   \
    PIV_REQUIRE((size_t)(F) * h * w < ((size_t)1 << 31), fn ": F*h*w=%zu nodes, must stay below 2^31 (32-bit node index)", (size_t)(F) * h * w)

#define PR_WORKSPACE(fn, F, h, w, ws, ws_bytes)                                                                                 \
    PIV_REQUIRE(ws != nullptr, fn ": null pointer (the workspace is required)");                                                \
    PIV_REQUIRE(reinterpret_cast<size_t>(ws) % 8 == 0, fn ": the workspace must be 8-byte aligned");                            \
    PIV_REQUIRE(ws_bytes >= pressure_workspace_bytes(F, h, w), fn ": workspace of %zu bytes, pivlfn_pressure_workspace_bytes asks for %zu", \
                (size_t)(ws_bytes), pressure_workspace_bytes(F, h, w))

int launch_pressure_gradient(const float *flows, int B, int h, int w, double s, double nu, double *g, unsigned char *valid, hipStream_t st)
{
    PIV_REQUIRE(B >= 3, "pressure_gradient: B=%d flows, a frame needs three consecutive ones", B);
    PR_SHAPE("pressure_gradient", B - 2, h, w);
    PIV_REQUIRE(std::isfinite(s) && s > 0.0, "pressure_gradient: s=%g must be finite and positive (pixels per node)", s);
    PIV_REQUIRE(std::isfinite(nu), "pressure_gradient: nu=%g must be finite", nu);
    PIV_REQUIRE(flows && g && valid, "pressure_gradient: null pointer (flows, g and valid are required)");
    const int F = B - 2;
    const size_t N = (size_t)h * w;
    const Span in = {flows, (size_t)B * 2 * N * 4, "flows"}, grad = {g, (size_t)F * 2 * N * 8, "g"}, val = {valid, (size_t)F * N, "valid"};
    if (int rc = check_apart("pressure_gradient", grad, in)) return rc;
    if (int rc = check_apart("pressure_gradient", val, in)) return rc;
    if (int rc = check_apart("pressure_gradient", val, grad)) return rc;
    const unsigned total = (unsigned)((size_t)F * N);
    hipLaunchKernelGGL(pressure_gradient_kernel, dim3((total + PR_THREADS - 1) / PR_THREADS), dim3(PR_THREADS), 0, st, flows, F, h, w, s, nu, g,
                       valid);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

int launch_pressure_setup(const double *g, const unsigned char *valid, int F, int h, int w, double s, void *ws, size_t ws_bytes, hipStream_t st)
{
    PIV_REQUIRE(F >= 1, "pressure_setup: F=%d frames, must be positive", F);
    PR_SHAPE("pressure_setup", F, h, w);
    PIV_REQUIRE(std::isfinite(s) && s > 0.0, "pressure_setup: s=%g must be finite and positive (pixels per node)", s);
    PIV_REQUIRE(g && valid, "pressure_setup: null pointer (g and valid are required)");
    PR_WORKSPACE("pressure_setup", F, h, w, ws, ws_bytes);
    const size_t N = (size_t)h * w, need = pressure_workspace_bytes(F, h, w);
    if (int rc = check_alias_by_input("pressure_setup", {{ws, need, "the workspace"}}, {{g, (size_t)F * 2 * N * 8, "g"}, {valid, (size_t)F * N, "valid"}}, ""))
        return rc;
    const PrLayout L = pr_layout(ws, F, h, w);
    hipLaunchKernelGGL(pressure_setup_kernel, dim3((unsigned)F * (unsigned)L.ws.NB), dim3(PR_THREADS), 0, st, g, valid, s, L.ws);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

int launch_pressure_cg(void *ws, size_t ws_bytes, int F, int h, int w, double tol, int iters, hipStream_t st)
{
    PIV_REQUIRE(F >= 1, "pressure_cg: F=%d frames, must be positive", F);
    PR_SHAPE("pressure_cg", F, h, w);
    PIV_REQUIRE(std::isfinite(tol) && tol > 0.0, "pressure_cg: tol=%g must be finite and positive", tol);
    PIV_REQUIRE(iters >= 0, "pressure_cg: iters=%d must not be negative", iters);
    PR_WORKSPACE("pressure_cg", F, h, w, ws, ws_bytes);
    if (iters == 0) return PIVLFN_OK;                                          // nothing to enqueue
    const PrLayout L = pr_layout(ws, F, h, w);
    const dim3 grid((unsigned)F * (unsigned)L.ws.NB), block(PR_THREADS);
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(pressure_cg_dq_kernel, grid, block, 0, st, L.ws, tol);
        hipLaunchKernelGGL(pressure_cg_xr_kernel, grid, block, 0, st, L.ws);
    }
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

int launch_pressure_read(const void *ws, size_t ws_bytes, int F, int h, int w, double *p, unsigned char *flag, double *status, hipStream_t st)
{
    PIV_REQUIRE(F >= 1, "pressure_read: F=%d frames, must be positive", F);
    PR_SHAPE("pressure_read", F, h, w);
    PIV_REQUIRE(p && flag && status, "pressure_read: null pointer (p, flag and status are required)");
    PR_WORKSPACE("pressure_read", F, h, w, ws, ws_bytes);
    const size_t N = (size_t)h * w, need = pressure_workspace_bytes(F, h, w);
    const Span outs[] = {{p, (size_t)F * N * 8, "p"}, {flag, (size_t)F * N, "flag"}, {status, (size_t)F * 32, "status"}};
    for (int a = 0; a < 3; ++a) {
        if (int rc = check_apart("pressure_read", outs[a], {ws, need, "the workspace"})) return rc;
        for (int b = a + 1; b < 3; ++b)
            if (int rc = check_apart("pressure_read", outs[a], outs[b])) return rc;
    }
    const PrLayout L = pr_layout(const_cast<void *>(ws), F, h, w);
    hipLaunchKernelGGL(pressure_read_kernel, dim3((unsigned)F * (unsigned)L.ws.NB), dim3(PR_THREADS), 0, st, L.ws, p, flag, status);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
