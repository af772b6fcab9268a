// Lagrangian flow maps of a flow sequence (gfx950): particles carried through consecutive displacement fields, and the largest
// stretching of the map they trace out (whose logarithm over the interval is the finite-time Lyapunov exponent).  An estimated flow
// is a displacement field -- F_k(x) is where the content at pixel x of frame k sits in frame k+1 -- so a step is one bilinear gather
// at the particle's position and one addition; nothing is integrated.  Arithmetic contract: include/pivlfn.h.
//
// flowmap_advect_kernel, one thread per particle: position and flag live in registers while the loop over the B fields of the call
// runs INSIDE the kernel, so a batch is one launch and the state is read and written once however many fields it passes.  The four
// corners of a sample are read straight from global memory, not through LDS: where a particle samples field k is known only after
// field k-1 has moved it, so a tile staged for a workgroup would need a halo as wide as the displacement accumulated over the whole
// call, and each staged vector would be used about once -- the reuse LDS pays for is not there.  What reuse there is sits in the
// caches already: a lattice of seeds stays spatially coherent, so the 64 lanes of a wave read four short runs of neighbouring floats
// per plane, and the lanes of the next row of seeds find those lines in L1 / L2.  A frozen lane (nonzero flag) skips the step and
// idles to the trace store and the next field; it takes no early return.
// flowmap_ftle_kernel, one thread per lattice node: four differences of neighbouring particles, the larger eigenvalue of the
// Cauchy-Green tensor in closed form and two square roots.  The logarithm is left to the caller (the device's log is not correctly
// rounded; a contract of bits cannot hold it).
#include <cmath>
#include "launch_checks.h"

namespace pivlfn {

constexpr unsigned FM_OUT = PIVLFN_FLOWMAP_OUT, FM_LOST = PIVLFN_FLOWMAP_LOST, FM_UNDEFINED = PIVLFN_FLOWMAP_UNDEFINED;

// S_k(x, y): 0 and the interpolated vector, or the flag the sample sets.  32-bit pixel index (the host checks H*W < 2^31).
__device__ __forceinline__ unsigned flowmap_sample(const float *__restrict__ u, const float *__restrict__ v,
                                                   const unsigned char *__restrict__ m, int H, int W, double x, double y, double &su,
                                                   double &sv)
{
#pragma clang fp contract(off)
    if (!(x >= 0.0 && x <= (double)(W - 1) && y >= 0.0 && y <= (double)(H - 1))) return FM_OUT;      // NaN compares false
    int ix = (int)floor(x), iy = (int)floor(y);
    ix = ix < W - 2 ? ix : W - 2;
    iy = iy < H - 2 ? iy : H - 2;
    const unsigned at = (unsigned)iy * (unsigned)W + (unsigned)ix, below = at + (unsigned)W;
    const double u00 = (double)u[at], u01 = (double)u[at + 1], u10 = (double)u[below], u11 = (double)u[below + 1];
    const double v00 = (double)v[at], v01 = (double)v[at + 1], v10 = (double)v[below], v11 = (double)v[below + 1];
    bool known = fabs(u00) <= 1e9 && fabs(u01) <= 1e9 && fabs(u10) <= 1e9 && fabs(u11) <= 1e9 &&
                 fabs(v00) <= 1e9 && fabs(v01) <= 1e9 && fabs(v10) <= 1e9 && fabs(v11) <= 1e9;
    if (m) known = known && (m[at] | m[at + 1] | m[below] | m[below + 1]) == 0;
    if (!known) return FM_LOST;
    const double fx = x - (double)ix, fy = y - (double)iy, gx = 1.0 - fx, gy = 1.0 - fy;
    const double ut = gx * u00 + fx * u01, ub = gx * u10 + fx * u11;
    const double vt = gx * v00 + fx * v01, vb = gx * v10 + fx * v11;
    su = ut * gy + ub * fy;
    sv = vt * gy + vb * fy;
    return 0u;
}

__global__ __launch_bounds__(256) void flowmap_advect_kernel(const float *__restrict__ flows, const unsigned char *__restrict__ mask, int B,
                                                             int H, int W, double *__restrict__ pos, unsigned char *__restrict__ flag, int N,
                                                             int backward, int iters, double *__restrict__ trace)
{
#pragma clang fp contract(off)
    const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= (size_t)N) return;
    const size_t HW = (size_t)H * (size_t)W;
    double x = pos[n], y = pos[(size_t)N + n];
    unsigned f = flag[n];
    for (int k = 0; k < B; ++k) {
        const float *u = flows + (size_t)k * 2 * HW, *v = u + HW;
        const unsigned char *m = mask ? mask + (size_t)k * HW : nullptr;
        if (f == 0) {
            double su = 0.0, sv = 0.0;
            if (!backward) {
                f = flowmap_sample(u, v, m, H, W, x, y, su, sv);
                if (f == 0) {
                    x = x + su;
                    y = y + sv;
                }
            } else {                                                // p_i = (x, y) - S_k(p_{i-1}), exactly `iters` times
                double px = x, py = y;
                for (int i = 0; i < iters && f == 0; ++i) {
                    f = flowmap_sample(u, v, m, H, W, px, py, su, sv);
                    if (f == 0) {
                        px = x - su;
                        py = y - sv;
                    }
                }
                if (f == 0) {
                    x = px;
                    y = py;
                }
            }
        }
        if (trace) {
            trace[(size_t)k * 2 * N + n] = x;
            trace[(size_t)k * 2 * N + (size_t)N + n] = y;
        }
    }
    pos[n] = x;
    pos[(size_t)N + n] = y;
    flag[n] = (unsigned char)f;
}

__global__ __launch_bounds__(256) void flowmap_seed_kernel(double *__restrict__ pos, unsigned char *__restrict__ flag, int h, int w, int spacing)
{
    const unsigned N = (unsigned)h * (unsigned)w, n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const unsigned i = n / (unsigned)w, j = n - i * (unsigned)w;
    pos[n] = (double)(j * (unsigned)spacing);                       // below 2^31: the host checks (w - 1) * spacing and (h - 1) * spacing
    pos[(size_t)N + n] = (double)(i * (unsigned)spacing);
    flag[n] = 0;
}

__global__ __launch_bounds__(256) void flowmap_ftle_kernel(const double *__restrict__ pos, const unsigned char *__restrict__ flag, int h, int w,
                                                           int spacing, double *__restrict__ stretch, unsigned char *__restrict__ oflag)
{
#pragma clang fp contract(off)
    const unsigned N = (unsigned)h * (unsigned)w, n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int i = (int)(n / (unsigned)w), j = (int)(n - (unsigned)i * (unsigned)w);
    const int jl = j > 0 ? j - 1 : 0, jr = j < w - 1 ? j + 1 : w - 1, iu = i > 0 ? i - 1 : 0, id = i < h - 1 ? i + 1 : h - 1;
    const unsigned l = (unsigned)i * w + jl, r = (unsigned)i * w + jr, up = (unsigned)iu * w + j, dn = (unsigned)id * w + j;
    const double *X = pos, *Y = pos + N;
    const unsigned own = flag[n];
    const bool undefined = (own | flag[l] | flag[r] | flag[up] | flag[dn]) != 0 || h < 2 || w < 2;
    const double dx = (double)((jr - jl) * spacing), dy = (double)((id - iu) * spacing);
    const double a = (X[r] - X[l]) / dx, b = (X[dn] - X[up]) / dy;
    const double c = (Y[r] - Y[l]) / dx, d = (Y[dn] - Y[up]) / dy;
    const double c11 = a * a + c * c, c22 = b * b + d * d, c12 = a * b + c * d;
    const double g = 0.5 * (c11 - c22);
    const double lam = 0.5 * (c11 + c22) + sqrt(g * g + c12 * c12);
    stretch[n] = undefined ? __builtin_nan("") : sqrt(lam);
    oflag[n] = (unsigned char)(own | (undefined ? FM_UNDEFINED : 0u));
}

int launch_flowmap_advect(const float *flows, const unsigned char *mask, int B, int H, int W, double *pos, unsigned char *flag, int N,
                          int backward, int iters, double *trace, hipStream_t st)
{
    PIV_REQUIRE(H >= 2 && W >= 2, "flowmap_advect: bad shape H=%d W=%d (a bilinear sample needs 2 x 2 vectors)", H, W);
    PIV_REQUIRE((size_t)H * W < ((size_t)1 << 31), "flowmap_advect: H*W=%zu pixels, must stay below 2^31 (32-bit pixel index)", (size_t)H * W);
    PIV_REQUIRE(B >= 0, "flowmap_advect: B=%d fields, must not be negative", B);
    PIV_REQUIRE(N >= 0, "flowmap_advect: N=%d particles, must not be negative", N);
    PIV_REQUIRE(backward == 0 || backward == 1, "flowmap_advect: backward=%d must be 0 or 1", backward);
    PIV_REQUIRE(iters >= 1 && iters <= 32, "flowmap_advect: iters=%d must be 1..32, the fixed-point iterations of a backward step", iters);
    if (N == 0 || B == 0) return PIVLFN_OK;                         // nothing to move, nothing to move through: no pointer is read
    PIV_REQUIRE(flows && pos && flag, "flowmap_advect: null pointer (flows, pos and flag are required)");
    const size_t px = (size_t)B * H * W;
    const Span ps = {pos, (size_t)N * 16, "pos"}, flg = {flag, (size_t)N, "flag"}, trc = {trace, (size_t)B * N * 16, "trace"};
    if (int rc = check_alias_by_output("flowmap_advect", {ps, flg, trc}, {{flows, px * 8, "flows"}, {mask, px, "mask"}},
                                       " (the state and the trace must not alias an input)"))
        return rc;
    if (int rc = check_apart("flowmap_advect", ps, flg)) return rc;
    if (int rc = check_apart("flowmap_advect", trc, ps)) return rc;
    if (int rc = check_apart("flowmap_advect", trc, flg)) return rc;
    hipLaunchKernelGGL(flowmap_advect_kernel, dim3((unsigned)(((size_t)N + 255) / 256)), dim3(256), 0, st, flows, mask, B, H, W, pos, flag, N,
                       backward, iters, trace);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

static int flowmap_lattice_ok(const char *what, int h, int w, int spacing)
{
    PIV_REQUIRE(h >= 1 && w >= 1, "%s: bad lattice h=%d w=%d (both must be positive)", what, h, w);
    PIV_REQUIRE((size_t)h * w < ((size_t)1 << 31), "%s: h*w=%zu nodes, must stay below 2^31 (32-bit node index)", what, (size_t)h * w);
    PIV_REQUIRE(spacing >= 1 && spacing <= 32768, "%s: spacing=%d must be 1..32768 pixels", what, spacing);
    PIV_REQUIRE((size_t)(h - 1) * spacing < ((size_t)1 << 31) && (size_t)(w - 1) * spacing < ((size_t)1 << 31),
                "%s: the lattice h=%d w=%d at spacing=%d reaches past pixel 2^31", what, h, w, spacing);
    return PIVLFN_OK;
}

int launch_flowmap_seed(double *pos, unsigned char *flag, int h, int w, int spacing, hipStream_t st)
{
    if (int rc = flowmap_lattice_ok("flowmap_seed", h, w, spacing)) return rc;
    PIV_REQUIRE(pos && flag, "flowmap_seed: null pointer (pos and flag are required)");
    const size_t N = (size_t)h * w;
    if (int rc = check_apart("flowmap_seed", {pos, N * 16, "pos"}, {flag, N, "flag"})) return rc;
    hipLaunchKernelGGL(flowmap_seed_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, pos, flag, h, w, spacing);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

int launch_flowmap_ftle(const double *pos, const unsigned char *flag, int h, int w, int spacing, double *stretch, unsigned char *oflag,
                        hipStream_t st)
{
    if (int rc = flowmap_lattice_ok("flowmap_ftle", h, w, spacing)) return rc;
    PIV_REQUIRE(pos && flag && stretch && oflag, "flowmap_ftle: null pointer (pos, flag, stretch and oflag are required)");
    const size_t N = (size_t)h * w;
    const Span str = {stretch, N * 8, "stretch"}, ofl = {oflag, N, "oflag"};
    if (int rc = check_alias_by_input("flowmap_ftle", {str, ofl}, {{pos, N * 16, "pos"}, {flag, N, "flag"}}, " (outputs must not alias an input)"))
        return rc;
    if (int rc = check_apart("flowmap_ftle", str, ofl)) return rc;
    hipLaunchKernelGGL(flowmap_ftle_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, pos, flag, h, w, spacing, stretch, oflag);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
