// Derived fields and streaming statistics of flow batches (gfx950): the reference's src/postpro.py (calc_vorticity :5-24,
// de_vort :27-50) and the per-pixel power sums a PIV sequence reports (mean, RMS, Reynolds stress, mean vorticity).
// Both kernels read a [B,2,H,W] NCHW flow -- what estimate(..., tensor=True) returns -- and work on the 3 x 3 neighbourhood
// of each pixel, the image edge repeated.  One thread per pixel.  Arithmetic contract: include/pivlfn.h.
#include <cmath>
#include "launch_checks.h"

namespace pivlfn {

struct PostproParams {
    double kv[9];       // calc_vorticity's taps for dv, K = [[1,0,-1],[2,0,-2],[1,0,-1]] / (8 calib), row-major
    double ku[9];       // ... and for du, -K^T (its zero taps carry the opposite sign of K's)
    float d32;          // de_vort's divisor, float32(8 calib)
    int H, W;
};

// The 3 x 3 neighbourhood of (y, x) in one plane, edge pixels repeated: n[r][c] = x[clamp(y + r - 1), clamp(x + c - 1)].
__device__ __forceinline__ void load3x3(const float *__restrict__ p, int y, int x, int H, int W, float n[3][3])
{
    const int ys[3] = {y > 0 ? y - 1 : 0, y, y + 1 < H ? y + 1 : H - 1};
    const int xs[3] = {x > 0 ? x - 1 : 0, x, x + 1 < W ? x + 1 : W - 1};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) n[r][c] = p[(unsigned)ys[r] * (unsigned)W + (unsigned)xs[c]];
}

// scipy.signal.convolve2d(x, k, 'same', boundary='symm') at one pixel: the taps of k in row-major order, k[p][q] times
// x[y + 1 - p, x + 1 - q], summed from +0.0 with every product rounded before it is added.  Zero taps included (0 * inf = NaN).
__device__ __forceinline__ double conv3x3(const double *k, const float n[3][3])
{
#pragma clang fp contract(off)
    double s = 0.0;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) s = s + k[3 * p + q] * (double)n[2 - p][2 - q];
    return s;
}

// calc_vorticity: dv = v conv K, du = u conv (-K^T); vort = dv - du, shear = dv + du, normal = -(dv + du)
__device__ __forceinline__ void calc_vorticity_at(const PostproParams &p, const float nu[3][3], const float nv[3][3], double o[3])
{
#pragma clang fp contract(off)
    const double dv = conv3x3(p.kv, nv), du = conv3x3(p.ku, nu);
    o[0] = dv - du;
    o[1] = dv + du;
    o[2] = -(dv + du);
}

// de_vort: fp32 sums over the edge-padded planes (the middle taps are not evaluated), divided in fp32; vort in fp64
__device__ __forceinline__ void de_vort_at(const PostproParams &p, const float nu[3][3], const float nv[3][3], double o[3])
{
#pragma clang fp contract(off)
    const float vx = (((nv[2][2] + 2.0f * nv[1][2]) + nv[0][2]) - ((nv[2][0] + 2.0f * nv[1][0]) + nv[0][0])) / p.d32;
    const float uy = (((nu[0][0] + 2.0f * nu[0][1]) + nu[0][2]) - ((nu[2][0] + 2.0f * nu[2][1]) + nu[2][2])) / p.d32;
    o[0] = (double)vx - (double)uy;
    o[1] = (double)uy;
    o[2] = (double)vx;
}

// flow [B,2,H,W] -> out [B,3,H,W] (T = double, or float: the fp64 result rounded once).  blockIdx.y = frame; 32-bit pixel
// index within a frame (the host checks H*W < 2^31): no 64-bit division in the index math.
template <int KIND, typename T>
__global__ __launch_bounds__(256) void flow_fields_kernel(const float *__restrict__ flow, T *__restrict__ out, const PostproParams p)
{
    const unsigned HW = (unsigned)p.H * (unsigned)p.W;
    const float *u = flow + (size_t)blockIdx.y * 2 * HW, *v = u + HW;
    T *o = out + (size_t)blockIdx.y * 3 * HW;
    for (unsigned pix = blockIdx.x * 256 + threadIdx.x; pix < HW; pix += gridDim.x * 256) {
        const int y = (int)(pix / (unsigned)p.W), x = (int)(pix - (unsigned)y * (unsigned)p.W);
        float nu[3][3], nv[3][3];
        load3x3(u, y, x, p.H, p.W, nu);
        load3x3(v, y, x, p.H, p.W, nv);
        double r[3];
        if (KIND == PIVLFN_FIELDS_CALC_VORTICITY)
            calc_vorticity_at(p, nu, nv, r);
        else
            de_vort_at(p, nu, nv, r);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[(size_t)c * HW + pix] = (T)r[c];
    }
}

// acc [7,H,W] fp64 += (u, v, u*u, v*v, u*v, w, w*w) of frames 0..B-1 in frame order, w = calc_vorticity's vort.  acc is read
// and written once per call, so any split of a sequence into calls gives the same bits.
__global__ __launch_bounds__(256) void flow_stats_kernel(const float *__restrict__ flow, double *__restrict__ acc, int B,
                                                         const PostproParams p)
{
#pragma clang fp contract(off)
    const unsigned HW = (unsigned)p.H * (unsigned)p.W;
    for (unsigned pix = blockIdx.x * 256 + threadIdx.x; pix < HW; pix += gridDim.x * 256) {
        const int y = (int)(pix / (unsigned)p.W), x = (int)(pix - (unsigned)y * (unsigned)p.W);
        double s[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) s[k] = acc[(size_t)k * HW + pix];
        for (int b = 0; b < B; ++b) {
            const float *u = flow + (size_t)b * 2 * HW, *v = u + HW;
            float nu[3][3], nv[3][3];
            load3x3(u, y, x, p.H, p.W, nu);
            load3x3(v, y, x, p.H, p.W, nv);
            double r[3];
            calc_vorticity_at(p, nu, nv, r);
            const double u0 = (double)nu[1][1], v0 = (double)nv[1][1], w = r[0];
            s[0] = s[0] + u0;
            s[1] = s[1] + v0;
            s[2] = s[2] + u0 * u0;
            s[3] = s[3] + v0 * v0;
            s[4] = s[4] + u0 * v0;
            s[5] = s[5] + w;
            s[6] = s[6] + w * w;
        }
#pragma unroll
        for (int k = 0; k < 7; ++k) acc[(size_t)k * HW + pix] = s[k];
    }
}

// flow_stats_kernel with a flag byte per frame and pixel (flow_validate's): frame b adds to u, v, uu, vv, uv only where its flag is 0
// and to w, ww only where the flags of all nine edge-clamped 3 x 3 neighbours are 0; cnt [2,H,W] counts both kinds of additions.
// A term that is left out is not computed into the sum at all (no 0 * NaN), so an all-zero flag gives flow_stats_kernel's bits.
__global__ __launch_bounds__(256) void flow_stats_masked_kernel(const float *__restrict__ flow, const unsigned char *__restrict__ flag,
                                                                double *__restrict__ acc, double *__restrict__ cnt, int B,
                                                                const PostproParams p)
{
#pragma clang fp contract(off)
    const unsigned HW = (unsigned)p.H * (unsigned)p.W;
    for (unsigned pix = blockIdx.x * 256 + threadIdx.x; pix < HW; pix += gridDim.x * 256) {
        const int y = (int)(pix / (unsigned)p.W), x = (int)(pix - (unsigned)y * (unsigned)p.W);
        const int ys[3] = {y > 0 ? y - 1 : 0, y, y + 1 < p.H ? y + 1 : p.H - 1};
        const int xs[3] = {x > 0 ? x - 1 : 0, x, x + 1 < p.W ? x + 1 : p.W - 1};
        double s[7], c0 = cnt[pix], c1 = cnt[(size_t)HW + pix];
#pragma unroll
        for (int k = 0; k < 7; ++k) s[k] = acc[(size_t)k * HW + pix];
        for (int b = 0; b < B; ++b) {
            const float *u = flow + (size_t)b * 2 * HW, *v = u + HW;
            const unsigned char *f = flag + (size_t)b * HW;
            unsigned any = 0;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) any |= f[(unsigned)ys[r] * (unsigned)p.W + (unsigned)xs[c]];
            if (f[pix] == 0) {
                const double u0 = (double)u[pix], v0 = (double)v[pix];
                s[0] = s[0] + u0;
                s[1] = s[1] + v0;
                s[2] = s[2] + u0 * u0;
                s[3] = s[3] + v0 * v0;
                s[4] = s[4] + u0 * v0;
                c0 = c0 + 1.0;
            }
            if (any == 0) {
                float nu[3][3], nv[3][3];
                load3x3(u, y, x, p.H, p.W, nu);
                load3x3(v, y, x, p.H, p.W, nv);
                double r[3];
                calc_vorticity_at(p, nu, nv, r);
                s[5] = s[5] + r[0];
                s[6] = s[6] + r[0] * r[0];
                c1 = c1 + 1.0;
            }
        }
#pragma unroll
        for (int k = 0; k < 7; ++k) acc[(size_t)k * HW + pix] = s[k];
        cnt[pix] = c0;
        cnt[(size_t)HW + pix] = c1;
    }
}

// Host-side checks shared by both entry points; fills the taps.
static int postpro_params(const char *what, int B, int H, int W, double calib, PostproParams &p)
{
    if (int rc = check_shape(what, B, H, W, "frames", false)) return rc;      // flow_fields bounds B itself, after calib
    PIV_REQUIRE(std::isfinite(calib) && calib != 0.0, "%s: calib=%g must be finite and non-zero", what, calib);
    const double d = 8.0 * calib;
    PIV_REQUIRE(std::isfinite(d), "%s: calib=%g must be finite and non-zero, and 8*calib finite", what, calib);
    static const double K[9] = {1, 0, -1, 2, 0, -2, 1, 0, -1};
    double kd[9];
    for (int i = 0; i < 9; ++i) kd[i] = K[i] / d;                         // each element divided in fp64, as numpy does
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            p.kv[3 * r + c] = kd[3 * r + c];
            p.ku[3 * r + c] = -kd[3 * c + r];
        }
    p.d32 = (float)d;                                                     // numpy >= 2: a Python float meets a float32 array
    p.H = H;
    p.W = W;
    return PIVLFN_OK;
}

int launch_flow_fields(const float *flow, void *out, int B, int H, int W, double calib, int kind, int out_f64, hipStream_t st)
{
    PIV_REQUIRE(flow && out, "flow_fields: null pointer (flow and out are required)");
    PostproParams p;
    const int rc = postpro_params("flow_fields", B, H, W, calib, p);
    if (rc != PIVLFN_OK) return rc;
    PIV_REQUIRE(B <= 65535, "flow_fields: B=%d frames, at most 65535 per call (grid y dimension)", B);
    PIV_REQUIRE(kind == PIVLFN_FIELDS_CALC_VORTICITY || kind == PIVLFN_FIELDS_DE_VORT,
                "flow_fields: unknown kind=%d (PIVLFN_FIELDS_CALC_VORTICITY 0 or PIVLFN_FIELDS_DE_VORT 1)", kind);
    PIV_REQUIRE(out_f64 == 0 || out_f64 == 1, "flow_fields: out_f64=%d must be 0 (fp32) or 1 (fp64)", out_f64);
    const dim3 grid(frame_grid((size_t)H * W, B), (unsigned)B);
    if (kind == PIVLFN_FIELDS_CALC_VORTICITY) {
        if (out_f64)
            hipLaunchKernelGGL((flow_fields_kernel<PIVLFN_FIELDS_CALC_VORTICITY, double>), grid, dim3(256), 0, st, flow, (double *)out, p);
        else
            hipLaunchKernelGGL((flow_fields_kernel<PIVLFN_FIELDS_CALC_VORTICITY, float>), grid, dim3(256), 0, st, flow, (float *)out, p);
    } else {
        if (out_f64)
            hipLaunchKernelGGL((flow_fields_kernel<PIVLFN_FIELDS_DE_VORT, double>), grid, dim3(256), 0, st, flow, (double *)out, p);
        else
            hipLaunchKernelGGL((flow_fields_kernel<PIVLFN_FIELDS_DE_VORT, float>), grid, dim3(256), 0, st, flow, (float *)out, p);
    }
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

int launch_flow_stats(const float *flow, double *acc, int B, int H, int W, double calib, hipStream_t st)
{
    PIV_REQUIRE(flow && acc, "flow_stats_accumulate: null pointer (flow and acc are required)");
    PostproParams p;
    const int rc = postpro_params("flow_stats_accumulate", B, H, W, calib, p);
    if (rc != PIVLFN_OK) return rc;
    hipLaunchKernelGGL(flow_stats_kernel, dim3(frame_grid((size_t)H * W, 1)), dim3(256), 0, st, flow, acc, B, p);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

int launch_flow_stats_masked(const float *flow, const unsigned char *flag, double *acc, double *cnt, int B, int H, int W, double calib,
                             hipStream_t st)
{
    PIV_REQUIRE(flow && flag && acc && cnt, "flow_stats_accumulate_masked: null pointer (flow, flag, acc and cnt are required)");
    PostproParams p;
    const int rc = postpro_params("flow_stats_accumulate_masked", B, H, W, calib, p);
    if (rc != PIVLFN_OK) return rc;
    hipLaunchKernelGGL(flow_stats_masked_kernel, dim3(frame_grid((size_t)H * W, 1)), dim3(256), 0, st, flow, flag, acc, cnt, B, p);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
