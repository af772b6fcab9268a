// Per-vector uncertainty of an estimated flow from correlation statistics (gfx950; Wieneke 2015): how asymmetric the correlation peak
// of image 1 against image 2 warped back by the flow may be, given the pixel-wise scatter of the products it is summed from, carried
// through the three-point Gaussian peak fit.  Arithmetic contract: include/pivlfn.h.
//
// Five kernels through the workspace.  quality.hip's warp kernel (launch_quality_warp): the gray values a, b and the byte of m and k.
// unc_highpass_kernel: a and b minus their means over the valid pixels of the (2r+1)^2 window.  unc_fields_kernel, one thread per
// pixel: the products p, s_e, d_e and a byte (bit 0: the pixel is valid, bit 1 / 2: so is its right / lower neighbour).
// unc_lagbox_kernel: g_e = d_e times the sum of d_e over the (2 lag+1)^2 box.  unc_window_kernel: the window sums and the finish.
//
// The three windowed kernels share one routine, box_sum: one workgroup per 32 x 32 tile stages one fp64 plane of the tile plus a halo
// of the box radius in LDS and forms the box sums in the contract's order -- per row left to right from +0.0, then the row sums top
// to bottom from +0.0 -- as a horizontal pass (row sums of 32 + 2r rows, kept in LDS) and a vertical one.  A term outside the image is
// +0.0 and a sum that starts at +0.0 never becomes -0.0, so x + 0.0 == x bit for bit: the clipped window is a full window over zero
// padding.  As in quality.hip a lane keeps 4 neighbouring outputs and adds every term it reads to those whose window holds it, the
// others get + 0.0.  The planes of a kernel go through the same LDS one after the other; the counts go through as one plane too (a
// valid pixel is 1.0, a valid x pair 1024.0, a valid y pair 1048576.0: a window holds at most 961 of each, the sum is exact in any
// order and is taken apart again as an integer).  At r = 15 the plane and its row sums take 46 KB of LDS: three workgroups on a CU.
#include <cmath>
#include "launch_checks.h"

namespace pivlfn {

constexpr int UQ_T = 32;              // the tile is UQ_T x UQ_T
constexpr int UQ_THREADS = 256;
constexpr int UQ_G = 4;               // outputs per lane: 4 neighbours along x in the horizontal pass, 4 along y in the vertical one

struct UncParams {
    const double *a, *b;              // [B,H,W] the planes the kernel reads (per kernel: see its comment)
    const double *c, *d, *e;
    const unsigned char *f;           // [B,H,W] the bytes the kernel reads
    double *o0, *o1;                  // [B,H,W] fp64 outputs
    float *unc;                       // [B,2,H,W]
    unsigned char *flag;              // [B,H,W]
    int H, W, r, min_count, tiles_x;
    double floor2;                    // floor * floor
};

// The box sums of radius r of one plane for this lane's UQ_G outputs: column (t & 31), rows 4 (t >> 5) .. + 3 of the tile whose
// first pixel is (y0, x0).  load(at) gives the term of pixel `at` of the frame.  All threads of the workgroup call it; it starts with
// a barrier (the plane before has been read).
template <class Load>
__device__ __forceinline__ void box_sum(double *sP, double *sH, int r, int y0, int x0, int H, int W, Load load, double (&out)[UQ_G])
{
#pragma clang fp contract(off)
    const int t = threadIdx.x, RW = UQ_T + 2 * r, RH = UQ_T + 2 * r;
    const unsigned span = 2u * (unsigned)r;
    __syncthreads();
    for (int i = t; i < RH * RW; i += UQ_THREADS) {
        const int ly = i / RW, lx = i - ly * RW, gy = y0 - r + ly, gx = x0 - r + lx;
        double term = 0.0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) term = load((unsigned)gy * (unsigned)W + (unsigned)gx);
        sP[i] = term;
    }
    __syncthreads();
    // rows: output column x of a staged row adds the staged columns x .. x + 2r, left to right
    for (int item = t; item < RH * (UQ_T / UQ_G); item += UQ_THREADS) {
        const int j = item >> 3, gx = item & 7, at = j * RW + UQ_G * gx;
        double acc[UQ_G];
#pragma unroll
        for (int g = 0; g < UQ_G; ++g) acc[g] = 0.0;
        for (int i = 0; i < 2 * r + UQ_G; ++i) {
            const double term = sP[at + i];
#pragma unroll
            for (int g = 0; g < UQ_G; ++g) acc[g] = acc[g] + ((unsigned)(i - g) <= span ? term : 0.0);
        }
#pragma unroll
        for (int g = 0; g < UQ_G; ++g) sH[j * UQ_T + UQ_G * gx + g] = acc[g];
    }
    __syncthreads();
    // columns: output row y adds the row sums y .. y + 2r, top to bottom
    const int x = t & 31, yg = t >> 5;
#pragma unroll
    for (int g = 0; g < UQ_G; ++g) out[g] = 0.0;
    for (int i = 0; i < 2 * r + UQ_G; ++i) {
        const double h = sH[(UQ_G * yg + i) * UQ_T + x];
#pragma unroll
        for (int g = 0; g < UQ_G; ++g) out[g] = out[g] + ((unsigned)(i - g) <= span ? h : 0.0);
    }
}

// where a workgroup's tile lies and which outputs a lane owns
struct UncTile {
    double *sP, *sH;                  // LDS: the staged plane [32 + 2r][32 + 2r], its row sums [32 + 2r][32]
    int y0, x0;                       // the tile's first pixel
    int x, yl;                        // this lane's column in the frame and the first of its UQ_G rows in the tile
    unsigned HW;
    size_t frame;                     // the pair's offset in a [B,H,W] plane
};

__device__ __forceinline__ UncTile unc_tile(const UncParams &p)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int side = UQ_T + 2 * p.r, t = threadIdx.x;
    const int ty = (int)blockIdx.x / p.tiles_x, tx = (int)blockIdx.x - ty * p.tiles_x;
    UncTile w;
    w.sP = reinterpret_cast<double *>(smem);
    w.sH = w.sP + side * side;
    w.y0 = ty * UQ_T, w.x0 = tx * UQ_T;
    w.x = w.x0 + (t & 31), w.yl = UQ_G * (t >> 5);
    w.HW = (unsigned)p.H * (unsigned)p.W;
    w.frame = (size_t)blockIdx.y * w.HW;
    return w;
}

// a, b, f: the warp kernel's outputs.  o0, o1: a', b' (+0.0 where the pixel is not valid).
__global__ __launch_bounds__(UQ_THREADS) void unc_highpass_kernel(const UncParams p)
{
#pragma clang fp contract(off)
    const UncTile w = unc_tile(p);
    const int r = p.r, x = w.x;
    const size_t frame = w.frame;
    const double *a = p.a + frame, *b = p.b + frame;
    const unsigned char *f = p.f + frame;
    double n1[UQ_G], A1[UQ_G], B1[UQ_G];
    box_sum(w.sP, w.sH, r, w.y0, w.x0, p.H, p.W, [&](unsigned at) { return (f[at] & 3) == 3 ? 1.0 : 0.0; }, n1);
    box_sum(w.sP, w.sH, r, w.y0, w.x0, p.H, p.W, [&](unsigned at) { return (f[at] & 3) == 3 ? a[at] : 0.0; }, A1);
    box_sum(w.sP, w.sH, r, w.y0, w.x0, p.H, p.W, [&](unsigned at) { return (f[at] & 3) == 3 ? b[at] : 0.0; }, B1);
#pragma unroll
    for (int g = 0; g < UQ_G; ++g) {
        const int y = w.y0 + w.yl + g;
        if (y >= p.H || x >= p.W) continue;
        const unsigned at = (unsigned)y * (unsigned)p.W + (unsigned)x;
        const bool v = (f[at] & 3) == 3;
        p.o0[frame + at] = v ? a[at] - A1[g] / n1[g] : 0.0;
        p.o1[frame + at] = v ? b[at] - B1[g] / n1[g] : 0.0;
    }
}

// blockIdx.y = pair, 32-bit pixel index within a frame.  ha, hb: a', b'; wf: the warp kernel's bytes.
__global__ __launch_bounds__(256) void unc_fields_kernel(const double *__restrict__ ha, const double *__restrict__ hb,
                                                         const unsigned char *__restrict__ wf, double *__restrict__ pp,
                                                         double *__restrict__ sx, double *__restrict__ sy, double *__restrict__ dx,
                                                         double *__restrict__ dy, unsigned char *__restrict__ code, int H, int W)
{
#pragma clang fp contract(off)
    const unsigned HW = (unsigned)H * (unsigned)W;
    const size_t frame = (size_t)blockIdx.y * HW;
    ha += frame, hb += frame, wf += frame;
    for (unsigned pix = blockIdx.x * 256 + threadIdx.x; pix < HW; pix += gridDim.x * 256) {
        const int y = (int)(pix / (unsigned)W), x = (int)(pix - (unsigned)y * (unsigned)W);
        const bool v = (wf[pix] & 3) == 3;
        const bool px = v && x + 1 < W && (wf[pix + 1] & 3) == 3, py = v && y + 1 < H && (wf[pix + (unsigned)W] & 3) == 3;
        const double a0 = ha[pix], b0 = hb[pix];
        double s[2] = {0.0, 0.0}, d[2] = {0.0, 0.0};
        if (px) {
            const double t1 = a0 * hb[pix + 1], t2 = ha[pix + 1] * b0;
            s[0] = t1 + t2, d[0] = t1 - t2;
        }
        if (py) {
            const double t1 = a0 * hb[pix + (unsigned)W], t2 = ha[pix + (unsigned)W] * b0;
            s[1] = t1 + t2, d[1] = t1 - t2;
        }
        pp[frame + pix] = v ? a0 * b0 : 0.0;
        sx[frame + pix] = s[0], sy[frame + pix] = s[1];
        dx[frame + pix] = d[0], dy[frame + pix] = d[1];
        code[frame + pix] = (unsigned char)((v ? 1 : 0) | (px ? 2 : 0) | (py ? 4 : 0));
    }
}

// a, b: d_x, d_y; f: the fields kernel's bytes; r: the lag.  o0, o1: g_x, g_y.
__global__ __launch_bounds__(UQ_THREADS) void unc_lagbox_kernel(const UncParams p)
{
#pragma clang fp contract(off)
    const UncTile w = unc_tile(p);
    const int r = p.r, x = w.x;
    const size_t frame = w.frame;
    const double *dx = p.a + frame, *dy = p.b + frame;
    const unsigned char *f = p.f + frame;
    double Dx[UQ_G], Dy[UQ_G];
    box_sum(w.sP, w.sH, r, w.y0, w.x0, p.H, p.W, [&](unsigned at) { return dx[at]; }, Dx);
    box_sum(w.sP, w.sH, r, w.y0, w.x0, p.H, p.W, [&](unsigned at) { return dy[at]; }, Dy);
#pragma unroll
    for (int g = 0; g < UQ_G; ++g) {
        const int y = w.y0 + w.yl + g;
        if (y >= p.H || x >= p.W) continue;
        const unsigned at = (unsigned)y * (unsigned)p.W + (unsigned)x;
        const unsigned char c = f[at];
        p.o0[frame + at] = (c & 2) ? dx[at] * Dx[g] : 0.0;
        p.o1[frame + at] = (c & 4) ? dy[at] * Dy[g] : 0.0;
    }
}

// one axis: the bits NO_PEAK and NO_VARIANCE it sets, and Cm, Cp
__device__ __forceinline__ unsigned unc_axis(double C0, double S, double V, double &Cm, double &Cp)
{
#pragma clang fp contract(off)
    const double sig = sqrt(V), Cpm = 0.5 * S;
    Cm = Cpm - 0.5 * sig;
    Cp = Cpm + 0.5 * sig;
    unsigned bits = 0;
    if (Cm <= 0.0 || C0 - Cp < 1e-6 * C0) bits |= 4u;
    if (V <= 0.0 || !(fabs(V) < __builtin_inf())) bits |= 8u;
    return bits;
}

// a: p; b, c: s_x, g_x; d, e: s_y, g_y; f: the fields kernel's bytes.
__global__ __launch_bounds__(UQ_THREADS) void unc_window_kernel(const UncParams p)
{
#pragma clang fp contract(off)
    const UncTile w = unc_tile(p);
    const int r = p.r, x = w.x;
    const size_t frame = w.frame;
    const double *pp = p.a + frame, *sx = p.b + frame, *gx = p.c + frame, *sy = p.d + frame, *gy = p.e + frame;
    const unsigned char *f = p.f + frame;
    double N[UQ_G], C0[UQ_G], Sx[UQ_G], Vx[UQ_G], Sy[UQ_G], Vy[UQ_G];
    box_sum(w.sP, w.sH, r, w.y0, w.x0, p.H, p.W, [&](unsigned at) {
        const unsigned c = f[at];
        return (double)((c & 1u) + ((c & 2u) << 9) + ((c & 4u) << 18));
    }, N);
    box_sum(w.sP, w.sH, r, w.y0, w.x0, p.H, p.W, [&](unsigned at) { return pp[at]; }, C0);
    box_sum(w.sP, w.sH, r, w.y0, w.x0, p.H, p.W, [&](unsigned at) { return sx[at]; }, Sx);
    box_sum(w.sP, w.sH, r, w.y0, w.x0, p.H, p.W, [&](unsigned at) { return gx[at]; }, Vx);
    box_sum(w.sP, w.sH, r, w.y0, w.x0, p.H, p.W, [&](unsigned at) { return sy[at]; }, Sy);
    box_sum(w.sP, w.sH, r, w.y0, w.x0, p.H, p.W, [&](unsigned at) { return gy[at]; }, Vy);
    float *unc = p.unc + frame * 2;
#pragma unroll
    for (int g = 0; g < UQ_G; ++g) {
        const int y = w.y0 + w.yl + g;
        if (y >= p.H || x >= p.W) continue;
        const unsigned at = (unsigned)y * (unsigned)p.W + (unsigned)x;
        const int n = (int)N[g], n0 = n & 1023, nx = (n >> 10) & 1023, ny = n >> 20;
        const bool few = n0 < p.min_count || nx < p.min_count || ny < p.min_count;
        unsigned flag = few ? 1u : (C0[g] < p.floor2 * (double)n0 ? 2u : 0u);
        float ux = __builtin_nanf(""), uy = __builtin_nanf("");
        if (flag == 0) {
            double xm, xp, ym, yp;
            flag = unc_axis(C0[g], Sx[g], Vx[g], xm, xp) | unc_axis(C0[g], Sy[g], Vy[g], ym, yp);
            if (flag == 0) {
                const double l0 = log(C0[g]);
                double lm = log(xm), lp = log(xp);
                ux = (float)fabs(0.5 * (lm - lp) / ((lm - 2.0 * l0) + lp));
                lm = log(ym), lp = log(yp);
                uy = (float)fabs(0.5 * (lm - lp) / ((lm - 2.0 * l0) + lp));
            }
        }
        if (!(f[at] & 1)) flag |= 16u;
        unc[at] = ux;
        unc[w.HW + at] = uy;
        p.flag[frame + at] = (unsigned char)flag;
    }
}

// one thread per pixel, the pairs in batch order
__global__ __launch_bounds__(256) void unc_accumulate_kernel(const float *__restrict__ unc, const unsigned char *__restrict__ flag,
                                                             double *__restrict__ sums, int B, unsigned HW)
{
#pragma clang fp contract(off)
    const unsigned pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    double sxx = sums[pix], syy = sums[(size_t)HW + pix], n = sums[2 * (size_t)HW + pix];
    for (int b = 0; b < B; ++b) {
        const size_t frame = (size_t)b * HW;
        if (flag[frame + pix] & 15) continue;
        const double ux = (double)unc[frame * 2 + pix], uy = (double)unc[frame * 2 + HW + pix];
        sxx = sxx + ux * ux;
        syy = syy + uy * uy;
        n = n + 1.0;
    }
    sums[pix] = sxx;
    sums[(size_t)HW + pix] = syy;
    sums[2 * (size_t)HW + pix] = n;
}

static size_t unc_lds_bytes(int r)
{
    const size_t side = (size_t)(UQ_T + 2 * r);
    return (side * side + side * UQ_T) * 8;
}

size_t flow_uncertainty_workspace_bytes(int B, int H, int W, int radius, int lag)
{
    if (B <= 0 || H <= 0 || W <= 0 || radius < 1 || radius > 15 || lag < 0 || lag > 4) return 0;
    const size_t bytes = (size_t)B * (size_t)H * (size_t)W * 74;          // nine fp64 planes and two bytes per pixel
    return (bytes + 255) / 256 * 256;
}

int launch_flow_uncertainty(const float *img1, const float *img2, int C, const float *flow, const unsigned char *mask, float *unc,
                            unsigned char *flag, int B, int H, int W, int radius, int lag, int min_count, double floor, void *ws,
                            size_t ws_bytes, hipStream_t st)
{
    PIV_REQUIRE(img1 && img2 && flow && unc && flag && ws,
                "flow_uncertainty: null pointer (img1, img2, flow, unc, flag and the workspace are required)");
    PIV_REQUIRE(C == 1 || C == 3, "flow_uncertainty: C=%d channels, must be 1 or 3", C);
    if (int rc = check_shape("flow_uncertainty", B, H, W, "pairs")) return rc;
    PIV_REQUIRE(radius >= 1 && radius <= 15, "flow_uncertainty: radius=%d must be 1..15", radius);
    PIV_REQUIRE(lag >= 0 && lag <= 4, "flow_uncertainty: lag=%d must be 0..4", lag);
    const int win = (2 * radius + 1) * (2 * radius + 1);
    PIV_REQUIRE(min_count >= 2 && min_count <= win, "flow_uncertainty: min_count=%d must be 2..%d, the pixels of the window", min_count,
                win);
    PIV_REQUIRE(std::isfinite(floor) && floor >= 0.0, "flow_uncertainty: floor=%g must be finite and not negative", floor);
    const size_t px = (size_t)B * H * W, need = flow_uncertainty_workspace_bytes(B, H, W, radius, lag);
    if (int rc = check_workspace("flow_uncertainty", ws, ws_bytes, need, "B=%d H=%d W=%d", B, H, W)) return rc;
    const Span uq = {unc, px * 8, "unc"}, flg = {flag, px, "flag"};
    if (int rc = check_alias_by_input("flow_uncertainty", {uq, flg},
                                      {{img1, px * C * 4, "img1"}, {img2, px * C * 4, "img2"}, {flow, px * 8, "flow"}, {mask, px, "mask"},
                                       {ws, need, "the workspace"}},
                                      " (outputs must not alias an input)"))
        return rc;
    if (int rc = check_apart("flow_uncertainty", uq, flg)) return rc;

    // wa and wb hold a and b until the high-pass has read them, then g_x and g_y
    double *wa = (double *)ws, *wb = wa + px, *ha = wb + px, *hb = ha + px, *pp = hb + px, *sx = pp + px, *sy = sx + px, *dx = sy + px,
           *dy = dx + px;
    unsigned char *wf = (unsigned char *)(dy + px), *code = wf + px;
    if (int rc = launch_quality_warp(img1, img2, C, flow, mask, wa, wb, wf, B, H, W, st)) return rc;

    const int tiles_x = cdiv(W, UQ_T);
    const dim3 tgrid((unsigned)((size_t)tiles_x * (size_t)cdiv(H, UQ_T)), (unsigned)B);              // < 2^31 / 1024 tiles
    UncParams p = {wa, wb, nullptr, nullptr, nullptr, wf, ha, hb, unc, flag, H, W, radius, min_count, tiles_x, floor * floor};
    hipLaunchKernelGGL(unc_highpass_kernel, tgrid, dim3(UQ_THREADS), unc_lds_bytes(radius), st, p);
    PIV_CHECK_HIP(hipGetLastError());

    hipLaunchKernelGGL(unc_fields_kernel, dim3(frame_grid((size_t)H * W, B), (unsigned)B), dim3(256), 0, st, ha, hb, wf, pp, sx, sy, dx, dy,
                       code, H, W);
    PIV_CHECK_HIP(hipGetLastError());

    p.a = dx, p.b = dy, p.f = code, p.o0 = wa, p.o1 = wb, p.r = lag;
    hipLaunchKernelGGL(unc_lagbox_kernel, tgrid, dim3(UQ_THREADS), unc_lds_bytes(lag), st, p);
    PIV_CHECK_HIP(hipGetLastError());

    p.a = pp, p.b = sx, p.c = wa, p.d = sy, p.e = wb, p.o0 = p.o1 = nullptr, p.r = radius;
    hipLaunchKernelGGL(unc_window_kernel, tgrid, dim3(UQ_THREADS), unc_lds_bytes(radius), st, p);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

int launch_uncertainty_accumulate(const float *unc, const unsigned char *flag, double *sums, int B, int H, int W, hipStream_t st)
{
    PIV_REQUIRE(unc && flag && sums, "uncertainty_accumulate: null pointer (unc, flag and sums are required)");
    if (int rc = check_shape("uncertainty_accumulate", B, H, W, "frames", false)) return rc;
    PIV_REQUIRE(((size_t)sums & 7) == 0, "uncertainty_accumulate: sums must be 8-byte aligned");
    const size_t px = (size_t)B * H * W, hw = (size_t)H * W;
    PIV_REQUIRE(!ranges_overlap(sums, hw * 24, unc, px * 8) && !ranges_overlap(sums, hw * 24, flag, px),
                "uncertainty_accumulate: sums overlaps an input");
    hipLaunchKernelGGL(unc_accumulate_kernel, dim3((unsigned)((hw + 255) / 256)), dim3(256), 0, st, unc, flag, sums, B, (unsigned)hw);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
