// Match quality of an estimated flow (gfx950): the normalised correlation between image 1 and image 2 warped back by the flow inside a
// (2r+1)^2 interrogation window around every pixel, at zero shift and at the four one-pixel shifts, and the sub-pixel position of its
// peak by a three-point Gaussian fit -- the peak height every classical PIV code reports beside a vector, and what a window-deformation
// pass would still add to it.  Arithmetic contract: include/pivlfn.h.
//
// Two kernels through the workspace.  quality_warp_kernel, one thread per pixel: the gray value a of image 1, the warped gray value b of
// image 2 (both fp64) and a byte (bit 0: the sample lies inside image 2, bit 1: the pixel is not masked).  quality_window_kernel, one
// workgroup per TY x 32 tile: a, b and the bytes of the tile plus a halo of r + 1 go to LDS once; then, per shift, the six window sums
// in the contract's order.  A term outside the image or of a pixel that takes no part is +0.0, and a sum that starts at +0.0 never
// becomes -0.0, so x + 0.0 == x bit for bit: the clipped window is a full window over zero padding, and "rows left to right, then the
// row sums top to bottom" is a horizontal pass (row sums of TY + 2r rows, kept in LDS) followed by a vertical one.  The fixed order
// rules out running sums, not register tiling: a lane keeps 4 neighbouring outputs of the horizontal pass (TY / 8 of the vertical
// one) and adds every term it reads to those whose window holds it, the others get + 0.0 -- 4 + 2r LDS reads and products for 4
// outputs instead of 4 (2r + 1).  The same lane owns the same outputs in all five shifts and keeps their correlations in registers.
#include <cmath>
#include "launch_checks.h"

namespace pivlfn {

constexpr int QL_TX = 32;             // tile width; the tile height TY is 16 or 32
constexpr int QL_THREADS = 256;
constexpr int QL_G = 4;               // neighbouring outputs per lane in the horizontal pass

struct QualParams {
    const double *a, *b;              // [B,H,W] gray value of image 1, warped gray value of image 2
    const unsigned char *f;           // [B,H,W] bit 0: m, bit 1: k
    float *quality;                   // [B,3,H,W]
    unsigned char *flag;              // [B,H,W]
    int H, W, r, min_count, tiles_x;
    double floor2;                    // floor * floor
};

template <int C>
__device__ __forceinline__ double gray_at(const float *__restrict__ img, unsigned HW, unsigned at)
{
#pragma clang fp contract(off)
    if (C == 1) return (double)img[at];
    return (((double)img[at] + (double)img[HW + at]) + (double)img[2 * (size_t)HW + at]) / 3.0;
}

// blockIdx.y = pair; 32-bit pixel index within a frame (the host checks H*W < 2^31)
template <int C>
__global__ __launch_bounds__(256) void quality_warp_kernel(const float *__restrict__ img1, const float *__restrict__ img2,
                                                           const float *__restrict__ flow, const unsigned char *__restrict__ mask,
                                                           double *__restrict__ wa, double *__restrict__ wb,
                                                           unsigned char *__restrict__ wf, int H, int W)
{
#pragma clang fp contract(off)
    const unsigned HW = (unsigned)H * (unsigned)W;
    const size_t frame = (size_t)blockIdx.y * HW;
    const float *i1 = img1 + frame * C, *i2 = img2 + frame * C;
    const float *u = flow + frame * 2, *v = u + HW;
    for (unsigned pix = blockIdx.x * 256 + threadIdx.x; pix < HW; pix += gridDim.x * 256) {
        const int y = (int)(pix / (unsigned)W), x = (int)(pix - (unsigned)y * (unsigned)W);
        const float xf = (float)x + u[pix], yf = (float)y + v[pix];
        // NaN fails every comparison; W - 1 and H - 1 are exact in fp64
        const bool m = (double)xf >= 0.0 && (double)xf <= (double)(W - 1) && (double)yf >= 0.0 && (double)yf <= (double)(H - 1);
        double bv = 0.0;
        if (m) {
            const int x0 = (int)xf, y0 = (int)yf;
            const int x1 = x0 + 1 < W ? x0 + 1 : W - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1;
            const double fx = (double)xf - (double)x0, fy = (double)yf - (double)y0;
            const unsigned r0 = (unsigned)y0 * (unsigned)W, r1 = (unsigned)y1 * (unsigned)W;
            const double top = (1.0 - fx) * gray_at<C>(i2, HW, r0 + x0) + fx * gray_at<C>(i2, HW, r0 + x1);
            const double bot = (1.0 - fx) * gray_at<C>(i2, HW, r1 + x0) + fx * gray_at<C>(i2, HW, r1 + x1);
            bv = (1.0 - fy) * top + fy * bot;
        }
        const bool k = !mask || mask[frame + pix] == 0;
        wa[frame + pix] = gray_at<C>(i1, HW, pix);
        wb[frame + pix] = bv;
        wf[frame + pix] = (unsigned char)((m ? 1 : 0) | (k ? 2 : 0));
    }
}

struct QualLds {
    double *A, *B, *Hs;               // staged a, b [RH][RW]; row sums [5][NR][32]
    int *Hn;                          // row counts [NR][32]
    const unsigned char *F;           // staged bytes [RH][RW]
    int RW, NR;
};

// The six window sums of shift (SX, SY) for this lane's VG outputs, then c_s and its status (bit 0 few, bit 1 flat) per output.
// All threads of the workgroup call it; it starts with a barrier (the row sums of the shift before have been read).
template <int TY, int SX, int SY>
__device__ __forceinline__ void shift_pass(const QualLds &s, const QualParams &p, double (&c)[TY / 8], unsigned (&st)[TY / 8])
{
#pragma clang fp contract(off)
    constexpr int VG = TY / 8;
    const int r = p.r, t = threadIdx.x, plane = s.NR * QL_TX;
    const unsigned span = 2u * (unsigned)r;
    __syncthreads();
    // rows: row j of the row sums is staged row j + 1; output column x is staged column x + r + 1
    for (int item = t; item < s.NR * (QL_TX / QL_G); item += QL_THREADS) {
        const int j = item >> 3, gx = item & 7;
        const int atA = (j + 1) * s.RW + QL_G * gx + 1, atB = atA + SY * s.RW + SX;
        double acc[QL_G][5];
        int cnt[QL_G];
#pragma unroll
        for (int g = 0; g < QL_G; ++g) {
            cnt[g] = 0;
#pragma unroll
            for (int q = 0; q < 5; ++q) acc[g][q] = 0.0;
        }
        for (int i = 0; i < 2 * r + QL_G; ++i) {            // columns QL_G gx - r .. QL_G gx + QL_G - 1 + r, left to right
            const double a = s.A[atA + i], b = s.B[atB + i];
            const bool ok = (s.F[atA + i] & 2) != 0 && (s.F[atB + i] & 1) != 0;
            const double term[5] = {ok ? a : 0.0, ok ? a * a : 0.0, ok ? b : 0.0, ok ? b * b : 0.0, ok ? a * b : 0.0};
#pragma unroll
            for (int g = 0; g < QL_G; ++g) {
                const bool in = (unsigned)(i - g) <= span;
                cnt[g] += (in && ok) ? 1 : 0;
#pragma unroll
                for (int q = 0; q < 5; ++q) acc[g][q] = acc[g][q] + (in ? term[q] : 0.0);
            }
        }
#pragma unroll
        for (int g = 0; g < QL_G; ++g) {
            s.Hn[j * QL_TX + QL_G * gx + g] = cnt[g];
#pragma unroll
            for (int q = 0; q < 5; ++q) s.Hs[q * plane + j * QL_TX + QL_G * gx + g] = acc[g][q];
        }
    }
    __syncthreads();
    // columns: output row y adds the row sums y .. y + 2r, top to bottom
    const int x = t & 31, yg = t >> 5;
    double acc[VG][5];
    int cnt[VG];
#pragma unroll
    for (int g = 0; g < VG; ++g) {
        cnt[g] = 0;
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[g][q] = 0.0;
    }
    for (int i = 0; i < 2 * r + VG; ++i) {
        const int at = (VG * yg + i) * QL_TX + x;
        const int hn = s.Hn[at];
        double h[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) h[q] = s.Hs[q * plane + at];
#pragma unroll
        for (int g = 0; g < VG; ++g) {
            const bool in = (unsigned)(i - g) <= span;
            cnt[g] += in ? hn : 0;
#pragma unroll
            for (int q = 0; q < 5; ++q) acc[g][q] = acc[g][q] + (in ? h[q] : 0.0);
        }
    }
#pragma unroll
    for (int g = 0; g < VG; ++g) {
        const double n = (double)cnt[g], A = acc[g][0], AA = acc[g][1], Bs = acc[g][2], BB = acc[g][3], AB = acc[g][4];
        const bool few = cnt[g] < p.min_count;
        const double va = AA - A * A / n, vb = BB - Bs * Bs / n, cov = AB - A * Bs / n;
        const double lim = p.floor2 * n;
        const bool flat = va < lim || vb < lim;
        c[g] = cov / sqrt(va * vb);
        st[g] = few ? 1u : (flat ? 2u : 0u);
    }
}

// one axis of the fit: false when a condition of the contract fails
__device__ __forceinline__ bool fit_axis(double c0, double cm, double cp, double l0, double &d)
{
#pragma clang fp contract(off)
    d = 0.0;
    if (!(cm > 0.0 && cp > 0.0 && c0 >= cm && c0 >= cp && (2.0 * c0 - cm) - cp >= 1e-6)) return false;
    const double lm = log(cm), lp = log(cp);
    d = 0.5 * (lm - lp) / ((lm - 2.0 * l0) + lp);
    return true;
}

template <int TY>
__global__ __launch_bounds__(QL_THREADS) void quality_window_kernel(const QualParams p)
{
#pragma clang fp contract(off)
    constexpr int VG = TY / 8;
    extern __shared__ __align__(16) unsigned char smem[];
    const int r = p.r, t = threadIdx.x;
    const int RW = QL_TX + 2 * r + 2, RH = TY + 2 * r + 2, NR = TY + 2 * r;
    double *sA = reinterpret_cast<double *>(smem), *sB = sA + RH * RW, *sH = sB + RH * RW;
    int *sN = reinterpret_cast<int *>(sH + 5 * NR * QL_TX);
    unsigned char *sF = reinterpret_cast<unsigned char *>(sN + NR * QL_TX);
    const int ty = (int)blockIdx.x / p.tiles_x, tx = (int)blockIdx.x - ty * p.tiles_x;
    const unsigned HW = (unsigned)p.H * (unsigned)p.W;
    const size_t frame = (size_t)blockIdx.y * HW;
    const int y_org = ty * TY - r - 1, x_org = tx * QL_TX - r - 1;
    for (int i = t; i < RH * RW; i += QL_THREADS) {
        const int ly = i / RW, lx = i - ly * RW, gy = y_org + ly, gx = x_org + lx;
        const bool in = gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
        const size_t at = frame + (in ? (unsigned)gy * (unsigned)p.W + (unsigned)gx : 0u);      // outside: a valid address, dropped
        const double a = p.a[at], b = p.b[at];
        const unsigned char f = p.f[at];
        sA[i] = in ? a : 0.0;
        sB[i] = in ? b : 0.0;
        sF[i] = in ? f : (unsigned char)0;
    }
    const QualLds s = {sA, sB, sH, sN, sF, RW, NR};
    double c0[VG], cxm[VG], cxp[VG], cym[VG], cyp[VG];
    unsigned s0[VG], sxm[VG], sxp[VG], sym[VG], syp[VG];
    shift_pass<TY, 0, 0>(s, p, c0, s0);
    shift_pass<TY, -1, 0>(s, p, cxm, sxm);
    shift_pass<TY, 1, 0>(s, p, cxp, sxp);
    shift_pass<TY, 0, -1>(s, p, cym, sym);
    shift_pass<TY, 0, 1>(s, p, cyp, syp);

    const int xl = t & 31, yg = t >> 5, x = tx * QL_TX + xl;
    float *qual = p.quality + frame * 3;
#pragma unroll
    for (int g = 0; g < VG; ++g) {
        const int yl = VG * yg + g, y = ty * TY + yl;
        if (y >= p.H || x >= p.W) continue;
        unsigned flag = s0[g];                                              // FEW or FLAT of shift 0
        double dx = 0.0, dy = 0.0;
        if (flag == 0) {
            bool ok = (sxm[g] | sxp[g] | sym[g] | syp[g]) == 0 && c0[g] > 0.0;
            if (ok) {
                const double l0 = log(c0[g]);
                ok = fit_axis(c0[g], cxm[g], cxp[g], l0, dx);
                ok = fit_axis(c0[g], cym[g], cyp[g], l0, dy) && ok;
            }
            if (!ok) {
                flag = 4u;
                dx = dy = 0.0;
            }
        }
        if ((sF[(yl + r + 1) * RW + xl + r + 1] & 3) != 3) flag |= 8u;
        const unsigned at = (unsigned)y * (unsigned)p.W + (unsigned)x;
        qual[at] = (flag & 3u) ? __builtin_nanf("") : (float)c0[g];
        qual[HW + at] = (float)dx;
        qual[2 * (size_t)HW + at] = (float)dy;
        p.flag[frame + at] = (unsigned char)flag;
    }
}

static size_t quality_lds_bytes(int TY, int r)
{
    const size_t region = (size_t)(TY + 2 * r + 2) * (QL_TX + 2 * r + 2), rows = (size_t)(TY + 2 * r) * QL_TX;
    return (region * 16 + rows * 44 + region + 15) / 16 * 16;
}

size_t match_quality_workspace_bytes(int B, int H, int W, int radius)
{
    if (B <= 0 || H <= 0 || W <= 0 || radius < 1 || radius > 15) return 0;
    const size_t bytes = (size_t)B * (size_t)H * (size_t)W * 17;          // a, b (fp64) and one byte per pixel
    return (bytes + 255) / 256 * 256;
}

// The first kernel of match_quality, shared with flow_uncertainty (uncertainty.hip): a, b and the byte of m and k of every pixel.  The
// caller has checked the arguments (C is 1 or 3, 0 < B <= 65535, H*W < 2^31).
int launch_quality_warp(const float *img1, const float *img2, int C, const float *flow, const unsigned char *mask, double *wa, double *wb,
                        unsigned char *wf, int B, int H, int W, hipStream_t st)
{
    const dim3 wgrid(frame_grid((size_t)H * W, B), (unsigned)B);
    if (C == 1)
        hipLaunchKernelGGL(quality_warp_kernel<1>, wgrid, dim3(256), 0, st, img1, img2, flow, mask, wa, wb, wf, H, W);
    else
        hipLaunchKernelGGL(quality_warp_kernel<3>, wgrid, dim3(256), 0, st, img1, img2, flow, mask, wa, wb, wf, H, W);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

int launch_match_quality(const float *img1, const float *img2, int C, const float *flow, const unsigned char *mask, float *quality,
                         unsigned char *flag, int B, int H, int W, int radius, int min_count, double floor, void *ws, size_t ws_bytes,
                         hipStream_t st)
{
    PIV_REQUIRE(img1 && img2 && flow && quality && flag && ws,
                "match_quality: null pointer (img1, img2, flow, quality, flag and the workspace are required)");
    PIV_REQUIRE(C == 1 || C == 3, "match_quality: C=%d channels, must be 1 or 3", C);
    if (int rc = check_shape("match_quality", B, H, W, "pairs")) return rc;
    PIV_REQUIRE(radius >= 1 && radius <= 15, "match_quality: radius=%d must be 1..15", radius);
    const int win = (2 * radius + 1) * (2 * radius + 1);
    PIV_REQUIRE(min_count >= 2 && min_count <= win, "match_quality: min_count=%d must be 2..%d, the pixels of the window", min_count, win);
    PIV_REQUIRE(std::isfinite(floor) && floor >= 0.0, "match_quality: floor=%g must be finite and not negative", floor);
    const size_t px = (size_t)B * H * W, need = match_quality_workspace_bytes(B, H, W, radius);
    if (int rc = check_workspace("match_quality", ws, ws_bytes, need, "B=%d H=%d W=%d", B, H, W)) return rc;
    const Span qual = {quality, px * 12, "quality"}, flg = {flag, px, "flag"};
    if (int rc = check_alias_by_input("match_quality", {qual, flg},
                                      {{img1, px * C * 4, "img1"}, {img2, px * C * 4, "img2"}, {flow, px * 8, "flow"}, {mask, px, "mask"},
                                       {ws, need, "the workspace"}},
                                      " (outputs must not alias an input)"))
        return rc;
    if (int rc = check_apart("match_quality", qual, flg)) return rc;

    double *wa = (double *)ws, *wb = wa + px;
    unsigned char *wf = (unsigned char *)(wb + px);
    if (int rc = launch_quality_warp(img1, img2, C, flow, mask, wa, wb, wf, B, H, W, st)) return rc;

    // 16-row tiles keep two workgroups on a CU up to r = 8; above, 32 rows halve the share of halo rows in the horizontal pass
    const int TY = radius <= 8 ? 16 : 32;
    QualParams p = {wa, wb, wf, quality, flag, H, W, radius, min_count, cdiv(W, QL_TX), floor * floor};
    const size_t tiles = (size_t)p.tiles_x * (size_t)cdiv(H, TY);             // < 2^31 / 512
    const int lds = (int)quality_lds_bytes(TY, radius);
    static LdsAttr attr16, attr32;
    if (TY == 16) {
        if (int rc = ensure_dyn_lds(attr16, reinterpret_cast<const void *>(quality_window_kernel<16>), lds)) return rc;
        hipLaunchKernelGGL(quality_window_kernel<16>, dim3((unsigned)tiles, (unsigned)B), dim3(QL_THREADS), lds, st, p);
    } else {
        if (int rc = ensure_dyn_lds(attr32, reinterpret_cast<const void *>(quality_window_kernel<32>), lds)) return rc;
        hipLaunchKernelGGL(quality_window_kernel<32>, dim3((unsigned)tiles, (unsigned)B), dim3(QL_THREADS), lds, st, p);
    }
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
