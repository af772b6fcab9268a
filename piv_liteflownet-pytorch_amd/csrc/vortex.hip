// Vortex identification of a flow field (gfx950): the functions Gamma1 and Gamma2 of Graftieaux, Michard and Grosjean (2001) over the
// (2r+1)^2 neighbours at spacing s around every vector.  Gamma2 is formed about the window's own mean, so it tells a vortex core
// (|Gamma2| > 2/pi) from a shear layer, which vorticity cannot.  Arithmetic contract: include/pivlfn.h.
//
// Two kernels through the workspace.  vortex_stage_kernel, one thread per pixel: the unit vector (fp64, a square root and two
// divisions) and the validity byte.  vortex_window_kernel, one workgroup per phase (y mod s, x mod s) of the lattice and per 16 x 32
// tile of that phase: within a phase the neighbours at spacing s are adjacent, so the tile plus a halo of r is dense in LDS whatever
// s is -- U and V as the fp32 they came as ((double)u is exact), the unit vectors in fp64, the byte, and the quarter of the direction
// table the others follow from by sign, (r+1)^2 values b / sqrt(a^2 + b^2).  A vector outside the image or invalid is staged as +0.0
// with byte 0.  A sum that starts at +0.0 never becomes -0.0, so adding a term of +-0.0 changes no bit: the clipped window is a full
// window over zero padding, and the centre needs no test (its directions are +0.0).  A lane owns two vertically neighbouring outputs
// and walks the 2r + 2 staged rows they share once per pass: every LDS read feeds both windows, and per output the rows arrive in the
// contract's order -- a row sum from +0.0 left to right, then added to the total.  Pass 1: the counts, the sums of U and V and the
// Gamma1 sum.  Pass 2, which needs the mean of pass 1: the Gamma2 sum, one fp64 square root and one fp64 division per neighbour --
// that arithmetic, not LDS, is what the kernel's time goes to.
#include <cmath>
#include "launch_checks.h"

namespace pivlfn {

constexpr int VX_TX = 32, VX_TY = 16;     // tile of one phase
constexpr int VX_THREADS = 256;
constexpr int VX_G = 2;                   // vertically neighbouring outputs per lane: VX_TY = 8 * VX_G

struct VortParams {
    const float *flow;                    // [B,2,H,W]
    const double *ux, *uy;                // [B,H,W] unit vector (workspace)
    const unsigned char *k;               // [B,H,W] validity (workspace)
    float *gamma;                         // [B,2,H,W]
    unsigned char *flag;                  // [B,H,W]
    int H, W, r, s, min_count, tiles_x;
};

// blockIdx.y = pair; 32-bit pixel index within a frame (the host checks H*W < 2^31)
__global__ __launch_bounds__(256) void vortex_stage_kernel(const float *__restrict__ flow, const unsigned char *__restrict__ mask,
                                                           double *__restrict__ wx, double *__restrict__ wy,
                                                           unsigned char *__restrict__ wk, int H, int W)
{
#pragma clang fp contract(off)
    const unsigned HW = (unsigned)H * (unsigned)W;
    const size_t frame = (size_t)blockIdx.y * HW;
    const float *u = flow + frame * 2, *v = u + HW;
    for (unsigned pix = blockIdx.x * 256 + threadIdx.x; pix < HW; pix += gridDim.x * 256) {
        const double uu = (double)u[pix], vv = (double)v[pix];
        // NaN fails every comparison
        const bool k = (!mask || mask[frame + pix] == 0) && fabs(uu) <= 1e9 && fabs(vv) <= 1e9;
        const double U = k ? uu : 0.0, V = k ? vv : 0.0;
        const double m = sqrt(U * U + V * V);
        wx[frame + pix] = m > 0.0 ? U / m : 0.0;
        wy[frame + pix] = m > 0.0 ? V / m : 0.0;
        wk[frame + pix] = k ? 1 : 0;
    }
}

struct VortLds {
    const double *X, *Y, *T;              // staged unit vectors [RH][RW]; quarter table [r+1][r+1]: T[a][b] = b / sqrt(a*a + b*b)
    const float *U, *V;                   // staged vectors [RH][RW]
    const unsigned char *K;               // staged validity [RH][RW]
    int RW, r;
};

// (i, j) / sqrt(i*i + j*j): negating a quotient is exact, and 0 / d = +0.0 takes no sign
__device__ __forceinline__ void direction(const VortLds &s, int i, int j, double &px, double &py)
{
    const int ai = i < 0 ? -i : i, aj = j < 0 ? -j : j;
    const double tx = s.T[aj * (s.r + 1) + ai], ty = s.T[ai * (s.r + 1) + aj];
    px = i < 0 ? -tx : tx;
    py = j < 0 ? -ty : ty;
}

__global__ __launch_bounds__(VX_THREADS) void vortex_window_kernel(const VortParams p)
{
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char smem[];
    const int r = p.r, s = p.s, t = threadIdx.x;
    const int RW = VX_TX + 2 * r, RH = VX_TY + 2 * r, region = RH * RW, q = r + 1;
    double *sX = reinterpret_cast<double *>(smem), *sY = sX + region, *sT = sY + region;
    float *sU = reinterpret_cast<float *>(sT + q * q), *sV = sU + region;
    unsigned char *sK = reinterpret_cast<unsigned char *>(sV + region);

    const int py = (int)blockIdx.z / s, px = (int)blockIdx.z - py * s;        // the phase
    const int Hp = py < p.H ? (p.H - py + s - 1) / s : 0, Wp = px < p.W ? (p.W - px + s - 1) / s : 0;
    const int ty = (int)blockIdx.x / p.tiles_x, tx = (int)blockIdx.x - ty * p.tiles_x;
    if (ty * VX_TY >= Hp || tx * VX_TX >= Wp) return;                         // the tiles are laid out for phase (0, 0), the largest
    const unsigned HW = (unsigned)p.H * (unsigned)p.W;
    const size_t frame = (size_t)blockIdx.y * HW;
    const float *u = p.flow + frame * 2, *v = u + HW;

    const int y_org = ty * VX_TY - r, x_org = tx * VX_TX - r;                 // phase coordinates
    for (int i = t; i < region; i += VX_THREADS) {
        const int ly = i / RW, lx = i - ly * RW, Y = y_org + ly, X = x_org + lx;
        const bool in = Y >= 0 && Y < Hp && X >= 0 && X < Wp;
        const unsigned at = in ? (unsigned)(py + Y * s) * (unsigned)p.W + (unsigned)(px + X * s) : 0u;   // outside: a valid address, dropped
        const bool k = in && p.k[frame + at] != 0;
        const float fu = u[at], fv = v[at];
        const double x = p.ux[frame + at], y = p.uy[frame + at];
        sU[i] = k ? fu : 0.0f;
        sV[i] = k ? fv : 0.0f;
        sX[i] = k ? x : 0.0;
        sY[i] = k ? y : 0.0;
        sK[i] = k ? 1 : 0;
    }
    for (int i = t; i < q * q; i += VX_THREADS) {
        const int a = i / q, b = i - a * q;
        sT[i] = i == 0 ? 0.0 : (double)b / sqrt((double)(a * a + b * b));
    }
    __syncthreads();

    const VortLds lds = {sX, sY, sT, sU, sV, sK, RW, r};
    const int xl = t & 31, yg = t >> 5;
    const unsigned span = 2u * (unsigned)r;
    // pass 1: the counts, the sums of U and V (centre included) and the Gamma1 sum
    double g1[VX_G], su[VX_G], sv[VX_G];
    int cnt[VX_G];
#pragma unroll
    for (int g = 0; g < VX_G; ++g) {
        g1[g] = su[g] = sv[g] = 0.0;
        cnt[g] = 0;
    }
    for (int rr = 0; rr < 2 * r + VX_G; ++rr) {                               // staged rows VX_G yg + rr: row j = rr - g - r of output g
        const int base = (VX_G * yg + rr) * RW + xl;
        double a1[VX_G], au[VX_G], av[VX_G];
#pragma unroll
        for (int g = 0; g < VX_G; ++g) a1[g] = au[g] = av[g] = 0.0;
        for (int ii = 0; ii <= 2 * r; ++ii) {                                 // i = ii - r, left to right
            const double U = (double)lds.U[base + ii], V = (double)lds.V[base + ii], X = lds.X[base + ii], Y = lds.Y[base + ii];
            const int k = lds.K[base + ii];
#pragma unroll
            for (int g = 0; g < VX_G; ++g) {
                if ((unsigned)(rr - g) > span) continue;                      // uniform over the workgroup
                double dx, dy;
                direction(lds, ii - r, rr - g - r, dx, dy);
                a1[g] = a1[g] + (dx * Y - dy * X);
                au[g] = au[g] + U;
                av[g] = av[g] + V;
                cnt[g] += k;
            }
        }
#pragma unroll
        for (int g = 0; g < VX_G; ++g) {
            if ((unsigned)(rr - g) > span) continue;
            g1[g] = g1[g] + a1[g];
            su[g] = su[g] + au[g];
            sv[g] = sv[g] + av[g];
        }
    }
    // pass 2: the Gamma2 sum about the window mean
    double mu[VX_G], mv[VX_G], g2[VX_G];
#pragma unroll
    for (int g = 0; g < VX_G; ++g) {
        mu[g] = su[g] / (double)cnt[g];                                       // n_all = 0: NaN, no term below is taken, and FEW is set
        mv[g] = sv[g] / (double)cnt[g];
        g2[g] = 0.0;
    }
    for (int rr = 0; rr < 2 * r + VX_G; ++rr) {
        const int base = (VX_G * yg + rr) * RW + xl;
        double a2[VX_G];
#pragma unroll
        for (int g = 0; g < VX_G; ++g) a2[g] = 0.0;
        for (int ii = 0; ii <= 2 * r; ++ii) {
            const double U = (double)lds.U[base + ii], V = (double)lds.V[base + ii];
            const bool k = lds.K[base + ii] != 0;
#pragma unroll
            for (int g = 0; g < VX_G; ++g) {
                if ((unsigned)(rr - g) > span) continue;
                double dx, dy;
                direction(lds, ii - r, rr - g - r, dx, dy);
                const double du = U - mu[g], dv = V - mv[g];
                const double m2 = sqrt(du * du + dv * dv);
                const double term = (dx * dv - dy * du) / m2;
                a2[g] = a2[g] + ((k && m2 > 0.0) ? term : 0.0);
            }
        }
#pragma unroll
        for (int g = 0; g < VX_G; ++g) {
            if ((unsigned)(rr - g) > span) continue;
            g2[g] = g2[g] + a2[g];
        }
    }

    const int X = tx * VX_TX + xl;
    float *gam = p.gamma + frame * 2;
#pragma unroll
    for (int g = 0; g < VX_G; ++g) {
        const int yl = VX_G * yg + g, Y = ty * VX_TY + yl;
        if (Y >= Hp || X >= Wp) continue;
        const int kc = lds.K[(yl + r) * RW + xl + r];
        const int N = cnt[g] - kc;
        const bool few = N < p.min_count;
        const unsigned at = (unsigned)(py + Y * s) * (unsigned)p.W + (unsigned)(px + X * s);
        gam[at] = few ? __builtin_nanf("") : (float)(g1[g] / (double)N);
        gam[HW + at] = few ? __builtin_nanf("") : (float)(g2[g] / (double)N);
        p.flag[frame + at] = (unsigned char)((few ? 1 : 0) | (kc ? 0 : 2));
    }
}

static size_t vortex_lds_bytes(int r)
{
    const size_t region = (size_t)(VX_TY + 2 * r) * (VX_TX + 2 * r);
    return (region * 25 + (size_t)(r + 1) * (r + 1) * 8 + 15) / 16 * 16;
}

size_t vortex_gamma_workspace_bytes(int B, int H, int W, int radius, int spacing)
{
    if (B <= 0 || H <= 0 || W <= 0 || radius < 1 || radius > 15 || spacing < 1 || spacing > 16) return 0;
    const size_t bytes = (size_t)B * (size_t)H * (size_t)W * 17;          // the unit vector (2 x fp64) and one byte per pixel
    return (bytes + 255) / 256 * 256;
}

int launch_vortex_gamma(const float *flow, const unsigned char *mask, float *gamma, unsigned char *flag, int B, int H, int W, int radius,
                        int spacing, int min_count, void *ws, size_t ws_bytes, hipStream_t st)
{
    PIV_REQUIRE(flow && gamma && flag && ws, "vortex_gamma: null pointer (flow, gamma, flag and the workspace are required)");
    if (int rc = check_shape("vortex_gamma", B, H, W, "pairs")) return rc;
    PIV_REQUIRE(radius >= 1 && radius <= 15, "vortex_gamma: radius=%d must be 1..15", radius);
    PIV_REQUIRE(spacing >= 1 && spacing <= 16, "vortex_gamma: spacing=%d must be 1..16", spacing);
    const int nb = (2 * radius + 1) * (2 * radius + 1) - 1;
    PIV_REQUIRE(min_count >= 1 && min_count <= nb, "vortex_gamma: min_count=%d must be 1..%d, the neighbours of the window", min_count, nb);
    const size_t px = (size_t)B * H * W, need = vortex_gamma_workspace_bytes(B, H, W, radius, spacing);
    if (int rc = check_workspace("vortex_gamma", ws, ws_bytes, need, "B=%d H=%d W=%d", B, H, W)) return rc;
    const Span gam = {gamma, px * 8, "gamma"}, flg = {flag, px, "flag"};
    if (int rc = check_alias_by_input("vortex_gamma", {gam, flg}, {{flow, px * 8, "flow"}, {mask, px, "mask"}, {ws, need, "the workspace"}},
                                      " (outputs must not alias an input)"))
        return rc;
    if (int rc = check_apart("vortex_gamma", gam, flg)) return rc;

    double *wx = (double *)ws, *wy = wx + px;
    unsigned char *wk = (unsigned char *)(wy + px);
    hipLaunchKernelGGL(vortex_stage_kernel, dim3(frame_grid((size_t)H * W, B), (unsigned)B), dim3(256), 0, st, flow, mask, wx, wy, wk, H, W);
    PIV_CHECK_HIP(hipGetLastError());

    VortParams p = {flow, wx, wy, wk, gamma, flag, H, W, radius, spacing, min_count, cdiv(cdiv(W, spacing), VX_TX)};
    const size_t tiles = (size_t)p.tiles_x * (size_t)cdiv(cdiv(H, spacing), VX_TY);      // < 2^31 / 512 + 2^16
    const int lds = (int)vortex_lds_bytes(radius);
    static LdsAttr attr;
    if (int rc = ensure_dyn_lds(attr, reinterpret_cast<const void *>(vortex_window_kernel), lds)) return rc;
    hipLaunchKernelGGL(vortex_window_kernel, dim3((unsigned)tiles, (unsigned)B, (unsigned)(spacing * spacing)), dim3(VX_THREADS), lds, st, p);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
