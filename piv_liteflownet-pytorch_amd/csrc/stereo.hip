// Stereoscopic 2D3C reconstruction (gfx950): two cameras' planar flows -> one three-component field in the .flo band order.
// Reference: stereo_run.py:153-163 (_stereo_cal), stereo/dewarp.py:255-270 (nl_trans), stereo/vel3d.py:4-24 (willert).
// One thread per output pixel, fused with estimate()'s output resize (inference.py:57-61) so the raw network output of an
// interleaved [L0, R0, L1, R1, ...] batch goes straight to the payload.  Arithmetic contract: include/pivlfn.h.
#include <cmath>
#include "launch_checks.h"
#include "bilinear.h"

namespace pivlfn {

struct StereoParams {
    float A[2][24];              // rational-polynomial coefficients, left camera then right (already rounded to fp32)
    double tL, tR, bL, bR;       // tan(theta_L), tan(theta_R), tan(beta_L), tan(beta_R), evaluated on the host
    float calib, fps;            // m/s scaling of stage 1 when `scaled`
    float sy, sx, mx, my;        // resize: source / output per axis and estimate()'s multipliers (W/W', H/H')
    int scaled, resize;
    int B, h, w, H, W;
};

// Every operation below is rounded on its own, in the order numpy evaluates the reference's expressions: no fma contraction.
// (Stages 1 and 2 only: the bilinear samples are bilinear.h's, whose roundings are spelled out there.)
__device__ __forceinline__ float poly6(const float *A, float x, float y)
{
#pragma clang fp contract(off)
    return ((((A[0] * x + A[1] * y) + A[2]) + A[3] * (x * x)) + A[4] * (y * y)) + (A[5] * x) * y;
}

// stage 1 (nl_trans + the optional calib * fps of _stereo_cal), fp32
__device__ __forceinline__ void map_camera(const float *A, float u, float v, const StereoParams &p, float &x, float &y)
{
#pragma clang fp contract(off)
    x = poly6(A, u, v) / poly6(A + 6, u, v);
    y = poly6(A + 12, u, v) / poly6(A + 18, u, v);
    if (p.scaled) {
        x = (x * p.calib) * p.fps;
        y = (y * p.calib) * p.fps;
    }
}

// stage 2 (willert), float64 where numpy promotes to it, fp32 where it does not
__device__ __forceinline__ void willert(float uL, float vL, float uR, float vR, const StereoParams &p, float *o)
{
#pragma clang fp contract(off)
    const double dT = p.tL - p.tR, dB = p.bR - p.bL;
    const float du = uR - uL;
    const float vm = (vL + vR) / 2.0f;
    const double U = ((double)uR * p.tL - (double)uL * p.tR) / dT;
    const double V = (double)vm + (((double)du * dB) / dT) / 2.0;
    const double Wc = (double)du / dT;
    o[0] = (float)U;
    o[1] = (float)V;
    o[2] = (float)Wc;
}

// flow: [2B,2,h,w] NCHW (even entries left, odd right); out: [B,H,W,3].  blockIdx.y = step; 32-bit pixel index within a
// step (the host checks H*W and h*w < 2^31): no 64-bit division in the index math
__global__ __launch_bounds__(256) void stereo_2d3c_kernel(const float *__restrict__ flow, float *__restrict__ out,
                                                          const StereoParams p)
{
    const unsigned HW = (unsigned)p.H * (unsigned)p.W, hw = (unsigned)p.h * (unsigned)p.w;
    const float *L = flow + (size_t)blockIdx.y * 4 * hw, *R = L + 2 * (size_t)hw;
    float *o = out + (size_t)blockIdx.y * 3 * HW;
    for (unsigned pix = blockIdx.x * 256 + threadIdx.x; pix < HW; pix += gridDim.x * 256) {
        float uL, vL, uR, vR;
        if (p.resize) {                  // resize_nchw_kernel's sample, then its `v *= m`
            const int oy = (int)(pix / (unsigned)p.W), ox = (int)(pix - (unsigned)oy * (unsigned)p.W);
            const Lin ly = lin_src(oy, p.sy, p.h), lx = lin_src(ox, p.sx, p.w);
            uL = bilinear_at(L, p.w, ly, lx) * p.mx;
            vL = bilinear_at(L + hw, p.w, ly, lx) * p.my;
            uR = bilinear_at(R, p.w, ly, lx) * p.mx;
            vR = bilinear_at(R + hw, p.w, ly, lx) * p.my;
        } else {                         // estimate() skips an identity resize
            uL = L[pix];
            vL = L[hw + pix];
            uR = R[pix];
            vR = R[hw + pix];
        }
        float xL, yL, xR, yR;
        map_camera(p.A[0], uL, vL, p, xL, yL);
        map_camera(p.A[1], uR, vR, p, xR, yR);
        willert(xL, yL, xR, yR, p, o + 3 * (size_t)pix);     // three consecutive dwords per lane: one dwordx3 store, a wave's 768 B contiguous
    }
}

int launch_stereo_2d3c(const float *flow, float *out, int B, int h, int w, int H, int W, const float *mul,
                       const float *coeff, const float *scale, const double *tan4, hipStream_t st)
{
    PIV_REQUIRE(flow && out && coeff && tan4, "stereo_2d3c: null pointer (flow, out, coeff and tangents are required)");
    PIV_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "stereo_2d3c: bad shape B=%d h=%d w=%d H=%d W=%d", B, h, w, H, W);
    PIV_REQUIRE((size_t)H * W < ((size_t)1 << 31) && (size_t)h * w < ((size_t)1 << 31) && B <= 65535,
                "stereo_2d3c: too large (H*W and h*w must stay below 2^31, B at most 65535)");
    for (int k = 0; k < 4; ++k)
        PIV_REQUIRE(std::isfinite(tan4[k]), "stereo_2d3c: tangent %d is not finite", k);
    PIV_REQUIRE(tan4[0] - tan4[1] != 0.0, "stereo_2d3c: tan(theta_L) == tan(theta_R): the two views do not resolve w");
    StereoParams p;
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 24; ++k) p.A[c][k] = coeff[24 * c + k];
    p.tL = tan4[0];
    p.tR = tan4[1];
    p.bL = tan4[2];
    p.bR = tan4[3];
    p.scaled = scale ? 1 : 0;
    p.calib = scale ? scale[0] : 1.f;
    p.fps = scale ? scale[1] : 1.f;
    p.resize = (h != H || w != W) ? 1 : 0;
    p.sy = (float)h / (float)H;              // launch_resize_nchw's scales and multipliers, bit for bit
    p.sx = (float)w / (float)W;
    p.mx = mul ? mul[0] : 1.f;
    p.my = mul ? mul[1] : 1.f;
    p.B = B; p.h = h; p.w = w; p.H = H; p.W = W;
    hipLaunchKernelGGL(stereo_2d3c_kernel, dim3(frame_grid((size_t)H * W, B), (unsigned)B), dim3(256), 0, st, flow, out, p);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
