// torch's bilinear interpolation (align_corners=False) as device code shared by every kernel that must reproduce
// estimate()'s output resize bit for bit: resize_nchw_kernel / resize_nhwc4_kernel (ops.hip) and the stereo kernel (stereo.hip).
// The roundings are spelled out: which products the compiler fuses into an fma under the default contraction depends on how
// the SLP vectoriser packs the surrounding kernel, so leaving it to the compiler would let the two kernels differ in the last
// bit.  The fmas below are the ones hipcc chose for resize_nchw_kernel before this header existed (its ISA is unchanged).
#pragma once
#include <hip/hip_runtime.h>

namespace pivlfn {

// ---- per-axis source index / weights of torch's bilinear, align_corners=False -----------------------------
struct Lin { int i0, i1; float w0, w1; };
__device__ __forceinline__ Lin lin_src(int d, float scale, int n)
{
#pragma clang fp contract(off)
    float src = __builtin_fmaf(scale, (float)d + 0.5f, -0.5f);
    src = src < 0.f ? 0.f : src;
    Lin l;
    l.i0 = (int)src;
    if (l.i0 > n - 1) l.i0 = n - 1;
    l.i1 = l.i0 + (l.i0 < n - 1 ? 1 : 0);
    l.w1 = src - (float)l.i0;
    l.w0 = 1.f - l.w1;
    return l;
}

// one plane of W columns: the value at the output position whose per-axis sources are ly, lx
__device__ __forceinline__ float bilinear_at(const float *__restrict__ base, int W, const Lin &ly, const Lin &lx)
{
#pragma clang fp contract(off)
    const float a = base[(size_t)ly.i0 * W + lx.i0], b = base[(size_t)ly.i0 * W + lx.i1];
    const float c = base[(size_t)ly.i1 * W + lx.i0], d = base[(size_t)ly.i1 * W + lx.i1];
    const float top = __builtin_fmaf(lx.w1, b, lx.w0 * a);
    const float bottom = __builtin_fmaf(lx.w0, c, lx.w1 * d);
    return ly.w0 * top + ly.w1 * bottom;
}

}  // namespace pivlfn
