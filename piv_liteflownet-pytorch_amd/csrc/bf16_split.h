// The exact three-piece bf16 split of an fp32 value, x = h + m + l with h = bf16(x), m = bf16(x - h), l = bf16(x - h - m) (round to
// nearest even; both differences are exact in fp32), shared by the kernels that multiply fp32 operands on the bf16 matrix cores
// (conv_wino_b3.hip, conv_dist_b3.hip): the device form for activations, the host form for weights packed at load time.
#pragma once
#include <cstring>
#include "common.h"
#include "wino_common.h"

namespace pivlfn {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

__device__ __forceinline__ unsigned cvt_pk_bf16(float a, float b)
{
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));      // v_cvt_pk_bf16_f32: round to nearest even
}

// x[0..7] -> three packed-bf16 operand fragments with x = h + m + l exactly
__device__ __forceinline__ void split8(const float *x, u32x4 &ph, u32x4 &pm, u32x4 &pl)
{
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const float x0 = x[2 * p], x1 = x[2 * p + 1];
        const unsigned h = cvt_pk_bf16(x0, x1);
        const float r0 = x0 - __builtin_bit_cast(float, h << 16), r1 = x1 - __builtin_bit_cast(float, h & 0xffff0000u);
        const unsigned m = cvt_pk_bf16(r0, r1);
        const float l0 = r0 - __builtin_bit_cast(float, m << 16), l1 = r1 - __builtin_bit_cast(float, m & 0xffff0000u);
        ph[p] = h;
        pm[p] = m;
        pl[p] = cvt_pk_bf16(l0, l1);
    }
}

// fp32 -> bf16 bits, round to nearest even (finite inputs)
static inline unsigned short bf16_rne(float f)
{
    unsigned u;
    memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
static inline float bf16_val(unsigned short h)
{
    const unsigned u = (unsigned)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// u = h + m + l exactly, on the host
static inline void bf16_split3(float u, unsigned short pc[3])
{
    pc[0] = bf16_rne(u);
    const float r1 = u - bf16_val(pc[0]);
    pc[1] = bf16_rne(r1);
    pc[2] = bf16_rne(r1 - bf16_val(pc[1]));
}

}  // namespace pivlfn
