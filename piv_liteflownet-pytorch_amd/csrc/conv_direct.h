// What the kernel families of the direct fp32 convolution share: conv_mfma.hip (v1, v2, the split-K reduce and the policy), conv_k1.hip,
// conv_c3k7.hip, conv_s2.hip.  A family file exports its choice alone; the choice's run pointer is what crosses the files.
#pragma once
#include <algorithm>
#include "common.h"

namespace pivlfn {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;

constexpr int PIXP = 12;
constexpr unsigned C2OOB = 0x80000000u;      // buffer-load offset beyond every descriptor: reads as zero

// A choice of this family (as ConvChoice, common.h): the launch function beside the plan; run wants p.ksplit = pl.ksplit (launch_conv)
struct ConvChoiceD {
    int (*run)(const ConvParams &, hipStream_t);
    ConvPlan pl;
};
// The dedicated kernels: whether the kernel applies to the layer, from the geometry alone, and then the choice
bool choose_conv_c3k7(const ConvParams &p, ConvChoiceD &ch);
bool choose_conv_k1(const ConvParams &p, bool any_tiles, ConvChoiceD &ch);
bool choose_conv_s2(const ConvParams &p, ConvChoiceD &ch);

// run() of a launcher L whose kernel takes dynamic LDS, at most `cap` bytes: the opt-in, once per launcher and device, and the launch
template <class L>
static inline int conv_run_d(void (*kernel)(const ConvParams), int cap, const ConvParams &p, hipStream_t st)
{
    static LdsAttr attr;
    if (int rc = ensure_dyn_lds(attr, reinterpret_cast<const void *>(kernel), cap)) return rc;
    hipLaunchKernelGGL(kernel, L::grid(p), dim3(256), L::lds_bytes(p), st, p);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
