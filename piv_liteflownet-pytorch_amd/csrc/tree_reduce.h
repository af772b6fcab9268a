// The fixed-order sum T(.) over the nodes of a frame (include/pivlfn.h, "pressure"), for smooth.hip: a thread owns four consecutive
// leaves, six levels cross the lanes of a wave, two the four waves of a workgroup in LDS (a chunk of 1024 leaves), a binary counter combines
// a workgroup's chunks into one partial, and every workgroup of the next launch finishes the tree over a frame's at most 2048 partials by
// itself.  This is pressure.hip's tree, text for text; that file keeps its own copy because tests/analysis_plans.py pins its constants and
// formulas where they stand.  pressure.hip's head explains why padding with +0.0 changes no bit.  Keep the two alike.
#pragma once
#include "common.h"

namespace pivlfn {

constexpr int PR_THREADS = 256, PR_OWN = 4, PR_CHUNK = PR_THREADS * PR_OWN, PR_MAX_PART = 2048;

// ---- the tree ---------------------------------------------------------------------------------------------------------------------------
// v[k]: the sum of a thread's four leaves, as (l0 + l1) + (l2 + l3).  Afterwards every thread holds the root of the workgroup's 1024
// leaves.  Called by whole workgroups; sw is [K][4].
template <int K>
__device__ __forceinline__ void pr_chunk_root(double (&v)[K], double (*sw)[4])
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = v[k] + __shfl_xor(v[k], m);
    __syncthreads();                                                           // the last chunk's sums have been read
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) sw[k][wave] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (sw[k][0] + sw[k][1]) + (sw[k][2] + sw[k][3]);
}

// The binary counter over the chunks of a workgroup: up[k] waits for its right sibling at level k above a chunk's root.
// Written without a break so that every index is static and the counter stays in registers.
struct PrCounter {
    double up[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    __device__ __forceinline__ double add(double root, int c)
    {
#pragma clang fp contract(off)
        bool carry = true;                                                     // still climbing: every lower bit of c was set
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const bool bit = (c >> k) & 1;
            const double sum = up[k] + root;
            up[k] = (carry && !bit) ? root : up[k];
            root = (carry && bit) ? sum : root;
            carry = carry && bit;
        }
        return root;                                                           // after the last of 2^n chunks: their root
    }
};

// The roots of the trees over a frame's NB <= 2048 partials, K trees at once, in every thread: the partials are the leaves of one or two
// chunks, reduced like the nodes' (the padding above a root of fewer than 1024 partials adds +0.0, which changes no result -- see the
// head of the file).  sw is [K][4].
template <int K>
__device__ __forceinline__ void pr_finish(const double *const (&part)[K], int NB, double (*sw)[4], double (&out)[K])
{
#pragma clang fp contract(off)
    for (int c = 0; c * PR_CHUNK < NB; ++c) {
        const int base = c * PR_CHUNK + (int)threadIdx.x * PR_OWN;
        double v[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double l[PR_OWN];
#pragma unroll
            for (int j = 0; j < PR_OWN; ++j) l[j] = base + j < NB ? part[k][base + j] : 0.0;
            v[k] = (l[0] + l[1]) + (l[2] + l[3]);
        }
        pr_chunk_root<K>(v, sw);
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = c ? out[k] + v[k] : v[k];
    }
}

}  // namespace pivlfn
