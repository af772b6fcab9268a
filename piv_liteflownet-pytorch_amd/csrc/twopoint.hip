// Two-point statistics of a flow sequence (gfx950): per image row the sums of the fifteen pair terms of include/pivlfn.h at separations
// r*step along the row (d = 0) and down the column (d = 1), from which the correlation functions and the structure functions follow.
// Arithmetic contract: include/pivlfn.h.
//
// One kernel, no workspace, no barrier.  A workgroup is four independent waves that share a base row y and a direction d; wave w of
// workgroup z takes the separations r = 4z + w, 4z + w + 4 gridDim.z, ...  A wave walks the frames in order and, per frame and
// separation, the row in chunks of 256 columns: a lane owns four consecutive columns, forms the pair terms of each (a pair that does not
// take part has its four values replaced by +0.0, so every product and difference of it is +0.0 and none is formed from a NaN) and adds
// them as the two lowest levels of the contract's tree.  The tree goes on across the lanes -- partner lane ^ 1, ^ 2, ... ^ 32, the two
// operands of an addition commute, so both lanes hold the bits of the node -- in a folding form: at each of the first four steps a lane
// keeps one half of its terms and hands the other half to its partner, so 8 + 4 + 2 + 1 values cross instead of 4 x 15, and after them
// lane l holds ONE term, the one whose index is the four low bits of l reversed; two more steps on that one value finish the chunk.
// Chunks are combined by a binary counter (six registers: 64 chunks, W <= 16384), which is again the tree's order.  A level above the
// root (the tree has log2 P levels, P the power of two >= W) must not add its +0.0 padding -- (-0.0) + (+0.0) is +0.0 --, so below P = 256
// the surplus steps pass the value of the lower lane on instead of adding.  Lanes 0..15 then own one term each: they keep its running
// sum over the frames in LDS, one slot per separation of the wave, loaded from acc at the start and stored at the end -- acc is read
// and written once, and no lane touches another lane's slot, which is why no barrier is needed.
// The flow row, its partner and the mask are read straight from global memory: a frame and its mask stay in L2, and consecutive
// separations of a row re-read lines the wave has just touched.
#include <cmath>
#include "launch_checks.h"

namespace pivlfn {

constexpr int TP_TERMS = PIVLFN_TWOPOINT_TERMS;
constexpr int TP_WAVES = 4, TP_THREADS = 64 * TP_WAVES;
constexpr int TP_OWN = 4;                      // consecutive columns per lane: tree levels 0 and 1
constexpr int TP_CHUNK = 64 * TP_OWN;          // columns per wave and pass: tree levels 2..7 cross the lanes
constexpr int TP_SLOT = 16;                    // doubles per separation slot in LDS: the 15 terms and one unused

struct TwoPointParams {
    const float *flow;                         // [B,2,H,W]
    const unsigned char *mask;                 // [B,H,W] or nullptr
    const double *mean;                        // [2,H,W] or nullptr
    double *acc;                               // [2,R+1,15,H]
    int B, H, W, R, step;
    int levels;                                // log2 of the power of two >= W
    int chunks;                                // max(1, 2^levels / TP_CHUNK)
    int slots;                                 // separations per wave
};

// One step of the tree across lanes on 2N values: the lane whose bit `hi` is clear keeps in[0..N), the other in[N..2N); each adds what
// its partner sends of the same terms.  Where the level lies above the root (add = false) both take the lower lane's value.
template <int N>
__device__ __forceinline__ void tp_fold(const double *in, double *out, bool hi, int partner, bool add)
{
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const double keep = hi ? in[j + N] : in[j], send = hi ? in[j] : in[j + N];
        const double recv = __shfl_xor(send, partner);
        out[j] = add ? keep + recv : (hi ? recv : keep);
    }
}

// The root of the 256 columns from x0 on of base row `row` (a row offset y*W) against the row `prow` of the partner, dx columns to the
// right: in every lane, for the term the lane owns.  Called by whole waves.
__device__ __forceinline__ double tp_chunk(const TwoPointParams &p, const float *u, const float *v, const unsigned char *m, unsigned row,
                                           unsigned prow, int dx, int d, int x0, int lane)
{
#pragma clang fp contract(off)
    const unsigned HW = (unsigned)p.H * (unsigned)p.W;
    const int lv = p.levels;
    double Ua[TP_OWN], Va[TP_OWN], Ub[TP_OWN], Vb[TP_OWN], n[TP_OWN], dL[TP_OWN], dT[TP_OWN];
#pragma unroll
    for (int j = 0; j < TP_OWN; ++j) {
        const int x = x0 + lane * TP_OWN + j;
        const bool in = x + dx < p.W;                                          // the partner is inside the row, hence the base point too
        const unsigned ia = in ? row + (unsigned)x : 0u, ib = in ? prow + (unsigned)(x + dx) : 0u;     // outside: a valid address, dropped
        const double ua = (double)u[ia], va = (double)v[ia], ub = (double)u[ib], vb = (double)v[ib];
        // NaN fails every comparison
        const bool take = in && (!m || (m[ia] == 0 && m[ib] == 0)) && fabs(ua) <= 1e9 && fabs(va) <= 1e9 && fabs(ub) <= 1e9 && fabs(vb) <= 1e9;
        const double mua = p.mean ? p.mean[ia] : 0.0, mva = p.mean ? p.mean[HW + ia] : 0.0;
        const double mub = p.mean ? p.mean[ib] : 0.0, mvb = p.mean ? p.mean[HW + ib] : 0.0;
        Ua[j] = take ? ua - mua : 0.0;
        Va[j] = take ? va - mva : 0.0;
        Ub[j] = take ? ub - mub : 0.0;
        Vb[j] = take ? vb - mvb : 0.0;
        n[j] = take ? 1.0 : 0.0;
        const double du = Ub[j] - Ua[j], dv = Vb[j] - Va[j];
        dL[j] = d ? dv : du;
        dT[j] = d ? du : dv;
    }
    // levels 0 and 1 in registers
#define TP_TREE(e0, e1, e2, e3) (lv >= 2 ? ((e0) + (e1)) + ((e2) + (e3)) : lv == 1 ? (e0) + (e1) : (e0))
#define TP_SUM(f) TP_TREE(f(0), f(1), f(2), f(3))
    double t[16];
#define F(j) n[j]
    t[0] = TP_SUM(F);
#undef F
#define F(j) Ua[j]
    t[1] = TP_SUM(F);
#undef F
#define F(j) Va[j]
    t[2] = TP_SUM(F);
#undef F
#define F(j) Ub[j]
    t[3] = TP_SUM(F);
#undef F
#define F(j) Vb[j]
    t[4] = TP_SUM(F);
#undef F
#define F(j) (Ua[j] * Ua[j])
    t[5] = TP_SUM(F);
#undef F
#define F(j) (Va[j] * Va[j])
    t[6] = TP_SUM(F);
#undef F
#define F(j) (Ub[j] * Ub[j])
    t[7] = TP_SUM(F);
#undef F
#define F(j) (Vb[j] * Vb[j])
    t[8] = TP_SUM(F);
#undef F
#define F(j) (Ua[j] * Ub[j])
    t[9] = TP_SUM(F);
#undef F
#define F(j) (Va[j] * Vb[j])
    t[10] = TP_SUM(F);
#undef F
#define F(j) (Ua[j] * Vb[j])
    t[11] = TP_SUM(F);
#undef F
#define F(j) (Va[j] * Ub[j])
    t[12] = TP_SUM(F);
#undef F
#define F(j) ((dL[j] * dL[j]) * dL[j])
    t[13] = TP_SUM(F);
#undef F
#define F(j) ((dL[j] * dT[j]) * dT[j])
    t[14] = TP_SUM(F);
#undef F
#undef TP_SUM
#undef TP_TREE
    t[15] = 0.0;
    // levels 2..5 fold the sixteen values onto the lanes, levels 6 and 7 finish the one that is left
    double t8[8], t4[4], t2[2], t1[1];
    tp_fold<8>(t, t8, (lane & 1) != 0, 1, lv > 2);
    tp_fold<4>(t8, t4, (lane & 2) != 0, 2, lv > 3);
    tp_fold<2>(t4, t2, (lane & 4) != 0, 4, lv > 4);
    tp_fold<1>(t2, t1, (lane & 8) != 0, 8, lv > 5);
    double val = t1[0];
#pragma unroll
    for (int k = 6; k < 8; ++k) {
        const int partner = 1 << (k - 2);
        const double recv = __shfl_xor(val, partner);
        val = lv > k ? val + recv : ((lane & partner) ? recv : val);
    }
    return val;
}

// blockIdx.x = base row, blockIdx.y = direction, blockIdx.z and the wave pick the separations; 32-bit pixel index within a frame (the
// host checks H*W < 2^31)
__global__ __launch_bounds__(TP_THREADS) void twopoint_kernel(const TwoPointParams p)
{
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int y = (int)blockIdx.x, d = (int)blockIdx.y;
    const int r_first = (int)blockIdx.z * TP_WAVES + wave, r_stride = (int)gridDim.z * TP_WAVES;
    if (r_first > p.R) return;                                                 // the whole wave: nothing below waits for it
    // the term a lane is left with after tp_fold<8>, <4>, <2>, <1>: each step halves the index range by one bit of the lane
    const int term = ((lane & 1) << 3) | ((lane & 2) << 1) | ((lane & 4) >> 1) | ((lane & 8) >> 3);
    const bool owner = lane < 16 && term < TP_TERMS;
    double *mine = reinterpret_cast<double *>(smem) + ((size_t)wave * p.slots) * TP_SLOT + (lane & 15);      // a lane's own column of the slots
    double *out = p.acc + (((size_t)d * (p.R + 1)) * TP_TERMS + (owner ? term : 0)) * (size_t)p.H + y;
    const size_t r_pitch = (size_t)TP_TERMS * p.H;
    if (owner)
        for (int r = r_first, s = 0; r <= p.R; r += r_stride, ++s) mine[s * TP_SLOT] = out[r * r_pitch];

    const unsigned HW = (unsigned)p.H * (unsigned)p.W, row = (unsigned)y * (unsigned)p.W;
    for (int b = 0; b < p.B; ++b) {
        const float *u = p.flow + (size_t)b * 2 * HW, *v = u + HW;
        const unsigned char *m = p.mask ? p.mask + (size_t)b * HW : nullptr;
        for (int r = r_first, s = 0; r <= p.R; r += r_stride, ++s) {
            const int sep = r * p.step, dx = d ? 0 : sep, dy = d ? sep : 0;
            const bool row_in = y + dy < p.H;
            const unsigned prow = row_in ? (unsigned)(y + dy) * (unsigned)p.W : 0u;
            double up[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                     // the binary counter: up[k] waits for its right sibling at level 8 + k
            double root = 0.0;
            for (int c = 0; c < p.chunks; ++c) {
                const int x0 = c * TP_CHUNK;
                // a chunk without a pair is +0.0 in every term, whatever the tree does with zeros
                root = (row_in && x0 + dx < p.W) ? tp_chunk(p, u, v, m, row, prow, dx, d, x0, lane) : 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    if (!((c >> k) & 1)) {
                        up[k] = root;
                        break;
                    }
                    root = up[k] + root;
                }
            }
            if (owner) mine[s * TP_SLOT] = mine[s * TP_SLOT] + root;
        }
    }
    if (owner)
        for (int r = r_first, s = 0; r <= p.R; r += r_stride, ++s) out[r * r_pitch] = mine[s * TP_SLOT];
}

int launch_twopoint_accumulate(const float *flow, const unsigned char *mask, const double *mean, double *acc, int B, int H, int W,
                               int max_sep, int step, hipStream_t st)
{
    PIV_REQUIRE(H > 0 && W > 0, "twopoint_accumulate: bad shape H=%d W=%d (both must be positive)", H, W);
    PIV_REQUIRE(B >= 0, "twopoint_accumulate: B=%d frames, must not be negative", B);
    PIV_REQUIRE((size_t)H * W < ((size_t)1 << 31), "twopoint_accumulate: H*W=%zu pixels, must stay below 2^31 (32-bit pixel index)", (size_t)H * W);
    PIV_REQUIRE(W <= 16384, "twopoint_accumulate: W=%d columns, at most 16384 (64 chunks of a row)", W);
    PIV_REQUIRE(max_sep >= 0 && max_sep <= 255, "twopoint_accumulate: max_sep=%d must be 0..255", max_sep);
    PIV_REQUIRE(step >= 1 && step <= 16, "twopoint_accumulate: step=%d must be 1..16", step);
    if (B == 0) return PIVLFN_OK;                                              // nothing to add: no pointer is read
    PIV_REQUIRE(flow && acc, "twopoint_accumulate: null pointer (flow and acc are required)");
    const size_t px = (size_t)H * W, acc_bytes = (size_t)2 * (max_sep + 1) * TP_TERMS * H * sizeof(double);
    if (int rc = check_alias_by_input("twopoint_accumulate", {{acc, acc_bytes, "acc"}},
                                      {{flow, (size_t)B * px * 8, "flow"}, {mask, (size_t)B * px, "mask"}, {mean, px * 16, "mean"}},
                                      " (the sums must not alias an input)"))
        return rc;

    TwoPointParams p = {flow, mask, mean, acc, B, H, W, max_sep, step, 0, 1, 1};
    while ((1 << p.levels) < W) ++p.levels;
    p.chunks = (1 << p.levels) > TP_CHUNK ? (1 << p.levels) / TP_CHUNK : 1;
    // enough workgroups for every CU from the rows and the two directions alone where the image is tall; the separations fill in otherwise
    const int groups = cdiv(max_sep + 1, TP_WAVES), want = cdiv(4096, H);
    const int z = want < groups ? want : groups;
    p.slots = cdiv(max_sep + 1, TP_WAVES * z);
    const size_t lds = (size_t)TP_WAVES * p.slots * TP_SLOT * sizeof(double);   // <= 32 KiB
    hipLaunchKernelGGL(twopoint_kernel, dim3((unsigned)H, 2u, (unsigned)z), dim3(TP_THREADS), lds, st, p);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
