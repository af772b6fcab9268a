// Velocity distributions of a flow sequence (gfx950): the per-pixel sums up to the fourth order with the quadrant split of U*V
// (flow_moments_kernel) and the pooled histograms -- marginal, joint, and of the sub-pixel fraction of the raw displacement
// (flow_hist_kernel).  Arithmetic contract: include/pivlfn.h.
//
// flow_moments_kernel is flow_stats_masked_kernel's shape: a thread owns a pixel, holds its 21 sums in registers across the frames of a
// call and walks the frames in order, so acc is read and written once and a sequence gives the same bits however it is cut.  The grid is
// the frame-grid rule with frames = 1, capped at MO_MAX_BLOCKS: a thread carries three times the state of the masked statistics, and
// 4096 workgroups are already sixteen for every CU.
//
// flow_hist_kernel: few persistent workgroups (at most HI_GROUPS, two for a CU) sweep the B*H*W vectors with a grid-stride loop, HI_OWN
// vectors a thread and sweep, loaded before any of them is counted.  A workgroup counts into a private table of 32-bit counters in LDS
// with LDS integer atomics and adds the non-zero ones to `hist` with 64-bit global integer atomics at the end -- and after every
// HI_SWEEPS sweeps, see flush below.  The table is the layout of `hist` itself where all of it fits HI_LDS_WORDS (64 KiB: two workgroups
// and more share a CU's 160 KiB); otherwise the joint table (up to 256 x 256 counters = 256 KiB) is left out of it and updated in
// global memory directly, and the marginals, the fractions and the three single words, at most 10247 counters, stay in LDS.  The
// counted / left-out words are kept in a register per thread between flushes.  Counts are integers: no value depends on the geometry.
#include <cmath>
#include "launch_checks.h"

namespace pivlfn {

constexpr int MO_TERMS = PIVLFN_MOMENT_TERMS;
constexpr int MO_MAX_BLOCKS = 4096;
constexpr int HI_THREADS = 512, HI_OWN = 4;    // threads of a workgroup; vectors a thread loads per sweep
constexpr int HI_GROUPS = 512;                 // persistent workgroups at most
constexpr int HI_LDS_WORDS = 16384;            // the LDS budget of a workgroup's table in 32-bit counters
constexpr int HI_SWEEPS = 1 << 20;             // sweeps between two flushes
constexpr double DIST_MAX = 1e9, DIST_FINITE = 1.7976931348623157e308;

__global__ __launch_bounds__(256) void flow_moments_kernel(const float *__restrict__ flow, const unsigned char *__restrict__ mask,
                                                           const double *__restrict__ mean, const double *__restrict__ thr,
                                                           double *__restrict__ acc, int B, unsigned HW)
{
#pragma clang fp contract(off)
    for (unsigned pix = blockIdx.x * 256 + threadIdx.x; pix < HW; pix += gridDim.x * 256) {
        const double mu = mean ? mean[pix] : 0.0, mv = mean ? mean[(size_t)HW + pix] : 0.0;
        if (!(fabs(mu) <= DIST_FINITE && fabs(mv) <= DIST_FINITE)) continue;         // every frame of this pixel is left out
        const double hole = thr ? thr[pix] : 0.0;
        double s[MO_TERMS];
#pragma unroll
        for (int k = 0; k < MO_TERMS; ++k) s[k] = acc[(size_t)k * HW + pix];
        for (int b = 0; b < B; ++b) {
            const float *u = flow + (size_t)b * 2 * HW, *v = u + HW;
            const double du = (double)u[pix], dv = (double)v[pix];
            if ((mask && mask[(size_t)b * HW + pix] != 0) || !(fabs(du) <= DIST_MAX && fabs(dv) <= DIST_MAX)) continue;     // NaN fails
            const double U = mean ? du - mu : du, V = mean ? dv - mv : dv;
            const double uu = U * U, vv = V * V, P = U * V;
            s[0] = s[0] + 1.0;
            s[1] = s[1] + U;
            s[2] = s[2] + V;
            s[3] = s[3] + uu;
            s[4] = s[4] + vv;
            s[5] = s[5] + P;
            s[6] = s[6] + uu * U;
            s[7] = s[7] + vv * V;
            s[8] = s[8] + uu * V;
            s[9] = s[9] + vv * U;
            s[10] = s[10] + uu * uu;
            s[11] = s[11] + vv * vv;
            s[12] = s[12] + uu * vv;
            if (fabs(P) > hole) {                                                  // a NaN hole admits nothing
                if (U > 0.0 && V > 0.0) { s[13] = s[13] + 1.0; s[17] = s[17] + P; }
                if (U < 0.0 && V > 0.0) { s[14] = s[14] + 1.0; s[18] = s[18] + P; }
                if (U < 0.0 && V < 0.0) { s[15] = s[15] + 1.0; s[19] = s[19] + P; }
                if (U > 0.0 && V < 0.0) { s[16] = s[16] + 1.0; s[20] = s[20] + P; }
            }
        }
#pragma unroll
        for (int k = 0; k < MO_TERMS; ++k) acc[(size_t)k * HW + pix] = s[k];
    }
}

struct HistParams {
    const float *flow;                         // [B,2,H,W]
    const unsigned char *mask;                 // [B,H,W] or nullptr
    const double *mean, *scale;                // [2,H,W] or nullptr
    unsigned long long *hist;
    size_t total, rounds;                      // B*H*W vectors; sweeps of the whole grid
    unsigned HW, step_pix, step_frame;         // a thread's next vector lies gridDim.x * HI_THREADS further: that many frames and pixels
    double lo, s, sj;
    int nbins, jbins, fbins, joint_in_lds, lds_words;
};

// the slot of a marginal: 0 under, 1 + bin, nbins + 1 over (a NaN t too)
__device__ __forceinline__ int hist_slot(double x, double lo, double s, int nbins)
{
#pragma clang fp contract(off)
    const double t = (x - lo) * s;
    return t < 0.0 ? 0 : (t < (double)nbins ? 1 + (int)t : nbins + 1);
}

__device__ __forceinline__ int hist_fraction(double d, int fbins)
{
#pragma clang fp contract(off)
    const double f = d - floor(d);
    const int k = (int)(f * (double)fbins);
    return k < fbins - 1 ? k : fbins - 1;
}

__global__ __launch_bounds__(HI_THREADS) void flow_hist_kernel(const HistParams p)
{
#pragma clang fp contract(off)
    extern __shared__ unsigned tab[];
    const int nb2 = p.nbins + 2, j2 = p.jbins * p.jbins;
    const int off_v = nb2, off_j = 2 * nb2;                                        // word offsets in hist
    const int cut = p.joint_in_lds ? 0 : j2;                                       // a word behind the joint table lies `cut` lower in LDS
    const int at_out = off_j + j2 - cut, at_fu = at_out + 1, at_fv = at_fu + p.fbins, at_n = at_fv + p.fbins;       // LDS indices
    for (int i = threadIdx.x; i < p.lds_words; i += HI_THREADS) tab[i] = 0u;
    __syncthreads();

    const unsigned HW = p.HW;
    const unsigned first = blockIdx.x * HI_THREADS + threadIdx.x;                  // < HI_GROUPS * HI_THREADS
    const size_t lanes = (size_t)gridDim.x * HI_THREADS;
    size_t idx = first, frame = first / HW;
    unsigned pix = first % HW;
    unsigned n_in = 0u, n_out = 0u;
    for (size_t round = 0; round < p.rounds; ++round) {                            // the same count for every thread of the grid
        float u[HI_OWN], v[HI_OWN];
        unsigned char m[HI_OWN];
        unsigned px[HI_OWN];
        bool in[HI_OWN];
#pragma unroll
        for (int j = 0; j < HI_OWN; ++j) {
            in[j] = idx < p.total;
            const size_t a = in[j] ? frame * 2 * HW + pix : 0;                     // past the end: a valid address, dropped
            u[j] = p.flow[a];
            v[j] = p.flow[a + HW];
            m[j] = p.mask ? p.mask[in[j] ? frame * HW + pix : 0] : (unsigned char)0;
            px[j] = pix;
            idx += lanes;
            frame += p.step_frame;
            pix += p.step_pix;                                                     // both below HW < 2^31: no wrap
            if (pix >= HW) {
                pix -= HW;
                ++frame;
            }
        }
#pragma unroll
        for (int j = 0; j < HI_OWN; ++j) {
            if (!in[j]) continue;
            const double du = (double)u[j], dv = (double)v[j];
            bool take = m[j] == 0 && fabs(du) <= DIST_MAX && fabs(dv) <= DIST_MAX;   // NaN fails
            double X = du, Y = dv;
            if (take && p.mean) {
                const double mu = p.mean[px[j]], mv = p.mean[(size_t)HW + px[j]];
                take = fabs(mu) <= DIST_FINITE && fabs(mv) <= DIST_FINITE;
                X = du - mu;
                Y = dv - mv;
            }
            if (take && p.scale) {
                const double su = p.scale[px[j]], sv = p.scale[(size_t)HW + px[j]];
                take = su > 0.0 && sv > 0.0 && su <= DIST_FINITE && sv <= DIST_FINITE;
                X = X / su;
                Y = Y / sv;
            }
            if (!take) {
                ++n_out;
                continue;
            }
            ++n_in;
            atomicAdd(&tab[hist_slot(X, p.lo, p.s, p.nbins)], 1u);
            atomicAdd(&tab[off_v + hist_slot(Y, p.lo, p.s, p.nbins)], 1u);
            const double tu = (X - p.lo) * p.sj, tv = (Y - p.lo) * p.sj;
            if (tu >= 0.0 && tu < (double)p.jbins && tv >= 0.0 && tv < (double)p.jbins) {
                const int w = (int)tv * p.jbins + (int)tu;                          // < jbins * jbins
                if (p.joint_in_lds)
                    atomicAdd(&tab[off_j + w], 1u);
                else
                    atomicAdd(&p.hist[off_j + w], 1ull);
            } else {
                atomicAdd(&tab[at_out], 1u);
            }
            if (p.fbins > 0) {
                atomicAdd(&tab[at_fu + hist_fraction(du, p.fbins)], 1u);
                atomicAdd(&tab[at_fv + hist_fraction(dv, p.fbins)], 1u);
            }
        }
        // flush.  No 32-bit counter can wrap: between two flushes a thread counts at most HI_OWN * HI_SWEEPS = 2^22 vectors (n_in, n_out)
        // and a workgroup HI_THREADS * HI_OWN * HI_SWEEPS = 2^31, which bounds every word of its table.  The condition is the same for
        // every thread of the workgroup, so the barriers are met by all.
        if (((round + 1) & (size_t)(HI_SWEEPS - 1)) == 0 || round + 1 == p.rounds) {
            if (n_in) atomicAdd(&tab[at_n], n_in);
            if (n_out) atomicAdd(&tab[at_n + 1], n_out);
            n_in = n_out = 0u;
            __syncthreads();
            for (int i = threadIdx.x; i < p.lds_words; i += HI_THREADS) {
                const unsigned c = tab[i];
                if (c) {
                    tab[i] = 0u;
                    atomicAdd(&p.hist[i < off_j ? i : i + cut], (unsigned long long)c);
                }
            }
            __syncthreads();
        }
    }
}

// the frame-grid rule with frames = 1, capped
static inline unsigned moment_blocks(size_t px)
{
    const unsigned blocks = frame_grid(px, 1);
    return blocks < (unsigned)MO_MAX_BLOCKS ? blocks : (unsigned)MO_MAX_BLOCKS;
}

// The launch plan from the sizes alone; everything launch_flow_hist refuses apart from its pointers and the range is refused here.
int choose_flow_hist(int B, int H, int W, int nbins, int jbins, int fbins, HistPlan &pl)
{
    if (int rc = check_shape("flow_hist_accumulate", B == 0 ? 1 : B, H, W, "frames", false)) return rc;
    PIV_REQUIRE(nbins >= 1 && nbins <= 4096, "flow_hist_accumulate: nbins=%d must be 1..4096", nbins);
    PIV_REQUIRE(jbins >= 0 && jbins <= 256, "flow_hist_accumulate: jbins=%d must be 0..256 (0: no joint histogram)", jbins);
    PIV_REQUIRE(fbins >= 0 && fbins <= 1024, "flow_hist_accumulate: fbins=%d must be 0..1024 (0: no fraction histogram)", fbins);
    pl.words = PIVLFN_HIST_WORDS(nbins, jbins, fbins);
    pl.joint_in_lds = pl.words <= (size_t)HI_LDS_WORDS;
    pl.lds_words = (int)(pl.joint_in_lds ? pl.words : pl.words - (size_t)jbins * jbins);          // at most 10247 without the joint table
    const size_t total = (size_t)B * H * W, per = (size_t)HI_THREADS * HI_OWN, want = (total + per - 1) / per;
    pl.groups = (int)(want < (size_t)HI_GROUPS ? want : (size_t)HI_GROUPS);
    pl.moment_blocks = (int)moment_blocks((size_t)H * W);
    return PIVLFN_OK;
}

int launch_flow_moments(const float *flow, const unsigned char *mask, const double *mean, const double *thr, double *acc, int B, int H,
                        int W, hipStream_t st)
{
    if (int rc = check_shape("flow_moments_accumulate", B == 0 ? 1 : B, H, W, "frames", false)) return rc;
    if (B == 0) return PIVLFN_OK;                                              // nothing to add: no pointer is read
    PIV_REQUIRE(flow && acc, "flow_moments_accumulate: null pointer (flow and acc are required)");
    const size_t px = (size_t)H * W;
    if (int rc = check_alias_by_input("flow_moments_accumulate", {{acc, (size_t)MO_TERMS * px * sizeof(double), "acc"}},
                                      {{flow, (size_t)B * px * 8, "flow"}, {mask, (size_t)B * px, "mask"}, {mean, px * 16, "mean"},
                                       {thr, px * 8, "thr"}},
                                      " (the sums must not alias an input)"))
        return rc;
    hipLaunchKernelGGL(flow_moments_kernel, dim3(moment_blocks(px)), dim3(256), 0, st, flow, mask, mean, thr, acc, B, (unsigned)px);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

int launch_flow_hist(const float *flow, const unsigned char *mask, const double *mean, const double *scale, unsigned long long *hist,
                     int B, int H, int W, double lo, double hi, int nbins, int jbins, int fbins, hipStream_t st)
{
    HistPlan pl;
    if (int rc = choose_flow_hist(B, H, W, nbins, jbins, fbins, pl)) return rc;
    PIV_REQUIRE(std::isfinite(lo) && std::isfinite(hi) && hi > lo, "flow_hist_accumulate: range lo=%g hi=%g must be finite with hi > lo", lo, hi);
    if (B == 0) return PIVLFN_OK;                                              // nothing to count: no pointer is read
    PIV_REQUIRE(flow && hist, "flow_hist_accumulate: null pointer (flow and hist are required)");
    const size_t px = (size_t)H * W;
    if (int rc = check_alias_by_input("flow_hist_accumulate", {{hist, pl.words * sizeof(unsigned long long), "hist"}},
                                      {{flow, (size_t)B * px * 8, "flow"}, {mask, (size_t)B * px, "mask"}, {mean, px * 16, "mean"},
                                       {scale, px * 16, "scale"}},
                                      " (the counters must not alias an input)"))
        return rc;
    HistParams p;
    p.flow = flow; p.mask = mask; p.mean = mean; p.scale = scale; p.hist = hist;
    p.total = (size_t)B * px;
    const size_t lanes = (size_t)pl.groups * HI_THREADS;
    p.rounds = (p.total + lanes * HI_OWN - 1) / (lanes * HI_OWN);
    p.HW = (unsigned)px;
    p.step_pix = (unsigned)(lanes % px);
    p.step_frame = (unsigned)(lanes / px);
    p.lo = lo;
    p.s = (double)nbins / (hi - lo);
    p.sj = (double)jbins / (hi - lo);
    p.nbins = nbins; p.jbins = jbins; p.fbins = fbins; p.joint_in_lds = pl.joint_in_lds; p.lds_words = pl.lds_words;
    hipLaunchKernelGGL(flow_hist_kernel, dim3((unsigned)pl.groups), dim3(HI_THREADS), (size_t)pl.lds_words * sizeof(unsigned), st, p);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
