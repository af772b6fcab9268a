// Vector validation of flow batches (gfx950): the normalized median test (Westerweel & Scarano, Exp. Fluids 39, 2005) with
// masking or median replacement of the vectors it rejects.  Reads a [B,2,H,W] NCHW flow -- what estimate(..., tensor=True)
// returns -- and works on the (2r+1)^2 - 1 neighbours of each pixel, r = 1 or 2, `spacing` pixels apart.  One thread per pixel.
// Arithmetic contract: include/pivlfn.h.
//
// Every median is taken from a compile-time sorting network over ALL N = 8 or 24 neighbour slots: a slot whose neighbour lies
// outside the image, is unknown or (pass 2) was flagged holds +inf, so the n valid values (all finite: unknown means |x| > 1e9)
// end up next to each other in order, and the middle one or two are picked by a chain of selects.  No register array is ever
// indexed with a runtime value.  A pixel with all N neighbours valid -- nearly every pixel, so whole waves -- takes the same network
// pruned at compile time to the compare-exchanges its two middle outputs depend on.
#include <cmath>
#include <utility>
#include "launch_checks.h"

namespace pivlfn {

#define PIV_HD __host__ __device__ __forceinline__

struct ValidateParams {
    int H, W, step;       // step = spacing
    float eps, thresh;
};

// Batcher's merge exchange (Knuth, TAOCP 3, 5.2.2 algorithm M) for N inputs, written out as a list of compare-exchange pairs.
template <int N>
struct SortNet {
    int n;
    unsigned char lo[N * 8], hi[N * 8];
};

template <int N>
constexpr SortNet<N> make_sort_net()
{
    SortNet<N> s{};
    int t = 0;
    while ((1 << t) < N) ++t;
    for (int p = 1 << (t - 1); p > 0; p >>= 1) {
        int q = 1 << (t - 1), r = 0, d = p;
        while (true) {
            for (int i = 0; i + d < N; ++i)
                if ((i & p) == r) {
                    s.lo[s.n] = (unsigned char)i;
                    s.hi[s.n] = (unsigned char)(i + d);
                    ++s.n;
                }
            if (q == p) break;
            d = q - p;
            q >>= 1;
            r = p;
        }
    }
    return s;
}

// The compare-exchanges of that network that lead to outputs N/2 - 1 and N/2 (the two a median of N values needs), found by
// walking the list backwards with the set of wires still wanted; the others are left out.
template <int N>
constexpr SortNet<N> make_median_net()
{
    const SortNet<N> full = make_sort_net<N>();
    bool want[N] = {}, keep[N * 8] = {};
    want[N / 2 - 1] = want[N / 2] = true;
    for (int k = full.n - 1; k >= 0; --k)
        if (want[full.lo[k]] || want[full.hi[k]]) keep[k] = want[full.lo[k]] = want[full.hi[k]] = true;
    SortNet<N> s{};
    for (int k = 0; k < full.n; ++k)
        if (keep[k]) {
            s.lo[s.n] = full.lo[k];
            s.hi[s.n] = full.hi[k];
            ++s.n;
        }
    return s;
}

template <int N>
struct FullNet {
    static constexpr SortNet<N> net = make_sort_net<N>();
};

template <int N>
struct MedianNet {
    static constexpr SortNet<N> net = make_median_net<N>();
};

// DESCENDING: the larger value goes to the lower wire.  The general path sorts that way so that its instructions differ from the
// pruned network's from the first one on: the compiler otherwise hoists the compare-exchanges the two have in common in front of
// the branch between them and then cannot drop, for the pruned side, what the other side still reads (seen in the ISA).
template <typename Net, bool DESCENDING, int N, size_t K>
PIV_HD void compare_exchange(float (&a)[N])
{
    constexpr int i = Net::net.lo[K], j = Net::net.hi[K];      // constant expressions: the array stays in registers
    const float x = a[i], y = a[j];
    a[i] = DESCENDING ? fmaxf(x, y) : fminf(x, y);
    a[j] = DESCENDING ? fminf(x, y) : fmaxf(x, y);
}

template <typename Net, bool DESCENDING, int N, size_t... K>
PIV_HD void run_network(float (&a)[N], std::index_sequence<K...>)
{
    (compare_exchange<Net, DESCENDING, N, K>(a), ...);
}

// Median of the n >= 1 finite values among a[0..N-1] (the other N - n slots hold +inf); a is left sorted descending, the +inf
// first: the k-th smallest value is a[N - 1 - k].
template <int N>
PIV_HD float median_of(float (&a)[N], int n)
{
#pragma clang fp contract(off)
    run_network<FullNet<N>, true, N>(a, std::make_index_sequence<FullNet<N>::net.n>{});
    const int k0 = N - 1 - ((n - 1) >> 1), k1 = N - 1 - (n >> 1);
    float lo = a[N - 1], hi = a[N - 1];
#pragma unroll
    for (int i = 0; i < N - 1; ++i) {
        lo = i == k0 ? a[i] : lo;
        hi = i == k1 ? a[i] : hi;
    }
    return (n & 1) ? lo : (lo + hi) * 0.5f;
}

// The same for n == N on the pruned network: a[N/2 - 1] and a[N/2] are right, the rest of a is not even a permutation of the
// input (where only one output of a compare-exchange is wanted the compiler drops the other).
template <int N>
PIV_HD float median_of_full(float (&a)[N])
{
#pragma clang fp contract(off)
    run_network<MedianNet<N>, false, N>(a, std::make_index_sequence<MedianNet<N>::net.n>{});
    return (a[N / 2 - 1] + a[N / 2]) * 0.5f;
}

PIV_HD bool unknown_flow(float u, float v)       // NaN fails both comparisons
{
    return !(fabsf(u) <= 1e9f) || !(fabsf(v) <= 1e9f);
}

// r_c of the contract for one component: the centre's distance to the neighbours' median over the median distance of the neighbours
template <int N>
PIV_HD float residual_of(float (&a)[N], int n, float centre, const ValidateParams &p)
{
#pragma clang fp contract(off)
    float m, r;
    if (n == N) {                                             // interior pixels, nearly all: whole waves take this side
        float d[N];
#pragma unroll
        for (int k = 0; k < N; ++k) d[k] = a[k];
        m = median_of_full<N>(d);
#pragma unroll
        for (int k = 0; k < N; ++k) d[k] = fabsf(a[k] - m);
        r = median_of_full<N>(d);
    } else {
        m = median_of<N>(a, n);
#pragma unroll
        for (int k = 0; k < N; ++k) a[k] = fabsf(a[k] - m);   // +inf stays +inf
        r = median_of<N>(a, n);
    }
    return fabsf(centre - m) / (r + p.eps);
}

// Pass 1 at one pixel: the flag byte (bit 0 outlier, bit 1 unknown) and the two residuals.
template <int R>
PIV_HD unsigned detect_at(const float *__restrict__ u, const float *__restrict__ v, unsigned pix, int y, int x,
                          const ValidateParams &p, float &ru, float &rv)
{
#pragma clang fp contract(off)
    constexpr int N = (2 * R + 1) * (2 * R + 1) - 1;
    const float inf = __builtin_inff();
    float au[N], av[N];
    int n = 0, k = 0;
#pragma unroll
    for (int i = -R; i <= R; ++i)
#pragma unroll
        for (int j = -R; j <= R; ++j) {
            if (i == 0 && j == 0) continue;
            // y < 2^31 and |i| * step < 2^16: the unsigned sum wraps for a negative coordinate only, and then exceeds any H
            const unsigned yy = (unsigned)y + (unsigned)(i * p.step), xx = (unsigned)x + (unsigned)(j * p.step);
            // loads that do not wait for each other: outside the image the pixel's own address stands in, and a select drops it
            const bool in = yy < (unsigned)p.H && xx < (unsigned)p.W;
            const unsigned q = in ? yy * (unsigned)p.W + xx : pix;
            const float lu = u[q] + 0.0f, lv = v[q] + 0.0f;
            const bool ok = in & !unknown_flow(lu, lv);
            au[k] = ok ? lu : inf;
            av[k] = ok ? lv : inf;
            n += ok;
            ++k;
        }
    const float cu = u[pix] + 0.0f, cv = v[pix] + 0.0f;
    ru = rv = 0.0f;
    if (unknown_flow(cu, cv)) return 2u;
    if (n == 0) return 0u;
    ru = residual_of<N>(au, n, cu, p);
    rv = residual_of<N>(av, n, cv, p);
    return (ru > p.thresh || rv > p.thresh) ? 1u : 0u;
}

// Pass 2 (REPLACE) at a pixel whose flag is non-zero: the medians of the neighbours pass 1 left unflagged.  False: there is none.
template <int R>
PIV_HD bool replace_at(const float *__restrict__ u, const float *__restrict__ v, const unsigned char *flag, unsigned pix, int y, int x,
                       const ValidateParams &p, float &ou, float &ov)
{
#pragma clang fp contract(off)
    constexpr int N = (2 * R + 1) * (2 * R + 1) - 1;
    const float inf = __builtin_inff();
    float au[N], av[N];
    int n = 0, k = 0;
#pragma unroll
    for (int i = -R; i <= R; ++i)
#pragma unroll
        for (int j = -R; j <= R; ++j) {
            if (i == 0 && j == 0) continue;
            const unsigned yy = (unsigned)y + (unsigned)(i * p.step), xx = (unsigned)x + (unsigned)(j * p.step);
            const bool in = yy < (unsigned)p.H && xx < (unsigned)p.W;
            const unsigned q = in ? yy * (unsigned)p.W + xx : pix;      // independent loads, as in pass 1
            const unsigned fq = flag[q];          // a neighbour's bit 2 may be set meanwhile: only where its flag was non-zero already
            const float lu = u[q], lv = v[q];
            const bool ok = in & (fq == 0);
            au[k] = ok ? lu + 0.0f : inf;
            av[k] = ok ? lv + 0.0f : inf;
            n += ok;
            ++k;
        }
    if (n == 0) return false;
    if (n == N) {
        ou = median_of_full<N>(au);
        ov = median_of_full<N>(av);
    } else {
        ou = median_of<N>(au, n);
        ov = median_of<N>(av, n);
    }
    return true;
}

// blockIdx.y = frame; 32-bit pixel index within a frame (the host checks H*W < 2^31).  masked != nullptr: MASK mode's output.
template <int R>
__global__ __launch_bounds__(256) void validate_detect_kernel(const float *__restrict__ flow, unsigned char *__restrict__ flag,
                                                              float *__restrict__ resid, float *__restrict__ masked,
                                                              const ValidateParams p)
{
    const unsigned HW = (unsigned)p.H * (unsigned)p.W;
    const float *u = flow + (size_t)blockIdx.y * 2 * HW, *v = u + HW;
    unsigned char *fl = flag + (size_t)blockIdx.y * HW;
    for (unsigned pix = blockIdx.x * 256 + threadIdx.x; pix < HW; pix += gridDim.x * 256) {
        const int y = (int)(pix / (unsigned)p.W), x = (int)(pix - (unsigned)y * (unsigned)p.W);
        float ru, rv;
        const unsigned f = detect_at<R>(u, v, pix, y, x, p, ru, rv);
        fl[pix] = (unsigned char)f;
        if (resid) {
            float *r = resid + (size_t)blockIdx.y * 2 * HW;
            r[pix] = ru;
            r[HW + pix] = rv;
        }
        if (masked) {
            float *o = masked + (size_t)blockIdx.y * 2 * HW;
            o[pix] = f ? 1e10f : u[pix];
            o[HW + pix] = f ? 1e10f : v[pix];
        }
    }
}

template <int R>
__global__ __launch_bounds__(256) void validate_replace_kernel(const float *__restrict__ flow, unsigned char *flag,
                                                               float *__restrict__ out, const ValidateParams p)
{
    const unsigned HW = (unsigned)p.H * (unsigned)p.W;
    const float *u = flow + (size_t)blockIdx.y * 2 * HW, *v = u + HW;
    unsigned char *fl = flag + (size_t)blockIdx.y * HW;
    float *o = out + (size_t)blockIdx.y * 2 * HW;
    for (unsigned pix = blockIdx.x * 256 + threadIdx.x; pix < HW; pix += gridDim.x * 256) {
        float ou = u[pix], ov = v[pix];
        const unsigned f = fl[pix];
        if (f != 0) {
            const int y = (int)(pix / (unsigned)p.W), x = (int)(pix - (unsigned)y * (unsigned)p.W);
            if (!replace_at<R>(u, v, fl, pix, y, x, p, ou, ov)) fl[pix] = (unsigned char)(f | 4u);      // a byte store of this pixel's own flag
        }
        o[pix] = ou;
        o[HW + pix] = ov;
    }
}

int launch_flow_validate(const float *flow, float *out, unsigned char *flag, float *resid, int B, int H, int W, int radius,
                         int spacing, float eps, float thresh, int mode, hipStream_t st)
{
    PIV_REQUIRE(flow && flag, "flow_validate: null pointer (flow and flag are required)");
    PIV_REQUIRE(mode == PIVLFN_VALIDATE_FLAG || mode == PIVLFN_VALIDATE_MASK || mode == PIVLFN_VALIDATE_REPLACE,
                "flow_validate: unknown mode=%d (PIVLFN_VALIDATE_FLAG 0, PIVLFN_VALIDATE_MASK 1 or PIVLFN_VALIDATE_REPLACE 2)", mode);
    PIV_REQUIRE(out || mode == PIVLFN_VALIDATE_FLAG, "flow_validate: null out (only PIVLFN_VALIDATE_FLAG has no flow output)");
    PIV_REQUIRE(out != flow, "flow_validate: out == flow (pass 2 reads the neighbours of what it writes; out must not overlap flow)");
    if (int rc = check_shape("flow_validate", B, H, W, "frames")) return rc;
    PIV_REQUIRE(radius == 1 || radius == 2, "flow_validate: radius=%d must be 1 or 2", radius);
    PIV_REQUIRE(spacing >= 1 && (long)radius * spacing < (1L << 15), "flow_validate: spacing=%d must be >= 1 and radius*spacing below 2^15",
                spacing);
    PIV_REQUIRE(std::isfinite(eps) && eps >= 0.0f, "flow_validate: eps=%g must be finite and not negative", (double)eps);
    PIV_REQUIRE(std::isfinite(thresh) && thresh > 0.0f, "flow_validate: thresh=%g must be finite and positive", (double)thresh);
    const ValidateParams p = {H, W, spacing, eps, thresh};
    const dim3 grid(frame_grid((size_t)H * W, B), (unsigned)B);
    float *masked = mode == PIVLFN_VALIDATE_MASK ? out : nullptr;
    if (radius == 1)
        hipLaunchKernelGGL(validate_detect_kernel<1>, grid, dim3(256), 0, st, flow, flag, resid, masked, p);
    else
        hipLaunchKernelGGL(validate_detect_kernel<2>, grid, dim3(256), 0, st, flow, flag, resid, masked, p);
    PIV_CHECK_HIP(hipGetLastError());
    if (mode == PIVLFN_VALIDATE_REPLACE) {
        if (radius == 1)
            hipLaunchKernelGGL(validate_replace_kernel<1>, grid, dim3(256), 0, st, flow, flag, out, p);
        else
            hipLaunchKernelGGL(validate_replace_kernel<2>, grid, dim3(256), 0, st, flow, flag, out, p);
        PIV_CHECK_HIP(hipGetLastError());
    }
    return PIVLFN_OK;
}

}  // namespace pivlfn
