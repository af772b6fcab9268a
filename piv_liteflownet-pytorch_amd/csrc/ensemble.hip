// Ensemble correlation (gfx950): the window sums of sum-of-correlation PIV (Meinhart, Wereley & Santiago 2000), added over the frames of
// a call and onto what earlier calls left.  Per interrogation window of image a and per displacement (dy, dx) of the window of image b:
// sum B, sum B^2, sum A*B; per window: sum A, sum A^2.  Arithmetic contract: include/pivlfn.h.  Every sum is an exact integer, so the
// result depends neither on the tiling nor on how a sequence is cut into calls.
//
// One kernel, modelled on template_match_kernel (calibrate.hip).  A workgroup owns one window and a block of its displacements, and
// loops over the B frames itself.  Per frame it stages the window of a (window^2 bytes, between ENS_R - 1 zero rows above and below)
// and the search region of b ((window + 2 search) rows of `pitch` bytes) in LDS.  The images may start at any address: a staged dword
// is two aligned global dwords realigned by the row's own address & 3 (the second one only where it still holds a byte of the row).
// A lane owns ENS_R vertically adjacent displacements (dy0 .. dy0 + ENS_R - 1, dx) and walks the window + ENS_R - 1 region rows under
// them once: four taps at a time, dword (dx >> 2) + k of the row realigned by dx & 3 with v_alignbyte, then v_dot4_u32_u8 against
// the row of a each of its displacements pairs with that region row (a region row outside a displacement's window meets a zero row),
// and against itself and against ones once per row for all of them.  Lanes of one dy0 read the same dwords of a: a broadcast.  A
// per-frame sum fits 32 bits (255^2 * 128^2 < 2^32) and is widened to 64 bits before the frames are added.  sum A and sum A^2 are
// formed by the first block of a window only: every lane takes a share of the dwords of a, a wave adds its lanes up with shuffles
// and one lane per wave adds that to a 64-bit pair in LDS that lives through all frames.  Because every entry has exactly one owner,
// the add into global memory is a plain 64-bit load, add and store: no atomics, the stream orders successive calls.
// The kernel is instantiated for windows of 16, 32 and 64 pixels (NK = 4, 8, 16 dwords per row: the row loop unrolls and its LDS reads
// go out together) and once with a run-time row length for every other window.
#include "launch_checks.h"

namespace pivlfn {

constexpr int ENS_R = 4;                             // displacement rows per lane
constexpr int ENS_MIN_T = 128, ENS_MAX_T = 512;      // threads per workgroup: the (row group, dx) items of a block, in whole waves

struct EnsParams {
    const unsigned char *a, *b;                      // [B,H,W]
    const int *offset;                               // [2,ny,nx] or null
    long long *sums, *sums_a;                        // [ny,nx,P,P,3], [ny,nx,2]
    int B, H, W, window, step, search, nx, nwin, P, pitch, items;
};

__device__ __forceinline__ unsigned ens_dot4(unsigned a, unsigned b, unsigned c)
{
#if __has_builtin(__builtin_amdgcn_udot4)
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    return c + (a & 255u) * (b & 255u) + ((a >> 8) & 255u) * ((b >> 8) & 255u) + ((a >> 16) & 255u) * ((b >> 16) & 255u) + (a >> 24) * (b >> 24);
#endif
}

// dst[y * dst_pitch4 + d], d < ndw = ceil(nbytes / 4), gets bytes 4d .. 4d+3 of the row src + y * src_pitch, whatever its alignment; the
// bytes past nbytes in the last dword are whatever the aligned global dword holds beside the row's last byte (never used)
__device__ __forceinline__ void ens_stage(unsigned *dst, int dst_pitch4, const unsigned char *src, size_t src_pitch, int nrows, int ndw,
                                          int nbytes, int t, int T)
{
    constexpr int U = 4;                             // steps whose loads go out before the first is waited for
    const int n = nrows * ndw;
    for (int q0 = t; q0 < n; q0 += U * T) {
        unsigned lo[U], hi[U], sh[U];
        int at[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = q0 + u * T;
            const bool in = q < n;
            const int qq = in ? q : t;                                                  // past the end: a valid address, dropped
            const int y = qq / ndw, d = qq - y * ndw;
            const unsigned char *row = src + (size_t)y * src_pitch;
            sh[u] = (unsigned)(reinterpret_cast<size_t>(row) & 3u);
            const unsigned *g = reinterpret_cast<const unsigned *>(row - sh[u]);
            const int last = (int)(sh[u] + (unsigned)nbytes - 1u) >> 2;                 // the last aligned dword with a byte of the row
            lo[u] = g[d];
            hi[u] = g[d + 1 <= last ? d + 1 : last];                                    // d == last: no byte of it is needed
            at[u] = in ? y * dst_pitch4 + d : -1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (at[u] >= 0) dst[at[u]] = __builtin_amdgcn_alignbyte(hi[u], lo[u], sh[u]);
    }
}

// blockIdx.x = window, blockIdx.y = block of blockDim.x items; item = (group of ENS_R displacement rows) * P + dx
template <int NK>                                    // dwords per window row, 0: read from p
__global__ __launch_bounds__(ENS_MAX_T) void ensemble_corr_kernel(const EnsParams p)
{
    extern __shared__ __align__(16) unsigned ens_lds[];
    __shared__ unsigned long long tot_a[2];
    const int t = threadIdx.x, T = blockDim.x;
    const int w = NK ? 4 * NK : p.window, s = p.search, nk = w >> 2, pitch4 = p.pitch >> 2, rows = w + 2 * s;
    const int win = (int)blockIdx.x, j = win / p.nx, i = win - j * p.nx;
    const int ya = s + j * p.step, xa = s + i * p.step;
    const long long oy = p.offset ? p.offset[p.nwin + win] : 0, ox = p.offset ? p.offset[win] : 0;
    const long long yb = (long long)ya + oy - s, xb = (long long)xa + ox - s;          // the region's top-left pixel in b
    if (yb < 0 || yb + rows > p.H || xb < 0 || xb + rows > p.W) return;                 // OUTSIDE: the whole workgroup, nothing added
    const int a_dwords = (w + 2 * (ENS_R - 1)) * nk;                                    // a with its zero rows
    unsigned *sA = ens_lds, *sB = ens_lds + a_dwords;
    const int item = (int)blockIdx.y * T + t, P = p.P;
    const bool owner = item < p.items, first = blockIdx.y == 0;
    const int g = owner ? item / P : 0, dx = owner ? item - g * P : 0, dy0 = g * ENS_R;
    const unsigned sh = (unsigned)dx & 3u;
    const int walk = min(w + ENS_R - 1, rows - dy0);                                    // region rows under this lane's displacements
    const size_t HW = (size_t)p.H * p.W;
    const size_t at_a = (size_t)ya * p.W + xa, at_b = (size_t)yb * p.W + (size_t)xb;
    unsigned long long accB[ENS_R], accBB[ENS_R], accAB[ENS_R];
#pragma unroll
    for (int o = 0; o < ENS_R; ++o) accB[o] = accBB[o] = accAB[o] = 0;
    if (t < 2) tot_a[t] = 0;
    for (int q = t; q < (ENS_R - 1) * nk; q += T) sA[q] = sA[a_dwords - 1 - q] = 0u;    // the zero rows: written once
    for (int f = 0; f < p.B; ++f) {
        const unsigned char *ia = p.a + f * HW + at_a, *ib = p.b + f * HW + at_b;
        __syncthreads();                                                                // the frame before has been read
        ens_stage(sA + (ENS_R - 1) * nk, nk, ia, (size_t)p.W, w, nk, w, t, T);
        ens_stage(sB, pitch4, ib, (size_t)p.W, rows, (rows + 3) >> 2, rows, t, T);
        __syncthreads();
        if (first) {
            unsigned sa = 0, saa = 0;
            for (int q = t; q < a_dwords; q += T) {                                     // the zero rows add nothing
                const unsigned v = sA[q];
                sa = ens_dot4(v, 0x01010101u, sa);
                saa = ens_dot4(v, v, saa);
            }
            unsigned long long wa = sa, waa = saa;                                      // 64 lanes of up to 2^30 each: widened first
            for (int m = 32; m > 0; m >>= 1) {
                wa += __shfl_xor(wa, m);
                waa += __shfl_xor(waa, m);
            }
            if ((t & 63) == 0) {
                atomicAdd(&tot_a[0], wa);                                               // LDS, integers: any order gives the same bits
                atomicAdd(&tot_a[1], waa);
            }
        }
        if (owner) {
            unsigned fB[ENS_R], fBB[ENS_R], fAB[ENS_R];
#pragma unroll
            for (int o = 0; o < ENS_R; ++o) fB[o] = fBB[o] = fAB[o] = 0u;
            for (int ry = 0; ry < walk; ++ry) {                                         // region row dy0 + ry is row ry - o of displacement o
                const unsigned *brow = sB + (dy0 + ry) * pitch4 + (dx >> 2);
                const unsigned *arow = sA + (ry + ENS_R - 1) * nk;                      // displacement o reads the row o rows above
                unsigned lo = brow[0], rI = 0u, rII = 0u;
#pragma unroll
                for (int k = 0; k < nk; ++k) {
                    const unsigned hi = brow[k + 1];
                    const unsigned v = __builtin_amdgcn_alignbyte(hi, lo, sh);
                    lo = hi;
                    rI = ens_dot4(v, 0x01010101u, rI);
                    rII = ens_dot4(v, v, rII);
#pragma unroll
                    for (int o = 0; o < ENS_R; ++o) fAB[o] = ens_dot4(v, arow[k - o * nk], fAB[o]);
                }
#pragma unroll
                for (int o = 0; o < ENS_R; ++o)
                    if (ry >= o && ry - o < w) { fB[o] += rI; fBB[o] += rII; }
            }
#pragma unroll
            for (int o = 0; o < ENS_R; ++o) {
                accB[o] += fB[o];
                accBB[o] += fBB[o];
                accAB[o] += fAB[o];
            }
        }
    }
    if (owner) {
#pragma unroll
        for (int o = 0; o < ENS_R; ++o) {
            if (dy0 + o >= P) break;
            long long *out = p.sums + ((size_t)win * P * P + (size_t)(dy0 + o) * P + dx) * 3;
            out[0] += (long long)accB[o];
            out[1] += (long long)accBB[o];
            out[2] += (long long)accAB[o];
        }
    }
    if (first) {
        __syncthreads();
        if (t < 2) p.sums_a[(size_t)win * 2 + t] += (long long)tot_a[t];
    }
}

static inline int ens_pitch(int window, int search) { return (window + 2 * search + 3) / 4 * 4 + 4; }    // the last dword: read, never used

int launch_ensemble_corr(const unsigned char *a, const unsigned char *b, const int *offset, long long *sums, long long *sums_a, int B,
                         int H, int W, int window, int step, int search, hipStream_t st)
{
    PIV_REQUIRE(a && b && sums && sums_a, "ensemble_corr: null pointer (a, b, sums and sums_a are required)");
    PIV_REQUIRE(B >= 0 && B <= 65535, "ensemble_corr: B=%d frames, must be 0..65535 per call", B);
    PIV_REQUIRE(H > 0 && W > 0, "ensemble_corr: bad shape H=%d W=%d (both must be positive)", H, W);
    PIV_REQUIRE((size_t)H * W < ((size_t)1 << 31), "ensemble_corr: H*W=%zu pixels, must stay below 2^31 (32-bit pixel index)", (size_t)H * W);
    PIV_REQUIRE(window >= 8 && window <= 128 && window % 4 == 0, "ensemble_corr: window=%d must be a multiple of 4 in 8..128", window);
    PIV_REQUIRE(search >= 1 && search <= 32, "ensemble_corr: search=%d must be 1..32", search);
    PIV_REQUIRE(step >= 1, "ensemble_corr: step=%d must be at least 1", step);
    const int span = window + 2 * search;
    PIV_REQUIRE(H >= span && W >= span, "ensemble_corr: H=%d x W=%d holds no window of %d + 2*%d pixels", H, W, window, search);
    const int ny = (H - span) / step + 1, nx = (W - span) / step + 1, P = 2 * search + 1;
    const size_t nwin = (size_t)ny * nx, px = (size_t)B * H * W;
    const Span out = {sums, nwin * P * P * 24, "sums"}, out_a = {sums_a, nwin * 16, "sums_a"};
    if (int rc = check_alias_by_input("ensemble_corr", {out, out_a}, {{a, px, "a"}, {b, px, "b"}, {offset, nwin * 8, "offset"}},
                                      " (outputs must not alias an input)"))
        return rc;
    if (int rc = check_apart("ensemble_corr", out, out_a)) return rc;
    if (B == 0) return PIVLFN_OK;

    const int items = cdiv(P, ENS_R) * P;
    int T = (items + 63) / 64 * 64;
    T = T < ENS_MIN_T ? ENS_MIN_T : (T > ENS_MAX_T ? ENS_MAX_T : T);
    const EnsParams p = {a, b, offset, sums, sums_a, B, H, W, window, step, search, nx, (int)nwin, P, ens_pitch(window, search), items};
    // at most (128 + 6) * 128 + 192 * 196 = 54784 bytes
    const size_t lds = (size_t)(window + 2 * (ENS_R - 1)) * window + (size_t)span * p.pitch;
    const dim3 grid((unsigned)nwin, (unsigned)cdiv(items, T));
    if (window == 16)
        hipLaunchKernelGGL(ensemble_corr_kernel<4>, grid, dim3(T), lds, st, p);
    else if (window == 32)
        hipLaunchKernelGGL(ensemble_corr_kernel<8>, grid, dim3(T), lds, st, p);
    else if (window == 64)
        hipLaunchKernelGGL(ensemble_corr_kernel<16>, grid, dim3(T), lds, st, p);
    else
        hipLaunchKernelGGL(ensemble_corr_kernel<0>, grid, dim3(T), lds, st, p);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
