// Temporal spectra of a flow sequence (include/pivlfn.h "temporal spectra"): one segment of Welch's method.  For every vector p and
// every basis pair k the four projections cu, su, cv, sv of the segment's L samples of u and v on C_k and S_k, each a sequential fp64
// fold without fma, and their quadratic forms Suu, Svv, Co, Qd added to acc[k][0..3][p].
//
// A workgroup of 8 waves owns SP_TILE = 64 vectors, one per lane.  The segment's samples of the tile are staged in LDS in chunks of
// SP_TC = 128 samples (128 x 2 x 64 floats = 64 KB, two workgroups per CU), read from there once per wave and frequency group, and the
// 8 waves share the chunk: wave w folds the groups w, w + 8, ... of SP_KG = 8 frequencies (32 fp64 accumulators per lane), one per
// round, and in the last round one of the K % 8 frequencies left over beside its group.  The basis values are uniform across a wave and come through
// the scalar cache; a lane's LDS reads are 64 consecutive floats.  With L <= 128 the tile is staged once; a longer segment is staged
// again for every round of items (and once for the validity scan), which the L2 serves.  A lane whose vector holds one value that is
// NaN or beyond 1e9 in the segment writes nothing; a tile without a valid vector folds nothing.
#include "common.h"

#pragma clang fp contract(off)

namespace pivlfn {

constexpr int SP_TILE = 64;
constexpr int SP_WAVES = 8;
constexpr int SP_THREADS = SP_TILE * SP_WAVES;
constexpr int SP_TC = 128;
constexpr int SP_KG = 8;

// the fold of samples t0 .. t0+nt-1 (staged in `tile`) into the projections of KN consecutive frequencies from k0
template <int KN>
__device__ __forceinline__ void spectrum_fold(const float *tile, int lane, int nt, const double *__restrict__ b, int L,
                                              double (&cu)[SP_KG], double (&su)[SP_KG], double (&cv)[SP_KG], double (&sv)[SP_KG])
{
    int t = 0;
    for (; t + 4 <= nt; t += 4) {                          // four samples per pass: a basis row's four values are one scalar load
        double u[4], v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            u[j] = (double)tile[(2 * (t + j)) * SP_TILE + lane];
            v[j] = (double)tile[(2 * (t + j) + 1) * SP_TILE + lane];
        }
#pragma unroll
        for (int i = 0; i < KN; ++i) {
            const double *c = b + (size_t)(2 * i) * L + t, *s = c + L;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cu[i] = cu[i] + c[j] * u[j];
                cv[i] = cv[i] + c[j] * v[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                su[i] = su[i] + s[j] * u[j];
                sv[i] = sv[i] + s[j] * v[j];
            }
        }
    }
    for (; t < nt; ++t) {
        const double u = (double)tile[(2 * t) * SP_TILE + lane], v = (double)tile[(2 * t + 1) * SP_TILE + lane];
#pragma unroll
        for (int i = 0; i < KN; ++i) {
            const double c = b[(size_t)(2 * i) * L + t], s = b[(size_t)(2 * i + 1) * L + t];
            cu[i] = cu[i] + c * u;
            su[i] = su[i] + s * u;
            cv[i] = cv[i] + c * v;
            sv[i] = sv[i] + s * v;
        }
    }
}

__global__ __launch_bounds__(SP_THREADS, 4) void spectrum_kernel(const float *__restrict__ X, int L, int first, long N, long ldx,
                                                              const double *__restrict__ basis, int K, double *__restrict__ acc,
                                                              int *__restrict__ count)
{
    __shared__ float tile[SP_TC * 2 * SP_TILE];
    const int lane = threadIdx.x & (SP_TILE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long p0 = (long)blockIdx.x * SP_TILE, p = p0 + lane;
    const bool live = p < N;
    const int nchunks = (L + SP_TC - 1) / SP_TC;

    // samples t0 .. t0+nt-1 of the tile: element e = (t - t0, component, lane); a thread stages its own lane's values only
    // (a lane past N stages vector N-1 again, so that no load is conditional)
    const float *xp = X + (live ? p : N - 1);
    auto stage = [&](int t0, int nt) {
#pragma unroll 8
        for (int e = threadIdx.x; e < nt * 2 * SP_TILE; e += SP_THREADS) {
            int row = first + t0 + (e >> 7);
            if (row >= L) row -= L;
            tile[e] = xp[(size_t)row * ldx + (size_t)((e >> 6) & 1) * N];
        }
    };

    bool ok = live;
    for (int c = 0; c < nchunks; ++c) {
        const int t0 = c * SP_TC, nt = L - t0 < SP_TC ? L - t0 : SP_TC;
        if (c > 0) __syncthreads();
        stage(t0, nt);
        __syncthreads();
        for (int t = 0; t < 2 * nt; ++t) ok = ok & (fabsf(tile[t * SP_TILE + lane]) <= 1e9f);     // NaN compares false
    }
    const bool any_ok = __builtin_amdgcn_ballot_w64(ok) != 0;      // the same in all 8 waves: they hold the same 64 vectors

    // work: nfull groups of SP_KG frequencies, wave w takes group r * 8 + w in round r; the K % SP_KG frequencies left over ride along
    // in the last round, one per wave, on the chunk that is staged anyway
    const int nfull = K / SP_KG, nsingle = K % SP_KG;
    const int rounds = nfull ? (nfull + SP_WAVES - 1) / SP_WAVES : 1;
    auto put = [&](int k, double cu, double su, double cv, double sv) {
        double *a = acc + (size_t)k * 4 * N + p;
        a[0] = a[0] + (cu * cu + su * su);
        a[N] = a[N] + (cv * cv + sv * sv);
        a[2 * N] = a[2 * N] + (cu * cv + su * sv);
        a[3 * N] = a[3 * N] + (cu * sv - su * cv);
    };
    for (int r = 0; r < rounds; ++r) {
        const int group = r * SP_WAVES + wave;
        const bool grouped = any_ok && group < nfull, single = any_ok && r == rounds - 1 && wave < nsingle;
        const int k0 = group * SP_KG, k1 = nfull * SP_KG + wave;
        double cu[SP_KG], su[SP_KG], cv[SP_KG], sv[SP_KG], cu1[SP_KG], su1[SP_KG], cv1[SP_KG], sv1[SP_KG];
#pragma unroll
        for (int i = 0; i < SP_KG; ++i) cu[i] = su[i] = cv[i] = sv[i] = 0.0;
        cu1[0] = su1[0] = cv1[0] = sv1[0] = 0.0;
        for (int c = 0; c < nchunks; ++c) {
            const int t0 = c * SP_TC, nt = L - t0 < SP_TC ? L - t0 : SP_TC;
            if (nchunks > 1) {                             // a single chunk is still there from the scan
                __syncthreads();
                stage(t0, nt);
                __syncthreads();
            }
            if (grouped) spectrum_fold<SP_KG>(tile, lane, nt, basis + (size_t)k0 * 2 * L + t0, L, cu, su, cv, sv);
            if (single) spectrum_fold<1>(tile, lane, nt, basis + (size_t)k1 * 2 * L + t0, L, cu1, su1, cv1, sv1);
        }
        if (!ok) continue;
        if (grouped) {
#pragma unroll
            for (int i = 0; i < SP_KG; ++i) put(k0 + i, cu[i], su[i], cv[i], sv[i]);
        }
        if (single) put(k1, cu1[0], su1[0], cv1[0], sv1[0]);
    }
    if (ok && wave == 0) count[p] += 1;
}

int launch_spectrum_accumulate(const float *X, int L, int first, long N, long ldx, const double *basis, int K, double *acc, int *count,
                               hipStream_t st)
{
    PIV_REQUIRE(X && basis && acc && count, "spectrum_accumulate: null pointer (X, basis, acc and count are required)");
    PIV_REQUIRE(L >= 2 && L <= 1024, "spectrum_accumulate: L=%d samples per segment, must be 2..1024", L);
    PIV_REQUIRE(first >= 0 && first < L, "spectrum_accumulate: first=%d, must be 0..L-1 = %d", first, L - 1);
    PIV_REQUIRE(K >= 1 && K <= 513, "spectrum_accumulate: K=%d basis pairs, must be 1..513", K);
    PIV_REQUIRE(N >= 1 && N < (1L << 30), "spectrum_accumulate: N=%ld vectors, must be 1..2^30-1 (2N values per snapshot below 2^31)", N);
    PIV_REQUIRE(ldx >= 2 * N, "spectrum_accumulate: row stride ldx=%ld is smaller than 2N=%ld", ldx, 2 * N);
    const dim3 grid((unsigned)((N + SP_TILE - 1) / SP_TILE));
    hipLaunchKernelGGL(spectrum_kernel, grid, dim3(SP_THREADS), 0, st, X, L, first, N, ldx, basis, K, acc, count);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
