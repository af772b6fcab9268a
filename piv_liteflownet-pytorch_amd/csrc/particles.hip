// Synthetic PIV images from a known flow (gfx950): particles carried through one displacement field, and particle images rendered as
// sums of Gaussian blobs.  Arithmetic contract: include/pivlfn.h.
//
// particles_displace_kernel, one thread per particle: one bilinear (4 taps) or Catmull-Rom (16 taps) gather of the field at the
// particle's clamped position, straight from global memory as flowmap.hip's sampler does and for its reasons, all in fp64 without fma.
//
// The renderer fixes the ORDER in which a pixel adds its particles (ascending particle index, from +0.0f), so an image does not depend
// on the launch geometry, on the binning, on the batch or on the run; there is no floating-point atomic.  Five launches on one stream:
//   particles_zero_kernel    clears the per-tile counters and the list cursor (the workspace needs no initial contents);
//   particles_bin_kernel     (count) one thread per particle: one integer atomic per 16 x 16 tile its footprint touches;
//   particles_offsets_kernel one thread per tile: its list's place in the workspace, taken from one cursor (one atomic per wave).  Where
//                            a tile's list lies does not reach the result, only what it holds;
//   particles_bin_kernel     (fill) the same walk again, writing the particle's index into each tile's list -- in any order;
//   particles_render_kernel  one 256-thread workgroup per tile and image, one pixel per thread.  It first ORDERS its list in LDS: a list
//                            of up to REN_CAP indices by rank (an index's place is the number of smaller ones; indices are distinct),
//                            a longer one -- thousands of particles on one tile -- window by window over the index range: the indices
//                            of [lo, lo + REN_CAP) are marked in an LDS table by a pass over the list and compacted in order by ballot.
//                            The ordered indices are then staged through LDS in chunks of 256 particles (x, y, w, amp, floor(x),
//                            floor(y)); every thread walks a chunk in order and adds the particles whose footprint holds its pixel.
//                            Lanes outside a footprint are masked off and a wave none of whose four rows meets it skips the particle.
//                            At PIV densities the call is bound by neither the exponentials nor memory: two 1024 x 1024 frames at
//                            0.05 particles per pixel are 1.5 % of the HBM bound (DESIGN 4.15 has the measurement and where the
//                            time goes).
#include <cmath>
#include "launch_checks.h"

namespace pivlfn {

constexpr unsigned PT_LOST = PIVLFN_PARTICLES_LOST, PT_BAD = PIVLFN_PARTICLES_BAD;
constexpr int REN_TILE = 16, REN_CAP = 2048, REN_CHUNK = 256;
constexpr int REN_MAX_SIDE = 2147483647 - REN_TILE;                // a tile's last pixel index, tile origin + 15, stays an int

// ---- the displacer --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool pt_known(double c) { return fabs(c) <= 1e9; }           // NaN compares false

// Catmull-Rom weights (Keys, a = -0.5) of the taps at -1, 0, 1, 2 around the cell, in Horner form as the header writes them
__device__ __forceinline__ void pt_keys(double f, double w[4])
{
#pragma clang fp contract(off)
    w[0] = ((-0.5 * f + 1.0) * f - 0.5) * f;
    w[1] = ((1.5 * f - 2.5) * f) * f + 1.0;
    w[2] = ((-1.5 * f + 2.0) * f + 0.5) * f;
    w[3] = ((0.5 * f - 0.5) * f) * f;
}

__global__ __launch_bounds__(256) void particles_displace_kernel(const double *__restrict__ pos, const float *__restrict__ flow,
                                                                 const unsigned char *__restrict__ mask, int H, int W, int N, int method,
                                                                 unsigned char *__restrict__ flag, double *__restrict__ out)
{
#pragma clang fp contract(off)
    const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= (size_t)N) return;
    const double x = pos[n], y = pos[(size_t)N + n];
    unsigned f = flag[n];
    double ox = x, oy = y;
    if (f == 0) {
        if (x != x || y != y) {
            f = PT_BAD;
        } else {
            const double xmax = (double)(W - 1), ymax = (double)(H - 1);
            const double xc = x < 0.0 ? 0.0 : (x > xmax ? xmax : x), yc = y < 0.0 ? 0.0 : (y > ymax ? ymax : y);
            int ix = (int)floor(xc), iy = (int)floor(yc);
            ix = ix < W - 2 ? ix : W - 2;
            iy = iy < H - 2 ? iy : H - 2;
            const double fx = xc - (double)ix, fy = yc - (double)iy;
            const float *u = flow, *v = flow + (size_t)H * (size_t)W;
            double su, sv;
            bool known = true;
            if (method == 0) {
                const unsigned at = (unsigned)iy * (unsigned)W + (unsigned)ix, below = at + (unsigned)W;
                const double u00 = (double)u[at], u01 = (double)u[at + 1], u10 = (double)u[below], u11 = (double)u[below + 1];
                const double v00 = (double)v[at], v01 = (double)v[at + 1], v10 = (double)v[below], v11 = (double)v[below + 1];
                known = pt_known(u00) && pt_known(u01) && pt_known(u10) && pt_known(u11) && pt_known(v00) && pt_known(v01) &&
                        pt_known(v10) && pt_known(v11);
                if (mask) known = known && (mask[at] | mask[at + 1] | mask[below] | mask[below + 1]) == 0;
                const double gx = 1.0 - fx, gy = 1.0 - fy;
                const double ut = gx * u00 + fx * u01, ub = gx * u10 + fx * u11;
                const double vt = gx * v00 + fx * v01, vb = gx * v10 + fx * v11;
                su = ut * gy + ub * fy;
                sv = vt * gy + vb * fy;
            } else {
                double wx[4], wy[4], ru[4], rv[4];
                pt_keys(fx, wx);
                pt_keys(fy, wy);
                int cols[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int j = ix - 1 + k;
                    cols[k] = j < 0 ? 0 : (j > W - 1 ? W - 1 : j);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    int i = iy - 1 + r;
                    i = i < 0 ? 0 : (i > H - 1 ? H - 1 : i);
                    const unsigned row = (unsigned)i * (unsigned)W;
                    double cu[4], cv[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        cu[k] = (double)u[row + (unsigned)cols[k]];
                        cv[k] = (double)v[row + (unsigned)cols[k]];
                        known = known && pt_known(cu[k]) && pt_known(cv[k]);
                        if (mask) known = known && mask[row + (unsigned)cols[k]] == 0;
                    }
                    ru[r] = ((wx[0] * cu[0] + wx[1] * cu[1]) + wx[2] * cu[2]) + wx[3] * cu[3];
                    rv[r] = ((wx[0] * cv[0] + wx[1] * cv[1]) + wx[2] * cv[2]) + wx[3] * cv[3];
                }
                su = ((wy[0] * ru[0] + wy[1] * ru[1]) + wy[2] * ru[2]) + wy[3] * ru[3];
                sv = ((wy[0] * rv[0] + wy[1] * rv[1]) + wy[2] * rv[2]) + wy[3] * rv[3];
            }
            if (known) {
                ox = x + su;
                oy = y + sv;
            } else {
                f = PT_LOST;
            }
        }
    }
    out[n] = ox;
    out[(size_t)N + n] = oy;
    flag[n] = (unsigned char)f;
}

// ---- the renderer ---------------------------------------------------------------------------------------------------------------------
// Workspace: [0] the list cursor (8 bytes) and 8 bytes unused; cnt[B*T] u32 (rounded up to a whole 8 bytes); off[B*T] u64;
// list[B*N*K] u32, K = the most tiles one footprint touches.
struct RenderWs {
    unsigned long long *cursor;
    unsigned *cnt;
    unsigned long long *off;
    unsigned *list;
};

static inline int render_tiles_per_axis(int radius) { return (2 * radius) / REN_TILE + 2; }      // a footprint is 2R+2 pixels wide

// bytes of the workspace, 0 where the arguments are out of range or the size does not fit
static size_t render_ws_layout(int B, int N, int H, int W, int radius, void *base, RenderWs *ws)
{
    if (B < 0 || N < 0 || H < 1 || W < 1 || H > REN_MAX_SIDE || W > REN_MAX_SIDE || radius < 1 || radius > 8 ||
        (size_t)H * W >= ((size_t)1 << 31))
        return 0;
    const size_t tiles = (size_t)B * cdiv(H, REN_TILE) * cdiv(W, REN_TILE), K = (size_t)render_tiles_per_axis(radius) * render_tiles_per_axis(radius);
    size_t entries, list_bytes;
    if (__builtin_mul_overflow((size_t)B * (size_t)N, K, &entries) || __builtin_mul_overflow(entries, (size_t)4, &list_bytes)) return 0;
    const size_t cnt_bytes = (tiles * 4 + 7) / 8 * 8, head = 16 + cnt_bytes + tiles * 8;
    if (list_bytes > ~(size_t)0 - head - 8) return 0;
    if (ws) {
        char *p = static_cast<char *>(base);
        ws->cursor = reinterpret_cast<unsigned long long *>(p);
        ws->cnt = reinterpret_cast<unsigned *>(p + 16);
        ws->off = reinterpret_cast<unsigned long long *>(p + 16 + cnt_bytes);
        ws->list = reinterpret_cast<unsigned *>(p + head);
    }
    return head + (list_bytes + 7) / 8 * 8;
}

size_t particles_render_workspace_bytes(int B, int N, int H, int W, int radius) { return render_ws_layout(B, N, H, W, radius, nullptr, nullptr); }

__global__ __launch_bounds__(256) void particles_zero_kernel(RenderWs ws, unsigned tiles)
{
    const unsigned t = blockIdx.x * 256 + threadIdx.x;
    if (t == 0) *ws.cursor = 0ull;
    if (t < tiles) ws.cnt[t] = 0u;
}

// Whether particle n of image b is drawn, and the tiles [tx0, tx1] x [ty0, ty1] its footprint touches (empty where it lies outside).
__device__ __forceinline__ bool particle_tiles(const double *__restrict__ pos, const float *__restrict__ diam, const float *__restrict__ amp,
                                               const unsigned char *__restrict__ flag, size_t b, size_t n, size_t N, int H, int W, int R,
                                               int &tx0, int &tx1, int &ty0, int &ty1)
{
#pragma clang fp contract(off)
    const size_t at = b * N + n;
    if (flag && flag[at]) return false;
    const double x = pos[b * 2 * N + n], y = pos[b * 2 * N + N + n];
    const float d = diam[at], a = amp[at];
    if (!(fabs(x) < 1073741824.0 && fabs(y) < 1073741824.0)) return false;                      // NaN and inf fail too
    if (!(d > 0.0f && d <= 3.402823466e38f && a >= 0.0f && a <= 3.402823466e38f)) return false;
    const float s = 0.5f * d, w = 1.0f / (s * s);
    if (!(w <= 3.402823466e38f)) return false;                                                 // a diameter below 4e-19 px: 1/s^2 overflows
    const int ix = (int)floor(x), iy = (int)floor(y);
    const int xa = max(ix - R, 0), xb = min(ix + R + 1, W - 1), ya = max(iy - R, 0), yb = min(iy + R + 1, H - 1);
    if (xa > xb || ya > yb) return false;
    tx0 = xa / REN_TILE; tx1 = xb / REN_TILE; ty0 = ya / REN_TILE; ty1 = yb / REN_TILE;
    return true;
}

template <bool FILL>
__global__ __launch_bounds__(256) void particles_bin_kernel(const double *__restrict__ pos, const float *__restrict__ diam,
                                                            const float *__restrict__ amp, const unsigned char *__restrict__ flag, int B, int N,
                                                            int H, int W, int R, RenderWs ws)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (size_t)B * (size_t)N) return;
    const size_t b = g / (size_t)N, n = g - b * (size_t)N;
    int tx0, tx1, ty0, ty1;
    if (!particle_tiles(pos, diam, amp, flag, b, n, (size_t)N, H, W, R, tx0, tx1, ty0, ty1)) return;
    const int TX = (W + REN_TILE - 1) / REN_TILE, TY = (H + REN_TILE - 1) / REN_TILE;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
            const size_t t = (b * TY + ty) * TX + tx;
            const unsigned k = atomicAdd(&ws.cnt[t], 1u);
            if (FILL) ws.list[ws.off[t] + k] = (unsigned)n;
        }
}

// off[t] = where tile t's list starts; cnt[t] back to 0 for the fill to count up again
__global__ __launch_bounds__(256) void particles_offsets_kernel(RenderWs ws, unsigned tiles)
{
    const unsigned t = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const unsigned c = t < tiles ? ws.cnt[t] : 0u;
    unsigned long long incl = c;                                    // inclusive prefix over the wave
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long up = __shfl_up(incl, d, 64);
        if ((int)lane >= d) incl += up;
    }
    const unsigned long long total = __shfl(incl, 63, 64);
    unsigned long long base = 0;
    if (lane == 63 && total) base = atomicAdd(ws.cursor, total);
    base = __shfl(base, 63, 64);
    if (t < tiles) {
        ws.off[t] = base + incl - c;
        ws.cnt[t] = 0u;
    }
}

__global__ __launch_bounds__(256) void particles_render_kernel(const double *__restrict__ pos, const float *__restrict__ diam,
                                                               const float *__restrict__ amp, int N, int H, int W, int R, RenderWs ws,
                                                               float *__restrict__ intensity, unsigned char *__restrict__ image)
{
#pragma clang fp contract(off)
    __shared__ unsigned s_in[REN_CAP];                              // the list as it lies in the workspace, or the table of one window
    __shared__ unsigned s_sorted[REN_CAP];
    __shared__ double s_x[REN_CHUNK], s_y[REN_CHUNK];
    __shared__ float s_w[REN_CHUNK], s_a[REN_CHUNK];
    __shared__ int s_ix[REN_CHUNK], s_iy[REN_CHUNK];
    __shared__ unsigned s_wave[4];

    const int TX = (W + REN_TILE - 1) / REN_TILE, TY = (H + REN_TILE - 1) / REN_TILE;
    const unsigned tile = blockIdx.x, tid = threadIdx.x;
    const unsigned b = tile / (unsigned)(TX * TY), tin = tile - b * (unsigned)(TX * TY);
    const int j = (int)(tin % (unsigned)TX) * REN_TILE + (int)(tid & 15u), i = (int)(tin / (unsigned)TX) * REN_TILE + (int)(tid >> 4);
    const unsigned L = ws.cnt[tile];
    const unsigned *__restrict__ list = ws.list + ws.off[tile];
    const double *px = pos + (size_t)b * 2 * N, *py = px + N;
    const float *pd = diam + (size_t)b * N, *pa = amp + (size_t)b * N;
    const double dj = (double)j, di = (double)i;
    const unsigned span = 2u * (unsigned)R + 1u;
    float acc = 0.0f;

    // windows of the index range: one that holds everything where the list fits the LDS, else [lo, lo + REN_CAP) for lo = 0, REN_CAP, ...
    const bool fits = L <= (unsigned)REN_CAP;
    for (unsigned lo = 0; lo < (fits ? 1u : (unsigned)N); lo += REN_CAP) {
        unsigned m;                                                 // s_sorted[0 .. m) = the indices of this window, ascending
        __syncthreads();                                            // the walk of the window before is over
        if (fits) {
            for (unsigned e = tid; e < L; e += 256) s_in[e] = list[e];
            __syncthreads();
            unsigned mine[REN_CAP / 256], rank[REN_CAP / 256];
#pragma unroll
            for (int r = 0; r < REN_CAP / 256; ++r) {
                const unsigned e = tid + 256u * r;
                mine[r] = e < L ? s_in[e] : 0xFFFFFFFFu;
                rank[r] = 0;
            }
            const unsigned rounds = (L + 255u) / 256u;              // uniform: how many of mine[] are in use
            for (unsigned k = 0; k < L; ++k) {
                const unsigned v = s_in[k];
#pragma unroll
                for (int r = 0; r < REN_CAP / 256; ++r)
                    if ((unsigned)r < rounds) rank[r] += v < mine[r] ? 1u : 0u;
            }
#pragma unroll
            for (int r = 0; r < REN_CAP / 256; ++r)
                if (tid + 256u * r < L) s_sorted[rank[r]] = mine[r];
            m = L;
        } else {
            for (unsigned e = tid; e < (unsigned)REN_CAP; e += 256) s_in[e] = 0u;
            __syncthreads();
            for (unsigned e = tid; e < L; e += 256) {
                const unsigned v = list[e];
                if (v - lo < (unsigned)REN_CAP) s_in[v - lo] = 1u;  // unsigned: v < lo wraps past REN_CAP
            }
            __syncthreads();
            m = 0;                                                  // every thread keeps the same running total
            for (unsigned r = 0; r < (unsigned)REN_CAP / 256u; ++r) {       // in-order compaction, 256 table entries a round
                const unsigned e = r * 256u + tid;
                const bool here = s_in[e] != 0u;
                const unsigned long long vote = __ballot(here);
                if ((tid & 63u) == 0u) s_wave[tid >> 6] = (unsigned)__popcll(vote);
                __syncthreads();
                unsigned before = m;
                for (unsigned wv = 0; wv < (tid >> 6); ++wv) before += s_wave[wv];
                if (here) s_sorted[before + (unsigned)__popcll(vote & ((1ull << (tid & 63u)) - 1ull))] = lo + e;
                m += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
                __syncthreads();                                    // s_wave is read before the next round writes it
            }
        }
        for (unsigned c0 = 0; c0 < m; c0 += REN_CHUNK) {
            __syncthreads();                                        // s_sorted is written; the chunk before has been walked
            const unsigned cn = min(m - c0, (unsigned)REN_CHUNK);
            if (tid < cn) {
                const unsigned p = s_sorted[c0 + tid];
                const double x = px[p], y = py[p];
                const float s = 0.5f * pd[p];
                s_x[tid] = x;
                s_y[tid] = y;
                s_w[tid] = 1.0f / (s * s);
                s_a[tid] = pa[p];
                s_ix[tid] = (int)floor(x);
                s_iy[tid] = (int)floor(y);
            }
            __syncthreads();
            for (unsigned p = 0; p < cn; ++p) {
                // j in [ix - R, ix + R + 1] and i in [iy - R, iy + R + 1], each as one unsigned comparison
                if ((unsigned)(j - s_ix[p] + R) <= span && (unsigned)(i - s_iy[p] + R) <= span) {
                    const float dx = (float)(dj - s_x[p]), dy = (float)(di - s_y[p]);
                    const float q = (dx * dx + dy * dy) * s_w[p];
                    const float t = s_a[p] * expf(-q);
                    acc = acc + t;
                }
            }
        }
    }
    if (i < H && j < W) {
        const size_t at = ((size_t)b * H + i) * W + j;
        intensity[at] = acc;
        image[at] = (unsigned char)fminf(acc, 255.0f);
    }
}

int launch_particles_displace(const double *pos, const float *flow, const unsigned char *mask, int H, int W, int N, int method,
                              unsigned char *flag, double *out, hipStream_t st)
{
    PIV_REQUIRE(H >= 2 && W >= 2, "particles_displace: bad shape H=%d W=%d (a sample needs 2 x 2 vectors)", H, W);
    PIV_REQUIRE((size_t)H * W < ((size_t)1 << 31), "particles_displace: H*W=%zu pixels, must stay below 2^31 (32-bit pixel index)", (size_t)H * W);
    PIV_REQUIRE(N >= 0, "particles_displace: N=%d particles, must not be negative", N);
    PIV_REQUIRE(method == 0 || method == 1, "particles_displace: method=%d must be 0 (bilinear) or 1 (Catmull-Rom bicubic)", method);
    if (N == 0) return PIVLFN_OK;                                   // nothing to move: no pointer is read
    PIV_REQUIRE(pos && flow && flag && out, "particles_displace: null pointer (pos, flow, flag and out are required)");
    const size_t px = (size_t)H * W;
    const Span moved = {out, (size_t)N * 16, "out"}, flg = {flag, (size_t)N, "flag"};
    if (int rc = check_alias_by_input("particles_displace", {moved, flg}, {{pos, (size_t)N * 16, "pos"}, {flow, px * 8, "flow"}, {mask, px, "mask"}},
                                      " (the outputs must not alias an input)"))
        return rc;
    if (int rc = check_apart("particles_displace", moved, flg)) return rc;
    hipLaunchKernelGGL(particles_displace_kernel, dim3((unsigned)(((size_t)N + 255) / 256)), dim3(256), 0, st, pos, flow, mask, H, W, N, method,
                       flag, out);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

int launch_particles_render(const double *pos, const float *diam, const float *amp, const unsigned char *flag, int B, int N, int H, int W,
                            int radius, float *intensity, unsigned char *image, void *workspace, size_t workspace_bytes, hipStream_t st)
{
    PIV_REQUIRE(H >= 1 && W >= 1, "particles_render: bad shape H=%d W=%d (both must be positive)", H, W);
    PIV_REQUIRE(H <= REN_MAX_SIDE && W <= REN_MAX_SIDE, "particles_render: H=%d W=%d, a side must not exceed 2^31 - 17 pixels", H, W);
    PIV_REQUIRE((size_t)H * W < ((size_t)1 << 31), "particles_render: H*W=%zu pixels, must stay below 2^31", (size_t)H * W);
    PIV_REQUIRE(B >= 0 && N >= 0, "particles_render: B=%d images of N=%d particles, neither may be negative", B, N);
    PIV_REQUIRE(radius >= 1 && radius <= 8, "particles_render: radius=%d must be 1..8 pixels", radius);
    if (B == 0) return PIVLFN_OK;                                   // no image: nothing is launched, no pointer is read
    const size_t tiles = (size_t)B * cdiv(H, REN_TILE) * cdiv(W, REN_TILE), bn = (size_t)B * (size_t)N;
    PIV_REQUIRE(tiles < ((size_t)1 << 31), "particles_render: %zu tiles of 16 x 16 pixels over the batch, must stay below 2^31", tiles);
    PIV_REQUIRE((bn + 255) / 256 < ((size_t)1 << 31), "particles_render: B*N=%zu particles, must stay below 2^39", bn);
    RenderWs ws;
    const size_t need = render_ws_layout(B, N, H, W, radius, workspace, &ws);
    PIV_REQUIRE(need > 0, "particles_render: the workspace of B=%d N=%d H=%d W=%d does not fit size_t", B, N, H, W);
    PIV_REQUIRE(intensity && image && workspace, "particles_render: null pointer (intensity, image and workspace are required)");
    PIV_REQUIRE(N == 0 || (pos && diam && amp), "particles_render: null pointer (pos, diam and amp are required)");
    PIV_REQUIRE(reinterpret_cast<size_t>(workspace) % 8 == 0, "particles_render: the workspace must be 8-byte aligned");
    PIV_REQUIRE(workspace_bytes >= need, "particles_render: workspace of %zu bytes, needs %zu (pivlfn_particles_render_workspace_bytes)",
                workspace_bytes, need);
    const size_t px = (size_t)B * H * W;
    const std::initializer_list<Span> outs = {{intensity, px * 4, "intensity"}, {image, px, "image"}, {workspace, need, "workspace"}};
    if (int rc = check_alias_by_output("particles_render", outs, {{pos, bn * 16, "pos"}, {diam, bn * 4, "diam"}, {amp, bn * 4, "amp"}, {flag, bn, "flag"}},
                                       " (what is written must not alias an input)"))
        return rc;
    if (int rc = check_outputs_apart("particles_render", outs)) return rc;
    const unsigned tb = (unsigned)((tiles + 255) / 256), pb = (unsigned)((bn + 255) / 256);
    hipLaunchKernelGGL(particles_zero_kernel, dim3(tb), dim3(256), 0, st, ws, (unsigned)tiles);
    if (pb) hipLaunchKernelGGL(particles_bin_kernel<false>, dim3(pb), dim3(256), 0, st, pos, diam, amp, flag, B, N, H, W, radius, ws);
    hipLaunchKernelGGL(particles_offsets_kernel, dim3(tb), dim3(256), 0, st, ws, (unsigned)tiles);
    if (pb) hipLaunchKernelGGL(particles_bin_kernel<true>, dim3(pb), dim3(256), 0, st, pos, diam, amp, flag, B, N, H, W, radius, ws);
    hipLaunchKernelGGL(particles_render_kernel, dim3((unsigned)tiles), dim3(256), 0, st, pos, diam, amp, N, H, W, radius, ws, intensity, image);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
