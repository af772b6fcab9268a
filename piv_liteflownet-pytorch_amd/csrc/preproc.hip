// Image pre-processing of uint8 frame batches (gfx950): background subtraction, sliding min-max normalisation (Westerweel 1993;
// Adrian & Westerweel 2011), conversion to the planar fp32 input of the network.  Reads [n,H,W,3] bytes -- what PairLoader uploads --
// and writes [n,3,H,W] floats in [0,1].  Arithmetic contract: include/pivlfn.h.  Everything up to the one division is integer.
//
// Min-max kernel: a 256-thread workgroup owns a 64 x 64 output tile of one channel of one frame and keeps every intermediate in LDS
// (r = k/2, NX = 64 + 4r, NM = 64 + 2r):
//   X   u8  [NX][NX]   the input with the background subtracted, coordinates clamped to the image
//   RM  u16 [NX][NM]   min | max << 8 over the k columns of a row                          (lanes over rows, runs along the row)
//   M   u32 [NM][NM]   min | max << 16 over the k rows of that: lo and hi of the contract  (lanes over columns, runs down the column)
//       positions outside the image then take the value of the clamped position (lo and hi are replicated, not recomputed)
//   RS  u32 [NM][64]   both row sums of M in one word (31 * 255 < 2^16)                    (lanes over rows)
//   L, S               the column sums of that, in registers; num, den, one division, one coalesced store per row
// A thread computes a run of RUN consecutive outputs of a line at once: the RUN windows share k - RUN + 1 elements, whose min / max
// is taken once, and each output adds a suffix of the RUN - 1 elements before and a prefix of the RUN - 1 after (k + RUN - 1 reads
// for RUN outputs instead of RUN * k); sums slide.  Row strides are odd numbers of dwords, so lanes that walk down rows hit 32
// different banks.  RS takes the place of RM, which is dead by then; 64 x 64 at k = 31 needs 74 KiB: two workgroups per CU.
#include "launch_checks.h"

namespace pivlfn {

constexpr int PT = 64;                     // tile edge

__host__ __device__ __forceinline__ int odd_dwords(int bytes)       // the next stride in bytes that is an odd number of dwords
{
    return (((bytes + 3) >> 2) | 1) << 2;
}

struct PreLayout {
    int NX, NM, SX, SRM, SM, SRS;          // SX in bytes, SRM in u16 elements, SM and SRS in dwords
    int offX, offRM, bytes;                // M at 0; RS shares RM's place
};

__host__ __device__ __forceinline__ PreLayout pre_layout(int r)
{
    PreLayout g;
    g.NX = PT + 4 * r;
    g.NM = PT + 2 * r;
    g.SX = odd_dwords(g.NX);
    g.SRM = odd_dwords(2 * g.NM) >> 1;
    g.SM = g.NM | 1;
    g.SRS = PT + 1;
    g.offX = g.NM * g.SM * 4;
    g.offRM = g.offX + g.NX * g.SX;
    const int rm = g.NX * g.SRM * 2, rs = g.NM * g.SRS * 4;
    g.bytes = g.offRM + (rm > rs ? rm : rs);
    return g;
}

struct Pair { int lo, hi; };

// lo[j], hi[j] = min, max of load(j) .. load(j + k - 1) for j < RUN; needs k >= RUN - 1.  Indices beyond `last` (read only by outputs
// the caller drops) are clamped to it.
template <int RUN, typename Load>
__device__ __forceinline__ void run_minmax(Load load, int k, int last, int (&lo)[RUN], int (&hi)[RUN])
{
    int cl = 255, ch = 0;
    for (int t = RUN - 1; t < k; ++t) {                        // the elements every window of the run holds
        const Pair v = load(t);
        cl = min(cl, v.lo);
        ch = max(ch, v.hi);
    }
    lo[RUN - 1] = cl;
    hi[RUN - 1] = ch;
    int sl = 255, sh = 0;
#pragma unroll
    for (int j = RUN - 2; j >= 0; --j) {                       // window j also holds j .. RUN - 2
        const Pair v = load(j);
        sl = min(sl, v.lo);
        sh = max(sh, v.hi);
        lo[j] = min(cl, sl);
        hi[j] = max(ch, sh);
    }
    int pl = 255, ph = 0;
#pragma unroll
    for (int j = 1; j < RUN; ++j) {                            // and k .. k + j - 1
        const Pair v = load(min(k + j - 1, last));
        pl = min(pl, v.lo);
        ph = max(ph, v.hi);
        lo[j] = min(lo[j], pl);
        hi[j] = max(hi[j], ph);
    }
}

template <int RUN>
__global__ __launch_bounds__(256) void frames_preprocess_minmax_kernel(const unsigned char *__restrict__ frames,
                                                                        const unsigned char *__restrict__ bg, float *__restrict__ out,
                                                                        int H, int W, int r, int floor_n, int tiles_x)
{
    extern __shared__ __align__(16) unsigned char lds[];
    const PreLayout g = pre_layout(r);
    const int k = 2 * r + 1, n = k * k;
    unsigned *M = reinterpret_cast<unsigned *>(lds);
    unsigned char *X = lds + g.offX;
    unsigned short *RM = reinterpret_cast<unsigned short *>(lds + g.offRM);
    unsigned *RS = reinterpret_cast<unsigned *>(lds + g.offRM);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int y0 = ty * PT, x0 = tx * PT, c = blockIdx.y;
    const size_t HW = (size_t)H * W;
    const unsigned char *src = frames + (size_t)blockIdx.z * HW * 3 + c;
    const unsigned char *sub = bg ? bg + c : nullptr;

    // X: rows over waves, columns over lanes
    for (int i = wave; i < g.NX; i += 4) {
        const int gy = min(max(y0 - 2 * r + i, 0), H - 1);
        for (int j = lane; j < g.NX; j += 64) {
            const int gx = min(max(x0 - 2 * r + j, 0), W - 1);
            const size_t o = ((size_t)gy * W + gx) * 3;
            int v = src[o];
            if (sub) v = max(v - (int)sub[o], 0);
            X[i * g.SX + j] = (unsigned char)v;
        }
    }
    __syncthreads();

    // RM: column j of a row is the min / max of X's columns j .. j + k - 1
    const int runs_m = (g.NM + RUN - 1) / RUN;
    for (int i = lane; i < g.NX; i += 64)
        for (int q = wave; q < runs_m; q += 4) {
            const unsigned char *in = X + i * g.SX + q * RUN;
            int lo[RUN], hi[RUN];
            run_minmax<RUN>([&](int t) { const int v = in[t]; return Pair{v, v}; }, k, g.NX - 1 - q * RUN, lo, hi);
#pragma unroll
            for (int j = 0; j < RUN; ++j)
                if (q * RUN + j < g.NM) RM[i * g.SRM + q * RUN + j] = (unsigned short)(lo[j] | (hi[j] << 8));
        }
    __syncthreads();

    // M: row i of a column is the min / max of RM's rows i .. i + k - 1
    for (int j = lane; j < g.NM; j += 64)
        for (int q = wave; q < runs_m; q += 4) {
            const unsigned short *in = RM + q * RUN * g.SRM + j;
            int lo[RUN], hi[RUN];
            run_minmax<RUN>([&](int t) { const int v = in[t * g.SRM]; return Pair{v & 255, v >> 8}; }, k, g.NX - 1 - q * RUN, lo, hi);
#pragma unroll
            for (int i = 0; i < RUN; ++i)
                if (q * RUN + i < g.NM) M[(q * RUN + i) * g.SM + j] = (unsigned)(lo[i] | (hi[i] << 16));
        }
    __syncthreads();

    // edge replication of lo and hi: a position outside the image holds what the nearest position inside holds.  Only positions
    // inside are read and only positions outside are written.
    if (y0 - r < 0 || x0 - r < 0 || y0 + PT + r > H || x0 + PT + r > W) {
        for (int i = wave; i < g.NM; i += 4) {
            const int gy = y0 - r + i, ci = min(max(gy, 0), H - 1) - (y0 - r);
            for (int j = lane; j < g.NM; j += 64) {
                const int gx = x0 - r + j, cj = min(max(gx, 0), W - 1) - (x0 - r);
                if (ci != i || cj != j) M[i * g.SM + j] = M[ci * g.SM + cj];
            }
        }
        __syncthreads();
    }

    // RS: column j of a row is the sum of M's columns j .. j + k - 1, both halves of the word at once
    for (int i = lane; i < g.NM; i += 64)
        for (int q = wave; q < PT / RUN; q += 4) {
            const unsigned *in = M + i * g.SM + q * RUN;
            unsigned acc = 0;
            for (int t = 0; t < k; ++t) acc += in[t];
            RS[i * g.SRS + q * RUN] = acc;
#pragma unroll
            for (int j = 1; j < RUN; ++j) {
                acc = acc + in[k + j - 1] - in[j - 1];                   // no borrow: each half of the new sum holds the old element
                RS[i * g.SRS + q * RUN + j] = acc;
            }
        }
    __syncthreads();

    // L, S: the sums of RS's rows i .. i + k - 1; one output row per step, 64 lanes side by side
    const int gx = x0 + lane;
    float *dst = out + ((size_t)blockIdx.z * 3 + c) * HW;
    for (int q = wave; q < PT / RUN; q += 4) {
        const unsigned *in = RS + q * RUN * g.SRS + lane;
        int L = 0, S = 0;
        for (int t = 0; t < k; ++t) {
            const unsigned v = in[t * g.SRS];
            L += (int)(v & 0xffffu);
            S += (int)(v >> 16);
        }
#pragma unroll
        for (int i = 0; i < RUN; ++i) {
            const int gy = y0 + q * RUN + i;
            if (i > 0) {
                const unsigned a = in[(k + i - 1) * g.SRS], b = in[(i - 1) * g.SRS];
                L += (int)(a & 0xffffu) - (int)(b & 0xffffu);
                S += (int)(a >> 16) - (int)(b >> 16);
            }
            if (gy < H && gx < W) {
                const int x = X[(q * RUN + i + 2 * r) * g.SX + lane + 2 * r];
                const int num = n * x - L, den = max(S - L, floor_n);
                dst[(size_t)gy * W + gx] = (float)num / (float)den;      // IEEE division (hipcc's default for HIP)
            }
        }
    }
}

// k = 0: (x - background, clamped at 0) / 255 and the transpose to planes.  VEC: four pixels per thread, 12 bytes in and a float4 per
// plane out (H*W a multiple of 4 and aligned pointers: the launcher decides); else one pixel per thread.
template <bool VEC>
__global__ __launch_bounds__(256) void frames_preprocess_scale_kernel(const unsigned char *__restrict__ frames,
                                                                       const unsigned char *__restrict__ bg, float *__restrict__ out,
                                                                       unsigned HW)
{
    constexpr unsigned P = VEC ? 4 : 1;
    const unsigned char *src = frames + (size_t)blockIdx.y * HW * 3;
    float *dst = out + (size_t)blockIdx.y * HW * 3;
    for (unsigned pix = (blockIdx.x * 256 + threadIdx.x) * P; pix < HW; pix += gridDim.x * 256 * P) {
        unsigned char v[3 * P], b[3 * P] = {};
        if (VEC) {
            const uint3 w = *reinterpret_cast<const uint3 *>(src + (size_t)pix * 3);
            memcpy(v, &w, 12);
            if (bg) {
                const uint3 wb = *reinterpret_cast<const uint3 *>(bg + (size_t)pix * 3);
                memcpy(b, &wb, 12);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                v[e] = src[(size_t)pix * 3 + e];
                if (bg) b[e] = bg[(size_t)pix * 3 + e];
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float f[P];
#pragma unroll
            for (unsigned e = 0; e < P; ++e) f[e] = (float)max((int)v[e * 3 + ch] - (int)b[e * 3 + ch], 0) / 255.0f;
            if (VEC)
                *reinterpret_cast<float4 *>(dst + (size_t)ch * HW + pix) = make_float4(f[0], f[1 % P], f[2 % P], f[3 % P]);
            else
                dst[(size_t)ch * HW + pix] = f[0];
        }
    }
}

// bg = min(bg, the frames), byte by byte.  VEC: four bytes per thread (a whole number of dwords per frame, aligned pointers).
template <bool VEC>
__global__ __launch_bounds__(256) void frames_background_min_kernel(const unsigned char *__restrict__ frames, unsigned char *bg, int n,
                                                                     size_t bytes)
{
    constexpr size_t P = VEC ? 4 : 1;
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * P; i < bytes; i += (size_t)gridDim.x * 256 * P) {
        if (VEC) {
            const unsigned w = *reinterpret_cast<const unsigned *>(bg + i);
            unsigned m0 = w & 255u, m1 = (w >> 8) & 255u, m2 = (w >> 16) & 255u, m3 = w >> 24;
            for (int t = 0; t < n; ++t) {
                const unsigned f = *reinterpret_cast<const unsigned *>(frames + (size_t)t * bytes + i);
                m0 = min(m0, f & 255u);
                m1 = min(m1, (f >> 8) & 255u);
                m2 = min(m2, (f >> 16) & 255u);
                m3 = min(m3, f >> 24);
            }
            *reinterpret_cast<unsigned *>(bg + i) = m0 | (m1 << 8) | (m2 << 16) | (m3 << 24);
        } else {
            unsigned m = bg[i];
            for (int t = 0; t < n; ++t) m = min(m, (unsigned)frames[(size_t)t * bytes + i]);
            bg[i] = (unsigned char)m;
        }
    }
}

static bool aligned_to(const void *p, size_t a) { return p == nullptr || (reinterpret_cast<size_t>(p) & (a - 1)) == 0; }

// the shape of byte frames: its bound is on H*W*3, the bytes of a frame, so it is not launch_checks.h's check_shape
static int check_frames(const char *what, int n, int H, int W)
{
    PIV_REQUIRE(n > 0 && H > 0 && W > 0, "%s: bad shape n=%d H=%d W=%d (all must be positive)", what, n, H, W);
    PIV_REQUIRE((size_t)H * W * 3 < ((size_t)1 << 31), "%s: H*W*3=%zu bytes per frame, must stay below 2^31", what, (size_t)H * W * 3);
    return PIVLFN_OK;
}

int launch_frames_background_min(const unsigned char *frames, unsigned char *bg, int n, int H, int W, hipStream_t st)
{
    PIV_REQUIRE(frames && bg, "frames_background_min: null pointer (frames and bg are required)");
    if (int rc = check_frames("frames_background_min", n, H, W)) return rc;
    const size_t bytes = (size_t)H * W * 3;
    PIV_REQUIRE(!ranges_overlap(frames, bytes * n, bg, bytes), "frames_background_min: bg aliases frames (bg must not overlap the frames)");
    const bool vec = bytes % 4 == 0 && aligned_to(frames, 4) && aligned_to(bg, 4);
    const unsigned blocks = frame_grid(vec ? bytes / 4 : bytes, 1);
    if (vec)
        hipLaunchKernelGGL(frames_background_min_kernel<true>, dim3(blocks), dim3(256), 0, st, frames, bg, n, bytes);
    else
        hipLaunchKernelGGL(frames_background_min_kernel<false>, dim3(blocks), dim3(256), 0, st, frames, bg, n, bytes);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

int launch_frames_preprocess(const unsigned char *frames, const unsigned char *bg, float *out, int n, int H, int W, int k, int floor,
                             hipStream_t st)
{
    PIV_REQUIRE(frames && out, "frames_preprocess: null pointer (frames and out are required)");
    if (int rc = check_frames("frames_preprocess", n, H, W)) return rc;
    PIV_REQUIRE(n <= 65535, "frames_preprocess: n=%d frames, at most 65535 per call (grid dimension)", n);
    PIV_REQUIRE(k == 0 || (k >= 3 && k <= 31 && (k & 1)), "frames_preprocess: k=%d must be 0 (no min-max) or odd in 3..31", k);
    PIV_REQUIRE(floor >= 1 && floor <= 255, "frames_preprocess: floor=%d must be in 1..255", floor);
    const size_t HW = (size_t)H * W;
    PIV_REQUIRE(!ranges_overlap(frames, HW * 3 * n, out, HW * 12 * n), "frames_preprocess: out aliases frames (out must not overlap the frames)");
    PIV_REQUIRE(!ranges_overlap(bg, HW * 3, out, HW * 12 * n), "frames_preprocess: out aliases bg (out must not overlap the background)");
    if (k == 0) {
        const bool vec = HW % 4 == 0 && aligned_to(frames, 4) && aligned_to(bg, 4) && aligned_to(out, 16);
        const dim3 grid(frame_grid(vec ? HW / 4 : HW, n), (unsigned)n);
        if (vec)
            hipLaunchKernelGGL(frames_preprocess_scale_kernel<true>, grid, dim3(256), 0, st, frames, bg, out, (unsigned)HW);
        else
            hipLaunchKernelGGL(frames_preprocess_scale_kernel<false>, grid, dim3(256), 0, st, frames, bg, out, (unsigned)HW);
        PIV_CHECK_HIP(hipGetLastError());
        return PIVLFN_OK;
    }
    const int r = k / 2, tiles_x = cdiv(W, PT), tiles_y = cdiv(H, PT);
    const PreLayout g = pre_layout(r);
    const dim3 grid((unsigned)(tiles_x * tiles_y), 3, (unsigned)n);
    static LdsAttr attr8, attr4;
    if (k >= 7) {                                              // a run of 8 needs k >= 7
        if (int rc = ensure_dyn_lds(attr8, reinterpret_cast<const void *>(frames_preprocess_minmax_kernel<8>), g.bytes)) return rc;
        hipLaunchKernelGGL(frames_preprocess_minmax_kernel<8>, grid, dim3(256), g.bytes, st, frames, bg, out, H, W, r, floor * k * k, tiles_x);
    } else {
        if (int rc = ensure_dyn_lds(attr4, reinterpret_cast<const void *>(frames_preprocess_minmax_kernel<4>), g.bytes)) return rc;
        hipLaunchKernelGGL(frames_preprocess_minmax_kernel<4>, grid, dim3(256), g.bytes, st, frames, bg, out, H, W, r, floor * k * k, tiles_x);
    }
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
