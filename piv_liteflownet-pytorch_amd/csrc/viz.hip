// Pictures of flows and scalar fields (gfx950): the Middlebury colour coding of the reference's src/utils_plot.py (motion_to_color
// :199-256) and src/utils_color.py (compute_color :57-93), a 256-entry colour map for scalar fields such as the vorticity, the per-image
// maxima that normalise both, and cell means for quiver plots.  Reads [B,2,H,W] NCHW flows (what estimate(..., tensor=True) returns),
// writes packed bytes [B,H,W,3].  Arithmetic contract: include/pivlfn.h.
//
// The byte images are contiguous over rows and images, so a picture batch is one flat run of B*H*W pixels of 3 bytes.  A thread owns 4
// consecutive pixels of that run: 12 bytes, three whole dwords at a 4-byte aligned offset whatever H and W are.  A row has no ragged
// edge of its own; the one partial group is the last of the buffer, which stores its 1..3 pixels byte by byte, and so does every
// group when the output pointer is not 4-byte aligned.  Loads take 16 bytes per plane where H*W is a multiple of 4 and the planes are
// 16-byte aligned (a group then lies inside one image), single floats otherwise.
#include <cmath>
#include "launch_checks.h"

namespace pivlfn {

constexpr int VZ_THREADS = 256;
constexpr int VZ_NCOLS = 55;          // RY + YG + GC + CB + BM + MR of the Middlebury wheel
constexpr unsigned VZ_MAX_BLOCKS = 4096;

struct WheelTable { double c[VZ_NCOLS * 3]; };

// colorwheel[k][b] / 255.0 of src/utils_color.py:23-54, in its operations: 255 * i / N is the quotient of two exact integers in fp64.
constexpr WheelTable make_wheel()
{
    WheelTable t{};
    const int len[6] = {15, 6, 4, 11, 13, 6};
    int k = 0;
    for (int seg = 0; seg < 6; ++seg)
        for (int i = 0; i < len[seg]; ++i, ++k) {
            const double up = (double)(255 * i) / (double)len[seg], down = 255.0 - up;
            double r = 0.0, g = 0.0, b = 0.0;
            if (seg == 0) { r = 255.0; g = up; }
            else if (seg == 1) { r = down; g = 255.0; }
            else if (seg == 2) { g = 255.0; b = up; }
            else if (seg == 3) { g = down; b = 255.0; }
            else if (seg == 4) { r = up; b = 255.0; }
            else { r = 255.0; b = down; }
            t.c[3 * k] = r / 255.0;
            t.c[3 * k + 1] = g / 255.0;
            t.c[3 * k + 2] = b / 255.0;
        }
    return t;
}

__constant__ WheelTable g_wheel = make_wheel();

__device__ __forceinline__ bool unknown_flow(float u, float v)      // the reference's _unknown_flow; NaN fails the comparison
{
    return !(fabsf(u) <= 1e9f) || !(fabsf(v) <= 1e9f);
}

__device__ __forceinline__ unsigned char level_of(double col)       // 255 * col truncated; a NaN or negative product stores 0
{
#pragma clang fp contract(off)
    const double x = 255.0 * col;
    return x >= 0.0 ? (unsigned char)(x < 255.0 ? (int)x : 255) : (unsigned char)0;
}

// One pixel of compute_color: the wheel's channels r, g, b into c[0..2].
__device__ __forceinline__ void wheel_pixel(float u, float v, float norm, bool ex, int original, const double *wheel, unsigned char c[3])
{
#pragma clang fp contract(off)
    if (ex) {
        c[0] = c[1] = c[2] = 0;
        return;
    }
    const float fx = u / norm, fy = v / norm;
    const float rad = sqrtf(fx * fx + fy * fy);
    const float a = atan2f(-fy, -fx) / 3.14159274f;
    const float fk = (a + 1.0f) / 2.0f * (float)(VZ_NCOLS - 1);
    int k0 = fk >= 0.0f ? (int)fminf(fk, (float)(VZ_NCOLS - 1)) : 0;          // fk lies in [0, 54]; the clamp is for a NaN normaliser
    const int k1 = k0 + 1 == VZ_NCOLS ? 0 : k0 + 1;
    const double f = original ? 0.0 : (double)fk - (double)k0;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const double col0 = wheel[3 * k0 + b], col1 = wheel[3 * k1 + b];
        double col = (1.0 - f) * col0 + f * col1;
        if (rad <= 1.0f) col = 1.0 - (double)rad * (1.0 - col);
        else if (rad > 1.0f) col = col * 0.75;
        c[b] = level_of(col);
    }
}

// The 12 bytes of a full group as three dwords, or the first n pixels byte by byte.
__device__ __forceinline__ void store_group(unsigned char *out, size_t p0, const unsigned char px[12], int n, int vec_out)
{
    if (n == 4 && vec_out) {
        unsigned *o = reinterpret_cast<unsigned *>(out + 3 * p0);
#pragma unroll
        for (int w = 0; w < 3; ++w)
            o[w] = (unsigned)px[4 * w] | ((unsigned)px[4 * w + 1] << 8) | ((unsigned)px[4 * w + 2] << 16) | ((unsigned)px[4 * w + 3] << 24);
    } else {
        for (int i = 0; i < 3 * n; ++i) out[3 * p0 + i] = px[i];
    }
}

// The 4 mask bytes of a group (0 without a mask).
__device__ __forceinline__ void load_mask(const unsigned char *mask, size_t p0, int n, int vec_in, unsigned char m[4])
{
    if (mask && vec_in) {
        const uchar4 q = *reinterpret_cast<const uchar4 *>(mask + p0);
        m[0] = q.x; m[1] = q.y; m[2] = q.z; m[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) m[i] = (mask && i < n) ? mask[p0 + i] : (unsigned char)0;
    }
}

__global__ __launch_bounds__(VZ_THREADS) void flow_color_kernel(const float *__restrict__ flow, const float *__restrict__ norm,
                                                                const unsigned char *__restrict__ mask, unsigned char *__restrict__ out,
                                                                size_t npix, unsigned HW, int original, int rgb, int vec_in, int vec_out)
{
    __shared__ double wheel[VZ_NCOLS * 3];
    for (int i = threadIdx.x; i < VZ_NCOLS * 3; i += VZ_THREADS) wheel[i] = g_wheel.c[i];
    __syncthreads();
    const size_t groups = (npix + 3) / 4;
    for (size_t g = (size_t)blockIdx.x * VZ_THREADS + threadIdx.x; g < groups; g += (size_t)gridDim.x * VZ_THREADS) {
        const size_t p0 = 4 * g;
        const int n = npix - p0 < 4 ? (int)(npix - p0) : 4;
        float u[4], v[4], nr[4];
        unsigned char m[4];
        if (vec_in) {                   // HW % 4 == 0: the group lies inside image b, 16-byte aligned in both planes
            const size_t b = p0 / HW, r = p0 - b * HW;
            const float4 a = *reinterpret_cast<const float4 *>(flow + b * 2 * HW + r);
            const float4 c = *reinterpret_cast<const float4 *>(flow + b * 2 * HW + HW + r);
            u[0] = a.x; u[1] = a.y; u[2] = a.z; u[3] = a.w;
            v[0] = c.x; v[1] = c.y; v[2] = c.z; v[3] = c.w;
            const float nb = norm[b];
            nr[0] = nr[1] = nr[2] = nr[3] = nb;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const size_t p = i < n ? p0 + i : p0, b = p / HW, r = p - b * HW;
                u[i] = flow[b * 2 * HW + r];
                v[i] = flow[b * 2 * HW + HW + r];
                nr[i] = norm[b];
            }
        }
        load_mask(mask, p0, n, vec_in, m);
        unsigned char px[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned char c[3];
            wheel_pixel(u[i], v[i], nr[i] == 0.0f ? 1.0f : nr[i], m[i] != 0 || unknown_flow(u[i], v[i]), original, wheel, c);
            px[3 * i] = rgb ? c[0] : c[2];
            px[3 * i + 1] = c[1];
            px[3 * i + 2] = rgb ? c[2] : c[0];
        }
        store_group(out, p0, px, n, vec_out);
    }
}

template <typename T>
__global__ __launch_bounds__(VZ_THREADS) void scalar_color_kernel(const T *__restrict__ field, const unsigned char *__restrict__ mask,
                                                                  const unsigned char *__restrict__ lut, unsigned char *__restrict__ out,
                                                                  size_t npix, double vmin, double scale, unsigned bad, int vec_in,
                                                                  int vec_out)
{
#pragma clang fp contract(off)
    __shared__ unsigned char tab[256 * 3];
    for (int i = threadIdx.x; i < 256 * 3; i += VZ_THREADS) tab[i] = lut[i];
    __syncthreads();
    const size_t groups = (npix + 3) / 4;
    for (size_t g = (size_t)blockIdx.x * VZ_THREADS + threadIdx.x; g < groups; g += (size_t)gridDim.x * VZ_THREADS) {
        const size_t p0 = 4 * g;
        const int n = npix - p0 < 4 ? (int)(npix - p0) : 4;
        T x[4];
        unsigned char m[4];
        if (vec_in) {                   // npix % 4 == 0 and a 32-byte aligned field
            if constexpr (sizeof(T) == 4) {
                const float4 a = *reinterpret_cast<const float4 *>(field + p0);
                x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
            } else {
                const double2 a = *reinterpret_cast<const double2 *>(field + p0), c = *reinterpret_cast<const double2 *>(field + p0 + 2);
                x[0] = a.x; x[1] = a.y; x[2] = c.x; x[3] = c.y;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = field[i < n ? p0 + i : p0];
        }
        load_mask(mask, p0, n, vec_in, m);
        unsigned char px[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double xd = (double)x[i];
            const bool ok = m[i] == 0 && fabs(xd) <= 1.7976931348623157e308;       // finite: NaN and inf fail
            const double t = floor((xd - vmin) * scale);
            const int idx = t >= 0.0 ? (t < 255.0 ? (int)t : 255) : 0;
            px[3 * i] = ok ? tab[3 * idx] : (unsigned char)(bad >> 16);
            px[3 * i + 1] = ok ? tab[3 * idx + 1] : (unsigned char)(bad >> 8);
            px[3 * i + 2] = ok ? tab[3 * idx + 2] : (unsigned char)bad;
        }
        store_group(out, p0, px, n, vec_out);
    }
}

// Largest value of a workgroup in thread 0.  V: float or double, values >= 0 and never NaN.
template <typename V>
__device__ __forceinline__ V block_max(V m, V *red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const V o = __shfl_down(m, off, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < VZ_THREADS / 64; ++w) m = red[w] > m ? red[w] : m;
    return m;
}

// maxrad[b] = max(maxrad[b], the largest known, unmasked radius of image b); the launcher zeroes maxrad first.  Values >= +0.0 order
// like their bit patterns, so the integer maximum is the floating-point one and no order of arrival changes it.
__global__ __launch_bounds__(VZ_THREADS) void flow_maxrad_kernel(const float *__restrict__ flow, const unsigned char *__restrict__ mask,
                                                                 float *__restrict__ maxrad, unsigned HW, int vec_in)
{
#pragma clang fp contract(off)
    __shared__ float red[VZ_THREADS / 64];
    const size_t b = blockIdx.y;
    const float *up = flow + b * 2 * HW, *vp = up + HW;
    const unsigned char *mk = mask ? mask + b * HW : nullptr;
    float best = 0.0f;
    const unsigned groups = (HW + 3) / 4;
    for (unsigned g = blockIdx.x * VZ_THREADS + threadIdx.x; g < groups; g += gridDim.x * VZ_THREADS) {
        const unsigned p0 = 4 * g;
        const int n = HW - p0 < 4 ? (int)(HW - p0) : 4;
        float u[4], v[4];
        unsigned char m[4];
        if (vec_in) {
            const float4 a = *reinterpret_cast<const float4 *>(up + p0), c = *reinterpret_cast<const float4 *>(vp + p0);
            u[0] = a.x; u[1] = a.y; u[2] = a.z; u[3] = a.w;
            v[0] = c.x; v[1] = c.y; v[2] = c.z; v[3] = c.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                u[i] = up[i < n ? p0 + i : p0];
                v[i] = vp[i < n ? p0 + i : p0];
            }
        }
        load_mask(mk, p0, n, vec_in, m);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float rad = sqrtf(u[i] * u[i] + v[i] * v[i]);
            if (i < n && m[i] == 0 && !unknown_flow(u[i], v[i]) && rad > best) best = rad;
        }
    }
    best = block_max(best, red);
    if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned *>(maxrad + b), __float_as_uint(best));
}

template <typename T>
__global__ __launch_bounds__(VZ_THREADS) void field_absmax_kernel(const T *__restrict__ field, const unsigned char *__restrict__ mask,
                                                                  double *__restrict__ absmax, unsigned HW)
{
    __shared__ double red[VZ_THREADS / 64];
    const size_t b = blockIdx.y;
    double best = 0.0;
    for (unsigned p = blockIdx.x * VZ_THREADS + threadIdx.x; p < HW; p += gridDim.x * VZ_THREADS) {
        const double a = fabs((double)field[b * HW + p]);
        if (a <= 1.7976931348623157e308 && !(mask && mask[b * HW + p] != 0) && a > best) best = a;
    }
    best = block_max(best, red);
    if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned long long *>(absmax + b), (unsigned long long)__double_as_longlong(best));
}

// One thread per cell: the known, unmasked vectors of the cell added in row-major order in fp64.
__global__ __launch_bounds__(VZ_THREADS) void flow_decimate_kernel(const float *__restrict__ flow, const unsigned char *__restrict__ mask,
                                                                   float *__restrict__ mean, int *__restrict__ count, size_t ncells,
                                                                   int H, int W, int ch, int cw, int cell)
{
#pragma clang fp contract(off)
    const size_t HW = (size_t)H * W, chw = (size_t)ch * cw;
    for (size_t i = (size_t)blockIdx.x * VZ_THREADS + threadIdx.x; i < ncells; i += (size_t)gridDim.x * VZ_THREADS) {
        const size_t b = i / chw, r = i - b * chw;
        const int cy = (int)(r / cw), cx = (int)(r - (size_t)cy * cw);
        const int y1 = min(H, (cy + 1) * cell), x1 = min(W, (cx + 1) * cell);
        const float *up = flow + b * 2 * HW, *vp = up + HW;
        const unsigned char *mk = mask ? mask + b * HW : nullptr;
        double su = 0.0, sv = 0.0;
        int n = 0;
        for (int y = cy * cell; y < y1; ++y)
            for (int x = cx * cell; x < x1; ++x) {
                const size_t at = (size_t)y * W + x;
                const float u = up[at], v = vp[at];
                if (unknown_flow(u, v) || (mk && mk[at] != 0)) continue;
                su = su + (double)u;
                sv = sv + (double)v;
                ++n;
            }
        mean[b * 2 * chw + r] = n ? (float)(su / (double)n) : 1e10f;
        mean[b * 2 * chw + chw + r] = n ? (float)(sv / (double)n) : 1e10f;
        count[i] = n;
    }
}

static unsigned viz_blocks(size_t items)
{
    const size_t g = (items + VZ_THREADS - 1) / VZ_THREADS;
    return (unsigned)(g > VZ_MAX_BLOCKS ? VZ_MAX_BLOCKS : (g ? g : 1));
}

static bool aligned_to(const void *p, size_t a) { return p == nullptr || ((size_t)p & (a - 1)) == 0; }

int launch_flow_maxrad(const float *flow, const unsigned char *mask, float *maxrad, int B, int H, int W, hipStream_t st)
{
    PIV_REQUIRE(flow && maxrad, "flow_maxrad: null pointer (flow and maxrad are required)");
    if (int rc = check_shape("flow_maxrad", B, H, W, "images")) return rc;
    const unsigned HW = (unsigned)H * (unsigned)W;
    const int vec = HW % 4 == 0 && aligned_to(flow, 16) && aligned_to(mask, 4);
    PIV_CHECK_HIP(hipMemsetAsync(maxrad, 0, (size_t)B * sizeof(float), st));
    const unsigned gx = viz_blocks((HW + 3) / 4);
    hipLaunchKernelGGL(flow_maxrad_kernel, dim3(gx > 256 ? 256 : gx, (unsigned)B), dim3(VZ_THREADS), 0, st, flow, mask, maxrad, HW, vec);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

int launch_flow_to_color(const float *flow, const float *norm, const unsigned char *mask, unsigned char *out, int B, int H, int W,
                         int wheel, int order, hipStream_t st)
{
    PIV_REQUIRE(flow && norm && out, "flow_to_color: null pointer (flow, norm and out are required)");
    if (int rc = check_shape("flow_to_color", B, H, W, "images")) return rc;
    PIV_REQUIRE(wheel == PIVLFN_WHEEL_INTERP || wheel == PIVLFN_WHEEL_ORIGINAL, "flow_to_color: wheel=%d must be 0 (interpolated) or 1 (original)",
                wheel);
    PIV_REQUIRE(order == PIVLFN_ORDER_RGB || order == PIVLFN_ORDER_BGR, "flow_to_color: order=%d must be 0 (rgb) or 1 (bgr)", order);
    const unsigned HW = (unsigned)H * (unsigned)W;
    const size_t npix = (size_t)B * HW;
    const int vec_in = HW % 4 == 0 && aligned_to(flow, 16) && aligned_to(mask, 4), vec_out = aligned_to(out, 4);
    hipLaunchKernelGGL(flow_color_kernel, dim3(viz_blocks((npix + 3) / 4)), dim3(VZ_THREADS), 0, st, flow, norm, mask, out, npix, HW,
                       wheel == PIVLFN_WHEEL_ORIGINAL, order == PIVLFN_ORDER_RGB, vec_in, vec_out);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

int launch_field_absmax(const void *field, int is_f64, const unsigned char *mask, double *absmax, int B, int H, int W, hipStream_t st)
{
    PIV_REQUIRE(field && absmax, "field_absmax: null pointer (field and absmax are required)");
    if (int rc = check_shape("field_absmax", B, H, W, "images")) return rc;
    PIV_REQUIRE(is_f64 == 0 || is_f64 == 1, "field_absmax: is_f64=%d must be 0 or 1", is_f64);
    const unsigned HW = (unsigned)H * (unsigned)W;
    PIV_CHECK_HIP(hipMemsetAsync(absmax, 0, (size_t)B * sizeof(double), st));
    const unsigned gx = viz_blocks(HW);
    const dim3 grid(gx > 256 ? 256 : gx, (unsigned)B);
    if (is_f64)
        hipLaunchKernelGGL(field_absmax_kernel<double>, grid, dim3(VZ_THREADS), 0, st, (const double *)field, mask, absmax, HW);
    else
        hipLaunchKernelGGL(field_absmax_kernel<float>, grid, dim3(VZ_THREADS), 0, st, (const float *)field, mask, absmax, HW);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

int launch_scalar_to_color(const void *field, int is_f64, const unsigned char *mask, const unsigned char *lut, unsigned char *out, int B,
                           int H, int W, double vmin, double vmax, int bad_rgb, hipStream_t st)
{
    PIV_REQUIRE(field && lut && out, "scalar_to_color: null pointer (field, lut and out are required)");
    if (int rc = check_shape("scalar_to_color", B, H, W, "images")) return rc;
    PIV_REQUIRE(is_f64 == 0 || is_f64 == 1, "scalar_to_color: is_f64=%d must be 0 or 1", is_f64);
    PIV_REQUIRE(std::isfinite(vmin) && std::isfinite(vmax), "scalar_to_color: vmin=%g vmax=%g must be finite", vmin, vmax);
    PIV_REQUIRE(vmax != vmin, "scalar_to_color: vmax == vmin = %g leaves no range to map", vmin);
    const double scale = 256.0 / (vmax - vmin);
    PIV_REQUIRE(std::isfinite(scale), "scalar_to_color: the range vmin=%g vmax=%g is too narrow (256 / (vmax - vmin) overflows)", vmin, vmax);
    PIV_REQUIRE(bad_rgb >= 0 && bad_rgb <= 0xFFFFFF, "scalar_to_color: bad_rgb=%d must be 0xRRGGBB", bad_rgb);
    const size_t npix = (size_t)B * H * W;
    const int vec_in = npix % 4 == 0 && aligned_to(field, 32) && aligned_to(mask, 4), vec_out = aligned_to(out, 4);
    const dim3 grid(viz_blocks((npix + 3) / 4));
    if (is_f64)
        hipLaunchKernelGGL(scalar_color_kernel<double>, grid, dim3(VZ_THREADS), 0, st, (const double *)field, mask, lut, out, npix, vmin,
                           scale, (unsigned)bad_rgb, vec_in, vec_out);
    else
        hipLaunchKernelGGL(scalar_color_kernel<float>, grid, dim3(VZ_THREADS), 0, st, (const float *)field, mask, lut, out, npix, vmin,
                           scale, (unsigned)bad_rgb, vec_in, vec_out);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

int launch_flow_decimate(const float *flow, const unsigned char *mask, float *mean, int *count, int B, int H, int W, int cell,
                         hipStream_t st)
{
    PIV_REQUIRE(flow && mean && count, "flow_decimate: null pointer (flow, mean and count are required)");
    if (int rc = check_shape("flow_decimate", B, H, W, "images")) return rc;
    PIV_REQUIRE(cell > 0 && cell <= 32768, "flow_decimate: cell=%d must be 1..32768", cell);
    const int ch = cdiv(H, cell), cw = cdiv(W, cell);
    const size_t ncells = (size_t)B * ch * cw;
    hipLaunchKernelGGL(flow_decimate_kernel, dim3(viz_blocks(ncells)), dim3(VZ_THREADS), 0, st, flow, mask, mean, count, ncells, H, W, ch,
                       cw, cell);
    PIV_CHECK_HIP(hipGetLastError());
    return PIVLFN_OK;
}

}  // namespace pivlfn
