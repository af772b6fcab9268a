// extern "C" surface of libpivlfn.so (declared in include/pivlfn.h).
#include <atomic>
#include <mutex>
#include <vector>
#include "net.h"

namespace pivlfn {

static thread_local char g_err[512] = "";
#ifdef PIVLFN_TOOLS
int g_knob[16] = {0};
#endif

// hipFuncSetAttribute is per device: the opt-in is remembered per (call site, device).  Fast path: one relaxed atomic read.
int ensure_dyn_lds(LdsAttr &slot, const void *fn, int bytes)
{
    static std::mutex mu;
    int dev = 0;
    PIV_CHECK_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) { set_error("device ordinal %d out of range", dev); return PIVLFN_ERR_ARG; }
    if (__atomic_load_n(&slot.bytes[dev], __ATOMIC_ACQUIRE) >= bytes) return PIVLFN_OK;
    std::lock_guard<std::mutex> lock(mu);
    if (slot.bytes[dev] >= bytes) return PIVLFN_OK;
    PIV_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    __atomic_store_n(&slot.bytes[dev], bytes, __ATOMIC_RELEASE);
    return PIVLFN_OK;
}

int device_cus()
{
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    int n = __atomic_load_n(&cus[dev], __ATOMIC_ACQUIRE);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        __atomic_store_n(&cus[dev], n, __ATOMIC_RELEASE);
    }
    return n;
}

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

}  // namespace pivlfn

using namespace pivlfn;

extern "C" {

const char *pivlfn_last_error(void) { return g_err; }
int pivlfn_abi_version(void) { return 3; }

#ifdef PIVLFN_TOOLS
int pivlfn_tune(int knob, int value)
{
    if (knob < 0 || knob >= 16) { set_error("tune: knob %d out of range", knob); return PIVLFN_ERR_ARG; }
    g_knob[knob] = value;
    return PIVLFN_OK;
}
#endif

int pivlfn_corr_fwd(const float *first, const float *second, float *out, int B, int C, int H, int W, int stride, void *stream)
{
    return launch_warp_corr(first, second, nullptr, 0.f, out, B, C, H, W, stride, 0, false, (hipStream_t)stream);
}

int pivlfn_corr_bwd(const float *first, const float *second, const float *grad_out, float *grad_first, float *grad_second,
                    int B, int C, int H, int W, int stride, void *stream)
{
    return launch_corr_bwd(first, second, grad_out, grad_first, grad_second, B, C, H, W, stride, (hipStream_t)stream);
}

int pivlfn_corr_bwd_channel_group(int B, int C, int H, int W, int stride)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || stride < 1 || stride > 4) { set_error("corr_bwd_channel_group: bad shape or stride"); return 0; }
    return corr_bwd_cgroup(B, C, H, W, stride);
}

int pivlfn_conv2d_nhwc_plan(int cout, int cin, int kh, int kw, int B, int H, int W, int stride, int pad_y, int pad_x,
                            int has_res, int leaky, int x_stride, int y_stride, int plan[5])
{
    PIV_REQUIRE(plan && cout > 0 && cin > 0 && kh > 0 && kw > 0, "conv2d_plan: bad arguments");
    static const float some_residual = 0.f;      // never read: the choice only asks whether there is one
    ConvParams p;
    ConvPlan pl;
    bool per_image;
    if (int rc = conv_forward_choose(conv_shape(cout, cin, kh, kw), x_stride, y_stride, has_res ? &some_residual : nullptr, B, H, W, stride,
                                     pad_y, pad_x, leaky, p, pl, per_image))
        return rc;
    plan[0] = pl.family; plan[1] = pl.rows; plan[2] = pl.chans; plan[3] = pl.staging; plan[4] = pl.ksplit;
    return PIVLFN_OK;
}

int pivlfn_conv2d_nhwc_kernel_plan(int kernel, int cout, int cin, int kh, int kw, int B, int H, int W, int stride, int pad_y, int pad_x,
                                   int terms, int x_is_f16, int x_stride, int y_stride, int cus, int plan[10])
{
    PIV_REQUIRE(plan && cout > 0 && cin > 0 && kh > 0 && kw > 0, "conv2d_kernel_plan: bad arguments");
    ConvKernelPlan pl;
    if (int rc = conv_kernel_plan(kernel, cout, cin, kh, kw, B, H, W, stride, pad_y, pad_x, terms, x_is_f16, x_stride, y_stride, cus, pl))
        return rc;
    plan[0] = pl.kernel; plan[1] = pl.terms; plan[2] = pl.rows; plan[3] = pl.chans; plan[4] = pl.staging; plan[5] = pl.occ;
    plan[6] = pl.ksplit; plan[7] = pl.fold; plan[8] = pl.per_image; plan[9] = pl.blocks;
    return PIVLFN_OK;
}

int pivlfn_conv_head_nhwc_plan(int k, int B, int H, int W, int plan[4])
{
    PIV_REQUIRE(plan, "conv_head_plan: bad arguments");
    HeadPlan pl;
    if (int rc = choose_conv_head(k, B, H, W, 0, pl)) return rc;
    plan[0] = pl.family; plan[1] = pl.rows; plan[2] = pl.cols; plan[3] = pl.blocks;
    return PIVLFN_OK;
}

int pivlfn_backwarp(const float *in, const float *flow, float *out, int B, int C, int H, int W, void *stream)
{
    return launch_backwarp_nchw(in, flow, out, B, C, H, W, (hipStream_t)stream);
}

int pivlfn_warp_corr_fwd(const float *first, const float *second, const float *flow, float flow_scale, float *out,
                         int B, int C, int H, int W, int stride, int leaky, void *stream)
{
    return launch_warp_corr(first, second, flow, flow_scale, out, B, C, H, W, stride, leaky, false, (hipStream_t)stream);
}

int pivlfn_warp_corr_nhwc(const float *first, const float *second, const float *flow, float flow_scale, float *out,
                          int B, int C, int H, int W, int stride, int leaky, void *stream)
{
    return launch_warp_corr(first, second, flow, flow_scale, out, B, C, H, W, stride, leaky, true, (hipStream_t)stream);
}

int pivlfn_resize_bilinear(const float *in, float *out, int B, int C, int H, int W, int Ho, int Wo, const float *mul,
                           void *stream)
{
    return launch_resize_nchw(in, out, B, C, H, W, Ho, Wo, mul ? mul[0] : 1.f, mul ? mul[1] : 1.f, mul ? 1 : 0,
                              (hipStream_t)stream);
}

int pivlfn_stereo_2d3c(const float *flow, float *out, int B, int h, int w, int H, int W, const float *mul,
                       const float *coeff, const float *scale, const double *tangents, void *stream)
{
    return launch_stereo_2d3c(flow, out, B, h, w, H, W, mul, coeff, scale, tangents, (hipStream_t)stream);
}

int pivlfn_flow_fields(const float *flow, void *out, int B, int H, int W, double calib, int kind, int out_f64, void *stream)
{
    return launch_flow_fields(flow, out, B, H, W, calib, kind, out_f64, (hipStream_t)stream);
}

int pivlfn_flow_stats_accumulate(const float *flow, double *acc, int B, int H, int W, double calib, void *stream)
{
    return launch_flow_stats(flow, acc, B, H, W, calib, (hipStream_t)stream);
}

int pivlfn_flow_validate(const float *flow, float *out, unsigned char *flag, float *resid, int B, int H, int W, int radius, int spacing,
                         float eps, float thresh, int mode, void *stream)
{
    return launch_flow_validate(flow, out, flag, resid, B, H, W, radius, spacing, eps, thresh, mode, (hipStream_t)stream);
}

int pivlfn_flow_stats_accumulate_masked(const float *flow, const unsigned char *flag, double *acc, double *cnt, int B, int H, int W,
                                        double calib, void *stream)
{
    return launch_flow_stats_masked(flow, flag, acc, cnt, B, H, W, calib, (hipStream_t)stream);
}

int pivlfn_frames_background_min(const unsigned char *frames, unsigned char *bg, int n, int H, int W, void *stream)
{
    return launch_frames_background_min(frames, bg, n, H, W, (hipStream_t)stream);
}

int pivlfn_frames_preprocess(const unsigned char *frames, const unsigned char *bg, float *out, int n, int H, int W, int k, int floor,
                             void *stream)
{
    return launch_frames_preprocess(frames, bg, out, n, H, W, k, floor, (hipStream_t)stream);
}

size_t pivlfn_flow_errors_workspace_bytes(int B, int H, int W) { return flow_errors_workspace_bytes(B, H, W); }

int pivlfn_flow_errors(const float *flow, const float *truth, const unsigned char *mask, int B, int H, int W, int k, double div_flow,
                       double *sums, float *err_map, void *workspace, size_t workspace_bytes, void *stream)
{
    return launch_flow_errors(flow, truth, mask, B, H, W, k, div_flow, sums, err_map, workspace, workspace_bytes, (hipStream_t)stream);
}

int pivlfn_level_errors(const float *levels, int lowest_level, const float *truth, const unsigned char *mask, int B, int H, int W,
                        double div_flow, double *sums, void *workspace, size_t workspace_bytes, void *stream)
{
    return launch_level_errors(levels, lowest_level, truth, mask, B, H, W, div_flow, sums, workspace, workspace_bytes,
                               (hipStream_t)stream);
}

int pivlfn_error_stats_accumulate(const float *flow, const float *truth, const unsigned char *mask, double *acc, int B, int H, int W,
                                  void *stream)
{
    return launch_error_stats(flow, truth, mask, acc, B, H, W, (hipStream_t)stream);
}

size_t pivlfn_match_quality_workspace_bytes(int B, int H, int W, int radius) { return match_quality_workspace_bytes(B, H, W, radius); }

int pivlfn_match_quality(const float *img1, const float *img2, int C, const float *flow, const unsigned char *mask, float *quality,
                         unsigned char *flag, int B, int H, int W, int radius, int min_count, double floor, void *workspace,
                         size_t workspace_bytes, void *stream)
{
    return launch_match_quality(img1, img2, C, flow, mask, quality, flag, B, H, W, radius, min_count, floor, workspace, workspace_bytes,
                                (hipStream_t)stream);
}

size_t pivlfn_flow_uncertainty_workspace_bytes(int B, int H, int W, int radius, int lag)
{
    return flow_uncertainty_workspace_bytes(B, H, W, radius, lag);
}

int pivlfn_flow_uncertainty(const float *img1, const float *img2, int C, const float *flow, const unsigned char *mask, float *unc,
                            unsigned char *flag, int B, int H, int W, int radius, int lag, int min_count, double floor, void *workspace,
                            size_t workspace_bytes, void *stream)
{
    return launch_flow_uncertainty(img1, img2, C, flow, mask, unc, flag, B, H, W, radius, lag, min_count, floor, workspace,
                                   workspace_bytes, (hipStream_t)stream);
}

int pivlfn_uncertainty_accumulate(const float *unc, const unsigned char *flag, double *sums, int B, int H, int W, void *stream)
{
    return launch_uncertainty_accumulate(unc, flag, sums, B, H, W, (hipStream_t)stream);
}

size_t pivlfn_vortex_gamma_workspace_bytes(int B, int H, int W, int radius, int spacing)
{
    return vortex_gamma_workspace_bytes(B, H, W, radius, spacing);
}

int pivlfn_vortex_gamma(const float *flow, const unsigned char *mask, float *gamma, unsigned char *flag, int B, int H, int W, int radius,
                        int spacing, int min_count, void *workspace, size_t workspace_bytes, void *stream)
{
    return launch_vortex_gamma(flow, mask, gamma, flag, B, H, W, radius, spacing, min_count, workspace, workspace_bytes,
                               (hipStream_t)stream);
}

int pivlfn_flowmap_advect(const float *flows, const unsigned char *mask, int B, int H, int W, double *pos, unsigned char *flag, int N,
                          int backward, int iters, double *trace, void *stream)
{
    return launch_flowmap_advect(flows, mask, B, H, W, pos, flag, N, backward, iters, trace, (hipStream_t)stream);
}

int pivlfn_flowmap_seed(double *pos, unsigned char *flag, int h, int w, int spacing, void *stream)
{
    return launch_flowmap_seed(pos, flag, h, w, spacing, (hipStream_t)stream);
}

int pivlfn_flowmap_ftle(const double *pos, const unsigned char *flag, int h, int w, int spacing, double *stretch, unsigned char *oflag,
                        void *stream)
{
    return launch_flowmap_ftle(pos, flag, h, w, spacing, stretch, oflag, (hipStream_t)stream);
}

int pivlfn_particles_displace(const double *pos, const float *flow, const unsigned char *mask, int H, int W, int N, int method,
                              unsigned char *flag, double *out, void *stream)
{
    return launch_particles_displace(pos, flow, mask, H, W, N, method, flag, out, (hipStream_t)stream);
}

size_t pivlfn_particles_render_workspace_bytes(int B, int N, int H, int W, int radius)
{
    return particles_render_workspace_bytes(B, N, H, W, radius);
}

int pivlfn_particles_render(const double *pos, const float *diam, const float *amp, const unsigned char *flag, int B, int N, int H, int W,
                            int radius, float *intensity, unsigned char *image, void *workspace, size_t workspace_bytes, void *stream)
{
    return launch_particles_render(pos, diam, amp, flag, B, N, H, W, radius, intensity, image, workspace, workspace_bytes,
                                   (hipStream_t)stream);
}

int pivlfn_twopoint_accumulate(const float *flow, const unsigned char *mask, const double *mean, double *acc, int B, int H, int W,
                               int max_sep, int step, void *stream)
{
    return launch_twopoint_accumulate(flow, mask, mean, acc, B, H, W, max_sep, step, (hipStream_t)stream);
}

int pivlfn_flow_moments_accumulate(const float *flow, const unsigned char *mask, const double *mean, const double *thr, double *acc,
                                   int B, int H, int W, void *stream)
{
    return launch_flow_moments(flow, mask, mean, thr, acc, B, H, W, (hipStream_t)stream);
}

int pivlfn_flow_hist_accumulate(const float *flow, const unsigned char *mask, const double *mean, const double *scale,
                                unsigned long long *hist, int B, int H, int W, double lo, double hi, int nbins, int jbins, int fbins,
                                void *stream)
{
    return launch_flow_hist(flow, mask, mean, scale, hist, B, H, W, lo, hi, nbins, jbins, fbins, (hipStream_t)stream);
}

int pivlfn_flow_hist_plan(int B, int H, int W, int nbins, int jbins, int fbins, int plan[5])
{
    PIV_REQUIRE(plan, "flow_hist_plan: bad arguments");
    HistPlan pl;
    if (int rc = choose_flow_hist(B, H, W, nbins, jbins, fbins, pl)) return rc;
    plan[0] = pl.groups; plan[1] = pl.lds_words; plan[2] = pl.joint_in_lds; plan[3] = (int)pl.words; plan[4] = pl.moment_blocks;
    return PIVLFN_OK;
}

int pivlfn_spectrum_accumulate(const float *X, int L, int first, long N, long ldx, const double *basis, int K, double *acc, int *count,
                               void *stream)
{
    return launch_spectrum_accumulate(X, L, first, N, ldx, basis, K, acc, count, (hipStream_t)stream);
}

int pivlfn_pressure_gradient(const float *flows, int B, int h, int w, double s, double nu, double *g, unsigned char *valid, void *stream)
{
    return launch_pressure_gradient(flows, B, h, w, s, nu, g, valid, (hipStream_t)stream);
}

size_t pivlfn_pressure_workspace_bytes(int F, int h, int w) { return pressure_workspace_bytes(F, h, w); }

size_t pivlfn_pressure_workspace_offset(int F, int h, int w, int what) { return pressure_workspace_offset(F, h, w, what); }

int pivlfn_pressure_setup(const double *g, const unsigned char *valid, int F, int h, int w, double s, void *workspace,
                          size_t workspace_bytes, void *stream)
{
    return launch_pressure_setup(g, valid, F, h, w, s, workspace, workspace_bytes, (hipStream_t)stream);
}

int pivlfn_pressure_cg(void *workspace, size_t workspace_bytes, int F, int h, int w, double tol, int iters, void *stream)
{
    return launch_pressure_cg(workspace, workspace_bytes, F, h, w, tol, iters, (hipStream_t)stream);
}

int pivlfn_pressure_read(const void *workspace, size_t workspace_bytes, int F, int h, int w, double *p, unsigned char *flag,
                         double *status, void *stream)
{
    return launch_pressure_read(workspace, workspace_bytes, F, h, w, p, flag, status, (hipStream_t)stream);
}

size_t pivlfn_dct2_workspace_bytes(int P, int H, int W) { return dct2_workspace_bytes(P, H, W); }

int pivlfn_dct2(const double *x, double *out, int P, int H, int W, int inverse, void *workspace, size_t workspace_bytes, void *stream)
{
    return launch_dct2(x, out, P, H, W, inverse, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t pivlfn_smooth_workspace_bytes(int F, int H, int W) { return smooth_workspace_bytes(F, H, W); }

int pivlfn_smooth_setup(const float *flows, const float *weights, const unsigned char *mask, int F, int H, int W, double s,
                        void *workspace, size_t workspace_bytes, void *stream)
{
    return launch_smooth_setup(flows, weights, mask, F, H, W, s, workspace, workspace_bytes, (hipStream_t)stream);
}

int pivlfn_smooth_pcg(void *workspace, size_t workspace_bytes, int F, int H, int W, double s, double tol, int iters, void *stream)
{
    return launch_smooth_pcg(workspace, workspace_bytes, F, H, W, s, tol, iters, (hipStream_t)stream);
}

int pivlfn_smooth_read(const void *workspace, size_t workspace_bytes, int F, int H, int W, double *z, float *z32, unsigned char *filled,
                       double *status, void *stream)
{
    return launch_smooth_read(workspace, workspace_bytes, F, H, W, z, z32, filled, status, (hipStream_t)stream);
}

int pivlfn_flow_maxrad(const float *flow, const unsigned char *mask, float *maxrad, int B, int H, int W, void *stream)
{
    return launch_flow_maxrad(flow, mask, maxrad, B, H, W, (hipStream_t)stream);
}

int pivlfn_flow_to_color(const float *flow, const float *norm, const unsigned char *mask, unsigned char *out, int B, int H, int W,
                         int wheel, int order, void *stream)
{
    return launch_flow_to_color(flow, norm, mask, out, B, H, W, wheel, order, (hipStream_t)stream);
}

int pivlfn_field_absmax(const void *field, int is_f64, const unsigned char *mask, double *absmax, int B, int H, int W, void *stream)
{
    return launch_field_absmax(field, is_f64, mask, absmax, B, H, W, (hipStream_t)stream);
}

int pivlfn_scalar_to_color(const void *field, int is_f64, const unsigned char *mask, const unsigned char *lut, unsigned char *out, int B,
                           int H, int W, double vmin, double vmax, int bad_rgb, void *stream)
{
    return launch_scalar_to_color(field, is_f64, mask, lut, out, B, H, W, vmin, vmax, bad_rgb, (hipStream_t)stream);
}

int pivlfn_flow_decimate(const float *flow, const unsigned char *mask, float *mean, int *count, int B, int H, int W, int cell,
                         void *stream)
{
    return launch_flow_decimate(flow, mask, mean, count, B, H, W, cell, (hipStream_t)stream);
}

size_t pivlfn_snapshot_gram_workspace_bytes(int n, long P) { return snapshot_gram_workspace_bytes(n, P); }

int pivlfn_snapshot_gram(const float *X, int n, long P, long ldx, double *G, void *ws, size_t ws_bytes, void *stream)
{
    return launch_snapshot_gram(X, n, P, ldx, G, ws, ws_bytes, (hipStream_t)stream);
}

int pivlfn_snapshot_project(const float *X, int n, long P, long ldx, const double *Wt, int K, double *out, void *stream)
{
    return launch_snapshot_project(X, n, P, ldx, Wt, K, out, (hipStream_t)stream);
}

size_t pivlfn_template_match_workspace_bytes(int th, int tw) { return template_match_workspace_bytes(th, tw); }

int pivlfn_template_match(const unsigned char *images, const unsigned char *templ, float *r, int B, int H, int W, int th, int tw,
                          void *workspace, size_t workspace_bytes, void *stream)
{
    return launch_template_match(images, templ, r, B, H, W, th, tw, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t pivlfn_target_points_workspace_bytes(int B, int H, int W) { return target_points_workspace_bytes(B, H, W); }

int pivlfn_target_points(const float *r, int B, int H, int W, float threshold, int cap, int *labels, int *count, long long *rec,
                         void *workspace, size_t workspace_bytes, void *stream)
{
    return launch_target_points(r, B, H, W, threshold, cap, labels, count, rec, workspace, workspace_bytes, (hipStream_t)stream);
}

int pivlfn_dewarp_frames(const void *frames, void *out, int is_f32, int B, int H, int W, const double *A, double x0, double y0,
                         int mode, double fill, void *stream)
{
    return launch_dewarp_frames(frames, out, is_f32, B, H, W, A, x0, y0, mode, fill, (hipStream_t)stream);
}

int pivlfn_ensemble_corr(const unsigned char *a, const unsigned char *b, const int *offset, long long *sums, long long *sums_a,
                         int B, int H, int W, int window, int step, int search, void *stream)
{
    return launch_ensemble_corr(a, b, offset, sums, sums_a, B, H, W, window, step, search, (hipStream_t)stream);
}

int pivlfn_create(const pivlfn_tensor *tensors, int n_tensors, float starting_scale, int lowest_level,
                  const float rgb_mean[6], pivlfn_net **out)
{
    return net_create(tensors, n_tensors, starting_scale, lowest_level, rgb_mean, out);
}

int pivlfn_destroy(pivlfn_net *net) { return net_destroy(net); }

size_t pivlfn_workspace_bytes(const pivlfn_net *net, int B, int H, int W)
{
    if (!net || B <= 0 || H <= 0 || W <= 0) return 0;
    return net_workspace_bytes(net, B, H, W);
}

size_t pivlfn_levels_floats(const pivlfn_net *net, int B, int H, int W)
{
    if (!net || B <= 0 || H <= 0 || W <= 0) return 0;
    return net_levels_floats(net, B, H, W);
}

int pivlfn_forward(pivlfn_net *net, const float *img1, const float *img2, float *flow, float *levels, int B, int H, int W,
                   void *workspace, size_t workspace_bytes, void *stream)
{
    return net_forward(net, img1, img2, flow, levels, B, H, W, workspace, workspace_bytes, (hipStream_t)stream);
}

int pivlfn_conv_create(const float *weight, const float *bias, int cout, int cin, int kh, int kw, pivlfn_conv **out)
{
    return conv_create(weight, bias, cout, cin, kh, kw, out);
}

int pivlfn_conv_destroy(pivlfn_conv *conv) { return conv_destroy(conv); }

int pivlfn_conv2d_nhwc(const pivlfn_conv *conv, const float *x, int x_stride, float *y, int y_stride, const float *res,
                       int res_stride, int B, int H, int W, int stride, int pad_y, int pad_x, int leaky, void *stream)
{
    return conv_forward(conv, x, x_stride, y, y_stride, res, res_stride, B, H, W, stride, pad_y, pad_x, leaky, (hipStream_t)stream);
}

int pivlfn_conv2d_nhwc_f16(const pivlfn_conv *conv, const void *x, int x_stride, int x_is_f16, void *y, int y_stride,
                           int y_is_f16, int B, int H, int W, int stride, int pad_y, int pad_x, int leaky, void *stream)
{
    return conv_forward_h(conv, x, x_stride, x_is_f16, y, y_stride, y_is_f16, B, H, W, stride, pad_y, pad_x, leaky, (hipStream_t)stream);
}

int pivlfn_conv2d_nhwc_split(const pivlfn_conv *conv, const float *x, int x_stride, float *y, int y_stride,
                             int B, int H, int W, int stride, int pad_y, int pad_x, int leaky, int terms, void *stream)
{
    return conv_forward_x(conv, x, x_stride, y, y_stride, B, H, W, stride, pad_y, pad_x, leaky, terms, (hipStream_t)stream);
}

int pivlfn_conv2d_nhwc_wino(const pivlfn_conv *conv, const float *x, int x_stride, float *y, int y_stride,
                            int B, int H, int W, int leaky, void *stream)
{
    return conv_forward_w(conv, x, x_stride, y, y_stride, B, H, W, leaky, (hipStream_t)stream, 2);
}

int pivlfn_conv2d_nhwc_wino_b3(const pivlfn_conv *conv, const float *x, int x_stride, float *y, int y_stride,
                               int B, int H, int W, int leaky, int terms, void *stream)
{
    return conv_forward_wb(conv, x, x_stride, y, y_stride, B, H, W, leaky, terms, (hipStream_t)stream);
}

int pivlfn_conv2d_nhwc_dist_b3(const pivlfn_conv *conv, const float *x, int x_stride, float *y, int y_stride,
                               int B, int H, int W, int terms, void *stream)
{
    return conv_forward_dist_b3(conv, x, x_stride, y, y_stride, B, H, W, terms, (hipStream_t)stream);
}

int pivlfn_conv2d_nhwc_dist_b3_plan(int cout, int cin, int kh, int kw, int B, int H, int W, int terms, int x_stride, int y_stride, int plan[4])
{
    return conv_dist_b3_plan(cout, cin, kh, kw, B, H, W, terms, x_stride, y_stride, plan);
}

#ifdef PIVLFN_TOOLS
int pivlfn_conv2d_nhwc_wino4(const pivlfn_conv *conv, const float *x, int x_stride, float *y, int y_stride,
                             int B, int H, int W, int leaky, void *stream)
{
    return conv_forward_w(conv, x, x_stride, y, y_stride, B, H, W, leaky, (hipStream_t)stream, 4);
}
#endif

int pivlfn_conv_create_cat(const float *weight, const float *bias, int cout, int nsrc, const int *channels, int kh, int kw, pivlfn_conv **out)
{
    return conv_create_cat(weight, bias, cout, nsrc, channels, kh, kw, out);
}

int pivlfn_conv2d_nhwc_cat(const pivlfn_conv *conv, int nsrc, const float *const *x, const int *x_stride, float *y, int y_stride,
                           int B, int H, int W, int leaky, void *stream)
{
    return conv_forward_cat(conv, nsrc, x, x_stride, y, y_stride, B, H, W, leaky, (hipStream_t)stream);
}

int pivlfn_set_precision(pivlfn_net *net, int precision) { return net_set_precision(net, precision); }

int pivlfn_conv_head_nhwc(const pivlfn_conv *conv, const float *x, const float *res4, float *out4, int B, int H, int W, void *stream)
{
    return conv_head_forward(conv, x, res4, out4, B, H, W, (hipStream_t)stream);
}

int pivlfn_warp_corr_nhwc_timed(const float *first, const float *second, const float *flow, float flow_scale, float *out,
                                int B, int C, int H, int W, int stride, int leaky, int launches, double *us_dispatch, void *stream)
{
    PIV_REQUIRE(launches >= 1 && launches <= 256 && us_dispatch, "warp_corr_nhwc_timed: launches=%d must be 1..256, us_dispatch non-null", launches);
    hipStream_t st = (hipStream_t)stream;
    std::vector<hipEvent_t> ev(2 * (size_t)launches, nullptr);
    int rc = PIVLFN_OK;
    for (auto &e : ev)
        if (hipEventCreate(&e) != hipSuccess) { set_error("hipEventCreate failed"); rc = PIVLFN_ERR_HIP; break; }
    for (int i = 0; rc == PIVLFN_OK && i < launches; ++i) {      // back to back: every dispatch carries its own start / stop events
        warp_corr_time_next(ev[2 * i], ev[2 * i + 1]);
        rc = launch_warp_corr(first, second, flow, flow_scale, out, B, C, H, W, stride, leaky, true, st);
    }
    warp_corr_time_next(nullptr, nullptr);
    double total = 0.0;
    if (rc == PIVLFN_OK && hipStreamSynchronize(st) != hipSuccess) { set_error("hipStreamSynchronize failed"); rc = PIVLFN_ERR_HIP; }
    for (int i = 0; rc == PIVLFN_OK && i < launches; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]) != hipSuccess) { set_error("hipEventElapsedTime failed"); rc = PIVLFN_ERR_HIP; break; }
        total += ms;
    }
    for (auto &e : ev) if (e) (void)hipEventDestroy(e);
    if (rc == PIVLFN_OK) *us_dispatch = total * 1e3 / launches;
    return rc;
}

// ---- per-layer checks of the level-pipeline ops that run only inside pivlfn_forward (include/pivlfn.h) -------------------------
int pivlfn_upconv_nhwc(const float *in, const float *w16, float *out, int B, int H, int W, int quads, int stride_in, int stride_out,
                       void *stream)
{
    return upconv_forward(in, w16, out, B, H, W, quads, stride_in, stride_out, (hipStream_t)stream);
}

int pivlfn_backwarp_nhwc(const float *in, const float *flow4, float scale, float *out, int B, int H, int W, int C, void *stream)
{
    PIV_REQUIRE(in && flow4 && out, "backwarp_nhwc: null argument");
    PIV_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "backwarp_nhwc: B=%d H=%d W=%d C=%d must be positive", B, H, W, C);
    return launch_backwarp_nhwc(in, flow4, scale, out, B, H, W, C, (hipStream_t)stream);
}

int pivlfn_reg_prep(const float *img1_4, const float *img2_4, const float *flow4, float scale, float *misc4, float *mean_out,
                    float *partial_ws, int B, int H, int W, int fused, void *stream)
{
    PIV_REQUIRE(img1_4 && img2_4 && flow4 && misc4 && mean_out && partial_ws, "reg_prep: null argument");
    PIV_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "reg_prep: B=%d (1..65535) H=%d W=%d", B, H, W);
    PIV_REQUIRE((long)H * W < (1L << 31) - 65536, "reg_prep: H=%d x W=%d pixels exceed the 32-bit index range", H, W);
    PIV_REQUIRE(fused == 0 || fused == 1, "reg_prep: fused=%d (0 or 1)", fused);
    const hipStream_t st = (hipStream_t)stream;
    if (fused) {      // pivlfn_forward's path: partial sums only, every reg_prep workgroup finishes the mean itself
        if (int rc = launch_flow_mean(flow4, partial_ws, nullptr, B, H * W, st)) return rc;
        return launch_reg_prep(img1_4, img2_4, flow4, mean_out, partial_ws, scale, misc4, B, H, W, st);
    }
    if (int rc = launch_flow_mean(flow4, partial_ws, mean_out, B, H * W, st)) return rc;
    return launch_reg_prep(img1_4, img2_4, flow4, mean_out, nullptr, scale, misc4, B, H, W, st);
}

int pivlfn_reg_tail(const float *dist, int dstride, const float *flow4, const float *wx, const float *wy, float bx, float by, int k,
                    float *out4, float *out_nchw, float out_scale, int B, int H, int W, void *stream)
{
    PIV_REQUIRE(dist && flow4 && wx && wy && (out4 || out_nchw), "reg_tail: null argument (dist, flow4, wx, wy and one output needed)");
    PIV_REQUIRE(k == 3 || k == 5 || k == 7, "reg_tail: k=%d (3, 5 or 7)", k);
    PIV_REQUIRE(B > 0 && H > 0 && W > 0 && dstride >= k * k, "reg_tail: B=%d H=%d W=%d dstride=%d (>= %d)", B, H, W, dstride, k * k);
    PIV_REQUIRE((long)cdiv(W, 16) * cdiv(H, 16) * B < (1L << 31), "reg_tail: %d images of %d x %d exceed the grid range", B, H, W);
    return launch_reg_tail(dist, dstride, flow4, wx, wy, bx, by, k, out4, out_nchw, out_scale, B, H, W, (hipStream_t)stream);
}

int pivlfn_prep_pyramid(const float *img1, const float *img2, const float *mean6, float *out_levels, int B, int H, int W, int levels,
                        void *stream)
{
    PIV_REQUIRE(img1 && img2 && mean6 && out_levels, "prep_pyramid: null argument");
    PIV_REQUIRE(levels >= 1 && levels <= 6, "prep_pyramid: levels=%d (1..6)", levels);
    PIV_REQUIRE(B > 0 && (H >> (levels - 1)) > 0 && (W >> (levels - 1)) > 0,
                "prep_pyramid: B=%d H=%d W=%d leave no pixel at level %d", B, H, W, levels);
    PIV_REQUIRE((long)H * W < (1L << 31), "prep_pyramid: H=%d x W=%d pixels exceed the 32-bit index range", H, W);
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = launch_prep_images(img1, img2, out_levels, B, H, W, mean6, st)) return rc;
    float *prev = out_levels;
    for (int L = 2; L <= levels; ++L) {
        const int h0 = H >> (L - 2), w0 = W >> (L - 2);
        float *next = prev + (size_t)2 * B * h0 * w0 * 4;
        if (int rc = launch_resize_nhwc4(prev, next, 2 * B, h0, w0, H >> (L - 1), W >> (L - 1), st)) return rc;
        prev = next;
    }
    return PIVLFN_OK;
}

int pivlfn_conv1_fused_nhwc(const float *w1, const float *b1, const float *w_ext, const float *b_ext, const float *w_feat,
                            const float *b_feat, const float *x, float *out, float *out_ext, float *out_feat, int N, int H, int W,
                            int B_feat, int *fused, void *stream)
{
    return conv1_fused_forward(w1, b1, w_ext, b_ext, w_feat, b_feat, x, out, out_ext, out_feat, N, H, W, B_feat, fused,
                               (hipStream_t)stream);
}

int pivlfn_profile_enable(pivlfn_net *net, int level) { return net_profile_enable(net, level); }

int pivlfn_profile_read(pivlfn_net *net, double *ms_total, double *ms_empty_pairs, long *launches, int reset)
{
    return net_profile_read(net, ms_total, ms_empty_pairs, launches, reset);
}

}  // extern "C"
