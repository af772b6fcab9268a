// Weight repacking and the network object behind pivlfn_create: every layer of the state dict in the fragment orders of the gfx950
// kernels (pack_conv: one ConvW with the packing of each kernel family that covers the layer), uploaded once.
#include <algorithm>
#include <map>
#include <string>
#include <vector>
#include "net.h"

namespace pivlfn {

typedef std::map<std::string, const pivlfn_tensor *> TMap;

static const pivlfn_tensor *find(const TMap &m, const std::string &name, int d0, int d1, int d2, int d3, int ndim)
{
    auto it = m.find(name);
    if (it == m.end()) {
        set_error("state dict: missing key '%s'", name.c_str());
        return nullptr;
    }
    const pivlfn_tensor *t = it->second;
    const int want[4] = {d0, d1, d2, d3};
    bool ok = t->ndim == ndim && t->data != nullptr;
    for (int i = 0; ok && i < ndim; ++i) ok = t->shape[i] == want[i];
    if (!ok) {
        set_error("state dict: '%s' has the wrong shape (want [%d,%d,%d,%d] ndim %d)", name.c_str(), d0, d1, d2, d3, ndim);
        return nullptr;
    }
    return t;
}

// OIHW weights -> [chunk][tap][half][cout_pad][4]; chunk = 8 staged input channels of one source.
// Element (chunk, tap, h, n, j) multiplies staged channel 8*chunk_in_seg + 4*h + j of that source; when only one quad
// of the source is left (its 4-channel tail) the chunk is a half chunk: channels 2*h + j, j < 2 (two MFMAs per tap).
int pack_conv(pivlfn_net *net, const char *name, const float *w, const float *b, int cout, int cin, int kh, int kw,
              const std::vector<SegDef> &segs, ConvW *out)
{
    int creal = 0, nchunk = 0;
    std::vector<int> cr, cl, co;       // the sources as the other kernel families' packers take them
    for (auto &s : segs) { creal += s.creal; nchunk += seg_chunks(s.cload); cr.push_back(s.creal); cl.push_back(s.cload); co.push_back(s.coff); }
    const int nseg = (int)segs.size();
    if (creal != cin) { set_error("internal: segment channels %d != cin %d for %s", creal, cin, name); return PIVLFN_ERR_WEIGHTS; }
    const int taps = kh * kw, cp = rup(cout, 32);
    std::vector<float> pk((size_t)nchunk * taps * 2 * cp * 4, 0.f), bias(cp, 0.f);
    int chunk = 0, run = 0, tail = 0;
    for (size_t si = 0; si < segs.size(); ++si) {
        const SegDef &s = segs[si];
        const int coff = s.coff >= 0 ? s.coff : run;
        if (s.cload % 8 == 4 && si + 1 != segs.size()) {
            set_error("internal: only the last source of %s may end in a 4-channel tail", name);
            return PIVLFN_ERR_WEIGHTS;
        }
        for (int c0 = 0; c0 < s.cload; c0 += 8, ++chunk) {
            const bool half = s.cload - c0 <= 4;     // 4-channel tail: lane half h holds channels {2h, 2h+1} in slots j = 0, 1
            if (half) tail = 1;
            for (int t = 0; t < taps; ++t)
                for (int h = 0; h < 2; ++h)
                    for (int j = 0; j < (half ? 2 : 4); ++j) {
                        const int c = c0 + (half ? 2 * h : 4 * h) + j;
                        if (c >= s.creal) continue;
                        for (int n = 0; n < cout; ++n)
                            pk[((((size_t)chunk * taps + t) * 2 + h) * cp + n) * 4 + j] =
                                w[((size_t)n * cin + coff + c) * taps + t];
                    }
        }
        run += s.creal;
    }
    for (int n = 0; n < cout; ++n) bias[n] = b[n];
    out->cout = cout; out->cout_pad = cp; out->KH = kh; out->KW = kw; out->nchunk = nchunk; out->tail = tail; out->cin = cin;
    int rc = upload(net, pk, &out->wpk);
    if (rc) return rc;
    {   // the fp16 packing of the same layer (optional reduced-precision mode)
        std::vector<unsigned short> ph;
        pack_conv_h(w, cout, cin, taps, cr.data(), cl.data(), co.data(), nseg, ph, &out->nchunk_h);
        rc = upload(net, ph, &out->wpk_h);
        if (rc) return rc;
    }
    if (packs_col7(cout, cin, kh, kw, segs.size(), segs[0].cload)) {   // conv_dist_R.0 of levels 1 and 2
        std::vector<float> pc((size_t)4 * 7 * 2 * 64 * 4, 0.f);
        for (int blk = 0; blk < 4; ++blk)
            for (int ky = 0; ky < 7; ++ky)
                for (int hh = 0; hh < 2; ++hh)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 4; ++j) {
                            // 49 channels: block 3 = channel 48 replicated over the slots (the kernel's fourth wave takes it on the vector unit)
                            const int o = (cout == 49 && blk == 3) ? 48 : 16 * blk + (lane & 15), c = 16 * hh + 4 * (lane >> 4) + j;
                            if (o < cout) pc[((((size_t)blk * 7 + ky) * 2 + hh) * 64 + lane) * 4 + j] = w[((size_t)o * 32 + c) * 7 + ky];
                        }
        rc = upload(net, pc, &out->wpk_c);
        if (rc) return rc;
    }
    if (packs_row7(cout, cin, kh, kw, segs.size(), segs[0].cload)) {   // conv_dist_R.1 of levels 1 and 2
        std::vector<float> pr((size_t)4 * 7 * 3 * 64 * 4, 0.f), p12((size_t)4 * 7 * 64, 0.f);
        for (int blk = 0; blk < 4; ++blk)
            for (int kx = 0; kx < 7; ++kx)
                for (int lane = 0; lane < 64; ++lane) {
                    // block 3 = output channel 48 replicated over the slots (the kernel's vector path)
                    const int o = blk == 3 ? 48 : 16 * blk + (lane & 15), kq = lane >> 4;
                    for (int g = 0; g < 3; ++g)
                        for (int j = 0; j < 4; ++j)
                            pr[((((size_t)blk * 7 + kx) * 3 + g) * 64 + lane) * 4 + j] = w[((size_t)o * 49 + 4 * (kq + 4 * g) + j) * 7 + kx];
                    if (kq == 0) p12[((size_t)blk * 7 + kx) * 64 + lane] = w[((size_t)o * 49 + 48) * 7 + kx];
                }
        rc = upload(net, pr, &out->wpk_r);
        if (rc) return rc;
        rc = upload(net, p12, &out->wpk_r12);
        if (rc) return rc;
    }
    if (packs_dist_b3(cout, cin, kh, kw, segs.size(), segs[0].cload)) {   // both once more as exactly split bf16 pieces (conv_dist_b3.hip)
        std::vector<unsigned short> pb;
        pack_conv_dist_b3(w, cin, pb);
        rc = upload(net, pb, kh == 7 ? &out->wpk_cb : &out->wpk_rb);
        if (rc) return rc;
    }
    if (kh == 3 && kw == 3) {      // 3 x 3: the Winograd-domain packing (used by the stride-1 call sites)
        std::vector<float> pw;
        pack_conv_w(w, cout, cin, cr.data(), cl.data(), co.data(), nseg, pw, &out->nchunk_w);
        rc = upload(net, pw, &out->wpk_w);
        if (rc) return rc;
        // F(4x4): 2.25 x the F(2x2) planes per layer -- only where something can launch it (round 4 packed and uploaded it for every
        // 3 x 3 layer of every network although pivlfn_forward never reaches that kernel outside the tools build's knob 13)
#ifdef PIVLFN_TOOLS
        pack_conv_w4(w, cout, cin, cr.data(), cl.data(), co.data(), nseg, pw, &out->nchunk_w4);
        rc = upload(net, pw, &out->wpk_w4);
        if (rc) return rc;
#endif
        if (conv_wino_b3_supports(cp)) {
            std::vector<unsigned short> pb;
            pack_conv_wb(w, cout, cin, cr.data(), cl.data(), co.data(), nseg, pb, &out->nstep_wb);
            rc = upload(net, pb, &out->wpk_wb);
            if (rc) return rc;
        }
    }
    if (conv_split_supports(kh, kw, 1, cp, 6)) {   // the split-operand packing of the same layer (fp32 on the fp16 matrix cores)
        std::vector<unsigned short> px;
        pack_conv_x(w, cout, cin, taps, cr.data(), cl.data(), co.data(), nseg, px, &out->nchunk_x, &out->scale_x);
        rc = upload(net, px, &out->wpk_x);
        if (rc) return rc;
        // a 4-lane tail (the last source's cload = 4 mod 16): the same channels again, taps folded into K, for the 16-row kernel
        const SegDef &ls = segs.back();
        if (kh == 3 && kw == 3 && ls.cload % 16 == 4) {
            int run = 0;
            for (size_t si = 0; si + 1 < segs.size(); ++si) run += segs[si].creal;
            const int first = (ls.coff >= 0 ? ls.coff : run) + ls.cload - 4;          // first weight channel of the tail lanes
            const int real = std::max(0, std::min(4, ls.creal - (ls.cload - 4)));
            std::vector<unsigned short> pt;
            pack_conv_x_tail(w, cout, cin, first, real, out->scale_x, pt);
            rc = upload(net, pt, &out->wtail_x);
            if (rc) return rc;
        }
    }
    return upload(net, bias, &out->bias);
}

// The OIHW weights of one source of a layer, [cout][creal of the source][taps]: the input channels pack_conv multiplies that
// source by (SegDef::coff, or the running offset of the sources before it)
static void seg_weights(const float *w, int cout, int cin, int taps, const std::vector<SegDef> &segs, size_t si, std::vector<float> &out)
{
    int run = 0;
    for (size_t i = 0; i < si; ++i) run += segs[i].creal;
    const int coff = segs[si].coff >= 0 ? segs[si].coff : run, cr = segs[si].creal;
    out.assign((size_t)cout * cr * taps, 0.f);
    for (int n = 0; n < cout; ++n)
        for (int c = 0; c < cr; ++c)
            for (int t = 0; t < taps; ++t) out[((size_t)n * cr + c) * taps + t] = w[((size_t)n * cin + coff + c) * taps + t];
}

// The same from the state dict: the layer's two tensors by name
static int pack_conv(pivlfn_net *net, const TMap &m, const std::string &name, int cout, int cin, int kh, int kw,
                     const std::vector<SegDef> &segs, ConvW *out)
{
    const pivlfn_tensor *w = find(m, name + ".weight", cout, cin, kh, kw, 4);
    const pivlfn_tensor *b = find(m, name + ".bias", cout, 0, 0, 0, 1);
    if (!w || !b) return PIVLFN_ERR_WEIGHTS;
    return pack_conv(net, name.c_str(), w->data, b->data, cout, cin, kh, kw, segs, out);
}

// Depthwise ConvTranspose2d k4 weights, OIHW [C,1,4,4] -> [16 taps][cpad channels] (padding channels zero: their outputs stay exact zeros)
void pack_dw_host(const float *w, int C, int cpad, std::vector<float> &h)
{
    h.assign((size_t)cpad * 16, 0.f);
    for (int c = 0; c < C; ++c)
        for (int t = 0; t < 16; ++t) h[(size_t)t * cpad + c] = w[(size_t)c * 16 + t];
}

static int pack_dw(pivlfn_net *net, const TMap &m, const std::string &name, int C, int cpad, float **dev)
{
    const pivlfn_tensor *w = find(m, name, C, 1, 4, 4, 4);
    if (!w) return PIVLFN_ERR_WEIGHTS;
    std::vector<float> h;
    pack_dw_host(w->data, C, cpad, h);
    return upload(net, h, dev);
}

// Level 1's NetC_ext (we [64,32], be [64]) and moduleFeat (wf [128,32], bfe [128]) in the fragment order of Conv1Fuse
void pack_conv1_fuse(const float *we, const float *be, const float *wf, const float *bfe, std::vector<float> &w11, std::vector<float> &b11)
{
    w11.assign((size_t)6 * 4 * 64 * 4, 0.f);
    b11.assign(192, 0.f);
    for (int blk = 0; blk < 6; ++blk)
        for (int g = 0; g < 4; ++g)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 4; ++e) {
                    const int c = 8 * g + 4 * (lane >> 5) + e, o = 32 * (blk < 2 ? blk : blk - 2) + (lane & 31);
                    w11[(((size_t)blk * 4 + g) * 64 + lane) * 4 + e] = blk < 2 ? we[(size_t)o * 32 + c] : wf[(size_t)o * 32 + c];
                }
    for (int o = 0; o < 64; ++o) b11[o] = be[o];
    for (int o = 0; o < 128; ++o) b11[64 + o] = bfe[o];
}

// Flow-head weights for conv_head.hip: OIHW [2,32,k,k] -> [tap][channel quad][4][output] (the two outputs of a channel adjacent:
// one 64-bit scalar operand of a packed fp32 fma)
int pack_head(pivlfn_net *net, const float *w, const float *b, int k, float **dev, float bias[2])
{
    // [k*k][8][4][2] for the vector kernels, followed by the A fragments of the matrix-core head (conv_head_mfma_kernel):
    // [ky][half h][lane 64][4]: lane = slot n (= 8 o + kx) + 16 kq, element j multiplies channel 16 h + 4 kq + j (zero for kx >= k)
    std::vector<float> h((size_t)k * k * 64 + (size_t)k * 2 * 64 * 4, 0.f);
    for (int t = 0; t < k * k; ++t)
        for (int q = 0; q < 8; ++q)
            for (int o = 0; o < 2; ++o)
                for (int j = 0; j < 4; ++j)
                    h[(((size_t)t * 8 + q) * 4 + j) * 2 + o] = w[((size_t)o * 32 + 4 * q + j) * k * k + t];
    for (int ky = 0; ky < k; ++ky)
        for (int hh = 0; hh < 2; ++hh)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j) {
                    const int n = lane & 15, kq = lane >> 4, o = n >> 3, kx = n & 7, c = 16 * hh + 4 * kq + j;
                    if (kx < k) h[(size_t)k * k * 64 + (((size_t)ky * 2 + hh) * 64 + lane) * 4 + j] = w[((size_t)o * 32 + c) * k * k + ky * k + kx];
                }
    bias[0] = b[0];
    bias[1] = b[1];
    return upload(net, h, dev);
}

static int pack_head(pivlfn_net *net, const TMap &m, const std::string &name, int k, float **dev, float bias[2])
{
    const pivlfn_tensor *w = find(m, name + ".weight", 2, 32, k, k, 4);
    const pivlfn_tensor *b = find(m, name + ".bias", 2, 0, 0, 0, 1);
    if (!w || !b) return PIVLFN_ERR_WEIGHTS;
    return pack_head(net, w->data, b->data, k, dev, bias);
}

int net_destroy(pivlfn_net *net)
{
    if (!net) return PIVLFN_OK;
    for (void *p : net->allocs) (void)hipFree(p);
    for (hipEvent_t e : net->ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : net->ev_fork) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : net->ev_join) if (e) (void)hipEventDestroy(e);
    if (net->ev_pfork) (void)hipEventDestroy(net->ev_pfork);
    for (hipEvent_t e : net->ev_pjoin) if (e) (void)hipEventDestroy(e);
    if (net->side) (void)hipStreamDestroy(net->side);
    delete net;
    return PIVLFN_OK;
}

// Per timed launch of the chosen level's warp+correlation: events [0,1] = start/stop of the dispatch itself
// (hipExtLaunchKernelGGL), events [2,3] = a plain hipEventRecord pair around it.  Read back after the timed region.
int net_profile_enable(pivlfn_net *net, int level)
{
    PIV_REQUIRE(net && level >= 0 && level <= 6, "profile_enable: bad arguments");
    net->prof_level = level;
    if (level && net->ev.empty()) {
        net->ev.resize(4 * 4096);
        for (auto &e : net->ev) PIV_CHECK_HIP(hipEventCreate(&e));
    }
    net->ev_used = 0;
    net->ev_dropped = 0;
    return PIVLFN_OK;
}

int net_profile_read(pivlfn_net *net, double *ms, double *ms_empty, long *launches, int reset)
{
    PIV_REQUIRE(net && ms && ms_empty && launches, "profile_read: null argument");
    double tot = 0.0, empty = 0.0;
    for (size_t i = 0; i + 3 < net->ev_used; i += 4) {
        PIV_CHECK_HIP(hipEventSynchronize(net->ev[i + 3]));
        float t = 0.f, e = 0.f;
        PIV_CHECK_HIP(hipEventElapsedTime(&t, net->ev[i], net->ev[i + 1]));
        PIV_CHECK_HIP(hipEventElapsedTime(&e, net->ev[i + 2], net->ev[i + 3]));
        tot += t;
        empty += e;
    }
    *ms = tot;
    *ms_empty = empty;
    *launches = (long)(net->ev_used / 4);
    if (reset) { net->ev_used = 0; net->ev_dropped = 0; }
    return PIVLFN_OK;
}

int net_create(const pivlfn_tensor *tensors, int n, float starting_scale, int lowest, const float mean[6], pivlfn_net **out)
{
    PIV_REQUIRE(tensors && n > 0 && out && mean, "create: null argument");
    PIV_REQUIRE(lowest >= 1 && lowest <= 6, "create: lowest_level=%d out of range", lowest);
    TMap m;
    for (int i = 0; i < n; ++i) {
        PIV_REQUIRE(tensors[i].name, "create: tensor %d has no name", i);
        m[tensors[i].name] = &tensors[i];
    }
    pivlfn_net *net = new pivlfn_net();
    net->lowest = lowest;
    for (int L = 0; L < 7; ++L) net->scale[L] = starting_scale / (float)(1 << L);     // src/models.py:61-63
    for (int i = 0; i < 6; ++i) net->mean[i] = mean[i];
    if (m.count("NetE_M.0.conv_M.10.weight")) {          // LiteFlowNet2 layout: five hidden layers per stack
        net->nstack = 5;
        const int w2[5] = {128, 128, 96, 64, 32};
        for (int j = 0; j < 5; ++j) net->width[j] = w2[j];
    }
#define TRY(expr) do { int _rc = (expr); if (_rc) { net_destroy(net); return _rc; } } while (0)
    // NetC (src/models.py:70-106); conv1 reads the 4-lane padded image
    struct { const char *name; int cout, cin, k; } nc[10] = {
        {"NetC.conv1.0", 32, 3, 7}, {"NetC.conv2.0", 32, 32, 3}, {"NetC.conv2.2", 32, 32, 3}, {"NetC.conv2.4", 32, 32, 3},
        {"NetC.conv3.0", 64, 32, 3}, {"NetC.conv3.2", 64, 64, 3}, {"NetC.conv4.0", 96, 64, 3}, {"NetC.conv4.2", 96, 96, 3},
        {"NetC.conv5.0", 128, 96, 3}, {"NetC.conv6.0", 192, 128, 3}};
    for (int i = 0; i < 10; ++i)
        TRY(pack_conv(net, m, nc[i].name, nc[i].cout, nc[i].cin, nc[i].k, nc[i].k, {{nc[i].cin, rup(nc[i].cin, 4)}}, &net->netc[i]));
    // NetC_ext (src/models.py:309-311, 353-355): idx = L-1; NetC_ext[idx-1], python negative index for L1
    const int n_ext = lowest <= 2 ? 2 - (lowest - 1) : 0;
    for (int L = lowest; L <= 2; ++L) {
        int j = (L - 1) - 1;
        if (j < 0) j += n_ext;
        TRY(pack_conv(net, m, "NetC_ext." + std::to_string(j) + ".conv_ext.0", 64, 32, 1, 1, {{32, 32}}, &net->ext[L]));
    }
    for (int L = lowest; L <= 6; ++L) {
        const int i = L - lowest, k = K_LEVEL[L], cm = C_MATCH[L];
        LevelW &lw = net->lv[L];
        const std::string pm = "NetE_M." + std::to_string(i) + ".", ps = "NetE_S." + std::to_string(i) + ".",
                          pr = "NetE_R." + std::to_string(i) + ".";
        if (L != 6) TRY(pack_dw(net, m, pm + "upConv_M.weight", 2, 4, &lw.upconv));
        if (L < 4) TRY(pack_dw(net, m, pm + "upCorr_M.weight", 49, 56, &lw.upcorr));
        {
            int cin = 49;
            for (int j = 0; j < net->nstack; ++j) {
                const int wd = net->width[j];
                const std::string nm = pm + "conv_M." + std::to_string(2 * j);
                if (j == 0) TRY(pack_conv(net, m, nm, wd, 49, 3, 3, {{49, 52}}, &lw.M[0]));
                else TRY(pack_conv(net, m, nm, wd, cin, 3, 3, {{cin, cin}}, &lw.M[j]));
                cin = wd;
            }
            const std::string hm = pm + "conv_M." + std::to_string(2 * net->nstack);
            TRY(pack_conv(net, m, hm, 2, 32, k, k, {{32, 32}}, &lw.M[net->nstack]));
            TRY(pack_head(net, m, hm, k, &lw.headM, lw.hbM));
            cin = 2 * cm + 2;
            for (int j = 0; j < net->nstack; ++j) {
                const int wd = net->width[j];
                const std::string nm = ps + "conv_S." + std::to_string(2 * j);
                if (j == 0) TRY(pack_conv(net, m, nm, wd, 2 * cm + 2, 3, 3, {{cm, cm}, {cm, cm}, {2, 4}}, &lw.S[0]));
                else TRY(pack_conv(net, m, nm, wd, cin, 3, 3, {{cin, cin}}, &lw.S[j]));
                cin = wd;
            }
            const std::string hs = ps + "conv_S." + std::to_string(2 * net->nstack);
            TRY(pack_conv(net, m, hs, 2, 32, k, k, {{32, 32}}, &lw.S[net->nstack]));
            TRY(pack_head(net, m, hs, k, &lw.headS, lw.hbS));
        }
        const int cfr = L < 5 ? 128 : C_FEAT[L];
        if (L < 5) TRY(pack_conv(net, m, pr + "moduleFeat.0", 128, C_FEAT[L], 1, 1, {{C_FEAT[L], C_FEAT[L]}}, &lw.feat));
        const std::vector<SegDef> r0segs = {{cfr, cfr, 3}, {3, 4, 0}};                                     // reference order is [norm, rm, feat] (:280)
        TRY(pack_conv(net, m, pr + "conv_R.0", 128, 3 + cfr, 3, 3, r0segs, &lw.R[0]));
        if (L < 5) {      // the same layer as two, one per source: a convolution is linear in its input channels
            const pivlfn_tensor *w0 = find(m, pr + "conv_R.0.weight", 128, 3 + cfr, 3, 3, 4), *b0 = find(m, pr + "conv_R.0.bias", 128, 0, 0, 0, 1);
            if (!w0 || !b0) { net_destroy(net); return PIVLFN_ERR_WEIGHTS; }
            std::vector<float> ws;
            const std::vector<float> zero(128, 0.f);
            seg_weights(w0->data, 128, 3 + cfr, 9, r0segs, 0, ws);
            TRY(pack_conv(net, "conv_R.0 (features)", ws.data(), zero.data(), 128, r0segs[0].creal, 3, 3, {{r0segs[0].creal, r0segs[0].cload}}, &lw.R0a));
            seg_weights(w0->data, 128, 3 + cfr, 9, r0segs, 1, ws);
            TRY(pack_conv(net, "conv_R.0 (flow)", ws.data(), b0->data, 128, r0segs[1].creal, 3, 3, {{r0segs[1].creal, r0segs[1].cload}}, &lw.R0b));
            if (r0segs[1].creal == 3) {      // the streaming kernel's order: [tap][channel][output]
                std::vector<float> wt((size_t)9 * 3 * 128);
                for (int n = 0; n < 128; ++n)
                    for (int c = 0; c < 3; ++c)
                        for (int t = 0; t < 9; ++t) wt[((size_t)t * 3 + c) * 128 + n] = ws[((size_t)n * 3 + c) * 9 + t];
                TRY(upload(net, wt, &lw.r0t));
            }
        }
        TRY(pack_conv(net, m, pr + "conv_R.2", 128, 128, 3, 3, {{128, 128}}, &lw.R[1]));
        TRY(pack_conv(net, m, pr + "conv_R.4", 64, 128, 3, 3, {{128, 128}}, &lw.R[2]));
        TRY(pack_conv(net, m, pr + "conv_R.6", 64, 64, 3, 3, {{64, 64}}, &lw.R[3]));
        TRY(pack_conv(net, m, pr + "conv_R.8", 32, 64, 3, 3, {{64, 64}}, &lw.R[4]));
        TRY(pack_conv(net, m, pr + "conv_R.10", 32, 32, 3, 3, {{32, 32}}, &lw.R[5]));
        const int kk = k * k;
        if (L < 5) {
            TRY(pack_conv(net, m, pr + "conv_dist_R.0", kk, 32, k, 1, {{32, 32}}, &lw.dist0));
            TRY(pack_conv(net, m, pr + "conv_dist_R.1", kk, kk, 1, k, {{kk, rup(kk, 4)}}, &lw.dist1));
        } else {
            TRY(pack_conv(net, m, pr + "conv_dist_R.0", kk, 32, k, k, {{32, 32}}, &lw.dist0));
        }
        const pivlfn_tensor *wx = find(m, pr + "moduleScaleX.weight", 1, kk, 1, 1, 4), *bx = find(m, pr + "moduleScaleX.bias", 1, 0, 0, 0, 1);
        const pivlfn_tensor *wy = find(m, pr + "moduleScaleY.weight", 1, kk, 1, 1, 4), *by = find(m, pr + "moduleScaleY.bias", 1, 0, 0, 0, 1);
        if (!wx || !bx || !wy || !by) { net_destroy(net); return PIVLFN_ERR_WEIGHTS; }
        TRY(upload(net, std::vector<float>(wx->data, wx->data + kk), &lw.wx));
        TRY(upload(net, std::vector<float>(wy->data, wy->data + kk), &lw.wy));
        lw.bx = bx->data[0];
        lw.by = by->data[0];
    }
    if (lowest == 1) {      // the two 1 x 1 layers that read NetC.conv1's output at level 1, in the fragment order of Conv1Fuse
        int j = -1;
        if (j < 0) j += n_ext;                       // NetC_ext index of level 1 (python negative index, as above)
        const pivlfn_tensor *we = find(m, "NetC_ext." + std::to_string(j) + ".conv_ext.0.weight", 64, 32, 1, 1, 4);
        const pivlfn_tensor *be = find(m, "NetC_ext." + std::to_string(j) + ".conv_ext.0.bias", 64, 0, 0, 0, 1);
        const pivlfn_tensor *wf = find(m, "NetE_R." + std::to_string(1 - lowest) + ".moduleFeat.0.weight", 128, 32, 1, 1, 4);
        const pivlfn_tensor *bfe = find(m, "NetE_R." + std::to_string(1 - lowest) + ".moduleFeat.0.bias", 128, 0, 0, 0, 1);
        if (!we || !be || !wf || !bfe) { net_destroy(net); return PIVLFN_ERR_WEIGHTS; }
        std::vector<float> w11, b11;
        pack_conv1_fuse(we->data, be->data, wf->data, bfe->data, w11, b11);
        TRY(upload(net, w11, &net->fuse1_w));
        TRY(upload(net, b11, &net->fuse1_b));
    }
#undef TRY
    if (hipStreamCreateWithFlags(&net->side, hipStreamNonBlocking) != hipSuccess) {
        set_error("create: side stream creation failed");
        net_destroy(net);
        return PIVLFN_ERR_HIP;
    }
    for (int L = lowest; L <= 6; ++L)
        if (hipEventCreateWithFlags(&net->ev_join[L], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&net->ev_fork[L], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&net->ev_pjoin[L], hipEventDisableTiming) != hipSuccess ||
            (!net->ev_pfork && hipEventCreateWithFlags(&net->ev_pfork, hipEventDisableTiming) != hipSuccess)) {
            set_error("create: event creation failed");
            net_destroy(net);
            return PIVLFN_ERR_HIP;
        }
    *out = net;
    return PIVLFN_OK;
}

int net_set_precision(pivlfn_net *net, int precision)
{
    PIV_REQUIRE(net && precision >= 0 && precision <= 5, "set_precision: 0 (fp32: Winograd with exactly split operands / fp32 instruction), 1 (fp16 multiplicands), 2 (fp32 by exact fp16 splitting), 3 (three-term splitting), 4 (fp32 instruction, direct convolution only) or 5 (fp32 instruction, Winograd) expected");
    net->precision = precision;
    return PIVLFN_OK;
}

}  // namespace pivlfn
