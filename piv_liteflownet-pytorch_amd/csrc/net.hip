// pivlfn_forward: the workspace plan and the coarse-to-fine level pipeline of LiteFlowNet.forward (src/models.py:319-370 of the
// reference) expressed as a fixed sequence of gfx950 kernel launches on one stream.  No allocation, no host sync inside forward.
// The weights are packed in net_weights.hip; which kernel a layer runs on is conv()'s choice in conv_layer.hip.
#include <algorithm>
#include <initializer_list>
#include <vector>
#include "net.h"

namespace pivlfn {

// ---- workspace plan -------------------------------------------------------------------------------------------
struct Plan {
    size_t off = 0;
    char *base = nullptr;
    float *take(size_t floats)
    {
        float *p = base ? reinterpret_cast<float *>(base + off) : nullptr;
        off += (floats * sizeof(float) + 255) / 256 * 256;
        return p;
    }
};

struct Buffers {
    float *img[7], *feat[7], *ext[3], *sa, *sb;
    float *flowA, *flowB, *flow_up, *flowM, *flowS, *corr, *corr_up, *t128a, *t128b, *t64a, *t64b, *t32a, *t32b,
        *f2w, *featR[7], *misc4, *d1, *dist, *partial, *mean, *ksplit, *part[7];
};

// Regularization's first layer, conv_R.0 over {featR[L], misc4} (:280), is nine-tenths flow-independent: eight of its nine 16-channel
// K steps multiply featR[L], which is ready after NetC.  At the levels where that layer is a Winograd launch of the fp32 modes on a
// grid of at least 256 x 256 per image (where CONV_WINO_B3 begins; per image, never a function of the batch) the forward computes
//     part[L] = W[:, feat] * featR[L]                              (R0a, no bias, no activation) on the side stream, and
//     R.0     = LReLU(W[:, misc] * misc4 + bias + part[L])          (reg_r0_tail_kernel, a streaming pass) on the main stream.
// Workspace: part[L] is B x h x w x 128 floats per split level -- 512 + 128 + 32 MiB per pair at 1024 x 1024.
static bool r0_split_level(const pivlfn_net *net, int L, int h, int w)
{
    return L >= net->lowest && L < 5 && (long)h * w >= 256 * 256 && (long)16 * w * 128 * 4 < (1L << 31);
}
// Compute units a side-stream launch of the persistent Winograd kernel leaves to the main stream's chains of small kernels
// (measured 0 / 32 / 64 / 96 and steps of 8 between: DESIGN.md 4.2g)
static const int SIDE_CU_RESERVE = 32;

static void plan(const pivlfn_net *net, int B, int H, int W, Plan &pl, Buffers &bf)
{
    int h[7], w[7];
    for (int L = 1; L <= 6; ++L) { h[L] = H >> (L - 1); w[L] = W >> (L - 1); }
    const size_t N2 = 2 * (size_t)B;
    for (int L = 1; L <= 6; ++L) bf.img[L] = pl.take(N2 * h[L] * w[L] * 4);
    for (int L = 1; L <= 6; ++L) bf.feat[L] = pl.take(N2 * h[L] * w[L] * C_FEAT[L]);
    for (int L = 1; L <= 2; ++L) bf.ext[L] = L >= net->lowest ? pl.take(N2 * h[L] * w[L] * 64) : nullptr;
    bf.sa = pl.take(N2 * h[2] * w[2] * 32);
    bf.sb = pl.take(N2 * h[2] * w[2] * 32);
    const int ll = net->lowest;
    const size_t px = (size_t)B * h[ll] * w[ll];
    size_t f2w = 0;
    for (int L = ll; L <= 6; ++L) f2w = std::max(f2w, (size_t)B * h[L] * w[L] * C_MATCH[L]);
    bf.flowA = pl.take(px * 4); bf.flowB = pl.take(px * 4); bf.flow_up = pl.take(px * 4);
    bf.flowM = pl.take(px * 4); bf.flowS = pl.take(px * 4);
    bf.corr = pl.take(px * 56); bf.corr_up = pl.take(px * 56);
    bf.t128a = pl.take(px * 128); bf.t128b = pl.take(px * 128);
    bf.t64a = pl.take(px * 64); bf.t64b = pl.take(px * 64);
    bf.t32a = pl.take(px * 32); bf.t32b = pl.take(px * 32);
    bf.f2w = pl.take(f2w);
    for (int L = 1; L <= 6; ++L) bf.featR[L] = (L >= ll && L < 5) ? pl.take((size_t)B * h[L] * w[L] * 128) : nullptr;   // one per level: filled on the side stream
    bf.misc4 = pl.take(px * 4);
    bf.d1 = pl.take(px * 56); bf.dist = pl.take(px * 56);
    bf.ksplit = pl.take(KSPLIT_FLOATS * 2 * B);     // per image (NetC runs 2B images): the split never depends on the batch
    bf.partial = pl.take((size_t)B * flow_mean_partials(0) * 2);
    bf.mean = pl.take((size_t)B * 2);
    // one per split level (not inside featR[1]: the deeper levels' sums are needed first and are computed first), in the modes that
    // split: the plan follows the precision set when it is made, and a forward in a mode that needs more than it was given is refused
    const bool splits = net->precision == 0 || net->precision == 5;
    for (int L = 1; L <= 6; ++L)
        bf.part[L] = (splits && r0_split_level(net, L, h[L], w[L])) ? pl.take((size_t)B * h[L] * w[L] * 128) : nullptr;
}

size_t net_workspace_bytes(const pivlfn_net *net, int B, int H, int W)
{
    Plan pl; Buffers bf;
    plan(net, B, H, W, pl, bf);
    return pl.off;
}

size_t net_levels_floats(const pivlfn_net *net, int B, int H, int W)
{
    size_t n = 0;
    for (int L = net->lowest; L <= 6; ++L) n += (size_t)3 * B * 2 * (H >> (L - 1)) * (W >> (L - 1));
    return n;
}

int net_forward(pivlfn_net *net, const float *img1, const float *img2, float *flow, float *levels, int B, int H, int W,
                void *ws, size_t ws_bytes, hipStream_t st)
{
    PIV_REQUIRE(net && img1 && img2 && flow && ws, "forward: null argument");
    PIV_REQUIRE(B > 0 && H >= 32 && W >= 32 && H % 32 == 0 && W % 32 == 0,
                "forward: H=%d W=%d must be positive multiples of 32 (use estimate() for other sizes)", H, W);
    PIV_REQUIRE((reinterpret_cast<size_t>(ws) & 255) == 0, "forward: workspace must be 256-byte aligned");
    Plan pl; Buffers bf;
    pl.base = reinterpret_cast<char *>(ws);
    plan(net, B, H, W, pl, bf);
    if (pl.off > ws_bytes) {
        set_error("forward: workspace of %zu bytes is too small, need %zu", ws_bytes, pl.off);
        return PIVLFN_ERR_WORKSPACE;
    }
    int h[7], w[7];
    for (int L = 1; L <= 6; ++L) { h[L] = H >> (L - 1); w[L] = W >> (L - 1); }
    const int N2 = 2 * B;
    // what conv() chooses by: PIVLFN_PRECISION_F32_WINO_MFMA32 (5) is precision 0 without the split-bf16 Winograd kernel
    const int reserve = PIV_KNOB(8) ? PIV_KNOB(8) - 1 : SIDE_CU_RESERVE;           // tools A/B: knob 8 = reserve + 1
    const ConvCtx ctx{net->precision == 5 ? 0 : net->precision, net->precision == 5, bf.ksplit, net->side,
                      std::max(8, (device_cus() - reserve) / 8 * 8)};
    auto conv = [&ctx](const ConvW &cw, std::initializer_list<ConvSeg> segs, float *out, int out_stride, int cout_store, const float *res,
                       int res_stride, int lrelu, int B, int H, int W, int S, int padY, int padX, hipStream_t st, int in16 = 0, int out16 = 0) {
        return pivlfn::conv(ctx, cw, conv_call(segs.begin(), (int)segs.size(), out, out_stride, cout_store, res, res_stride, lrelu, B, H, W, S,
                                               padY, padX, in16, out16), st);
    };
#define RUN(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)
    // mean subtraction + layout change (:321-323), image pyramid (:336-343)
    RUN(launch_prep_images(img1, img2, bf.img[1], B, H, W, net->mean, st));
    for (int L = 2; L <= 6; ++L) RUN(launch_resize_nhwc4(bf.img[L - 1], bf.img[L], N2, h[L - 1], w[L - 1], h[L], w[L], st));
    // Flow-independent 1x1 convs on the side stream: NetC_ext (:353-355) for levels <= 2 and Regularization.moduleFeat (:227-232,
    // applied at :280) for levels < 5; 1.8 GB of HBM traffic at 1024^2.  Where they run is a trade: beside NetC they slow its
    // MFMA-bound kernels and push the level-3 features out of the Infinity Cache; beside levels 6-4 those chains of tiny kernels
    // wait for CUs (the level-5 warp+correlation 15 -> 40 us).  Round 2, early: issued per level as soon as NetC had produced the
    // level's features (the level-3 launch gained 2.6 us).  Late round 2: the conv stacks are twice as fast, the prefetch pass below
    // restores the level-3 features whatever the order, and all of it after NetC is the faster step (10.58 vs 10.70 ms,
    // tools/net_ab.py --masks 0,4096, three interleaved rounds) -- the default again; the early order stays selectable in the tools build.
    const hipStream_t side = (PIV_KNOB(1) & 2048) ? st : net->side;        // tools A/B: everything on one stream
    // Whatever path leaves this function -- also an early error return -- the main stream joins every piece of side-stream work
    // that was forked and not yet waited for: an un-joined fork would invalidate a stream capture and let the side kernels run on
    // into the caller's next use of the workspace.
    struct SideJoin {
        hipStream_t st;
        hipEvent_t *ev, *evp;
        unsigned pending = 0;         // bit L: ev[L], bit 8 + L: evp[L] (the partial sums of conv_R.0)
        ~SideJoin()
        {
            for (int L = 0; L < 7; ++L) {
                if (pending & (1u << L)) (void)hipStreamWaitEvent(st, ev[L], 0);
                if (pending & (256u << L)) (void)hipStreamWaitEvent(st, evp[L], 0);
            }
        }
    } side_join{st, net->ev_join, net->ev_pjoin};
    const bool side_early = (PIV_KNOB(1) & 4096) != 0;                     // tools A/B: 4096 = each level's share right behind its NetC layer
    bool fused1 = false;          // level 1's two 1 x 1 layers were computed inside NetC.conv1's kernel (below)
    // conv_R.0's feature part (r0_split_level) on the side stream, directly behind the 1 x 1 layer that makes featR[L] (side_level
    // below issues it) and in front of the touch pass.  Not in the other modes, and not with everything on one stream: they keep
    // the single-launch layer.  tools A/B: 16777216 = no split; 33554432 = level 1's share right behind conv1's fused kernel (beside
    // NetC) instead of after NetC; 67108864 = level 1 keeps the single-launch layer
    bool split[7] = {false, false, false, false, false, false, false};
    int last_part = 0;            // the level whose partial sum went to the side stream last: once it is done, all of them are
    if ((net->precision == 0 || net->precision == 5) && side != st && !(PIV_KNOB(1) & 16777216))
        for (int L = 1; L <= 6; ++L) split[L] = r0_split_level(net, L, h[L], w[L]) && !(L == 1 && (PIV_KNOB(1) & 67108864));
    auto part_level = [&](int L) -> int {
        if (!split[L] || (side_join.pending & (256u << L))) return PIVLFN_OK;
        // featR[L] is the side stream's own, written by the launch (or the one but last launch) in front of this one: stream order,
        // with no event wait between producer and consumer (graph capture); part[L]'s last reader, the previous
        // forward's tail pass, is behind side_level's fork.  Level 1's fused featR is conv1's kernel's, on the main stream: that one
        // needs a fork of its own.
        if (L == 1 && fused1) {
            PIV_CHECK_HIP(hipEventRecord(net->ev_pfork, st));
            PIV_CHECK_HIP(hipStreamWaitEvent(side, net->ev_pfork, 0));
        }
        RUN(conv(net->lv[L].R0a, {{bf.featR[L], 128, 128}}, bf.part[L], 128, 128, nullptr, 0, 0, B, h[L], w[L], 1, 1, 1, side));
        PIV_CHECK_HIP(hipEventRecord(net->ev_pjoin[L], side));
        side_join.pending |= 256u << L;
        last_part = L;
        return PIVLFN_OK;
    };
    auto side_level = [&](int L) -> int {
        if (L < net->lowest || L > 4) return PIVLFN_OK;
        if (L == 1 && fused1) return part_level(L);
        if (side != st) {
            PIV_CHECK_HIP(hipEventRecord(net->ev_fork[L], st));
            PIV_CHECK_HIP(hipStreamWaitEvent(side, net->ev_fork[L], 0));
        }
        RUN(conv(net->lv[L].feat, {{bf.feat[L], C_FEAT[L], C_FEAT[L]}}, bf.featR[L], 128, 128, nullptr, 0, 1, B, h[L], w[L], 1, 0, 0, side));
        if (L <= 2)
            RUN(conv(net->ext[L], {{bf.feat[L], 32, 32}}, bf.ext[L], 64, 64, nullptr, 0, 1, N2, h[L], w[L], 1, 0, 0, side));
        PIV_CHECK_HIP(hipEventRecord(net->ev_join[L], side));
        if (side != st) side_join.pending |= 1u << L;
        return part_level(L);
    };
    // NetC on both frames as one batch of 2B (:325-326, Features.forward :108-116)
    const ConvW *nc = net->netc;
    // Level 1's NetC_ext (32 -> 64, both frames) and moduleFeat (32 -> 128, first frame) read nothing but conv1's output: in the fp32
    // modes they are computed from conv1's activated accumulators in its own kernel -- their 1 GB of writes goes out under conv1's
    // matrix work instead of beside the latency-bound chains of levels 6-4, and conv1's output is not read back twice.
    if (net->lowest == 1 && net->fuse1_w && (ctx.precision == 0 || ctx.precision == 4) && !(PIV_KNOB(1) & 536870912)) {
        const ConvSeg s1{bf.img[1], 4, 4};
        const ConvParams p1 = conv_params(nc[0], conv_call(&s1, 1, bf.feat[1], 32, 32, nullptr, 0, 1, N2, h[1], w[1], 1, 3, 3));
        const Conv1Fuse f1{net->fuse1_w, net->fuse1_b, bf.ext[1], bf.featR[1], B};
        const int rc1 = launch_conv1_fused(p1, f1, st);
        if (rc1 > 0) return rc1;
        fused1 = rc1 == 0;
    }
    if (!fused1) RUN(conv(nc[0], {{bf.img[1], 4, 4}}, bf.feat[1], 32, 32, nullptr, 0, 1, N2, h[1], w[1], 1, 3, 3, st));
    if (fused1 ? (PIV_KNOB(1) & 33554432) != 0 : side_early) RUN(side_level(1));
    RUN(conv(nc[1], {{bf.feat[1], 32, 32}}, bf.sa, 32, 32, nullptr, 0, 1, N2, h[1], w[1], 2, 1, 1, st));
    RUN(conv(nc[2], {{bf.sa, 32, 32}}, bf.sb, 32, 32, nullptr, 0, 1, N2, h[2], w[2], 1, 1, 1, st));
    RUN(conv(nc[3], {{bf.sb, 32, 32}}, bf.feat[2], 32, 32, nullptr, 0, 1, N2, h[2], w[2], 1, 1, 1, st));
    if (side_early) RUN(side_level(2));
    RUN(conv(nc[4], {{bf.feat[2], 32, 32}}, bf.sa, 64, 64, nullptr, 0, 1, N2, h[2], w[2], 2, 1, 1, st));
    RUN(conv(nc[5], {{bf.sa, 64, 64}}, bf.feat[3], 64, 64, nullptr, 0, 1, N2, h[3], w[3], 1, 1, 1, st));
    if (side_early) RUN(side_level(3));
    RUN(conv(nc[6], {{bf.feat[3], 64, 64}}, bf.sa, 96, 96, nullptr, 0, 1, N2, h[3], w[3], 2, 1, 1, st));
    RUN(conv(nc[7], {{bf.sa, 96, 96}}, bf.feat[4], 96, 96, nullptr, 0, 1, N2, h[4], w[4], 1, 1, 1, st));
    if (side_early) RUN(side_level(4));
    RUN(conv(nc[8], {{bf.feat[4], 96, 96}}, bf.feat[5], 128, 128, nullptr, 0, 1, N2, h[4], w[4], 2, 1, 1, st));
    RUN(conv(nc[9], {{bf.feat[5], 128, 128}}, bf.feat[6], 192, 192, nullptr, 0, 1, N2, h[5], w[5], 2, 1, 1, st));
    // deepest first, the order the main stream wants the partial sums in; each R0a directly behind its level's 1 x 1 layers
    for (int L = 4; L >= net->lowest; --L)
        if (!side_early || (L == 1 && fused1)) RUN(side_level(L));
    // The side stream's 1x1 outputs (1.5 GB at 1024^2) pass through the Infinity Cache after NetC wrote the level-3 features and
    // push them out; the level-3 warp+correlation -- one tile per CU, nothing to overlap a miss with -- then gathers from HBM.  A
    // read-only pass over those features at the tail of the side stream (it runs beside levels 6-4, which use a fraction of the
    // chip) brings them back.  Nothing depends on it; it is joined at the end of the forward.
    bool touched = false;
    if (side != st && net->lowest <= 3 && !(PIV_KNOB(1) & 16384)) {
        RUN(launch_touch(bf.feat[3], (size_t)N2 * h[3] * w[3] * C_FEAT[3], bf.mean, side));
        PIV_CHECK_HIP(hipEventRecord(net->ev_join[6], side));      // joined at the very end of the forward (stream capture needs it)
        side_join.pending |= 1u << 6;
        touched = true;
    }

    float *prev = nullptr, *cur = bf.flowA;
    size_t lvoff = 0;
    for (int L = 6; L >= net->lowest; --L) {
        const LevelW &lw = net->lv[L];
        const int hh = h[L], ww = w[L], k = K_LEVEL[L], cm = C_MATCH[L], cf = C_FEAT[L];
        const size_t half = (size_t)B * hh * ww;
        const float *f1m = L <= 2 ? bf.ext[L] : bf.feat[L];
        const float *f2m = f1m + half * cm;
        const float *f1raw = bf.feat[L];
        const float *im1 = bf.img[L], *im2 = bf.img[L] + half * 4;
        const float sc = net->scale[L];
        const int s = L >= 4 ? 1 : 2;
        // fp16 mode: the hidden activations of this level's conv stacks are stored as fp16 (same size test as conv())
        const int h16 = (ctx.precision == 1 && (long)hh * ww >= 64 * 64) ? 1 : 0;
        // Join the side stream only where its results are first read: NetC_ext feeds Matching at levels <= 2, moduleFeat feeds
        // Regularization at levels 3 and 4.  (A cross-queue wait costs a barrier packet and a cold start for the next
        // kernel: in front of the level-3 warp+correlation it cost that launch 2 us.)
        if (L <= 2 && !(L == 1 && fused1)) { PIV_CHECK_HIP(hipStreamWaitEvent(st, net->ev_join[L], 0)); side_join.pending &= ~(1u << L); }
        // Every partial sum is joined before level 3 starts: its warp+correlation is one tile per CU, and beside a persistent R0a
        // launch a tile waits for a CU (14 -> 47 us).  The R0a launches fit the window of NetC's tail and levels 6-4 or nearly so;
        // what is left of them delays level 3 instead of slowing it.  tools A/B: 268435456 = each joined in front of its own tail pass
        // (one wait, for the launch that went last: the side stream runs them in order; the others are joined in front of their tails)
        if (!(PIV_KNOB(1) & 268435456) && L == 3 && (side_join.pending & (256u << last_part))) {
            PIV_CHECK_HIP(hipStreamWaitEvent(st, net->ev_pjoin[last_part], 0));
            side_join.pending &= ~(256u << last_part);
        }
        // ---- Matching (:165-187)
        const float *fup = nullptr;
        if (prev) {
            RUN(launch_dwconvT(prev, lw.upconv, bf.flow_up, B, h[L + 1], w[L + 1], 2, 4, 4, 4, st));
            fup = bf.flow_up;
        }
        const bool prof = net->prof_level == L && net->ev_used + 4 <= net->ev.size();
        if (net->prof_level == L && !prof) net->ev_dropped++;
        if (prof) {
            // (a) start/stop events attached to the dispatch itself; (b) a plain event pair around it (reported for reference)
            warp_corr_time_next(net->ev[net->ev_used], net->ev[net->ev_used + 1]);
            PIV_CHECK_HIP(hipEventRecord(net->ev[net->ev_used + 2], st));
        }
        RUN(launch_warp_corr(f1m, f2m, fup, sc, bf.corr, B, cm, hh, ww, s, 1, true, st));
        if (prof) {
            PIV_CHECK_HIP(hipEventRecord(net->ev[net->ev_used + 3], st));
            net->ev_used += 4;
        }
        const float *cin = bf.corr;
        if (s == 2) {
            RUN(launch_dwconvT(bf.corr, lw.upcorr, bf.corr_up, B, hh / 2, ww / 2, 49, 56, 56, 56, st));
            cin = bf.corr_up;
        }
        const float *hid = nullptr;       // output of the last hidden layer (32 channels)
        {
            const float *src = cin;
            int cprev = 0;
            for (int j = 0; j < net->nstack; ++j) {
                const int wd = net->width[j];
                float *dst = (j & 1) ? bf.t128b : bf.t128a;
                const int o16 = (j + 1 < net->nstack) ? h16 : 0;      // the flow head reads fp32
                if (j == 0) RUN(conv(lw.M[0], {{src, 52, 56}}, dst, wd, wd, nullptr, 0, 1, B, hh, ww, 1, 1, 1, st, 0, o16));
                else RUN(conv(lw.M[j], {{src, cprev, cprev}}, dst, wd, wd, nullptr, 0, 1, B, hh, ww, 1, 1, 1, st, h16, o16));
                src = dst;
                cprev = wd;
            }
            hid = src;
        }
        if (PIV_KNOB(1) & 1)    // A/B: heads on the matrix cores (30 of 32 output columns wasted)
            RUN(conv(lw.M[net->nstack], {{hid, 32, 32}}, bf.flowM, 4, 4, fup, 4, 0, B, hh, ww, 1, k / 2, k / 2, st));
        else
            RUN(launch_conv_head(hid, lw.headM, lw.hbM[0], lw.hbM[1], fup, bf.flowM, B, hh, ww, k, st));
        // ---- Subpixel (:209-217)
        RUN(launch_backwarp_nhwc(f2m, bf.flowM, sc, bf.f2w, B, hh, ww, cm, st));
        {
            const float *src = nullptr;
            int cprev = 0;
            for (int j = 0; j < net->nstack; ++j) {
                const int wd = net->width[j];
                float *dst = (j & 1) ? bf.t128b : bf.t128a;
                const int o16 = (j + 1 < net->nstack) ? h16 : 0;
                if (j == 0) RUN(conv(lw.S[0], {{f1m, cm, cm}, {bf.f2w, cm, cm}, {bf.flowM, 4, 4}}, dst, wd, wd, nullptr, 0, 1, B, hh, ww, 1, 1, 1, st, 0, o16));
                else RUN(conv(lw.S[j], {{src, cprev, cprev}}, dst, wd, wd, nullptr, 0, 1, B, hh, ww, 1, 1, 1, st, h16, o16));
                src = dst;
                cprev = wd;
            }
            hid = src;
        }
        if (PIV_KNOB(1) & 1)
            RUN(conv(lw.S[net->nstack], {{hid, 32, 32}}, bf.flowS, 4, 4, bf.flowM, 4, 0, B, hh, ww, 1, k / 2, k / 2, st));
        else
            RUN(launch_conv_head(hid, lw.headS, lw.hbS[0], lw.hbS[1], bf.flowM, bf.flowS, B, hh, ww, k, st));
        // ---- Regularization (:274-303); note it takes the RAW NetC feature (:361)
        RUN(launch_flow_mean(bf.flowS, bf.partial, nullptr, B, hh * ww, st));       // partial sums only: reg_prep finishes the mean
        RUN(launch_reg_prep(im1, im2, bf.flowS, bf.mean, bf.partial, sc, bf.misc4, B, hh, ww, st));
        if (L == 3 || L == 4) { PIV_CHECK_HIP(hipStreamWaitEvent(st, net->ev_join[L], 0)); side_join.pending &= ~(1u << L); }
        const float *fr = L < 5 ? bf.featR[L] : f1raw;
        const int cfr = L < 5 ? 128 : cf;
        if (split[L]) {
            // the tail of the split layer: the three flow-dependent channels, the bias, part[L], the LeakyReLU -- a streaming pass
            // (ops.hip).  Outside that kernel's grid range (more than 65535 pairs or 131070 rows), and under tools knob 512 for A/B runs,
            // the direct kernel with part[L] as its residual: one K chunk, nothing to split-K, and no scratch is offered.  (R0b comes
            // from pack_conv, which makes every family's packing of a layer; only the direct one is read.)
            if (side_join.pending & (256u << L)) { PIV_CHECK_HIP(hipStreamWaitEvent(st, net->ev_pjoin[L], 0)); side_join.pending &= ~(256u << L); }
            if (lw.r0t && reg_r0_tail_supports(B, hh, ww) && !(PIV_KNOB(1) & 512)) {
                RUN(launch_reg_r0_tail(bf.misc4, lw.r0t, lw.R0b.bias, bf.part[L], bf.t128a, B, hh, ww, st));
            } else {
                const ConvCtx tail_ctx{ctx.precision, ctx.no_b3, nullptr, ctx.side, 0};
                const ConvSeg sm{bf.misc4, 4, 4};
                RUN(pivlfn::conv(tail_ctx, lw.R0b, conv_call(&sm, 1, bf.t128a, 128, 128, bf.part[L], 128, 1, B, hh, ww, 1, 1, 1), st));
            }
        } else {
            RUN(conv(lw.R[0], {{fr, cfr, cfr}, {bf.misc4, 4, 4}}, bf.t128a, 128, 128, nullptr, 0, 1, B, hh, ww, 1, 1, 1, st, 0, h16));
        }
        RUN(conv(lw.R[1], {{bf.t128a, 128, 128}}, bf.t128b, 128, 128, nullptr, 0, 1, B, hh, ww, 1, 1, 1, st, h16, h16));
        RUN(conv(lw.R[2], {{bf.t128b, 128, 128}}, bf.t64a, 64, 64, nullptr, 0, 1, B, hh, ww, 1, 1, 1, st, h16, h16));
        RUN(conv(lw.R[3], {{bf.t64a, 64, 64}}, bf.t64b, 64, 64, nullptr, 0, 1, B, hh, ww, 1, 1, 1, st, h16, h16));
        RUN(conv(lw.R[4], {{bf.t64b, 64, 64}}, bf.t32a, 32, 32, nullptr, 0, 1, B, hh, ww, 1, 1, 1, st, h16, h16));
        RUN(conv(lw.R[5], {{bf.t32a, 32, 32}}, bf.t32b, 32, 32, nullptr, 0, 1, B, hh, ww, 1, 1, 1, st, h16, h16));
        const int kk = k * k, kkp = rup(kk, 4);
        if (L < 5) {     // (k x 1) then (1 x k), no activation in between (:253-261); d1 and dist stay fp32
            RUN(conv(lw.dist0, {{bf.t32b, 32, 32}}, bf.d1, kkp, kkp, nullptr, 0, 0, B, hh, ww, 1, k / 2, 0, st, h16, 0));
            RUN(conv(lw.dist1, {{bf.d1, kkp, kkp}}, bf.dist, kkp, kkp, nullptr, 0, 0, B, hh, ww, 1, 0, k / 2, st));
        } else {
            RUN(conv(lw.dist0, {{bf.t32b, 32, 32}}, bf.dist, kkp, kkp, nullptr, 0, 0, B, hh, ww, 1, k / 2, k / 2, st, h16, 0));
        }
        const bool last = L == net->lowest;
        RUN(launch_reg_tail(bf.dist, kkp, bf.flowS, lw.wx, lw.wy, lw.bx, lw.by, k, cur, last ? flow : nullptr,
                            net->scale[1], B, hh, ww, st));
        if (levels) {
            RUN(launch_flow4_to_nchw(bf.flowM, levels + lvoff, B, hh, ww, st)); lvoff += half * 2;
            RUN(launch_flow4_to_nchw(bf.flowS, levels + lvoff, B, hh, ww, st)); lvoff += half * 2;
            RUN(launch_flow4_to_nchw(cur, levels + lvoff, B, hh, ww, st)); lvoff += half * 2;
        }
        prev = cur;
        cur = (cur == bf.flowA) ? bf.flowB : bf.flowA;
    }
    if (touched) { PIV_CHECK_HIP(hipStreamWaitEvent(st, net->ev_join[6], 0)); side_join.pending &= ~(1u << 6); }
#undef RUN
    return PIVLFN_OK;
}

// ---- per-layer checks of the level-pipeline ops that have no layer of their own (pivlfn_upconv_nhwc, pivlfn_conv1_fused_nhwc) -------
// Host weights are packed by the network's own packers and uploaded per call; the call synchronises `st` before it frees them.
int upconv_forward(const float *in, const float *w, float *out, int B, int H, int W, int quads, int stride_in, int stride_out,
                   hipStream_t st)
{
    PIV_REQUIRE(in && w && out, "upconv: null argument");
    PIV_REQUIRE(quads == 1 || quads == 14, "upconv: quads=%d (1 = flow, 2 channels; 14 = correlation, 49 channels)", quads);
    PIV_REQUIRE(B > 0 && H > 0 && W > 0, "upconv: B=%d H=%d W=%d must be positive", B, H, W);
    PIV_REQUIRE(stride_in % 4 == 0 && stride_in >= 4 * quads && stride_out % 4 == 0 && stride_out >= 4 * quads,
                "upconv: strides %d / %d must be multiples of 4 and >= %d", stride_in, stride_out, 4 * quads);
    PIV_REQUIRE(2 * (long)H <= 65535 && B <= 65535, "upconv: %ld output rows / %d images exceed the grid range", 2 * (long)H, B);
    PIV_REQUIRE((long)2 * (W + 1) * quads < (1L << 30) && (long)B * 2 * H < (1L << 31),
                "upconv: B=%d H=%d W=%d exceed the kernel's 32-bit index range", B, H, W);
    const int C = quads == 1 ? 2 : 49, cpad = 4 * quads;
    std::vector<float> h;
    pack_dw_host(w, C, cpad, h);
    pivlfn_net *owner = new pivlfn_net();
    float *dw = nullptr;
    int rc = upload(owner, h, &dw);
    if (!rc) rc = launch_dwconvT(in, dw, out, B, H, W, C, stride_in, stride_out, cpad, st);
    if (hipStreamSynchronize(st) != hipSuccess && !rc) { set_error("upconv: hipStreamSynchronize failed"); rc = PIVLFN_ERR_HIP; }
    net_destroy(owner);
    return rc;
}

int conv1_fused_forward(const float *w1, const float *b1, const float *we, const float *be, const float *wf, const float *bfe,
                        const float *x, float *out, float *out_ext, float *out_feat, int N, int H, int W, int B_feat, int *fused,
                        hipStream_t st)
{
    PIV_REQUIRE(w1 && b1 && we && be && wf && bfe && x && out && out_ext && out_feat, "conv1_fused: null argument");
    PIV_REQUIRE(N > 0 && H > 0 && W > 0 && B_feat >= 1 && B_feat <= N, "conv1_fused: N=%d H=%d W=%d B_feat=%d (1 <= B_feat <= N)", N, H, W, B_feat);
    PIV_REQUIRE((long)N * H < (1L << 31) && (long)H * W < (1L << 31), "conv1_fused: N=%d H=%d W=%d exceed the 32-bit index range", N, H, W);
    if (fused) *fused = 0;
    pivlfn_net *owner = new pivlfn_net();
    ConvW c1, ext, feat;
    std::vector<float> w11, b11;
    pack_conv1_fuse(we, be, wf, bfe, w11, b11);
    float *dw11 = nullptr, *db11 = nullptr;
    int rc = pack_conv(owner, "c1", w1, b1, 32, 3, 7, 7, {{3, 4}}, &c1);
    if (!rc) rc = pack_conv(owner, "ext", we, be, 64, 32, 1, 1, {{32, 32}}, &ext);
    if (!rc) rc = pack_conv(owner, "feat", wf, bfe, 128, 32, 1, 1, {{32, 32}}, &feat);
    if (!rc) rc = upload(owner, w11, &dw11);
    if (!rc) rc = upload(owner, b11, &db11);
    if (!rc) {      // net_forward's level-1 path in the fp32 modes, on one stream and without split-K
        const ConvCtx ctx{0, false, nullptr, nullptr};
        const ConvSeg sx{x, 4, 4}, so{out, 32, 32};
        const ConvCall call1 = conv_call(&sx, 1, out, 32, 32, nullptr, 0, 1, N, H, W, 1, 3, 3);
        const ConvParams p1 = conv_params(c1, call1);
        const Conv1Fuse f1{dw11, db11, out_ext, out_feat, B_feat};
        const int rc1 = launch_conv1_fused(p1, f1, st);
        if (rc1 > 0) rc = rc1;
        else if (rc1 == 0) { if (fused) *fused = 1; }
        else {
            rc = conv(ctx, c1, call1, st);
            if (!rc) rc = conv(ctx, feat, conv_call(&so, 1, out_feat, 128, 128, nullptr, 0, 1, B_feat, H, W, 1, 0, 0), st);
            if (!rc) rc = conv(ctx, ext, conv_call(&so, 1, out_ext, 64, 64, nullptr, 0, 1, N, H, W, 1, 0, 0), st);
        }
    }
    if (hipStreamSynchronize(st) != hipSuccess && !rc) { set_error("conv1_fused: hipStreamSynchronize failed"); rc = PIVLFN_ERR_HIP; }
    net_destroy(owner);
    return rc;
}

}  // namespace pivlfn
