#!/usr/bin/env python3
"""A/B micro-benchmarks of single kernels at the shapes of the 1024x1024 PIV forward (one process, interleaved rounds).

  python tools/bench_ops.py warp_corr [--batch 1] [--variants 0,8,9]   (0 shipped policy, 8 v7, 9 v6)
  python tools/bench_ops.py twopoint                                  (pivlfn_twopoint_accumulate against its HBM and fp64 bounds)
  python tools/bench_ops.py distribution                              (pivlfn_flow_hist_accumulate and _moments_accumulate against torch.bincount / elementwise torch)
  python tools/bench_ops.py spectrum                                  (pivlfn_spectrum_accumulate, and the same sums from snapshot_project + torch)
  python tools/bench_ops.py pressure                                  (pivlfn_pressure_cg: us per iteration at 256^2 x 8 and 1024^2 x 1)
  python tools/bench_ops.py calibrate                                 (pivlfn_template_match, _target_points, _dewarp_frames at --size squared)
  python tools/bench_ops.py ensemble                                  (pivlfn_ensemble_corr, 8 frames at --size squared, against its integer-MAC bound)
Times N back-to-back launches between two events on the current stream (so each figure includes one ~1.5 us
kernel boundary) and checks that all variants agree.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "piv_liteflownet-pytorch_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _toolslib  # noqa: E402


def _chk(rc, what=""):
    _toolslib.check(_toolslib.load(), rc, what)


LEVELS = {1: (64, 1024, 2), 2: (64, 512, 2), 3: (64, 256, 2), 4: (96, 128, 1), 5: (128, 64, 1), 6: (192, 32, 1)}


def time_it(fn, n=50, rounds=5):
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / n * 1e3)
    return min(ts), sorted(ts)[len(ts) // 2]


def bench_warp_corr(args):
    lib = _toolslib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    B = args.batch
    variants = [int(v) for v in (args.variants or "0,8,9").split(",")]
    for L in [int(x) for x in args.levels.split(",")]:
        C, n, s = LEVELS[L]
        n = n * args.size // 1024
        vs = [v for v in variants if not (v == 8 and C % 64)]          # v7 needs whole 64-channel groups (not level 4's C = 96)
        f1 = torch.randn(B, n, n, C, device=dev)
        f2 = torch.randn(B, n, n, C, device=dev)
        fl = torch.zeros(B, n, n, 4, device=dev)
        fl[..., :2] = torch.randn(B, n, n, 2, device=dev) * 0.8
        no = -(-n // s)
        flow_ptr = fl.data_ptr() if L < 6 else None
        outs = {}
        alg = 4 * B * (C * no * no + C * n * n + (2 * n * n if L < 6 else 0) + 49 * no * no)
        fns = {}
        for v in vs:
            out = torch.empty(B, no, no, 56, device=dev)
            outs[v] = out

            def fn(v=v, out=out):
                lib.pivlfn_tune(0, v)
                _chk(lib.pivlfn_warp_corr_nhwc(f1.data_ptr(), f2.data_ptr(), flow_ptr, 1.25, out.data_ptr(), B, C, n, n, s, 1, st), "wc")
            fns[v] = fn
        # interleaved rounds (clock state and neighbours are shared by all variants): min / median over the rounds
        times = {v: [] for v in vs}
        for _ in range(3):
            for v in vs:
                fns[v]()
        for rnd in range(args.rounds):
            for v in (vs if rnd % 2 == 0 else vs[::-1]):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                fns[v]()
                torch.cuda.synchronize()
                a.record()
                for _ in range(50):
                    fns[v]()
                b.record()
                torch.cuda.synchronize()
                times[v].append(a.elapsed_time(b) / 50 * 1e3)
        for v in vs:
            tmin, tmed = min(times[v]), sorted(times[v])[len(times[v]) // 2]
            print(f"L{L} B={B} C={C} {n}x{n} s={s} variant {v}: min {tmin:8.2f} us  med {tmed:8.2f} us   "
                  f"{alg / tmin / 1e3:8.1f} GB/s algorithmic ({alg / 1e6:.2f} MB)", flush=True)
        ref = outs[vs[0]]
        for v in vs[1:]:
            d = (outs[v] - ref).abs().max().item()
            print(f"    variant {v} vs {vs[0]}: max abs diff {d:.3e}")
    lib.pivlfn_tune(0, 0)


def bench_wc_ablate(args):
    """Ablation of the shipped warp+correlation kernel (mask bits: 1 no dot products, 2 no gathers, 4 no store, 8 empty)."""
    lib = _toolslib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    B = args.batch
    for L in [int(x) for x in args.levels.split(",")]:
        C, n, s = LEVELS[L]
        f1 = torch.randn(B, n, n, C, device=dev)
        f2 = torch.randn(B, n, n, C, device=dev)
        fl = torch.zeros(B, n, n, 4, device=dev)
        if args.smooth:      # a smooth sub-pixel flow, as the network's own are (bench.py's roofline_batch8 uses the same): every byte of f2 is touched
            yy, xx = torch.meshgrid(torch.arange(n, device=dev, dtype=torch.float32), torch.arange(n, device=dev, dtype=torch.float32), indexing="ij")
            ph = torch.arange(B, device=dev, dtype=torch.float32).view(B, 1, 1)
            fl[..., 0] = 0.8 * torch.sin(yy * (6.2832 * 3 / n) + ph)
            fl[..., 1] = 0.8 * torch.cos(xx * (6.2832 * 2 / n) + 0.5 * ph)
        else:
            fl[..., :2] = torch.randn(B, n, n, 2, device=dev) * 0.8
        no = -(-n // s)
        out = torch.empty(B, no, no, 56, device=dev)
        for mask in [int(m) for m in args.masks.split(",")]:
            def fn():
                _chk(lib.pivlfn_warp_corr_nhwc(f1.data_ptr(), f2.data_ptr(), fl.data_ptr() if L < 6 else None, 1.25, out.data_ptr(), B, C, n, n, s, 1, st), "wc")
            lib.pivlfn_tune(2, mask)
            tmin, tmed = time_it(fn)
            print(f"L{L} B={B} ablation mask {mask}: min {tmin:8.2f} us  med {tmed:8.2f} us", flush=True)
        lib.pivlfn_tune(2, 0)


def _level_layers(L, n):
    """Every dense conv of level L's Matching / Subpixel / Regularization stacks (src/models.py:154-163, 197-207, 236-267) at
    the level's resolution n x n; staged input channels (multiples of 4) as pivlfn_forward stages them."""
    return [(f"L{L} M.0 49->128", 128, 56, 3, 1, n, 1), (f"L{L} M.2 128->64", 64, 128, 3, 1, n, 1), (f"L{L} M.4 64->32", 32, 64, 3, 1, n, 1),
            (f"L{L} S.0 130->128", 128, 136, 3, 1, n, 1), (f"L{L} S.2 128->64", 64, 128, 3, 1, n, 1), (f"L{L} S.4 64->32", 32, 64, 3, 1, n, 1),
            (f"L{L} R.0 131->128", 128, 132, 3, 1, n, 1), (f"L{L} R.2 128->128", 128, 128, 3, 1, n, 1), (f"L{L} R.4 128->64", 64, 128, 3, 1, n, 1),
            (f"L{L} R.6 64->64", 64, 64, 3, 1, n, 1), (f"L{L} R.8 64->32", 32, 64, 3, 1, n, 1), (f"L{L} R.10 32->32", 32, 32, 3, 1, n, 1)]


CONV_SHAPES = _level_layers(1, 1024) + _level_layers(2, 512) + _level_layers(3, 256) + [
    # name, cout, cin, k, stride, H(=W) at the 1024x1024 PIV forward, batch multiplier
    ("L3 conv 128->128", 128, 128, 3, 1, 256, 1),
    ("L4 conv 128->128", 128, 128, 3, 1, 128, 1), ("L5 conv 128->128", 128, 128, 3, 1, 64, 1), ("L6 conv 128->128", 128, 128, 3, 1, 32, 1),
    ("L6 S.conv_S.0 386->128", 128, 392, 3, 1, 32, 1), ("L5 S.conv_S.0 258->128", 128, 264, 3, 1, 64, 1),
    ("NetC.conv1 7x7 3->32", 32, 4, 7, 1, 1024, 2), ("NetC.conv2.0 s2 32->32", 32, 32, 3, 2, 1024, 2),
    ("NetC.conv2.2 32->32 @512", 32, 32, 3, 1, 512, 2), ("NetC.conv3.0 s2 32->64", 64, 32, 3, 2, 512, 2),
    ("NetC.conv3.2 64->64 @256", 64, 64, 3, 1, 256, 2), ("NetC.conv5.0 s2 96->128", 128, 96, 3, 2, 128, 2),
    ("L1 moduleFeat 1x1 32->128", 128, 32, 1, 1, 1024, 1), ("L1 NetC_ext 1x1 32->64", 64, 32, 1, 1, 1024, 2),
    ("L1 dist 7x1 32->49", 49, 32, (7, 1), 1, 1024, 1),
    ("L1 dist 1x7 49->49", 49, 49, (1, 7), 1, 1024, 1),
    ("L2 dist 7x1 32->49", 49, 32, (7, 1), 1, 512, 1), ("L2 dist 1x7 49->49", 49, 49, (1, 7), 1, 512, 1),
]


def bench_conv(args):
    import ctypes
    lib = _toolslib.load()
    lib.pivlfn_tune(3, args.tune3)
    lib.pivlfn_tune(7, args.tune7)
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    variants = [int(v) for v in (args.variants or "6,8,5").split(",")]
    for name, co, ci, k, s, n, bm in CONV_SHAPES:
        if args.filter and args.filter not in name:
            continue
        kh, kw = (k, k) if isinstance(k, int) else k
        B = args.batch * bm
        w = (torch.randn(co, ci, kh, kw) / (ci * kh * kw) ** 0.5).contiguous()
        b = torch.randn(co).contiguous()
        h = ctypes.c_void_p()
        _chk(lib.pivlfn_conv_create(w.data_ptr(), b.data_ptr(), co, ci, kh, kw, ctypes.byref(h)), "create")
        xs = -(-ci // 4) * 4                      # stored lanes of the input (zeros behind the real channels)
        x = torch.randn(B, n, n, xs, device=dev)
        x[..., ci:] = 0
        no = (n + 2 * (kh // 2) - kh) // s + 1
        mo = (n + 2 * (kw // 2) - kw) // s + 1
        ys = -(-co // 4) * 4
        flop = 2.0 * B * no * mo * co * ci * kh * kw
        outs = {}
        xh = None
        for v in variants:
            # variants >= 100000 select the fp16-multiplicand kernel: even = fp32 in / fp32 out, odd = fp16 in / fp16 out;
            # (v - 100000) >> 1 goes to the tuning knob (pivlfn_tune(1, .)): 100000/100001 shipped policy, 100128/100129 = knob 64
            # variants >= 2000000: the split-operand fp32 kernel (conv_split.hip), stride-1 layers only; 2xxxxxx = six terms,
            # 3xxxxxx = three terms; v % 1000000 goes to the knob
            split = v >= 2000000
            if split and not (s == 1 or (s == 2 and v >= 3000000 and kh == 3 and kw == 3)):
                continue
            f16io = 100000 <= v < 2000000 and (v & 1) == 1
            y = torch.empty(B, no, mo, ys, device=dev, dtype=torch.float16 if f16io else torch.float32)
            outs[v] = y
            if f16io and xh is None and ci % 8 == 0:
                xh = x.half()

            def fn(v=v, y=y, f16io=f16io):
                lib.pivlfn_tune(1, (v % 1000000) if split else ((v - 100000) >> 1 if v >= 100000 else v))
                if split:
                    _chk(lib.pivlfn_conv2d_nhwc_split(h, x.data_ptr(), xs, y.data_ptr(), ys, B, n, n, s, kh // 2, kw // 2, 1, 3 if v >= 3000000 else 6, st), "conv")
                elif v >= 100000:
                    if f16io and ci % 8 == 0:
                        _chk(lib.pivlfn_conv2d_nhwc_f16(h, xh.data_ptr(), ci, 1, y.data_ptr(), ys, 1, B, n, n, s, kh // 2, kw // 2, 1, st), "conv")
                    else:
                        _chk(lib.pivlfn_conv2d_nhwc_f16(h, x.data_ptr(), xs, 0, y.data_ptr(), ys, 1 if f16io else 0, B, n, n, s, kh // 2, kw // 2, 1, st), "conv")
                else:
                    _chk(lib.pivlfn_conv2d_nhwc(h, x.data_ptr(), xs, y.data_ptr(), ys, None, 0, B, n, n, s, kh // 2, kw // 2, 1, st), "conv")
            tmin, tmed = time_it(fn, n=10 if flop > 2e10 else 30, rounds=4)
            print(f"{name:28s} B={B} variant {v}: min {tmin:9.1f} us  med {tmed:9.1f} us  {flop / tmin / 1e6:7.1f} TFLOP/s (staged K)", flush=True)
        for v in variants[1:]:
            if v not in outs or variants[0] not in outs:
                continue
            d = (outs[v].float() - outs[variants[0]].float()).abs().max().item()
            print(f"    variant {v} vs {variants[0]}: max abs diff {d:.3e}")
        lib.pivlfn_conv_destroy(h)
    lib.pivlfn_tune(1, 0)


def bench_conv_stamps(args):
    """Phase times of the fp16 conv kernel (wave 0 of every workgroup, s_memtime ticks): where a workgroup's time goes."""
    import ctypes
    lib = _toolslib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    for name, co, ci, k, s, n, bm in CONV_SHAPES:
        if args.filter and args.filter not in name:
            continue
        kh, kw = (k, k) if isinstance(k, int) else k
        B = args.batch * bm
        w = (torch.randn(co, ci, kh, kw) / (ci * kh * kw) ** 0.5).contiguous()
        b = torch.randn(co).contiguous()
        h = ctypes.c_void_p()
        _chk(lib.pivlfn_conv_create(w.data_ptr(), b.data_ptr(), co, ci, kh, kw, ctypes.byref(h)), "create")
        fp32 = args.tune3 == -1                     # --tune3 -1: stamp the fp32 kernel instead
        f16 = ci % 8 == 0 and not fp32
        x = torch.randn(B, n, n, ci, device=dev)
        xin = x.half() if f16 else x
        no = (n + 2 * (kh // 2) - kh) // s + 1
        mo = (n + 2 * (kw // 2) - kw) // s + 1
        ys = -(-co // 4) * 4
        y = torch.empty(B, no, mo, ys, device=dev, dtype=torch.float32 if fp32 else torch.float16)
        stamps = torch.zeros(65536 * 8, dtype=torch.int64, device=dev)
        ptr = stamps.data_ptr()

        def run():
            if fp32:
                _chk(lib.pivlfn_conv2d_nhwc(h, x.data_ptr(), ci, y.data_ptr(), ys, None, 0, B, n, n, s, kh // 2, kw // 2, 1, st), "conv")
            else:
                _chk(lib.pivlfn_conv2d_nhwc_f16(h, xin.data_ptr(), ci, 1 if f16 else 0, y.data_ptr(), ys, 1, B, n, n, s, kh // 2, kw // 2, 1, st), "conv")
        for _ in range(3):
            run()
        lib.pivlfn_tune(5, ctypes.c_int32(ptr & 0xFFFFFFFF).value)
        lib.pivlfn_tune(6, ctypes.c_int32((ptr >> 32) & 0xFFFFFFFF).value)
        run()
        torch.cuda.synchronize()
        lib.pivlfn_tune(5, 0)
        lib.pivlfn_tune(6, 0)
        t = stamps.view(-1, 8).cpu().numpy()
        t = t[t[:, 6] > 0]
        names = ["commit+wait", "barrier1", "load issue", "tap loop", "barrier2", "epilogue", "whole"]
        tot = t[:, 6].mean()
        print(f"{name}: {len(t)} workgroups, ticks per workgroup (mean): " +
              "  ".join(f"{nm} {t[:, i].mean():.0f} ({100 * t[:, i].mean() / tot:.0f}%)" for i, nm in enumerate(names)))
        span = (t[:, 7] + t[:, 6]).max() - t[:, 7].min()
        print(f"    kernel span {span} ticks; per-workgroup whole min {t[:, 6].min()} max {t[:, 6].max()}")
        lib.pivlfn_conv_destroy(h)


def bench_head(args):
    """The 32 -> 2 k x k flow heads (conv_M.6 / conv_S.6) at the fine levels: knob 524288 + 8192 = one pixel per lane (round 1),
    524288 = four rows per lane (round 2), 0 = shipped (7 x 7 on >= 256 x 256 images: the matrix-core formulation)."""
    import ctypes
    lib = _toolslib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    for name, n, k in (("L1 head 7x7", 1024, 7), ("L2 head 7x7", 512, 7), ("L3 head 5x5", 256, 5)):
        n = n * args.size // 1024
        B = args.batch
        w = (torch.randn(2, 32, k, k) / (32 * k * k) ** 0.5).contiguous()
        b = torch.randn(2).contiguous()
        h = ctypes.c_void_p()
        _chk(lib.pivlfn_conv_create(w.data_ptr(), b.data_ptr(), 2, 32, k, k, ctypes.byref(h)), "create")
        x = torch.randn(B, n, n, 32, device=dev)
        res = torch.randn(B, n, n, 4, device=dev)
        outs = {}
        for v in (524288 + 8192, 524288, 0):
            y = torch.empty(B, n, n, 4, device=dev)
            outs[v] = y

            def fn(v=v, y=y):
                lib.pivlfn_tune(1, v)
                _chk(lib.pivlfn_conv_head_nhwc(h, x.data_ptr(), res.data_ptr(), y.data_ptr(), B, n, n, st), "head")
            tmin, tmed = time_it(fn, n=20, rounds=4)
            flop = 2.0 * B * n * n * 2 * 32 * k * k
            print(f"{name} B={B} {n}x{n} knob {v}: min {tmin:8.1f} us  med {tmed:8.1f} us  {flop / tmin / 1e6:6.1f} TFLOP/s", flush=True)
        want = torch.nn.functional.conv2d(x[:1].permute(0, 3, 1, 2).double().cpu(), w.double(), b.double(), padding=k // 2).permute(0, 2, 3, 1)
        want = want + res[:1, ..., :2].double().cpu()
        for v in (524288 + 8192, 524288, 0):
            err = (outs[v][:1, ..., :2].double().cpu() - want).abs().max().item() / want.abs().max().item()
            pad = outs[v][..., 2:].abs().max().item()
            print(f"    knob {v}: max rel err vs float64 conv {err:.2e}, padding lanes max {pad:.1e}")
        lib.pivlfn_conv_destroy(h)
    lib.pivlfn_tune(1, 0)


HBM_BYTES_PER_S = 8.0e12      # the MI355X's HBM peak the shares below refer to


def preproc_hbm_bound_us(n, H, W, background):
    """The time the algorithmic traffic of pivlfn_frames_preprocess takes at the HBM peak: 3 bytes per pixel read (6 with a
    background, counted once per frame) and 12 written."""
    return ((6 if background else 3) + 12) * n * H * W / HBM_BYTES_PER_S * 1e6


def bench_preproc(args):
    """pivlfn_frames_preprocess (csrc/preproc.hip) on particle-like frames with a background: n = 2 and 16 frames of --size squared,
    k = 0, 15, 31; and pivlfn_frames_background_min over 16 frames.  Beside each time its share of the HBM bound.  `--once`: one
    launch per shape and nothing else, for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/bench_ops.py preproc
    --once)."""
    from pivlfn import _lib
    lib = _lib.load()                      # no knobs: the production library
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    S = args.size
    g = torch.Generator().manual_seed(1)
    sparse = (torch.rand(16, S, S, 3, generator=g) < 0.05).to(torch.uint8) * torch.randint(60, 200, (16, S, S, 3), generator=g, dtype=torch.uint8)
    bg = torch.randint(0, 56, (S, S, 3), generator=g, dtype=torch.uint8)
    frames = (sparse + bg[None]).to(dev)
    bg = bg.to(dev)
    for n in (2, 16):
        out = torch.empty(n, 3, S, S, device=dev)
        for k in (0, 15, 31):
            def fn(k=k, n=n, out=out):
                _lib.check(lib.pivlfn_frames_preprocess(frames.data_ptr(), bg.data_ptr(), out.data_ptr(), n, S, S, k, 16, st), "preproc")
            bound = preproc_hbm_bound_us(n, S, S, True)
            if args.once:
                fn()
                torch.cuda.synchronize()
                print(f"preprocess n={n:2d} {S}x{S} k={k:2d}: HBM bound {bound:7.1f} us", flush=True)
                continue
            tmin, tmed = time_it(fn, n=20, rounds=5)
            print(f"preprocess n={n:2d} {S}x{S} k={k:2d}: min {tmin:8.1f} us  med {tmed:8.1f} us  {tmed / n:7.1f} us/frame  "
                  f"HBM bound {bound:7.1f} us = {100 * bound / tmed:5.1f} % of the time", flush=True)
    acc = torch.full((S, S, 3), 255, dtype=torch.uint8, device=dev)

    def fn_bg():
        _lib.check(lib.pivlfn_frames_background_min(frames.data_ptr(), acc.data_ptr(), 16, S, S, st), "background_min")
    bound = (16 * 3 + 6) * S * S / HBM_BYTES_PER_S * 1e6
    if args.once:
        fn_bg()
        torch.cuda.synchronize()
        print(f"background_min n=16 {S}x{S}: HBM bound {bound:7.1f} us", flush=True)
    else:
        tmin, tmed = time_it(fn_bg, n=20, rounds=5)
        print(f"background_min n=16 {S}x{S}: min {tmin:8.1f} us  med {tmed:8.1f} us  HBM bound {bound:7.1f} us = "
              f"{100 * bound / tmed:5.1f} % of the time", flush=True)


def bench_evaluate(args):
    """pivlfn_flow_errors at 8 x --size squared, k = 0 (with and without the error map), pivlfn_level_errors on the piv pyramid (levels
    6..1, three stages each) and pivlfn_error_stats_accumulate, on the production library.  Beside each time the share of it that
    the bytes it must move take at the HBM peak: 8 B of truth and 8 B of flow per pixel (level_errors: the flows of all levels and
    stages, 3 x 4/3 x 8 B per pixel; the error map adds 12 B; error_stats reads and writes 48 B of sums per pixel and call)."""
    from pivlfn import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    B, S = 8, args.size
    truth = torch.randn(B, 2, S, S, device=dev)
    flow = truth + 0.1 * torch.randn(B, 2, S, S, device=dev)
    levels = torch.randn(sum(3 * B * 2 * (S >> k) * (S >> k) for k in range(6)), device=dev)
    nws = lib.pivlfn_flow_errors_workspace_bytes(B, S, S)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    sums = torch.empty(B, 6, 3, 7, dtype=torch.float64, device=dev)
    emap = torch.empty(B, 3, S, S, device=dev)
    acc = torch.zeros(6, S, S, dtype=torch.float64, device=dev)
    px = B * S * S

    def fe(m):
        _lib.check(lib.pivlfn_flow_errors(flow.data_ptr(), truth.data_ptr(), None, B, S, S, 0, 1.0, sums.data_ptr(), m, ws.data_ptr(), nws, st),
                   "flow_errors")

    def le():
        _lib.check(lib.pivlfn_level_errors(levels.data_ptr(), 1, truth.data_ptr(), None, B, S, S, 0.2, sums.data_ptr(), ws.data_ptr(), nws, st),
                   "level_errors")

    def es():
        _lib.check(lib.pivlfn_error_stats_accumulate(flow.data_ptr(), truth.data_ptr(), None, acc.data_ptr(), B, S, S, st), "error_stats")
    for name, fn, nbytes in (("flow_errors k=0", lambda: fe(None), 16 * px), ("flow_errors k=0 + err_map", lambda: fe(emap.data_ptr()), 28 * px),
                             ("level_errors piv (18 flows)", le, 8 * px + 4 * levels.numel()),
                             ("error_stats_accumulate", es, 16 * px + 96 * S * S)):
        bound = nbytes / HBM_BYTES_PER_S * 1e6
        tmin, tmed = time_it(fn, n=20, rounds=5)
        print(f"{name:28s} B={B} {S}x{S}: min {tmin:8.1f} us  med {tmed:8.1f} us  HBM bound {bound:7.1f} us = "
              f"{100 * bound / tmed:5.1f} % of the time", flush=True)


FP64_VECTOR_FLOP_PER_S = 78.6e12      # half the MI355X's fp32 vector peak of 157.3 TFLOP/s, an fma counted as two operations


def bench_twopoint(args):
    """pivlfn_twopoint_accumulate (csrc/twopoint.hip) at 8 x --size squared, R = 64, step 1, with and without a mask, on the production
    library.  Beside the median time per frame two bounds: the bytes of the frame (and its mask) read once at the HBM peak, and the
    arithmetic at the fp64 vector peak -- 2 * 65 * 15 * H * W additions of the trees plus as many products and differences, counted
    as the contract counts them (the contract forbids fma, so a kernel can reach half that peak at the most)."""
    from pivlfn import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    B, S, R = 8, args.size, 64
    g = torch.Generator().manual_seed(2)
    flow = torch.randn(B, 2, S, S, generator=g).to(dev)
    mask = (torch.rand(B, S, S, generator=g) < 0.05).to(torch.uint8).to(dev)
    acc = torch.zeros(2, R + 1, 15, S, dtype=torch.float64, device=dev)
    flops = 2 * (2 * (R + 1) * 15 * S * S)
    for name, m in (("no mask", None), ("mask", mask)):
        def fn(m=m):
            _lib.check(lib.pivlfn_twopoint_accumulate(flow.data_ptr(), m.data_ptr() if m is not None else None, None, acc.data_ptr(), B, S, S,
                                                      R, 1, st), "twopoint_accumulate")
        tmin, tmed = time_it(fn, n=5, rounds=7)
        hbm = (8 + (1 if m is not None else 0)) * S * S / HBM_BYTES_PER_S * 1e6
        alu = flops / FP64_VECTOR_FLOP_PER_S * 1e6
        print(f"twopoint_accumulate {name:7s} B={B} {S}x{S} R={R}: min {tmin:9.1f} us  med {tmed:9.1f} us  {tmed / B:8.1f} us/frame  "
              f"HBM bound {hbm:5.2f} us/frame = {100 * hbm * B / tmed:5.2f} %  fp64 bound {alu:6.1f} us/frame = {100 * alu * B / tmed:5.2f} % of the time",
              flush=True)


def _torch_hist(flow, lo, hi, nbins, jbins, fbins):
    """What a user writes without the kernel: the histograms of pivlfn_flow_hist_accumulate from torch.bincount on fp64 copies, no mask,
    mean or scale.  Returns the words in the layout of include/pivlfn.h."""
    u, v = flow[:, 0].reshape(-1).double(), flow[:, 1].reshape(-1).double()
    ok = (u.abs() <= 1e9) & (v.abs() <= 1e9)
    u, v = u[ok], v[ok]

    def slots(x, n):
        t = (x - lo) * (n / (hi - lo))
        return t, torch.where(t < 0, 0, torch.where(t < n, 1 + t.clamp(0, n - 1).long(), n + 1))
    parts = [torch.bincount(slots(u, nbins)[1], minlength=nbins + 2), torch.bincount(slots(v, nbins)[1], minlength=nbins + 2)]
    tu, tv = slots(u, jbins)[0], slots(v, jbins)[0]
    inside = (tu >= 0) & (tu < jbins) & (tv >= 0) & (tv < jbins)
    parts.append(torch.bincount(tv[inside].long() * jbins + tu[inside].long(), minlength=jbins * jbins))
    parts.append((~inside).sum().reshape(1))
    for d in (u, v):
        parts.append(torch.bincount(((d - d.floor()) * fbins).long().clamp(max=fbins - 1), minlength=fbins))
    parts.append(torch.stack([ok.sum(), (~ok).sum()]))
    return torch.cat(parts)


def _torch_moments(flow, acc):
    """The 21 sums of pivlfn_flow_moments_accumulate from elementwise torch operations, frame by frame, no mask, mean or thr."""
    for b in range(flow.size(0)):
        U, V = flow[b, 0].double(), flow[b, 1].double()
        ok = (U.abs() <= 1e9) & (V.abs() <= 1e9)
        uu, vv, P = U * U, V * V, U * V
        terms = [torch.ones_like(U), U, V, uu, vv, P, uu * U, vv * V, uu * V, vv * U, uu * uu, vv * vv, uu * vv]
        event = ok & (P.abs() > 0)
        quads = [event & (U > 0) & (V > 0), event & (U < 0) & (V > 0), event & (U < 0) & (V < 0), event & (U > 0) & (V < 0)]
        for t, term in enumerate(terms):
            acc[t] = torch.where(ok, acc[t] + term, acc[t])
        for q, inq in enumerate(quads):
            acc[13 + q] = torch.where(inq, acc[13 + q] + 1.0, acc[13 + q])
            acc[17 + q] = torch.where(inq, acc[17 + q] + P, acc[17 + q])
    return acc


def _rounds(fns, n, rounds):
    """us per call of each function of `fns`: `rounds` windows of n back-to-back calls each, the functions taking turns."""
    out = [[] for _ in fns]
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) / n * 1e3)
    return [sorted(t) for t in out]


def bench_distribution(args):
    """pivlfn_flow_hist_accumulate and pivlfn_flow_moments_accumulate (csrc/distribution.hip) at 8 x --size squared on the production
    library, beside the same results from torch.bincount / elementwise torch operations on the same inputs, timed in alternating
    windows.  Per frame: the median with the smallest and largest window, the bytes a frame must move (8 bytes of flow a vector; the
    moments also read and write 21 sums a pixel once per call) and their time at the HBM peak."""
    from pivlfn import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    B, S, lo, hi = 8, args.size, -8.0, 8.0
    g = torch.Generator().manual_seed(2)
    random = (2.0 * torch.randn(B, 2, S, S, generator=g)).to(dev)
    constant = torch.full((B, 2, S, S), 0.3, device=dev)
    for name, flow, table in (("default table", random, (256, 64, 64)), ("largest table", random, (4096, 256, 1024)),
                              ("one bin, default table", constant, (256, 64, 64))):
        words = 2 * (table[0] + 2) + table[1] ** 2 + 1 + 2 * table[2] + 2
        hist = torch.zeros(words, dtype=torch.int64, device=dev)

        def hip(flow=flow, table=table, hist=hist):
            _lib.check(lib.pivlfn_flow_hist_accumulate(flow.data_ptr(), None, None, None, hist.data_ptr(), B, S, S, lo, hi, *table, st),
                       "flow_hist_accumulate")

        def composed(flow=flow, table=table):
            return _torch_hist(flow, lo, hi, *table)
        hip()
        assert torch.equal(hist, composed()), f"{name}: the kernel and the torch composition disagree"
        t_hip, t_torch = _rounds([hip, composed], n=10, rounds=7)
        bound = 8 * S * S / HBM_BYTES_PER_S * 1e6
        print(f"flow_hist_accumulate {name:22s} B={B} {S}x{S}: {t_hip[3] / B:8.2f} us/frame ({t_hip[0] / B:.2f} - {t_hip[-1] / B:.2f})  "
              f"HBM bound {bound:5.2f} us/frame = {100 * bound * B / t_hip[3]:5.1f} %  torch {t_torch[3] / B:9.1f} us/frame "
              f"({t_torch[0] / B:.1f} - {t_torch[-1] / B:.1f}) = {t_torch[3] / t_hip[3]:6.1f} x", flush=True)
    for name, flow in (("random", random), ("constant", constant)):
        acc = torch.zeros(21, S, S, dtype=torch.float64, device=dev)
        ref = torch.zeros(21, S, S, dtype=torch.float64, device=dev)

        def hip(flow=flow, acc=acc):
            _lib.check(lib.pivlfn_flow_moments_accumulate(flow.data_ptr(), None, None, None, acc.data_ptr(), B, S, S, st), "flow_moments_accumulate")

        def composed(flow=flow, ref=ref):
            return _torch_moments(flow, ref)
        hip()
        assert torch.equal(acc, composed()), f"{name}: the kernel and the torch composition disagree"
        t_hip, t_torch = _rounds([hip, composed], n=10, rounds=7)
        bound = (8 * B + 2 * 21 * 8) * S * S / HBM_BYTES_PER_S * 1e6
        print(f"flow_moments_accumulate {name:9s} B={B} {S}x{S}: {t_hip[3]:8.1f} us/call ({t_hip[0]:.1f} - {t_hip[-1]:.1f}) = {t_hip[3] / B:7.2f} "
              f"us/frame  HBM bound {bound:6.1f} us/call = {100 * bound / t_hip[3]:5.1f} %  torch {t_torch[3]:9.1f} us/call "
              f"({t_torch[0]:.1f} - {t_torch[-1]:.1f}) = {t_torch[3] / t_hip[3]:6.1f} x", flush=True)


def bench_spectrum(args):
    """pivlfn_spectrum_accumulate (csrc/spectrum.hip): one segment call at L = 256 with all 129 frequencies of the Hann basis, at
    N = --size squared and at N = 256 squared vectors, on the production library; and the same sums formed from
    pivlfn_snapshot_project (the [L, 2K] basis as weights, 64 columns per call) plus torch for the squares and the accumulation.
    Beside each median two bounds: the ring read once and acc read and written once at the HBM peak, and the contract's
    4 K L N products and as many additions at the fp64 vector peak (the contract forbids fma, so half of it is the most a kernel
    can reach).  The torch arm has no validity rule: it times the arithmetic alone."""
    from pivlfn import _lib
    from pivlfn.spectrum import basis
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    L, K = 256, 129
    b = torch.from_numpy(basis(L, "hann", "constant", K)).to(dev)
    wt = b.reshape(2 * K, L).t().contiguous()                                 # [L, 2K]: column 2k is C_k, column 2k+1 is S_k
    for S in (args.size, 256):
        N = S * S
        g = torch.Generator().manual_seed(3)
        ring = torch.randn(L, 2 * N, generator=g).to(dev)
        acc = torch.zeros(K, 4, N, dtype=torch.float64, device=dev)
        count = torch.zeros(N, dtype=torch.int32, device=dev)
        out = torch.empty(64, 2 * N, dtype=torch.float64, device=dev)

        def fused():
            _lib.check(lib.pivlfn_spectrum_accumulate(ring.data_ptr(), L, 0, N, 2 * N, b.data_ptr(), K, acc.data_ptr(), count.data_ptr(), st),
                       "spectrum_accumulate")

        def pieced():
            for c0 in range(0, 2 * K, 64):
                w = wt[:, c0:c0 + 64].contiguous()
                n = w.size(1)
                _lib.check(lib.pivlfn_snapshot_project(ring.data_ptr(), L, 2 * N, 2 * N, w.data_ptr(), n, out.data_ptr(), st), "snapshot_project")
                cu, su, cv, sv = out[0:n:2, :N], out[1:n:2, :N], out[0:n:2, N:], out[1:n:2, N:]
                a = acc[c0 // 2:c0 // 2 + n // 2]
                a[:, 0] += cu * cu + su * su
                a[:, 1] += cv * cv + sv * sv
                a[:, 2] += cu * cv + su * sv
                a[:, 3] += cu * sv - su * cv
            count.add_(1)

        fused()
        one = acc.clone()
        acc.zero_()
        pieced()
        torch.cuda.synchronize()
        same = bool(torch.equal(one.view(torch.int64), acc.view(torch.int64)))
        hbm = (L * 2 * N * 4 + 2 * K * 4 * N * 8) / HBM_BYTES_PER_S * 1e6
        alu = 8.0 * K * L * N / FP64_VECTOR_FLOP_PER_S * 1e6
        for name, fn in (("spectrum_accumulate", fused), ("snapshot_project + torch", pieced)):
            tmin, tmed = time_it(fn, n=5, rounds=7)
            print(f"{name:24s} L={L} K={K} N={S}x{S}: min {tmin:10.1f} us  med {tmed:10.1f} us  HBM bound {hbm:8.1f} us = {100 * hbm / tmed:5.2f} %  "
                  f"fp64 bound {alu:8.1f} us = {100 * alu / tmed:5.2f} % of the time", flush=True)
        print(f"  the two arms give {'the same bits' if same else 'different bits'} from a zero acc at N={S}x{S}", flush=True)
        del ring, acc, count, out, one


def bench_pressure(args):
    """pivlfn_pressure_cg (csrc/pressure.hip): microseconds per conjugate-gradient iteration at 256 x 256 nodes x 8 frames and at
    1024 x 1024 x 1, on the production library.  A timed call is setup + n iterations at a tolerance that never stops a frame (a
    stopped frame's launches return at once); the time of an iteration is the difference between n = 200 and n = 100, over 100, so
    the set-up and the first launch cancel.  Beside it the bound: the 90 bytes per node an iteration moves (11 doubles and 2 bytes, see
    the head of the kernel file) at the HBM peak, the figure bench.py quotes its rooflines against.  Then bench_pressure_wall."""
    from pivlfn import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    for F, S in ((8, 256), (1, 1024)):
        gen = torch.Generator().manual_seed(4)
        flows = torch.randn(F + 2, 2, S, S, generator=gen).to(dev)
        g = torch.empty(F, 2, S, S, dtype=torch.float64, device=dev)
        valid = torch.empty(F, S, S, dtype=torch.uint8, device=dev)
        nws = lib.pivlfn_pressure_workspace_bytes(F, S, S)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        status = torch.empty(F, 4, dtype=torch.float64, device=dev)
        p, flag = torch.empty(F, S, S, dtype=torch.float64, device=dev), torch.empty(F, S, S, dtype=torch.uint8, device=dev)
        _lib.check(lib.pivlfn_pressure_gradient(flows.data_ptr(), F + 2, S, S, 4.0, 0.01, g.data_ptr(), valid.data_ptr(), st), "gradient")

        def fn(n):
            _lib.check(lib.pivlfn_pressure_setup(g.data_ptr(), valid.data_ptr(), F, S, S, 4.0, ws.data_ptr(), nws, st), "setup")
            _lib.check(lib.pivlfn_pressure_cg(ws.data_ptr(), nws, F, S, S, 1e-200, n, st), "cg")
        t100, t200 = time_it(lambda: fn(100), n=3, rounds=7)[1], time_it(lambda: fn(200), n=3, rounds=7)[1]
        _lib.check(lib.pivlfn_pressure_read(ws.data_ptr(), nws, F, S, S, p.data_ptr(), flag.data_ptr(), status.data_ptr(), st), "read")
        running = int((status[:, 0] == 1).sum())
        per = (t200 - t100) / 100.0
        hbm = 90.0 * F * S * S / HBM_BYTES_PER_S * 1e6
        print(f"pressure_cg F={F} {S}x{S}: setup + 100 it {t100:9.1f} us, + 200 it {t200:9.1f} us -> {per:7.2f} us per iteration (2 launches); "
              f"HBM bound {hbm:6.2f} us = {100 * hbm / per:5.1f} % of the time; {running} of {F} frames still running after 200", flush=True)
        del flows, g, valid, ws, p, flag
    bench_pressure_wall(dev)


def bench_pressure_wall(dev):
    """Wall time of pivlfn.PressureField.update per frame at 1024 x 1024 flows, cell 4 (256 x 256 nodes), tol 1e-8: decaying vortices of
    wavelength 256 px plus noise of 0.05 px; a host timer around update() and a synchronisation.  Ten flows in one update() (eight
    frames share their launches), three times -- the first includes the warm-up --, then one flow per update()."""
    import time

    import numpy as np
    from pivlfn import PressureField
    H = W = 1024
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    k = 2 * np.pi / 256
    flows = np.stack([np.stack([2 * np.sin(k * x) * np.cos(k * y), -2 * np.cos(k * x) * np.sin(k * y)]) * np.exp(-0.01 * n) for n in range(10)])
    flows = torch.from_numpy((flows + np.random.default_rng(0).normal(0, 0.05, flows.shape)).astype(np.float32)).to(dev)
    for sync_every in (64, None):
        for _ in range(3):
            pf = PressureField(H, W, 4, tol=1e-8, sync_every=sync_every, device=dev)
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = pf.update(flows)
            it = res.iterations                       # copies the status back: synchronises
            dt = time.perf_counter() - t
            print(f"sync_every={sync_every}: {len(res)} frames in one update, {dt * 1e3:.1f} ms = {dt * 1e3 / len(res):.2f} ms per frame; "
                  f"iterations {it.min()}..{it.max()} of max_iter {pf.max_iter}; converged {int(res.converged.sum())}; residual max "
                  f"{res.residual.max():.2e}", flush=True)
        pf = PressureField(H, W, 4, tol=1e-8, sync_every=sync_every, device=dev)
        pf.update(flows[:2])
        torch.cuda.synchronize()
        t = time.perf_counter()
        for n in range(2, 10):
            _ = pf.update(flows[n:n + 1]).iterations
        dt = time.perf_counter() - t
        print(f"sync_every={sync_every}: one frame per update, {dt * 1e3 / 8:.2f} ms per frame", flush=True)


INT_MAC_PER_S = 256 * 4 * 32 * 4 * 2.4e9      # 1024 SIMDs x 32 lanes per cycle x 4 MACs of a v_dot4_u32_u8 x 2.4 GHz


def bench_calibrate(args):
    """The three entry points of csrc/calibrate.hip at 1 x --size squared (DESIGN quotes --size 2048) with the 25 x 25 cross
    template, on the production library.  template_match against the integer-MAC bound 3 N H W (I.T, I.I and I.1 per tap) at the
    v_dot4_u32_u8 rate; dewarp_frames against its byte bound (one read and one write of the frame) at the HBM peak; target_points (six
    launches) on the correlation map of a rendered cross lattice, as a time alone."""
    import ctypes
    import numpy as np
    from pivlfn import _lib, calibrate as cal
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    S = args.size
    templ = cal.gen_template(11, 25, 25)
    yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    dx, dy = (xx % 48) - 24, (yy % 48) - 24
    image = np.where(((abs(dx) <= 12) & (abs(dy) <= 5)) | ((abs(dx) <= 5) & (abs(dy) <= 12)), 255, 0).astype(np.uint8)
    img, t = torch.from_numpy(image[None]).to(dev), torch.from_numpy(templ).to(dev)
    r = torch.empty(1, S, S, device=dev)
    nws = lib.pivlfn_template_match_workspace_bytes(25, 25)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    n, med = time_it(lambda: _lib.check(lib.pivlfn_template_match(img.data_ptr(), t.data_ptr(), r.data_ptr(), 1, S, S, 25, 25, ws.data_ptr(), nws, st)),
                     n=20, rounds=7)
    bound = 3.0 * 625 * S * S / INT_MAC_PER_S * 1e6
    print(f"template_match 1x{S}x{S}, 25x25: min {n:8.1f} us, median {med:8.1f} us (2 launches); integer-MAC bound {bound:7.1f} us = "
          f"{100 * bound / med:5.1f} % of the time", flush=True)
    cap = 4096
    nws2 = lib.pivlfn_target_points_workspace_bytes(1, S, S)
    ws2 = torch.empty(nws2, dtype=torch.uint8, device=dev)
    labels, count = torch.empty(1, S, S, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    rec = torch.empty(1, cap, 4, dtype=torch.int64, device=dev)
    n, med = time_it(lambda: _lib.check(lib.pivlfn_target_points(r.data_ptr(), 1, S, S, 0.7, cap, labels.data_ptr(), count.data_ptr(), rec.data_ptr(),
                                                                 ws2.data_ptr(), nws2, st)), n=20, rounds=7)
    print(f"target_points 1x{S}x{S}: min {n:8.1f} us, median {med:8.1f} us (6 launches); {int(count[0])} components", flush=True)
    A = np.zeros(24)
    A[[0, 8, 13, 20]] = 1.0
    A[[1, 6, 7, 12, 18, 19]] = (0.02, 2e-5, -1e-5, -0.015, 1e-5, 2e-5)
    a_c = (ctypes.c_double * 24)(*A.tolist())
    for f32, mode in ((0, 0), (0, 1), (1, 0), (1, 1)):
        src = torch.rand(1, S, S, device=dev) if f32 else img
        out = torch.empty_like(src)
        n, med = time_it(lambda: _lib.check(lib.pivlfn_dewarp_frames(src.data_ptr(), out.data_ptr(), f32, 1, S, S, a_c, S / 2.0, S / 2.0, mode, 0.0, st)),
                         n=20, rounds=7)
        bound = 2.0 * S * S * (4 if f32 else 1) / HBM_BYTES_PER_S * 1e6
        print(f"dewarp_frames 1x{S}x{S} {'f32' if f32 else 'u8 '} {'bilinear' if mode else 'nearest '}: min {n:8.1f} us, median {med:8.1f} us; "
              f"byte bound {bound:6.2f} us = {100 * bound / med:5.1f} % of the time", flush=True)


def bench_ensemble(args):
    """pivlfn_ensemble_corr on 8 frames of --size squared (DESIGN quotes --size 1024), window 32, step 16, search 8, on the production
    library, against the integer-MAC bound nwin P^2 window^2 B (the A.B products alone) at the v_dot4_u32_u8 rate."""
    import numpy as np
    from pivlfn import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    S, B, window, step, search = args.size, 8, 32, 16, 8
    n1 = (S - window - 2 * search) // step + 1
    P = 2 * search + 1
    rng = np.random.default_rng(0)
    a, b = (torch.from_numpy(rng.integers(0, 256, (B, S, S), dtype=np.uint8)).to(dev) for _ in range(2))
    sums = torch.zeros(n1, n1, P, P, 3, dtype=torch.int64, device=dev)
    sums_a = torch.zeros(n1, n1, 2, dtype=torch.int64, device=dev)
    n, med = time_it(lambda: _lib.check(lib.pivlfn_ensemble_corr(a.data_ptr(), b.data_ptr(), None, sums.data_ptr(), sums_a.data_ptr(), B, S, S, window,
                                                                 step, search, st)), n=20, rounds=7)
    bound = float(n1 * n1) * P * P * window * window * B / INT_MAC_PER_S * 1e6
    print(f"ensemble_corr {B}x{S}x{S}, window {window}, step {step}, search {search} ({n1 * n1} windows): min {n:8.1f} us, median {med:8.1f} us; "
          f"integer-MAC bound {bound:6.1f} us = {100 * bound / med:5.1f} % of the time", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["warp_corr", "wc_ablate", "conv", "conv_stamps", "head", "preproc", "evaluate", "twopoint", "distribution", "spectrum", "pressure",
                                     "calibrate", "ensemble"])
    ap.add_argument("--once", action="store_true", help="preproc: one launch per shape, for a kernel trace")
    ap.add_argument("--filter", default="")
    ap.add_argument("--tune3", type=int, default=0, help="ablation mask of the fp16 conv kernel (pivlfn_tune(3, mask))")
    ap.add_argument("--tune7", type=int, default=0, help="ablation mask of the fp32 conv kernel in a -DPIVLFN_STAMPS build (pivlfn_tune(7, mask))")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--size", type=int, default=1024, help="input image size the level shapes are derived from")
    ap.add_argument("--variants", help="comma-separated variant list (default: warp_corr 0,8,9; conv 6,8,5)")
    ap.add_argument("--levels", default="3,1,2,4,5,6")
    ap.add_argument("--smooth", action="store_true", help="wc_ablate: smooth flow instead of per-pixel noise")
    ap.add_argument("--masks", default="0,8,1,2,4,3,7", help="wc_ablate: pivlfn_tune(2, .) masks")
    ap.add_argument("--rounds", type=int, default=8, help="interleaved timing rounds per variant (warp_corr)")
    a = ap.parse_args()
    {"conv_stamps": bench_conv_stamps, "warp_corr": bench_warp_corr, "wc_ablate": bench_wc_ablate, "conv": bench_conv, "head": bench_head,
     "preproc": bench_preproc, "evaluate": bench_evaluate, "twopoint": bench_twopoint, "distribution": bench_distribution, "spectrum": bench_spectrum, "pressure": bench_pressure,
     "calibrate": bench_calibrate, "ensemble": bench_ensemble}[a.what](a)
