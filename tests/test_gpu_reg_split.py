"""GPU: Regularization's first layer (conv_R.0) computed as two layers from a 256 x 256 output grid per image up -- its 128
feature channels on the side stream (flow-independent, stored as a partial sum), its three [difference, flow - mean] channels on
the main stream with the partial sum as residual -- against the oracle, against float64, across batches, across dirty workspaces,
under graph capture, and with the other conv modes left on the single-launch layer.  The smallest shapes that reach the path."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pivlfn
import pivlfn_oracle as orc
from pivlfn import _lib, synth

pytestmark = pytest.mark.gpu

# End-to-end fp32 tolerance (as tests/test_gpu_net.py): max-abs <= 1e-4 * max(1, max|flow|) px, mean-abs
# an order of magnitude below that.
E2E_MAX = 1e-4
E2E_MEAN = 1e-5
PIVLFN_ERR_WORKSPACE = 3


def _check(got, want, what):
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    scale = max(1.0, np.abs(want).max())
    err = np.abs(got - want)
    print(f"{what}: max-abs {err.max():.3e} mean-abs {err.mean():.3e} at flow scale {scale:.2f}")
    assert err.max() <= E2E_MAX * scale, f"{what}: max-abs {err.max():.3e} vs flow scale {scale:.2f}"
    assert err.mean() <= E2E_MEAN * scale, f"{what}: mean-abs {err.mean():.3e}"


@pytest.fixture(scope="module")
def nets(dev):
    return {m: pivlfn.Network(model=m, params=synth.generate_weights(m, 0)).to(dev).eval() for m in ("piv", "hui")}


_ORACLE = {}


def _oracle(model, B, H, W, seed):
    """The oracle's flow and per-level flows on the CPU, computed once per case and shared (never modified)."""
    key = (model, B, H, W, seed)
    if key not in _ORACLE:
        a, b = synth.particle_batch(B, H, W, seed=seed)
        onet = orc.make_net(model, synth.generate_weights(model, 0), corr="c")
        with torch.no_grad():
            want, want_levels = onet.forward(torch.from_numpy(a), torch.from_numpy(b), return_levels=True)
        _ORACLE[key] = (a, b, want.numpy(), [[t.numpy() for t in trio] for trio in want_levels])
    return _ORACLE[key]


# piv 256 x 256: level 1 split, every deeper level on the single-launch layer; piv 512 x 256: levels 1 and 2, not square;
# hui 512 x 512: the lowest level is 2, at 256 x 256; piv 256 x 288: a width that is no multiple of the tail pass's 64-pixel tile
@pytest.mark.parametrize("model,H,W", [("piv", 256, 256), ("piv", 512, 256), ("hui", 512, 512), ("piv", 256, 288)])
def test_every_level_against_the_oracle(model, H, W, nets, dev):
    a, b, want, want_levels = _oracle(model, 1, H, W, 4545)
    flow, levels = nets[model].forward_levels(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
    assert len(levels) == len(want_levels)
    for j, (trio, wtrio) in enumerate(zip(levels, want_levels)):          # a wrong channel slice shows in the R of its own level
        for name, t, w in zip("MSR", trio, wtrio):
            _check(t.cpu().numpy(), w, f"{model} 1x{H}x{W} level#{j} {name}")
    _check(flow.cpu().numpy(), want, f"{model} 1x{H}x{W}")


def _create(w, b):
    h = ctypes.c_void_p()
    co, ci, kh, kw = w.shape
    _lib.check(_lib.load().pivlfn_conv_create(w.data_ptr(), b.data_ptr(), co, ci, kh, kw, ctypes.byref(h)), "conv_create")
    return h


def test_the_layer_alone_against_float64(dev):
    """conv_R.0 at 1 x 256 x 256 on random inputs: 128 -> 128 without bias or activation on the split-operand Winograd kernel, then
    3 -> 128 with the bias, the partial sum as residual and the LeakyReLU on the direct kernel; against the single launch over both
    sources.  One more fp32 rounding of a partial sum of the layer's own magnitude: at most twice the single launch's error."""
    lib = _lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    H = W = 256
    g = torch.Generator().manual_seed(2801)
    w = (torch.randn(128, 131, 3, 3, generator=g) / (131 * 9) ** 0.5).contiguous()      # the reference's order: [misc 3, features 128]
    b = (torch.randn(128, generator=g) * 0.1).contiguous()
    feat = torch.randn(1, 128, H, W, generator=g)
    misc = torch.randn(1, 3, H, W, generator=g)
    w_feat, w_misc = w[:, 3:].contiguous(), w[:, :3].contiguous()
    want = F.leaky_relu(F.conv2d(torch.cat([misc, feat], 1).double(), w.double(), b.double(), padding=1), 0.1)
    x_feat = feat.permute(0, 2, 3, 1).contiguous().to(dev)
    m4 = torch.zeros(1, H, W, 4)
    m4[..., :3] = misc.permute(0, 2, 3, 1)
    x_misc = m4.to(dev)
    zero = torch.zeros(128)
    ha, hb, hc = _create(w_feat, zero), _create(w_misc, b), ctypes.c_void_p()
    w_cat = torch.cat([w_feat, w_misc], 1).contiguous()                                   # the staged order: {features}, {misc}
    _lib.check(lib.pivlfn_conv_create_cat(w_cat.data_ptr(), b.data_ptr(), 128, 2, (ctypes.c_int * 2)(128, 3), 3, 3, ctypes.byref(hc)), "conv_create_cat")
    try:
        part = torch.full((1, H, W, 128), float("nan"), device=dev)
        y2 = torch.full((1, H, W, 128), float("nan"), device=dev)
        y1 = torch.full((1, H, W, 128), float("nan"), device=dev)
        _lib.check(lib.pivlfn_conv2d_nhwc_wino_b3(ha, x_feat.data_ptr(), 128, part.data_ptr(), 128, 1, H, W, 0, 6, st), "wino_b3")
        _lib.check(lib.pivlfn_conv2d_nhwc(hb, x_misc.data_ptr(), 4, y2.data_ptr(), 128, part.data_ptr(), 128, 1, H, W, 1, 1, 1, 1, st), "conv2d")
        ptrs = (ctypes.c_void_p * 2)(x_feat.data_ptr(), x_misc.data_ptr())
        _lib.check(lib.pivlfn_conv2d_nhwc_cat(hc, 2, ptrs, (ctypes.c_int * 2)(128, 4), y1.data_ptr(), 128, 1, H, W, 1, st), "conv2d_cat")
        e2 = (y2.cpu().permute(0, 3, 1, 2).double() - want).abs().max().item()
        e1 = (y1.cpu().permute(0, 3, 1, 2).double() - want).abs().max().item()
        print(f"conv_R.0 at 256x256 against float64: split {e2:.3e}, single launch {e1:.3e}, max |out| {want.abs().max().item():.2f}")
        assert e2 <= 2 * e1, (e2, e1)
    finally:
        for h in (ha, hb, hc):
            lib.pivlfn_conv_destroy(h)


def _forward_c(net, i1, i2, ws, ws_bytes, dev):
    """pivlfn_forward on a caller's workspace (as tests/test_gpu_guarded.py reaches it); returns (rc, flow)."""
    lib = _lib.load()
    B, _, H, W = i1.shape
    div = 2 ** (net.lowest_level - 1)
    flow = torch.full((B, 2, H // div, W // div), float("nan"), device=dev)
    rc = lib.pivlfn_forward(net._native(), i1.data_ptr(), i2.data_ptr(), flow.data_ptr(), None, B, H, W, ws.data_ptr(), ws_bytes,
                            torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return rc, flow


def test_batch_determinism_and_a_dirty_workspace(nets, dev):
    """A missing join, or a partial sum read before it is written, shows as a pair that depends on its batch mates, on the run, or
    on what the workspace held."""
    net = nets["piv"]
    a, b = synth.particle_batch(3, 256, 256, seed=61)
    i1, i2 = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    full = net(i1, i2).clone()
    for k in range(3):
        assert torch.equal(net(i1[k:k + 1], i2[k:k + 1])[0], full[k]), f"pair {k} depends on its batch mates"
    assert torch.equal(net(i1, i2), full)
    # eight pairs: the tail pass takes its 8-row tile from 1024 workgroups up (one 256 x 256 pair alone: 2-row tiles)
    big = net(torch.cat([i1, i1, i1[:2]]), torch.cat([i2, i2, i2[:2]]))
    for k in range(8):
        assert torch.equal(big[k], full[k % 3]), f"pair {k} of eight differs from its single-pair flow"
    need = _lib.load().pivlfn_workspace_bytes(net._native(), 3, 256, 256)
    ws = torch.zeros(need // 4, dtype=torch.float32, device=dev)
    rc, f0 = _forward_c(net, i1, i2, ws, need, dev)
    assert rc == 0 and torch.equal(f0, full)
    ws.fill_(float("nan"))
    torch.cuda.synchronize()
    rc, f1 = _forward_c(net, i1, i2, ws, need, dev)
    assert rc == 0 and torch.equal(f1, full), "the flow depends on what the workspace held"


def test_ragged_width_on_either_tail_tile(nets, dev):
    """256 x 288: the tail pass's last 64-pixel tile of a row is half empty.  One pair runs its 2-row tile (checked against the oracle
    above), eight pairs its 8-row tile: the same bits."""
    a, b, _, _ = _oracle("piv", 1, 256, 288, 4545)
    i1, i2 = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    one = nets["piv"](i1, i2).clone()
    big = nets["piv"](i1.expand(8, -1, -1, -1).contiguous(), i2.expand(8, -1, -1, -1).contiguous())
    for k in range(8):
        assert torch.equal(big[k], one[0]), f"pair {k} of eight differs from the single pair"


# 256 x 256: level 1 split, its features from the side stream's own 1 x 1 layer; 1024 x 1024: levels 1-3 split, level 1's features
# from conv1's fused kernel on the main stream, the side stream forked once per level in front of the deeper levels' partial sums
@pytest.mark.parametrize("size", [256, 1024])
def test_capture_and_replay(size, nets, dev):
    """As test_forward_is_graph_capturable, at the sizes from which the partial sums go to the side stream: replays against eager runs."""
    a, b = synth.particle_batch(1, size, size, seed=41)
    i1, i2 = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    net = nets["piv"]
    ref = net(i1, i2).clone()
    ref_swapped = net(i2.clone(), i1.clone()).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        net(i1, i2)                                   # workspace allocated outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = net(i1, i2)
    i1.copy_(torch.from_numpy(b).to(dev))
    i2.copy_(torch.from_numpy(a).to(dev))
    g.replay()
    torch.cuda.synchronize()
    swapped = out.clone()
    i1.copy_(torch.from_numpy(a).to(dev))
    i2.copy_(torch.from_numpy(b).to(dev))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert torch.equal(swapped, ref_swapped)


def test_other_modes_keep_the_single_launch_layer(dev):
    """fp32_direct and fp16 at 1 x 256 x 256: the checks their own tests apply (tests/test_gpu_wino.py, tests/test_gpu_split.py,
    tests/test_gpu_f16.py), the workspace query honoured, a workspace one byte short refused."""
    a, b, want, _ = _oracle("piv", 1, 256, 256, 4545)
    i1, i2 = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    net = pivlfn.Network(model="piv", params=synth.generate_weights("piv", 0)).to(dev).eval()
    f32 = net(i1, i2).clone()
    lib = _lib.load()
    for mode in ("fp32_direct", "fp16"):
        net.precision = mode
        need = lib.pivlfn_workspace_bytes(net._native(), 1, 256, 256)
        ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=dev)
        rc, flow = _forward_c(net, i1, i2, ws, need, dev)
        assert rc == 0, lib.pivlfn_last_error()
        assert torch.equal(net(i1, i2), flow)                    # reproducible, and the same on the module's own workspace
        assert not torch.equal(flow, f32)                        # the mode really ran
        if mode == "fp32_direct":
            d = (flow - f32).abs().max().item()
            assert d < 1e-4 * max(1.0, flow.abs().max().item())
            _check(flow.cpu().numpy(), want, "piv 1x256x256 fp32_direct")
        else:
            e = np.sqrt(((flow.cpu().numpy().astype(np.float64) - f32.cpu().numpy().astype(np.float64)) ** 2).sum(1))
            print(f"piv 256x256 fp16-mode EPE vs fp32 mode: mean {e.mean():.2e} px, max {e.max():.2e} px")
            assert e.mean() <= 0.05 and e.max() <= 0.5
        rc, _ = _forward_c(net, i1, i2, ws, need - 1, dev)
        assert rc == PIVLFN_ERR_WORKSPACE and b"workspace" in lib.pivlfn_last_error()
        # these modes do not hold the partial sums: a smaller workspace, which the splitting mode refuses
        net.precision = "fp32"
        need32 = lib.pivlfn_workspace_bytes(net._native(), 1, 256, 256)
        assert need32 == need + 256 * 256 * 128 * 4
        rc, _ = _forward_c(net, i1, i2, ws, need, dev)
        assert rc == PIVLFN_ERR_WORKSPACE and b"workspace" in lib.pivlfn_last_error()
    assert torch.equal(net(i1, i2), f32)
