"""GPU: pivlfn_forward in the default mode with Regularization's distance layers on the split-bf16 streaming kernels
(csrc/conv_dist_b3.hip) -- the part of tests/test_gpu_dist_b3.py that creates networks (side streams), a capture stream and a graph.
Not collected by name: tests/test_gpu_dist_b3.py::test_forward_in_a_process_of_its_own runs this file in a fresh pytest process, for the
reason tests/test_gpu_flowmap.py::test_stream_contract_and_run_py_in_a_process_of_their_own gives (streams made here would change
which hardware queue a later module's side stream shares with the default stream)."""
import pytest
import torch

import pivlfn
from pivlfn import synth

pytestmark = pytest.mark.gpu


# ---- the forward in the default mode: level 1 of a 256 x 256 pair runs both kernels ------------------------------------------------
@pytest.fixture(scope="module")
def net(dev):
    return pivlfn.Network(model="piv", params=synth.generate_weights("piv", 0)).to(dev).eval()


@pytest.fixture(scope="module")
def pairs(dev):
    a, b = synth.particle_batch(2, 256, 256, seed=77)
    return torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)


def test_forward_batch_invariance_and_graph_replay(net, pairs, dev):
    i1, i2 = pairs
    full = net(i1, i2).clone()
    for k in range(2):
        assert torch.equal(net(i1[k:k + 1], i2[k:k + 1])[0], full[k]), f"pair {k} depends on its batch mate"
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        net(i1, i2)                                   # workspace allocated outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = net(i1, i2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, full)


def test_forward_beside_the_fp32_instruction_mode(net, pairs, dev):
    """fp32_wino_mfma32 keeps the distance layers (and the Winograd layers) on the fp32 instruction: the default mode's flow lies within the
    end-to-end tolerance of tests/test_gpu_net.py of it."""
    i1, i2 = pairs
    flow = net(i1, i2).clone()
    other = pivlfn.Network(model="piv", params=synth.generate_weights("piv", 0)).to(dev).eval()
    other.precision = "fp32_wino_mfma32"
    ref = other(i1, i2)
    scale = max(1.0, ref.abs().max().item())
    err = (flow - ref).abs()
    print(f"default vs fp32_wino_mfma32 at 2 x 256 x 256: max {err.max().item():.3e} mean {err.mean().item():.3e} px, flow scale {scale:.2f}")
    assert err.max().item() <= 1e-4 * scale
    assert err.mean().item() <= 1e-5 * scale
