"""What the streaming accumulators share (pivlfn/_accum.py), without a GPU: the constructor refusals recorded from the commit before the
classes were given one base (tests/golden/accumulator_refusals.json, written by tools/gen_accumulator_golden.py), the one merge() of
FlowStats, MaskedFlowStats, ErrorStats and TwoPointStats under gloo, and that the shared pieces exist once."""
import json
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import accumulator_cases as cases
from conftest import GOLD, PKG


def test_constructor_refusals_are_those_recorded():
    want = json.load(open(os.path.join(GOLD, "accumulator_refusals.json")))["constructor"]
    got = cases.constructor_cases()
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key
    assert sum(v is not None for v in want.values()) == len(want) == 3 * 11 - 1 + 2


def test_cuda_device_refuses_and_passes_without_touching_a_gpu():
    from pivlfn import _accum
    assert _accum.cuda_device("cuda:3", "x") == torch.device("cuda", 3) == _accum.cuda_device(torch.device("cuda", 3))
    with pytest.raises(NotImplementedError, match="^someone: GPU only$"):
        _accum.cuda_device("cpu", "someone: GPU only")
    assert _accum.cuda_device("cpu") == torch.device("cpu")


def test_save_npz_adds_the_suffix_once(tmp_path):
    import numpy as np
    from pivlfn import _accum
    a = _accum.save_npz(str(tmp_path / "a"), x=np.arange(3))
    b = _accum.save_npz(str(tmp_path / "b.npz"), x=np.arange(3))
    assert (os.path.basename(a), os.path.basename(b)) == ("a.npz", "b.npz") and sorted(os.listdir(tmp_path)) == ["a.npz", "b.npz"]
    assert np.load(a)["x"].tolist() == [0, 1, 2]


def test_the_shared_pieces_exist_once():
    """Under pivlfn/: the rank-ordered merge (dist.py's gather of flows is something else), the .npz suffix rule and the fallback to the
    current device each stand in one file, _accum.py."""
    src = {}
    for name in sorted(os.listdir(os.path.join(PKG, "pivlfn"))):
        if name.endswith(".py"):
            src[name] = open(os.path.join(PKG, "pivlfn", name)).read()
    for pattern, n in ((r"dist\.all_gather\(", 2), (r'endswith\("\.npz"\)', 1), (r"torch\.cuda\.current_device\(\)", 1)):
        found = {k: len(re.findall(pattern, v)) for k, v in src.items() if k != "dist.py" and re.search(pattern, v)}
        assert found == {"_accum.py": n}, (pattern, found)
    assert "current_device" not in src["dist.py"]


# ---- merge -------------------------------------------------------------------------------------------------------------------------
MERGED = {"FlowStats": {"acc": (7, 2, 3)}, "MaskedFlowStats": {"acc": (7, 2, 3), "cnt": (2, 2, 3)}, "ErrorStats": {"acc": (6, 2, 3)},
          "TwoPointStats": {"acc": (2, 3, 15, 4)}}
AT = 5                                                    # the flat index of the element the three-rank case looks at


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _bare(name):
    """Accumulators injected on the host: the constructor wants a GPU."""
    from pivlfn import evaluate, postpro, twopoint, validate
    cls = {"FlowStats": postpro.FlowStats, "MaskedFlowStats": validate.MaskedFlowStats, "ErrorStats": evaluate.ErrorStats,
           "TwoPointStats": twopoint.TwoPointStats}[name]
    st = cls.__new__(cls)
    st.H, st.W, st.device = 2, 3, torch.device("cpu")
    if name == "TwoPointStats":
        st.H, st.W, st.max_sep, st.step, st.mean = 4, 5, 2, 1, None
    return st


def _merge_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ok = {}
    for name, shapes in MERGED.items():
        st, want = _bare(name), {}
        for attr, shape in shapes.items():
            n = int(torch.tensor(shape).prod())
            base = torch.arange(n, dtype=torch.float64).view(shape)
            if world == 2:
                setattr(st, attr, base * (rank + 1) + 0.1 * rank)
                want[attr] = base + (base * 2 + 0.1)                  # rank 0 + rank 1, in rank order
            else:
                t = torch.zeros(n, dtype=torch.float64)
                t[AT] = (1e16, 1.0, -1e16)[rank]
                setattr(st, attr, t.view(shape))
                want[attr] = torch.zeros(shape, dtype=torch.float64)  # (1e16 + 1) + (-1e16) = 0; any other association gives 1
        st.count = 4 + rank
        st.merge()
        ok[name] = all(bool(torch.equal(getattr(st, attr), want[attr])) for attr in shapes) and st.count == (9 if world == 2 else 15)
    q.put((rank, ok))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_merge_adds_in_rank_order_on_every_rank_gloo(world):
    """All four classes that have a merge(), in one process group.  Two ranks: the sums and the count of both, the same bits on either.
    Three ranks hold 1e16, 1.0 and -1e16 at one element: the spacing of float64 at 1e16 is 2, so the rank-order sum
    (1e16 + 1) + (-1e16) is 0.0 and every other association gives 1.0; MaskedFlowStats shows it in `acc` and in `cnt`."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_merge_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == [(r, dict.fromkeys(MERGED, True)) for r in range(world)]
