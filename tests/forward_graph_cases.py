"""GPU: the two-stream schedule of pivlfn_forward (csrc/net.hip), checked on the dependency graph of a captured forward.  Not collected
by name: tests/test_gpu_forward_graph.py runs this file in a pytest process of its own, for the reason tests/test_gpu_flowmap.py gives.

What is checked, and why two replays are enough.  The forward issues launches on two streams, ordered between the streams by event
edges (ev_fork, ev_pfork, ev_join, ev_pjoin).  A result test cannot see a missing edge: the side stream's few launches are nearly
always done before the main stream reaches their consumer.  The captured forward is a DAG that the runtime hands back, and the DAG is
all that orders the launches: a pair of launches that no path connects may run either way round, and the forward is right only if it
gives the same bits both ways, for every such pair.

    1. The launches of a stream form a chain, so the DAG is two chains, main and side, plus edges between them (two_chains refuses
       anything else).  Launches of one chain are ordered; an unordered pair is one main launch m and one side launch s.
    2. Take the order "side first": Kahn's algorithm, always a ready side node before a ready main node.  Suppose m is taken while s is
       not yet.  Then no side node is ready; the first side node s' not yet taken (s' = s or before s) waits for a main node m' not yet
       taken.  m is ready and m' is not, so m runs before m' or is m': m -> m' -> s' -> s is a path, and the pair was ordered.  So in
       this order every unordered pair runs s before m; by the same argument "main first" runs every one of them m before s.
    3. Both are topological orders of the DAG, so a replay in either is a legal execution of the schedule.  Replayed as chains (an
       edge between consecutive launches: nothing left to the runtime), on a workspace that holds another pair's intermediates, the two
       of them run every unordered pair both ways round.  If launches a and b touch the same buffer with a write among them and no
       path orders them, one of the two replays runs the consumer on the other pair's stale data, or lets the producer overwrite
       what the consumer was to read, and the bits differ from the eager forward's -- unless the stale and the fresh values agree,
       which is why the stale workspace comes from a different particle pair, and why the sharpness runs below remove each
       essential edge in turn and require the difference to show.
    4. Pairs that are ordered need no replay: every execution of the DAG runs them the one way the eager forward ran them.

The workspace is never filled with NaN or any other poison here: stale means an eager forward of other, valid inputs in the same
workspace.  The sharpness runs reorder launches over that valid, finite memory and change nothing else: one edge less, no pointer
other, no buffer smaller."""
import time

import pytest
import torch

import forward_graph as fg
from guarded import check_guards, guarded, poison, same_bits
from pivlfn import _lib, synth
from test_gpu_guarded import _net

pytestmark = pytest.mark.gpu

_NETS = {}


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A device error ends the run: nothing more is started on a GPU that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:       # noqa: BLE001
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def _network(model, precision, dev):
    if (model, precision) not in _NETS:
        _NETS[(model, precision)] = _net(model, dev, precision)
    return _NETS[(model, precision)]


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class _Fw:
    """One forward on fixed, guarded buffers: images, flow and levels.  pairs["X"] is the pair that leaves stale intermediates,
    pairs["Y"] the one whose flow is asked for."""

    def __init__(self, model, precision, B, H, W, dev, seeds):
        self.what = f"{model} {precision} {B}x{H}x{W}"
        self.net, self.B, self.H, self.W, self.dev = _network(model, precision, dev), B, H, W, dev
        self.h, lib = self.net._native(), _lib.load()
        self.need = lib.pivlfn_workspace_bytes(self.h, B, H, W)
        div = 2 ** (self.net.lowest_level - 1)
        self.i1, self.i2 = (guarded((B, 3, H, W), torch.float32, dev, "nan") for _ in range(2))
        self.flow = guarded((B, 2, H // div, W // div), torch.float32, dev, "sentinel")
        self.lv = guarded((lib.pivlfn_levels_floats(self.h, B, H, W),), torch.float32, dev, "sentinel")
        self.pairs = {}
        for key, seed in zip("XY", seeds):
            a, b = synth.particle_batch(B, H, W, seed=seed)
            self.pairs[key] = (torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
        assert not torch.equal(self.pairs["X"][0], self.pairs["Y"][0])

    def load(self, key):
        self.i1.copy_(self.pairs[key][0])
        self.i2.copy_(self.pairs[key][1])

    def enqueue(self, ws, stream):
        _lib.check(_lib.load().pivlfn_forward(self.h, self.i1.data_ptr(), self.i2.data_ptr(), self.flow.data_ptr(), self.lv.data_ptr(),
                                              self.B, self.H, self.W, ws.data_ptr(), self.need, stream), "forward")

    def clear(self):
        for t in (self.flow, self.lv):
            poison(t, slice(0, t.shape[-1]), "sentinel")

    def result(self):
        return self.flow.cpu(), self.lv.cpu()

    def check_guards(self, what):
        for t in (self.i1, self.i2, self.flow, self.lv):
            check_guards(t, what)


def _workspace(fws, dev):
    """One guarded workspace for all forwards of a case.  guarded() pre-fills its payload with the guards' pattern: it is zeroed here,
    before anything is launched on it."""
    ws = guarded((max(fw.need for fw in fws) // 4,), torch.float32, dev, "nan")
    ws.zero_()
    return ws


def _fill(fws, ws, fill, dev):
    """zero: a zeroed workspace.  stale: what eager forwards of the other pairs, in the captured order, leave in it.  Then the real pairs
    in the input buffers and the sentinel in the outputs."""
    if fill == "zero":
        ws.zero_()
    else:
        for fw in fws:
            fw.load("X")
            fw.enqueue(ws, _st(dev))
    for fw in fws:
        fw.load("Y")
        fw.clear()
    torch.cuda.synchronize()


def _differences(fws, truth):
    """[] if every forward's flow and levels hold the eager bits, else one line per output that does not."""
    out = []
    for fw, (flow0, lv0) in zip(fws, truth):
        flow, lv = fw.result()
        for name, got, want in (("flow", flow, flow0), ("levels", lv, lv0)):
            if not same_bits(got, want):
                bad = got.view(torch.int32) != want.view(torch.int32)
                d = (got.double() - want.double()).abs()
                out.append(f"{name} of {fw.what}: {int(bad.sum())} of {bad.numel()} elements differ, by up to "
                           f"{float(d[torch.isfinite(d)].max()) if bool(torch.isfinite(d).any()) else float('nan'):.3g}"
                           + ("" if bool(torch.isfinite(got).all()) else " (some never written)"))
    return out


def _guards(fws, ws, what):
    check_guards(ws, f"{what}: workspace")
    for fw in fws:
        fw.check_guards(what)


def _label(dag, chains, v):
    main, side = chains
    where = f"main[{main.index(v)}]" if v in main else f"side[{side.index(v)}]"
    return f"{where} {fg.short_name(dag.names[v])}"


class _Case:
    """Eager truth, warm-up, capture and the structure checks of one case; the replays and the sharpness runs work on it."""

    def __init__(self, what, fws, dev, touch, tails, fused):
        self.what, self.fws, self.dev = what, fws, dev
        self.ws = _workspace(fws, dev)
        self.truth = []
        for fw in fws:                                           # eager, each on a zeroed workspace
            self.ws.zero_()
            fw.load("Y")
            fw.clear()
            fw.enqueue(self.ws, _st(dev))
            torch.cuda.synchronize()
            self.truth.append(fw.result())
            assert all(bool(torch.isfinite(t).all()) for t in self.truth[-1])
        _guards(fws, self.ws, f"{what}, eager")
        side_stream = torch.cuda.Stream(dev)                     # the warm-up forward on a side stream, as the other capture tests do
        side_stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side_stream):
            for fw in fws:
                fw.enqueue(self.ws, side_stream.cuda_stream)
        torch.cuda.current_stream(dev).wait_stream(side_stream)
        torch.cuda.synchronize()

        def enqueue(stream):
            for fw in fws:
                fw.enqueue(self.ws, stream)
        self.keep, self.graph = fg.capture(enqueue, dev)
        self.dag = self.graph.dag()
        self.chains = fg.two_chains(self.dag)
        self._structure(touch, tails, fused)

    def _structure(self, touch, tails, fused):
        dag, (main, side) = self.dag, self.chains
        names = dag.names
        assert all(not n.startswith("<") for n in names), f"{self.what}: nodes that are no named kernels: {sorted(set(names))[:4]}"
        self.pairs = fg.unordered_pairs(dag)
        self.essential = fg.essential_cross_edges(dag, self.chains)
        print(f"forward-graph | {self.what} | nodes {dag.n} | side nodes {len(side)} | cross edges {len(fg.cross_edges(dag, self.chains))} | "
              f"essential cross edges {len(self.essential)} | unordered pairs {len(self.pairs)}")
        for a, b in self.essential:
            print(f"forward-graph essential | {self.what} | {'join' if a in side else 'fork'} | {_label(dag, self.chains, a)} -> "
                  f"{_label(dag, self.chains, b)}")
        assert side and self.pairs, f"{self.what}: the capture shows no second stream"

        def find(base, first_bool=None):
            return [v for v in range(dag.n) if fg.kernel_is(names[v], base, first_bool)]
        assert len(find("touch_kernel")) == touch and set(find("touch_kernel")) <= set(side), f"{self.what}: touch_kernel is not on the side chain"
        got = find("reg_r0_tail_kernel")
        assert len(got) == tails and set(got) <= set(main), f"{self.what}: {len(got)} reg_r0_tail_kernel nodes, {tails} split levels expected"
        assert len(find("conv_c3k7_kernel", True)) == fused, f"{self.what}: {len(find('conv_c3k7_kernel', True))} fused conv1 launches, expected {fused}"

    def replay(self, graph, fill):
        """One replay of `graph` on a `fill` workspace -> the differences from the eager bits; the guards are checked here."""
        ex = graph.instantiate()
        try:
            _fill(self.fws, self.ws, fill, self.dev)
            ex.launch(_st(self.dev))
            torch.cuda.synchronize()
        finally:
            ex.destroy()
        _guards(self.fws, self.ws, f"{self.what}, replay on a {fill} workspace")
        return _differences(self.fws, self.truth)

    def three_graphs(self):
        dag, chains = self.dag, self.chains
        orders = {"side-earliest": fg.order(dag, "side", chains), "side-latest": fg.order(dag, "main", chains)}
        wrong = {}
        for name in ("side-earliest", "side-latest", "as captured"):
            g = self.graph if name == "as captured" else fg.linearised(self.graph, orders[name])
            try:
                for fill in ("zero", "stale"):
                    diff = self.replay(g, fill)
                    if diff:
                        wrong[(name, fill)] = diff
            finally:
                if g is not self.graph:
                    g.destroy()
        print(f"forward-graph replays | {self.what} | " + " | ".join(
            f"{name}: {'eager bits' if not any(k[0] == name for k in wrong) else 'DIFFERS'}" for name in ("as captured", "side-earliest", "side-latest")))
        lines = []
        for (name, fill), diff in wrong.items():
            if name == "as captured":
                continue
            other = "side-latest" if name == "side-earliest" else "side-earliest"
            u, v = fg.first_inverted_pair(dag, orders[name], orders[other])
            lines.append(f"{name} on a {fill} workspace: {'; '.join(diff)}.  The first pair it runs the other way round than {other}: "
                         f"{_label(dag, chains, u)} before {_label(dag, chains, v)}")
        assert not lines, f"{self.what}: a legal order of the captured launches does not give the eager bits -- a schedule bug in net.hip\n" + "\n".join(lines)
        assert not wrong, (f"{self.what}: both total orders of the captured launches give the eager bits, so the dependency graph is right, but the "
                           f"graph as captured, replayed by the runtime with its branches side by side, does not: {wrong}")

    def sharpness(self):
        """Each essential fork and join but touch_kernel's (nothing reads what it does) removed in turn, in the order that then runs the
        edge's consumer first: the stale workspace must show."""
        dag, chains = self.dag, self.chains
        on_side, missed, seen = set(chains[1]), [], 0
        for a, b in self.essential:
            if fg.kernel_is(dag.names[a], "touch_kernel"):
                continue
            kind, prefer = ("join", "main") if a in on_side else ("fork", "side")
            cut_dag = dag.without((a, b))
            o = fg.order(cut_dag, prefer, chains)
            assert o.index(b) < o.index(a)
            cut = self.graph.clone()
            try:
                cut.remove_edge((a, b))
                assert sorted(set(cut.edges())) == cut_dag.edges
                lin = fg.linearised(cut, o)
            finally:
                cut.destroy()
            try:
                diff = self.replay(lin, "stale")
            finally:
                lin.destroy()
            edge = f"{kind} {_label(dag, chains, a)} -> {_label(dag, chains, b)}"
            print(f"forward-graph edge | {self.what} | {edge} | " + (f"detected: {diff[0]}" if diff else "NOT DETECTED"))
            seen += 1
            if not diff:
                missed.append(edge)
        assert seen >= 2, f"{self.what}: {seen} essential edges"
        assert not missed, (f"{self.what}: without these edges, with their consumer run first on a stale workspace, flow and levels still hold the "
                            f"eager bits -- the edge orders nothing, or the inputs do not discriminate: {missed}")


# model, precision, B, H, W, split levels (reg_r0_tail_kernel launches), conv1 fused with level 1's 1 x 1 layers
CASES = [
    ("piv", "fp32", 2, 64, 96, 0, 0),                   # no split, no fusion: four moduleFeat, two NetC_ext and touch on the side stream
    ("piv", "fp32", 1, 256, 256, 1, 0),                 # split[1] with featR[1] from the side stream's own 1 x 1 layer
    ("piv", "fp32", 1, 256, 512, 1, 1),                 # fused1 (16 x 32 = 512 tiles) with ev_pfork and split[1]
    ("piv", "fp32", 2, 512, 512, 2, 1),                 # fused1, split[1] and split[2]: the join in front of level 3 is last_part = 1's
    ("hui", "fp32", 1, 512, 512, 1, 0),                 # lowest level 2: split[2] without fusion, ext[2] from the side stream
    ("piv", "fp32_wino_mfma32", 1, 256, 256, 1, 0),     # the split with R0a on the fp32-instruction Winograd kernel
    ("piv", "fp32_direct", 1, 256, 512, 0, 1),          # fused1 without a split: side_level(1) issues nothing
    ("piv", "fp16", 1, 256, 256, 0, 0),                 # neither split nor fusion, fp16 activations
    ("piv2-L3", "fp32", 1, 96, 160, 0, 0),              # lowest level 3: only levels 4 and 3 on the side stream
]


def _single(case, dev):
    model, precision, B, H, W, tails, fused = case
    fw = _Fw(model, precision, B, H, W, dev, seeds=(11, 12))
    return _Case(fw.what, [fw], dev, 1, tails, fused)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}x{c[4]}")
def test_both_orders_of_every_unordered_pair(case, dev):
    t0 = time.time()
    c = _single(case, dev)
    c.three_graphs()
    print(f"forward-graph time | {c.what} | {time.time() - t0:.1f} s")


@pytest.mark.parametrize("first,second,tails,fused", [((1, 256, 256), (1, 256, 256), 2, 0), ((1, 256, 512), (2, 64, 96), 1, 1)],
                         ids=["256x256-twice", "256x512-then-64x96"])
def test_two_forwards_in_one_capture(first, second, tails, fused, dev):
    """forward(Y -> out1, lv1), then forward(Z -> out2, lv2) on the same workspace: side-earliest is the order that would let the second
    forward's side launches overwrite featR or part under the first forward's readers."""
    t0 = time.time()
    fws = [_Fw("piv", "fp32", *first, dev, seeds=(21, 22)), _Fw("piv", "fp32", *second, dev, seeds=(23, 24))]
    c = _Case(f"{fws[0].what} then {second[0]}x{second[1]}x{second[2]}", fws, dev, 2, tails, fused)
    c.three_graphs()
    print(f"forward-graph time | {c.what} | {time.time() - t0:.1f} s")


@pytest.mark.parametrize("case", CASES[:2], ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}x{c[4]}")
def test_every_essential_edge_is_needed_and_its_absence_is_seen(case, dev):
    t0 = time.time()
    c = _single(case, dev)
    c.sharpness()
    print(f"forward-graph time | {c.what} sharpness | {time.time() - t0:.1f} s")
