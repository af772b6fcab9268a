"""CPU: the graph algorithms of tests/forward_graph.py, on which tests/forward_graph_cases.py rests, and the runtime symbols it binds.

The property the method needs: for a graph of two chains, order(dag, "side") and order(dag, "main") are both topological and every
pair of nodes that no path connects runs one way round in the first and the other way round in the second.  It is asserted pair by
pair over seeded random two-chain graphs with random forks, joins and redundant edges, and over one hand-written graph per pattern
of event edges in csrc/net.hip."""
import random

import pytest

import forward_graph as fg
from forward_graph import Dag


# ---- planted graphs ---------------------------------------------------------------------------------------------------------------------
def planted(seed):
    """A random graph of a main chain 0..m-1 and a side chain m..m+s-1.  Side node i runs beside main nodes t[i] and t[i] + 1 (t rises
    by 2 or more): forks come from main nodes <= t[i] - 1, joins go to main nodes >= t[i] + 2, so the graph is acyclic and a detour over
    side nodes is always shorter than the main nodes it passes -- the main chain is the one longest path.  Returns the Dag, the chains,
    and the essential forks and joins by the rule of the construction: a fork (a, i) is essential unless another fork (a', i') has
    a' >= a and i' <= i (then a -> a' -> i' -> i is a second path); a join (j, b) unless another has j' >= j and b' <= b."""
    rng = random.Random(seed)
    s = rng.randint(1, 8)
    t, at = [], rng.randint(0, 3)
    for _ in range(s):
        t.append(at)
        at += rng.randint(2, 4)
    m = t[-1] + 2 + rng.randint(0, 4)
    assert m + s <= 42
    side = list(range(m, m + s))
    edges = [(k, k + 1) for k in range(m - 1)] + [(a, b) for a, b in zip(side, side[1:])]
    forks, joins = set(), set()
    for i in range(s):
        for _ in range(rng.choice((0, 1, 1, 2, 3))):
            if t[i] >= 1:
                forks.add((rng.randint(0, t[i] - 1), i))
        for _ in range(rng.choice((0, 1, 1, 2, 3))):
            if t[i] + 2 <= m - 1:
                joins.add((i, rng.randint(t[i] + 2, m - 1)))
    edges += [(a, m + i) for a, i in forks] + [(m + j, b) for j, b in joins]
    for _ in range(rng.randint(0, 6)):                  # redundant edges inside a chain
        a = rng.randint(0, m - 2)
        edges.append((a, rng.randint(a + 1, m - 1)))
        if s > 1:
            i = rng.randint(0, s - 2)
            edges.append((m + i, m + rng.randint(i + 1, s - 1)))
    rng.shuffle(edges)
    ess = {(a, m + i) for a, i in forks if not any((a2, i2) != (a, i) and a2 >= a and i2 <= i for a2, i2 in forks)}
    ess |= {(m + j, b) for j, b in joins if not any((j2, b2) != (j, b) and j2 >= j and b2 <= b for j2, b2 in joins)}
    return Dag(m + s, edges), list(range(m)), side, ess


def _paths(dag):
    """Reachability once more, by a search from every node: the check of Dag.reach."""
    out = []
    for v in range(dag.n):
        seen, stack = set(), [v]
        while stack:
            for s in dag.succ[stack.pop()]:
                if s not in seen:
                    seen.add(s)
                    stack.append(s)
        out.append(seen)
    return out


# main chain 0..11, side nodes from 12; (edges between the chains, the essential ones among them)
HAND = {
    "fork -> A -> B -> join": (12, [12, 13], [(1, 12), (13, 6)], [(1, 12), (13, 6)]),
    # ev_fork[4..1] recorded one behind the other on the main stream: one node forks all of the side chain, the later forks are redundant
    "one node forks every side launch": (12, [12, 13, 14], [(2, 12), (2, 13), (2, 14), (12, 5), (13, 8), (14, 10)],
                                         [(2, 12), (12, 5), (13, 8), (14, 10)]),
    # ev_fork[L] and ev_pfork: a second fork from a later main node onto the same side chain
    "two forks onto one chain": (12, [12, 13, 14], [(1, 12), (4, 13), (0, 14), (14, 10)], [(1, 12), (4, 13), (14, 10)]),
    # SideJoin waits once more for an event the forward has waited for already
    "a join waited twice": (12, [12, 13], [(1, 12), (12, 4), (12, 8), (13, 10)], [(1, 12), (12, 4), (13, 10)]),
    # ev_pjoin[last_part] in front of level 3: it orders every earlier side launch in front of the later joins' consumers
    "a late launch joined early": (12, [12, 13, 14], [(0, 12), (12, 3), (14, 5), (13, 8), (14, 9)], [(0, 12), (12, 3), (14, 5)]),
    # touch_kernel: joined by the end of the capture only, where no node follows
    "a side node nobody joins until the end": (12, [12, 13], [(2, 12), (12, 6)], [(2, 12), (12, 6)]),
}


def _hand(name):
    m, side, cross, ess = HAND[name]
    edges = [(k, k + 1) for k in range(m - 1)] + list(zip(side, side[1:])) + cross
    return Dag(m + len(side), edges), list(range(m)), side, set(ess)


def _check(dag, main, side, ess, what):
    got_main, got_side = fg.two_chains(dag)
    assert (got_main, got_side) == (main, side), what
    reach = _paths(dag)
    for a in range(dag.n):
        for b in range(dag.n):
            assert dag.before(a, b) == (b in reach[a]), (what, a, b)
    pairs = fg.unordered_pairs(dag)
    assert pairs == [(a, b) for a in range(dag.n) for b in range(a + 1, dag.n) if b not in reach[a] and a not in reach[b]], what
    on_side = set(side)
    orders = {p: fg.order(dag, p) for p in ("side", "main")}
    where = {p: {v: k for k, v in enumerate(o)} for p, o in orders.items()}
    for p, o in orders.items():
        assert sorted(o) == list(range(dag.n)), (what, p)
        for a, b in dag.edges:                                              # topological
            assert where[p][a] < where[p][b], (what, p, a, b)
        for a in range(dag.n):                                              # ordered pairs keep their order
            for b in reach[a]:
                assert where[p][a] < where[p][b], (what, p, a, b)
    for a, b in pairs:                                                      # the property the method rests on, pair by pair
        assert (a in on_side) != (b in on_side), (what, a, b)
        s, m = (a, b) if a in on_side else (b, a)
        assert where["side"][s] < where["side"][m], f"{what}: side-earliest runs main node {m} before side node {s}"
        assert where["main"][m] < where["main"][s], f"{what}: side-latest runs side node {s} before main node {m}"
    first = fg.first_inverted_pair(dag, orders["side"], orders["main"])
    if pairs:
        assert first is not None and tuple(sorted(first)) in pairs and first[0] in on_side, what
    else:
        assert orders["side"] == orders["main"] and first is None, what
    assert set(fg.essential_cross_edges(dag)) == ess, what
    assert set(fg.cross_edges(dag)) == {(a, b) for a, b in dag.edges if (a in on_side) != (b in on_side)}
    for e in fg.cross_edges(dag):                                           # the definition itself: removal leaves the ends unordered
        assert (not dag.without(e).ordered(*e)) == (e in ess), (what, e)
    return len(pairs)


@pytest.mark.parametrize("block", range(4))
def test_random_two_chain_graphs(block):
    total = 0
    for seed in range(100 * block, 100 * block + 100):
        dag, main, side, ess = planted(seed)
        total += _check(dag, main, side, ess, f"seed {seed}")
    assert total > 1000                                                     # the graphs are not all chains


@pytest.mark.parametrize("name", list(HAND))
def test_the_patterns_of_the_forward(name):
    dag, main, side, ess = _hand(name)
    assert _check(dag, main, side, ess, name) > 0


def test_an_essential_edge_removed_inverts_its_pair():
    """What the sharpness runs do: without an essential fork the side-earliest order, without an essential join the side-latest order
    (on the chains of the whole graph) runs the edge's consumer in front of its producer."""
    for name in HAND:
        dag, main, side, ess = _hand(name)
        for a, b in ess:
            o = fg.order(dag.without((a, b)), "side" if b in side else "main", (main, side))
            assert o.index(b) < o.index(a), (name, a, b)


def test_three_chains_are_refused():
    dag = Dag(7, [(0, 1), (1, 2), (2, 3), (3, 4), (0, 5), (0, 6), (5, 4)], names=list("abcdefg"))
    with pytest.raises(ValueError, match=r"not two chains: nodes 5 \(f\) and 6 \(g\) are both off the longest path \(5 of 7 nodes\)"):
        fg.two_chains(dag)
    with pytest.raises(ValueError, match="not two chains"):
        fg.order(dag, "side")


def test_leftover_nodes_that_are_no_chain_are_refused():
    """Two chains 0..4 and 5..8 with one edge 7 -> 2: the longest path 5 6 7 2 3 4 leaves 0, 1 and 8, of which 8 is unordered with both."""
    dag = Dag(9, [(0, 1), (1, 2), (2, 3), (3, 4), (5, 6), (6, 7), (7, 8), (7, 2)])
    assert len(fg.unordered_pairs(dag)) > 0
    with pytest.raises(ValueError, match=r"not two chains: nodes \d \(node\d\) and 8 \(node8\) are both off the longest path \(6 of 9 nodes\)"):
        fg.two_chains(dag)


def test_cycles_and_bad_edges_are_refused():
    with pytest.raises(ValueError, match="cycle"):
        Dag(3, [(0, 1), (1, 2), (2, 0)])
    with pytest.raises(ValueError, match="edge"):
        Dag(2, [(0, 2)])


def test_kernel_names_mangled_and_plain():
    fused = "_ZN6pivlfn16conv_c3k7_kernelILb1ELi0EEEvNS_10ConvParamsENS_9Conv1FuseE"
    plain = "_ZN6pivlfn16conv_c3k7_kernelILb0ELi0EEEvNS_10ConvParamsENS_9Conv1FuseE"
    assert fg.kernel_is(fused, "conv_c3k7_kernel") and fg.kernel_is(fused, "conv_c3k7_kernel", True)
    assert fg.kernel_is(plain, "conv_c3k7_kernel") and not fg.kernel_is(plain, "conv_c3k7_kernel", True)
    assert fg.kernel_is(plain, "conv_c3k7_kernel", False) and not fg.kernel_is(fused, "c3k7_kernel")
    assert fg.kernel_is("_ZN6pivlfn12touch_kernelEPKDv4_fmPf", "touch_kernel") and not fg.kernel_is("_ZN6pivlfn13touch_kernel2EPKf", "touch_kernel")
    assert fg.kernel_is("void pivlfn::conv_c3k7_kernel<true, 0>(pivlfn::ConvParams, pivlfn::Conv1Fuse)", "conv_c3k7_kernel", True)
    assert not fg.kernel_is("void pivlfn::conv_c3k7_kernel<false, 0>(pivlfn::ConvParams, pivlfn::Conv1Fuse)", "conv_c3k7_kernel", True)
    assert fg.kernel_is("pivlfn::reg_r0_tail_kernel<8>(float const*)", "reg_r0_tail_kernel") and not fg.kernel_is("<kernel 1234>", "touch_kernel")
    assert not fg.kernel_is("pivlfn::retouch_kernel(float*)", "touch_kernel")


def test_every_graph_call_resolves_in_the_loaded_runtime():
    """dlsym of every symbol forward_graph.py binds, in the libamdhip64 that torch has loaded; no device is needed for that."""
    path = fg.runtime_path()
    with open("/proc/self/maps") as f:
        assert any(ln.rstrip().endswith(path) for ln in f)
    lib = fg.runtime()
    assert len(fg.SIGNATURES) == 15
    for name, (res, args) in fg.SIGNATURES.items():
        fn = getattr(lib, name)                       # AttributeError: the runtime does not export it
        assert fn.restype is res and list(fn.argtypes) == args, name
