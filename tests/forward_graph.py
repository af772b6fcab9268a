"""The dependency graph of a captured pivlfn_forward: what HIP hands back for it, and the two orders that realise both orders of every
pair of launches it leaves unordered.  A helper, not a test: tests/test_forward_graph.py checks the graph algorithms on the CPU,
tests/forward_graph_cases.py uses all of it on the GPU (the argument is in that file's docstring).

Two halves.  The lower one is plain Python on (n_nodes, edges) and needs no device: reachability, the decomposition into a main and a
side chain, Kahn's algorithm with a preferred chain, the unordered pairs and the essential cross edges.  The upper one is a ctypes
binding of the HIP graph calls on the libamdhip64 the process has already loaded (no second runtime is opened), a capture through
torch.cuda.CUDAGraph(keep_graph=True), and linearised(): a clone of a captured graph with an edge between every two consecutive
nodes of an order, i.e. the same launches as one chain."""
import ctypes
import re


# ---- pure Python on (n_nodes, edges) ------------------------------------------------------------------------------------------
class Dag:
    """n nodes 0..n-1 and a set of edges (a, b): a runs before b.  names[i] is only for messages."""

    def __init__(self, n, edges, names=None):
        self.n = int(n)
        self.edges = sorted({(int(a), int(b)) for a, b in edges})
        for a, b in self.edges:
            if not (0 <= a < self.n and 0 <= b < self.n) or a == b:
                raise ValueError(f"edge ({a}, {b}) in a graph of {self.n} nodes")
        self.names = list(names) if names is not None else [f"node{i}" for i in range(self.n)]
        self.succ = [[] for _ in range(self.n)]
        self.pred = [[] for _ in range(self.n)]
        for a, b in self.edges:
            self.succ[a].append(b)
            self.pred[b].append(a)
        self.topo = self._topological()
        self.reach = self._reachability()

    def _topological(self):
        left = [len(p) for p in self.pred]
        ready = [i for i in range(self.n) if not left[i]]
        out = []
        while ready:
            v = ready.pop()
            out.append(v)
            for s in self.succ[v]:
                left[s] -= 1
                if not left[s]:
                    ready.append(s)
        if len(out) != self.n:
            raise ValueError("the graph has a cycle")
        return out

    def _reachability(self):
        """reach[a]: a bit set of the nodes b != a with a path a -> b."""
        reach = [0] * self.n
        for v in reversed(self.topo):
            r = 0
            for s in self.succ[v]:
                r |= reach[s] | (1 << s)
            reach[v] = r
        return reach

    def before(self, a, b):
        """True if a path leads from a to b."""
        return bool(self.reach[a] >> b & 1)

    def ordered(self, a, b):
        return self.before(a, b) or self.before(b, a)

    def without(self, edge):
        assert tuple(edge) in self.edges
        return Dag(self.n, [e for e in self.edges if e != tuple(edge)], self.names)

    def label(self, v):
        return f"{v} ({self.names[v]})"


def two_chains(dag):
    """-> (main, side): the main chain is the longest path (the first found among equals), the remaining nodes, which must be totally
    ordered by reachability, are the side chain; both in running order.  Anything else is refused: a graph of width 3 or more, or one
    whose nodes off the longest path are no chain, is not the schedule of two streams."""
    length, nxt = [1] * dag.n, [-1] * dag.n
    for v in reversed(dag.topo):
        for s in sorted(dag.succ[v]):
            if length[s] + 1 > length[v]:
                length[v], nxt[v] = length[s] + 1, s
    if not dag.n:
        return [], []
    v = max(range(dag.n), key=lambda i: (length[i], -i))
    main = []
    while v >= 0:
        main.append(v)
        v = nxt[v]
    on_main = set(main)
    place = {v: k for k, v in enumerate(dag.topo)}
    side = sorted((v for v in range(dag.n) if v not in on_main), key=place.get)
    for a, b in zip(side, side[1:]):                 # reachability is transitive: consecutive pairs are enough
        if not dag.before(a, b):
            a, b = sorted((a, b))
            raise ValueError(f"not two chains: nodes {dag.label(a)} and {dag.label(b)} are both off the longest path "
                             f"({len(main)} of {dag.n} nodes) and neither runs before the other -- a third stream?")
    return main, side


def order(dag, prefer, chains=None):
    """A topological order by Kahn's algorithm that always takes a ready node of the preferred chain ("side" or "main") first: the side
    chain as early, or as late, as the edges allow.  chains: (main, side) of another graph on the same nodes (one with an edge more)."""
    if prefer not in ("side", "main"):
        raise ValueError(prefer)
    main, side = chains if chains is not None else two_chains(dag)
    first, second = (side, main) if prefer == "side" else (main, side)
    rank = {v: (0, k) for k, v in enumerate(first)}
    rank.update({v: (1, k) for k, v in enumerate(second)})
    assert len(rank) == dag.n
    left = [len(p) for p in dag.pred]
    ready = {v for v in range(dag.n) if not left[v]}
    out = []
    while ready:
        v = min(ready, key=rank.get)
        ready.remove(v)
        out.append(v)
        for s in dag.succ[v]:
            left[s] -= 1
            if not left[s]:
                ready.add(s)
    assert len(out) == dag.n
    return out


def unordered_pairs(dag):
    """The pairs (a, b), a < b, that no path connects either way."""
    return [(a, b) for a in range(dag.n) for b in range(a + 1, dag.n) if not dag.ordered(a, b)]


def cross_edges(dag, chains=None):
    main, side = chains if chains is not None else two_chains(dag)
    on_side = set(side)
    return [(a, b) for a, b in dag.edges if (a in on_side) != (b in on_side)]


def essential_cross_edges(dag, chains=None):
    """The edges between the chains whose removal leaves their two ends unordered: the forks (main -> side) and joins (side -> main)
    that carry an ordering no other path carries."""
    out = []
    for a, b in cross_edges(dag, chains):
        if not any(c != b and dag.before(c, b) for c in dag.succ[a]):
            out.append((a, b))
    return out


def first_inverted_pair(dag, this, other):
    """The first pair (u, v) in running order `this` -- u runs before v -- that runs the other way round in `other`, or None."""
    where = {v: k for k, v in enumerate(other)}
    for k, v in enumerate(this):
        for u in this[:k]:
            if where[u] > where[v]:
                return u, v
    return None


# ---- kernel names ---------------------------------------------------------------------------------------------------------------------
def kernel_is(name, base, first_bool=None):
    """Whether a kernel name as the runtime gives it, mangled (_ZN6pivlfn16conv_c3k7_kernelILb1ELi0EEEv...) or not
    (void pivlfn::conv_c3k7_kernel<true, 0>(...)), is the function `base`; first_bool: and its first template argument is that bool."""
    if name.startswith("_Z"):
        key = f"{len(base)}{base}"
        if first_bool is not None:
            key += "ILb1E" if first_bool else "ILb0E"
        return re.search(r"(?<![0-9])" + re.escape(key), name) is not None           # the length in front makes the match whole
    m = re.search(r"(?<![A-Za-z0-9_])" + re.escape(base) + r"(?![A-Za-z0-9_])\s*(<\s*(true|false))?", name)
    if m is None:
        return False
    return first_bool is None or m.group(2) == ("true" if first_bool else "false")


def short_name(name):
    """pivlfn::conv_c3k7_kernel<true,0> from _ZN6pivlfn16conv_c3k7_kernelILb1ELi0EEEv...: the nested name and its literal template
    arguments, for messages.  A name that is not mangled comes back as it is."""
    m = re.match(r"_ZN?", name)
    if not m:
        return name
    at, parts = m.end(), []
    while True:
        d = re.match(r"\d+", name[at:])
        if not d:
            break
        at += d.end()
        parts.append(name[at:at + int(d.group())])
        at += int(d.group())
    args = []
    if name[at:at + 1] == "I":
        at += 1
        while True:
            lit = re.match(r"L([a-z])(n?\d+)E", name[at:])
            if not lit:
                break
            args.append({"0": "false", "1": "true"}[lit.group(2)] if lit.group(1) == "b" else lit.group(2).replace("n", "-"))
            at += lit.end()
    return "::".join(parts) + (f"<{','.join(args)}>" if args else "") if parts else name


# ---- the HIP graph calls ----------------------------------------------------------------------------------------------------------------
class Dim3(ctypes.Structure):
    _fields_ = [("x", ctypes.c_uint32), ("y", ctypes.c_uint32), ("z", ctypes.c_uint32)]


class KernelNodeParams(ctypes.Structure):
    """struct hipKernelNodeParams"""
    _fields_ = [("blockDim", Dim3), ("extra", ctypes.c_void_p), ("func", ctypes.c_void_p), ("gridDim", Dim3),
                ("kernelParams", ctypes.c_void_p), ("sharedMemBytes", ctypes.c_uint)]


_P, _PP, _SZ = ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t
# name -> (restype, argtypes), as hip_runtime_api.h of ROCm 7 declares them
SIGNATURES = {
    "hipGraphGetNodes": (ctypes.c_int, [_P, _PP, ctypes.POINTER(_SZ)]),
    "hipGraphGetEdges": (ctypes.c_int, [_P, _PP, _PP, ctypes.POINTER(_SZ)]),
    "hipGraphNodeGetType": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int)]),
    "hipGraphKernelNodeGetParams": (ctypes.c_int, [_P, ctypes.POINTER(KernelNodeParams)]),
    "hipKernelNameRefByPtr": (ctypes.c_char_p, [_P, _P]),
    "hipGraphClone": (ctypes.c_int, [_PP, _P]),
    "hipGraphNodeFindInClone": (ctypes.c_int, [_PP, _P, _P]),
    "hipGraphAddDependencies": (ctypes.c_int, [_P, _PP, _PP, _SZ]),
    "hipGraphRemoveDependencies": (ctypes.c_int, [_P, _PP, _PP, _SZ]),
    "hipGraphInstantiate": (ctypes.c_int, [_PP, _P, _PP, ctypes.c_char_p, _SZ]),
    "hipGraphLaunch": (ctypes.c_int, [_P, _P]),
    "hipGraphExecDestroy": (ctypes.c_int, [_P]),
    "hipGraphDestroy": (ctypes.c_int, [_P]),
    # only if torch's keep_graph is not to be had: capture on a stream handle through the same runtime
    "hipStreamBeginCapture": (ctypes.c_int, [_P, ctypes.c_int]),
    "hipStreamEndCapture": (ctypes.c_int, [_P, _PP]),
}
NODE_TYPES = ("kernel", "memcpy", "memset", "host", "graph", "empty", "wait-event", "event-record", "semaphore-signal", "semaphore-wait",
              "mem-alloc", "mem-free", "memcpy-from-symbol", "memcpy-to-symbol", "batch-mem-op")
_runtime = None


def runtime_path():
    """The libamdhip64 this process has mapped (torch loads it); binding that file again gives the loaded library, not a second one."""
    import torch  # noqa: F401
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if re.search(r"/libamdhip64\.so[.0-9]*$", ln.split()[-1])})
    if len(paths) != 1:
        raise RuntimeError(f"expected one loaded libamdhip64, found {paths}")
    return paths[0]


def runtime():
    global _runtime
    if _runtime is None:
        lib = ctypes.CDLL(runtime_path())
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _runtime = lib
    return _runtime


def _ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed with hipError_t {rc}")


def _array(handles):
    return (ctypes.c_void_p * len(handles))(*handles)


class Graph:
    """A hipGraph_t and its nodes in a fixed numbering: a clone numbers its nodes as the graph it was cloned from."""

    def __init__(self, handle, nodes=None, owned=False):
        self.hip, self.handle, self.owned = runtime(), int(handle), owned
        self.nodes = list(nodes) if nodes is not None else self._get_nodes()

    def _get_nodes(self):
        n = _SZ(0)
        _ok(self.hip.hipGraphGetNodes(self.handle, None, ctypes.byref(n)), "hipGraphGetNodes")
        buf = (ctypes.c_void_p * max(1, n.value))()
        _ok(self.hip.hipGraphGetNodes(self.handle, buf, ctypes.byref(n)), "hipGraphGetNodes")
        return [int(buf[i]) for i in range(n.value)]

    def edges(self):
        """[(a, b)] in this graph's numbering."""
        n = _SZ(0)
        _ok(self.hip.hipGraphGetEdges(self.handle, None, None, ctypes.byref(n)), "hipGraphGetEdges")
        a, b = (ctypes.c_void_p * max(1, n.value))(), (ctypes.c_void_p * max(1, n.value))()
        _ok(self.hip.hipGraphGetEdges(self.handle, a, b, ctypes.byref(n)), "hipGraphGetEdges")
        index = {h: i for i, h in enumerate(self.nodes)}
        return [(index[int(a[i])], index[int(b[i])]) for i in range(n.value)]

    def names(self):
        """Per node: the kernel's name, or <type> for a node that is no kernel."""
        out = []
        for h in self.nodes:
            t = ctypes.c_int(-1)
            _ok(self.hip.hipGraphNodeGetType(h, ctypes.byref(t)), "hipGraphNodeGetType")
            if t.value != 0:
                out.append(f"<{NODE_TYPES[t.value] if 0 <= t.value < len(NODE_TYPES) else t.value}>")
                continue
            p = KernelNodeParams()
            _ok(self.hip.hipGraphKernelNodeGetParams(h, ctypes.byref(p)), "hipGraphKernelNodeGetParams")
            name = self.hip.hipKernelNameRefByPtr(p.func, None) if p.func else None
            out.append(name.decode() if name else f"<kernel {p.func}>")
        return out

    def dag(self):
        return Dag(len(self.nodes), self.edges(), self.names())

    def clone(self):
        """A copy the caller owns, with the same nodes (in this graph's numbering) and the same edges."""
        c = ctypes.c_void_p()
        _ok(self.hip.hipGraphClone(ctypes.byref(c), self.handle), "hipGraphClone")
        mapped = []
        for h in self.nodes:
            m = ctypes.c_void_p()
            _ok(self.hip.hipGraphNodeFindInClone(ctypes.byref(m), h, c), "hipGraphNodeFindInClone")
            mapped.append(int(m.value))
        g = Graph(c.value, mapped, owned=True)
        assert len(set(mapped)) == len(self.nodes) and sorted(g._get_nodes()) == sorted(mapped), "the clone has other nodes"
        assert sorted(set(g.edges())) == sorted(set(self.edges())), "the clone has other edges"
        return g

    def add_edges(self, edges):
        if edges:
            _ok(self.hip.hipGraphAddDependencies(self.handle, _array([self.nodes[a] for a, _ in edges]),
                                                 _array([self.nodes[b] for _, b in edges]), len(edges)), "hipGraphAddDependencies")

    def remove_edge(self, edge):
        a, b = edge
        _ok(self.hip.hipGraphRemoveDependencies(self.handle, _array([self.nodes[a]]), _array([self.nodes[b]]), 1),
            "hipGraphRemoveDependencies")

    def instantiate(self):
        return Exec(self)

    def destroy(self):
        if self.owned and self.handle:
            _ok(self.hip.hipGraphDestroy(self.handle), "hipGraphDestroy")
            self.handle = 0


class Exec:
    def __init__(self, graph):
        self.hip = graph.hip
        e = ctypes.c_void_p()
        _ok(self.hip.hipGraphInstantiate(ctypes.byref(e), graph.handle, None, None, 0), "hipGraphInstantiate")
        self.handle = e.value

    def launch(self, stream):
        _ok(self.hip.hipGraphLaunch(self.handle, stream), "hipGraphLaunch")

    def destroy(self):
        if self.handle:
            _ok(self.hip.hipGraphExecDestroy(self.handle), "hipGraphExecDestroy")
        self.handle = 0


def linearised(graph, order_):
    """A clone of `graph` with an edge added between consecutive nodes of `order_` (node numbers) where there is none: the same
    launches as one chain.  The clone is checked to have the graph's nodes and edges before any is added."""
    assert sorted(order_) == list(range(len(graph.nodes)))
    g = graph.clone()
    have = set(g.edges())
    g.add_edges([(a, b) for a, b in zip(order_, order_[1:]) if (a, b) not in have])
    chain = Dag(len(g.nodes), g.edges())
    assert not unordered_pairs(chain) and chain.topo == list(order_), "the linearised clone is not the chain asked for"
    return g


def capture(enqueue, dev):
    """Capture enqueue(stream handle) -> (keep-alive object, Graph).  torch's own capture with keep_graph=True; where that is not to be
    had, hipStreamBeginCapture / hipStreamEndCapture on a torch side stream's handle through the same binding."""
    import torch
    try:
        g = torch.cuda.CUDAGraph(keep_graph=True)
        raw = g.raw_cuda_graph
    except (TypeError, AttributeError):
        g = raw = None
    if g is not None:
        with torch.cuda.graph(g):
            enqueue(torch.cuda.current_stream(dev).cuda_stream)
        return g, Graph(raw())
    hip, s, h = runtime(), torch.cuda.Stream(dev), ctypes.c_void_p()
    s.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    _ok(hip.hipStreamBeginCapture(s.cuda_stream, 0), "hipStreamBeginCapture")
    try:
        enqueue(s.cuda_stream)
    finally:
        _ok(hip.hipStreamEndCapture(s.cuda_stream, ctypes.byref(h)), "hipStreamEndCapture")
    graph = Graph(h.value, owned=True)
    return (s, graph), graph
