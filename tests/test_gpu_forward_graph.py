"""GPU: the two-stream schedule of pivlfn_forward on the dependency graph of its captured forward.  The cases, and the argument why two
total orders of the captured launches cover both orders of every pair the graph leaves unordered, are in tests/forward_graph_cases.py;
the graph algorithms are checked on the CPU in tests/test_forward_graph.py."""
import os
import re
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu


def test_forward_graph_cases_in_a_process_of_their_own(dev):
    """tests/forward_graph_cases.py in a fresh pytest process: 13 tests, all passing, a table line for each of their 13 captures, the
    verdict on the three replays of 11 of them and a line for each essential edge the two sharpness cases remove.  Why not in this process:
    tests/test_gpu_flowmap.py::test_stream_contract_and_run_py_in_a_process_of_their_own says it."""
    here = os.path.dirname(os.path.abspath(__file__))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "pytest", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                                                                          os.path.join(here, "forward_graph_cases.py")]
    t0 = time.time()
    r = subprocess.run(cmd, cwd=here, capture_output=True, text=True, timeout=600)
    lines = [ln[ln.index("forward-graph"):] for ln in r.stdout.splitlines() if "forward-graph" in ln]       # behind pytest's progress dots
    print("\n".join(lines))
    print(f"forward-graph wall time: {time.time() - t0:.0f} s")
    assert r.returncode == 0 and re.search(r"\b13 passed", r.stdout), r.stdout[-8000:] + r.stderr[-2000:]
    assert len([ln for ln in lines if ln.startswith("forward-graph |")]) == 13 and len([ln for ln in lines if ln.startswith("forward-graph replays |")]) == 11
    edges = [ln for ln in lines if ln.startswith("forward-graph edge |")]
    assert len(edges) >= 4 and all("| detected: " in ln for ln in edges), edges
