"""CPU: tests/analysis_plans.py against the sources and against itself.  The constexpr values its formulas use are read out of the .hip
text; where the library can be asked for a plan (the pressure workspace) it is; and every case of its lists crosses the branch it is
named for."""
import inspect
import os
import re

import pytest

import analysis_plans as ap


@pytest.mark.parametrize("name", sorted(ap.CONSTANTS))
def test_the_constants_are_the_sources(name):
    found = ap.source_constants(name)
    for key, value in ap.CONSTANTS[name].items():
        assert key in found, f"csrc/{name} no longer defines constexpr {key}: tests/analysis_plans.py restates a plan that is gone"
        assert found[key] == value, f"csrc/{name}: {key} = {found[key]}, tests/analysis_plans.py assumes {value}: its cases may miss their branches"


def test_the_formulas_are_the_sources():
    """The expressions the restated plans copy, as they stand in the launchers (whitespace apart)."""
    squeeze = lambda s: re.sub(r"\s+", "", s)      # noqa: E731
    want = {
        # the partials plan and the tree stand once, in the header; pr_layout and sm_layout call pr_plan
        "cg_shared.h": ["chunks = P2 > (size_t)PR_CHUNK * PR_MAX_PART ? P2 / ((size_t)PR_CHUNK * PR_MAX_PART) : 1",
                        "tile = chunks * PR_CHUNK, NB = (N + tile - 1) / tile", "c * PR_CHUNK < NB"],
        "pressure.hip": ["plan = pr_plan(N)"],
        "smooth.hip": ["plan = pr_plan(N)", "grid((unsigned)cdiv(W, DC_BLK), (unsigned)cdiv(H, DC_BLK), (unsigned)P)",
                       "m0 = blockIdx.y * DC_BLK, n0 = blockIdx.x * DC_BLK", "chunks = (p.K + DC_KC - 1) / DC_KC", "a.K = W", "b.K = H"],
        "calibrate.hip": ["per = (nblk + 255) / 256", "lo = min((int)threadIdx.x * per, nblk), hi = min(lo + per, nblk)",
                          "nblk = (hw + TP_BLOCK - 1) / TP_BLOCK"],
        "twopoint.hip": ["p.chunks = (1 << p.levels) > TP_CHUNK ? (1 << p.levels) / TP_CHUNK : 1",
                         "groups = cdiv(max_sep + 1, TP_WAVES), want = cdiv(4096, H)", "z = want < groups ? want : groups",
                         "p.slots = cdiv(max_sep + 1, TP_WAVES * z)", "lds = (size_t)TP_WAVES * p.slots * TP_SLOT * sizeof(double)"],
        # the frame-grid rule stands once, in the header; each of its nine call sites calls it (no private copy can come back unnoticed)
        "launch_checks.h": ["g = (items + FRAME_GRID_THREADS - 1) / FRAME_GRID_THREADS",
                            "cap = FRAME_GRID_BLOCKS / (size_t)frames > FRAME_GRID_MIN_BLOCKS ? FRAME_GRID_BLOCKS / (size_t)frames : FRAME_GRID_MIN_BLOCKS",
                            "return (unsigned)(g > cap ? cap : g)"],
        "postpro.hip": ["dim3 grid(frame_grid((size_t)H * W, B), (unsigned)B)", "flow_stats_kernel, dim3(frame_grid((size_t)H * W, 1))",
                        "flow_stats_masked_kernel, dim3(frame_grid((size_t)H * W, 1))"],
        "validate.hip": ["dim3 grid(frame_grid((size_t)H * W, B), (unsigned)B)"],
        "quality.hip": ["dim3 wgrid(frame_grid((size_t)H * W, B), (unsigned)B)"],
        "vortex.hip": ["vortex_stage_kernel, dim3(frame_grid((size_t)H * W, B), (unsigned)B)"],
        "stereo.hip": ["stereo_2d3c_kernel, dim3(frame_grid((size_t)H * W, B), (unsigned)B)"],
        "uncertainty.hip": ["unc_fields_kernel, dim3(frame_grid((size_t)H * W, B), (unsigned)B)"],
        "preproc.hip": ["dim3 grid(frame_grid(vec ? HW / 4 : HW, n), (unsigned)n)", "blocks = frame_grid(vec ? bytes / 4 : bytes, 1)"],
        "evaluate.hip": ["error_stats_kernel, dim3(frame_grid((size_t)H * W, 1))"],
        "viz.hip": ["g = (items + VZ_THREADS - 1) / VZ_THREADS", "g > VZ_MAX_BLOCKS ? VZ_MAX_BLOCKS : (g ? g : 1)", "gx = viz_blocks((HW + 3) / 4)",
                    "gx = viz_blocks(HW)", "gx > 256 ? 256 : gx", "viz_blocks((npix + 3) / 4)", "viz_blocks(ncells)"],
        "particles.hip": ["tiles = (size_t)B * cdiv(H, REN_TILE) * cdiv(W, REN_TILE)", "tb = (unsigned)((tiles + 255) / 256)"],
        "spectrum.hip": ["nfull = K / SP_KG, nsingle = K % SP_KG", "rounds = nfull ? (nfull + SP_WAVES - 1) / SP_WAVES : 1"],
        "pod.hip": ["if (K <= 4)", "else if (K <= 16)"],
    }
    for name, lines in want.items():
        text = squeeze(open(os.path.join(ap.CSRC, name)).read())
        for line in lines:
            assert squeeze(line) in text, f"csrc/{name} no longer holds `{line}`: restate the plan in tests/analysis_plans.py and revisit its cases"
    for name in sorted(os.listdir(ap.CSRC)):
        if name.endswith(".hip"):
            text = squeeze(open(os.path.join(ap.CSRC, name)).read())
            assert "16384/(size_t)" not in text, f"csrc/{name} has a frame-grid cap of its own"
            assert "PR_CHUNK*PR_MAX_PART" not in text, f"csrc/{name} has a partials plan of its own: call pr_plan of cg_shared.h"
            assert "PR_CHUNK" not in ap.source_constants(name) and "PR_CHUNK=" not in text, f"csrc/{name} defines PR_CHUNK: the tree is cg_shared.h's"


@pytest.mark.parametrize("op,case", [(op, c) for op, cases in ap.ALL_CASES.items() for c in cases], ids=lambda v: v if isinstance(v, str) else str(v.shape))
def test_every_case_crosses_its_branch(op, case):
    nargs = len(inspect.signature(case.plan).parameters)
    plan = case.plan(*case.shape[:nargs])
    assert case.crosses(plan), f"{op} {case.shape} was to reach `{case.branch}`, its plan is {plan}"


def test_the_smaller_neighbour_of_a_case_stays_below_its_branch():
    """One step down and the branch is not taken: the cases are the first sizes, not just large ones."""
    assert ap.pressure(512, 512) == {"N": 1 << 18, "chunks": 1, "NB": 256} and ap.pressure(1024, 1024)["NB"] == 1024
    assert ap.pressure(2048, 1024)["chunks"] == 1 and ap.pressure(2048, 2048)["chunks"] == 2
    assert ap.smooth_solve(24, 20)["NB"] == 1 and ap.smooth_solve(33, 17)["NB"] == 1 and ap.smooth_solve(64, 64)["dct"]["blocks"] == 1
    assert ap.dct(64, 64) == {"grid": (1, 1), "blocks": 1, "ragged": (False, False), "chunks": (2, 2)} and ap.dct(65, 130)["grid"] == (3, 2)
    assert ap.tp_scan(256, 256)["per"] == 1 and ap.tp_scan(192, 320) == {"nblk": 240, "per": 1, "short": [], "empty": list(range(240, 256))}
    assert ap.twopoint(65, 300, 255)["slots"] == 1 and ap.twopoint(70, 131, 16)["slots"] == 1 and ap.twopoint(20, 300, 255)["chunks"] == 2
    assert ap.twopoint(5, 512, 8)["chunks"] == 2 and ap.twopoint(1024, 1024, 64) == {"levels": 10, "chunks": 4, "z": 4, "slots": 5, "lds": 2560}
    assert ap.capped_frame_grid(128 * 128, 256)["visits"] == 1 and ap.capped_frame_grid(2048 * 2048, 1)["visits"] == 1
    assert ap.capped_frame_grid(1024 * 1024, 3)["visits"] == 1           # the largest case of the older analysis ops: below the cap
    assert ap.capped_frame_grid(130 * 128, 52)["visits"] == 1            # the five calls of 52 frames the capped cases are compared with
    assert ap.capped_frame_grid(256 * 256 // 4, 260)["visits"] == 1 and ap.capped_frame_grid(128 * 128, 260)["visits"] == 1
    assert ap.viz_absmax(256, 256)["blocks"] == 256 and ap.viz_maxrad(512, 512)["blocks"] == 256
    assert ap.viz_color(4, 1024, 1024)["blocks"] == ap.VZ_MAX_BLOCKS and ap.viz_color(1, 67, 131)["grid"] == 9
    assert ap.particles_tiles(1, 37, 53)["tiles"] == 12 and ap.particles_tiles(1, 16, 1024)["waves"] == 1
    assert ap.spectrum(256, 129) == {"chunks": 2, "groups": 16, "singles": 1, "rounds": 2}


def test_the_library_gives_the_partials_of_the_pressure_plan():
    """pivlfn_pressure_workspace_offset(F, h, w, PIVLFN_PRESSURE_WS_B) = 128 F + 24 NB F: the two records of 64 bytes and the three
    arrays of block partials that lie in front of b.  A host-only query: no device is touched."""
    from pivlfn import _lib
    lib = _lib.load()
    shapes = ap.shapes(ap.PRESSURE_CASES) + [(1, 1), (70, 131), (512, 512), (1024, 1024), (2048, 2048), (1, 1 << 23), (4096, 4096)]
    for h, w in shapes:
        for F in (1, 2, 3):
            if F * h * w < 1 << 31:
                assert lib.pivlfn_pressure_workspace_offset(F, h, w, 0) == ap.pressure_offset_b(F, h, w), (F, h, w)
    assert ap.pressure(4096, 4096) == {"N": 1 << 24, "chunks": 8, "NB": 2048}


def test_the_table_names_every_analysis_entry_point():
    """The docstring of tests/analysis_plans.py names every entry point of include/pivlfn.h between pivlfn_stereo_2d3c and the network's
    own (pivlfn_create): a new one has to be entered there, with its size steps or `none`."""
    header = open(os.path.join(os.path.dirname(ap.CSRC), "..", "include", "pivlfn.h")).read()
    names = re.findall(r"^(?:int|size_t)\s+(pivlfn_\w+)\(", header, re.M)
    first, last = names.index("pivlfn_stereo_2d3c"), names.index("pivlfn_create")
    analysis = [n for n in names[first:last] if not n.endswith("_workspace_bytes") and not n.endswith("_workspace_offset")]
    assert len(analysis) >= 33 and "pivlfn_dewarp_frames" in analysis and "pivlfn_pressure_cg" in analysis
    analysis += ["pivlfn_flow_uncertainty", "pivlfn_uncertainty_accumulate"]          # declared at the end of the header
    assert set(analysis[-2:]) <= set(names)
    doc = ap.__doc__
    expand = {"pivlfn_pressure_setup / _cg / _read": ["pivlfn_pressure_setup", "pivlfn_pressure_cg", "pivlfn_pressure_read"],
              "pivlfn_flowmap_advect / _seed / _ftle": ["pivlfn_flowmap_advect", "pivlfn_flowmap_seed", "pivlfn_flowmap_ftle"],
              "pivlfn_flow_stats_accumulate(_masked)": ["pivlfn_flow_stats_accumulate", "pivlfn_flow_stats_accumulate_masked"]}
    named = set(re.findall(r"pivlfn_\w+", doc))
    for text, members in expand.items():
        if text in doc:
            named.update(members)
    missing = [n for n in analysis if n not in named]
    assert not missing, f"tests/analysis_plans.py does not say where the plans of {missing} change"
