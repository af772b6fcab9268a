"""The host-side launch plans of the analysis kernels, restated, and the shapes at which they change.  A helper, not a test:
tests/test_analysis_plans.py holds it to the sources (the constexpr values below are read back out of the .hip text) and shows that every
case crosses the branch it is named for; the tests/test_gpu_*.py of each op take their large shapes from the lists at the end.

Every analysis entry point of include/pivlfn.h, the size steps of its launcher, and the test that reaches each.  A later kernel gets a
line here, and a case where its plan has a step.

  pivlfn_pressure_gradient        none: one thread per node, a flat grid.
  pivlfn_pressure_setup / _cg / _read   NB = ceil(N / (chunks * 1024)) block partials per frame; NB > 256 puts partials into a second wave
                                  of pr_finish, NB > 1024 into its second chunk, N > 2^21 starts the PrCounter (chunks = 2), N > 2^22
                                  carries in it (chunks = 4).  PRESSURE_CASES, test_gpu_pressure.py::test_bits_where_the_partials_plan_changes.
  pivlfn_smooth_setup / _pcg / _read   the same plan (pr_plan of csrc/cg_shared.h) with N = H W per system, a system being one component of
                                  a frame.  SMOOTH_CASES, test_gpu_smooth.py::test_bb_where_the_partials_plan_changes (the setup
                                  alone).  SMOOTH_SOLVE_CASES iterate: NB = 3 with a ragged last tile and rows that straddle a
                                  thread's four nodes (37 x 61), NB = 9 (70 x 131), NB = 257 (513 x 512);
                                  test_gpu_smooth.py::test_rr_follows_the_restated_iteration, test_solve_against_the_sparse_operator,
                                  test_batch_cuts_and_frozen_systems, test_guarded_solve.  The matrix products of the
                                  preconditioner are pivlfn_dct2's.
  pivlfn_dct2                     none in P (grid z); ceil(W / 64) x ceil(H / 64) workgroups a plane and ceil(K / 32) staged chunks of
                                  the inner index, ragged edges staged as +0.0 (dct below): the shapes of
                                  test_gpu_smooth.py::test_dct2_against_scipy ((63, 65), (64, 64), (65, 130), (129, 31): around a tile
                                  and around a chunk).  With the Gamma epilogue and the skip of stopped planes: SMOOTH_SOLVE_CASES,
                                  70 x 131 being 3 x 2 ragged blocks a plane with 5 and 3 chunks of the inner index.
  pivlfn_template_match           none in H, W (64 x 16 tiles, a flat 3-D grid); the template steps the packed row length and, from
                                  64 KiB of LDS on, the opt-in attribute: test_gpu_calibrate.py::test_match_reaches_the_32_bit_headroom
                                  (255 x 255) and the 25 x 25 / 5 x 5 cases of test_match_bits_of_the_restatement.
  pivlfn_target_points            nblk = ceil(HW / 256) blocks; tp_scan_kernel gives per = ceil(nblk / 256) of them to a thread:
                                  per = 2 from HW > 65536.  TARGET_POINTS_CASES, test_gpu_calibrate.py::test_points_where_the_scan_plan_changes.
  pivlfn_dewarp_frames            none: one thread per pixel, grid (ceil(HW / 256), B), no cap.
  pivlfn_twopoint_accumulate      slots = ceil((R + 1) / (4 z)) separations per wave, z = min(ceil(4096 / H), ceil((R + 1) / 4)):
                                  slots = 2 from H = 66 at R = 255; chunks = 2^levels / 256 of a row: 4 from W = 513, 64 at W = 16384.
                                  TWOPOINT_CASES, test_gpu_twopoint.py::test_bits_where_the_plan_changes.
  pivlfn_spectrum_accumulate      bounded domain (L <= 1024, K <= 513): ceil(L / 128) staged chunks, ceil((K // 8) / 8) rounds, K % 8
                                  singles.  SPECTRUM_CASES (the corner L = 1024, K = 513) in test_gpu_spectrum.py::test_bits_of_the_restatement.
  pivlfn_vortex_gamma             vortex_stage_kernel: frame_grid of csrc/launch_checks.h, min(ceil(HW / 256), max(16384 / B, 64)) blocks per
                                  frame and a grid-stride loop above; vortex_window_kernel: flat.  VORTEX_CASES,
                                  test_gpu_vortex.py::test_bits_where_the_stage_grid_is_capped.
  pivlfn_match_quality            quality_warp_kernel: frame_grid; quality_window_kernel: flat.  QUALITY_CASES,
                                  test_gpu_quality.py::test_bits_where_the_warp_grid_is_capped.
  pivlfn_flow_uncertainty         quality_warp_kernel and unc_fields_kernel: frame_grid; the three tiled kernels: flat.  UNCERTAINTY_CASES,
                                  test_gpu_uncertainty.py::test_bits_where_the_frame_grid_is_capped.
  pivlfn_uncertainty_accumulate   none: one thread per pixel, a flat grid, the frames a loop of the kernel.
  pivlfn_stereo_2d3c              frame_grid.  STEREO_CASES in test_gpu_stereo.py::test_kernel_matches_restatement_random (its
                                  1024 x 1024 case has 4096 blocks, below the cap of 16384).
  pivlfn_field_absmax             grid min(ceil(HW / 256), 256) per image.  VIZ_ABSMAX_CASES, test_gpu_viz.py::test_field_absmax_where_the_grid_is_capped.
  pivlfn_flow_maxrad              grid min(ceil(ceil(HW / 4) / 256), 256) per image.  VIZ_MAXRAD_CASES,
                                  test_gpu_viz.py::test_flow_maxrad_and_its_picture_where_the_grid_is_capped.
  pivlfn_flow_to_color, pivlfn_scalar_to_color   grid min(ceil(ceil(B HW / 4) / 256), VZ_MAX_BLOCKS) over the batch.  VIZ_COLOR_CASES,
                                  test_gpu_viz.py::test_pictures_and_cell_means_where_the_grid_is_capped.
  pivlfn_flow_decimate            grid min(ceil(cells / 256), VZ_MAX_BLOCKS) over the batch.  VIZ_COLOR_CASES at cell 1, the same test.
  pivlfn_particles_displace       none: one thread per particle, a flat grid.
  pivlfn_particles_render         tiles = B ceil(H / 16) ceil(W / 16); particles_offsets_kernel: a wave prefix (> 64 tiles: a second wave,
                                  > 256: a second workgroup) and one atomic cursor; a tile's list beyond REN_CAP is ordered window by
                                  window.  PARTICLES_CASES, test_gpu_particles.py::test_seedings_of_many_tiles.
  pivlfn_flowmap_advect / _seed / _ftle   none: one thread per particle or node, flat grids
                                  (test_gpu_flowmap.py::test_particle_lists has 257 particles: a second block).
  pivlfn_snapshot_gram            n = 1985 is the first n whose plan walks all slabs in one workgroup:
                                  test_gpu_pod.py::test_gram_of_many_snapshots_adds_its_slabs_itself.
  pivlfn_snapshot_project         none in P (flat); K picks the kernel: K <= 4, <= 16, <= 64.  test_gpu_pod.py::
                                  test_project_equals_the_sequential_loop has K = 1, 3 | 5, 16 | 17, 64 (PROJECT_CASES adds 5 and 16).
  pivlfn_flow_fields              frame_grid.  FIELDS_CASES, test_gpu_postpro.py::test_fields_where_the_frame_grid_is_capped.
  pivlfn_flow_validate            frame_grid, both kernels.  VALIDATE_CASES, test_gpu_validate.py::test_bits_where_the_frame_grid_is_capped.
  pivlfn_frames_preprocess        k = 0: frame_grid over the pixels of a frame, or over groups of four where H*W is a multiple of 4 and
                                  the pointers are aligned.  PREPROC_CASES, test_gpu_preproc.py::test_scale_where_the_frame_grid_is_capped.
                                  Min-max: tiles, a flat grid.
  pivlfn_flow_stats_accumulate(_masked), pivlfn_error_stats_accumulate   frame_grid with frames = 1 (the frames are a loop of the kernel): capped
                                  at 16384 blocks.  ACCUMULATOR_CASES, test_gpu_postpro.py::test_stats_where_the_grid_is_capped,
                                  test_gpu_validate.py::test_masked_stats_where_the_grid_is_capped,
                                  test_gpu_evaluate.py::test_error_stats_where_the_grid_is_capped.
  pivlfn_frames_background_min    frame_grid with frames = 1 over the bytes of a frame (or groups of four); 1024 x 1024 x 3 bytes are
                                  3072 blocks of four-byte groups, below the cap.
  pivlfn_flow_errors, pivlfn_level_errors   tiles, flat grids; the second pass of pivlfn_flow_errors from 32 x 32 tiles:
                                  test_gpu_evaluate.py, the 1024 x 1024 cases.
"""
import os
import re
from collections import namedtuple

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "piv_liteflownet-pytorch_amd", "csrc")

# the constexpr values the formulas below depend on, per source file; tests/test_analysis_plans.py reads them back out of the text
CONSTANTS = {
    "launch_checks.h": {"FRAME_GRID_THREADS": 256, "FRAME_GRID_BLOCKS": 16384, "FRAME_GRID_MIN_BLOCKS": 64},
    "cg_shared.h": {"PR_THREADS": 256, "PR_OWN": 4, "PR_CHUNK": 1024, "PR_MAX_PART": 2048},
    "smooth.hip": {"DC_BLK": 64, "DC_KC": 32},
    "calibrate.hip": {"TP_BLOCK": 256},
    "twopoint.hip": {"TP_WAVES": 4, "TP_CHUNK": 256, "TP_SLOT": 16},
    "viz.hip": {"VZ_THREADS": 256, "VZ_MAX_BLOCKS": 4096},
    "particles.hip": {"REN_TILE": 16, "REN_CAP": 2048},
    "spectrum.hip": {"SP_TC": 128, "SP_KG": 8, "SP_WAVES": 8, "SP_TILE": 64},
}
FRAME_GRID_THREADS, FRAME_GRID_BLOCKS, FRAME_GRID_MIN_BLOCKS = (CONSTANTS["launch_checks.h"][k] for k in
                                                                 ("FRAME_GRID_THREADS", "FRAME_GRID_BLOCKS", "FRAME_GRID_MIN_BLOCKS"))
PR_THREADS, PR_OWN, PR_CHUNK, PR_MAX_PART = (CONSTANTS["cg_shared.h"][k] for k in ("PR_THREADS", "PR_OWN", "PR_CHUNK", "PR_MAX_PART"))
DC_BLK, DC_KC = CONSTANTS["smooth.hip"]["DC_BLK"], CONSTANTS["smooth.hip"]["DC_KC"]
TP_BLOCK = CONSTANTS["calibrate.hip"]["TP_BLOCK"]
TP_WAVES, TP_CHUNK, TP_SLOT = (CONSTANTS["twopoint.hip"][k] for k in ("TP_WAVES", "TP_CHUNK", "TP_SLOT"))
VZ_THREADS, VZ_MAX_BLOCKS = CONSTANTS["viz.hip"]["VZ_THREADS"], CONSTANTS["viz.hip"]["VZ_MAX_BLOCKS"]
REN_TILE, REN_CAP = CONSTANTS["particles.hip"]["REN_TILE"], CONSTANTS["particles.hip"]["REN_CAP"]
SP_TC, SP_KG, SP_WAVES, SP_TILE = (CONSTANTS["spectrum.hip"][k] for k in ("SP_TC", "SP_KG", "SP_WAVES", "SP_TILE"))


def source_constants(name):
    """Every `constexpr int|unsigned NAME = <integer expression of literals and earlier names>` of csrc/<name>, evaluated."""
    text = open(os.path.join(CSRC, name)).read()
    found = {}
    for stmt in re.findall(r"^constexpr\s+(?:int|unsigned)\s+([^;{]+);", text, re.M):
        for part in stmt.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*=\s*([\w\s*+\-/()]+?)\s*", part)
            if not m:
                continue
            try:
                found[m.group(1)] = int(eval(m.group(2).replace("/", "//"), {"__builtins__": {}}, dict(found)))       # noqa: S307
            except (NameError, SyntaxError):
                pass                                       # defined by a macro of the header: not one this module uses
    return found


def cdiv(a, b):
    return -(-a // b)


def pow2_at_least(n):
    p = 1
    while p < n:
        p *= 2
    return p


# ---- the plans ------------------------------------------------------------------------------------------------------------------------
def pressure(h, w):
    """pr_plan of csrc/cg_shared.h, which pr_layout (pressure.hip) and sm_layout (smooth.hip) call: chunks per workgroup and block
    partials per frame, or per system of the smoothing solver."""
    N = h * w
    P2 = pow2_at_least(N)
    chunks = P2 // (PR_CHUNK * PR_MAX_PART) if P2 > PR_CHUNK * PR_MAX_PART else 1
    tile = chunks * PR_CHUNK
    return {"N": N, "chunks": chunks, "NB": cdiv(N, tile)}


def dct(H, W):
    """dct_enqueue and dct_mm_kernel of csrc/smooth.hip: the grid of 64 x 64 blocks of a plane (x, y), whether its edge blocks are ragged,
    and the staged chunks of the inner index of the product along the rows (K = W) and along the columns (K = H)."""
    return {"grid": (cdiv(W, DC_BLK), cdiv(H, DC_BLK)), "blocks": cdiv(W, DC_BLK) * cdiv(H, DC_BLK),
            "ragged": (W % DC_BLK != 0, H % DC_BLK != 0), "chunks": (cdiv(W, DC_KC), cdiv(H, DC_KC))}


def smooth_solve(H, W):
    """A system of the smoothing solver: the partials plan, the nodes of its last tile, and the matrix products of its preconditioner."""
    p = pressure(H, W)
    p["last_tile"] = p["N"] - (p["NB"] - 1) * p["chunks"] * PR_CHUNK
    p["dct"] = dct(H, W)
    return p


def pressure_offset_b(F, h, w):
    """What pivlfn_pressure_workspace_offset(F, h, w, PIVLFN_PRESSURE_WS_B) returns: two 64-byte records and three partials per frame."""
    return 128 * F + 24 * pressure(h, w)["NB"] * F


def tp_scan(H, W):
    """tp_scan_kernel of csrc/calibrate.hip: blocks of the image, blocks per thread, and the threads whose range is short or empty."""
    nblk = cdiv(H * W, TP_BLOCK)
    per = cdiv(nblk, 256)
    ranges = [(min(t * per, nblk), min(min(t * per, nblk) + per, nblk)) for t in range(256)]
    return {"nblk": nblk, "per": per, "short": [t for t, (lo, hi) in enumerate(ranges) if 0 < hi - lo < per],
            "empty": [t for t, (lo, hi) in enumerate(ranges) if hi == lo]}


def twopoint(H, W, R):
    """launch_twopoint_accumulate of csrc/twopoint.hip."""
    levels = 0
    while (1 << levels) < W:
        levels += 1
    chunks = (1 << levels) // TP_CHUNK if (1 << levels) > TP_CHUNK else 1
    z = min(cdiv(4096, H), cdiv(R + 1, TP_WAVES))
    slots = cdiv(R + 1, TP_WAVES * z)
    return {"levels": levels, "chunks": chunks, "z": z, "slots": slots, "lds": TP_WAVES * slots * TP_SLOT * 8}


def capped_frame_grid(items, frames):
    """frame_grid of csrc/launch_checks.h: blocks of 256 items per frame, capped at max(16384 / frames, 64); frames = 1 for a launch that
    is not per frame."""
    g = cdiv(items, FRAME_GRID_THREADS)
    cap = max(FRAME_GRID_BLOCKS // frames, FRAME_GRID_MIN_BLOCKS)
    return {"blocks": g, "cap": cap, "grid": min(g, cap), "visits": cdiv(g, min(g, cap))}


def viz_blocks(items):
    g = cdiv(items, VZ_THREADS)
    return min(g, VZ_MAX_BLOCKS) if g else 1


def viz_absmax(H, W):
    g = cdiv(H * W, VZ_THREADS)
    return {"blocks": g, "grid": min(viz_blocks(H * W), 256), "sweep": min(viz_blocks(H * W), 256) * VZ_THREADS}


def viz_maxrad(H, W):
    groups = cdiv(H * W, 4)
    return {"blocks": cdiv(groups, VZ_THREADS), "grid": min(viz_blocks(groups), 256), "sweep": min(viz_blocks(groups), 256) * VZ_THREADS * 4}


def viz_color(B, H, W):
    """flow_to_color and scalar_to_color (groups of four pixels over the batch) and flow_decimate at cell 1 (one cell a thread)."""
    npix = B * H * W
    groups = cdiv(npix, 4)
    return {"blocks": cdiv(groups, VZ_THREADS), "grid": viz_blocks(groups), "sweep": viz_blocks(groups) * VZ_THREADS * 4,
            "decimate_blocks": cdiv(npix, VZ_THREADS), "decimate_grid": viz_blocks(npix)}


def particles_tiles(B, H, W):
    tiles = B * cdiv(H, REN_TILE) * cdiv(W, REN_TILE)
    return {"tiles": tiles, "waves": cdiv(tiles, 64), "workgroups": cdiv(tiles, 256)}


def spectrum(L, K):
    nfull, nsingle = K // SP_KG, K % SP_KG
    return {"chunks": cdiv(L, SP_TC), "groups": nfull, "singles": nsingle, "rounds": cdiv(nfull, SP_WAVES) if nfull else 1}


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
# shape: what the GPU test is parametrised with; branch: why the case exists; crosses: the plan of `shape` -> whether it is there
Case = namedtuple("Case", "shape branch plan crosses")


def _case(shape, branch, plan, crosses):
    return Case(shape, branch, plan, crosses)


PRESSURE_CASES = [          # (h, w), one frame; three iterations each (the restatement of 2048 x 2049 takes about a second an iteration)
    _case((513, 512), "NB = 257: a partial in the second wave of pr_finish", pressure, lambda p: p["NB"] == 257 and p["chunks"] == 1),
    _case((1024, 1025), "NB = 1025: the second chunk of pr_finish holds one partial", pressure,
          lambda p: p["NB"] == PR_CHUNK + 1 and p["chunks"] == 1),
    _case((2048, 1025), "chunks = 2: PrCounter level 0", pressure, lambda p: p["chunks"] == 2 and p["NB"] == 1025 and p["NB"] <= PR_MAX_PART),
    _case((2048, 2049), "chunks = 4: a carry in PrCounter", pressure, lambda p: p["chunks"] == 4 and p["NB"] == 1025 and p["NB"] <= PR_MAX_PART),
]

SMOOTH_CASES = [            # (H, W), one frame: setup and read-out alone (bb of both systems against the restated tree)
    _case((513, 512), "NB = 257: a partial in the second wave of pr_finish", pressure, lambda p: p["NB"] == 257 and p["chunks"] == 1),
    _case((1024, 1025), "NB = 1025: the second chunk of pr_finish holds one partial", pressure,
          lambda p: p["NB"] == PR_CHUNK + 1 and p["chunks"] == 1),
    _case((2048, 1025), "chunks = 2: PrCounter level 0", pressure, lambda p: p["chunks"] == 2 and p["NB"] == 1025 and p["NB"] <= PR_MAX_PART),
    _case((2048, 2049), "chunks = 4: a carry in PrCounter", pressure, lambda p: p["chunks"] == 4 and p["NB"] == 1025 and p["NB"] <= PR_MAX_PART),
]

SMOOTH_SOLVE_CASES = [      # (H, W, iterations of the trajectory test): the smallest frames whose solve crosses tile seams and matrix blocks
    _case((37, 61, 6), "NB = 3, a ragged last tile, rows that straddle a thread's four nodes, one matrix block", smooth_solve,
          lambda p: p["NB"] == 3 and p["last_tile"] == 209 and 61 % PR_OWN != 0 and p["dct"]["blocks"] == 1 and p["dct"]["chunks"] == (2, 2)),
    _case((70, 131, 6), "NB = 9; 3 x 2 ragged matrix blocks a plane: Gamma and the skip at m0, n0 > 0; 5 and 3 chunks of the inner index",
          smooth_solve, lambda p: p["NB"] == 9 and p["dct"]["grid"] == (3, 2) and p["dct"]["ragged"] == (True, True)
          and p["dct"]["chunks"] == (5, 3)),
    _case((513, 512, 3), "NB = 257: the second wave of pr_finish inside the iteration kernels and cg_alpha", smooth_solve,
          lambda p: p["NB"] == 257 and p["chunks"] == 1 and p["dct"]["grid"] == (8, 9)),
]

TARGET_POINTS_CASES = [     # (H, W)
    _case((257, 256), "per = 2, only thread 128 has a short range", tp_scan,
          lambda p: p["nblk"] == 257 and p["per"] == 2 and p["per"] * 256 > p["nblk"] and p["short"] == [128] and p["empty"][0] == 129),
    _case((349, 513), "per = 3, threads from 234 on are empty", tp_scan,
          lambda p: p["nblk"] == 700 and p["per"] == 3 and p["per"] * 256 > p["nblk"] and p["short"] == [233] and p["empty"][0] == 234),
    _case((1024, 1280), "the workload's size: per = 20", tp_scan, lambda p: p["nblk"] == 5120 and p["per"] == 20 and not p["empty"]),
]

TWOPOINT_CASES = [          # (H, W, R, step), B = 2
    _case((66, 300, 255, 1), "slots = 2", lambda H, W, R, s: twopoint(H, W, R), lambda p: p["slots"] == 2 and p["z"] == 63),
    _case((4096, 5, 255, 1), "z = 1, slots = 64: the largest LDS request", lambda H, W, R, s: twopoint(H, W, R),
          lambda p: p["z"] == 1 and p["slots"] == 64 and p["lds"] == 32768),
    _case((1024, 40, 64, 1), "the workload's z = 4, slots = 5", lambda H, W, R, s: twopoint(H, W, R), lambda p: p["z"] == 4 and p["slots"] == 5),
    _case((5, 520, 8, 1), "4 chunks: counter level 1", lambda H, W, R, s: twopoint(H, W, R), lambda p: p["chunks"] == 4),
    _case((3, 1030, 8, 3), "8 chunks: counter level 2", lambda H, W, R, s: twopoint(H, W, R), lambda p: p["chunks"] == 8),
    _case((2, 16384, 4, 1), "64 chunks: every counter register", lambda H, W, R, s: twopoint(H, W, R), lambda p: p["chunks"] == 64 and p["levels"] == 14),
]

_over_the_cap = lambda p: p["blocks"] > p["cap"] and p["grid"] == p["cap"] and p["visits"] == 2      # noqa: E731
VORTEX_CASES = [            # (B, H, W, radius, spacing)
    _case((260, 130, 128, 2, 1), "65 blocks a frame, capped at 64", lambda B, H, W, r, s: capped_frame_grid(H * W, B),
          lambda p: _over_the_cap(p) and p["cap"] == 64 and p["blocks"] == 65),
    _case((1, 2049, 2048, 1, 1), "16392 blocks, capped at 16384", lambda B, H, W, r, s: capped_frame_grid(H * W, B),
          lambda p: _over_the_cap(p) and p["cap"] == 16384),
]
QUALITY_CASES = [           # (B, H, W, radius)
    _case((260, 130, 128, 1), "65 blocks a frame, capped at 64", lambda B, H, W, r: capped_frame_grid(H * W, B),
          lambda p: _over_the_cap(p) and p["cap"] == 64),
]
STEREO_CASES = [            # (B, h, w)
    _case((260, 130, 128), "65 blocks a pair, capped at 64", lambda B, h, w: capped_frame_grid(h * w, B), lambda p: _over_the_cap(p) and p["cap"] == 64),
    _case((1, 2049, 2048), "16392 blocks, capped at 16384", lambda B, h, w: capped_frame_grid(h * w, B), lambda p: _over_the_cap(p) and p["cap"] == 16384),
]
_frames_of = lambda B, H, W: capped_frame_grid(H * W, B)      # noqa: E731
FIELDS_CASES = [            # (B, H, W); compared with the same frames in calls of FRAMES_PER_UNCAPPED_CALL, which are not capped
    _case((260, 130, 128), "65 blocks a frame, capped at 64", _frames_of, lambda p: _over_the_cap(p) and p["cap"] == 64 and p["blocks"] == 65),
]
VALIDATE_CASES = [          # (B, H, W)
    _case((260, 130, 128), "65 blocks a frame, capped at 64", _frames_of, lambda p: _over_the_cap(p) and p["cap"] == 64 and p["blocks"] == 65),
]
UNCERTAINTY_CASES = [       # (B, H, W, radius, lag)
    _case((260, 130, 128, 1, 1), "65 blocks a frame, capped at 64", lambda B, H, W, r, lag: capped_frame_grid(H * W, B),
          lambda p: _over_the_cap(p) and p["cap"] == 64 and p["blocks"] == 65),
]
PREPROC_CASES = [           # (n, H, W), k = 0
    _case((260, 258, 256), "16512 four-pixel items: 65 blocks a frame, capped at 64", lambda n, H, W: capped_frame_grid(H * W // 4, n),
          lambda p: _over_the_cap(p) and p["cap"] == 64 and p["blocks"] == 65 and 258 * 256 % 4 == 0),
    _case((260, 129, 129), "16641 pixels, odd: the byte path, 66 blocks a frame, capped at 64", lambda n, H, W: capped_frame_grid(H * W, n),
          lambda p: _over_the_cap(p) and p["cap"] == 64 and p["blocks"] == 66 and 129 * 129 % 4 != 0),
]
ACCUMULATOR_CASES = [       # (B, H, W): flow_stats_accumulate, _masked and error_stats_accumulate
    _case((2, 2049, 2048), "16392 blocks, capped at 16384", lambda B, H, W: capped_frame_grid(H * W, 1),
          lambda p: _over_the_cap(p) and p["cap"] == 16384 and p["blocks"] == 16392),
]
FRAMES_PER_UNCAPPED_CALL = 52     # 52 frames are capped at 315 blocks a frame: the five calls a batch of 260 is compared with are not capped

VIZ_ABSMAX_CASES = [        # (B, H, W)
    _case((1, 257, 256), "257 blocks, capped at 256: one block comes round again", lambda B, H, W: viz_absmax(H, W),
          lambda p: p["blocks"] == 257 and p["grid"] == 256),
    _case((2, 1024, 1024), "4096 blocks an image on a grid of 256: sixteen visits", lambda B, H, W: viz_absmax(H, W),
          lambda p: p["blocks"] == 16 * p["grid"] and p["grid"] == 256),
]
VIZ_MAXRAD_CASES = [        # (B, H, W)
    _case((1, 513, 512), "257 blocks of 4-pixel groups, capped at 256", lambda B, H, W: viz_maxrad(H, W),
          lambda p: p["blocks"] == 257 and p["grid"] == 256),
]
VIZ_COLOR_CASES = [         # (B, H, W)
    _case((5, 1024, 1024), "5120 blocks over the batch, capped at VZ_MAX_BLOCKS", viz_color,
          lambda p: p["blocks"] == 5120 and p["grid"] == VZ_MAX_BLOCKS and p["decimate_blocks"] > p["decimate_grid"] == VZ_MAX_BLOCKS),
    _case((1, 2049, 2048), "4098 blocks, two over VZ_MAX_BLOCKS", viz_color,
          lambda p: p["blocks"] == VZ_MAX_BLOCKS + 2 and p["grid"] == VZ_MAX_BLOCKS and p["decimate_grid"] == VZ_MAX_BLOCKS),
]

PARTICLES_CASES = [         # (B, H, W), about 0.05 particles per pixel
    _case((1, 16, 1040), "65 tiles: a second wave of the offsets", particles_tiles, lambda p: p["tiles"] == 65 and p["waves"] == 2 and p["workgroups"] == 1),
    _case((1, 16, 4112), "257 tiles: a second workgroup of the offsets", particles_tiles, lambda p: p["tiles"] == 257 and p["workgroups"] == 2),
    _case((2, 272, 256), "544 tiles over two images: three workgroups", particles_tiles, lambda p: p["tiles"] == 544 and p["workgroups"] == 3),
]

SPECTRUM_CASES = [          # (L, N, K, first, pad)
    _case((1024, 65, 513, 1000, 1), "the corner of the domain: 8 chunks re-staged in each of 8 rounds, one single", lambda L, N, K, f, p: spectrum(L, K),
          lambda p: p == {"chunks": 8, "groups": 64, "singles": 1, "rounds": 8}),
    _case((1000, 64, 501, 0, 0), "a short last chunk, a ragged last round, five singles", lambda L, N, K, f, p: spectrum(L, K),
          lambda p: p["chunks"] == 8 and 1000 % SP_TC and p["groups"] == 62 and p["groups"] % SP_WAVES and p["singles"] == 5 and p["rounds"] == 8),
]

PROJECT_CASES = [(9, 5, 70), (9, 16, 300)]              # (n, K, P): the first and the last K of project_kernel<16>

ALL_CASES = {"pressure": PRESSURE_CASES, "smooth": SMOOTH_CASES, "smooth_solve": SMOOTH_SOLVE_CASES, "target_points": TARGET_POINTS_CASES, "twopoint": TWOPOINT_CASES, "vortex": VORTEX_CASES,
             "quality": QUALITY_CASES, "stereo": STEREO_CASES, "field_absmax": VIZ_ABSMAX_CASES, "flow_maxrad": VIZ_MAXRAD_CASES,
             "viz_color": VIZ_COLOR_CASES, "particles": PARTICLES_CASES, "spectrum": SPECTRUM_CASES, "flow_fields": FIELDS_CASES,
             "flow_validate": VALIDATE_CASES, "flow_uncertainty": UNCERTAINTY_CASES, "frames_preprocess": PREPROC_CASES,
             "accumulators": ACCUMULATOR_CASES}


def shapes(cases):
    return [c.shape for c in cases]
