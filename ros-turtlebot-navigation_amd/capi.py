"""ctypes binding of the C-ABI declared in include/tbnav_*.h (libtbnav_hip.so).

This is plumbing for tests, smoke() and bench.py: it loads the in-tree shared library and exposes
the entry points with typed signatures.  There is NO fallback: if the library is missing or a call
fails, it raises.  Nothing here imports or calls oracle/.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtbnav_hip.so")
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

TBNAV_MPPI_REC = 8

# tbnav_status.h
OK, ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_OUT_OF_WORLD, ERR_ETA_ZERO, ERR_PDF_VARIANCE, \
    ERR_BRESENHAM, ERR_UNSUPPORTED, ERR_POOL_EXHAUSTED = range(10)

# tbnav_mppi.h options
MPPI_OPT_KERNEL, MPPI_OPT_TRIG, MPPI_OPT_NO_LDS_STAGING, MPPI_OPT_KEEP_J, MPPI_OPT_REG_TAIL, MPPI_OPT_BATCH_GRAPH, MPPI_OPT_PREFIX_FORM = 1, 2, 3, 4, 5, 6, 7
MPPI_OPT_DIRECT_EXCHANGE, MPPI_OPT_SAMPLER, MPPI_OPT_FAULT_INJECT, MPPI_OPT_WIDE_COMBINE = 8, 9, 10, 11
MPPI_OPT_NOISE_AHEAD = 12

# tbnav_rbpf.h options
RBPF_OPT_DF_MODE, RBPF_OPT_RAYCAST_ORDERED, RBPF_OPT_RAYCAST_THREADS, RBPF_OPT_COUNT_CELLS, RBPF_OPT_RAYCAST_FORM = 1, 2, 3, 4, 5
RBPF_OPT_RAYCAST_BAND_ROWS = 6
RBPF_OPT_RAYCAST_ADAPT = 9
RBPF_OPT_RAYCAST_CELL16 = 10
RBPF_OPT_NOISE_IN_KERNEL = 11
RBPF_OPT_BATCH_PIPELINE = 7
RBPF_OPT_HOST_THREADS = 8
RBPF_OPT_REF_REACH = 12
RBPF_DF = {"full": 0, "window": 1, "query": 2, "reference": 3}


class TbnavError(RuntimeError):
    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        super().__init__(f"{where}: status {status}" + (f" ({detail})" if detail else ""))


class MppiParams(C.Structure):
    """tbnav_mppi_params (include/tbnav_mppi.h)."""
    _fields_ = [
        ("wheel_radius", C.c_double), ("wheel_base", C.c_double), ("lam", C.c_double),
        ("max_wheel_vel", C.c_double), ("ul_var", C.c_double), ("ur_var", C.c_double),
        ("horizon", C.c_double), ("dt", C.c_double),
        ("Q", C.c_double * 3), ("R", C.c_double * 2), ("P1", C.c_double * 3),
        ("rollouts", C.c_int32), ("device", C.c_int32),
    ]


class MppiCostField(C.Structure):
    """tbnav_mppi_cost_field (include/tbnav_mppi.h, COST FIELD)."""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("xmin", C.c_double), ("ymin", C.c_double), ("resolution", C.c_double),
                ("weight", C.c_double)]


MPPI_FIELD_MAX_SIDE = 4096


class NavParams(C.Structure):
    """tbnav_nav_params (include/tbnav_nav.h, G1)."""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("xmin", C.c_double), ("ymin", C.c_double), ("resolution", C.c_double),
                ("device", C.c_int32), ("reserved", C.c_int32)]


class NavSolveInfo(C.Structure):
    """tbnav_nav_solve_info."""
    _fields_ = [("solved", C.c_int32), ("goal", C.c_int32 * 2), ("rounds", C.c_int32), ("launches", C.c_int32), ("tiles", C.c_int32 * 2),
                ("tile_visits", C.c_int64)]


NAV_MAX_SIDE, NAV_MAX_COST, NAV_UNREACHED = 2048, 64, 0xFFFFFFFF
NAV_MAX_REACH, NAV_BEST_PARTICLE = 32, -1
NAV_MAX_VISIT_RADIUS = 64


class NavFrontierInfo(C.Structure):
    """tbnav_nav_frontier_info (G13)."""
    _fields_ = [("found", C.c_int32), ("min_cells", C.c_int32), ("cells", C.c_int32), ("clusters", C.c_int32), ("seed_clusters", C.c_int32),
                ("seed_cells", C.c_int32), ("rounds", C.c_int32), ("launches", C.c_int32), ("tile_visits", C.c_int64)]


class NavFrontier(C.Structure):
    """tbnav_nav_frontier (G16)."""
    _fields_ = [("root", C.c_int32 * 2), ("size", C.c_int32), ("seeds", C.c_int32), ("box", C.c_int32 * 4), ("sum_ix", C.c_int64),
                ("sum_iy", C.c_int64)]


NAV_MAX_GAIN_RANGE, NAV_MAX_GAIN_WEIGHT = 128, 4096


class NavGainInfo(C.Structure):
    """tbnav_nav_gain_info (G19)."""
    _fields_ = [("computed", C.c_int32), ("range_cells", C.c_int32), ("rays", C.c_int32), ("viewpoints", C.c_int32), ("gain_min", C.c_int32),
                ("gain_max", C.c_int32), ("best", C.c_int32 * 2)]


class NavFrontierGain(C.Structure):
    """tbnav_nav_frontier_gain (G19)."""
    _fields_ = [("root", C.c_int32 * 2), ("gain_max", C.c_int32), ("best", C.c_int32 * 2)]


class RbpfParams(C.Structure):
    """tbnav_rbpf_params (include/tbnav_rbpf.h)."""
    _fields_ = [
        ("num_particles", C.c_int32), ("num_samples_mode", C.c_int32),
        ("srr", C.c_double), ("srt", C.c_double), ("str_", C.c_double), ("stt", C.c_double),
        ("motion_noise", C.c_double * 3), ("sample_range", C.c_double * 3),
        ("scan_likelihood_min", C.c_double), ("scan_likelihood_max", C.c_double),
        ("pose_likelihood_min", C.c_double), ("pose_likelihood_max", C.c_double),
        ("beam_min", C.c_float), ("beam_max", C.c_float), ("beam_delta", C.c_float),
        ("range_min", C.c_float), ("range_max", C.c_float), ("device", C.c_int32),
        ("z_hit", C.c_double), ("z_short", C.c_double), ("z_max", C.c_double), ("z_rand", C.c_double),
        ("sigma_hit", C.c_double),
        ("Trs", C.c_double * 3),
        ("resolution", C.c_double), ("xmin", C.c_double), ("xmax", C.c_double), ("ymin", C.c_double),
        ("ymax", C.c_double),
        ("pose0", C.c_double * 3),
    ]


class RbpfStats(C.Structure):
    """tbnav_rbpf_stats."""
    _fields_ = [("sum_w", C.c_double), ("sq_sum", C.c_double), ("neff", C.c_int32), ("resampled", C.c_int32),
                ("status", C.c_int32), ("n_valid_beams", C.c_int32)]


class IcpParams(C.Structure):
    """tbnav_icp_params (include/tbnav_icp.h)."""
    _fields_ = [
        ("beam_min", C.c_float), ("beam_max", C.c_float), ("beam_delta", C.c_float),
        ("range_min", C.c_float), ("range_max", C.c_float), ("max_iter", C.c_int32),
        ("Trs", C.c_double * 3), ("max_corr_dist", C.c_double), ("transform_eps", C.c_double),
        ("fitness_eps", C.c_double), ("device", C.c_int32), ("reserved", C.c_int32),
    ]


class IcpInfo(C.Structure):
    """tbnav_icp_info."""
    _fields_ = [("iterations", C.c_int32), ("correspondences", C.c_int32), ("mse", C.c_double), ("criterion", C.c_int32),
                ("reserved", C.c_int32)]


# tbnav_icp_criterion
ICP_NOT_RUN, ICP_ITERATIONS, ICP_TRANSFORM, ICP_ABS_MSE, ICP_REL_MSE, ICP_NO_CORRESPONDENCES, ICP_DEGENERATE = range(7)
# tbnav_icp_set_metric
ICP_METRIC_POINT, ICP_METRIC_LINE = 0, 1
ICP_LINE_MAX_BEAMS, ICP_LINE_MAX_WINDOW = 2048, 16


class IcpSearchParams(C.Structure):
    """tbnav_icp_search_params (include/tbnav_icp.h, CORRELATIVE SEARCH)."""
    _fields_ = [("resolution", C.c_double), ("half_extent", C.c_double), ("sigma", C.c_double), ("ang_step", C.c_double),
                ("min_quality", C.c_double), ("stamp_cells", C.c_int32), ("lin_cells", C.c_int32), ("ang_steps", C.c_int32),
                ("slack_q10", C.c_int32)]


class IcpSearchInfo(C.Structure):
    """tbnav_icp_search_info."""
    _fields_ = [("T", C.c_double * 3), ("quality", C.c_double), ("score", C.c_uint32), ("points", C.c_int32),
                ("candidates", C.c_int32), ("ia", C.c_int32), ("iy", C.c_int32), ("ix", C.c_int32), ("at_edge", C.c_int32),
                ("accepted", C.c_int32), ("searched", C.c_int32), ("reserved", C.c_int32)]


class IcpSearchShapeParams(C.Structure):
    """tbnav_icp_search_shape_params (include/tbnav_icp.h, F1)."""
    _fields_ = [("drop_q10", C.c_int32), ("reserved", C.c_int32), ("flat_cells2", C.c_double)]


class IcpSearchShape(C.Structure):
    """tbnav_icp_search_shape (F6)."""
    _fields_ = [("S0", C.c_int64), ("Sx", C.c_int64), ("Sy", C.c_int64), ("Sxx", C.c_int64), ("Sxy", C.c_int64), ("Syy", C.c_int64),
                ("l1", C.c_double), ("l2", C.c_double), ("ex", C.c_double), ("ey", C.c_double), ("T_raw", C.c_double * 3),
                ("cells", C.c_int32), ("kind", C.c_int32), ("computed", C.c_int32), ("reserved", C.c_int32)]


ICP_SEARCH_MAX_SIDE, ICP_SEARCH_MAX_STAMP, ICP_SEARCH_MAX_LIN, ICP_SEARCH_MAX_ANG = 208, 8, 16, 90


class IcpSearchWideParams(C.Structure):
    """tbnav_icp_search_wide_params (include/tbnav_icp.h, W1)."""
    _fields_ = [("lin_cells", C.c_int32), ("ang_steps", C.c_int32), ("when", C.c_int32), ("reserved", C.c_int32)]


class IcpSearchWideInfo(C.Structure):
    """tbnav_icp_search_wide_info (W5)."""
    _fields_ = [("first", IcpSearchInfo), ("ran", C.c_int32), ("reserved", C.c_int32)]


ICP_SEARCH_WIDE_MAX_LIN, ICP_SEARCH_WIDE_MAX_ANG, ICP_SEARCH_WIDE_MAX_TABLE = 64, 180, 176
ICP_WIDE_ON_REJECT, ICP_WIDE_ON_REJECT_OR_EDGE, ICP_WIDE_ALWAYS = 0, 1, 2
ICP_MAP_BEST_PARTICLE = -1


class IcpGlobalParams(C.Structure):
    """tbnav_icp_global_params (include/tbnav_icp.h, GLOBAL SEARCH, L1)."""
    _fields_ = [("ang_step", C.c_double), ("min_quality", C.c_double), ("ang_count", C.c_int32), ("pool_log2", C.c_int32),
                ("region", C.c_int32 * 4), ("reserved", C.c_int32)]


class IcpGlobalInfo(C.Structure):
    """tbnav_icp_global_info (L7)."""
    _fields_ = [("T", C.c_double * 3), ("quality", C.c_double), ("blocks", C.c_int64), ("refined_blocks", C.c_int64),
                ("score", C.c_uint32), ("points", C.c_int32), ("occupied", C.c_int32), ("ia", C.c_int32), ("tx", C.c_int32),
                ("ty", C.c_int32), ("rounds", C.c_int32), ("accepted", C.c_int32), ("searched", C.c_int32), ("reserved", C.c_int32)]


class IcpHypParams(C.Structure):
    """tbnav_icp_hyp_params (include/tbnav_icp.h, HYPOTHESES, H1)."""
    _fields_ = [("max_hyp", C.c_int32), ("floor_q10", C.c_int32), ("sep_cells", C.c_int32), ("sep_steps", C.c_int32), ("wrap", C.c_int32),
                ("reserved", C.c_int32)]


class IcpHypothesis(C.Structure):
    """tbnav_icp_hypothesis (H5)."""
    _fields_ = [("T", C.c_double * 3), ("quality", C.c_double), ("score", C.c_uint32), ("ia", C.c_int32), ("tx", C.c_int32), ("ty", C.c_int32),
                ("accepted", C.c_int32), ("reserved", C.c_int32)]


class IcpHypInfo(C.Structure):
    """tbnav_icp_hyp_info (H7)."""
    _fields_ = [("blocks", C.c_int64), ("floor_blocks", C.c_int64), ("refined_blocks", C.c_int64), ("candidates", C.c_int64),
                ("best_score", C.c_uint32), ("floor_score", C.c_uint32), ("points", C.c_int32), ("occupied", C.c_int32), ("n", C.c_int32),
                ("n_peaks", C.c_int32), ("rounds", C.c_int32), ("searched", C.c_int32)]


ICP_HYP_MAX, ICP_HYP_MAX_BINS, ICP_HYP_MAX_REFINE, ICP_HYP_MAX_CANDIDATES = 64, 1 << 22, 1 << 18, 1 << 20


class IcpAlignMapParams(C.Structure):
    """tbnav_icp_align_map_params (include/tbnav_icp.h, MAP ALIGNMENT, A1a)."""
    _fields_ = [("max_flatness", C.c_double), ("half_cells", C.c_int32), ("gate_cells", C.c_int32), ("feature_cells", C.c_int32),
                ("reserved", C.c_int32)]


class IcpAlignMapPair(C.Structure):
    """tbnav_icp_align_map_pair (A10): the test hook's record of one beam."""
    _fields_ = [("bx", C.c_double), ("by", C.c_double), ("nx", C.c_float), ("ny", C.c_float), ("hi", C.c_int32), ("hj", C.c_int32),
                ("mi", C.c_int32), ("mj", C.c_int32), ("D", C.c_int32), ("has_home", C.c_int32), ("has_normal", C.c_int32),
                ("kept", C.c_int32)]


class IcpVerifyMapParams(C.Structure):
    """tbnav_icp_verify_map_params (include/tbnav_icp.h, MAP CHECK, V1a)."""
    _fields_ = [("half_cells", C.c_int32), ("slack_cells", C.c_int32), ("max_through_q10", C.c_int32), ("max_missing_q10", C.c_int32),
                ("min_hit_q10", C.c_int32), ("reserved", C.c_int32)]


class IcpVerifyMapInfo(C.Structure):
    """tbnav_icp_verify_map_info (V7)."""
    _fields_ = [("free_cells", C.c_int64), ("unknown_cells", C.c_int64), ("points", C.c_int32), ("outside", C.c_int32), ("walked", C.c_int32),
                ("hit", C.c_int32), ("through", C.c_int32), ("missing", C.c_int32), ("unseen", C.c_int32), ("undecided", C.c_int32),
                ("sensor_cell", C.c_int32 * 2), ("sensor_class", C.c_int32), ("accepted", C.c_int32)]


class IcpVerifyMapBeam(C.Structure):
    """tbnav_icp_verify_map_beam (V9): the test hook's record of one beam."""
    _fields_ = [("cls", C.c_int32), ("e", C.c_int32 * 2), ("n", C.c_int32), ("b", C.c_int32), ("D", C.c_int32), ("free_cells", C.c_int32),
                ("unknown_cells", C.c_int32)]


ICP_VERIFY_NONE, ICP_VERIFY_OUTSIDE, ICP_VERIFY_HIT, ICP_VERIFY_THROUGH, ICP_VERIFY_MISSING, ICP_VERIFY_UNSEEN, ICP_VERIFY_UNDECIDED = range(7)
ICP_VERIFY_MAP_MAX_HALF, ICP_VERIFY_MAP_MAX_SLACK = 128, 8
ICP_ALIGN_MAP_MAX_HALF = 256
ICP_GLOBAL_STAGES = 9
ICP_GLOBAL_MAX_SIDE, ICP_GLOBAL_MAX_ANG, ICP_GLOBAL_MAX_BLOCKS, ICP_GLOBAL_MAX_HOOK_SCORES = 2048, 720, 1 << 26, 1 << 24


_lib = None


def declared_symbols() -> list[str]:
    """Every function name declared in include/tbnav_*.h (used by the symbol-export test)."""
    names: list[str] = []
    for fn in sorted(os.listdir(INCLUDE_DIR)):
        if not (fn.startswith("tbnav_") and fn.endswith(".h")):
            continue
        text = open(os.path.join(INCLUDE_DIR, fn)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        names += re.findall(r"\b(tbnav_[a-z0-9_]+)\s*\(", text)
    return sorted(set(names))


def lib() -> C.CDLL:
    """Load libtbnav_hip.so (once).  Raises if it has not been built — never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch bundles its own HIP runtime (torch/lib/libamdhip64.so) and must be the first to load
    # one: if /opt/rocm's copy (our DT_NEEDED) is mapped first, torch later maps a second runtime
    # and sees "No HIP GPUs".  With torch first, our NEEDED resolves to the already-loaded SONAME
    # and the process has ONE runtime, so torch streams/pointers are valid in our kernels.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the HIP path has no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    dp, vp, i32, u64, dbl = C.POINTER(C.c_double), C.c_void_p, C.c_int32, C.c_uint64, C.c_double
    sig = {
        "tbnav_status_string": (C.c_char_p, [C.c_int]),
        "tbnav_last_hip_error": (C.c_char_p, []),
        "tbnav_device_count": (C.c_int, []),
        # MPPI
        "tbnav_mppi_create": (C.c_int, [C.POINTER(MppiParams), C.POINTER(vp)]),
        "tbnav_mppi_destroy": (None, [vp]),
        "tbnav_mppi_steps": (C.c_int, [vp]),
        "tbnav_mppi_rollouts": (C.c_int, [vp]),
        "tbnav_mppi_rollout_variant": (C.c_int, [vp]),
        "tbnav_mppi_streaming_form": (C.c_int, [vp]),
        "tbnav_mppi_graph_replayed_ticks": (C.c_int64, [vp]),
        "tbnav_mppi_set_dynamics": (C.c_int, [vp, i32]),
        "tbnav_mppi_set_option": (C.c_int, [vp, i32, i32]),
        "tbnav_mppi_set_rng_shard": (C.c_int, [vp, u64, u64]),
        "tbnav_mppi_records_per_step": (C.c_int, [vp]),
        "tbnav_mppi_set_initial_controls": (C.c_int, [vp, dbl, dbl]),
        "tbnav_mppi_set_waypoint": (C.c_int, [vp, dbl, dbl, dbl]),
        "tbnav_mppi_get_controls": (C.c_int, [vp, vp]),
        "tbnav_mppi_set_controls": (C.c_int, [vp, vp]),
        "tbnav_mppi_new_controls": (C.c_int, [vp, dp, vp, dp]),
        "tbnav_mppi_new_controls_dev": (C.c_int, [vp, dp, vp, vp, vp, dp]),
        "tbnav_mppi_enqueue_dev": (C.c_int, [vp, dp, vp, vp, vp]),
        "tbnav_mppi_last_controls": (C.c_int, [vp, vp, dp]),
        "tbnav_mppi_sample_noise": (C.c_int, [vp, u64, u64, vp]),
        "tbnav_mppi_enqueue_rng": (C.c_int, [vp, dp, u64, u64, vp]),
        "tbnav_mppi_enqueue_rng_batch": (C.c_int, [vp, dp, i32, u64, u64, i32, vp]),
        "tbnav_mppi_new_controls_rng": (C.c_int, [vp, dp, u64, u64, vp, dp]),
        "tbnav_mppi_get_noise": (C.c_int, [vp, vp, vp]),
        "tbnav_mppi_shard_partials": (C.c_int, [vp, dp, vp, vp, vp, vp]),
        "tbnav_mppi_shard_combine": (C.c_int, [vp, vp, i32, vp]),
        "tbnav_mppi_shard_partials_rng": (C.c_int, [vp, dp, u64, u64, vp, vp]),
        "tbnav_mppi_get_cost_to_go": (C.c_int, [vp, vp]),
        "tbnav_mppi_debug_sincos": (C.c_int, [vp, i32, vp, vp]),
        "tbnav_mppi_debug_div_lambda": (C.c_int, [vp, i32, dbl, vp, C.POINTER(C.c_int32)]),
        "tbnav_mppi_debug_combine_general": (C.c_int, [vp, vp]),
        "tbnav_mppi_profile_tick": (C.c_int, [vp, dp, vp, vp, vp, C.POINTER(C.c_float)]),
        "tbnav_mppi_profile_kernels": (C.c_int, [vp, dp, vp, vp, vp, i32, C.POINTER(C.c_float)]),
        "tbnav_mppi_profile_kernels_rng": (C.c_int, [vp, dp, C.c_uint64, C.c_uint64, vp, i32, C.POINTER(C.c_float)]),
        "tbnav_mppi_last_kernel_names": (C.c_int, [vp, C.c_char_p, i32, C.c_char_p, i32]),
        "tbnav_mppi_set_cost_field": (C.c_int, [vp, C.POINTER(MppiCostField), vp]),
        "tbnav_mppi_get_cost_field": (C.c_int, [vp, C.POINTER(i32), C.POINTER(MppiCostField)]),
        "tbnav_mppi_cost_field_lookup": (C.c_int, [vp, vp, i32, vp]),
        "tbnav_mppi_group_set_cost_field": (C.c_int, [vp, C.POINTER(MppiCostField), vp]),
        # goal field (include/tbnav_nav.h)
        "tbnav_nav_create": (C.c_int, [C.POINTER(NavParams), C.POINTER(vp)]),
        "tbnav_nav_destroy": (None, [vp]),
        "tbnav_nav_set_cost": (C.c_int, [vp, vp]),
        "tbnav_nav_solve": (C.c_int, [vp, i32, i32]),
        "tbnav_nav_cell_of": (C.c_int, [vp, dbl, dbl, C.POINTER(i32), C.POINTER(i32)]),
        "tbnav_nav_get_cost_to_go": (C.c_int, [vp, vp]),
        "tbnav_nav_get_field": (C.c_int, [vp, dbl, vp]),
        "tbnav_nav_path": (C.c_int, [vp, i32, i32, vp, i32, C.POINTER(i32)]),
        "tbnav_nav_last_solve": (C.c_int, [vp, C.POINTER(NavSolveInfo), C.c_char_p, i32]),
        "tbnav_nav_apply_to_mppi": (C.c_int, [vp, vp, dbl, dbl]),
        "tbnav_nav_apply_to_mppi_group": (C.c_int, [vp, vp, dbl, dbl]),
        "tbnav_nav_get_cost": (C.c_int, [vp, vp]),
        "tbnav_nav_inflation_tables": (C.c_int, [dbl, dbl, dbl, dbl, vp, vp, i32, C.POINTER(i32), C.POINTER(i32)]),
        "tbnav_nav_set_cost_from_rbpf": (C.c_int, [vp, vp, i32, dbl, dbl, dbl]),
        "tbnav_nav_profile_cost_from_rbpf": (C.c_int, [vp, vp, i32, dbl, dbl, dbl, i32, C.POINTER(C.c_float)]),
        "tbnav_mppi_set_cost_field_from_rbpf": (C.c_int, [vp, vp, i32, dbl, dbl, dbl]),
        "tbnav_nav_last_cost_kernel": (C.c_int, [vp, C.c_char_p, i32]),
        "tbnav_nav_find_frontiers": (C.c_int, [vp, vp, i32, i32, C.POINTER(NavFrontierInfo)]),
        "tbnav_nav_profile_find_frontiers": (C.c_int, [vp, vp, i32, i32, C.POINTER(NavFrontierInfo), C.POINTER(C.c_float)]),
        "tbnav_nav_last_frontiers": (C.c_int, [vp, C.POINTER(NavFrontierInfo)]),
        "tbnav_nav_last_frontier_kernels": (C.c_int, [vp, C.c_char_p, i32]),
        "tbnav_nav_mark_visited": (C.c_int, [vp, i32, i32, i32]),
        "tbnav_nav_clear_visited": (C.c_int, [vp]),
        "tbnav_nav_get_visited": (C.c_int, [vp, vp]),
        "tbnav_nav_solve_goals": (C.c_int, [vp, vp, i32]),
        "tbnav_nav_solve_frontiers": (C.c_int, [vp]),
        "tbnav_nav_get_frontier_labels": (C.c_int, [vp, vp]),
        "tbnav_nav_frontier_list": (C.c_int, [vp, vp, i32, C.POINTER(i32)]),
        "tbnav_nav_gain_rays": (C.c_int, [i32, vp, i32, C.POINTER(i32)]),
        "tbnav_nav_find_frontiers_gain": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(NavFrontierInfo), C.POINTER(NavGainInfo)]),
        "tbnav_nav_profile_find_frontiers_gain": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(NavFrontierInfo), C.POINTER(NavGainInfo),
                                                            C.POINTER(C.c_float)]),
        "tbnav_nav_last_gain": (C.c_int, [vp, C.POINTER(NavGainInfo)]),
        "tbnav_nav_last_gain_kernels": (C.c_int, [vp, C.c_char_p, i32]),
        "tbnav_nav_get_frontier_gain": (C.c_int, [vp, vp]),
        "tbnav_nav_frontier_gain_list": (C.c_int, [vp, vp, i32, C.POINTER(i32)]),
        "tbnav_nav_solve_frontiers_ranked": (C.c_int, [vp, i32]),
        # communicators (include/tbnav_comm.h) and the sharded MPPI tick
        "tbnav_comm_unique_id": (C.c_int, [vp]),
        "tbnav_comm_unique_id_ipc": (C.c_int, [vp]),
        "tbnav_comm_create": (C.c_int, [vp, i32, i32, i32, C.POINTER(vp)]),
        "tbnav_comm_create_local": (C.c_int, [i32, vp, vp]),
        "tbnav_comm_destroy": (None, [vp]),
        "tbnav_comm_selftest": (C.c_int, [vp, u64]),
        "tbnav_comm_rank": (C.c_int, [vp]),
        "tbnav_comm_size": (C.c_int, [vp]),
        "tbnav_comm_device": (C.c_int, [vp]),
        "tbnav_comm_uses_rccl": (C.c_int, [vp]),
        "tbnav_mppi_attach_comm": (C.c_int, [vp, vp]),
        "tbnav_mppi_exchange_kind": (C.c_int, [vp]),
        "tbnav_mppi_exchange_probe": (C.c_int, [vp, i32, vp, C.POINTER(C.c_double)]),
        "tbnav_mppi_group_create": (C.c_int, [C.POINTER(MppiParams), i32, vp, C.POINTER(vp)]),
        "tbnav_mppi_group_destroy": (None, [vp]),
        "tbnav_mppi_group_size": (C.c_int, [vp]),
        "tbnav_mppi_group_member": (C.c_int, [vp, i32, C.POINTER(vp)]),
        "tbnav_mppi_group_set_waypoint": (C.c_int, [vp, dbl, dbl, dbl]),
        "tbnav_mppi_group_set_initial_controls": (C.c_int, [vp, dbl, dbl]),
        "tbnav_mppi_group_set_controls": (C.c_int, [vp, vp]),
        "tbnav_mppi_group_get_controls": (C.c_int, [vp, vp]),
        "tbnav_mppi_group_set_dynamics": (C.c_int, [vp, i32]),
        "tbnav_mppi_group_set_option": (C.c_int, [vp, i32, i32]),
        "tbnav_mppi_group_new_controls": (C.c_int, [vp, dp, vp, dp]),
        "tbnav_mppi_group_new_controls_rng": (C.c_int, [vp, dp, u64, u64, dp]),
        "tbnav_mppi_group_enqueue_rng": (C.c_int, [vp, dp, u64, u64]),
        "tbnav_mppi_group_enqueue_rng_batch": (C.c_int, [vp, vp, i32, u64, u64, i32]),
        "tbnav_mppi_group_last_controls": (C.c_int, [vp, dp]),
        "tbnav_mppi_group_synchronize": (C.c_int, [vp]),
        # RBPF
        "tbnav_rbpf_attach_comm": (C.c_int, [vp, vp]),
        "tbnav_rbpf_group_create": (C.c_int, [C.POINTER(RbpfParams), i32, vp, u64, C.POINTER(vp)]),
        "tbnav_rbpf_group_destroy": (None, [vp]),
        "tbnav_rbpf_group_size": (C.c_int, [vp]),
        "tbnav_rbpf_group_member": (C.c_int, [vp, i32, C.POINTER(vp)]),
        "tbnav_rbpf_group_set_seed": (C.c_int, [vp, u64]),
        "tbnav_rbpf_group_set_option": (C.c_int, [vp, i32, i32]),
        "tbnav_rbpf_group_num_normals": (C.c_int64, [vp, i32]),
        "tbnav_rbpf_group_slam": (C.c_int, [vp, vp, i32, dp, dp, dp, i32, dp, vp, C.POINTER(RbpfStats)]),
        "tbnav_rbpf_group_best_state": (C.c_int, [vp, dp, C.POINTER(i32)]),
        "tbnav_rbpf_group_best_map": (C.c_int, [vp, vp]),
        "tbnav_rbpf_create": (C.c_int, [C.POINTER(RbpfParams), C.POINTER(vp)]),
        "tbnav_rbpf_create_pool": (C.c_int, [C.POINTER(RbpfParams), u64, C.POINTER(vp)]),
        "tbnav_rbpf_pool_stats": (C.c_int, [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
        "tbnav_rbpf_set_option": (C.c_int, [vp, i32, i32]),
        "tbnav_rbpf_integrate_scan": (C.c_int, [vp, i32, vp, i32, dp]),
        "tbnav_rbpf_integrate_scan_many": (C.c_int, [vp, i32, i32, vp, i32, vp]),
        "tbnav_rbpf_likelihood": (C.c_int, [vp, i32, vp, i32, dp, dp]),
        "tbnav_rbpf_particle_map": (C.c_int, [vp, i32, vp]),
        "tbnav_rbpf_scan_counts": (C.c_int, [vp, C.POINTER(u64), C.POINTER(u64), i32]),
        "tbnav_rbpf_reference_field_counts": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_int64)]),
        "tbnav_rbpf_reference_field_stats": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "tbnav_rbpf_destroy": (None, [vp]),
        "tbnav_rbpf_grid_size": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32)]),
        "tbnav_rbpf_num_normals": (C.c_int64, [vp, i32]),
        "tbnav_rbpf_set_seed": (C.c_int, [vp, u64]),
        "tbnav_rbpf_set_rng_shard": (C.c_int, [vp, u64, u64]),
        "tbnav_rbpf_get_normals": (C.c_int, [vp, vp, C.c_int64]),
        "tbnav_rbpf_slam": (C.c_int, [vp, vp, i32, dp, dp, dp, i32, dp, vp, C.POINTER(RbpfStats)]),
        "tbnav_rbpf_slam_local": (C.c_int, [vp, vp, i32, dp, dp, dp, i32, dp, vp, C.POINTER(RbpfStats)]),
        "tbnav_rbpf_slam_batch": (C.c_int, [vp, vp, i32, i32, vp, vp, vp, vp, vp]),
        "tbnav_rbpf_resample_global": (C.c_int, [vp, C.c_int64, dbl, vp, vp, C.POINTER(RbpfStats)]),
        "tbnav_rbpf_add_repeated": (C.c_int, [vp, vp, vp, vp, C.c_int64]),
        "tbnav_rbpf_pool_selftest": (C.c_int, [C.c_uint32, i32, i32, i32, i32, vp, vp, vp]),
        "tbnav_rbpf_gather_local": (C.c_int, [vp, vp]),
        "tbnav_rbpf_copy_weights_dev": (C.c_int, [vp, vp]),
        "tbnav_rbpf_resample_global_dev": (C.c_int, [vp, vp, C.c_int64, C.c_int64, dbl, vp, C.POINTER(RbpfStats)]),
        "tbnav_rbpf_set_weights_from_global_dev": (C.c_int, [vp, vp]),
        "tbnav_rbpf_export_size": (C.c_int, [vp, i32, C.POINTER(u64)]),
        "tbnav_rbpf_export_particle_dev": (C.c_int, [vp, i32, vp, u64, C.POINTER(u64)]),
        "tbnav_rbpf_import_particle_dev": (C.c_int, [vp, i32, vp, u64]),
        "tbnav_rbpf_export_batch_sizes": (C.c_int, [vp, i32, vp, vp]),
        "tbnav_rbpf_export_batch_dev": (C.c_int, [vp, i32, vp, vp, u64, vp]),
        "tbnav_rbpf_import_batch_dev": (C.c_int, [vp, i32, vp, vp, u64, vp]),
        "tbnav_rbpf_copy_particle": (C.c_int, [vp, i32, vp, i32]),
        "tbnav_rbpf_best_state": (C.c_int, [vp, dp, C.POINTER(i32)]),
        "tbnav_rbpf_best_map": (C.c_int, [vp, vp]),
        "tbnav_rbpf_get_particles": (C.c_int, [vp, vp, vp, vp]),
        "tbnav_rbpf_set_particles": (C.c_int, [vp, vp, vp, vp]),
        "tbnav_rbpf_get_log_odds": (C.c_int, [vp, i32, vp]),
        "tbnav_rbpf_set_log_odds": (C.c_int, [vp, i32, vp]),
        "tbnav_rbpf_get_occ_dist": (C.c_int, [vp, i32, vp]),
        "tbnav_rbpf_set_occ_dist": (C.c_int, [vp, i32, vp]),
        "tbnav_rbpf_get_dist_code": (C.c_int, [vp, i32, vp]),
        "tbnav_rbpf_get_occupied_count": (C.c_int, [vp, vp]),
        "tbnav_rbpf_get_trace": (C.c_int, [vp] + [vp] * 9),
        "tbnav_rbpf_get_children": (C.c_int, [vp, vp]),
        "tbnav_rbpf_last_kernel_ms": (C.c_int, [vp, C.POINTER(C.c_float)]),
        "tbnav_rbpf_raycast_box_cells": (C.c_int, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "tbnav_rbpf_last_kernel_names": (C.c_int, [vp, C.c_char_p, i32, C.c_char_p, i32, C.POINTER(C.c_int32)]),
        "tbnav_rbpf_last_field_kernels": (C.c_int, [vp, vp, C.POINTER(C.c_int32)]),
        "tbnav_rbpf_set_timing": (C.c_int, [vp, i32]),
        "tbnav_rbpf_set_scan_matching": (C.c_int, [vp, i32, C.c_double, C.c_double, i32]),
        "tbnav_rbpf_get_scan_match": (C.c_int, [vp, vp, vp]),
        # ICP (include/tbnav_icp.h)
        "tbnav_icp_default_params": (None, [C.POINTER(IcpParams)]),
        "tbnav_icp_create": (C.c_int, [C.POINTER(IcpParams), C.POINTER(vp)]),
        "tbnav_icp_destroy": (None, [vp]),
        "tbnav_icp_reset": (C.c_int, [vp]),
        "tbnav_icp_match": (C.c_int, [vp, vp, vp, i32, dp, dp, C.POINTER(IcpInfo)]),
        "tbnav_icp_step": (C.c_int, [vp, vp, i32, dp, dp, C.POINTER(i32), C.POINTER(IcpInfo)]),
        "tbnav_icp_step_batch": (C.c_int, [vp, vp, i32, i32, vp, vp, vp, vp]),
        "tbnav_icp_cloud": (C.c_int, [vp, vp, i32, vp, C.POINTER(i32)]),
        "tbnav_icp_last_batch_launches": (C.c_int, [vp]),
        "tbnav_icp_set_metric": (C.c_int, [vp, i32, i32, C.c_double]),
        "tbnav_icp_get_metric": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_double)]),
        "tbnav_icp_normals": (C.c_int, [vp, vp, i32, vp, vp]),
        "tbnav_icp_default_search_params": (None, [C.POINTER(IcpSearchParams)]),
        "tbnav_icp_set_search": (C.c_int, [vp, C.POINTER(IcpSearchParams)]),
        "tbnav_icp_get_search": (C.c_int, [vp, C.POINTER(i32), C.POINTER(IcpSearchParams)]),
        "tbnav_icp_last_search": (C.c_int, [vp, C.POINTER(IcpSearchInfo)]),
        "tbnav_icp_search": (C.c_int, [vp, vp, vp, i32, dp, dp, C.POINTER(IcpSearchInfo)]),
        "tbnav_icp_search_scores": (C.c_int, [vp, vp, vp, i32, dp, dp, C.POINTER(IcpSearchInfo), vp]),
        "tbnav_icp_search_table": (C.c_int, [vp, vp, i32, vp]),
        "tbnav_icp_default_search_shape_params": (None, [C.POINTER(IcpSearchShapeParams)]),
        "tbnav_icp_set_search_shape": (C.c_int, [vp, C.POINTER(IcpSearchShapeParams)]),
        "tbnav_icp_get_search_shape": (C.c_int, [vp, C.POINTER(i32), C.POINTER(IcpSearchShapeParams)]),
        "tbnav_icp_last_search_shape": (C.c_int, [vp, C.POINTER(IcpSearchShape)]),
        "tbnav_icp_search_with_shape": (C.c_int, [vp, vp, vp, i32, dp, dp, C.POINTER(IcpSearchInfo), C.POINTER(IcpSearchShape)]),
        "tbnav_icp_default_search_wide_params": (None, [C.POINTER(IcpSearchWideParams)]),
        "tbnav_icp_set_search_wide": (C.c_int, [vp, C.POINTER(IcpSearchWideParams)]),
        "tbnav_icp_get_search_wide": (C.c_int, [vp, C.POINTER(i32), C.POINTER(IcpSearchWideParams)]),
        "tbnav_icp_last_search_wide": (C.c_int, [vp, C.POINTER(IcpSearchWideInfo)]),
        "tbnav_icp_search_wide_scores": (C.c_int, [vp, vp, vp, i32, dp, dp, C.POINTER(IcpSearchInfo), vp]),
        "tbnav_icp_search_map": (C.c_int, [vp, vp, i32, vp, i32, dp, C.POINTER(IcpSearchInfo)]),
        "tbnav_icp_search_map_batch": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, vp]),
        "tbnav_icp_search_map_table": (C.c_int, [vp, vp, i32, dp, vp, C.POINTER(C.c_uint32)]),
        "tbnav_icp_search_map_scores": (C.c_int, [vp, vp, i32, vp, i32, dp, C.POINTER(IcpSearchInfo), vp]),
        "tbnav_icp_search_map_wide_scores": (C.c_int, [vp, vp, i32, vp, i32, dp, C.POINTER(IcpSearchInfo), vp]),
        "tbnav_icp_last_map_kernel": (C.c_int, [vp, C.c_char_p, i32]),
        "tbnav_icp_default_global_params": (None, [C.POINTER(IcpGlobalParams)]),
        "tbnav_icp_localize_map": (C.c_int, [vp, vp, i32, vp, i32, C.POINTER(IcpGlobalParams), C.POINTER(IcpGlobalInfo)]),
        "tbnav_icp_localize_map_timed": (C.c_int, [vp, vp, i32, vp, i32, C.POINTER(IcpGlobalParams), C.POINTER(IcpGlobalInfo), vp]),
        "tbnav_icp_last_global": (C.c_int, [vp, C.POINTER(IcpGlobalInfo)]),
        "tbnav_icp_last_global_kernels": (C.c_int, [vp, C.c_char_p, i32]),
        "tbnav_icp_localize_map_field": (C.c_int, [vp, vp, i32, C.POINTER(IcpGlobalParams), vp, vp, C.POINTER(i32)]),
        "tbnav_icp_localize_map_bounds": (C.c_int, [vp, vp, i32, vp, i32, C.POINTER(IcpGlobalParams), vp]),
        "tbnav_icp_localize_map_scores": (C.c_int, [vp, vp, i32, vp, i32, C.POINTER(IcpGlobalParams), vp]),
        "tbnav_icp_default_hyp_params": (None, [C.POINTER(IcpHypParams)]),
        "tbnav_icp_localize_map_hyp": (C.c_int, [vp, vp, i32, vp, i32, C.POINTER(IcpGlobalParams), C.POINTER(IcpHypParams), vp, i32,
                                                 C.POINTER(IcpHypInfo)]),
        "tbnav_icp_last_hyp": (C.c_int, [vp, C.POINTER(IcpHypInfo)]),
        "tbnav_icp_last_hyp_kernels": (C.c_int, [vp, C.c_char_p, i32]),
        "tbnav_icp_localize_map_hyp_candidates": (C.c_int, [vp, vp, i32, vp, i32, C.POINTER(IcpGlobalParams), C.POINTER(IcpHypParams), vp, vp, vp,
                                                            C.c_int64, C.POINTER(C.c_int64)]),
        "tbnav_icp_default_align_map_params": (None, [C.POINTER(IcpAlignMapParams)]),
        "tbnav_icp_align_map": (C.c_int, [vp, vp, i32, vp, i32, dp, C.POINTER(IcpAlignMapParams), dp, C.POINTER(i32), C.POINTER(IcpInfo)]),
        "tbnav_icp_align_map_batch": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, C.POINTER(IcpAlignMapParams), vp, vp, vp]),
        "tbnav_icp_align_map_pairs": (C.c_int, [vp, vp, i32, vp, i32, dp, C.POINTER(IcpAlignMapParams), vp]),
        "tbnav_icp_last_align_map_kernel": (C.c_int, [vp, C.c_char_p, i32]),
        "tbnav_icp_default_verify_map_params": (None, [C.POINTER(IcpVerifyMapParams)]),
        "tbnav_icp_verify_map": (C.c_int, [vp, vp, i32, vp, i32, dp, C.POINTER(IcpVerifyMapParams), C.POINTER(IcpVerifyMapInfo)]),
        "tbnav_icp_verify_map_batch": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, C.POINTER(IcpVerifyMapParams), vp]),
        "tbnav_icp_verify_map_beams": (C.c_int, [vp, vp, i32, vp, i32, dp, C.POINTER(IcpVerifyMapParams), C.POINTER(IcpVerifyMapInfo), vp]),
        "tbnav_icp_last_verify_map_kernel": (C.c_int, [vp, C.c_char_p, i32]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(status: int, where: str) -> None:
    if status != OK:
        L = lib()
        detail = L.tbnav_status_string(status).decode()
        hip = L.tbnav_last_hip_error().decode()
        raise TbnavError(status, where, detail + (": " + hip if hip else ""))
