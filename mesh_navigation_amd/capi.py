"""ctypes binding of the C ABI in include/mnav.h (libmnav.so).

Plumbing only: numpy arrays in, numpy arrays out.  There is no CPU fallback -- if the HIP
library is missing or no GPU is usable, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import time
import weakref
from dataclasses import dataclass

import numpy as np

from . import build as _build

NONE = 0xFFFFFFFF
SUCCESS, CANCELED, INVALID_START, INVALID_GOAL, NO_PATH_FOUND, INTERNAL_ERROR = 0, 51, 52, 53, 54, 60
SCHEDULE_NONE, SCHEDULE_COMMITTED, SCHEDULE_NO_SLOT, SCHEDULE_OPEN = 0, 1, 2, 3     # mnav_fleet_schedule: status per robot
SCHEDULE_SEED_FREE = 1      # mnav_fleet_schedule: flag bit 0
BEYOND_FIELD = 70           # mnav_fleet_paths: the resident field cannot answer for this robot
WALK_NO_FACE = -3           # mnav_fleet_walks: no face at the start

# every symbol include/mnav.h declares
SYMBOLS = [
    "mnav_create", "mnav_destroy", "mnav_last_error", "mnav_set_face_circulation", "mnav_upload_mesh", "mnav_upload_costs",
    "mnav_compute_edge_weights", "mnav_combine_costs", "mnav_plan_dijkstra", "mnav_plan_cvp", "mnav_plan_dijkstra_batch", "mnav_plan_cvp_batch",
    "mnav_cancel", "mnav_get_stats", "mnav_get_timing", "mnav_tb_finalize_stats", "mnav_tb_engine_stats", "mnav_set_band_width", "mnav_set_dijkstra_engine", "mnav_device_output",
    "mnav_algorithmic_bytes", "mnav_shard_setup", "mnav_shard_setup_partition", "mnav_shard_walk", "mnav_device_bytes", "mnav_shard_info", "mnav_shard_begin", "mnav_shard_rounds", "mnav_shard_apply", "mnav_shard_rounds_async", "mnav_shard_apply_async",
    "mnav_shard_finalize", "mnav_update_costs", "mnav_update_edge_weights", "mnav_download_costs", "mnav_set_resident_outputs", "mnav_download_output",
    "mnav_vector_at", "mnav_backtrack_cvp", "mnav_backtrack_cvp_batch", "mnav_layer_upload", "mnav_layer_steepness", "mnav_layer_inflation", "mnav_layer_download",
    "mnav_combine_layers", "mnav_layer_stats", "mnav_layer_download_vectors", "mnav_combine_layers_update",
    "mnav_layer_obstacle", "mnav_obstacle_stats",
    "mnav_layer_height_diff", "mnav_layer_roughness", "mnav_layer_ridge", "mnav_neighbourhood_stats",
    "mnav_layer_border", "mnav_layer_clearance", "mnav_clearance_download", "mnav_clearance_stats",
    "mnav_locate", "mnav_locate_stats", "mnav_plan_dijkstra_batch_at", "mnav_plan_cvp_batch_at",
    "mnav_follow_batch", "mnav_follow_stats", "mnav_follow_rollout", "mnav_rollout_stats", "mnav_fleet_rollout", "mnav_fleet_rollout_stats",
    "mnav_fleet_rollout_yield", "mnav_fleet_yield_stats", "mnav_fleet_rollout_rings", "mnav_fleet_ring_stats",
    "mnav_follow_sample", "mnav_sample_stats",
    "mnav_map_configure", "mnav_map_compute", "mnav_map_layer_changed", "mnav_map_update_layer", "mnav_map_obstacle", "mnav_map_stats",
    "mnav_replan_dijkstra_batch", "mnav_replan_plans", "mnav_replan_stats", "mnav_replan_dijkstra_each", "mnav_replan_each_stats",
    "mnav_replan_warm_stats",
    "mnav_fleet_paths", "mnav_fleet_walks", "mnav_fleet_stats",
    "mnav_upload_face_normals", "mnav_fleet_plans", "mnav_fleet_walk_plans",
    "mnav_fleet_costs", "mnav_fleet_assign", "mnav_dispatch_stats",
    "mnav_fleet_traffic", "mnav_traffic_download", "mnav_traffic_stats", "mnav_layer_traffic", "mnav_map_traffic",
    "mnav_fleet_timed_traffic", "mnav_timed_traffic_download", "mnav_timed_traffic_stats", "mnav_layer_timed_traffic", "mnav_map_timed_traffic",
    "mnav_fleet_schedule", "mnav_schedule_stats",
    "mnav_set_option", "mnav_get_option", "mnav_shard_set_goal_tie", "mnav_last_engine",
]


class _PathRows:
    """The vertex paths of a batch, row k copied out when it is asked for (valid until the context's next batch call)."""

    def __init__(self, buf, lens, cap):
        self._buf, self._lens, self._cap = buf, lens, cap

    def __len__(self):
        return self._lens.shape[0]

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self[i] for i in range(*k.indices(len(self)))]
        if k < 0:
            k += len(self)
        return self._buf[k, : min(int(self._lens[k]), self._cap)].copy()

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class Stats(C.Structure):
    _fields_ = [("steps", C.c_uint32), ("launches", C.c_uint32), ("bands", C.c_uint32), ("armed", C.c_uint32),
                ("goal_dist", C.c_float), ("n_plans", C.c_uint32), ("evals", C.c_uint64), ("settled", C.c_uint64),
                ("ms_init", C.c_float), ("ms_propagation", C.c_float), ("ms_vector_map", C.c_float),
                ("ms_path", C.c_float), ("ms_download", C.c_float), ("ms_total", C.c_float), ("ms_step_kernels", C.c_float),
                ("band_shrinks", C.c_uint32), ("band_cuts", C.c_uint32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class FollowConfig(C.Structure):
    """mnav_follow_config (include/mnav.h): the parameters of mesh_controller.h:193-200 with their defaults."""
    _fields_ = [("max_lin_velocity", C.c_double), ("max_ang_velocity", C.c_double), ("arrival_fading", C.c_double),
                ("ang_vel_factor", C.c_double), ("lin_vel_factor", C.c_double), ("max_angle", C.c_double),
                ("max_search_radius", C.c_double), ("max_search_distance", C.c_double)]
    DEFAULTS = dict(max_lin_velocity=1.0, max_ang_velocity=0.5, arrival_fading=0.5, ang_vel_factor=1.0, lin_vel_factor=1.0,
                    max_angle=20.0, max_search_radius=0.4, max_search_distance=0.4)

    def __init__(self, **kw):
        super().__init__(**{**self.DEFAULTS, **kw})


FOLLOW_OK, FOLLOW_OUT_OF_MAP, FOLLOW_NO_FIELD = 0, 1, 2


class RolloutConfig(C.Structure):
    """mnav_rollout_config (include/mnav.h): the tick length, isGoalReached's tolerances, the ticks of the call and the
    stride of the optional trace."""
    _fields_ = [("dt", C.c_double), ("dist_tolerance", C.c_double), ("angle_tolerance", C.c_double), ("ticks", C.c_uint32),
                ("trace_stride", C.c_uint32)]
    DEFAULTS = dict(dt=0.1, dist_tolerance=0.2, angle_tolerance=0.8, ticks=1, trace_stride=0)

    def __init__(self, **kw):
        super().__init__(**{**self.DEFAULTS, **kw})


ROLLOUT_RUNNING, ROLLOUT_REACHED, ROLLOUT_OUT_OF_MAP, ROLLOUT_NO_FIELD = 0, 1, 2, 3


class SeparationConfig(C.Structure):
    """mnav_separation_config (include/mnav.h): the radius of the separation check of a fleet rollout, the ticks between
    two checks and the MNAV_SEP_* flags."""
    _fields_ = [("radius", C.c_double), ("check_stride", C.c_uint32), ("flags", C.c_uint32)]
    DEFAULTS = dict(radius=0.5, check_stride=1, flags=0)

    def __init__(self, **kw):
        super().__init__(**{**self.DEFAULTS, **kw})


SEP_WAITING_PRESENT, SEP_REACHED_PRESENT = 1, 2


class YieldConfig(C.Structure):
    """mnav_yield_config (include/mnav.h): the cosine of the half angle of the cone in which a partner counts as ahead, and
    the reserved flags (0)."""
    _fields_ = [("ahead_cos", C.c_double), ("flags", C.c_uint32)]
    DEFAULTS = dict(ahead_cos=0.5, flags=0)

    def __init__(self, **kw):
        super().__init__(**{**self.DEFAULTS, **kw})


class RingConfig(C.Structure):
    """mnav_ring_config (include/mnav.h): the MNAV_RING_* flags of the wait-for analysis of a yielding fleet rollout."""
    _fields_ = [("flags", C.c_uint32)]
    DEFAULTS = dict(flags=0)

    def __init__(self, **kw):
        super().__init__(**{**self.DEFAULTS, **kw})


RING_RELEASE = 1
WAIT_FREE, WAIT_QUEUED, WAIT_PARKED, WAIT_RING_TAIL, WAIT_RING_MEMBER = 0, 1, 2, 3, 4


class SampleConfig(C.Structure):
    """mnav_sample_config (include/mnav.h): the weights of a candidate row's score J (potential, cost integral, time), the
    vertex cost from which a row counts as lethal, and the reserved flags (0)."""
    _fields_ = [("w_potential", C.c_double), ("w_cost", C.c_double), ("w_time", C.c_double), ("lethal_cost", C.c_double), ("flags", C.c_uint32)]
    DEFAULTS = dict(w_potential=1.0, w_cost=0.0, w_time=0.0, lethal_cost=1.0, flags=0)

    def __init__(self, **kw):
        super().__init__(**{**self.DEFAULTS, **kw})


SAMPLE_PICKS = ("best_k", "best_score", "best_cmd", "n_feasible")
SAMPLE_ROWS = ("status", "ticks", "score", "potential", "lethal", "cost_integral", "travel", "pos")


class MapNode(C.Structure):
    """mnav_map_node (include/mnav.h): one node of the resident layer graph"""
    _fields_ = [("layer", C.c_uint32), ("kind", C.c_uint32), ("n_inputs", C.c_uint32), ("inputs", C.c_uint32 * 8),
                ("weights", C.c_float * 8), ("inflation_radius", C.c_double), ("inscribed_radius", C.c_double),
                ("inscribed_value", C.c_double), ("lethal_value", C.c_double), ("cost_scaling_factor", C.c_double)]


NODE_KINDS = {"input": 0, "inflation": 1, "max": 2, "avg": 3}


@dataclass
class FollowOut:
    """One mnav_follow_batch call: an array per output, one row per robot (None where the output was not asked for)."""
    code: np.ndarray | None
    face: np.ndarray | None
    bary: np.ndarray | None
    pos: np.ndarray | None
    mesh_dir: np.ndarray | None
    cost: np.ndarray | None
    cmd: np.ndarray | None        # (n, 2) float64: linear x, angular z
    how: np.ndarray | None


@dataclass
class RolloutOut:
    """One mnav_follow_rollout call: an array per output, one row per robot (None where the output was not asked for).
    `cancelled`: mnav_cancel ended the call early (`ticks` tells how far each robot came)."""
    status: np.ndarray | None
    ticks: np.ndarray | None
    pos: np.ndarray | None
    dir: np.ndarray | None
    face: np.ndarray | None
    travel: np.ndarray | None
    cost_integral: np.ndarray | None
    min_goal_dist: np.ndarray | None
    trace: np.ndarray | None      # (n, ticks // trace_stride, 3) float32, or None without a trace
    cancelled: bool = False


@dataclass
class FleetRolloutOut(RolloutOut):
    """One mnav_fleet_rollout call: RolloutOut and the separation outputs, one row per robot (None without a separation
    config or where not asked for).  `skipped`: the guard skipped at least one check (fleet_rollout_stats tells which)."""
    near_checks: np.ndarray | None = None
    max_partners: np.ndarray | None = None
    first_near_tick: np.ndarray | None = None
    first_near_robot: np.ndarray | None = None
    min_sep2: np.ndarray | None = None
    min_sep_tick: np.ndarray | None = None
    min_sep_robot: np.ndarray | None = None
    skipped: bool = False


@dataclass
class FleetYieldOut(FleetRolloutOut):
    """One mnav_fleet_rollout_yield call: FleetRolloutOut and the yield outputs, one row per robot (None without a yield
    config or where not asked for).  `hold`: the flags after the last check, what a resumed call takes as hold_in."""
    hold: np.ndarray | None = None             # (n,) uint8, 0 or 1
    hold_checks: np.ndarray | None = None
    held_ticks: np.ndarray | None = None
    first_hold_tick: np.ndarray | None = None
    first_hold_robot: np.ndarray | None = None


@dataclass
class FleetRingOut(FleetYieldOut):
    """One mnav_fleet_rollout_rings call: FleetYieldOut and the ring outputs, one row per robot (None without a ring config
    or where not asked for).  `wait_class` (WAIT_*) and `wait_anchor` are those of the last check of the call."""
    wait_class: np.ndarray | None = None       # (n,) uint8
    wait_anchor: np.ndarray | None = None
    ring_checks: np.ndarray | None = None
    first_ring_tick: np.ndarray | None = None
    parked_checks: np.ndarray | None = None
    released_checks: np.ndarray | None = None


RING_OUTPUTS = ("wait_class", "wait_anchor", "ring_checks", "first_ring_tick", "parked_checks", "released_checks")
YIELD_OUTPUTS = ("hold", "hold_checks", "held_ticks", "first_hold_tick", "first_hold_robot")
SEPARATION_OUTPUTS = ("near_checks", "max_partners", "first_near_tick", "first_near_robot", "min_sep2", "min_sep_tick", "min_sep_robot")

_lib = None


def load(path: str | None = None):
    """Load libmnav.so (building it in-tree if the sources are newer).  Raises if unavailable."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("MNAV_LIB") or _build.LIB      # MNAV_LIB: a differently built libmnav.so (perf experiments)
    if path is None and not os.path.exists(p):
        _build.build_lib()
    if not os.path.exists(p):
        raise RuntimeError(f"HIP library {p} is missing -- run `python -m mesh_navigation_amd.build`")
    L = C.CDLL(p)
    vp, u32, f64 = C.c_void_p, C.c_uint32, C.c_double
    L.mnav_create.restype = vp
    L.mnav_create.argtypes = [C.c_int]
    L.mnav_destroy.argtypes = [vp]
    L.mnav_last_error.restype = C.c_char_p
    L.mnav_last_error.argtypes = [vp]
    L.mnav_set_face_circulation.restype = C.c_int
    L.mnav_set_face_circulation.argtypes = [vp, u32, u32, vp, vp]
    L.mnav_upload_mesh.restype = C.c_int
    L.mnav_upload_mesh.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp]
    L.mnav_upload_costs.restype = C.c_int
    L.mnav_upload_costs.argtypes = [vp, vp, vp, vp]
    L.mnav_compute_edge_weights.restype = C.c_int
    L.mnav_compute_edge_weights.argtypes = [vp, vp, vp, f64, vp, vp]
    L.mnav_combine_costs.restype = C.c_int
    L.mnav_combine_costs.argtypes = [vp, C.c_int, u32, vp, vp, vp, f64, vp, vp, vp]
    L.mnav_plan_dijkstra.restype = u32
    L.mnav_plan_dijkstra.argtypes = [vp, u32, u32, f64, f64, vp, vp, vp, u32, C.POINTER(u32), vp]
    L.mnav_plan_cvp.restype = u32
    L.mnav_plan_cvp.argtypes = [vp, vp, u32, u32, f64, f64, vp, vp, vp, vp, vp]
    L.mnav_plan_dijkstra_batch.restype = u32
    L.mnav_plan_dijkstra_batch.argtypes = [vp, u32, vp, vp, f64, f64, vp, vp, vp, vp, u32, vp]
    L.mnav_plan_cvp_batch.restype = u32
    L.mnav_plan_cvp_batch.argtypes = [vp, u32, vp, vp, vp, f64, f64, vp, vp, vp, vp]
    L.mnav_locate.restype = C.c_int
    L.mnav_locate.argtypes = [vp, u32, vp, vp, vp, vp, vp]
    L.mnav_locate_stats.restype = C.c_int
    L.mnav_locate_stats.argtypes = [vp, C.POINTER(u32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
    L.mnav_plan_dijkstra_batch_at.restype = u32
    L.mnav_plan_dijkstra_batch_at.argtypes = [vp, u32, vp, vp, f64, f64, vp, vp, vp, vp, vp, vp, u32, vp]
    L.mnav_plan_cvp_batch_at.restype = u32
    L.mnav_plan_cvp_batch_at.argtypes = [vp, u32, vp, vp, f64, f64, vp, vp, vp, vp, vp, vp]
    L.mnav_follow_batch.restype = C.c_int
    L.mnav_follow_batch.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, C.POINTER(FollowConfig), vp, vp, vp, vp, vp, vp, vp, vp]
    L.mnav_follow_stats.restype = C.c_int
    L.mnav_follow_stats.argtypes = [vp] + [C.POINTER(u32)] * 6 + [C.POINTER(C.c_float)] * 2
    L.mnav_follow_rollout.restype = C.c_int
    L.mnav_follow_rollout.argtypes = [vp, u32] + [vp] * 8 + [C.POINTER(FollowConfig), C.POINTER(RolloutConfig)] + [vp] * 9
    L.mnav_fleet_rollout.restype = C.c_int
    L.mnav_fleet_rollout.argtypes = [vp, u32] + [vp] * 8 + [C.POINTER(FollowConfig), C.POINTER(RolloutConfig), vp, C.POINTER(SeparationConfig)] + [vp] * 16
    L.mnav_fleet_rollout_stats.restype = C.c_int
    L.mnav_fleet_rollout_stats.argtypes = [vp] + [vp] * 20
    L.mnav_fleet_rollout_yield.restype = C.c_int
    L.mnav_fleet_rollout_yield.argtypes = L.mnav_fleet_rollout.argtypes + [C.POINTER(YieldConfig)] + [vp] * 7
    L.mnav_fleet_yield_stats.restype = C.c_int
    L.mnav_fleet_yield_stats.argtypes = [vp] + [vp] * 12
    L.mnav_fleet_rollout_rings.restype = C.c_int
    L.mnav_fleet_rollout_rings.argtypes = L.mnav_fleet_rollout_yield.argtypes + [C.POINTER(RingConfig)] + [vp] * 6
    L.mnav_fleet_ring_stats.restype = C.c_int
    L.mnav_fleet_ring_stats.argtypes = [vp] + [vp] * 17
    L.mnav_follow_sample.restype = C.c_int
    L.mnav_follow_sample.argtypes = [vp, u32] + [vp] * 8 + [C.POINTER(FollowConfig), C.POINTER(RolloutConfig), u32, vp, C.POINTER(SampleConfig)] + [vp] * 12
    L.mnav_sample_stats.restype = C.c_int
    L.mnav_sample_stats.argtypes = [vp, C.POINTER(u32 * 4)] + [C.POINTER(u32)] * 3 + [C.POINTER(C.c_uint64)] * 4 + [C.POINTER(u32)] + [C.POINTER(C.c_float)] * 4
    L.mnav_rollout_stats.restype = C.c_int
    L.mnav_rollout_stats.argtypes = [vp, C.POINTER(u32 * 4)] + [C.POINTER(C.c_uint64)] * 4 + [C.POINTER(u32)] + [C.POINTER(C.c_float)] * 2
    L.mnav_map_configure.restype = C.c_int
    L.mnav_map_configure.argtypes = [vp, u32, C.POINTER(MapNode), u32, f64, vp]
    L.mnav_map_compute.restype = C.c_int
    L.mnav_map_compute.argtypes = [vp]
    L.mnav_map_layer_changed.restype = C.c_int
    L.mnav_map_layer_changed.argtypes = [vp, u32, u32, vp, vp, C.POINTER(u32)]
    L.mnav_map_update_layer.restype = C.c_int
    L.mnav_map_update_layer.argtypes = [vp, u32, u32, vp, vp, vp, vp, C.POINTER(u32)]
    L.mnav_map_obstacle.restype = C.c_int
    L.mnav_map_obstacle.argtypes = [vp, u32, u32, vp, u32, vp, vp, f64, f64, vp, C.POINTER(u32)]
    L.mnav_map_stats.restype = C.c_int
    L.mnav_map_stats.argtypes = [vp] + [C.POINTER(u32)] * 4 + [C.POINTER(C.c_float)] * 2
    L.mnav_replan_dijkstra_batch.restype = u32
    L.mnav_replan_dijkstra_batch.argtypes = [vp, u32, vp, f64, vp, vp, vp, vp, u32, vp]
    L.mnav_replan_dijkstra_each.restype = u32
    L.mnav_replan_dijkstra_each.argtypes = [vp, u32, vp, f64, vp, vp, vp, vp, u32, vp]
    L.mnav_replan_each_stats.restype = C.c_int
    L.mnav_replan_each_stats.argtypes = ([vp] + [C.POINTER(u32)] * 3 + [vp, vp, vp] + [C.POINTER(C.c_uint64)] * 2 + [C.POINTER(u32)] * 2
                                         + [C.POINTER(C.c_int32), vp])
    L.mnav_replan_warm_stats.restype = C.c_int
    L.mnav_replan_warm_stats.argtypes = [vp] + [C.POINTER(u32)] * 3 + [C.POINTER(C.c_uint64)] * 2 + [vp] + [C.POINTER(u32)] * 2
    L.mnav_replan_plans.restype = u32
    L.mnav_replan_plans.argtypes = [vp]
    L.mnav_replan_stats.restype = C.c_int
    L.mnav_replan_stats.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), vp] + [C.POINTER(C.c_uint64)] * 2 + [C.POINTER(u32)] * 2 + [C.POINTER(C.c_float)] * 4
    L.mnav_cancel.argtypes = [vp]
    L.mnav_get_stats.restype = C.c_int
    L.mnav_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.mnav_get_timing.restype = C.c_int
    L.mnav_get_timing.argtypes = [vp, C.POINTER(Stats)]
    L.mnav_tb_finalize_stats.restype = C.c_int
    L.mnav_tb_finalize_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(u32)]
    L.mnav_tb_engine_stats.restype = C.c_int
    L.mnav_tb_engine_stats.argtypes = [vp, C.POINTER(u32)] + [C.POINTER(C.c_uint64)] * 4
    L.mnav_set_band_width.restype = C.c_int
    L.mnav_set_band_width.argtypes = [vp, C.c_float]
    L.mnav_set_dijkstra_engine.restype = C.c_int
    L.mnav_set_dijkstra_engine.argtypes = [vp, C.c_int]
    L.mnav_shard_set_goal_tie.restype = C.c_int
    L.mnav_shard_set_goal_tie.argtypes = [vp, u32]
    L.mnav_set_option.restype = C.c_int
    L.mnav_set_option.argtypes = [vp, C.c_char_p, C.c_double]
    L.mnav_get_option.restype = C.c_double
    L.mnav_get_option.argtypes = [vp, C.c_char_p]
    L.mnav_device_output.restype = vp
    L.mnav_device_output.argtypes = [vp, u32, C.c_int]
    L.mnav_set_resident_outputs.restype = C.c_int
    L.mnav_set_resident_outputs.argtypes = [vp, C.c_int]
    L.mnav_download_output.restype = C.c_int
    L.mnav_download_output.argtypes = [vp, u32, C.c_int, vp]
    L.mnav_backtrack_cvp_batch.restype = C.c_int
    L.mnav_backtrack_cvp_batch.argtypes = [vp, u32, vp, vp, vp, vp, C.c_double, C.c_int32, u32, vp, vp, vp, vp]
    L.mnav_backtrack_cvp.restype = C.c_int
    L.mnav_backtrack_cvp.argtypes = [vp, vp, u32, vp, u32, C.c_double, C.c_int32, u32, vp, vp, vp]
    L.mnav_vector_at.restype = C.c_int
    L.mnav_vector_at.argtypes = [vp, u32, vp, vp, vp]
    L.mnav_update_costs.restype = C.c_int
    L.mnav_update_costs.argtypes = [vp, u32, vp, vp]
    L.mnav_update_edge_weights.restype = C.c_int
    L.mnav_update_edge_weights.argtypes = [vp, u32, vp, vp]
    L.mnav_download_costs.restype = C.c_int
    L.mnav_download_costs.argtypes = [vp, vp, vp]
    L.mnav_layer_upload.restype = C.c_int
    L.mnav_layer_upload.argtypes = [vp, u32, vp, vp]
    L.mnav_layer_steepness.restype = C.c_int
    L.mnav_layer_steepness.argtypes = [vp, u32, f64]
    L.mnav_layer_inflation.restype = C.c_int
    L.mnav_layer_inflation.argtypes = [vp, u32, u32, f64, f64, f64, f64, f64, vp]
    L.mnav_layer_download.restype = C.c_int
    L.mnav_layer_download.argtypes = [vp, u32, vp, vp, vp]
    L.mnav_combine_layers_update.restype = C.c_int
    L.mnav_combine_layers_update.argtypes = [vp, C.c_int, u32, vp, vp, u32, vp]
    L.mnav_layer_download_vectors.restype = C.c_int
    L.mnav_layer_download_vectors.argtypes = [vp, u32, vp, vp]
    L.mnav_combine_layers.restype = C.c_int
    L.mnav_combine_layers.argtypes = [vp, C.c_int, u32, vp, vp, f64, vp]
    L.mnav_layer_stats.restype = C.c_int
    L.mnav_layer_stats.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(u32), C.POINTER(C.c_float)]
    L.mnav_layer_obstacle.restype = C.c_int
    L.mnav_layer_obstacle.argtypes = [vp, u32, u32, vp, u32, vp, vp, f64, f64, vp, C.POINTER(u32), C.POINTER(u32)]
    L.mnav_obstacle_stats.restype = C.c_int
    L.mnav_obstacle_stats.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    for name in ("mnav_layer_height_diff", "mnav_layer_roughness", "mnav_layer_ridge"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [vp, u32, f64, f64]
    L.mnav_neighbourhood_stats.restype = C.c_int
    L.mnav_neighbourhood_stats.argtypes = [vp, C.POINTER(u32), C.POINTER(C.c_uint64), C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_float)]
    for name in ("mnav_layer_border", "mnav_layer_clearance"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [vp, u32, f64, f64, vp, C.POINTER(u32), C.POINTER(u32)]
    L.mnav_clearance_download.restype = C.c_int
    L.mnav_clearance_download.argtypes = [vp, vp]
    L.mnav_clearance_stats.restype = C.c_int
    L.mnav_clearance_stats.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.mnav_shard_setup.restype = C.c_int
    L.mnav_shard_setup.argtypes = [vp, u32, u32]
    L.mnav_shard_setup_partition.restype = C.c_int
    L.mnav_shard_setup_partition.argtypes = [vp, u32, C.POINTER(u32), C.POINTER(C.c_uint8)]
    L.mnav_shard_walk.restype = C.c_int
    L.mnav_shard_walk.argtypes = [vp, u32, u32, u32, C.POINTER(u32)]
    L.mnav_device_bytes.restype = C.c_uint64
    L.mnav_device_bytes.argtypes = [vp]
    L.mnav_shard_info.restype = C.c_int
    L.mnav_shard_info.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.mnav_shard_begin.restype = C.c_int
    L.mnav_shard_begin.argtypes = [vp, u32, u32, f64, f64]
    L.mnav_shard_rounds.restype = C.c_int
    L.mnav_shard_rounds.argtypes = [vp, u32, vp]
    L.mnav_shard_rounds_async.restype = C.c_int
    L.mnav_shard_rounds_async.argtypes = [vp, u32, vp, vp]
    L.mnav_shard_apply_async.restype = C.c_int
    L.mnav_shard_apply_async.argtypes = [vp, vp, vp, vp]
    L.mnav_shard_apply.restype = C.c_int
    L.mnav_shard_apply.argtypes = [vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.mnav_shard_finalize.restype = C.c_int
    L.mnav_shard_finalize.argtypes = [vp, vp, vp]
    L.mnav_algorithmic_bytes.restype = C.c_uint64
    L.mnav_algorithmic_bytes.argtypes = [vp]
    L.mnav_last_engine.restype = C.c_int
    L.mnav_last_engine.argtypes = [vp]
    L.mnav_fleet_paths.restype = C.c_int
    L.mnav_fleet_paths.argtypes = [vp, u32] + [vp] * 9 + [C.c_uint64, vp]
    L.mnav_fleet_walks.restype = C.c_int
    L.mnav_fleet_walks.argtypes = [vp, u32, vp, u32, vp, vp, vp, vp, f64, C.c_int32, u32] + [vp] * 6 + [C.c_uint64, vp]
    L.mnav_upload_face_normals.restype = C.c_int
    L.mnav_upload_face_normals.argtypes = [vp, u32, vp]
    L.mnav_fleet_plans.restype = C.c_int
    L.mnav_fleet_plans.argtypes = [vp, u32, vp, vp, vp, u32] + [vp] * 8 + [C.c_uint64, vp]
    L.mnav_fleet_walk_plans.restype = C.c_int
    L.mnav_fleet_walk_plans.argtypes = [vp, u32, vp, u32, vp, vp, vp, vp, vp, f64, C.c_int32, u32] + [vp] * 6 + [C.c_uint64, vp]
    L.mnav_fleet_stats.restype = C.c_int
    L.mnav_fleet_stats.argtypes = [vp] + [C.POINTER(u32)] * 4 + [C.POINTER(C.c_uint64)] + [C.POINTER(u32)] * 2 + [C.POINTER(C.c_float)] * 2
    L.mnav_fleet_costs.restype = C.c_int
    L.mnav_fleet_costs.argtypes = [vp, u32, vp, vp, u32] + [vp] * 6
    L.mnav_fleet_assign.restype = C.c_int
    L.mnav_fleet_assign.argtypes = [vp, u32, vp, vp, u32, vp, f64] + [vp] * 6
    L.mnav_dispatch_stats.restype = C.c_int
    L.mnav_dispatch_stats.argtypes = [vp] + [vp] * 11
    L.mnav_fleet_traffic.restype = C.c_int
    L.mnav_fleet_traffic.argtypes = [vp, u32, vp, vp, vp, vp, C.c_int, vp, vp, vp]
    L.mnav_traffic_download.restype = C.c_int
    L.mnav_traffic_download.argtypes = [vp, vp]
    L.mnav_traffic_stats.restype = C.c_int
    L.mnav_traffic_stats.argtypes = [vp, C.POINTER(u32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)] + [C.POINTER(u32)] * 3 + [C.POINTER(C.c_float)] * 2
    L.mnav_fleet_timed_traffic.restype = C.c_int
    L.mnav_fleet_timed_traffic.argtypes = [vp, u32] + [vp] * 7 + [u32, f64, u32, C.c_int] + [vp] * 8
    L.mnav_timed_traffic_download.restype = C.c_int
    L.mnav_timed_traffic_download.argtypes = [vp] * 5
    L.mnav_timed_traffic_stats.restype = C.c_int
    L.mnav_timed_traffic_stats.argtypes = [vp, C.POINTER(u32)] + [C.POINTER(C.c_uint64)] * 5 + [C.POINTER(u32)] * 4 + [C.POINTER(C.c_float)] * 2
    L.mnav_fleet_schedule.restype = C.c_int
    L.mnav_fleet_schedule.argtypes = [vp, u32] + [vp] * 7 + [u32, f64] + [u32] * 4 + [C.c_int] + [vp] * 7
    L.mnav_schedule_stats.restype = C.c_int
    L.mnav_schedule_stats.argtypes = [vp] + [C.POINTER(u32)] * 7 + [C.POINTER(C.c_uint64)] * 2 + [C.POINTER(u32)] + [C.POINTER(C.c_float)] * 2
    for name in ("mnav_layer_traffic", "mnav_map_traffic", "mnav_layer_timed_traffic", "mnav_map_timed_traffic"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [vp, u32, u32, f64, f64, vp, C.POINTER(u32)]
    if path is None:
        _lib = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def quat_to_matrix(q_wxyz, translation) -> np.ndarray:
    """Row-major 3x4 float32 [R | t]: R = Eigen::Quaternionf(w, x, y, z).normalized().toRotationMatrix(), restated in
    float32 with Eigen's formula (Quaternion.h toRotationMatrix); bit equality with Eigen's build is not pinned."""
    f = np.float32
    q = np.asarray(q_wxyz, f).reshape(4)
    nrm = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3], dtype=f)
    w, x, y, z = (q / nrm).astype(f)
    tx, ty, tz = f(2) * x, f(2) * y, f(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = f(1)
    R = np.array([[one - (tyy + tzz), txy - twz, txz + twy],
                  [txy + twz, one - (txx + tzz), tyz - twx],
                  [txz - twy, tyz + twx, one - (txx + tyy)]], f)
    return np.ascontiguousarray(np.concatenate([R, np.asarray(translation, f).reshape(3, 1)], axis=1), f)


@dataclass
class DijkstraOut:
    code: int
    dist: np.ndarray | None
    pred: np.ndarray | None
    path: np.ndarray          # dijkstra() list order: seed first ... pred[target]
    vecmap: np.ndarray | None
    stats: dict


@dataclass
class CvpOut:
    code: int
    dist: np.ndarray | None
    pred: np.ndarray | None
    direction: np.ndarray | None
    cutface: np.ndarray | None
    vecmap: np.ndarray | None
    stats: dict


def _engine_name(e: int) -> str:
    return {0: "k_tile_round (tile rounds)", 1: "k_step (band steps)", 5: "k_tb_solve_q (tile-batch engine, quarters of a wave, distances in LDS)",
            21: "k_tbv_solve (tile-batch engine, one wave per tile, distances in VGPRs)", 6: "k_plan_async (asynchronous tile engine)"}.get(e, "none")


def _warm_name(kernel: int) -> str:
    return "k_tb_warm + %s (tile-batch engine started from the rewound fields)" % ("k_tbv_solve" if kernel == 1 else "k_tb_solve_q")


class MnavContext:
    """One device context = one planner instance's device state (mnav_ctx)."""

    def __init__(self, device: int = 0):
        self._L = load()
        self._h = self._L.mnav_create(int(device))
        if not self._h:
            raise RuntimeError("mnav_create failed: no usable MI355X/HIP device (there is no CPU fallback)")
        self.V = self.F = self.E = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.mnav_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _err(self) -> str:
        return (self._L.mnav_last_error(self._h) or b"").decode()

    def upload_mesh(self, xyz, faces, edges, vertex_normals=None, face_circulation=None):
        """face_circulation: optional (vf_ptr[V+1], vf[3F]) = getFacesOfVertex rows of the caller's half-edge
        mesh; by default the library replays the half-edge construction over `faces` itself."""
        xyz, faces, edges = _f32(xyz), _u32(faces), _u32(edges)
        vn = None if vertex_normals is None else _f32(vertex_normals)
        self.V, self.F, self.E = xyz.shape[0], faces.shape[0], edges.shape[0]
        if face_circulation is not None:
            ptr, vf = _u32(face_circulation[0]), _u32(face_circulation[1])
            self._L.mnav_set_face_circulation(self._h, self.V, self.F, _p(ptr), _p(vf))
        else:
            self._L.mnav_set_face_circulation(self._h, self.V, self.F, None, None)
        rc = self._L.mnav_upload_mesh(self._h, self.V, self.F, self.E, _p(xyz), _p(faces), _p(edges), _p(vn))
        if rc != 0:
            raise RuntimeError(f"mnav_upload_mesh failed ({rc}): {self._err()}")

    def upload_costs(self, vertex_costs, edge_weights, invalid=None):
        vc, w = _f32(vertex_costs), _f32(edge_weights)
        inv = None if invalid is None else np.ascontiguousarray(invalid, dtype=np.uint8)
        rc = self._L.mnav_upload_costs(self._h, _p(vc), _p(w), _p(inv))
        if rc != 0:
            raise RuntimeError(f"mnav_upload_costs failed ({rc}): {self._err()}")

    def compute_edge_weights(self, vertex_costs, edge_distances, edge_cost_factor: float, invalid=None) -> np.ndarray:
        vc, ed = _f32(vertex_costs), _f32(edge_distances)
        inv = None if invalid is None else np.ascontiguousarray(invalid, dtype=np.uint8)
        out = np.empty(self.E, dtype=np.float32)
        rc = self._L.mnav_compute_edge_weights(self._h, _p(vc), _p(ed), float(edge_cost_factor), _p(inv), _p(out))
        if rc != 0:
            raise RuntimeError(f"mnav_compute_edge_weights failed ({rc}): {self._err()}")
        return out

    def combine_costs(self, layers, weights, edge_distances, edge_cost_factor: float, mode: str = "avg", invalid=None):
        """Max/Avg combination of dense V-sized cost layers + edge weights, on the device.
        Returns (vertex_costs, edge_weights); both also become the context's planning inputs."""
        arrs = [_f32(a) for a in layers]
        ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
        w = _f32(weights if weights is not None else np.ones(len(arrs), np.float32))
        ed = _f32(edge_distances)
        inv = None if invalid is None else np.ascontiguousarray(invalid, dtype=np.uint8)
        vc = np.empty(self.V, dtype=np.float32)
        ew = np.empty(self.E, dtype=np.float32)
        rc = self._L.mnav_combine_costs(self._h, 0 if mode == "max" else 1, len(arrs), C.cast(ptrs, C.c_void_p), _p(w), _p(ed),
                                        float(edge_cost_factor), _p(inv), _p(vc), _p(ew))
        if rc != 0:
            raise RuntimeError(f"mnav_combine_costs failed ({rc}): {self._err()}")
        return vc, ew

    def set_band_width(self, delta: float):
        self._L.mnav_set_band_width(self._h, float(delta))

    def set_dijkstra_engine(self, engine: str):
        """'auto' (default), 'tiled', 'band', 'tile_batch' (large batches: one plan per lane)
        or 'async' (the tiles without rounds, mnav_async.h: what 'auto' takes for single plans and small batches)."""
        if self._L.mnav_set_dijkstra_engine(self._h, {"tiled": 0, "band": 1, "auto": 3, "tile_batch": 5, "async": 6}[engine]) != 0:
            raise ValueError(f"engine {engine!r} refused")

    def set_option(self, name: str, value=None):
        """Tuning / debug option by name (csrc/mnav_options.h); None restores the built-in default.  The library reads the
        environment once, in mnav_create: after that this is the only way to change an option."""
        if self._L.mnav_set_option(self._h, name.encode(), float("nan") if value is None else float(value)) != 0:
            raise ValueError(f"mnav_set_option: {self._err()}")

    def get_option(self, name: str):
        v = self._L.mnav_get_option(self._h, name.encode())
        return None if v != v else v

    def set_resident_outputs(self, on: bool = True):
        self._L.mnav_set_resident_outputs(self._h, 1 if on else 0)

    def download_output(self, what: str, slot: int = 0) -> np.ndarray:
        code = {"dist": 0, "pred": 1, "direction": 2, "cutface": 3, "vecmap": 4, "popped": 5}[what]
        out = np.empty((self.V, 3) if code == 4 else self.V, np.uint32 if code in (1, 3) else np.float32)
        if self._L.mnav_download_output(self._h, int(slot), code, _p(out)) != 0:
            raise RuntimeError(f"mnav_download_output failed: {self._err()}")
        return out

    def vector_at(self, vs, bary, slot: int = 0):
        out = np.zeros(3, np.float32)
        rc = self._L.mnav_vector_at(self._h, int(slot), _p(_u32(vs)), _p(_f32(bary)), _p(out))
        if rc < 0:
            raise RuntimeError(f"mnav_vector_at failed: {self._err()}")
        return out if rc == 1 else None

    def backtrack_cvp_batch(self, seed_pos, seed_faces, target_pos, target_faces, step_width: float = 0.4, inflation_layer: int = -1,
                            cap: int = 4096):
        """CVPMeshPlanner's back-tracking (cvp_mesh_planner.cpp:920-951) on the resident vector maps of the last CVP call:
        list of (status, positions[n,3], faces[n]) per plan, reference list order (seed first); status 1 = reached."""
        sp, tp = _f32(seed_pos).reshape(-1, 3), _f32(target_pos).reshape(-1, 3)
        sf, tf = _u32(seed_faces).reshape(-1), _u32(target_faces).reshape(-1)
        n = sf.shape[0]
        pos = np.empty((n, cap, 3), np.float32)
        face = np.empty((n, cap), np.uint32)
        cnt = np.zeros(n, np.uint32)
        st = np.zeros(n, np.int32)
        rc = self._L.mnav_backtrack_cvp_batch(self._h, n, _p(sp), _p(sf), _p(tp), _p(tf), float(step_width), int(inflation_layer), int(cap),
                                              _p(pos), _p(face), _p(cnt), _p(st))
        if rc != 0:
            raise RuntimeError(f"mnav_backtrack_cvp_batch failed ({rc}): {self._err()}")
        return [(int(st[i]), pos[i, : cnt[i]].copy(), face[i, : cnt[i]].copy()) for i in range(n)]

    def backtrack_cvp(self, seed_pos, seed_face, target_pos, target_face, step_width: float = 0.4, inflation_layer: int = -1, cap: int = 4096):
        return self.backtrack_cvp_batch([seed_pos], [seed_face], [target_pos], [target_face], step_width, inflation_layer, cap)[0]

    def update_costs(self, vertex_ids, values):
        """Incremental cost change (layerChanged + updateEdgeWeights(changed)) on the device."""
        ids, vals = _u32(vertex_ids), _f32(values)
        rc = self._L.mnav_update_costs(self._h, ids.shape[0], _p(ids), _p(vals))
        if rc != 0:
            raise RuntimeError(f"mnav_update_costs failed ({rc}): {self._err()}")

    def update_edge_weights(self, edge_ids, values):
        """The caller's own incremental edge weights (MeshMap::updateEdgeWeights ran on the host): scatter into the resident weights."""
        ids, vals = _u32(edge_ids), _f32(values)
        rc = self._L.mnav_update_edge_weights(self._h, ids.shape[0], _p(ids), _p(vals))
        if rc != 0:
            raise RuntimeError(f"mnav_update_edge_weights failed ({rc}): {self._err()}")

    def download_costs(self):
        vc = np.empty(self.V, np.float32)
        w = np.empty(self.E, np.float32)
        if self._L.mnav_download_costs(self._h, _p(vc), _p(w)) != 0:
            raise RuntimeError(f"mnav_download_costs failed: {self._err()}")
        return vc, w

    # ---- cost layers on the device (mesh_layers: Steepness, Inflation, Combination) ----
    def layer_upload(self, layer: int, costs, lethal=None):
        c = np.ascontiguousarray(costs, np.float32)
        le = None if lethal is None else np.ascontiguousarray(lethal, np.uint8)
        if self._L.mnav_layer_upload(self._h, int(layer), _p(c), None if le is None else _p(le)) != 0:
            raise RuntimeError(f"mnav_layer_upload failed: {self._err()}")

    def layer_steepness(self, layer: int, threshold: float = 0.3):
        if self._L.mnav_layer_steepness(self._h, int(layer), float(threshold)) != 0:
            raise RuntimeError(f"mnav_layer_steepness failed: {self._err()}")

    def layer_inflation(self, layer: int, input_layer: int, inflation_radius=0.4, inscribed_radius=0.25, inscribed_value=0.99,
                        lethal_value=1.0, cost_scaling_factor=1.0, invalid=None) -> dict:
        """InflationLayer defaults: inflation_layer.cpp:676-712.  Returns the wave's counters."""
        inv = None if invalid is None else np.ascontiguousarray(invalid, np.uint8)
        rc = self._L.mnav_layer_inflation(self._h, int(layer), int(input_layer), float(inflation_radius), float(inscribed_radius),
                                          float(inscribed_value), float(lethal_value), float(cost_scaling_factor),
                                          None if inv is None else _p(inv))
        if rc != 0:
            raise RuntimeError(f"mnav_layer_inflation failed: {self._err()}")
        a, b, e, ms, vs, mw = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_float(), C.c_uint32(), C.c_float()
        self._L.mnav_layer_stats(self._h, C.byref(a), C.byref(b), C.byref(e), C.byref(ms), C.byref(vs), C.byref(mw))
        return dict(steps=a.value, bands=b.value, evals=e.value, ms=ms.value, ms_wave=mw.value, verify_sweeps=vs.value)

    def layer_obstacle(self, layer: int, points, sensor_to_map=None, rotation_wxyz=None, translation=None,
                       down_axis=(0.0, 0.0, -1.0), robot_height: float = np.inf, max_obstacle_dist: float = np.inf) -> dict:
        """ObstacleLayer::processPointCloud on the device (mnav_layer_obstacle, include/mnav.h).

        points: an (n, 3) float32 array, or a structured array whose float32 fields x, y, z sit at byte offsets 0, 4, 8
        (any itemsize: it is the point_step).  The sensor-to-map transform is either `sensor_to_map`, a row-major 3x4
        matrix, or `rotation_wxyz` + `translation`, turned into one here with Eigen's Quaternion::toRotationMatrix formula
        after normalising the quaternion, in float32 (the reference does that conversion with Eigen; that the two agree
        bit for bit is not pinned).  Neither = identity.  down_axis is already in the map frame and used as given.
        Returns dict(changed = ascending uint32 ids whose lethal flag changed, n_lethal, stats = the call's counters)."""
        args = self._obstacle_args(points, sensor_to_map, rotation_wxyz, translation, down_axis, robot_height, max_obstacle_dist)
        out = self._change_layer("mnav_layer_obstacle", layer, *args[1:])
        out["stats"] = self.obstacle_stats()
        return out

    @staticmethod
    def _obstacle_args(points, sensor_to_map, rotation_wxyz, translation, down_axis, robot_height, max_obstacle_dist):
        """the arguments of mnav_layer_obstacle from n_points to max_obstacle_dist, behind the arrays they point into"""
        pts = np.asarray(points)
        if pts.dtype.names:
            f = pts.dtype.fields
            if any(k not in f or f[k][0] != np.float32 or f[k][1] != o for k, o in (("x", 0), ("y", 4), ("z", 8))):
                raise ValueError("structured points need float32 fields x, y, z at byte offsets 0, 4, 8")
            pts = np.ascontiguousarray(pts.reshape(-1))
            step = pts.dtype.itemsize
        else:
            pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
            step = 12
        n = int(pts.shape[0])
        if sensor_to_map is not None and rotation_wxyz is not None:
            raise ValueError("give sensor_to_map or rotation_wxyz / translation, not both")
        m = None
        if sensor_to_map is not None:
            m = _f32(sensor_to_map).reshape(3, 4)
        elif rotation_wxyz is not None:
            m = quat_to_matrix(rotation_wxyz, (0.0, 0.0, 0.0) if translation is None else translation)
        d = _f32(down_axis).reshape(3)
        return (pts, m, d), n, _p(pts) if n else None, int(step), _p(m), _p(d), float(robot_height), float(max_obstacle_dist)

    def obstacle_stats(self) -> dict:
        k, h, lr, mb, mc, mt = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_float(), C.c_float(), C.c_float()
        self._L.mnav_obstacle_stats(self._h, C.byref(k), C.byref(h), C.byref(lr), C.byref(mb), C.byref(mc), C.byref(mt))
        return dict(rays_kept=k.value, hits=h.value, lethal_rays=lr.value, ms_bvh_build=mb.value, ms_cast=mc.value, ms_total=mt.value)

    # local-neighbourhood layers (mnav_layer_height_diff / _roughness / _ridge, include/mnav.h); defaults: the reference's
    # height_diff_layer.h:132-133, roughness_layer.h:133-134, ridge_layer.h:135-136.  Each returns neighbourhood_stats().
    def layer_height_diff(self, layer: int, radius: float = 0.3, threshold: float = 0.185) -> dict:
        return self._nbhd("mnav_layer_height_diff", layer, radius, threshold)

    def layer_roughness(self, layer: int, radius: float = 0.3, threshold: float = 0.3) -> dict:
        return self._nbhd("mnav_layer_roughness", layer, radius, threshold)

    def layer_ridge(self, layer: int, radius: float = 0.3, threshold: float = 0.3) -> dict:
        return self._nbhd("mnav_layer_ridge", layer, radius, threshold)

    def _nbhd(self, name: str, layer: int, radius: float, threshold: float) -> dict:
        if getattr(self._L, name)(self._h, int(layer), float(radius), float(threshold)) != 0:
            raise RuntimeError(f"{name} failed: {self._err()}")
        return self.neighbourhood_stats()

    def neighbourhood_stats(self) -> dict:
        """The last neighbourhood layer call: centres, sum and maximum of |N(v)|, centres that left the LDS path, device ms."""
        c, v, m, s, ms = C.c_uint32(), C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_float()
        self._L.mnav_neighbourhood_stats(self._h, C.byref(c), C.byref(v), C.byref(m), C.byref(s), C.byref(ms))
        return dict(centres=c.value, visits=v.value, max_size=m.value, spilled=s.value, ms=ms.value)

    # border and clearance layers (mnav_layer_border / mnav_layer_clearance, include/mnav.h); defaults: the reference's
    # border_layer.h:132-133 and clearance_layer.h:135-136.  Both return dict(changed = ascending uint32 ids whose lethal
    # flag or cost bits changed, n_lethal, stats).
    def layer_border(self, layer: int, border_cost: float = 1.0, threshold: float = 0.5) -> dict:
        """stats: the host wall-clock milliseconds of the call (ms_wall)"""
        t0 = time.perf_counter()
        out = self._change_layer("mnav_layer_border", layer, float(border_cost), float(threshold))
        out["stats"] = dict(ms_wall=(time.perf_counter() - t0) * 1e3)
        return out

    def layer_clearance(self, layer: int, robot_height: float = 0.5, height_inflation: float = 0.3) -> dict:
        """the first call after upload_mesh casts the rays (and builds the BVH if no obstacle call did); later calls only
        recompute the costs from the cached clearance.  stats: clearance_stats()"""
        out = self._change_layer("mnav_layer_clearance", layer, float(robot_height), float(height_inflation))
        out["stats"] = self.clearance_stats()
        return out

    def _change_layer(self, name: str, layer: int, *args) -> dict:
        """a layer call whose C signature ends in (changed_out, n_changed, n_lethal): dict(changed, n_lethal)"""
        changed = np.empty(max(self.V, 1), np.uint32)
        nc, nl = C.c_uint32(), C.c_uint32()
        if getattr(self._L, name)(self._h, int(layer), *args, _p(changed), C.byref(nc), C.byref(nl)) != 0:
            raise RuntimeError(f"{name} failed: {self._err()}")
        return dict(changed=changed[:nc.value].copy(), n_lethal=nl.value)

    def clearance(self) -> np.ndarray:
        """the cached clearance: float32[V], +inf where the vertex's ray hit nothing"""
        c = np.empty(max(self.V, 1), np.float32)
        if self._L.mnav_clearance_download(self._h, _p(c)) != 0:
            raise RuntimeError(f"mnav_clearance_download failed: {self._err()}")
        return c[:self.V]

    def clearance_stats(self) -> dict:
        """the last clearance call: cast (1) or reused the cache (0), rays cast and rays that hit by it, device ms of its BVH
        build (0 if none), of the cast (0 if reused) and of the whole call"""
        cast, r, h, mb, mc, mt = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_float(), C.c_float(), C.c_float()
        self._L.mnav_clearance_stats(self._h, C.byref(cast), C.byref(r), C.byref(h), C.byref(mb), C.byref(mc), C.byref(mt))
        return dict(cast=cast.value, rays=r.value, hits=h.value, ms_bvh_build=mb.value, ms_cast=mc.value, ms_total=mt.value)

    def layer_download(self, layer: int, distances: bool = False):
        c = np.empty(self.V, np.float32)
        le = np.empty(self.V, np.uint8)
        d = np.empty(self.V, np.float32) if distances else None
        if self._L.mnav_layer_download(self._h, int(layer), _p(c), _p(le), None if d is None else _p(d)) != 0:
            raise RuntimeError(f"mnav_layer_download failed: {self._err()}")
        return (c, le, d) if distances else (c, le)

    def layer_vectors(self, layer: int):
        """vector_map_ of an inflation layer: (V, 3) floats and the has-entry flags"""
        vec = np.empty((self.V, 3), np.float32)
        has = np.empty(self.V, np.uint8)
        if self._L.mnav_layer_download_vectors(self._h, int(layer), _p(vec), _p(has)) != 0:
            raise RuntimeError(f"mnav_layer_download_vectors failed: {self._err()}")
        return vec, has

    def combine_layers(self, layers, weights=None, mode: str = "avg", edge_cost_factor: float = 1.0, invalid=None):
        ls = np.ascontiguousarray(layers, np.uint32)
        w = np.ascontiguousarray(weights if weights is not None else [1.0] * len(ls), np.float32)
        inv = None if invalid is None else np.ascontiguousarray(invalid, np.uint8)
        if self._L.mnav_combine_layers(self._h, 0 if mode == "max" else 1, len(ls), _p(ls), _p(w), float(edge_cost_factor),
                                       None if inv is None else _p(inv)) != 0:
            raise RuntimeError(f"mnav_combine_layers failed: {self._err()}")

    def combine_layers_update(self, layers, ids, weights=None, mode: str = "avg"):
        ls = np.ascontiguousarray(layers, np.uint32)
        w = np.ascontiguousarray(weights if weights is not None else [1.0] * len(ls), np.float32)
        ii = np.ascontiguousarray(ids, np.uint32)
        if self._L.mnav_combine_layers_update(self._h, 0 if mode == "max" else 1, len(ls), _p(ls), _p(w), ii.shape[0], _p(ii)) != 0:
            raise RuntimeError(f"mnav_combine_layers_update failed: {self._err()}")

    # ---- the resident layer graph (mnav_map_*, include/mnav.h) ----
    def map_configure(self, nodes, default_layer: int, edge_cost_factor: float = 0.0, invalid=None):
        """nodes: dicts with layer, kind ("input" | "inflation" | "max" | "avg"), inputs (slots), weights (avg), and for an
        inflation node any of inflation_radius, inscribed_radius, inscribed_value, lethal_value, cost_scaling_factor
        (defaults: layer_inflation's)."""
        arr = (MapNode * max(len(nodes), 1))()
        for a, n in zip(arr, nodes):
            ins = list(n.get("inputs", ()))
            if len(ins) > 8:
                raise ValueError("a node takes at most 8 inputs")
            ws = list(n.get("weights", [1.0] * len(ins)))
            a.layer, a.kind, a.n_inputs = int(n["layer"]), NODE_KINDS[n["kind"]], len(ins)
            for k, i in enumerate(ins):
                a.inputs[k] = int(i)
            for k, w in enumerate(ws[:8]):
                a.weights[k] = float(w)
            a.inflation_radius = float(n.get("inflation_radius", 0.4))
            a.inscribed_radius = float(n.get("inscribed_radius", 0.25))
            a.inscribed_value = float(n.get("inscribed_value", 0.99))
            a.lethal_value = float(n.get("lethal_value", 1.0))
            a.cost_scaling_factor = float(n.get("cost_scaling_factor", 1.0))
        inv = None if invalid is None else np.ascontiguousarray(invalid, np.uint8)
        if self._L.mnav_map_configure(self._h, len(nodes), arr, int(default_layer), float(edge_cost_factor),
                                      None if inv is None else _p(inv)) != 0:
            raise RuntimeError(f"mnav_map_configure failed: {self._err()}")

    def map_compute(self):
        if self._L.mnav_map_compute(self._h) != 0:
            raise RuntimeError(f"mnav_map_compute failed: {self._err()}")

    def _map_call(self, name: str, layer: int, *args) -> dict:
        """an update call of the graph: dict(changed = D ascending, stats = map_stats())"""
        changed = np.empty(max(self.V, 1), np.uint32)
        nc = C.c_uint32()
        if getattr(self._L, name)(self._h, int(layer), *args, _p(changed), C.byref(nc)) != 0:
            raise RuntimeError(f"{name} failed: {self._err()}")
        return dict(changed=changed[:nc.value].copy(), stats=self.map_stats())

    def map_layer_changed(self, layer: int, ids) -> dict:
        ii = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        return self._map_call("mnav_map_layer_changed", layer, ii.shape[0], _p(ii))

    def map_update_layer(self, layer: int, ids, costs, lethal=None) -> dict:
        ii = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        cc = np.ascontiguousarray(costs, np.float32).reshape(-1)
        le = None if lethal is None else np.ascontiguousarray(lethal, np.uint8).reshape(-1)
        if cc.shape[0] != ii.shape[0] or (le is not None and le.shape[0] != ii.shape[0]):
            raise ValueError("ids, costs and lethal must have one length")
        return self._map_call("mnav_map_update_layer", layer, ii.shape[0], _p(ii), _p(cc), None if le is None else _p(le))

    def map_obstacle(self, layer: int, points, sensor_to_map=None, rotation_wxyz=None, translation=None,
                     down_axis=(0.0, 0.0, -1.0), robot_height: float = np.inf, max_obstacle_dist: float = np.inf) -> dict:
        """layer_obstacle on an input node of the graph, then the propagation; same keyword arguments"""
        args = self._obstacle_args(points, sensor_to_map, rotation_wxyz, translation, down_axis, robot_height, max_obstacle_dist)
        return self._map_call("mnav_map_obstacle", layer, *args[1:])

    def map_stats(self) -> dict:
        w, r, d, e, mt, mw = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_float(), C.c_float()
        self._L.mnav_map_stats(self._h, C.byref(w), C.byref(r), C.byref(d), C.byref(e), C.byref(mt), C.byref(mw))
        return dict(waves=w.value, recombined=r.value, default_changed=d.value, edges_reweighted=e.value, ms_total=mt.value, ms_wave=mw.value)

    # ---- one plan over several GPUs (mesh_navigation_amd/sharded.py drives these) ----
    def shard_setup(self, rank: int, world: int) -> int:
        n = self._L.mnav_shard_setup(self._h, int(rank), int(world))
        if n < 0:
            raise RuntimeError(f"mnav_shard_setup failed: {self._err()}")
        return n

    def shard_setup_partition(self, exchange_vertex: np.ndarray, owned: np.ndarray) -> int:
        """This context holds ONE PART of a partitioned mesh (include/mnav.h): `exchange_vertex[i]` = local id of interface
        vertex i or 0xFFFFFFFF, `owned[v]` = 1 for the vertices this process owns.  Returns the floats in the exchange buffer."""
        ex = np.ascontiguousarray(exchange_vertex, np.uint32)
        ow = np.ascontiguousarray(owned, np.uint8)
        if ow.shape[0] != self.V:
            raise ValueError("owned: one byte per local vertex")
        n = self._L.mnav_shard_setup_partition(self._h, ex.shape[0], ex.ctypes.data_as(C.POINTER(C.c_uint32)), ow.ctypes.data_as(C.POINTER(C.c_uint8)))
        if n < 0:
            raise RuntimeError(f"mnav_shard_setup_partition failed: {self._err()}")
        return n

    def shard_walk(self, start: int, seed: int, cap: int = 4096) -> np.ndarray:
        """One path segment inside this part (include/mnav.h): [hops, stop vertex, status, local ids...]."""
        out = np.zeros(cap + 3, np.uint32)
        if self._L.mnav_shard_walk(self._h, int(start), int(seed), int(cap), out.ctypes.data_as(C.POINTER(C.c_uint32))) != 0:
            raise RuntimeError(f"mnav_shard_walk failed: {self._err()}")
        return out

    def device_bytes(self) -> int:
        return int(self._L.mnav_device_bytes(self._h))

    def shard_info(self) -> dict:
        a, b, c, d = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        if self._L.mnav_shard_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)) != 0:
            raise RuntimeError("mnav_shard_setup has not been called")
        return dict(t_lo=a.value, t_hi=b.value, ntiles=c.value, n_exchange=d.value)

    def shard_set_goal_tie(self, tie_id: int):
        self._L.mnav_shard_set_goal_tie(self._h, int(tie_id))

    def shard_begin(self, seed: int, target: int, goal_dist_offset: float = 0.3, cost_limit: float = 1.0):
        if self._L.mnav_shard_begin(self._h, int(seed), int(target), float(goal_dist_offset), float(cost_limit)) != 0:
            raise RuntimeError(f"mnav_shard_begin failed: {self._err()}")

    def shard_rounds(self, rounds: int, buf_ptr: int) -> int:
        rc = self._L.mnav_shard_rounds(self._h, int(rounds), C.c_void_p(buf_ptr))
        if rc < 0:
            raise RuntimeError(f"mnav_shard_rounds failed: {self._err()}")
        return rc

    def shard_apply(self, buf_ptr: int):
        lm, td = C.c_float(), C.c_float()
        if self._L.mnav_shard_apply(self._h, C.c_void_p(buf_ptr), C.byref(lm), C.byref(td)) != 0:
            raise RuntimeError(f"mnav_shard_apply failed: {self._err()}")
        return lm.value, td.value

    def shard_rounds_async(self, rounds: int, buf_ptr: int, stream: int):
        if self._L.mnav_shard_rounds_async(self._h, int(rounds), C.c_void_p(buf_ptr), C.c_void_p(stream)) != 0:
            raise RuntimeError(f"mnav_shard_rounds_async failed: {self._err()}")

    def shard_apply_async(self, buf_ptr: int, ctl_ptr: int, stream: int):
        if self._L.mnav_shard_apply_async(self._h, C.c_void_p(buf_ptr), C.c_void_p(ctl_ptr), C.c_void_p(stream)) != 0:
            raise RuntimeError(f"mnav_shard_apply_async failed: {self._err()}")

    def shard_finalize(self, dist_ptr: int, pred_ptr: int):
        rc = self._L.mnav_shard_finalize(self._h, C.c_void_p(dist_ptr), C.c_void_p(pred_ptr))
        if rc != 0:
            raise RuntimeError(f"mnav_shard_finalize failed ({rc}): {self._err()}")

    def stats(self) -> dict:
        s = Stats()
        self._L.mnav_get_stats(self._h, C.byref(s))
        d = s.as_dict()
        d["algorithmic_bytes"] = int(self._L.mnav_algorithmic_bytes(self._h))
        return d

    def tb_finalize_stats(self) -> dict:
        """What the last tile-batch call's finalize pass kept (mnav_tb_finalize_stats): (tile, plan) pairs whose stores it
        skipped, pairs whose distance slice it reset itself, whether the call filled the distance buffer at its start."""
        sk, rs, fl = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        if self._L.mnav_tb_finalize_stats(self._h, C.byref(sk), C.byref(rs), C.byref(fl)) != 0:
            raise RuntimeError(f"mnav_tb_finalize_stats failed: {self._err()}")
        return dict(skipped_pairs=int(sk.value), reset_pairs=int(rs.value), filled_at_start=bool(fl.value))

    def tb_engine_stats(self) -> dict:
        """Counters of the last tile-batch engine run (mnav_tb_engine_stats); sweeps_per_item is what `tb_sweep_seq` lowers."""
        it = C.c_uint32(0)
        items, acts, sweeps, wakes = (C.c_uint64(0) for _ in range(4))
        if self._L.mnav_tb_engine_stats(self._h, C.byref(it), C.byref(items), C.byref(acts), C.byref(sweeps), C.byref(wakes)) != 0:
            raise RuntimeError(f"mnav_tb_engine_stats failed: {self._err()}")
        return dict(iterations=int(it.value), items=int(items.value), activations=int(acts.value), sweeps=int(sweeps.value), wakes=int(wakes.value),
                    sweeps_per_item=(sweeps.value / items.value) if items.value else 0.0)

    def last_engine(self) -> str:
        """Engine / kernel of the last Dijkstra call, by name (mnav_last_engine)."""
        e = int(self._L.mnav_last_engine(self._h))
        if e >= 256:                                                   # replan_dijkstra_each: the repair's rounds or warm start and / or the FRESH batch's engine
            ran = (["k_tile_round (tile rounds)"] if e & 128 else []) + ([_warm_name(1 if e & 1024 else 0)] if e & 512 else [])
            ran += [_engine_name(e & 127)] if (e & 127) != 127 else []
            return " + ".join(ran) if ran else "none (every plan kept)"
        if e in (5, 21) and self.replan_warm_stats()["live"]:          # replan_dijkstra, all plans warm
            return _warm_name(1 if e == 21 else 0)
        return _engine_name(e)

    def timing(self) -> dict:
        """Event timings of the last call; never triggers the (lazy) settled-vertex count of a tile-batch call."""
        s = Stats()
        self._L.mnav_get_timing(self._h, C.byref(s))
        return s.as_dict()

    def cancel(self):
        self._L.mnav_cancel(self._h)

    def device_output(self, slot: int, what: int) -> int:
        return int(self._L.mnav_device_output(self._h, slot, what) or 0)

    def plan_dijkstra(self, seed_vertex: int, target_vertex: int, goal_dist_offset: float = 0.3,
                      cost_limit: float = 1.0, want_fields: bool = True, want_vecmap: bool = False) -> DijkstraOut:
        V = self.V
        dist = np.empty(V, np.float32) if want_fields else None
        pred = np.empty(V, np.uint32) if want_fields else None
        vm = np.empty((V, 3), np.float32) if want_vecmap else None
        path = np.empty(max(V, 1), np.uint32)
        n = C.c_uint32(0)
        code = self._L.mnav_plan_dijkstra(self._h, int(seed_vertex) & 0xFFFFFFFF, int(target_vertex) & 0xFFFFFFFF,
                                          float(goal_dist_offset), float(cost_limit), _p(dist), _p(pred), _p(path),
                                          path.shape[0], C.byref(n), _p(vm))
        if code == INTERNAL_ERROR:
            raise RuntimeError(f"mnav_plan_dijkstra internal error: {self._err()}")
        return DijkstraOut(code, dist, pred, path[: n.value].copy(), vm, self.stats())

    def _lease_paths(self, n: int, cap: int):
        """An (n, cap) path buffer that no result handed out earlier still refers to, and the lease list a new result signs."""
        # the rows of the path buffer are only touched where a path lands: keep the (mostly untouched) buffers between calls --
        # a fresh 335 MB buffer per call costs one page fault per row (12 ms per 5120-plan batch).  A small pool, because the
        # caller usually still holds the previous call's result (which refers to its buffer) while the next call runs.
        key = (n, max(cap, 1))
        if getattr(self, "_path_buf_key", None) != key:
            self._path_pool, self._path_buf_key = [], key
        # a pooled buffer is free when no result that was handed out still refers to it: every _PathRows takes a LEASE on its
        # buffer (a weak reference to the rows object kept next to the buffer), released when the rows object dies
        paths = None
        for entry in self._path_pool:
            entry[1] = [r for r in entry[1] if r() is not None]
            if not entry[1]:
                paths = entry[0]
                lease = entry[1]
                break
        if paths is None:
            paths = np.empty(key, np.uint32)
            lease = []
            if len(self._path_pool) < 3:
                self._path_pool.append([paths, lease])
        return paths, lease

    def plan_dijkstra_batch(self, seeds, targets, goal_dist_offset: float = 0.3, cost_limit: float = 1.0,
                            want_fields: bool = False, path_cap: int | None = None, want_stats: bool = True):
        seeds, targets = _u32(seeds), _u32(targets)
        n = seeds.shape[0]
        V = self.V
        cap = int(path_cap if path_cap is not None else V)
        codes = np.empty(n, np.uint32)
        dist = np.empty((n, V), np.float32) if want_fields else None
        pred = np.empty((n, V), np.uint32) if want_fields else None
        paths, lease = self._lease_paths(n, cap)
        lens = np.zeros(n, np.uint32)
        rc = self._L.mnav_plan_dijkstra_batch(self._h, n, _p(seeds), _p(targets), float(goal_dist_offset),
                                              float(cost_limit), _p(codes), _p(dist), _p(pred), _p(paths), cap, _p(lens))
        if rc == INTERNAL_ERROR:
            raise RuntimeError(f"mnav_plan_dijkstra_batch internal error: {self._err()}")
        rows = _PathRows(paths, lens, cap)
        lease.append(weakref.ref(rows))
        return dict(rc=rc, codes=codes, dist=dist, pred=pred, paths=rows, path_len=lens,
                    stats=self.stats() if want_stats else self.timing())

    def replan_dijkstra(self, targets=None, goal_dist_offset: float = 0.3, want_dist: bool = False, want_pred: bool = False,
                        path_cap: int | None = None, want_stats: bool = True):
        """Brings the plans of the last Dijkstra call up to date with the resident costs and, when `targets` is given, with new
        robot vertices (mnav_replan_dijkstra_batch, include/mnav.h): the result of plan_dijkstra_batch on the resident map, from
        the part of the resident fields the changes cannot have touched.  Adds `replan` = replan_stats() to the dict (want_stats
        False: None, and `stats` is timing() as in plan_dijkstra_batch -- the two calls then do the same work around the C call)."""
        n = int(self._L.mnav_replan_plans(self._h)) if targets is None else int(_u32(targets).shape[0])
        tg = None if targets is None else _u32(targets)
        V = self.V
        cap = int(path_cap if path_cap is not None else V)
        codes = np.empty(n, np.uint32)
        dist = np.empty((n, V), np.float32) if want_dist else None
        pred = np.empty((n, V), np.uint32) if want_pred else None
        paths, lease = self._lease_paths(n, cap)
        lens = np.zeros(n, np.uint32)
        rc = self._L.mnav_replan_dijkstra_batch(self._h, n, _p(tg), float(goal_dist_offset), _p(codes), _p(dist), _p(pred), _p(paths), cap, _p(lens))
        if rc == INTERNAL_ERROR:
            raise RuntimeError(f"mnav_replan_dijkstra_batch internal error: {self._err()}")
        rows = _PathRows(paths, lens, cap)
        lease.append(weakref.ref(rows))
        return dict(rc=rc, codes=codes, dist=dist, pred=pred, paths=rows, path_len=lens, stats=self.stats() if want_stats else self.timing(),
                    replan=self.replan_stats(n) if want_stats else None, warm=self.replan_warm_stats() if want_stats else None)

    def replan_dijkstra_each(self, targets=None, goal_dist_offset: float = 0.3, want_dist: bool = False, want_pred: bool = False,
                             path_cap: int | None = None, want_stats: bool = True):
        """replan_dijkstra plan by plan (mnav_replan_dijkstra_each, include/mnav.h): every plan of the last Dijkstra call is kept
        as it is, repaired or planned afresh, whatever its own field needs; the outputs are those of plan_dijkstra_batch on the
        resident map.  The same dict as replan_dijkstra plus `each` = replan_each_stats()."""
        n = int(self._L.mnav_replan_plans(self._h)) if targets is None else int(_u32(targets).shape[0])
        tg = None if targets is None else _u32(targets)
        V = self.V
        cap = int(path_cap if path_cap is not None else V)
        codes = np.empty(n, np.uint32)
        dist = np.empty((n, V), np.float32) if want_dist else None
        pred = np.empty((n, V), np.uint32) if want_pred else None
        paths, lease = self._lease_paths(n, cap)
        lens = np.zeros(n, np.uint32)
        rc = self._L.mnav_replan_dijkstra_each(self._h, n, _p(tg), float(goal_dist_offset), _p(codes), _p(dist), _p(pred), _p(paths), cap, _p(lens))
        if rc == INTERNAL_ERROR:
            raise RuntimeError(f"mnav_replan_dijkstra_each internal error: {self._err()}")
        rows = _PathRows(paths, lens, cap)
        lease.append(weakref.ref(rows))
        return dict(rc=rc, codes=codes, dist=dist, pred=pred, paths=rows, path_len=lens, stats=self.stats() if want_stats else self.timing(),
                    replan=self.replan_stats(n) if want_stats else None, each=self.replan_each_stats(n) if want_stats else None,
                    warm=self.replan_warm_stats() if want_stats else None)

    def replan_warm_stats(self) -> dict:
        """The warm repair of the last replan call of either kind (mnav_replan_warm_stats): plans repaired on the tile-batch
        engine from their rewound fields (0: none), its solve kernel, iterations, (tile, plan) pairs woken and slice words
        written by k_tb_warm, device milliseconds, and whether (and why) the call fell back to the tile rounds."""
        pl, kn, it, fb, lv = (C.c_uint32() for _ in range(5))
        wk, wd = C.c_uint64(), C.c_uint64()
        ms = np.zeros(3, np.float32)
        self._L.mnav_replan_warm_stats(self._h, C.byref(pl), C.byref(kn), C.byref(it), C.byref(wk), C.byref(wd), _p(ms), C.byref(fb), C.byref(lv))
        why = {0: None, 1: "more than 65535 repaired plans", 2: "the tile-batch engine could not be allocated"}.get(fb.value, str(fb.value))
        return dict(plans=pl.value, kernel=("k_tbv_solve" if kn.value == 1 else "k_tb_solve_q") if pl.value else None, iterations=it.value,
                    pairs_woken=wk.value, words=wd.value, ms_warm=float(ms[0]), ms_engine=float(ms[1]), ms_finalize=float(ms[2]),
                    fallback=fb.value, fallback_reason=why, live=bool(lv.value))

    def replan_each_stats(self, n: int = 0) -> dict:
        """The last replan_dijkstra_each call (mnav_replan_each_stats); n: its plan count, for the classes (0 KEPT, 1 REPAIRED,
        2 FRESH) and rewind levels in the caller's order."""
        r, wf, ll, tw, rd = (C.c_uint32() for _ in range(5))
        k, w = C.c_uint64(), C.c_uint64()
        fe = C.c_int32()
        counts = np.zeros(3, np.uint32)
        ms = np.zeros(5, np.float32)
        self._L.mnav_replan_each_stats(self._h, C.byref(r), C.byref(wf), C.byref(ll), None, None, _p(counts), C.byref(k), C.byref(w), C.byref(tw),
                                       C.byref(rd), C.byref(fe), _p(ms))
        cls = lv = None
        if n and int(counts.sum()) == n:
            cls, lv = np.zeros(n, np.uint8), np.zeros(n, np.float32)
            self._L.mnav_replan_each_stats(self._h, None, None, None, _p(cls), _p(lv), *([None] * 7))
        return dict(reason=r.value, whole_fresh=bool(wf.value), log_len=ll.value, classes=cls, levels=lv, kept_plans=int(counts[0]),
                    repaired_plans=int(counts[1]), fresh_plans=int(counts[2]), kept=k.value, rewound=w.value, tiles_woken=tw.value,
                    rounds=rd.value, fresh_engine=_engine_name(fe.value) if fe.value >= 0 else None, ms_classify=float(ms[0]),
                    ms_rewind=float(ms[1]), ms_rounds=float(ms[2]), ms_finalize=float(ms[3]), ms_fresh=float(ms[4]))

    def replan_stats(self, n: int = 0) -> dict:
        """The last replan_dijkstra call (mnav_replan_stats); n: its plan count, for the rewind levels (reason 0 only)."""
        r, ll, tw, rd = (C.c_uint32() for _ in range(4))
        k, w = C.c_uint64(), C.c_uint64()
        ms = [C.c_float() for _ in range(4)]
        self._L.mnav_replan_stats(self._h, C.byref(r), C.byref(ll), None, C.byref(k), C.byref(w), C.byref(tw), C.byref(rd), *[C.byref(x) for x in ms])
        lv = None
        if r.value == 0 and n:
            lv = np.zeros(n, np.float32)
            self._L.mnav_replan_stats(self._h, None, None, _p(lv), *([None] * 8))
        return dict(reason=r.value, log_len=ll.value, levels=lv, kept=k.value, rewound=w.value, tiles_woken=tw.value, rounds=rd.value,
                    ms_level=ms[0].value, ms_rewind=ms[1].value, ms_rounds=ms[2].value, ms_finalize=ms[3].value)

    @staticmethod
    def _fleet_robots(who, slots, start_vertex, start_pos, weights=None, depart=None, pace=None, key=None):
        """the per-robot arrays of a fleet call as its C signature takes them: (n, slots, start_vertex, start_pos, weights,
        depart, pace, key), None where None was given"""
        sl = _u32(slots).reshape(-1)
        n = int(sl.shape[0])
        sv, w, ky = (None if a is None else _u32(a).reshape(-1) for a in (start_vertex, weights, key))
        sp = None if start_pos is None else _f32(start_pos).reshape(-1, 3)
        dp, pc = (None if a is None else _f32(a).reshape(-1) for a in (depart, pace))
        if any(a is not None and a.shape[0] != n for a in (sv, sp if sv is None else None, w, ky, dp, pc)):
            raise ValueError(f"{who}: the per-robot arrays differ in length")
        return n, sl, sv, sp, w, dp, pc, ky

    def fleet_paths(self, slots, start_vertex=None, start_pos=None, ids_cap: int | None = None) -> dict:
        """Vertex paths of n robots out of the resident fields of the last Dijkstra call or replan (mnav_fleet_paths,
        include/mnav.h): robot i stands on start_vertex[i] (or on the vertex nearest to start_pos[i]) of plan slots[i].
        Returns dict(rc, codes, vertex, potential, path_len, offsets, ids, total): the ids of robot i are
        ids[offsets[i]:offsets[i + 1]], seed first.  Without ids_cap the call sizes the buffer itself (two calls); with it,
        rc = 1 and ids = None tell that `total` ids did not fit."""
        n, sl, sv, sp = self._fleet_robots("fleet_paths", slots, start_vertex, start_pos)[:4]
        codes, vtx, lens = (np.zeros(n, np.uint32) for _ in range(3))
        pot = np.zeros(n, np.float32)
        off = np.zeros(n + 1, np.uint64)
        total = C.c_uint64(0)

        def call(ids, cap):
            rc = self._L.mnav_fleet_paths(self._h, n, _p(sl), _p(sv), _p(sp), _p(codes), _p(vtx), _p(pot), _p(lens), _p(off), _p(ids), int(cap), C.byref(total))
            if rc < 0:
                raise RuntimeError(f"mnav_fleet_paths failed: {self._err()}")
            return rc

        ids = None
        if ids_cap is None:
            rc = call(None, 0) if n else 0
            ids = np.empty(int(total.value), np.uint32)
            if n and ids.size:
                rc = call(ids, ids.size)
            elif n:
                rc = 0
        else:
            ids = np.empty(int(ids_cap), np.uint32)
            rc = call(ids, ids.size) if n else 0
            ids = ids[: int(total.value)] if rc == 0 else None
        return dict(rc=rc, codes=codes, vertex=vtx, potential=pot, path_len=lens, offsets=off, ids=ids, total=int(total.value))

    def fleet_walks(self, slots, seed_pos, seed_faces, start_pos, start_faces=None, step_width: float = 0.4, inflation_layer: int = -1,
                    walk_cap: int = 4096, entries_cap: int | None = None) -> dict:
        """The back-tracking walk for n robots over the resident vector maps of the last plan call (mnav_fleet_walks,
        include/mnav.h): robot i walks from start_pos[i] to the seed end of plan slots[i].  seed_pos / seed_faces: one row
        per plan of that call.  Returns dict(rc, status, start_face, path_len, offsets, positions, faces, total), rows seed
        first: positions[offsets[i]:offsets[i + 1]].  Without entries_cap a first call without row buffers sizes
        them (the walks run twice; no buffer is larger than the result); with it, one call: rc = 1 and positions = None
        tell that `total` entries did not fit."""
        sl = _u32(slots).reshape(-1)
        n = int(sl.shape[0])
        sp, sf = _f32(seed_pos).reshape(-1, 3), _u32(seed_faces).reshape(-1)
        tp = _f32(start_pos).reshape(-1, 3)
        tf = None if start_faces is None else _u32(start_faces).reshape(-1)
        if sp.shape[0] != sf.shape[0] or tp.shape[0] != n or (tf is not None and tf.shape[0] != n):
            raise ValueError("fleet_walks: array lengths differ")
        st = np.zeros(n, np.int32)
        face0, lens = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        off = np.zeros(n + 1, np.uint64)
        total = C.c_uint64(0)

        def call(pos, face, cap):
            rc = self._L.mnav_fleet_walks(self._h, n, _p(sl), int(sf.shape[0]), _p(sp), _p(sf), _p(tp), _p(tf), float(step_width), int(inflation_layer),
                                          int(walk_cap), _p(st), _p(face0), _p(lens), _p(off), _p(pos), _p(face), int(cap), C.byref(total)) if n else 0
            if rc < 0:
                raise RuntimeError(f"mnav_fleet_walks failed: {self._err()}")
            return rc

        if entries_cap is None:
            call(None, None, 0)                                              # sizing only: statuses, lengths, total
            cap = int(total.value)
        else:
            cap = int(entries_cap)
        pos, face = np.empty((max(cap, 1), 3), np.float32), np.empty(max(cap, 1), np.uint32)
        rc = call(pos, face, cap)
        t = int(total.value)
        return dict(rc=rc, status=st, start_face=face0, path_len=lens, offsets=off, positions=pos[:t] if rc == 0 else None,
                    faces=face[:t] if rc == 0 else None, total=t)

    def upload_face_normals(self, face_normals):
        """MeshMap::faceNormals() for fleet_walk_plans (mnav_upload_face_normals): F x 3, resident until the next upload_mesh."""
        fn = _f32(face_normals).reshape(-1, 3)
        if self._L.mnav_upload_face_normals(self._h, int(fn.shape[0]), _p(fn)) != 0:
            raise RuntimeError(f"mnav_upload_face_normals failed: {self._err()}")

    def fleet_plans(self, slots, start_pos, goal_pos, start_vertex=None, poses_cap: int | None = None) -> dict:
        """makePlan's pose list and cost of n robots out of the resident fields of the last Dijkstra call or replan
        (mnav_fleet_plans, include/mnav.h): robot i stands at start_pos[i] on start_vertex[i] (None: the vertex nearest to
        it) of plan slots[i]; goal_pos: one row per plan of that call.  Returns dict(rc, codes, vertex, potential, path_len,
        offsets, cost, poses, total): the poses of robot i are poses[offsets[i]:offsets[i + 1]], 7 doubles each, robot side
        first.  Without poses_cap the call sizes the buffer itself (two calls); with it, rc = 1 and poses = None tell that
        `total` poses did not fit."""
        sl = _u32(slots).reshape(-1)
        n = int(sl.shape[0])
        sv = None if start_vertex is None else _u32(start_vertex).reshape(-1)
        sp = None if start_pos is None else _f32(start_pos).reshape(-1, 3)
        gp = None if goal_pos is None else _f32(goal_pos).reshape(-1, 3)
        if (sv is not None and sv.shape[0] != n) or (sp is not None and sp.shape[0] != n):
            raise ValueError("fleet_plans: the per-robot arrays differ in length")
        codes, vtx, lens = (np.zeros(n, np.uint32) for _ in range(3))
        pot = np.zeros(n, np.float32)
        off = np.zeros(n + 1, np.uint64)
        cost = np.zeros(n, np.float64)
        total = C.c_uint64(0)

        def call(poses, cap):
            rc = self._L.mnav_fleet_plans(self._h, n, _p(sl), _p(sv), _p(sp), 0 if gp is None else int(gp.shape[0]), _p(gp), _p(codes), _p(vtx), _p(pot), _p(lens),
                                          _p(off), _p(cost), _p(poses), int(cap), C.byref(total)) if n else 0
            if rc < 0:
                raise RuntimeError(f"mnav_fleet_plans failed: {self._err()}")
            return rc

        if poses_cap is None:
            rc = call(None, 0)
            poses = np.empty((int(total.value), 7), np.float64)
            rc = call(poses, poses.shape[0]) if poses.shape[0] else 0
        else:
            poses = np.empty((int(poses_cap), 7), np.float64)
            rc = call(poses, poses.shape[0])
            poses = poses[: int(total.value)] if rc == 0 else None
        return dict(rc=rc, codes=codes, vertex=vtx, potential=pot, path_len=lens, offsets=off, cost=cost, poses=poses, total=int(total.value))

    def fleet_walk_plans(self, slots, seed_pos, seed_faces, goal_pose, start_pos, start_faces=None, step_width: float = 0.4, inflation_layer: int = -1,
                         walk_cap: int = 4096, poses_cap: int | None = None) -> dict:
        """makePlan's pose list and cost over the walks of fleet_walks (mnav_fleet_walk_plans, include/mnav.h; face normals:
        upload_face_normals).  goal_pose: 7 doubles per plan, the last pose of every row.  Returns dict(rc, status,
        start_face, path_len, offsets, cost, poses, total), poses robot side first; sizing as in fleet_walks."""
        sl = _u32(slots).reshape(-1)
        n = int(sl.shape[0])
        sp, sf = _f32(seed_pos).reshape(-1, 3), _u32(seed_faces).reshape(-1)
        gp = None if goal_pose is None else np.ascontiguousarray(goal_pose, np.float64).reshape(-1, 7)
        tp = _f32(start_pos).reshape(-1, 3)
        tf = None if start_faces is None else _u32(start_faces).reshape(-1)
        if sp.shape[0] != sf.shape[0] or (gp is not None and gp.shape[0] != sf.shape[0]) or tp.shape[0] != n or (tf is not None and tf.shape[0] != n):
            raise ValueError("fleet_walk_plans: array lengths differ")
        st = np.zeros(n, np.int32)
        face0, lens = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        off = np.zeros(n + 1, np.uint64)
        cost = np.zeros(n, np.float64)
        total = C.c_uint64(0)

        def call(poses, cap):
            rc = self._L.mnav_fleet_walk_plans(self._h, n, _p(sl), int(sf.shape[0]), _p(sp), _p(sf), _p(gp), _p(tp), _p(tf), float(step_width), int(inflation_layer),
                                               int(walk_cap), _p(st), _p(face0), _p(lens), _p(off), _p(cost), _p(poses), int(cap), C.byref(total)) if n else 0
            if rc < 0:
                raise RuntimeError(f"mnav_fleet_walk_plans failed: {self._err()}")
            return rc

        if poses_cap is None:
            call(None, 0)                                                    # sizing only: statuses, lengths, costs, total
            cap = int(total.value)
        else:
            cap = int(poses_cap)
        poses = np.empty((max(cap, 1), 7), np.float64)
        rc = call(poses, cap)
        t = int(total.value)
        return dict(rc=rc, status=st, start_face=face0, path_len=lens, offsets=off, cost=cost, poses=poses[:t] if rc == 0 else None, total=t)

    def _dispatch_args(self, who, start_vertex, start_pos, slots, m):
        sv = None if start_vertex is None else _u32(start_vertex).reshape(-1)
        sp = None if start_pos is None else _f32(start_pos).reshape(-1, 3)
        if sv is None and sp is None:
            raise RuntimeError(f"{who}: neither start vertices nor start positions")
        n = int(sv.shape[0] if sv is not None else sp.shape[0])
        sl = None if slots is None else _u32(slots).reshape(-1)
        if sl is None and m is None:
            raise ValueError(f"{who}: slots=None needs m, the plan count of the recorded call")
        return n, sv, sp, int(sl.shape[0] if sl is not None else m), sl

    def fleet_costs(self, start_vertex=None, start_pos=None, slots=None, m: int | None = None, want_matrix: bool = True) -> dict:
        """The robot-to-goal matrix over the resident fields of the last Dijkstra call or replan (mnav_fleet_costs,
        include/mnav.h): entry (i, j) is what fleet_paths gives robot i on plan slots[j] (slots None: all m plans in order),
        without the walk of the chain.  Returns dict(codes (n x m uint8), potential (n x m), vertex, nearest_slot (column
        index per robot), nearest_robot (per column)); want_matrix=False leaves the matrix on the device (codes and
        potential are None)."""
        n, sv, sp, m, sl = self._dispatch_args("fleet_costs", start_vertex, start_pos, slots, m)
        codes = np.zeros((n, m), np.uint8) if want_matrix else None
        pot = np.zeros((n, m), np.float32) if want_matrix else None
        vtx, ns, nr = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(m, np.uint32)
        if self._L.mnav_fleet_costs(self._h, n, _p(sv), _p(sp), m, _p(sl), _p(codes), _p(pot), _p(vtx), _p(ns), _p(nr)) != 0:
            raise RuntimeError(f"mnav_fleet_costs failed: {self._err()}")
        return dict(codes=codes, potential=pot, vertex=vtx, nearest_slot=ns, nearest_robot=nr)

    def fleet_assign(self, start_vertex=None, start_pos=None, slots=None, m: int | None = None, quantum: float = 1e-3) -> dict:
        """The optimal one-to-one assignment of robots to goals (mnav_fleet_assign, include/mnav.h): maximum size, then the
        minimum sum of q = floor(potential / quantum + 0.5).  Returns dict(slot_of_robot (plan slot ids, NONE: unassigned),
        robot_of_slot (per column), potential, assigned, total_q, total_potential)."""
        n, sv, sp, m, sl = self._dispatch_args("fleet_assign", start_vertex, start_pos, slots, m)
        sor, ros, pot = np.zeros(n, np.uint32), np.zeros(m, np.uint32), np.zeros(n, np.float32)
        a, tq, tp = C.c_uint32(0), C.c_int64(0), C.c_double(0.0)
        if self._L.mnav_fleet_assign(self._h, n, _p(sv), _p(sp), m, _p(sl), float(quantum), _p(sor), _p(ros), _p(pot), C.byref(a), C.byref(tq), C.byref(tp)) != 0:
            raise RuntimeError(f"mnav_fleet_assign failed: {self._err()}")
        return dict(slot_of_robot=sor, robot_of_slot=ros, potential=pot, assigned=a.value, total_q=tq.value, total_potential=tp.value)

    def dispatch_stats(self) -> dict:
        """The last fleet_costs / fleet_assign that succeeded (mnav_dispatch_stats)."""
        pairs = (C.c_uint64 * 4)()
        f, r, tr, b = (C.c_uint64(0) for _ in range(4))
        a, ph, bi = (C.c_uint32(0) for _ in range(3))
        mc, ma, mt = (C.c_float(0) for _ in range(3))
        self._L.mnav_dispatch_stats(self._h, pairs, C.byref(f), C.byref(a), C.byref(ph), C.byref(r), C.byref(tr), C.byref(b), C.byref(bi), C.byref(mc), C.byref(ma),
                                    C.byref(mt))
        return dict(served=pairs[0], beyond_field=pairs[1], no_path=pairs[2], invalid=pairs[3], feasible=f.value, assigned=a.value, phases=ph.value,
                    rounds=r.value, tail_rounds=tr.value, bids=b.value, built_index=bi.value, ms_costs=mc.value, ms_assign=ma.value, ms_total=mt.value)

    # ---- fleet traffic (mnav_fleet_traffic, mnav_layer_traffic, mnav_map_traffic; include/mnav.h) ----
    def fleet_traffic(self, slots, start_vertex=None, start_pos=None, weights=None, accumulate: bool = False) -> dict:
        """Adds the paths of n robots to the context's per-vertex counts (mnav_fleet_traffic): robots as in fleet_paths,
        weights uint32 per robot (None: 1), accumulate False: the counts start from zero.  Returns dict(codes, vertex,
        potential) -- fleet_paths' values; the counts stay on the device (traffic_download, traffic_stats)."""
        n, sl, sv, sp, w = self._fleet_robots("fleet_traffic", slots, start_vertex, start_pos, weights)[:5]
        codes, vtx, pot = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float32)
        if self._L.mnav_fleet_traffic(self._h, n, _p(sl), _p(sv), _p(sp), _p(w), 1 if accumulate else 0, _p(codes), _p(vtx), _p(pot)) != 0:
            raise RuntimeError(f"mnav_fleet_traffic failed: {self._err()}")
        return dict(codes=codes, vertex=vtx, potential=pot)

    def traffic_download(self) -> np.ndarray:
        """the counts: uint32[V]"""
        c = np.zeros(max(self.V, 1), np.uint32)
        if self._L.mnav_traffic_download(self._h, _p(c)) != 0:
            raise RuntimeError(f"mnav_traffic_download failed: {self._err()}")
        return c[:self.V]

    def traffic_stats(self) -> dict:
        """The last fleet_traffic that succeeded (mnav_traffic_stats)."""
        a, t = C.c_uint64(), C.c_uint64()
        c, o, p, b = (C.c_uint32() for _ in range(4))
        mk, mt = C.c_float(), C.c_float()
        self._L.mnav_traffic_stats(self._h, C.byref(c), C.byref(a), C.byref(t), C.byref(o), C.byref(p), C.byref(b), C.byref(mk), C.byref(mt))
        return dict(contributing=c.value, adds=a.value, total_weight=t.value, occupied=o.value, peak=p.value, built_index=b.value,
                    ms_kernels=mk.value, ms_total=mt.value)

    def _traffic_layer(self, name: str, layer: int, free_count: int, gain: float, cap: float) -> dict:
        """mnav_layer_traffic or mnav_layer_timed_traffic: dict(changed)"""
        changed = np.empty(max(self.V, 1), np.uint32)
        nc = C.c_uint32()
        if getattr(self._L, name)(self._h, int(layer), int(free_count), float(gain), float(cap), _p(changed), C.byref(nc)) != 0:
            raise RuntimeError(f"{name} failed: {self._err()}")
        return dict(changed=changed[:nc.value].copy())

    def layer_traffic(self, layer: int, free_count: int = 0, gain: float = 1.0, cap: float = np.inf) -> dict:
        """the traffic layer from the counts as they stand (mnav_layer_traffic): dict(changed = ascending uint32 ids whose
        cost bits or lethal flag changed)"""
        return self._traffic_layer("mnav_layer_traffic", layer, free_count, gain, cap)

    def map_traffic(self, layer: int, free_count: int = 0, gain: float = 1.0, cap: float = np.inf) -> dict:
        """layer_traffic on an input node of the graph, then the propagation; same arguments"""
        return self._map_call("mnav_map_traffic", layer, int(free_count), float(gain), float(cap))

    # ---- timed fleet traffic (mnav_fleet_timed_traffic, mnav_layer_timed_traffic, mnav_map_timed_traffic; include/mnav.h) ----
    def fleet_timed_traffic(self, slots, start_vertex=None, start_pos=None, weights=None, depart=None, pace=None, key=None, windows: int = 64,
                            tau: float = 1.0, free_count: int = 0, accumulate: bool = False) -> dict:
        """Adds the paths of n robots to the context's cells per (vertex, time window) and reports who yields
        (mnav_fleet_timed_traffic): robots and weights as in fleet_traffic; per robot depart (float32, None: 0), pace (float32,
        None: 1) and key (uint32, None: the index; smaller wins).  Returns dict(codes, vertex, potential, conflict_hops,
        yield_hops, first_yield_vertex, first_yield_window, first_yield_time); the cells stay on the device
        (timed_traffic_download, timed_traffic_stats)."""
        n, sl, sv, sp, w, dp, pc, ky = self._fleet_robots("fleet_timed_traffic", slots, start_vertex, start_pos, weights, depart, pace, key)
        codes, vtx, conflict, yld, fv, fw = (np.zeros(n, np.uint32) for _ in range(6))
        pot, ft = np.zeros(n, np.float32), np.zeros(n, np.float32)
        if self._L.mnav_fleet_timed_traffic(self._h, n, _p(sl), _p(sv), _p(sp), _p(w), _p(dp), _p(pc), _p(ky), int(windows), float(tau), int(free_count),
                                            1 if accumulate else 0, _p(codes), _p(vtx), _p(pot), _p(conflict), _p(yld), _p(fv), _p(fw), _p(ft)) != 0:
            raise RuntimeError(f"mnav_fleet_timed_traffic failed: {self._err()}")
        return dict(codes=codes, vertex=vtx, potential=pot, conflict_hops=conflict, yield_hops=yld, first_yield_vertex=fv, first_yield_window=fw,
                    first_yield_time=ft)

    def timed_traffic_download(self, want_cells: bool = True) -> dict:
        """dict(peak uint32[V], window uint32[V], cells and holders uint32[V, windows] (None without want_cells)); windows =
        timed_traffic_stats()["windows"], 0 when no timed call has run since upload_mesh"""
        B = self.timed_traffic_stats()["windows"]
        peak, window = np.zeros(max(self.V, 1), np.uint32), np.zeros(max(self.V, 1), np.uint32)
        cells = np.zeros((self.V, B), np.uint32) if want_cells else None
        holders = np.zeros((self.V, B), np.uint32) if want_cells else None
        if self._L.mnav_timed_traffic_download(self._h, _p(peak), _p(window), _p(cells), _p(holders)) != 0:
            raise RuntimeError(f"mnav_timed_traffic_download failed: {self._err()}")
        return dict(peak=peak[:self.V], window=window[:self.V], cells=cells, holders=holders)

    def timed_traffic_stats(self) -> dict:
        """The last fleet_timed_traffic that succeeded (mnav_timed_traffic_stats)."""
        a, bh, t, oc, ov = (C.c_uint64() for _ in range(5))
        c, lg, y, w, b = (C.c_uint32() for _ in range(5))
        mk, mt = C.c_float(), C.c_float()
        self._L.mnav_timed_traffic_stats(self._h, C.byref(c), C.byref(a), C.byref(bh), C.byref(t), C.byref(oc), C.byref(ov), C.byref(lg), C.byref(y), C.byref(w),
                                         C.byref(b), C.byref(mk), C.byref(mt))
        return dict(contributing=c.value, adds=a.value, beyond_horizon=bh.value, total_weight=t.value, occupied_cells=oc.value, over_cells=ov.value,
                    largest_cell=lg.value, yielding=y.value, windows=w.value, built_index=b.value, ms_kernels=mk.value, ms_total=mt.value)

    def layer_timed_traffic(self, layer: int, free_count: int = 0, gain: float = 1.0, cap: float = np.inf) -> dict:
        """the traffic rule on the peaks as they stand (mnav_layer_timed_traffic): dict(changed = ascending uint32 ids whose
        cost bits or lethal flag changed)"""
        return self._traffic_layer("mnav_layer_timed_traffic", layer, free_count, gain, cap)

    def map_timed_traffic(self, layer: int, free_count: int = 0, gain: float = 1.0, cap: float = np.inf) -> dict:
        """layer_timed_traffic on an input node of the graph, then the propagation; same arguments"""
        return self._map_call("mnav_map_timed_traffic", layer, int(free_count), float(gain), float(cap))

    # ---- fleet schedule (mnav_fleet_schedule, mnav_schedule_stats; include/mnav.h) ----
    def fleet_schedule(self, slots, start_vertex=None, start_pos=None, weights=None, depart=None, pace=None, key=None, windows: int = 64,
                       tau: float = 1.0, capacity: int = 1, max_delay: int = 0, max_rounds: int = 0, flags: int = 0, accumulate: bool = False) -> dict:
        """A departure delay per robot, in whole windows, such that no (vertex, window) cell holds more than `capacity`
        (mnav_fleet_schedule): the robots and their arrays are those of fleet_timed_traffic; max_delay in 0 .. windows - 1,
        max_rounds 0: no limit, flags: SCHEDULE_SEED_FREE or 0.  Returns dict(codes, vertex, potential, status, delay,
        depart (the committed departure, +inf otherwise), round); the cells are the timed cells (timed_traffic_download,
        timed_traffic_stats), the call's own figures are schedule_stats()."""
        n, sl, sv, sp, w, dp, pc, ky = self._fleet_robots("fleet_schedule", slots, start_vertex, start_pos, weights, depart, pace, key)
        codes, vtx, status, delay, rnd = (np.zeros(n, np.uint32) for _ in range(5))
        pot, out = np.zeros(n, np.float32), np.zeros(n, np.float32)
        if self._L.mnav_fleet_schedule(self._h, n, _p(sl), _p(sv), _p(sp), _p(w), _p(dp), _p(pc), _p(ky), int(windows), float(tau), int(capacity), int(max_delay),
                                       int(max_rounds), int(flags), 1 if accumulate else 0, _p(codes), _p(vtx), _p(pot), _p(status), _p(delay), _p(out), _p(rnd)) != 0:
            raise RuntimeError(f"mnav_fleet_schedule failed: {self._err()}")
        return dict(codes=codes, vertex=vtx, potential=pot, status=status, delay=delay, depart=out, round=rnd)

    def schedule_stats(self) -> dict:
        """The last fleet_schedule that succeeded (mnav_schedule_stats)."""
        v = [C.c_uint32() for _ in range(7)]
        cl, cv = C.c_uint64(), C.c_uint64()
        b = C.c_uint32()
        mk, mt = C.c_float(), C.c_float()
        self._L.mnav_schedule_stats(self._h, *[C.byref(x) for x in v], C.byref(cl), C.byref(cv), C.byref(b), C.byref(mk), C.byref(mt))
        names = ("contributing", "committed", "no_slot", "open", "rounds", "delayed", "max_delay_used")
        return dict({k: x.value for k, x in zip(names, v)}, claims=cl.value, committed_visits=cv.value, built_index=b.value, ms_kernels=mk.value, ms_total=mt.value)

    def fleet_stats(self) -> dict:
        """The last fleet_paths / fleet_walks / fleet_plans / fleet_walk_plans call (mnav_fleet_stats; entries: ids, walk entries or poses)."""
        v = [C.c_uint32() for _ in range(4)]
        e = C.c_uint64()
        b, ch = C.c_uint32(), C.c_uint32()
        mk, mt = C.c_float(), C.c_float()
        self._L.mnav_fleet_stats(self._h, *[C.byref(x) for x in v], C.byref(e), C.byref(b), C.byref(ch), C.byref(mk), C.byref(mt))
        names = ("served", "beyond_field", "no_path", "invalid")
        return dict(**{k: x.value for k, x in zip(names, v)}, entries=e.value, built_index=b.value, chunks=ch.value, ms_kernels=mk.value, ms_total=mt.value)

    def plan_cvp_batch(self, seed_pos, seed_faces, target_faces, goal_dist_offset: float = 0.3, cost_limit: float = 1.0,
                       want_fields: bool = False, want_vecmap: bool = False):
        sp = _f32(seed_pos).reshape(-1, 3)
        sf, tf = _u32(seed_faces), _u32(target_faces)
        n, V = sf.shape[0], self.V
        codes = np.empty(n, np.uint32)
        dist = np.empty((n, V), np.float32) if want_fields else None
        pred = np.empty((n, V), np.uint32) if want_fields else None
        vm = np.empty((n, V, 3), np.float32) if want_vecmap else None
        rc = self._L.mnav_plan_cvp_batch(self._h, n, _p(sp), _p(sf), _p(tf), float(goal_dist_offset), float(cost_limit),
                                         _p(codes), _p(dist), _p(pred), _p(vm))
        if rc == INTERNAL_ERROR:
            raise RuntimeError(f"mnav_plan_cvp_batch internal error: {self._err()}")
        return dict(rc=rc, codes=codes, dist=dist, pred=pred, vecmap=vm, stats=self.stats())

    def locate(self, points, want_vertex: bool = True, want_face: bool = True, want_bary: bool = True, want_dist: bool = True) -> dict:
        """MeshMap::getNearestVertexHandle and searchContainingFace for an (n, 3) batch of positions (mnav_locate,
        include/mnav.h).  Returns dict(vertex, face, bary, dist): uint32 ids (NONE = 0xFFFFFFFF where there is none), the
        barycentric coordinates and the signed distance to the face's plane (zeros without a face); an output that was not
        asked for is None."""
        pts = _f32(points).reshape(-1, 3)
        n = int(pts.shape[0])
        vtx = np.empty(n, np.uint32) if want_vertex else None
        face = np.empty(n, np.uint32) if want_face else None
        bary = np.empty((n, 3), np.float32) if want_bary else None
        dist = np.empty(n, np.float32) if want_dist else None
        if self._L.mnav_locate(self._h, n, _p(pts) if n else None, _p(vtx), _p(face), _p(bary), _p(dist)) != 0:
            raise RuntimeError(f"mnav_locate failed: {self._err()}")
        return dict(vertex=vtx, face=face, bary=bary, dist=dist)

    def locate_stats(self) -> dict:
        b, mb, mq, c = C.c_uint32(), C.c_float(), C.c_float(), C.c_uint64()
        self._L.mnav_locate_stats(self._h, C.byref(b), C.byref(mb), C.byref(mq), C.byref(c))
        return dict(built=b.value, ms_build=mb.value, ms_query=mq.value, candidates=c.value)

    def follow(self, pos, direction, up, face_in, slots, seed_faces=None, config: FollowConfig | None = None, outputs=None) -> FollowOut:
        """One controller tick of mesh_controller::MeshController for n robots over the resident vector maps of the last
        plan call (mnav_follow_batch, include/mnav.h).  pos / direction / up: (n, 3); face_in: the face of the last tick
        or NONE; slots: the plan each robot follows; seed_faces: that plan's seed face per robot (optional).  `outputs`:
        the names of the FollowOut fields to fetch (default: all)."""
        p, d, u = (_f32(a).reshape(-1, 3) for a in (pos, direction, up))
        fi, sl = _u32(face_in).reshape(-1), _u32(slots).reshape(-1)
        n = int(p.shape[0])
        if not (d.shape[0] == u.shape[0] == fi.shape[0] == sl.shape[0] == n):
            raise ValueError("follow: the per-robot arrays differ in length")
        sf = None if seed_faces is None else _u32(seed_faces).reshape(-1)
        if sf is not None and sf.shape[0] != n:
            raise ValueError("follow: seed_faces needs one entry per robot")
        cfg = config if config is not None else FollowConfig()
        want = set(FollowOut.__dataclass_fields__) if outputs is None else set(outputs)
        shapes = dict(code=((n,), np.int32), face=((n,), np.uint32), bary=((n, 3), np.float32), pos=((n, 3), np.float32),
                      mesh_dir=((n, 3), np.float32), cost=((n,), np.float32), cmd=((n, 2), np.float64), how=((n,), np.int32))
        o = {k: (np.zeros(*shapes[k]) if k in want else None) for k in shapes}
        rc = self._L.mnav_follow_batch(self._h, n, _p(p), _p(d), _p(u), _p(fi), _p(sl), _p(sf), C.byref(cfg), _p(o["code"]), _p(o["face"]),
                                       _p(o["bary"]), _p(o["pos"]), _p(o["mesh_dir"]), _p(o["cost"]), _p(o["cmd"]), _p(o["how"]))
        if rc != 0:
            raise RuntimeError(f"mnav_follow_batch failed: {self._err()}")
        return FollowOut(**o)

    def follow_stats(self) -> dict:
        v = [C.c_uint32() for _ in range(6)]
        mk, mt = C.c_float(), C.c_float()
        self._L.mnav_follow_stats(self._h, *[C.byref(x) for x in v], C.byref(mk), C.byref(mt))
        names = ("stayed", "neighbour", "global", "lost", "no_field", "built_index")
        return dict(**{k: x.value for k, x in zip(names, v)}, ms_kernels=mk.value, ms_total=mt.value)

    def _rollout(self, name, fn, pos, direction, up, face_in, slots, ids, ids_error, goal_pos, goal_dir, config, rollout, outputs,
                 more=(), extra=(), with_extra=False):
        """What rollout() and fleet_rollout() share: the conversions, the length checks (`name` prefixes their ValueErrors),
        the output arrays and the call of the C function `fn`, whose arguments are mnav_follow_rollout's with the caller's
        additions in between.  ids: the optional uint32 per-robot inputs, seed_faces first (the others follow the rollout
        config in the call), ids_error: what to say when one has another length; more: ready arguments after those; extra:
        the dtypes by name of per-robot outputs that follow the trace in the call, allocated with_extra, else NULL.
        Returns the outputs by name and the return code."""
        p, d, u = (_f32(a).reshape(-1, 3) for a in (pos, direction, up))
        fi, sl = _u32(face_in).reshape(-1), _u32(slots).reshape(-1)
        n = int(p.shape[0])
        if not (d.shape[0] == u.shape[0] == fi.shape[0] == sl.shape[0] == n):
            raise ValueError(f"{name}: the per-robot arrays differ in length")
        ids = [None if a is None else _u32(a).reshape(-1) for a in ids]
        if any(a is not None and a.shape[0] != n for a in ids):
            raise ValueError(f"{name}: {ids_error}")
        gp = None if goal_pos is None else _f32(goal_pos).reshape(-1, 3)
        gd = None if goal_dir is None else _f32(goal_dir).reshape(-1, 3)
        if any(g is not None and g.shape[0] != n for g in (gp, gd)):
            raise ValueError(f"{name}: goal_pos / goal_dir need one row per robot")
        cfg = config if config is not None else FollowConfig()
        ro = rollout if rollout is not None else RolloutConfig()
        rows = int(ro.ticks) // int(ro.trace_stride) if ro.trace_stride else 0
        shapes = dict(status=((n,), np.int32), ticks=((n,), np.uint32), pos=((n, 3), np.float32), dir=((n, 3), np.float32), face=((n,), np.uint32),
                      travel=((n,), np.float64), cost_integral=((n,), np.float64), min_goal_dist=((n,), np.float32))
        state = [*shapes, "trace"]
        if with_extra:
            shapes.update({k: ((n,), t) for k, t in extra.items()})
        want = set(shapes) if outputs is None else set(outputs)
        o = {k: (np.zeros(*shapes[k]) if k in want else None) for k in shapes}
        o["trace"] = np.zeros((n, rows, 3), np.float32) if ro.trace_stride else None
        rc = fn(self._h, n, _p(p), _p(d), _p(u), _p(fi), _p(sl), _p(ids[0]), _p(gp), _p(gd), C.byref(cfg), C.byref(ro), *[_p(a) for a in ids[1:]], *more,
                *[_p(o[k]) for k in state], *[_p(o.get(k)) for k in extra])
        if rc < 0:
            raise RuntimeError(f"{fn.__name__} failed: {self._err()}")
        return o, rc

    def rollout(self, pos, direction, up, face_in, slots, seed_faces=None, goal_pos=None, goal_dir=None, config: FollowConfig | None = None,
                rollout: RolloutConfig | None = None, outputs=None) -> RolloutOut:
        """`rollout.ticks` controller ticks of n robots over the resident vector maps of the last plan call, the robots'
        state resident and the loop on the device (mnav_follow_rollout, include/mnav.h).  The per-robot arrays are those
        of follow(); goal_pos / goal_dir: (n, 3) each, both or neither.  `outputs`: the names of the RolloutOut fields to
        fetch (default: all; the trace whenever rollout.trace_stride is set)."""
        o, rc = self._rollout("rollout", self._L.mnav_follow_rollout, pos, direction, up, face_in, slots, [seed_faces], "seed_faces needs one entry per robot",
                              goal_pos, goal_dir, config, rollout, outputs)
        return RolloutOut(**o, cancelled=rc == 1)

    def rollout_stats(self) -> dict:
        sc = (C.c_uint32 * 4)()
        v = [C.c_uint64() for _ in range(4)]
        b, mk, mt = C.c_uint32(), C.c_float(), C.c_float()
        self._L.mnav_rollout_stats(self._h, C.byref(sc), *[C.byref(x) for x in v], C.byref(b), C.byref(mk), C.byref(mt))
        names = ("robot_ticks", "stayed", "neighbour", "global")
        return dict(running=sc[0], reached=sc[1], out_of_map=sc[2], no_field=sc[3], **{k: x.value for k, x in zip(names, v)},
                    built_index=b.value, ms_kernels=mk.value, ms_total=mt.value)

    def follow_sample(self, pos, direction, up, face_in, slots, candidates, seed_faces=None, goal_pos=None, goal_dir=None, config: FollowConfig | None = None,
                      rollout: RolloutConfig | None = None, sample: SampleConfig | None = None, outputs=None) -> dict:
        """K candidate controls per robot, rolled out for rollout.ticks ticks, scored on the resident potential and picked
        per robot on the device (mnav_follow_sample, include/mnav.h).  The per-robot arrays are those of rollout();
        candidates: (K, 4) doubles, lin_gain, lin_bias, ang_gain, ang_bias.  Returns a dict: the picks best_k (NONE: no
        feasible row), best_score, best_cmd (n, 2), n_feasible; the per-row outputs SAMPLE_ROWS, each (n, K) (pos: (n, K, 3)),
        or None where `outputs` (names; default: all) leaves one out; and `cancelled`."""
        p, d, u = (_f32(a).reshape(-1, 3) for a in (pos, direction, up))
        fi, sl = _u32(face_in).reshape(-1), _u32(slots).reshape(-1)
        n = int(p.shape[0])
        if not (d.shape[0] == u.shape[0] == fi.shape[0] == sl.shape[0] == n):
            raise ValueError("follow_sample: the per-robot arrays differ in length")
        sf = None if seed_faces is None else _u32(seed_faces).reshape(-1)
        if sf is not None and sf.shape[0] != n:
            raise ValueError("follow_sample: seed_faces needs one entry per robot")
        gp = None if goal_pos is None else _f32(goal_pos).reshape(-1, 3)
        gd = None if goal_dir is None else _f32(goal_dir).reshape(-1, 3)
        if any(g is not None and g.shape[0] != n for g in (gp, gd)):
            raise ValueError("follow_sample: goal_pos / goal_dir need one row per robot")
        tab = np.ascontiguousarray(candidates, np.float64).reshape(-1, 4)
        K = int(tab.shape[0])
        cfg = config if config is not None else FollowConfig()
        ro = rollout if rollout is not None else RolloutConfig()
        sa = sample if sample is not None else SampleConfig()
        shapes = dict(best_k=((n,), np.uint32), best_score=((n,), np.float64), best_cmd=((n, 2), np.float64), n_feasible=((n,), np.uint32),
                      status=((n, K), np.int32), ticks=((n, K), np.uint32), score=((n, K), np.float64), potential=((n, K), np.float32),
                      lethal=((n, K), np.uint8), cost_integral=((n, K), np.float64), travel=((n, K), np.float64), pos=((n, K, 3), np.float32))
        want = set(shapes) if outputs is None else set(outputs)
        o = {k: (np.zeros(*shapes[k]) if k in want else None) for k in shapes}
        rc = self._L.mnav_follow_sample(self._h, n, _p(p), _p(d), _p(u), _p(fi), _p(sl), _p(sf), _p(gp), _p(gd), C.byref(cfg), C.byref(ro), K, _p(tab) if K else None,
                                        C.byref(sa), *[_p(o[k]) for k in SAMPLE_PICKS + SAMPLE_ROWS])
        if rc < 0:
            raise RuntimeError(f"mnav_follow_sample failed: {self._err()}")
        return dict(o, cancelled=rc == 1)

    def sample_stats(self) -> dict:
        sc = (C.c_uint32 * 4)()
        c = [C.c_uint32() for _ in range(3)]
        v = [C.c_uint64() for _ in range(4)]
        b = C.c_uint32()
        ms = [C.c_float() for _ in range(4)]
        self._L.mnav_sample_stats(self._h, C.byref(sc), *[C.byref(x) for x in c], *[C.byref(x) for x in v], C.byref(b), *[C.byref(x) for x in ms])
        return dict(running=sc[0], reached=sc[1], out_of_map=sc[2], no_field=sc[3],
                    **{k: x.value for k, x in zip(("lethal_rows", "feasible_rows", "robots_without_pick"), c)},
                    **{k: x.value for k, x in zip(("row_ticks", "stayed", "neighbour", "global"), v)}, built_index=b.value,
                    **{k: x.value for k, x in zip(("ms_expand", "ms_pick", "ms_kernels", "ms_total"), ms)})

    def fleet_rollout(self, pos, direction, up, face_in, slots, seed_faces=None, goal_pos=None, goal_dir=None, config: FollowConfig | None = None,
                      rollout: RolloutConfig | None = None, start_tick=None, separation: SeparationConfig | None = None, outputs=None) -> FleetRolloutOut:
        """rollout() with a departure tick per robot (start_tick: n entries or None) and, with `separation`, a check between
        the robots on the device after every separation.check_stride-th tick (mnav_fleet_rollout, include/mnav.h).
        `outputs`: the names of the FleetRolloutOut fields to fetch (default: all; the separation outputs only with
        `separation`)."""
        o, rc = self._rollout("fleet_rollout", self._L.mnav_fleet_rollout, pos, direction, up, face_in, slots, [seed_faces, start_tick],
                              "seed_faces / start_tick need one entry per robot", goal_pos, goal_dir, config, rollout, outputs,
                              more=[None if separation is None else C.byref(separation)],
                              extra={k: np.float32 if k == "min_sep2" else np.uint32 for k in SEPARATION_OUTPUTS}, with_extra=separation is not None)
        return FleetRolloutOut(**o, cancelled=rc == 1, skipped=rc == 2)

    def fleet_rollout_stats(self) -> dict:
        sc, pair = (C.c_uint32 * 4)(), (C.c_uint32 * 2)()
        u64, u32, f32 = C.c_uint64, C.c_uint32, C.c_float
        spec = [("robot_ticks", u64), ("stayed", u64), ("neighbour", u64), ("global", u64), ("built_index", u32), ("checks_run", u32), ("checks_skipped", u32),
                ("first_skipped_tick", u32), ("robots_near", u32), ("near_pairs", u64), ("max_pairs", u64), ("max_pairs_tick", u32), ("min_sep2", f32),
                ("min_pair", None), ("tests", u64), ("max_cell", u32), ("ms_separation", f32), ("ms_kernels", f32), ("ms_total", f32)]
        v = {k: (pair if t is None else t()) for k, t in spec}
        self._L.mnav_fleet_rollout_stats(self._h, C.byref(sc), *[C.byref(v[k]) for k, _ in spec])
        out = dict(running=sc[0], reached=sc[1], out_of_map=sc[2], no_field=sc[3])
        out.update({k: ((pair[0], pair[1]) if t is None else v[k].value) for k, t in spec})
        return out

    def fleet_rollout_yield(self, pos, direction, up, face_in, slots, seed_faces=None, goal_pos=None, goal_dir=None, config: FollowConfig | None = None,
                            rollout: RolloutConfig | None = None, start_tick=None, separation: SeparationConfig | None = None,
                            yield_config: YieldConfig | None = None, priority=None, hold_in=None, outputs=None, _rings=None) -> FleetYieldOut:
        """fleet_rollout() in which a robot that has to yield to a partner ahead of it has no tick until the next check
        (mnav_fleet_rollout_yield, include/mnav.h).  yield_config None: fleet_rollout() bit for bit.  priority: n uint32 or
        None (the index decides); hold_in: n bytes or None, the `hold` of the call this one resumes.  `outputs`: the names of
        the FleetYieldOut fields to fetch (default: all; the yield outputs only with `yield_config`)."""
        n = int(_f32(pos).reshape(-1, 3).shape[0])
        prio = None if priority is None else _u32(priority).reshape(-1)
        hin = None if hold_in is None else np.ascontiguousarray(hold_in, np.uint8).reshape(-1)
        if any(a is not None and a.shape[0] != n for a in (prio, hin)):
            raise ValueError("fleet_rollout_yield: priority / hold_in need one entry per robot")
        want = set(YIELD_OUTPUTS) if outputs is None else set(outputs) & set(YIELD_OUTPUTS)
        y = {k: (np.zeros(n, np.uint8 if k == "hold" else np.uint32) if yield_config is not None and k in want else None) for k in YIELD_OUTPUTS}
        tail = [None if yield_config is None else C.byref(yield_config), _p(prio), _p(hin), *[_p(y[k]) for k in YIELD_OUTPUTS]]

        if _rings is None:
            def fn(*args):
                return self._L.mnav_fleet_rollout_yield(*args, *tail)

            fn.__name__ = "mnav_fleet_rollout_yield"
        else:                                                             # fleet_rollout_rings(): the same call with the ring group behind
            def fn(*args):
                return self._L.mnav_fleet_rollout_rings(*args, *tail, *_rings)

            fn.__name__ = "mnav_fleet_rollout_rings"
        o, rc = self._rollout("fleet_rollout_yield", fn, pos, direction, up, face_in, slots, [seed_faces, start_tick],
                              "seed_faces / start_tick need one entry per robot", goal_pos, goal_dir, config, rollout,
                              None if outputs is None else [k for k in outputs if k not in YIELD_OUTPUTS + RING_OUTPUTS],
                              more=[None if separation is None else C.byref(separation)],
                              extra={k: np.float32 if k == "min_sep2" else np.uint32 for k in SEPARATION_OUTPUTS}, with_extra=separation is not None)
        return FleetYieldOut(**o, **y, cancelled=rc == 1, skipped=rc == 2)

    def fleet_yield_stats(self) -> dict:
        u64, u32, f32 = C.c_uint64, C.c_uint32, C.c_float
        spec = [("robots_held", u32), ("held_ticks", u64), ("max_held", u32), ("max_held_tick", u32), ("held_last", u32), ("checks_run", u32), ("checks_skipped", u32),
                ("first_skipped_tick", u32), ("ms_pair", f32), ("ms_separation", f32),
                ("ms_kernels", f32), ("ms_total", f32)]
        v = {k: t() for k, t in spec}
        self._L.mnav_fleet_yield_stats(self._h, *[C.byref(v[k]) for k, _ in spec])
        return {k: v[k].value for k, _ in spec}

    def fleet_rollout_rings(self, pos, direction, up, face_in, slots, seed_faces=None, goal_pos=None, goal_dir=None, config: FollowConfig | None = None,
                            rollout: RolloutConfig | None = None, start_tick=None, separation: SeparationConfig | None = None,
                            yield_config: YieldConfig | None = None, priority=None, hold_in=None, ring_config: RingConfig | None = None, outputs=None) -> FleetRingOut:
        """fleet_rollout_yield() with a wait-for analysis behind every check: the class of every held robot (queued, parked,
        tail or member of a ring), its anchor, and with RING_RELEASE the release of every ring's leader
        (mnav_fleet_rollout_rings, include/mnav.h).  ring_config None: fleet_rollout_yield() bit for bit.  `outputs`: the names
        of the FleetRingOut fields to fetch (default: all; the ring outputs only with `ring_config`)."""
        n = int(_f32(pos).reshape(-1, 3).shape[0])
        want = set(RING_OUTPUTS) if outputs is None else set(outputs) & set(RING_OUTPUTS)
        r = {k: (np.full(n, 0xFFFFFFFF if k == "wait_anchor" else 0, np.uint8 if k == "wait_class" else np.uint32) if ring_config is not None and k in want else None)
             for k in RING_OUTPUTS}
        y = self.fleet_rollout_yield(pos, direction, up, face_in, slots, seed_faces, goal_pos, goal_dir, config, rollout, start_tick, separation, yield_config, priority,
                                     hold_in, outputs, _rings=[None if ring_config is None else C.byref(ring_config), *[_p(r[k]) for k in RING_OUTPUTS]])
        return FleetRingOut(**{k: getattr(y, k) for k in FleetYieldOut.__dataclass_fields__}, **r)

    def fleet_ring_stats(self) -> dict:
        u64, u32, f32 = C.c_uint64, C.c_uint32, C.c_float
        spec = [("robots_ring", u32), ("rings", u64), ("max_rings", u32), ("max_rings_tick", u32), ("releases", u64), ("members_last", u32), ("tails_last", u32),
                ("parked_last", u32), ("queued_last", u32), ("rings_last", u32), ("checks_run", u32), ("checks_skipped", u32), ("first_skipped_tick", u32),
                ("ms_ring", f32), ("ms_separation", f32), ("ms_kernels", f32), ("ms_total", f32)]
        v = {k: t() for k, t in spec}
        self._L.mnav_fleet_ring_stats(self._h, *[C.byref(v[k]) for k, _ in spec])
        return {k: v[k].value for k, _ in spec}

    def plan_dijkstra_batch_at(self, goal_pos, start_pos, goal_dist_offset: float = 0.3, cost_limit: float = 1.0,
                               want_fields: bool = False, path_cap: int | None = None, want_stats: bool = True):
        """plan_dijkstra_batch from positions: goal -> seed vertex, start -> target vertex on the device (`seeds`, `targets`
        in the result)."""
        gp, sp = _f32(goal_pos).reshape(-1, 3), _f32(start_pos).reshape(-1, 3)
        n, V = int(gp.shape[0]), self.V
        if sp.shape[0] != n:
            raise ValueError("goal_pos and start_pos differ in length")
        cap = int(path_cap if path_cap is not None else V)
        codes = np.empty(n, np.uint32)
        seeds, targets = np.empty(n, np.uint32), np.empty(n, np.uint32)
        dist = np.empty((n, V), np.float32) if want_fields else None
        pred = np.empty((n, V), np.uint32) if want_fields else None
        paths, lease = self._lease_paths(n, cap)
        lens = np.zeros(n, np.uint32)
        rc = self._L.mnav_plan_dijkstra_batch_at(self._h, n, _p(gp), _p(sp), float(goal_dist_offset), float(cost_limit), _p(codes),
                                                 _p(seeds), _p(targets), _p(dist), _p(pred), _p(paths), cap, _p(lens))
        if rc == INTERNAL_ERROR:
            raise RuntimeError(f"mnav_plan_dijkstra_batch_at internal error: {self._err()}")
        rows = _PathRows(paths, lens, cap)
        lease.append(weakref.ref(rows))
        return dict(rc=rc, codes=codes, seeds=seeds, targets=targets, dist=dist, pred=pred, paths=rows, path_len=lens,
                    stats=self.stats() if want_stats else self.timing())

    def plan_cvp_batch_at(self, goal_pos, start_pos, goal_dist_offset: float = 0.3, cost_limit: float = 1.0,
                          want_fields: bool = False, want_vecmap: bool = False):
        """plan_cvp_batch from positions: the wave seed is the goal position as given, the two faces are the containing
        faces found on the device (`seed_faces`, `target_faces` in the result)."""
        gp, sp = _f32(goal_pos).reshape(-1, 3), _f32(start_pos).reshape(-1, 3)
        n, V = int(gp.shape[0]), self.V
        if sp.shape[0] != n:
            raise ValueError("goal_pos and start_pos differ in length")
        codes = np.empty(n, np.uint32)
        sf, tf = np.empty(n, np.uint32), np.empty(n, np.uint32)
        dist = np.empty((n, V), np.float32) if want_fields else None
        pred = np.empty((n, V), np.uint32) if want_fields else None
        vm = np.empty((n, V, 3), np.float32) if want_vecmap else None
        rc = self._L.mnav_plan_cvp_batch_at(self._h, n, _p(gp), _p(sp), float(goal_dist_offset), float(cost_limit), _p(codes), _p(sf), _p(tf),
                                            _p(dist), _p(pred), _p(vm))
        if rc == INTERNAL_ERROR:
            raise RuntimeError(f"mnav_plan_cvp_batch_at internal error: {self._err()}")
        return dict(rc=rc, codes=codes, seed_faces=sf, target_faces=tf, dist=dist, pred=pred, vecmap=vm, stats=self.stats())

    def plan_cvp(self, seed_pos, seed_face: int, target_face: int, goal_dist_offset: float = 0.3,
                 cost_limit: float = 1.0, want_fields: bool = True, want_vecmap: bool = True) -> CvpOut:
        V = self.V
        sp = _f32(seed_pos)
        dist = np.empty(V, np.float32) if want_fields else None
        pred = np.empty(V, np.uint32) if want_fields else None
        dirn = np.empty(V, np.float32) if want_fields else None
        cutf = np.empty(V, np.uint32) if want_fields else None
        vm = np.empty((V, 3), np.float32) if want_vecmap else None
        code = self._L.mnav_plan_cvp(self._h, _p(sp), int(seed_face) & 0xFFFFFFFF, int(target_face) & 0xFFFFFFFF,
                                     float(goal_dist_offset), float(cost_limit), _p(dist), _p(pred), _p(dirn),
                                     _p(cutf), _p(vm))
        if code == INTERNAL_ERROR:
            raise RuntimeError(f"mnav_plan_cvp internal error: {self._err()}")
        return CvpOut(code, dist, pred, dirn, cutf, vm, self.stats())
