"""Python host binding of the C ABI (include/mrs_tg.h) -- ctypes only, no numerics here.

The library is the product; this module only marshals buffers.  There is no CPU fallback: if
libmrs_tg.so is missing or no HIP device is usable, the calls raise.

Two ways in, mirroring the ABI:
  * Context.solve_batch(batch, seg_times, ...)  host numpy arrays in / out (the nodelet-style call,
    /root/reference/src/mrs_trajectory_generation.cpp:1046-1169 for a whole batch);
  * Plan(...)  analysis once, then device-resident torch tensors, asynchronous on torch's current
    stream (what bench.py times).
"""
import ctypes as C
import os

import numpy as np

from .problem import Batch, N_COEFF, N_DIM

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MRS_TG_LIB_PATH") or os.path.join(_HERE, "libmrs_tg.so")   # (the override: experiment builds)

TIME_ALLOC_NONE = -1
TIME_ALLOC_SQUARED_TIME = 0
TIME_ALLOC_RICHTER_TIME = 1
TIME_ALLOC_MELLINGER = 2
TIME_ALLOC_SQUARED_TIME_AND_CONSTRAINTS = 3
TIME_ALLOC_RICHTER_TIME_AND_CONSTRAINTS = 4
FLAG_FUSED_ASSEMBLY = 1        # the default since ABI 2
FLAG_MATERIALIZED_BLOCKS = 2   # assembly kernel + solve from the materialised H / A^-1 blocks
FLAG_GENERAL_PATTERNS = 16     # vertices without a position constraint may occur (general 5 x 5 route, every mode)
FLAG_CAREFUL_COST = 8          # Mellinger mode: re-run the paths whose fast cost evaluation failed its guard with primal costs
FLAG_SHARED_DEVICE = 4         # hint: several batches are in flight on this device (results unaffected)
FLAG_POSITIONS_ARE_WAYPOINTS = 32   # every vertex's position constraint is its waypoint (checked at bind time): read the compact array
FLAG_REFERENCE_STATUS = 128         # Mellinger: the outer loop's own code, no runaway rule (MRS_TG_FLAG_REFERENCE_STATUS)
FLAG_CONSTRAINED_SLOTS = 64         # hint: interior vertices may hold constrained derivative slots (stop_at) under min-snap
FLAG_REFINE = 256                   # refine the final solve's coefficients and cost (double-double residual; MRS_TG_FLAG_REFINE)

STATUS_ROUNDOFF_LIMITED = -4   # MRS_TG_STATUS_ROUNDOFF_LIMITED: the feasibility scaling ran away (include/mrs_tg.h)
RUNAWAY_TIME_FACTOR = 25.0     # MRS_TG_RUNAWAY_TIME_FACTOR

# mrs_tg_find_trajectory_info: which of findTrajectory's gates discarded the trajectory (MRS_TG_FIND_*)
FIND_ACCEPTED, FIND_REJECTED_CODE, FIND_REJECTED_TOO_LONG, FIND_REJECTED_TOO_SHORT = 0, 1, 2, 3

STATE_ORDERS = 5   # derivative orders 0..4 per sample of Plan.sample_states (MRS_TG_STATE_ORDERS)
KERNEL_ASSEMBLE, KERNEL_SOLVE_LINEAR, KERNEL_NONLINEAR, KERNEL_VJP, KERNEL_MAXIMA_VJP = 0, 1, 2, 3, 4
KERNEL_SAMPLE_VJP = 5
KERNEL_EVALUATE, KERNEL_EVALUATE_VJP = 6, 7
KERNEL_DEVIATION, KERNEL_DEVIATION_VJP = 8, 9
KERNEL_ESTIMATE, KERNEL_ESTIMATE_VJP = 10, 11
KERNEL_PASSAGE, KERNEL_PASSAGE_VJP = 12, 13
KERNEL_BACA, KERNEL_BACA_VJP, KERNEL_LENGTH_GATE = 14, 15, 16
KERNEL_UNWRAP_HEADINGS, KERNEL_FALLBACK_SAMPLE, KERNEL_FALLBACK_SAMPLE_VJP = 17, 18, 19
KERNEL_PREPROCESS_PATH, KERNEL_INSERT_MIDPOINTS, KERNEL_PATH_EDIT_VJP = 20, 21, 22
KERNEL_TRAVEL_HEADING, KERNEL_TRAVEL_HEADING_VJP = 23, 24
KERNEL_INITIAL_CONDITION, KERNEL_PREPEND_INITIAL_CONDITION, KERNEL_SPLICE_PREDICTION = 25, 26, 27
KERNEL_SPLICE_PREDICTION_VJP, KERNEL_INITIAL_CONDITION_VJP, KERNEL_PREPEND_INITIAL_CONDITION_VJP = 28, 29, 30
KERNEL_REQUEST_VERTICES, KERNEL_REQUEST_VERTICES_VJP, KERNEL_REQUEST_LIMITS, KERNEL_REQUEST_LIMITS_VJP = 31, 32, 33, 34
KERNEL_MUTUAL_CLEARANCE, KERNEL_MUTUAL_CLEARANCE_VJP = 35, 36
KERNEL_OBSTACLE_CLEARANCE, KERNEL_OBSTACLE_CLEARANCE_VJP = 37, 38
KERNEL_FIELD_CLEARANCE, KERNEL_FIELD_CLEARANCE_VJP = 39, 40
KERNEL_FIELD_FROM_OCCUPANCY = 41   # edt_x_kernel's start to edt_z_kernel's end


class MrsTgError(RuntimeError):
    pass


class Options(C.Structure):
    _fields_ = [("derivative_to_optimize", C.c_int32), ("time_alloc_method", C.c_int32),
                ("estimate_times", C.c_int32), ("max_iterations", C.c_int32),
                ("f_rel", C.c_double), ("f_abs", C.c_double), ("x_rel", C.c_double), ("x_abs", C.c_double),
                ("sampling_dt", C.c_double), ("sample_capacity", C.c_int32), ("flags", C.c_int32),
                ("time_penalty", C.c_double), ("soft_constraint_weight", C.c_double),
                ("use_soft_constraints", C.c_int32), ("reserved_", C.c_int32), ("initial_stepsize_rel", C.c_double),
                ("max_time_s", C.c_double),
                ("max_trajectory_len_factor", C.c_double), ("min_trajectory_len_factor", C.c_double)]   # (ABI 5)


class PolicyOptions(C.Structure):
    _fields_ = [("solver", Options), ("check_deviation_enabled", C.c_int32), ("max_deviation", C.c_double),
                ("max_deviation_iterations", C.c_int32), ("max_deviation_first_segment", C.c_int32),
                ("min_waypoint_distance", C.c_double), ("path_straightener_enabled", C.c_int32),
                ("path_straightener_max_deviation", C.c_double), ("path_straightener_max_hdg_deviation", C.c_double),
                ("max_trajectory_len_factor", C.c_double), ("min_trajectory_len_factor", C.c_double),
                ("fallback_sampling", C.c_int32), ("fallback_speed_factor", C.c_double),
                ("fallback_accel_factor", C.c_double), ("fallback_stopping_time", C.c_double),
                ("override_heading_atan2", C.c_int32), ("reserved_", C.c_int32), ("max_execution_time_s", C.c_double)]


class Waypoint(C.Structure):
    _fields_ = [("coords", C.c_double * 4), ("stop_at", C.c_uint8)]


class InitialState(C.Structure):
    _fields_ = [("heading", C.c_double), ("velocity", C.c_double * 4), ("acceleration", C.c_double * 4),
                ("jerk", C.c_double * 4)]


class Prediction(C.Structure):
    _fields_ = [("n_samples", C.c_int32), ("position", C.c_void_p), ("velocity", C.c_void_p),
                ("acceleration", C.c_void_p), ("jerk", C.c_void_p)]


class _FieldGeometryStruct(C.Structure):   # mrs_tg_field_geometry (FieldGeometry fills it)
    _fields_ = [("origin", C.c_double * 3), ("spacing", C.c_double * 3), ("dims", C.c_int32 * 3), ("n_fields", C.c_int32)]


class FieldRegion(C.Structure):   # mrs_tg_field_region: a grid of the stack and a box of its nodes, x y z, inclusive
    _fields_ = [("field", C.c_int32), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3)]


class FieldUpdateInfo(C.Structure):   # mrs_tg_field_update_info (field_update_query returns it as a dict)
    _fields_ = [("reach", C.c_int32 * 3), ("core_lo", C.c_int32 * 3), ("core_hi", C.c_int32 * 3), ("window_lo", C.c_int32 * 3),
                ("window_hi", C.c_int32 * 3), ("whole_grid", C.c_int32), ("workspace_bytes", C.c_int64)]


EXPORTED_SYMBOLS = [
    "mrs_tg_create", "mrs_tg_destroy", "mrs_tg_last_error", "mrs_tg_abi_version", "mrs_tg_capabilities", "mrs_tg_default_options",
    "mrs_tg_kernel_trace_reset", "mrs_tg_kernel_trace", "mrs_tg_plan_explain",
    "mrs_tg_set_stream", "mrs_tg_reset_stream", "mrs_tg_synchronize", "mrs_tg_solve_batch", "mrs_tg_plan_create", "mrs_tg_plan_destroy",
    "mrs_tg_plan_n_paths", "mrs_tg_plan_n_segments", "mrs_tg_plan_max_segments", "mrs_tg_plan_get_order",
    "mrs_tg_plan_assemble", "mrs_tg_plan_block_bytes", "mrs_tg_plan_solve", "mrs_tg_plan_bind_solve",
    "mrs_tg_bound_solve_launch", "mrs_tg_bound_solve_launch_many", "mrs_tg_bound_solve_launch_many_mt", "mrs_tg_bound_solve_launch_group",
    "mrs_tg_bound_solve_destroy", "mrs_tg_host_alloc", "mrs_tg_host_free", "mrs_tg_host_register",
    "mrs_tg_host_unregister", "mrs_tg_plan_cost_gradient",
    "mrs_tg_plan_segment_maxima", "mrs_tg_plan_sample_states", "mrs_tg_plan_careful_count", "mrs_tg_set_profiling", "mrs_tg_last_kernel_ms", "mrs_tg_kernel_ms_history",
    "mrs_tg_find_trajectory", "mrs_tg_find_trajectory_info", "mrs_tg_estimate_times_baca",
    "mrs_tg_default_policy_options", "mrs_tg_optimize_paths", "mrs_tg_waypoint_trajectory_idxs",
    "mrs_tg_create_multi", "mrs_tg_destroy_multi", "mrs_tg_multi_n_devices", "mrs_tg_multi_context", "mrs_tg_multi_shard",
    "mrs_tg_multi_solve_batch", "mrs_tg_multi_last_error",
    "mrs_tg_prepare_initial_condition", "mrs_tg_splice_prediction", "mrs_tg_plan_solve_vjp",
    "mrs_tg_plan_segment_maxima_vjp", "mrs_tg_plan_sample", "mrs_tg_plan_sample_states_vjp",
    "mrs_tg_plan_evaluate", "mrs_tg_plan_evaluate_vjp",
    "mrs_tg_plan_path_deviation", "mrs_tg_plan_path_deviation_vjp",
    "mrs_tg_plan_estimate_times", "mrs_tg_plan_estimate_times_vjp",
    "mrs_tg_plan_waypoint_passage", "mrs_tg_plan_waypoint_passage_vjp",
    "mrs_tg_plan_estimate_times_baca", "mrs_tg_plan_estimate_times_baca_vjp", "mrs_tg_plan_length_gate",
    "mrs_tg_plan_unwrap_headings", "mrs_tg_plan_fallback_sample", "mrs_tg_plan_fallback_sample_vjp",
    "mrs_tg_plan_preprocess_path", "mrs_tg_plan_insert_midpoints", "mrs_tg_plan_path_edit_vjp",
    "mrs_tg_plan_travel_heading", "mrs_tg_plan_travel_heading_vjp",
    "mrs_tg_plan_initial_condition", "mrs_tg_plan_initial_condition_vjp", "mrs_tg_plan_prepend_initial_condition",
    "mrs_tg_plan_prepend_initial_condition_vjp", "mrs_tg_plan_splice_prediction", "mrs_tg_plan_splice_prediction_vjp",
    "mrs_tg_plan_request_vertices", "mrs_tg_plan_request_vertices_vjp", "mrs_tg_plan_request_limits",
    "mrs_tg_plan_request_limits_vjp",
    "mrs_tg_plan_mutual_clearance", "mrs_tg_plan_mutual_clearance_vjp",
    "mrs_tg_plan_obstacle_clearance", "mrs_tg_plan_obstacle_clearance_vjp",
    "mrs_tg_plan_field_clearance", "mrs_tg_plan_field_clearance_vjp",
    "mrs_tg_field_from_occupancy", "mrs_tg_field_update_query", "mrs_tg_field_update_region",
]

_lib = None


def load_library():
    """dlopen libmrs_tg.so (built in-tree by mrs_uav_trajectory_generation_amd.build). Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MrsTgError("HIP extension %s is missing: run `python -m mrs_uav_trajectory_generation_amd.build` "
                         "(there is no CPU fallback)" % LIB_PATH)
    # PyTorch wheels bundle their own libamdhip64.so.7 / libhsa-runtime64 pair.  The dynamic loader keeps ONE library per
    # SONAME: if libmrs_tg.so pulled in the system libamdhip64.so.7 first, torch would later run its bundled HSA runtime
    # under the system HIP runtime and one of the two fails with "no ROCm-capable device".  In a process that uses both,
    # torch therefore has to be loaded first; a host without torch (the C++ hosts) simply uses the system runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, dp, ip, bp = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p  # raw addresses (host or device)
    L.mrs_tg_create.restype = C.c_int
    L.mrs_tg_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.mrs_tg_destroy.restype = None
    L.mrs_tg_destroy.argtypes = [vp]
    L.mrs_tg_last_error.restype = C.c_char_p
    L.mrs_tg_last_error.argtypes = [vp]
    L.mrs_tg_abi_version.restype = C.c_int
    L.mrs_tg_capabilities.restype = C.c_int
    L.mrs_tg_kernel_trace_reset.restype = None
    L.mrs_tg_kernel_trace.restype = C.c_int
    L.mrs_tg_kernel_trace.argtypes = [C.POINTER(C.c_char_p), C.c_int]
    L.mrs_tg_plan_explain.restype = C.c_int
    L.mrs_tg_plan_explain.argtypes = [vp, C.POINTER(Options), C.c_int32, C.POINTER(C.c_char_p), C.c_int32]
    L.mrs_tg_default_options.restype = None
    L.mrs_tg_default_options.argtypes = [C.POINTER(Options)]
    L.mrs_tg_host_alloc.restype = C.c_int
    L.mrs_tg_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.mrs_tg_host_free.restype = None
    L.mrs_tg_host_free.argtypes = [vp]
    L.mrs_tg_host_register.restype = C.c_int
    L.mrs_tg_host_register.argtypes = [vp, C.c_size_t]
    L.mrs_tg_host_unregister.restype = C.c_int
    L.mrs_tg_host_unregister.argtypes = [vp]
    L.mrs_tg_set_stream.restype = C.c_int
    L.mrs_tg_set_stream.argtypes = [vp, vp]
    L.mrs_tg_reset_stream.restype = C.c_int
    L.mrs_tg_reset_stream.argtypes = [vp]
    L.mrs_tg_synchronize.restype = C.c_int
    L.mrs_tg_synchronize.argtypes = [vp]
    L.mrs_tg_solve_batch.restype = C.c_int
    L.mrs_tg_solve_batch.argtypes = [vp, C.c_int32, ip, dp, bp, dp, dp, C.POINTER(Options), dp, dp, ip, dp, ip, dp]
    L.mrs_tg_plan_create.restype = C.c_int
    L.mrs_tg_plan_create.argtypes = [vp, C.c_int32, ip, C.POINTER(vp)]
    L.mrs_tg_plan_destroy.restype = None
    L.mrs_tg_plan_destroy.argtypes = [vp]
    for name in ("mrs_tg_plan_n_paths", "mrs_tg_plan_n_segments", "mrs_tg_plan_max_segments"):
        getattr(L, name).restype = C.c_int32
        getattr(L, name).argtypes = [vp]
    L.mrs_tg_plan_get_order.restype = C.c_int
    L.mrs_tg_plan_get_order.argtypes = [vp, ip]
    L.mrs_tg_plan_assemble.restype = C.c_int
    L.mrs_tg_plan_assemble.argtypes = [vp, C.c_int32, dp, dp, dp]
    L.mrs_tg_plan_block_bytes.restype = C.c_size_t
    L.mrs_tg_plan_block_bytes.argtypes = [vp]
    L.mrs_tg_plan_solve.restype = C.c_int
    L.mrs_tg_plan_solve.argtypes = [vp, dp, bp, dp, dp, C.POINTER(Options), dp, dp, ip, dp, ip, dp]
    L.mrs_tg_plan_bind_solve.restype = C.c_int
    L.mrs_tg_plan_bind_solve.argtypes = [vp, dp, bp, dp, dp, C.POINTER(Options), dp, dp, ip, dp, ip, dp, C.POINTER(vp)]
    L.mrs_tg_bound_solve_launch.restype = C.c_int
    L.mrs_tg_bound_solve_launch.argtypes = [vp]
    L.mrs_tg_bound_solve_launch_many.restype = C.c_int
    L.mrs_tg_bound_solve_launch_many.argtypes = [C.POINTER(vp), C.c_int32, C.c_int32]
    L.mrs_tg_bound_solve_launch_many_mt.restype = C.c_int
    L.mrs_tg_bound_solve_launch_many_mt.argtypes = [C.POINTER(vp), C.c_int32, C.c_int32, C.c_int32]
    L.mrs_tg_bound_solve_launch_group.restype = C.c_int
    L.mrs_tg_bound_solve_launch_group.argtypes = [C.POINTER(vp), C.c_int32, C.c_int32]
    L.mrs_tg_bound_solve_destroy.restype = None
    L.mrs_tg_bound_solve_destroy.argtypes = [vp]
    L.mrs_tg_plan_cost_gradient.restype = C.c_int
    L.mrs_tg_plan_cost_gradient.argtypes = [vp, C.c_int32, bp, dp, dp, dp, dp]
    L.mrs_tg_plan_segment_maxima.restype = C.c_int
    L.mrs_tg_plan_segment_maxima.argtypes = [vp, dp, dp, dp]
    L.mrs_tg_plan_solve_vjp.restype = C.c_int
    L.mrs_tg_plan_solve_vjp.argtypes = [vp, C.c_int32, bp, dp, dp, dp, ip, dp, dp, dp, dp]
    L.mrs_tg_plan_segment_maxima_vjp.restype = C.c_int
    L.mrs_tg_plan_segment_maxima_vjp.argtypes = [vp, dp, dp, dp, dp, dp, dp]
    L.mrs_tg_plan_careful_count.restype = C.c_int
    L.mrs_tg_plan_careful_count.argtypes = [vp, ip]
    L.mrs_tg_plan_sample_states.restype = C.c_int
    L.mrs_tg_plan_sample_states.argtypes = [vp, dp, dp, C.c_double, C.c_int32, ip, dp]
    L.mrs_tg_plan_sample.restype = C.c_int
    L.mrs_tg_plan_sample.argtypes = [vp, dp, dp, C.c_double, C.c_int32, ip, dp]
    L.mrs_tg_plan_sample_states_vjp.restype = C.c_int
    L.mrs_tg_plan_sample_states_vjp.argtypes = [vp, dp, dp, C.c_double, C.c_int32, C.c_int32, dp, ip, dp, dp, ip, dp, ip]
    L.mrs_tg_plan_evaluate.restype = C.c_int
    L.mrs_tg_plan_evaluate.argtypes = [vp, dp, dp, dp, C.c_int32, C.c_int32, dp, ip, dp]
    L.mrs_tg_plan_evaluate_vjp.restype = C.c_int
    L.mrs_tg_plan_evaluate_vjp.argtypes = [vp, dp, dp, dp, C.c_int32, C.c_int32, dp, ip, dp, dp, dp]
    L.mrs_tg_plan_path_deviation.restype = C.c_int
    L.mrs_tg_plan_path_deviation.argtypes = [vp, dp, ip, C.c_int32, dp, C.c_int32, ip, dp, ip, dp, ip, dp]
    L.mrs_tg_plan_path_deviation_vjp.restype = C.c_int
    L.mrs_tg_plan_path_deviation_vjp.argtypes = [vp, dp, ip, C.c_int32, dp, ip, dp, dp, dp]
    L.mrs_tg_plan_estimate_times.restype = C.c_int
    L.mrs_tg_plan_estimate_times.argtypes = [vp, dp, dp, dp]
    L.mrs_tg_plan_estimate_times_vjp.restype = C.c_int
    L.mrs_tg_plan_estimate_times_vjp.argtypes = [vp, dp, dp, dp, dp, dp, ip]
    L.mrs_tg_plan_waypoint_passage.restype = C.c_int
    L.mrs_tg_plan_waypoint_passage.argtypes = [vp, dp, ip, C.c_int32, ip, dp, ip, ip, ip, dp, dp]
    L.mrs_tg_plan_waypoint_passage_vjp.restype = C.c_int
    L.mrs_tg_plan_waypoint_passage_vjp.argtypes = [vp, dp, ip, C.c_int32, ip, dp, ip, dp, dp, dp, dp]
    L.mrs_tg_plan_estimate_times_baca.restype = C.c_int
    L.mrs_tg_plan_estimate_times_baca.argtypes = [vp, dp, dp, dp]
    L.mrs_tg_plan_estimate_times_baca_vjp.restype = C.c_int
    L.mrs_tg_plan_estimate_times_baca_vjp.argtypes = [vp, dp, dp, dp, dp, dp, ip]
    L.mrs_tg_plan_length_gate.restype = C.c_int
    L.mrs_tg_plan_length_gate.argtypes = [vp, dp, ip, C.c_double, C.c_double, C.c_double, ip, dp, ip]
    L.mrs_tg_plan_unwrap_headings.restype = C.c_int
    L.mrs_tg_plan_unwrap_headings.argtypes = [vp, dp, dp]
    L.mrs_tg_plan_fallback_sample.restype = C.c_int
    L.mrs_tg_plan_fallback_sample.argtypes = [vp, dp, vp, dp, C.c_double, C.c_double, C.c_int32, ip, dp, ip]
    L.mrs_tg_plan_fallback_sample_vjp.restype = C.c_int
    L.mrs_tg_plan_fallback_sample_vjp.argtypes = [vp, vp, dp, C.c_double, C.c_double, C.c_int32, dp, dp]
    L.mrs_tg_plan_preprocess_path.restype = C.c_int
    L.mrs_tg_plan_preprocess_path.argtypes = [vp, dp, vp, C.c_double, C.c_int32, C.c_double, C.c_double, ip, dp, vp, ip]
    L.mrs_tg_plan_insert_midpoints.restype = C.c_int
    L.mrs_tg_plan_insert_midpoints.argtypes = [vp, dp, vp, dp, C.c_double, C.c_int32, vp, ip, dp, vp, ip, vp]
    L.mrs_tg_plan_path_edit_vjp.restype = C.c_int
    L.mrs_tg_plan_path_edit_vjp.argtypes = [vp, ip, ip, vp, dp, dp]
    L.mrs_tg_plan_travel_heading.restype = C.c_int
    L.mrs_tg_plan_travel_heading.argtypes = [vp, dp, ip, C.c_int32, ip, C.c_double, dp, ip]
    L.mrs_tg_plan_travel_heading_vjp.restype = C.c_int
    L.mrs_tg_plan_travel_heading_vjp.argtypes = [vp, dp, ip, C.c_int32, ip, C.c_double, dp, dp]
    L.mrs_tg_plan_initial_condition.restype = C.c_int
    L.mrs_tg_plan_initial_condition.argtypes = [vp, ip, dp, dp, dp, C.c_double, dp, ip, dp, dp, dp, dp, ip, C.c_int32, ip, ip, dp]
    L.mrs_tg_plan_initial_condition_vjp.restype = C.c_int
    L.mrs_tg_plan_initial_condition_vjp.argtypes = [vp, ip, ip, dp, C.c_int32, dp, dp, dp, dp, dp, dp]
    L.mrs_tg_plan_prepend_initial_condition.restype = C.c_int
    L.mrs_tg_plan_prepend_initial_condition.argtypes = [vp, ip, C.c_int32, dp, vp, ip, dp, ip, dp, vp, ip]
    L.mrs_tg_plan_prepend_initial_condition_vjp.restype = C.c_int
    L.mrs_tg_plan_prepend_initial_condition_vjp.argtypes = [vp, ip, C.c_int32, ip, ip, C.c_int32, dp, dp, dp]
    L.mrs_tg_plan_splice_prediction.restype = C.c_int
    L.mrs_tg_plan_splice_prediction.argtypes = [vp, dp, ip, C.c_int32, ip, ip, ip, dp, dp, ip, C.c_int32, dp, ip, ip]
    L.mrs_tg_plan_splice_prediction_vjp.restype = C.c_int
    L.mrs_tg_plan_splice_prediction_vjp.argtypes = [vp, ip, C.c_int32, ip, ip, ip, dp, ip, C.c_int32, dp, dp, dp]
    L.mrs_tg_plan_request_vertices.restype = C.c_int
    L.mrs_tg_plan_request_vertices.argtypes = [vp, dp, bp, bp, dp, C.c_int32, dp, bp, dp]
    L.mrs_tg_plan_request_vertices_vjp.restype = C.c_int
    L.mrs_tg_plan_request_vertices_vjp.argtypes = [vp, bp, dp, dp, dp, dp]
    L.mrs_tg_plan_request_limits.restype = C.c_int
    L.mrs_tg_plan_request_limits.argtypes = [vp, dp, dp, ip, bp, dp, C.c_int32, C.c_double, C.c_double, dp, ip]
    L.mrs_tg_plan_request_limits_vjp.restype = C.c_int
    L.mrs_tg_plan_request_limits_vjp.argtypes = [vp, ip, C.c_int32, C.c_double, C.c_double, dp, dp, dp]
    L.mrs_tg_plan_mutual_clearance.restype = C.c_int
    L.mrs_tg_plan_mutual_clearance.argtypes = [vp, dp, ip, C.c_int32, ip, C.c_int32, ip, ip, C.c_double, dp, ip, dp, ip]
    L.mrs_tg_plan_mutual_clearance_vjp.restype = C.c_int
    L.mrs_tg_plan_mutual_clearance_vjp.argtypes = [vp, dp, ip, C.c_int32, ip, C.c_int32, ip, ip, C.c_double, ip, dp, dp]
    L.mrs_tg_plan_obstacle_clearance.restype = C.c_int
    L.mrs_tg_plan_obstacle_clearance.argtypes = [vp, dp, ip, C.c_int32, dp, C.c_int32, ip, C.c_int32, ip, ip, C.c_double, dp, ip, dp, ip]
    L.mrs_tg_plan_obstacle_clearance_vjp.restype = C.c_int
    L.mrs_tg_plan_obstacle_clearance_vjp.argtypes = [vp, dp, ip, C.c_int32, dp, C.c_int32, ip, C.c_int32, ip, ip, C.c_double, ip, dp, dp]
    gp = C.POINTER(_FieldGeometryStruct)
    L.mrs_tg_plan_field_clearance.restype = C.c_int
    L.mrs_tg_plan_field_clearance.argtypes = [vp, dp, ip, C.c_int32, dp, gp, ip, ip, C.c_double, dp, ip, dp, dp, ip]
    L.mrs_tg_plan_field_clearance_vjp.restype = C.c_int
    L.mrs_tg_plan_field_clearance_vjp.argtypes = [vp, dp, ip, C.c_int32, dp, gp, ip, ip, ip, dp, dp]
    L.mrs_tg_field_from_occupancy.restype = C.c_int
    L.mrs_tg_field_from_occupancy.argtypes = [vp, vp, gp, C.c_double, C.c_double, C.c_int32, dp]
    rp = C.POINTER(FieldRegion)
    L.mrs_tg_field_update_query.restype = C.c_int
    L.mrs_tg_field_update_query.argtypes = [gp, C.c_double, C.c_double, rp, C.POINTER(FieldUpdateInfo)]
    L.mrs_tg_field_update_region.restype = C.c_int
    L.mrs_tg_field_update_region.argtypes = [vp, vp, gp, C.c_double, C.c_double, C.c_int32, rp, vp, C.c_int64, dp]
    L.mrs_tg_set_profiling.restype = C.c_int
    L.mrs_tg_set_profiling.argtypes = [vp, C.c_int]
    L.mrs_tg_last_kernel_ms.restype = C.c_int
    L.mrs_tg_last_kernel_ms.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.mrs_tg_kernel_ms_history.restype = C.c_int
    L.mrs_tg_kernel_ms_history.argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.c_int]
    L.mrs_tg_find_trajectory_info.restype = C.c_int
    L.mrs_tg_find_trajectory_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.mrs_tg_estimate_times_baca.restype = C.c_int
    L.mrs_tg_estimate_times_baca.argtypes = [dp, C.c_int32, dp, dp]
    L.mrs_tg_find_trajectory.restype = C.c_int
    L.mrs_tg_find_trajectory.argtypes = [vp, C.POINTER(Waypoint), C.c_int32, C.POINTER(InitialState), dp,
                                         C.POINTER(Options), C.c_int32, dp, dp, ip, ip, dp]
    L.mrs_tg_default_policy_options.restype = None
    L.mrs_tg_default_policy_options.argtypes = [C.POINTER(PolicyOptions)]
    L.mrs_tg_optimize_paths.restype = C.c_int
    L.mrs_tg_optimize_paths.argtypes = [vp, C.c_int32, ip, C.POINTER(Waypoint), C.POINTER(InitialState), bp, dp, bp,
                                        C.POINTER(PolicyOptions), C.c_int32, ip, ip, dp, dp, ip, ip]
    L.mrs_tg_waypoint_trajectory_idxs.restype = C.c_int32
    L.mrs_tg_waypoint_trajectory_idxs.argtypes = [dp, C.c_int32, C.POINTER(Waypoint), C.c_int32, ip]
    L.mrs_tg_create_multi.restype = C.c_int
    L.mrs_tg_create_multi.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
    L.mrs_tg_destroy_multi.restype = None
    L.mrs_tg_destroy_multi.argtypes = [vp]
    L.mrs_tg_multi_n_devices.restype = C.c_int
    L.mrs_tg_multi_n_devices.argtypes = [vp]
    L.mrs_tg_multi_context.restype = vp
    L.mrs_tg_multi_context.argtypes = [vp, C.c_int]
    L.mrs_tg_multi_shard.restype = C.c_int
    L.mrs_tg_multi_shard.argtypes = [vp, C.c_int32, ip, ip]
    L.mrs_tg_multi_solve_batch.restype = C.c_int
    L.mrs_tg_multi_solve_batch.argtypes = [vp, C.c_int32, ip, dp, bp, dp, dp, C.POINTER(Options), dp, dp, ip, dp, ip, dp]
    L.mrs_tg_multi_last_error.restype = C.c_char_p
    L.mrs_tg_multi_last_error.argtypes = [vp]
    L.mrs_tg_prepare_initial_condition.restype = C.c_int
    L.mrs_tg_prepare_initial_condition.argtypes = [C.POINTER(Waypoint), C.POINTER(InitialState), C.c_double, C.POINTER(Prediction),
                                                   dp, C.c_double, C.c_double, C.c_int32, C.c_int32, C.POINTER(Waypoint),
                                                   C.POINTER(InitialState), ip, ip, ip, ip]
    L.mrs_tg_splice_prediction.restype = C.c_int32
    L.mrs_tg_splice_prediction.argtypes = [C.POINTER(Prediction), C.c_int32, C.c_double, dp, C.c_int32, C.c_int32]
    _lib = L
    return L


CAP_CAREFUL_COST = 1   # MRS_TG_CAP_CAREFUL_COST
CAP_FUTURE_PATHS = 2   # MRS_TG_CAP_FUTURE_PATHS: prepare_initial_condition / splice_prediction
CAP_REFINE = 4         # MRS_TG_CAP_REFINE: FLAG_REFINE is honoured
CAP_GRADIENT = 8       # MRS_TG_CAP_GRADIENT: Plan.solve_vjp (the backward pass of the fixed-times solve)
CAP_MAXIMA_GRADIENT = 16   # MRS_TG_CAP_MAXIMA_GRADIENT: Plan.segment_maxima_vjp (the backward pass of the segment maxima)
CAP_SAMPLE_GRADIENT = 32   # MRS_TG_CAP_SAMPLE_GRADIENT: Plan.sample_states_vjp (the backward pass of the sampler), Plan.sample
CAP_EVALUATE = 64          # MRS_TG_CAP_EVALUATE: Plan.evaluate (the state at caller-given times), Plan.evaluate_vjp
CAP_DEVIATION = 128        # MRS_TG_CAP_DEVIATION: Plan.path_deviation (samples against the waypoint polyline), Plan.path_deviation_vjp
CAP_ESTIMATE_GRADIENT = 256   # MRS_TG_CAP_ESTIMATE_GRADIENT: Plan.estimate_times (the Euclidean estimate as a plan step), Plan.estimate_times_vjp
CAP_WAYPOINT_PASSAGE = 512    # MRS_TG_CAP_WAYPOINT_PASSAGE: Plan.waypoint_passage (where the samples pass the requested waypoints), Plan.waypoint_passage_vjp
CAP_BACA = 1024               # MRS_TG_CAP_BACA: Plan.estimate_times_baca (the Baca estimate as a plan step), Plan.estimate_times_baca_vjp, Plan.length_gate
CAP_PATH_EDIT = 4096          # MRS_TG_CAP_PATH_EDIT: Plan.preprocess_path (preprocessPath's thinning), Plan.insert_midpoints (the mid-points of unsafe segments), Plan.path_edit_vjp
CAP_FALLBACK_SAMPLE = 2048    # MRS_TG_CAP_FALLBACK_SAMPLE: Plan.unwrap_headings, Plan.fallback_sample (findTrajectoryFallback's rows as a plan step), Plan.fallback_sample_vjp
CAP_TRAVEL_HEADING = 8192     # MRS_TG_CAP_TRAVEL_HEADING: Plan.travel_heading (the heading along the direction of travel, override_heading_atan2), Plan.travel_heading_vjp
CAP_INITIAL_CONDITION = 16384  # MRS_TG_CAP_INITIAL_CONDITION: Plan.initial_condition, Plan.prepend_initial_condition, Plan.splice_prediction and their three backward passes
# Plan.initial_condition's decision word (MRS_TG_IC_*) and its flags input (bit 0 tracker command, bit 1 UAV state, bit 2 dont_prepend)
IC_PREPEND, IC_FROM_FUTURE, IC_DROP_FIRST, IC_FROM_TRACKER, IC_FROM_UAV, IC_FROM_PREDICTION, IC_INVALID = 1, 2, 4, 8, 16, 32, 64
IC_FLAG_TRACKER, IC_FLAG_UAV, IC_FLAG_DONT_PREPEND = 1, 2, 4
CAP_REQUEST = 32768   # MRS_TG_CAP_REQUEST: Plan.request_vertices, Plan.request_limits (findTrajectory's vertices and limits as plan steps) and their two backward passes
CAP_MUTUAL_CLEARANCE = 65536   # MRS_TG_CAP_MUTUAL_CLEARANCE: Plan.mutual_clearance (the nearest other path of a row's group at the same step), Plan.mutual_clearance_vjp
CAP_OBSTACLE_CLEARANCE = 131072   # MRS_TG_CAP_OBSTACLE_CLEARANCE: Plan.obstacle_clearance (the nearest sphere or point of the path's obstacle set, signed), Plan.obstacle_clearance_vjp
CAP_FIELD_CLEARANCE = 262144   # MRS_TG_CAP_FIELD_CLEARANCE: Plan.field_clearance (the trilinear interpolant of a voxel grid of signed distances, its cell and gradient), Plan.field_clearance_vjp
CAP_FIELD_FROM_OCCUPANCY = 524288   # MRS_TG_CAP_FIELD_FROM_OCCUPANCY: Context.field_from_occupancy (that grid built on the device from an occupancy grid, an exact Euclidean distance transform)
CAP_FIELD_UPDATE_REGION = 1048576   # MRS_TG_CAP_FIELD_UPDATE_REGION: field_update_query, Context.field_update_region (that grid brought up to date after the occupancy changed inside a box)
FIELD_SIGNED, FIELD_MAX_DIM = 1, 1024  # MRS_TG_FIELD_SIGNED (mrs_tg_field_from_occupancy's flag), MRS_TG_FIELD_MAX_DIM (its largest dim)
# Plan.request_limits' flags input (MRS_TG_REQ_*) and its branch word (MRS_TG_LIM_*)
REQ_OVERRIDE, REQ_RELAX_HEADING = 1, 2
LIM_OVERRIDDEN, LIM_OVERRIDE_REFUSED, LIM_RELAXED, LIM_V_DESCENDING, LIM_A_DESCENDING, LIM_J_DESCENDING, LIM_FALLBACK = 1, 2, 4, 8, 16, 32, 64
# Plan.estimate_times_baca_vjp's flags: the branches of the Baca estimate a segment's time took, as bits (MRS_TG_BACA_*)
BACA_V_VERTICAL, BACA_A_VERTICAL, BACA_J_VERTICAL, BACA_T1_CAPPED, BACA_T2_CAPPED = 1, 2, 4, 8, 16
BACA_DOT1_CLAMPED, BACA_DOT2_CLAMPED, BACA_FLOOR, BACA_HEADING, BACA_HEADING_CRUISE, BACA_HEADING_ACC = 32, 64, 128, 256, 512, 1024
# Plan.estimate_times_vjp's term: the term of the estimate a segment's time came from (MRS_TG_ESTIMATE_TERM_*)
ESTIMATE_TERM_HORIZONTAL, ESTIMATE_TERM_VERTICAL, ESTIMATE_TERM_FLOOR, ESTIMATE_TERM_HEADING = 0, 1, 2, 3


def capabilities():
    return load_library().mrs_tg_capabilities()


def kernel_trace_reset():
    load_library().mrs_tg_kernel_trace_reset()


def kernel_trace():
    """Names of the kernels this thread has launched through the library since kernel_trace_reset() (newest 32, oldest first)."""
    buf = (C.c_char_p * 32)()
    n = load_library().mrs_tg_kernel_trace(buf, 32)
    return [buf[i].decode() for i in range(n)]


def default_policy_options(solver=None, **overrides):
    opt = PolicyOptions()
    load_library().mrs_tg_default_policy_options(C.byref(opt))
    for k, v in (solver or {}).items():
        if not hasattr(opt.solver, k):
            raise TypeError("unknown solver option %r" % k)
        setattr(opt.solver, k, v)
    for k, v in overrides.items():
        if not hasattr(opt, k):
            raise TypeError("unknown policy option %r" % k)
        setattr(opt, k, v)
    return opt


def estimate_times_baca(waypoints, limits9):
    """estimateSegmentTimesBaca for one path (mrs_tg_estimate_times_baca): waypoints [V][4], headings already unwrapped"""
    wp = np.ascontiguousarray(waypoints, dtype=np.float64).reshape(-1, 4)
    lim = np.ascontiguousarray(limits9, dtype=np.float64)
    out = np.zeros(wp.shape[0] - 1)
    rc = load_library().mrs_tg_estimate_times_baca(_np_ptr(wp), wp.shape[0], _np_ptr(lim), _np_ptr(out))
    if rc != 0:
        raise MrsTgError("mrs_tg_estimate_times_baca failed (%d)" % rc)
    return out


def _prediction(prediction):
    """(Prediction, arrays kept alive) from a dict of [n][4] arrays position / velocity / acceleration / jerk, or None"""
    if prediction is None:
        return None, ()
    arrs = [np.ascontiguousarray(prediction[k], dtype=np.float64).reshape(-1, 4)
            for k in ("position", "velocity", "acceleration", "jerk")]
    n = arrs[0].shape[0]
    if any(a.shape[0] != n for a in arrs):
        raise ValueError("the prediction's four arrays need the same number of samples")
    return Prediction(n, *(a.ctypes.data for a in arrs)), arrs


def prepare_initial_condition(tracker=None, tracker_age=0.0, prediction=None, uav_pose=None, takeoff_height=0.0,
                              path_time_offset=0.0, n_path_waypoints=1, dont_prepend=False):
    """prepareInitialCondition (mrs_trajectory_generation.cpp:506-614) + the first-waypoint rule (:650-655) for one request
    (mrs_tg_prepare_initial_condition; host arithmetic, no device).
    tracker: None or a dict with "position" (x, y, z, heading) and "velocity" / "acceleration" / "jerk" (4 each, the 4th the
    heading's); prediction: None or a dict of [n][4] arrays "position" / "velocity" / "acceleration" / "jerk";
    uav_pose: None or (x, y, z, heading).  Returns a dict: has_initial_condition, from_future, sample_offset,
    drop_first_waypoint, waypoint (4,) and initial_state (dict in optimize_paths' form) -- the latter two None without one."""
    L = load_library()
    pose = st = None
    if tracker is not None:
        pose = Waypoint()
        st = InitialState()
        for i in range(4):
            pose.coords[i] = float(tracker["position"][i])
            st.velocity[i] = float(tracker["velocity"][i])
            st.acceleration[i] = float(tracker["acceleration"][i])
            st.jerk[i] = float(tracker["jerk"][i])
        st.heading = float(tracker["position"][3])
    pred, _keep = _prediction(prediction)
    uav = None if uav_pose is None else np.ascontiguousarray(uav_pose, dtype=np.float64).reshape(4)
    wp_out, st_out = Waypoint(), InitialState()
    flags = np.zeros(4, dtype=np.int32)
    rc = L.mrs_tg_prepare_initial_condition(C.byref(pose) if pose is not None else None, C.byref(st) if st is not None else None,
                                            float(tracker_age), C.byref(pred) if pred is not None else None, _np_ptr(uav),
                                            float(takeoff_height), float(path_time_offset), int(n_path_waypoints), int(bool(dont_prepend)),
                                            C.byref(wp_out), C.byref(st_out), flags[0:].ctypes.data, flags[1:].ctypes.data,
                                            flags[2:].ctypes.data, flags[3:].ctypes.data)
    if rc != 0:
        raise MrsTgError("mrs_tg_prepare_initial_condition failed (%d): %s" % (rc, L.mrs_tg_last_error(None).decode()))
    has = bool(flags[0])
    return dict(has_initial_condition=has, from_future=bool(flags[1]), sample_offset=int(flags[2]),
                drop_first_waypoint=bool(flags[3]),
                waypoint=np.array(wp_out.coords[:]) if has else None,
                initial_state=dict(heading=st_out.heading, velocity=np.array(st_out.velocity[:]),
                                   acceleration=np.array(st_out.acceleration[:]), jerk=np.array(st_out.jerk[:])) if has else None)


def splice_prediction(prediction, sample_offset, prediction_age, samples, sample_capacity=None):
    """The pre-trajectory of a path from the future (mrs_trajectory_generation.cpp:801-838, mrs_tg_splice_prediction): returns
    a new [m][4] array -- prediction rows 0 .. sample_offset-1 in front of samples [n][4] when sample_offset exceeds the
    prediction's current index, else samples unchanged.  sample_capacity (default: room for the whole prediction) is the
    buffer handed to the library; when the result does not fit, MrsTgError names the count needed."""
    L = load_library()
    pred, _keep = _prediction(prediction)
    smp = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1, 4)
    n = smp.shape[0]
    cap = n + (pred.n_samples if pred is not None else 0) if sample_capacity is None else int(sample_capacity)
    buf = np.zeros((max(cap, n, 1), 4))
    buf[:n] = smp
    m = L.mrs_tg_splice_prediction(C.byref(pred) if pred is not None else None, int(sample_offset), float(prediction_age),
                                   _np_ptr(buf), n, cap)
    if m < 0:
        raise MrsTgError("mrs_tg_splice_prediction failed (%d): %s" % (m, L.mrs_tg_last_error(None).decode()))
    if m > cap:
        raise MrsTgError("mrs_tg_splice_prediction: %d samples need a capacity of %d, not %d" % (m, m, cap))
    return buf[:m].copy()


def default_options(**overrides):
    opt = Options()
    load_library().mrs_tg_default_options(C.byref(opt))
    for k, v in overrides.items():
        if not hasattr(opt, k):
            raise TypeError("unknown option %r" % k)
        setattr(opt, k, v)
    return opt


def _np_ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


class _PinnedOwner:
    """frees a block of mrs_tg_host_alloc when the last reference to it is gone"""

    def __init__(self, nbytes):
        self._L = load_library()
        self.ptr = C.c_void_p()
        rc = self._L.mrs_tg_host_alloc(C.c_size_t(nbytes), C.byref(self.ptr))
        if rc:
            raise MrsTgError("mrs_tg_host_alloc failed (%d): %s" % (rc, self._L.mrs_tg_last_error(None).decode()))

    def __del__(self):
        if getattr(self, "ptr", None) is not None and self.ptr.value:
            self._L.mrs_tg_host_free(self.ptr)
            self.ptr = C.c_void_p()


def pinned_empty(shape, dtype=np.float64):
    """A numpy array in pinned host memory (mrs_tg_host_alloc): the GPU's DMA engines read / write it directly, so
    mrs_tg_solve_batch neither stages nor pins it per call.  The block lives as long as ANY array that views it: numpy
    collapses chains of views onto the buffer object they all come from (here the ctypes array), so the owner of the block
    hangs on that object -- not on the first array handed out, which a slice or a ravel() of it does not keep alive."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) if np.ndim(shape) else int(shape)
    owner = _PinnedOwner(n * dtype.itemsize)
    buf = (C.c_char * max(n * dtype.itemsize, 1)).from_address(owner.ptr.value)
    buf._owner = owner   # buffer object -> owner; every view -> buffer object
    return np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)


def pinned_copy(a):
    out = pinned_empty(a.shape, a.dtype)
    out[...] = a
    return out


def _t_ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _check_offsets(offsets, name, end, end_name):
    """host offsets as a contiguous int32 array, or ValueError: they start at 0, do not decrease and end at `end`"""
    try:
        raw = np.asarray(offsets)
    except Exception as e:
        raise ValueError("%s is not an array of integers: %s" % (name, e))
    if raw.ndim != 1 or raw.size < 1 or raw.dtype.kind not in "iu":
        raise ValueError("%s must be a one-dimensional array of at least one integer" % name)
    g = raw.astype(np.int64)
    if g[0] != 0 or g[-1] != int(end) or np.any(np.diff(g) < 0):
        raise ValueError("%s must start at 0, not decrease and end at %s = %d (got %s)" % (name, end_name, end, g.tolist()))
    return np.ascontiguousarray(g, dtype=np.int32)


def check_group_offsets(group_offsets, n_paths):
    """Host group offsets of Plan.mutual_clearance as a contiguous int32 array [n_groups + 1], or ValueError: they start at 0,
    do not decrease and end at n_paths (a group may be empty).  No device is needed."""
    return _check_offsets(group_offsets, "group_offsets", n_paths, "n_paths")


def check_set_offsets(set_offsets, n_obstacles):
    """Host set offsets of Plan.obstacle_clearance as a contiguous int32 array [n_sets + 1], or ValueError: they start at 0, do
    not decrease and end at n_obstacles (a set may be empty).  No device is needed."""
    return _check_offsets(set_offsets, "set_offsets", n_obstacles, "n_obstacles")


class FieldGeometry:
    """mrs_tg_field_geometry: the geometry the grids of one fields array [n_fields][nz][ny][nx] share -- origin (x, y, z of
    node (0, 0, 0)), spacing (hx, hy, hz), dims (nx, ny, nz), n_fields.  Node-centred: a caller with cell-centred voxels
    passes the centre of voxel 0 as the origin."""

    def __init__(self, origin, spacing, dims, n_fields=1):
        self.origin = tuple(float(x) for x in origin)
        self.spacing = tuple(float(x) for x in spacing)
        self.dims = tuple(int(x) for x in dims)
        self.n_fields = int(n_fields)
        if len(self.origin) != 3 or len(self.spacing) != 3 or len(self.dims) != 3:
            raise ValueError("origin, spacing and dims have three entries each: x, y, z")

    def fields_shape(self):
        return (self.n_fields, self.dims[2], self.dims[1], self.dims[0])

    def as_struct(self):
        g = _FieldGeometryStruct()
        g.origin[:], g.spacing[:], g.dims[:], g.n_fields = self.origin, self.spacing, self.dims, self.n_fields
        return g

    def __repr__(self):
        return "FieldGeometry(origin=%r, spacing=%r, dims=%r, n_fields=%d)" % (self.origin, self.spacing, self.dims, self.n_fields)


def check_field_geometry(fields_shape, geometry):
    """The geometry of Plan.field_clearance against the shape of its fields tensor, or ValueError: dims each >= 2, spacing
    finite and positive, origin finite, n_fields >= 0, n_fields nz ny nx at most 2^31 - 1 (a cell is an int32), and the shape
    [n_fields][nz][ny][nx].  No device is needed.  Returns the geometry."""
    if not isinstance(geometry, FieldGeometry):
        raise ValueError("geometry must be an api.FieldGeometry")
    if any(n < 2 for n in geometry.dims):
        raise ValueError("every dim of a field must be at least 2 (a 2-D map is two equal layers), not %r" % (geometry.dims,))
    if not all(np.isfinite(h) and h > 0.0 for h in geometry.spacing):
        raise ValueError("spacing must be finite and positive, not %r" % (geometry.spacing,))
    if not all(np.isfinite(o) for o in geometry.origin):
        raise ValueError("origin must be finite, not %r" % (geometry.origin,))
    if geometry.n_fields < 0:
        raise ValueError("n_fields %d is negative" % geometry.n_fields)
    nx, ny, nz = geometry.dims
    if geometry.n_fields * nz * ny * nx > 2 ** 31 - 1:
        raise ValueError("n_fields nz ny nx = %d exceeds 2^31 - 1: a cell is an int32" % (geometry.n_fields * nz * ny * nx))
    if tuple(int(x) for x in fields_shape) != geometry.fields_shape():
        raise ValueError("fields must be [n_fields][nz][ny][nx] = %s, not %s" % (list(geometry.fields_shape()), list(fields_shape)))
    return geometry


def _check_operand(name, t, dtype, shape, like=None, optional=False):
    """a device tensor as a plan step takes it, or ValueError: dtype, device (`like`'s), contiguous, the shape (None in it: any
    extent)"""
    import torch
    if t is None:
        if optional:
            return
        raise ValueError("%s is required" % name)
    if not isinstance(t, torch.Tensor) or not t.is_cuda or (like is not None and t.device != like.device):
        raise ValueError("%s must be a tensor on the device%s" % (name, "" if like is None else " of samples"))
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s tensor" % (name, dtype))
    if t.dim() != len(shape) or any(want is not None and have != want for have, want in zip(t.shape, shape)):
        raise ValueError("%s must be %s, not %s" % (name, "".join("[%s]" % ("." if w is None else w) for w in shape),
                                                    list(t.shape)))


def check_occupancy_operands(occupancy, geometry, z_scale, max_distance, out=None, device=None):
    """What Context.field_from_occupancy checks before anything reaches the library, or ValueError; no device is needed to be
    refused.  The geometry as check_field_geometry checks it against occupancy's shape [n_fields][nz][ny][nx], every dim at
    most FIELD_MAX_DIM, z_scale finite and positive, max_distance positive (inf: no cap; nan refused); occupancy a contiguous
    uint8 tensor on the device (`device`: the context's ordinal, None = any), out None or a contiguous float64 tensor of the
    same shape on the same device."""
    import torch
    if not isinstance(occupancy, torch.Tensor):
        raise ValueError("occupancy must be a tensor")
    check_field_geometry(occupancy.shape, geometry)
    if any(n > FIELD_MAX_DIM for n in geometry.dims):
        raise ValueError("every dim of an occupancy grid is at most %d, not %r" % (FIELD_MAX_DIM, geometry.dims))
    if not (np.isfinite(z_scale) and z_scale > 0.0):
        raise ValueError("z_scale must be finite and positive, not %r" % (z_scale,))
    if not max_distance > 0.0:
        raise ValueError("max_distance must be positive (inf: no cap), not %r" % (max_distance,))
    shape = geometry.fields_shape()
    _check_operand("occupancy", occupancy, torch.uint8, shape)
    _check_operand("out", out, torch.float64, shape, occupancy, optional=True)
    if device is not None and occupancy.device.index != device:
        raise ValueError("occupancy must be on the context's device %d, not %s" % (device, occupancy.device))


def _check_region(geometry, lo, hi, field):
    """the box lo .. hi (x, y, z node indices, inclusive) of grid `field` of a checked geometry as a FieldRegion, or ValueError"""
    if geometry.n_fields == 0:
        raise ValueError("n_fields is 0: there is no grid to update")
    try:
        lo, hi, field = tuple(int(x) for x in lo), tuple(int(x) for x in hi), int(field)
    except (TypeError, ValueError):
        raise ValueError("lo and hi are three node indices each (x, y, z) and field is an integer")
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("lo and hi have three entries each: x, y, z")
    if not 0 <= field < geometry.n_fields:
        raise ValueError("field %d is outside [0, %d)" % (field, geometry.n_fields))
    for a in range(3):
        if not 0 <= lo[a] <= hi[a] < geometry.dims[a]:
            raise ValueError("axis %d of the box: [%d, %d] is empty or not inside [0, %d]" % (a, lo[a], hi[a], geometry.dims[a] - 1))
    r = FieldRegion()
    r.field, r.lo[:], r.hi[:] = field, lo, hi
    return r


def field_update_query(geometry, lo, hi, field=0, z_scale=1.0, max_distance=float("inf")):
    """mrs_tg_field_update_query: what Context.field_update_region does for a change of the occupancy inside the box lo .. hi (x,
    y, z node indices, inclusive) of grid `field`, as a dict: reach [3] (how many nodes a voxel is felt along each axis under the
    cap max_distance), core_lo / core_hi (the nodes that are recomputed and written: the box grown by the reach, clipped),
    window_lo / window_hi (the occupancy that is read: the core grown by the reach, clipped), whole_grid (the window is the whole
    grid -- always with max_distance = inf: the full transform runs on that grid, the core is the whole grid) and
    workspace_bytes (0 with whole_grid).  Host only: no context, no device.  ValueError for a geometry, scalar or box the library
    would refuse."""
    if not isinstance(geometry, FieldGeometry):
        raise ValueError("geometry must be an api.FieldGeometry")
    check_field_geometry(geometry.fields_shape(), geometry)
    if any(n > FIELD_MAX_DIM for n in geometry.dims):
        raise ValueError("every dim of an occupancy grid is at most %d, not %r" % (FIELD_MAX_DIM, geometry.dims))
    if not (np.isfinite(z_scale) and z_scale > 0.0):
        raise ValueError("z_scale must be finite and positive, not %r" % (z_scale,))
    if not max_distance > 0.0:
        raise ValueError("max_distance must be positive (inf: no cap), not %r" % (max_distance,))
    region = _check_region(geometry, lo, hi, field)
    L = load_library()
    g, info = geometry.as_struct(), FieldUpdateInfo()
    rc = L.mrs_tg_field_update_query(C.byref(g), float(z_scale), float(max_distance), C.byref(region), C.byref(info))
    if rc != 0:
        raise MrsTgError("mrs_tg_field_update_query failed (%d): %s" % (rc, L.mrs_tg_last_error(None).decode()))
    out = {k: list(getattr(info, k)) for k in ("reach", "core_lo", "core_hi", "window_lo", "window_hi")}
    out["whole_grid"], out["workspace_bytes"] = int(info.whole_grid), int(info.workspace_bytes)
    return out


def check_region_operands(occupancy, fields, geometry, lo, hi, field=0, z_scale=1.0, max_distance=float("inf"), workspace=None,
                          device=None):
    """What Context.field_update_region checks before anything reaches the library, or ValueError; no device is needed to be
    refused.  Everything check_occupancy_operands checks, with fields (required) in the place of out; the box as
    field_update_query takes it; workspace None or a contiguous float64 tensor on occupancy's device that holds at least the
    query's workspace_bytes and shares no memory with occupancy or fields.  Returns (the FieldRegion, the query's dict)."""
    import torch
    if fields is None:
        raise ValueError("fields is required: the field of the old occupancy, updated in place")
    check_occupancy_operands(occupancy, geometry, z_scale, max_distance, None, device)
    _check_operand("fields", fields, torch.float64, geometry.fields_shape(), occupancy)
    region = _check_region(geometry, lo, hi, field)
    info = field_update_query(geometry, lo, hi, field, z_scale, max_distance)
    if workspace is not None:
        _check_operand("workspace", workspace, torch.float64, (None,), occupancy)
        if workspace.numel() * 8 < info["workspace_bytes"]:
            raise ValueError("workspace holds %d bytes, the update needs %d" % (workspace.numel() * 8, info["workspace_bytes"]))
        for name, t in (("occupancy", occupancy), ("fields", fields)):
            a, b = workspace.data_ptr(), t.data_ptr()
            if a < b + t.numel() * t.element_size() and b < a + workspace.numel() * 8:
                raise ValueError("workspace overlaps %s" % name)
    return region, info


class Context:
    """One HIP device + stream (mrs_tg_ctx)."""

    def __init__(self, device=0):
        self._L = load_library()
        h = C.c_void_p()
        rc = self._L.mrs_tg_create(int(device), C.byref(h))
        if rc != 0:
            raise MrsTgError("mrs_tg_create failed (%d): %s" % (rc, self._L.mrs_tg_last_error(None).decode()))
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._L.mrs_tg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise MrsTgError("%s failed (%d): %s" % (what, rc, self._L.mrs_tg_last_error(self._h).decode()))

    def use_torch_stream(self):
        """Launch on torch's current HIP stream so torch events / allocator ordering apply."""
        import torch
        self._check(self._L.mrs_tg_set_stream(self._h, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "set_stream")

    def synchronize(self):
        self._check(self._L.mrs_tg_synchronize(self._h), "synchronize")

    def set_profiling(self, enabled):
        self._check(self._L.mrs_tg_set_profiling(self._h, int(bool(enabled))), "set_profiling")

    def last_kernel_ms(self, kernel_id):
        ms = C.c_float(0)
        self._check(self._L.mrs_tg_last_kernel_ms(self._h, int(kernel_id), C.byref(ms)), "last_kernel_ms")
        return ms.value

    def kernel_ms_history(self, kernel_id, capacity=512):
        """Per-dispatch durations (ms) of the newest timed launches since set_profiling(True), oldest first."""
        buf = (C.c_float * capacity)()
        n = self._L.mrs_tg_kernel_ms_history(self._h, int(kernel_id), buf, capacity)
        if n < 0:
            self._check(n, "kernel_ms_history")
        return [buf[i] for i in range(n)]

    def field_from_occupancy(self, occupancy, geometry, z_scale=1.0, max_distance=float("inf"), signed=True, out=None):
        """mrs_tg_field_from_occupancy: the voxel grid of distances Plan.field_clearance reads, built on the device from an
        occupancy grid by an exact Euclidean distance transform.  occupancy [n_fields][nz][ny][nx] uint8 on the context's
        device (non-zero: occupied) with geometry (an api.FieldGeometry, every dim at most FIELD_MAX_DIM; checked: ValueError)
        -> the float64 tensor of the same shape (out, or a new one): at a free node the distance to the nearest occupied node of
        its own grid, sqrt((hx^2 di^2 + hy^2 dj^2) + (z_scale hz)^2 dk^2) minimised over the nodes, capped at max_distance; at
        an occupied node minus the capped distance to the nearest free node (signed) or 0 (signed=False).  The definition's
        bits, whatever the grid.  THE TRAP of max_distance = inf: an all-free or all-occupied grid
        yields +-inf voxels and Plan.field_clearance's lerp(inf, inf, t) is NaN -- pass a finite cap to a field that is looked
        up (it also bounds the cost on a sparse map).  There is no autograd entry: occupancy is discrete, nothing here has a
        gradient.  Asynchronous on the context's stream; occupancy is never written."""
        import torch
        check_occupancy_operands(occupancy, geometry, z_scale, max_distance, out, self.device)
        if out is None:
            out = torch.empty(geometry.fields_shape(), dtype=torch.float64, device=occupancy.device)
        g = geometry.as_struct()
        self._check(self._L.mrs_tg_field_from_occupancy(self._h, _t_ptr(occupancy), C.byref(g), float(z_scale), float(max_distance),
                                                        FIELD_SIGNED if signed else 0, _t_ptr(out)),
                    "mrs_tg_field_from_occupancy")
        return out

    def field_update_region(self, occupancy, fields, geometry, lo, hi, field=0, z_scale=1.0, max_distance=float("inf"), signed=True,
                            workspace=None):
        """mrs_tg_field_update_region: the field of field_from_occupancy brought up to date after the occupancy changed inside
        a box.  occupancy is the NEW occupancy of the whole stack; fields holds the field of the OLD one, built with the same
        z_scale, max_distance and signed; lo .. hi (x, y, z node indices, inclusive) holds every voxel of grid `field` whose
        byte may differ.  Updates fields IN PLACE and returns it: afterwards it is field_from_occupancy(occupancy, ...) in every
        bit, and only the nodes of the core (field_update_query) were written.  workspace: a float64 tensor of at least the
        query's workspace_bytes, or None -- then one is allocated here (a caller in a loop passes its own).  With
        max_distance = inf, or a box whose window is the whole grid, the full transform runs on that grid (DESIGN.md section
        11m).  No autograd entry.  Asynchronous on the context's stream; occupancy is never written."""
        import torch
        region, info = check_region_operands(occupancy, fields, geometry, lo, hi, field, z_scale, max_distance, workspace, self.device)
        if workspace is None and info["workspace_bytes"] > 0:
            workspace = torch.empty((info["workspace_bytes"] // 8,), dtype=torch.float64, device=occupancy.device)
        g = geometry.as_struct()
        self._check(self._L.mrs_tg_field_update_region(self._h, _t_ptr(occupancy), C.byref(g), float(z_scale), float(max_distance),
                                                       FIELD_SIGNED if signed else 0, C.byref(region),
                                                       None if workspace is None else _t_ptr(workspace),
                                                       0 if workspace is None else workspace.numel() * 8, _t_ptr(fields)),
                    "mrs_tg_field_update_region")
        return fields

    def solve_batch(self, batch: Batch, seg_times=None, out=None, **opts):
        """Host arrays in, host arrays out (mrs_tg_solve_batch).  seg_times None => estimate_times.
        out: the dict of a previous call with the same shapes (or arrays from pinned_empty): its arrays are written in place
        instead of allocating new ones -- what a server that calls in a loop does; `times` is then used as given AND
        overwritten unless seg_times is passed."""
        opt = default_options(derivative_to_optimize=batch.derivative_to_optimize, **opts)
        nS, P = batch.n_segments, batch.n_paths
        sampling = opt.sampling_dt > 0
        if out is not None:
            t, coeffs, status, cost = out["times"], out["coeffs"], out["status"], out["cost"]
            n_samples, samples = (out["n_samples"], out["samples"]) if sampling else (None, None)
            if seg_times is None:
                opt.estimate_times = 1
            else:
                t[:] = seg_times
            assert t.size == nS and coeffs.shape == (nS, N_DIM, N_COEFF) and status.size == P
        else:
            if seg_times is None:
                opt.estimate_times = 1
                t = np.zeros(nS)
            else:
                t = np.ascontiguousarray(seg_times, dtype=np.float64).copy()
                assert t.size == nS
            coeffs = np.zeros((nS, N_DIM, N_COEFF))
            status = np.zeros(P, dtype=np.int32)
            cost = np.zeros(P)
            n_samples = np.zeros(P, dtype=np.int32) if sampling else None
            samples = np.zeros((P, max(opt.sample_capacity, 1), N_DIM)) if sampling else None
        rc = self._L.mrs_tg_solve_batch(self._h, P, _np_ptr(batch.seg_offsets), _np_ptr(batch.waypoints),
                                        _np_ptr(batch.fixed_mask), _np_ptr(batch.fixed_values), _np_ptr(batch.limits),
                                        C.byref(opt), _np_ptr(t), _np_ptr(coeffs), _np_ptr(status), _np_ptr(cost),
                                        _np_ptr(n_samples), _np_ptr(samples))
        self._check(rc, "mrs_tg_solve_batch")
        return dict(times=t, coeffs=coeffs, status=status, cost=cost, n_samples=n_samples, samples=samples)

    def bind_find_trajectory(self, waypoints, stop_at=None, initial_state=None, limits=None, relax_heading=False,
                             sample_capacity=4096, **opts):
        """The arguments of mrs_tg_find_trajectory marshalled ONCE: returns (call, result) -- call() is the foreign call alone
        (what a C++ host pays per request; the ctypes structures and output arrays are reused), result() reads its outputs."""
        from .problem import DEFAULT_LIMITS
        wp = np.asarray(waypoints, dtype=np.float64).reshape(-1, 4)
        n = wp.shape[0]
        arr = (Waypoint * n)()
        for i in range(n):
            for k in range(4):
                arr[i].coords[k] = wp[i, k]
            arr[i].stop_at = int(bool(stop_at[i])) if stop_at is not None else 0
        init = None
        if initial_state is not None:
            init = InitialState()
            init.heading = float(initial_state["heading"])
            for k in range(4):
                init.velocity[k] = float(initial_state["velocity"][k])
                init.acceleration[k] = float(initial_state["acceleration"][k])
                init.jerk[k] = float(initial_state["jerk"][k])
        lim = np.ascontiguousarray(DEFAULT_LIMITS if limits is None else limits, dtype=np.float64)
        opts.setdefault("time_alloc_method", TIME_ALLOC_MELLINGER)
        opts.setdefault("sampling_dt", 0.2)
        opt = default_options(sample_capacity=sample_capacity, **opts)
        S = n - 1
        times = np.zeros(S)
        coeffs = np.zeros((S, N_DIM, N_COEFF))
        status = C.c_int32(0)
        ns = C.c_int32(0)
        samples = np.zeros((sample_capacity, N_DIM))
        fn, h, check = self._L.mrs_tg_find_trajectory, self._h, self._check
        a_init = C.byref(init) if init is not None else None
        a_lim, a_opt, a_relax, a_t, a_c = _np_ptr(lim), C.byref(opt), int(bool(relax_heading)), _np_ptr(times), _np_ptr(coeffs)
        a_st, a_ns, a_smp = C.cast(C.byref(status), C.c_void_p), C.cast(C.byref(ns), C.c_void_p), _np_ptr(samples)
        keep = (arr, init, lim, opt, times, coeffs, status, ns, samples)

        def call(_keep=keep):
            rc = fn(h, arr, n, a_init, a_lim, a_opt, a_relax, a_t, a_c, a_st, a_ns, a_smp)
            if rc:
                check(rc, "mrs_tg_find_trajectory")

        L = self._L

        def result():
            rej, baca = C.c_int32(0), C.c_double(0.0)
            L.mrs_tg_find_trajectory_info(h, C.byref(rej), C.byref(baca))
            return dict(times=times.copy(), coeffs=coeffs.copy(), status=status.value, n_samples=ns.value,
                        samples=samples[:min(ns.value, sample_capacity)].copy(), rejection=rej.value,
                        baca_total_time=baca.value,
                        message=(L.mrs_tg_last_error(h).decode() if rej.value else ""))
        return call, result

    def find_trajectory(self, waypoints, stop_at=None, initial_state=None, limits=None, relax_heading=False,
                        sample_capacity=4096, **opts):
        """findTrajectory() for one path (mrs_tg_find_trajectory)."""
        call, result = self.bind_find_trajectory(waypoints, stop_at, initial_state, limits, relax_heading, sample_capacity, **opts)
        call()
        return result()


class MultiContext:
    """Several devices (mrs_tg_multi): a batch is sharded over them, one host thread per device."""

    def __init__(self, devices):
        self._L = load_library()
        arr = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        rc = self._L.mrs_tg_create_multi(arr, len(devices), C.byref(h))
        if rc != 0:
            raise MrsTgError("mrs_tg_create_multi failed (%d): %s" % (rc, self._L.mrs_tg_last_error(None).decode()))
        self._h = h
        self.n_devices = self._L.mrs_tg_multi_n_devices(h)

    def close(self):
        if getattr(self, "_h", None):
            self._L.mrs_tg_destroy_multi(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def shard(self, seg_offsets):
        so = np.ascontiguousarray(seg_offsets, dtype=np.int32)
        out = np.zeros(so.size - 1, dtype=np.int32)
        rc = self._L.mrs_tg_multi_shard(self._h, so.size - 1, _np_ptr(so), _np_ptr(out))
        if rc != 0:
            raise MrsTgError("mrs_tg_multi_shard failed (%d)" % rc)
        return out

    def solve_batch(self, batch: Batch, seg_times=None, **opts):
        """Context.solve_batch over all devices (mrs_tg_multi_solve_batch)."""
        opt = default_options(derivative_to_optimize=batch.derivative_to_optimize, **opts)
        nS, P = batch.n_segments, batch.n_paths
        if seg_times is None:
            opt.estimate_times = 1
            t = np.zeros(nS)
        else:
            t = np.ascontiguousarray(seg_times, dtype=np.float64).copy()
        coeffs = np.zeros((nS, N_DIM, N_COEFF))
        status = np.zeros(P, dtype=np.int32)
        cost = np.zeros(P)
        sampling = opt.sampling_dt > 0
        n_samples = np.zeros(P, dtype=np.int32) if sampling else None
        samples = np.zeros((P, max(opt.sample_capacity, 1), N_DIM)) if sampling else None
        rc = self._L.mrs_tg_multi_solve_batch(self._h, P, _np_ptr(batch.seg_offsets), _np_ptr(batch.waypoints),
                                              _np_ptr(batch.fixed_mask), _np_ptr(batch.fixed_values), _np_ptr(batch.limits),
                                              C.byref(opt), _np_ptr(t), _np_ptr(coeffs), _np_ptr(status), _np_ptr(cost),
                                              _np_ptr(n_samples), _np_ptr(samples))
        if rc != 0:
            raise MrsTgError("mrs_tg_multi_solve_batch failed (%d): %s" % (rc, self._L.mrs_tg_multi_last_error(self._h).decode()))
        return dict(times=t, coeffs=coeffs, status=status, cost=cost, n_samples=n_samples, samples=samples)


_WAYPOINT_DTYPE = np.dtype([("coords", "<f8", (4,)), ("stop_at", "u1"), ("pad", "u1", (7,))])   # = mrs_tg_waypoint (40 bytes)


def _waypoint_array(paths, stop_flags=None):
    """the requests' waypoints as one mrs_tg_waypoint array + CSR offsets (numpy: a Python loop over 50 000 waypoints of 4096
    requests was a third of the wrapper's time)"""
    assert _WAYPOINT_DTYPE.itemsize == C.sizeof(Waypoint)
    pts = [np.asarray(p, dtype=np.float64).reshape(-1, 4) for p in paths]
    counts = np.array([q.shape[0] for q in pts], dtype=np.int64)
    off = np.zeros(len(pts) + 1, dtype=np.int32)
    off[1:] = np.cumsum(counts)
    arr = np.zeros(int(off[-1]), dtype=_WAYPOINT_DTYPE)
    if pts:
        arr["coords"] = np.concatenate(pts, axis=0) if len(pts) > 1 else pts[0]
    if stop_flags is not None:
        for pi, f in enumerate(stop_flags):
            if f is not None:
                arr["stop_at"][off[pi]:off[pi + 1]] = np.asarray(f, dtype=bool)
    return arr, off


def waypoint_trajectory_idxs(samples, waypoints):
    """getWaypointInTrajectoryIdxs (mrs_trajectory_generation.cpp:1461-1499) for one path: the sample indices at which the
    trajectory passes its waypoints (mrs_tg_waypoint_trajectory_idxs; host arithmetic, no device work)"""
    wp = np.ascontiguousarray(waypoints, dtype=np.float64)
    arr, _ = _waypoint_array([wp])
    smp = np.ascontiguousarray(samples, dtype=np.float64)
    idx = np.zeros(wp.shape[0] + 4, dtype=np.int32)
    k = load_library().mrs_tg_waypoint_trajectory_idxs(_np_ptr(smp), smp.shape[0], arr.ctypes.data_as(C.POINTER(Waypoint)),
                                                       wp.shape[0], _np_ptr(idx))
    return idx[:k].copy()


def optimize_paths(ctx, paths, limits=None, stop_flags=None, initial_states=None, relax_heading=None, policy=None,
                   sample_capacity=4096, out=None):
    """mrs_tg_optimize_paths: the reference's optimize() policy loop for a list of waypoint paths
    (each [n][4] array; its first row is the initial condition when initial_states[p] is given).
    out: the dict of a previous call with the same number of requests and capacity -- its arrays are written in place (a
    server that answers batch after batch keeps its response arrays: a fresh [P][capacity][4] array is 67 MB of page faults
    per 1024 requests at capacity 2048)."""
    from .problem import DEFAULT_LIMITS
    P = len(paths)
    arr, off = _waypoint_array(paths, stop_flags)
    lim = np.ascontiguousarray(np.tile(DEFAULT_LIMITS, (P, 1)) if limits is None else limits, dtype=np.float64).reshape(P, 9)
    inits = (InitialState * max(P, 1))()
    has = np.zeros(max(P, 1), dtype=np.uint8)
    if initial_states is not None:
        for p, st in enumerate(initial_states):
            if st is None:
                continue
            has[p] = 1
            inits[p].heading = float(st["heading"])
            for k in range(4):
                inits[p].velocity[k] = float(st["velocity"][k])
                inits[p].acceleration[k] = float(st["acceleration"][k])
                inits[p].jerk[k] = float(st["jerk"][k])
    relax = np.ascontiguousarray(relax_heading if relax_heading is not None else np.zeros(max(P, 1)), dtype=np.uint8)
    pol = policy or default_policy_options()
    if out is not None:
        success, ns, samples, maxdev, nwp, iters = (out[k] for k in ("success", "n_samples", "samples", "max_deviation",
                                                                      "n_waypoints", "iterations"))
        assert samples.shape == (P, sample_capacity, 4) and success.size == P
    else:
        success = np.zeros(P, dtype=np.int32)
        ns = np.zeros(P, dtype=np.int32)
        samples = np.zeros((P, sample_capacity, 4))
        maxdev = np.zeros(P)
        nwp = np.zeros(P, dtype=np.int32)
        iters = np.zeros(P, dtype=np.int32)
    rc = ctx._L.mrs_tg_optimize_paths(ctx._h, P, _np_ptr(off), arr.ctypes.data_as(C.POINTER(Waypoint)), inits, _np_ptr(has), _np_ptr(lim), _np_ptr(relax),
                                      C.byref(pol), int(sample_capacity), _np_ptr(success), _np_ptr(ns), _np_ptr(samples),
                                      _np_ptr(maxdev), _np_ptr(nwp), _np_ptr(iters))
    ctx._check(rc, "mrs_tg_optimize_paths")
    return dict(success=success, n_samples=ns, samples=samples, max_deviation=maxdev, n_waypoints=nwp, iterations=iters)


class Plan:
    """Batch structure analysed once; device-resident (torch) operands afterwards (mrs_tg_plan)."""

    def __init__(self, ctx: Context, seg_offsets):
        self.ctx = ctx
        self._L = ctx._L
        so = np.ascontiguousarray(seg_offsets, dtype=np.int32)
        h = C.c_void_p()
        ctx._check(self._L.mrs_tg_plan_create(ctx._h, so.size - 1, _np_ptr(so), C.byref(h)), "mrs_tg_plan_create")
        self._h = h
        self.seg_offsets = so
        self.n_paths = self._L.mrs_tg_plan_n_paths(h)
        self.n_segments = self._L.mrs_tg_plan_n_segments(h)
        self.max_segments = self._L.mrs_tg_plan_max_segments(h)
        order = np.zeros(max(self.n_paths, 1), dtype=np.int32)
        ctx._check(self._L.mrs_tg_plan_get_order(h, _np_ptr(order)), "mrs_tg_plan_get_order")
        self.order = order[:self.n_paths]
        self._bound = []

    def explain(self, opt, group_size=0):
        """The kernels a solve of this plan under `opt` WOULD launch, in order (mrs_tg_plan_explain: the launchers run dry);
        group_size 1 .. 16: one dispatch of the grouped issue carrying that many batches."""
        buf = (C.c_char_p * 32)()
        n = self._L.mrs_tg_plan_explain(self._h, C.byref(opt), int(group_size), buf, 32)
        if n < 0:
            self.ctx._check(n, "mrs_tg_plan_explain")
        return [buf[i].decode() for i in range(n)]

    def close(self):
        if getattr(self, "_h", None):
            for b in self._bound:
                self._L.mrs_tg_bound_solve_destroy(b)
            self._bound = []
            self._L.mrs_tg_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def block_doubles(self):
        return self._L.mrs_tg_plan_block_bytes(self._h) // 8

    def assemble(self, derivative, seg_times_dev, H_dev, Ainv_dev):
        self.ctx._check(self._L.mrs_tg_plan_assemble(self._h, int(derivative), _t_ptr(seg_times_dev), _t_ptr(H_dev),
                                                     _t_ptr(Ainv_dev)), "mrs_tg_plan_assemble")

    def blocks_to_segments(self, blocks):
        """Slot-major SoA block buffer (torch or numpy) -> numpy [sum S][10][10] in CSR segment order."""
        arr = blocks.detach().cpu().numpy() if hasattr(blocks, "detach") else np.asarray(blocks)
        P = self.n_paths
        soa = arr.reshape(self.max_segments, 100, P)
        out = np.zeros((self.n_segments, 10, 10))
        for q, p in enumerate(self.order):
            s0, s1 = int(self.seg_offsets[p]), int(self.seg_offsets[p + 1])
            out[s0:s1] = soa[:s1 - s0, :, q].reshape(s1 - s0, 10, 10)
        return out

    def solve(self, opt, fixed_mask, fixed_values, seg_times, coeffs, status, cost=None, waypoints=None, limits=None,
              n_samples=None, samples=None):
        self.ctx._check(self._L.mrs_tg_plan_solve(self._h, _t_ptr(waypoints), _t_ptr(fixed_mask), _t_ptr(fixed_values),
                                                  _t_ptr(limits), C.byref(opt), _t_ptr(seg_times), _t_ptr(coeffs),
                                                  _t_ptr(status), _t_ptr(cost), _t_ptr(n_samples), _t_ptr(samples)),
                        "mrs_tg_plan_solve")

    def bind_solve(self, opt, fixed_mask, fixed_values, seg_times, coeffs, status, cost=None, waypoints=None, limits=None,
                   n_samples=None, samples=None):
        """solve() with its arguments fixed once (mrs_tg_plan_bind_solve): returns a callable that enqueues the same solve
        again on the context's stream for one foreign call with one pointer -- a server that keeps several batches in flight
        on several streams issues steps faster than the GPU finishes them only if the per-call host cost is small.
        The tensors must stay alive and in place for as long as the callable is used."""
        keep = (opt, fixed_mask, fixed_values, seg_times, coeffs, status, cost, waypoints, limits, n_samples, samples)
        h = C.c_void_p()
        self.ctx._check(self._L.mrs_tg_plan_bind_solve(self._h, _t_ptr(waypoints), _t_ptr(fixed_mask), _t_ptr(fixed_values),
                                                       _t_ptr(limits), C.byref(opt), _t_ptr(seg_times), _t_ptr(coeffs),
                                                       _t_ptr(status), _t_ptr(cost), _t_ptr(n_samples), _t_ptr(samples),
                                                       C.byref(h)), "mrs_tg_plan_bind_solve")
        self._bound.append(h)
        fn, check = self._L.mrs_tg_bound_solve_launch, self.ctx._check

        def enqueue(_keep=keep, _h=h):
            rc = fn(_h)
            if rc:
                check(rc, "mrs_tg_bound_solve_launch")
        enqueue.handle = h
        enqueue.ctx = self.ctx
        return enqueue

    def cost_gradient(self, derivative, fixed_mask, fixed_values, seg_times, cost, grad):
        self.ctx._check(self._L.mrs_tg_plan_cost_gradient(self._h, int(derivative), _t_ptr(fixed_mask),
                                                          _t_ptr(fixed_values), _t_ptr(seg_times), _t_ptr(cost),
                                                          _t_ptr(grad)), "mrs_tg_plan_cost_gradient")

    def segment_maxima(self, coeffs, seg_times, maxima):
        self.ctx._check(self._L.mrs_tg_plan_segment_maxima(self._h, _t_ptr(coeffs), _t_ptr(seg_times), _t_ptr(maxima)),
                        "mrs_tg_plan_segment_maxima")

    def solve_vjp(self, derivative, fixed_mask, fixed_values, seg_times, coeffs, status, grad_coeffs=None, grad_cost=None,
                  grad_fixed_values=None, grad_seg_times=None):
        """mrs_tg_plan_solve_vjp: dL/dfixed_values and dL/dseg_times (device tensors, written) from dL/dcoeffs and dL/dcost
        (NULL = zero) at what a fixed-times solve returned (coeffs, status); asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_solve_vjp(self._h, int(derivative), _t_ptr(fixed_mask), _t_ptr(fixed_values),
                                                      _t_ptr(seg_times), _t_ptr(coeffs), _t_ptr(status), _t_ptr(grad_coeffs),
                                                      _t_ptr(grad_cost), _t_ptr(grad_fixed_values), _t_ptr(grad_seg_times)),
                        "mrs_tg_plan_solve_vjp")

    def segment_maxima_vjp(self, coeffs, seg_times, grad_maxima, grad_coeffs=None, grad_seg_times=None, argmax=None):
        """mrs_tg_plan_segment_maxima_vjp: dL/dcoeffs [sum S][4][10], dL/dseg_times [sum S] and the maximisers t* [sum S][3][3]
        in seconds (device tensors, written; None = not wanted, at least one given) from dL/dmaxima [sum S][3][3] at
        (coeffs, seg_times); asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_segment_maxima_vjp(self._h, _t_ptr(coeffs), _t_ptr(seg_times), _t_ptr(grad_maxima),
                                                               _t_ptr(grad_coeffs), _t_ptr(grad_seg_times), _t_ptr(argmax)),
                        "mrs_tg_plan_segment_maxima_vjp")

    def careful_count(self):
        n = C.c_int32(0)
        self.ctx._check(self._L.mrs_tg_plan_careful_count(self._h, C.byref(n)), "mrs_tg_plan_careful_count")
        return n.value

    def sample_states(self, coeffs, seg_times, sampling_dt, sample_capacity, n_samples, states):
        """sampleWholeTrajectory with all fields: states [n_paths][capacity][STATE_ORDERS][4] (device tensors)."""
        self.ctx._check(self._L.mrs_tg_plan_sample_states(self._h, _t_ptr(coeffs), _t_ptr(seg_times), float(sampling_dt),
                                                          int(sample_capacity), _t_ptr(n_samples), _t_ptr(states)),
                        "mrs_tg_plan_sample_states")

    def sample(self, coeffs, seg_times, sampling_dt, sample_capacity, n_samples, samples):
        """mrs_tg_plan_sample: positions + wrapped heading, samples [n_paths][capacity][4] (order 0 of sample_states)."""
        self.ctx._check(self._L.mrs_tg_plan_sample(self._h, _t_ptr(coeffs), _t_ptr(seg_times), float(sampling_dt),
                                                   int(sample_capacity), _t_ptr(n_samples), _t_ptr(samples)),
                        "mrs_tg_plan_sample")

    def sample_states_vjp(self, coeffs, seg_times, sampling_dt, sample_capacity, grad_states, status=None, grad_coeffs=None,
                          grad_seg_times=None, sample_segment=None, sample_time=None, n_samples=None):
        """mrs_tg_plan_sample_states_vjp: dL/dcoeffs [sum S][4][10] and dL/dseg_times [sum S] from dL/dsamples (grad_states
        [n_paths][capacity][n_orders][4], n_orders 1 or STATE_ORDERS; a 3-D tensor [n_paths][capacity][4] means 1; None when
        no gradient is wanted), and the walk's own sample_segment (int32) / sample_time [n_paths][capacity] and n_samples
        [n_paths] (device tensors, written; None = not wanted, at least one given); asynchronous on the context's stream."""
        n_orders = 1 if grad_states is None or grad_states.dim() == 3 else int(grad_states.shape[2])
        self.ctx._check(self._L.mrs_tg_plan_sample_states_vjp(self._h, _t_ptr(coeffs), _t_ptr(seg_times), float(sampling_dt),
                                                              int(sample_capacity), n_orders, _t_ptr(grad_states),
                                                              _t_ptr(status), _t_ptr(grad_coeffs), _t_ptr(grad_seg_times),
                                                              _t_ptr(sample_segment), _t_ptr(sample_time), _t_ptr(n_samples)),
                        "mrs_tg_plan_sample_states_vjp")

    def evaluate(self, coeffs, seg_times, query_times, states, query_segment=None, query_local_time=None):
        """mrs_tg_plan_evaluate: the state of every path at query_times [n_paths][n_queries] (seconds from the path's start; NaN
        = padding) into states [n_paths][n_queries][n_orders][4] (n_orders 1 or STATE_ORDERS; a 3-D tensor
        [n_paths][n_queries][4] means 1), with the segment (int32, -1 = out of range: a zero row) and the time in it
        [n_paths][n_queries] (device tensors, written; None = not wanted); asynchronous on the context's stream."""
        n_orders = 1 if states.dim() == 3 else int(states.shape[2])
        self.ctx._check(self._L.mrs_tg_plan_evaluate(self._h, _t_ptr(coeffs), _t_ptr(seg_times), _t_ptr(query_times),
                                                     int(query_times.shape[1]), n_orders, _t_ptr(states), _t_ptr(query_segment),
                                                     _t_ptr(query_local_time)), "mrs_tg_plan_evaluate")

    def evaluate_vjp(self, coeffs, seg_times, query_times, grad_states, status=None, grad_coeffs=None, grad_seg_times=None,
                     grad_query_times=None):
        """mrs_tg_plan_evaluate_vjp: dL/dcoeffs [sum S][4][10], dL/dseg_times [sum S] and dL/dquery_times [n_paths][n_queries]
        (device tensors, written; None = not wanted, at least one given) from dL/dstates (grad_states
        [n_paths][n_queries][n_orders][4]; a 3-D tensor means n_orders 1) at (coeffs, seg_times, query_times); asynchronous on the
        context's stream."""
        n_orders = 1 if grad_states.dim() == 3 else int(grad_states.shape[2])
        self.ctx._check(self._L.mrs_tg_plan_evaluate_vjp(self._h, _t_ptr(coeffs), _t_ptr(seg_times), _t_ptr(query_times),
                                                         int(query_times.shape[1]), n_orders, _t_ptr(grad_states), _t_ptr(status),
                                                         _t_ptr(grad_coeffs), _t_ptr(grad_seg_times), _t_ptr(grad_query_times)),
                        "mrs_tg_plan_evaluate_vjp")

    def path_deviation(self, samples, n_samples, waypoints, first_segment=True, status=None, deviation=None, cursor=None,
                       max_deviation=None, argmax=None, segment_max=None):
        """mrs_tg_plan_path_deviation: validateTrajectorySpatial's scan of samples [n_paths][capacity][4] (n_samples [n_paths]
        int32) against waypoints [sum V][4] into deviation [n_paths][capacity], cursor [n_paths][capacity] (int32, -1 behind the
        scanned rows), max_deviation [n_paths], argmax [n_paths] (int32) and segment_max [sum S] (device tensors, written; None =
        not wanted, at least one given); asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_path_deviation(self._h, _t_ptr(samples), _t_ptr(n_samples), int(samples.shape[1]),
                                                           _t_ptr(waypoints), 1 if first_segment else 0, _t_ptr(status),
                                                           _t_ptr(deviation), _t_ptr(cursor), _t_ptr(max_deviation),
                                                           _t_ptr(argmax), _t_ptr(segment_max)), "mrs_tg_plan_path_deviation")

    def path_deviation_vjp(self, samples, n_samples, waypoints, grad_deviation, status=None, grad_samples=None,
                           grad_waypoints=None):
        """mrs_tg_plan_path_deviation_vjp: dL/dsamples [n_paths][capacity][4] and dL/dwaypoints [sum V][4] (device tensors,
        written; None = not wanted, at least one given) from dL/ddeviation (grad_deviation [n_paths][capacity]), the cursors
        held fixed; asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_path_deviation_vjp(self._h, _t_ptr(samples), _t_ptr(n_samples),
                                                               int(samples.shape[1]), _t_ptr(waypoints), _t_ptr(status),
                                                               _t_ptr(grad_deviation), _t_ptr(grad_samples),
                                                               _t_ptr(grad_waypoints)), "mrs_tg_plan_path_deviation_vjp")

    @staticmethod
    def _offsets_dev(offsets, name, count_name, end, end_name, beside):
        """Offsets as a clearance step takes them: a device int32 tensor on `beside`'s device is the caller's statement and
        passes as it is; a host sequence or array is checked (_check_offsets: ValueError) and uploaded to that device -- a
        blocking copy, so a caller in a loop keeps the tensor this returns"""
        import torch
        if isinstance(offsets, torch.Tensor) and offsets.is_cuda:
            if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.numel() < 1 or not offsets.is_contiguous() or \
                    offsets.device != beside.device:
                raise ValueError("%s on the device must be a contiguous int32 tensor [%s + 1] on the device of its operands"
                                 % (name, count_name))
            return offsets
        if isinstance(offsets, torch.Tensor):
            offsets = offsets.numpy()
        g = torch.from_numpy(_check_offsets(offsets, name, end, end_name)).to(beside.device)
        torch.cuda.current_stream(beside.device).synchronize()
        return g

    def _group_offsets_dev(self, group_offsets, like):
        return self._offsets_dev(group_offsets, "group_offsets", "n_groups", self.n_paths, "n_paths", like)

    def mutual_clearance(self, samples, n_samples, group_offsets, first_step=None, status=None, z_scale=1.0, clearance=None,
                         partner=None, min_clearance=None, argmin=None):
        """mrs_tg_plan_mutual_clearance: per row of samples [n_paths][capacity][4] (n_samples [n_paths] int32) the distance to the
        nearest other path of the row's group at the same common step -- group_offsets [n_groups + 1] (a device int32 tensor, or
        a host sequence, which is checked and uploaded), first_step [n_paths] int32 (None: all 0), z_scale the weight of the
        vertical separation -- into clearance [n_paths][capacity] (+inf without a neighbour), partner [n_paths][capacity] (int32,
        the neighbour's path index, -1 where clearance is +inf), min_clearance [n_paths] and argmin [n_paths][2] (int32: row,
        partner) (device tensors, written; None = not wanted, at least one given); asynchronous on the context's stream."""
        g = self._group_offsets_dev(group_offsets, samples)
        self.ctx._check(self._L.mrs_tg_plan_mutual_clearance(self._h, _t_ptr(samples), _t_ptr(n_samples), int(samples.shape[1]),
                                                             _t_ptr(g), int(g.numel()) - 1, _t_ptr(first_step), _t_ptr(status),
                                                             float(z_scale), _t_ptr(clearance), _t_ptr(partner),
                                                             _t_ptr(min_clearance), _t_ptr(argmin)),
                        "mrs_tg_plan_mutual_clearance")

    def mutual_clearance_vjp(self, samples, n_samples, group_offsets, partner, grad_clearance, grad_samples, first_step=None,
                             status=None, z_scale=1.0):
        """mrs_tg_plan_mutual_clearance_vjp: dL/dsamples [n_paths][capacity][4] (grad_samples, written, zeros included) from
        dL/dclearance (grad_clearance [n_paths][capacity]) with the forward's partner [n_paths][capacity] (int32) held fixed;
        the other arguments are the forward's; asynchronous on the context's stream."""
        g = self._group_offsets_dev(group_offsets, samples)
        self.ctx._check(self._L.mrs_tg_plan_mutual_clearance_vjp(self._h, _t_ptr(samples), _t_ptr(n_samples),
                                                                 int(samples.shape[1]), _t_ptr(g), int(g.numel()) - 1,
                                                                 _t_ptr(first_step), _t_ptr(status), float(z_scale),
                                                                 _t_ptr(partner), _t_ptr(grad_clearance), _t_ptr(grad_samples)),
                        "mrs_tg_plan_mutual_clearance_vjp")

    def _set_offsets_dev(self, set_offsets, obstacles):
        return self._offsets_dev(set_offsets, "set_offsets", "n_sets", int(obstacles.shape[0]), "n_obstacles", obstacles)

    def _obstacle_operands(self, samples, n_samples, obstacles, set_offsets, path_set, status):
        """the operand checks the two obstacle calls share -> (set_offsets on the device, capacity)"""
        import torch
        P = self.n_paths
        _check_operand("samples", samples, torch.float64, (P, None, N_DIM))
        _check_operand("n_samples", n_samples, torch.int32, (P,), samples)
        _check_operand("obstacles", obstacles, torch.float64, (None, 4), samples)
        _check_operand("path_set", path_set, torch.int32, (P,), samples, optional=True)
        _check_operand("status", status, torch.int32, (P,), samples, optional=True)
        return self._set_offsets_dev(set_offsets, obstacles), int(samples.shape[1])

    def obstacle_clearance(self, samples, n_samples, obstacles, set_offsets, path_set=None, status=None, z_scale=1.0,
                           clearance=None, nearest=None, min_clearance=None, argmin=None):
        """mrs_tg_plan_obstacle_clearance: per row of samples [n_paths][capacity][4] (n_samples [n_paths] int32) the signed
        distance to the nearest obstacle of the path's set -- obstacles [n_obstacles][4] = (x, y, z, radius), set_offsets
        [n_sets + 1] (a device int32 tensor, or a host sequence, which is checked and uploaded), path_set [n_paths] int32 (None:
        every path sees set 0), z_scale the weight of the vertical separation -- into clearance [n_paths][capacity] (+inf
        without an obstacle; negative inside a sphere), nearest [n_paths][capacity] (int32, the obstacle's index in the whole
        array, -1 where clearance is +inf), min_clearance [n_paths] and argmin [n_paths][2] (int32: row, obstacle) (device
        tensors, written; None = not wanted, at least one given); asynchronous on the context's stream."""
        import torch
        g, cap = self._obstacle_operands(samples, n_samples, obstacles, set_offsets, path_set, status)
        P = self.n_paths
        _check_operand("clearance", clearance, torch.float64, (P, cap), samples, optional=True)
        _check_operand("nearest", nearest, torch.int32, (P, cap), samples, optional=True)
        _check_operand("min_clearance", min_clearance, torch.float64, (P,), samples, optional=True)
        _check_operand("argmin", argmin, torch.int32, (P, 2), samples, optional=True)
        self.ctx._check(self._L.mrs_tg_plan_obstacle_clearance(self._h, _t_ptr(samples), _t_ptr(n_samples), cap, _t_ptr(obstacles),
                                                               int(obstacles.shape[0]), _t_ptr(g), int(g.numel()) - 1,
                                                               _t_ptr(path_set), _t_ptr(status), float(z_scale),
                                                               _t_ptr(clearance), _t_ptr(nearest), _t_ptr(min_clearance),
                                                               _t_ptr(argmin)),
                        "mrs_tg_plan_obstacle_clearance")

    def obstacle_clearance_vjp(self, samples, n_samples, obstacles, set_offsets, nearest, grad_clearance, grad_samples,
                               path_set=None, status=None, z_scale=1.0):
        """mrs_tg_plan_obstacle_clearance_vjp: dL/dsamples [n_paths][capacity][4] (grad_samples, written, zeros included) from
        dL/dclearance (grad_clearance [n_paths][capacity]) with the forward's nearest [n_paths][capacity] (int32) held fixed;
        the other arguments are the forward's; asynchronous on the context's stream."""
        import torch
        g, cap = self._obstacle_operands(samples, n_samples, obstacles, set_offsets, path_set, status)
        P = self.n_paths
        _check_operand("nearest", nearest, torch.int32, (P, cap), samples)
        _check_operand("grad_clearance", grad_clearance, torch.float64, (P, cap), samples)
        _check_operand("grad_samples", grad_samples, torch.float64, (P, cap, N_DIM), samples)
        self.ctx._check(self._L.mrs_tg_plan_obstacle_clearance_vjp(self._h, _t_ptr(samples), _t_ptr(n_samples), cap,
                                                                   _t_ptr(obstacles), int(obstacles.shape[0]), _t_ptr(g),
                                                                   int(g.numel()) - 1, _t_ptr(path_set), _t_ptr(status),
                                                                   float(z_scale), _t_ptr(nearest), _t_ptr(grad_clearance),
                                                                   _t_ptr(grad_samples)),
                        "mrs_tg_plan_obstacle_clearance_vjp")

    def _field_operands(self, samples, n_samples, fields, geometry, path_field, status):
        """the operand checks the two field calls share -> (the C geometry, capacity)"""
        import torch
        P = self.n_paths
        _check_operand("samples", samples, torch.float64, (P, None, N_DIM))
        _check_operand("n_samples", n_samples, torch.int32, (P,), samples)
        _check_operand("fields", fields, torch.float64, (None, None, None, None), samples)
        check_field_geometry(fields.shape, geometry)
        _check_operand("path_field", path_field, torch.int32, (P,), samples, optional=True)
        _check_operand("status", status, torch.int32, (P,), samples, optional=True)
        return geometry.as_struct(), int(samples.shape[1])

    def field_clearance(self, samples, n_samples, fields, geometry, path_field=None, status=None, outside_value=float("inf"),
                        clearance=None, cell=None, gradient=None, min_clearance=None, argmin=None):
        """mrs_tg_plan_field_clearance: per row of samples [n_paths][capacity][4] (n_samples [n_paths] int32) the trilinear
        interpolant of the voxel grid of signed distances the path sees -- fields [n_fields][nz][ny][nx] float64 with geometry
        (an api.FieldGeometry, checked: ValueError), path_field [n_paths] int32 (None: every path sees grid 0), outside_value
        for a live row outside the grid -- into clearance [n_paths][capacity] (+inf behind a path's rows and without a grid),
        cell [n_paths][capacity] (int32, the low corner's index in the whole fields array, -1 where there is none), gradient
        [n_paths][capacity][4] (the field's gradient, column 3 zero), min_clearance [n_paths] and argmin [n_paths][2] (int32:
        row, cell) (device tensors, written; None = not wanted, at least one given); asynchronous on the context's stream."""
        import torch
        g, cap = self._field_operands(samples, n_samples, fields, geometry, path_field, status)
        P = self.n_paths
        _check_operand("clearance", clearance, torch.float64, (P, cap), samples, optional=True)
        _check_operand("cell", cell, torch.int32, (P, cap), samples, optional=True)
        _check_operand("gradient", gradient, torch.float64, (P, cap, N_DIM), samples, optional=True)
        _check_operand("min_clearance", min_clearance, torch.float64, (P,), samples, optional=True)
        _check_operand("argmin", argmin, torch.int32, (P, 2), samples, optional=True)
        self.ctx._check(self._L.mrs_tg_plan_field_clearance(self._h, _t_ptr(samples), _t_ptr(n_samples), cap, _t_ptr(fields),
                                                            C.byref(g), _t_ptr(path_field), _t_ptr(status), float(outside_value),
                                                            _t_ptr(clearance), _t_ptr(cell), _t_ptr(gradient),
                                                            _t_ptr(min_clearance), _t_ptr(argmin)),
                        "mrs_tg_plan_field_clearance")

    def field_clearance_vjp(self, samples, n_samples, fields, geometry, cell, grad_clearance, grad_samples, path_field=None,
                            status=None):
        """mrs_tg_plan_field_clearance_vjp: dL/dsamples [n_paths][capacity][4] (grad_samples, written, zeros included) from
        dL/dclearance (grad_clearance [n_paths][capacity]) with the forward's cell [n_paths][capacity] (int32) held fixed; the
        other arguments are the forward's; asynchronous on the context's stream."""
        import torch
        g, cap = self._field_operands(samples, n_samples, fields, geometry, path_field, status)
        P = self.n_paths
        _check_operand("cell", cell, torch.int32, (P, cap), samples)
        _check_operand("grad_clearance", grad_clearance, torch.float64, (P, cap), samples)
        _check_operand("grad_samples", grad_samples, torch.float64, (P, cap, N_DIM), samples)
        self.ctx._check(self._L.mrs_tg_plan_field_clearance_vjp(self._h, _t_ptr(samples), _t_ptr(n_samples), cap, _t_ptr(fields),
                                                                C.byref(g), _t_ptr(path_field), _t_ptr(status), _t_ptr(cell),
                                                                _t_ptr(grad_clearance), _t_ptr(grad_samples)),
                        "mrs_tg_plan_field_clearance_vjp")

    def estimate_times(self, waypoints, limits, seg_times):
        """mrs_tg_plan_estimate_times: the Euclidean segment-time estimate of waypoints [sum V][4] under limits [n_paths][9] into
        seg_times [sum S] (device tensors; seg_times written) -- the times a solve with estimate_times = 1 starts from, in the
        same bits; asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_estimate_times(self._h, _t_ptr(waypoints), _t_ptr(limits), _t_ptr(seg_times)),
                        "mrs_tg_plan_estimate_times")

    def estimate_times_vjp(self, waypoints, limits, grad_seg_times=None, grad_waypoints=None, grad_limits=None, term=None):
        """mrs_tg_plan_estimate_times_vjp: dL/dwaypoints [sum V][4], dL/dlimits [n_paths][9] and the term of every segment
        [sum S] (int32, ESTIMATE_TERM_*) (device tensors, written; None = not wanted, at least one given) from dL/dseg_times
        (grad_seg_times [sum S]; the gradients need it, term alone does not), every branch of the forward held fixed;
        asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_estimate_times_vjp(self._h, _t_ptr(waypoints), _t_ptr(limits),
                                                               _t_ptr(grad_seg_times), _t_ptr(grad_waypoints),
                                                               _t_ptr(grad_limits), _t_ptr(term)),
                        "mrs_tg_plan_estimate_times_vjp")

    def waypoint_passage(self, samples, n_samples, waypoints, wp_offsets=None, status=None, index=None, count=None, miss=None,
                         fraction=None):
        """mrs_tg_plan_waypoint_passage: getWaypointInTrajectoryIdxs' scan of samples [n_paths][capacity][4] (n_samples
        [n_paths] int32) for the waypoints [sum W][4] that wp_offsets [n_paths + 1] (int32 device tensor; None = the plan's own
        vertices) gives every path, into index [sum W] (int32, -1 from the first waypoint not reached on), count [n_paths]
        (int32), miss [sum W] and fraction [sum W] (device tensors, written; None = not wanted, at least one given): waypoint k
        is passed at (index[k] + fraction[k]) * sampling_dt; asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_waypoint_passage(self._h, _t_ptr(samples), _t_ptr(n_samples), int(samples.shape[1]),
                                                             _t_ptr(wp_offsets), _t_ptr(waypoints), _t_ptr(status),
                                                             _t_ptr(index), _t_ptr(count), _t_ptr(miss), _t_ptr(fraction)),
                        "mrs_tg_plan_waypoint_passage")

    def waypoint_passage_vjp(self, samples, n_samples, waypoints, grad_miss=None, grad_fraction=None, wp_offsets=None,
                             status=None, grad_samples=None, grad_waypoints=None):
        """mrs_tg_plan_waypoint_passage_vjp: dL/dsamples [n_paths][capacity][4] and dL/dwaypoints [sum W][4] (device tensors,
        written; None = not wanted, at least one given) from dL/dmiss and dL/dfraction (grad_miss, grad_fraction [sum W]; None =
        zero), the indices held fixed; asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_waypoint_passage_vjp(self._h, _t_ptr(samples), _t_ptr(n_samples),
                                                                 int(samples.shape[1]), _t_ptr(wp_offsets), _t_ptr(waypoints),
                                                                 _t_ptr(status), _t_ptr(grad_miss), _t_ptr(grad_fraction),
                                                                 _t_ptr(grad_samples), _t_ptr(grad_waypoints)),
                        "mrs_tg_plan_waypoint_passage_vjp")

    def estimate_times_baca(self, waypoints, limits, seg_times):
        """mrs_tg_plan_estimate_times_baca: the Baca segment-time estimate (estimateSegmentTimesBaca) of waypoints [sum V][4]
        under limits [n_paths][9] (entries 0 .. 7 are read) into seg_times [sum S] (device tensors; seg_times written) -- within
        1e-13 of the host's estimate_times_baca, not in its bits; asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_estimate_times_baca(self._h, _t_ptr(waypoints), _t_ptr(limits), _t_ptr(seg_times)),
                        "mrs_tg_plan_estimate_times_baca")

    def estimate_times_baca_vjp(self, waypoints, limits, grad_seg_times=None, grad_waypoints=None, grad_limits=None, flags=None):
        """mrs_tg_plan_estimate_times_baca_vjp: dL/dwaypoints [sum V][4], dL/dlimits [n_paths][9] and the branches of every
        segment [sum S] (int32, bits BACA_*) (device tensors, written; None = not wanted, at least one given) from dL/dseg_times
        (grad_seg_times [sum S]; the gradients need it, flags alone do not), every branch of the forward held fixed;
        asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_estimate_times_baca_vjp(self._h, _t_ptr(waypoints), _t_ptr(limits),
                                                                    _t_ptr(grad_seg_times), _t_ptr(grad_waypoints),
                                                                    _t_ptr(grad_limits), _t_ptr(flags)),
                        "mrs_tg_plan_estimate_times_baca_vjp")

    def length_gate(self, seg_times, n_samples, sampling_dt, max_factor=3.0, min_factor=0.33, status=None, total=None,
                    verdict=None):
        """mrs_tg_plan_length_gate: per path the total of seg_times [sum S] (total [n_paths], written) and the nodelet's verdict
        on n_samples [n_paths] (int32, the raw count a solve leaves) * sampling_dt against it (verdict [n_paths] int32, written:
        FIND_REJECTED_CODE first when status [n_paths] is given and rejects, then FIND_REJECTED_TOO_LONG / _TOO_SHORT /
        FIND_ACCEPTED; a factor <= 0 switches its side off); at least one output; asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_length_gate(self._h, _t_ptr(seg_times), _t_ptr(n_samples), float(sampling_dt),
                                                        float(max_factor), float(min_factor), _t_ptr(status), _t_ptr(total),
                                                        _t_ptr(verdict)), "mrs_tg_plan_length_gate")

    def unwrap_headings(self, waypoints, waypoints_out=None):
        """mrs_tg_plan_unwrap_headings: the headings of waypoints [sum V][4] unwrapped along every path (vertex v against the
        unwrapped vertex v - 1) into waypoints_out (device tensors; None = in place), x, y, z copied, in the host's bits;
        asynchronous on the context's stream."""
        out = waypoints if waypoints_out is None else waypoints_out
        self.ctx._check(self._L.mrs_tg_plan_unwrap_headings(self._h, _t_ptr(waypoints), _t_ptr(out)),
                        "mrs_tg_plan_unwrap_headings")

    def fallback_sample(self, waypoints, seg_times, sampling_dt, sample_capacity, n_samples, samples, stop_at=None,
                        stopping_time=2.0, seg_first_row=None):
        """mrs_tg_plan_fallback_sample: findTrajectoryFallback's rows -- constant-rate interpolation of the RAW waypoints
        [sum V][4] on seg_times [sum S], a dwell of round(stopping_time / sampling_dt) repeated rows where stop_at [sum V]
        (uint8, optional) is set -- into samples [n_paths][sample_capacity][4] and n_samples [n_paths] int32 (the count, or
        sample_capacity + 1 when it does not fit; rows from the count on are not written); seg_first_row [sum S] int32
        (optional) gets the row every segment starts at.  Device tensors; asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_fallback_sample(self._h, _t_ptr(waypoints), _t_ptr(stop_at), _t_ptr(seg_times),
                                                            float(sampling_dt), float(stopping_time), int(sample_capacity),
                                                            _t_ptr(n_samples), _t_ptr(samples), _t_ptr(seg_first_row)),
                        "mrs_tg_plan_fallback_sample")

    def fallback_sample_vjp(self, seg_times, sampling_dt, sample_capacity, grad_samples, grad_waypoints, stop_at=None,
                            stopping_time=2.0):
        """mrs_tg_plan_fallback_sample_vjp: dL/dwaypoints [sum V][4] (written, zeros included) from dL/dsamples
        [n_paths][sample_capacity][4] with the forward's counts held fixed (seg_times gets no gradient), every sum in a
        stated order; asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_fallback_sample_vjp(self._h, _t_ptr(stop_at), _t_ptr(seg_times), float(sampling_dt),
                                                                float(stopping_time), int(sample_capacity),
                                                                _t_ptr(grad_samples), _t_ptr(grad_waypoints)),
                        "mrs_tg_plan_fallback_sample_vjp")

    def preprocess_path(self, waypoints, vertex_offsets, waypoints_out, min_waypoint_distance=0.05, stop_at=None,
                        straightener_enabled=False, straightener_max_deviation=0.0, straightener_max_hdg_deviation=0.0,
                        stop_at_out=None, source=None):
        """mrs_tg_plan_preprocess_path: preprocessPath's thinning of waypoints [sum V][4] (raw headings; stop_at [sum V] uint8,
        optional) into a PACKED batch: vertex_offsets [n_paths + 1] int32, waypoints_out [sum V][4] and, optional, stop_at_out
        [sum V] uint8 and source [sum V] int32 (the input vertex every output vertex copies) -- rows below
        vertex_offsets[n_paths] are written, the rest is not; device tensors, asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_preprocess_path(self._h, _t_ptr(waypoints), _t_ptr(stop_at),
                                                            float(min_waypoint_distance), 1 if straightener_enabled else 0,
                                                            float(straightener_max_deviation),
                                                            float(straightener_max_hdg_deviation), _t_ptr(vertex_offsets),
                                                            _t_ptr(waypoints_out), _t_ptr(stop_at_out), _t_ptr(source)),
                        "mrs_tg_plan_preprocess_path")

    def insert_midpoints(self, waypoints, segment_max, max_deviation, vertex_offsets, waypoints_out, first_segment=True,
                         stop_at=None, active=None, stop_at_out=None, source=None, inserted=None):
        """mrs_tg_plan_insert_midpoints: a mid-point into every segment whose segment_max [sum S] (Plan.path_deviation's)
        exceeds max_deviation, by the reference's rule (:739-753), for the paths active [n_paths] uint8 (optional: all) marks;
        the others are copied.  Packed as preprocess_path packs: vertex_offsets [n_paths + 1] int32, waypoints_out
        [sum V + sum S][4] and, optional, stop_at_out uint8, source int32, inserted uint8 [sum V + sum S]; device tensors,
        asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_insert_midpoints(self._h, _t_ptr(waypoints), _t_ptr(stop_at), _t_ptr(segment_max),
                                                             float(max_deviation), 1 if first_segment else 0, _t_ptr(active),
                                                             _t_ptr(vertex_offsets), _t_ptr(waypoints_out), _t_ptr(stop_at_out),
                                                             _t_ptr(source), _t_ptr(inserted)),
                        "mrs_tg_plan_insert_midpoints")

    def path_edit_vjp(self, vertex_offsets, source, grad_waypoints_edited, grad_waypoints, inserted=None):
        """mrs_tg_plan_path_edit_vjp: dL/dwaypoints [sum V][4] of this (the input) plan's vertices (written, zeros included) from
        dL/d(edited waypoints) [sum V'][4] and what the edit step wrote (vertex_offsets, source, inserted; inserted None after
        thinning), every sum in a stated order; asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_path_edit_vjp(self._h, _t_ptr(vertex_offsets), _t_ptr(source), _t_ptr(inserted),
                                                          _t_ptr(grad_waypoints_edited), _t_ptr(grad_waypoints)),
                        "mrs_tg_plan_path_edit_vjp")

    def travel_heading(self, samples, n_samples, samples_out=None, status=None, min_step=0.05, source=None):
        """mrs_tg_plan_travel_heading: getTrajectoryReference's override_heading_atan2 on samples [n_paths][capacity][4]
        (n_samples [n_paths] int32): the heading of the rows 0 .. n-2 becomes atan2 of the step to the next row, a row that moves
        less than min_step keeping the heading of the row in front; row n-1 keeps its own.  samples_out None = in place (only
        those headings are stored), else rows 0 .. n-1 are written whole; source [n_paths][capacity] int32 (optional) gets the
        row whose step gave a row's heading, -1 for row n-1.  A path with status [n_paths] <= 0 (optional) is not touched.
        Device tensors; asynchronous on the context's stream."""
        out = samples if samples_out is None else samples_out
        self.ctx._check(self._L.mrs_tg_plan_travel_heading(self._h, _t_ptr(samples), _t_ptr(n_samples), int(samples.shape[1]),
                                                           _t_ptr(status), float(min_step), _t_ptr(out), _t_ptr(source)),
                        "mrs_tg_plan_travel_heading")

    def travel_heading_vjp(self, samples, n_samples, grad_out, grad_samples, status=None, min_step=0.05):
        """mrs_tg_plan_travel_heading_vjp: dL/dsamples [n_paths][capacity][4] of the INPUT rows (written, zeros included) from
        dL/d(output rows) (grad_out [n_paths][capacity][4]), the sources recomputed from samples and held fixed, every sum in a
        stated order; asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_travel_heading_vjp(self._h, _t_ptr(samples), _t_ptr(n_samples),
                                                               int(samples.shape[1]), _t_ptr(status), float(min_step),
                                                               _t_ptr(grad_out), _t_ptr(grad_samples)),
                        "mrs_tg_plan_travel_heading_vjp")

    def initial_condition(self, flags, tracker, tracker_age, uav_pose, takeoff_height, path_time_offset, vertex_offsets,
                          prediction, n_pred, decision, sample_offset, initial):
        """mrs_tg_plan_initial_condition: prepareInitialCondition and the first-waypoint rule for every path, one lane per path.
        [n_paths] each: flags int32 (IC_FLAG_*), tracker [.][4][4] (pose, velocity, acceleration, jerk; xyz + the heading's),
        tracker_age, uav_pose [.][4], path_time_offset, n_pred int32; vertex_offsets [n_paths + 1] int32 of the requested
        waypoints; prediction: the four arrays [.][pred_capacity][4] position, velocity, acceleration, jerk.  Written: decision
        int32 (IC_*), sample_offset int32 (k) and initial [.][4][4] (row 0 the prepended waypoint, rows 1 .. 3 the derivatives;
        zeros where IC_PREPEND is not set).  Device tensors; asynchronous on the context's stream."""
        pos, vel, acc, jerk = prediction
        self.ctx._check(self._L.mrs_tg_plan_initial_condition(
            self._h, _t_ptr(flags), _t_ptr(tracker), _t_ptr(tracker_age), _t_ptr(uav_pose), float(takeoff_height),
            _t_ptr(path_time_offset), _t_ptr(vertex_offsets), _t_ptr(pos), _t_ptr(vel), _t_ptr(acc), _t_ptr(jerk), _t_ptr(n_pred),
            int(pos.shape[1]), _t_ptr(decision), _t_ptr(sample_offset), _t_ptr(initial)), "mrs_tg_plan_initial_condition")

    def initial_condition_vjp(self, decision, sample_offset, grad_initial, grad_tracker, grad_uav, grad_prediction):
        """mrs_tg_plan_initial_condition_vjp: from grad_initial [n_paths][4][4], the decision and k held fixed, grad_tracker
        [.][4][4], grad_uav [.][4] and the four grad_prediction arrays [.][pred_capacity][4] (row k of each; all written, zeros
        included); asynchronous on the context's stream."""
        pos, vel, acc, jerk = grad_prediction
        self.ctx._check(self._L.mrs_tg_plan_initial_condition_vjp(
            self._h, _t_ptr(decision), _t_ptr(sample_offset), _t_ptr(grad_initial), int(pos.shape[1]), _t_ptr(grad_tracker),
            _t_ptr(grad_uav), _t_ptr(pos), _t_ptr(vel), _t_ptr(acc), _t_ptr(jerk)), "mrs_tg_plan_initial_condition_vjp")

    def prepend_initial_condition(self, vertex_offsets, waypoints, decision, initial, vertex_offsets_out, waypoints_out,
                                  stop_at=None, stop_at_out=None, source=None):
        """mrs_tg_plan_prepend_initial_condition: the first requested waypoint goes where decision has IC_DROP_FIRST, row 0 of
        initial [n_paths][4][4] comes in front (stop_at 0) where it has IC_PREPEND.  waypoints [n_vertices][4] addressed by
        vertex_offsets [n_paths + 1] int32 (a path may have no vertex or one); packed as preprocess_path packs:
        vertex_offsets_out [n_paths + 1] int32, waypoints_out [n_vertices + n_paths][4] and, optional, stop_at_out uint8 and
        source int32 (the input vertex, -1 for the prepended row).  Device tensors; asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_prepend_initial_condition(
            self._h, _t_ptr(vertex_offsets), int(waypoints.shape[0]), _t_ptr(waypoints), _t_ptr(stop_at), _t_ptr(decision),
            _t_ptr(initial), _t_ptr(vertex_offsets_out), _t_ptr(waypoints_out), _t_ptr(stop_at_out), _t_ptr(source)),
            "mrs_tg_plan_prepend_initial_condition")

    def prepend_initial_condition_vjp(self, vertex_offsets, decision, vertex_offsets_edited, grad_waypoints_edited,
                                      grad_waypoints, grad_initial_row):
        """mrs_tg_plan_prepend_initial_condition_vjp: grad_waypoints [n_vertices][4] of the requested vertices (a dropped one
        gets zeros) and grad_initial_row [n_paths][4] (row 0 of the state block) from grad_waypoints_edited [n_edited][4];
        asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_prepend_initial_condition_vjp(
            self._h, _t_ptr(vertex_offsets), int(grad_waypoints.shape[0]), _t_ptr(decision), _t_ptr(vertex_offsets_edited),
            int(grad_waypoints_edited.shape[0]), _t_ptr(grad_waypoints_edited), _t_ptr(grad_waypoints), _t_ptr(grad_initial_row)),
            "mrs_tg_plan_prepend_initial_condition_vjp")

    def splice_prediction(self, samples, n_samples, decision, sample_offset, prediction_age, pred_position, n_pred,
                          samples_out=None, n_samples_out=None, status=None, status_out=None):
        """mrs_tg_plan_splice_prediction: where a path is live, IC_FROM_FUTURE is set and k = sample_offset exceeds the
        prediction's current index, prediction rows 0 .. k-1 go in front of the n rows of samples [n_paths][capacity][4] and
        n_samples_out = n + k (reported, nothing written, when that exceeds the capacity).  samples_out / n_samples_out None =
        in place.  status_out [n_paths] int32 (optional) passes status on, -2 where the prediction has fewer than k rows.
        Device tensors; asynchronous on the context's stream."""
        out = samples if samples_out is None else samples_out
        n_out = n_samples if n_samples_out is None else n_samples_out
        self.ctx._check(self._L.mrs_tg_plan_splice_prediction(
            self._h, _t_ptr(samples), _t_ptr(n_samples), int(samples.shape[1]), _t_ptr(status), _t_ptr(decision),
            _t_ptr(sample_offset), _t_ptr(prediction_age), _t_ptr(pred_position), _t_ptr(n_pred), int(pred_position.shape[1]),
            _t_ptr(out), _t_ptr(n_out), _t_ptr(status_out)), "mrs_tg_plan_splice_prediction")

    def splice_prediction_vjp(self, n_samples, decision, sample_offset, prediction_age, n_pred, grad_out, grad_samples,
                              grad_pred_position, status=None):
        """mrs_tg_plan_splice_prediction_vjp: grad_samples [n_paths][capacity][4] and grad_pred_position
        [n_paths][pred_capacity][4] (all written, zeros included) from grad_out [n_paths][capacity][4]; n_samples and status are
        the forward's inputs; asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_splice_prediction_vjp(
            self._h, _t_ptr(n_samples), int(grad_out.shape[1]), _t_ptr(status), _t_ptr(decision), _t_ptr(sample_offset),
            _t_ptr(prediction_age), _t_ptr(n_pred), int(grad_pred_position.shape[1]), _t_ptr(grad_out), _t_ptr(grad_samples),
            _t_ptr(grad_pred_position)), "mrs_tg_plan_splice_prediction_vjp")

    def request_vertices(self, waypoints, waypoints_out=None, fixed_mask=None, fixed_values=None, stop_at=None, has_state=None,
                         state=None, derivative_to_optimize=4):
        """mrs_tg_plan_request_vertices: the vertices findTrajectory builds (:923-977) from the RAW waypoints [sum V][4] -- the
        headings unwrapped along every path, the chain starting from the heading of state [n_paths][4][4] (row 0 column 3; rows
        1 .. 3 velocity, acceleration, jerk) where has_state [n_paths] uint8 says the path has one, else from its first raw
        heading -- into waypoints_out [sum V][4] (may be waypoints), fixed_mask [sum V][5] uint8 and fixed_values [sum V][5][4]
        (each optional, not all None): positions fixed everywhere, derivatives 1 .. d at the ends, 1 .. 3 (the state's rows) at
        the first vertex of a path with a state, 1 .. 3 (zero) at a stop_at [sum V] uint8 vertex between the ends.  Device
        tensors; asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_request_vertices(
            self._h, _t_ptr(waypoints), _t_ptr(stop_at), _t_ptr(has_state), _t_ptr(state), int(derivative_to_optimize),
            _t_ptr(waypoints_out), _t_ptr(fixed_mask), _t_ptr(fixed_values)), "mrs_tg_plan_request_vertices")

    def request_vertices_vjp(self, grad_waypoints=None, grad_fixed_values=None, grad_waypoints_out=None, grad_state=None,
                             has_state=None):
        """mrs_tg_plan_request_vertices_vjp: grad_waypoints_out [sum V][4] = grad_waypoints + grad_fixed_values[:, 0] (an upstream
        that is None counts as zero, not both) and grad_state [n_paths][4][4] (rows 1 .. 3 from the first vertex's value rows
        where has_state, zeros elsewhere); all written, zeros included; asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_request_vertices_vjp(
            self._h, _t_ptr(has_state), _t_ptr(grad_waypoints), _t_ptr(grad_fixed_values), _t_ptr(grad_waypoints_out),
            _t_ptr(grad_state)), "mrs_tg_plan_request_vertices_vjp")

    def request_limits(self, constraints, limits=None, branch=None, override=None, flags=None, has_state=None, state=None,
                       fallback=False, speed_factor=1.0, accel_factor=1.0):
        """mrs_tg_plan_request_limits: limits [n_paths][9] (v, a, j x horizontal, vertical, heading) and branch [n_paths] int32
        (LIM_*) from constraints [n_paths][12] (horizontal v, a, j; vertical ascending / descending v, a, j pairwise; heading v,
        a, j), override [n_paths][6] (v h, v; a h, v; j h, v) with flags [n_paths] int32 (REQ_*; flags needs override) and the
        state as request_vertices takes it: the smaller of a vertical pair, the override where can_change holds against the
        state (fallback: always), the relaxed heading, and with fallback the speed / acceleration factors on entries 0, 1 / 3, 4.
        Device tensors; asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_request_limits(
            self._h, _t_ptr(constraints), _t_ptr(override), _t_ptr(flags), _t_ptr(has_state), _t_ptr(state), int(bool(fallback)),
            float(speed_factor), float(accel_factor), _t_ptr(limits), _t_ptr(branch)), "mrs_tg_plan_request_limits")

    def request_limits_vjp(self, branch, grad_limits, grad_constraints=None, grad_override=None, fallback=False, speed_factor=1.0,
                           accel_factor=1.0):
        """mrs_tg_plan_request_limits_vjp: grad_constraints [n_paths][12] and grad_override [n_paths][6] (all written, zeros
        included) from grad_limits [n_paths][9], the branch word held fixed; fallback and the factors are the forward's;
        asynchronous on the context's stream."""
        self.ctx._check(self._L.mrs_tg_plan_request_limits_vjp(
            self._h, _t_ptr(branch), int(bool(fallback)), float(speed_factor), float(accel_factor), _t_ptr(grad_limits),
            _t_ptr(grad_constraints), _t_ptr(grad_override)), "mrs_tg_plan_request_limits_vjp")


class RoundRobin:
    """The issue loop of a host that keeps several batches in flight, in C (mrs_tg_bound_solve_launch_many): launch k goes to
    calls[k % len(calls)], each a callable returned by Plan.bind_solve (one per context + stream)."""

    def __init__(self, calls, threads=1, grouped=False):
        """grouped: mrs_tg_bound_solve_launch_group -- the launches of a round go out as ONE dispatch (bound solves of one
        plan, fixed times, default solve)."""
        self._calls = list(calls)
        self._arr = (C.c_void_p * len(self._calls))(*[c.handle for c in self._calls])
        self._fn = load_library().mrs_tg_bound_solve_launch_many_mt
        self._group = load_library().mrs_tg_bound_solve_launch_group if grouped else None
        self._threads = int(threads)

    def __call__(self, n_launches):
        if self._group is not None:
            rc = self._group(self._arr, len(self._calls), int(n_launches))
        else:
            rc = self._fn(self._arr, len(self._calls), int(n_launches), self._threads)
        if rc:
            for c in self._calls:
                c.ctx._check(rc, "mrs_tg_bound_solve_launch_group" if self._group is not None else "mrs_tg_bound_solve_launch_many")


class DeviceBatch:
    """A Batch uploaded to HBM as torch tensors, plus output tensors, for the plan interface."""


    def __init__(self, batch: Batch, device="cuda:0", sample_capacity=0):
        import torch
        dev = torch.device(device)
        self.batch = batch
        self.waypoints = torch.from_numpy(batch.waypoints).to(dev)
        self.fixed_mask = torch.from_numpy(batch.fixed_mask).to(dev)
        self.fixed_values = torch.from_numpy(batch.fixed_values).to(dev)
        self.limits = torch.from_numpy(batch.limits).to(dev)
        nS, P = batch.n_segments, batch.n_paths
        self.seg_times = torch.zeros(nS, dtype=torch.float64, device=dev)
        self.coeffs = torch.zeros((nS, N_DIM, N_COEFF), dtype=torch.float64, device=dev)
        self.status = torch.zeros(P, dtype=torch.int32, device=dev)
        self.cost = torch.zeros(P, dtype=torch.float64, device=dev)
        self.n_samples = torch.zeros(P, dtype=torch.int32, device=dev)
        self.samples = torch.zeros((P, max(sample_capacity, 1), N_DIM), dtype=torch.float64, device=dev)
