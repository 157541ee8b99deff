"""ctypes binding of libfrenetgpu.so (include/frenet_gpu.h).

There is no CPU implementation behind this module: loading fails loudly when the
HIP library has not been built, and every call fails when no GPU is visible.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfrenetgpu.so")

FP_ABI_VERSION = 18
FP_FISS, FP_FISS_PLUS = 0, 1
FP_MEM_HOST, FP_MEM_DEVICE = 0, 1
FP_MAX_POINTS, FP_MAX_KNOTS, FP_MAX_CAND, FP_MAX_POLY_VERTS = 256, 1024, 16384, 128
FP_FAST_POINTS, FP_DEFAULT_STRIDE = 128, 128  # the fast paths' points per trajectory; columns of a series row when traj_stride = 0
FP_MAX_CAND_SEARCH = 4096  # device-side FISS / FISS+ walks (fp_plan_fiss)
FP_MAX_RANK = 64  # K of fp_rank_feasible
FP_MAX_GATES = 32  # gates per frame of fp_gate_mask
FLAG_SPEED, FLAG_ACCEL, FLAG_COLLISION, FLAG_TRUNCATED = 1, 2, 4, 8
FLAG_CURVATURE, FLAG_KAPPA_D, FLAG_KAPPA_DD = 16, 32, 64   # optional checks (fp_params.curvature_mask)
FLAG_CONSTRAINTS = FLAG_SPEED | FLAG_ACCEL | FLAG_CURVATURE | FLAG_KAPPA_D | FLAG_KAPPA_DD
FLAG_BOUNDARY = 128  # the candidate leaves the road corridor (written by fp_boundary_mask only)
FLAG_INFEASIBLE = FLAG_CONSTRAINTS | FLAG_COLLISION | FLAG_BOUNDARY
FLAG_N_SHIFT, FLAG_M_SHIFT = 8, 20

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_up = C.POINTER(C.c_uint32)

# every symbol include/frenet_gpu.h declares (tests check the library exports all of them)
EXPORTED_SYMBOLS = ("fp_abi_version", "fp_build_flags", "fp_build_compiler", "fp_last_error", "fp_device_count", "fp_device_info", "fp_ctx_create", "fp_ctx_destroy", "fp_ctx_set_option", "fp_ctx_get_option", "fp_ctx_join",
                    "fp_plan_dense", "fp_winner_trajs", "fp_rank_feasible", "fp_boundary_mask", "fp_speed_envelope", "fp_gate_mask", "fp_gap_mask", "fp_rules_eval", "fp_traj_margins", "fp_fallback_stop", "fp_fallback_stop_rules", "fp_obstacles_predict", "fp_obstacles_from_plans", "fp_eval_trajs", "fp_plan_fiss", "fp_advance", "fp_plan_step", "fp_plan_fiss_step", "fp_plan_fiss_rules", "fp_loop_record", "fp_frames_build", "fp_from_state", "fp_materialize_all",
                    "fp_group_create", "fp_group_destroy", "fp_group_submit", "fp_group_wait")


class FpParams(C.Structure):
    _fields_ = [("nd", C.c_int32), ("nv", C.c_int32), ("nt", C.c_int32), ("check_stride", C.c_int32),
                ("tick_t", C.c_double), ("cost_horizon", C.c_double),
                ("w_speed", C.c_double), ("w_accel", C.c_double), ("w_jerk", C.c_double), ("w_offset", C.c_double),
                ("veh_l", C.c_double), ("veh_w", C.c_double), ("max_speed", C.c_double), ("max_accel", C.c_double),
                ("curvature_mask", C.c_int32), ("points_max", C.c_int32),
                ("max_curvature", C.c_double), ("max_kappa_d", C.c_double), ("max_kappa_dd", C.c_double),
                ("w_obstacle", C.c_double)]


class FpBatch(C.Structure):
    _fields_ = [("B", C.c_int32), ("F", C.c_int32), ("NX", C.c_int32), ("S", C.c_int32), ("T_obs", C.c_int32), ("n_obs", C.c_int32),
                ("d_samples", C.c_void_p), ("t_samples", C.c_void_p), ("v_samples", C.c_void_p), ("target_speed", C.c_void_p),
                ("ego", C.c_void_p), ("frame_of", C.c_void_p), ("scene_of", C.c_void_p), ("t_now", C.c_void_p),
                ("nx", C.c_void_p), ("knots", C.c_void_p), ("coef", C.c_void_p),
                ("obs_pose", C.c_void_p), ("obs_dims", C.c_void_p), ("final_time_step", C.c_void_p), ("skip", C.c_void_p),
                ("tables_tag", C.c_int32), ("poly_stride", C.c_int32), ("obs_poly", C.c_void_p), ("obs_nvert", C.c_void_p),
                ("launch_order", C.c_void_p)]


class FpResult(C.Structure):
    _fields_ = [("best_idx", C.c_void_p), ("best_cost", C.c_void_p), ("cost_tbl", C.c_void_p), ("flag_tbl", C.c_void_p),
                ("stats", C.c_void_p), ("best_flags", C.c_void_p), ("best_traj", C.c_void_p), ("fopplus", C.c_void_p), ("audit", C.c_void_p),
                ("traj_stride", C.c_int32), ("traj_sparse", C.c_int32)]


class FpCorridor(C.Structure):
    """The road edges as lateral offsets per reference-line knot (fp_boundary_mask)."""
    _fields_ = [("left", C.c_void_p), ("right", C.c_void_p), ("margin", C.c_double)]


class FpSpeedProfile(C.Structure):
    """Per-segment speed limits, read at s + front, and the lateral-acceleration bound on the reference line (fp_speed_envelope)."""
    _fields_ = [("v_limit", C.c_void_p), ("front", C.c_double), ("tol", C.c_double), ("max_lat_accel", C.c_double)]


class FpGates(C.Structure):
    """Stop lines with a state per absolute time step (fp_gate_mask)."""
    _fields_ = [("gate_s", C.c_void_p), ("closed", C.c_void_p), ("gate_stride", C.c_int32), ("T_gate", C.c_int32), ("front", C.c_double),
                ("max_decel", C.c_double)]


class FpTimeGap(C.Structure):
    """A time gap to moving obstacles, in steps of tick_t (fp_gap_mask)."""
    _fields_ = [("lag_follow", C.c_int32), ("lag_lead", C.c_int32), ("first", C.c_int32), ("reserved0", C.c_int32)]


# fp_rules_eval: which rule an explicit end state violates (rule_bits), and the columns of its per-ego counts (log2 of the bit)
RULE_LIMIT, RULE_LATERAL, RULE_GATE, RULE_BOUNDARY, RULE_GAP = 1, 2, 4, 8, 16
FP_RULE_COUNT = 5


class FpRuleSet(C.Structure):
    """The rules fp_rules_eval evaluates: a pointer to each rule's own struct, NULL = that rule is off."""
    _fields_ = [("envelope", C.POINTER(FpSpeedProfile)), ("gates", C.POINTER(FpGates)), ("boundary", C.POINTER(FpCorridor)), ("gaps", C.POINTER(FpTimeGap))]


# fp_fallback_stop: candidates per family, the reversing tolerance (m/s), the status words (also the columns of its per-ego counts)
FP_MAX_FALLBACK, FP_FALLBACK_REVERSE_TOL = 256, 1e-6
FALLBACK_NOT_NEEDED, FALLBACK_CLEAR, FALLBACK_CONTACT, FALLBACK_NONE = 0, 1, 2, 3


class FpFallback(C.Structure):
    """The family of stopping manoeuvres fp_fallback_stop chooses from: n_d lateral end offsets x n_stop stop times."""
    _fields_ = [("n_d", C.c_int32), ("n_stop", C.c_int32), ("d_targets", C.c_void_p), ("stop_T", C.c_void_p), ("max_decel", C.c_double)]


FP_TRACK_NONE, FP_TRACK_LANE, FP_TRACK_ARC = 0, 1, 2  # fp_tracks.model (fp_obstacles_predict)


class FpTracks(C.Structure):
    """The obstacle tracks a pose table is predicted from (fp_obstacles_predict)."""
    _fields_ = [("model", C.c_void_p), ("state", C.c_void_p), ("frame_of_scene", C.c_void_p), ("t0", C.c_void_p), ("n_rows", C.c_int32)]


FP_TAIL_NONE, FP_TAIL_HOLD, FP_TAIL_COAST = 0, 1, 2  # fp_agents.tail (fp_obstacles_from_plans)


class FpAgents(C.Structure):
    """The groups of egos that see each other's plans (fp_obstacles_from_plans)."""
    _fields_ = [("G", C.c_int32), ("n_members", C.c_int32), ("group_ptr", C.c_void_p), ("members", C.c_void_p), ("col_base", C.c_int32),
                ("n_rows", C.c_int32), ("tail", C.c_int32), ("reserved0", C.c_int32)]


AUDIT_NEAR_TIE, AUDIT_CONTACT, AUDIT_REORDERED, AUDIT_TIES_OVERFLOW = 1, 2, 4, 8


class FpFissOpts(C.Structure):
    _fields_ = [("kind", C.c_int32), ("max_refine_iters", C.c_int32), ("w_heuristic", C.c_double), ("decaying_factor", C.c_double)]


class FpFissIo(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("samp_min", "samp_max", "samp_res", "prev_best_idx", "best_ijk", "best_cost", "end_state",
                                          "refined", "stats", "trace", "best_flags", "best_traj")] + \
               [("traj_stride", C.c_int32), ("traj_sparse", C.c_int32)]


class FpLoopIo(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("ego", "t_now", "done", "cycles", "goal_xy", "cart_state", "goal_poly", "goal_nv", "goal_intervals")] + \
               [("goal_max_vertices", C.c_int32), ("reserved0", C.c_int32)]


RUNNING, DONE_GOAL, DONE_END_OF_LINE, DONE_NO_SOLUTION, DONE_GOAL_REGION = 0, 1, 2, 3, 4


# columns of a loop-log row (fp_loop_log.rows [B][max_rows][FP_LOG_COLS], include/frenet_gpu.h)
FP_LOG_COLS = 16
(LOG_TIME_STEP, LOG_X, LOG_Y, LOG_YAW, LOG_VELOCITY, LOG_VELOCITY_Y, LOG_S, LOG_S_DD, LOG_D, LOG_D_DD, LOG_COST, LOG_D_END, LOG_V_END,
 LOG_T_END, LOG_BEST_IDX, LOG_DONE) = range(FP_LOG_COLS)


class FpLoopLog(C.Structure):
    """The driven-trajectory log of a device-resident loop (fp_loop_record)."""
    _fields_ = [("max_rows", C.c_int32), ("reserved0", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("rows", "row_stats", "n_rows", "sealed", "stats_sum", "n_running")]


class FpCopy(C.Structure):
    _fields_ = [("dst", C.c_void_p), ("src", C.c_void_p), ("bytes", C.c_size_t)]


class FpShardCall(C.Structure):
    """One shard's call of an fp_group round (include/frenet_gpu.h: which entry point runs follows from the pointers that are set)."""
    _fields_ = [("params", C.POINTER(FpParams)), ("batch", C.POINTER(FpBatch)), ("result", C.POINTER(FpResult)), ("loop", C.POINTER(FpLoopIo)),
                ("fiss_opts", C.POINTER(FpFissOpts)), ("fiss_io", C.POINTER(FpFissIo)), ("stream", C.c_void_p),
                ("copies", C.POINTER(FpCopy)), ("n_copies", C.c_int32), ("reserved0", C.c_int32)]


class FrenetGpuError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libfrenetgpu error {code}: {msg}")
        self.code = code


_lib = None


def load() -> C.CDLL:
    """Load libfrenetgpu.so (built by `make -C fiss_plus_planner_amd/csrc` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C fiss_plus_planner_amd/csrc).  There is no CPU fallback.")
    # PyTorch-ROCm wheels bundle their own HIP runtime.  If torch is going to be used in this process (device tensors as
    # plumbing), its runtime must be the one both sides share: load it first, otherwise a later `torch.cuda` init finds the
    # system runtime already initialised and reports "No HIP GPUs are available".
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    L.fp_abi_version.restype = C.c_int
    L.fp_last_error.restype = C.c_char_p
    L.fp_build_flags.restype = C.c_char_p
    L.fp_build_compiler.restype = C.c_char_p
    flags = (L.fp_build_flags() or b"").decode()
    if flags and not os.environ.get("FP_ALLOW_DIAGNOSTIC_BUILD"):
        raise ImportError(
            f"{LIB_PATH} is a DIAGNOSTIC build ({flags}): timing ablations and stamp / counter builds share the production file name and ABI "
            "version, and some of them produce wrong results by design.  Rebuild without EXTRA (make -B -C fiss_plus_planner_amd/csrc), or set "
            "FP_ALLOW_DIAGNOSTIC_BUILD=1 if this is a profiling run.")
    L.fp_device_count.argtypes = [C.POINTER(C.c_int)]
    L.fp_device_info.argtypes = [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    L.fp_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.fp_ctx_destroy.argtypes = [C.c_void_p]
    L.fp_ctx_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.fp_ctx_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
    L.fp_ctx_join.argtypes = [C.c_void_p, C.c_void_p]
    L.fp_plan_dense.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.POINTER(FpResult), C.c_int, C.c_void_p]
    L.fp_winner_trajs.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                  C.c_int, C.c_void_p]
    L.fp_rank_feasible.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_void_p]
    # (added within ABI 18: a library of the same version built before it lacks the symbol, and the attribute look-up says so)
    L.fp_boundary_mask.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.POINTER(FpCorridor), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(L, "fp_speed_envelope"):  # (a library of the same ABI version built before the symbol existed lacks it)
        L.fp_speed_envelope.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.POINTER(FpSpeedProfile), C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(L, "fp_gate_mask"):  # (likewise)
        L.fp_gate_mask.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.POINTER(FpGates), C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(L, "fp_gap_mask"):  # (likewise)
        L.fp_gap_mask.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.POINTER(FpTimeGap), C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(L, "fp_rules_eval"):  # (likewise)
        L.fp_rules_eval.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.POINTER(FpRuleSet), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_int, C.c_void_p]
    L.fp_traj_margins.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(L, "fp_fallback_stop"):  # (likewise)
        L.fp_fallback_stop.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.POINTER(FpFallback), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(L, "fp_fallback_stop_rules"):  # (likewise)
        L.fp_fallback_stop_rules.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.POINTER(FpFallback), C.POINTER(FpRuleSet), C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_int, C.c_void_p]
    L.fp_obstacles_predict.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.POINTER(FpTracks), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(L, "fp_obstacles_from_plans"):  # (likewise)
        L.fp_obstacles_from_plans.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.POINTER(FpAgents), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_int, C.c_void_p]
    L.fp_eval_trajs.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_int32, C.c_int32, C.c_int, C.c_void_p]
    L.fp_plan_fiss.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.POINTER(FpFissOpts), C.POINTER(FpFissIo), C.c_int, C.c_void_p]
    L.fp_advance.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.c_void_p, C.c_void_p, C.POINTER(FpLoopIo), C.c_int, C.c_void_p]
    L.fp_plan_step.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.POINTER(FpResult), C.POINTER(FpLoopIo), C.c_int, C.c_void_p]
    L.fp_plan_fiss_step.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.POINTER(FpFissOpts), C.POINTER(FpFissIo), C.POINTER(FpLoopIo), C.c_int, C.c_void_p]
    if hasattr(L, "fp_plan_fiss_rules"):  # (likewise)
        L.fp_plan_fiss_rules.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.POINTER(FpFissOpts), C.POINTER(FpFissIo), C.POINTER(FpRuleSet),
                                         C.POINTER(FpLoopIo), C.c_void_p, C.c_int, C.c_void_p]
    L.fp_loop_record.argtypes =[C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.POINTER(FpLoopIo), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.POINTER(FpLoopLog), C.c_int, C.c_void_p]
    L.fp_frames_build.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.fp_from_state.argtypes = [C.c_void_p, C.POINTER(FpBatch), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.fp_materialize_all.argtypes = [C.c_void_p, C.POINTER(FpParams), C.POINTER(FpBatch), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int, C.c_void_p]
    L.fp_group_create.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p)]
    L.fp_group_destroy.argtypes = [C.c_void_p]
    L.fp_group_submit.argtypes = [C.c_void_p, C.POINTER(FpShardCall)]
    L.fp_group_wait.argtypes = [C.c_void_p]
    if L.fp_abi_version() != FP_ABI_VERSION:
        raise ImportError(f"libfrenetgpu ABI {L.fp_abi_version()} != binding {FP_ABI_VERSION}: rebuild")
    _lib = L
    return L


def check(rc: int):
    if rc != 0:
        raise FrenetGpuError(rc, load().fp_last_error().decode(errors="replace"))
