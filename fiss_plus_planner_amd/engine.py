"""FrenetEngine - thin Python handle on one fp_ctx (one GPU).

Two ways in, matching the two memory spaces of the C ABI:

* numpy (`plan_dense`, `eval_trajs`): host arrays; the library stages them through its own
  device arena, runs the kernels and copies the results back (FP_MEM_HOST).  This is what
  the drop-in planner classes use.
* device pointers (`plan_dense_device`, `eval_trajs_device`): the caller keeps the problem
  batch resident in HBM (e.g. torch tensors; only `.data_ptr()` crosses the boundary) and the
  calls just enqueue kernels on the given HIP stream (FP_MEM_DEVICE).  This is what bench.py
  and the multi-GPU shard runner use.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

from . import _abi, rules
from . import rules as rules_mod  # (`rules` is an argument name of rules_eval / plan_fiss)
from .batch import ProblemBatch
from .rules import _time_gap  # (its home is the table of rule passes; callers find it here as before)

TRAJ_STRIDE = _abi.FP_DEFAULT_STRIDE

# CostFunction("WX1") weights, reference common/cost/cost_function.py:6-12 (w_T and w_D are unused there)
COST_WX1 = dict(cost_horizon=10.0, w_speed=1.0, w_accel=0.1, w_jerk=0.1, w_offset=10.0)


def make_params(batch, nd=None, nv=None, nt=None) -> _abi.FpParams:
    """fp_params of a batch.  A planner re-plans with the same batch object every cycle: the struct is cached on it, keyed on
    every scalar it is built from."""
    lim0 = getattr(batch, "curvature_limits", None)
    key = (nd or batch.nd, nv or batch.nv, nt or batch.nt, batch.check_stride, batch.tick_t, batch.veh_l, batch.veh_w, batch.max_speed, batch.max_accel,
           None if lim0 is None else tuple(lim0), getattr(batch, "w_obstacle", 0.0), _t_max(batch))  # (the VALUE points_max is derived from: an in-place edit of the arrays is seen)
    cached = getattr(batch, "__dict__", {}).get("_fp_cache")
    if cached is not None and cached[0] == key:
        return _abi.FpParams.from_buffer_copy(cached[1])  # a copy: callers may edit their struct
    p = _make_params(batch, nd, nv, nt)
    if hasattr(batch, "__dict__"):
        batch.__dict__["_fp_cache"] = (key, bytes(p))
    return p


def _t_max(batch) -> float:
    """The longest time horizon a call on this batch can sample: max(t_samples), and for the FISS planners the sampling box's upper edge."""
    t_max = float(np.max(batch.t_samples)) if len(batch.t_samples) else 0.0
    if getattr(batch, "samp_max", None) is not None and len(batch.samp_max):
        t_max = max(t_max, float(np.nanmax(batch.samp_max[:, 2])))
    return t_max


def _make_params(batch, nd=None, nv=None, nt=None) -> _abi.FpParams:
    p = _abi.FpParams()
    p.nd, p.nv, p.nt = nd or batch.nd, nv or batch.nv, nt or batch.nt
    p.check_stride = int(batch.check_stride)
    p.tick_t = float(batch.tick_t)
    p.cost_horizon, p.w_speed, p.w_accel, p.w_jerk, p.w_offset = (COST_WX1[k] for k in ("cost_horizon", "w_speed", "w_accel", "w_jerk", "w_offset"))
    p.veh_l, p.veh_w, p.max_speed, p.max_accel = float(batch.veh_l), float(batch.veh_w), float(batch.max_speed), float(batch.max_accel)
    # fp_params.points_max: what a FP_MEM_DEVICE call cannot see for itself - the points per trajectory (> 128: tick_t below 0.08 s)
    t_max = _t_max(batch)
    n_pts = int(np.ceil(t_max / float(batch.tick_t))) if t_max > 0 else 0
    p.points_max = min(n_pts, _abi.FP_MAX_POINTS) if n_pts > _abi.FP_FAST_POINTS else 0
    lim = getattr(batch, "curvature_limits", None)
    if lim is not None:  # optional checks of check_constraints (reference :145-150, commented out there)
        p.curvature_mask = 1
        p.max_curvature, p.max_kappa_d, p.max_kappa_dd = (float(v) for v in lim)
    p.w_obstacle = float(getattr(batch, "w_obstacle", 0.0))  # optional clearance cost term (a stub in the reference, cost_function.py:9,21-27,43)
    return p


_BATCH_PTRS = ("d_samples", "t_samples", "v_samples", "target_speed", "ego", "frame_of", "scene_of", "t_now", "nx", "knots", "coef",
               "obs_pose", "obs_dims", "final_time_step")


def _ptr(a: np.ndarray) -> int:
    """Address of a contiguous array's data (several times cheaper than a.ctypes.data, which builds a helper object)."""
    return a.__array_interface__["data"][0]


def _host_batch(batch: ProblemBatch) -> _abi.FpBatch:
    """FpBatch over the batch's own numpy arrays.  A planner re-plans with the same (in-place updated) arrays every cycle, so
    the struct is cached on the batch and rebuilt only when one of the arrays was replaced."""
    arrays = [getattr(batch, name) for name in _BATCH_PTRS]
    poly = [batch.obs_poly, batch.obs_nvert] if getattr(batch, "obs_nvert", None) is not None else []
    tag = int(getattr(batch, "tables_tag", 0) or 0)  # fp_batch.tables_tag: the frame / scene tables stay on the device between calls
    key = tuple(map(id, arrays + poly)) + (tag,)
    cached = batch.__dict__.get("_fb_cache")
    if cached is not None and cached[0] == key:
        return _abi.FpBatch.from_buffer_copy(cached[1])  # a copy: callers may edit their struct
    fb = _abi.FpBatch()
    fb.B, fb.F, fb.NX, fb.S, fb.T_obs, fb.n_obs = batch.B, batch.F, batch.NX, batch.S, batch.T_obs, batch.n_obs
    for name, a in zip(_BATCH_PTRS, arrays):
        setattr(fb, name, _ptr(a) if a.size else None)
    fb.tables_tag = tag
    if poly and batch.S > 0 and batch.n_obs > 0:  # convex-polygon obstacle columns (fp_batch.obs_poly / obs_nvert)
        fb.obs_poly, fb.obs_nvert, fb.poly_stride = _ptr(poly[0]), _ptr(poly[1]), int(poly[0].shape[2])
    batch.__dict__["_fb_cache"] = (key, _abi.FpBatch.from_buffer_copy(fb), arrays + poly)  # the arrays are kept alive with the pointers
    return fb


def host_structs(batch: ProblemBatch, freeze: bool = False):
    """(fp_params, fp_batch) of a host batch.  freeze=True pins them on the batch: for a caller that owns the batch, never replaces
    its arrays and never changes its scalars (planners.py updates the start state in place) later calls skip even the cache checks."""
    st = batch.__dict__.get("_structs")
    if st is not None:
        return st
    st = (make_params(batch), _host_batch(batch))
    if freeze:
        batch.__dict__["_structs"] = st
    return st


def device_batch(sizes, ptrs: dict) -> _abi.FpBatch:
    """FpBatch from raw device addresses (ints).  sizes: object with B, F, NX, S, T_obs, n_obs."""
    fb = _abi.FpBatch()
    fb.B, fb.F, fb.NX, fb.S, fb.T_obs, fb.n_obs = sizes.B, sizes.F, sizes.NX, sizes.S, sizes.T_obs, sizes.n_obs
    for name in _BATCH_PTRS:
        setattr(fb, name, ptrs.get(name) or None)
    if ptrs.get("obs_nvert"):
        fb.obs_poly, fb.obs_nvert, fb.poly_stride = ptrs["obs_poly"], ptrs["obs_nvert"], int(sizes.poly_stride)
    fb.launch_order = ptrs.get("launch_order") or None  # (fp_batch.launch_order: the caller's launch-order hint, see launch_order_hint)
    return fb


def launch_order_hint(batch) -> np.ndarray:
    """fp_batch.launch_order for a resident batch: the egos by descending speed (ties in index order).  A launch of more egos than the
    device holds workgroups ends on the egos that start last, and an ego's work grows with its speed (a faster ego reaches more obstacle
    rows: more group-test survivors, longer walks) - measured on BASELINE config 3: 136.8 -> 130.9 us per 2048-ego step, the same as the
    order learnt from the batch's own durations.  Input-only, computed once at upload; results do not depend on it."""
    return np.argsort(-np.asarray(batch.ego)[:, 1], kind="stable").astype(np.int32)


def fiss_rounds(kind, max_refine_iters: int) -> int:
    """Refinement rounds a plan_fiss call runs (the rule FrenetEngine.plan_fiss applies): FISS+ by name or by its ABI constant."""
    return int(max_refine_iters) if kind in ("FISS+", _abi.FP_FISS_PLUS) else 0


def _check_out(out: SimpleNamespace, B: int, spec: dict) -> None:
    """Caller-provided output arrays cross the C ABI as bare addresses: every array the call writes must be a writable,
    C-contiguous array of the dtype and shape [B, ...] the engine would have allocated itself (a strided or wrong-dtype array
    would be written out of bounds by the C side)."""
    for k, want in spec.items():
        if want is None:
            continue
        dtype, tail = np.dtype(want[0]), (B,) + tuple(want[1])
        a = getattr(out, k, None)
        if not isinstance(a, np.ndarray) or a.shape != tail or a.dtype != dtype or not a.flags.c_contiguous or not a.flags.writeable:
            raise ValueError(f"out.{k}: need a writable C-contiguous {dtype} array of shape {tail}, got "
                             f"{type(a).__name__ if not isinstance(a, np.ndarray) else (str(a.dtype), a.shape, bool(a.flags.c_contiguous))}")


def unpack_flags(flags: np.ndarray):
    """flag word -> (bits, N, M)."""
    return flags & 0xFF, (flags >> _abi.FLAG_N_SHIFT) & 0xFFF, (flags >> _abi.FLAG_M_SHIFT) & 0xFFF


class FrenetEngine:
    def __init__(self, device: int = 0):
        self._lib = _abi.load()
        self._ctx = C.c_void_p()
        _abi.check(self._lib.fp_ctx_create(int(device), C.byref(self._ctx)))
        self.device = int(device)

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx:
            self._lib.fp_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def set_option(self, name: str, value: int):
        """Diagnostic knobs of the ctx, e.g. set_option("lattice_kernel", 1) pins the lane-per-candidate kernel."""
        _abi.check(self._lib.fp_ctx_set_option(self._ctx, name.encode(), int(value)))

    def join(self, stream: int = 0):
        """set_option("overlap", 1): orders `stream` after every dense call of this engine that is still in flight on its internal streams
        (fp_ctx_join).  With overlap on, plan_dense_device returns with `stream` ordered after the PREVIOUS call's results only."""
        _abi.check(self._lib.fp_ctx_join(self._ctx, stream or None))

    def get_option(self, name: str) -> int:
        v = C.c_int(0)
        _abi.check(self._lib.fp_ctx_get_option(self._ctx, name.encode(), C.byref(v)))
        return v.value

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------ host arrays
    @staticmethod
    def dense_outputs(B: int, Cn: int, tables: bool = True, winner: bool = False, traj_stride: int = TRAJ_STRIDE, traj_sparse: bool = False,
                      audit: bool = False):
        """Output arrays of plan_dense for B egos (ShardedEngine allocates them once and hands every shard its slice)."""
        return SimpleNamespace(
            audit=np.zeros(B, dtype=np.uint32) if audit else None,
            best_idx=np.empty(B, dtype=np.int32), best_cost=np.empty(B), stats=np.empty((B, 4), dtype=np.int32),
            cost=np.empty((B, Cn)) if tables else None, flags=np.empty((B, Cn), dtype=np.uint32) if tables else None,
            best_flags=np.empty(B, dtype=np.uint32) if winner else None,
            # sparse: the kernels write only the elements that exist; everything else keeps this NaN fill
            best_traj=(np.full((B, 16, traj_stride), np.nan) if traj_sparse else np.empty((B, 16, traj_stride))) if winner else None)

    def plan_dense(self, batch: ProblemBatch, tables: bool = True, winner: bool = False, traj_stride: int = TRAJ_STRIDE, traj_sparse: bool = False,
                   out: SimpleNamespace | None = None, audit: bool = False, top_k: int = 0, boundary: bool = False, margins: bool = False,
                   envelope: bool = False, gates: bool = False, gaps: bool = False, fallback=None):
        """FrenetOptimalPlanner.plan() for every ego of the batch (reference frenet_optimal_planner.py:247-270).

        Returns best_idx [B] (flat (i_d*nt+i_T)*nv+i_v, -1 = none), best_cost [B], stats [B,4] and, with
        tables=True, cost [B,C] and flags [B,C]; with winner=True also best_flags [B] and best_traj [B,16,128]
        (the argmin's full series, written by the lattice kernel itself).  audit=True: also `audit` [B] (FP_AUDIT_* bits: another
        feasible candidate within 1e-9 of the winner's cost - settled by point-by-point sums -, a collision verdict within 1e-9 m of
        contact; include/frenet_gpu.h).  top_k > 0: also rank_idx [top_k, B], rank_cost [top_k, B] and n_feasible [B], the top_k
        cheapest survivors of every ego ranked on the device (rank_feasible); the tables are computed for it whether asked for or not
        (`cost` / `flags` are returned only with tables=True).  boundary=True (the batch must carry a corridor: bound_left /
        bound_right): the road-boundary check (boundary_mask) runs behind the dense call over its tables - computed for it whether
        asked for or not -; best_idx / best_cost are the argmin among the candidates that stay inside the corridor, `flags` carry
        FLAG_BOUNDARY, top_k ranks the masked tables, also n_masked [B]; with winner=True the series come from winner_trajs on the new
        best_idx (the lattice launch's own series may belong to a masked winner).  margins=True: also margin_dist / margin_step /
        margin_obs (traj_margins at the batch's check_stride) of the result - [B] for best_idx, or [top_k, B] for rank_idx together with
        top_k; with boundary=True they are taken on the masked result.  envelope=True (the batch must carry a speed profile:
        speed_limit and / or max_lat_accel): the position-dependent speed limits (speed_envelope) run behind the dense call over its
        tables; best_idx / best_cost are the argmin among the candidates that obey the envelope (and the other rules asked for), `flags`
        carry the added FLAG_SPEED / FLAG_ACCEL bits, also n_limited [B]; top_k, margins and winner=True follow the masked result like
        with boundary=True.  gates=True (the batch must carry gates: gate_s / gate_closed): the stop lines that open and close
        (gate_mask); `flags` carry the added FLAG_SPEED bits of the candidates that cross a closed gate, also n_gated [B]; everything
        else follows the masked result likewise.  gaps=True (the batch must carry a time gap: gap_follow / gap_lead > 0): the time gap
        to moving obstacles (gap_mask); `flags` carry the added FLAG_COLLISION bits, also n_close [B].  The passes asked for run in the
        order of rules.TABLE, whatever the order of the keywords: every argmin honours the bits set before it.
        fallback=FallbackStop(...): behind the last pass asked for, the egos whose best_idx is -1 get a stopping manoeuvre
        (fallback_stop): also `fallback`, its namespace - fallback.end_state [B, 3] is the plan every ego drives.  best_idx, the tables
        and everything taken on them (winner, top_k, margins) are the call's own answer without it.  A fallback with obey=... ranks its
        clear stops by those rules (fp_fallback_stop_rules; fallback.rule_bits [B] = what the chosen stop violates) - whichever passes
        the keywords above switched on.
        """
        if fallback is not None:
            if getattr(fallback, "obey", ()):
                fallback.rules_for(batch, "plan_dense(fallback=...)")  # (a rule without data: refused before anything runs)
            out = self.plan_dense(batch, tables, winner, traj_stride, traj_sparse, out, audit, top_k, boundary, margins, envelope, gates, gaps)
            out.fallback = self.fallback_stop(batch, fallback, best_idx=out.best_idx)
            return out
        if margins:
            out = self.plan_dense(batch, tables, winner, traj_stride, traj_sparse, out, audit, top_k, boundary, envelope=envelope, gates=gates, gaps=gaps)
            plans = out.rank_idx if top_k else out.best_idx
            if batch.B:
                out.margin_dist, out.margin_step, out.margin_obs = self.traj_margins(batch, best_idx=plans)
            else:
                out.margin_dist, out.margin_step, out.margin_obs = np.empty(plans.shape), np.empty(plans.shape, dtype=np.int32), np.empty(plans.shape, dtype=np.int32)
            return out
        if boundary or envelope or gates or gaps or top_k:
            asked = dict(boundary=boundary, envelope=envelope, gates=gates, gaps=gaps)
            passes = [r for r in rules.TABLE if asked[r.name]]  # (in the table's order, not the keywords': every argmin honours the bits set before it)
            for r in passes:
                if not r.carried(batch):
                    raise rules.missing(r, f"plan_dense({r.name}=True)")
            if passes and audit:
                raise ValueError("plan_dense(boundary / envelope / gates / gaps=True, audit=True): the audit bits describe the dense call's own answer, not the masked one")
            if top_k and not 1 <= int(top_k) <= _abi.FP_MAX_RANK:
                raise ValueError(f"top_k={top_k}: 0 (off) or 1 .. FP_MAX_RANK ({_abi.FP_MAX_RANK})")
            B, want_tables = batch.B, tables
            if out is not None and not tables:  # the caller's arrays hold no tables: the call brings its own
                out.cost, out.flags = np.empty((B, batch.C)), np.empty((B, batch.C), dtype=np.uint32)
                out.__dict__.pop("_res", None)
            out = self.plan_dense(batch, True, winner, traj_stride, traj_sparse, out, audit)
            for r in passes:
                if B:
                    _, bi, bc, n = self._table_pass(r, batch, out.cost, out.flags, None, True)
                else:
                    n = np.empty(0, dtype=np.int32)
                setattr(out, r.count, n)
            if passes and B:
                out.best_idx[...], out.best_cost[...] = bi, bc  # (the last pass' argmin)
                if winner:
                    w = self.winner_trajs(batch, out.best_idx, traj_stride, traj_sparse)
                    out.best_flags[...], out.best_traj[...] = w.best_flags, w.best_traj
            if top_k and B:
                out.rank_idx, out.rank_cost, out.n_feasible = self.rank_feasible(batch, out.cost, out.flags, int(top_k))
            elif top_k:
                out.rank_idx, out.rank_cost, out.n_feasible = np.empty((int(top_k), 0), dtype=np.int32), np.empty((int(top_k), 0)), np.empty(0, dtype=np.int32)
            if not want_tables:
                out.cost = out.flags = None
                out.__dict__.pop("_res", None)
            return out
        B, Cn = batch.B, batch.C
        if out is None:  # (out: arrays of dense_outputs' shapes, e.g. contiguous slices of a bigger batch's outputs)
            out = self.dense_outputs(B, Cn, tables, winner, traj_stride, traj_sparse, audit)
        elif "_res" not in out.__dict__:  # caller's arrays, first use: they cross the ABI as bare addresses
            _check_out(out, B, dict(best_idx=("int32", ()), best_cost=("float64", ()), stats=("int32", (4,)),
                                    cost=("float64", (Cn,)) if tables else None, flags=("uint32", (Cn,)) if tables else None,
                                    best_flags=("uint32", ()) if winner else None, best_traj=("float64", (16, traj_stride)) if winner else None))
        if B == 0:
            return out
        # a caller that re-plans into the same `out` every cycle (planners.py) finds the fp_result of its arrays cached on it
        # (building the struct costs several microseconds of a ~55 us plan cycle); the arrays of `out` must not be replaced then
        key = (tables, winner, int(traj_stride), int(traj_sparse), bool(audit))
        cached = out.__dict__.get("_res")
        if cached is not None and cached[0] == key:
            res = cached[1]
        else:
            res = _abi.FpResult()
            res.best_idx, res.best_cost, res.stats = _ptr(out.best_idx), _ptr(out.best_cost), _ptr(out.stats)
            res.cost_tbl = _ptr(out.cost) if tables else None
            res.flag_tbl = _ptr(out.flags) if tables else None
            res.best_flags = _ptr(out.best_flags) if winner else None
            res.best_traj = _ptr(out.best_traj) if winner else None
            res.audit = _ptr(out.audit) if audit else None
            res.traj_stride, res.traj_sparse = int(traj_stride), int(traj_sparse)
            out.__dict__["_res"] = (key, res)
        p, fb = host_structs(batch)
        _abi.check(self._lib.fp_plan_dense(self._ctx, C.byref(p), C.byref(fb), C.byref(res), _abi.FP_MEM_HOST, None))
        return out

    def rank_feasible(self, batch: ProblemBatch, cost: np.ndarray, flags: np.ndarray, k: int):
        """The k cheapest survivors of every ego from plan_dense's tables (fp_rank_feasible): cost [B,C], flags [B,C] ->
        rank_idx [k,B] (flat FOP index, -1 past the last survivor), rank_cost [k,B] (the table's entry, NaN where -1), n_feasible [B]
        (all survivors of the ego).  Ascending cost, the higher index first among equal costs: row 0 is plan_dense's best_idx /
        best_cost, and every row is a best_idx argument for winner_trajs."""
        B, Cn, k = batch.B, batch.C, int(k)
        cost = np.ascontiguousarray(cost, dtype=np.float64)
        flags = np.ascontiguousarray(flags, dtype=np.uint32)
        if cost.shape != (B, Cn) or flags.shape != (B, Cn):
            raise ValueError(f"rank_feasible: cost / flags must be [B={B}, C={Cn}] tables, got {cost.shape} / {flags.shape}")
        rank_idx = np.empty((max(k, 0), B), dtype=np.int32); rank_cost = np.empty((max(k, 0), B)); n_feasible = np.empty(B, dtype=np.int32)
        p, fb = host_structs(batch)
        # (B == 0 still crosses the ABI: the argument checks are the library's)
        _abi.check(self._lib.fp_rank_feasible(self._ctx, C.byref(p), C.byref(fb), _ptr(cost), _ptr(flags), k, _ptr(rank_idx), _ptr(rank_cost),
                                              _ptr(n_feasible), _abi.FP_MEM_HOST, None))
        return rank_idx, rank_cost, n_feasible

    def rank_feasible_device(self, params: _abi.FpParams, fb: _abi.FpBatch, cost_tbl: int, flag_tbl: int, k: int, rank_idx: int, rank_cost: int,
                             n_feasible: int = 0, stream: int = 0):
        """Enqueue the ranking behind a dense call (device addresses): rank_idx / rank_cost [k][B], n_feasible [B] or 0.
        rank_idx + 4 * j * B is the best_idx argument of winner_trajs_device / fp_advance for the j-th alternatives."""
        _abi.check(self._lib.fp_rank_feasible(self._ctx, C.byref(params), C.byref(fb), cost_tbl or None, flag_tbl or None, int(k), rank_idx or None,
                                              rank_cost or None, n_feasible or None, _abi.FP_MEM_DEVICE, stream or None))

    def _table_pass(self, rule: rules.Rule, batch: ProblemBatch, cost, flags, skip, inplace: bool, struct=None):
        """One rule pass over host tables -> (flags, best_idx, best_cost, count).  struct None = the rule's own, from the batch, which must
        carry the rule's data then."""
        held = {}

        def addr(name):
            held[name] = rules.array(batch, name)  # (kept alive over the call)
            return _ptr(held[name])

        if struct is None:
            if not rule.carried(batch):
                raise rules.missing(rule, rule.fn)
            struct = rule.struct(batch, addr)
        B, Cn = batch.B, batch.C
        cost = np.ascontiguousarray(cost, dtype=np.float64)
        if not (inplace and isinstance(flags, np.ndarray) and flags.dtype == np.uint32 and flags.flags.c_contiguous and flags.flags.writeable):
            flags = np.array(flags, dtype=np.uint32, order="C", copy=True)
        if cost.shape != (B, Cn) or flags.shape != (B, Cn):
            raise ValueError(f"{rule.fn}: cost / flags must be [B={B}, C={Cn}] tables, got {cost.shape} / {flags.shape}")
        best_idx = np.empty(B, dtype=np.int32); best_cost = np.empty(B); count = np.empty(B, dtype=np.int32)
        p, fb = host_structs(batch)
        if skip is not None:
            skip = np.ascontiguousarray(skip, dtype=np.int32)
            assert skip.shape == (B,)
            fb.skip = _ptr(skip)
        _abi.check(getattr(self._lib, rule.fn)(self._ctx, C.byref(p), C.byref(fb), C.byref(struct), _ptr(cost), _ptr(flags), _ptr(best_idx), _ptr(best_cost),
                                               _ptr(count), _abi.FP_MEM_HOST, None))
        return flags, best_idx, best_cost, count

    def _table_pass_device(self, rule: rules.Rule, params: _abi.FpParams, fb: _abi.FpBatch, struct, cost_tbl: int, flag_tbl: int, best_idx: int,
                           best_cost: int, count: int, stream: int):
        """Enqueue one rule pass over device tables (addresses; count or 0)."""
        _abi.check(getattr(self._lib, rule.fn)(self._ctx, C.byref(params), C.byref(fb), C.byref(struct), cost_tbl or None, flag_tbl or None, best_idx or None,
                                               best_cost or None, count or None, _abi.FP_MEM_DEVICE, stream or None))

    def boundary_mask(self, batch: ProblemBatch, cost: np.ndarray, flags: np.ndarray, skip: np.ndarray | None = None, inplace: bool = False):
        """The road-boundary check over plan_dense's tables (fp_boundary_mask; the definition: include/frenet_gpu.h): cost [B,C],
        flags [B,C] and the batch's corridor (bound_left / bound_right [F,NX], bound_margin) -> (flags, best_idx, best_cost, n_masked):
        the flag words with FLAG_BOUNDARY written (a copy, unless inplace=True and `flags` is a contiguous uint32 array), the argmin
        among the candidates without a FLAG_INFEASIBLE bit - which includes FLAG_BOUNDARY - and the number of candidates per ego that
        carry the bit.  skip [B] (optional): egos whose rows are neither read nor written (-1 / NaN / 0)."""
        return self._table_pass(rules.by_name["boundary"], batch, cost, flags, skip, inplace)

    def boundary_mask_device(self, params: _abi.FpParams, fb: _abi.FpBatch, left: int, right: int, margin: float, cost_tbl: int, flag_tbl: int,
                             best_idx: int, best_cost: int, n_masked: int = 0, stream: int = 0):
        """Enqueue the road-boundary check behind a dense call (device addresses): left / right [F][NX], the dense call's cost_tbl /
        flag_tbl [B][C] (flag_tbl in/out), best_idx / best_cost [B] out, n_masked [B] or 0.  best_idx is a valid argument of
        winner_trajs_device / fp_advance as it stands."""
        cor = _abi.FpCorridor(left or None, right or None, float(margin))
        self._table_pass_device(rules.by_name["boundary"], params, fb, cor, cost_tbl, flag_tbl, best_idx, best_cost, n_masked, stream)

    def speed_envelope(self, batch: ProblemBatch, cost: np.ndarray, flags: np.ndarray, skip: np.ndarray | None = None, inplace: bool = False):
        """Position-dependent speed limits and stop lines over plan_dense's tables (fp_speed_envelope; the definition:
        include/frenet_gpu.h): cost [B,C], flags [B,C] and the batch's speed profile (speed_limit [F,NX] - None = no limit anywhere -,
        limit_front, limit_tol, max_lat_accel) -> (flags, best_idx, best_cost, n_limited): the flag words with FLAG_SPEED / FLAG_ACCEL
        ORed in where a checked point violates (a copy, unless inplace=True and `flags` is a contiguous uint32 array; no bit is ever
        cleared), the argmin among the candidates without a FLAG_INFEASIBLE bit, and the number of candidates per ego that violate in
        this call.  skip [B] (optional): egos whose rows are neither read nor written (-1 / NaN / 0)."""
        return self._table_pass(rules.by_name["envelope"], batch, cost, flags, skip, inplace)

    def speed_envelope_device(self, params: _abi.FpParams, fb: _abi.FpBatch, v_limit: int, front: float, tol: float, max_lat_accel: float,
                              cost_tbl: int, flag_tbl: int, best_idx: int, best_cost: int, n_limited: int = 0, stream: int = 0):
        """Enqueue the speed envelope behind a dense call (device addresses): v_limit [F][NX], the dense call's cost_tbl / flag_tbl
        [B][C] (flag_tbl in/out), best_idx / best_cost [B] out, n_limited [B] or 0.  best_idx is a valid argument of
        winner_trajs_device / fp_advance as it stands, the tables of boundary_mask_device / rank_feasible_device."""
        prof = _abi.FpSpeedProfile(v_limit or None, float(front), float(tol), float(max_lat_accel))
        self._table_pass_device(rules.by_name["envelope"], params, fb, prof, cost_tbl, flag_tbl, best_idx, best_cost, n_limited, stream)

    def gate_mask(self, batch: ProblemBatch, cost: np.ndarray, flags: np.ndarray, skip: np.ndarray | None = None, inplace: bool = False):
        """Stop lines that open and close over plan_dense's tables (fp_gate_mask; the definition: include/frenet_gpu.h): cost [B,C],
        flags [B,C] and the batch's gates (gate_s [F,G], gate_closed [F,T_gate] uint32, gate_front, gate_max_decel) -> (flags, best_idx,
        best_cost, n_gated): the flag words with FLAG_SPEED ORed in where the candidate's front bumper moves over the line of a gate that
        is closed at that step (a copy, unless inplace=True and `flags` is a contiguous uint32 array; no bit is ever cleared), the argmin
        among the candidates without a FLAG_INFEASIBLE bit, and the number of candidates per ego that violate in this call.  The step is
        batch.t_now[b] + the point's index.  skip [B] (optional): egos whose rows are neither read nor written (-1 / NaN / 0)."""
        return self._table_pass(rules.by_name["gates"], batch, cost, flags, skip, inplace)

    def gate_mask_device(self, params: _abi.FpParams, fb: _abi.FpBatch, gate_s: int, closed: int, gate_stride: int, T_gate: int, front: float,
                         max_decel: float, cost_tbl: int, flag_tbl: int, best_idx: int, best_cost: int, n_gated: int = 0, stream: int = 0):
        """Enqueue the gates behind a dense call (device addresses): gate_s [F][gate_stride], closed [F][T_gate], the dense call's cost_tbl
        / flag_tbl [B][C] (flag_tbl in/out), best_idx / best_cost [B] out, n_gated [B] or 0.  t_now, ego and the gate arrays are read when
        the kernel runs.  best_idx is a valid argument of winner_trajs_device / fp_advance as it stands, the tables of
        speed_envelope_device / boundary_mask_device / rank_feasible_device."""
        g = _abi.FpGates(gate_s or None, closed or None, int(gate_stride), int(T_gate), float(front), float(max_decel))
        self._table_pass_device(rules.by_name["gates"], params, fb, g, cost_tbl, flag_tbl, best_idx, best_cost, n_gated, stream)

    def gap_mask(self, batch: ProblemBatch, cost: np.ndarray, flags: np.ndarray, skip: np.ndarray | None = None, inplace: bool = False,
                 follow: int | None = None, lead: int | None = None, first: int | None = None):
        """A time gap to moving obstacles over plan_dense's tables (fp_gap_mask; the definition: include/frenet_gpu.h): cost [B,C], flags
        [B,C] and the batch's gap_follow / gap_lead / gap_first in steps of tick_t (follow / lead / first override them) -> (flags,
        best_idx, best_cost, n_close): the flag words with FLAG_COLLISION ORed in where a survivor's footprint at point a overlaps an
        obstacle's at step r with 0 < a - r <= follow or 0 < r - a <= lead, a >= first, both on the check grid (a copy, unless
        inplace=True and `flags` is a contiguous uint32 array; no bit is ever cleared), the argmin among the candidates without a
        FLAG_INFEASIBLE bit, and the number of survivors per ego that violate in this call.  Both lags 0 flags nothing, and so does a
        `first` beyond every pose (any value up to INT32_MAX); lags outside 0 .. FP_MAX_POINTS or a `first` outside 1 .. INT32_MAX raise
        ValueError.
        skip [B] (optional): egos whose rows are neither read nor written (-1 / NaN / 0)."""
        g = _time_gap(batch.gap_follow if follow is None else follow, batch.gap_lead if lead is None else lead,
                      batch.gap_first if first is None else first, "gap_mask")  # (its own struct: no test for a gap on the batch, both lags 0 flag nothing)
        return self._table_pass(rules.by_name["gaps"], batch, cost, flags, skip, inplace, g)

    def gap_mask_device(self, params: _abi.FpParams, fb: _abi.FpBatch, follow: int, lead: int, first: int, cost_tbl: int, flag_tbl: int,
                        best_idx: int, best_cost: int, n_close: int = 0, stream: int = 0):
        """Enqueue the time gap behind a dense call or another pass (device addresses): the lags and `first` in steps, cost_tbl / flag_tbl
        [B][C] (flag_tbl in/out), best_idx / best_cost [B] out, n_close [B] or 0.  t_now, ego and the obstacle table are read when the
        kernel runs.  best_idx is a valid argument of winner_trajs_device / fp_advance as it stands."""
        g = _time_gap(follow, lead, first, "gap_mask_device")
        self._table_pass_device(rules.by_name["gaps"], params, fb, g, cost_tbl, flag_tbl, best_idx, best_cost, n_close, stream)

    def rules_eval(self, batch: ProblemBatch, end_states: np.ndarray, flags: np.ndarray | None = None, rules=None, counts: np.ndarray | None = None,
                   skip: np.ndarray | None = None):
        """The rule verdicts of explicit end states (fp_rules_eval; the definition: include/frenet_gpu.h): end_states [B, K, 3] = (d, v,
        T) as eval_trajs takes them, flags [B, K] their flag words (None: eval_trajs runs first and supplies them), rules = names of
        rules.TABLE (None: every rule the batch carries data for; a named rule without data raises rules.missing), counts [B, 5] int32
        to accumulate into (None: zeros) -> namespace(flags [B, K] - a copy with the rules' bits: FLAG_SPEED / FLAG_ACCEL ORed in by the
        envelope, FLAG_SPEED by the gates, FLAG_BOUNDARY written by the corridor, FLAG_COLLISION ORed in by the time gap -, rule_bits
        [B, K] - the _abi.RULE_* each trajectory violates in this call -, counts [B, 5] - per ego and rule (column log2 of the RULE_* bit)
        the violating trajectories, added to what `counts` held).  The rules run in the order of rules.TABLE, the time gap only on
        trajectories still feasible after the others.  skip [B] (optional): egos whose trajectories are not evaluated."""
        es = np.ascontiguousarray(end_states, dtype=np.float64)
        B = batch.B
        if es.ndim != 3 or es.shape[0] != B or es.shape[1] < 1 or es.shape[2] != 3:
            raise ValueError(f"rules_eval: end_states must be [B={B}, K >= 1, 3], got {es.shape}")
        K = es.shape[1]
        names = rules_mod.carried_names(batch) if rules is None else rules_mod.check_names(rules, batch, "rules_eval")
        if not names:
            raise ValueError("rules_eval: no rule to evaluate (the batch carries data for none)" if rules is None else "rules_eval: rules is empty")
        if flags is not None and np.shape(flags) != (B, K):
            raise ValueError(f"rules_eval: flags must be [B={B}, K={K}], got {np.shape(flags)}")
        if counts is not None and np.shape(counts) != (B, _abi.FP_RULE_COUNT):
            raise ValueError(f"rules_eval: counts must be [B={B}, {_abi.FP_RULE_COUNT}], got {np.shape(counts)}")
        if flags is None:
            flags = self.eval_trajs(batch, es).flags if B else np.empty((B, K), dtype=np.uint32)
        flags = np.array(flags, dtype=np.uint32, order="C", copy=True)
        counts = np.zeros((B, _abi.FP_RULE_COUNT), dtype=np.int32) if counts is None else np.array(counts, dtype=np.int32, order="C", copy=True)
        rule_bits = np.zeros((B, K), dtype=np.uint32)
        held = {}

        def addr(name):
            held[name] = np.ascontiguousarray(rules_mod.array(batch, name))  # (kept alive over the call)
            return _ptr(held[name])

        rs, structs = rules_mod.rule_set(batch, addr, names)
        p, fb = host_structs(batch)
        if skip is not None:
            skip = np.ascontiguousarray(skip, dtype=np.int32)
            assert skip.shape == (B,)
            fb.skip = _ptr(skip)
        _abi.check(self._lib.fp_rules_eval(self._ctx, C.byref(p), C.byref(fb), C.byref(rs), K, _ptr(es), _ptr(flags), _ptr(rule_bits), _ptr(counts),
                                           _abi.FP_MEM_HOST, None))
        return SimpleNamespace(flags=flags, rule_bits=rule_bits, counts=counts)

    def rules_eval_device(self, params: _abi.FpParams, fb: _abi.FpBatch, rule_set: _abi.FpRuleSet, K: int, end_states: int, flags: int, rule_bits: int = 0,
                          counts: int = 0, stream: int = 0):
        """Enqueue the rule verdicts of explicit end states (device addresses; rule_set from rules.rule_set with device addresses):
        end_states [B][K][3], flags [B][K] in/out (eval_trajs_device's words, or plan_fiss_device's best_flags with K = 1), rule_bits
        [B][K] or 0, counts [B][5] int32 in/out or 0.  One launch, nothing allocated, nothing waited for; t_now, ego, the gate phases and
        the obstacle table are read when the kernel runs."""
        _abi.check(self._lib.fp_rules_eval(self._ctx, C.byref(params), C.byref(fb), C.byref(rule_set), int(K), end_states or None, flags or None,
                                           rule_bits or None, counts or None, _abi.FP_MEM_DEVICE, stream or None))

    def traj_margins(self, batch: ProblemBatch, best_idx: np.ndarray | None = None, end_state: np.ndarray | None = None, pose_stride: int | None = None,
                     skip: np.ndarray | None = None):
        """The obstacle margin of chosen plans (fp_traj_margins; the definition: include/frenet_gpu.h): best_idx [B] or [K, B] flat FOP
        indices (plan_dense's best_idx, rank_feasible's rank_idx), or end_state [B, 3] / [K, B, 3] explicit (d, v, T) end states
        (plan_fiss' end_state; NaN = none) -> (min_dist, min_step, min_obs), each shaped like the plans: the smallest distance between
        the footprint at a checked pose and an obstacle valid there (0 on contact, +inf without a pair, NaN without a trajectory), and the
        point index and obstacle column where it occurs (-1, -1 for +inf / NaN).  pose_stride None = the batch's check_stride (the
        collision check's pose set), 1 = every pose.  skip [B] (optional): egos that have no plan (NaN, their rows are not read)."""
        if (best_idx is None) == (end_state is None):
            raise ValueError("traj_margins: exactly one of best_idx / end_state")
        B = batch.B
        if best_idx is not None:
            plans = np.ascontiguousarray(best_idx, dtype=np.int32)
            flat = plans.ndim == 1
            if plans.shape[-1:] != (B,) or plans.ndim not in (1, 2):
                raise ValueError(f"traj_margins: best_idx must be [B={B}] or [K, B], got {plans.shape}")
            K = 1 if flat else plans.shape[0]
        else:
            plans = np.ascontiguousarray(end_state, dtype=np.float64)
            flat = plans.ndim == 2
            if plans.shape[-2:] != (B, 3) or plans.ndim not in (2, 3):
                raise ValueError(f"traj_margins: end_state must be [B={B}, 3] or [K, B, 3], got {plans.shape}")
            K = 1 if flat else plans.shape[0]
        shape = (B,) if flat else (K, B)
        dist = np.empty(shape); step = np.empty(shape, dtype=np.int32); obs = np.empty(shape, dtype=np.int32)
        p, fb = host_structs(batch)
        if skip is not None:
            skip = np.ascontiguousarray(skip, dtype=np.int32)
            assert skip.shape == (B,)
            fb.skip = _ptr(skip)
        ps = int(batch.check_stride if pose_stride is None else pose_stride)
        # (B == 0 still crosses the ABI: the argument checks are the library's)
        _abi.check(self._lib.fp_traj_margins(self._ctx, C.byref(p), C.byref(fb), K, _ptr(plans) if best_idx is not None else None,
                                             _ptr(plans) if best_idx is None else None, ps, _ptr(dist), _ptr(step), _ptr(obs), _abi.FP_MEM_HOST, None))
        return dist, step, obs

    def traj_margins_device(self, params: _abi.FpParams, fb: _abi.FpBatch, k: int, min_dist: int, min_step: int, min_obs: int, best_idx: int = 0,
                            end_state: int = 0, pose_stride: int | None = None, stream: int = 0):
        """Enqueue the plan margins behind a dense / ranking / FISS call (device addresses): best_idx [k][B] (rank_idx of
        rank_feasible_device, or best_idx with k = 1) or end_state [k][B][3]; min_dist / min_step / min_obs [k][B].  pose_stride None =
        params.check_stride.  One launch, nothing allocated, nothing waited for."""
        _abi.check(self._lib.fp_traj_margins(self._ctx, C.byref(params), C.byref(fb), int(k), best_idx or None, end_state or None,
                                             int(params.check_stride if pose_stride is None else pose_stride), min_dist or None, min_step or None, min_obs or None,
                                             _abi.FP_MEM_DEVICE, stream or None))

    def fallback_stop(self, batch: ProblemBatch, fallback, best_idx: np.ndarray | None = None, end_state: np.ndarray | None = None, cand: bool = False,
                      skip: np.ndarray | None = None, counts: np.ndarray | None = None, rule_counts: np.ndarray | None = None):
        """A stopping manoeuvre for the egos without a plan (fp_fallback_stop; the definition: include/frenet_gpu.h).  fallback: a
        FallbackStop.  best_idx [B] (plan_dense's or a rule pass' argmin, < 0 = needs a fallback), or end_state [B, 3] (plan_fiss'
        end_state, NaN = needs one) - exactly one of the two; the caller's arrays are not modified.  Returns a namespace: end_state
        [B, 3] (the plan every ego drives: the lattice sample's or the untouched (d, v, T) of an ego with a plan, the chosen (d, 0, T) of
        one without, NaN where nothing is admissible), status [B] (_abi.FALLBACK_*), fb_idx [B], hit_step / hit_obs / hit_speed [B],
        counts [B, 4] (the caller's array plus one per ego in its status' column) and, with cand=True, cand [B, F] (-2 inadmissible,
        -1 clear, else the first hit step; -3 in the rows of the egos that need none).  skip [B] (optional): egos that are not planned.
        With fallback.obey set the call is fp_fallback_stop_rules: the clear stops are ranked by the obeyed rules (the batch must carry
        each one's data: rules.missing otherwise) and the namespace also has rule_bits [B] (the _abi.RULE_* the chosen stop violates, 0 =
        clean), rule_counts [B, 5] (the caller's `rule_counts` plus one per bit of rule_bits) and, with cand=True, cand_rules [B, F]
        uint32 (the verdict of every admissible, clear candidate; 0 elsewhere)."""
        obey = fallback.rules_for(batch, "fallback_stop") if getattr(fallback, "obey", ()) else ()
        if rule_counts is not None and not obey:
            raise ValueError("fallback_stop: rule_counts needs a fallback with obey=...")
        if (best_idx is None) == (end_state is None):
            raise ValueError("fallback_stop: exactly one of best_idx / end_state")
        B = batch.B
        if best_idx is not None:
            bi = np.ascontiguousarray(best_idx, dtype=np.int32)
            if bi.shape != (B,):
                raise ValueError(f"fallback_stop: best_idx must be [B={B}], got {bi.shape}")
            es = np.full((B, 3), np.nan)
        else:
            bi = None
            es = np.array(end_state, dtype=np.float64, order="C")
            if es.shape != (B, 3):
                raise ValueError(f"fallback_stop: end_state must be [B={B}, 3], got {es.shape}")
        held = {}

        def addr(name, a):
            held[name] = a
            return _ptr(a)

        fs = fallback.struct(batch, addr)
        F = fs.n_d * fs.n_stop
        out = SimpleNamespace(end_state=es, status=np.empty(B, dtype=np.int32), fb_idx=np.empty(B, dtype=np.int32), hit_step=np.empty(B, dtype=np.int32),
                              hit_obs=np.empty(B, dtype=np.int32), hit_speed=np.empty(B), cand=np.full((B, F), -3, dtype=np.int32) if cand else None,
                              counts=np.zeros((B, 4), dtype=np.int32) if counts is None else np.array(counts, dtype=np.int32, order="C"))
        if out.counts.shape != (B, 4):
            raise ValueError(f"fallback_stop: counts must be [B={B}, 4], got {out.counts.shape}")
        p, fb = host_structs(batch)
        if skip is not None:
            skip = np.ascontiguousarray(skip, dtype=np.int32)
            assert skip.shape == (B,)
            fb.skip = _ptr(skip)
        # (B == 0 still crosses the ABI: the argument checks are the library's)
        if not obey:
            _abi.check(self._lib.fp_fallback_stop(self._ctx, C.byref(p), C.byref(fb), C.byref(fs), _ptr(bi) if bi is not None else None, _ptr(es), _ptr(out.status),
                                                  _ptr(out.fb_idx), _ptr(out.hit_step), _ptr(out.hit_obs), _ptr(out.hit_speed), _ptr(out.cand) if cand else None,
                                                  _ptr(out.counts), _abi.FP_MEM_HOST, None))
            return out
        out.rule_bits = np.zeros(B, dtype=np.uint32)
        out.cand_rules = np.zeros((B, F), dtype=np.uint32) if cand else None
        out.rule_counts = np.zeros((B, _abi.FP_RULE_COUNT), dtype=np.int32) if rule_counts is None else np.array(rule_counts, dtype=np.int32, order="C")
        if out.rule_counts.shape != (B, _abi.FP_RULE_COUNT):
            raise ValueError(f"fallback_stop: rule_counts must be [B={B}, {_abi.FP_RULE_COUNT}], got {out.rule_counts.shape}")

        def rule_addr(name):
            held[name] = np.ascontiguousarray(rules_mod.array(batch, name))  # (kept alive over the call)
            return _ptr(held[name])

        rs, structs = rules_mod.rule_set(batch, rule_addr, obey)
        _abi.check(self._lib.fp_fallback_stop_rules(self._ctx, C.byref(p), C.byref(fb), C.byref(fs), C.byref(rs), _ptr(bi) if bi is not None else None, _ptr(es),
                                                    _ptr(out.status), _ptr(out.fb_idx), _ptr(out.hit_step), _ptr(out.hit_obs), _ptr(out.hit_speed),
                                                    _ptr(out.cand) if cand else None, _ptr(out.cand_rules) if cand else None, _ptr(out.rule_bits),
                                                    _ptr(out.counts), _ptr(out.rule_counts), _abi.FP_MEM_HOST, None))
        return out

    def fallback_stop_device(self, params: _abi.FpParams, fb: _abi.FpBatch, fallback: _abi.FpFallback, end_state: int, status: int, fb_idx: int, hit_step: int,
                             hit_obs: int, hit_speed: int, best_idx: int = 0, cand: int = 0, counts: int = 0, stream: int = 0):
        """Enqueue the fallback behind a plan call (device addresses; `fallback` holds device addresses too): best_idx [B] or 0 (then
        end_state [B][3] says who needs one), cand [B][F] / counts [B][4] or 0.  params.points_max must cover the longest stop time.
        One launch, nothing allocated, nothing waited for."""
        _abi.check(self._lib.fp_fallback_stop(self._ctx, C.byref(params), C.byref(fb), C.byref(fallback), best_idx or None, end_state or None, status or None,
                                              fb_idx or None, hit_step or None, hit_obs or None, hit_speed or None, cand or None, counts or None,
                                              _abi.FP_MEM_DEVICE, stream or None))

    def fallback_stop_rules_device(self, params: _abi.FpParams, fb: _abi.FpBatch, fallback: _abi.FpFallback, rule_set: _abi.FpRuleSet, end_state: int, status: int,
                                   fb_idx: int, hit_step: int, hit_obs: int, hit_speed: int, rule_bits: int, best_idx: int = 0, cand: int = 0, cand_rules: int = 0,
                                   counts: int = 0, rule_counts: int = 0, stream: int = 0):
        """Enqueue the fallback that obeys the rules behind a plan call (fp_fallback_stop_rules; device addresses, rule_set from
        rules.rule_set with device addresses): as fallback_stop_device, plus rule_bits [B], cand_rules [B][F] or 0 and rule_counts [B][5]
        in/out or 0.  One launch, nothing allocated, nothing waited for."""
        _abi.check(self._lib.fp_fallback_stop_rules(self._ctx, C.byref(params), C.byref(fb), C.byref(fallback), C.byref(rule_set), best_idx or None, end_state or None,
                                                    status or None, fb_idx or None, hit_step or None, hit_obs or None, hit_speed or None, cand or None,
                                                    cand_rules or None, rule_bits or None, counts or None, rule_counts or None, _abi.FP_MEM_DEVICE, stream or None))

    def predict_obstacles(self, batch, model, state, frame_of_scene=None, t0=0, n_rows: int | None = None, out: np.ndarray | None = None):
        """The obstacle pose table of `batch` predicted from tracks (fp_obstacles_predict through FP_MEM_HOST; the definition:
        include/frenet_gpu.h): model [S, n_obs] FP_TRACK_*, state [S, n_obs, 6], frame_of_scene [S] or None, t0 an int or [S],
        n_rows (default: T_obs) -> (obs_pose [S, T_obs, n_obs, 4], final_time_step [S]).  Of `batch` only S, T_obs, n_obs, the frames
        (nx, knots, coef) and tick_t are read - any object that carries them will do; its obs_pose is not read.  Rows outside
        max(t0, 0) .. min(T_obs, t0 + n_rows) - 1 are not written: they keep the content of `out` (a contiguous float64 array of the
        table's shape, returned as obs_pose) or, without one, zeros (= no obstacle has a pose there)."""
        S, T_obs, n_obs = int(batch.S), int(batch.T_obs), int(batch.n_obs)
        model = np.ascontiguousarray(model, dtype=np.int32)
        state = np.ascontiguousarray(state, dtype=np.float64)
        if model.shape != (S, n_obs) or state.shape != (S, n_obs, 6):
            raise ValueError(f"predict_obstacles: model / state must be [S={S}, n_obs={n_obs}] / [S, n_obs, 6], got {model.shape} / {state.shape}")
        t0 = np.ascontiguousarray(np.broadcast_to(np.asarray(t0, dtype=np.int32), (S,)))
        if frame_of_scene is not None:
            frame_of_scene = np.ascontiguousarray(frame_of_scene, dtype=np.int32)
            if frame_of_scene.shape != (S,):
                raise ValueError(f"predict_obstacles: frame_of_scene must be [S={S}], got {frame_of_scene.shape}")
        if out is None:
            out = np.zeros((S, T_obs, n_obs, 4))
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == (S, T_obs, n_obs, 4) and out.flags.c_contiguous and out.flags.writeable):
            raise ValueError(f"predict_obstacles: out must be a writable C-contiguous float64 array of shape {(S, T_obs, n_obs, 4)}")
        fts = np.zeros(S, dtype=np.int32)
        nx = np.ascontiguousarray(batch.nx, dtype=np.int32)
        knots = np.ascontiguousarray(batch.knots, dtype=np.float64)
        coef = np.ascontiguousarray(batch.coef, dtype=np.float64)
        p = _abi.FpParams()
        p.tick_t = float(batch.tick_t)
        fb = _abi.FpBatch()
        fb.S, fb.T_obs, fb.n_obs, fb.F, fb.NX = S, T_obs, n_obs, int(knots.shape[0]), int(knots.shape[1]) if knots.ndim == 2 else 0
        if knots.size:
            fb.nx, fb.knots, fb.coef = _ptr(nx), _ptr(knots), _ptr(coef)
        tr = _abi.FpTracks(_ptr(model) if model.size else None, _ptr(state) if state.size else None,
                           None if frame_of_scene is None else _ptr(frame_of_scene), _ptr(t0) if t0.size else None, int(T_obs if n_rows is None else n_rows))
        if S == 0 or n_obs == 0 or T_obs == 0:
            return out, fts
        _abi.check(self._lib.fp_obstacles_predict(self._ctx, C.byref(p), C.byref(fb), C.byref(tr), _ptr(out), _ptr(fts), _abi.FP_MEM_HOST, None))
        return out, fts

    def predict_obstacles_device(self, params: _abi.FpParams, fb: _abi.FpBatch, ftracks: _abi.FpTracks, obs_pose_ptr: int, fts_ptr: int = 0, stream: int = 0):
        """Enqueue the prediction kernel (device addresses in fb / ftracks; obs_pose_ptr [S][T_obs][n_obs][4], 16-byte aligned,
        fts_ptr [S] or 0): one launch, nothing allocated, nothing waited for.  model / state / t0 are read when the kernel runs, so a
        captured call replays against whatever the tracks hold then."""
        _abi.check(self._lib.fp_obstacles_predict(self._ctx, C.byref(params), C.byref(fb), C.byref(ftracks), obs_pose_ptr or None, fts_ptr or None,
                                                  _abi.FP_MEM_DEVICE, stream or None))

    def share_plans(self, batch: ProblemBatch, agents, best_idx: np.ndarray | None = None, end_state: np.ndarray | None = None,
                    skip: np.ndarray | None = None):
        """The chosen plans of grouped egos written into each other's obstacle tables (fp_obstacles_from_plans through FP_MEM_HOST; the
        definition: include/frenet_gpu.h).  agents: an AgentGroups; best_idx [B] (plan_dense's or a rule pass' argmin) or end_state
        [B, 3] (plan_fiss' or the fallback's end_state) - exactly one of the two; skip [B] (optional): egos that have no plan.  `batch`
        holds the plans' START states (the call goes before the hand-over).  Returns (obs_pose, final_time_step): copies of the batch's
        arrays with the members' columns and clocks rewritten; the batch itself is not modified."""
        if (best_idx is None) == (end_state is None):
            raise ValueError("share_plans: exactly one of best_idx / end_state")
        if not hasattr(self._lib, "fp_obstacles_from_plans"):
            raise RuntimeError("share_plans: libfrenetgpu.so was built before fp_obstacles_from_plans existed: rebuild")
        B = batch.B
        if best_idx is not None:
            plans = np.ascontiguousarray(best_idx, dtype=np.int32)
            if plans.shape != (B,):
                raise ValueError(f"share_plans: best_idx must be [B={B}], got {plans.shape}")
        else:
            plans = np.ascontiguousarray(end_state, dtype=np.float64)
            if plans.shape != (B, 3):
                raise ValueError(f"share_plans: end_state must be [B={B}, 3], got {plans.shape}")
        pose = np.array(batch.obs_pose, dtype=np.float64, order="C")
        fts = np.array(batch.final_time_step, dtype=np.int32, order="C")
        held = {}

        def addr(name, a):
            held[name] = a
            return _ptr(a)

        fa = agents.struct(batch, addr)
        p, fb = host_structs(batch)
        if skip is not None:
            skip = np.ascontiguousarray(skip, dtype=np.int32)
            assert skip.shape == (B,)
            fb.skip = _ptr(skip)
        _abi.check(self._lib.fp_obstacles_from_plans(self._ctx, C.byref(p), C.byref(fb), C.byref(fa), _ptr(plans) if best_idx is not None else None,
                                                     _ptr(plans) if best_idx is None else None, _ptr(pose) if pose.size else None,
                                                     _ptr(fts) if fts.size else None, _abi.FP_MEM_HOST, None))
        return pose, fts

    def share_plans_device(self, params: _abi.FpParams, fb: _abi.FpBatch, fagents: _abi.FpAgents, best_idx: int, end_state: int, obs_pose_ptr: int,
                           fts_ptr: int = 0, stream: int = 0):
        """Enqueue the shared-plans kernel between a plan (or its fallback) and fp_advance (device addresses in fb / fagents; best_idx
        [B] or 0, end_state [B][3] or 0 - exactly one; obs_pose_ptr [S][T_obs][n_obs][4], 16-byte aligned; fts_ptr [S] or 0): one
        launch, nothing allocated, nothing waited for.  The groups, the plans, ego and t_now are read when the kernel runs, so a
        captured call replays."""
        _abi.check(self._lib.fp_obstacles_from_plans(self._ctx, C.byref(params), C.byref(fb), C.byref(fagents), best_idx or None, end_state or None,
                                                     obs_pose_ptr or None, fts_ptr or None, _abi.FP_MEM_DEVICE, stream or None))

    def plan_fopplus(self, batch: ProblemBatch, winner: bool = False, traj_stride: int = TRAJ_STRIDE, traj_sparse: bool = False):
        """FopPlusPlanner.plan() for every ego of the batch (fop_plus_planner.py:16-41) on the device: the cheapest feasible
        candidate + Stats = how many candidates the cost-ordered lazy validation pops before it.  Egos whose outcome hangs on an
        exact cost tie (mirror-symmetric start states) are replayed with the reference's heap order over their dense tables
        (search.fopplus_search); `replayed` lists them.  Same result object as plan_dense plus `fopplus` [B,2]."""
        from . import search

        B = batch.B
        out = self.dense_outputs(B, batch.C, False, winner, traj_stride, traj_sparse)
        out.fopplus = np.zeros((B, 2), dtype=np.int32)
        out.replayed = np.zeros(0, dtype=np.int64)
        if B == 0:
            return out
        res = _abi.FpResult()
        res.best_idx, res.best_cost, res.stats, res.fopplus = _ptr(out.best_idx), _ptr(out.best_cost), _ptr(out.stats), _ptr(out.fopplus)
        res.best_flags = _ptr(out.best_flags) if winner else None
        res.best_traj = _ptr(out.best_traj) if winner else None
        res.traj_stride, res.traj_sparse = int(traj_stride), int(traj_sparse)
        p = make_params(batch)
        fb = _host_batch(batch)
        _abi.check(self._lib.fp_plan_dense(self._ctx, C.byref(p), C.byref(fb), C.byref(res), _abi.FP_MEM_HOST, None))
        ties = np.nonzero(out.fopplus[:, 1])[0]
        if len(ties):  # exact ties: CPython's heap order decides, as in the reference
            sub = batch.take(ties)
            tab = self.plan_dense(sub, tables=True)
            for k, e in enumerate(ties):
                idx, st = search.fopplus_search(tab.cost[k], tab.flags[k])
                out.best_idx[e] = -1 if idx is None else idx
                out.best_cost[e] = np.nan if idx is None else tab.cost[k, idx]
                out.stats[e] = st
            if winner:
                w = self.winner_trajs(sub, out.best_idx[ties], traj_stride, traj_sparse)
                out.best_flags[ties] = w.best_flags
                out.best_traj[ties] = w.best_traj
            out.replayed = ties
        return out

    def eval_trajs(self, batch: ProblemBatch, end_states: np.ndarray, dump: bool = False, traj_stride: int = TRAJ_STRIDE, traj_sparse: bool = False):
        """Explicit end states [B,K,3] = (d_end, v_end, T_end) -> cost [B,K], flags [B,K] (+ traj [B,K,16,stride])."""
        es = np.ascontiguousarray(end_states, dtype=np.float64)
        B, K = es.shape[0], es.shape[1]
        assert B == batch.B and es.shape[2] == 3
        cost = np.empty((B, K)); flags = np.empty((B, K), dtype=np.uint32)
        traj = (np.full((B, K, 16, traj_stride), np.nan) if traj_sparse else np.empty((B, K, 16, traj_stride))) if dump else None
        p = make_params(batch)
        fb = _host_batch(batch)
        _abi.check(self._lib.fp_eval_trajs(self._ctx, C.byref(p), C.byref(fb), K, es.ctypes.data, cost.ctypes.data, flags.ctypes.data,
                                           traj.ctypes.data if dump else None, int(traj_stride), int(traj_sparse), _abi.FP_MEM_HOST, None))
        return SimpleNamespace(cost=cost, flags=flags, traj=traj)

    @staticmethod
    def fiss_outputs(B: int, R: int, winner: bool = False, trace: bool = False, traj_stride: int = TRAJ_STRIDE, traj_sparse: bool = False):
        """Output arrays of plan_fiss for B egos with R refinement rounds (prev_best_idx is the in / out history array)."""
        return SimpleNamespace(prev_best_idx=np.empty((B, 3), dtype=np.int32), best_ijk=np.empty((B, 3), dtype=np.int32), best_cost=np.empty(B),
                               end_state=np.empty((B, 3)), refined=np.empty(B, dtype=np.int32), stats=np.empty((B, 4), dtype=np.int32),
                               trace=np.empty((B, max(R, 1) * 7, 4)) if trace and R > 0 else None,
                               best_flags=np.empty(B, dtype=np.uint32) if winner else None,
                               best_traj=(np.full((B, 16, traj_stride), np.nan) if traj_sparse else np.empty((B, 16, traj_stride))) if winner else None)

    def plan_fiss(self, batch: ProblemBatch, kind: str = "FISS+", prev_best_idx: np.ndarray | None = None, w_heuristic: float = 10.0,
                  max_refine_iters: int = 3, decaying_factor: float = 0.5, winner: bool = False, trace: bool = False,
                  traj_stride: int = TRAJ_STRIDE, traj_sparse: bool = False, out: SimpleNamespace | None = None, rules=(), enforce=(), fallback=None):
        """FissPlanner.plan / FissPlusPlanner.plan for every ego of the batch, entirely on the device (fp_plan_fiss):
        dense tables -> per-ego search walk -> (FISS+) refinement -> optional winner series.

        batch.d_samples must be the FISS lattice (max_road_width - w + 0.3) and batch.samp_min/max/res must be set.
        prev_best_idx [B,3] (-1 = None) is not modified; the updated copy is returned.
        rules: names of rules.TABLE the batch carries data for - the returned end state is audited by rules_eval (K = 1): also rule_bits
        [B], the _abi.RULE_* the plan violates (0 for an ego without a plan).  The plan itself is the one the call returns without
        `rules`: the walks do not look at the verdict.  The flag word comes from the call's best_flags when winner=True (the series
        writer fills it), else from eval_trajs on the end state.
        enforce: names of rules.TABLE the batch carries data for - the walks OBEY them (fp_plan_fiss_rules): the dense tables are masked
        by those rules' passes before the search reads them, and a refined candidate that violates one is rejected when it is popped;
        also `rejected` [B], the consumed refined candidates per ego that only a rule rejected.  The visiting order stays cost-only.
        May be combined with rules= (the audit of what is returned).
        fallback=FallbackStop(...): behind the walks (enforce= included), the egos whose end_state is NaN get a stopping manoeuvre
        (fallback_stop): also `fallback`, its namespace - fallback.end_state [B, 3] is the plan every ego drives.  end_state, rule_bits
        and the series are the call's own answer without it.  A fallback with obey=... ranks its clear stops by those rules
        (fp_fallback_stop_rules; fallback.rule_bits [B] = what the chosen stop violates), whatever rules= / enforce= name.
        """
        B = batch.B
        if fallback is not None and getattr(fallback, "obey", ()):
            fallback.rules_for(batch, "plan_fiss(fallback=...)")  # (a rule without data: refused before anything runs)
        audit = rules_mod.check_names(rules, batch, "plan_fiss(rules=...)") if rules else ()
        enforced = rules_mod.check_names(enforce, batch, "plan_fiss(enforce=...)") if enforce else ()
        plus = kind in ("FISS+", _abi.FP_FISS_PLUS)
        R = fiss_rounds(kind, max_refine_iters)
        if out is None:
            out = self.fiss_outputs(B, R, winner, trace, traj_stride, traj_sparse)
        elif "_io" not in out.__dict__:
            _check_out(out, B, dict(prev_best_idx=("int32", (3,)), best_ijk=("int32", (3,)), best_cost=("float64", ()), end_state=("float64", (3,)),
                                    refined=("int32", ()), stats=("int32", (4,)), trace=("float64", (max(R, 1) * 7, 4)) if trace and R > 0 else None,
                                    best_flags=("uint32", ()) if winner else None, best_traj=("float64", (16, traj_stride)) if winner else None))
        out.prev_best_idx[...] = -1 if prev_best_idx is None else np.asarray(prev_best_idx, dtype=np.int32)
        prev = out.prev_best_idx
        if enforced:
            out.rejected = np.zeros(B, dtype=np.int32)
        if B == 0:
            if audit:
                out.rule_bits = np.zeros(0, dtype=np.uint32)
            if fallback is not None:
                out.fallback = self.fallback_stop(batch, fallback, end_state=out.end_state)
            return out
        okey = (plus, R, w_heuristic, decaying_factor)
        ocached = out.__dict__.get("_opts")
        if ocached is not None and ocached[0] == okey:
            opts = ocached[1]
        else:
            opts = _abi.FpFissOpts(_abi.FP_FISS_PLUS if plus else _abi.FP_FISS, R, w_heuristic, decaying_factor)
            out.__dict__["_opts"] = (okey, opts)
        # (a caller that re-plans into the same `out` with the same batch arrays finds its fp_fiss_io cached, like plan_dense's fp_result)
        key = (winner, int(traj_stride), int(traj_sparse), id(batch.samp_min), id(batch.samp_max), id(batch.samp_res))
        cached = out.__dict__.get("_io")
        if cached is not None and cached[0] == key:
            io = cached[1]
        else:
            io = _abi.FpFissIo()
            io.samp_min, io.samp_max, io.samp_res = _ptr(batch.samp_min), _ptr(batch.samp_max), _ptr(batch.samp_res)
            io.prev_best_idx, io.best_ijk, io.best_cost = _ptr(prev), _ptr(out.best_ijk), _ptr(out.best_cost)
            io.end_state, io.refined, io.stats = _ptr(out.end_state), _ptr(out.refined), _ptr(out.stats)
            io.trace = _ptr(out.trace) if out.trace is not None else None
            io.best_flags = _ptr(out.best_flags) if winner else None
            io.best_traj = _ptr(out.best_traj) if winner else None
            io.traj_stride, io.traj_sparse = int(traj_stride), int(traj_sparse)
            out.__dict__["_io"] = (key, io, batch.samp_min, batch.samp_max, batch.samp_res)  # (the arrays kept alive: their ids are the key)
        p, fb = host_structs(batch)
        if enforced:
            held = {}

            def addr(name):
                held[name] = np.ascontiguousarray(rules_mod.array(batch, name))  # (kept alive over the call)
                return _ptr(held[name])

            rs, structs = rules_mod.rule_set(batch, addr, enforced)
            _abi.check(self._lib.fp_plan_fiss_rules(self._ctx, C.byref(p), C.byref(fb), C.byref(opts), C.byref(io), C.byref(rs), None, _ptr(out.rejected),
                                                    _abi.FP_MEM_HOST, None))
        else:
            _abi.check(self._lib.fp_plan_fiss(self._ctx, C.byref(p), C.byref(fb), C.byref(opts), C.byref(io), _abi.FP_MEM_HOST, None))
        if audit:
            out.rule_bits = self.rules_eval(batch, out.end_state[:, None, :], out.best_flags[:, None] if winner else None, audit).rule_bits[:, 0]
        if fallback is not None:
            out.fallback = self.fallback_stop(batch, fallback, end_state=out.end_state)
        return out

    def materialize_all(self, batch: ProblemBatch, traj_stride: int = TRAJ_STRIDE, traj_sparse: bool = False):
        """Full series of every lattice candidate (fp_materialize_all): traj [B,C,16,traj_stride], flags [B,C] (N, M, truncated)."""
        B, Cn = batch.B, batch.C
        traj = np.full((B, Cn, 16, traj_stride), np.nan) if traj_sparse else np.empty((B, Cn, 16, traj_stride))
        flags = np.empty((B, Cn), dtype=np.uint32)
        p = make_params(batch)
        fb = _host_batch(batch)
        _abi.check(self._lib.fp_materialize_all(self._ctx, C.byref(p), C.byref(fb), flags.ctypes.data, traj.ctypes.data, int(traj_stride), int(traj_sparse),
                                                _abi.FP_MEM_HOST, None))
        return SimpleNamespace(traj=traj, flags=flags)

    def materialize_all_device(self, params: _abi.FpParams, fb: _abi.FpBatch, flags: int, traj: int, stream: int = 0,
                               traj_stride: int = TRAJ_STRIDE, traj_sparse: bool = False):
        _abi.check(self._lib.fp_materialize_all(self._ctx, C.byref(params), C.byref(fb), flags, traj, int(traj_stride), int(traj_sparse),
                                                _abi.FP_MEM_DEVICE, stream or None))

    def build_frames(self, points: np.ndarray, n: np.ndarray | None = None):
        """CubicSpline2D construction for F centerlines on the GPU (fp_frames_build): points [F,NX,2] -> knots [F,NX], coef [F,8,NX]."""
        pts = np.ascontiguousarray(points, dtype=np.float64)
        if pts.ndim == 2:
            pts = pts[None]
        F, NX, _ = pts.shape
        n = np.full(F, NX, dtype=np.int32) if n is None else np.ascontiguousarray(n, dtype=np.int32)
        knots = np.empty((F, NX)); coef = np.empty((F, 8, NX))
        _abi.check(self._lib.fp_frames_build(self._ctx, F, NX, n.ctypes.data, pts.ctypes.data, knots.ctypes.data, coef.ctypes.data, _abi.FP_MEM_HOST, None))
        return knots, coef

    def from_state(self, knots: np.ndarray, coef: np.ndarray, nx: np.ndarray, frame_of: np.ndarray, states: np.ndarray) -> np.ndarray:
        """FrenetState.from_state for B Cartesian states [B,4] = x, y, yaw, v (fp_from_state) -> ego [B,6]."""
        st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 4)
        knots = np.ascontiguousarray(knots, dtype=np.float64); coef = np.ascontiguousarray(coef, dtype=np.float64)
        nx = np.ascontiguousarray(nx, dtype=np.int32); fo = np.ascontiguousarray(frame_of, dtype=np.int32)
        fb = _abi.FpBatch()
        fb.B, fb.F, fb.NX = st.shape[0], knots.shape[0], knots.shape[1]
        fb.frame_of, fb.nx, fb.knots, fb.coef = fo.ctypes.data, nx.ctypes.data, knots.ctypes.data, coef.ctypes.data
        ego = np.empty((st.shape[0], 6))
        _abi.check(self._lib.fp_from_state(self._ctx, C.byref(fb), st.ctypes.data, ego.ctypes.data, _abi.FP_MEM_HOST, None))
        return ego

    def build_frames_device(self, F: int, NX: int, n: int, points: int, knots: int, coef: int, stream: int = 0):
        """Enqueue the frame build (device addresses: n [F] int32, points [F,NX,2], knots [F,NX], coef [F,8,NX])."""
        _abi.check(self._lib.fp_frames_build(self._ctx, int(F), int(NX), n, points, knots, coef, _abi.FP_MEM_DEVICE, stream or None))

    def from_state_device(self, fb: _abi.FpBatch, states: int, ego: int, stream: int = 0):
        """Enqueue the projection (device addresses in fb: frame_of, nx, knots, coef; states [B,4], ego [B,6]).  An ego that cannot be
        projected (non-finite state, unusable frame) gets a NaN row instead of the host path's FP_EINVAL."""
        _abi.check(self._lib.fp_from_state(self._ctx, C.byref(fb), states, ego, _abi.FP_MEM_DEVICE, stream or None))

    # ------------------------------------------------------------------ resident device memory
    def plan_dense_device(self, params: _abi.FpParams, fb: _abi.FpBatch, best_idx: int, best_cost: int, stats: int = 0,
                          cost_tbl: int = 0, flag_tbl: int = 0, stream: int = 0, best_flags: int = 0, best_traj: int = 0,
                          traj_stride: int = TRAJ_STRIDE, traj_sparse: bool = False):
        """Enqueue the dense pass on `stream`; every argument is a device address (int)."""
        res = _abi.FpResult()
        res.best_idx, res.best_cost = best_idx, best_cost
        res.stats, res.cost_tbl, res.flag_tbl = stats or None, cost_tbl or None, flag_tbl or None
        res.best_flags, res.best_traj = best_flags or None, best_traj or None
        res.traj_stride, res.traj_sparse = int(traj_stride), int(traj_sparse)
        _abi.check(self._lib.fp_plan_dense(self._ctx, C.byref(params), C.byref(fb), C.byref(res), _abi.FP_MEM_DEVICE, stream or None))

    def plan_step_device(self, params: _abi.FpParams, fb: _abi.FpBatch, io: _abi.FpLoopIo, best_idx: int, best_cost: int, stats: int = 0,
                         stream: int = 0, best_flags: int = 0, best_traj: int = 0, traj_stride: int = TRAJ_STRIDE, traj_sparse: bool = False):
        """One cycle of the simulation loop (planning.py:120-162) for every running ego in ONE launch (fp_plan_step): the dense FOP
        pass, and the workgroup that finds an ego's argmin hands the ego over to its next state.  Device addresses throughout."""
        res = _abi.FpResult()
        res.best_idx, res.best_cost, res.stats = best_idx, best_cost, stats or None
        res.best_flags, res.best_traj = best_flags or None, best_traj or None
        res.traj_stride, res.traj_sparse = int(traj_stride), int(traj_sparse)
        _abi.check(self._lib.fp_plan_step(self._ctx, C.byref(params), C.byref(fb), C.byref(res), C.byref(io), _abi.FP_MEM_DEVICE, stream or None))

    def winner_trajs(self, batch: ProblemBatch, best_idx: np.ndarray, traj_stride: int = TRAJ_STRIDE, traj_sparse: bool = False):
        """The standalone winner epilogue (fp_winner_trajs): series of lattice candidate best_idx[b] for every ego
        -> best_flags [B], best_traj [B,16,128] (NaN rows and flag 0 where best_idx < 0)."""
        bi = np.ascontiguousarray(best_idx, dtype=np.int32)
        out = SimpleNamespace(best_flags=np.empty(batch.B, dtype=np.uint32),
                              best_traj=np.full((batch.B, 16, traj_stride), np.nan) if traj_sparse else np.empty((batch.B, 16, traj_stride)))
        p = make_params(batch)
        fb = _host_batch(batch)
        _abi.check(self._lib.fp_winner_trajs(self._ctx, C.byref(p), C.byref(fb), _ptr(bi), _ptr(out.best_flags), _ptr(out.best_traj),
                                             int(traj_stride), int(traj_sparse), _abi.FP_MEM_HOST, None))
        return out

    def winner_trajs_device(self, params: _abi.FpParams, fb: _abi.FpBatch, best_idx: int, best_flags: int, best_traj: int, stream: int = 0,
                            traj_stride: int = TRAJ_STRIDE, traj_sparse: bool = False):
        """Enqueue the winner epilogue alone (device addresses)."""
        _abi.check(self._lib.fp_winner_trajs(self._ctx, C.byref(params), C.byref(fb), best_idx, best_flags, best_traj,
                                             int(traj_stride), int(traj_sparse), _abi.FP_MEM_DEVICE, stream or None))

    def plan_fiss_device(self, params: _abi.FpParams, fb: _abi.FpBatch, opts: _abi.FpFissOpts, io: _abi.FpFissIo, stream: int = 0):
        """Enqueue the whole FISS / FISS+ pipeline (lattice, search, refinement, winner series); device addresses in `io`."""
        _abi.check(self._lib.fp_plan_fiss(self._ctx, C.byref(params), C.byref(fb), C.byref(opts), C.byref(io), _abi.FP_MEM_DEVICE, stream or None))

    def plan_fiss_rules_device(self, params: _abi.FpParams, fb: _abi.FpBatch, opts: _abi.FpFissOpts, io: _abi.FpFissIo, rule_set: _abi.FpRuleSet,
                               loop: _abi.FpLoopIo | None = None, rejected: int = 0, stream: int = 0):
        """Enqueue the FISS / FISS+ pipeline that obeys `rule_set` (fp_plan_fiss_rules; rule_set from rules.rule_set with device
        addresses): the rules' table passes between the lattice and the search, the refinement's rule instances; with `loop` the
        hand-over of fp_plan_fiss_step follows.  rejected [B] int32 in / out or 0.  A linear chain of launches, nothing waited for."""
        _abi.check(self._lib.fp_plan_fiss_rules(self._ctx, C.byref(params), C.byref(fb), C.byref(opts), C.byref(io), C.byref(rule_set),
                                                None if loop is None else C.byref(loop), rejected or None, _abi.FP_MEM_DEVICE, stream or None))

    def plan_fiss_step_device(self, params: _abi.FpParams, fb: _abi.FpBatch, opts: _abi.FpFissOpts, io: _abi.FpFissIo, loop: _abi.FpLoopIo, stream: int = 0):
        """One cycle of the simulation loop with FISS / FISS+ planning it (fp_plan_fiss_step): plan_fiss_device and the hand-over - FISS+
        hands the egos over inside its refinement launch, FISS by the advance kernel behind the pipeline.  Device addresses throughout."""
        _abi.check(self._lib.fp_plan_fiss_step(self._ctx, C.byref(params), C.byref(fb), C.byref(opts), C.byref(io), C.byref(loop), _abi.FP_MEM_DEVICE,
                                               stream or None))

    def advance_device(self, params: _abi.FpParams, fb: _abi.FpBatch, loop: _abi.FpLoopIo, best_idx: int = 0, end_state: int = 0, stream: int = 0):
        """Enqueue the hand-over alone behind a plan call (fp_advance; device addresses): every running ego moves on along its plan -
        best_idx [B] (a lattice candidate) or end_state [B][3], exactly one, the other 0.  One launch, nothing waited for."""
        _abi.check(self._lib.fp_advance(self._ctx, C.byref(params), C.byref(fb), best_idx or None, end_state or None, C.byref(loop), _abi.FP_MEM_DEVICE,
                                        stream or None))

    def loop_record_device(self, params: _abi.FpParams, fb: _abi.FpBatch, loop: _abi.FpLoopIo, best_idx: int, end_state: int, best_cost: int, stats: int,
                           log: _abi.FpLoopLog, stream: int = 0):
        """Enqueue the record kernel behind a cycle's hand-over (fp_loop_record; device addresses in loop / log): every running ego's new
        state goes to its next log row.  best_idx [B] or end_state [B][3]: the plan the hand-over drove, the other 0."""
        _abi.check(self._lib.fp_loop_record(self._ctx, C.byref(params), C.byref(fb), C.byref(loop), best_idx or None, end_state or None, best_cost or None,
                                            stats or None, C.byref(log), _abi.FP_MEM_DEVICE, stream or None))

    def eval_trajs_device(self, params: _abi.FpParams, fb: _abi.FpBatch, K: int, end_states: int, cost: int, flags: int,
                          traj: int = 0, stream: int = 0, traj_stride: int = TRAJ_STRIDE, traj_sparse: bool = False):
        _abi.check(self._lib.fp_eval_trajs(self._ctx, C.byref(params), C.byref(fb), K, end_states, cost or None, flags or None,
                                           traj or None, int(traj_stride), int(traj_sparse), _abi.FP_MEM_DEVICE, stream or None))


def device_count() -> int:
    n = C.c_int(0)
    lib = _abi.load()
    rc = lib.fp_device_count(C.byref(n))
    return n.value if rc == 0 else 0
