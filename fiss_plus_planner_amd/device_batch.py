"""Problem batches resident in HBM and closed-loop stepping without host round trips.

PyTorch is plumbing here (device allocations + the stream handle); every array crosses the C ABI as a raw
device address.  `DeviceBatch` uploads a ProblemBatch once; `ClosedLoopRunner` enqueues
[plan -> advance] x cycles on one stream (reference loop: planners/benchmark/planning.py:120-162) and only
reads back at the end (or per cycle, when a trace is requested).  With rules=(...) the cycle is [plan -> rule passes -> advance]: the
speed envelope, the gates, the road-boundary check and the time gap to moving obstacles run over the dense call's tables, in the order of
rules.TABLE, and decide which candidate the ego follows.
With record=True the driven trajectory of every ego - what the reference's loop returns as state_list - is written on the device by
fp_loop_record behind every step and read back once.
With audit=(...) a FISS / FISS+ cycle is [plan -> rule verdict of the returned end state -> advance] (fp_rules_eval, K = 1): the plan is
not changed, the violations are counted per ego and rule on the device.
With enforce=(...) a FISS / FISS+ cycle is ONE fp_plan_fiss_rules call with the loop's hand-over: the walks obey the rules (their validation
sees the rules' verdicts, the visiting order stays cost-only); audit=(...) may follow it (plan, verdict, advance).
With agents=AgentGroups(...) the members of a group see each other's plans: fp_obstacles_from_plans writes every member's chosen plan
into the resident obstacle tables of the others in front of fp_advance.
"""
from __future__ import annotations

from functools import partial
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np

from . import _abi
from . import rules as _rules  # (`rules` is an argument name here)
from .batch import ProblemBatch
from .closed_loop import LoopLog
from .engine import FrenetEngine, device_batch, launch_order_hint, make_params

_NAMES = ("d_samples", "t_samples", "v_samples", "target_speed", "ego", "frame_of", "scene_of", "t_now", "nx", "knots", "coef",
          "obs_pose", "obs_dims", "final_time_step")

RULES = tuple(r.name for r in _rules.TABLE if r.arrays)  # the rule passes of ClosedLoopRunner(rules=...) that read arrays of their own, in the order they run
OBSTACLE_RULES = tuple(r.name for r in _rules.TABLE if not r.arrays)  # ... and the passes that do geometry against the obstacle table instead: behind the others

LOG_POLL_CYCLES = 16  # run(record=True) reads the log's 4-byte count of running egos this often and stops enqueueing at 0


class DeviceBatch:
    def __init__(self, batch: ProblemBatch, device: int = 0, order_hint: bool = True):
        """order_hint: pass fp_batch.launch_order = the egos by descending speed (engine.launch_order_hint; results do not depend on it)."""
        import torch

        self.torch = torch
        self.host = batch
        self.dev = torch.device("cuda", device)
        self.t = {k: torch.from_numpy(np.ascontiguousarray(getattr(batch, k))).to(self.dev) for k in _NAMES}
        for k in ("samp_min", "samp_max", "samp_res", "obs_poly", "obs_nvert", "track_model", "track_state", "track_frame"):  # (the obstacle tracks: predict)
            if getattr(batch, k, None) is not None:
                self.t[k] = torch.from_numpy(getattr(batch, k)).to(self.dev)
        for rule in _rules.TABLE:  # what the rule passes the batch carries data for read (the *_device methods, ClosedLoopRunner(rules=...))
            if rule.carried(batch):
                self.t.update((k, torch.from_numpy(_rules.array(batch, k)).to(self.dev)) for k in rule.arrays)
        if order_hint and batch.B > 0:
            self.t["launch_order"] = torch.from_numpy(launch_order_hint(batch)).to(self.dev)
        self.params = make_params(batch)
        self.fb = device_batch(batch, {k: (v.data_ptr() if v.numel() else 0) for k, v in self.t.items() if k in _NAMES + ("obs_poly", "obs_nvert", "launch_order")})

    def predict(self, engine: FrenetEngine, t0, n_rows: int, stream: int = 0):
        """Rewrite the resident obs_pose / final_time_step in place from the batch's tracks (fp_obstacles_predict, one launch enqueued
        on `stream`): rows max(t0, 0) .. min(T_obs, t0 + n_rows) - 1 of every scene.  t0: a device int32 tensor [S] - the absolute
        time step the track states are valid at; it is read when the kernel runs, like t["track_state"] / t["track_model"], which a
        caller that re-perceives updates in place between calls."""
        if "track_model" not in self.t:
            raise ValueError("DeviceBatch.predict: the batch carries no tracks (ProblemBatch.track_model / track_state)")
        if not (t0.is_cuda and t0.dtype == self.torch.int32 and tuple(t0.shape) == (self.host.S,) and t0.is_contiguous()):
            raise ValueError(f"DeviceBatch.predict: t0 must be a contiguous device int32 tensor of shape ({self.host.S},)")
        if self.host.S == 0 or self.host.n_obs == 0:
            return
        tr = _abi.FpTracks(self.t["track_model"].data_ptr(), self.t["track_state"].data_ptr(),
                           self.t["track_frame"].data_ptr() if "track_frame" in self.t else None, t0.data_ptr(), int(n_rows))
        engine.predict_obstacles_device(self.params, self.fb, tr, self.t["obs_pose"].data_ptr(), self.t["final_time_step"].data_ptr(), stream)

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype, device=self.dev)

    def addr(self, k: str) -> int:
        """The device address of the resident array `k` (what rules.Rule.struct / rules.rule_set ask for)."""
        return self.t[k].data_ptr()

    def uploader(self, held: dict):
        """addr(name, array) for FallbackStop.struct / AgentGroups.struct: the array goes to the device and stays alive in `held`."""
        def addr(name, a):
            held[name] = self.torch.from_numpy(a).to(self.dev)
            return held[name].data_ptr()

        return addr

    @property
    def B(self):
        return self.host.B

    @property
    def C(self):
        return self.host.C


STAGES = ("plan", "rules", "audit", "fallback", "share", "advance")  # a cycle is a subset of these, in this order, on one stream


class CyclePlan(NamedTuple):
    stages: tuple           # of STAGES
    plan_call: str          # the ABI entry point of the plan stage
    tables: bool            # fp_plan_dense fills the runner's [B][C] cost / flag tables (the rule passes read them)
    handover_inside: bool   # the plan call hands the egos over itself: no advance stage
    drives: str             # "best_idx" or "end_state": the plan the hand-over (and the shared plans, the log) follows
    later_params: str       # "params" or "fb_params": the fp_params of share / advance / record (the fallback's cover its longest stop)
    fallback_call: str | None


def cycle_plan(planner: str, fused, rules, audit, enforce, fallback, obey, agents) -> CyclePlan:
    """One cycle of ClosedLoopRunner, from its (validated) arguments; the stage arguments count as present / absent.  No device."""
    between = bool(rules or audit or fallback or agents)  # something stands between the plan and the hand-over
    inside = not between and bool(enforce or fused)
    if planner == "FOP":
        call = "fp_plan_step" if inside else "fp_plan_dense"
    elif enforce:
        call = "fp_plan_fiss_rules"  # (loop = the runner's fp_loop_io iff the hand-over is inside, else NULL)
    else:
        call = "fp_plan_fiss_step" if inside else "fp_plan_fiss"
    present = dict(plan=True, rules=rules, audit=audit, fallback=fallback, share=agents, advance=not inside)
    return CyclePlan(tuple(s for s in STAGES if present[s]), call, bool(rules), inside, "end_state" if planner != "FOP" or fallback else "best_idx",
                     "fb_params" if fallback else "params", ("fp_fallback_stop_rules" if obey else "fp_fallback_stop") if fallback else None)


class ClosedLoopRunner:
    """[plan -> advance] for a whole batch on the device.  planner: "FOP" (fp_plan_dense) or "FISS"/"FISS+" (fp_plan_fiss)."""

    def __init__(self, engine: FrenetEngine, dbatch: DeviceBatch, goal_xy: np.ndarray, planner: str = "FOP", fused: bool = True,
                 goal_poly: np.ndarray | None = None, goal_nv: np.ndarray | None = None, goal_intervals: np.ndarray | None = None,
                 rules=(), audit=(), enforce=(), fallback=None, agents=None):
        """The cycle is one linear chain on one stream, eager and from a graph (cycle_plan above):
            plan -> rule passes -> audit verdict -> fallback stop -> share plans -> advance
        with the stages the arguments below ask for.  When nothing stands between the plan and the hand-over, and `fused` or enforce= is
        set, the plan call hands the egos over itself and there is no advance stage (fp_plan_step; fp_plan_fiss_step: FISS+ hands over
        inside its refinement launch, FISS by the advance kernel behind the pipeline; fp_plan_fiss_rules with the loop's fp_loop_io);
        fused=False then gives the plan call + fp_advance (same results; the A/B of tests and bench).  In every other cycle the plan call
        is the one without a hand-over (fp_plan_dense, fp_plan_fiss, fp_plan_fiss_rules with loop = NULL) and `fused` is not looked at.
        The hand-over follows FOP's best_idx, or end_state for FISS / FISS+ and whenever a fallback is present.
        rules: any subset of the names in rules.TABLE - FOP only, and the batch must carry each rule's data (speed profile / gates /
        corridor / a time gap with a lag above 0).  fp_plan_dense then fills the runner's own [B][C] tables and the passes asked for run
        in the table's order, whatever the caller's, each writing best_idx / best_cost: the hand-over follows the last one's winner.
        audit: any subset of the names in rules.TABLE - FISS / FISS+ only (FOP enforces its rules with rules=), and the batch must carry
        each rule's data.  The plan call is asked for best_flags (its series writer fills them beside best_traj) and fp_rules_eval (K = 1
        on end_state, counts = self.violations) takes the verdict before the hand-over moves ego / t_now; the plan is the one the loop
        drives without audit.  self.violations [B, 5] int32 counts, per ego and FP_RULE_* bit (column log2 of the bit), the cycles whose
        plan violated; run / run_graph return them as `violations` (rule name -> [B]; the envelope's entry adds its two columns) and
        `violation_counts` [B, 5].
        enforce: any subset of the names in rules.TABLE - FISS / FISS+ only (FOP enforces with rules=), and the batch must carry each
        rule's data.  The plan call is fp_plan_fiss_rules: the walks obey the rules.  self.rejected [B] int32 sums, per ego, the refined
        candidates a rule alone rejected; run / run_graph return it.
        fallback: a FallbackStop - FOP (with or without rules=) and FISS / FISS+ (with or without enforce=).  fp_fallback_stop follows the
        plan and the rule passes: an ego whose plan call found nothing brakes to a stop along the lane instead of ending with
        FP_DONE_NO_SOLUTION, and plans again in the next cycle.  self.fallback_counts [B, 4] int32 counts, per ego, the cycles by fallback
        status (_abi.FALLBACK_*: column 0 = the ego had a plan or was finished); run / run_graph return it.  With record=True the log is
        written from end_state for FOP too: its FP_LOG_BEST_IDX column is then -1 in every row.  fallback= with audit= is not done
        (ValueError).  A fallback with obey=(...) (any subset of the names in rules.TABLE; the batch must carry each rule's data,
        whichever rules= / enforce= name) makes the call fp_fallback_stop_rules: the clear stops are ranked by those rules - an ego in
        front of a closed gate stops before the line.  self.fallback_rule_counts [B, 5] int32 counts, per ego and FP_RULE_* bit (column
        log2 of the bit), the cycles whose chosen stop violated the rule; run / run_graph return it.
        agents: an AgentGroups - the members see each other's plans.  The batch must give every member a scene of its own
        (AgentGroups.attach).  fp_obstacles_from_plans writes the plans the hand-over is about to follow into the RESIDENT table
        (dbatch.t["obs_pose"] / t["final_time_step"] are rewritten in place, cycle after cycle).  The first cycle plans against whatever
        the table holds.  The table is what rules=("gaps",) reads, so agents keep a time gap to each other with no further code.
        agents= with audit= is not done (ValueError).
        goal_poly [B, V, 2] + goal_nv [B] (+ goal_intervals [B, 6] = time_step / velocity / orientation lo, hi; NaN = undefined): the
        goal region of goal_region.is_reached() (planning.py:150-153), see fp_loop_io in include/frenet_gpu.h."""
        self.rules = self._check_rules(rules, planner, dbatch.host)  # (first: the argument errors need no device)
        self.audit = self._check_audit(audit, planner, dbatch.host)
        self.enforce = self._check_enforce(enforce, planner, dbatch.host, self.rules)
        if fallback is not None and self.audit:
            raise ValueError("ClosedLoopRunner: fallback= with audit= is not done (the audit's verdict is taken on the planner's own end state)")
        if agents is not None and self.audit:
            raise ValueError("ClosedLoopRunner: agents= with audit= is not done (the audit's verdict is taken on the planner's own end state)")
        if agents is not None:
            agents.check(dbatch.host)
        self.fallback, self.agents = fallback, agents
        self.obey = fallback.rules_for(dbatch.host, "ClosedLoopRunner(fallback=FallbackStop") if fallback is not None and getattr(fallback, "obey", ()) else ()
        self.plan = cycle_plan(planner, fused, self.rules, self.audit, self.enforce, fallback is not None, self.obey, agents is not None)
        torch = dbatch.torch
        self.eng, self.db, self.planner, self.fused = engine, dbatch, planner, fused
        B = dbatch.B
        i32, f64 = torch.int32, torch.float64
        zeros = lambda shape: torch.zeros(shape, dtype=i32, device=dbatch.dev)  # noqa: E731
        self.best_idx = dbatch.empty(B, i32)
        self.best_cost = dbatch.empty(B, f64)
        self.stats = dbatch.empty((B, 4), i32)
        self.done, self.cycles = zeros(B), zeros(B)
        self.goal = torch.from_numpy(np.ascontiguousarray(goal_xy, dtype=np.float64).reshape(B, 2)).to(dbatch.dev)
        self.cart = torch.full((B, 3), float("nan"), dtype=f64, device=dbatch.dev)
        # the runner's OWN view of the resident batch (the shared DeviceBatch keeps its skip mask and its launch-order hint for other callers)
        self.fb = _abi.FpBatch.from_buffer_copy(dbatch.fb)
        self.fb.skip = self.done.data_ptr()  # finished egos are not planned any more
        self.fb.launch_order = None  # (the egos' states move on: the order the ctx learns from its own launches follows them, the upload's hint would not)
        self.io = _abi.FpLoopIo()
        self.io.ego, self.io.t_now = dbatch.addr("ego"), dbatch.addr("t_now")
        self.io.done, self.io.cycles = self.done.data_ptr(), self.cycles.data_ptr()
        self.io.goal_xy, self.io.cart_state = self.goal.data_ptr(), self.cart.data_ptr()
        if goal_poly is not None:
            gp = np.ascontiguousarray(goal_poly, dtype=np.float64).reshape(B, -1, 2)
            self.goal_poly = torch.from_numpy(gp).to(dbatch.dev)
            self.goal_nv = torch.from_numpy(np.ascontiguousarray(goal_nv, dtype=np.int32).reshape(B)).to(dbatch.dev)
            self.io.goal_poly, self.io.goal_nv, self.io.goal_max_vertices = self.goal_poly.data_ptr(), self.goal_nv.data_ptr(), gp.shape[1]
            if goal_intervals is not None:
                self.goal_iv = torch.from_numpy(np.ascontiguousarray(goal_intervals, dtype=np.float64).reshape(B, 6)).to(dbatch.dev)
                self.io.goal_intervals = self.goal_iv.data_ptr()
        if self.rules:  # the tables the passes mask, and how many candidates each pass flagged in the last cycle
            self.cost_tbl = dbatch.empty((B, dbatch.C), f64)
            self.flag_tbl = zeros((B, dbatch.C))
            self.n_flagged = {r: zeros(B) for r in self.rules}
            self.passes = [(p, p.struct(dbatch.host, dbatch.addr), self.n_flagged[p.name].data_ptr()) for p in map(_rules.by_name.get, self.rules)]
        if planner != "FOP":
            self.prev = torch.full((B, 3), -1, dtype=i32, device=dbatch.dev)
            self.ijk = dbatch.empty((B, 3), i32)
            self.end_state = dbatch.empty((B, 3), f64)
            self.refined = dbatch.empty(B, i32)
            self.fopts = _abi.FpFissOpts(_abi.FP_FISS_PLUS if planner == "FISS+" else _abi.FP_FISS, 3 if planner == "FISS+" else 0, 10.0, 0.5)
            f = _abi.FpFissIo()
            f.samp_min, f.samp_max, f.samp_res = (dbatch.addr(k) for k in ("samp_min", "samp_max", "samp_res"))
            f.prev_best_idx, f.best_ijk, f.best_cost, f.end_state = self.prev.data_ptr(), self.ijk.data_ptr(), self.best_cost.data_ptr(), self.end_state.data_ptr()
            f.refined, f.stats, f.trace, f.best_flags, f.best_traj = self.refined.data_ptr(), self.stats.data_ptr(), None, None, None
            self.fio = f
        if self.audit:  # the plan's flag word (fp_plan_fiss writes best_flags with the series), the rule set on device addresses, the counts
            stride = max(_abi.FP_DEFAULT_STRIDE, int(dbatch.params.points_max))
            self.best_flags = zeros(B)
            self.best_traj = dbatch.empty((B, 16, stride), f64)
            self.fio.best_flags, self.fio.best_traj = self.best_flags.data_ptr(), self.best_traj.data_ptr()
            self.fio.traj_stride, self.fio.traj_sparse = stride, 1
            self.violations = zeros((B, _abi.FP_RULE_COUNT))
            self.rule_set, self._rule_structs = _rules.rule_set(dbatch.host, dbatch.addr, self.audit)
        self._uploads = {}  # the fallback's and the agents' own arrays on the device
        if fallback is not None:  # the family on device addresses, the call's outputs, and the per-ego counts by status
            if planner == "FOP":
                self.end_state = torch.full((B, 3), float("nan"), dtype=f64, device=dbatch.dev)
            self.fb_struct = fallback.struct(dbatch.host, dbatch.uploader(self._uploads))
            self.fb_status, self.fb_idx, self.fb_hit_step, self.fb_hit_obs = (zeros(B) for _ in range(4))
            self.fb_hit_speed = torch.full((B,), float("nan"), dtype=f64, device=dbatch.dev)
            self.fallback_counts = zeros((B, 4))
            if self.obey:  # the obeyed set on device addresses (DeviceBatch has uploaded the arrays of every rule the batch carries), the verdicts, the counts
                self.fb_rule_bits = zeros(B)
                self.fallback_rule_counts = zeros((B, _abi.FP_RULE_COUNT))
                self.obey_set, self._obey_structs = _rules.rule_set(dbatch.host, dbatch.addr, self.obey)
            # (the fallback's own calls are sized for its longest stop time; the plan calls keep the batch's params)
            self.fb_params = _abi.FpParams.from_buffer_copy(dbatch.params)
            pts = max(fallback.points_max(dbatch.host.tick_t), int(dbatch.params.points_max))
            self.fb_params.points_max = min(pts, _abi.FP_MAX_POINTS) if pts > _abi.FP_FAST_POINTS else 0
        if agents is not None:  # the groups on device addresses
            self.ag_struct = agents.struct(dbatch.host, dbatch.uploader(self._uploads))
        if self.enforce:  # the enforced set on device addresses, and the per-ego count of rule-rejected refined candidates
            self.rejected = zeros(B)
            self.enforce_set, self._enforce_structs = _rules.rule_set(dbatch.host, dbatch.addr, self.enforce)
        self.chain = self._chain()

    @staticmethod
    def _names(asked) -> tuple:
        return (asked,) if isinstance(asked, str) else tuple(asked)

    @classmethod
    def _check_rules(cls, rules, planner, batch) -> tuple:
        """The rules in the order they run; ValueError for an unknown rule, a planner that is not FOP, or a rule without its data."""
        asked = cls._names(rules)
        for r in asked:
            if r not in _rules.by_name:
                raise ValueError(f"ClosedLoopRunner: unknown rule {r!r} (rules are a subset of {tuple(_rules.by_name)})")
        if asked and planner != "FOP":
            raise ValueError(f"ClosedLoopRunner: rules are defined for the FOP planner only ({planner} orders candidates by cost before validation)")
        for r in asked:
            if not _rules.by_name[r].carried(batch):
                raise _rules.missing(_rules.by_name[r], f"ClosedLoopRunner(rules={r!r})")
        return tuple(r for r in _rules.by_name if r in asked)

    @classmethod
    def _check_enforce(cls, enforce, planner, batch, rules) -> tuple:
        """The enforced rules in the order they run; ValueError for an unknown rule, the FOP planner, rules= beside it, or a rule without
        its data."""
        asked = cls._names(enforce)
        if asked and rules:
            raise ValueError("ClosedLoopRunner: enforce= (FISS / FISS+) and rules= (FOP) do not combine")
        if asked and planner == "FOP":
            raise ValueError("ClosedLoopRunner: enforce is for the FISS / FISS+ planners (FOP enforces its rules with rules=...)")
        return _rules.check_names(asked, batch, "ClosedLoopRunner(enforce=...)")

    @classmethod
    def _check_audit(cls, audit, planner, batch) -> tuple:
        """The audited rules in the order they run; ValueError for an unknown rule, the FOP planner, or a rule without its data."""
        asked = cls._names(audit)
        names = _rules.check_names(asked, batch, "ClosedLoopRunner(audit=...)")
        if asked and planner == "FOP":
            raise ValueError("ClosedLoopRunner: audit is for the FISS / FISS+ planners (FOP enforces its rules with rules=...)")
        return names

    def _chain(self) -> list:
        """The calls of one cycle, stage by stage as self.plan lists them: callables of `stream=`.  Every address is fixed from here on
        (state lives in HBM and is updated in place), so the arguments are bound once - to the engine's methods, not to the runner:
        a dropped runner is freed at once, without waiting for the cycle collector."""
        eng, db, fb, plan = self.eng, self.db, self.fb, self.plan
        bi, bc, stats = self.best_idx.data_ptr(), self.best_cost.data_ptr(), self.stats.data_ptr()
        # what the hand-over follows, for share / advance / record: (params, best_idx, end_state), one of the two addresses 0
        self.driven = (self.fb_params if plan.later_params == "fb_params" else db.params,
                       bi if plan.drives == "best_idx" else 0, self.end_state.data_ptr() if plan.drives == "end_state" else 0)
        chain = []
        for stage in plan.stages:
            if stage == "plan":
                loop = self.io if plan.handover_inside else None
                if plan.plan_call == "fp_plan_step":
                    chain.append(partial(eng.plan_step_device, db.params, fb, loop, bi, bc, stats))
                elif plan.plan_call == "fp_plan_dense":
                    tables = dict(cost_tbl=self.cost_tbl.data_ptr(), flag_tbl=self.flag_tbl.data_ptr()) if plan.tables else {}
                    chain.append(partial(eng.plan_dense_device, db.params, fb, bi, bc, stats, **tables))
                elif plan.plan_call == "fp_plan_fiss_rules":  # (with `loop`: the rules' passes, the walks and the hand-over in one call)
                    chain.append(partial(eng.plan_fiss_rules_device, db.params, fb, self.fopts, self.fio, self.enforce_set, loop, self.rejected.data_ptr()))
                elif plan.plan_call == "fp_plan_fiss_step":
                    chain.append(partial(eng.plan_fiss_step_device, db.params, fb, self.fopts, self.fio, loop))
                else:
                    chain.append(partial(eng.plan_fiss_device, db.params, fb, self.fopts, self.fio))
            elif stage == "rules":
                cost, flags = self.cost_tbl.data_ptr(), self.flag_tbl.data_ptr()
                chain += [partial(eng._table_pass_device, rule, db.params, fb, struct, cost, flags, bi, bc, n) for rule, struct, n in self.passes]
            elif stage == "audit":  # (taken before the hand-over moves ego / t_now)
                chain.append(partial(eng.rules_eval_device, db.params, fb, self.rule_set, 1, self.end_state.data_ptr(), self.best_flags.data_ptr(), 0,
                                     self.violations.data_ptr()))
            elif stage == "fallback":
                out = [getattr(self, k).data_ptr() for k in ("end_state", "fb_status", "fb_idx", "fb_hit_step", "fb_hit_obs", "fb_hit_speed")]
                kw = dict(best_idx=bi if self.planner == "FOP" else 0, counts=self.fallback_counts.data_ptr())
                if plan.fallback_call == "fp_fallback_stop_rules":
                    chain.append(partial(eng.fallback_stop_rules_device, self.fb_params, fb, self.fb_struct, self.obey_set, *out, self.fb_rule_bits.data_ptr(),
                                         rule_counts=self.fallback_rule_counts.data_ptr(), **kw))
                else:
                    chain.append(partial(eng.fallback_stop_device, self.fb_params, fb, self.fb_struct, *out, **kw))
            elif stage == "share":
                params, plan_bi, plan_es = self.driven
                chain.append(partial(eng.share_plans_device, params, fb, self.ag_struct, plan_bi, plan_es, db.addr("obs_pose"), db.addr("final_time_step")))
            else:
                chain.append(partial(eng.advance_device, self.driven[0], fb, self.io, *self.driven[1:]))
        return chain

    def step(self, stream: int = 0):
        """One plan cycle for every running ego + the state hand-over, enqueued on `stream`."""
        for call in self.chain:
            call(stream=stream)

    def log_reset(self, max_rows: int, poll: bool = True):
        """A fresh device log for the cycles that follow (fp_loop_log): max_rows rows per ego beyond the cycles driven so far, egos that are
        already finished sealed.  poll=False: no count of running egos (one memset less per record call)."""
        torch = self.db.torch
        B, dev = self.db.B, self.db.dev
        self.log_row0 = self.cycles.cpu().numpy().copy()
        rows = int(max_rows) + (int(self.log_row0.max()) if B else 0)
        self.log_rows = torch.full((B, rows, _abi.FP_LOG_COLS), float("nan"), dtype=torch.float64, device=dev)
        self.log_row_stats = torch.zeros((B, rows, 4), dtype=torch.int32, device=dev)
        self.log_n_rows = self.cycles.clone()
        self.log_sealed = (self.done != 0).to(torch.int32)
        self.log_stats_sum = torch.zeros((B, 4), dtype=torch.int64, device=dev)
        self.log_running = torch.full((1,), -1, dtype=torch.int32, device=dev)
        lg = _abi.FpLoopLog()
        lg.max_rows = rows
        lg.rows, lg.row_stats, lg.n_rows = self.log_rows.data_ptr(), self.log_row_stats.data_ptr(), self.log_n_rows.data_ptr()
        lg.sealed, lg.stats_sum = self.log_sealed.data_ptr(), self.log_stats_sum.data_ptr()
        lg.n_running = self.log_running.data_ptr() if poll else None
        self.flog = lg

    def record(self, stream: int = 0):
        """fp_loop_record behind the step just enqueued on `stream`: every running ego's new state goes to its next log row."""
        params, bi, es = self.driven  # (with a fallback the driven plan is end_state for every planner)
        self.eng.loop_record_device(params, self.fb, self.io, bi, es, self.best_cost.data_ptr(), self.stats.data_ptr(), self.flog, stream)

    def log_fetch(self) -> LoopLog:
        """The log as numpy arrays (one read-back; synchronises)."""
        return LoopLog(rows=self.log_rows.cpu().numpy(), n_rows=self.log_n_rows.cpu().numpy(), row_stats=self.log_row_stats.cpu().numpy(),
                       stats_sum=self.log_stats_sum.cpu().numpy(), sealed=self.log_sealed.cpu().numpy(), row0=self.log_row0)

    def _result(self, rows, record):
        out = SimpleNamespace(done=self.done.cpu().numpy(), cycles=self.cycles.cpu().numpy(), ego=self.db.t["ego"].cpu().numpy(),
                              t_now=self.db.t["t_now"].cpu().numpy(), cart=self.cart.cpu().numpy(), trace=rows)
        if record:
            out.log = self.log_fetch()
        if self.enforce:
            out.rejected = self.rejected.cpu().numpy()
        if self.fallback is not None:
            out.fallback_counts = self.fallback_counts.cpu().numpy()
            if self.obey:
                out.fallback_rule_counts = self.fallback_rule_counts.cpu().numpy()
        if self.audit:
            out.violation_counts = self.violations.cpu().numpy()
            cols = lambda bits: [i for i in range(_abi.FP_RULE_COUNT) if bits >> i & 1]  # noqa: E731
            out.violations = {n: out.violation_counts[:, cols(_rules.BITS[n])].sum(axis=1) for n in self.audit}
        return out

    def run_graph(self, max_cycles: int, record: bool = False):
        """The same loop as run(), but one [plan -> advance] cycle is captured into a HIP graph once and replayed: the cycle is
        launch-bound for small batches (2-5 short kernels), and every pointer it touches is fixed (state lives in HBM and is
        updated in place), so a replay needs no host work beyond hipGraphLaunch.
        record: fp_loop_record is captured behind the step - the log's row index lives on the device, so every replay appends."""
        torch = self.db.torch
        if record:
            self.log_reset(max_cycles, poll=False)  # (nobody polls between replays)
        self.step(torch.cuda.current_stream(self.db.dev).cuda_stream)  # warm-up outside capture: first-use allocations, LDS attributes
        if record:
            self.record(torch.cuda.current_stream(self.db.dev).cuda_stream)
        torch.cuda.synchronize(self.db.dev)
        side = torch.cuda.Stream(self.db.dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            self.step(side.cuda_stream)
            if record:
                self.record(side.cuda_stream)
        torch.cuda.synchronize(self.db.dev)
        import time
        t0 = time.perf_counter()
        for _ in range(max_cycles - 1):
            graph.replay()
        torch.cuda.synchronize(self.db.dev)
        self.replay_seconds = time.perf_counter() - t0  # capture / instantiation excluded
        return self._result([], record)

    def run(self, max_cycles: int, trace: bool = False, record: bool = False):
        """trace: the host reads every cycle back (five blocking copies per cycle).  record: the device keeps the driven trajectory
        (out.log, a closed_loop.LoopLog; closed_loop.result_from_log makes a ClosedLoopResult of one ego's rows) and the loop stops
        enqueueing once no ego is running - the count is read every LOG_POLL_CYCLES cycles."""
        torch = self.db.torch
        stream = torch.cuda.current_stream(self.db.dev).cuda_stream
        rows = []
        if record:
            self.log_reset(max_cycles)
        for i in range(max_cycles):
            if trace:
                start = self.db.t["ego"].cpu().numpy().copy()
            self.step(stream)
            if record:
                self.record(stream)
                if not trace and (i + 1) % LOG_POLL_CYCLES == 0 and int(self.log_running.item()) == 0:
                    break
            if trace:
                rows.append(SimpleNamespace(start=start, cost=self.best_cost.cpu().numpy().copy(), stats=self.stats.cpu().numpy().copy(),
                                            done=self.done.cpu().numpy().copy(), cart=self.cart.cpu().numpy().copy()))
                if (rows[-1].done != 0).all():
                    break
        torch.cuda.synchronize(self.db.dev)
        return self._result(rows, record)
