"""Fixtures of the suites of fp_fallback_stop_rules (tests/test_fallback_rules_cpu.py, tests/test_gpu_fallback_rules.py).

  - the fixtures of fallback_cases.py (imported, not edited) with the data of all four rules added: "base", "many poses", "off LDS",
    "ties", "no obstacles", "rings";
  - "analytic": a straight line, two egos at v0 = 8, a0 = 0, no obstacle, stop times (2, 3, 4.5, 6) - a stop (d, 0, T) travels
    v0 T / 2 = 8, 12, 18, 24 m - and one gate 14 m in front of ego 0's bumper, closed throughout, gates.max_decel = 4 (stopping distance
    8 m < 14 m: not waived).  Rule-blind the choice is T = 6, across the line; obeying it is T = 3, rule_bits 0.  Ego 1 stands 5 m in
    front of the line: waived, it chooses as the rule-blind call does.  "analytic soft" is the same batch with the fallback's
    max_decel = 3: the peak deceleration of a stop is 1.5 v0 / T = 6, 4, 2.67, 2 m/s^2, so only T = 4.5 and T = 6 are admissible, both
    cross, and the choice is T = 4.5 with FP_RULE_GATE: the hardest brake when nothing is clean;
  - one small fixture per rule in which that rule alone decides: "corridor", "zero limit", "time gap"; "fewest rules": every stop
    violates, and the number of rules broken decides;
  - "all contact": a wall in front of the ego - every candidate hits and no rule is consulted;
  - the closed-loop scenario: fallback_cases.loop_scenario() with a gate instead of the wall.

Every reference (tests/fallback_rules_ref.py) is computed once per process and left unchanged."""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np

import boundary_ref as BR
import envelope_ref as ER
import fallback_cases as FC
import fallback_ref as FR
import fallback_rules_ref as FRR
import gaps_ref as PR
import gates_ref as GR

RULE_LIMIT, RULE_LATERAL, RULE_GATE, RULE_BOUNDARY, RULE_GAP = 1, 2, 4, 8, 16
ALL = ("envelope", "gates", "boundary", "gaps")
STOP_T = FC.STOP_T
GATES_AHEAD = (12.0, 22.0)  # m in front of each ego's s: inside the reach of the family's stops (8 .. 24 m at 8 m/s)


def with_rules(batch):
    """`batch` carrying all four rules: the siblings' wavy limit with the lateral bound, two lights per frame, the widened wavy corridor,
    the time gap 20 / 10 / 2."""
    b = GR.with_gates(ER.with_profile(batch, max_lat_accel=ER.MAX_LAT_ACCEL), ahead=GATES_AHEAD)
    dl, dr = BR.wavy_corridor(b.knots)
    return dataclasses.replace(PR.with_gap(b), bound_left=dl + BR.WIDEN, bound_right=dr - BR.WIDEN, bound_margin=0.05)


def _carried(name):
    def make():
        c = FC.case(name)
        return SimpleNamespace(batch=with_rules(c.batch), stop_T=c.stop_T, d_targets=c.d_targets, max_decel=c.max_decel, best_idx=c.best_idx, skip=c.skip,
                               obey=ALL)
    return make


def straight(ego, n_obs=1, T_obs=80, length=90.0, NX=19, d_samples=(-0.8, 0.0, 0.8)):
    """A straight line along x with one frame and one scene shared by all egos; the obstacle columns hold no state (fill them in)."""
    from fiss_plus_planner_amd.batch import ProblemBatch
    from fiss_plus_planner_amd.spline import build_frames
    from fiss_plus_planner_amd.vehicle import Vehicle

    ego = np.atleast_2d(np.asarray(ego, dtype=np.float64))
    B = len(ego)
    veh = Vehicle()
    pts = np.zeros((1, NX, 2))
    pts[0, :, 0] = np.linspace(0.0, length, NX)
    knots, coef = build_frames(pts)
    return ProblemBatch(d_samples=np.asarray(d_samples), t_samples=np.array([4.0, 5.0]), v_samples=np.tile(np.array([4.0, 8.0]), (B, 1)),
                        target_speed=np.full(B, 8.0), ego=ego, frame_of=np.zeros(B), scene_of=np.zeros(B), t_now=np.zeros(B), nx=[NX], knots=knots, coef=coef,
                        obs_pose=np.zeros((1, T_obs, n_obs, 4)), obs_dims=np.full((1, n_obs, 2), 2.0), final_time_step=[T_obs - 1], veh_l=veh.l, veh_w=veh.w,
                        max_speed=veh.max_speed, max_accel=veh.max_accel, tick_t=0.1, check_stride=2)


ANALYTIC_S0, ANALYTIC_V0, ANALYTIC_AHEAD, ANALYTIC_NEAR = 10.0, 8.0, 14.0, 5.0


def _analytic(max_decel):
    def make():
        from fiss_plus_planner_amd.spline import gate_bits

        b = straight([[ANALYTIC_S0, ANALYTIC_V0, 0, 0, 0, 0], [0.0, ANALYTIC_V0, 0, 0, 0, 0]])
        front = 0.5 * b.veh_l
        line = ANALYTIC_S0 + front + ANALYTIC_AHEAD
        b.ego[1, 0] = line - front - ANALYTIC_NEAR
        b = dataclasses.replace(b, gate_s=np.array([[line]]), gate_closed=gate_bits(np.ones((1, 1, 1), dtype=bool)), gate_front=front, gate_max_decel=4.0)
        return SimpleNamespace(batch=b, stop_T=STOP_T, d_targets=np.array([np.nan, -0.5, 0.5]), max_decel=max_decel, best_idx=np.full(2, -1, dtype=np.int32),
                               skip=None, obey=("gates",))
    return make


def corridor():
    """d0 = 0.3, targets 0.9 and -0.6: rule-blind the nearer target 0.9 wins (every stop is clear, the lateral key decides); the corridor's
    left edge at 1.6 m cuts it off (0.9 + veh_w / 2 > 1.6) and the obeying call goes to -0.6, which the right edge at -3 m allows."""
    b = straight([[10.0, 8.0, 0, 0.3, 0, 0]])
    edge = np.full(b.knots.shape, 1.6)
    b = dataclasses.replace(b, bound_left=edge, bound_right=np.full(b.knots.shape, -3.0), bound_margin=0.0)
    return SimpleNamespace(batch=b, stop_T=STOP_T, d_targets=np.array([0.9, -0.6]), max_decel=np.inf, best_idx=np.full(1, -1, dtype=np.int32), skip=None,
                           obey=("boundary",))


def fewest_rules():
    """The corridor fixture behind a gate 5 m ahead that is closed throughout and not waived: every stop crosses it.  The stops to 0.9
    also leave the corridor (two rules), the stops to -0.6 do not (one): the number of rules broken decides before the lateral key,
    which alone would take the nearer target 0.9."""
    from fiss_plus_planner_amd.spline import gate_bits

    c = corridor()
    b = c.batch
    front = 0.5 * b.veh_l
    c.batch = dataclasses.replace(b, gate_s=np.array([[b.ego[0, 0] + front + 5.0]]), gate_closed=gate_bits(np.ones((1, 1, 1), dtype=bool)), gate_front=front)
    c.obey = ("gates", "boundary")
    return c


def zero_limit():
    """The limit is 0 from the knot at s = 30 m on (17.75 m in front of the bumper), no limit before it: the 24 m stop drives into it."""
    b = straight([[10.0, 8.0, 0, 0, 0, 0]])
    lim = np.where(b.knots >= 30.0, 0.0, np.inf)
    b = dataclasses.replace(b, speed_limit=lim, limit_front=0.5 * b.veh_l, limit_tol=0.05)
    return SimpleNamespace(batch=b, stop_T=STOP_T, d_targets=np.array([np.nan]), max_decel=np.inf, best_idx=np.full(1, -1, dtype=np.int32), skip=None,
                           obey=("envelope",))


GAP_S0 = 31.5


def time_gap():
    """A column ahead brakes from 3 m/s to a crawl of 1 m/s.  Every stop ends clear of it, but the 24 m stop ends 1 m behind its rear
    bumper - where the column stood 1 s before, inside the time gap of 2 s; the 18 m stop ends 5.5 m behind it."""
    b = straight([[10.0, 8.0, 0, 0, 0, 0]], n_obs=1, T_obs=80)
    t = 0.1 * np.arange(b.T_obs)
    s_o = GAP_S0 + np.where(t < 2.0, 3.0 * t - 0.5 * t * t, 2.0 + t)
    b.obs_pose[0, :, 0] = np.stack([s_o, np.zeros_like(t), np.zeros_like(t), np.ones_like(t)], axis=1)
    b.obs_dims[0, 0] = (b.veh_l, 1.8)
    b = PR.with_gap(b, follow=20, lead=0, first=2)
    return SimpleNamespace(batch=b, stop_T=STOP_T, d_targets=np.array([np.nan]), max_decel=np.inf, best_idx=np.full(1, -1, dtype=np.int32), skip=None,
                           obey=("gaps",))


def all_contact():
    """A wall 7 m in front of the bumper: every candidate hits, no rule is consulted (the gate behind the wall is closed throughout)."""
    from fiss_plus_planner_amd.spline import gate_bits

    b = straight([[10.0, 10.0, 0, 0, 0, 0]])
    front = 0.5 * b.veh_l
    b.obs_pose[0, :, 0] = (10.0 + front + 7.0 + 1.0, 0.0, 0.0, 1.0)
    b.obs_dims[0, 0] = (2.0, 9.0)
    b = dataclasses.replace(b, gate_s=np.array([[10.0 + front + 3.0]]), gate_closed=gate_bits(np.ones((1, 1, 1), dtype=bool)), gate_front=front)
    return SimpleNamespace(batch=b, stop_T=STOP_T, d_targets=FC.D3, max_decel=np.inf, best_idx=np.full(1, -1, dtype=np.int32), skip=None, obey=("gates",))


FIXTURES = {name: _carried(name) for name in FC.FIXTURES}
FIXTURES.update({"analytic": _analytic(np.inf), "analytic soft": _analytic(3.0), "corridor": corridor, "fewest rules": fewest_rules, "zero limit": zero_limit, "time gap": time_gap,
                 "all contact": all_contact})


@functools.lru_cache(maxsize=None)
def case(name):
    """The fixture (built once; nobody writes to it)."""
    return FIXTURES[name]()


_REFS = {}


def reference(O, name, obey=None):
    """fallback_rules_ref.fallback_rules of the fixture (obey: the fixture's own by default), computed once per process."""
    c = case(name)
    obey = tuple(c.obey if obey is None else obey)
    if (name, obey) not in _REFS:
        _REFS[name, obey] = FRR.fallback_rules(O, c.batch, c.stop_T, c.d_targets, c.max_decel, obey, best_idx=c.best_idx, skip=c.skip)
    return _REFS[name, obey]


def blind(O, name):
    """fallback_ref.fallback (the rule-blind call) of the fixture, computed once per process."""
    if (name, "blind") not in _REFS:
        c = case(name)
        _REFS[name, "blind"] = FR.fallback(O, c.batch, c.stop_T, c.d_targets, c.max_decel, best_idx=c.best_idx, skip=c.skip)
    return _REFS[name, "blind"]


def silent(batch):
    """`batch` with a rule set that cannot speak: limits +inf, a gate that is never closed, a corridor 1 km wide (the caller adds lags
    where the batch has no obstacle)."""
    from fiss_plus_planner_amd.spline import gate_bits

    F = batch.F
    wide = np.full(batch.knots.shape, 1000.0)
    return dataclasses.replace(batch, speed_limit=np.full(batch.knots.shape, np.inf), limit_front=0.0, limit_tol=0.0, max_lat_accel=0.0,
                               gate_s=np.full((F, 1), 20.0), gate_closed=gate_bits(np.zeros((F, 4, 1), dtype=bool)), gate_front=0.0, gate_max_decel=0.0,
                               bound_left=wide, bound_right=-wide, bound_margin=0.0)


# ---------------------------------------------------------------------------
# the closed-loop scenario: fallback_cases.loop_scenario() with a gate instead of the wall
# ---------------------------------------------------------------------------
LOOP_LINE = 45.0    # m: the stop line
K_CLOSE = 24        # the gate is closed in steps K_CLOSE .. K_OPEN - 1
K_OPEN = 90
LOOP_CYCLES = 230
LOOP_STOP_T = np.array([2.0, 3.0, 4.0, 6.0, 8.0])  # (the gentlest stop covers 4 v0 = 32 m: further than the line is away when the lattice gives up)
T_GATE = 128


def loop_scenario():
    """-> (batch, goal_xy): the four egos of fallback_cases.loop_scenario on its 90 m line, the wall gone, a gate at LOOP_LINE that closes
    at step K_CLOSE - while the egos approach, close enough that every lattice candidate crosses it - and opens at K_OPEN.  No waiver."""
    from fiss_plus_planner_amd.spline import gate_bits

    batch, goal_xy = FC.loop_scenario()
    batch.obs_pose[..., 3] = 0.0
    closed = np.zeros((1, T_GATE, 1), dtype=bool)
    closed[0, K_CLOSE:K_OPEN, 0] = True
    batch = dataclasses.replace(batch, gate_s=np.array([[LOOP_LINE]]), gate_closed=gate_bits(closed), gate_front=0.5 * batch.veh_l, gate_max_decel=0.0)
    return batch, goal_xy


_LOOPS = {}


def loop_reference(O, obey, cycles=LOOP_CYCLES):
    """The scenario driven on the CPU: the oracle's dense tables masked by gates_ref.ego_gates, the fallback for the egos that leaves
    without a plan - rule-blind (fallback_ref, obey=False) or obeying the gates (fallback_rules_ref, obey=True) - and advance_ref's
    hand-over.  -> SimpleNamespace(states [cycles + 1, B, 6], done, cycles [B], status [cycles, B], counts [B, 4], rule_counts [B, 5],
    undecided, crossed_closed [B] (cycles in which the front bumper moved over the line into a closed step))."""
    import advance_ref as AR

    if obey in _LOOPS:
        return _LOOPS[obey]
    batch, goal_xy = loop_scenario()
    B = batch.B
    front, line = float(batch.gate_front), LOOP_LINE
    ego, t_now, done, ncyc = batch.ego.copy(), batch.t_now.copy(), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    states = np.full((cycles + 1, B, 6), np.nan)
    states[0] = ego
    status = np.full((cycles, B), -1, dtype=np.int32)
    counts, rule_counts = np.zeros((B, 4), dtype=np.int32), np.zeros((B, 5), dtype=np.int32)
    crossed = np.zeros(B, dtype=np.int32)
    undecided = 0
    for k in range(cycles):
        if (done != 0).all():
            break
        now = dataclasses.replace(batch, ego=ego.copy(), t_now=t_now.copy())
        best = np.full(B, -1, dtype=np.int32)
        for b in range(B):
            if not done[b]:
                g = GR.ego_gates(O, now, b)
                best[b] = g.best_idx
                undecided += int(g.undecided.any())
        if obey:
            r = FRR.fallback_rules(O, now, LOOP_STOP_T, None, np.inf, ("gates",), best_idx=best, skip=done)
            rule_counts += r.rule_counts
        else:
            r = FR.fallback(O, now, LOOP_STOP_T, None, np.inf, best_idx=best, skip=done)
        counts += r.counts
        status[k] = np.where(done != 0, -1, r.status)
        undecided += int((r.need & ~r.counted).sum())
        for b in range(B):
            a = AR.advance(O, tick_t=batch.tick_t, veh_l=batch.veh_l, knots=batch.knots[0], coef=batch.coef[0], ego=ego[b], t_now=t_now[b], cycles=ncyc[b],
                           done=done[b], end_state=r.end_state[b], goal_xy=goal_xy[b])
            if a.moved:
                word = int(batch.gate_closed[0, min(a.t_now, T_GATE - 1)])
                crossed[b] += int(ego[b, 0] + front <= line < a.ego[0] + front and word & 1)
                states[k + 1, b] = a.ego
            ego[b], t_now[b], ncyc[b], done[b] = a.ego, a.t_now, a.cycles, a.done
    _LOOPS[obey] = SimpleNamespace(states=states, done=done, cycles=ncyc, status=status, counts=counts, rule_counts=rule_counts, undecided=undecided,
                                   crossed_closed=crossed)
    return _LOOPS[obey]


# ---------------------------------------------------------------------------
# the same scenario under FISS+ with the gates enforced (fp_plan_fiss_rules, loop = NULL) and the fallback that obeys them
# ---------------------------------------------------------------------------
def fiss_loop_scenario():
    """loop_scenario() with the FISS sampling box of its lattice (range and spacing of the samples, as fiss_rules_ref.loop_batch)."""
    b, goal_xy = loop_scenario()
    d, t, v = np.asarray(b.d_samples), np.asarray(b.t_samples), np.asarray(b.v_samples)
    one = np.ones(b.B)
    b = dataclasses.replace(b, samp_min=np.column_stack([one * d.min(), v.min(axis=1), one * t.min()]),
                            samp_max=np.column_stack([one * d.max(), v.max(axis=1), one * t.max()]),
                            samp_res=np.column_stack([one * (d[1] - d[0]), v[:, 1] - v[:, 0], one * (t[1] - t[0])]))
    return b, goal_xy


def fiss_loop_reference(O, cycles=LOOP_CYCLES):
    """The scenario driven on the CPU under FISS+: fiss_rules_ref.plan with the gates enforced (prev_best_idx carried along), the fallback
    that obeys the gates for the egos it leaves without an end state, advance_ref's hand-over.  -> loop_reference's namespace, and
    first_undecided [B]: the first cycle whose plan or fallback the reference could not decide for that ego (a cost gap below
    fiss_rules_ref.COST_TOL between two refined candidates, a verdict on its threshold) - two implementations may part there, as in
    fiss_rules_ref.ref_loop; `cycles` + 1 when there is none."""
    import advance_ref as AR
    import fiss_rules_ref as FRF

    if "fiss" in _LOOPS:
        return _LOOPS["fiss"]
    batch, goal_xy = fiss_loop_scenario()
    B = batch.B
    front, line = float(batch.gate_front), LOOP_LINE
    ego, t_now, done, ncyc = batch.ego.copy(), batch.t_now.copy(), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    prev = [None] * B
    states = np.full((cycles + 1, B, 6), np.nan)
    states[0] = ego
    status = np.full((cycles, B), -1, dtype=np.int32)
    counts, rule_counts = np.zeros((B, 4), dtype=np.int32), np.zeros((B, 5), dtype=np.int32)
    crossed = np.zeros(B, dtype=np.int32)
    first_undecided = np.full(B, cycles + 1, dtype=np.int32)
    undecided = 0
    for k in range(cycles):
        if (done != 0).all():
            break
        now = dataclasses.replace(batch, ego=ego.copy(), t_now=t_now.copy())
        es = np.full((B, 3), np.nan)
        for b in range(B):
            if not done[b]:
                r = FRF.plan(O, now, b, "FISS+", ("gates",), prev[b])
                es[b], prev[b] = r.end_state, r.prev_best_idx
                undecided += int(r.undecided)
                if r.undecided:
                    first_undecided[b] = min(first_undecided[b], k)
        r = FRR.fallback_rules(O, now, LOOP_STOP_T, None, np.inf, ("gates",), end_state=es, skip=done)
        rule_counts += r.rule_counts
        counts += r.counts
        status[k] = np.where(done != 0, -1, r.status)
        undecided += int((r.need & ~r.counted).sum())
        first_undecided[r.need & ~r.counted] = np.minimum(first_undecided[r.need & ~r.counted], k)
        for b in range(B):
            a = AR.advance(O, tick_t=batch.tick_t, veh_l=batch.veh_l, knots=batch.knots[0], coef=batch.coef[0], ego=ego[b], t_now=t_now[b], cycles=ncyc[b],
                           done=done[b], end_state=r.end_state[b], goal_xy=goal_xy[b])
            if a.moved:
                word = int(batch.gate_closed[0, min(a.t_now, T_GATE - 1)])
                crossed[b] += int(ego[b, 0] + front <= line < a.ego[0] + front and word & 1)
                states[k + 1, b] = a.ego
            ego[b], t_now[b], ncyc[b], done[b] = a.ego, a.t_now, a.cycles, a.done
    _LOOPS["fiss"] = SimpleNamespace(states=states, done=done, cycles=ncyc, status=status, counts=counts, rule_counts=rule_counts, undecided=undecided,
                                     crossed_closed=crossed, first_undecided=first_undecided)
    return _LOOPS["fiss"]
