"""The hand-over of one ego between two plan cycles, restated in plain Python from the reference's simulation loop
(planners/benchmark/planning.py:131-162) - the reference of tests/test_gpu_advance.py.  No GPU, no product code.

    best_traj_ego is None                                -> the run ends (:131-133)
    state_at_time_step(1), frenet_state_at_time_step(1)  -> the new Cartesian / Frenet state (:135-138); an IndexError ends the run
    state.time_step = i, the loop index                  (:139)
    goal_region.is_reached(state)                        (:150-153)
    hypot(position - goal_center) <= vehicle.l / 2       (:155-158)
    hypot(position - ref_ego_lane_pts[-1]) <= 3.0        (:159-162)

The trajectory is the oracle's (oracle.Problem.eval_traj with dump=True: its series are pinned bit for bit against the reference's
by the golden fixtures), column 1 of the dump is the state at time step 1.  The stop rules are the three lines above, in that order;
the region predicate is oracle.goal_reached, the last point of the resampled line is evaluated with oracle.spline2d_eval.

Every threshold the function evaluates is reported with its signed distance from the bound (`margins`): a case whose smallest
absolute margin is large against the arithmetic's error is decided the same way by every correct implementation.
"""
from types import SimpleNamespace

import numpy as np

RUNNING, DONE_GOAL, DONE_END_OF_LINE, DONE_NO_SOLUTION, DONE_GOAL_REGION = 0, 1, 2, 3, 4
STEP = 0.1  # generate_frenet_frame resamples the line every 0.1 m (frenet_optimal_planner.py:274)
END_OF_MAP = 3.0


def end_point_count(s_last):
    """Points of the resampled line: len(np.arange(0, s_last, 0.1)), less one when the last sample is >= s_last (the quotient
    s_last / 0.1 rounds up across an integer when s_last is within an ulp of a multiple of 0.1; the spline has no segment at s_last
    and the line loses that point - the rule of the state projection, restated).  Fewer than two points: 0, the line has no end point."""
    if not np.isfinite(s_last) or not s_last > 0.0:
        return 0
    pts = np.arange(0, s_last, STEP)
    n = len(pts)
    if n and pts[-1] >= s_last:
        n -= 1
    return n if n >= 2 else 0


def decode_index(best_idx, nd, nt, nv):
    """Flat index of the reference's sampling loops (frenet_optimal_planner.py:75-89): for d: for T: for v -> (id, it, iv)"""
    idd, it, iv = np.unravel_index(int(best_idx), (nd, nt, nv))
    return int(idd), int(it), int(iv)


def _interval_margins(name, v, lo, hi, out):
    """closed interval, a NaN bound = the goal state does not define the attribute"""
    if np.isnan(lo) or np.isnan(hi):
        return
    out[name + "_lo"] = v - lo
    out[name + "_hi"] = hi - v


def advance(O, *, tick_t, veh_l, knots, coef, ego, t_now, cycles=0, done=RUNNING, end_state=None, best_idx=None, d_samples=None,
            v_samples=None, t_samples=None, goal_xy=(1e9, 1e9), goal_poly=None, goal_nv=0, goal_max_vertices=0, goal_intervals=None,
            series_tol=None):
    """One hand-over.  O: the oracle module.  knots [nx], coef [8, nx]: the ego's frame.  ego [6], t_now, cycles, done: the loop state
    on entry.  The chosen trajectory: end_state = (d, v, T) (NaN = none), or best_idx (negative = none) with d_samples [nd],
    t_samples [nt] and the ego's v_samples [nv].  goal_poly [V, 2] with goal_nv vertices (outside 3 .. goal_max_vertices: no region),
    goal_intervals None or [6].
    -> ego [6], t_now, cycles, done, cart [3] (NaN when the ego did not move), moved, margins {name: signed distance}, yaw_tol (the
    bound on the heading for this step's ds; series_tol = conftest.series_tol), dump (the trajectory's [16, N] series or None)."""
    ego = np.array(ego, dtype=np.float64).reshape(6)
    out = SimpleNamespace(ego=ego.copy(), t_now=int(t_now), cycles=int(cycles), done=int(done), cart=np.full(3, np.nan), moved=False,
                          margins={}, yaw_tol=np.inf, dump=None, end_state=None)
    if out.done != RUNNING:
        return out
    if end_state is None:
        es = np.full(3, np.nan)
        if best_idx is not None and best_idx >= 0:
            idd, it, iv = decode_index(best_idx, len(d_samples), len(t_samples), len(v_samples))
            es = np.array([d_samples[idd], v_samples[iv], t_samples[it]], dtype=np.float64)
    else:
        es = np.array(end_state, dtype=np.float64).reshape(3)
    out.end_state = es
    if np.isnan(es).any():  # plan() returned None
        out.done = DONE_NO_SOLUTION
        return out
    knots = np.ascontiguousarray(knots, dtype=np.float64)
    nx = len(knots)
    cx, cy = np.ascontiguousarray(coef[0:4, :nx]), np.ascontiguousarray(coef[4:8, :nx])
    prob = O.Problem(d_samples=[0.0], v_samples=[1.0], t_samples=[1.0], tick_t=tick_t, target_speed=1.0, veh_l=veh_l, veh_w=1.0,
                     max_speed=1e9, max_accel=1e9, ego=ego, knots=knots, coef_x=cx, coef_y=cy)
    tr = prob.eval_traj(float(es[0]), float(es[1]), float(es[2]), collision=False, dump=True, stride=max(128, int(np.ceil(es[2] / tick_t)) + 1))
    if tr.N < 2 or tr.M < 2:  # state_at_time_step(1) / frenet_state_at_time_step(1) raise IndexError
        out.done = DONE_NO_SOLUTION
        return out
    a = tr.arrays
    out.dump = a[:, :tr.N]
    out.ego = a[1:9, 1][[0, 1, 2, 4, 5, 6]].copy()  # s, s_d, s_dd, d, d_d, d_dd
    x, y, yaw = a[9, 1], a[10, 1], a[11, 1]
    out.cart = np.array([x, y, yaw])
    out.moved = True
    if series_tol is not None:
        out.yaw_tol = float(series_tol(out.dump, tick_t)[11, 1])
    time_step = out.t_now  # state.time_step = i
    out.t_now += 1
    out.cycles += 1
    m = out.margins
    # goal_region.is_reached(state)
    if goal_poly is not None and 3 <= int(goal_nv) <= int(goal_max_vertices):
        poly = np.asarray(goal_poly, dtype=np.float64).reshape(-1, 2)[: int(goal_nv)]
        iv = None if goal_intervals is None else np.asarray(goal_intervals, dtype=np.float64).reshape(6)
        if iv is not None:
            _interval_margins("time_step", float(time_step), iv[0], iv[1], m)
            _interval_margins("velocity", out.ego[1], iv[2], iv[3], m)
            _interval_margins("orientation", yaw, iv[4], iv[5], m)
        m["polygon"] = polygon_margin(poly, x, y)
        if O.goal_reached(poly, x, y, time_step, out.ego[1], yaw, iv):
            out.done = DONE_GOAL_REGION
            return out
    m["goal_centre"] = float(np.hypot(x - goal_xy[0], y - goal_xy[1]) - veh_l / 2)
    if np.hypot(x - goal_xy[0], y - goal_xy[1]) <= veh_l / 2:
        out.done = DONE_GOAL
        return out
    n = end_point_count(knots[-1])
    if n:
        s_ref = np.arange(0, knots[-1], STEP)[n - 1]
        p = O.spline2d_eval(knots, cx, cy, s_ref)
        assert p is not None, (knots[-1], n)
        m["end_of_map"] = float(np.hypot(x - p[0], y - p[1]) - END_OF_MAP)
        if np.hypot(x - p[0], y - p[1]) <= END_OF_MAP:
            out.done = DONE_END_OF_LINE
    return out


def polygon_margin(poly, x, y):
    """Distance of (x, y) from the polygon's boundary (unsigned: the decidability of the containment test)"""
    p = np.asarray(poly, dtype=np.float64)
    q = np.roll(p, -1, axis=0)
    e = q - p
    w = np.array([x, y]) - p
    t = np.clip((w * e).sum(1) / np.maximum((e * e).sum(1), 1e-300), 0.0, 1.0)
    return float(np.min(np.hypot(*(w - t[:, None] * e).T)))


def decidability(margins):
    """The smallest absolute margin (m, m/s, rad) of a case, inf when no threshold was evaluated.  The time step is an integer compared
    with integers: exact in every implementation, not part of the measure."""
    return min((abs(v) for k, v in margins.items() if not k.startswith("time_step")), default=np.inf)
