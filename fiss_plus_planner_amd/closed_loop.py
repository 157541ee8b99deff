"""Closed-loop simulation harness = the planning loop of the reference's planners/benchmark/planning.py:101-162
(frenet frame, initial Cartesian->Frenet projection, `for i in range(final_time_step): plan(...)`, next state = point 1
of the winner, the three stop rules) without its commonroad / matplotlib dependencies.

Inputs are plain arrays: centerline [n,2], initial state (x, y, yaw, v), an ObstacleTable, the goal-lanelet centre.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np

from .frenet import FrenetState, State
from .obstacles import ObstacleTable
from .planners import Stats


@dataclass
class CycleRecord:
    start: list           # s, s_d, s_dd, d, d_d, d_dd fed to plan()
    cost: float
    N: int
    M: int
    idx: np.ndarray
    stats: tuple
    end: list             # end state (d, v, T) of the winner
    seconds: float        # wall time of plan(), measured where the reference measures it (planning.py:124-128)


@dataclass
class ClosedLoopResult:
    cycles: list = field(default_factory=list)
    states: list = field(default_factory=list)   # x, y, yaw after every cycle
    goal_reached: bool = False
    stats: Stats = field(default_factory=Stats)

    @property
    def plan_seconds(self):
        return np.array([c.seconds for c in self.cycles])


@dataclass
class LoopLog:
    """The driven trajectory of a device-resident loop, as fp_loop_record (include/frenet_gpu.h) leaves it: plain numpy arrays.
    rows [B, max_rows, 16] (columns: _abi.LOG_*), n_rows [B] = cycles driven so far (rows past max_rows are counted, not written),
    row_stats [B, max_rows, 4] or None, stats_sum [B, 4] (the loop's `stats += planner.stats`, incl. the plan that found no solution).
    row0 [B] or None: the ego's row index when the log was reset (a runner that had already driven cycles), 0 when None."""
    rows: np.ndarray
    n_rows: np.ndarray
    row_stats: np.ndarray | None = None
    stats_sum: np.ndarray | None = None
    sealed: np.ndarray | None = None
    row0: np.ndarray | None = None

    @property
    def max_rows(self) -> int:
        return self.rows.shape[1]

    def span(self, b: int):
        """[first, end) of ego b's written rows"""
        return (0 if self.row0 is None else int(self.row0[b])), min(int(self.n_rows[b]), self.max_rows)

    def ego_rows(self, b: int) -> np.ndarray:
        lo, hi = self.span(b)
        return self.rows[b, lo:max(hi, lo)]

    def states(self, b: int) -> np.ndarray:
        """[n, 3] x, y, yaw after every recorded cycle of ego b = the reference's state_list positions (planning.py:135-148)"""
        from ._abi import LOG_X, LOG_YAW

        return self.ego_rows(b)[:, LOG_X:LOG_YAW + 1].copy()


def result_from_log(log: LoopLog, b: int, start=None) -> ClosedLoopResult:
    """What run_closed_loop returns, from ego b's rows of a device loop's log: states, one CycleRecord per recorded cycle (cost, Stats
    and end state of the plan that drove it; `start` = the previous row's Frenet state, or the caller's initial state - s, s_d, s_dd,
    d, d_d, d_dd - for the first row; the log does not hold N, M (-1) and knows the winner as the flat FOP index (idx = [flat], -1 for
    a trajectory that is no lattice sample); seconds = nan: nothing was timed per cycle), the summed Stats and goal_reached (the last
    driven cycle ended on one of the goal rules; a log that overflowed max_rows has lost that row: False)."""
    from . import _abi as A

    res = ClosedLoopResult()
    lo, hi = log.span(b)
    rows = log.ego_rows(b)
    prev = [float("nan")] * 6 if start is None else [float(v) for v in start]
    for i, r in enumerate(rows):
        st = tuple(int(v) for v in log.row_stats[b, lo + i]) if log.row_stats is not None else ()
        res.cycles.append(CycleRecord(prev, float(r[A.LOG_COST]), -1, -1, np.array([int(r[A.LOG_BEST_IDX])]), st,
                                      [float(r[A.LOG_D_END]), float(r[A.LOG_V_END]), float(r[A.LOG_T_END])], float("nan")))
        res.states.append([float(r[A.LOG_X]), float(r[A.LOG_Y]), float(r[A.LOG_YAW])])
        prev = [float(r[c]) for c in (A.LOG_S, A.LOG_VELOCITY, A.LOG_S_DD, A.LOG_D, A.LOG_VELOCITY_Y, A.LOG_D_DD)]
    if log.stats_sum is not None:
        res.stats = Stats(*(int(v) for v in log.stats_sum[b]))
    if len(rows) and int(log.n_rows[b]) <= log.max_rows:
        res.goal_reached = int(rows[-1][A.LOG_DONE]) in (A.DONE_GOAL, A.DONE_END_OF_LINE, A.DONE_GOAL_REGION)
    return res


def run_closed_loop(planner, centerline: np.ndarray, init_state, obstacles: ObstacleTable, goal_center, max_speed: float = 13.5,
                    max_cycles: int | None = None) -> ClosedLoopResult:
    sp, ref = planner.generate_frenet_frame(centerline)
    cur = FrenetState()
    if getattr(planner, "frame_on", "host") == "device":
        # Cartesian -> Frenet projection on the GPU (fp_from_state), same rules as FrenetState.from_state
        e = planner._engine.from_state(sp.knots[None], sp.coef[None], [len(sp.knots)], [0], np.asarray(init_state, dtype=np.float64)[None, :4])[0]
        cur = FrenetState(t=0.0, s=e[0], s_d=e[1], s_dd=e[2], d=e[3], d_d=e[4], d_dd=e[5])
    else:
        cur.from_state(State(t=0.0, x=init_state[0], y=init_state[1], yaw=init_state[2], v=init_state[3], a=0.0), ref)
    res = ClosedLoopResult()
    n_cycles = obstacles.final_time_step if max_cycles is None else min(max_cycles, obstacles.final_time_step)
    half_len = planner.vehicle.l / 2
    for i in range(n_cycles):
        start = [cur.s, cur.s_d, cur.s_dd, cur.d, cur.d_d, cur.d_dd]
        t0 = time.perf_counter()
        best = planner.plan(cur, max_speed, obstacles, i)
        dt = time.perf_counter() - t0
        res.stats += planner.stats
        if best is None:
            break
        cs = best.state_at_time_step(1)
        cur = best.frenet_state_at_time_step(1)
        es = best.end_state
        res.cycles.append(CycleRecord(start, best.cost_final, len(best.t), len(best.x), best.idx, planner.stats.as_tuple(),
                                      [es.d, es.s_d, es.t] if es is not None else [np.nan] * 3, dt))
        res.states.append([cs.x, cs.y, cs.yaw])
        if np.hypot(cs.x - goal_center[0], cs.y - goal_center[1]) <= half_len:     # planning.py:154-157
            res.goal_reached = True
            break
        if np.hypot(cs.x - ref[-1, 0], cs.y - ref[-1, 1]) <= 3.0:                   # planning.py:158-161
            res.goal_reached = True
            break
    return res
