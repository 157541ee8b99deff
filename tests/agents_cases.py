"""Fixtures of the shared-plans tests (fp_obstacles_from_plans): the smallest shapes at which the kernel can still go wrong, and the
closed-loop scenarios.  Each case is a SimpleNamespace(batch, groups, n_rows, tail, col_base, best_idx | end_state, skip).

    analytic        one group of 2 on a straight line along x: x = s, y = d, yaw = 0; the expected table is written out by hand (hand_table)
    ragged          groups of 1, 2, 3 and 5 plus one ego in no group; members non-contiguous and permuted against ego order, every ego on its
                    own curved frame; col_base = 2 behind two static columns, one trailing column behind; t_now differs between groups and
                    one group's rows are clipped by T_obs
    kinds idx / es  the same plans as lattice indices and as end states: a plain plan, index -1 / a NaN end state, a skipped ego, a plan
                    that leaves its line (M < N; under each tail: kinds ... none / hold / coast) and one with M < 2
    wide            one group of 65 (more than a wavefront of sources, more than 64 columns) at n_rows = 130, 129 points per plan
    stopping        v0 = 8 -> v_end = 0 within 4 s (shortest step ~3.5 mm) beside a standing ego (steps exactly zero, yaw exactly 0)
"""
import dataclasses
from types import SimpleNamespace

import numpy as np

from fiss_plus_planner_amd import synth
from fiss_plus_planner_amd.agents import TAILS, AgentGroups
from fiss_plus_planner_amd.batch import ProblemBatch
from fiss_plus_planner_amd.spline import build_frames
from fiss_plus_planner_amd.vehicle import Vehicle


def straight_batch(ego, v_samples, target, t_samples=(2.0, 4.0), length=190.0, NX=39, nd=3):
    """Egos on one straight line along the x axis (x = s, y = d), no scenes yet."""
    veh = Vehicle()
    ego = np.asarray(ego, dtype=np.float64)
    B = len(ego)
    pts = np.zeros((1, NX, 2))
    pts[0, :, 0] = np.linspace(0.0, length, NX)
    knots, coef = build_frames(pts)
    sw = 3.5 - veh.w
    return ProblemBatch(d_samples=np.linspace(-sw / 2, sw / 2, nd), t_samples=np.asarray(t_samples, dtype=np.float64), v_samples=np.asarray(v_samples, dtype=np.float64),
                        target_speed=np.asarray(target, dtype=np.float64), ego=ego, frame_of=np.zeros(B), scene_of=np.full(B, -1), t_now=np.zeros(B), nx=[NX],
                        knots=knots, coef=coef, obs_pose=np.zeros((0, 1, 0, 4)), obs_dims=np.zeros((0, 0, 2)), final_time_step=np.zeros(0), veh_l=veh.l, veh_w=veh.w,
                        max_speed=veh.max_speed, max_accel=veh.max_accel, tick_t=0.1, check_stride=2)


def _case(batch, groups, n_rows, tail, col_base=0, best_idx=None, end_state=None, skip=None):
    return SimpleNamespace(batch=batch, groups=groups, n_rows=n_rows, tail=TAILS[tail], col_base=col_base, best_idx=None if best_idx is None else np.asarray(best_idx, dtype=np.int32),
                           end_state=None if end_state is None else np.asarray(end_state, dtype=np.float64), skip=None if skip is None else np.asarray(skip, dtype=np.int32),
                           agents=AgentGroups(groups, n_rows, tail, col_base))


# ---- 1. analytic
AN_T_NOW, AN_ROWS, AN_T_OBS = 2, 24, 30
AN_EGO = np.array([[5.0, 5.0, 0.0, 0.0, 0.0, 0.0], [20.0, 4.0, 0.0, 0.5, 0.0, 0.0]])
AN_END = np.array([[0.0, 5.0, 2.0], [0.5, 4.0, 2.0]])  # constant speed, constant offset: s = s0 + v t, d = d0


def analytic():
    b = straight_batch(AN_EGO, [[0.0, 5.0], [0.0, 4.0]], [5.0, 4.0])
    ag = AgentGroups([[0, 1]], AN_ROWS, "coast")
    b = ag.attach(b, AN_T_OBS)
    b.t_now[:] = AN_T_NOW
    return _case(b, [[0, 1]], AN_ROWS, "coast", end_state=AN_END)


def hand_table():
    """The table of `analytic`, written out: ego 0 is column 0 of ego 1's scene (scene 1) and the other way round; 20 points of the
    plan (T = 2 s), then the last step repeated; rows 2 .. 25; an ego's own column in its own scene is zeros."""
    pose = np.zeros((2, AN_T_OBS, 2, 4))
    for src, dst in ((0, 1), (1, 0)):
        s0, v, d = AN_EGO[src, 0], AN_EGO[src, 1], AN_EGO[src, 3]
        for i in range(AN_ROWS):
            pose[dst, AN_T_NOW + i, src] = (s0 + v * (i * 0.1), d, 0.0, 1.0)
    written = np.zeros((2, AN_T_OBS, 2), dtype=bool)
    written[:, AN_T_NOW:AN_T_NOW + AN_ROWS, :] = True
    return pose, written, np.array([AN_T_NOW + AN_ROWS] * 2)


# ---- 2. ragged
RAGGED_GROUPS = [[7], [3, 0], [9, 1, 5], [11, 2, 8, 6, 4]]  # ego 10 is in no group


def _moving_indices(batch, rng):
    """One lattice index per ego whose end speed is not the lowest sample (0 m/s): no plan of the fixture comes to a stop."""
    i_d, i_t, i_v = rng.integers(0, batch.nd, batch.B), rng.integers(0, batch.nt, batch.B), rng.integers(1, batch.nv, batch.B)
    return ((i_d * batch.nt + i_t) * batch.nv + i_v).astype(np.int32)


def ragged():
    rng = np.random.default_rng(20240611)
    b = synth.make_batch(12, 3, 3, 2, 2, 40, True, seed=7101)
    ag = AgentGroups(RAGGED_GROUPS, 60, "hold", col_base=2)
    b = ag.attach(b, 100, extra_cols=1)
    t_now = np.zeros(12, dtype=np.int32)
    for g, t in zip(RAGGED_GROUPS, (3, 0, 11, 70)):  # (the last group: 70 + 60 > T_obs = 100, its rows are clipped)
        t_now[g] = t
    t_now[10] = 5
    b.t_now[:] = t_now
    return _case(b, RAGGED_GROUPS, 60, "hold", col_base=2, best_idx=_moving_indices(b, rng))


# ---- 3. plan kinds
def kinds(as_index: bool, tail: str):
    rng = np.random.default_rng(99)
    b = synth.make_batch(8, 3, 3, 2, 0, 1, False, seed=7202)
    b.ego[3, 0] = b.knots[3, b.nx[3] - 1] - 30.0  # leaves its line within the plan: M < N
    b.ego[3, 1] = 9.0
    b.ego[4, 0] = b.knots[4, b.nx[4] - 1] - 0.01  # point 0 on the line, point 1 beyond it: M = 1
    b.ego[4, 1] = 5.0
    groups = [[0, 1, 2, 3], [7, 6, 5, 4]]
    ag = AgentGroups(groups, 110, tail)
    b = ag.attach(b, 120)
    b.t_now[:] = (0, 0, 0, 0, 4, 4, 4, 4)
    idx = _moving_indices(b, rng)
    idx[1] = -1
    skip = np.zeros(8, dtype=np.int32)
    skip[2] = 1
    if as_index:
        return _case(b, groups, 110, tail, best_idx=idx, skip=skip)
    es = np.array([[np.nan] * 3 if c < 0 else [b.d_samples[c // (b.nv * b.nt)], b.v_samples[e, c % b.nv], b.t_samples[(c // b.nv) % b.nt]] for e, c in enumerate(idx)])
    return _case(b, groups, 110, tail, end_state=es, skip=skip)


# ---- 4. wide
def wide():
    rng = np.random.default_rng(5)
    b = synth.make_batch(65, 3, 3, 2, 0, 1, False, seed=7303)
    b = dataclasses.replace(b, t_samples=np.array([8.0, 12.85]), samp_max=None, samp_min=None, samp_res=None)  # 129 points at tick 0.1: beyond the fast paths' 128
    groups = [list(rng.permutation(65))]
    ag = AgentGroups(groups, 130, "coast")
    b = ag.attach(b, 140)
    b.t_now[:] = 6
    return _case(b, groups, 130, "coast", best_idx=_moving_indices(b, rng))


# ---- 5. stopping
def stopping():
    ego = np.array([[10.0, 8.0, 0.0, 0.2, 0.0, 0.0], [60.0, 0.0, 0.0, -0.4, 0.0, 0.0], [100.0, 6.0, 0.0, 0.0, 0.0, 0.0]])
    b = straight_batch(ego, [[0.0, 8.0], [0.0, 8.0], [0.0, 6.0]], [8.0, 8.0, 6.0])
    groups = [[2, 0, 1]]
    ag = AgentGroups(groups, 48, "hold")
    b = ag.attach(b, 50)
    b.t_now[:] = 1
    es = np.array([[0.2, 0.0, 4.0], [-0.4, 0.0, 4.0], [0.0, 6.0, 4.0]])  # ego 0 brakes to a stop, ego 1 stands, ego 2 cruises
    return _case(b, groups, 48, "hold", end_state=es)


FIXTURES = {"analytic": analytic, "ragged": ragged, "wide": wide, "stopping": stopping}
for _t in ("none", "hold", "coast"):
    FIXTURES[f"kinds idx {_t}"] = (lambda t: lambda: kinds(True, t))(_t)
    FIXTURES[f"kinds es {_t}"] = (lambda t: lambda: kinds(False, t))(_t)

_cache = {}


def case(name):
    """The fixture (built once; tests do not modify it)."""
    if name not in _cache:
        _cache[name] = FIXTURES[name]()
    return _cache[name]


_refs = {}


def reference(O, name):
    """agents_ref.table of the fixture on a table pre-filled with SENTINEL (computed once, shared by the tests, never modified)."""
    import agents_ref as GR

    if name not in _refs:
        c = case(name)
        _refs[name] = GR.table(O, c.batch, c.groups, c.n_rows, c.tail, c.col_base, best_idx=c.best_idx, end_state=c.end_state, skip=c.skip,
                               obs_pose=sentinel_table(c.batch), final_time_step=np.full(c.batch.S, SENTINEL_FTS, dtype=np.int32))
    return _refs[name]


SENTINEL = np.frombuffer(np.uint64(0x7FF8DEADBEEF1234).tobytes(), dtype=np.float64)[0]  # a NaN with a payload: no computed value has these bits
SENTINEL_FTS = -12345


def sentinel_table(batch):
    return np.full(batch.obs_pose.shape, SENTINEL)


# ---------------------------------------------------------------------------
# closed-loop scenarios: egos on one lane, the rear one with the higher target speed
# ---------------------------------------------------------------------------
LOOP_STOP_T = np.array([2.0, 3.0, 4.0])
LOOP_T_OBS = 160
LOOP_ROWS = 60     # the longest plan has 50 points (T = 5 s; the longest stop 40): N + 1 rows and some
LOOP_CYCLES = 60


def loop_scenario(kind="follower", attach=True, kindp="FOP"):
    """follower: two egos 22 m apart on a straight 300 m line, the rear one at 11 m/s with target 11, the front one at 4 with target 4.
    platoon: three egos, rear to front at 12 / 8 / 4 m/s.  One group; -> (batch, goal_xy [B, 2], AgentGroups)"""
    if kind == "follower":
        s0, v0 = (10.0, 32.0), (11.0, 4.0)
    else:
        s0, v0 = (10.0, 36.0, 60.0), (12.0, 8.0, 4.0)
    B = len(s0)
    ego = np.zeros((B, 6))
    ego[:, 0], ego[:, 1] = s0, v0
    v_samples = np.stack([np.linspace(0.0, v, 5) for v in v0])
    b = straight_batch(ego, v_samples, v0, t_samples=(3.0, 5.0), length=300.0, NX=61)
    if kindp != "FOP":
        sw = 3.5 - b.veh_w + 0.3
        b = dataclasses.replace(b, d_samples=np.linspace(-sw / 2, sw / 2, 3), samp_min=np.column_stack([np.full(B, -sw / 2), np.zeros(B), np.full(B, 3.0)]),
                                samp_max=np.column_stack([np.full(B, sw / 2), np.asarray(v0), np.full(B, 5.0)]),
                                samp_res=np.column_stack([np.full(B, sw / 2), np.asarray(v0) / 4, np.full(B, 2.0)]))
    ag = AgentGroups([list(range(B))], LOOP_ROWS, "coast")
    if attach:
        b = ag.attach(b, LOOP_T_OBS)
    return b, np.full((B, 2), 1e6), ag
