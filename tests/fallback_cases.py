"""Fixtures of the fallback suites (tests/test_fallback_cpu.py, tests/test_gpu_fallback.py): small batches whose egos are placed by hand so
that each one reaches a named path of fp_fallback_stop, the call's arguments, and the restatement (tests/fallback_ref.py) computed once
per process and left unchanged.  tests/test_fallback_cpu.py proves on the CPU that every fixture reaches its paths and that the
restatement leaves out at most fallback_ref.MAX_LEFT_OUT egos of each."""
import functools
from types import SimpleNamespace

import numpy as np

import fallback_ref as FR
from fiss_plus_planner_amd import synth

STOP_T = np.array([2.0, 3.0, 4.5, 6.0])
D3 = np.array([np.nan, -0.6, 0.6])
LDS_BUDGET = 144 * 1024  # kFallbackLdsBytes: what launch_fallback_stop hands ego_lds_bytes


def place(batch, sc, j, s, d, length, width, rows=slice(None)):
    """Column j of scene sc parked at arclength s, lateral offset d of the scene's own line (frame sc), valid in `rows` only."""
    px, py, yaw = synth.sample_frames(batch.knots[sc:sc + 1], batch.coef[sc:sc + 1], np.array([[float(s)]]))
    x, y, yaw = float(px[0, 0]), float(py[0, 0]), float(yaw[0, 0])
    batch.obs_pose[sc, :, j] = (x - d * np.sin(yaw), y + d * np.cos(yaw), yaw, 0.0)
    batch.obs_pose[sc, rows, j, 3] = 1.0
    batch.obs_dims[sc, j] = (length, width)


def empty_scene(batch, sc):
    batch.obs_pose[sc, :, :, 3] = 0.0


def stop_s(ego, T, t):
    """s(t) of the longitudinal quartic from (s0, v0, a0) to v = 0, s_dd = 0 at T (the closed form of the header's comment)."""
    s0, v0, a0 = ego[0], ego[1], ego[2]
    V, A = -v0 - a0 * T, -a0
    a3, a4 = (3 * V - A * T) / (3 * T * T), (A * T - 2 * V) / (4 * T ** 3)
    return s0 + v0 * t + 0.5 * a0 * t * t + a3 * t ** 3 + a4 * t ** 4


def base():
    """B = 8, lattice 3 x 3 x 2, family 3 d x 4 T, 10 obstacles, T_obs 60, check_stride 2.
    ego 0  near the end of its line: the longer stops leave it (M < N)
    ego 1  brakes hard already (v0 = 5, a0 = -4) on an empty road: the long stop times reverse, a shorter clear one wins
    ego 2  a wall 7 m ahead: every candidate hits (CONTACT, the latest hit wins)
    ego 3  0.05 m before the end of the line: M = 1, nothing is admissible
    ego 4  has a plan (best_idx 5)            ego 5  skipped, with an index beyond the lattice that nobody may read
    ego 6  t_now = 7 among moving obstacles   ego 7  a wall it would reach at about step 12, but final_time_step - t_now = 9"""
    b = synth.make_batch(8, 3, 3, 2, 10, 60, True, 7101)
    last = b.knots[0, -1]
    b.ego[0, :3] = (last - 12.0, 9.0, 0.0)
    b.ego[1] = (30.0, 5.0, -4.0, 0.2, 0.0, 0.0)
    empty_scene(b, 1)
    b.ego[2, :3] = (40.0, 10.0, 0.0)
    empty_scene(b, 2)
    place(b, 2, 0, 40.0 + 7.0 + 0.5 * b.veh_l + 1.0, 0.0, 2.0, 9.0)
    b.ego[3, :3] = (b.knots[3, -1] - 0.05, 5.0, 0.0)
    b.t_now[6] = 7
    b.ego[7] = (20.0, 8.0, 0.0, 0.0, 0.0, 0.0)
    empty_scene(b, 7)
    place(b, 7, 0, stop_s(b.ego[7], 2.0, 1.2) + 0.5 * b.veh_l + 1.0, 0.0, 2.0, 9.0)
    b.final_time_step[7] = 9
    best_idx = np.array([-1, -1, -1, -1, 5, 10 ** 6, -1, -1], dtype=np.int32)
    skip = np.array([0, 0, 0, 0, 0, 1, 0, 0], dtype=np.int32)
    return SimpleNamespace(batch=b, stop_T=STOP_T, d_targets=D3, max_decel=np.inf, best_idx=best_idx, skip=skip)


def many_poses():
    """tick_t = 0.05, stop times up to 8 s (160 points), check_stride 1, B = 4: three rounds of 64 poses per candidate.  Egos 0 and 1 meet
    a wall where the 8 s stop is at its points 80 and 140 (a hit in the second and in the third round); ego 2 drives an empty road;
    ego 3 keeps the drawn scene."""
    b = synth.make_batch(4, 3, 3, 2, 6, 170, False, 7102)
    b.tick_t, b.check_stride = 0.05, 1
    b.t_samples = np.array([4.0, 8.0])
    stop_T = np.array([3.0, 5.0, 6.5, 8.0])
    for e, point in ((0, 80), (1, 140)):
        b.ego[e] = (20.0, 10.0, 0.0, 0.1, 0.0, 0.0)
        empty_scene(b, e)
        place(b, e, 0, stop_s(b.ego[e], 8.0, point * 0.05) + 0.5 * b.veh_l + 1.0, 0.0, 2.0, 9.0)
    empty_scene(b, 2)
    return SimpleNamespace(batch=b, stop_T=stop_T, d_targets=D3, max_decel=np.inf, best_idx=np.full(4, -1, dtype=np.int32), skip=None)


def off_lds():
    """48 obstacles x T_obs 200 at check_stride 1, B = 2: 128 rows x 48 columns x 32 bytes = 196 KB, past the kernel's budget - the rows
    are read from the scene table.  Ego 0 meets a wall (column 47, the last one: the walk passes every other column first)."""
    b = synth.make_batch(2, 3, 3, 2, 48, 200, True, 7103)
    b.check_stride = 1
    b.ego[0, :3] = (30.0, 9.0, 0.0)
    place(b, 0, 47, 30.0 + 9.0 + 0.5 * b.veh_l + 1.0, 0.0, 2.0, 9.0)
    return SimpleNamespace(batch=b, stop_T=STOP_T, d_targets=D3, max_decel=np.inf, best_idx=np.full(2, -1, dtype=np.int32), skip=None)


def ties():
    """Family [-0.6, +0.6] x 4 T, B = 4.  Ego 0 sits on the line (d0 = 0) with scene_of = -1: both targets are equally far, the smaller
    i_d wins.  Ego 1: the same on an empty scene.  Egos 2, 3 as drawn, with a deceleration bound of 4 m/s^2 that the short stops break."""
    b = synth.make_batch(4, 3, 3, 2, 4, 60, True, 7104)
    for e in (0, 1):
        b.ego[e] = (25.0 + e, 6.0, 0.0, 0.0, 0.0, 0.0)
    b.scene_of[0] = -1
    empty_scene(b, 1)
    return SimpleNamespace(batch=b, stop_T=STOP_T, d_targets=np.array([-0.6, 0.6]), max_decel=4.0, best_idx=np.full(4, -1, dtype=np.int32), skip=None)


def no_obstacles():
    """A batch without any scene (n_obs = 0, scene_of = -1), B = 2, and a family of one candidate (F = 1)."""
    b = synth.make_batch(2, 3, 3, 2, 0, 1, False, 7105)
    return SimpleNamespace(batch=b, stop_T=np.array([5.0]), d_targets=np.array([np.nan]), max_decel=np.inf, best_idx=np.full(2, -1, dtype=np.int32), skip=None)


def rings():
    """The drawn scenes with most columns turned into convex polygons, B = 4; egos 0 and 1 drive at a polygon column parked in their
    lane (a hexagon 9 m wide; ego 1 can no longer stop in front of it), so the contact verdicts are the ring's."""
    b = synth.make_batch(4, 3, 3, 2, 8, 60, True, 7106)
    for e in (0, 1):
        b.ego[e] = (30.0, 9.0 + e, 0.0, 0.1, 0.0, 0.0)
        place(b, e, 0, 30.0 + (10.0, 4.0)[e] + 0.5 * b.veh_l + 2.0, 0.0, 4.0, 9.0)
    b = synth.with_random_shapes(b, 7106, frac=0.7)
    ang = np.arange(6) * np.pi / 3
    for e in (0, 1):
        b.obs_poly[e, 0] = 0.0
        b.obs_poly[e, 0, :6] = np.stack([2.0 * np.cos(ang), 4.5 * np.sin(ang)], axis=1)
        b.obs_nvert[e, 0] = 6
        b.obs_dims[e, 0] = 2.0 * np.abs(b.obs_poly[e, 0, :6]).max(axis=0)
    return SimpleNamespace(batch=b, stop_T=STOP_T, d_targets=D3, max_decel=np.inf, best_idx=np.full(4, -1, dtype=np.int32), skip=None)


FIXTURES = {"base": base, "many poses": many_poses, "off LDS": off_lds, "ties": ties, "no obstacles": no_obstacles, "rings": rings}


@functools.lru_cache(maxsize=None)
def case(name):
    """The fixture (built once; nobody writes to it)."""
    return FIXTURES[name]()


_REFS = {}


def reference(O, name):
    """fallback_ref.fallback of the fixture, computed once per process."""
    if name not in _REFS:
        c = case(name)
        _REFS[name] = FR.fallback(O, c.batch, c.stop_T, c.d_targets, c.max_decel, best_idx=c.best_idx, skip=c.skip)
    return _REFS[name]


# ---------------------------------------------------------------------------
# csrc/frenet_ego.h restated: does the launch keep the obstacle rows in LDS?
# ---------------------------------------------------------------------------
def rows_in_lds(batch, cap):
    """ego_lds_bytes / lds_layout_doubles: (doubles of the full layout, True when the launch reserves them)."""
    cs = int(batch.check_stride)
    rows = min(-(-cap // cs), -(-batch.T_obs // cs))
    full = batch.NX * 9 + batch.n_obs * 4 + rows * batch.n_obs * 4
    return full, full * 8 <= LDS_BUDGET


# ---------------------------------------------------------------------------
# the closed-loop scenario: a wall across the whole sampling width that opens at step K_OPEN
# ---------------------------------------------------------------------------
K_OPEN = 80
LOOP_STOP_T = np.array([2.0, 3.0, 4.0])
LOOP_CYCLES = 220


def loop_scenario():
    """A straight 90 m line, B = 4 egos at about 8 m/s, a lattice 3 x 2 x 2 whose lowest speed sample is 4 m/s (no lattice candidate can
    stop), and a parked column 12 m wide across the road at s = 45 m, valid until step K_OPEN - 1 and gone afterwards.
    -> (batch, goal_xy [B, 2])"""
    from fiss_plus_planner_amd.batch import ProblemBatch
    from fiss_plus_planner_amd.spline import build_frames
    from fiss_plus_planner_amd.vehicle import Vehicle

    B, NX, T_obs = 4, 19, 120
    veh = Vehicle()
    pts = np.zeros((1, NX, 2))
    pts[0, :, 0] = np.linspace(0.0, 90.0, NX)
    knots, coef = build_frames(pts)
    ego = np.zeros((B, 6))
    ego[:, 0] = (5.0, 7.0, 9.0, 11.0)
    ego[:, 1] = (8.0, 7.5, 8.5, 8.0)
    ego[:, 3] = (0.0, 0.3, -0.3, 0.1)
    pose = np.zeros((1, T_obs, 1, 4))
    pose[0, :, 0] = (45.0, 0.0, 0.0, 0.0)
    pose[0, :K_OPEN, 0, 3] = 1.0
    sw = 3.5 - veh.w
    v_samples = np.tile(np.array([4.0, 8.0]), (B, 1))
    batch = ProblemBatch(d_samples=np.linspace(-sw / 2, sw / 2, 3), t_samples=np.array([4.0, 5.0]), v_samples=v_samples, target_speed=np.full(B, 8.0),
                         ego=ego, frame_of=np.zeros(B), scene_of=np.zeros(B), t_now=np.zeros(B), nx=[NX], knots=knots, coef=coef, obs_pose=pose,
                         obs_dims=np.array([[[2.0, 12.0]]]), final_time_step=[T_obs - 1], veh_l=veh.l, veh_w=veh.w, max_speed=veh.max_speed,
                         max_accel=veh.max_accel, tick_t=0.1, check_stride=2)
    goal_xy = np.tile(np.array([[1e6, 1e6]]), (B, 1))  # (no goal lanelet: the egos end at the end of the line)
    return batch, goal_xy


def loop_reference(O, fallback=True, cycles=LOOP_CYCLES):
    """The scenario driven on the CPU: the oracle's FOP plan, the restatement of the fallback for the egos it leaves without one, and
    advance_ref's hand-over, cycle by cycle.  -> SimpleNamespace(states [cycles + 1, B, 6] (NaN behind an ego's last cycle), done [B],
    cycles [B], status [cycles, B] (-1: the ego was finished), counts [B, 4], undecided (cycles whose fallback ego was not counted))."""
    import advance_ref as AR

    batch, goal_xy = loop_scenario()
    B = batch.B
    ego, t_now, done, ncyc = batch.ego.copy(), batch.t_now.copy(), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    states = np.full((cycles + 1, B, 6), np.nan)
    states[0] = ego
    status = np.full((cycles, B), -1, dtype=np.int32)
    counts = np.zeros((B, 4), dtype=np.int32)
    undecided = 0
    for k in range(cycles):
        if (done != 0).all():
            break
        batch.ego[...], batch.t_now[...] = ego, t_now
        best = np.array([-1 if done[b] else O.problems_from_batch(batch, egos=[b])[0].fop_plan().best_idx for b in range(B)], dtype=np.int32)
        if fallback:
            r = FR.fallback(O, batch, LOOP_STOP_T, None, np.inf, best_idx=best, skip=done)
            es = r.end_state
            counts += r.counts
            status[k] = np.where(done != 0, -1, r.status)
            undecided += int((r.need & ~r.counted).sum())
        else:
            es = np.array([FR.decode(batch, b, int(best[b])) if best[b] >= 0 else (np.nan,) * 3 for b in range(B)])
        for b in range(B):
            a = AR.advance(O, tick_t=batch.tick_t, veh_l=batch.veh_l, knots=batch.knots[0], coef=batch.coef[0], ego=ego[b], t_now=t_now[b], cycles=ncyc[b],
                           done=done[b], end_state=es[b], goal_xy=goal_xy[b])
            ego[b], t_now[b], ncyc[b], done[b] = a.ego, a.t_now, a.cycles, a.done
            if a.moved:
                states[k + 1, b] = a.ego
    return SimpleNamespace(states=states, done=done, cycles=ncyc, status=status, counts=counts, undecided=undecided)
