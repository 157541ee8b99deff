"""CPU: the definition of fp_traj_margins restated (tests/margins_ref.py) on hand-made cases with known answers, and the facts about
the fixture batches that let tests/test_gpu_margins.py compare min_step / min_obs exactly (decidability: no pair distance in
(0, 1e-6), at least 90 % of the plans with a pair separated from their runner-up by more than 1e-6 or in double contact)."""
import numpy as np
import pytest

import clearance_ref as CR
import margins_ref as MR
import rank_ref as R
from fiss_plus_planner_amd import synth
from fiss_plus_planner_amd.batch import ProblemBatch
from fiss_plus_planner_amd.spline import build_frames
from test_rank_cpu import oracle_tables

# The kernel gives every pose of a plan `split` lanes, which share the pose's columns round-robin (csrc/frenet_margins.hip): the
# largest power of two <= kMarginSplit = 8 with n_pose * split <= 64, so 8 for up to 8 poses, 4 for 9 .. 16, 2 for 17 .. 32, else 1.
# SPLIT_CASES: split -> the horizon (final_time_step at t_now = 0) that gives every plan 8, 16 and 32 poses at pose_stride 2; each runs
# with n_obs one below, at and one above its split (test_split_fixtures_reach_their_split asserts the pose counts from the reference).
SPLIT_STRIDE = 2
SPLIT_CASES = {8: 15, 4: 31, 2: 63}


def kernel_split(n_pose):
    """margins_kernel's lanes per pose for a plan of n_pose checked poses."""
    split = 1
    while split < 8 and n_pose * split * 2 <= 64:
        split *= 2
    return split


def _split(split, n_obs, seed):
    b = synth.make_batch(5, 5, 5, 5, n_obs, 100, True, seed)
    b.final_time_step[:] = SPLIT_CASES[split]
    return b

# one row more than fits the kernel's LDS budget at pose_stride 1 (kMarginLdsBytes = 144 KB: 128 rows x 40 obstacles x 32 bytes = 160 KB)
GLOBAL_SHAPE = (40, 130)


def _edges():
    """scene_of = -1 for ego 1, t_now at final_time_step - 1 (one pose) for ego 2 and beyond it (none) for ego 3; the GPU test also
    skips ego 4."""
    b = synth.make_batch(5, 5, 5, 5, 10, 100, True, 4101)
    b.scene_of[1] = -1
    b.t_now[2] = b.final_time_step[2] - 1
    b.t_now[3] = b.final_time_step[3] + 2
    return b


def _truncated():
    """egos 40 .. 4 m before the end of their 400 m lines: M < N for most plans, M = 2 .. for the last"""
    b = synth.make_batch(5, 5, 5, 5, 10, 100, True, 4102)
    b.ego[:, 0] = b.knots[:, -1] - np.array([40.0, 25.0, 12.0, 6.0, 1.5])
    return b


def _tick005():
    b = synth.make_batch(5, 5, 5, 5, 10, 200, True, 4103)
    b.tick_t = 0.05  # 160 .. 200 points per trajectory
    return b


# name -> (batch, pose strides the GPU test runs); every batch is 5 egos x 5 x 5 x 5
FIXTURES = {
    "1 obstacle": (lambda: synth.make_batch(5, 5, 5, 5, 1, 100, True, 4001), (1, 2, 5)),
    "3 obstacles": (lambda: synth.make_batch(5, 5, 5, 5, 3, 100, True, 4002), (1, 2, 5)),
    "50 obstacles": (lambda: synth.make_batch(5, 5, 5, 5, 50, 100, True, 4003), (1, 2, 5)),
    "rings": (lambda: synth.with_random_shapes(synth.make_batch(5, 5, 5, 5, 10, 100, True, 4004), 3), (1, 2)),
    "edges": (_edges, (1, 2)),
    "truncated": (_truncated, (1, 2)),
    "tick 0.05": (_tick005, (1, 5)),
    "rows beyond LDS": (lambda: synth.make_batch(5, 5, 5, 5, GLOBAL_SHAPE[0], GLOBAL_SHAPE[1], True, 4008), (1,)),
}
for _sp in SPLIT_CASES:
    for _k, _n in enumerate((_sp - 1, _sp, _sp + 1)):
        FIXTURES[f"split {_sp}, {_n} obstacles"] = (lambda sp=_sp, n=_n, k=_k: _split(sp, n, 4200 + 10 * sp + k), (SPLIT_STRIDE,))
KS = (1, 7, 64)


def fixture_planes(cost, flags, K):
    """The planes the GPU test feeds in: K = 1 the argmin, else the K cheapest survivors (-1 past the last one)."""
    return R.rank_tables(cost, flags, K)[0]


# the reference is computed once per (fixture, stride) for the K = 64 planes; K = 1 and 7 are its first planes
_cache = {}


def fixture_reference(oracle, name, stride, planes=None):
    key = (name, stride)
    if key not in _cache or planes is not None:
        batch = FIXTURES[name][0]()
        if planes is None:
            planes = fixture_planes(*oracle_tables(oracle, batch), 64)
        out = (batch, planes, MR.margins(oracle, batch, best_idx=planes, pose_stride=stride))
        if key in _cache:
            return out
        _cache[key] = out
    return _cache[key]


def straight_batch(obs_pose, obs_dims, t_now=0, final=None, T=5.0, v=8.0, obs_poly=None, obs_nvert=None, n_ego=1):
    """n_ego identical egos at s = 20 on the straight line y = 0, driving at a constant 8 m/s with d = 0: point i sits at x = 20 + 0.8 i,
    y = 0, yaw = 0, exactly.  One scene: obs_pose [T_obs, n, 4], obs_dims [n, 2]."""
    xs = np.linspace(0.0, 400.0, 81)
    knots, coef = build_frames(np.stack([xs, np.zeros_like(xs)], axis=1)[None])
    base = synth.make_batch(1, 2, 2, 2, 0, 10, False, 1)
    obs_pose = np.asarray(obs_pose, dtype=np.float64)[None]
    return ProblemBatch(d_samples=[0.0], t_samples=[T], v_samples=np.full((n_ego, 1), v), target_speed=np.full(n_ego, v),
                        ego=np.tile([20.0, v, 0.0, 0.0, 0.0, 0.0], (n_ego, 1)), frame_of=np.zeros(n_ego), scene_of=np.zeros(n_ego),
                        t_now=np.full(n_ego, t_now), nx=[81], knots=knots, coef=coef, obs_pose=obs_pose, obs_dims=np.asarray(obs_dims, dtype=np.float64)[None],
                        final_time_step=[obs_pose.shape[1] - 1 if final is None else final], veh_l=base.veh_l, veh_w=base.veh_w, max_speed=base.max_speed,
                        max_accel=base.max_accel, tick_t=0.1, check_stride=2,
                        obs_poly=None if obs_poly is None else np.asarray(obs_poly, dtype=np.float64)[None],
                        obs_nvert=None if obs_nvert is None else np.asarray(obs_nvert, dtype=np.int32)[None])


def static_rows(T_obs, poses):
    """[T_obs, n, 4] with every obstacle (x, y, yaw) valid in every row."""
    p = np.asarray(poses, dtype=np.float64)
    return np.tile(np.concatenate([p, np.ones((len(p), 1))], axis=1)[None], (T_obs, 1, 1))


def hand_cases():
    """name -> (batch, pose_stride, (min_dist, min_step, min_obs)); shared with the GPU test."""
    veh = synth.make_batch(1, 2, 2, 2, 0, 10, False, 1)
    l, w = veh.veh_l, veh.veh_w
    x = lambda i: 20.0 + 0.8 * i  # noqa: E731
    cases = {}
    # a 6 x 2 box 1.25 m beside the line, centred at point 10: every pose whose footprint overlaps it in x is 1.25 away; the first is
    # the smallest even i with x(i) + l/2 >= x(10) - 3
    first = next(i for i in range(0, 50, 2) if x(i) + 0.5 * l >= x(10) - 3.0)
    cases["beside"] = (straight_batch(static_rows(60, [[x(10), 0.5 * w + 1.0 + 1.25, 0.0]]), [[6.0, 2.0]]), 2, (1.25, first, 0))
    # a 4 x 2 box ahead whose rear edge is 0.1 m behind the ego's front at point 3 (0.7 m ahead of it at point 2)
    ahead = [[x(3) + 0.5 * l - 0.1 + 2.0, 0.0, 0.0]]
    cases["contact at 3"] = (straight_batch(static_rows(60, ahead), [[4.0, 2.0]]), 1, (0.0, 3, 0))
    # a triangle whose apex points at the line from the right, 2 m from the footprint's edge, at x(5): first pose that reaches over it
    tri = np.array([[-1.0, -1.0], [1.0, -1.0], [0.0, 1.0]])
    first_t = next(i for i in range(0, 50) if x(i) + 0.5 * l >= x(5))
    cases["ring"] = (straight_batch(static_rows(60, [[x(5), -(0.5 * w + 2.0 + 1.0), 0.0]]), [[2.0, 2.0]], obs_poly=tri[None], obs_nvert=[3]), 1, (2.0, first_t, 0))
    # t_now = final_time_step: no pose in the horizon
    cases["empty horizon"] = (straight_batch(static_rows(60, ahead), [[4.0, 2.0]], t_now=30, final=30), 1, (np.inf, -1, -1))
    # the obstacle of "contact at 3" valid in row 3 only: stride 1 finds the contact, stride 2 steps over it and finds no pair at all
    odd = static_rows(60, ahead)
    odd[np.arange(60) != 3, :, 3] = 0.0
    cases["odd row, stride 1"] = (straight_batch(odd, [[4.0, 2.0]]), 1, (0.0, 3, 0))
    cases["odd row, stride 2"] = (straight_batch(odd, [[4.0, 2.0]]), 2, (np.inf, -1, -1))
    # two identical columns: the smaller column wins; with a third, nearer one behind them it wins
    twin = static_rows(60, [[x(10), 0.5 * w + 1.0 + 1.25, 0.0]] * 2 + [[x(20), 0.5 * w + 1.0 + 0.5, 0.0]])
    cases["tie"] = (straight_batch(twin[:, :2], [[6.0, 2.0]] * 2), 2, (1.25, first, 0))
    first_n = next(i for i in range(0, 50, 2) if x(i) + 0.5 * l >= x(20) - 3.0)
    cases["nearer later"] = (straight_batch(twin, [[6.0, 2.0]] * 3), 2, (0.5, first_n, 2))
    return cases


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_made_cases(oracle, name):
    batch, stride, (dist, step, obs) = hand_cases()[name]
    got = MR.margins(oracle, batch, best_idx=[0], pose_stride=stride)
    assert (got.min_step[0, 0], got.min_obs[0, 0]) == (step, obs), name
    assert got.min_dist[0, 0] == dist if not np.isfinite(dist) or dist == 0.0 else abs(got.min_dist[0, 0] - dist) < 1e-12, (name, got.min_dist)


def test_tie_rule_is_smallest_step_then_smallest_column():
    d = np.array([[3.0, 2.0, 2.0], [2.0, np.nan, 5.0], [np.nan, np.nan, np.nan]])
    assert MR.lex_min([0, 4, 8], d) == (2.0, 0, 1)
    assert MR.lex_min([0, 4, 8], d[::-1]) == (2.0, 4, 0)
    assert MR.lex_min([0], np.full((1, 3), np.nan)) == (np.inf, -1, -1)


def test_inf_nan_and_minus_one_conventions(oracle):
    batch = _edges()
    C = batch.C
    planes = np.array([[0, -1, 7, 7, 7], [C, 3, -5, 7, 7]])  # (an index beyond the lattice is "no trajectory" for the reference too)
    skip = np.array([0, 0, 0, 0, 1])
    ref = MR.margins(oracle, batch, best_idx=planes, pose_stride=1, skip=skip)
    assert np.isfinite(ref.min_dist[0, 0]) and ref.min_step[0, 0] >= 0 and ref.min_obs[0, 0] >= 0
    for k, b in ((0, 1), (1, 0), (1, 2), (0, 4), (1, 4)):  # index < 0, index >= C, skipped
        assert np.isnan(ref.min_dist[k, b]) and ref.min_step[k, b] == -1 and ref.min_obs[k, b] == -1
    assert ref.min_dist[1, 1] == np.inf and ref.min_step[1, 1] == -1  # scene_of = -1
    assert np.isfinite(ref.min_dist[0, 2]) and ref.min_step[0, 2] == 0  # one pose left
    assert ref.min_dist[0, 3] == np.inf and ref.min_obs[0, 3] == -1  # none
    es = np.full((1, 5, 3), np.nan)
    es[0, 0] = MR.end_state_of(batch, 0, 0)
    by_state = MR.margins(oracle, batch, end_state=es, pose_stride=1)
    assert by_state.min_dist[0, 0] == ref.min_dist[0, 0] and np.isnan(by_state.min_dist[0, 1:]).all()


def test_batched_rectangle_distance_is_convex_distance(oracle):
    """pair_distances goes a column at a time through the oracle's batch call: the same numbers as convex_distance pair by pair."""
    batch = FIXTURES["3 obstacles"][0]()
    prob = oracle.problems_from_batch(batch, egos=[1])[0]
    r = prob.eval_traj(*MR.end_state_of(batch, 1, 62), dump=True, stride=256)
    idx = np.arange(0, min(r.M, 99), 3)
    x, y, yaw = r.arrays[9, :r.M], r.arrays[10, :r.M], r.arrays[11, :r.M]
    dist = MR.pair_distances(oracle, batch, 1, x, y, yaw, idx)
    for q, i in enumerate(idx):
        for j in range(batch.n_obs):
            pose = batch.obs_pose[1, i, j]
            want = CR.convex_distance(oracle, (batch.veh_l, batch.veh_w, x[i], y[i], yaw[i]), (batch.obs_dims[1, j, 0], batch.obs_dims[1, j, 1], *pose[:3]))
            assert dist[q, j] == want


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_gpu_fixtures_are_decidable(oracle, name):
    for stride in FIXTURES[name][1]:
        batch, planes, ref = fixture_reference(oracle, name, stride)
        clean, share = MR.decidable(ref)
        assert clean, (name, stride, float(ref.min_nonzero.min()))
        assert share >= MR.MIN_COUNTED, (name, stride, share)
        has = ref.n_pairs > 0
        assert has.any() or name == "edges"


@pytest.mark.parametrize("split", sorted(SPLIT_CASES))
def test_split_fixtures_reach_their_split(oracle, split):
    """Every plan of a split fixture has the pose count that gives the kernel the intended lanes per pose, and n_obs sits one below, at
    and one above it - from the reference's M and the horizon, not from the kernel."""
    for n in (split - 1, split, split + 1):
        batch, planes, ref = fixture_reference(oracle, f"split {split}, {n} obstacles", SPLIT_STRIDE)
        assert batch.n_obs == n and (batch.t_now == 0).all()
        live = ref.M >= 2
        assert live.sum() >= 64 and np.array_equal(live, planes >= 0)
        n_pose = -(-np.minimum(ref.M[live], int(batch.final_time_step[0])) // SPLIT_STRIDE)
        assert {kernel_split(int(v)) for v in n_pose} == {split}, (split, n, sorted(set(n_pose.tolist())))
        assert (ref.n_pairs[live] == n_pose * n).all()  # every column is valid at every pose: each lane slice is walked
