"""Inputs for two places of the fused lattice kernel (csrc/frenet_lattice_fused.hip): the row ranges of the group test (section RANGES:
the shaped instances evaluate the lon profiles of the smallest and the largest end speed alone) and the argmin (section ARGMIN: one
wavefront reduces the workgroup).  tests/test_gpu_range_argmin.py runs them through every kernel instance against the oracle;
tests/test_range_argmin_cpu.py checks with the oracle alone that each one is what its name says.

RANGE_CASES, ARGMIN_CASES: name -> builder of a ProblemBatch.  SHAPED_997 / SHAPED_555: the names whose batch has one of the two
compiled-in shapes."""
import math

import numpy as np

import adversarial as A
import prologue_cases as P
from fiss_plus_planner_amd import synth
from prologue_cases import base997

K_LATE = 48  # the last checked step of the 9 x 9 x 7 shape (25 rows, stride 2)


def base555(seed, B=12):
    return synth.make_batch(B, 5, 5, 5, 10, 100, True, seed)


def parked(batch):
    """Every other ego gets an obstacle on its line (a colliding candidate for sure), the others keep the scene they drew."""
    return P.park(batch, range(0, batch.B, 2), ahead=7.0)


# ---------------------------------------------------------------- row ranges
def middle_extremes(n):
    """A permutation of range(n) (ascending samples, n >= 4) that puts the largest and the smallest sample next to each other in the
    middle and two neighbours of the median on the first and the last index."""
    mids = list(range(1, n - 1))
    first, last = mids[len(mids) // 2], mids[len(mids) // 2 - 1]
    rest = [i for i in mids if i not in (first, last)]
    order = [first] + rest[:len(rest) // 2] + [n - 1, 0] + rest[len(rest) // 2:] + [last]
    assert sorted(order) == list(range(n)) and order[0] not in (0, n - 1) and order[-1] not in (0, n - 1)
    return order


def with_v(batch, how):
    v = np.sort(batch.v_samples, axis=1)
    n = v.shape[1]
    if how == "descending":
        v = v[:, ::-1].copy()
    elif how == "permuted":
        v = v[:, middle_extremes(n)]
    elif how == "equal extremes":  # the smallest and the largest sample twice each, at distant indices
        v[:, n // 2] = v[:, 0]
        v[:, 1] = v[:, n - 1]
    elif how == "negative smallest":
        v[:, 0] = -2.5
        v = v[:, middle_extremes(n)]
    elif how == "nan middle":
        v[:, n // 2] = np.nan
    elif how == "nan end":
        v[:, n - 1] = np.nan
    elif how == "inf largest":
        v[:, n - 1] = np.inf
        v = v[:, middle_extremes(n)]
    else:
        assert how == "ascending"
    return A._copy(batch, v_samples=np.ascontiguousarray(v))


def extreme_only_obstacles(batch, k=K_LATE, egos=None):
    """Two obstacles per chosen ego that exist at step k alone (no state at any other step): a 1 m square 2 m in front of where the
    FASTEST lon profile of any slice stands at step k, on the reference line, and one 2 m behind where the SLOWEST stands.  Those egos
    drive straight along the line (no lateral start state), so that the group circle adds as little as it can."""
    egos = list(range(0, batch.B, 2)) if egos is None else egos
    ego, pose, dims = batch.ego.copy(), batch.obs_pose.copy(), batch.obs_dims.copy()
    ego[egos, 3:] = 0.0
    tmp = A._copy(batch, ego=ego)
    for b in egos:
        f, sc = int(batch.frame_of[b]), int(batch.scene_of[b])
        s_k = P.lon_positions(tmp, b)[:, k]
        for j, s in ((0, np.nanmax(s_k) + 2.0), (1, np.nanmin(s_k) - 2.0)):
            px, py, yaw = synth.sample_frames(batch.knots[f:f + 1], batch.coef[f:f + 1], np.array([[s]]))
            pose[sc, :, j, 3] = 0.0
            pose[sc, k, j] = (px[0, 0], py[0, 0], yaw[0, 0], 1.0)
            dims[sc, j] = (1.0, 1.0)
    return A._copy(batch, ego=ego, obs_pose=pose, obs_dims=dims)


PERMUTED_SPREAD = np.array([6.0, 5.0, 13.4, 6.5, 0.0, 5.5, 7.0, 6.2, 5.8])  # extremes on indices 4 and 2, 6.0 and 5.8 at the ends


def _permuted_extreme_only():
    base = base997(9301)
    ego = base.ego.copy()
    ego[:, 0], ego[:, 1], ego[:, 2] = 30.0 + np.arange(base.B), 6.0, 0.0  # (start at the samples' median: the spread is the samples')
    pose = base.obs_pose.copy()
    pose[..., 1] += 100.0  # (the scene it drew stands beside the road: the two obstacles below decide alone)
    base = A._copy(base, ego=ego, obs_pose=pose, v_samples=np.tile(PERMUTED_SPREAD, (base.B, 1)))
    return extreme_only_obstacles(base)


def _lattice(nd, nv, nt, seed, how="permuted"):
    return with_v(parked(synth.make_batch(8, nd, nv, nt, 12, 40, True, seed, layout="survey8d")), how if nv > 2 else "ascending")


def _late_and_windowed(which):
    if which == "t_now odd":
        base = with_v(parked(base997(9310)), "permuted")
        return A._copy(base, t_now=np.array([1, 3, 7, 15, 21, 31, 39, 45, 49, 5, 11, 33]))
    return with_v(parked(base997(9311, n_knots=220)), "permuted")


RANGE_CASES = {}
for _how in ("ascending", "descending", "permuted", "equal extremes", "negative smallest", "nan middle", "nan end", "inf largest"):
    RANGE_CASES[f"9 x 9 x 7, v_samples {_how}"] = (lambda h: lambda: with_v(parked(base997(9300)), h))(_how)
    RANGE_CASES[f"5 x 5 x 5, v_samples {_how}"] = (lambda h: lambda: with_v(parked(base555(9350)), h))(_how)
RANGE_CASES.update({
    "nv = 1": lambda: _lattice(5, 1, 3, 9320),
    "nv != nd (4 x 7 x 3)": lambda: _lattice(4, 7, 3, 9321),
    "permuted, obstacles only the fastest and only the slowest profile reach": _permuted_extreme_only,
    "permuted, t_now odd": lambda: _late_and_windowed("t_now odd"),
    "permuted, 220 knots (coefficient window)": lambda: _late_and_windowed("window"),
})
SHAPED_997 = {n for n in RANGE_CASES if n.startswith("9 x 9 x 7") or n.startswith("permuted")}
SHAPED_555 = {n for n in RANGE_CASES if n.startswith("5 x 5 x 5")}


# ---------------------------------------------------------------- argmin
def straight(batch, egos=None):
    """No lateral start state: the lateral cost sums are even in the end offset (mirrored samples tie bit for bit)."""
    ego = batch.ego.copy()
    ego[:, 3:] = 0.0
    return A._copy(batch, ego=ego)


def _winner_shares(zero_at):
    """The cheapest end offset is the one nearest the line, pulled towards the ego's lateral start offset: the d_samples are shifted so
    that sample `zero_at` is 0, the egos start on offsets spread over the samples, and the target speed walks over the v_samples.  A
    lateral sample is 63 indices - about a wavefront's share of 64 - so the batches of WINNER_ZEROS together put winners into every
    wavefront's share and, with the last sample, at indices >= 512: the assembly loop's second trip."""
    base = synth.make_batch(12, 9, 9, 7, 0, 50, True, 9400 + zero_at)
    d = base.d_samples - base.d_samples[zero_at]
    ego, ts = base.ego.copy(), base.target_speed.copy()
    ego[:, 3], ego[:, 4], ego[:, 5] = np.linspace(d[0], d[-1], base.B), 0.0, 0.0
    for b in range(base.B):
        ts[b] = base.v_samples[b, b % base.nv]
    return A._copy(base, ego=ego, target_speed=ts, d_samples=d)


def _one_feasible(where):
    """One candidate passes the limits: every end speed but one is far above max_speed, every lateral sample but one is NaN (a NaN cost
    never wins), and the braking from 13 m/s to the one end speed, 0, stays below max_accel on the longest horizon alone (peak
    1.5 x 13 / T: 1.95 at T = 10, 2.02 at the next sample).  t_samples descend for index 0, so that the longest horizon is slice 0.
    The scene stands 100 m beside the road (the one candidate is free); the profiles that leave the line at once collide as the
    reference has it (a trajectory of one point has no heading), and so do the NaN offsets."""
    base = base997(9410)
    pose = base.obs_pose.copy()
    pose[..., 1] += 100.0
    base = A._copy(base, obs_pose=pose)
    ego = base.ego.copy()
    ego[:, 1], ego[:, 2] = 13.0, 0.0
    v = np.full_like(base.v_samples, 1e3)
    d = np.full_like(base.d_samples, np.nan)
    t = np.sort(base.t_samples)
    if where == "first":
        v[:, 0], d[0], t = 0.0, base.d_samples[0], t[::-1].copy()
    else:
        v[:, -1], d[-1] = 0.0, base.d_samples[-1]
    return A._copy(base, ego=ego, v_samples=v, d_samples=d, t_samples=t, max_accel=1.98)


def _mirror_tie(shape):
    """Symmetric d_samples without a zero (the middle one is NaN and never wins), an ego on the line with no lateral motion, no
    obstacle: the two innermost samples tie bit for bit and FOP's `>=` keeps the higher index."""
    nd = 9 if shape == "997" else 5
    base = straight(synth.make_batch(12, nd, nd, 7 if shape == "997" else 5, 0, 50, True, 9420))
    half = np.linspace(0.2, 0.8, nd // 2)
    # (9 x 9 x 7: the NaN in the middle, the innermost pair 126 indices apart; 5 x 5 x 5: one pair on the first two samples, indices
    # below 50, and NaN behind them)
    d = np.concatenate([-half[::-1], [np.nan], half]) if shape == "997" else np.array([-0.2, 0.2, np.nan, np.nan, np.nan])
    return A._copy(base, d_samples=d)


def _without_obstacles():
    return synth.make_batch(12, 9, 9, 7, 0, 50, True, 9430)


ARGMIN_CASES = {
    **{f"winners in the share of lateral sample {z}": (lambda zz: lambda: _winner_shares(zz))(z) for z in (0, 1, 2, 4, 6, 7, 8)},
    "the only feasible candidate is index 0": lambda: _one_feasible("first"),
    "the only feasible candidate is index C - 1": lambda: _one_feasible("last"),
    "no feasible candidate": lambda: A._copy(parked(base997(9411)), max_accel=1e-3),
    "C < 64 (3 x 3 x 3)": lambda: parked(synth.make_batch(8, 3, 3, 3, 12, 40, True, 9412, layout="survey8d")),
    "mirror tie inside one wavefront's share (5 x 5 x 5)": lambda: _mirror_tie("555"),
    "mirror tie across two wavefronts' shares (9 x 9 x 7)": lambda: _mirror_tie("997"),
    "no obstacles (the smallest layout)": _without_obstacles,
}
# (latency mode, one workgroup per ego and the tail split are the MODES every case runs through; the grouped 1024-thread launch is
# tests/test_gpu_range_argmin.py's own mode)
WINNER_SHARES = [n for n in ARGMIN_CASES if n.startswith("winners in")]
NO_OBSTACLES = {*WINNER_SHARES, "mirror tie inside one wavefront's share (5 x 5 x 5)",
                "mirror tie across two wavefronts' shares (9 x 9 x 7)", "no obstacles (the smallest layout)"}


def share_of(c, threads=512):
    """The wavefront whose lanes assemble candidate c (thread c % threads) and the trip of the assembly loop it does so in."""
    return (c % threads) // 64, c // threads


def group_reach(batch, b, obstacle_dims):
    """What the group circle of ego b adds to half its arclength range, generously: ego half diagonal + the bound of |d| + the obstacle's
    half diagonal (csrc/frenet_lattice_fused.hip, DALL and CIRCLES)."""
    T = float(np.max(batch.t_samples))
    d_all = max(abs(batch.ego[b, 3]), float(np.nanmax(np.abs(batch.d_samples)))) + 0.1976 * abs(batch.ego[b, 4]) * T + 0.01729 * abs(batch.ego[b, 5]) * T * T
    return 0.5 * math.hypot(batch.veh_l, batch.veh_w) + d_all + 0.5 * math.hypot(*obstacle_dims)
