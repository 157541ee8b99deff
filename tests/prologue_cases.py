"""Inputs for the fused lattice kernel's prologue and group test (csrc/frenet_lattice_fused.hip: sections STAGE .. G), one per place where
the code that deals that work to lanes and wavefronts can go wrong.  tests/test_gpu_prologue_paths.py runs them through every kernel
instance against the oracle; tests/test_prologue_paths_cpu.py checks with the oracle alone that each one decides something.

CASES: name -> builder of a ProblemBatch.  The (9, 9, 7, stride 2, 50 obstacles, 25 rows) batches take the shaped instances."""
import numpy as np

import adversarial as A
from fiss_plus_planner_amd import synth


def base997(seed, B=12, **kw):
    return synth.make_batch(B, 9, 9, 7, 50, 50, True, seed, layout="survey8d", **kw)


def park(batch, egos, ahead=1.0, j=0, size=None):
    """Obstacle j of the egos' scenes stands on their reference line, `ahead` metres in front of them, at every step."""
    pose, dims = batch.obs_pose.copy(), batch.obs_dims.copy()
    for b in egos:
        f, sc = int(batch.frame_of[b]), int(batch.scene_of[b])
        px, py, yaw = synth.sample_frames(batch.knots[f:f + 1], batch.coef[f:f + 1], np.array([[batch.ego[b, 0] + ahead]]))
        pose[sc, :, j, 0], pose[sc, :, j, 1], pose[sc, :, j, 2], pose[sc, :, j, 3] = px[0, 0], py[0, 0], yaw[0, 0], 1.0
        if size is not None:
            dims[sc, j] = size
    return A._copy(batch, obs_pose=pose, obs_dims=dims)


def lon_positions(batch, b):
    """s(t_k) of every lon profile (slice, end speed) of ego b at every step k of the obstacle table: [nt * nv, T_obs], NaN behind the
    profile's horizon.  The quartic with s'(T) = v, s''(T) = 0 (planners/frenet_optimal_planner.py:69-104)."""
    s0, v0, a0 = batch.ego[b, :3]
    t = np.arange(batch.T_obs) * batch.tick_t
    out = []
    for T in batch.t_samples:
        for v1 in batch.v_samples[b]:
            A_, B_ = v1 - v0 - a0 * T, -a0
            a4 = (B_ - 2.0 * A_ / T) / (4.0 * T * T)
            a3 = (A_ - 4.0 * T ** 3 * a4) / (3.0 * T * T)
            s = s0 + v0 * t + 0.5 * a0 * t ** 2 + a3 * t ** 3 + a4 * t ** 4
            out.append(np.where(t < T, s, np.nan))
    return np.array(out)


CONVOY_DS, CONVOY_D = 1.5, 2.2  # the convoy's spread along the line (+-) and its lateral offset (m)


def convoy(batch):
    """Every obstacle rides beside its ego at every step: on the line at the mean arclength of the ego's lon profiles (inside their range,
    so within the group circle's half range of its centre), up to CONVOY_DS before or behind it and CONVOY_D to the left.  That offset is
    shorter than the ego's half diagonal + the largest lateral sample, which the circle's radius adds: EVERY (row, obstacle) item
    survives the group test - more than any instance's list holds (256 / 320 / 512) - and the chunked redo runs."""
    pose, dims = batch.obs_pose.copy(), batch.obs_dims.copy()
    n = batch.n_obs
    ds = np.linspace(-CONVOY_DS, CONVOY_DS, n)
    for b in range(batch.B):
        f, sc = int(batch.frame_of[b]), int(batch.scene_of[b])
        s_mean = np.nanmean(lon_positions(batch, b), axis=0)  # [T_obs]
        px, py, yaw = synth.sample_frames(batch.knots[f:f + 1], batch.coef[f:f + 1], (s_mean[:, None] + ds[None, :])[None])
        pose[sc, :, :, 0] = px[0] - CONVOY_D * np.sin(yaw[0])
        pose[sc, :, :, 1] = py[0] + CONVOY_D * np.cos(yaw[0])
        pose[sc, :, :, 2], pose[sc, :, :, 3] = yaw[0], 1.0
        dims[sc] = (5.0, 1.6)
    return A._copy(batch, obs_pose=pose, obs_dims=dims)


def _t_now_and_short_tables():
    """t_now odd at stride 2, and so late that the table ends inside the horizon (T_obs - t_now cuts the staged rows: 10, 6, 3, 1 of 25)."""
    base = park(base997(9102), range(0, 12, 2), ahead=6.0)
    return A._copy(base, t_now=np.array([1, 3, 7, 15, 21, 31, 39, 45, 49, 5, 11, 33]))


def _invalid_poses():
    base = park(base997(9103), range(0, 12, 3), ahead=8.0, j=1)
    rng = np.random.default_rng(9103)
    pose = base.obs_pose.copy()
    gone = rng.uniform(size=pose.shape[:3])
    pose[..., 3] = np.where(gone < 0.3, 0.0, 1.0)
    pose[..., 0] = np.where((gone >= 0.3) & (gone < 0.4), np.nan, pose[..., 0])
    return A._copy(base, obs_pose=pose)


def _ego_without_scene():
    base = park(base997(9104), range(0, 12, 2), ahead=6.0)
    scene_of = base.scene_of.copy()
    scene_of[[3, 7]] = -1
    return A._copy(base, scene_of=scene_of)


def _blocked_in_the_first_round():
    """Every other ego stands inside an obstacle from step 0 on: each of its profiles is blocked by the list's first items."""
    return park(base997(9105), range(0, 12, 2), ahead=1.0, size=(6.0, 12.0))


def _lattice(nd, nv, nt, seed):
    return park(synth.make_batch(8, nd, nv, nt, 12, 40, True, seed, layout="survey8d"), range(0, 8, 2), ahead=7.0)


def _d_samples(order):
    base = park(base997(9107, B=8), range(0, 8, 2), ahead=7.0)
    d = base.d_samples.copy()
    if order == "descending":
        d = d[::-1].copy()
    else:
        d[4] = np.nan
    return A._copy(base, d_samples=d)


def _degenerate_line():
    """Ego 0's reference line has all its knots in one place: bucket width 0."""
    base = park(base997(9108, B=8), range(2, 8, 2), ahead=7.0)
    knots = base.knots.copy()
    knots[int(base.frame_of[0]), :] = base.ego[0, 0]
    return A._copy(base, knots=knots)


def _square_vehicle():
    base = park(base997(9110, B=8), range(0, 8, 2), ahead=7.0)
    return A._copy(base, veh_l=base.veh_w)


CASES = {
    "the compiled-in 25 x 50 table": lambda: park(base997(9100), range(0, 12, 2), ahead=6.0),
    "13 rows x 7 obstacles": lambda: park(synth.make_batch(8, 5, 4, 3, 7, 26, True, 9101, layout="survey8d"), range(0, 8, 2), ahead=5.0),
    "one obstacle": lambda: park(synth.make_batch(8, 5, 4, 3, 1, 40, True, 9111, layout="survey8d"), range(0, 8, 2), ahead=5.0),
    "t_now odd, tables shorter than the horizon": _t_now_and_short_tables,
    "poses without a state": _invalid_poses,
    "an ego without a scene": _ego_without_scene,
    "blocked in the first round": _blocked_in_the_first_round,
    "more survivors than the list holds": lambda: convoy(base997(9106, B=8)),
    "9 x 5 x 7 (98 sum lanes)": lambda: _lattice(9, 5, 7, 9120),
    "3 x 9 x 2 (24 sum lanes)": lambda: _lattice(3, 9, 2, 9121),
    "9 x 11 x 7 (140 sum lanes)": lambda: _lattice(9, 11, 7, 9122),
    "d_samples descending": lambda: _d_samples("descending"),
    "d_samples with a NaN": lambda: _d_samples("nan"),
    "a line with all knots in one place": _degenerate_line,
    "220 knots (coefficient window)": lambda: park(base997(9109, n_knots=220), range(0, 12, 2), ahead=6.0),
    "veh_l == veh_w": _square_vehicle,
}
SHAPED = {"the compiled-in 25 x 50 table", "t_now odd, tables shorter than the horizon", "poses without a state", "an ego without a scene",
          "blocked in the first round", "more survivors than the list holds", "d_samples descending", "d_samples with a NaN",
          "a line with all knots in one place", "220 knots (coefficient window)", "veh_l == veh_w"}
