"""Inputs for the walk's stage S (csrc/frenet_lattice_fused.hip, `// [section S]`): a blocked lon profile ends on one SURE hit - both
ends of its fan of ego centres closer to an obstacle's box than thr = min(half length, half width) - before prep, B and N.
tests/test_gpu_sure_hit.py runs every case through every kernel instance against the oracle; tests/test_sure_hit_cpu.py proves with the
oracle and the numpy test of tools/sure_hit_estimate.py alone that each case is what its name says.

Eight egos per case.  Every case moves the scene it drew 100 m beside the road and decides with obstacles of its own (columns 0..),
which exist only at the steps the case names.  SHAPES: 9 x 9 x 7, whose three- and four-per-CU rectangle instances have the stage;
5 x 5 x 5, whose shaped instances run two per CU only and have none, and a run-time 5 x 4 x 3: the controls.

CASES: name -> (builder(shape) -> ProblemBatch, kind), kind in
  "sure"    every lon profile with a checked pose at the case's step has a sure item there (EXPECT: the step and the list position)
  "silent"  no lon profile has a sure item
  "mixed"   what the case's own check in tests/test_sure_hit_cpu.py says
"""
import os
import sys

import numpy as np

import adversarial as A
import prologue_cases as P
from fiss_plus_planner_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import sure_hit_estimate as E  # noqa: E402

_kind = ["FOP"]  # (fiss_twin builds its case on the FISS+ lattice of the same seed)
SHAPES = {
    "9 x 9 x 7": lambda seed: synth.make_batch(8, 9, 9, 7, 50, 50, True, seed, kind=_kind[0], layout="survey8d"),
    "5 x 5 x 5": lambda seed: synth.make_batch(8, 5, 5, 5, 10, 100, True, seed),
    "5 x 4 x 3 (run-time shape: no stage S)": lambda seed: synth.make_batch(8, 5, 4, 3, 12, 40, True, seed, layout="survey8d"),
}
K_EARLY = 8


def cleared(batch, straight=True):
    """The drawn scene 100 m beside the road (it decides nothing), the egos on the line with no lateral motion unless told otherwise."""
    pose = batch.obs_pose.copy()
    pose[..., 1] += 100.0
    ego = batch.ego.copy()
    if straight:
        ego[:, 3:] = 0.0
    return A._copy(batch, obs_pose=pose, ego=ego)


def k_last(batch):
    """The last checked step every ego of the batch has (stride, table length, t_now)."""
    n = min(batch.T_obs - int(batch.t_now.max()), int(batch.final_time_step.min()) - int(batch.t_now.max()), 101)
    return (n - 1) // batch.check_stride * batch.check_stride


def frame_at(batch, b, s):
    f = int(batch.frame_of[b])
    px, py, yaw = synth.sample_frames(batch.knots[f:f + 1], batch.coef[f:f + 1], np.array([[s]]))
    return np.array([px[0, 0], py[0, 0]]), float(yaw[0, 0])


def put(pose, dims, batch, b, j, k, centre, yaw, size, steps=None):
    """Obstacle j of ego b's scene: a box at `centre` at step t_now + k alone (or at `steps`, relative to t_now), no state elsewhere."""
    sc, t0 = int(batch.scene_of[b]), int(batch.t_now[b])
    pose[sc, :, j, 3] = 0.0
    for kk in ([k] if steps is None else steps):
        if 0 <= t0 + kk < batch.T_obs:
            pose[sc, t0 + kk, j] = (centre[0], centre[1], yaw, 1.0)
    dims[sc, j] = size


def across(batch, k, j=0, width=14.0, margin=10.0, egos=None, steps=None):
    """A box squarely across the line at step k: it covers where every lon profile of the ego stands then, +- margin / 2 along the line."""
    pose, dims = batch.obs_pose.copy(), batch.obs_dims.copy()
    for b in (range(batch.B) if egos is None else egos):
        s_k = P.lon_positions(batch, b)[:, k]
        lo, hi = np.nanmin(s_k), np.nanmax(s_k)
        c, yaw = frame_at(batch, b, 0.5 * (lo + hi))
        put(pose, dims, batch, b, j, k, c, yaw, (hi - lo + margin, width), steps)
    return A._copy(batch, obs_pose=pose, obs_dims=dims)


ALONGSIDE = 3.4  # m to the left of the line: free of every candidate (0.83 + 0.92 + what the heading adds), inside the group circle


def alongside(batch, n, offset=ALONGSIDE, cols_from=1):
    """n obstacles ride beside every ego at every step, `offset` m to the left of the mean of its lon profiles: inside the group
    circle's reach (they survive G, n items per row in time order), too far for any candidate to touch."""
    pose, dims = batch.obs_pose.copy(), batch.obs_dims.copy()
    for b in range(batch.B):
        sc, f = int(batch.scene_of[b]), int(batch.frame_of[b])
        s_mean = np.nanmean(P.lon_positions(batch, b), axis=0)
        s_mean = np.where(np.isnan(s_mean), s_mean[np.isfinite(s_mean)][-1], s_mean)
        ds = np.linspace(-0.5, 0.5, n)
        px, py, yaw = synth.sample_frames(batch.knots[f:f + 1], batch.coef[f:f + 1], (s_mean[:, None] + ds[None, :])[None])
        t0 = int(batch.t_now[b])
        T = batch.T_obs - t0
        cols = slice(cols_from, cols_from + n)
        pose[sc, t0:, cols, 0] = px[0][:T] - offset * np.sin(yaw[0][:T])
        pose[sc, t0:, cols, 1] = py[0][:T] + offset * np.cos(yaw[0][:T])
        pose[sc, t0:, cols, 2], pose[sc, t0:, cols, 3] = yaw[0][:T], 1.0
        dims[sc, cols] = (1.0, 1.0)
    return A._copy(batch, obs_pose=pose, obs_dims=dims)


K_BOUNDARY = 16  # the step of the boundary cases: by then the other lateral samples have left the extreme one by 6 mm and more


def straight_lines(batch):
    """Every ego on a straight line of its own along x (y = 40 b), 400 m like the drawn lines: the egos' s0 stays inside, the tangent is
    (1, 0) and the normal (0, 1) at every point, to the last bit."""
    from fiss_plus_planner_amd.spline import build_frames

    pts = np.empty((batch.B, batch.NX, 2))
    for b in range(batch.B):
        pts[b, :, 0], pts[b, :, 1] = np.linspace(0.0, 400.0, batch.NX), 40.0 * b
    knots, coef = build_frames(pts)
    nx = np.full(batch.B, batch.NX, dtype=batch.nx.dtype)
    return A._copy(batch, knots=knots, coef=coef, nx=nx, frame_of=np.arange(batch.B, dtype=batch.frame_of.dtype))


def boundary(batch, delta):
    """A REAL candidate stands at the fan's outside end.  Every ego drives a straight line of its own and starts, with no lateral
    motion, on the extreme lateral sample (even egos the largest, odd egos the smallest): that sample's d is constant, its heading
    is the tangent exactly, and dm[k] is its |d| - the candidate's centre IS the end E+ (E- for the odd egos) of P_k +- dm n_k at
    every step.  One long box beside the line at step K_BOUNDARY, parallel to it, covers the other end and every profile's pose;
    its near face is thr + delta from the extreme candidate's centre.
      delta > 0   that end is outside thr by delta: S must not fire, N decides - the extreme candidate passes the box by delta - 1e-6
                  (its side is rho from its centre), every other lateral sample has moved towards the box by more than delta and collides
      delta < 0   both ends inside: S fires, and the extreme candidate overlaps the box by 1e-6 - delta."""
    batch = straight_lines(batch)
    d_top, d_bot = float(np.max(batch.d_samples)), float(np.min(batch.d_samples))
    ego = batch.ego.copy()
    ego[0::2, 3], ego[1::2, 3] = d_top, d_bot
    ego[:, 4:] = 0.0
    batch = A._copy(batch, ego=ego)
    pose, dims = batch.obs_pose.copy(), batch.obs_dims.copy()
    thr, hw_o = E.threshold(batch), 1.5
    for b in range(batch.B):
        s_k = P.lon_positions(batch, b)[:, K_BOUNDARY]
        lo, hi = np.nanmin(s_k), np.nanmax(s_k)
        side = 1.0 if b % 2 == 0 else -1.0  # the extreme candidate's side; the box lies towards the line from it
        y_face = 40.0 * b + batch.ego[b, 3] - side * (thr + delta)
        put(pose, dims, batch, b, 0, K_BOUNDARY, (0.5 * (lo + hi), y_face - side * hw_o), 0.0, (hi - lo + 12.0, 2.0 * hw_o))
    return A._copy(batch, obs_pose=pose, obs_dims=dims)


def wide_vehicle(batch):
    """veh_l < veh_w: rho is the half LENGTH.  A box ahead of every profile's pose at K_EARLY, its near face 0.53 m in front of the
    fastest profile's fan: within the half width (1.5), 3 cm beyond the half length (0.5) - no candidate touches it."""
    batch = A._copy(batch, veh_l=1.0, veh_w=3.0)
    pose, dims = batch.obs_pose.copy(), batch.obs_dims.copy()
    for b in range(batch.B):
        s_k = P.lon_positions(batch, b)[:, K_EARLY]
        c, yaw = frame_at(batch, b, np.nanmax(s_k) + 0.53 + 1.0)  # the fastest profile's centre + the gap + the box's half length
        put(pose, dims, batch, b, 0, K_EARLY, c, yaw, (2.0, 8.0))
    return A._copy(batch, obs_pose=pose, obs_dims=dims)


def near_miss(batch, gap=0.02):
    """A box beside every ego at step 0, its near face `gap` beyond the half width from the line: at row 0 the fan is a point (the
    egos start on the line), both ends are gap outside thr, S is silent and every candidate passes the box by that gap - a threshold
    that is too large by more than the gap blocks them all."""
    pose, dims = batch.obs_pose.copy(), batch.obs_dims.copy()
    for b in range(batch.B):
        c, yaw = frame_at(batch, b, batch.ego[b, 0])
        n = np.array([-np.sin(yaw), np.cos(yaw)])
        put(pose, dims, batch, b, 0, 0, c + (0.5 * min(batch.veh_l, batch.veh_w) + gap + 0.5) * n, yaw, (8.0, 1.0))
    return A._copy(batch, obs_pose=pose, obs_dims=dims)


def far_off_the_line(batch):
    """The egos start 3 m left of the line: dm = 3 m at the first rows, the fan +-dm is 6 m wide, the candidates themselves all start in
    one place - inside a box that stands there at the first four steps.  S is silent (E- is 6 m away), N blocks every profile."""
    ego = batch.ego.copy()
    ego[:, 3], ego[:, 4], ego[:, 5] = 3.0, 0.0, 0.0
    batch = A._copy(batch, ego=ego)
    pose, dims = batch.obs_pose.copy(), batch.obs_dims.copy()
    for b in range(batch.B):
        c, yaw = frame_at(batch, b, batch.ego[b, 0])
        n = np.array([-np.sin(yaw), np.cos(yaw)])
        put(pose, dims, batch, b, 0, 0, c + 3.0 * n, yaw, (3.0, 1.0), steps=range(0, 4))
    return A._copy(batch, obs_pose=pose, obs_dims=dims)


def line_ends_early(batch):
    """The egos stand 5.5 points before the end of their line (M = 6 or so); a box across the line's end from step 12 on - where poses
    k >= M would be.  Nothing is ended by it, nothing collides."""
    ego = batch.ego.copy()
    pose, dims = batch.obs_pose.copy(), batch.obs_dims.copy()
    for b in range(batch.B):
        f = int(batch.frame_of[b])
        end = float(batch.knots[f, int(batch.nx[f]) - 1])
        ego[b, 2] = 0.0
        ego[b, 0] = end - 5.5 * ego[b, 1] * batch.tick_t
        c, yaw = frame_at(batch, b, end - 0.5)
        put(pose, dims, batch, b, 0, 0, c, yaw, (30.0, 14.0), steps=range(12, batch.T_obs))
    return A._copy(batch, ego=ego, obs_pose=pose, obs_dims=dims)


def tight_bend(batch):
    """Every ego on its own line through an arc of 12 m radius (n_k turns by ~5 degrees between rows at 10 m/s), the box across it."""
    from fiss_plus_planner_amd.spline import build_frames

    th = np.linspace(0.0, 400.0 / 12.0, batch.NX)  # arclength 400 m like the drawn lines: the egos' s0 stays inside
    pts = np.empty((batch.B, batch.NX, 2))
    for b in range(batch.B):
        pts[b, :, 0], pts[b, :, 1] = 12.0 * np.sin(th) + 40.0 * b, 12.0 * (1.0 - np.cos(th))
    knots, coef = build_frames(pts)
    nx = np.full(batch.B, batch.NX, dtype=batch.nx.dtype)
    return across(A._copy(batch, knots=knots, coef=coef, nx=nx, frame_of=np.arange(batch.B, dtype=batch.frame_of.dtype)), K_EARLY, width=30.0, margin=30.0)


def _base(shape, seed, straight=True):
    return cleared(SHAPES[shape](seed), straight)


def _variant(shape, what):
    base = _base(shape, 9720)
    if what == "t_now odd":
        base = A._copy(base, t_now=np.minimum(np.array([1, 3, 7, 15, 21, 31, 35, 37]), base.T_obs - 7).astype(base.t_now.dtype))  # (odd; at least 3 rows left)
        return across(base, 2)
    if what == "nan d_sample":
        d = base.d_samples.copy()
        d[len(d) // 2] = np.nan
        return across(A._copy(base, d_samples=d), K_EARLY)
    if what == "pose without a state":
        out = across(base, K_EARLY)
        pose = out.obs_pose.copy()
        for b in range(0, out.B, 2):
            pose[int(out.scene_of[b]), :, 0, 3] = 0.0
        for b in range(1, out.B, 4):
            pose[int(out.scene_of[b]), :, 0, 0] = np.nan
        return A._copy(out, obs_pose=pose)
    if what == "size 0":
        out = across(base, K_EARLY)
        dims = out.obs_dims.copy()
        dims[out.scene_of, 0] = (0.0, 0.0)
        return A._copy(out, obs_dims=dims)
    assert what == "no scene"
    out = across(base, K_EARLY)
    scene_of = out.scene_of.copy()
    scene_of[[1, 5]] = -1
    return A._copy(out, scene_of=scene_of)


CASES = {
    "box across the line at an early row": (lambda s: across(_base(s, 9700), K_EARLY), "sure"),
    "box across the line at row 0": (lambda s: across(_base(s, 9701), 0), "sure"),
    "box across the line at the last checked row": (lambda s: across(_base(s, 9702), k_last(_base(s, 9702)), margin=16.0, width=30.0), "sure"),
    "boundary: one end outside thr by 1e-5": (lambda s: boundary(_base(s, 9703), 1e-5), "mixed"),
    "boundary: one end outside thr by 1e-3": (lambda s: boundary(_base(s, 9703), 1e-3), "mixed"),
    "boundary: both ends inside thr by 1e-5": (lambda s: boundary(_base(s, 9703), -1e-5), "mixed"),
    "veh_l < veh_w, a box within the half width ahead": (lambda s: wide_vehicle(_base(s, 9704)), "silent"),
    "egos far off the line": (lambda s: far_off_the_line(_base(s, 9705)), "silent"),
    "a near miss at row 0, 2 cm beyond thr": (lambda s: near_miss(_base(s, 9710)), "silent"),
    "the sure item behind 64 survivors": (lambda s: across(alongside(_base(s, 9706), 4), k_last(_base(s, 9706)), margin=16.0, width=30.0), "sure"),
    "the sure item in a later chunk of the list": (lambda s: across(alongside(_base(s, 9707), _base(s, 9707).n_obs - 1), k_last(_base(s, 9707)), margin=16.0, width=30.0), "sure"),  # (every other column rides alongside)
    "the line ends inside the checked rows": (lambda s: line_ends_early(_base(s, 9708)), "silent"),
    "t_now odd, the table ends inside the horizon": (lambda s: _variant(s, "t_now odd"), "sure"),
    "a NaN in d_samples": (lambda s: _variant(s, "nan d_sample"), "silent"),
    "poses without a state": (lambda s: _variant(s, "pose without a state"), "mixed"),
    "an obstacle of size 0": (lambda s: _variant(s, "size 0"), "mixed"),
    "egos without a scene": (lambda s: _variant(s, "no scene"), "mixed"),
    "a tight bend": (lambda s: tight_bend(_base(s, 9709)), "sure"),
}
# the step and the least list position (items before it in time order) of the sure item, where the case states them
EXPECT = {
    "box across the line at an early row": (K_EARLY, 0),
    "box across the line at row 0": (0, 0),
    "box across the line at the last checked row": ("last", 0),
    "the sure item behind 64 survivors": ("last", 64),
    "the sure item in a later chunk of the list": ("last", 256),
    "t_now odd, the table ends inside the horizon": (2, 0),
    "a tight bend": (K_EARLY, 0),
}


def build(name, shape):
    fn, kind = CASES[name]
    return fn(shape), kind


FISS_TWINS = {"box across the line at an early row": 9700, "poses without a state": 9720}  # name -> the case's seed


def fiss_twin(name):
    """The 9 x 9 x 7 case built on the FISS+ lattice of its seed, with that lattice's sampling box (which adversarial._copy drops)."""
    _kind[0] = "FISS+"
    try:
        batch, _ = build(name, "9 x 9 x 7")
        box = SHAPES["9 x 9 x 7"](FISS_TWINS[name])
    finally:
        _kind[0] = "FOP"
    assert np.array_equal(box.v_samples, batch.v_samples) and np.array_equal(box.d_samples, batch.d_samples)
    return A._copy(batch, samp_min=box.samp_min, samp_max=box.samp_max, samp_res=box.samp_res)
