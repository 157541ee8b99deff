"""Inputs for the fused lattice kernel's kernel-wide scalars (csrc/frenet_lattice_fused.hip: slot / part / nsplit at the entry, t_now, the
rows staged / checked / compiled in, horizon_cap, pose_limit, hp, item_base, the coefficient window, it_lo / it_hi, the ego's index
after the walk).  The kernel derives some of them in another way per instance (the three- and four-per-CU instances read nsplit as 1
or 2), so the failure mode is one scalar read as another or as its default: in every case the scalars it is about take values that
differ from their defaults and from each other.  tests/test_gpu_scalar_paths.py runs the cases through every launch path against the
oracle; tests/test_scalar_paths_cpu.py proves with the oracle alone that each case is what its name says.

CASES: name -> builder of a ProblemBatch of at most 8 egos.  SHAPED_997 / SHAPED_555: the names whose batch has a compiled-in shape.
FISS_CASES: the same modifiers on FISS+ lattices (the twin instances with the appended search)."""
import numpy as np

import adversarial as A
import prologue_cases as P
from fiss_plus_planner_amd import synth

B = 8
T_NOW_SHORT = 25   # 50-step table, stride 2: ceil((50 - 25) / 2) = 13 rows staged of the 25 compiled in
HORIZON_CAP = 21   # final_time_step - t_now: ceil(21 / 2) = 11 rows checked, pose_limit 21, hp 22
T_NOW_CAP = 3
CONVOY_ROWS_MIN = 6  # (a 256-entry list holds five whole rows of 50)


def _keep(batch, **kw):
    """adversarial._copy that keeps a FISS batch's sampling box."""
    if batch.samp_min is not None:
        kw = dict(dict(samp_min=batch.samp_min, samp_max=batch.samp_max, samp_res=batch.samp_res), **kw)
    return A._copy(batch, **kw)


def base997(seed, kind="FOP", **kw):
    return synth.make_batch(B, 9, 9, 7, 50, 50, True, seed, kind=kind, layout="survey8d", **kw)


def base555(seed, kind="FOP"):
    return synth.make_batch(B, 5, 5, 5, 10, 100, True, seed, kind=kind)


def base_runtime(seed, kind="FOP"):
    return synth.make_batch(B, 5, 4, 3, 7, 50, True, seed, kind=kind, layout="survey8d")  # nv != nd, 7 obstacles: no compiled-in shape


def park(batch, ahead=6.0, egos=None):
    """Every other ego gets an obstacle on its line `ahead` metres in front of it at every step: colliding candidates for sure; P.park
    rebuilt so that a FISS batch keeps its sampling box."""
    egos = range(0, batch.B, 2) if egos is None else egos
    q = P.park(batch, egos, ahead=ahead)
    return _keep(batch, obs_pose=q.obs_pose, obs_dims=q.obs_dims)


def t_now_odd(batch):
    return _keep(batch, t_now=np.array([1, 3, 5, 7, 9, 11, 13, 15], dtype=batch.t_now.dtype)[:batch.B])


def short_table(batch):
    """t_now so late that the pose table ends inside the horizon; final_time_step far behind it, so that only the table cuts the rows."""
    return _keep(batch, t_now=np.full(batch.B, T_NOW_SHORT, dtype=batch.t_now.dtype),
                 final_time_step=np.full(len(batch.final_time_step), 10000, dtype=batch.final_time_step.dtype))


def early_final_step(batch):
    """final_time_step - t_now = HORIZON_CAP: fewer rows than the table still holds from t_now on, and fewer than are compiled in."""
    return _keep(batch, t_now=np.full(batch.B, T_NOW_CAP, dtype=batch.t_now.dtype),
                 final_time_step=np.full(len(batch.final_time_step), T_NOW_CAP + HORIZON_CAP, dtype=batch.final_time_step.dtype))


def line_ends_early(batch):
    """Every other ego stands a few points before the end of its reference line, egos 0 and 4 with an obstacle on the line's end: M <= k_last + 1."""
    ego, pose, dims = batch.ego.copy(), batch.obs_pose.copy(), batch.obs_dims.copy()
    points = [3, 6, 21, 44]
    for b in range(0, batch.B, 2):
        f, sc = int(batch.frame_of[b]), int(batch.scene_of[b])
        k_last = float(batch.knots[f, int(batch.nx[f]) - 1])
        ego[b, 2] = 0.0
        ego[b, 0] = k_last - (points[(b // 2) % len(points)] - 0.5) * ego[b, 1] * batch.tick_t
        if b % 4:  # (egos 2 and 6 end early before the scene they drew)
            continue
        px, py, yaw = synth.sample_frames(batch.knots[f:f + 1], batch.coef[f:f + 1], np.array([[k_last - 0.5]]))
        pose[sc, :, 0, 0], pose[sc, :, 0, 1], pose[sc, :, 0, 2], pose[sc, :, 0, 3] = px[0, 0], py[0, 0], yaw[0, 0], 1.0
        dims[sc, 0] = (3.0, 2.0)  # (narrower than the fan of lateral samples)
    return _keep(batch, ego=ego, obs_pose=pose, obs_dims=dims)


def crowded(batch):
    q = P.convoy(batch)
    return _keep(batch, obs_pose=q.obs_pose, obs_dims=q.obs_dims)


def permuted(batch):
    """frame_of / scene_of no longer the identity: ego b drives on line PERM_F[b] before scene PERM_S[b]; ego 5 has no scene.  Each ego
    keeps its start arclength on the new line (all lines sample the same road), every other ego an obstacle in front of it."""
    frame_of = np.array([3, 0, 6, 1, 7, 2, 5, 4], dtype=batch.frame_of.dtype)
    scene_of = np.array([1, 2, 3, 4, 5, -1, 7, 6], dtype=batch.scene_of.dtype)
    return park(_keep(batch, frame_of=frame_of, scene_of=scene_of), egos=[0, 2, 4, 6])


CASES = {
    "t_now odd": lambda: t_now_odd(park(base997(9400))),
    "table shorter than the horizon (13 of 25 rows staged)": lambda: short_table(park(base997(9401))),
    "final_time_step inside the table (11 rows checked)": lambda: early_final_step(park(base997(9402))),
    "a line that ends inside the checked rows": lambda: line_ends_early(base997(9403)),
    "more survivors than the 256-entry list holds": lambda: crowded(base997(9404)),
    "frame_of / scene_of permuted, one ego without a scene": lambda: permuted(base997(9405)),
    "220 knots (coefficient window), t_now odd": lambda: t_now_odd(park(base997(9406, n_knots=220))),
    "5 x 5 x 5: t_now odd, final_time_step inside the table": lambda: early_final_step(park(base555(9407))),
    "5 x 5 x 5: permuted, one ego without a scene": lambda: permuted(base555(9408)),
    "5 x 4 x 3 (nv != nd): t_now odd, final_time_step inside the table": lambda: early_final_step(park(base_runtime(9409))),
    "5 x 4 x 3 (nv != nd): table shorter than the horizon": lambda: short_table(park(base_runtime(9410))),
}
SHAPED_997 = {n for n in CASES if not n.startswith("5 x")}
SHAPED_555 = {n for n in CASES if n.startswith("5 x 5 x 5")}
# the skipped ego stands between two live ones (fp_batch.skip: the device entry point alone takes it)
SKIP = np.array([0, 0, 0, 1, 0, 0, 1, 0], dtype=np.int32)
ORDER = np.array([5, 2, 7, 0, 3, 6, 1, 4], dtype=np.int32)  # a caller's launch order: no ego in its own slot

FISS_CASES = {
    "FISS+ 9 x 9 x 7: t_now odd, final_time_step inside the table": lambda: early_final_step(park(base997(9420, kind="FISS+"))),
    "FISS+ 9 x 9 x 7: permuted, one ego without a scene": lambda: permuted(base997(9421, kind="FISS+")),
    # (a run-time shape the appended search takes: more than 256 candidates)
    "FISS+ 7 x 8 x 6: table shorter than the horizon": lambda: short_table(park(synth.make_batch(B, 7, 8, 6, 7, 50, True, 9422, kind="FISS+", layout="survey8d"))),
}
