"""Reference of fp_from_state for the tests: what the reference program does with one frame's tables, in float64, every decision made
by sequential code.

    resample(knots, coef)   generate_frenet_frame (frenet_optimal_planner.py:272-278): CubicSpline2D over the tables,
                            s = np.arange(0, s_last, 0.1), then x, y, yaw at every s - the polyline [n, 3]
    project(pl, pose)       FrenetState.from_state on that polyline (the oracle's orc_from_state)
    decide(pl, pose)        the reference's own decision margins for the pose: how far its two discrete choices (the nearest point, the
                            side of pi/2) are from flipping

A pose is DECIDABLE when the two smallest distances differ by >= GAP_MIN and |angle - pi/2| >= ANGLE_MIN: two correct implementations
whose resampled points differ by rounding (1e-13 m at a 500 m offset) then take the same branches.  assert_projection compares s, s_d
and d_d on decidable poses; d where |d_ref| >= D_MIN, otherwise only |d| < D_MIN (the sign rule `wp_yaw <= x_yaw` flips on the line
itself).  These are conditions on the input, not measurements of the code under test.

Also the seeded generators the CPU and GPU tests share (ragged_frames, random_poses, clamp_poses)."""
import math
from types import SimpleNamespace

import numpy as np

from fiss_plus_planner_amd.spline import CubicSpline2D

GAP_MIN, ANGLE_MIN, D_MIN = 1e-9, 1e-9, 1e-6
EGO_ATOL = 1e-8  # the project's tolerance on ego rows (tests/test_gpu_frame.py, golden G7)
STEP = 0.1


def resample(knots, coef):
    """knots [n], coef [8, n] of ONE frame (used rows only) -> polyline [len(np.arange(0, s_last, 0.1)), 3] = x, y, yaw.
    Raises like the reference where it raises: IndexError when a sampled arclength reaches s_last (the spline has no segment there),
    ValueError when s_last is not finite."""
    sp = CubicSpline2D(None, None, tables=(np.asarray(knots, dtype=np.float64), np.asarray(coef, dtype=np.float64)))
    s_last = sp.s[-1]
    if not math.isfinite(s_last):
        raise ValueError(f"s_last={s_last}")
    s = np.arange(0, s_last, STEP)
    pl = np.empty((len(s), 3))
    for i, si in enumerate(s):
        pl[i, 0], pl[i, 1] = sp.calc_position(si)
        pl[i, 2] = sp.calc_yaw(si)
    return pl


def project(oracle, pl, pose):
    """-> [6] = s, s_d, 0, d, d_d, 0"""
    return oracle.from_state(pose[0], pose[1], pose[2], pose[3], pl)


def decide(pl, pose):
    dist = np.hypot(pl[:, 0] - pose[0], pl[:, 1] - pose[1])
    nearest = int(np.argmin(dist))
    two = np.partition(dist, 1)[:2] if len(dist) > 1 else np.array([dist[0], np.inf])
    heading = math.atan2(pl[nearest, 1] - pose[1], pl[nearest, 0] - pose[0])
    angle = abs(pose[2] - heading)
    angle = min(2 * math.pi - angle, angle)
    raw_next = nearest + 1 if angle > math.pi / 2 else nearest
    return SimpleNamespace(nearest=nearest, gap=float(two[1] - two[0]), angle=angle, angle_margin=abs(angle - math.pi / 2), raw_next=raw_next,
                           n=len(pl), decidable=bool(two[1] - two[0] >= GAP_MIN and abs(angle - math.pi / 2) >= ANGLE_MIN))


def reference_rows(oracle, knots, coef, nx, frame_of, poses):
    """The whole batch: -> (ref [B, 6], decisions [B], polylines {f: pl}).  Every referenced frame is resampled once."""
    pls = {int(f): resample(knots[f, : nx[f]], coef[f][:, : nx[f]]) for f in np.unique(frame_of)}
    ref = np.empty((len(poses), 6))
    dec = []
    for b, (f, pose) in enumerate(zip(frame_of, poses)):
        ref[b] = project(oracle, pls[int(f)], pose)
        dec.append(decide(pls[int(f)], pose))
    return ref, dec, pls


def assert_projection(got, ref, dec, max_undecidable=0.01, atol=EGO_ATOL, what=""):
    """The comparison rules above.  -> SimpleNamespace(undecidable share, largest errors) for the report."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape == (len(dec), 6), what
    ok = np.array([d.decidable for d in dec])
    share = 1.0 - ok.mean()
    assert share <= max_undecidable, f"{what}: {share:.4f} of the poses are undecidable"
    assert (got[:, [2, 5]] == 0).all(), what
    err = np.abs(got - ref)
    for col, name in ((0, "s"), (1, "s_d"), (4, "d_d")):
        bad = ok & ~(err[:, col] <= atol)
        assert not bad.any(), f"{what}: {name} of egos {np.nonzero(bad)[0][:8].tolist()} err {err[bad, col][:8]}"
    on_line = np.abs(ref[:, 3]) < D_MIN
    bad = ok & ~on_line & ~(err[:, 3] <= atol)
    assert not bad.any(), f"{what}: d of egos {np.nonzero(bad)[0][:8].tolist()} err {err[bad, 3][:8]} ref {ref[bad, 3][:8]}"
    bad = ok & on_line & ~(np.abs(got[:, 3]) < D_MIN)
    assert not bad.any(), f"{what}: d of egos {np.nonzero(bad)[0][:8].tolist()} on the line: {got[bad, 3][:8]}"
    m = ok & ~on_line
    return SimpleNamespace(undecidable=share, n=len(dec), err_s=float(err[ok, 0].max()), err_sd=float(err[ok, 1].max()),
                           err_d=float(err[m, 3].max()) if m.any() else 0.0, err_dd=float(err[ok, 4].max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# generators
def rotate_shift(xy, angle, shift):
    c, s = math.cos(angle), math.sin(angle)
    return np.column_stack([c * xy[:, 0] - s * xy[:, 1], s * xy[:, 0] + c * xy[:, 1]]) + np.asarray(shift)


def ragged_frames(seed=11, F=7, NX=96, shift=500.0):
    """F gentle sines of 2 .. NX knots, 0.5 - 3 m apart, each rotated by a random angle and shifted by up to +-shift m per axis:
    -> points [F, NX, 2] (rows >= n[f] zero), n [F] with n[0] = 2 and n[1] = NX."""
    rng = np.random.default_rng(seed)
    n = rng.integers(3, NX + 1, F).astype(np.int32)
    n[0], n[1] = 2, NX
    pts = np.zeros((F, NX, 2))
    for f in range(F):
        x = np.cumsum(rng.uniform(0.5, 3.0, n[f]))
        y = rng.uniform(0, 6) * np.sin(x / rng.uniform(20, 70))
        pts[f, : n[f]] = rotate_shift(np.column_stack([x, y]), rng.uniform(-math.pi, math.pi), rng.uniform(-shift, shift, 2))
    return pts, n


def random_poses(knots, coef, nx, frames, per_frame=200, seed=12):
    """per_frame poses on each of `frames`: arclength uniform over the line, lateral offset +-4 m, yaw offset uniform in +-pi (the
    nearest point lies ahead of some and behind others), speed 0 - 15 m/s.  -> frame_of [B], poses [B, 4], in frame order."""
    rng = np.random.default_rng(seed)
    fo, poses = [], []
    for f in frames:
        sp = CubicSpline2D(None, None, tables=(knots[f, : nx[f]], coef[f][:, : nx[f]]))
        s = rng.uniform(0.0, sp.s[-1], per_frame)
        off = rng.uniform(-4.0, 4.0, per_frame)
        x, y, yaw, _ = sp.sample(s)
        poses.append(np.column_stack([x - off * np.sin(yaw), y + off * np.cos(yaw), yaw + rng.uniform(-math.pi, math.pi, per_frame), rng.uniform(0, 15, per_frame)]))
        fo.append(np.full(per_frame, f, dtype=np.int32))
    return np.concatenate(fo), np.concatenate(poses)


def clamp_poses(knots, coef, nx, frames):
    """Two poses per frame, looking along the line: 2 m behind the first waypoint (the next-waypoint index is clamped up to 1) and 1 m
    past the last resampled one (clamped down to n - 1)."""
    fo, poses = [], []
    for f in frames:
        pl = resample(knots[f, : nx[f]], coef[f][:, : nx[f]])
        for (x, y, yaw), dist in ((pl[0], -2.0), (pl[-1], 1.0)):
            poses.append([x + dist * math.cos(yaw), y + dist * math.sin(yaw), yaw, 5.0])
            fo.append(f)
    return np.asarray(fo, dtype=np.int32), np.asarray(poses)


def point_count_margin(knots, nx):
    """Distance of s_last / 0.1 from the nearest integer, per frame: kernel and reference agree on the number of resampled points
    without any doubt when it is far from 0."""
    q = np.array([knots[f, nx[f] - 1] for f in range(len(nx))]) / STEP
    return np.abs(q - np.rint(q))
