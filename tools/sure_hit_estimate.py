#!/usr/bin/env python3
"""How often the walk's stage S (csrc/frenet_lattice_fused.hip, `// [section S]`) can end a blocked lon profile: a CPU estimate from
the oracle and numpy alone, for any layout and config.

  python tools/sure_hit_estimate.py [config number | layout] [--B 2048] [--offset 0] [--every 16] [--margin 1e-6]

A lon profile (horizon T, end speed v) is BLOCKED when all nd lateral candidates collide.  It has a SURE hit at a checked pose k
when, for one obstacle with a state there, both ends of the segment that holds the nd ego centres are closer to the obstacle's box
than thr = min(veh_l, veh_w) / 2 * (1 - 1e-9) - margin: the ego box contains the disk of that radius about its centre at any heading,
and the distance to a convex box is convex along the segment, so every candidate collides at k.  Two forms of the segment:

  +-dm    the symmetric fan P_k +- dm n_k, dm = the largest |d| of the two extreme lateral samples at k (what the kernel tests:
          it is the bound stage B already reads; the kernel's is rounded up to fp32 / fp16, this one is not)
  ends    the true ends: the centres of the two extreme-d candidates themselves

For every lon profile the two extreme-d candidates are dumped with Problem.eval_traj(dump=True); the reference point and normal come
from the spline at the dumped arclength.  Reported: the blocked share, the sure share of either form, the first sure row and the
number of sure profiles that the oracle does NOT call blocked - which must be 0.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fiss_plus_planner_amd import synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

ORC_S, ORC_D, ORC_X, ORC_Y = 1, 5, 9, 10  # slots of the oracle's trajectory dump (oracle/frenet_oracle.h)
MARGIN = 1e-6


def threshold(batch, margin=MARGIN):
    return 0.5 * min(batch.veh_l, batch.veh_w) * (1.0 - 1e-9) - margin


def box_distance(pts, pose, dims):
    """Distance from points [K, 2] to the boxes of poses [K, J, 4] (x, y, yaw, valid) with sizes [J, 2] (length, width): [K, J]."""
    dx, dy = pts[:, None, 0] - pose[..., 0], pts[:, None, 1] - pose[..., 1]
    c, s = np.cos(pose[..., 2]), np.sin(pose[..., 2])
    u, w = dx * c + dy * s, -dx * s + dy * c
    qx, qy = np.abs(u) - 0.5 * dims[None, :, 0], np.abs(w) - 0.5 * dims[None, :, 1]
    out = np.hypot(np.where(qx < 0, 0.0, qx), np.where(qy < 0, 0.0, qy))  # (np.where keeps a NaN; np.maximum would too, fmax would not)
    return out


def profile_segments(batch, b, prob, it, iv):
    """The checked poses of lon profile (it, iv) of ego b and, at each, the ends of both segments.

    Returns (k [K], Em, Ep, lo, hi) - the pose indices and four [K, 2] arrays - or None when the profile has no checked pose
    (fewer than two points, no scene, a NaN lateral sample)."""
    sc = int(batch.scene_of[b])
    if sc < 0 or batch.n_obs == 0 or not np.all(np.isfinite(batch.d_samples)):
        return None
    d_lo, d_hi = float(np.min(batch.d_samples)), float(np.max(batch.d_samples))
    T, v = float(batch.t_samples[it]), float(batch.v_samples[b, iv])
    lo = prob.eval_traj(d_lo, v, T, collision=False, dump=True)
    hi = prob.eval_traj(d_hi, v, T, collision=False, dump=True)
    M = lo.M
    k_end = min(M, int(batch.final_time_step[sc]) - int(batch.t_now[b]), batch.T_obs - int(batch.t_now[b]))
    if M < 2 or k_end <= 0:
        return None
    k = np.arange(0, k_end, batch.check_stride)
    f = int(batch.frame_of[b])
    px, py, yaw = synth.sample_frames(batch.knots[f:f + 1], batch.coef[f:f + 1], lo.arrays[ORC_S][k][None])
    P = np.stack([px[0], py[0]], axis=1)
    n = np.stack([-np.sin(yaw[0]), np.cos(yaw[0])], axis=1)
    dm = np.maximum(np.abs(lo.arrays[ORC_D][k]), np.abs(hi.arrays[ORC_D][k]))
    c_lo = np.stack([lo.arrays[ORC_X][k], lo.arrays[ORC_Y][k]], axis=1)
    c_hi = np.stack([hi.arrays[ORC_X][k], hi.arrays[ORC_Y][k]], axis=1)
    return k, P - dm[:, None] * n, P + dm[:, None] * n, c_lo, c_hi


def sure_table(batch, b, prob, it, iv, margin=MARGIN):
    """(k [K], signed distances of the four ends to every obstacle's box minus thr: [4, K, J] in the order E-, E+, lo, hi; NaN where the
    obstacle has no state) or None.  An item (k, j) is sure with +-dm when both of the first two are <= 0, with the true ends when
    both of the last two are."""
    seg = profile_segments(batch, b, prob, it, iv)
    if seg is None:
        return None
    k = seg[0]
    sc, t_now = int(batch.scene_of[b]), int(batch.t_now[b])
    pose = batch.obs_pose[sc, k + t_now]  # [K, J, 4]
    gone = (pose[..., 3] == 0.0) | ~np.isfinite(pose[..., :3]).all(axis=-1)
    thr = threshold(batch, margin)
    out = np.stack([box_distance(e, pose, batch.obs_dims[sc]) - thr for e in seg[1:]])
    out[:, gone] = np.nan
    return k, out


def first_sure(signed):
    """(row index into k, obstacle) of the first sure item in time order, or None: signed is [2, K, J]."""
    with np.errstate(invalid="ignore"):
        sure = (signed[0] <= 0) & (signed[1] <= 0)
    at = np.argwhere(sure)
    return (int(at[0, 0]), int(at[0, 1])) if len(at) else None


def ego_report(batch, b, margin=MARGIN):
    """Per lon profile of ego b: blocked (oracle), first sure pose with +-dm and with the true ends (-1: none)."""
    prob = O.problems_from_batch(batch, [b])[0]
    coll = ((prob.fop_plan().flags & 4) != 0).reshape(batch.nd, batch.nt, batch.nv)  # c = (id * nt + it) * nv + iv
    rows = []
    for it in range(batch.nt):
        for iv in range(batch.nv):
            tab = sure_table(batch, b, prob, it, iv, margin)
            pm = ends = None
            if tab is not None and threshold(batch, margin) > 0:
                pm, ends = first_sure(tab[1][:2]), first_sure(tab[1][2:])
            rows.append((it, iv, bool(coll[:, it, iv].all()), bool(coll[:, it, iv].any()),
                         -1 if pm is None else int(tab[0][pm[0]]), -1 if ends is None else int(tab[0][ends[0]])))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", nargs="?", default="survey8d")
    ap.add_argument("--B", type=int, default=2048)
    ap.add_argument("--offset", type=int, default=0, help="ego offset of the batch (bench.py steps through offsets)")
    ap.add_argument("--every", type=int, default=16, help="sample every n-th ego")
    ap.add_argument("--margin", type=float, default=MARGIN)
    a = ap.parse_args()
    config, layout = (int(a.what), "survey8d") if a.what.isdigit() else (3, a.what)
    kw = {"ego_offset": a.offset} if a.offset else {}
    batch = synth.make_config(config, B=a.B, layout=layout, **kw)
    rows = [r for b in range(0, batch.B, a.every) for r in ego_report(batch, b, a.margin)]
    n = len(rows)
    blocked = sum(r[2] for r in rows)
    pm = [r for r in rows if r[4] >= 0]
    ends = [r for r in rows if r[5] >= 0]
    unsound = sum(1 for r in rows if (r[4] >= 0 or r[5] >= 0) and not r[2])
    print(f"config {config}, layout {layout}, offset {a.offset}: {batch.B // a.every} egos, {n} lon profiles, margin {a.margin:g} m")
    print(f"  blocked (all {batch.nd} lateral candidates collide)   {blocked:6d}  {100 * blocked / n:5.1f} %")
    print(f"  sure hit with +-dm                               {len(pm):6d}  {100 * len(pm) / n:5.1f} %  ({100 * len(pm) / max(blocked, 1):.1f} % of the blocked)")
    print(f"  sure hit with the true fan ends                  {len(ends):6d}  {100 * len(ends) / n:5.1f} %")
    if pm:
        rws = np.array([r[4] for r in pm]) // batch.check_stride
        print(f"  first sure row (+-dm): median {np.median(rws):.0f}, p90 {np.percentile(rws, 90):.0f}, max {rws.max()}")
    print(f"  sure profiles the oracle does not call blocked   {unsound:6d}  (must be 0)")
    return 1 if unsound else 0


if __name__ == "__main__":
    sys.exit(main())
