#!/usr/bin/env python3
"""How often stage W of the lattice kernel (csrc/frenet_lattice_fused.hip, `// [section WEXIT]`) finds a WHOLE ego blocked - every
candidate collides, the answer is "none" whatever the assembly and the argmin do - and how much of that an earlier verdict could
reach: a CPU estimate from the oracle and numpy alone, for any layout and config.

  python tools/whole_hit_estimate.py [config number | layout] [--B 2048] [--offset 0] [--every 16]

Three shares of the sampled egos:

  all collide   every candidate collides in the oracle.  The kernel reaches its verdict for these egos unless a lon profile has fewer
                than two points on the line (M < 2: never walked, never marked; the assembly flags it) - counted beside it.
  V ends all    stage V's circle (tools/group_hit_estimate.py: kernel_circle) ends all nv end-speed groups before the walk.
  one circle    ONE circle per checked row around the ego centres of ALL lon profiles - kernel_circle over every end speed and
                horizon, the row a pose of every profile - lies within stage S's sure-hit distance of an obstacle's box: the test a
                verdict in front of stage V's own circles would make.

and the number of egos a circle ended although the oracle keeps a candidate free, which must be 0.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import group_hit_estimate as G  # noqa: E402
from fiss_plus_planner_amd import synth  # noqa: E402

E, O = G.E, G.O
M_SHIFT = 20  # the truncation index M in a flag word (FP_FLAG_M_SHIFT)


def whole_circle_row(batch, b, prob):
    """The first checked pose at which the one circle around ALL lon profiles of ego b ends the ego (dist + radius <= thr for an
    obstacle with a state there), or -1.  Rows are the poses every profile of every end speed has."""
    if not E.threshold(batch) > 0:
        return -1
    groups = [G.group_rows(batch, b, prob, iv) for iv in range(batch.nv)]
    if any(g is None for g in groups):
        return -1
    n = min(len(g[0]) for g in groups)
    sc, t_now = int(batch.scene_of[b]), int(batch.t_now[b])
    thr = E.threshold(batch)
    for r in range(n):
        k = int(groups[0][0][r])
        circ = G.kernel_circle(batch, b, np.concatenate([g[1][:, r] for g in groups]), np.concatenate([g[2][:, :, r].ravel() for g in groups]))
        if circ is None:
            continue
        pose = batch.obs_pose[sc, t_now + k][None]
        gone = (pose[0, :, 3] == 0.0) | ~np.isfinite(pose[0, :, :3]).all(axis=-1)
        with np.errstate(invalid="ignore"):
            signed = E.box_distance(circ[0][None], pose, batch.obs_dims[sc])[0] + circ[1] - thr
        if (signed[~gone] <= 0).any():
            return k
    return -1


def ego_verdicts(batch, b):
    """(every candidate collides (oracle), the kernel's verdict is reached - that and every lon profile has M >= 2 -, V ends all nv
    groups, the row at which the one circle ends the ego or -1)."""
    prob = O.problems_from_batch(batch, [b])[0]
    flags = prob.fop_plan().flags
    all_coll = bool(((flags & 4) != 0).all())
    reached = all_coll and bool(((flags >> M_SHIFT) >= 2).all())
    v_all = all(g[2] >= 0 for g in G.ego_groups(batch, b))
    return all_coll, reached, v_all, whole_circle_row(batch, b, prob)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", nargs="?", default="survey8d")
    ap.add_argument("--B", type=int, default=2048)
    ap.add_argument("--offset", type=int, default=0)
    ap.add_argument("--every", type=int, default=16, help="sample every n-th ego")
    a = ap.parse_args()
    config, layout = (int(a.what), "survey8d") if a.what.isdigit() else (3, a.what)
    kw = {"ego_offset": a.offset} if a.offset else {}
    batch = synth.make_config(config, B=a.B, layout=layout, **kw)
    n = n_coll = n_reached = n_v = n_w = unsound = 0
    rows = []
    for b in range(0, batch.B, a.every):
        all_coll, reached, v_all, k_w = ego_verdicts(batch, b)
        n += 1
        n_coll += all_coll
        n_reached += reached
        n_v += v_all
        n_w += k_w >= 0
        unsound += (v_all or k_w >= 0) and not all_coll
        if k_w >= 0:
            rows.append(k_w // batch.check_stride)
    print(f"config {config}, layout {layout}, offset {a.offset}: {n} egos of {batch.nd} x {batch.nv} x {batch.nt} candidates")
    print(f"  every candidate collides (oracle)                   {n_coll:6d}  {100 * n_coll / n:5.1f} %")
    print(f"  ... and every lon profile has M >= 2: the kernel's verdict (assembly and argmin skipped) {n_reached:6d}  {100 * n_reached / n:5.1f} %")
    print(f"  stage V ends all {batch.nv} end-speed groups                 {n_v:6d}  {100 * n_v / n:5.1f} %")
    print(f"  one circle per row around all lon profiles ends the ego {n_w:6d}  {100 * n_w / n:5.1f} %")
    if rows:
        print(f"  row of that circle's hit: median {np.median(rows):.0f}, max {max(rows)}")
    print(f"  egos ended by a circle in which the oracle keeps a candidate free {unsound:6d}  (must be 0)")
    return 1 if unsound else 0


if __name__ == "__main__":
    sys.exit(main())
