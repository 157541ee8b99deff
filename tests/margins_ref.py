"""Independent restatement of fp_traj_margins (the obstacle margin of chosen plans), numpy + the CPU oracle only.

For plane k and ego b of a ProblemBatch the plan's series come from the ORACLE (eval_traj(..., dump=True), exactly as
clearance_ref.ego_table obtains them) and the margin is restated from its definition (include/frenet_gpu.h):

    trajectory  lattice candidate best_idx[k, b], or the explicit end state end_state[k, b] = (d, v, T); points 0 .. M-1 with
                x, y, yaw from the dump.  M < 2: no heading, no pose.
    poses       i = 0, ps, 2 ps, ... < min(M, final_time_step - t_now) with 0 <= i + t_now < T_obs: the veh_l x veh_w rectangle
    obstacles   the columns with a valid pose at row i + t_now (rectangle of obs_dims, or the column's ring)
    dist        clearance_ref.convex_distance: 0 when the two shapes intersect (the oracle's boxes_intersect / box_ring_intersect),
                else the brute-force vertex-to-edge distance both ways.  Rectangle columns go through the oracle's batch call and
                clearance_ref.ring_distance a column at a time - the same arithmetic (tests/test_margins_cpu.py compares the two)
    min_dist    minimum over all pairs; +inf without a pair; NaN without a trajectory (index < 0, NaN end state, skipped ego)
    min_step, min_obs   i and j of the minimum; among equal distances the smallest i, then the smallest j (a plain loop); -1, -1
                when min_dist is +inf or NaN

Per plan it also returns `gap`, the difference between the second-smallest and the smallest pair distance (inf with fewer than two
pairs), and `min_nonzero`, the smallest pair distance that is not 0 (inf without one): what decides whether the comparison of
min_step / min_obs with another implementation of the same definition is meaningful (DECIDE_TOL).

Nothing here calls the library under test."""
from types import SimpleNamespace

import numpy as np

import clearance_ref as CR

DIST_TOL = 1e-9     # min_dist: the distance within which the project's audit bits call a verdict near contact (FP_AUDIT_GAP_TOL)
DECIDE_TOL = 1e-6   # a plan's min_step / min_obs count when its gap exceeds this, or when smallest and second smallest are both 0
MIN_COUNTED = 0.9   # share of the plans with a pair that must count, per fixture


def end_state_of(batch, b, idx):
    """(d, v, T) of flat FOP index idx of ego b."""
    iv, it, i_d = idx % batch.nv, (idx // batch.nv) % batch.nt, idx // (batch.nv * batch.nt)
    return float(batch.d_samples[i_d]), float(batch.v_samples[b, iv]), float(batch.t_samples[it])


def pair_distances(O, batch, b, x, y, yaw, idx):
    """dist [P, n_obs] of the poses idx (point indices) of one series against the ego's scene; NaN where the column has no valid pose."""
    sc, t_now = int(batch.scene_of[b]), int(batch.t_now[b])
    pose_tab, dims = batch.obs_pose[sc], batch.obs_dims[sc]
    nvert = batch.obs_nvert[sc] if getattr(batch, "obs_nvert", None) is not None else np.zeros(batch.n_obs, dtype=np.int32)
    out = np.full((len(idx), batch.n_obs), np.nan)
    E = CR.box_corners(batch.veh_l, batch.veh_w, x[idx], y[idx], yaw[idx])
    rows = pose_tab[idx + t_now]
    for j in range(batch.n_obs):
        ok = rows[:, j, 3] != 0.0
        if not ok.any():
            continue
        pj, n = rows[ok, j], int(ok.sum())
        ego_boxes = np.stack([np.full(n, batch.veh_l), np.full(n, batch.veh_w), x[idx][ok], y[idx][ok], yaw[idx][ok]], axis=1)
        if nvert[j] > 0:
            ring = np.asarray(batch.obs_poly[sc, j, :nvert[j]], float)
            out[ok, j] = [CR.convex_distance(O, ego_boxes[k], ring, pj[k, :3]) for k in range(n)]
        else:
            obs_boxes = np.stack([np.full(n, dims[j, 0]), np.full(n, dims[j, 1]), pj[:, 0], pj[:, 1], pj[:, 2]], axis=1)
            hit = O.boxes_intersect_batch(ego_boxes, obs_boxes) != 0
            out[ok, j] = np.where(hit, 0.0, CR.ring_distance(E[ok], CR.box_corners(dims[j, 0], dims[j, 1], pj[:, 0], pj[:, 1], pj[:, 2])))
    return out


def lex_min(idx, dist):
    """(min_dist, min_step, min_obs) of dist [P, n] (NaN = no pair) by the definition's tie rule, as a plain loop."""
    best, bi, bj = np.inf, -1, -1
    for q, i in enumerate(idx):
        for j in range(dist.shape[1]):
            v = dist[q, j]
            if v == v and (bi < 0 or v < best):
                best, bi, bj = float(v), int(i), int(j)
    return best, bi, bj


def plan_margin(O, batch, prob, b, d_end, v_end, T_end, pose_stride):
    """One plan of ego b -> SimpleNamespace(min_dist, min_step, min_obs, gap, min_nonzero, n_pairs, N, M)."""
    none = SimpleNamespace(min_dist=np.nan, min_step=-1, min_obs=-1, gap=np.inf, min_nonzero=np.inf, n_pairs=0, N=0, M=0)
    if not (d_end == d_end and v_end == v_end and T_end == T_end):
        return none
    r = prob.eval_traj(d_end, v_end, T_end, dump=True, stride=256)
    out = SimpleNamespace(min_dist=np.inf, min_step=-1, min_obs=-1, gap=np.inf, min_nonzero=np.inf, n_pairs=0, N=r.N, M=r.M)
    sc = int(batch.scene_of[b])
    if sc < 0 or batch.n_obs == 0 or r.M < 2:
        return out
    t_now, T_obs = int(batch.t_now[b]), batch.obs_pose.shape[1]
    horizon = int(batch.final_time_step[sc]) - t_now
    idx = np.array([i for i in range(0, max(min(r.M, horizon), 0), int(pose_stride)) if 0 <= i + t_now < T_obs], dtype=int)
    if not idx.size:
        return out
    x, y, yaw = r.arrays[9, :r.M], r.arrays[10, :r.M], r.arrays[11, :r.M]
    dist = pair_distances(O, batch, b, x, y, yaw, idx)
    v = np.sort(dist[~np.isnan(dist)])
    if not v.size:
        return out
    out.min_dist, out.min_step, out.min_obs = lex_min(idx, dist)
    out.n_pairs = int(v.size)
    out.gap = float(v[1] - v[0]) if v.size > 1 else np.inf
    out.min_nonzero = float(v[v > 0][0]) if (v > 0).any() else np.inf
    return out


def margins(O, batch, best_idx=None, end_state=None, pose_stride=None, skip=None):
    """The three outputs [K, B] plus gap, min_nonzero, n_pairs and M (the series' Cartesian points, 0 without a trajectory) [K, B]
    for best_idx [K, B] (or [B]) / end_state [K, B, 3] (or [B, 3]); pose_stride None = the batch's check_stride."""
    assert (best_idx is None) != (end_state is None)
    ps = int(batch.check_stride if pose_stride is None else pose_stride)
    if best_idx is not None:
        best_idx = np.asarray(best_idx, dtype=np.int64).reshape(-1, batch.B)
        K = best_idx.shape[0]
    else:
        end_state = np.asarray(end_state, dtype=np.float64).reshape(-1, batch.B, 3)
        K = end_state.shape[0]
    res = SimpleNamespace(min_dist=np.full((K, batch.B), np.nan), min_step=np.full((K, batch.B), -1, dtype=np.int32),
                          min_obs=np.full((K, batch.B), -1, dtype=np.int32), gap=np.full((K, batch.B), np.inf),
                          min_nonzero=np.full((K, batch.B), np.inf), n_pairs=np.zeros((K, batch.B), dtype=np.int64),
                          M=np.zeros((K, batch.B), dtype=np.int64))
    for b in range(batch.B):
        if skip is not None and skip[b]:
            continue
        prob = O.problems_from_batch(batch, egos=[b])[0]
        seen = {}
        for k in range(K):
            if best_idx is not None:
                c = int(best_idx[k, b])
                es = end_state_of(batch, b, c) if 0 <= c < batch.C else (np.nan, np.nan, np.nan)
            else:
                es = tuple(float(v) for v in end_state[k, b])
            if es not in seen:
                seen[es] = plan_margin(O, batch, prob, b, *es, ps)
            m = seen[es]
            res.min_dist[k, b], res.min_step[k, b], res.min_obs[k, b] = m.min_dist, m.min_step, m.min_obs
            res.gap[k, b], res.min_nonzero[k, b], res.n_pairs[k, b], res.M[k, b] = m.gap, m.min_nonzero, m.n_pairs, m.M
    return res


def counted(ref):
    """Plans whose min_step / min_obs are compared: they have a pair, and the minimum is separated from the runner-up by more than
    DECIDE_TOL or both are exactly 0 (two contacts: the tie rule decides, and 0 is exact on both sides)."""
    has = ref.n_pairs > 0
    both_zero = (ref.min_dist == 0.0) & (ref.gap == 0.0)
    return has & ((ref.gap > DECIDE_TOL) | both_zero)


def decidable(ref):
    """(no pair distance in (0, DECIDE_TOL), share of the plans with a pair that count)."""
    has = ref.n_pairs > 0
    return bool((ref.min_nonzero[has] >= DECIDE_TOL).all()), float(counted(ref)[has].mean()) if has.any() else 1.0
