"""Independent restatement of the obstacle-clearance cost term (fp_params.w_obstacle), numpy + the CPU oracle only.

For one ego of a ProblemBatch everything about a candidate comes from the ORACLE - its flag word, its base cost, its dumped
x / y / yaw series - and the term is restated from its definition (include/frenet_gpu.h):

    poses      i = 0, cs, 2 cs, ... < min(M, final_time_step - t_now), the veh_l x veh_w rectangle at (x[i], y[i], yaw[i])
    obstacles  the columns with a valid pose at step i + t_now (rectangle of obs_dims, or the column's ring)
    dist       0 when the two shapes intersect (the oracle's boxes_intersect / box_ring_intersect), else the smallest
               vertex-to-segment distance both ways (brute force over all vertices and all edges)
    clearance  sum_i sum_j exp(-dist)
    cost       (base * N + w * clearance) / N   for survivors (no infeasible bit); every other candidate keeps the oracle's cost
    winner     minimum of the new cost over survivors, the LAST one in FOP index order on exact ties

Nothing here calls the library under test."""
import numpy as np

FLAG_INFEASIBLE = 1 | 2 | 4 | 16 | 32 | 64  # FP_FLAG_CONSTRAINTS | FP_FLAG_COLLISION (include/frenet_gpu.h)


def box_corners(l, w, x, y, yaw):
    """Corners [..., 4, 2] of l x w rectangles centred on (x, y), counter-clockwise."""
    x, y, yaw = np.broadcast_arrays(np.asarray(x, float), np.asarray(y, float), np.asarray(yaw, float))
    c, s = np.cos(yaw), np.sin(yaw)
    u = np.array([[0.5, 0.5], [-0.5, 0.5], [-0.5, -0.5], [0.5, -0.5]]) * np.array([l, w])
    px = x[..., None] + c[..., None] * u[:, 0] - s[..., None] * u[:, 1]
    py = y[..., None] + s[..., None] * u[:, 0] + c[..., None] * u[:, 1]
    return np.stack([px, py], axis=-1)


def ring_at(ring, x, y, yaw):
    """World vertices [..., n, 2] of a ring [n, 2] (relative to its rotation centre) at poses (x, y, yaw)."""
    x, y, yaw = np.broadcast_arrays(np.asarray(x, float), np.asarray(y, float), np.asarray(yaw, float))
    c, s = np.cos(yaw), np.sin(yaw)
    px = x[..., None] + c[..., None] * ring[:, 0] - s[..., None] * ring[:, 1]
    py = y[..., None] + s[..., None] * ring[:, 0] + c[..., None] * ring[:, 1]
    return np.stack([px, py], axis=-1)


def _points_to_segments(P, A):
    """Smallest distance of any point of P [..., m, 2] to any edge of the closed ring A [..., n, 2]."""
    a = A[..., None, :, :]                                   # [..., 1, n, 2]
    e = np.roll(A, -1, axis=-2)[..., None, :, :] - a         # edge vectors
    r = P[..., :, None, :] - a                               # [..., m, n, 2]
    len2 = np.sum(e * e, axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(len2 > 0, np.sum(r * e, axis=-1) / len2, 0.0)
    t = np.clip(t, 0.0, 1.0)
    q = r - t[..., None] * e
    return np.sqrt(np.sum(q * q, axis=-1)).min(axis=(-1, -2))


def ring_distance(A, B):
    """Brute-force distance of two DISJOINT convex rings [..., n, 2] / [..., m, 2]: every vertex against every edge, both ways."""
    return np.minimum(_points_to_segments(A, B), _points_to_segments(B, A))


def convex_distance(O, ego_box, shape, pose=None):
    """dist of the definition for one pair.  ego_box = (l, w, x, y, yaw); shape = an obstacle box (l, w, x, y, yaw), or - with pose -
    a ring [n, 2] relative to its rotation centre at pose (x, y, yaw)."""
    E = box_corners(*ego_box)
    if pose is None:
        if O.boxes_intersect(ego_box, shape):
            return 0.0
        return float(ring_distance(E, box_corners(*shape)))
    if O.box_ring_intersect(ego_box, shape, pose):
        return 0.0
    return float(ring_distance(E, ring_at(np.asarray(shape, float), *pose)))


def ego_table(O, batch, b, w_obstacle=None, details=False):
    """(cost [C], flags [C], best_idx, best_cost) of ego b under the clearance term; w_obstacle None = the batch's own weight.
    details=True: also {candidate: (clearance, poses, pairs)} for the survivors."""
    w = float(getattr(batch, "w_obstacle", 0.0) if w_obstacle is None else w_obstacle)
    prob = O.problems_from_batch(batch, egos=[b])[0]
    cost, flags = prob.dense_tables()
    cost = cost.copy()
    info = {}
    sc = int(batch.scene_of[b])
    has_obs = sc >= 0 and batch.n_obs > 0
    nv, nt = batch.nv, batch.nt
    cs, t_now = int(batch.check_stride), int(batch.t_now[b])
    stride = 256
    survivors = np.nonzero((flags & FLAG_INFEASIBLE) == 0)[0]
    if w > 0.0 and has_obs:
        pose_tab, dims = batch.obs_pose[sc], batch.obs_dims[sc]
        T_obs = pose_tab.shape[0]
        horizon = int(batch.final_time_step[sc]) - t_now
        nvert = batch.obs_nvert[sc] if getattr(batch, "obs_nvert", None) is not None else np.zeros(batch.n_obs, dtype=np.int32)
        for c in survivors:
            iv, it, i_d = c % nv, (c // nv) % nt, c // (nv * nt)
            r = prob.eval_traj(float(batch.d_samples[i_d]), float(batch.v_samples[b, iv]), float(batch.t_samples[it]), dump=True, stride=stride)
            N, M = r.N, r.M
            assert N == (int(flags[c]) >> 8) & 0xFFF and M == int(flags[c]) >> 20
            x, y, yaw = r.arrays[9, :M], r.arrays[10, :M], r.arrays[11, :M]
            idx = np.array([i for i in range(0, max(min(M, horizon), 0), cs) if 0 <= i + t_now < T_obs], dtype=int)
            clear, pairs = 0.0, 0
            if idx.size:
                E = box_corners(batch.veh_l, batch.veh_w, x[idx], y[idx], yaw[idx])          # [P, 4, 2]
                rows = pose_tab[idx + t_now]                                                   # [P, n_obs, 4]
                for j in range(batch.n_obs):
                    ok = rows[:, j, 3] != 0.0
                    if not ok.any():
                        continue
                    pj = rows[ok, j]
                    ego_boxes = np.stack([np.full(ok.sum(), batch.veh_l), np.full(ok.sum(), batch.veh_w), x[idx][ok], y[idx][ok], yaw[idx][ok]], axis=1)
                    if nvert[j] > 0:
                        ring = np.asarray(batch.obs_poly[sc, j, :nvert[j]], float)
                        hit = np.array([bool(O.box_ring_intersect(ego_boxes[k], ring, pj[k, :3])) for k in range(len(pj))])
                        Bv = ring_at(ring, pj[:, 0], pj[:, 1], pj[:, 2])
                    else:
                        obs_boxes = np.stack([np.full(len(pj), dims[j, 0]), np.full(len(pj), dims[j, 1]), pj[:, 0], pj[:, 1], pj[:, 2]], axis=1)
                        hit = O.boxes_intersect_batch(ego_boxes, obs_boxes) != 0
                        Bv = box_corners(dims[j, 0], dims[j, 1], pj[:, 0], pj[:, 1], pj[:, 2])
                    dist = np.where(hit, 0.0, ring_distance(E[ok], Bv))
                    clear += float(np.sum(np.exp(-dist)))
                    pairs += int(ok.sum())
            cost[c] = (cost[c] * N + w * clear) / N
            info[int(c)] = (clear, int(idx.size), pairs)
    best_idx, best_cost = -1, np.nan
    for c in survivors:  # `min_cost >= cost`: the last minimum wins; a NaN cost never does (frenet_optimal_planner.py:264-268)
        if cost[c] == cost[c] and (best_idx < 0 or best_cost >= cost[c]):
            best_idx, best_cost = int(c), float(cost[c])
    out = (cost, flags, best_idx, best_cost)
    return out + (info,) if details else out


def batch_tables(O, batch, w_obstacle=None, egos=None):
    """cost [B', C], flags [B', C], best_idx [B'], best_cost [B'] for the egos asked for (all by default)."""
    rows = [ego_table(O, batch, b, w_obstacle) for b in (range(batch.B) if egos is None else egos)]
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.array([r[2] for r in rows], dtype=np.int32),
            np.array([r[3] for r in rows]))


def winner_series(O, batch, b, best_idx, stride=128):
    """The oracle's dumped [16, stride] series of candidate best_idx of ego b."""
    prob = O.problems_from_batch(batch, egos=[b])[0]
    iv, it, i_d = best_idx % batch.nv, (best_idx // batch.nv) % batch.nt, best_idx // (batch.nv * batch.nt)
    return prob.eval_traj(float(batch.d_samples[i_d]), float(batch.v_samples[b, iv]), float(batch.t_samples[it]), dump=True, stride=stride).arrays


def margin(cost, flags):
    """Relative gap between the best and the second-best survivor cost of one ego (inf with fewer than two)."""
    v = np.sort(cost[((flags & FLAG_INFEASIBLE) == 0) & ~np.isnan(cost)])
    return np.inf if v.size < 2 else (v[1] - v[0]) / max(1.0, abs(v[0]))
