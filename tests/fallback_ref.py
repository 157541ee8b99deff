"""Independent restatement of fp_fallback_stop (a stopping manoeuvre for the egos without a plan), numpy + the CPU oracle only.

For every ego of a ProblemBatch that needs a fallback (best_idx < 0, or a NaN end state; not skipped) the family's candidates
f = i_d * n_stop + i_T = (d_targets[i_d] or d0, 0, stop_T[i_T]) are restated from the definition (include/frenet_gpu.h):

    series       prob.eval_traj(d, 0.0, T, dump=True), as margins_ref obtains them
    admissible   N <= the points the call is sized for, M >= 2, every s_d[i] >= -REVERSE_TOL and every -s_dd[i] <= max_decel, i < N,
                 from the dumped s_d / s_dd rows
    contact      the oracle's boxes_intersect / box_ring_intersect, pose by pose over i = 0, check_stride, ... < min(M, final_time_step
                 - t_now) with 0 <= i + t_now < T_obs; the first pose with a hit and its smallest column
    choice       a plain loop over the key (contact, -i_T | (-hit_step, i_T), |d_end - d0|, i_d)

It also reports what makes a comparison meaningful: per candidate the slack of the two admissibility thresholds, and whether its
(hit_step, hit_obs) stays the same with every obstacle's obs_dims (and ring) grown and shrunk by PERTURB.  An ego counts when every
candidate's slack exceeds SLACK_MIN and every verdict is stable under both perturbations; otherwise it is left out as a whole.

Nothing here calls the library under test."""
from types import SimpleNamespace

import numpy as np

REVERSE_TOL = 1e-6   # FP_FALLBACK_REVERSE_TOL
MAX_FALLBACK = 256   # FP_MAX_FALLBACK
NOT_NEEDED, CLEAR, CONTACT, NONE = 0, 1, 2, 3
SLACK_MIN = 1e-9     # m/s, m/s^2: an admissibility threshold closer than this to a series value is not compared
PERTURB = 2e-6       # m: obstacle sizes grown / shrunk by this must give the same first contact
SPEED_TOL = 1e-9     # hit_speed
MAX_LEFT_OUT = 1     # egos per fixture the reference may leave out
FAST_POINTS, MAX_POINTS = 128, 256


def points_cap(batch, stop_T):
    """The points a FP_MEM_HOST call is sized for: the largest ceil(T / tick_t) over the lattice's time samples and the stop times,
    FP_FAST_POINTS at the least, FP_MAX_POINTS at the most (host_points_max / points_cap of the library, restated)."""
    n = max(np.ceil(np.asarray(t, dtype=np.float64) / batch.tick_t).max() for t in (batch.t_samples, stop_T))
    return int(min(n, MAX_POINTS)) if n > FAST_POINTS else FAST_POINTS


def decode(batch, b, idx):
    """(d, v, T) of flat FOP index idx of ego b (for d: for T: for v)."""
    iv, it, i_d = idx % batch.nv, (idx // batch.nv) % batch.nt, idx // (batch.nv * batch.nt)
    return float(batch.d_samples[i_d]), float(batch.v_samples[b, iv]), float(batch.t_samples[it])


def _grown_ring(ring, by):
    r = np.hypot(ring[:, 0], ring[:, 1])
    return ring * (1.0 + by / np.maximum(r, 1e-300))[:, None]


def first_contact(O, batch, b, x, y, yaw, M, grow=0.0):
    """(hit_step, hit_obs) of one series against the ego's scene, (-1, -1) without contact; every obstacle's dims (and ring) grown by `grow`."""
    sc = int(batch.scene_of[b])
    if sc < 0 or batch.n_obs == 0 or M < 2:
        return -1, -1
    t_now, T_obs, cs = int(batch.t_now[b]), batch.T_obs, int(batch.check_stride)
    horizon = int(batch.final_time_step[sc]) - t_now
    idx = np.array([i for i in range(0, max(min(M, horizon), 0), cs) if 0 <= i + t_now < T_obs], dtype=int)
    if not idx.size:
        return -1, -1
    rows = batch.obs_pose[sc][idx + t_now]  # [P, n, 4]
    dims = batch.obs_dims[sc] + grow
    nvert = batch.obs_nvert[sc] if getattr(batch, "obs_nvert", None) is not None else np.zeros(batch.n_obs, dtype=np.int32)
    P, n = rows.shape[:2]
    hit = np.zeros((P, n), dtype=bool)
    valid = rows[:, :, 3] != 0.0
    rect = valid & (nvert[None, :] == 0)
    q, j = np.nonzero(rect)
    if q.size:
        ego = np.stack([np.full(q.size, batch.veh_l), np.full(q.size, batch.veh_w), x[idx][q], y[idx][q], yaw[idx][q]], axis=1)
        obs = np.stack([dims[j, 0], dims[j, 1], rows[q, j, 0], rows[q, j, 1], rows[q, j, 2]], axis=1)
        res = O.boxes_intersect_batch(ego, obs)
        assert (res >= 0).all()
        hit[q, j] = res != 0
    for q, j in zip(*np.nonzero(valid & (nvert[None, :] > 0))):
        ring = _grown_ring(np.asarray(batch.obs_poly[sc, j, :nvert[j]], dtype=np.float64), grow)
        i = idx[q]
        hit[q, j] = bool(O.box_ring_intersect((batch.veh_l, batch.veh_w, x[i], y[i], yaw[i]), ring, rows[q, j, :3]))
    for q in range(P):  # poses ascending, then columns ascending: a plain loop
        for j in range(n):
            if hit[q, j]:
                return int(idx[q]), int(j)
    return -1, -1


def candidate(O, batch, prob, b, d_end, T, max_decel, cap):
    """One candidate -> SimpleNamespace(adm, N, M, slack, hit_step, hit_obs, hit_speed, stable)."""
    N = int(np.ceil(T / batch.tick_t))
    out = SimpleNamespace(adm=False, N=N, M=0, slack=np.inf, hit_step=-1, hit_obs=-1, hit_speed=np.nan, stable=True)
    if N < 1 or N > cap:
        return out
    r = prob.eval_traj(d_end, 0.0, T, dump=True, stride=MAX_POINTS)
    assert r.N == N, (r.N, N)
    out.M = r.M
    s_d, s_dd = r.arrays[2, :N], r.arrays[3, :N]
    slack = [np.abs(s_d + REVERSE_TOL).min()]
    if np.isfinite(max_decel):
        slack.append(np.abs(max_decel + s_dd).min())
    out.slack = float(min(slack))
    out.adm = bool(r.M >= 2 and (s_d >= -REVERSE_TOL).all() and (-s_dd <= max_decel).all())
    if not out.adm:
        return out
    x, y, yaw = r.arrays[9, :r.M], r.arrays[10, :r.M], r.arrays[11, :r.M]
    out.hit_step, out.hit_obs = first_contact(O, batch, b, x, y, yaw, r.M)
    out.stable = all(first_contact(O, batch, b, x, y, yaw, r.M, g) == (out.hit_step, out.hit_obs) for g in (PERTURB, -PERTURB))
    if out.hit_step >= 0:
        out.hit_speed = float(s_d[out.hit_step])
    return out


def choose(cands, d_ends, d0, n_stop):
    """The winner's f among the admissible candidates (None: none) by the definition's order, as a plain loop over the key."""
    best, best_key = None, None
    for f, c in enumerate(cands):
        if not c.adm:
            continue
        i_d, i_T = divmod(f, n_stop)
        key = (0, -i_T, 0) if c.hit_step < 0 else (1, -c.hit_step, i_T)
        key = key + (abs(d_ends[i_d] - d0), i_d)
        if best is None or key < best_key:
            best, best_key = f, key
    return best


def fallback(O, batch, stop_T, d_targets=None, max_decel=np.inf, best_idx=None, end_state=None, skip=None, cap=None):
    """The call's outputs for every ego, plus `counted` [B] (False: the ego is left out of a comparison), `slack`, `stable` and the series'
    N and M [B, F] (0 where no series was made)."""
    assert (best_idx is None) != (end_state is None)
    stop_T = np.asarray(stop_T, dtype=np.float64)
    d_targets = np.concatenate([[np.nan], batch.d_samples]) if d_targets is None else np.asarray(d_targets, dtype=np.float64)
    n_d, n_stop = len(d_targets), len(stop_T)
    F, B = n_d * n_stop, batch.B
    assert 1 <= F <= MAX_FALLBACK
    cap = points_cap(batch, stop_T) if cap is None else cap
    es = np.full((B, 3), np.nan) if best_idx is not None else np.array(end_state, dtype=np.float64).reshape(B, 3)
    res = SimpleNamespace(end_state=es, status=np.zeros(B, dtype=np.int32), fb_idx=np.full(B, -1, dtype=np.int32), hit_step=np.full(B, -1, dtype=np.int32),
                          hit_obs=np.full(B, -1, dtype=np.int32), hit_speed=np.full(B, np.nan), cand=np.full((B, F), -3, dtype=np.int32),
                          counted=np.ones(B, dtype=bool), slack=np.full((B, F), np.inf), stable=np.ones((B, F), dtype=bool), need=np.zeros(B, dtype=bool),
                          counts=np.zeros((B, 4), dtype=np.int32), N=np.zeros((B, F), dtype=np.int32), M=np.zeros((B, F), dtype=np.int32))
    for b in range(B):
        skipped = skip is not None and bool(skip[b])
        need = not skipped and (int(best_idx[b]) < 0 if best_idx is not None else bool(np.isnan(es[b, 0])))
        res.need[b] = need
        if not need:
            if best_idx is not None and not skipped:
                es[b] = decode(batch, b, int(best_idx[b]))
            res.counts[b, NOT_NEEDED] += 1
            continue
        prob = O.problems_from_batch(batch, egos=[b])[0]
        d0 = float(batch.ego[b, 3])
        d_ends = [d0 if np.isnan(d) else float(d) for d in d_targets]
        cands = [candidate(O, batch, prob, b, d_ends[f // n_stop], float(stop_T[f % n_stop]), max_decel, cap) for f in range(F)]
        res.cand[b] = [-2 if not c.adm else c.hit_step for c in cands]
        res.slack[b] = [c.slack for c in cands]
        res.stable[b] = [c.stable for c in cands]
        res.N[b], res.M[b] = [c.N for c in cands], [c.M for c in cands]
        res.counted[b] = bool((res.slack[b] > SLACK_MIN).all() and res.stable[b].all())
        f = choose(cands, d_ends, d0, n_stop)
        if f is None:
            res.status[b] = NONE
            es[b] = np.nan
        else:
            c = cands[f]
            res.status[b] = CLEAR if c.hit_step < 0 else CONTACT
            res.fb_idx[b], res.hit_step[b], res.hit_obs[b], res.hit_speed[b] = f, c.hit_step, c.hit_obs, c.hit_speed
            es[b] = (d_ends[f // n_stop], 0.0, stop_T[f % n_stop])
        res.counts[b, res.status[b]] += 1
    return res
