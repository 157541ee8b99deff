"""Independent restatement of fp_obstacles_from_plans (the egos' chosen plans as obstacle columns of each other's scenes), plain loops
over the CPU oracle's series, and a reference closed loop built from the project's existing reference pieces.

For member k of group g (ego a, column c = col_base + k) the plan's series come from the ORACLE (prob.eval_traj(d, v, T, dump=True), as
margins_ref.plan_margin obtains them) and the table is restated from the definition (include/frenet_gpu.h):

    a has a plan     skip[a] == 0; lattice index in 0 .. C-1 (decoded like margins_ref.end_state_of) or three finite end-state numbers;
                     N = ceil(T / tick_t) in 1 .. the points the call is sized for; the series has M >= 2 Cartesian points
    pose at step i   i < M: rows 9-11 (x, y, yaw) of the dump; i >= M: NONE nothing, HOLD pose M-1, COAST p[M-1] + (i-M+1)(p[M-1]-p[M-2])
    written          i = 0 .. n_rows-1, r = t_now[a] + i in 0 .. T_obs-1: [scene_of[b']][r][c] of every other member b' = (x, y, yaw, 1)
                     or zeros; [scene_of[a]][r][c] = zeros; nothing else is touched
    final_time_step  [scene_of[a]] = min(T_obs, max(t_now[a] + n_rows, 0))

Besides the expected table it returns `written` (the elements of the written set), `tol` (the tolerance of every written element: the
project's own series_tol of the reference dump for rows i < M, 1e-8 on x / y and the last yaw's tolerance for tail rows, 0 for
`valid`) and per ego N, M and whether it has a plan.

Nothing here calls the library under test."""
from types import SimpleNamespace

import numpy as np

import advance_ref as AR
import fallback_ref as FR
from conftest import series_tol

TAIL_NONE, TAIL_HOLD, TAIL_COAST = 0, 1, 2
FAST_POINTS, MAX_POINTS = 128, 256
POS_TOL = 1e-8


def points_cap(batch, extra_T=()):
    """The points a call is sized for: the largest ceil(T / tick_t) over the lattice's time samples and `extra_T` (NaN ignored),
    FP_FAST_POINTS at the least, FP_MAX_POINTS at the most."""
    ts = np.concatenate([np.asarray(batch.t_samples, dtype=np.float64).ravel(), np.asarray(extra_T, dtype=np.float64).ravel()])
    n = np.ceil(ts / batch.tick_t)
    n = n[~np.isnan(n)]
    n = n.max() if n.size else 0
    return int(min(n, MAX_POINTS)) if n > FAST_POINTS else FAST_POINTS


def end_state_of(batch, b, idx):
    """(d, v, T) of flat FOP index idx of ego b (for d: for T: for v)."""
    iv, it, i_d = idx % batch.nv, (idx // batch.nv) % batch.nt, idx // (batch.nv * batch.nt)
    return float(batch.d_samples[i_d]), float(batch.v_samples[b, iv]), float(batch.t_samples[it])


def plan_of(O, batch, b, best_idx, end_state, skip, cap):
    """-> SimpleNamespace(has, N, M, dump [16, N] or None) of ego b's plan."""
    none = SimpleNamespace(has=False, N=0, M=0, dump=None)
    if skip is not None and skip[b]:
        return none
    if best_idx is not None:
        c = int(best_idx[b])
        if not 0 <= c < batch.C:
            return none
        d, v, T = end_state_of(batch, b, c)
    else:
        d, v, T = (float(x) for x in end_state[b])
        if not (np.isfinite(d) and np.isfinite(v) and np.isfinite(T)):
            return none
    N = int(np.ceil(T / batch.tick_t))
    if N < 1 or N > cap:
        return none
    r = O.problems_from_batch(batch, egos=[b])[0].eval_traj(d, v, T, collision=False, dump=True, stride=MAX_POINTS)
    assert r.N == N, (r.N, N)
    return SimpleNamespace(has=r.M >= 2, N=r.N, M=r.M, dump=r.arrays[:, :r.N].copy())


def table(O, batch, groups, n_rows, tail, col_base=0, best_idx=None, end_state=None, skip=None, obs_pose=None, final_time_step=None, cap=None):
    """The call on `batch` (whose ego / t_now are the plans' start) -> SimpleNamespace(pose [S, T_obs, n_obs, 4], fts [S], written
    [S, T_obs, n_obs] bool, tol [S, T_obs, n_obs, 4], fts_written [S] bool, has / N / M [B], plans).  obs_pose / final_time_step: the
    table before the call (default: the batch's); they are not modified."""
    assert (best_idx is None) != (end_state is None)
    pose = np.array(batch.obs_pose if obs_pose is None else obs_pose, dtype=np.float64, copy=True)
    fts = np.array(batch.final_time_step if final_time_step is None else final_time_step, dtype=np.int32, copy=True)
    S, T_obs, n_obs = pose.shape[:3]
    if cap is None:
        cap = points_cap(batch, () if end_state is None else np.asarray(end_state)[:, 2])
    written = np.zeros((S, T_obs, n_obs), dtype=bool)
    tol = np.zeros((S, T_obs, n_obs, 4))
    fts_written = np.zeros(S, dtype=bool)
    B = batch.B
    has, Ns, Ms = np.zeros(B, dtype=bool), np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    plans = {}
    for members in groups:
        for k, a in enumerate(members):
            c = col_base + k
            pl = plans[a] = plan_of(O, batch, a, best_idx, end_state, skip, cap)
            has[a], Ns[a], Ms[a] = pl.has, pl.N, pl.M
            t_now = int(batch.t_now[a])
            sa = int(batch.scene_of[a])
            fts[sa] = min(T_obs, max(t_now + n_rows, 0))
            fts_written[sa] = True
            stol = series_tol(pl.dump, batch.tick_t) if pl.has else None
            if pl.has:  # a step of exactly zero length has no bound there (2 pos_err / 0): its heading is atan2(0, 0) = 0 on both sides, exactly
                stol[11] = np.where(np.isfinite(stol[11]), stol[11], 0.0)
            for i in range(n_rows):
                r = t_now + i
                if not 0 <= r < T_obs:
                    continue
                el, et = np.zeros(4), np.zeros(4)
                if pl.has:
                    M = pl.M
                    x, y, yaw = pl.dump[9], pl.dump[10], pl.dump[11]
                    if i < M:
                        el = np.array([x[i], y[i], yaw[i], 1.0])
                        et = np.array([stol[9, i], stol[10, i], stol[11, i], 0.0])
                    elif tail == TAIL_HOLD:
                        el = np.array([x[M - 1], y[M - 1], yaw[M - 1], 1.0])
                        et = np.array([POS_TOL, POS_TOL, stol[11, M - 1], 0.0])
                    elif tail == TAIL_COAST:
                        n = i - M + 1
                        el = np.array([x[M - 1] + n * (x[M - 1] - x[M - 2]), y[M - 1] + n * (y[M - 1] - y[M - 2]), yaw[M - 1], 1.0])
                        et = np.array([POS_TOL, POS_TOL, stol[11, M - 1], 0.0])
                scenes = np.asarray(batch.scene_of)[list(members)]  # every member's scene gets the element, a's own scene zeros
                written[scenes, r, c] = True
                pose[scenes, r, c], tol[scenes, r, c] = el, et
                pose[sa, r, c], tol[sa, r, c] = 0.0, 0.0
    return SimpleNamespace(pose=pose, fts=fts, written=written, tol=tol, fts_written=fts_written, has=has, N=Ns, M=Ms, plans=plans)


def step_lengths(pl):
    """The lengths of the steps between consecutive Cartesian points of a plan's series (what the yaw tolerance divides by)."""
    x, y = pl.dump[9, :pl.M], pl.dump[10, :pl.M]
    return np.hypot(np.diff(x), np.diff(y))


# ---------------------------------------------------------------------------
# the reference closed loop: the oracle's plan, the fallback's restatement, this file's table, advance_ref's hand-over
# ---------------------------------------------------------------------------
def footprints_overlap(O, batch, cart, pairs):
    """cart [B, 3] = x, y, yaw (NaN: the ego did not move) -> True when the veh_l x veh_w footprints of some pair (a, b) intersect."""
    for a, b in pairs:
        if np.isnan(cart[a]).any() or np.isnan(cart[b]).any():
            continue
        if O.boxes_intersect((batch.veh_l, batch.veh_w, *cart[a]), (batch.veh_l, batch.veh_w, *cart[b])):
            return True
    return False


def group_pairs(groups):
    return [(a, b) for g in groups for i, a in enumerate(g) for b in g[i + 1:]]


def loop(O, batch, goal_xy, groups, n_rows, tail, col_base, cycles, stop_T=None, share=True, planner="FOP", plan=None):
    """The loop on the CPU: per cycle the oracle's plan of every running ego (FOP: fop_plan; or `plan`(batch, b, cycle) -> (d, v, T) / NaNs),
    the restatement of the fallback (stop_T given) for the egos it leaves without a plan, the table of the plans (share=True) written
    into the batch's own obs_pose / final_time_step, and advance_ref's hand-over.  `batch` is modified in place (pass a copy).
    -> SimpleNamespace(states [cycles + 1, B, 6] (NaN behind an ego's last cycle), cart [cycles, B, 3], done, cycles [B], overlap
    [cycles] bool (some pair of group members' footprints intersects after that cycle), undecided (fallback egos not counted))."""
    B = batch.B
    ego, t_now, done, ncyc = batch.ego.copy(), batch.t_now.copy(), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    states = np.full((cycles + 1, B, 6), np.nan)
    states[0] = ego
    carts = np.full((cycles, B, 3), np.nan)
    overlap = np.zeros(cycles, dtype=bool)
    pairs = group_pairs(groups)
    undecided = 0
    cap = FR.points_cap(batch, stop_T) if stop_T is not None else points_cap(batch)
    for k in range(cycles):
        if (done != 0).all():
            break
        batch.ego[...], batch.t_now[...] = ego, t_now
        es = np.full((B, 3), np.nan)
        best = np.full(B, -1, dtype=np.int32)
        for b in range(B):
            if done[b]:
                continue
            prob = O.problems_from_batch(batch, egos=[b])[0]
            if plan is None:
                best[b] = prob.fop_plan().best_idx
                if best[b] >= 0:
                    es[b] = end_state_of(batch, b, int(best[b]))
            else:
                es[b] = plan(batch, b, k)
        if stop_T is not None:
            r = FR.fallback(O, batch, stop_T, None, np.inf, end_state=es, skip=done, cap=cap)
            es = r.end_state
            undecided += int((r.need & ~r.counted).sum())
        if share:
            t = table(O, batch, groups, n_rows, tail, col_base, end_state=es, skip=done, cap=cap)
            batch.obs_pose[...], batch.final_time_step[...] = t.pose, t.fts
        for b in range(B):
            f = int(batch.frame_of[b])
            nx = int(batch.nx[f])
            a = AR.advance(O, tick_t=batch.tick_t, veh_l=batch.veh_l, knots=batch.knots[f, :nx], coef=batch.coef[f][:, :nx], ego=ego[b], t_now=t_now[b],
                           cycles=ncyc[b], done=done[b], end_state=es[b], goal_xy=goal_xy[b])
            ego[b], t_now[b], ncyc[b], done[b] = a.ego, a.t_now, a.cycles, a.done
            if a.moved:
                states[k + 1, b] = a.ego
                carts[k, b] = a.cart
        overlap[k] = footprints_overlap(O, batch, carts[k], pairs)
    return SimpleNamespace(states=states, cart=carts, done=done, cycles=ncyc, overlap=overlap, undecided=undecided)
