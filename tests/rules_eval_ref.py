"""Independent restatement of fp_rules_eval (the four road rules on explicit end states), numpy + the CPU oracle only.

For one trajectory of one ego - an end state (d, v, T) - the series come from the ORACLE (prob.eval_traj(d, v, T, dump=True), as
margins_ref.plan_margin obtains them) and the four definitions of include/frenet_gpu.h are restated point by point, in the order the
passes run, by calling the sibling references' helpers where they exist:

    envelope    envelope_ref._segment / line_curvature: s_d > lim + tol at s + front (RULE_LIMIT, FLAG_SPEED); s_d^2 |kappa_r| >
                max_lat_accel (RULE_LATERAL, FLAG_ACCEL)
    gates       gates_ref.waived_gates: q_{i-1} <= gate_s < q_i of a gate that is not waived and closed at step t_now + i (RULE_GATE,
                FLAG_SPEED)
    boundary    boundary_ref._point_terms: d + h + margin > L or d - h - margin < R (RULE_BOUNDARY; FLAG_BOUNDARY written, set or cleared)
    gaps        gaps_ref.pose_set / box_gap / sat_gap: only when the word carries no infeasible bit after the three rules above; the
                collision predicates with the two time indices apart (RULE_GAP, FLAG_COLLISION)

N and M are taken from the flag word given (by default the oracle's own word of the end state).  A NaN in the end state or M <= 1:
nothing is checked.  Like its siblings it returns per trajectory the SLACK - the smallest distance of any deciding comparison from its
threshold, with each sibling's own terms - and marks a trajectory undecided when that is below UNDECIDED_TOL: another rounding of the
same numbers may decide it either way.  A trajectory the gaps did not evaluate BECAUSE an earlier rule flagged it carries that rule's
slack: if the earlier verdict is undecided, so is everything behind it.

Nothing here calls the library under test."""
from types import SimpleNamespace

import numpy as np

import boundary_ref as BR
import envelope_ref as ER
import gaps_ref as PR
import gates_ref as GR

FLAG_SPEED, FLAG_ACCEL, FLAG_COLLISION, FLAG_BOUNDARY = 1, 2, 4, 128
FLAG_INFEASIBLE = 1 | 2 | 4 | 16 | 32 | 64 | 128
RULE_LIMIT, RULE_LATERAL, RULE_GATE, RULE_BOUNDARY, RULE_GAP = 1, 2, 4, 8, 16
RULE_NAMES = ("envelope", "gates", "boundary", "gaps")  # the order the rules run in (rules.TABLE)
UNDECIDED_TOL = 1e-9        # FP_AUDIT_GAP_TOL (include/frenet_gpu.h): the siblings' tolerance
MAX_UNDECIDED_SHARE = 0.005  # of the trajectories of a test batch: the siblings' cap
MAX_EXCLUDED_EGOS = 1        # per test batch: the siblings' cap
S, S_D, D, D_D, X, Y, YAW = 1, 2, 5, 6, 9, 10, 11  # rows of a [16, stride] dump (FP_ARR_*)
SEED = 33055                 # the siblings' seed


def carried(batch):
    """The rules the batch carries data for, restated (rules.TABLE's `carried` column)."""
    out = []
    if getattr(batch, "speed_limit", None) is not None or float(getattr(batch, "max_lat_accel", 0.0) or 0.0) > 0.0:
        out.append("envelope")
    if getattr(batch, "gate_s", None) is not None:
        out.append("gates")
    if getattr(batch, "bound_left", None) is not None:
        out.append("boundary")
    if int(getattr(batch, "gap_follow", 0) or 0) > 0 or int(getattr(batch, "gap_lead", 0) or 0) > 0:
        out.append("gaps")
    return tuple(out)


def _envelope(batch, b, arr, M):
    """-> (bit_a, bit_b, slack) of one series: envelope_ref.ego_envelope's body."""
    f = int(batch.frame_of[b])
    nx = int(batch.nx[f])
    knots, coef = batch.knots[f, :nx], batch.coef[f][:, :nx]
    lim_seg = (np.full(nx, np.inf) if batch.speed_limit is None else batch.speed_limit[f, :nx])[: nx - 1]
    front, tol, max_lat = float(batch.limit_front), float(batch.limit_tol), float(batch.max_lat_accel)
    s, s_d = arr[S, 1:M], arr[S_D, 1:M]
    s_q = s + front
    kq = ER._segment(knots, s_q)
    lim = lim_seg[kq]
    viol = s_d > lim + tol
    gaps = [np.abs(s_d - lim - tol)[np.isfinite(lim)]]
    lo = kq > 0
    other = s_d[lo] > lim_seg[kq[lo] - 1] + tol
    gaps.append(np.abs(s_q[lo] - knots[kq[lo]])[other != viol[lo]])
    hi = kq < nx - 2
    other = s_d[hi] > lim_seg[kq[hi] + 1] + tol
    gaps.append(np.abs(s_q[hi] - knots[kq[hi] + 1])[other != viol[hi]])
    bit_b = False
    if max_lat > 0.0:
        a_lat = s_d * s_d * np.abs(ER.line_curvature(knots, coef, s))
        bit_b = bool((a_lat > max_lat).any())
        gaps.append(np.abs(a_lat - max_lat))
    gaps = np.concatenate(gaps)
    return bool(viol.any()), bit_b, float(gaps.min()) if gaps.size else np.inf


def _gates(batch, b, arr, M):
    """-> (gated, slack) of one series: gates_ref.ego_gates' body."""
    f = int(batch.frame_of[b])
    line, words = batch.gate_s[f], batch.gate_closed[f]
    T_gate, t_now, front = len(words), int(batch.t_now[b]), float(batch.gate_front)
    waived, waiver_gap = GR.waived_gates(batch, b)
    used = np.nonzero(~np.isnan(line))[0]
    slack = float(waiver_gap.min()) if len(used) else np.inf
    q = np.concatenate(([batch.ego[b, 0] + front], arr[S, 1:M] + front))
    gated = False
    for i in range(1, M):
        w = int(words[min(max(t_now + i, 0), T_gate - 1)])
        for g in used:
            slack = min(slack, abs(q[i] - line[g]))
            if q[i - 1] <= line[g] < q[i] and not waived[g] and (w >> int(g)) & 1:
                gated = True
    return gated, slack


def _boundary(batch, b, arr, M):
    """-> (bit, slack) of one series: boundary_ref.ego_mask's body."""
    f = int(batch.frame_of[b])
    nx = int(batch.nx[f])
    knots, left, right = batch.knots[f, :nx], batch.bound_left[f, :nx], batch.bound_right[f, :nx]
    margin = float(batch.bound_margin)
    up, dn, L, R = BR._point_terms(knots, left, right, batch.veh_l, batch.veh_w, arr[S, 1:M], arr[S_D, 1:M], arr[D, 1:M], arr[D_D, 1:M])
    bit = bool(np.any(up + margin > L) | np.any(dn - margin < R))
    gaps = np.concatenate([np.abs(L - (up + margin))[np.isfinite(L)], np.abs((dn - margin) - R)[np.isfinite(R)]])
    return bit, float(gaps.min()) if gaps.size else np.inf


def _gaps(O, batch, b, arr, M):
    """-> (close, slack) of one series: gaps_ref.ego_gaps' body for one survivor."""
    follow, lead, first = int(batch.gap_follow), int(batch.gap_lead), int(batch.gap_first)
    sc, t_now, cs = int(batch.scene_of[b]), int(batch.t_now[b]), int(batch.check_stride)
    if not (sc >= 0 and batch.n_obs > 0 and (follow > 0 or lead > 0)):
        return False, np.inf
    pose, dims = batch.obs_pose[sc], batch.obs_dims[sc]
    nvert = None if getattr(batch, "obs_nvert", None) is None else batch.obs_nvert[sc]
    horizon = int(batch.final_time_step[sc]) - t_now
    r_e = 0.5 * np.hypot(batch.veh_l, batch.veh_w)
    r_o = 0.5 * np.hypot(dims[:, 0], dims[:, 1])
    P = PR.pose_set(M, horizon, t_now, batch.T_obs, cs)
    A = P[P >= first]
    if not len(A):
        return False, np.inf
    lag = A[:, None] - P[None, :]
    pair = ((lag > 0) & (lag <= follow)) | ((lag < 0) & (-lag <= lead))
    rows = pose[P + t_now]
    ex, ey, eyaw = arr[X, A], arr[Y, A], arr[YAW, A]
    dist = np.hypot(rows[None, :, :, 0] - ex[:, None, None], rows[None, :, :, 1] - ey[:, None, None])
    near = pair[:, :, None] & (rows[None, :, :, 3] != 0.0) & (dist <= r_e + r_o[None, None, :] + PR.NEAR)
    ia, ir, ij = np.nonzero(near)
    if not len(ia):
        return False, np.inf
    ego_box = np.column_stack([np.full(len(ia), batch.veh_l), np.full(len(ia), batch.veh_w), ex[ia], ey[ia], eyaw[ia]])
    obs_box = np.column_stack([dims[ij, 0], dims[ij, 1], rows[ir, ij, 0], rows[ir, ij, 1], rows[ir, ij, 2]])
    is_poly = np.zeros(len(ia), dtype=bool) if nvert is None else nvert[ij] > 0
    hit = np.zeros(len(ia), dtype=bool)
    slack = np.inf
    if (~is_poly).any():
        hit[~is_poly] = O.boxes_intersect_batch(ego_box[~is_poly], obs_box[~is_poly]) > 0
        slack = min(slack, float(np.abs(PR.box_gap(ego_box[~is_poly], obs_box[~is_poly])).min()))
    for k in np.nonzero(is_poly)[0]:
        j = ij[k]
        res, world = O.box_ring_intersect(ego_box[k], batch.obs_poly[sc, j, :nvert[j]], obs_box[k, 2:5], world=True)
        hit[k] = bool(res)
        slack = min(slack, abs(PR.sat_gap(PR._corners(*ego_box[k]), world)))
    return bool(hit.any()), slack


def _problem(O, batch, b):
    # (the oracle's series do not depend on t_now; a negative one is the gates' business alone: gates_ref.ego_gates does the same)
    import dataclasses

    return O.problems_from_batch(dataclasses.replace(batch, t_now=np.maximum(batch.t_now, 0)), egos=[b])[0]


def traj_rules(O, batch, b, prob, end_state, word_in=None, names=None):
    """One trajectory of ego b -> SimpleNamespace(word_in, word (the flag word the call leaves), rule_bits, slack, undecided, N, M)."""
    names = carried(batch) if names is None else tuple(n for n in RULE_NAMES if n in names)
    d, v, T = (float(x) for x in end_state)
    if not (d == d and v == v and T == T):
        w = 0 if word_in is None else int(word_in)
        return SimpleNamespace(word_in=w, word=w, rule_bits=0, slack=np.inf, undecided=False, N=0, M=0)
    r = prob.eval_traj(d, v, T, dump=True, stride=256)
    w_in = (int(r.flags) & 0xFF) | (r.N << 8) | (r.M << 20) if word_in is None else int(word_in)  # (fp_eval_trajs' word: the bits, N, M)
    M = w_in >> 20
    assert M == r.M and (w_in >> 8) & 0xFFF == r.N, (b, end_state, hex(w_in), r.N, r.M)
    out = SimpleNamespace(word_in=w_in, word=w_in, rule_bits=0, slack=np.inf, undecided=False, N=r.N, M=M)
    if M <= 1:
        return out
    word, bits, slack = w_in, 0, np.inf
    if "envelope" in names:
        a, lat, sl = _envelope(batch, b, r.arrays, M)
        word |= (FLAG_SPEED if a else 0) | (FLAG_ACCEL if lat else 0)
        bits |= (RULE_LIMIT if a else 0) | (RULE_LATERAL if lat else 0)
        slack = min(slack, sl)
    if "gates" in names:
        g, sl = _gates(batch, b, r.arrays, M)
        word |= FLAG_SPEED if g else 0
        bits |= RULE_GATE if g else 0
        slack = min(slack, sl)
    if "boundary" in names:
        bd, sl = _boundary(batch, b, r.arrays, M)
        word = (word & ~FLAG_BOUNDARY) | (FLAG_BOUNDARY if bd else 0)
        bits |= RULE_BOUNDARY if bd else 0
        slack = min(slack, sl)
    if "gaps" in names and not (word & FLAG_INFEASIBLE):
        c, sl = _gaps(O, batch, b, r.arrays, M)
        word |= FLAG_COLLISION if c else 0
        bits |= RULE_GAP if c else 0
        slack = min(slack, sl)
    out.word, out.rule_bits, out.slack, out.undecided = word, bits, slack, bool(slack < UNDECIDED_TOL)
    return out


def batch_rules(O, batch, end_states, flags=None, names=None, skip=None):
    """The call on end_states [B, K, 3] (flags [B, K] or None: the oracle's own words) -> SimpleNamespace(flags_in, flags, rule_bits
    [B, K], counts [B, 5], slack, undecided [B, K]).  skip [B]: egos that are not evaluated (their words stay, rule_bits 0)."""
    es = np.asarray(end_states, dtype=np.float64)
    B, K = es.shape[:2]
    fin, fout = np.zeros((B, K), dtype=np.uint32), np.zeros((B, K), dtype=np.uint32)
    bits = np.zeros((B, K), dtype=np.uint32)
    slack, und = np.full((B, K), np.inf), np.zeros((B, K), dtype=bool)
    counts = np.zeros((B, 5), dtype=np.int32)
    for b in range(B):
        if skip is not None and skip[b]:
            if flags is not None:
                fin[b] = fout[b] = flags[b]
            continue
        prob = _problem(O, batch, b)
        for k in range(K):
            t = traj_rules(O, batch, b, prob, es[b, k], None if flags is None else flags[b, k], names)
            fin[b, k], fout[b, k], bits[b, k], slack[b, k], und[b, k] = t.word_in, t.word, t.rule_bits, t.slack, t.undecided
            for i in range(5):
                counts[b, i] += (t.rule_bits >> i) & 1
    return SimpleNamespace(flags_in=fin, flags=fout, rule_bits=bits, counts=counts, slack=slack, undecided=und)


def check_caps(ref, what=""):
    """The siblings' caps: at most 0.5 % of the batch's trajectories undecided, at most one ego excluded for having one."""
    und, egos = int(ref.undecided.sum()), int(ref.undecided.any(axis=1).sum())
    assert und <= MAX_UNDECIDED_SHARE * ref.undecided.size, (what, und, ref.undecided.size)
    assert egos <= MAX_EXCLUDED_EGOS, (what, egos)
    return und, egos


def lattice_end_states(batch):
    """[B, C, 3]: the end states of the lattice's candidates in flat FOP order ((i_d * nt + i_t) * nv + i_v)."""
    c = np.arange(batch.C)
    iv, it, i_d = c % batch.nv, (c // batch.nv) % batch.nt, c // (batch.nv * batch.nt)
    es = np.empty((batch.B, batch.C, 3))
    es[:, :, 0] = np.asarray(batch.d_samples)[i_d][None, :]
    es[:, :, 1] = np.asarray(batch.v_samples)[:, iv]
    es[:, :, 2] = np.asarray(batch.t_samples)[it][None, :]
    return es


# ---------------------------------------------------------------------------
# the off-lattice inputs (shared by tests/test_rules_eval_cpu.py, which checks the caps on the reference alone, and
# tests/test_gpu_rules_eval.py)
# ---------------------------------------------------------------------------
OFF_K = 7          # end states per ego
OFF_SKIP = 2       # the ego that is skipped
OFF_NAN = (0, 3)   # (ego, trajectory) whose end state is NaN
OFF_SHORT = (1, 5)  # (ego, trajectory) whose T is shorter than two ticks


def all_rules_batch(seed=SEED):
    """The siblings' B = 5, 5 x 4 x 3 shape with 12 moving obstacles (gaps_ref.moving_batch) carrying all four rules: the envelope's
    wavy limit and lateral bound, the gates' two lights per frame, the widened wavy corridor, the time gap 20 / 10 / 2.  The FISS
    sampling box of the batch is its lattice's own range."""
    import dataclasses

    b = PR.moving_batch(seed=seed)
    b = GR.with_gates(ER.with_profile(b, max_lat_accel=ER.MAX_LAT_ACCEL))
    dl, dr = BR.wavy_corridor(b.knots)
    return dataclasses.replace(PR.with_gap(b), bound_left=dl + BR.WIDEN, bound_right=dr - BR.WIDEN, bound_margin=0.05)


def off_lattice(batch, seed=SEED, K=OFF_K):
    """[B, K, 3] random end states inside the batch's sampling box samp_min .. samp_max, T off the tick grid; one T below two ticks, one
    NaN end state."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(batch.samp_min)[:, None, :], np.asarray(batch.samp_max)[:, None, :]
    es = lo + (hi - lo) * rng.random((batch.B, K, 3))
    # (a random T is off the tick grid with probability 1; tests/test_rules_eval_cpu.py asserts it for the seed)
    es[OFF_SHORT[0], OFF_SHORT[1], 2] = 1.6 * batch.tick_t
    es[OFF_NAN[0], OFF_NAN[1], 0] = np.nan
    return es


def off_skip(batch):
    s = np.zeros(batch.B, dtype=np.int32)
    s[OFF_SKIP] = 1
    return s
