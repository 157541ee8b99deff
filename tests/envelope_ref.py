"""Independent restatement of the speed envelope (fp_speed_envelope), numpy + the CPU oracle only.

For one ego of a ProblemBatch everything about a candidate comes from the ORACLE - its flag word, its cost (dense_tables), its dumped
S / S_D series and N / M (eval_traj) - and the check is restated from its definition (include/frenet_gpu.h), point by point:

    points      i = 1 .. M-1 (M <= 1: nothing is checked, no bit)
    limit       s_q = s + front;  k_q = searchsorted(knots, s_q, 'right') - 1 clamped to [0, nx-2];  lim = speed_limit[f, k_q]
    violation A s_d > lim + tol (never for lim = +inf)
    lateral     (max_lat_accel > 0)  k = searchsorted(knots, s, 'right') - 1 clamped to [0, nx-2], dx = s - knots[k],
                x' = bx + 2 cx dx + 3 dx_ dx^2, x'' = 2 cx + 6 dx_ dx (y likewise), kappa_r = (x' y'' - y' x'') / (x'^2 + y'^2)^1.5
    violation B s_d^2 |kappa_r| > max_lat_accel
    bits        A ORs FLAG_SPEED, B ORs FLAG_ACCEL into the flag word; nothing is ever cleared, no other bit touched
    winner      minimum cost over candidates without an infeasible bit and a non-NaN cost, the LAST one in FOP index order on exact ties

Per candidate it also returns the SLACK, the smallest of
    |s_d - lim - tol|                 over the checked points with a finite limit,
    |s_d^2 |kappa_r| - max_lat_accel| over all checked points when the lateral check is on,
    |s_q - knot|                      for either end knot of segment k_q, when the neighbouring segment's limit would give the other
                                      verdict at that point.
The kernel evaluates the series by fma Horner, the oracle point by point: a candidate with slack < UNDECIDED_TOL (the project's
FP_AUDIT_GAP_TOL) may be decided either way and is excluded from exact comparisons; the tests cap how many there may be.

Nothing here calls the library under test."""
import dataclasses
from types import SimpleNamespace

import numpy as np

import rule_ref_common as common
from rule_ref_common import argmin, plain_batch  # noqa: F401  (the tests reach plain_batch through this module too)

FLAG_SPEED, FLAG_ACCEL, FLAG_BOUNDARY = 1, 2, 128
FLAG_INFEASIBLE = 1 | 2 | 4 | 16 | 32 | 64 | FLAG_BOUNDARY  # FP_FLAG_CONSTRAINTS | FP_FLAG_COLLISION | FP_FLAG_BOUNDARY
UNDECIDED_TOL = 1e-9                                         # FP_AUDIT_GAP_TOL (include/frenet_gpu.h)
MAX_UNDECIDED_SHARE = 0.005                                  # of the candidates of a test batch
MAX_EXCLUDED_EGOS = 1                                        # per test batch
S, S_D = 1, 2                                                # rows of a [16, stride] dump (FP_ARR_*)

# Chosen on the CPU, on this reference alone (tests/test_envelope_cpu.py asserts what they were chosen for):
SEED = 33055          # the seed of every test batch (the boundary check's batches use the same one)
TOL = 0.05            # m/s
# m/s^2: the synthetic lines could bend by up to ~0.009 1/m (1.6 m/s^2 at 13.5 m/s), the five lines of SEED bend far less where their egos
# drive: on the reference, 0.3 binds for 5 % of the base batch's candidates, 0.2 for 10 %, 0.1 for 30 %, 0.05 for 47 %
MAX_LAT_ACCEL = 0.10
STOP_AHEAD = 50.0     # m: the stop case's zero stretch starts at the first knot at least this far ahead of each ego


def wavy_limit(knots):
    """The limit of the test batches: 8.5 + 3.5 sin(knots / 31) m/s (5 .. 12), a smooth function of the knot position; padding stays +inf."""
    k = np.asarray(knots, dtype=np.float64)
    return np.where(np.isfinite(k), 8.5 + 3.5 * np.sin(np.where(np.isfinite(k), k, 0.0) / 31.0), np.inf)


def with_profile(batch, limit="wavy", front=None, tol=TOL, max_lat_accel=0.0, **kw):
    """A copy of `batch` that carries a speed profile.  limit: "wavy" (wavy_limit), None (+inf everywhere) or an [F, NX] array;
    front None = veh_l / 2; kw overrides any other ProblemBatch field."""
    knots = np.asarray(kw.get("knots", batch.knots))
    if limit is None:
        lim = np.full(knots.shape, np.inf)
    elif isinstance(limit, str):
        lim = wavy_limit(knots)
    else:
        lim = np.broadcast_to(np.asarray(limit, dtype=np.float64), knots.shape).copy()
    return dataclasses.replace(batch, speed_limit=lim, limit_front=0.5 * batch.veh_l if front is None else front, limit_tol=tol,
                               max_lat_accel=max_lat_accel, **kw)


def _segment(knots, s):
    return np.clip(np.searchsorted(knots, s, "right") - 1, 0, len(knots) - 2)


def line_curvature(knots, coef, s):
    """kappa_r of the definition at the arclengths s (coef [8, nx]: a, b, c, d of x, then of y)."""
    k = _segment(knots, s)
    dx = s - knots[k]
    x1 = coef[1, k] + 2.0 * coef[2, k] * dx + 3.0 * coef[3, k] * dx * dx
    y1 = coef[5, k] + 2.0 * coef[6, k] * dx + 3.0 * coef[7, k] * dx * dx
    x2 = 2.0 * coef[2, k] + 6.0 * coef[3, k] * dx
    y2 = 2.0 * coef[6, k] + 6.0 * coef[7, k] * dx
    return (x1 * y2 - y1 * x2) / (x1 * x1 + y1 * y1) ** 1.5


def ego_envelope(O, batch, b, tables=None):
    """The check for ego b of a batch that carries a speed profile.  tables = (cost [C], flags [C]) to mask (default: the oracle's dense
    tables).  Returns a namespace: cost [C], flags_in [C], flags [C] (bits ORed in), bit_a [C], bit_b [C], limited [C], slack [C],
    undecided [C], M [C], N [C], best_idx, best_cost (the masked winner), best_in (the winner of flags_in), n_limited."""
    prob = O.problems_from_batch(batch, egos=[b])[0]
    cost, flags_in = prob.dense_tables() if tables is None else (np.asarray(tables[0], dtype=np.float64), np.asarray(tables[1], dtype=np.uint32))
    f = int(batch.frame_of[b])
    nx = int(batch.nx[f])
    knots, coef = batch.knots[f, :nx], batch.coef[f][:, :nx]
    lim_seg = (np.full(nx, np.inf) if batch.speed_limit is None else batch.speed_limit[f, :nx])[: nx - 1]
    front, tol, max_lat = float(batch.limit_front), float(batch.limit_tol), float(batch.max_lat_accel)
    Cn, nv, nt = batch.C, batch.nv, batch.nt
    bit_a, bit_b = np.zeros(Cn, dtype=bool), np.zeros(Cn, dtype=bool)
    slack = np.full(Cn, np.inf)
    Ms, Ns = np.zeros(Cn, dtype=np.int64), np.zeros(Cn, dtype=np.int64)
    for c in range(Cn):
        iv, it, i_d = c % nv, (c // nv) % nt, c // (nv * nt)
        r = prob.eval_traj(float(batch.d_samples[i_d]), float(batch.v_samples[b, iv]), float(batch.t_samples[it]), dump=True, stride=256)
        N, M = r.N, r.M
        assert N == (int(flags_in[c]) >> 8) & 0xFFF and M == int(flags_in[c]) >> 20, (b, c, N, M, hex(int(flags_in[c])))
        Ns[c], Ms[c] = N, M
        if M <= 1:
            continue
        s, s_d = r.arrays[S, 1:M], r.arrays[S_D, 1:M]
        s_q = s + front
        kq = _segment(knots, s_q)
        lim = lim_seg[kq]
        viol = s_d > lim + tol
        bit_a[c] = bool(viol.any())
        gaps = [np.abs(s_d - lim - tol)[np.isfinite(lim)]]
        lo = kq > 0                # the segment below would decide otherwise: how far s_q is from the knot between them
        other = s_d[lo] > lim_seg[kq[lo] - 1] + tol
        gaps.append(np.abs(s_q[lo] - knots[kq[lo]])[other != viol[lo]])
        hi = kq < nx - 2
        other = s_d[hi] > lim_seg[kq[hi] + 1] + tol
        gaps.append(np.abs(s_q[hi] - knots[kq[hi] + 1])[other != viol[hi]])
        if max_lat > 0.0:
            a_lat = s_d * s_d * np.abs(line_curvature(knots, coef, s))
            bit_b[c] = bool((a_lat > max_lat).any())
            gaps.append(np.abs(a_lat - max_lat))
        gaps = np.concatenate(gaps)
        slack[c] = gaps.min() if gaps.size else np.inf
    flags = flags_in | np.where(bit_a, FLAG_SPEED, 0).astype(np.uint32) | np.where(bit_b, FLAG_ACCEL, 0).astype(np.uint32)
    return SimpleNamespace(cost=cost, flags_in=flags_in, flags=flags, bit_a=bit_a, bit_b=bit_b, limited=bit_a | bit_b, slack=slack,
                           undecided=slack < UNDECIDED_TOL, M=Ms, N=Ns, best_idx=argmin(cost, flags)[0], best_cost=argmin(cost, flags)[1],
                           best_in=argmin(cost, flags_in)[0], n_limited=int((bit_a | bit_b).sum()))


def batch_envelope(O, batch, tables=None, egos=None):
    """ego_envelope for the egos asked for (all by default) -> list; tables = (cost [B, C], flags [B, C]) or None."""
    egos = range(batch.B) if egos is None else egos
    return [ego_envelope(O, batch, b, None if tables is None else (tables[0][b], tables[1][b])) for b in egos]


def check_caps(refs, what=""):
    """The caps the tests rely on: at most 0.5 % of the batch's candidates undecided, at most one ego excluded for having one."""
    return common.check_caps(refs, MAX_UNDECIDED_SHARE, MAX_EXCLUDED_EGOS, what)


def limited_share(refs):
    return sum(r.n_limited for r in refs) / sum(len(r.slack) for r in refs)


# ---------------------------------------------------------------------------
# the test batches (shared by tests/test_envelope_cpu.py, which checks caps and shares on the reference alone, and
# tests/test_gpu_envelope.py)
# ---------------------------------------------------------------------------
def stop_limit(batch, ahead=STOP_AHEAD):
    """+inf, except 0 on every segment from the first knot at least `ahead` metres in front of each ego's s onward -> ([F, NX] limits,
    [B] the arclength where each ego's zero stretch starts).  One frame per ego (synth.make_batch)."""
    lim = np.full(batch.knots.shape, np.inf)
    start = np.zeros(batch.B)
    for b in range(batch.B):
        f = int(batch.frame_of[b])
        k = int(np.searchsorted(batch.knots[f, : batch.nx[f]], batch.ego[b, 0] + ahead, "left"))
        lim[f, k:] = 0.0
        start[b] = batch.knots[f, k]
    return lim, start


def _stop():
    b = plain_batch()
    return with_profile(b, limit=stop_limit(b)[0])


def stop_egos(O):
    """The egos of the stop case whose unmasked winner runs the red light while a masked winner exists."""
    _, refs = case(O, "stop")
    return [b for b, r in enumerate(refs) if r.best_in >= 0 and r.bit_a[r.best_in] and r.best_idx >= 0]


CASES = {
    "base": lambda: with_profile(plain_batch()),                                              # a wavy limit, lateral off
    "lat": lambda: with_profile(plain_batch(), limit=None, max_lat_accel=MAX_LAT_ACCEL),      # no limits, lateral on
    "both": lambda: with_profile(plain_batch(), max_lat_accel=MAX_LAT_ACCEL),                 # limits and lateral together
    "stop": _stop,                                                                            # a red light ~50 m ahead of every ego
    "tick005": lambda: with_profile(plain_batch(), max_lat_accel=MAX_LAT_ACCEL, tick_t=0.05),  # N up to 200 (needs points_max): four lane rounds
    "line_ends": lambda: common._line_ends(plain_batch(), lambda b, ego: with_profile(b, max_lat_accel=MAX_LAT_ACCEL, ego=ego)),  # M < N and M <= 1
    "chunks": lambda: with_profile(plain_batch(2, 9, 9, 7), max_lat_accel=MAX_LAT_ACCEL),     # C = 567: three chunks of the row pass, 63 profiles
    "unlimited": lambda: with_profile(plain_batch(), limit=None),                             # all +inf, lateral off: nothing may change
}
_cache = {}


def case(O, name):
    """(batch, refs) of a named test batch; the reference is computed once per process and shared (do not modify it)."""
    if name not in _cache:
        batch = CASES[name]()
        _cache[name] = (batch, batch_envelope(O, batch))
    return _cache[name]
