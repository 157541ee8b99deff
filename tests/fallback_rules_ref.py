"""Independent restatement of fp_fallback_stop_rules (the stopping manoeuvre that obeys the road rules), numpy + the CPU oracle only.

The definition (include/frenet_gpu.h) is fp_fallback_stop's with one more key, and so is this file: need(b), the family, admissibility
and the first contact are fallback_ref's pieces (candidate, first_contact), called as they stand; the verdict of an admissible candidate
without contact is rules_eval_ref.traj_rules on the end state (d, 0, T) with a flag word that carries the series' N and M and no flag
bit; the choice is a plain loop over the key

    (contact, violates, popcount(verdict) if violating, -i_T (clean) | i_T (violating) | (-hit_step, i_T) (contact), |d_end - d0|, i_d)

It carries over both siblings' stability reporting: the admissibility slack and the contact under obstacles grown and shrunk
(fallback_ref), and a rule verdict within UNDECIDED_TOL of its threshold (rules_eval_ref).  An ego with any such candidate is left out of
a comparison as a whole (`counted`); at most MAX_LEFT_OUT egos per fixture.

Nothing here calls the library under test."""
from types import SimpleNamespace

import numpy as np

import fallback_ref as FR
import rules_eval_ref as RR

NOT_NEEDED, CLEAR, CONTACT, NONE = FR.NOT_NEEDED, FR.CLEAR, FR.CONTACT, FR.NONE
UNDECIDED_TOL = RR.UNDECIDED_TOL  # 1e-9: a rule verdict closer than this to its threshold is not compared
MAX_LEFT_OUT = 1                  # egos per fixture the reference may leave out (a condition, not a measurement)
RULE_COUNT = 5


def popcount(x):
    return bin(int(x)).count("1")


def verdict(O, batch, b, prob, d_end, T, cand, obey):
    """The rule verdict of one admissible, clear candidate -> (rule_bits, slack).  The word on entry carries N and M alone."""
    t = RR.traj_rules(O, batch, b, prob, (d_end, 0.0, T), word_in=(cand.N << 8) | (cand.M << 20), names=obey)
    return int(t.rule_bits), float(t.slack)


def choose(cands, verdicts, d_ends, d0, n_stop):
    """The winner's f among the admissible candidates (None: none) by the definition's order, as a plain loop over the key."""
    best, best_key = None, None
    for f, c in enumerate(cands):
        if not c.adm:
            continue
        i_d, i_T = divmod(f, n_stop)
        if c.hit_step >= 0:
            key = (1, 0, 0, -c.hit_step, i_T)
        elif verdicts[f]:
            key = (0, 1, popcount(verdicts[f]), i_T, 0)
        else:
            key = (0, 0, 0, -i_T, 0)
        key = key + (abs(d_ends[i_d] - d0), i_d)
        if best is None or key < best_key:
            best, best_key = f, key
    return best


def fallback_rules(O, batch, stop_T, d_targets=None, max_decel=np.inf, obey=None, best_idx=None, end_state=None, skip=None, cap=None):
    """The call's outputs for every ego (fallback_ref.fallback's namespace plus rule_bits [B], cand_rules [B, F], rule_counts [B, 5],
    rule_slack [B, F]); `counted` [B] False: the ego is left out of a comparison.  obey: rule names (None: every rule the batch carries)."""
    assert (best_idx is None) != (end_state is None)
    obey = RR.carried(batch) if obey is None else tuple(n for n in RR.RULE_NAMES if n in obey)
    assert obey and all(n in RR.carried(batch) for n in obey), obey
    stop_T = np.asarray(stop_T, dtype=np.float64)
    d_targets = np.concatenate([[np.nan], batch.d_samples]) if d_targets is None else np.asarray(d_targets, dtype=np.float64)
    n_d, n_stop = len(d_targets), len(stop_T)
    F, B = n_d * n_stop, batch.B
    assert 1 <= F <= FR.MAX_FALLBACK
    cap = FR.points_cap(batch, stop_T) if cap is None else cap
    es = np.full((B, 3), np.nan) if best_idx is not None else np.array(end_state, dtype=np.float64).reshape(B, 3)
    res = SimpleNamespace(end_state=es, status=np.zeros(B, dtype=np.int32), fb_idx=np.full(B, -1, dtype=np.int32), hit_step=np.full(B, -1, dtype=np.int32),
                          hit_obs=np.full(B, -1, dtype=np.int32), hit_speed=np.full(B, np.nan), cand=np.full((B, F), -3, dtype=np.int32),
                          counted=np.ones(B, dtype=bool), slack=np.full((B, F), np.inf), stable=np.ones((B, F), dtype=bool), need=np.zeros(B, dtype=bool),
                          counts=np.zeros((B, 4), dtype=np.int32), N=np.zeros((B, F), dtype=np.int32), M=np.zeros((B, F), dtype=np.int32),
                          rule_bits=np.zeros(B, dtype=np.uint32), cand_rules=np.zeros((B, F), dtype=np.uint32), rule_counts=np.zeros((B, RULE_COUNT), dtype=np.int32),
                          rule_slack=np.full((B, F), np.inf), obey=obey)
    for b in range(B):
        skipped = skip is not None and bool(skip[b])
        need = not skipped and (int(best_idx[b]) < 0 if best_idx is not None else bool(np.isnan(es[b, 0])))
        res.need[b] = need
        if not need:
            if best_idx is not None and not skipped:
                es[b] = FR.decode(batch, b, int(best_idx[b]))
            res.counts[b, NOT_NEEDED] += 1
            continue
        prob = O.problems_from_batch(batch, egos=[b])[0]
        d0 = float(batch.ego[b, 3])
        d_ends = [d0 if np.isnan(d) else float(d) for d in d_targets]
        cands = [FR.candidate(O, batch, prob, b, d_ends[f // n_stop], float(stop_T[f % n_stop]), max_decel, cap) for f in range(F)]
        verdicts = [0] * F
        for f, c in enumerate(cands):
            if c.adm and c.hit_step < 0:  # (an inadmissible candidate and one with contact: no rule is evaluated)
                verdicts[f], res.rule_slack[b, f] = verdict(O, batch, b, prob, d_ends[f // n_stop], float(stop_T[f % n_stop]), c, obey)
        res.cand[b] = [-2 if not c.adm else c.hit_step for c in cands]
        res.cand_rules[b] = verdicts
        res.slack[b] = [c.slack for c in cands]
        res.stable[b] = [c.stable for c in cands]
        res.N[b], res.M[b] = [c.N for c in cands], [c.M for c in cands]
        res.counted[b] = bool((res.slack[b] > FR.SLACK_MIN).all() and res.stable[b].all() and (res.rule_slack[b] >= UNDECIDED_TOL).all())
        f = choose(cands, verdicts, d_ends, d0, n_stop)
        if f is None:
            res.status[b] = NONE
            es[b] = np.nan
        else:
            c = cands[f]
            res.status[b] = CLEAR if c.hit_step < 0 else CONTACT
            res.fb_idx[b], res.hit_step[b], res.hit_obs[b], res.hit_speed[b] = f, c.hit_step, c.hit_obs, c.hit_speed
            res.rule_bits[b] = verdicts[f]
            es[b] = (d_ends[f // n_stop], 0.0, stop_T[f % n_stop])
        res.counts[b, res.status[b]] += 1
        for i in range(RULE_COUNT):
            res.rule_counts[b, i] += (int(res.rule_bits[b]) >> i) & 1
    return res
