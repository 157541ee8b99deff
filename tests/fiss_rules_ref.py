"""Independent restatement of fp_plan_fiss_rules (FISS / FISS+ whose validation sees the road rules): numpy, the CPU oracle, the rules'
reference (tests/rules_eval_ref.py, which stands on the four sibling references) and the host walk of search.py - pinned to the
reference planner by G6 / tests/test_host_search.py - and nothing else of the library under test.

Per ego: the oracle's dense tables; the enforced rules' words of every lattice end state (rules_eval_ref.traj_rules: on the lattice it
is the chain of the four table references, tests/test_rules_eval_cpu.py); bit 128 folded into a constraint bit of a COPY of the flags
(the walk reads nothing but F & CONSTRAINTS and F & COLLISION); search.fiss_search / fissplus_search over search.cost_est_table; then
the refinement rounds with the oracle's costs and search.refine_step, the coarse winner priced by the same evaluator, and the pop loop
by (cost, generation index) while cost <= coarse cost, a feasible candidate's rule bits from traj_rules on its own word.

Beside the result the reference reports the slack of every comparison that decides it: the rules' slack of every masked lattice sample
the walk pops and of every consumed refined candidate, the relative cost gap between successive pops with different end states and
between a pop and the coarse cost.  An ego with a slack below rules_eval_ref.UNDECIDED_TOL (cost gaps: COST_TOL, the project's
FP_AUDIT_COST_TOL) is undecided and left out as a whole; the cap is the siblings' MAX_EXCLUDED_EGOS per batch."""
import dataclasses
from types import SimpleNamespace

import numpy as np

import boundary_ref as BR
import envelope_ref as ER
import gaps_ref as PR
import gates_ref as GR
import rules_eval_ref as R
from fiss_plus_planner_amd import search, synth

COST_TOL = 1e-9  # FP_AUDIT_COST_TOL (include/frenet_gpu.h), relative
CONSTRAINT_BITS = search.FLAG_CONSTRAINTS | R.FLAG_BOUNDARY


def _cost_gap(costs):
    """Smallest relative gap between successive DIFFERENT values of a cost sequence in pop order (inf when there is none)."""
    c = np.asarray([v for v in costs if np.isfinite(v)], dtype=np.float64)
    if len(c) < 2:
        return np.inf
    d = np.abs(np.diff(np.sort(c)))
    rel = d / np.maximum(np.abs(np.sort(c)[1:]), 1e-300)
    rel = rel[d > 0]
    return float(rel.min()) if len(rel) else np.inf


def masked_tables(O, batch, b, prob, names):
    """The oracle's dense tables of ego b with the enforced rules' words -> (cost [C], words [C], slack [C]) in flat FOP order."""
    cost, flags = prob.dense_tables()
    es = R.lattice_end_states(batch)[b]
    words = np.zeros(len(cost), dtype=np.uint32)
    slack = np.full(len(cost), np.inf)
    for c in range(len(cost)):
        t = R.traj_rules(O, batch, b, prob, es[c], None, names)
        assert (t.word_in & 0xFF) == (int(flags[c]) & 0xFF), (b, c)  # the end state IS the candidate
        words[c], slack[c] = t.word, t.slack
    return cost, words, slack


def plan(O, batch, b, kind, names, prev=None, max_refine_iters=3, decaying_factor=0.5, w_heuristic=10.0):
    """fp_plan_fiss_rules for ego b -> SimpleNamespace(best_ijk, end_state, best_cost, refined, stats, rejected, prev_best_idx, slack,
    cost_gap, undecided, popped_boundary_only (a sample whose only bit is 128 was popped before the winner), coarse_ijk_free (the coarse
    winner without rules), trace [n, 4] (the refinement's candidates in generation order: end state, cost))."""
    prob = R._problem(O, batch, b)
    nd, nv, nt = batch.nd, batch.nv, batch.nt
    cost, words, lat_slack = masked_tables(O, batch, b, prob, names)
    folded = np.where(words & np.uint32(R.FLAG_BOUNDARY), words | np.uint32(search.FLAG_SPEED), words) & np.uint32(0xFF)
    J, F = search.tables_to_dvt(cost, folded, nd, nv, nt)
    _, W = search.tables_to_dvt(cost, words & np.uint32(0xFF), nd, nv, nt)
    _, S = search.tables_to_dvt(cost, lat_slack, nd, nv, nt)
    pv = None if prev is None or prev[0] < 0 else np.asarray(prev)
    E = search.cost_est_table(batch.d_samples, batch.v_samples[b], batch.t_samples, batch.samp_min[b], batch.samp_max[b], pv, w_heuristic)
    walk = search.fiss_search if kind == "FISS" else search.fissplus_search
    order = []
    idx, stats = walk(J, F, E, generated_order=order)
    _, F_free = search.tables_to_dvt(cost, prob.dense_tables()[1] & np.uint32(0xFF), nd, nv, nt)
    free_idx, _ = walk(J, F_free, E)
    out = SimpleNamespace(best_ijk=np.full(3, -1, dtype=np.int32), end_state=np.full(3, np.nan), best_cost=np.nan, refined=False,
                          stats=np.array(stats, dtype=np.int32), rejected=0, prev_best_idx=np.full(3, -1, dtype=np.int32) if pv is None else pv.astype(np.int32),
                          slack=np.inf, cost_gap=np.inf, undecided=False, popped_boundary_only=False,
                          coarse_ijk_free=np.full(3, -1) if free_idx is None else np.asarray(free_idx), trace=np.empty((0, 4)))
    # the pops of the cost-ordered validation: every generated sample that is not behind the winner in (cost, raster) order
    gen = [tuple(i) for i in order]
    key = lambda i: (float(J[i]), (i[0] * nv + i[1]) * nt + i[2])  # noqa: E731
    popped = [i for i in gen if np.isfinite(J[i]) and (idx is None or key(i) <= key(tuple(idx)))]
    out.slack = min([float(S[i]) for i in popped], default=np.inf)
    out.cost_gap = _cost_gap([J[i] for i in popped])
    out.popped_boundary_only = any((int(W[i]) & R.FLAG_INFEASIBLE) == R.FLAG_BOUNDARY for i in popped if idx is None or i != tuple(idx))
    if idx is None:
        out.undecided = bool(out.slack < R.UNDECIDED_TOL or out.cost_gap < COST_TOL)
        return out
    idx = tuple(int(v) for v in idx)
    out.best_ijk[:] = out.prev_best_idx[:] = idx
    x = np.array([batch.d_samples[idx[0]], batch.v_samples[b][idx[1]], batch.t_samples[idx[2]]], dtype=np.float64)
    out.end_state, out.best_cost = x.copy(), float(J[idx])
    if kind != "FISS" and max_refine_iters > 0:
        lo, hi = np.asarray(batch.samp_min[b], dtype=np.float64), np.asarray(batch.samp_max[b], dtype=np.float64)
        res = np.array(batch.samp_res[b], dtype=np.float64)
        price = lambda e: prob.eval_traj(float(e[0]), float(e[1]), float(e[2]))  # noqa: E731
        coarse_x, coarse_cost = x.copy(), price(x).cost
        cand = []  # (cost, generation index, end state, the trajectory's own word)
        for _ in range(max_refine_iters):
            probes, x_l, x_r = np.empty((6, 3)), [], []
            for dim in range(3):
                lft, rgt = x.copy(), x.copy()
                lft[dim] -= res[dim]
                rgt[dim] += res[dim]
                lft, rgt = np.clip(lft, lo, hi), np.clip(rgt, lo, hi)
                probes[2 * dim], probes[2 * dim + 1] = lft, rgt
                x_l.append(lft)
                x_r.append(rgt)
            if np.isnan(probes).any():
                break
            ev = [price(p) for p in probes]
            for p, r in zip(probes, ev):
                cand.append((r.cost, len(cand), p.copy(), (int(r.flags) & 0xFF) | (r.N << 8) | (r.M << 20)))
            x_new, res = search.refine_step([r.cost for r in ev[0::2]], [r.cost for r in ev[1::2]], x_l, x_r, x, res, decaying_factor, lo, hi)
            if x_new is None:
                break
            r = price(x_new)
            cand.append((r.cost, len(cand), x_new.copy(), (int(r.flags) & 0xFF) | (r.N << 8) | (r.M << 20)))
            x = x_new
        out.trace = np.array([[*es, c] for c, _, es, _ in cand], dtype=np.float64).reshape(-1, 4)
        validated = checks = 0
        consumed = []
        for c, _, es, word in sorted(cand, key=lambda t: (t[0], t[1])):
            if c > coarse_cost:
                if not np.array_equal(es, coarse_x):
                    out.cost_gap = min(out.cost_gap, abs(c - coarse_cost) / max(abs(coarse_cost), 1e-300))  # the comparison that ended the loop
                break
            validated += 1
            consumed.append((c, es))
            if not np.array_equal(es, coarse_x) and c != coarse_cost:
                out.cost_gap = min(out.cost_gap, abs(c - coarse_cost) / max(abs(coarse_cost), 1e-300))
            if not word & R.FLAG_INFEASIBLE:
                t = R.traj_rules(O, batch, b, prob, es, word, names)
                out.slack = min(out.slack, t.slack)
                out.rejected += bool(t.word & R.FLAG_INFEASIBLE)
                word = t.word
            if word & CONSTRAINT_BITS:
                continue
            checks += 1
            if not word & search.FLAG_COLLISION:
                out.refined, out.end_state, out.best_cost = True, es.copy(), c
                break
        if not out.refined:
            out.best_cost = coarse_cost
        # successive pops with different end states
        for (c0, e0), (c1, e1) in zip(consumed, consumed[1:]):
            if c0 != c1 and not np.array_equal(e0, e1):
                out.cost_gap = min(out.cost_gap, abs(c1 - c0) / max(abs(c1), 1e-300))
        out.stats = out.stats + np.array([0, len(cand), validated, checks], dtype=np.int32)
    out.undecided = bool(out.slack < R.UNDECIDED_TOL or out.cost_gap < COST_TOL)
    return out


_cache = {}


def batch_plan(O, batch, kind, names, prev=None, key=None, **kw):
    """[plan(ego b)] for a whole batch; with `key` the result is computed once per process and shared (do not modify it)."""
    if key is not None and (key, kind, tuple(names)) in _cache:
        return _cache[(key, kind, tuple(names))]
    out = [plan(O, batch, b, kind, names, None if prev is None else prev[b], **kw) for b in range(batch.B)]
    if key is not None:
        _cache[(key, kind, tuple(names))] = out
    return out


def check_caps(refs, what=""):
    egos = sum(r.undecided for r in refs)
    assert egos <= R.MAX_EXCLUDED_EGOS, (what, egos)
    return egos


# ---------------------------------------------------------------------------
# the test batches (shared by tests/test_fiss_rules_cpu.py, which proves on the reference alone that they reach the paths they exist
# for, and tests/test_gpu_fiss_rules.py)
# ---------------------------------------------------------------------------
NAMES = R.RULE_NAMES


def with_rules(b):
    """`b` carrying all four rules: the envelope's wavy limit and lateral bound, two lights per frame, the widened wavy corridor, the time
    gap 20 / 10 / 2 (the data of rules_eval_ref.all_rules_batch, on a FISS lattice)."""
    b = GR.with_gates(ER.with_profile(b, max_lat_accel=ER.MAX_LAT_ACCEL))
    dl, dr = BR.wavy_corridor(b.knots)
    return dataclasses.replace(PR.with_gap(b), bound_left=dl + BR.WIDEN, bound_right=dr - BR.WIDEN, bound_margin=0.05)


def silent(b):
    """`b` carrying a rule set that cannot speak: no limit anywhere, gates that are never closed, a corridor a kilometre wide, and a time
    gap beside obstacles that do not move (a lagged row of a standing obstacle is its row at lag 0: the collision check has spoken)."""
    b = ER.with_profile(b, limit=None)
    G = 2
    b = GR.with_gates(b, closed=np.zeros((b.F, GR.T_GATE, G), dtype=bool))
    wide = np.where(np.isfinite(b.knots), 1.0e3, np.nan)
    return dataclasses.replace(PR.with_gap(b), bound_left=wide, bound_right=-wide, bound_margin=0.0)


_batches = {}


def case(name):
    """The test batches, built once (do not modify).  small: 12 egos x 5 x 5 x 5 (the one-wavefront search, NCH = 2); wide: 3 egos x 9 x 9
    x 7 (C = 567: the four-wavefront search); long: tick_t = 0.05, T up to 7 s = 140 points (NCH = 4)."""
    if name not in _batches:
        if name == "small":
            b = with_rules(synth.make_batch(12, 5, 5, 5, 12, 120, True, 4711, kind="FISS+"))
        elif name == "wide":
            b = with_rules(synth.make_batch(3, 9, 9, 7, 12, 120, True, 4712, kind="FISS+"))
        elif name == "long":
            b = with_rules(dataclasses.replace(synth.make_batch(6, 5, 5, 5, 12, 240, True, 4713, kind="FISS+"), tick_t=0.05))
        elif name == "silent":
            b = silent(synth.make_batch(12, 5, 5, 5, 10, 120, False, 4714, kind="FISS+"))
        elif name == "silent_long":
            b = silent(dataclasses.replace(synth.make_batch(4, 5, 5, 5, 10, 240, False, 4715, kind="FISS+"), tick_t=0.05))
        _batches[name] = b
    return _batches[name]


# (batch, enforced rules, planner): what the GPU test compares with this reference, and the path each exists for
CASES = [("small", NAMES, "FISS+"),                   # all four rules: coarse winners move, egos without a rule-clean sample, bit 128 alone popped
         ("small", ("envelope",), "FISS+"),          # rejected > 0 and the coarse winner stands
         ("small", ("gates", "boundary"), "FISS+"),  # rejected > 0 and a later refined candidate wins
         ("small", NAMES, "FISS"),
         ("long", ("envelope",), "FISS+"),           # 140 points: the refinement's four-points-per-lane instance
         ("wide", ("gates", "boundary"), "FISS+")]    # 567 samples: the four-wavefront search


# ---------------------------------------------------------------------------
# the loop at the red light: gates_ref.loop_batch with the FISS sampling box of its lattice, driven through plan() and advance_ref
# ---------------------------------------------------------------------------
def loop_batch():
    """gates_ref.loop_batch(OPEN_STEPS) - one gate at s = 60, closed before each ego's opening step - with samp_min / samp_max / samp_res
    = the range and spacing of its lattice (the box tests/test_gpu_rules_eval.py gives its audited loop)."""
    b = GR.loop_batch(GR.OPEN_STEPS)
    d, t, v = np.asarray(b.d_samples), np.asarray(b.t_samples), np.asarray(b.v_samples)
    one = np.ones(b.B)
    return dataclasses.replace(b, samp_min=np.column_stack([one * d.min(), v.min(axis=1), one * t.min()]),
                               samp_max=np.column_stack([one * d.max(), v.max(axis=1), one * t.max()]),
                               samp_res=np.column_stack([one * (d[1] - d[0]), v[:, 1] - v[:, 0], one * (t[1] - t[0])]))


def ref_loop(O, batch, b, cycles, kind="FISS+", names=("gates",)):
    """Ego b through `cycles` cycles of [plan() -> hand-over (advance_ref)], prev_best_idx carried along -> list of rows, one per cycle
    driven: t_now (on entry), planned, ego [6] (after the hand-over), done, rejected, undecided, q_before / q_after (the bumper)."""
    import advance_ref

    f = int(batch.frame_of[b])
    nx = int(batch.nx[f])
    ego, t_now, done, n_cycles, prev = batch.ego[b].copy(), int(batch.t_now[b]), 0, 0, None
    rows = []
    for _ in range(cycles):
        if done:
            break
        e2, tn = batch.ego.copy(), batch.t_now.copy()
        e2[b], tn[b] = ego, t_now
        r = plan(O, dataclasses.replace(batch, ego=e2, t_now=tn), b, kind, names, prev)
        a = advance_ref.advance(O, tick_t=batch.tick_t, veh_l=batch.veh_l, knots=batch.knots[f, :nx], coef=batch.coef[f][:, :nx], ego=ego, t_now=t_now,
                                cycles=n_cycles, end_state=r.end_state)
        rows.append(SimpleNamespace(t_now=t_now, planned=bool(r.best_ijk[0] >= 0), ego=a.ego.copy(), done=a.done, rejected=r.rejected, undecided=r.undecided,
                                    q_before=ego[0] + batch.gate_front, q_after=a.ego[0] + batch.gate_front))
        ego, t_now, done, n_cycles, prev = a.ego, a.t_now, a.done, a.cycles, r.prev_best_idx
    return rows


_loops = {}


def loop_case(O, cycles=None):
    """(batch, [rows of ego b]) of the scenario under FISS+ with the gates enforced; computed once per process and shared."""
    cycles = GR.LOOP_CYCLES if cycles is None else cycles
    if cycles not in _loops:
        batch = loop_batch()
        _loops[cycles] = (batch, [ref_loop(O, batch, b, cycles) for b in range(batch.B)])
    return _loops[cycles]
