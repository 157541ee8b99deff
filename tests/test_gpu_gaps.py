"""GPU: fp_gap_mask (a time gap to moving obstacles behind the dense pass) against its numpy + oracle restatement (tests/gaps_ref.py):
flag words exact on every candidate the reference decides by more than 1e-9, FP_FLAG_COLLISION only ever added and no other bit moved,
the cost table untouched, the argmin and the violation count exact, through both memory spaces, with a launch order and a skipped ego;
idempotence and the ranking on its outputs, the cases whose outcome follows from the definition, the error codes, plan_dense(gaps=True),
the planner class - and the rule in the device-resident closed loop (ClosedLoopRunner(rules=("gaps",))) against the reference's loop."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import gaps_ref as R
import rule_pass as RP
from fiss_plus_planner_amd import _abi, synth
from rule_pass import same_bits

pytestmark = pytest.mark.gpu
RULE = "gaps"
COLLISION = np.uint32(R.FLAG_COLLISION)
INT32_MAX = 2**31 - 1
POS_TOL = 1e-8  # the six ego numbers of a hand-over (tests/test_gpu_advance.py)


def dense_and_gaps(engine, batch):
    return RP.dense_and_pass(engine, RULE, batch)


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("name", list(R.CASES))
def test_parity_host(engine, oracle, name):
    batch, refs, out, got = RP.host_parity(engine, oracle, RULE, name, skip_ego=2 if name in R.BASE_CASES else None)
    assert got[3].sum() > 0, name
    if name == "line_ends":  # past the end: M <= 1, nothing is checked, no bit
        assert (out.flags[3] >> 20 <= 1).all() and np.array_equal(got[0][3], out.flags[3]) and got[3][3] == 0
    if name == "short_table":  # an ego whose survivors all violate: -1 / NaN
        b = next(i for i, r in enumerate(refs) if r.best_idx < 0 < r.survivors)
        assert got[1][b] == -1 and np.isnan(got[2][b]) and got[3][b] == refs[b].survivors
    if name == "lead":  # lag_follow = 0: the lead direction alone
        assert batch.gap_follow == 0 and got[3][0] == refs[0].n_close >= 1


@pytest.mark.parametrize("name", ["base", "t_now", "chunks", "cull_only", "no_lds", "polygons"])
def test_parity_device_with_order_and_skip(engine, oracle, name):
    RP.device_parity(engine, oracle, RULE, name, skip_ego=R.case(oracle, name)[0].B - 1)  # (the last ego: the chunks and table cases have two)


def test_idempotence_and_rank(engine, oracle):
    for batch, out, first in RP.idempotence(engine, oracle, RULE, ("base", "dense24")):  # (on the masked tables the violators are no longer evaluated: 0)
        flags, bi, bc, _ = first
        ri, rc, nf = engine.rank_feasible(batch, out.cost, flags, 4)  # plane 0 of the ranking on the masked tables
        assert np.array_equal(ri[0], bi) and same_bits(np.where(bi < 0, 0.0, rc[0]), np.where(bi < 0, 0.0, bc)) and np.array_equal(np.isnan(rc[0]), bi < 0)
        for b in range(batch.B):
            assert nf[b] == np.count_nonzero(((flags[b] & _abi.FLAG_INFEASIBLE) == 0) & ~np.isnan(out.cost[b]))
        w = engine.winner_trajs(batch, bi)  # a valid argument of the calls that take an argmin
        md, _, _ = engine.traj_margins(batch, best_idx=bi)
        assert np.array_equal(w.best_flags != 0, bi >= 0) and np.array_equal(np.isnan(md), bi < 0)


def test_outcomes_that_follow_from_the_definition(engine, oracle):
    batch, refs = R.case(oracle, "base")
    out = engine.plan_dense(batch, tables=True)
    horizon = int(np.ceil(batch.t_samples.max() / batch.tick_t))
    # no lag; `first` beyond every pose - just, by far, and at the largest value the struct holds -; lags below one grid step
    for kw in (dict(follow=0, lead=0), dict(first=horizon), dict(first=_abi.FP_MAX_POINTS), dict(first=_abi.FP_MAX_POINTS + 1), dict(first=INT32_MAX - 1),
               dict(first=INT32_MAX), dict(follow=1, lead=1)):
        flags, bi, bc, nc = engine.gap_mask(batch, out.cost, out.flags, **kw)
        assert np.array_equal(flags, out.flags) and np.array_equal(bi, out.best_idx) and same_bits(bc, out.best_cost) and (nc == 0).all(), kw
    res = RP.Resident(engine, RULE, batch)  # ... and through FP_MEM_DEVICE, and at check_stride 1 (another rounding of first to the grid)
    res.dense()
    res.call(first=INT32_MAX)
    got = res.fetch()
    assert np.array_equal(got[0], out.flags) and np.array_equal(got[1], out.best_idx) and same_bits(got[2], out.best_cost) and (got[3] == 0).all()
    dense1 = dataclasses.replace(batch, check_stride=1)
    o1 = engine.plan_dense(dense1, tables=True)
    assert engine.gap_mask(dense1, o1.cost, o1.flags)[3].sum() > 0
    for first in (INT32_MAX, INT32_MAX - 1):
        flags, bi, bc, nc = engine.gap_mask(dense1, o1.cost, o1.flags, first=first)
        assert np.array_equal(flags, o1.flags) and np.array_equal(bi, o1.best_idx) and same_bits(bc, o1.best_cost) and (nc == 0).all(), first
    # a `first` one step short of the last pose looks at that pose alone: the reference's verdicts
    last = [R.ego_gaps(oracle, batch, b, first=horizon - 2) for b in range(batch.B)]
    RP.check_against(RULE, last, (out.cost, out.flags), engine.gap_mask(batch, out.cost, out.flags, first=horizon - 2), "first = horizon - 2")
    for kw in (dict(follow=-1), dict(lead=_abi.FP_MAX_POINTS + 1), dict(first=0), dict(first=INT32_MAX + 1), dict(first=2**32 + 2), dict(follow=2**32 + 20)):
        with pytest.raises(ValueError):  # (a ctypes field would wrap these silently)
            engine.gap_mask(batch, out.cost, out.flags, **kw)
    full = engine.gap_mask(batch, out.cost, out.flags, follow=horizon, lead=horizon)
    more = engine.gap_mask(batch, out.cost, out.flags, follow=_abi.FP_MAX_POINTS, lead=_abi.FP_MAX_POINTS)
    for a, b in zip(full, more):
        assert same_bits(a, b)  # lags longer than the horizon
    want = [R.ego_gaps(oracle, batch, b, follow=horizon, lead=horizon) for b in range(batch.B)]
    RP.check_against(RULE, want, (out.cost, out.flags), full, "lag = horizon")
    no_scene = dataclasses.replace(batch, scene_of=np.full(batch.B, -1))
    o2, got = dense_and_gaps(engine, no_scene)
    assert np.array_equal(got[0], o2.flags) and np.array_equal(got[1], o2.best_idx) and same_bits(got[2], o2.best_cost) and (got[3] == 0).all()
    assert not (o2.flags & COLLISION).any()


# ---------------------------------------------------------------- composition
def full_batch():
    """The base batch with the gates tests' lines, the envelope tests' profile and the boundary tests' corridor (widened)."""
    import boundary_ref
    import envelope_ref
    import gates_ref

    b = envelope_ref.with_profile(gates_ref.with_gates(R.CASES["base"]()), max_lat_accel=envelope_ref.MAX_LAT_ACCEL)
    left, right = boundary_ref.wavy_corridor(b.knots)
    return dataclasses.replace(b, bound_left=left + 0.6, bound_right=right - 0.6, bound_margin=0.05)


def test_plan_dense_with_gaps_is_the_chain_of_calls(engine, oracle):
    batch, refs = R.case(oracle, "base")
    out, got = dense_and_gaps(engine, batch)
    one = engine.plan_dense(batch, tables=True, winner=True, gaps=True, top_k=3)
    assert np.array_equal(one.flags, got[0]) and same_bits(one.cost, out.cost) and np.array_equal(one.best_idx, got[1]) and same_bits(one.best_cost, got[2])
    assert np.array_equal(one.n_close, got[3]) and np.array_equal(one.rank_idx[0], got[1])
    w = engine.winner_trajs(batch, got[1])
    assert same_bits(one.best_traj, w.best_traj) and np.array_equal(one.best_flags, w.best_flags)
    lean = engine.plan_dense(batch, tables=False, gaps=True)
    assert lean.cost is None and lean.flags is None and np.array_equal(lean.best_idx, got[1])
    # behind the other three passes: fewer survivors reach it
    every = full_batch()
    o = engine.plan_dense(every, tables=True)
    f1, _, _, nl = engine.speed_envelope(every, o.cost, o.flags)
    f2, _, _, ng = engine.gate_mask(every, o.cost, f1)
    f3, _, _, nm = engine.boundary_mask(every, o.cost, f2)
    f4, bi4, bc4, ncl = engine.gap_mask(every, o.cost, f3)
    chained = engine.plan_dense(every, tables=True, envelope=True, gates=True, boundary=True, gaps=True)
    assert np.array_equal(chained.flags, f4) and np.array_equal(chained.best_idx, bi4) and same_bits(chained.best_cost, bc4)
    assert np.array_equal(chained.n_limited, nl) and np.array_equal(chained.n_gated, ng) and np.array_equal(chained.n_masked, nm) and np.array_equal(chained.n_close, ncl)
    assert ncl.sum() > 0 and ((f3 & _abi.FLAG_INFEASIBLE) != 0).sum() > ((o.flags & _abi.FLAG_INFEASIBLE) != 0).sum()
    for b in range(every.B):  # the reference over the tables the three passes left
        r = R.ego_gaps(oracle, every, b, tables=(o.cost[b], f3[b]))
        ok = ~r.undecided
        assert np.array_equal(f4[b][ok], r.flags[ok]) and (r.undecided.any() or (bi4[b], ncl[b]) == (r.best_idx, r.n_close)), b
    with pytest.raises(ValueError):
        engine.plan_dense(R.moving_batch(), gaps=True)  # both lags 0: no rule on the batch
    with pytest.raises(ValueError):
        engine.plan_dense(batch, gaps=True, audit=True)


RULES_ON = dict(envelope=True, gates=True, boundary=True, gaps=True)
COUNTS = ("n_limited", "n_gated", "n_masked", "n_close")


def test_plan_dense_every_rule_into_the_callers_arrays_without_tables(engine):
    """The caller's arrays hold no tables: the call brings its own, twice into the same arrays, and leaves nothing of them behind."""
    every = full_batch()
    want = engine.plan_dense(every, tables=True, top_k=3, **RULES_ON)
    out = engine.dense_outputs(every.B, every.C, tables=False)
    for call in range(2):
        got = engine.plan_dense(every, tables=False, out=out, top_k=3, **RULES_ON)
        assert got is out and got.cost is None and got.flags is None, call
        assert np.array_equal(got.best_idx, want.best_idx) and same_bits(got.best_cost, want.best_cost), call
        for name in COUNTS:
            assert np.array_equal(getattr(got, name), getattr(want, name)) and getattr(got, name).dtype == np.int32, (call, name)
        assert np.array_equal(got.rank_idx, want.rank_idx) and same_bits(got.rank_cost, want.rank_cost) and np.array_equal(got.n_feasible, want.n_feasible), call
    assert want.n_close.sum() > 0  # (the passes have work on this batch)
    plain, fresh = engine.plan_dense(every, tables=False, out=out), engine.plan_dense(every, tables=False)
    assert plain.cost is None and np.array_equal(plain.best_idx, fresh.best_idx) and same_bits(plain.best_cost, fresh.best_cost)  # the unmasked winner: no stale fp_result


def test_plan_dense_every_rule_on_a_batch_without_egos(engine):
    every = full_batch()
    none = dataclasses.replace(every, v_samples=every.v_samples[:0], target_speed=every.target_speed[:0], ego=every.ego[:0], frame_of=every.frame_of[:0],
                               scene_of=every.scene_of[:0], t_now=every.t_now[:0])  # (frames, scenes and the rules' data stay)
    assert none.B == 0 and none.F == every.F and none.S == every.S and none.gate_s is every.gate_s
    out = engine.plan_dense(none, top_k=3, margins=True, **RULES_ON)
    for name in COUNTS:
        assert getattr(out, name).shape == (0,) and getattr(out, name).dtype == np.int32, name
    assert out.rank_idx.shape == (3, 0) and out.rank_cost.shape == (3, 0) and out.n_feasible.shape == (0,)
    assert out.margin_dist.shape == (3, 0) and out.margin_step.shape == (3, 0) and out.margin_obs.shape == (3, 0)
    assert out.best_idx.shape == (0,)


def test_plan_dense_audit_goes_with_top_k_and_with_no_rule(engine):
    every = full_batch()
    out = engine.plan_dense(every, audit=True, top_k=3)
    assert out.audit.shape == (every.B,) and out.audit.dtype == np.uint32 and out.rank_idx.shape == (3, every.B)
    assert np.array_equal(out.rank_idx[0], out.best_idx)
    for name in RULES_ON:
        with pytest.raises(ValueError):
            engine.plan_dense(every, audit=True, top_k=3, **{name: True})


def test_dense_and_gaps_replay_from_a_graph(engine, oracle):
    RP.graph_replay(engine, oracle, RULE, "base")


def test_a_ctx_that_never_asks_pays_nothing(oracle):
    RP.never_asks(oracle, RULE, "base")


# ---------------------------------------------------------------- the planner class
def test_planner_class(engine, oracle):
    from fiss_plus_planner_amd import planners as P
    from fiss_plus_planner_amd.frenet import FrenetState
    from fiss_plus_planner_amd.obstacles import ObstacleTable

    batch, refs = R.case(oracle, "base")
    b = next(i for i, r in enumerate(refs) if r.best_idx >= 0 and r.best_idx != r.best_in and not r.undecided.any())
    st = P.FrenetOptimalPlannerSettings(batch.nd, batch.nv, batch.nt)
    planner = P.FrenetOptimalPlanner(st, synth.Vehicle(), engine=engine, frame_on="host")
    planner.generate_frenet_frame(np.column_stack((batch.coef[b, 0], batch.coef[b, 4])))  # the ego's own centre line, from its spline's knot values
    assert np.allclose(planner.cubic_spline.knots, batch.knots[b], atol=1e-9)
    e = batch.ego[b]
    fs = FrenetState(t=0.0, s=e[0], s_d=e[1], s_dd=e[2], d=e[3], d_d=e[4], d_dd=e[5])
    speed = float(batch.target_speed[b])
    table = ObstacleTable(batch.obs_pose[b].copy(), batch.obs_dims[b].copy(), int(batch.final_time_step[b]))
    assert planner.plan(fs, speed, table, 0).lattice_index == refs[b].best_in
    planner.set_time_gap(batch.gap_follow * batch.tick_t, batch.gap_lead * batch.tick_t, batch.gap_first * batch.tick_t)
    traj = planner.plan(fs, speed, table, 0)
    assert traj.lattice_index == refs[b].best_idx and np.array_equal(planner.last_tables[1], refs[b].flags)
    w = engine.winner_trajs(batch, np.array([r.best_idx for r in refs], dtype=np.int32))
    M = int(w.best_flags[b]) >> 20
    assert np.array_equal(traj.x, w.best_traj[b, 9, :M]) and np.array_equal(traj.y, w.best_traj[b, 10, :M])  # ... and its series
    planner.set_time_gap(0.0)
    assert planner.plan(fs, speed, table, 0).lattice_index == refs[b].best_in and np.array_equal(planner.last_tables[1], refs[b].flags_in)


# ---------------------------------------------------------------- errors
def test_host_error_codes(engine, oracle):
    batch, _ = R.case(oracle, "base")

    def good(follow=20, lead=10, first=2):
        return _abi.FpTimeGap(follow, lead, first, 0)

    RP.host_error_codes(engine, RULE, batch, [good(follow=-1), good(lead=-1), good(follow=_abi.FP_MAX_POINTS + 1), good(lead=_abi.FP_MAX_POINTS + 1), good(first=0),
                                              good(first=-3)])


def test_device_error_codes(engine, oracle):
    batch, _ = R.case(oracle, "base")
    res, n = RP.device_error_codes(engine, RULE, batch, [])
    first = res.fetch()
    for kw in (dict(follow=-1), dict(lead=-2), dict(follow=_abi.FP_MAX_POINTS + 1), dict(lead=_abi.FP_MAX_POINTS + 1), dict(first=0), dict(first=2**31)):
        with pytest.raises(ValueError):  # the binding refuses what the struct cannot hold or the library would refuse
            res.call(**kw)
    for g in (_abi.FpTimeGap(-1, 0, 1, 0), _abi.FpTimeGap(0, -2, 1, 0), _abi.FpTimeGap(_abi.FP_MAX_POINTS + 1, 0, 1, 0), _abi.FpTimeGap(0, _abi.FP_MAX_POINTS + 1, 1, 0),
              _abi.FpTimeGap(20, 10, 0, 0), _abi.FpTimeGap(20, 10, -5, 0)):  # ... and so does the library itself
        rc = engine._lib.fp_gap_mask(engine._ctx, C.byref(res.db.params), C.byref(res.fb), C.byref(g), res.cost.data_ptr(), res.flags.data_ptr(), res.bi.data_ptr(),
                                     res.bc.data_ptr(), None, _abi.FP_MEM_DEVICE, None)
        assert rc == -1
    rc = engine._lib.fp_gap_mask(engine._ctx, C.byref(res.db.params), C.byref(res.fb), None, res.cost.data_ptr(), res.flags.data_ptr(), res.bi.data_ptr(),
                                 res.bc.data_ptr(), None, _abi.FP_MEM_DEVICE, None)
    assert rc == -1
    assert RP.launches(engine, RULE) == n  # (none of them launched or wrote)
    for a, b in zip(first, res.fetch()):
        assert same_bits(a, b)


# ---------------------------------------------------------------- the closed loop
def logged_ego(rows):
    return rows[:, [_abi.LOG_S, _abi.LOG_VELOCITY, _abi.LOG_S_DD, _abi.LOG_D, _abi.LOG_VELOCITY_Y, _abi.LOG_D_DD]]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_closed_loop_keeps_the_gap(engine, oracle, graph):
    """The scenario of tests/test_gaps_cpu.py: every cycle's winner is the reference loop's, the logged state its state, every cycle has
    a plan."""
    cycles = R.LOOP_CYCLES
    batch, rows = R.loop_case(oracle)
    assert not any(r.undecided for r in rows)  # (state-exact on every cycle: none is undecided)
    n0 = {k: engine.get_option(k) for k in ("gap_launches", "lattice_launches", "gate_launches")}
    runner, out = RP.run_loop(engine, batch, cycles, graph, rules=(RULE,))
    calls = 2 if graph else cycles  # (a graph: the warm-up and the capture; a replay is not a call)
    assert engine.get_option("gap_launches") == n0["gap_launches"] + calls and engine.get_option("gate_launches") == n0["gate_launches"]
    log = out.log
    assert (log.n_rows == cycles).all() and (out.done == 0).all() and (out.t_now == cycles).all()
    got = log.rows[0, :cycles]
    assert np.array_equal(got[:, _abi.LOG_TIME_STEP], [r.t_now for r in rows])
    assert np.array_equal(got[:, _abi.LOG_BEST_IDX], [r.best_idx for r in rows]), np.nonzero(got[:, _abi.LOG_BEST_IDX] != [r.best_idx for r in rows])[0][:4]
    assert (got[:, _abi.LOG_BEST_IDX] >= 0).all()
    ego, want = logged_ego(got), np.array([r.ego for r in rows])
    assert np.abs(ego - want).max() <= POS_TOL, np.abs(ego - want).max()
    assert np.abs(out.ego[0] - rows[-1].ego).max() <= POS_TOL
    assert runner.n_flagged["gaps"].cpu().numpy()[0] == rows[-1].n_close


def test_closed_loop_without_the_rule_closes_in(engine, oracle):
    """rules=() on the same batch: the driven ego comes closer to the lead than with the rule - the rule, not the lattice, kept the
    distance; and the runner makes the calls it made before the rules existed."""
    cycles = R.LOOP_CYCLES
    batch, free = R.loop_case(oracle, gaps=False)
    n0 = engine.get_option("gap_launches")
    runner, out = RP.run_loop(engine, batch, cycles, graph=False, rules=())
    assert engine.get_option("gap_launches") == n0 and not hasattr(runner, "cost_tbl")
    got = out.log.rows[0, :cycles]
    assert np.array_equal(got[:, _abi.LOG_BEST_IDX], [r.best_idx for r in free])
    steps = np.arange(1, cycles + 1)
    came = R.bumper_distance(batch, got[:, _abi.LOG_S], steps)
    kept = R.bumper_distance(batch, RP.run_loop(engine, batch, cycles, graph=False, rules=(RULE,))[1].log.rows[0, :cycles, _abi.LOG_S], steps)
    assert came < batch.veh_l < R.LOOP_FOLLOW * batch.tick_t * R.LEAD_V < kept, (came, kept)


def test_closed_loop_with_all_four_rules_replays_from_a_graph(engine, oracle):
    batch, cycles = full_batch(), 4
    runner, out = RP.run_loop(engine, batch, cycles, graph=False, rules=("gaps", "boundary", "envelope", "gates"))
    assert runner.rules == ("envelope", "gates", "boundary", "gaps")
    graphed = RP.run_loop(engine, batch, cycles, graph=True, rules=runner.rules)[1]
    assert same_bits(out.ego, graphed.ego) and np.array_equal(out.t_now, graphed.t_now) and np.array_equal(out.done, graphed.done)
    assert np.array_equal(out.cycles, graphed.cycles) and same_bits(out.cart, graphed.cart)
    for b in range(batch.B):
        n = int(out.log.n_rows[b])
        assert n == int(graphed.log.n_rows[b]) and same_bits(out.log.rows[b, :n], graphed.log.rows[b, :n]), b
    assert (out.cycles > 0).any()
    # cycle 0 of the chain by hand: the runner's first winners
    o = engine.plan_dense(batch, tables=True, envelope=True, gates=True, boundary=True, gaps=True)
    first = np.array([out.log.rows[b, 0, _abi.LOG_BEST_IDX] if out.log.n_rows[b] else -1 for b in range(batch.B)])
    assert np.array_equal(first[o.best_idx >= 0], o.best_idx[o.best_idx >= 0])
