"""GPU: fp_gate_mask (stop lines that open and close behind the dense pass) against its numpy + oracle restatement (tests/gates_ref.py):
flag words exact on every candidate the reference decides by more than 1e-9, bits only ever added, every other bit and the cost table
untouched, the argmin and the violation count exact, through both memory spaces, with a launch order and a skipped ego; idempotence,
the ranking and the two other rule passes on its outputs, the waiver, graph capture, a ctx that never asks, the planner class, the error
codes - and the rule passes in the device-resident closed loop (ClosedLoopRunner(rules=...)) against the reference's loop."""
import dataclasses

import numpy as np
import pytest

import gates_ref as R
import rule_pass as RP
from fiss_plus_planner_amd import _abi, synth
from rule_pass import same_bits

pytestmark = pytest.mark.gpu
RULE = "gates"
OPEN_AT, LOOP_CYCLES, check_loop_invariants = R.OPEN_STEPS, R.LOOP_CYCLES, R.check_loop_invariants
SPEED = np.uint32(R.FLAG_SPEED)
POS_TOL = 1e-8  # the six ego numbers and x, y of a hand-over (tests/test_gpu_advance.py)


def dense_and_gates(engine, batch):
    return RP.dense_and_pass(engine, RULE, batch)


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("name", list(R.CASES))
def test_parity_host(engine, oracle, name):
    batch, refs, out, got = RP.host_parity(engine, oracle, RULE, name, skip_ego=2 if name in R.BASE_CASES else None)
    if name == "open":  # no bit closed: no bit may change, the winner is the dense call's
        assert np.array_equal(got[0], out.flags) and np.array_equal(got[1], out.best_idx) and same_bits(got[2], out.best_cost) and (got[3] == 0).all()
    if name == "line_ends":  # past the end: M <= 1, nothing is checked, no bit
        assert (out.flags[3] >> 20 <= 1).all() and np.array_equal(got[0][3], out.flags[3]) and got[3][3] == 0


@pytest.mark.parametrize("name", ["base", "t_now", "tick005", "stride32"])
def test_parity_device_with_order_and_skip(engine, oracle, name):
    RP.device_parity(engine, oracle, RULE, name)


def test_idempotence_and_rank(engine, oracle):
    for batch, out, first in RP.idempotence(engine, oracle, RULE, ("base", "waiver")):
        flags, bi, bc, _ = first
        ri, rc, nf = engine.rank_feasible(batch, out.cost, flags, 4)  # plane 0 of the ranking on the masked tables
        assert np.array_equal(ri[0], bi) and same_bits(np.where(bi < 0, 0.0, rc[0]), np.where(bi < 0, 0.0, bc)) and np.array_equal(np.isnan(rc[0]), bi < 0)
        for b in range(batch.B):
            assert nf[b] == np.count_nonzero(((flags[b] & _abi.FLAG_INFEASIBLE) == 0) & ~np.isnan(out.cost[b]))


def test_waiver_on_against_off(engine, oracle):
    (off_b, off_r), (on_b, on_r) = R.case(oracle, "base"), R.case(oracle, "waiver")
    off, on = dense_and_gates(engine, off_b)[1], dense_and_gates(engine, on_b)[1]
    egos = [b for b, r in enumerate(on_r) if r.waived.any()]
    assert egos and not any(r.waived.any() for r in off_r)
    for b in range(on_b.B):
        if b in egos:  # the waived line gates nobody any more: fewer violations, and here a plan where there was none
            assert on[3][b] < off[3][b] and np.array_equal(on[0][b] & off[0][b], on[0][b])
        else:
            assert np.array_equal(on[0][b], off[0][b]) and on[1][b] == off[1][b]
    assert any(off[1][b] < 0 <= on[1][b] for b in egos)


# ---------------------------------------------------------------- composition
CORRIDOR_WIDEN = 0.2


def full_batch():
    """The base gates batch with the envelope tests' profile and the boundary tests' corridor (both edges CORRIDOR_WIDEN further out)."""
    import boundary_ref
    import envelope_ref

    b = envelope_ref.with_profile(R.CASES["base"](), max_lat_accel=envelope_ref.MAX_LAT_ACCEL)
    left, right = boundary_ref.wavy_corridor(b.knots)
    return dataclasses.replace(b, bound_left=left + CORRIDOR_WIDEN, bound_right=right - CORRIDOR_WIDEN, bound_margin=0.05)


def composed(oracle, batch):
    """[(envelope, gates, boundary)] references per ego, each over the tables the one before it left."""
    import boundary_ref
    import envelope_ref

    out = []
    for b in range(batch.B):
        e = envelope_ref.ego_envelope(oracle, batch, b)
        g = R.ego_gates(oracle, batch, b, (e.cost, e.flags))
        out.append((e, g, boundary_ref.ego_mask(oracle, batch, b, (g.cost, g.flags))))
    return out


def test_envelope_gates_and_boundary_compose(engine, oracle):
    batch = full_batch()
    refs = composed(oracle, batch)
    assert all(sum(n) > 0 for n in zip(*[(e.n_limited, g.n_gated, m.n_masked) for e, g, m in refs]))  # every pass decides something ...
    assert len({tuple(r.best_idx for r in stage) for stage in zip(*refs)}) == 3                       # ... and moves a winner
    assert sum(m.best_idx >= 0 for _, _, m in refs) >= 2
    out = engine.plan_dense(batch, tables=True)
    f1, _, _, nl = engine.speed_envelope(batch, out.cost, out.flags)
    f2, bi2, bc2, ng = engine.gate_mask(batch, out.cost, f1)
    f3, bi3, bc3, nm = engine.boundary_mask(batch, out.cost, f2)
    for b, (e, g, m) in enumerate(refs):
        ok = ~(e.undecided | g.undecided | m.undecided)
        assert np.array_equal(f2[b][ok], g.flags[ok]) and np.array_equal(f3[b][ok], m.flags[ok]), b
        if ok.all():
            assert (bi2[b], ng[b], bi3[b], nm[b]) == (g.best_idx, g.n_gated, m.best_idx, m.n_masked), b
        if bi3[b] >= 0:
            assert same_bits(bc3[b:b + 1], out.cost[b, bi3[b]:bi3[b] + 1])
    assert sum((e.undecided | g.undecided | m.undecided).any() for e, g, m in refs) <= R.MAX_EXCLUDED_EGOS
    K = 3
    one = engine.plan_dense(batch, tables=True, winner=True, top_k=K, envelope=True, gates=True, boundary=True, margins=True)
    assert np.array_equal(one.flags, f3) and same_bits(one.cost, out.cost) and np.array_equal(one.best_idx, bi3) and same_bits(one.best_cost, bc3)
    assert np.array_equal(one.n_limited, nl) and np.array_equal(one.n_gated, ng) and np.array_equal(one.n_masked, nm)
    ri, rc, nf = engine.rank_feasible(batch, out.cost, f3, K)
    assert np.array_equal(one.rank_idx, ri) and same_bits(one.rank_cost, rc) and np.array_equal(one.n_feasible, nf) and np.array_equal(ri[0], bi3)
    w = engine.winner_trajs(batch, bi3)
    assert same_bits(one.best_traj, w.best_traj) and np.array_equal(one.best_flags, w.best_flags)
    md, ms, mo = engine.traj_margins(batch, best_idx=ri)
    assert same_bits(one.margin_dist, md) and np.array_equal(one.margin_step, ms) and np.array_equal(one.margin_obs, mo)
    lean = engine.plan_dense(batch, tables=False, gates=True)
    assert lean.cost is None and lean.flags is None and np.array_equal(lean.best_idx, engine.gate_mask(batch, out.cost, out.flags)[1])
    with pytest.raises(ValueError):
        engine.plan_dense(R.plain_batch(), gates=True)
    with pytest.raises(ValueError):
        engine.plan_dense(batch, gates=True, audit=True)
    with pytest.raises(ValueError):
        engine.gate_mask(R.plain_batch(), out.cost, out.flags)


# ---------------------------------------------------------------- capture
def test_dense_and_gates_replay_from_a_graph(engine, oracle):
    res, graph, host, n0 = RP.graph_replay(engine, oracle, RULE, "t_now")
    # t_now is read when the kernel runs: the replayed graph follows the clocks the base case has
    res.db.t["t_now"].zero_()
    graph.replay()
    _, base = R.case(oracle, "base")
    RP.check_against(RULE, base, (host.cost, host.flags), res.fetch(), "replay on another clock")
    assert RP.launches(engine, RULE) == n0 + 3  # a replay is not a call


# ---------------------------------------------------------------- off unless called
def test_a_ctx_that_never_asks_pays_nothing(oracle):
    RP.never_asks(oracle, RULE, "base")


# ---------------------------------------------------------------- the planner class
def test_planner_class(engine, oracle):
    from fiss_plus_planner_amd import planners as P
    from fiss_plus_planner_amd.frenet import FrenetState

    batch, refs = R.case(oracle, "t_now")
    b = next(i for i, r in enumerate(refs) if r.best_idx >= 0 and r.best_idx != r.best_in and not r.undecided.any())
    st = P.FrenetOptimalPlannerSettings(batch.nd, batch.nv, batch.nt)
    planner = P.FrenetOptimalPlanner(st, synth.Vehicle(), engine=engine, frame_on="host")
    planner.generate_frenet_frame(np.column_stack((batch.coef[b, 0], batch.coef[b, 4])))  # the ego's own centre line, from its spline's knot values
    assert np.allclose(planner.cubic_spline.knots, batch.knots[b], atol=1e-9)
    e = batch.ego[b]
    fs = FrenetState(t=0.0, s=e[0], s_d=e[1], s_dd=e[2], d=e[3], d_d=e[4], d_dd=e[5])
    speed, t_now = float(batch.target_speed[b]), int(batch.t_now[b])
    assert planner.plan(fs, speed, None, t_now).lattice_index == refs[b].best_in
    closed = (batch.gate_closed[b][:, None] >> np.arange(2, dtype=np.uint32)) & 1
    planner.set_gates(batch.gate_s[b], closed)  # front=None: vehicle.l / 2
    assert planner._gates[2] == batch.gate_front and np.array_equal(planner._gates[1], batch.gate_closed[b])
    assert planner.plan(fs, speed, None, t_now).lattice_index == refs[b].best_idx and np.array_equal(planner.last_tables[1], refs[b].flags)
    planner.set_gates(None, None)
    assert planner.plan(fs, speed, None, t_now).lattice_index == refs[b].best_in and np.array_equal(planner.last_tables[1], refs[b].flags_in)


# ---------------------------------------------------------------- errors
def test_host_error_codes(engine, oracle):
    batch, _ = R.case(oracle, "base")

    def good(s=batch.gate_s, c=batch.gate_closed, stride=2, T=R.T_GATE, front=2.0, decel=0.0):
        return _abi.FpGates(s.ctypes.data if s is not None else None, c.ctypes.data if c is not None else None, stride, T, front, decel)

    RP.host_error_codes(engine, RULE, batch, [good(s=None), good(c=None), good(stride=0), good(stride=33), good(stride=-1), good(T=0), good(T=-3), good(front=-1.0),
                                              good(front=float("nan")), good(front=float("inf")), good(decel=-0.1), good(decel=float("nan")), good(decel=float("inf"))])


def test_device_error_codes(engine, oracle):
    batch, _ = R.case(oracle, "base")
    RP.device_error_codes(engine, RULE, batch, [dict(gate_s=0), dict(closed=0), dict(gate_stride=0), dict(gate_stride=33), dict(T_gate=0), dict(front=-1.0),
                                                dict(front=float("nan")), dict(max_decel=-1.0), dict(max_decel=float("inf"))])


# ---------------------------------------------------------------- the closed loop
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_closed_loop_waits_for_the_gate(engine, oracle, graph):
    """The scenario of tests/test_gates_cpu.py, four egos with four opening steps: every cycle's winner is the reference loop's, the
    logged state its state, and the two invariants hold on the logged rows."""
    batch, loops = R.loop_case(oracle, OPEN_AT, LOOP_CYCLES)
    n0 = {k: engine.get_option(k) for k in ("gate_launches", "lattice_launches", "looplog_launches", "envelope_launches", "boundary_launches")}
    runner, out = RP.run_loop(engine, batch, LOOP_CYCLES, graph, rules=(RULE,))
    calls = 2 if graph else LOOP_CYCLES  # (a graph: the warm-up and the capture; a replay is not a call)
    assert engine.get_option("gate_launches") == n0["gate_launches"] + calls and engine.get_option("looplog_launches") == n0["looplog_launches"] + calls
    assert engine.get_option("envelope_launches") == n0["envelope_launches"] and engine.get_option("boundary_launches") == n0["boundary_launches"]
    log = out.log
    assert (log.n_rows == LOOP_CYCLES).all() and (out.done == 0).all() and (out.t_now == LOOP_CYCLES).all()
    for b, rows in enumerate(loops):
        got = log.rows[b, :LOOP_CYCLES]
        assert np.array_equal(got[:, _abi.LOG_TIME_STEP], [r.t_now for r in rows]), b
        assert np.array_equal(got[:, _abi.LOG_BEST_IDX], [r.best_idx for r in rows]), (b, np.nonzero(got[:, _abi.LOG_BEST_IDX] != [r.best_idx for r in rows])[0][:4])
        ego = got[:, [_abi.LOG_S, _abi.LOG_VELOCITY, _abi.LOG_S_DD, _abi.LOG_D, _abi.LOG_VELOCITY_Y, _abi.LOG_D_DD]]
        want = np.array([r.ego for r in rows])
        assert np.abs(ego - want).max() <= POS_TOL, (b, np.abs(ego - want).max())
        s_before = np.concatenate(([batch.ego[b, 0]], ego[:-1, 0]))
        arrival = check_loop_invariants(batch, b, got[:, _abi.LOG_TIME_STEP].astype(np.int64), got[:, _abi.LOG_BEST_IDX], s_before + batch.gate_front,
                                        ego[:, 0] + batch.gate_front, OPEN_AT[b])
        assert arrival == [r.t_now + 1 for r in rows if r.crossed][0]
        assert np.abs(out.ego[b] - rows[-1].ego).max() <= POS_TOL


def test_closed_loop_without_rules_runs_the_light(engine, oracle):
    """rules=() on the same batch: the lattice's own winner drives over the line while it is closed - the gate, not the lattice, held the
    ego; and the runner makes the calls it made before the rules existed."""
    cycles = 70
    batch, free = R.loop_case(oracle, OPEN_AT, cycles, gates=False)
    n0 = engine.get_option("gate_launches")
    runner, out = RP.run_loop(engine, batch, cycles, graph=False, rules=())
    assert engine.get_option("gate_launches") == n0 and not hasattr(runner, "cost_tbl")
    for b in (0, 2, 3):
        got = out.log.rows[b, :cycles]
        s_after = got[:, _abi.LOG_S]
        q_before, q_after = np.concatenate(([batch.ego[b, 0]], s_after[:-1])) + batch.gate_front, s_after + batch.gate_front
        crossed = (q_before <= R.GATE_S) & (R.GATE_S < q_after)
        arrival = got[crossed, _abi.LOG_TIME_STEP] + 1
        assert len(arrival) == 1 and arrival[0] < OPEN_AT[b] and arrival[0] == [r.t_now + 1 for r in free[b] if r.crossed][0], (b, arrival)
        assert np.array_equal(got[:, _abi.LOG_BEST_IDX], [r.best_idx for r in free[b]])


def test_closed_loop_with_every_rule_equals_the_calls_made_one_by_one(engine, oracle):
    import torch

    from fiss_plus_planner_amd.device_batch import DeviceBatch

    batch, cycles = full_batch(), 4
    runner, out = RP.run_loop(engine, batch, cycles, graph=False, rules=("boundary", "envelope", "gates"))
    assert runner.rules == ("envelope", "gates", "boundary")
    graphed = RP.run_loop(engine, batch, cycles, graph=True, rules=runner.rules)[1]
    # the same cycle by hand on a fresh resident batch
    db = DeviceBatch(batch, 0)
    B, Cn, dev = batch.B, batch.C, db.dev
    bi, bc, stats = db.empty(B, torch.int32), db.empty(B, torch.float64), db.empty((B, 4), torch.int32)
    cost, flags = db.empty((B, Cn), torch.float64), torch.zeros((B, Cn), dtype=torch.int32, device=dev)
    done, cyc = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    goal = torch.full((B, 2), 1e9, dtype=torch.float64, device=dev)
    cart = torch.full((B, 3), float("nan"), dtype=torch.float64, device=dev)
    fb = _abi.FpBatch.from_buffer_copy(db.fb)
    fb.skip, fb.launch_order = done.data_ptr(), None
    io = _abi.FpLoopIo()
    io.ego, io.t_now, io.done, io.cycles, io.goal_xy, io.cart_state = (t.data_ptr() for t in (db.t["ego"], db.t["t_now"], done, cyc, goal, cart))
    picked = []
    for _ in range(cycles):
        engine.plan_dense_device(db.params, fb, bi.data_ptr(), bc.data_ptr(), stats.data_ptr(), cost_tbl=cost.data_ptr(), flag_tbl=flags.data_ptr())
        engine.speed_envelope_device(db.params, fb, db.t["speed_limit"].data_ptr(), batch.limit_front, batch.limit_tol, batch.max_lat_accel, cost.data_ptr(),
                                     flags.data_ptr(), bi.data_ptr(), bc.data_ptr())
        engine.gate_mask_device(db.params, fb, db.t["gate_s"].data_ptr(), db.t["gate_closed"].data_ptr(), 2, R.T_GATE, batch.gate_front, batch.gate_max_decel,
                                cost.data_ptr(), flags.data_ptr(), bi.data_ptr(), bc.data_ptr())
        engine.boundary_mask_device(db.params, fb, db.t["bound_left"].data_ptr(), db.t["bound_right"].data_ptr(), batch.bound_margin, cost.data_ptr(), flags.data_ptr(),
                                    bi.data_ptr(), bc.data_ptr())
        engine.advance_device(db.params, fb, io, best_idx=bi.data_ptr())
        picked.append(bi.cpu().numpy().copy())
    torch.cuda.synchronize(dev)
    for got in (out, graphed):
        assert same_bits(got.ego, db.t["ego"].cpu().numpy()) and np.array_equal(got.t_now, db.t["t_now"].cpu().numpy())
        assert np.array_equal(got.done, done.cpu().numpy()) and np.array_equal(got.cycles, cyc.cpu().numpy()) and same_bits(got.cart, cart.cpu().numpy())
        for b in range(B):
            n = int(got.log.n_rows[b])
            assert np.array_equal(got.log.rows[b, :n, _abi.LOG_BEST_IDX], [p[b] for p in picked[:n]]), b
    assert same_bits(runner.flag_tbl.cpu().numpy(), flags.cpu().numpy()) and same_bits(runner.best_idx.cpu().numpy(), bi.cpu().numpy())
    # cycle 0 is the composition of the three references; some ego drives and some ego's first winner is not the lattice's
    refs = composed(oracle, batch)
    for b, (e, g, m) in enumerate(refs):
        if not (e.undecided | g.undecided | m.undecided).any():
            assert picked[0][b] == m.best_idx, b
    assert (out.cycles > 0).any() and any(m.best_idx != e.best_in for e, g, m in refs)
