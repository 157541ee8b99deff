"""GPU: fp_plan_fiss_rules - FISS / FISS+ whose validation sees the road rules (FrenetEngine.plan_fiss(enforce=...),
plan_fiss_rules_device, ClosedLoopRunner(enforce=...)).

  1. identity: a rule set that cannot speak leaves every output of plan_fiss, bit for bit, in both memory modes;
  2. the lattice stage, exact: the host walk (search.py) over the device's own masked tables (plan_dense with the same passes), bit 128
     folded into a constraint bit;
  3. the refinement, exact, by composition on the device: the call's own trace, eval_trajs' words of its rows, rules_eval's rule bits of
     those words, the pop loop of the contract in numpy;
  4. every case of tests/test_fiss_rules_cpu.py against the CPU reference (tests/fiss_rules_ref.py);
  5. the winner's series; 6. the closed loop at the red light; 7. a launch order and a second call; 8. the errors of the C ABI;
  9. the outputs recorded before the rule instance shared the rules' evaluation, exactly.
"""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import fiss_rules_parent
import fiss_rules_ref as FR
import gates_ref as GR
from conftest import GOLDEN
from fiss_plus_planner_amd import _abi, rules, search, synth
from fiss_plus_planner_amd.engine import host_structs

pytestmark = pytest.mark.gpu
NAMES = ("envelope", "gates", "boundary", "gaps")
INFEASIBLE = np.uint32(_abi.FLAG_INFEASIBLE)
CONSTRAINT_BITS = np.uint32(_abi.FLAG_CONSTRAINTS | _abi.FLAG_BOUNDARY)
COLLISION = np.uint32(_abi.FLAG_COLLISION)
POS_TOL = 1e-8  # the six ego numbers of a hand-over (tests/test_gpu_advance.py)
OUT_KEYS = ("best_ijk", "best_cost", "end_state", "refined", "stats", "prev_best_idx")


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


with_rules, silent, case = FR.with_rules, FR.silent, FR.case


def history(b, seed=5):
    rng = np.random.default_rng(seed)
    return np.where(rng.uniform(size=(b.B, 1)) < 0.5, -1, np.column_stack([rng.integers(0, b.nd, b.B), rng.integers(0, b.nv, b.B),
                                                                          rng.integers(0, b.nt, b.B)])).astype(np.int32)


# ---------------------------------------------------------------- the resident call
class Resident:
    """The batch and the outputs of one fp_plan_fiss_rules call in device memory."""

    def __init__(self, engine, batch, kind, names, prev=None, order=None, R=3):
        import torch

        from fiss_plus_planner_amd.device_batch import DeviceBatch

        self.torch, self.engine, self.db = torch, engine, DeviceBatch(batch, 0, order_hint=False)
        db, B = self.db, batch.B
        self.fb = _abi.FpBatch.from_buffer_copy(db.fb)
        if order is not None:
            self.order = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(db.dev)
            self.fb.launch_order = self.order.data_ptr()
        i32, f64 = torch.int32, torch.float64
        self.prev = torch.from_numpy(np.full((B, 3), -1, dtype=np.int32) if prev is None else np.ascontiguousarray(prev, dtype=np.int32)).to(db.dev)
        self.o = dict(best_ijk=db.empty((B, 3), i32), best_cost=db.empty(B, f64), end_state=db.empty((B, 3), f64), refined=db.empty(B, i32),
                      stats=db.empty((B, 4), i32))
        self.rejected = torch.zeros(B, dtype=i32, device=db.dev)
        plus = kind == "FISS+"
        self.opts = _abi.FpFissOpts(_abi.FP_FISS_PLUS if plus else _abi.FP_FISS, R if plus else 0, 10.0, 0.5)
        f = _abi.FpFissIo()
        f.samp_min, f.samp_max, f.samp_res = (db.t[k].data_ptr() for k in ("samp_min", "samp_max", "samp_res"))
        f.prev_best_idx = self.prev.data_ptr()
        for k, t in self.o.items():
            setattr(f, k, t.data_ptr())
        self.fio = f
        self.rule_set, self.structs = rules.rule_set(batch, lambda k: db.t[k].data_ptr(), names)

    def call(self, stream=0):
        self.engine.plan_fiss_rules_device(self.db.params, self.fb, self.opts, self.fio, self.rule_set, None, self.rejected.data_ptr(), stream)

    def fetch(self):
        self.torch.cuda.synchronize(self.db.dev)
        out = {k: t.cpu().numpy() for k, t in self.o.items()}
        out["prev_best_idx"] = self.prev.cpu().numpy()
        out["rejected"] = self.rejected.cpu().numpy()
        return out


# ---------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("kind", ["FISS", "FISS+"])
@pytest.mark.parametrize("name", ["silent", "silent_long"])
def test_identity(engine, kind, name):
    batch = case(name)
    prev = history(batch)
    plain = engine.plan_fiss(batch, kind, prev_best_idx=prev, trace=True, winner=True, traj_stride=256)
    n0 = engine.get_option("fiss_rules_calls")
    got = engine.plan_fiss(batch, kind, prev_best_idx=prev, trace=True, winner=True, traj_stride=256, enforce=NAMES)
    assert engine.get_option("fiss_rules_calls") == n0 + 1
    found = plain.best_ijk[:, 0] >= 0
    assert found.any() and (kind == "FISS" or plain.refined.any())
    for k in OUT_KEYS + ("best_flags", "best_traj"):
        assert same_bits(getattr(got, k), getattr(plain, k)), (kind, name, k)
    if kind == "FISS+":
        assert same_bits(got.trace[found], plain.trace[found])
    assert not got.rejected.any()
    dev = Resident(engine, batch, kind, NAMES, prev=prev)
    dev.call()
    d = dev.fetch()
    for k in OUT_KEYS:
        assert same_bits(d[k], getattr(plain, k)), (kind, name, k, "device")
    assert not d["rejected"].any()


# ---------------------------------------------------------------- 2. the lattice stage
def host_walk(batch, tab, kind, prev):
    """The host walk over the masked tables `tab` (bit 128 folded into a constraint bit of a copy) -> best_ijk, stats, prev_best_idx,
    end_state, best_cost per ego."""
    B = batch.B
    ijk = np.full((B, 3), -1, dtype=np.int32)
    stats = np.zeros((B, 4), dtype=np.int32)
    prev_out = prev.copy()
    end = np.full((B, 3), np.nan)
    cost = np.full(B, np.nan)
    for e in range(B):
        J, F = search.tables_to_dvt(tab.cost[e], tab.flags[e], batch.nd, batch.nv, batch.nt)
        F = np.where(F & np.uint32(_abi.FLAG_BOUNDARY), F | np.uint32(_abi.FLAG_SPEED), F) & np.uint32(0xFF)
        E = search.cost_est_table(batch.d_samples, batch.v_samples[e], batch.t_samples, batch.samp_min[e], batch.samp_max[e],
                                  None if prev[e, 0] < 0 else prev[e])
        idx, st = (search.fiss_search if kind == "FISS" else search.fissplus_search)(J, F, E)
        stats[e] = st
        if idx is not None:
            ijk[e] = prev_out[e] = idx
            end[e] = batch.d_samples[idx[0]], batch.v_samples[e][idx[1]], batch.t_samples[idx[2]]
            cost[e] = J[tuple(idx)]
    return ijk, stats, prev_out, end, cost


@pytest.mark.parametrize("kind", ["FISS", "FISS+"])
@pytest.mark.parametrize("names", [(n,) for n in NAMES] + [NAMES], ids=list(NAMES) + ["all"])
@pytest.mark.parametrize("name", ["small", "wide"])
def test_lattice_stage(engine, name, names, kind):
    batch = case(name)
    prev = history(batch)
    tab = engine.plan_dense(batch, tables=True, **{n: True for n in names})
    plain = engine.plan_dense(batch, tables=True)
    got = engine.plan_fiss(batch, kind, prev_best_idx=prev, max_refine_iters=0, enforce=names)
    ijk, stats, prev_out, end, cost = host_walk(batch, tab, kind, prev)
    assert np.array_equal(got.best_ijk, ijk) and np.array_equal(got.stats, stats) and np.array_equal(got.prev_best_idx, prev_out), (name, names, kind)
    assert same_bits(got.end_state, end) and same_bits(got.best_cost, cost)
    assert not got.refined.any() and not got.rejected.any()
    if names == NAMES and kind == "FISS+" and name == "small":  # the case reaches the paths it exists for
        free = host_walk(batch, plain, kind, prev)[0]
        assert (tab.flags != plain.flags).any() and (free != ijk).any()  # a rule moves some ego's coarse winner
        assert ((tab.flags & INFEASIBLE) == np.uint32(_abi.FLAG_BOUNDARY)).any()  # a sample only the corridor rejects


def test_boundary_only_sample_is_popped_as_a_constraint_failure(engine):
    """The corrected test of the search kernels: a sample whose only bit is 128 is popped before the winner and is no collision check."""
    batch = case("small")
    prev = np.full((batch.B, 3), -1, dtype=np.int32)
    tab = engine.plan_dense(batch, tables=True, boundary=True)
    hit = 0
    for kind in ("FISS", "FISS+"):
        got = engine.plan_fiss(batch, kind, max_refine_iters=0, enforce=("boundary",))
        ijk, stats, _, _, cost = host_walk(batch, tab, kind, prev)
        assert np.array_equal(got.best_ijk, ijk) and np.array_equal(got.stats, stats)
        for e in range(batch.B):
            J, F = search.tables_to_dvt(tab.cost[e], tab.flags[e], batch.nd, batch.nv, batch.nt)
            only = (F & INFEASIBLE) == np.uint32(_abi.FLAG_BOUNDARY)
            if ijk[e, 0] >= 0 and (only & (J < cost[e])).any():
                hit += 1  # cheaper than the winner: the cost-ordered validation pops it first
                assert stats[e, 2] > stats[e, 3]  # validated, not collision-checked
    assert hit > 0


# ---------------------------------------------------------------- 3. the refinement
def coarse_costs(engine, batch, names, prev):
    """The coarse winner's cost as the refinement prices it (the probes' evaluator): with a sampling resolution of 0 every probe of the
    first round IS the coarse winner, so row 0 of that call's trace carries it."""
    still = dataclasses.replace(batch, samp_res=np.zeros_like(batch.samp_res))
    return engine.plan_fiss(still, "FISS+", prev_best_idx=prev, max_refine_iters=1, trace=True, enforce=names).trace[:, 0, 3]


def pop_loop(cost, base, ruled, coarse):
    """Contract 3 on one ego's candidate list -> (winner or -1, validated, checks, rejected)."""
    validated = checks = rejected = 0
    for c in sorted(range(len(cost)), key=lambda c: (cost[c], c)):
        if cost[c] > coarse:
            break
        validated += 1
        word = base[c]
        if not word & INFEASIBLE:
            word = ruled[c]
            rejected += bool(word & INFEASIBLE)
        if word & CONSTRAINT_BITS:
            continue
        checks += 1
        if not word & COLLISION:
            return c, validated, checks, rejected
    return -1, validated, checks, rejected


@pytest.mark.parametrize("name", ["small", "long"])
def test_refinement_by_composition(engine, name):
    batch = case(name)
    prev = history(batch)
    R = 3
    coarse = engine.plan_fiss(batch, "FISS+", prev_best_idx=prev, max_refine_iters=0, enforce=NAMES)
    got = engine.plan_fiss(batch, "FISS+", prev_best_idx=prev, max_refine_iters=R, trace=True, enforce=NAMES)
    found = coarse.best_ijk[:, 0] >= 0
    assert np.array_equal(got.best_ijk, coarse.best_ijk) and np.array_equal(got.prev_best_idx, coarse.prev_best_idx)
    # (rows the call did not write - an ego without a coarse winner, rounds that ended early - are never read below: any valid end state)
    filler = np.column_stack([np.full(batch.B, batch.d_samples[0]), batch.v_samples[:, 0], np.full(batch.B, batch.t_samples[0])])[:, None, :]
    es = np.where(found[:, None, None] & ~np.isnan(got.trace[:, :, 3:4]), got.trace[:, :, :3], filler)
    base = engine.eval_trajs(batch, es).flags
    ruled = engine.rules_eval(batch, es, base, rules=NAMES).flags
    c0 = coarse_costs(engine, batch, NAMES, prev)
    ahead = 0
    for e in range(batch.B):
        if not found[e]:
            assert np.array_equal(got.stats[e], coarse.stats[e]) and got.refined[e] == 0 and got.rejected[e] == 0 and np.isnan(got.best_cost[e])
            continue
        n = int((~np.isnan(got.trace[e, :, 3])).sum())
        assert n > 0 and not np.isnan(got.trace[e, :n, 3]).any()
        w, validated, checks, rejected = pop_loop(got.trace[e, :n, 3], base[e, :n], ruled[e, :n], c0[e])
        assert np.array_equal(got.stats[e], coarse.stats[e] + [0, n, validated, checks]), (name, e)
        assert got.rejected[e] == rejected and got.refined[e] == (w >= 0), (name, e)
        assert same_bits(got.end_state[e], got.trace[e, w, :3] if w >= 0 else coarse.end_state[e]), (name, e)
        assert same_bits(got.best_cost[e:e + 1], got.trace[e, w:w + 1, 3] if w >= 0 else c0[e:e + 1]), (name, e)
        ahead += rejected > 0
    assert ahead > 0, name  # a base-feasible candidate that a rule rejected, consumed before some ego's result
    # the same call on resident data, and with a launch order
    for order in (None, np.arange(batch.B)[::-1]):
        dev = Resident(engine, batch, "FISS+", NAMES, prev=prev, order=order, R=R)
        dev.call()
        d = dev.fetch()
        for k in OUT_KEYS + ("rejected",):
            assert same_bits(d[k], getattr(got, k)), (name, k, order is not None)


# ---------------------------------------------------------------- 4. against the CPU reference
@pytest.mark.parametrize("name,names,kind", FR.CASES, ids=[f"{n}-{'+'.join(r)}-{k}" for n, r, k in FR.CASES])
def test_against_the_cpu_reference(engine, oracle, name, names, kind):
    batch = case(name)
    refs = FR.batch_plan(oracle, batch, kind, names, key=name)
    FR.check_caps(refs, name)
    got = engine.plan_fiss(batch, kind, enforce=names)
    compared = 0
    for e, r in enumerate(refs):
        if r.undecided:
            continue
        compared += 1
        assert np.array_equal(got.best_ijk[e], r.best_ijk) and np.array_equal(got.stats[e], r.stats) and np.array_equal(got.prev_best_idx[e], r.prev_best_idx), (name, e)
        assert bool(got.refined[e]) == r.refined and got.rejected[e] == r.rejected, (name, e)
        if r.best_ijk[0] < 0:
            assert np.isnan(got.best_cost[e]) and np.isnan(got.end_state[e]).all()
            continue
        assert np.abs(got.end_state[e] - r.end_state).max() <= 1e-9 and abs(got.best_cost[e] - r.best_cost) <= 1e-6, (name, e)
    assert compared >= batch.B - 1


# ---------------------------------------------------------------- 5. the winner's series
def test_winner_series(engine):
    batch = case("small")
    got = engine.plan_fiss(batch, "FISS+", winner=True, enforce=NAMES)
    bare = engine.plan_fiss(batch, "FISS+", enforce=NAMES)
    for k in OUT_KEYS + ("rejected",):
        assert same_bits(getattr(got, k), getattr(bare, k)), k
    found = got.best_ijk[:, 0] >= 0
    assert found.any() and got.refined.any()
    filler = np.column_stack([np.full(batch.B, batch.d_samples[0]), batch.v_samples[:, 0], np.full(batch.B, batch.t_samples[0])])
    ends = np.where(found[:, None], got.end_state, filler)[:, None, :]  # (an ego without a plan: any valid end state, not compared)
    ev = engine.eval_trajs(batch, ends, dump=True)
    assert np.array_equal(got.best_flags[found], ev.flags[found, 0]) and not (got.best_flags[found] & INFEASIBLE).any()
    assert same_bits(got.best_traj[found], ev.traj[found, 0])
    assert not got.best_flags[~found].any() and np.isnan(got.best_traj[~found]).all()
    sparse = engine.plan_fiss(batch, "FISS+", winner=True, traj_sparse=True, enforce=NAMES)
    evs = engine.eval_trajs(batch, ends, dump=True, traj_sparse=True)
    assert same_bits(sparse.best_traj[found], evs.traj[found, 0]) and np.array_equal(sparse.best_flags, got.best_flags)


# ---------------------------------------------------------------- 6. the closed loop
loop_batch = FR.loop_batch


def runner_for(engine, batch, planner="FISS+", **kw):
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch

    return ClosedLoopRunner(engine, DeviceBatch(batch, 0), np.full((batch.B, 2), 1e6), planner=planner, **kw)  # (nobody arrives)


def test_closed_loop_waits_at_the_red_light(engine, oracle):
    cycles = GR.LOOP_CYCLES
    batch, loops = FR.loop_case(oracle, cycles)
    free = runner_for(engine, batch, audit=("gates",)).run(30)
    assert free.violations["gates"].any()  # the unenforced loop drives through the closed gate
    eager = runner_for(engine, batch, enforce=("gates",), audit=("gates",)).run(cycles, record=True)
    graph = runner_for(engine, batch, enforce=("gates",), audit=("gates",)).run_graph(cycles)
    plain = runner_for(engine, batch, enforce=("gates",)).run(cycles)  # one call per cycle, the hand-over inside the refinement's rule instance
    for out in (eager, graph):
        assert not out.violations["gates"].any() and not out.violation_counts.any()
    for out in (graph, plain):
        for k in ("ego", "t_now", "done", "cycles"):
            assert same_bits(getattr(out, k), getattr(eager, k)), k
    assert np.array_equal(plain.rejected, eager.rejected) and np.array_equal(graph.rejected, eager.rejected)
    log = eager.log
    assert (log.n_rows == cycles).all() and (eager.done == 0).all()
    for b in range(batch.B):
        rows = log.rows[b, :cycles]
        s_before = np.concatenate(([batch.ego[b, 0]], rows[:-1, _abi.LOG_S]))
        planned = np.where(np.isfinite(rows[:, _abi.LOG_COST]), 0, -1)  # (a refined plan has no lattice index: a plan is a cost)
        GR.check_loop_invariants(batch, b, rows[:, _abi.LOG_TIME_STEP].astype(np.int64), planned, s_before + batch.gate_front,
                                 rows[:, _abi.LOG_S] + batch.gate_front, GR.OPEN_STEPS[b])
        # the driven states are the CPU reference loop's (up to a cycle the reference could not decide: the loops may part there)
        ref = loops[b]
        n = next((i for i, r in enumerate(ref) if r.undecided), len(ref))
        assert n >= cycles - 1, (b, n)
        ego = rows[:n][:, [_abi.LOG_S, _abi.LOG_VELOCITY, _abi.LOG_S_DD, _abi.LOG_D, _abi.LOG_VELOCITY_Y, _abi.LOG_D_DD]]
        assert np.abs(ego - np.array([r.ego for r in ref[:n]])).max() <= POS_TOL, (b, np.abs(ego - np.array([r.ego for r in ref[:n]])).max())
    assert np.array_equal(eager.rejected, [sum(r.rejected for r in rows) for rows in loops])


@pytest.mark.parametrize("planner", ["FISS", "FISS+"])
def test_step_with_loop_equals_plan_then_advance(engine, planner):
    """FISS+: the hand-over inside the refinement's rule instance; FISS: the advance kernel behind the pipeline."""
    batch = loop_batch()
    a = runner_for(engine, batch, planner=planner, enforce=("gates",))
    b = runner_for(engine, batch, planner=planner, enforce=("gates",))
    torch, stream = a.db.torch, 0
    for _ in range(3):
        a.step(stream)
        engine.plan_fiss_rules_device(b.db.params, b.fb, b.fopts, b.fio, b.enforce_set, None, b.rejected.data_ptr(), stream)
        engine.advance_device(b.db.params, b.fb, b.io, end_state=b.end_state.data_ptr())
    torch.cuda.synchronize(a.db.dev)
    for x, y in ((a.db.t["ego"], b.db.t["ego"]), (a.db.t["t_now"], b.db.t["t_now"]), (a.done, b.done), (a.cycles, b.cycles), (a.cart, b.cart),
                 (a.end_state, b.end_state), (a.stats, b.stats), (a.best_cost, b.best_cost), (a.rejected, b.rejected), (a.prev, b.prev)):
        assert same_bits(x.cpu().numpy(), y.cpu().numpy())
    assert (a.cycles.cpu().numpy() == 3).all()


# ---------------------------------------------------------------- 7. a second call
def test_second_call_on_resident_data(engine):
    batch = case("small")
    dev = Resident(engine, batch, "FISS+", NAMES)
    dev.call()
    first = dev.fetch()
    dev.prev.fill_(-1)  # (prev_best_idx is in / out: passed fresh)
    dev.call()
    second = dev.fetch()
    for k in OUT_KEYS:
        assert same_bits(first[k], second[k]), k
    assert np.array_equal(second["rejected"], 2 * first["rejected"]) and first["rejected"].any()  # in / out: the call adds


# ---------------------------------------------------------------- 8. errors through the ABI
def raw_call(engine, batch, rule_set, loop=None, mem=_abi.FP_MEM_HOST, R=3):
    B = batch.B
    out = engine.fiss_outputs(B, R)
    out.prev_best_idx[...] = -1
    io = _abi.FpFissIo()
    io.samp_min, io.samp_max, io.samp_res = (np.ascontiguousarray(getattr(batch, k)).ctypes.data for k in ("samp_min", "samp_max", "samp_res"))
    for k in ("prev_best_idx", "best_ijk", "best_cost", "end_state", "refined", "stats"):
        setattr(io, k, getattr(out, k).ctypes.data)
    opts = _abi.FpFissOpts(_abi.FP_FISS_PLUS, R, 10.0, 0.5)
    p, fb = host_structs(batch)
    return engine._lib.fp_plan_fiss_rules(engine._ctx, C.byref(p), C.byref(fb), C.byref(opts), C.byref(io), None if rule_set is None else C.byref(rule_set),
                                          None if loop is None else C.byref(loop), None, mem, None)


def test_errors_and_the_call_counter(engine):
    batch = case("small")
    held = {}

    def addr(k):
        held[k] = np.ascontiguousarray(rules.array(batch, k))
        return held[k].ctypes.data

    rs, structs = rules.rule_set(batch, addr, NAMES)
    n0 = engine.get_option("fiss_rules_calls")
    engine.plan_fiss(batch, "FISS+")
    assert engine.get_option("fiss_rules_calls") == n0  # fp_plan_fiss does not count
    assert raw_call(engine, batch, _abi.FpRuleSet()) == -1 and b"every rule" in engine._lib.fp_last_error()
    assert raw_call(engine, batch, None) == -1
    loop = _abi.FpLoopIo()
    assert raw_call(engine, batch, rs, loop=loop) == -1 and b"FP_MEM_DEVICE" in engine._lib.fp_last_error()
    assert engine.get_option("fiss_rules_calls") == n0  # refused before anything ran
    assert raw_call(engine, batch, rs) == 0 and engine.get_option("fiss_rules_calls") == n0 + 1
    with pytest.raises(_abi.FrenetGpuError, match="fp_boundary_mask: margin"):
        engine.plan_fiss(dataclasses.replace(batch, bound_margin=-1.0), "FISS+", enforce=("boundary",))
    # the LDS limit of the refinement's rule instances: 1024 knots carry 72 KB of spline and 40 KB of limits and corridor; with the 12 KB of
    # pose scratch and 38 KB of pair table (60 rows x 40 obstacles) the refinement alone fits a workgroup, with the rules' tables it does not
    big = with_rules(synth.make_batch(2, 5, 5, 5, 40, 120, True, 4716, kind="FISS+", n_knots=_abi.FP_MAX_KNOTS))
    assert (engine.plan_fiss(big, "FISS+").best_ijk[:, 0] >= -1).all()
    with pytest.raises(_abi.FrenetGpuError, match="bytes of LDS") as err:
        engine.plan_fiss(big, "FISS+", enforce=NAMES)
    assert err.value.code == -4
    # without refinement rounds there is nothing to fit: the call runs, and is the host walk over the masked tables
    coarse = engine.plan_fiss(big, "FISS+", max_refine_iters=0, enforce=NAMES)
    ijk, stats, _, _, _ = host_walk(big, engine.plan_dense(big, tables=True, **{n: True for n in NAMES}), "FISS+", np.full((big.B, 3), -1, dtype=np.int32))
    assert np.array_equal(coarse.best_ijk, ijk) and np.array_equal(coarse.stats, stats)


# ---------------------------------------------------------------- 9. the recorded outputs
def test_outputs_are_the_recorded_ones(engine):
    """Every output of the calls of tests/fiss_rules_parent.py, exactly as the library recorded them before the refinement's rule
    instance took its rule evaluation from frenet_rules.h (tests/golden/fiss_rules_parent.npz)."""
    want = np.load(os.path.join(GOLDEN, "fiss_rules_parent.npz"))
    got = fiss_rules_parent.run_all(engine)
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k], equal_nan=got[k].dtype.kind == "f"), k
