"""GPU: fp_fallback_stop (a stopping manoeuvre for the egos without a plan) against its restatement (tests/fallback_ref.py) on the
fixtures of tests/fallback_cases.py - every output exact on every counted ego, hit_speed within 1e-9 (tests/test_fallback_cpu.py shows
that the fixtures reach their paths and that at most one ego per fixture is left out); then the memory modes, the launch order and a
second call bit for bit, the egos that need none, the cross-checks against fp_traj_margins / fp_eval_trajs / fp_advance, plan_dense /
plan_fiss(fallback=), the refusals, the launch counter, the closed-loop scenario and the drop-in classes."""
import ctypes as C
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

import fallback_cases as FC
import fallback_ref as FR
from fiss_plus_planner_amd import _abi, synth
from fiss_plus_planner_amd.engine import host_structs
from fiss_plus_planner_amd.fallback import FallbackStop

pytestmark = pytest.mark.gpu

OUTS = ("end_state", "status", "fb_idx", "hit_step", "hit_obs", "hit_speed", "cand", "counts")


def stop_of(c):
    return FallbackStop(c.stop_T, c.d_targets, c.max_decel)


def host(engine, c, **kw):
    """engine.fallback_stop (FP_MEM_HOST) on a fixture."""
    kw.setdefault("best_idx", c.best_idx)
    return engine.fallback_stop(c.batch, stop_of(c), cand=True, skip=c.skip, **kw)


def device(engine, c, order=None, best_idx=True, end_state=None):
    """fp_fallback_stop(FP_MEM_DEVICE) on a fixture: resident batch and arrays, one launch, read back.  order: fp_batch.launch_order."""
    import torch

    from fiss_plus_planner_amd.device_batch import DeviceBatch

    db = DeviceBatch(c.batch, order_hint=False)
    dev, B = db.dev, c.batch.B
    fs = stop_of(c)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    held = {}

    def addr(name, a):
        held[name] = up(a)
        return held[name].data_ptr()

    st = fs.struct(c.batch, addr)
    F = st.n_d * st.n_stop
    p = _abi.FpParams.from_buffer_copy(db.params)
    pts = max(fs.points_max(c.batch.tick_t), int(p.points_max))
    p.points_max = min(pts, _abi.FP_MAX_POINTS) if pts > _abi.FP_FAST_POINTS else 0
    fb = _abi.FpBatch.from_buffer_copy(db.fb)
    if c.skip is not None:
        held["skip"] = up(c.skip)
        fb.skip = held["skip"].data_ptr()
    if order is not None:
        held["order"] = up(np.asarray(order, dtype=np.int32))
        fb.launch_order = held["order"].data_ptr()
    t = dict(end_state=up(np.full((B, 3), np.nan) if end_state is None else end_state), status=up(np.full(B, -7, dtype=np.int32)), fb_idx=up(np.full(B, -7, dtype=np.int32)),
             hit_step=up(np.full(B, -7, dtype=np.int32)), hit_obs=up(np.full(B, -7, dtype=np.int32)), hit_speed=up(np.full(B, -7.0)),
             cand=up(np.full((B, F), -3, dtype=np.int32)), counts=up(np.zeros((B, 4), dtype=np.int32)))
    bi = up(c.best_idx) if best_idx else None
    engine.fallback_stop_device(p, fb, st, t["end_state"].data_ptr(), t["status"].data_ptr(), t["fb_idx"].data_ptr(), t["hit_step"].data_ptr(), t["hit_obs"].data_ptr(),
                                t["hit_speed"].data_ptr(), best_idx=bi.data_ptr() if best_idx else 0, cand=t["cand"].data_ptr(), counts=t["counts"].data_ptr(),
                                stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return SimpleNamespace(**{k: v.cpu().numpy() for k, v in t.items()})


def same_bits(a, b, what):
    for k in OUTS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


def assert_matches(got, ref, what):
    """Every output exact on the counted egos (hit_speed within SPEED_TOL); the egos that need none are always compared."""
    ok = ref.counted
    assert (ref.need & ~ok).sum() <= FR.MAX_LEFT_OUT, what
    print(f"{what}: status {got.status.tolist()} fb_idx {got.fb_idx.tolist()} hit_step {got.hit_step.tolist()} hit_obs {got.hit_obs.tolist()}, "
          f"{int((ref.need & ok).sum())} of {int(ref.need.sum())} fallback egos compared")
    for k in ("status", "fb_idx", "hit_step", "hit_obs", "cand", "counts"):
        assert np.array_equal(getattr(got, k)[ok], getattr(ref, k)[ok]), (what, k, getattr(got, k)[ok].tolist(), getattr(ref, k)[ok].tolist())
    assert np.array_equal(got.end_state[ok], ref.end_state[ok], equal_nan=True), (what, got.end_state, ref.end_state)
    assert np.array_equal(np.isnan(got.hit_speed[ok]), np.isnan(ref.hit_speed[ok])), what
    hit = ok & ~np.isnan(ref.hit_speed)
    err = np.abs(got.hit_speed[hit] - ref.hit_speed[hit])
    print(f"{what}: max |hit_speed - ref| = {err.max() if err.size else 0.0:.3e}")
    assert (err <= FR.SPEED_TOL).all(), (what, err)


@pytest.mark.parametrize("name", sorted(FC.FIXTURES))
def test_fixtures_against_the_reference(engine, oracle, name):
    c, ref = FC.case(name), FC.reference(oracle, name)
    got = host(engine, c)
    assert_matches(got, ref, name)
    assert (got.cand[~ref.need] == -3).all()  # (the sentinel of the rows nobody may touch)


@pytest.mark.parametrize("name", ["base", "many poses", "off LDS", "rings"])
def test_memory_modes_launch_order_and_a_second_call_give_the_same_bits(engine, oracle, name):
    c = FC.case(name)
    h = host(engine, c)
    d = device(engine, c)
    same_bits(h, d, f"{name}: host / device")
    same_bits(d, device(engine, c, order=np.arange(c.batch.B)[::-1]), f"{name}: reversed launch order")
    same_bits(d, device(engine, c), f"{name}: second call")


def test_largest_family_and_one_more(engine, oracle):
    """F = FP_MAX_FALLBACK = 64 lateral targets x 4 stop times against the reference (F = 1: the "no obstacles" fixture); F + 1 is FP_ELIMIT."""
    b = FC.case("ties").batch
    c = SimpleNamespace(batch=b, stop_T=FC.STOP_T, d_targets=np.linspace(-0.8, 0.8, 64), max_decel=np.inf, best_idx=np.full(b.B, -1, dtype=np.int32), skip=None)
    ref = FR.fallback(oracle, b, c.stop_T, c.d_targets, c.max_decel, best_idx=c.best_idx)
    got = host(engine, c)
    assert got.cand.shape == (b.B, _abi.FP_MAX_FALLBACK)
    assert_matches(got, ref, "F = 256")
    same_bits(got, device(engine, c), "F = 256: host / device")
    rc, msg = raw(engine, b, n_d=257, n_stop=1, d_targets=np.zeros(257), stop_T=np.array([2.0]))
    assert rc == -4 and "FP_MAX_FALLBACK" in msg


def advance(engine, batch, best_idx=None, end_state=None):
    """fp_advance(FP_MEM_HOST) on copies of the batch's state -> (ego, t_now, done, cycles, cart)."""
    b = dataclasses.replace(batch, ego=batch.ego.copy(), t_now=batch.t_now.copy())
    B = b.B
    done, cycles, goal, cart = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.full((B, 2), 1e6), np.full((B, 3), -7.5)
    io = _abi.FpLoopIo()
    io.ego, io.t_now, io.done, io.cycles, io.goal_xy, io.cart_state = (a.ctypes.data for a in (b.ego, b.t_now, done, cycles, goal, cart))
    p, fb = host_structs(b)
    bi = None if best_idx is None else np.ascontiguousarray(best_idx, dtype=np.int32)
    es = None if end_state is None else np.ascontiguousarray(end_state, dtype=np.float64)
    _abi.check(engine._lib.fp_advance(engine._ctx, C.byref(p), C.byref(fb), None if bi is None else bi.ctypes.data, None if es is None else es.ctypes.data,
                                      C.byref(io), _abi.FP_MEM_HOST, None))
    return b.ego, b.t_now, done, cycles, cart


def test_egos_that_need_none(engine):
    """Every ego has a plan: end_state is the decoded lattice sample bit for bit, fp_advance(end_state) leaves exactly the state
    fp_advance(best_idx) leaves, cand keeps its sentinel; with best_idx NULL the end states are untouched."""
    b = synth.make_batch(8, 3, 3, 2, 10, 60, True, 7111)
    out = engine.plan_dense(b)
    bi = np.where(out.best_idx >= 0, out.best_idx, 4).astype(np.int32)
    c = SimpleNamespace(batch=b, stop_T=FC.STOP_T, d_targets=FC.D3, max_decel=np.inf, best_idx=bi, skip=None)
    for got in (host(engine, c), device(engine, c)):
        assert (got.status == 0).all() and (got.fb_idx == -1).all() and (got.hit_step == -1).all() and (got.hit_obs == -1).all() and np.isnan(got.hit_speed).all()
        assert (got.cand == -3).all() and np.array_equal(got.counts, np.tile([1, 0, 0, 0], (b.B, 1)))
        want = np.array([FR.decode(b, e, int(bi[e])) for e in range(b.B)])
        assert got.end_state.tobytes() == want.tobytes()
        for x, y in zip(advance(engine, b, best_idx=bi), advance(engine, b, end_state=got.end_state)):
            assert x.tobytes() == y.tobytes()
    es = np.arange(24, dtype=np.float64).reshape(8, 3) + 0.5
    for got in (host(engine, c, best_idx=None, end_state=es), device(engine, c, best_idx=False, end_state=es)):
        assert got.end_state.tobytes() == es.tobytes() and (got.status == 0).all() and (got.cand == -3).all()


def test_end_state_says_who_needs_one(engine, oracle):
    """best_idx NULL: a NaN end state needs a fallback, the others keep theirs - against the reference, host and device."""
    c = FC.case("base")
    es = np.tile([0.3, 4.0, 5.0], (c.batch.B, 1))
    es[[0, 2, 3, 7]] = np.nan
    ref = FR.fallback(oracle, c.batch, c.stop_T, c.d_targets, c.max_decel, end_state=es, skip=c.skip)
    got = host(engine, c, best_idx=None, end_state=es)
    assert_matches(got, ref, "base, end_state")
    assert got.end_state[[1, 4, 5, 6]].tobytes() == es[[1, 4, 5, 6]].tobytes()
    same_bits(got, device(engine, c, best_idx=False, end_state=es), "base, end_state: host / device")


@pytest.mark.parametrize("name", ["base", "rings", "off LDS"])
def test_cross_check_against_margins_and_eval_trajs(engine, name):
    """fp_traj_margins(end_state, pose_stride = check_stride) has min_dist == 0 exactly when there is a hit and names the same step and
    column; fp_eval_trajs has FP_FLAG_COLLISION exactly for status CONTACT."""
    c = FC.case(name)
    got = host(engine, c)
    has = got.status != _abi.FALLBACK_NONE
    has &= ~np.isnan(got.end_state[:, 0])
    d, i, j = engine.traj_margins(c.batch, end_state=got.end_state, skip=c.skip)
    fb = np.isin(got.status, (_abi.FALLBACK_CLEAR, _abi.FALLBACK_CONTACT))
    assert fb.any()
    assert np.array_equal(d[fb] == 0.0, got.status[fb] == _abi.FALLBACK_CONTACT)
    hit = got.status == _abi.FALLBACK_CONTACT
    assert np.array_equal(i[hit], got.hit_step[hit]) and np.array_equal(j[hit], got.hit_obs[hit])
    es = np.where(np.isnan(got.end_state), 1.0, got.end_state)  # (an ego without a trajectory prices a dummy; it is not looked at)
    ev = engine.eval_trajs(c.batch, es[:, None, :])
    assert np.array_equal((ev.flags[fb, 0] & _abi.FLAG_COLLISION) != 0, got.status[fb] == _abi.FALLBACK_CONTACT)
    if name != "off LDS":
        assert hit.any()


def test_plan_dense_fallback_behind_a_rule_pass(engine, oracle):
    """Gates 3 m ahead, closed for ever, in front of egos 0, 2 and 5: every candidate of theirs is flagged, best_idx is -1, and exactly
    they get a fallback; everybody else's end state is the masked winner's."""
    import gates_ref as GR

    b = synth.make_batch(8, 3, 3, 2, 6, 60, True, 7112)
    closed = np.zeros((b.F, 4, 1), dtype=bool)
    closed[[0, 2, 5]] = True
    b = GR.with_gates(b, ahead=(3.0,), T_gate=4, closed=closed)
    fs = FallbackStop(FC.STOP_T, FC.D3)
    plain = engine.plan_dense(b, gates=True)
    out = engine.plan_dense(b, gates=True, fallback=fs)
    assert np.array_equal(out.best_idx, plain.best_idx) and np.array_equal(out.flags, plain.flags)
    assert (out.best_idx[[0, 2, 5]] == -1).all() and (out.n_gated[[0, 2, 5]] > 0).all()
    ref = FR.fallback(oracle, b, FC.STOP_T, FC.D3, np.inf, best_idx=out.best_idx)
    ref.cand = None
    got = out.fallback
    got.cand = None
    for k in ("status", "fb_idx", "hit_step", "hit_obs", "counts"):
        assert np.array_equal(getattr(got, k)[ref.counted], getattr(ref, k)[ref.counted]), k
    assert np.array_equal(got.end_state[ref.counted], ref.end_state[ref.counted], equal_nan=True)
    assert np.array_equal(got.status != 0, out.best_idx < 0) and (ref.need & ~ref.counted).sum() <= FR.MAX_LEFT_OUT


def test_plan_fiss_fallback(engine, oracle):
    """FISS+ with a wall in front of ego 0: its end state is NaN, the fallback fills it; the others keep the planner's."""
    b = synth.make_batch(4, 5, 5, 5, 6, 110, True, 7113, kind="FISS+")
    b.ego[0, :3] = (30.0, 9.0, 0.0)
    FC.place(b, 0, 0, 30.0 + 4.0 + 0.5 * b.veh_l + 1.0, 0.0, 2.0, 9.0)
    fs = FallbackStop(FC.STOP_T, FC.D3)
    plain = engine.plan_fiss(b, "FISS+")
    out = engine.plan_fiss(b, "FISS+", fallback=fs)
    assert np.array_equal(out.end_state, plain.end_state, equal_nan=True) and np.isnan(out.end_state[0]).all() and not np.isnan(out.end_state[1:]).all()
    ref = FR.fallback(oracle, b, FC.STOP_T, FC.D3, np.inf, end_state=out.end_state)
    got = out.fallback
    ok = ref.counted
    assert ok[0]
    for k in ("status", "fb_idx", "hit_step", "hit_obs", "counts"):
        assert np.array_equal(getattr(got, k)[ok], getattr(ref, k)[ok]), k
    assert np.array_equal(got.end_state[ok], ref.end_state[ok], equal_nan=True) and got.status[0] == _abi.FALLBACK_CONTACT
    keep = ~np.isnan(out.end_state[:, 0])
    assert got.end_state[keep].tobytes() == out.end_state[keep].tobytes() and (got.status[keep] == 0).all()


def raw(engine, batch, n_d=1, n_stop=1, d_targets=None, stop_T=None, max_decel=np.inf, best_idx=True, null=(), mem=_abi.FP_MEM_HOST, struct=True):
    """fp_fallback_stop through ctypes with every argument in the caller's hands -> (rc, message)."""
    B = batch.B
    d = np.ascontiguousarray(np.zeros(n_d) if d_targets is None else d_targets, dtype=np.float64)
    t = np.ascontiguousarray(np.arange(1, n_stop + 1, dtype=np.float64) if stop_T is None else stop_T, dtype=np.float64)
    st = _abi.FpFallback(n_d, n_stop, None if "d_targets" in null else d.ctypes.data, None if "stop_T" in null else t.ctypes.data, max_decel)
    bi = np.ascontiguousarray(np.full(B, -1) if best_idx is True else best_idx, dtype=np.int32)
    a = dict(end_state=np.full((B, 3), np.nan), status=np.zeros(B, dtype=np.int32), fb_idx=np.zeros(B, dtype=np.int32), hit_step=np.zeros(B, dtype=np.int32),
             hit_obs=np.zeros(B, dtype=np.int32), hit_speed=np.zeros(B))
    ptr = lambda k: None if k in null else a[k].ctypes.data  # noqa: E731
    p, fb = host_structs(batch)
    rc = engine._lib.fp_fallback_stop(engine._ctx, C.byref(p), C.byref(fb), C.byref(st) if struct else None, bi.ctypes.data, ptr("end_state"), ptr("status"),
                                      ptr("fb_idx"), ptr("hit_step"), ptr("hit_obs"), ptr("hit_speed"), None, None, mem, None)
    return rc, engine._lib.fp_last_error().decode(errors="replace")


def test_every_error_of_the_contract(engine):
    b = FC.case("ties").batch
    before = engine.get_option("fallback_launches")
    EINVAL, ELIMIT = -1, -4
    assert raw(engine, b, struct=False)[0] == EINVAL
    for k in ("d_targets", "stop_T", "end_state", "status", "fb_idx", "hit_step", "hit_obs", "hit_speed"):
        assert raw(engine, b, null=(k,))[0] == EINVAL, k
    assert raw(engine, b, n_d=0)[0] == EINVAL and raw(engine, b, n_stop=0)[0] == EINVAL
    assert raw(engine, b, n_d=257, n_stop=1, d_targets=np.zeros(257))[0] == ELIMIT
    assert raw(engine, b, n_d=16, n_stop=17, d_targets=np.zeros(16))[0] == ELIMIT
    for md in (0.0, -1.0, np.nan):
        assert raw(engine, b, max_decel=md)[0] == EINVAL, md
    for bad, entry in (([1.0, np.inf], 1), ([0.0, 1.0], 0), ([1.0, 2.0, 2.0], 2), ([2.0, 1.0], 1), ([np.nan], 0), ([-1.0], 0)):
        rc, msg = raw(engine, b, n_stop=len(bad), stop_T=bad)
        assert rc == EINVAL and f"stop_T[{entry}]" in msg, (bad, msg)
    rc, msg = raw(engine, b, n_stop=2, stop_T=[1.0, 25.7])  # 257 points at tick 0.1
    assert rc == ELIMIT and "stop_T[1]" in msg
    rc, msg = raw(engine, b, best_idx=np.array([-1, b.C, 0, 0]))
    assert rc == EINVAL and "ego 1" in msg
    # (the device-side limits come before any launch too)
    assert raw(engine, b, n_d=257, n_stop=1, d_targets=np.zeros(257), mem=_abi.FP_MEM_DEVICE)[0] == ELIMIT
    assert raw(engine, b, max_decel=0.0, mem=_abi.FP_MEM_DEVICE)[0] == EINVAL
    assert engine.get_option("fallback_launches") == before
    assert raw(engine, b)[0] == 0 and engine.get_option("fallback_launches") == before + 1


def test_fallback_launches_counts_the_kernels_launches():
    """0 for a caller that never asks, one per call afterwards; the other counters do not move."""
    from fiss_plus_planner_amd.engine import FrenetEngine

    c = FC.case("ties")
    with FrenetEngine(0) as eng:
        eng.plan_dense(c.batch)
        eng.traj_margins(c.batch, best_idx=np.zeros(c.batch.B, dtype=np.int32))
        assert eng.get_option("fallback_launches") == 0
        m = eng.get_option("margin_launches")
        host(eng, c)
        device(eng, c)
        assert eng.get_option("fallback_launches") == 2 and eng.get_option("margin_launches") == m


# ---------------------------------------------------------------------------
# the closed-loop scenario
# ---------------------------------------------------------------------------
def _runner(engine, fallback, planner="FOP", **kw):
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch

    batch, goal_xy = FC.loop_scenario()
    return batch, ClosedLoopRunner(engine, DeviceBatch(batch), goal_xy, planner, fallback=fallback, **kw)


def test_loop_scenario(engine, oracle):
    from fiss_plus_planner_amd.closed_loop import LoopLog  # noqa: F401

    ref = FC.loop_reference(oracle)
    batch, plain = _runner(engine, None, fused=False)
    out0 = plain.run(FC.LOOP_CYCLES)
    assert (out0.done == _abi.DONE_NO_SOLUTION).all()  # the need: without a fallback every ego leaves the simulation in front of the wall
    fs = FallbackStop(FC.LOOP_STOP_T)
    _, run = _runner(engine, fs)
    out = run.run(FC.LOOP_CYCLES, record=True)
    assert np.isin(out.done, (_abi.DONE_GOAL, _abi.DONE_END_OF_LINE)).all() and np.array_equal(out.done, ref.done) and np.array_equal(out.cycles, ref.cycles)
    assert (out.fallback_counts[:, 1] > 0).all() and np.array_equal(out.fallback_counts[:, 1:], ref.counts[:, 1:])
    worst = 0.0
    for b in range(batch.B):
        rows = out.log.ego_rows(b)
        assert len(rows) == ref.cycles[b]
        assert (rows[:, _abi.LOG_BEST_IDX] == -1).all()
        got = rows[:, [_abi.LOG_S, _abi.LOG_VELOCITY, _abi.LOG_S_DD, _abi.LOG_D, _abi.LOG_VELOCITY_Y, _abi.LOG_D_DD]]
        want = ref.states[1:ref.cycles[b] + 1, b]
        worst = max(worst, float(np.abs(got - want).max()))
        # never in contact: the wall (2 x 12 m at x = 45, the line is the x axis) stands at the steps < K_OPEN; row r is the ego at step r + 1
        standing = np.arange(len(rows)) + 1 < FC.K_OPEN
        assert standing.any() and (rows[standing, _abi.LOG_X] + 0.5 * batch.veh_l < 44.0).all()
        assert (rows[standing, _abi.LOG_DONE] == _abi.RUNNING).all()  # RUNNING while the wall stands
    print(f"loop: driven states within {worst:.3e} of the CPU reference loop, cycles {out.cycles.tolist()}, fallback counts {out.fallback_counts[:, 1:].tolist()}")
    assert worst <= 1e-8
    # the graph replays the same cycle: bit for bit, with and without the log
    _, g = _runner(engine, fs)
    outg = g.run_graph(FC.LOOP_CYCLES, record=True)
    for k in ("done", "cycles", "ego", "t_now", "cart"):
        assert getattr(outg, k).tobytes() == getattr(out, k).tobytes(), k
    # (column 0 also counts the cycles enqueued behind an ego's last one: the eager loop stops polling, the graph replays them all)
    assert np.array_equal(outg.fallback_counts[:, 1:], out.fallback_counts[:, 1:]) and (outg.fallback_counts.sum(axis=1) == FC.LOOP_CYCLES).all()
    for b in range(batch.B):
        assert outg.log.ego_rows(b).tobytes() == out.log.ego_rows(b).tobytes()
    _, e = _runner(engine, fs)
    oute = e.run(FC.LOOP_CYCLES)
    _, g2 = _runner(engine, fs)
    outg2 = g2.run_graph(FC.LOOP_CYCLES)
    for k in ("done", "cycles", "ego", "t_now", "cart"):
        assert getattr(oute, k).tobytes() == getattr(out, k).tobytes() and getattr(outg2, k).tobytes() == getattr(out, k).tobytes(), k


def test_loop_runner_refusals_and_fiss(engine):
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch

    fs = FallbackStop(FC.LOOP_STOP_T)
    b = synth.make_batch(4, 5, 5, 5, 6, 110, True, 7113, kind="FISS+")
    b.speed_limit = np.full((b.F, b.NX), 40.0)
    with pytest.raises(ValueError, match="not done"):
        ClosedLoopRunner(engine, DeviceBatch(b), np.full((4, 2), 1e6), "FISS+", audit=("envelope",), fallback=fs)
    b.ego[0, :3] = (30.0, 9.0, 0.0)
    FC.place(b, 0, 0, 30.0 + 4.0 + 0.5 * b.veh_l + 1.0, 0.0, 2.0, 9.0)
    for kw in ({}, {"enforce": ("envelope",)}):
        plain = ClosedLoopRunner(engine, DeviceBatch(dataclasses.replace(b, ego=b.ego.copy(), t_now=b.t_now.copy())), np.full((4, 2), 1e6), "FISS+", fused=False, **kw).run(3)
        out = ClosedLoopRunner(engine, DeviceBatch(dataclasses.replace(b, ego=b.ego.copy(), t_now=b.t_now.copy())), np.full((4, 2), 1e6), "FISS+", fallback=fs, **kw).run(3)
        assert plain.done[0] == _abi.DONE_NO_SOLUTION and out.done[0] == _abi.RUNNING and out.cycles[0] == 3
        assert out.fallback_counts[0, 1:].sum() == 3 and out.fallback_counts[1:, 0].sum() + out.fallback_counts[1:, 1:].sum() == 9
        same = plain.done[1:] == _abi.RUNNING
        # the egos with a plan drive what they drove before (enforce=: the plain runner hands over inside the refinement launch, this one by fp_advance)
        if kw:
            assert np.allclose(out.ego[1:][same], plain.ego[1:][same], rtol=0, atol=1e-9)
        else:
            assert out.ego[1:][same].tobytes() == plain.ego[1:][same].tobytes()


# ---------------------------------------------------------------------------
# the drop-in classes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["FOP", "FISS+"])
def test_drop_in_classes(engine, kind):
    from test_gpu_planners import _inputs, _planner

    b = synth.make_batch(2, 5, 5, 5, 6, 110, True, 7113, kind=kind)
    b.ego[0] = (30.0, 9.0, 0.0, 0.1, 0.0, 0.0)
    for j in range(b.n_obs):
        b.obs_pose[0, :, j, 3] = 0.0
    FC.place(b, 0, 0, 30.0 + 12.0 + 0.5 * b.veh_l + 1.0, 0.0, 2.0, 9.0)
    pts, fs, obs = _inputs(b, 0)
    pl = _planner(kind, b, engine)
    pl.generate_frenet_frame(pts)
    assert pl.plan(fs, float(b.target_speed[0]), obs, 0) is None and not hasattr(pl, "fallback_info")  # as before
    stop = FallbackStop(FC.STOP_T, FC.D3)
    pl.set_fallback(stop)
    tr = pl.plan(fs, float(b.target_speed[0]), obs, 0)
    assert tr is not None and tr.is_fallback and pl.fallback_info.status == _abi.FALLBACK_CLEAR and pl.fallback_info.hit_step == -1
    assert np.isnan(pl.fallback_info.hit_speed)
    one = pl._batch_cache[1]  # (the planner's own B = 1 batch of this plan() call)
    r = engine.fallback_stop(one, stop, best_idx=np.array([-1], dtype=np.int32))
    assert r.fb_idx[0] == pl.fallback_info.fb_idx
    ev = engine.eval_trajs(one, r.end_state[:, None, :], dump=True)
    N = int((ev.flags[0, 0] >> _abi.FLAG_N_SHIFT) & 0xFFF)
    for row, name in ((0, "t"), (1, "s"), (2, "s_d"), (5, "d"), (9, "x"), (10, "y")):
        want = ev.traj[0, 0, row]
        want = want[~np.isnan(want)][:N]
        assert np.asarray(getattr(tr, name)).tobytes() == want.tobytes(), name
    assert tr.s_d[-1] < 0.2 * tr.s_d[0] and (tr.end_state.d, tr.end_state.s_d, tr.end_state.t) == tuple(r.end_state[0])
    pl.set_fallback(None)
    assert pl.plan(fs, float(b.target_speed[0]), obs, 0) is None
    # an ego with a plan is not touched
    pts, fs, obs = _inputs(b, 1)
    pl2 = _planner(kind, b, engine)
    pl2.generate_frenet_frame(pts)
    pl2.set_fallback(stop)
    tr2 = pl2.plan(fs, float(b.target_speed[1]), obs, 0)
    assert tr2 is not None and not tr2.is_fallback and not hasattr(pl2, "fallback_info")
