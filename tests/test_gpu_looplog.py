"""GPU: the device-side log of a resident closed loop (fp_loop_record, ABI 17).  The recorder only copies what a step left in its
arrays, so every comparison with the host-traced loop (ClosedLoopRunner.run(trace=True): five blocking read-backs per cycle) and
with the numpy bookkeeping reference (tests/looplog_ref.py) is exact - no tolerance anywhere except where the drop-in planner
classes are the other side (the demo-scenario test's own 1e-6)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import looplog_ref as R
from conftest import load_golden
from fiss_plus_planner_amd import _abi, synth
from test_gpu_closed_loop_device import _flensburg_batch

pytestmark = pytest.mark.gpu

FRENET_COLS = [R.S, R.VELOCITY, R.S_DD, R.D, R.VELOCITY_Y, R.D_DD]   # a row's Frenet state in fp_batch.ego order
MODES = [("FOP", True), ("FOP", False), ("FISS", True), ("FISS+", True), ("FISS+", False)]


def _fixture(which, kind):
    """(batch, goal, cycles): the fixtures of tests/test_gpu_closed_loop_device.py - G5 (Flensburg, three copies, reaches the goal after
    44 cycles) and a synthetic batch of different egos (48: not a multiple of 64; some finish, FISS kinds run out of solutions)."""
    if which == "g5":
        g = load_golden("g5_closed_loop.npz")
        return _flensburg_batch(g, kind, copies=3), np.tile(g["goal_center"], (3, 1)), 100
    batch = synth.make_batch(48, 5, 5, 5, 10, 100, False, 62, kind=kind)
    return batch, np.stack([batch.coef[:, 0, 30], batch.coef[:, 4, 30]], axis=1), 14


def _runner(engine, which, kind, fused=True):
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch

    batch, goal, cycles = _fixture(which, kind)
    return ClosedLoopRunner(engine, DeviceBatch(batch, 0), goal, kind, fused=fused), batch, cycles


def _assert_logs_equal(a, b):
    for k in ("rows", "n_rows", "row_stats", "stats_sum", "sealed"):
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), k


@pytest.mark.parametrize("which", ["g5", "synth"])
@pytest.mark.parametrize("kind,fused", MODES)
def test_log_equals_the_host_trace_bit_for_bit(engine, which, kind, fused):
    run_t, batch, cycles = _runner(engine, which, kind, fused)
    t0 = batch.t_now.copy()
    tr = run_t.run(cycles, trace=True)
    run_r, _, _ = _runner(engine, which, kind, fused)
    rec = run_r.run(cycles, record=True)
    log = rec.log
    for k in ("done", "cycles", "t_now"):
        np.testing.assert_array_equal(getattr(rec, k), getattr(tr, k), err_msg=k)
    assert np.array_equal(rec.ego, tr.ego) and np.array_equal(rec.cart, tr.cart, equal_nan=True)
    B = batch.B
    n = np.zeros(B, dtype=int)
    ssum = np.zeros((B, 4), dtype=np.int64)
    running = np.ones(B, dtype=bool)
    for i, row in enumerate(tr.trace):
        nxt = tr.trace[i + 1].start if i + 1 < len(tr.trace) else tr.ego
        for b in np.nonzero(running)[0]:
            ssum[b] += row.stats[b]
            if row.done[b] != _abi.DONE_NO_SOLUTION:   # the ego moved: one row
                r = log.rows[b, n[b]]
                assert np.array_equal(r[R.X:R.YAW + 1], row.cart[b]), (b, i)
                assert np.array_equal(r[FRENET_COLS], nxt[b]), (b, i)
                assert r[R.TIME_STEP] == t0[b] + n[b] and r[R.COST] == row.cost[b] and r[R.DONE] == row.done[b], (b, i)
                assert np.array_equal(log.row_stats[b, n[b]], row.stats[b]), (b, i)
                assert (r[R.BEST_IDX] >= 0) == (kind == "FOP") and np.isfinite(r[R.D_END:R.T_END + 1]).all(), (b, i)
                n[b] += 1
        running &= row.done == 0
    np.testing.assert_array_equal(log.n_rows, tr.cycles)
    np.testing.assert_array_equal(n, tr.cycles)
    np.testing.assert_array_equal(log.stats_sum, ssum)
    np.testing.assert_array_equal(log.sealed, (tr.done != 0).astype(np.int32))
    for b in range(B):
        assert np.isnan(log.rows[b, n[b]:]).all()       # nothing beyond an ego's rows was touched
        assert np.array_equal(log.states(b), log.rows[b, :n[b], R.X:R.YAW + 1]) and log.states(b).shape == (n[b], 3)
    assert tr.cycles.sum() > B and (which != "g5" or (tr.done == _abi.DONE_GOAL).all())


def _snapshot(run):
    fop = run.planner == "FOP"
    g = lambda t: t.cpu().numpy().copy()
    return SimpleNamespace(ego=g(run.db.t["ego"]), t_now=g(run.db.t["t_now"]), done=g(run.done), cycles=g(run.cycles), cart=g(run.cart),
                           best_cost=g(run.best_cost), stats=g(run.stats), best_idx=g(run.best_idx) if fop else None,
                           end_state=None if fop else g(run.end_state))


@pytest.mark.parametrize("kind", ["FOP", "FISS+"])
def test_log_equals_the_bookkeeping_reference_cycle_by_cycle(engine, kind):
    """The per-cycle snapshots of the loop fed to tests/looplog_ref.py: every array of the log after every cycle, sealed and n_running
    included.  max_rows is smaller than the cycles driven, so the overflow rule is part of it."""
    import torch

    run, batch, cycles = _runner(engine, "synth", kind)
    max_rows = 9
    run.log_reset(max_rows)
    ref = R.LoopLogRef(batch.B, max_rows)
    for i in range(cycles):
        run.step()
        run.record()
        torch.cuda.synchronize()
        ref.record(_snapshot(run), batch.d_samples, batch.v_samples, batch.t_samples)
        log = run.log_fetch()
        _assert_logs_equal(log, ref)
        assert int(run.log_running.item()) == ref.n_running, i
    assert (ref.n_rows > max_rows).any() and (ref.sealed == 0).any()


@pytest.mark.parametrize("kind", ["FOP", "FISS+"])
def test_graph_replay_records_the_same_log(engine, kind):
    """A captured [step, record] pair replayed: the row index lives on the device, so every replay appends to the log."""
    outs = []
    for use_graph in (False, True):
        run, _, _ = _runner(engine, "synth", kind)
        outs.append(run.run_graph(9, record=True) if use_graph else run.run(9, record=True))
    a, b = outs
    _assert_logs_equal(a.log, b.log)
    for k in ("done", "cycles", "t_now", "ego"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)
    assert (a.log.n_rows > 1).any() and np.array_equal(a.log.n_rows, a.cycles)


@pytest.mark.parametrize("kind", ["FISS", "FISS+"])
def test_result_from_log_agrees_with_the_drop_in_planner_classes(engine, kind):
    """A demo scenario (tests/golden/g11_demo_scenarios.npz) driven twice: by the drop-in planner class through run_closed_loop (one
    plan() per cycle through the host ABI) and by the resident device loop with a log.  result_from_log(...).states against
    run_closed_loop(...).states, compared as tests/test_gpu_demo_scenarios.py compares states (1e-6)."""
    from fiss_plus_planner_amd import planners as P
    from fiss_plus_planner_amd.closed_loop import result_from_log, run_closed_loop
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch
    from fiss_plus_planner_amd.frenet import FrenetState
    from fiss_plus_planner_amd.obstacles import ObstacleTable
    from fiss_plus_planner_amd.vehicle import Vehicle

    g = load_golden("g11_demo_scenarios.npz")
    name = str(g["names"][0])
    cls, st = {"FISS": (P.FissPlanner, P.FissPlannerSettings), "FISS+": (P.FissPlusPlanner, P.FissPlusPlannerSettings)}[kind]
    fts = int(g[f"{name}_final_time_step"])
    max_speed = float(g[f"{name}_max_speed"])
    centerline, init, goal = g[f"{name}_centerline"], g[f"{name}_init_state"], g[f"{name}_goal_center"]
    want = run_closed_loop(cls(st(5, 5, 5), Vehicle(), None, engine=engine), centerline, init,
                           ObstacleTable(g[f"{name}_obs_pose"], g[f"{name}_obs_dims"], fts), goal, max_speed=max_speed)
    # the same problem as a resident batch of one ego: the planner class's own marshalling of its first cycle
    pl = cls(st(5, 5, 5), Vehicle(), None, engine=engine, cache_tables=False)
    sp, _ = pl.generate_frenet_frame(centerline)
    e = engine.from_state(sp.knots[None], sp.coef[None], [len(sp.knots)], [0], np.asarray(init, dtype=np.float64)[None, :4])[0]
    pl.settings.highest_speed = max_speed
    batch = pl._make_batch(FrenetState(t=0.0, s=e[0], s_d=e[1], s_dd=e[2], d=e[3], d_d=e[4], d_dd=e[5]),
                           ObstacleTable(g[f"{name}_obs_pose"], g[f"{name}_obs_dims"], fts), 0)
    out = ClosedLoopRunner(engine, DeviceBatch(batch, 0), np.asarray(goal, dtype=np.float64)[None, :2], kind).run(fts, record=True)
    got = result_from_log(out.log, 0, start=e)
    assert len(got.states) == len(want.states) >= 40 and len(got.cycles) == len(want.cycles)
    np.testing.assert_allclose(np.array(got.states), np.array(want.states), rtol=0, atol=1e-6)
    assert got.goal_reached == want.goal_reached
    assert [c.stats for c in got.cycles] == [c.stats for c in want.cycles]
    assert got.stats.as_tuple() == want.stats.as_tuple()
    np.testing.assert_allclose([c.start for c in got.cycles], [c.start for c in want.cycles], rtol=0, atol=1e-6)


# ---- the entry point on its own: hand-made loop states, device and host arrays ----------------------------------------------------
GUARD = 97


class _Direct:
    """fp_loop_record called directly on hand-made loop arrays (it only copies: no plan needed).  mem = device: torch tensors with guard
    words behind rows / row_stats; host: numpy arrays."""

    def __init__(self, engine, B, max_rows, device=True, done=None, seed=5):
        import torch

        from fiss_plus_planner_amd.device_batch import DeviceBatch
        from fiss_plus_planner_amd.engine import _host_batch, make_params

        self.eng, self.B, self.max_rows, self.device = engine, B, max_rows, device
        self.batch = synth.make_batch(B, 5, 5, 5, 4, 20, False, seed)
        self.rng = np.random.default_rng(seed)
        self.h = SimpleNamespace(ego=np.zeros((B, 6)), t_now=np.array(self.rng.integers(0, 5, B), dtype=np.int32), cycles=np.zeros(B, dtype=np.int32),
                                 done=np.zeros(B, dtype=np.int32) if done is None else np.array(done, dtype=np.int32), cart=np.full((B, 3), np.nan),
                                 best_idx=np.full(B, -1, dtype=np.int32), end_state=None, best_cost=np.full(B, np.nan), stats=np.zeros((B, 4), dtype=np.int32))
        self.rows = np.full(B * max_rows * 16 + GUARD, -7.25)
        self.row_stats = np.full(B * max_rows * 4 + GUARD, -77, dtype=np.int32)
        self.n_rows, self.sealed = np.zeros(B, dtype=np.int32), (self.h.done != 0).astype(np.int32)
        self.stats_sum, self.n_running = np.zeros((B, 4), dtype=np.int64), np.full(1, -1, dtype=np.int32)
        self.ref = R.LoopLogRef(B, max_rows, done=self.h.done)
        self.ref.rows[:] = -7.25
        self.ref.row_stats[:] = -77
        if device:
            self.db = DeviceBatch(self.batch, 0)
            self.fb, self.params = self.db.fb, self.db.params
            self.t = {k: torch.from_numpy(v).to(self.db.dev) for k, v in (("rows", self.rows), ("row_stats", self.row_stats), ("n_rows", self.n_rows),
                                                                         ("sealed", self.sealed), ("stats_sum", self.stats_sum), ("n_running", self.n_running))}
        else:
            self.fb, self.params = _host_batch(self.batch), make_params(self.batch)

    def move(self, use_end_state=False):
        """one made-up step: running egos move (most of them), some finish, some find no solution"""
        h, B = self.h, self.B
        for b in range(B):
            if h.done[b] != 0:
                continue
            h.stats[b] = self.rng.integers(1, 200, 4)
            u = self.rng.random()
            if u < 0.08:
                h.done[b] = _abi.DONE_NO_SOLUTION
                h.best_idx[b], h.best_cost[b] = -1, np.nan
                continue
            h.ego[b] = self.rng.normal(size=6)
            h.cart[b] = self.rng.normal(size=3)
            h.t_now[b] += 1
            h.cycles[b] += 1
            h.best_idx[b] = self.rng.integers(0, 125)
            h.best_cost[b] = self.rng.random()
            if u > 0.9:
                h.done[b] = int(self.rng.integers(1, 5))
                h.done[b] = _abi.DONE_GOAL if h.done[b] == _abi.DONE_NO_SOLUTION else h.done[b]
        h.end_state = self.rng.normal(size=(B, 3)) if use_end_state else None

    def call(self, mem=None, **over):
        """-> rc.  over: replace an argument (io / log fields by name, or best_idx / end_state / best_cost / stats)"""
        import torch

        h = self.h
        mem = (_abi.FP_MEM_DEVICE if self.device else _abi.FP_MEM_HOST) if mem is None else mem
        if self.device:
            self.keep = {k: torch.from_numpy(np.ascontiguousarray(v)).to(self.db.dev) for k, v in vars(h).items() if v is not None}
            ptr = lambda k: self.keep[k].data_ptr() if k in self.keep else None
            lp = lambda k: self.t[k].data_ptr()
        else:
            ptr = lambda k: getattr(h, k).ctypes.data if getattr(h, k) is not None else None
            lp = lambda k: getattr(self, k).ctypes.data
        io = _abi.FpLoopIo()
        io.ego, io.t_now, io.done, io.cycles, io.cart_state = ptr("ego"), ptr("t_now"), ptr("done"), ptr("cycles"), ptr("cart")
        lg = _abi.FpLoopLog()
        lg.max_rows = self.max_rows
        lg.rows, lg.row_stats, lg.n_rows, lg.sealed, lg.stats_sum, lg.n_running = (lp(k) for k in ("rows", "row_stats", "n_rows", "sealed", "stats_sum", "n_running"))
        args = dict(best_idx=None if h.end_state is not None else ptr("best_idx"), end_state=ptr("end_state"), best_cost=ptr("best_cost"), stats=ptr("stats"))
        io_p, lg_p = C.byref(io), C.byref(lg)
        for k, v in over.items():
            if k in args:
                args[k] = v
            elif k == "io":
                io_p = v
            elif k == "log":
                lg_p = v
            elif hasattr(_abi.FpLoopLog, k) and k in [f[0] for f in _abi.FpLoopLog._fields_]:
                setattr(lg, k, v)
            else:
                setattr(io, k, v)
        rc = self.eng._lib.fp_loop_record(self.eng._ctx, C.byref(self.params), C.byref(self.fb), io_p, args["best_idx"], args["end_state"],
                                          args["best_cost"], args["stats"], lg_p, mem, None)
        if self.device:
            torch.cuda.synchronize()
        return rc

    def record_and_check(self):
        h = self.h
        assert self.call() == 0, self.eng._lib.fp_last_error()
        snap = {k: (None if v is None else v.copy()) for k, v in vars(h).items()}
        if h.end_state is not None:
            snap["best_idx"] = None   # (the call passes exactly one of the two)
        self.ref.record(SimpleNamespace(**snap), self.batch.d_samples, self.batch.v_samples, self.batch.t_samples)
        get = (lambda k: self.t[k].cpu().numpy()) if self.device else (lambda k: getattr(self, k))
        n = self.B * self.max_rows
        rows, row_stats = get("rows"), get("row_stats")
        assert np.array_equal(rows[:n * 16].reshape(self.B, self.max_rows, 16), self.ref.rows, equal_nan=True)
        assert np.array_equal(row_stats[:n * 4].reshape(self.B, self.max_rows, 4), self.ref.row_stats)
        assert (rows[n * 16:] == -7.25).all() and (row_stats[n * 4:] == -77).all()      # the guard words behind the arrays
        for k in ("n_rows", "sealed", "stats_sum"):
            np.testing.assert_array_equal(get(k), getattr(self.ref, k), err_msg=k)
        assert int(get("n_running")[0]) == self.ref.n_running


@pytest.mark.parametrize("B", [1, 70, 333])
@pytest.mark.parametrize("device", [True, False])
def test_record_on_hand_made_steps(engine, B, device):
    """B = 1, B not a multiple of 64, device and FP_MEM_HOST arrays; max_rows (3) smaller than the cycles driven (8): rows past the end
    are counted, nothing is written behind the arrays; lattice indices and explicit end states; egos finished before the first step stay
    sealed with 0 rows; an ego without a solution in its first cycle adds Stats and no row."""
    done0 = np.zeros(B, dtype=np.int32)
    done0[B // 2::7] = _abi.DONE_GOAL if B > 1 else 0
    d = _Direct(engine, B, 3, device=device, done=done0, seed=10 + B)
    n0 = engine.get_option("looplog_launches")
    for k in range(8):
        d.move(use_end_state=(k % 3 == 2))
        if k == 0 and B > 1:   # no solution in cycle 0 for ego 1 (whatever move() drew for it)
            h = d.h
            if h.cycles[1] == 1:
                h.cycles[1], h.t_now[1] = 0, h.t_now[1] - 1
            h.done[1], h.best_idx[1], h.best_cost[1] = _abi.DONE_NO_SOLUTION, -1, np.nan
            stats1 = h.stats[1].copy()
        d.record_and_check()
    assert engine.get_option("looplog_launches") == n0 + 8
    assert (d.ref.n_rows[done0 != 0] == 0).all() and (d.ref.stats_sum[done0 != 0] == 0).all()
    if B > 1:
        assert d.ref.n_rows[1] == 0 and d.ref.sealed[1] == 1 and np.array_equal(d.ref.stats_sum[1], stats1) and stats1.sum() > 0
        assert (d.ref.n_rows > 3).any()


@pytest.mark.parametrize("device", [True, False])
def test_every_einval_case(engine, device):
    d = _Direct(engine, 5, 2, device=device)
    d.move()
    lib = engine._lib
    bad_batch = _abi.FpBatch.from_buffer_copy(d.fb)
    bad_batch.ego = None
    cases = [
        (dict(best_idx=None, end_state=None), "exactly one of best_idx / end_state"),
        (dict(end_state=1 << 20), "exactly one of best_idx / end_state"),   # both given (never dereferenced: the call is rejected first)
        (dict(io=None), "fp_loop_io"),
        (dict(ego=None), "fp_loop_io"), (dict(t_now=None), "fp_loop_io"), (dict(done=None), "fp_loop_io"), (dict(cycles=None), "fp_loop_io"),
        (dict(cart_state=None), "cart_state is mandatory"),
        (dict(best_cost=None), "best_cost"),
        (dict(log=None), "fp_loop_log"), (dict(rows=None), "fp_loop_log"), (dict(n_rows=None), "fp_loop_log"), (dict(sealed=None), "fp_loop_log"),
        (dict(max_rows=-1), "max_rows"),
        (dict(stats=None), "stats is NULL"),
        (dict(mem=7), "mem must be"),
    ]
    for over, text in cases:
        rc = d.call(**over)
        assert rc == -1 and text in lib.fp_last_error().decode(), (over, lib.fp_last_error())
    if device:  # the vector stores need aligned rows
        lg_rows = d.t["rows"].data_ptr() + 8
        assert d.call(rows=lg_rows) == -1 and "16-byte aligned" in lib.fp_last_error().decode()
    for args in ((None, C.byref(d.params), C.byref(d.fb)), (engine._ctx, None, C.byref(d.fb)), (engine._ctx, C.byref(d.params), None),
                 (engine._ctx, C.byref(d.params), C.byref(bad_batch))):
        assert lib.fp_loop_record(*args, None, None, None, None, None, None, _abi.FP_MEM_DEVICE if device else _abi.FP_MEM_HOST, None) == -1
    # stats may be NULL when the log asks for none; nothing of the rejected calls reached the log
    assert d.call(stats=None, row_stats=None, stats_sum=None) == 0
    get = (lambda k: d.t[k].cpu().numpy()) if device else (lambda k: getattr(d, k))
    np.testing.assert_array_equal(get("n_rows"), d.h.cycles)
    assert (get("stats_sum") == 0).all() and (get("row_stats") == -77).all()


def test_recording_is_opt_in(engine):
    """A loop that does not ask for a log launches no record kernel - the ctx's counter does not move (on a ctx that never recorded it
    is still 0: the session's engine has, so the count before is the zero here) - and ends exactly where the recorded loop ends."""
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch

    outs = {}
    n0 = engine.get_option("looplog_launches")
    for kind in ("FOP", "FISS+"):
        batch, goal, cycles = _fixture("synth", kind)
        outs[kind] = ClosedLoopRunner(engine, DeviceBatch(batch, 0), goal, kind).run(cycles)
        assert not hasattr(outs[kind], "log") and outs[kind].trace == []
        assert ClosedLoopRunner(engine, DeviceBatch(_fixture("synth", kind)[0], 0), goal, kind).run_graph(5).trace == []
    assert engine.get_option("looplog_launches") - n0 == 0
    for kind in ("FOP", "FISS+"):
        batch, goal, cycles = _fixture("synth", kind)
        n0 = engine.get_option("looplog_launches")
        rec = ClosedLoopRunner(engine, DeviceBatch(batch, 0), goal, kind).run(cycles, record=True)
        assert engine.get_option("looplog_launches") == n0 + cycles
        for k in ("done", "cycles", "t_now", "ego"):
            np.testing.assert_array_equal(getattr(rec, k), getattr(outs[kind], k), err_msg=k)
        assert np.array_equal(rec.cart, outs[kind].cart, equal_nan=True)


def test_recorded_loop_stops_enqueueing_when_every_ego_is_done(engine):
    """G5 reaches its goal after 44 cycles: with a log the loop sees the count of running egos reach 0 at its next poll (cycle 48) and
    stops; without one all 100 steps are enqueued."""
    from fiss_plus_planner_amd.device_batch import LOG_POLL_CYCLES

    run, _, cycles = _runner(engine, "g5", "FOP")
    n0 = engine.get_option("lattice_launches")
    out = run.run(cycles, record=True)
    steps = engine.get_option("lattice_launches") - n0
    assert (out.done == _abi.DONE_GOAL).all() and (out.cycles == 44).all()
    print(f"lattice launches of the recorded loop: {steps} of {cycles}")
    assert 44 <= steps < cycles and LOG_POLL_CYCLES == 16
    run2, _, _ = _runner(engine, "g5", "FOP")
    n0 = engine.get_option("lattice_launches")
    run2.run(cycles)
    assert engine.get_option("lattice_launches") - n0 > steps
