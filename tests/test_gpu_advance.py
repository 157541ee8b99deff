"""GPU: the closed-loop hand-over (csrc/frenet_advance.h: advance_kernel, the tail of the lattice kernel, the tail of the FISS+
refinement kernel) against tests/advance_ref.py - the reference's loop body restated on the oracle's series - rule by rule, on the
case table of tests/advance_cases.py.  tests/test_advance_ref_cpu.py proves on the CPU that the reference reproduces the recorded
runs and that every case of the table is decidable (margin >= 1e-6), so nothing is skipped here.

Tolerances (tests/conftest.py): integers and codes exact; the six ego numbers and x, y within 1e-8 (the series rows 0-10 bound);
the heading within series_tol's yaw bound for the step's ds (a stationary ego's heading is noise in any implementation).
The largest error of every test is printed (EXPERIMENTS.md, "Hand-over parity").
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import advance_cases as AC
import advance_ref as R
from conftest import series_tol

pytestmark = pytest.mark.gpu
POS_TOL = 1e-8
MARGIN = 1e-6


@pytest.fixture(scope="module")
def tables(oracle):
    return {k: AC.build(oracle, k) for k in AC.LATTICES}


def _batch(T, state=None):
    from fiss_plus_planner_amd.batch import ProblemBatch

    st = state or T
    return ProblemBatch(d_samples=T.d_samples, t_samples=T.t_samples, v_samples=T.v_samples, target_speed=np.full(T.B, 10.0), ego=st.ego.copy(),
                        frame_of=T.frame_of, scene_of=np.full(T.B, -1), t_now=st.t_now.copy(), nx=T.nx, knots=T.knots, coef=T.coef,
                        obs_pose=np.zeros((0, 1, 0, 4)), obs_dims=np.zeros((0, 0, 2)), final_time_step=np.zeros(0), veh_l=T.veh_l, veh_w=1.8,
                        max_speed=40.0, max_accel=10.0, tick_t=T.tick_t)


def _goal_arrays(T, variant, goal_xy):
    """(goal_xy, goal_poly, goal_nv, goal_intervals) of a variant: "full", "no_intervals", "no_poly" """
    g = np.ascontiguousarray(T.goal_xy if goal_xy is None else goal_xy)
    if variant == "no_poly":
        return g, None, None, None
    return g, T.goal_poly, T.goal_nv, None if variant == "no_intervals" else T.goal_intervals


def advance_host(engine, T, use_idx, variant="full", state=None, goal_xy=None, rc_only=False, best_idx=None):
    """fp_advance on host arrays -> the loop state after the call"""
    from fiss_plus_planner_amd import _abi
    from fiss_plus_planner_amd.engine import _host_batch, make_params

    st = state or T
    hb = _batch(T, st)
    out = SimpleNamespace(ego=hb.ego, t_now=hb.t_now, done=st.done.copy(), cycles=st.cycles.copy(), cart=np.full((T.B, 3), -7.5))
    g, poly, nv, iv = _goal_arrays(T, variant, goal_xy)
    io = _abi.FpLoopIo()
    io.ego, io.t_now, io.done, io.cycles, io.goal_xy, io.cart_state = (a.ctypes.data for a in (out.ego, out.t_now, out.done, out.cycles, g, out.cart))
    if poly is not None:
        io.goal_poly, io.goal_nv, io.goal_max_vertices = poly.ctypes.data, nv.ctypes.data, T.goal_max_vertices
        if iv is not None:
            io.goal_intervals = iv.ctypes.data
    idx = np.ascontiguousarray(T.best_idx if best_idx is None else best_idx, dtype=np.int32)
    es = np.ascontiguousarray(T.end_state)
    p, fb = make_params(hb), _host_batch(hb)
    rc = engine._lib.fp_advance(engine._ctx, C.byref(p), C.byref(fb), idx.ctypes.data if use_idx else None, None if use_idx else es.ctypes.data,
                                C.byref(io), _abi.FP_MEM_HOST, None)
    if rc_only:
        return rc, out
    _abi.check(rc)
    return out


class DeviceLoop:
    """The same call on device arrays (FP_MEM_DEVICE); the loop state stays on the device between steps"""

    def __init__(self, engine, T, use_idx, variant="full", goal_xy=None):
        import torch

        from fiss_plus_planner_amd import _abi
        from fiss_plus_planner_amd.device_batch import DeviceBatch

        self.eng, self.T, self.torch = engine, T, torch
        self.db = DeviceBatch(_batch(T), 0)
        dev = self.db.dev
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        g, poly, nv, iv = _goal_arrays(T, variant, goal_xy)
        self.t = dict(done=up(T.done), cycles=up(T.cycles), goal=up(g), cart=torch.full((T.B, 3), float("nan"), dtype=torch.float64, device=dev),
                      idx=up(T.best_idx), es=up(T.end_state))
        io = _abi.FpLoopIo()
        io.ego, io.t_now = self.db.t["ego"].data_ptr(), self.db.t["t_now"].data_ptr()
        io.done, io.cycles, io.goal_xy, io.cart_state = (self.t[k].data_ptr() for k in ("done", "cycles", "goal", "cart"))
        if poly is not None:
            self.t.update(poly=up(poly), nv=up(nv))
            io.goal_poly, io.goal_nv, io.goal_max_vertices = self.t["poly"].data_ptr(), self.t["nv"].data_ptr(), T.goal_max_vertices
            if iv is not None:
                self.t["iv"] = up(iv)
                io.goal_intervals = self.t["iv"].data_ptr()
        self.io, self.use_idx = io, use_idx

    def step(self):
        from fiss_plus_planner_amd import _abi

        self.t["cart"].fill_(float("nan"))
        _abi.check(self.eng._lib.fp_advance(self.eng._ctx, C.byref(self.db.params), C.byref(self.db.fb), self.t["idx"].data_ptr() if self.use_idx else None,
                                            None if self.use_idx else self.t["es"].data_ptr(), C.byref(self.io), _abi.FP_MEM_DEVICE, None))
        self.torch.cuda.synchronize(self.db.dev)
        return SimpleNamespace(ego=self.db.t["ego"].cpu().numpy(), t_now=self.db.t["t_now"].cpu().numpy(), done=self.t["done"].cpu().numpy(),
                               cycles=self.t["cycles"].cpu().numpy(), cart=self.t["cart"].cpu().numpy())


def compare(what, names, got, ref, before):
    """Every ego of `got` (arrays) against its reference result; `before`: the loop state on entry (egos that do not move keep it)."""
    err = dict(ego=0.0, xy=0.0, yaw=0.0, yaw_over_tol=0.0)
    for b, (name, r) in enumerate(zip(names, ref)):
        tag = f"{what}: ego {b} ({name})"
        assert R.decidability(r.margins) >= MARGIN, tag
        assert (got.done[b], got.t_now[b], got.cycles[b]) == (r.done, r.t_now, r.cycles), (tag, got.done[b], got.t_now[b], got.cycles[b], r.done, r.t_now, r.cycles)
        if not r.moved:
            assert np.array_equal(got.ego[b], before.ego[b], equal_nan=True) and np.isnan(got.cart[b]).all(), (tag, got.ego[b], got.cart[b])
            continue
        e_ego, e_xy, e_yaw = np.abs(got.ego[b] - r.ego).max(), np.abs(got.cart[b, :2] - r.cart[:2]).max(), abs(got.cart[b, 2] - r.cart[2])
        assert e_ego <= POS_TOL and e_xy <= POS_TOL, (tag, e_ego, e_xy)
        assert e_yaw <= r.yaw_tol, (tag, e_yaw, r.yaw_tol)
        err["ego"], err["xy"] = max(err["ego"], e_ego), max(err["xy"], e_xy)
        if np.isfinite(r.yaw_tol):
            err["yaw"], err["yaw_over_tol"] = max(err["yaw"], e_yaw), max(err["yaw_over_tol"], e_yaw / r.yaw_tol)
    print(f"PARITY {what}: " + " ".join(f"{k}={v:.3e}" for k, v in err.items()))


@pytest.mark.parametrize("variant", ["full", "no_intervals", "no_poly"])
@pytest.mark.parametrize("lattice", ["A", "B"])
def test_fp_advance_host_against_the_reference(oracle, engine, tables, lattice, variant):
    """The whole table through FP_MEM_HOST: once by end state, once by best_idx (the cases that have one); goal_intervals = NULL and
    goal_poly = NULL are the same table with that pointer left out."""
    T = tables[lattice]
    ref = AC.reference(oracle, T, variant, series_tol=series_tol)
    compare(f"host end_state {lattice} {variant}", T.names, advance_host(engine, T, False, variant), ref, T)
    sub = AC.take(T, T.has_idx)
    assert sub.B >= np.prod(T.lattice)
    compare(f"host best_idx {lattice} {variant}", sub.names, advance_host(engine, sub, True, variant), [r for r, h in zip(ref, T.has_idx) if h], sub)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_fp_advance_batch_sizes(oracle, engine, tables, n):
    """The partial last workgroup of advance_kernel (64 lanes): the first n egos of the table"""
    T = AC.take(tables["A"], slice(0, n))
    compare(f"host end_state B={n}", T.names, advance_host(engine, T, False), AC.reference(oracle, T, series_tol=series_tol), T)


@pytest.mark.parametrize("use_idx", [False, True], ids=["end_state", "best_idx"])
def test_fp_advance_device_equals_host_bit_for_bit(engine, tables, use_idx):
    for key in ("A", "B"):
        T = tables[key] if not use_idx else AC.take(tables[key], tables[key].has_idx)
        host = advance_host(engine, T, use_idx)
        dev = DeviceLoop(engine, T, use_idx).step()
        for k in ("done", "t_now", "cycles"):
            np.testing.assert_array_equal(getattr(dev, k), getattr(host, k), err_msg=k)
        assert np.array_equal(dev.ego, host.ego, equal_nan=True) and np.array_equal(dev.cart, host.cart, equal_nan=True)
        assert (~np.isnan(host.cart[:, 0])).sum() > T.B // 2


def test_closed_interval_of_the_goal_centre_rule_is_exact(oracle, engine, tables):
    """`<=`, not `<`: the goal centre exactly l/2 from the position the KERNEL returned (x1 -+ 2.25 is exact: 2.25 is a multiple of the
    ulp of these coordinates, and the offset points towards 0, so the exponent cannot grow) ends the run; one ulp further away does not."""
    T = AC.take(tables["A"], tables["A"].generic)
    free = advance_host(engine, T, False, "no_poly", goal_xy=np.full((T.B, 2), AC.FAR))
    moved = ~np.isnan(free.cart[:, 0])
    assert moved.sum() >= 100
    x1, y1 = free.cart[:, 0], free.cart[:, 1]
    half = T.veh_l / 2
    gx = np.where(moved, x1 - np.copysign(half, x1), AC.FAR)
    assert (np.abs(x1[moved]) > half).all() and (np.abs(x1[moved] - gx[moved]) == half).all()  # the test's construction, not a skip
    on = advance_host(engine, T, False, "no_poly", goal_xy=np.column_stack([gx, np.where(moved, y1, AC.FAR)]))
    np.testing.assert_array_equal(on.done[moved], R.DONE_GOAL)
    gx2 = np.where(moved, np.nextafter(gx, -np.copysign(np.inf, x1)), AC.FAR)
    assert (np.abs(x1[moved] - gx2[moved]) > half).all()
    off = advance_host(engine, T, False, "no_poly", goal_xy=np.column_stack([gx2, np.where(moved, y1, AC.FAR)]))
    assert (off.done[moved] != R.DONE_GOAL).all()
    np.testing.assert_array_equal(off.done, free.done)  # (what the other rules say without a goal centre)


def test_closed_interval_of_the_end_of_map_rule_is_exact(oracle, engine, tables):
    """`<=`, not `<`, in the second distance rule: lines whose last resampled point is a knot (evaluated with dx == 0: the knot's
    coefficients, bit for bit) placed exactly 3.0 m from the position the KERNEL returned end the run; one ulp further away they do not."""
    T = AC.exact_end_of_map_table(tables["A"])
    free = advance_host(engine, T, False, "no_poly")
    assert (free.done == R.RUNNING).all() and (free.cycles == 1).all()  # (the lines' own end points are 20 m away)
    on, off = AC.exact_end_of_map_goals(T, free.cart[:, 0], free.cart[:, 1])
    got = advance_host(engine, on, False, "no_poly")
    assert np.array_equal(got.cart, free.cart) and np.array_equal(got.ego, free.ego)  # (the first segment's coefficients are untouched)
    np.testing.assert_array_equal(got.done, R.DONE_END_OF_LINE)
    np.testing.assert_array_equal(advance_host(engine, off, False, "no_poly").done, R.RUNNING)
    np.testing.assert_array_equal(DeviceLoop(engine, on, False, "no_poly").step().done, R.DONE_END_OF_LINE)


def test_three_cycles_in_a_row(oracle, engine, tables):
    """The generic cases for three cycles on the device: after every cycle the device's state against the reference applied to the
    device's PREVIOUS state (t_now / cycles drift, finished egos left alone)."""
    T = AC.take(tables["A"], tables["A"].generic)
    for use_idx in (False, True):
        Tk = AC.take(T, T.has_idx) if use_idx else T
        loop = DeviceLoop(engine, Tk, use_idx)
        state = SimpleNamespace(ego=Tk.ego, t_now=Tk.t_now, cycles=Tk.cycles, done=Tk.done)
        for cycle in range(3):
            got = loop.step()
            compare(f"device cycle {cycle} {'best_idx' if use_idx else 'end_state'}", Tk.names, got, AC.reference(oracle, Tk, state=state, series_tol=series_tol), state)
            state = got
        assert (state.cycles - Tk.cycles == 3).sum() > Tk.B // 3 and (state.done != 0).any()


def test_fp_advance_refuses_an_index_beyond_the_lattice(engine, tables):
    """FP_MEM_HOST only: best_idx >= nd * nv * nt of a running ego is refused before anything is staged, ego and value named; nothing
    is written.  (The device path's contract is the caller's: no out-of-range index is ever handed to a launch.)"""
    from fiss_plus_planner_amd import _abi

    T = AC.take(tables["A"], tables["A"].has_idx & (tables["A"].done == 0))
    Cn = int(np.prod(T.lattice))
    for bad in (Cn, Cn + 1, 2 ** 31 - 1):
        idx = T.best_idx.copy()
        idx[3] = bad
        rc, out = advance_host(engine, T, True, rc_only=True, best_idx=idx)
        msg = engine._lib.fp_last_error().decode()
        assert rc == -1 and f"best_idx[3]={bad}" in msg and str(Cn) in msg, (rc, msg)
        assert np.array_equal(out.ego, T.ego) and np.array_equal(out.done, T.done) and np.array_equal(out.cycles, T.cycles) and (out.cart == -7.5).all()
    idx = T.best_idx.copy()
    idx[3] = Cn - 1
    _abi.check(advance_host(engine, T, True, rc_only=True, best_idx=idx)[0])


# ---- the fused hand-overs: fp_plan_step (the lattice kernel's last thread) and fp_plan_fiss_step (the refinement kernel's tail; the
# advance kernel behind the FISS pipeline) against the reference - not just against each other
def _fused(oracle, engine, planner, B, n_batches):
    """n_batches batches of B egos (config-2-sized lattice).  A free cycle tells where every ego lands; then a quarter of the moving
    egos each get: nothing, a goal centre within l/2, a goal region with intervals around the landing point, a reference line that
    ends within 3 m of it.  Expected: advance_ref on the start state and the best_idx / end state THE CALL returned."""
    from fiss_plus_planner_amd import synth
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch

    plan = np.zeros(4, dtype=int)  # egos planned to keep running / reach the centre / reach the region / reach the end of the map, over all batches
    names, ref_all, got_all, before_all = [], [], [], []
    for k in range(n_batches):
        mk = lambda: synth.make_config(2, B=B, ego_offset=k * B, kind=planner)
        far = np.full((B, 2), AC.FAR)
        free = ClosedLoopRunner(engine, DeviceBatch(mk(), 0), far, planner).run(1)
        batch = mk()
        moved = free.cycles == 1
        goal = far.copy(); poly = np.zeros((B, 4, 2)); nv = np.zeros(B, dtype=np.int32); iv = np.full((B, 6), np.nan)
        for b in np.nonzero(moved)[0]:
            x, y, yaw = free.cart[b]
            kn = batch.knots[b]
            j = int(np.searchsorted(kn, free.ego[b, 0], side="right"))
            gap = kn[j] - free.ego[b, 0]
            kind = 3 if (0.5 < gap < 2.6 and plan[3] <= plan[:3].min()) else int(np.argmin(plan[:3]))
            plan[kind] += 1
            if kind == 1:
                goal[b] = [x + 1.0, y - 0.5]
            elif kind == 2:
                poly[b] = [[x - 2, y - 2], [x + 2, y - 2], [x + 2, y + 2], [x - 2, y + 2]]
                nv[b] = 4
                iv[b] = [0, 0, free.ego[b, 1] - 0.5, free.ego[b, 1] + 0.5, yaw - 0.05, yaw + 0.05]
            elif kind == 3:  # the line ends at the next knot
                batch.nx[b] = j + 1
                batch.knots[b, j + 1:] = np.inf
        start = SimpleNamespace(ego=batch.ego.copy(), t_now=batch.t_now.copy(), cycles=np.zeros(B, dtype=np.int32), done=np.zeros(B, dtype=np.int32))
        run = ClosedLoopRunner(engine, DeviceBatch(batch, 0), goal, planner, goal_poly=poly, goal_nv=nv, goal_intervals=iv)
        got = run.run(1)
        idx = run.best_idx.cpu().numpy() if planner == "FOP" else None
        es = None if planner == "FOP" else run.end_state.cpu().numpy()
        for b in range(B):
            n = batch.nx[b]
            kw = dict(best_idx=int(idx[b]), d_samples=batch.d_samples, t_samples=batch.t_samples, v_samples=batch.v_samples[b]) if planner == "FOP" else dict(end_state=es[b])
            ref_all.append(R.advance(oracle, tick_t=batch.tick_t, veh_l=batch.veh_l, knots=batch.knots[b, :n], coef=batch.coef[b, :, :n], ego=start.ego[b], t_now=0,
                                     goal_xy=goal[b], goal_poly=poly[b], goal_nv=nv[b], goal_max_vertices=4, goal_intervals=iv[b], series_tol=series_tol, **kw))
            names.append(f"batch {k} ego {b}")
        got_all.append(got); before_all.append(start)
    cat = lambda xs, k: np.concatenate([getattr(x, k) for x in xs])
    got = SimpleNamespace(**{k: cat(got_all, k) for k in ("ego", "t_now", "done", "cycles", "cart")})
    before = SimpleNamespace(ego=cat(before_all, "ego"))
    assert all(np.isfinite(r.yaw_tol) for r in ref_all if r.moved)  # (every moving ego's heading is held to a finite bound: none stands still)
    compare(f"fused {planner} B={B}", names, got, ref_all, before)
    counts = np.bincount(got.done, minlength=5)
    assert (counts >= 10).all(), counts  # at least ten egos keep running and ten stop by each of the four codes


def test_plan_step_latency_instances_against_the_reference(oracle, engine):
    _fused(oracle, engine, "FOP", 7, 24)


def test_plan_step_multi_round_instances_against_the_reference(oracle, engine):
    """resident_groups = 2 models a one-CU device: twelve egos take the multi-round instances with their tail split"""
    engine.set_option("resident_groups", 2)
    try:
        _fused(oracle, engine, "FOP", 12, 14)
    finally:
        engine.set_option("resident_groups", 0)


@pytest.mark.parametrize("planner", ["FISS+", "FISS"])
def test_plan_fiss_step_against_the_reference(oracle, engine, planner):
    """FISS+: the refinement workgroup hands the ego over (the end state in registers); FISS: the advance kernel behind the pipeline"""
    _fused(oracle, engine, planner, 7, 24)
