"""GPU: fp_obstacles_from_plans (the egos' chosen plans as obstacle columns of each other's scenes) against its restatement
(tests/agents_ref.py) on the fixtures of tests/agents_cases.py - x, y, yaw of the rows inside a plan within conftest.series_tol of the
oracle's dump, tail rows within 1e-8 and the last yaw's tolerance, `valid` exact, everything outside the written set bit for bit the
sentinel the table was filled with (tests/test_agents_cpu.py shows that the fixtures reach their paths); then the memory modes, a second
call and reversed member lists bit for bit, the cross-check against fp_eval_trajs, the refusals, the launch counter, plan_dense on the
shared table, and ClosedLoopRunner(agents=): eager and graph state-identical and state-exact against the reference loop, no two group
members in contact, the time gap, and agents=None bit for bit what the commit before the feature produced."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import agents_cases as AC
import agents_none_loops
import agents_ref as GR
from conftest import GOLDEN, series_tol
from fiss_plus_planner_amd import _abi
from fiss_plus_planner_amd.agents import AgentGroups
from fiss_plus_planner_amd.engine import host_structs
from fiss_plus_planner_amd.fallback import FallbackStop

pytestmark = pytest.mark.gpu
POS_TOL = 1e-8  # the hand-over tolerance of tests/test_gpu_advance.py


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def sentinel_batch(c):
    return dataclasses.replace(c.batch, obs_pose=AC.sentinel_table(c.batch), final_time_step=np.full(c.batch.S, AC.SENTINEL_FTS, dtype=np.int32))


def host(engine, c, groups=None):
    """engine.share_plans (FP_MEM_HOST) on a fixture whose table is filled with the sentinel -> (obs_pose, final_time_step)"""
    ag = c.agents if groups is None else AgentGroups(groups, c.n_rows, c.tail, c.col_base)
    return engine.share_plans(sentinel_batch(c), ag, best_idx=c.best_idx, end_state=c.end_state, skip=c.skip)


def device(engine, c, groups=None, calls=1):
    """fp_obstacles_from_plans(FP_MEM_DEVICE): resident batch and arrays, `calls` launches, read back."""
    import torch

    from fiss_plus_planner_amd.device_batch import DeviceBatch

    db = DeviceBatch(sentinel_batch(c), order_hint=False)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(db.dev)  # noqa: E731
    held = {}

    def addr(name, a):
        held[name] = up(a)
        return held[name].data_ptr()

    ag = c.agents if groups is None else AgentGroups(groups, c.n_rows, c.tail, c.col_base)
    st = ag.struct(c.batch, addr)
    fb = _abi.FpBatch.from_buffer_copy(db.fb)
    if c.skip is not None:
        held["skip"] = up(c.skip)
        fb.skip = held["skip"].data_ptr()
    plans = up(c.best_idx if c.best_idx is not None else c.end_state)
    for _ in range(calls):
        engine.share_plans_device(db.params, fb, st, plans.data_ptr() if c.best_idx is not None else 0, plans.data_ptr() if c.best_idx is None else 0,
                                  db.t["obs_pose"].data_ptr(), db.t["final_time_step"].data_ptr(), torch.cuda.current_stream(db.dev).cuda_stream)
    torch.cuda.synchronize(db.dev)
    return db.t["obs_pose"].cpu().numpy(), db.t["final_time_step"].cpu().numpy()


def assert_matches(pose, fts, ref, what):
    w = ref.written
    assert np.array_equal(pose[..., 3][w], ref.pose[..., 3][w]), f"{what}: valid"
    err = np.abs(pose[w] - ref.pose[w])
    bad = ~(err <= ref.tol[w])
    assert not bad.any(), f"{what}: {int(bad.sum())} elements, first {np.argwhere(bad)[:4].tolist()} err {err[bad][:4]} tol {ref.tol[w][bad][:4]}"
    assert np.array_equal(bits(pose[~w]), bits(ref.pose[~w])), f"{what}: an element outside the written set changed"
    assert np.array_equal(fts, ref.fts), f"{what}: final_time_step {fts.tolist()} != {ref.fts.tolist()}"
    return float(err[:, :2].max()) if err.size else 0.0, float(err[:, 2].max()) if err.size else 0.0


@pytest.mark.parametrize("name", sorted(AC.FIXTURES))
def test_fixtures_against_the_reference_in_both_memory_modes(engine, oracle, name):
    c, ref = AC.case(name), AC.reference(oracle, name)
    hp, hf = host(engine, c)
    e_xy, e_yaw = assert_matches(hp, hf, ref, f"{name} host")
    dp, df = device(engine, c)
    assert_matches(dp, df, ref, f"{name} device")
    assert np.array_equal(bits(hp), bits(dp)) and np.array_equal(hf, df)  # the two memory spaces: the same bits
    assert (ref.fts[~ref.fts_written] == AC.SENTINEL_FTS).all()
    print(f"{name}: {int(ref.written.sum())} elements, max |dx, dy| {e_xy:.2e} m, max |dyaw| {e_yaw:.2e} rad")


def test_lattice_index_and_end_state_give_the_same_bits(engine):
    for tail in ("none", "hold", "coast"):
        pi, fi = host(engine, AC.case(f"kinds idx {tail}"))
        pe, fe = host(engine, AC.case(f"kinds es {tail}"))
        assert np.array_equal(bits(pi), bits(pe)) and np.array_equal(fi, fe), tail


@pytest.mark.parametrize("name", ["ragged", "kinds idx coast", "wide", "stopping"])
def test_a_second_call_and_reversed_members_give_the_same_bits(engine, name):
    c = AC.case(name)
    p1, f1 = device(engine, c)
    p2, f2 = device(engine, c, calls=2)
    assert np.array_equal(bits(p1), bits(p2)) and np.array_equal(f1, f2)
    rev = [list(g)[::-1] for g in c.groups]
    p3, f3 = device(engine, c, groups=rev)
    assert np.array_equal(f1, f3)
    for g in c.groups:  # per (scene, row, ego): member k's column is the mirrored one in the reversed launch
        scenes = c.batch.scene_of[list(g)]
        for k in range(len(g)):
            assert np.array_equal(bits(p1[scenes, :, c.col_base + k]), bits(p3[scenes, :, c.col_base + len(g) - 1 - k])), (name, g, k)


@pytest.mark.parametrize("name", ["ragged", "kinds es coast", "stopping", "wide"])
def test_cross_check_against_eval_trajs(engine, oracle, name):
    """Rows inside a plan are the FP_ARR_X / Y / YAW rows of fp_eval_trajs for the same end states."""
    c, ref = AC.case(name), AC.reference(oracle, name)
    b = c.batch
    pose, _ = host(engine, c)
    es = c.end_state if c.end_state is not None else np.array([GR.end_state_of(b, e, int(i)) if 0 <= i < b.C else (np.nan,) * 3 for e, i in enumerate(c.best_idx)])
    filler = np.array([b.d_samples[0], b.v_samples[0, 0] + 1.0, b.t_samples[0]])
    ev = engine.eval_trajs(b, np.where(np.isnan(es), filler, es)[:, None, :], dump=True, traj_stride=256)
    compared, equal = 0, 0
    for g in c.groups:
        for k, a in enumerate(g):
            if not ref.has[a] or len(g) < 2:
                continue
            s2 = int(b.scene_of[g[(k + 1) % len(g)]])  # a neighbour's scene
            t0 = int(b.t_now[a])
            m = min(int(ref.M[a]), c.n_rows, b.T_obs - t0)
            got = pose[s2, t0:t0 + m, c.col_base + k, :3].T
            want = ev.traj[a, 0][:, :int(ref.N[a])]
            tol = series_tol(want, b.tick_t)[9:12, :m]
            tol[2] = np.where(np.isfinite(tol[2]), tol[2], 0.0)  # (a step of exactly zero length: yaw 0 on both sides)
            assert (np.abs(got - want[9:12, :m]) <= tol).all(), (name, a)
            compared += got.size
            equal += int((bits(got) == bits(want[9:12, :m])).sum())
    assert compared > 0
    print(f"{name}: {equal} of {compared} series elements bit-equal to fp_eval_trajs")


def raw(engine, batch, group_ptr=(0, 2), members=(0, 1), G=None, n_members=None, col_base=0, n_rows=4, tail=2, best_idx=None, end_state=True, null=(), mem=_abi.FP_MEM_HOST,
        struct=True):
    """fp_obstacles_from_plans through ctypes with every argument in the caller's hands -> (rc, message)."""
    gp, mb = np.ascontiguousarray(group_ptr, dtype=np.int32), np.ascontiguousarray(members, dtype=np.int32)
    st = _abi.FpAgents(len(gp) - 1 if G is None else G, len(mb) if n_members is None else n_members, None if "group_ptr" in null else gp.ctypes.data,
                       None if "members" in null else mb.ctypes.data, col_base, n_rows, tail, 0)
    bi = None if best_idx is None else np.ascontiguousarray(best_idx, dtype=np.int32)
    es = np.tile(np.array([0.0, 3.0, 2.0]), (batch.B, 1)) if end_state is True else end_state
    pose, fts = batch.obs_pose.copy(), batch.final_time_step.copy()
    p, fb = host_structs(batch)
    rc = engine._lib.fp_obstacles_from_plans(engine._ctx, C.byref(p), C.byref(fb), C.byref(st) if struct else None, None if bi is None else bi.ctypes.data,
                                             None if es is None else es.ctypes.data, None if "obs_pose" in null else pose.ctypes.data, fts.ctypes.data, mem, None)
    return rc, engine._lib.fp_last_error().decode(errors="replace")


def test_every_error_of_the_host_path(engine):
    b = AC.case("ragged").batch  # 12 egos, 8 columns, every ego a scene of its own
    before = engine.get_option("from_plans_launches")
    EINVAL = -1
    assert raw(engine, b, struct=False)[0] == EINVAL
    for k in ("group_ptr", "members", "obs_pose"):
        assert raw(engine, b, null=(k,))[0] == EINVAL, k
    assert raw(engine, b, end_state=None)[0] == EINVAL and raw(engine, b, best_idx=np.zeros(12))[0] == EINVAL  # neither, both
    for kw, word in ((dict(n_rows=0), "n_rows=0"), (dict(n_rows=-3), "n_rows=-3"), (dict(tail=3), "tail=3"), (dict(tail=-1), "tail=-1"),
                     (dict(members=(0, 12)), "member 1 of group 0 is ego 12"), (dict(members=(-1, 1)), "member 0 of group 0 is ego -1"),
                     (dict(group_ptr=(0, 2, 4), members=(0, 1, 2, 1)), "ego 1 is a member of group 0 and of group 1"),
                     (dict(col_base=-1), "col_base=-1"), (dict(col_base=7), "group 0: col_base + group size = 7 + 2 exceeds n_obs = 8"),
                     (dict(group_ptr=(0, 3, 2), members=(0, 1, 2)), "not ascending at group 1"), (dict(n_members=3), "n_members=3 is not group_ptr[G]=2"),
                     (dict(group_ptr=(1, 2)), "group_ptr[0]=1"),
                     (dict(end_state=None, best_idx=np.where(np.arange(12) == 4, b.C, 0)), "best_idx of ego 4")):
        rc, msg = raw(engine, b, **kw)
        assert rc == EINVAL and word in msg, (kw, msg)
    rc, msg = raw(engine, dataclasses.replace(b, scene_of=np.where(np.arange(12) == 1, -1, b.scene_of)))
    assert rc == EINVAL and "member 1 of group 0 (ego 1) has no scene" in msg, msg
    rc, msg = raw(engine, dataclasses.replace(b, scene_of=np.where(np.arange(12) == 1, b.scene_of[0], b.scene_of)))
    assert rc == EINVAL and f"ego 0 and ego 1 share scene {int(b.scene_of[0])}" in msg, msg
    # (the argument checks of the device path come before any launch too)
    assert raw(engine, b, n_rows=0, mem=_abi.FP_MEM_DEVICE)[0] == EINVAL and raw(engine, b, tail=5, mem=_abi.FP_MEM_DEVICE)[0] == EINVAL
    assert raw(engine, b, group_ptr=(0,), members=())[0] == 0 and raw(engine, b, group_ptr=(0, 0), members=())[0] == 0  # G == 0, n_members == 0: nothing to write
    assert engine.get_option("from_plans_launches") == before  # a refused call launches nothing
    assert raw(engine, b)[0] == 0 and engine.get_option("from_plans_launches") == before + 1
    assert raw(engine, b, end_state=None, best_idx=np.where(np.arange(12) == 4, -1, 0))[0] == 0  # (a negative index is "no plan")


def test_from_plans_launches_counts_the_kernels_launches():
    """0 for a caller that never asks, one per call afterwards; no other launch counter moves."""
    from fiss_plus_planner_amd.engine import FrenetEngine

    c = AC.case("stopping")
    others = ("predict_launches", "margin_launches", "fallback_launches", "lattice_launches", "gap_launches", "rules_eval_launches", "looplog_launches", "from_state_launches")
    with FrenetEngine(0) as eng:
        eng.plan_dense(c.batch)
        assert eng.get_option("from_plans_launches") == 0
        n0 = [eng.get_option(k) for k in others]
        host(eng, c)
        device(eng, c, calls=2)
        assert eng.get_option("from_plans_launches") == 3 and [eng.get_option(k) for k in others] == n0


def test_plan_dense_on_the_shared_table(engine, oracle):
    """An ego whose neighbour's plan crosses its lane gets FP_FLAG_COLLISION on exactly the candidates the oracle flags against the
    reference table."""
    ego = np.array([[10.0, 9.0, 0.0, 0.0, 0.0, 0.0], [26.0, 3.0, 0.0, -0.8, 0.0, 0.0]])
    b = AC.straight_batch(ego, [np.linspace(0.0, 9.0, 5), np.linspace(0.0, 3.0, 5)], [9.0, 3.0], t_samples=(3.0, 5.0), nd=5)
    ag = AgentGroups([[0, 1]], 60, "coast")
    b = ag.attach(b, 70)
    es = np.array([[0.0, 9.0, 5.0], [0.8, 3.0, 4.0]])  # ego 1 moves across the lane in front of ego 0
    pose, fts = engine.share_plans(b, ag, end_state=es)
    ref = GR.table(oracle, b, ag.groups, ag.n_rows, ag.tail, 0, end_state=es)
    got = engine.plan_dense(dataclasses.replace(b, obs_pose=pose, final_time_step=fts))
    shared = dataclasses.replace(b, obs_pose=ref.pose, final_time_step=ref.fts)
    blind = engine.plan_dense(b)
    for e in range(2):
        _, flags = oracle.problems_from_batch(shared, egos=[e])[0].dense_tables()
        assert np.array_equal(got.flags[e] & _abi.FLAG_COLLISION, flags & _abi.FLAG_COLLISION), e
    hit = (got.flags[0] & _abi.FLAG_COLLISION) != 0
    assert hit.any() and not hit.all() and not (blind.flags & _abi.FLAG_COLLISION).any()


# ---------------------------------------------------------------------------
# ClosedLoopRunner(agents=)
# ---------------------------------------------------------------------------
STATE_KEYS = ("done", "cycles", "ego", "t_now", "cart")
EGO_COLS = [_abi.LOG_S, _abi.LOG_VELOCITY, _abi.LOG_S_DD, _abi.LOG_D, _abi.LOG_VELOCITY_Y, _abi.LOG_D_DD]


def run_loop(engine, kind, planner="FOP", agents=True, graph=False, record=True, cycles=AC.LOOP_CYCLES, batch_kw=None, **kw):
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch

    b, goal, ag = AC.loop_scenario(kind, kindp=planner)
    if batch_kw:
        b = dataclasses.replace(b, **batch_kw)
    kw.setdefault("fallback", FallbackStop(AC.LOOP_STOP_T))
    r = ClosedLoopRunner(engine, DeviceBatch(b), goal, planner, agents=ag if agents else None, **kw)
    out = r.run_graph(cycles, record=record) if graph else r.run(cycles, record=record)
    out.table = r.db.t["obs_pose"].cpu().numpy()
    return b, ag, out


def logged_overlap(oracle, b, ag, log, lag=0):
    """[cycles] bool: after that cycle the footprints of two group members intersect (lag: the rear member against the front member's
    footprints up to `lag` cycles earlier)."""
    n = min(log.span(e)[1] for e in range(b.B))
    hit = np.zeros(n, dtype=bool)
    for a, c in GR.group_pairs(ag.groups):
        ra, rc = log.ego_rows(a), log.ego_rows(c)
        for k in range(n):
            for j in range(max(k - lag, 0), k + 1):
                box = lambda r: (b.veh_l, b.veh_w, r[_abi.LOG_X], r[_abi.LOG_Y], r[_abi.LOG_YAW])  # noqa: E731
                hit[k] |= bool(oracle.boxes_intersect(box(ra[k]), box(rc[j])))
    return hit


@pytest.mark.parametrize("kind", ["follower", "platoon"])
def test_loop_fop_with_fallback_against_the_reference_loop(engine, oracle, kind):
    b, ag, eager = run_loop(engine, kind)
    _, _, graph = run_loop(engine, kind, graph=True)
    for k in STATE_KEYS + ("table",):
        assert getattr(graph, k).tobytes() == getattr(eager, k).tobytes(), k
    for e in range(b.B):
        assert graph.log.ego_rows(e).tobytes() == eager.log.ego_rows(e).tobytes()
    rb, goal, _ = AC.loop_scenario(kind)
    ref = GR.loop(oracle, rb, goal, ag.groups, ag.n_rows, ag.tail, ag.col_base, AC.LOOP_CYCLES, stop_T=AC.LOOP_STOP_T)
    assert ref.undecided == 0 and np.array_equal(eager.done, ref.done) and np.array_equal(eager.cycles, ref.cycles)
    worst = 0.0
    for e in range(b.B):
        rows = eager.log.ego_rows(e)
        assert len(rows) == ref.cycles[e]
        worst = max(worst, float(np.abs(rows[:, EGO_COLS] - ref.states[1:ref.cycles[e] + 1, e]).max()))
    print(f"{kind}: driven states within {worst:.3e} of the CPU reference loop over {AC.LOOP_CYCLES} cycles")
    assert worst <= POS_TOL
    # no two group members in contact in any recorded cycle, every ego still running; the same scenario without agents overlaps
    assert not logged_overlap(oracle, b, ag, eager.log).any() and (eager.done == _abi.RUNNING).all()
    _, _, none = run_loop(engine, kind, agents=False)
    assert logged_overlap(oracle, b, ag, none.log).any()


def test_loop_fop_without_a_fallback_and_refusals(engine, oracle):
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch

    b, ag, eager = run_loop(engine, "follower", fallback=None, cycles=20)
    _, _, graph = run_loop(engine, "follower", fallback=None, cycles=20, graph=True)
    for k in STATE_KEYS + ("table",):
        assert getattr(graph, k).tobytes() == getattr(eager, k).tobytes(), k
    rb, goal, _ = AC.loop_scenario("follower")
    ref = GR.loop(oracle, rb, goal, ag.groups, ag.n_rows, ag.tail, ag.col_base, 20)
    assert np.array_equal(eager.done, ref.done) and np.array_equal(eager.cycles, ref.cycles)
    for e in range(b.B):
        rows = eager.log.ego_rows(e)
        assert (rows[:, _abi.LOG_BEST_IDX] >= 0).all()  # FOP without a fallback drives its lattice index
        assert np.abs(rows[:, EGO_COLS] - ref.states[1:ref.cycles[e] + 1, e]).max() <= POS_TOL
    fb, goal, ag = AC.loop_scenario("follower", kindp="FISS+")
    with pytest.raises(ValueError, match="agents= with audit="):
        ClosedLoopRunner(engine, DeviceBatch(dataclasses.replace(fb, gap_follow=5)), goal, "FISS+", audit=("gaps",), agents=ag)
    plain = AC.loop_scenario("follower", attach=False)[0]  # (not attached: no scene holds a column)
    with pytest.raises(ValueError, match="exceeds n_obs = 0"):
        ClosedLoopRunner(engine, DeviceBatch(plain), goal, "FOP", agents=ag)
    with pytest.raises(ValueError, match="has no scene"):
        ClosedLoopRunner(engine, DeviceBatch(dataclasses.replace(b, scene_of=np.array([-1, 1]))), goal, "FOP", agents=ag)


@pytest.mark.parametrize("kind", ["follower", "platoon"])
def test_loop_fissplus_with_fallback_against_the_reference_loop(engine, oracle, kind):
    """FISS+ + fallback: eager and graph state-identical; state-exact against the reference loop up to the first cycle whose refined
    candidates the reference cannot order (the convention of tests/test_gpu_fiss_rules.py)."""
    import fiss_rules_ref as FR

    b, ag, eager = run_loop(engine, kind, "FISS+")
    _, _, graph = run_loop(engine, kind, "FISS+", graph=True)
    for k in STATE_KEYS + ("table",):
        assert getattr(graph, k).tobytes() == getattr(eager, k).tobytes(), k
    rb, goal, _ = AC.loop_scenario(kind, kindp="FISS+")
    prev = {e: None for e in range(b.B)}
    undecided = []

    def plan(batch, e, cycle):
        r = FR.plan(oracle, batch, e, "FISS+", (), prev[e])
        prev[e] = r.prev_best_idx
        if r.undecided:
            undecided.append(cycle)
        return r.end_state

    ref = GR.loop(oracle, rb, goal, ag.groups, ag.n_rows, ag.tail, ag.col_base, AC.LOOP_CYCLES, stop_T=AC.LOOP_STOP_T, plan=plan)
    n = min(undecided) if undecided else AC.LOOP_CYCLES
    assert ref.undecided == 0 and n >= 10, (n, undecided[:4])
    worst = 0.0
    for e in range(b.B):
        rows = eager.log.ego_rows(e)[:n]
        worst = max(worst, float(np.abs(rows[:, EGO_COLS] - ref.states[1:len(rows) + 1, e]).max()))
    print(f"{kind} FISS+: driven states within {worst:.3e} of the CPU reference loop over {n} cycles (first undecided cycle: {n})")
    assert worst <= POS_TOL


def test_loop_keeps_the_time_gap(engine, oracle):
    """rules=("gaps",) reads the table the agents write: the follower settles at least the configured gap behind, with no further code."""
    lag = 15
    b, ag, out = run_loop(engine, "follower", rules=("gaps",), batch_kw=dict(gap_follow=lag, gap_lead=0, gap_first=1), cycles=90)
    assert (out.done == _abi.RUNNING).all()
    hit = logged_overlap(oracle, b, ag, out.log, lag=lag)
    first_clear = int(np.nonzero(hit)[0].max()) + 1 if hit.any() else 0
    print(f"time gap of {lag} steps: kept from cycle {first_clear} on ({len(hit)} cycles recorded)")
    assert not hit[-30:].any()  # settled: for the last 30 cycles the follower is never where the leader was up to `lag` steps before
    assert not logged_overlap(oracle, b, ag, out.log).any()


def test_agents_none_reproduces_the_recorded_loops(engine):
    """ClosedLoopRunner without agents=: bit for bit what the commit before the feature produced (tests/golden/agents_none_loops.npz)."""
    want = np.load(os.path.join(GOLDEN, "agents_none_loops.npz"))
    n0 = engine.get_option("from_plans_launches")
    got = agents_none_loops.run_all(engine)
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert engine.get_option("from_plans_launches") == n0
