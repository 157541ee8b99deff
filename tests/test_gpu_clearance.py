"""GPU: the obstacle-clearance cost term (fp_params.w_obstacle) against its independent restatement (tests/clearance_ref.py: oracle
tables + brute-force distances).  Costs within the project's bar (|d| <= 1e-9 max(1, |ref|), tests/test_gpu_edges.py::cost_close),
flags and Stats exact, best_idx exact for every ego.  tests/test_clearance_cpu.py shows that the cases could not pass by returning the
plain winner."""
import ctypes as C

import numpy as np
import pytest

import clearance_ref as R
from conftest import assert_series_close, load_golden
from fiss_plus_planner_amd import _abi, synth
from fiss_plus_planner_amd.engine import host_structs
from test_clearance_cpu import CASES, W_TEST
from test_gpu_edges import cost_close

pytestmark = pytest.mark.gpu


def weighted(batch, w=W_TEST):
    batch.w_obstacle = w
    return batch


def check_against_restatement(engine, oracle, batch, egos=None, stride=128, what=""):
    """plan_dense with tables and without them, both against the restatement; returns the table call's output."""
    launches = engine.get_option("clearance_launches")
    out = engine.plan_dense(batch, tables=True, winner=True, traj_stride=stride)
    bare = engine.plan_dense(batch, tables=False, winner=True, traj_stride=stride)
    assert engine.get_option("clearance_launches") == launches + 2
    egos = list(range(batch.B)) if egos is None else egos
    cost, flags, idx, best = R.batch_tables(oracle, batch, egos=egos)
    assert np.array_equal(out.flags[egos], flags), what
    cost_close(out.cost[egos], cost, what + " cost table")
    assert np.array_equal(out.best_idx[egos], idx), (what, out.best_idx[egos], idx)
    cost_close(out.best_cost[egos], best, what + " best cost")
    assert np.array_equal(out.stats, np.tile([0, batch.C, batch.C, batch.C], (batch.B, 1))), what
    assert np.array_equal(bare.best_idx, out.best_idx) and np.array_equal(bare.best_cost, out.best_cost, equal_nan=True), what
    assert np.array_equal(bare.best_flags, out.best_flags) and np.array_equal(bare.best_traj, out.best_traj, equal_nan=True), what
    for k, e in enumerate(egos):
        if idx[k] >= 0:
            assert out.best_flags[e] == flags[k, idx[k]], what
            assert_series_close(out.best_traj[e], R.winner_series(oracle, batch, e, int(idx[k]), stride), batch.tick_t, f"{what} ego {e}")
        else:
            assert out.best_flags[e] == 0 and np.isnan(out.best_traj[e]).all() and np.isnan(out.best_cost[e]), what
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_dense_against_restatement(engine, oracle, name):
    batch = weighted(CASES[name]())
    out = check_against_restatement(engine, oracle, batch, what=name)
    plain = engine.plan_dense(weighted(CASES[name](), 0.0))
    assert (out.best_idx != plain.best_idx).sum() >= 2  # the term moved winners (the CPU fixture search says how many)


@pytest.mark.parametrize("stride", [1, 2])
def test_check_stride_invalid_rows_and_no_scene(engine, oracle, stride):
    batch = synth.make_batch(16, 5, 5, 5, 10, 100, True, 101)
    batch.check_stride = stride
    batch.obs_pose[:, 7::9, ::2, 3] = 0.0   # obstacles without a state at some steps
    batch.obs_pose[:, 30:, 1, 3] = 0.0      # an obstacle whose prediction ends early
    batch.scene_of[[2, 5]] = -1             # no obstacles: clearance 0, the plain winner and its cost, bit for bit
    weighted(batch)
    out = check_against_restatement(engine, oracle, batch, what=f"stride {stride}")
    plain = engine.plan_dense(weighted(batch, 0.0))
    for e in (2, 5):
        assert out.best_idx[e] == plain.best_idx[e] and np.array_equal(out.cost[e], plain.cost[e], equal_nan=True)


def test_ego_without_survivor(engine, oracle):
    batch = synth.make_batch(6, 5, 5, 5, 10, 100, True, 101)
    batch.max_speed = 1.0  # every candidate of these egos breaks the speed limit
    out = check_against_restatement(engine, oracle, weighted(batch), what="no survivor")
    assert (out.best_idx == -1).all()


def test_polygon_scenes(engine, oracle):
    from shapes_util import g12_batch, with_random_shapes

    g = load_golden("g12_shapes.npz")
    names = sorted({f[:-len("_in_ego")] for f in g.files if f.endswith("_in_ego") and "FISS" not in f})
    batch = weighted(g12_batch(g, names[0]))
    assert batch.obs_nvert is not None
    check_against_restatement(engine, oracle, batch, egos=list(range(min(batch.B, 6))), what="g12 " + names[0])
    rnd = weighted(with_random_shapes(synth.make_batch(8, 5, 5, 5, 10, 100, True, 101), 3))
    check_against_restatement(engine, oracle, rnd, what="random rings")


@pytest.mark.parametrize("kernel", [1, 2])
def test_lattice_kernel_options(engine, oracle, kernel):
    batch = weighted(synth.make_batch(8, 5, 5, 5, 10, 100, True, 101))
    engine.set_option("lattice_kernel", kernel)
    try:
        check_against_restatement(engine, oracle, batch, what=f"lattice_kernel {kernel}")
    finally:
        engine.set_option("lattice_kernel", 0)


def test_long_horizon(engine, oracle):
    batch = synth.make_batch(4, 5, 5, 3, 10, 200, True, 101)
    batch.tick_t = 0.05  # 160 .. 200 points per trajectory
    check_against_restatement(engine, oracle, weighted(batch), stride=208, what="tick 0.05")


def test_big_batch_invariants(engine):
    batch = synth.make_config(3)
    assert batch.B == 2048
    plain = engine.plan_dense(batch, winner=True)
    launches = engine.get_option("clearance_launches")
    zero = engine.plan_dense(weighted(batch, 0.0), winner=True)
    assert engine.get_option("clearance_launches") == launches  # w_obstacle = 0 launches nothing extra
    for k in ("best_idx", "best_cost", "cost", "flags", "stats", "best_flags", "best_traj"):
        assert np.array_equal(getattr(zero, k), getattr(plain, k), equal_nan=k in ("best_cost", "cost", "best_traj")), k
    one = engine.plan_dense(weighted(batch), winner=True)
    two = engine.plan_dense(batch, winner=True)
    for k in ("best_idx", "best_cost", "cost", "flags", "stats", "best_flags", "best_traj"):
        assert np.array_equal(getattr(one, k).view(np.uint8), getattr(two, k).view(np.uint8)), k  # two runs, the same bits
    assert np.array_equal(one.flags, plain.flags) and np.array_equal(one.stats, plain.stats)
    dead = (plain.flags & R.FLAG_INFEASIBLE) != 0
    assert np.array_equal(one.cost[dead], plain.cost[dead], equal_nan=True)
    assert (one.cost[~dead] >= plain.cost[~dead]).all() and (one.cost[~dead] > plain.cost[~dead]).any()
    assert np.array_equal(one.best_idx >= 0, plain.best_idx >= 0)
    rows = np.nonzero(one.best_idx >= 0)[0]
    assert np.array_equal(one.best_cost[rows], one.cost[rows, one.best_idx[rows]])
    assert (one.best_cost[rows] <= np.where(dead, np.inf, one.cost)[rows].min(axis=1)).all()


def test_device_calls_equal_host_calls(engine, oracle):
    import torch

    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch

    def fresh():
        return weighted(synth.make_batch(24, 5, 5, 5, 10, 100, True, 101))

    host = engine.plan_dense(fresh(), tables=True, winner=True)
    goal = np.tile([1e6, 1e6], (24, 1))
    results = []
    for fused in (True, False):
        run = ClosedLoopRunner(engine, DeviceBatch(fresh(), 0), goal, "FOP", fused=fused)
        run.done[[3, 4]] = 1  # finished egos (fp_batch.skip): not planned, not advanced
        launches = engine.get_option("clearance_launches")
        run.step()
        torch.cuda.synchronize()
        assert engine.get_option("clearance_launches") == launches + 1
        idx, cost = run.best_idx.cpu().numpy(), run.best_cost.cpu().numpy()
        live = np.ones(24, dtype=bool)
        live[[3, 4]] = False
        assert np.array_equal(idx[live], host.best_idx[live]) and np.array_equal(cost[live], host.best_cost[live], equal_nan=True)
        assert (idx[~live] == -1).all()
        free = torch.cuda.mem_get_info()[0]
        run.step()  # a second call of the same size allocates nothing
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free
        results.append((run.db.t["ego"].cpu().numpy(), run.db.t["t_now"].cpu().numpy(), run.done.cpu().numpy(), run.best_idx.cpu().numpy()))
    for a, b in zip(*results):  # fp_plan_step = fp_plan_dense + fp_advance
        assert np.array_equal(a, b, equal_nan=True)
    # the state the first cycle left behind is the winner's point 1 under the NEW cost
    b1 = fresh()
    for e in (0, 1, 2):
        if host.best_idx[e] >= 0:
            w = host.best_traj[e]
            start = ClosedLoopRunner(engine, DeviceBatch(fresh(), 0), goal, "FOP")
            start.step()
            torch.cuda.synchronize()
            got = start.db.t["ego"].cpu().numpy()[e]
            np.testing.assert_allclose(got, [w[1, 1], w[2, 1], w[3, 1], w[5, 1], w[6, 1], w[7, 1]], rtol=0, atol=1e-9)
            break
    assert b1.w_obstacle == W_TEST


def test_planner_classes(engine, oracle):
    from fiss_plus_planner_amd import planners as P
    from fiss_plus_planner_amd.closed_loop import run_closed_loop
    from fiss_plus_planner_amd.obstacles import ObstacleTable
    from fiss_plus_planner_amd.vehicle import Vehicle

    g = load_golden("g11_demo_scenarios.npz")
    name = str(g["names"][0])
    table = ObstacleTable(g[f"{name}_obs_pose"], g[f"{name}_obs_dims"], int(g[f"{name}_final_time_step"]))
    args = (g[f"{name}_centerline"], g[f"{name}_init_state"], table, g[f"{name}_goal_center"])
    st = P.FrenetOptimalPlannerSettings(5, 5, 5)
    st.w_obstacle = 0.1
    pl = P.FrenetOptimalPlanner(st, Vehicle(), None, engine=engine)
    launches = engine.get_option("clearance_launches")
    res = run_closed_loop(pl, *args, max_speed=float(g[f"{name}_max_speed"]), max_cycles=3)
    assert len(res.cycles) == 3 and engine.get_option("clearance_launches") == launches + 3
    batch = pl._batch_cache[1]  # the last cycle's problem
    assert batch.w_obstacle == 0.1
    out = engine.plan_dense(batch, winner=True)
    assert pl.best_traj.lattice_index == out.best_idx[0] and pl.best_traj.cost_final == out.best_cost[0]
    cost, flags, idx, best = R.ego_table(oracle, batch, 0)
    assert out.best_idx[0] == idx
    cost_close(out.cost[0], cost, "planner cycle")
    cost_close([pl.best_traj.cost_final], [best], "plan().cost_final")
    base = oracle.problems_from_batch(batch)[0].fop_plan()
    assert best >= base.cost[idx]  # (the term only ever adds)
    for cls, scls in ((P.FopPlusPlanner, P.FrenetOptimalPlannerSettings), (P.FissPlanner, P.FissPlannerSettings), (P.FissPlusPlanner, P.FissPlusPlannerSettings)):
        s2 = scls(5, 5, 5)
        s2.w_obstacle = 0.1
        with pytest.raises(ValueError, match="w_obstacle"):
            run_closed_loop(cls(s2, Vehicle(), None, engine=engine), *args, max_speed=float(g[f"{name}_max_speed"]), max_cycles=1)


def test_refusals_name_the_field(engine):
    batch = weighted(synth.make_batch(4, 5, 5, 5, 10, 100, True, 101, kind="FISS+"))
    launches = engine.get_option("clearance_launches")
    with pytest.raises(_abi.FrenetGpuError, match="w_obstacle"):
        engine.plan_fiss(batch, "FISS+")
    with pytest.raises(_abi.FrenetGpuError, match="w_obstacle"):
        engine.plan_fiss(batch, "FISS")
    with pytest.raises(_abi.FrenetGpuError, match="w_obstacle"):
        engine.plan_fopplus(batch)
    with pytest.raises(_abi.FrenetGpuError, match="w_obstacle"):
        engine.plan_dense(batch, audit=True)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(_abi.FrenetGpuError, match="w_obstacle"):
            engine.plan_dense(weighted(batch, bad))
    assert engine.get_option("clearance_launches") == launches
    # fp_eval_trajs prices arbitrary end states and ignores the weight
    es = np.tile([[0.3, 8.0, 9.0]], (4, 1, 1))
    a = engine.eval_trajs(weighted(batch, W_TEST), es)
    b = engine.eval_trajs(weighted(batch, 0.0), es)
    assert np.array_equal(a.cost, b.cost, equal_nan=True) and np.array_equal(a.flags, b.flags)
