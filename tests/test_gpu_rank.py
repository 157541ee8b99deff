"""GPU: fp_rank_feasible (the K cheapest survivors of every ego, ranked on the device) against its numpy restatement
(tests/rank_ref.py) on the GPU's own tables - bit for bit: the kernel only orders what it is given -, against the oracle's tables on
the fixture batches (tests/test_rank_cpu.py shows they have no near ties, so every rank position is compared), and through the entry
points that take a rank plane as their best_idx."""
import ctypes as C

import numpy as np
import pytest

import rank_ref as R
from conftest import load_golden, batch_from_golden
from fiss_plus_planner_amd import _abi, synth
from fiss_plus_planner_amd.engine import host_structs
from lattice_paths import cost_close
from test_gpu_edges import series_check
from test_rank_cpu import FIXTURES, oracle_tables, tie_batch

pytestmark = pytest.mark.gpu
KS = (1, 7, 64)


def rank(engine, batch, cost, flags, K, skip=None, count=True):
    """fp_rank_feasible(FP_MEM_HOST) through ctypes."""
    B = batch.B
    p, fb = host_structs(batch)
    cost, flags = np.ascontiguousarray(cost, dtype=np.float64), np.ascontiguousarray(flags, dtype=np.uint32)
    assert cost.shape == flags.shape == (B, batch.C)
    if skip is not None:
        skip = np.ascontiguousarray(skip, dtype=np.int32)
        fb.skip = skip.ctypes.data
    ri, rc, n = np.full((K, B), -7, dtype=np.int32), np.full((K, B), -7.0), np.full(B, -7, dtype=np.int32)
    _abi.check(engine._lib.fp_rank_feasible(engine._ctx, C.byref(p), C.byref(fb), cost.ctypes.data, flags.ctypes.data, K, ri.ctypes.data, rc.ctypes.data,
                                            n.ctypes.data if count else None, _abi.FP_MEM_HOST, None))
    return ri, rc, n


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def assert_ranked(got, want, what):
    (ri, rc, n), (wi, wc, wn) = got, want
    assert np.array_equal(ri, wi), (what, np.argwhere(ri != wi)[:4].tolist())
    assert np.array_equal(np.isnan(rc), wi < 0) and same_bits(np.where(wi < 0, 0.0, rc), np.where(wi < 0, 0.0, wc)), what
    assert np.array_equal(n, wn), what


def check_tables(engine, batch, cost, flags, what, Ks=KS, skip=None):
    for K in Ks:
        assert_ranked(rank(engine, batch, cost, flags, K, skip), R.rank_tables(cost, flags, K, skip), f"{what} K={K}")


def check_batch(engine, batch, what, Ks=KS):
    """plan_dense + ranking of its tables: the restatement on the same tables, and plane 0 == best_idx / best_cost of the call."""
    out = engine.plan_dense(batch, tables=True)
    check_tables(engine, batch, out.cost, out.flags, what, Ks)
    ri, rc, n = rank(engine, batch, out.cost, out.flags, Ks[0])
    assert np.array_equal(ri[0], out.best_idx), what
    assert same_bits(np.where(ri[0] < 0, 0.0, rc[0]), np.where(out.best_idx < 0, 0.0, out.best_cost)) and np.array_equal(np.isnan(rc[0]), np.isnan(out.best_cost)), what
    return out


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixture_batches_against_restatement_and_oracle(engine, oracle, name):
    batch = FIXTURES[name]()
    out = check_batch(engine, batch, name)
    # the oracle's tables, every rank position: indices and counts exact, costs within the project's bar
    ocost, oflags = oracle_tables(oracle, batch)
    ri, rc, n = rank(engine, batch, out.cost, out.flags, 64)
    wi, wc, wn = R.rank_tables(ocost, oflags, 64)
    assert np.array_equal(ri, wi), (name, np.argwhere(ri != wi)[:4].tolist())
    assert np.array_equal(n, wn)
    cost_close(rc, wc, name + " rank_cost")
    assert (n > 64).any() or name == "5x5x5"


def test_polygon_scenes_and_clearance_tables(engine):
    poly = synth.with_random_shapes(synth.make_batch(8, 5, 5, 5, 10, 100, True, 101), 3)
    assert poly.obs_nvert is not None
    check_batch(engine, poly, "random rings")
    priced = synth.make_batch(16, 5, 5, 5, 10, 100, True, 101)
    plain = engine.plan_dense(priced, tables=True)
    priced.w_obstacle = 0.1
    n0 = engine.get_option("clearance_launches")
    out = check_batch(engine, priced, "w_obstacle")
    assert engine.get_option("clearance_launches") > n0 and not np.array_equal(out.cost, plain.cost, equal_nan=True)


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 5, 5), (9, 9, 7), (10, 10, 41), (64, 16, 16)])
def test_lattice_sizes_all_surviving_and_none(engine, shape):
    nd, nv, nt = shape
    batch = synth.make_batch(3 if nd < 64 else 1, nd, nv, nt, 6, 50, True, 3500)
    Cn = batch.C
    assert Cn == nd * nv * nt and Cn in (1, 125, 567, 4100, _abi.FP_MAX_CAND)
    out = check_batch(engine, batch, f"C={Cn}")
    idx = np.arange(Cn, dtype=np.float64)
    every = out.flags & ~np.uint32(R.FLAG_INFEASIBLE)
    # all survive: the GPU's costs (NaN replaced), descending costs (every chunk beats the threshold: the most cuts the kernel can
    # take), a handful of values repeated across the whole row (ties across cuts), all equal
    for label, cost in (("own", np.where(np.isnan(out.cost), 1e3 + idx, out.cost)), ("descending", np.tile(Cn - idx, (batch.B, 1))),
                        ("repeats", np.tile(idx % 7, (batch.B, 1))), ("equal", np.full((batch.B, Cn), 2.5)),
                        ("signed zeros and infinities", np.tile(np.where(idx % 3 == 0, -0.0, np.where(idx % 3 == 1, 0.0, np.inf)), (batch.B, 1)))):
        check_tables(engine, batch, cost, every, f"C={Cn} all survive, {label}")
        ri, rc, n = rank(engine, batch, cost, every, 64)
        assert (n == Cn).all()
        again = rank(engine, batch, cost, every, 64)
        assert same_bits(ri, again[0]) and same_bits(rc, again[1])  # two runs, the same bits
    none = out.flags | np.uint32(_abi.FLAG_SPEED)
    check_tables(engine, batch, out.cost, none, f"C={Cn} none survive")
    ri, rc, n = rank(engine, batch, out.cost, none, 7)
    assert (ri == -1).all() and np.isnan(rc).all() and (n == 0).all()
    ri, _, n = rank(engine, batch, np.full((batch.B, Cn), np.nan), every, 7)  # NaN costs without a bit: no survivors either
    assert (ri == -1).all() and (n == 0).all()
    ri2, rc2, n2 = rank(engine, batch, out.cost, out.flags, 7, count=False)  # n_feasible is optional
    assert (n2 == -7).all() and np.array_equal(ri2, R.rank_tables(out.cost, out.flags, 7)[0])


def test_skipped_egos_rows_are_not_read(engine):
    batch = FIXTURES["5x5x5"]()
    out = engine.plan_dense(batch, tables=True)
    skip = np.zeros(batch.B, dtype=np.int32)
    skip[[0, 3, 17, 63]] = 1
    cost, flags = out.cost.copy(), out.flags.copy()
    cost[skip != 0], flags[skip != 0] = -1.0, 0  # rows that WOULD rank if they were read
    check_tables(engine, batch, cost, flags, "skip", skip=skip)
    ri, rc, n = rank(engine, batch, cost, flags, 7, skip)
    assert (ri[:, skip != 0] == -1).all() and np.isnan(rc[:, skip != 0]).all() and (n[skip != 0] == 0).all()
    assert np.array_equal(ri[0, skip == 0], out.best_idx[skip == 0])


def test_exact_ties_put_the_higher_index_first(engine, oracle):
    batch = tie_batch()
    out = check_batch(engine, batch, "mirror ties")
    ri, rc, n = rank(engine, batch, out.cost, out.flags, 64)
    m = min(int(n[0]), 64)
    same = np.nonzero(rc[:m - 1, 0] == rc[1:m, 0])[0]
    assert same.size >= 2 and (ri[same, 0] > ri[same + 1, 0]).all()
    assert ri[0, 0] == oracle.problems_from_batch(batch)[0].fop_plan().best_idx


def test_multi_round_dispatch(engine):
    """resident_groups = 2: a handful of egos takes the dense pass's multi-round instances; the ranking sees their tables."""
    batch = synth.make_batch(12, 9, 9, 7, 50, 100, True, 7)
    ref = engine.plan_dense(batch, tables=True)
    engine.set_option("resident_groups", 2)
    try:
        out = check_batch(engine, batch, "resident_groups 2", Ks=(7,))
    finally:
        engine.set_option("resident_groups", 0)
    assert np.array_equal(out.best_idx, ref.best_idx) and np.array_equal(out.flags, ref.flags)


def test_rank_planes_through_winner_trajs(engine, oracle):
    batch = synth.make_batch(16, 5, 5, 5, 10, 100, True, 101)
    out = engine.plan_dense(batch, tables=True)
    K = 7
    ri, rc, n = rank(engine, batch, out.cost, out.flags, K)
    seen = 0
    for k in (0, 1, K - 1):
        w = engine.winner_trajs(batch, ri[k])
        seen += series_check(oracle, batch, ri[k], w.best_traj, 128, f"rank plane {k}")
        live = ri[k] >= 0
        assert np.array_equal(w.best_flags[live], out.flags[live, ri[k][live]]) and (w.best_flags[~live] == 0).all()
    assert seen >= 3 * 8


def test_engine_api(engine):
    batch = FIXTURES["5x5x5"]()
    ref = engine.plan_dense(batch, tables=True)
    want = R.rank_tables(ref.cost, ref.flags, 7)
    assert_ranked(engine.rank_feasible(batch, ref.cost, ref.flags, 7), want, "rank_feasible")
    out = engine.plan_dense(batch, tables=False, top_k=7)
    assert out.cost is None and out.flags is None and np.array_equal(out.best_idx, ref.best_idx)
    assert_ranked((out.rank_idx, out.rank_cost, out.n_feasible), want, "plan_dense(top_k)")
    out = engine.plan_dense(batch, tables=True, winner=True, top_k=64)
    assert np.array_equal(out.cost, ref.cost, equal_nan=True)
    assert_ranked((out.rank_idx, out.rank_cost, out.n_feasible), R.rank_tables(ref.cost, ref.flags, 64), "plan_dense(tables, top_k)")
    assert not hasattr(engine.plan_dense(batch), "rank_idx")
    with pytest.raises(ValueError, match="top_k"):
        engine.plan_dense(batch, top_k=65)


def test_device_calls_graph_replay_and_counter(engine):
    import torch

    from fiss_plus_planner_amd.device_batch import DeviceBatch

    first, second = synth.make_batch(48, 9, 9, 7, 50, 100, True, 7), synth.make_batch(48, 9, 9, 7, 50, 100, True, 8)
    K, B, Cn = 7, first.B, first.C
    db = DeviceBatch(first, 0)
    dev = db.dev
    best_idx, best_cost = db.empty(B, torch.int32), db.empty(B, torch.float64)
    cost, flags = db.empty((B, Cn), torch.float64), db.empty((B, Cn), torch.int32)
    ri, rc, nf = db.empty((K, B), torch.int32), db.empty((K, B), torch.float64), db.empty(B, torch.int32)

    def pair(stream):
        engine.plan_dense_device(db.params, db.fb, best_idx.data_ptr(), best_cost.data_ptr(), cost_tbl=cost.data_ptr(), flag_tbl=flags.data_ptr(), stream=stream)
        engine.rank_feasible_device(db.params, db.fb, cost.data_ptr(), flags.data_ptr(), K, ri.data_ptr(), rc.data_ptr(), nf.data_ptr(), stream=stream)

    def fetch():
        torch.cuda.synchronize(dev)
        return ri.cpu().numpy(), rc.cpu().numpy(), nf.cpu().numpy(), best_idx.cpu().numpy(), best_cost.cpu().numpy()

    def load(batch):  # a second batch state in the same device arrays
        for k in ("ego", "v_samples", "target_speed", "knots", "coef", "obs_pose", "obs_dims"):
            db.t[k].copy_(torch.from_numpy(np.ascontiguousarray(getattr(batch, k))))

    def clear():
        ri.fill_(-9); rc.fill_(-9.0); nf.fill_(-9)

    n0 = engine.get_option("rank_launches")
    pair(torch.cuda.current_stream(dev).cuda_stream)  # eager, first state (also the warm-up of the capture)
    eager1 = fetch()
    assert engine.get_option("rank_launches") == n0 + 1
    host1 = engine.plan_dense(first, tables=True)
    assert_ranked(eager1[:3], R.rank_tables(host1.cost, host1.flags, K), "device call, first state")
    assert np.array_equal(eager1[0][0], eager1[3]) and np.array_equal(eager1[1][0], eager1[4], equal_nan=True)
    free = torch.cuda.mem_get_info()[0]
    pair(torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert torch.cuda.mem_get_info()[0] == free  # enqueue only: a second call allocates nothing
    side = torch.cuda.Stream(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        pair(side.cuda_stream)
    torch.cuda.synchronize(dev)
    assert engine.get_option("rank_launches") == n0 + 3
    load(second)
    clear()
    pair(torch.cuda.current_stream(dev).cuda_stream)  # eager, second state
    eager2 = fetch()
    clear()
    graph.replay()
    replay2 = fetch()
    for a, b in zip(eager2, replay2):
        assert same_bits(a, b)
    host2 = engine.plan_dense(second, tables=True)
    assert_ranked(replay2[:3], R.rank_tables(host2.cost, host2.flags, K), "graph replay, second state")
    assert not np.array_equal(eager1[0], eager2[0])
    assert engine.get_option("rank_launches") == n0 + 4  # (a replay is not a call)
    # the k-th plane is a best_idx argument as it stands: the series of the runners-up, on the device
    bf, bt = db.empty(B, torch.int32), db.empty((B, 16, 128), torch.float64)
    engine.winner_trajs_device(db.params, db.fb, ri.data_ptr() + 4 * B, bf.data_ptr(), bt.data_ptr())
    torch.cuda.synchronize(dev)
    w = engine.winner_trajs(second, replay2[0][1])
    assert same_bits(bt.cpu().numpy(), w.best_traj) and np.array_equal(bf.cpu().numpy().view(np.uint32), w.best_flags)


def test_ranking_is_opt_in(engine):
    """A caller that never asks launches no ranking kernel: a plain dense call, a FISS+ call and a closed loop leave the ctx's counter
    where it was (on a ctx that never ranked it is still 0; the session's engine has, so the count before is the zero here)."""
    import torch

    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch

    n0 = engine.get_option("rank_launches")
    engine.plan_dense(synth.make_batch(8, 5, 5, 5, 10, 100, True, 101), tables=True, winner=True)
    engine.plan_fiss(synth.make_batch(8, 5, 5, 5, 10, 100, True, 101, kind="FISS+"), "FISS+")
    batch = synth.make_batch(8, 5, 5, 5, 10, 100, True, 101)
    ClosedLoopRunner(engine, DeviceBatch(batch, 0), np.tile([1e6, 1e6], (8, 1)), "FOP").run(3)
    torch.cuda.synchronize()
    assert engine.get_option("rank_launches") - n0 == 0
    out = engine.plan_dense(batch)
    engine.rank_feasible(batch, out.cost, out.flags, 3)
    assert engine.get_option("rank_launches") - n0 == 1


def test_errors(engine):
    batch = synth.make_batch(4, 5, 5, 5, 10, 100, True, 101)
    out = engine.plan_dense(batch, tables=True)
    n0 = engine.get_option("rank_launches")
    for K in (0, 65, -1):
        with pytest.raises(_abi.FrenetGpuError, match="K=") as ex:
            _raw(engine, batch, out, K)
        assert ex.value.code == -1
    p, fb = host_structs(batch)
    ri, rc = np.empty((4, 4), dtype=np.int32), np.empty((4, 4))
    args = dict(cost=out.cost.ctypes.data, flags=out.flags.ctypes.data, ri=ri.ctypes.data, rc=rc.ctypes.data)
    for missing in args:
        a = dict(args, **{missing: None})
        rcode = engine._lib.fp_rank_feasible(engine._ctx, C.byref(p), C.byref(fb), a["cost"], a["flags"], 4, a["ri"], a["rc"], None, _abi.FP_MEM_HOST, None)
        assert rcode == -1, missing
    big = _abi.FpParams.from_buffer_copy(p)
    big.nd, big.nv, big.nt = 5, 29, 113  # FP_MAX_CAND + 1
    rcode = engine._lib.fp_rank_feasible(engine._ctx, C.byref(big), C.byref(fb), args["cost"], args["flags"], 4, args["ri"], args["rc"], None, _abi.FP_MEM_HOST, None)
    assert rcode == -4 and b"FP_MAX_CAND" in engine._lib.fp_last_error()
    assert engine.get_option("rank_launches") == n0


def _raw(engine, batch, out, K):
    p, fb = host_structs(batch)
    ri, rc = np.empty((65, batch.B), dtype=np.int32), np.empty((65, batch.B))
    _abi.check(engine._lib.fp_rank_feasible(engine._ctx, C.byref(p), C.byref(fb), out.cost.ctypes.data, out.flags.ctypes.data, K, ri.ctypes.data, rc.ctypes.data,
                                            None, _abi.FP_MEM_HOST, None))


def test_planner_class_alternatives(engine):
    from fiss_plus_planner_amd import planners as P
    from test_gpu_planners import TOL, _check_winner, _g4_keys, _inputs, _planner

    g = load_golden("g4_plan.npz")
    key = [k for k in _g4_keys() if k.endswith("_FOP")][0]
    b = batch_from_golden(g, f"{key}_in_")
    e = int(np.nonzero(g[f"{key}_found"])[0][0])
    pts, fs, obs = _inputs(b, e)
    pl = _planner("FOP", b, engine)
    pl.settings.num_alternatives = 5
    pl.generate_frenet_frame(pts)
    n0 = engine.get_option("rank_launches")
    best = pl.plan(fs, float(b.target_speed[e]), obs, int(b.t_now[e]))
    assert engine.get_option("rank_launches") == n0 + 1
    alts = pl.alternatives
    assert 1 <= len(alts) <= 5 and alts[0] is best
    assert alts[0].lattice_index == g[f"{key}_flat"][e] and abs(alts[0].cost_final - g[f"{key}_cost"][e]) < TOL
    _check_winner(alts[0], g[f"{key}_win"][e], g[f"{key}_NM"][e])
    costs = [a.cost_final for a in alts]
    assert costs == sorted(costs)
    wi, wc, wn = R.rank_tables(pl.last_tables[0][None], pl.last_tables[1][None], 5)
    assert [a.lattice_index for a in alts] == wi[:len(alts), 0].tolist() and len(alts) == min(5, int(wn[0]))
    assert np.array_equal(costs, wc[:len(alts), 0])
    for a in alts[1:]:
        fl = int(pl.last_tables[1][a.lattice_index])
        assert len(a.t) == (fl >> 8) & 0xFFF and len(a.x) == fl >> 20 and a.lattice_index != best.lattice_index
    # off unless asked for
    pl.settings.num_alternatives = 0
    n0 = engine.get_option("rank_launches")
    pl.plan(fs, float(b.target_speed[e]), obs, int(b.t_now[e]))
    assert not hasattr(pl, "alternatives") and engine.get_option("rank_launches") == n0
    fresh = _planner("FOP", b, engine)
    fresh.generate_frenet_frame(pts)
    fresh.plan(fs, float(b.target_speed[e]), obs, int(b.t_now[e]))
    assert not hasattr(fresh, "alternatives") and P.FrenetOptimalPlannerSettings().num_alternatives == 0
    for kind in ("FOP+", "FISS", "FISS+"):
        other = _planner(kind, b, engine)
        other.settings.num_alternatives = 3
        other.generate_frenet_frame(pts)
        with pytest.raises(ValueError, match="num_alternatives"):
            other.plan(fs, float(b.target_speed[e]), obs, int(b.t_now[e]))
    assert engine.get_option("rank_launches") == n0
