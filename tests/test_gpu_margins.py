"""GPU: fp_traj_margins (the obstacle margin of chosen plans) through ctypes against its restatement (tests/margins_ref.py): min_dist
within 1e-9 m, +inf / NaN exact, a reference 0 is 0, min_step / min_obs exact on every counted plan (tests/test_margins_cpu.py shows
the fixtures are decidable); then consistency with the dense pass, the end-state path, determinism and neutrality, the refusals and
the planner classes."""
import ctypes as C

import numpy as np
import pytest

import margins_ref as MR
from fiss_plus_planner_amd import _abi, synth
from fiss_plus_planner_amd.engine import host_structs
from test_margins_cpu import FIXTURES, KS, _edges, fixture_reference, hand_cases
from test_gpu_rank import rank, same_bits

pytestmark = pytest.mark.gpu


def margins(engine, batch, best_idx=None, end_state=None, pose_stride=None, skip=None):
    """fp_traj_margins(FP_MEM_HOST) through ctypes: best_idx [K, B] / end_state [K, B, 3] -> (min_dist, min_step, min_obs) [K, B]."""
    B = batch.B
    p, fb = host_structs(batch)
    if skip is not None:
        skip = np.ascontiguousarray(skip, dtype=np.int32)
        fb.skip = skip.ctypes.data
    if best_idx is not None:
        plans = np.ascontiguousarray(best_idx, dtype=np.int32).reshape(-1, B)
    else:
        plans = np.ascontiguousarray(end_state, dtype=np.float64).reshape(-1, B, 3)
    K = plans.shape[0]
    d, i, j = np.full((K, B), -7.0), np.full((K, B), -7, dtype=np.int32), np.full((K, B), -7, dtype=np.int32)
    _abi.check(engine._lib.fp_traj_margins(engine._ctx, C.byref(p), C.byref(fb), K, plans.ctypes.data if best_idx is not None else None,
                                           plans.ctypes.data if best_idx is None else None, int(batch.check_stride if pose_stride is None else pose_stride),
                                           d.ctypes.data, i.ctypes.data, j.ctypes.data, _abi.FP_MEM_HOST, None))
    return d, i, j


def assert_margins(got, ref, what, planes=slice(None), min_share=MR.MIN_COUNTED):
    d, i, j = got
    rd, ri, rj = ref.min_dist[planes], ref.min_step[planes], ref.min_obs[planes]
    assert d.shape == rd.shape, what
    assert np.array_equal(np.isnan(d), np.isnan(rd)), (what, np.argwhere(np.isnan(d) != np.isnan(rd))[:4].tolist())
    assert np.array_equal(np.isinf(d), np.isinf(rd)) and (d[np.isinf(d)] > 0).all(), (what, np.argwhere(np.isinf(d) != np.isinf(rd))[:4].tolist())
    fin = np.isfinite(rd)
    err = np.abs(d[fin] - rd[fin])
    print(f"{what}: {int(fin.sum())} finite plans, max |min_dist - ref| = {err.max() if err.size else 0.0:.3e}, contacts {int((rd[fin] == 0).sum())}")
    assert (err <= MR.DIST_TOL).all(), (what, float(err.max()))
    assert (d[rd == 0.0] == 0.0).all(), what
    none = ~fin
    assert (i[none] == -1).all() and (j[none] == -1).all(), what
    cnt = MR.counted(ref)[planes]
    assert np.array_equal(i[cnt], ri[cnt]) and np.array_equal(j[cnt], rj[cnt]), (what, np.argwhere(cnt & ((i != ri) | (j != rj)))[:4].tolist())
    has = ref.n_pairs[planes] > 0
    if has.any():
        assert cnt[has].mean() >= min_share, (what, float(cnt[has].mean()))
    assert ((i[fin] >= 0) & (j[fin] >= 0)).all(), what


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_made_cases(engine, name):
    batch, stride, (dist, step, obs) = hand_cases()[name]
    d, i, j = margins(engine, batch, best_idx=[[0]], pose_stride=stride)
    assert (int(i[0, 0]), int(j[0, 0])) == (step, obs), (name, d, i, j)
    assert d[0, 0] == dist if not np.isfinite(dist) or dist == 0.0 else abs(d[0, 0] - dist) < 1e-9, (name, d)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixtures_against_the_reference(engine, oracle, name):
    """K = 1 (plain best_idx), K = 7 and 64 (planes of fp_rank_feasible on the GPU's own tables, with their -1 planes) at every pose
    stride of the fixture."""
    batch = FIXTURES[name][0]()
    out = engine.plan_dense(batch, tables=True)
    ri = rank(engine, batch, out.cost, out.flags, 64)[0]
    assert np.array_equal(ri[0], out.best_idx)
    for stride in FIXTURES[name][1]:
        _, planes, ref = fixture_reference(oracle, name, stride)
        if not np.array_equal(planes, ri):  # (the GPU ranks a near tie the other way: the reference of ITS planes)
            _, planes, ref = fixture_reference(oracle, name, stride, planes=ri)
        for K in KS:
            got = margins(engine, batch, best_idx=out.best_idx[None] if K == 1 else ri[:K], pose_stride=stride)
            assert_margins(got, ref, f"{name} stride {stride} K={K}", slice(0, K), min_share=0.0 if K < 64 else MR.MIN_COUNTED)
    if name == "truncated":
        live = ri >= 0
        assert ((out.flags[np.nonzero(live)[1], ri[live]] & _abi.FLAG_TRUNCATED) != 0).any()
    if name == "tick 0.05":
        assert ((out.flags >> 8) & 0xFFF).max() > 128


def test_skip_scene_and_horizon_edges(engine, oracle):
    batch = _edges()
    out = engine.plan_dense(batch, tables=True)
    skip = np.array([0, 0, 0, 0, 1], dtype=np.int32)
    planes = np.stack([out.best_idx, np.full(5, 62), np.full(5, -1)]).astype(np.int32)
    planes[1, 4] = 10 ** 6  # the skipped ego's entries are not looked at, whatever they hold
    for stride in (1, 2):
        ref = MR.margins(oracle, batch, best_idx=planes, pose_stride=stride, skip=skip)
        got = margins(engine, batch, best_idx=planes, pose_stride=stride, skip=skip)
        assert_margins(got, ref, f"edges stride {stride}", min_share=0.0)
        d, i, j = got
        assert np.isnan(d[:, 4]).all() and np.isnan(d[2]).all() and (d[1, 1] == np.inf) and (d[1, 3] == np.inf)
        assert np.isfinite(d[1, 2]) and i[1, 2] == 0 and np.isfinite(d[1, 0])


def test_consistent_with_the_dense_pass(engine, oracle):
    """pose_stride = check_stride on plan_dense's tables: a survivor never touches anything, a candidate the collision check rejected
    is in contact - at the reference's first contact pose."""
    batch = synth.make_batch(5, 5, 5, 5, 50, 100, True, 4003)
    out = engine.plan_dense(batch, tables=True)
    bits = out.flags & _abi.FLAG_INFEASIBLE
    alive = (bits == 0) & ~np.isnan(out.cost)
    hit = (out.flags & _abi.FLAG_COLLISION) != 0
    assert alive.sum() >= 20 and hit.sum() >= 20
    every = np.tile(np.arange(batch.C, dtype=np.int32)[:, None], (1, batch.B))  # [C, B]: every candidate as a plane, 64 at a time
    chunks = [margins(engine, batch, best_idx=every[c0:c0 + 64]) for c0 in range(0, batch.C, 64)]
    d, i = np.concatenate([c[0] for c in chunks]).T, np.concatenate([c[1] for c in chunks]).T
    assert (d[alive] > 0).all()
    assert (d[hit] == 0).all()
    cand = np.argwhere(hit)[:: max(1, int(hit.sum()) // 24)]
    for b, c in cand:
        planes = np.full((1, batch.B), -1)
        planes[0, b] = c
        ref = MR.margins(oracle, batch, best_idx=planes)
        assert ref.min_dist[0, b] == 0.0 and i[b, c] == ref.min_step[0, b], (b, c)


@pytest.mark.parametrize("horizon", [99, 15])
def test_rows_in_lds_and_rows_from_the_scene_table_give_the_same_bits(engine, horizon):
    """One batch through both kernel paths: 40 obstacles x 100 rows are staged in LDS at pose_stride 1 (128 KB of rows); the same
    table padded with 30 rows in which no column is valid (beyond final_time_step: never looked at) is past the staging budget and
    is read from the scene table.  horizon 15: 15 poses per plan, four lanes per pose on both paths."""
    staged = synth.make_batch(5, 5, 5, 5, 40, 100, True, 4008)
    staged.final_time_step[:] = horizon
    padded = synth.make_batch(5, 5, 5, 5, 40, 100, True, 4008)
    padded.final_time_step[:] = horizon
    padded.obs_pose = np.ascontiguousarray(np.concatenate([padded.obs_pose, np.zeros((5, 30, 40, 4))], axis=1))
    assert padded.T_obs == 130 and staged.T_obs * 40 * 32 < 144 * 1024 - 9 * 81 * 8 - 40 * 32 < 144 * 1024 < 128 * 40 * 32
    out = engine.plan_dense(staged, tables=True)
    ri = rank(engine, staged, out.cost, out.flags, 64)[0]
    a, b = margins(engine, staged, best_idx=ri, pose_stride=1), margins(engine, padded, best_idx=ri, pose_stride=1)
    for x, y in zip(a, b):
        assert same_bits(x, y)
    assert np.isfinite(a[0]).sum() >= 64


def test_end_states_of_lattice_candidates_give_the_same_bits(engine):
    batch = FIXTURES["3 obstacles"][0]()
    out = engine.plan_dense(batch, tables=True)
    ri = rank(engine, batch, out.cost, out.flags, 7)[0]
    es = np.full((7, batch.B, 3), np.nan)
    for k in range(7):
        for b in range(batch.B):
            if ri[k, b] >= 0:
                es[k, b] = MR.end_state_of(batch, b, int(ri[k, b]))
    for stride in (1, 2):
        a, b2 = margins(engine, batch, best_idx=ri, pose_stride=stride), margins(engine, batch, end_state=es, pose_stride=stride)
        for x, y in zip(a, b2):
            assert same_bits(x, y)
    assert np.isfinite(a[0]).any()


def test_refined_fissplus_winner(engine, oracle):
    batch = synth.make_batch(8, 5, 5, 5, 10, 100, True, 101, kind="FISS+")
    out = engine.plan_fiss(batch, "FISS+")
    assert (out.refined != 0).any()
    for stride in (1, 2):
        ref = MR.margins(oracle, batch, end_state=out.end_state[None], pose_stride=stride)
        assert_margins(margins(engine, batch, end_state=out.end_state[None], pose_stride=stride), ref, f"FISS+ winners stride {stride}", min_share=0.0)
        d = margins(engine, batch, end_state=out.end_state[None], pose_stride=stride)[0]
        assert np.array_equal(np.isnan(d[0]), np.isnan(out.best_cost))
    assert (margins(engine, batch, end_state=out.end_state[None])[0][0][~np.isnan(out.best_cost)] > 0).all()  # (winners passed the collision check)


def test_device_calls_equal_host_calls_and_replay_in_a_graph(engine):
    import torch

    from fiss_plus_planner_amd.device_batch import DeviceBatch

    batch = synth.make_batch(48, 9, 9, 7, 50, 100, True, 7)
    K, B, Cn = 7, batch.B, batch.C
    db = DeviceBatch(batch, 0)
    dev = db.dev
    best_idx, best_cost = db.empty(B, torch.int32), db.empty(B, torch.float64)
    cost, flags = db.empty((B, Cn), torch.float64), db.empty((B, Cn), torch.int32)
    ri, rc = db.empty((K, B), torch.int32), db.empty((K, B), torch.float64)
    md, ms, mo = db.empty((K, B), torch.float64), db.empty((K, B), torch.int32), db.empty((K, B), torch.int32)

    def chain(stream, stride=None):
        engine.plan_dense_device(db.params, db.fb, best_idx.data_ptr(), best_cost.data_ptr(), cost_tbl=cost.data_ptr(), flag_tbl=flags.data_ptr(), stream=stream)
        engine.rank_feasible_device(db.params, db.fb, cost.data_ptr(), flags.data_ptr(), K, ri.data_ptr(), rc.data_ptr(), stream=stream)
        engine.traj_margins_device(db.params, db.fb, K, md.data_ptr(), ms.data_ptr(), mo.data_ptr(), best_idx=ri.data_ptr(), pose_stride=stride, stream=stream)

    def fetch():
        torch.cuda.synchronize(dev)
        return md.cpu().numpy(), ms.cpu().numpy(), mo.cpu().numpy()

    def clear():
        md.fill_(-9.0); ms.fill_(-9); mo.fill_(-9)

    cur = torch.cuda.current_stream(dev).cuda_stream
    n0 = engine.get_option("margin_launches")
    chain(cur)
    eager = fetch()
    assert engine.get_option("margin_launches") == n0 + 1
    host = margins(engine, batch, best_idx=ri.cpu().numpy())
    for a, b in zip(eager, host):
        assert same_bits(a, b)  # FP_MEM_DEVICE equals FP_MEM_HOST
    clear()  # (before the measurement: the first fill kernel of a process loads its code object)
    torch.cuda.synchronize(dev)
    free = torch.cuda.mem_get_info()[0]
    chain(cur)
    again = fetch()
    assert torch.cuda.mem_get_info()[0] == free  # enqueue only: nothing is allocated
    for a, b in zip(eager, again):
        assert same_bits(a, b)  # two runs, the same bits
    # with a launch order
    order = torch.from_numpy(np.ascontiguousarray(np.argsort(-batch.ego[:, 1], kind="stable").astype(np.int32))).to(dev)
    fb2 = _abi.FpBatch.from_buffer_copy(db.fb)
    fb2.launch_order = order.data_ptr()
    clear()
    engine.traj_margins_device(db.params, fb2, K, md.data_ptr(), ms.data_ptr(), mo.data_ptr(), best_idx=ri.data_ptr(), stream=cur)
    for a, b in zip(eager, fetch()):
        assert same_bits(a, b)
    # pose_stride 1 through the device entry, against the host entry
    clear()
    engine.traj_margins_device(db.params, db.fb, K, md.data_ptr(), ms.data_ptr(), mo.data_ptr(), best_idx=ri.data_ptr(), pose_stride=1, stream=cur)
    for a, b in zip(fetch(), margins(engine, batch, best_idx=ri.cpu().numpy(), pose_stride=1)):
        assert same_bits(a, b)
    # an index beyond the lattice is "no trajectory" for a device caller
    bad = ri.clone()
    bad[0, 0] = Cn
    clear()
    engine.traj_margins_device(db.params, db.fb, K, md.data_ptr(), ms.data_ptr(), mo.data_ptr(), best_idx=bad.data_ptr(), stream=cur)
    d, i, j = fetch()
    assert np.isnan(d[0, 0]) and i[0, 0] == -1 and j[0, 0] == -1 and same_bits(d[1:], eager[0][1:])
    # captured behind the dense call and the ranking
    side = torch.cuda.Stream(dev)
    graph = torch.cuda.CUDAGraph()
    n1 = engine.get_option("margin_launches")
    with torch.cuda.graph(graph, stream=side):
        chain(side.cuda_stream)
    torch.cuda.synchronize(dev)
    clear()
    graph.replay()
    for a, b in zip(eager, fetch()):
        assert same_bits(a, b)
    assert engine.get_option("margin_launches") == n1 + 1  # (a replay is not a call)


def test_margins_are_opt_in(engine):
    """A fresh ctx has launched nothing; a caller that never asks gets the bits and the launch counts it got before."""
    from fiss_plus_planner_amd.engine import FrenetEngine

    batch = synth.make_batch(8, 5, 5, 5, 10, 100, True, 101)
    with FrenetEngine(0) as fresh:
        assert fresh.get_option("margin_launches") == 0
        names = ("margin_launches", "rank_launches", "boundary_launches", "clearance_launches", "lattice_launches")
        before = [fresh.get_option(n) for n in names]
        plain = fresh.plan_dense(batch, tables=True, winner=True)
        after = [fresh.get_option(n) for n in names]
        assert [a - b for a, b in zip(after, before)] == [0, 0, 0, 0, 1]
        assert not hasattr(plain, "margin_dist")
        with_m = fresh.plan_dense(batch, tables=True, winner=True, margins=True)
        assert fresh.get_option("margin_launches") == 1 and fresh.get_option("lattice_launches") == after[4] + 1
        for k in ("best_idx", "best_cost", "cost", "flags", "best_traj", "best_flags", "stats"):
            assert same_bits(getattr(plain, k), getattr(with_m, k)), k
        d, i, j = margins(fresh, batch, best_idx=plain.best_idx[None])
        assert same_bits(with_m.margin_dist, d[0]) and same_bits(with_m.margin_step, i[0]) and same_bits(with_m.margin_obs, j[0])
        top = fresh.plan_dense(batch, top_k=7, margins=True)
        d, i, j = margins(fresh, batch, best_idx=top.rank_idx)
        assert top.margin_dist.shape == (7, 8) and same_bits(top.margin_dist, d) and same_bits(top.margin_step, i) and same_bits(top.margin_obs, j)
        e = fresh.traj_margins(batch, end_state=np.array([MR.end_state_of(batch, b, 62) for b in range(8)]), pose_stride=1)
        assert e[0].shape == (8,) and same_bits(e[0], margins(fresh, batch, best_idx=np.full((1, 8), 62), pose_stride=1)[0][0])


def test_margins_on_the_boundary_masked_result(engine):
    import boundary_ref as BR

    batch = BR.widened(BR.with_corridor(synth.make_batch(5, 5, 5, 5, 10, 100, True, 4004)))
    out = engine.plan_dense(batch, boundary=True, top_k=7, margins=True)
    d, i, j = margins(engine, batch, best_idx=out.rank_idx)
    assert same_bits(out.margin_dist, d) and same_bits(out.margin_step, i) and same_bits(out.margin_obs, j)
    assert np.array_equal(out.rank_idx[0], out.best_idx)


def test_refusals(engine):
    batch = synth.make_batch(4, 5, 5, 5, 10, 100, True, 101)
    p, fb = host_structs(batch)
    B = batch.B
    idx = np.zeros((65, B), dtype=np.int32)
    es = np.tile([0.0, 5.0, 8.0], (65, B, 1))
    d, i, j = np.empty((65, B)), np.empty((65, B), dtype=np.int32), np.empty((65, B), dtype=np.int32)
    n0 = engine.get_option("margin_launches")

    def call(K=2, best_idx=idx, end_state=None, stride=2, dd=d, ii=i, jj=j, params=p, mem=_abi.FP_MEM_HOST, batch_struct=fb):
        rc = engine._lib.fp_traj_margins(engine._ctx, C.byref(params), C.byref(batch_struct), K, None if best_idx is None else best_idx.ctypes.data,
                                         None if end_state is None else end_state.ctypes.data, stride, None if dd is None else dd.ctypes.data,
                                         None if ii is None else ii.ctypes.data, None if jj is None else jj.ctypes.data, mem, None)
        return rc, engine._lib.fp_last_error().decode()

    for K in (0, -1, 65):
        rc, msg = call(K=K)
        assert rc == -1 and "K=" in msg, (K, msg)
    for stride in (0, -2):
        rc, msg = call(stride=stride)
        assert rc == -1 and "pose_stride" in msg
    for kw in (dict(best_idx=None), dict(end_state=es)):
        rc, msg = call(**kw)
        assert rc == -1 and "best_idx" in msg and "end_state" in msg
    for kw in (dict(dd=None), dict(ii=None), dict(jj=None)):
        rc, msg = call(**kw)
        assert rc == -1 and "min_dist" in msg
    big = _abi.FpParams.from_buffer_copy(p)
    big.nd, big.nv, big.nt = 5, 29, 113  # FP_MAX_CAND + 1, as fp_winner_trajs answers
    rc, msg = call(params=big)
    assert rc == -4 and "FP_MAX_CAND" in msg
    bad = idx.copy()
    bad[1, 2] = batch.C
    rc, msg = call(best_idx=bad)
    assert rc == -1 and "ego 2" in msg and "plane 1" in msg
    skip = np.array([0, 0, 1, 0], dtype=np.int32)
    fbs = _abi.FpBatch.from_buffer_copy(fb)
    fbs.skip = skip.ctypes.data
    rc, msg = call(best_idx=bad, batch_struct=fbs)  # ... unless the ego is skipped
    assert rc == 0, msg
    long_T = es.copy()
    long_T[0, 1, 2] = 0.1 * (_abi.FP_MAX_POINTS + 1)
    rc, msg = call(best_idx=None, end_state=long_T)
    assert rc == -4 and "FP_MAX_POINTS" in msg and "ego 1" in msg
    assert engine.get_option("margin_launches") == n0 + 1
    with pytest.raises(ValueError, match="exactly one"):
        engine.traj_margins(batch)
    with pytest.raises(ValueError, match="best_idx must be"):
        engine.traj_margins(batch, best_idx=np.zeros(3))


def test_planner_classes_report_the_margin_of_what_they_return(engine, oracle):
    """report_margins on the demo-scenario fixture inputs (g4_plan.npz): best_margin is the reference's margin of the trajectory
    plan() returned - a lattice candidate for FOP / FOP+ / FISS, the refined off-lattice winner for FISS+."""
    from conftest import batch_from_golden, load_golden
    from fiss_plus_planner_amd import planners as P
    from test_gpu_planners import _g4_keys, _inputs, _planner

    g = load_golden("g4_plan.npz")
    assert P.FrenetOptimalPlannerSettings().report_margins is False
    refined = 0
    for kind in ("FOP", "FOP+", "FISS", "FISS+"):
        key = [k for k in _g4_keys() if k.endswith("_" + kind)][0]
        b = batch_from_golden(g, f"{key}_in_")
        e = int(np.nonzero(g[f"{key}_found"])[0][0])
        pts, fs, obs = _inputs(b, e)
        pl = _planner(kind, b, engine)
        pl.generate_frenet_frame(pts)
        n0 = engine.get_option("margin_launches")
        pl.plan(fs, float(b.target_speed[e]), obs, int(b.t_now[e]))
        assert not hasattr(pl, "best_margin") and engine.get_option("margin_launches") == n0
        pl = _planner(kind, b, engine)
        pl.generate_frenet_frame(pts)
        pl.settings.report_margins = True
        if kind == "FOP":
            pl.settings.num_alternatives = 3
        best = pl.plan(fs, float(b.target_speed[e]), obs, int(b.t_now[e]))
        assert best is not None
        one = pl._make_batch(fs, obs, int(b.t_now[e]))  # the one-ego batch the planner planned on
        idx = best.__dict__.get("lattice_index")
        if idx is not None:
            ref = MR.margins(oracle, one, best_idx=[[idx]])
        else:
            es = best.end_state
            ref = MR.margins(oracle, one, end_state=[[[es.d, es.s_d, es.t]]])
            refined += int((np.asarray(best.idx) < 0).all())
        dist, step, col = pl.best_margin
        print(f"{kind}: best_margin {pl.best_margin}, reference {ref.min_dist[0, 0]}, {ref.min_step[0, 0]}, {ref.min_obs[0, 0]}, gap {ref.gap[0, 0]}")
        assert dist == ref.min_dist[0, 0] or abs(dist - ref.min_dist[0, 0]) <= MR.DIST_TOL, (kind, dist, ref.min_dist)
        if MR.counted(ref)[0, 0]:
            assert (step, col) == (int(ref.min_step[0, 0]), int(ref.min_obs[0, 0])), kind
        if kind == "FOP":
            assert len(pl.alternative_margins) == len(pl.alternatives) and pl.alternative_margins[0] == pl.best_margin
        else:
            assert not hasattr(pl, "alternative_margins")
