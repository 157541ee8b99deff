"""GPU: fp_obstacles_predict (the obstacle pose table built on the device from tracks) against its numpy restatement
(tests/predict_ref.py) through both memory spaces: `valid` and the zeros of invalid elements exact, x / y within 1e-9 m and yaw within
1e-9 rad, host and device bit-identical, rows outside the range untouched; stops, line ends, frames, the ARC branch point, the synthetic
scenes, the dense pass on a predicted table against the oracle, graph capture, the planner class and the error codes."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import predict_cases as PC
import predict_ref as R
from fiss_plus_planner_amd import _abi, synth
from fiss_plus_planner_amd.engine import FrenetEngine
from fiss_plus_planner_amd.obstacles import ObstacleTable, ObstacleTracks

pytestmark = pytest.mark.gpu
POS_TOL = 1e-9   # m:   coordinates of at most 1e3 m and a few tens of FP64 operations per element keep rounding below ~1e-11
YAW_TOL = 1e-9   # rad
NAN_FILL = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]  # a NaN with a payload: an untouched element keeps these bits


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def run_host(engine, case, fill=NAN_FILL):
    out = np.full((case["model"].shape[0], case["T_obs"], case["model"].shape[1], 4), fill)
    pose, fts = engine.predict_obstacles(PC.shape_of(case), case["model"], case["state"], case["frame_of_scene"], case["t0"], case["n_rows"], out=out)
    assert pose is out
    return pose, fts


class OnDevice:
    """A case's arrays in device memory and the fp_batch / fp_tracks over them."""

    def __init__(self, case, fill=NAN_FILL):
        import torch

        self.torch, self.dev = torch, torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        S, n = case["model"].shape
        self.t = dict(model=up(case["model"]), state=up(case["state"]), t0=up(case["t0"]), nx=up(case["nx"]), knots=up(case["knots"]), coef=up(case["coef"]))
        if case["frame_of_scene"] is not None:
            self.t["frame"] = up(case["frame_of_scene"])
        self.pose = up(np.full((S, case["T_obs"], n, 4), fill))
        self.fts = torch.full((S,), -7, dtype=torch.int32, device=self.dev)
        self.params = _abi.FpParams()
        self.params.tick_t = case["tick_t"]
        self.fb = _abi.FpBatch()
        self.fb.S, self.fb.T_obs, self.fb.n_obs, self.fb.F, self.fb.NX = S, case["T_obs"], n, case["knots"].shape[0], case["knots"].shape[1]
        self.fb.nx, self.fb.knots, self.fb.coef = self.t["nx"].data_ptr(), self.t["knots"].data_ptr(), self.t["coef"].data_ptr()
        self.tr = _abi.FpTracks(self.t["model"].data_ptr(), self.t["state"].data_ptr(), self.t["frame"].data_ptr() if "frame" in self.t else None,
                                self.t["t0"].data_ptr(), case["n_rows"])

    def run(self, engine, stream=0):
        engine.predict_obstacles_device(self.params, self.fb, self.tr, self.pose.data_ptr(), self.fts.data_ptr(), stream)

    def fetch(self):
        self.torch.cuda.synchronize(self.dev)
        return self.pose.cpu().numpy(), self.fts.cpu().numpy()


def run_device(engine, case):
    d = OnDevice(case)
    d.run(engine)
    return d.fetch()


MAXIMA = {}


def check(case, pose, fts, what):
    ref = case["ref"]
    R.check_caps(ref.undecided, what)
    assert np.array_equal(fts, ref.fts), (what, fts, ref.fts)
    w = ref.written
    keep = np.array([NAN_FILL]).view(np.uint64)[0]
    assert np.all(pose[~w].view(np.uint64) == keep), (what, "a row outside the range was written")  # every row outside the range keeps its bits
    got, want = pose[w], ref.pose[w]
    assert np.array_equal(got[..., 3], want[..., 3]), (what, "valid", np.argwhere(got[..., 3] != want[..., 3])[:4].tolist())
    inv = want[..., 3] == 0
    assert not got[inv].view(np.uint64).any(), (what, "an invalid element is not +0, +0, +0, +0")
    err_xy = float(np.abs(got[..., :2] - want[..., :2]).max(initial=0.0))
    err_yaw = float(np.abs(got[..., 2] - want[..., 2]).max(initial=0.0))
    m = MAXIMA.setdefault(what.split("(")[0].split("[")[0], [0.0, 0.0])
    m[0], m[1] = max(m[0], err_xy), max(m[1], err_yaw)
    print(f"{what}: max |dx, dy| = {err_xy:.3e} m, max |dyaw| = {err_yaw:.3e} rad")
    assert err_xy <= POS_TOL and err_yaw <= YAW_TOL, (what, err_xy, err_yaw)


def both_spaces(engine, case, what):
    hp, hf = run_host(engine, case)
    dp, df = run_device(engine, case)
    check(case, hp, hf, what + " host")
    check(case, dp, df, what + " device")
    assert same_bits(hp, dp) and np.array_equal(hf, df), (what, "host and device differ")
    return hp


@pytest.mark.parametrize("key", PC.SWEEP, ids=[f"n{n}-T{T}-nx{nx}" for n, T, nx in PC.SWEEP])
def test_main_sweep(engine, key):
    both_spaces(engine, PC.sweep(*key), f"sweep{key}")


@pytest.mark.parametrize("k", range(5), ids=["t0=0", "t0=3", "t0=-2", "t0=T-1", "t0=T+4"])
def test_row_range(engine, k):
    case = PC.row_range(k)
    both_spaces(engine, case, f"row_range[{k}]")
    t0 = (0, 3, -2, 22, 27)[k]
    assert case["ref"].fts[1] == min(23, t0 + case["n_rows"]) and case["ref"].written[1].sum() == max(0, 23 - max(t0, 0))


def test_stops(engine):
    pose = both_spaces(engine, PC.stops(), "stops")[0]
    for j in (0, 4):   # the stop at 0.25 s lies between rows 2 and 3
        assert all(same_bits(pose[r, j], pose[3, j]) for r in range(3, 12)) and not same_bits(pose[2, j], pose[3, j])
    for j in (1, 5):   # the stop at 0.2 s is row 2
        assert all(same_bits(pose[r, j], pose[2, j]) for r in range(2, 12)) and not same_bits(pose[1, j], pose[2, j])
    assert same_bits(pose[:, 2], pose[:, 3]) and same_bits(pose[:, 6], pose[:, 7])  # v < 0 behaves as v = 0
    assert all(same_bits(pose[r, 8:10], pose[0, 8:10]) for r in range(12))           # v < 0 and braking: never moves, never reverses


def test_line_ends(engine):
    pose = both_spaces(engine, PC.line_ends(), "line_ends")[0]
    v = pose[..., 3]
    assert v[0, 0] == 1 and v[-1, 0] == 0 and v[0, 1] == 0 and v[-1, 1] == 1 and not v[:, 2].any() and v[:, 3].all()


def test_frames(engine):
    """Two scenes on one frame; on the device path a NULL frame pointer and an out-of-range frame index make LANE columns invalid and leave
    the ARC columns of the same scene alone; on the host path the same inputs are FP_EINVAL naming the scene and the column."""
    shared = PC.frames_shared()
    pose = both_spaces(engine, shared, "frames_shared")
    assert pose[..., 3][np.broadcast_to((shared["model"] == R.LANE)[:, None, :], pose[..., 3].shape)].any()
    for name, fos in (("frames_out_of_range", (0, 7, -1)), ("frames_null", None)):
        case = PC.frames_shared(fos)
        dp, df = run_device(engine, case)
        check(case, dp, df, name + " device")
        lane = np.broadcast_to((case["model"] == R.LANE)[:, None, :], dp[..., 3].shape)
        arc = np.broadcast_to((case["model"] == R.ARC)[:, None, :], dp[..., 3].shape)
        bad_scene = np.array([fos is None, True, True])
        assert not dp[..., 3][lane & bad_scene[:, None, None]].any() and dp[..., 3][arc].all()
        assert same_bits(dp[..., 3][arc], pose[..., 3][arc]) and same_bits(dp[arc], pose[arc])  # ARC columns are unaffected
        with pytest.raises(_abi.FrenetGpuError) as ei:
            run_host(engine, case)
        s_bad = 0 if fos is None else 1
        j_bad = int(np.nonzero(case["model"][s_bad] == R.LANE)[0][0])
        assert ei.value.code == -1 and f"scene {s_bad}, column {j_bad}" in str(ei.value), str(ei.value)


def test_arc_branch(engine):
    both_spaces(engine, PC.arc_branch(), "arc_branch")


def test_two_runs_and_another_slab_cut_give_the_same_bits(engine):
    """An element is a function of its (scene, row, column): the same scenes predicted alone (one workgroup per row) and inside a
    300-scene table (slabs of 8 rows, the last one of 2) have the same bits."""
    case = PC.sweep(67, 50, 81)
    a, _ = run_device(engine, case)
    b, _ = run_device(engine, case)
    assert same_bits(a, b)
    reps = 100
    big = dict(case, model=np.tile(case["model"], (reps, 1)), state=np.tile(case["state"], (reps, 1, 1)), frame_of_scene=np.tile(case["frame_of_scene"], reps),
               t0=np.tile(case["t0"], reps))
    d = OnDevice(big)
    d.run(engine)
    got, fts = d.fetch()
    assert same_bits(got[:3], a) and same_bits(got[-3:], a) and same_bits(got[150:153], a) and np.array_equal(fts, np.tile(case["ref"].fts, reps))


@pytest.mark.parametrize("cfg", [3, 2])
def test_synthetic_scenes(engine, cfg):
    """predict(make_tracks(...)) against make_batch(...).obs_pose: B = 4 on config 3 sizes, B = 2 on config 2 sizes (static, T_obs = 100)."""
    args = {3: (4, 9, 9, 7, 50, 50, True, synth.CONFIG_SEEDS[3]), 2: (2, 5, 5, 5, 10, 100, False, synth.CONFIG_SEEDS[2])}[cfg]
    batch, tr = synth.make_batch(*args, layout="survey8d"), synth.make_tracks(*args, layout="survey8d")
    pose, fts = engine.predict_obstacles(batch, tr.model, tr.state, tr.frame_of_scene, 0, batch.T_obs)
    with_tr = dataclasses.replace(batch, obs_pose=np.full(batch.obs_pose.shape, NAN_FILL), track_model=tr.model, track_state=tr.state, track_frame=tr.frame_of_scene)
    import torch

    from fiss_plus_planner_amd.device_batch import DeviceBatch

    db = DeviceBatch(with_tr, 0)
    db.predict(engine, torch.zeros(batch.S, dtype=torch.int32, device=db.dev), batch.T_obs)
    torch.cuda.synchronize()
    assert same_bits(db.t["obs_pose"].cpu().numpy(), pose) and np.array_equal(db.t["final_time_step"].cpu().numpy(), fts) and np.all(fts == batch.T_obs)
    assert np.array_equal(pose[..., 3], batch.obs_pose[..., 3])
    err_xy, err_yaw = np.abs(pose[..., :2] - batch.obs_pose[..., :2]).max(), np.abs(pose[..., 2] - batch.obs_pose[..., 2]).max()
    print(f"config {cfg}: max |dx, dy| = {err_xy:.3e} m, max |dyaw| = {err_yaw:.3e} rad against make_batch")
    assert err_xy <= POS_TOL and err_yaw <= YAW_TOL


def _mixed_batch():
    """8 egos, 5 x 5 x 5, 10 obstacles, T_obs = 100: make_batch's scenes with every second column turned into the ARC track that starts at
    the same pose (heading along the lane, a mild curvature, braking or accelerating) and one column per scene without a pose."""
    args = (8, 5, 5, 5, 10, 100, True, 20261)
    batch, tr = synth.make_batch(*args), synth.make_tracks(*args)
    rng = np.random.default_rng(7)
    model, state = tr.model.copy(), tr.state.copy()
    state[..., 3] = rng.uniform(-1.0, 0.5, model.shape)  # LANE: a
    for s in range(batch.S):
        for j in range(1, 10, 2):
            x, y, yaw, _ = batch.obs_pose[s, 0, j]
            model[s, j] = R.ARC
            state[s, j] = (x, y, yaw, tr.state[s, j, 2], rng.uniform(-1.5, 1.0), rng.uniform(-0.02, 0.02))
        model[s, 8] = R.NONE
    return dataclasses.replace(batch, obs_pose=np.full(batch.obs_pose.shape, NAN_FILL), track_model=model, track_state=state, track_frame=tr.frame_of_scene)


def test_end_to_end_dense_on_a_predicted_table(engine, oracle):
    """DeviceBatch.predict in place, then plan_dense with tables on the resident batch; the oracle runs on the READ-BACK table, so both
    sides see identical poses: flag words, best_idx and Stats exact, cost within 1e-9."""
    import torch

    from fiss_plus_planner_amd.device_batch import DeviceBatch

    batch = _mixed_batch()
    db = DeviceBatch(batch, 0)
    B, Cn = batch.B, batch.C
    stream = torch.cuda.current_stream(db.dev).cuda_stream
    db.predict(engine, torch.zeros(batch.S, dtype=torch.int32, device=db.dev), batch.T_obs, stream=stream)
    bi, bc, st = db.empty(B, torch.int32), db.empty(B, torch.float64), db.empty((B, 4), torch.int32)
    cost, flags = db.empty((B, Cn), torch.float64), db.empty((B, Cn), torch.int32)
    engine.plan_dense_device(db.params, db.fb, bi.data_ptr(), bc.data_ptr(), st.data_ptr(), cost_tbl=cost.data_ptr(), flag_tbl=flags.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    table, fts = db.t["obs_pose"].cpu().numpy(), db.t["final_time_step"].cpu().numpy()
    assert np.isfinite(table).all() and np.all(fts == 100) and set(np.unique(table[..., 3])) == {0.0, 1.0}
    ref_pose = R.predict(batch.track_model, batch.track_state, batch.track_frame, 0, 100, 100, batch.tick_t, batch.nx, batch.knots, batch.coef)[0]
    assert np.array_equal(table[..., 3], ref_pose[..., 3]) and np.abs(table - ref_pose).max() <= POS_TOL
    seen = dataclasses.replace(batch, obs_pose=table, final_time_step=fts, track_model=None, track_state=None, track_frame=None)
    res = [p.fop_plan() for p in oracle.problems_from_batch(seen)]
    got_flags = flags.cpu().numpy().view(np.uint32)
    ref_flags = np.stack([r.flags for r in res])
    assert np.array_equal(got_flags, ref_flags)
    assert (ref_flags & _abi.FLAG_COLLISION).any() and not (ref_flags & _abi.FLAG_COLLISION).all()  # the predicted obstacles matter
    ref_bi = np.array([r.best_idx for r in res])
    assert np.array_equal(bi.cpu().numpy(), ref_bi) and np.array_equal(st.cpu().numpy(), np.stack([r.stats for r in res]))
    assert np.abs(cost.cpu().numpy() - np.stack([r.cost for r in res])).max() <= 1e-9
    got_bc = bc.cpu().numpy()
    assert np.abs(got_bc[ref_bi >= 0] - np.array([r.best_cost for r in res])[ref_bi >= 0]).max(initial=0.0) <= 1e-9 and np.isnan(got_bc[ref_bi < 0]).all()
    # the host path on the same batch: the same table, the same plan
    host_out = engine.plan_dense(seen, tables=True)
    assert np.array_equal(host_out.flags, got_flags) and np.array_equal(host_out.best_idx, ref_bi)


def test_graph_capture_replays_against_new_tracks(engine):
    """One captured predict_obstacles_device call: a replay after state and t0 were overwritten on the device gives the table of the new
    tracks.  predict_launches counts calls, as the library's other launch counters do: the eager call and the capture, not the replays."""
    import torch

    first, second = PC.sweep(67, 50, 81), PC.sweep(67, 50, 220)
    new = PC.finish(first["model"], second["state"], first["frame_of_scene"], [3, 0, -2], first["n_rows"], first["T_obs"], first["nx"], first["knots"], first["coef"])
    R.check_caps(new["ref"].undecided, "graph, second tracks")
    d = OnDevice(first)
    n0 = engine.get_option("predict_launches")
    d.run(engine, torch.cuda.current_stream(d.dev).cuda_stream)  # eager (also the warm-up of the capture)
    check(first, *d.fetch(), "graph eager")
    free = torch.cuda.mem_get_info()[0]
    d.run(engine, torch.cuda.current_stream(d.dev).cuda_stream)
    torch.cuda.synchronize(d.dev)
    assert torch.cuda.mem_get_info()[0] == free  # enqueue only: a second call allocates nothing
    side = torch.cuda.Stream(d.dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        d.run(engine, side.cuda_stream)
    torch.cuda.synchronize(d.dev)
    assert engine.get_option("predict_launches") == n0 + 3
    d.pose.copy_(torch.from_numpy(np.full(d.pose.shape, NAN_FILL)))
    graph.replay()
    check(first, *d.fetch(), "graph replay, first tracks")
    d.t["state"].copy_(torch.from_numpy(new["state"]))
    d.t["t0"].copy_(torch.from_numpy(new["t0"]))
    d.pose.copy_(torch.from_numpy(np.full(d.pose.shape, NAN_FILL)))
    graph.replay()
    got = d.fetch()
    check(new, *got, "graph replay, second tracks")
    assert not same_bits(got[0], first["ref"].pose)
    assert engine.get_option("predict_launches") == n0 + 3  # (a replay is not a call)


def test_prediction_is_opt_in(engine):
    """A caller that never calls the entry point launches no prediction kernel."""
    n0 = engine.get_option("predict_launches")
    engine.plan_dense(synth.make_batch(8, 5, 5, 5, 10, 100, True, 101), tables=True, winner=True)
    engine.plan_fiss(synth.make_batch(8, 5, 5, 5, 10, 100, True, 101, kind="FISS+"), "FISS+")
    assert engine.get_option("predict_launches") == n0
    with FrenetEngine(0) as other:
        other.plan_dense(synth.make_batch(2, 5, 5, 5, 10, 100, True, 101))
        assert other.get_option("predict_launches") == 0 and other.get_option("lattice_launches") == 1


def _planner_and_inputs(engine, kind="FOP"):
    from fiss_plus_planner_amd import planners as P
    from fiss_plus_planner_amd.frenet import FrenetState
    from fiss_plus_planner_amd.vehicle import Vehicle

    batch = _mixed_batch()
    cls, st = {"FOP": (P.FrenetOptimalPlanner, P.FrenetOptimalPlannerSettings), "FOP+": (P.FopPlusPlanner, P.FrenetOptimalPlannerSettings),
               "FISS": (P.FissPlanner, P.FissPlannerSettings), "FISS+": (P.FissPlusPlanner, P.FissPlusPlannerSettings)}[kind]
    pl = cls(st(5, 5, 5), Vehicle(), None, engine=engine)
    nx = int(batch.nx[0])
    pl.generate_frenet_frame(np.column_stack([batch.coef[0, 0, :nx], batch.coef[0, 4, :nx]]))
    s, s_d, s_dd, d, d_d, d_dd = batch.ego[0]
    fs = FrenetState(t=0.0, s=s, s_d=s_d, s_dd=s_dd, d=d, d_d=d_d, d_dd=d_dd)
    tracks = ObstacleTracks(batch.track_model[0], batch.track_state[0], batch.obs_dims[0])
    return pl, fs, tracks


def _traj_bits(t):
    return [np.asarray(getattr(t, k)) for k in ("t", "s", "d", "x", "y", "yaw")] + [np.array([t.cost_final if hasattr(t, "cost_final") else 0.0])]


def test_planner_class_takes_tracks(engine):
    """FrenetOptimalPlanner.plan(..., obstacles=ObstacleTracks) equals plan on the ObstacleTable from tracks.table(...) bit for bit; a
    second call at the same time_step_now launches no predict kernel; after tracks.update(...) it launches one."""
    pl, fs, tracks = _planner_and_inputs(engine)
    t_now, n_rows = 4, int(np.ceil(pl.settings.max_t / pl.settings.tick_t))
    n0 = engine.get_option("predict_launches")
    best = pl.plan(fs, 13.0, tracks, t_now)
    assert engine.get_option("predict_launches") == n0 + 1 and best is not None
    tables = [a.copy() for a in pl.last_tables]
    assert (tables[1] & _abi.FLAG_COLLISION).any()
    again = pl.plan(fs, 13.0, tracks, t_now)
    assert engine.get_option("predict_launches") == n0 + 1
    sp = pl.cubic_spline
    tab = tracks.table(engine, sp.knots, sp.coef, pl.settings.tick_t, t_now + n_rows, t0=t_now, n_rows=n_rows)
    assert isinstance(tab, ObstacleTable) and tab.final_time_step == t_now + n_rows and not tab.pose[:t_now].any() and tab.pose[t_now:, :, 3].any()
    n1 = engine.get_option("predict_launches")
    pl2, _, _ = _planner_and_inputs(engine)
    want = pl2.plan(fs, 13.0, tab, t_now)
    assert engine.get_option("predict_launches") == n1  # a table launches no prediction
    for got in (best, again):
        assert got.lattice_index == want.lattice_index
        for a, b in zip(_traj_bits(got), _traj_bits(want)):
            assert same_bits(a, b)
    assert same_bits(tables[0], pl2.last_tables[0]) and np.array_equal(tables[1], pl2.last_tables[1])
    with pytest.raises(ValueError):
        tracks.state[0, 0] = 0.0  # frozen while the planner holds the prediction
    moved = tracks.state.copy()
    moved[:, 0] += np.where(tracks.model == R.LANE, 3.0, 0.0)
    tracks.update(state=moved)
    pl.plan(fs, 13.0, tracks, t_now)
    assert engine.get_option("predict_launches") == n1 + 1
    pl.plan(fs, 13.0, tracks, t_now + 1)  # another time step: the states are valid there, another prediction
    assert engine.get_option("predict_launches") == n1 + 2


@pytest.mark.parametrize("kind", ["FOP+", "FISS", "FISS+"])
def test_other_planner_classes_take_tracks(engine, kind):
    pl, fs, tracks = _planner_and_inputs(engine, kind)
    n0 = engine.get_option("predict_launches")
    got = pl.plan(fs, 13.0, tracks, 2)
    assert engine.get_option("predict_launches") == n0 + 1
    sp = pl.cubic_spline
    tab = tracks.table(engine, sp.knots, sp.coef, pl.settings.tick_t, 2 + 100, t0=2, n_rows=100)
    pl2, _, _ = _planner_and_inputs(engine, kind)
    want = pl2.plan(fs, 13.0, tab, 2)
    assert (got is None) == (want is None)
    if got is not None:
        for a, b in zip(_traj_bits(got), _traj_bits(want)):
            assert same_bits(a, b)


def test_errors(engine):
    case = PC.frames_shared()
    shape = PC.shape_of(case)
    lib, ctx = engine._lib, engine._ctx
    S, n = case["model"].shape
    out, fts = np.zeros((S, case["T_obs"], n, 4)), np.zeros(S, dtype=np.int32)
    p = _abi.FpParams()
    p.tick_t = 0.1
    fb = _abi.FpBatch()
    fb.S, fb.T_obs, fb.n_obs, fb.F, fb.NX = S, case["T_obs"], n, 2, 81
    nx, knots, coef = (np.ascontiguousarray(case[k]) for k in ("nx", "knots", "coef"))
    fb.nx, fb.knots, fb.coef = nx.ctypes.data, knots.ctypes.data, coef.ctypes.data
    ptr = lambda a: a.ctypes.data

    def call(tr, params=p, pose=out, mem=_abi.FP_MEM_HOST):
        return lib.fp_obstacles_predict(ctx, C.byref(params), C.byref(fb), None if tr is None else C.byref(tr), None if pose is None else ptr(pose), ptr(fts), mem, None)

    good = lambda: _abi.FpTracks(ptr(case["model"]), ptr(case["state"]), ptr(case["frame_of_scene"]), ptr(case["t0"]), 5)
    assert call(good()) == 0
    for mem in (_abi.FP_MEM_HOST, _abi.FP_MEM_DEVICE):  # (the argument checks come before anything touches the pointers)
        assert call(None, mem=mem) == -1
        for field in ("model", "state", "t0"):
            tr = good()
            setattr(tr, field, None)
            assert call(tr, mem=mem) == -1 and b"must not be NULL" in lib.fp_last_error(), field
        assert call(good(), pose=None, mem=mem) == -1
        for n_rows in (0, -3):
            tr = good()
            tr.n_rows = n_rows
            assert call(tr, mem=mem) == -1 and b"n_rows" in lib.fp_last_error()
        for tick in (0.0, -0.1, float("nan"), float("inf")):
            bad = _abi.FpParams()
            bad.tick_t = tick
            assert call(good(), params=bad, mem=mem) == -1 and b"tick_t" in lib.fp_last_error(), tick
    assert lib.fp_obstacles_predict(ctx, C.byref(p), C.byref(fb), C.byref(good()), ptr(out), ptr(fts), 7, None) == -1
    for bad_model in (3, -1):
        m = case["model"].copy()
        m[2, 4] = bad_model
        with pytest.raises(_abi.FrenetGpuError) as ei:
            engine.predict_obstacles(shape, m, case["state"], case["frame_of_scene"], 0, 5)
        assert ei.value.code == -1 and "scene 2, column 4" in str(ei.value)
        d = OnDevice(dict(case, model=m))  # the device path: such a column has no pose
        d.run(engine)
        got, _ = d.fetch()
        assert not got[2, :, 4].view(np.uint64).any()
    with pytest.raises(ValueError):
        engine.predict_obstacles(shape, case["model"][:, :3], case["state"], case["frame_of_scene"], 0, 5)
    with pytest.raises(ValueError):
        engine.predict_obstacles(shape, case["model"], case["state"], case["frame_of_scene"], 0, 5, out=np.zeros((S, case["T_obs"], n, 4), dtype=np.float32))
    with pytest.raises(_abi.FrenetGpuError):
        engine.predict_obstacles(shape, case["model"], case["state"], case["frame_of_scene"], 0, 0)
    import torch

    from fiss_plus_planner_amd.device_batch import DeviceBatch

    db = DeviceBatch(synth.make_batch(2, 5, 5, 5, 4, 20, True, 3), 0)
    with pytest.raises(ValueError):
        db.predict(engine, torch.zeros(2, dtype=torch.int32, device=db.dev), 20)  # the batch carries no tracks
    d = OnDevice(case)
    with pytest.raises(_abi.FrenetGpuError):  # a table that is not 16-byte aligned
        engine.predict_obstacles_device(d.params, d.fb, d.tr, d.pose.data_ptr() + 8, 0)


def test_report_observed_maxima():
    """(runs last: the observed parity maxima of this session, for EXPERIMENTS.md)"""
    for k, (xy, yaw) in sorted(MAXIMA.items()):
        print(f"observed maximum {k}: {xy:.3e} m, {yaw:.3e} rad")
