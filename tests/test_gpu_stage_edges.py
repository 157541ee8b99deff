"""GPU: the FP_MEM_HOST path (every array placed by plan_stage, csrc/frenet_stage_plan.h) against the FP_MEM_DEVICE path on the same
inputs, at the edges of the staging regimes: every output bit-equal.

B = 8 / 9 is the latency switch (zero-copy outputs up to 8 egos).  16 x 8 x 8 candidates make the cost table of 8 egos exactly 64 KiB
(the largest array of the small window), 17 x 8 x 8 is the next lattice above it.  The obstacle tables take the inputs of an
8-ego call to 249.5 KiB in all (everything below the 256 KiB the kernels may read from the pinned block), to a 250 KiB table (still one
array of the window, but 300 KiB in all) and to a 257.5 KiB table (its own copy in every regime).  17 egos make the in/out flag table
of the boundary mask larger than the window takes.

The second half pins the same equality for every other entry point that serves both memory spaces, on one tiny batch (3 egos, 3 x 3 x 3
candidates, 4 obstacles over 20 steps, all four rules, K = 2 explicit plans): one ego is skipped, one has no plan.  Every entry point is
called twice with the same arguments, once on numpy arrays (FP_MEM_HOST) and once on their uploaded copies (FP_MEM_DEVICE), and every
array comes back with the same bits."""
import ctypes as C
import functools

import numpy as np
import pytest

import boundary_ref as R
import fallback_rules_cases as FRC
import rule_pass as RP
from fiss_plus_planner_amd import _abi, synth
from fiss_plus_planner_amd import rules as rules_mod

pytestmark = pytest.mark.gpu

SMALL, SMALL_OBS = (16, 8, 8), (4, 20)
CASES = [(B, lat, SMALL_OBS) for B in (8, 9) for lat in (SMALL, (17, 8, 8))] + \
        [(B, SMALL, obs) for B in (8, 9) for obs in ((8, 100), (10, 100), (10, 103))]
IDS = [f"B{B}-{'x'.join(map(str, lat))}-obs{n}x{T}" for B, lat, (n, T) in CASES]
K = 7


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@functools.lru_cache(maxsize=None)
def make(B, lat, obs):
    return R.with_corridor(synth.make_batch(B, *lat, obs[0], obs[1], True, 7300 + B))


_RESIDENT = {}


def resident(eng, B, lat, obs):
    """The batch, and what the device path gives for it (computed once): the dense pass with tables, the ranking and the boundary mask
    over them."""
    if (B, lat, obs) in _RESIDENT:
        return _RESIDENT[(B, lat, obs)]
    import torch

    from fiss_plus_planner_amd.device_batch import DeviceBatch

    batch = make(B, lat, obs)
    Cn = batch.C
    db = DeviceBatch(batch, 0, order_hint=False)
    i32, f64 = torch.int32, torch.float64
    t = dict(best_idx=db.empty(B, i32), best_cost=db.empty(B, f64), stats=db.empty((B, 4), i32), cost=db.empty((B, Cn), f64), flags=db.empty((B, Cn), i32),
             rank_idx=db.empty((K, B), i32), rank_cost=db.empty((K, B), f64), n_feasible=db.empty(B, i32),
             mask_idx=db.empty(B, i32), mask_cost=db.empty(B, f64), n_masked=db.empty(B, i32))
    p = {k: v.data_ptr() for k, v in t.items()}
    eng.plan_dense_device(db.params, db.fb, p["best_idx"], p["best_cost"], p["stats"], p["cost"], p["flags"])
    eng.rank_feasible_device(db.params, db.fb, p["cost"], p["flags"], K, p["rank_idx"], p["rank_cost"], p["n_feasible"])
    torch.cuda.synchronize(db.dev)
    dev = {k: v.cpu().numpy() for k, v in t.items()}
    eng.boundary_mask_device(db.params, db.fb, db.t["bound_left"].data_ptr(), db.t["bound_right"].data_ptr(), float(batch.bound_margin), p["cost"], p["flags"],
                             p["mask_idx"], p["mask_cost"], p["n_masked"])
    torch.cuda.synchronize(db.dev)
    dev.update({k: t[k].cpu().numpy() for k in ("mask_idx", "mask_cost", "n_masked")}, mask_flags=t["flags"].cpu().numpy())
    for v in dev.values():
        v.setflags(write=False)
    _RESIDENT[(B, lat, obs)] = batch, dev
    return batch, dev


def input_bytes(batch):
    """Bytes of a host dense call's inputs as the staging list places them (each array on the next multiple of 256)."""
    arrays = [batch.d_samples, batch.t_samples, batch.v_samples, batch.target_speed, batch.ego, batch.frame_of, batch.scene_of, batch.t_now, batch.nx,
              batch.knots, batch.coef, batch.obs_pose, batch.obs_dims, batch.final_time_step]
    end = 0
    for a in arrays:
        end = -(-end // 256) * 256 + a.nbytes
    return end


def test_the_cases_sit_where_the_docstring_says():
    b8 = {obs: make(8, SMALL, obs) for obs in ((8, 100), (10, 100), (10, 103))}
    assert make(8, SMALL, SMALL_OBS).C * 8 * 8 == 64 << 10 and make(8, (17, 8, 8), SMALL_OBS).C * 8 * 8 > 64 << 10
    assert input_bytes(b8[(8, 100)]) <= 256 << 10 < input_bytes(b8[(10, 100)])
    assert b8[(10, 100)].obs_pose.nbytes <= 256 << 10 < b8[(10, 103)].obs_pose.nbytes
    assert make(17, SMALL, SMALL_OBS).C * 17 * 4 > 64 << 10


@pytest.mark.parametrize("B,lat,obs", CASES, ids=IDS)
def test_dense_tables_rank_and_mask_host_equals_device(engine, B, lat, obs):
    batch, dev = resident(engine, B, lat, obs)
    tag = 9400 + CASES.index((B, lat, obs))
    try:
        for zero_copy_in in (0, 1, 2):
            engine.set_option("zero_copy_in", zero_copy_in)
            for tagged in (0, tag, tag):  # (the tagged call twice: the upload of the tables, then the call that finds them resident)
                batch.tables_tag = tagged
                what = (zero_copy_in, tagged)
                out = engine.plan_dense(batch, tables=True)
                for k in ("best_idx", "best_cost", "stats", "cost", "flags"):
                    assert same_bits(getattr(out, k), dev[k]), (what, k)
            batch.tables_tag = 0
            rank_idx, rank_cost, n_feasible = engine.rank_feasible(batch, out.cost, out.flags, K)
            assert same_bits(rank_idx, dev["rank_idx"]) and same_bits(rank_cost, dev["rank_cost"]) and same_bits(n_feasible, dev["n_feasible"]), what
            flags, mask_idx, mask_cost, n_masked = engine.boundary_mask(batch, out.cost, out.flags)
            assert same_bits(flags, dev["mask_flags"]) and same_bits(mask_idx, dev["mask_idx"]) and same_bits(mask_cost, dev["mask_cost"]), what
            assert same_bits(n_masked, dev["n_masked"]), what
            assert (flags != out.flags).any()  # (the mask wrote the in/out table)
    finally:
        batch.tables_tag = 0
        engine.set_option("zero_copy_in", 0)


def test_mask_with_a_flag_table_beyond_the_window(engine):
    batch, dev = resident(engine, 17, SMALL, SMALL_OBS)
    out = engine.plan_dense(batch, tables=True)
    assert same_bits(out.cost, dev["cost"]) and same_bits(out.flags, dev["flags"]) and same_bits(out.best_idx, dev["best_idx"])
    flags, mask_idx, mask_cost, n_masked = engine.boundary_mask(batch, out.cost, out.flags)
    assert same_bits(flags, dev["mask_flags"]) and same_bits(mask_idx, dev["mask_idx"]) and same_bits(mask_cost, dev["mask_cost"])
    assert same_bits(n_masked, dev["n_masked"]) and (flags != out.flags).any()


def test_predict_part_of_the_rows_from_mixed_t0(engine):
    """n_rows < T_obs and another t0 per scene: the host path predicts into a compact [S][n_rows] buffer and copies the written rows
    back run by run; every element, written or not, equals the device path's in-place table."""
    import torch

    S, n_obs, T_obs, n_rows = 4, 5, 23, 9
    batch = synth.make_batch(S, 5, 5, 5, n_obs, T_obs, True, 7350)
    tr = synth.make_tracks(S, 5, 5, 5, n_obs, T_obs, True, 7350)
    t0 = np.array([0, 4, -3, 20], dtype=np.int32)  # rows 0..8, 4..12, 0..5, 20..22
    fill = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]  # an untouched element keeps these bits
    pose, fts = engine.predict_obstacles(batch, tr.model, tr.state, tr.frame_of_scene, t0, n_rows, out=np.full((S, T_obs, n_obs, 4), fill))

    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    t = dict(model=up(tr.model), state=up(tr.state), frame=up(tr.frame_of_scene), t0=up(t0), nx=up(batch.nx.astype(np.int32)), knots=up(batch.knots),
             coef=up(batch.coef), pose=up(np.full((S, T_obs, n_obs, 4), fill)), fts=torch.zeros(S, dtype=torch.int32, device=dev))
    p = _abi.FpParams()
    p.tick_t = float(batch.tick_t)
    fb = _abi.FpBatch()
    fb.S, fb.T_obs, fb.n_obs, fb.F, fb.NX = S, T_obs, n_obs, batch.knots.shape[0], batch.knots.shape[1]
    fb.nx, fb.knots, fb.coef = t["nx"].data_ptr(), t["knots"].data_ptr(), t["coef"].data_ptr()
    ftr = _abi.FpTracks(t["model"].data_ptr(), t["state"].data_ptr(), t["frame"].data_ptr(), t["t0"].data_ptr(), n_rows)
    engine.predict_obstacles_device(p, fb, ftr, t["pose"].data_ptr(), t["fts"].data_ptr())
    torch.cuda.synchronize(dev)
    assert same_bits(pose, t["pose"].cpu().numpy()) and np.array_equal(fts, t["fts"].cpu().numpy())
    written = ~(pose.view(np.uint64) == np.array([fill]).view(np.uint64)[0]).all(axis=(2, 3))
    assert [np.nonzero(w)[0].tolist() for w in written] == [list(range(0, 9)), list(range(4, 13)), list(range(0, 6)), list(range(20, 23))]


# ---------------------------------------------------------------- the other entry points, host against device on one tiny batch
TINY_B, TINY_LAT, TINY_K = 3, (3, 3, 3), 2
NO_PLAN, SKIPPED = 1, 2  # ego 1 has no plan (best_idx -1, NaN end state), ego 2 is skipped (fp_batch.skip; done in the loop calls)
STOP_T = np.array([2.0, 3.0, 4.5, 6.0])
_TINY = {}


class Tiny:
    """The tiny batch in both memory spaces, the dense tables the passes read and the plans the other calls take."""

    def __init__(self, eng):
        import torch

        from fiss_plus_planner_amd.device_batch import DeviceBatch
        from fiss_plus_planner_amd.engine import host_structs

        self.eng, self.torch = eng, torch
        self.batch = b = FRC.with_rules(synth.make_batch(TINY_B, *TINY_LAT, *SMALL_OBS, True, 7400))
        self.db = DeviceBatch(b, 0, order_hint=False)  # (a host call has no launch order)
        self.skip = np.zeros(TINY_B, dtype=np.int32)
        self.skip[SKIPPED] = 1
        self.skip_dev = self.up(self.skip)
        self.params, self.fb_host = host_structs(b)
        self.fb_host.skip = self.skip.ctypes.data
        self.fb_dev = _abi.FpBatch.from_buffer_copy(self.db.fb)
        self.fb_dev.skip = self.skip_dev.data_ptr()
        out = eng.plan_dense(b, tables=True)
        self.cost, self.flags = out.cost, out.flags
        self.best_idx = out.best_idx.astype(np.int32)
        self.best_idx[NO_PLAN] = -1
        d, t, v = np.asarray(b.d_samples), np.asarray(b.t_samples), np.asarray(b.v_samples)
        self.end_states = np.empty((TINY_B, TINY_K, 3))  # two lattice samples per ego as explicit (d, v, T)
        for e in range(TINY_B):
            self.end_states[e] = [(d[0], v[e, 1], t[2]), (d[2], v[e, 0], t[1])]
        self.end_states[NO_PLAN] = np.nan
        self.rule_arrays = {name: np.ascontiguousarray(rules_mod.array(b, name)) for r in rules_mod.TABLE for name in r.arrays}

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.db.dev)

    def both(self, fn, arrays, args, device_fill=None, host_null=()):
        """fn(ctx, *args(params, fb, addr, hold), mem, stream) on `arrays` (name -> numpy array, inputs and pre-filled outputs) in both
        memory spaces; addr(name) = the address of that array in the call's space, hold = a list that keeps the call's structs alive.
        device_fill: name -> the byte the device copy of an output starts from (where the host path defines the untouched elements).
        host_null: optional outputs the host call passes NULL for (they are not compared).
        Asserts that every array holds the same bits after the two calls -> the arrays after the host call."""
        got = []
        for mem in (_abi.FP_MEM_HOST, _abi.FP_MEM_DEVICE):
            hold = []
            if mem == _abi.FP_MEM_HOST:
                a = {k: v.copy() for k, v in arrays.items()}
                _abi.check(fn(self.eng._ctx, *args(self.params, self.fb_host, lambda k: None if k in host_null else a[k].ctypes.data, hold), mem, None))
            else:
                t = {k: self.up(v) for k, v in arrays.items()}
                for k, byte in (device_fill or {}).items():
                    t[k].view(self.torch.uint8).fill_(byte)
                _abi.check(fn(self.eng._ctx, *args(self.db.params, self.fb_dev, lambda k: t[k].data_ptr(), hold), mem, None))
                self.torch.cuda.synchronize(self.db.dev)
                a = {k: v.cpu().numpy() for k, v in t.items()}
            got.append(a)
        diff = [k for k in arrays if k not in host_null and not same_bits(got[0][k], got[1][k])]
        assert not diff, {k: (got[0][k], got[1][k]) for k in diff}
        return got[0]

    def rule_set(self, addr, hold, names=None):
        rs, structs = rules_mod.rule_set(self.batch, addr, names)
        hold.append(structs)
        return rs


@pytest.fixture
def tiny(engine):
    if "t" not in _TINY:
        _TINY["t"] = Tiny(engine)
    return _TINY["t"]


def test_tiny_winner_trajs(tiny):
    B = TINY_B
    for sparse in (0, 1):
        arrays = dict(best_idx=tiny.best_idx, best_flags=np.zeros(B, dtype=np.uint32), best_traj=np.full((B, 16, 128), -7.5))
        got = tiny.both(tiny.eng._lib.fp_winner_trajs, arrays,
                        lambda p, fb, addr, hold: (C.byref(p), C.byref(fb), addr("best_idx"), addr("best_flags"), addr("best_traj"), 128, sparse))
        none = got["best_traj"][NO_PLAN]
        assert np.isnan(none[none != -7.5]).all() and np.isfinite(got["best_traj"][0, 0, :10]).all()  # (no plan: NaN wherever anything is written)


@pytest.mark.parametrize("rule", ["envelope", "gates", "gaps"])
def test_tiny_table_passes(tiny, rule):
    """(the boundary pass: test_dense_tables_rank_and_mask_host_equals_device above)"""
    p = RP.PASSES[rule]
    host = getattr(tiny.eng, p.method)(tiny.batch, tiny.cost, tiny.flags, skip=tiny.skip)
    res = RP.Resident(tiny.eng, rule, tiny.batch, skip=tiny.skip)
    res.cost.copy_(tiny.up(tiny.cost))
    res.flags.copy_(tiny.up(tiny.flags.view(np.int32)))
    res.call()
    for a, b in zip(host, res.fetch()):
        assert same_bits(a, b), rule
    assert host[1][SKIPPED] == -1 and np.array_equal(host[0][SKIPPED], tiny.flags[SKIPPED])


def test_tiny_rules_eval(tiny):
    B, K = TINY_B, TINY_K
    flags = tiny.eng.eval_trajs(tiny.batch, tiny.end_states).flags
    arrays = dict(tiny.rule_arrays, end_states=tiny.end_states, flags=flags, rule_bits=np.zeros((B, K), dtype=np.uint32),
                  counts=np.ones((B, _abi.FP_RULE_COUNT), dtype=np.int32))
    got = tiny.both(tiny.eng._lib.fp_rules_eval, arrays,
                    lambda p, fb, addr, hold: (C.byref(p), C.byref(fb), C.byref(tiny.rule_set(addr, hold)), K, addr("end_states"), addr("flags"), addr("rule_bits"),
                                               addr("counts")))
    assert (got["counts"][SKIPPED] == 1).all()


@pytest.mark.parametrize("by", ["best_idx", "end_state"])
def test_tiny_traj_margins(tiny, by):
    B, K = TINY_B, TINY_K
    plans = np.stack([tiny.best_idx, np.where(tiny.best_idx < 0, -1, 0).astype(np.int32)]) if by == "best_idx" else np.ascontiguousarray(tiny.end_states.transpose(1, 0, 2))
    arrays = dict(plans=plans, min_dist=np.zeros((K, B)), min_step=np.zeros((K, B), dtype=np.int32), min_obs=np.zeros((K, B), dtype=np.int32))
    got = tiny.both(tiny.eng._lib.fp_traj_margins, arrays,
                    lambda p, fb, addr, hold: (C.byref(p), C.byref(fb), K, addr("plans") if by == "best_idx" else None, addr("plans") if by == "end_state" else None, 1,
                                               addr("min_dist"), addr("min_step"), addr("min_obs")))
    assert np.isnan(got["min_dist"][:, [NO_PLAN, SKIPPED]]).all() and not np.isnan(got["min_dist"][:, 0]).any()


@pytest.mark.parametrize("obey", [False, True])
def test_tiny_fallback_stop(tiny, obey):
    B = TINY_B
    d_targets = np.concatenate([[np.nan], np.asarray(tiny.batch.d_samples, dtype=np.float64)])
    F = d_targets.size * STOP_T.size
    arrays = dict(tiny.rule_arrays, d_targets=d_targets, stop_T=STOP_T, best_idx=tiny.best_idx, end_state=np.full((B, 3), np.nan), status=np.zeros(B, dtype=np.int32),
                  fb_idx=np.zeros(B, dtype=np.int32), hit_step=np.zeros(B, dtype=np.int32), hit_obs=np.zeros(B, dtype=np.int32), hit_speed=np.zeros(B),
                  cand=np.full((B, F), -3, dtype=np.int32), counts=np.ones((B, 4), dtype=np.int32), cand_rules=np.zeros((B, F), dtype=np.uint32),
                  rule_bits=np.zeros(B, dtype=np.uint32), rule_counts=np.ones((B, _abi.FP_RULE_COUNT), dtype=np.int32))

    def args(p, fb, addr, hold):
        fs = _abi.FpFallback(d_targets.size, STOP_T.size, addr("d_targets"), addr("stop_T"), float("inf"))
        hold.append(fs)
        head = (C.byref(p), C.byref(fb), C.byref(fs)) + ((C.byref(tiny.rule_set(addr, hold)),) if obey else ())
        outs = tuple(addr(k) for k in ("best_idx", "end_state", "status", "fb_idx", "hit_step", "hit_obs", "hit_speed", "cand"))
        return head + outs + ((addr("cand_rules"), addr("rule_bits"), addr("counts"), addr("rule_counts")) if obey else (addr("counts"),))

    got = tiny.both(tiny.eng._lib.fp_fallback_stop_rules if obey else tiny.eng._lib.fp_fallback_stop, arrays, args)
    assert got["status"][NO_PLAN] != _abi.FALLBACK_NOT_NEEDED and got["status"][0] == _abi.FALLBACK_NOT_NEEDED and (got["cand"][NO_PLAN] != -3).all()
    assert got["counts"][SKIPPED].tolist() == [2, 1, 1, 1]  # (a skipped ego counts as "not needed")


def test_tiny_share_plans(tiny):
    b = tiny.batch
    group_ptr, members = np.array([0, 2], dtype=np.int32), np.array([0, NO_PLAN], dtype=np.int32)
    arrays = dict(group_ptr=group_ptr, members=members, best_idx=tiny.best_idx, obs_pose=np.array(b.obs_pose, dtype=np.float64), fts=np.array(b.final_time_step, dtype=np.int32))
    for tail in (_abi.FP_TAIL_NONE, _abi.FP_TAIL_COAST):
        def args(p, fb, addr, hold):
            fa = _abi.FpAgents(1, 2, addr("group_ptr"), addr("members"), 2, 12, tail, 0)
            hold.append(fa)
            return C.byref(p), C.byref(fb), C.byref(fa), addr("best_idx"), None, addr("obs_pose"), addr("fts")

        got = tiny.both(tiny.eng._lib.fp_obstacles_from_plans, arrays, args)
        assert not same_bits(got["obs_pose"], arrays["obs_pose"])


def test_tiny_materialize_all(tiny):
    B, Cn = TINY_B, tiny.batch.C
    for sparse in (0, 1):
        arrays = dict(flags=np.zeros((B, Cn), dtype=np.uint32), traj=np.full((B, Cn, 16, 128), -7.5))
        tiny.both(tiny.eng._lib.fp_materialize_all, arrays, lambda p, fb, addr, hold: (C.byref(p), C.byref(fb), addr("flags"), addr("traj"), 128, sparse))


def _loop_arrays(tiny):
    b, B = tiny.batch, TINY_B
    done = np.zeros(B, dtype=np.int32)
    done[SKIPPED] = _abi.DONE_GOAL
    return dict(ego=np.array(b.ego, dtype=np.float64), t_now=np.array(b.t_now, dtype=np.int32), done=done, cycles=np.arange(B, dtype=np.int32),
                goal_xy=np.full((B, 2), 1e9), cart_state=np.zeros((B, 3)))


def _loop_io(addr, hold):
    io = _abi.FpLoopIo()
    io.ego, io.t_now, io.done, io.cycles, io.goal_xy, io.cart_state = (addr(k) for k in ("ego", "t_now", "done", "cycles", "goal_xy", "cart_state"))
    hold.append(io)
    return io


@pytest.mark.parametrize("by", ["best_idx", "end_state"])
def test_tiny_advance(tiny, by):
    """(the host path fills cart_state with 0xFF bytes - NaN - before the kernel writes the egos that move: the device copy starts there)"""
    arrays = dict(_loop_arrays(tiny), best_idx=tiny.best_idx, end_state=np.ascontiguousarray(tiny.end_states[:, 0]))
    got = tiny.both(tiny.eng._lib.fp_advance, arrays,
                    lambda p, fb, addr, hold: (C.byref(p), C.byref(fb), addr("best_idx") if by == "best_idx" else None, addr("end_state") if by == "end_state" else None,
                                               C.byref(_loop_io(addr, hold))), device_fill=dict(cart_state=0xFF))
    assert got["done"].tolist() == [_abi.RUNNING, _abi.DONE_NO_SOLUTION, _abi.DONE_GOAL] and got["cycles"][0] == 1 and got["cycles"][SKIPPED] == 2
    assert np.isfinite(got["cart_state"][0]).all() and np.isnan(got["cart_state"][1:]).all()


def test_tiny_loop_record(tiny):
    B, rows = TINY_B, 2
    arrays = dict(_loop_arrays(tiny), best_idx=tiny.best_idx, best_cost=np.array([1.5, np.nan, 2.5]), stats=np.arange(B * 4, dtype=np.int32).reshape(B, 4),
                  rows=np.full((B, rows, _abi.FP_LOG_COLS), -7.25), row_stats=np.full((B, rows, 4), -77, dtype=np.int32), n_rows=np.zeros(B, dtype=np.int32),
                  sealed=np.array([0, 0, 1], dtype=np.int32), stats_sum=np.zeros((B, 4), dtype=np.int64), n_running=np.full(1, -1, dtype=np.int32))
    arrays["done"][NO_PLAN] = _abi.DONE_NO_SOLUTION
    arrays["cycles"][:] = (1, 1, 2)  # (egos 0 and 1 have driven a cycle that is not in the log yet)

    def args(p, fb, addr, hold):
        lg = _abi.FpLoopLog()
        lg.max_rows = rows
        lg.rows, lg.row_stats, lg.n_rows, lg.sealed, lg.stats_sum, lg.n_running = (addr(k) for k in ("rows", "row_stats", "n_rows", "sealed", "stats_sum", "n_running"))
        hold.append(lg)
        return C.byref(p), C.byref(fb), C.byref(_loop_io(addr, hold)), addr("best_idx"), None, addr("best_cost"), addr("stats"), C.byref(lg)

    got = tiny.both(tiny.eng._lib.fp_loop_record, arrays, args)
    assert got["n_rows"].tolist() == [1, 1, 0] and got["sealed"].tolist() == [0, 1, 1] and got["n_running"][0] == 1


def test_tiny_build_frames_and_from_state(tiny):
    b = tiny.batch
    F, NX = b.knots.shape
    rng = np.random.default_rng(7401)
    pts = np.cumsum(np.stack([np.full((F, NX), 5.0), rng.normal(0.0, 0.4, (F, NX))], axis=2), axis=1)
    arrays = dict(n=np.full(F, NX, dtype=np.int32), points=pts, knots=np.zeros((F, NX)), coef=np.zeros((F, 8, NX)))
    got = tiny.both(tiny.eng._lib.fp_frames_build, arrays, lambda p, fb, addr, hold: (F, NX, addr("n"), addr("points"), addr("knots"), addr("coef")))
    assert np.isfinite(got["coef"]).all() and (np.diff(got["knots"], axis=1) > 0).all()

    s = np.asarray(b.ego)[:, 0] + 3.0
    px, py, yaw = synth.sample_frames(b.knots[b.frame_of], b.coef[b.frame_of], s[:, None])
    states = np.ascontiguousarray(np.stack([px[:, 0] + 0.3, py[:, 0] - 0.2, yaw[:, 0] + 0.05, np.full(TINY_B, 6.0)], axis=1))
    arrays = dict(states=states, ego=np.zeros((TINY_B, 6)))
    got = tiny.both(lambda ctx, p, fb, *rest: tiny.eng._lib.fp_from_state(ctx, fb, *rest), arrays,
                    lambda p, fb, addr, hold: (C.byref(p), C.byref(fb), addr("states"), addr("ego")))
    assert np.isfinite(got["ego"]).all()


@pytest.mark.parametrize("outputs", ["all", "traj only"])
def test_tiny_eval_trajs(tiny, outputs):
    """("traj only": the host call passes NULL for cost and flags and gives the kernel temporaries instead; its series are the ones of the
    device call, which has to pass both)"""
    B, K = TINY_B, TINY_K
    for sparse in (0, 1):
        arrays = dict(end_states=tiny.end_states, cost=np.zeros((B, K)), flags=np.zeros((B, K), dtype=np.uint32), traj=np.full((B, K, 16, 128), -7.5))
        got = tiny.both(tiny.eng._lib.fp_eval_trajs, arrays,
                        lambda p, fb, addr, hold: (C.byref(p), C.byref(fb), K, addr("end_states"), addr("cost"), addr("flags"), addr("traj"), 128, sparse),
                        host_null=("cost", "flags") if outputs == "traj only" else ())
        assert np.isfinite(got["traj"][0, :, 0, :10]).all() and (outputs == "all") == bool(np.isnan(got["cost"][NO_PLAN]).all())
