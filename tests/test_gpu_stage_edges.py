"""GPU: the FP_MEM_HOST path (every array placed by plan_stage, csrc/frenet_stage_plan.h) against the FP_MEM_DEVICE path on the same
inputs, at the edges of the staging regimes: every output bit-equal.

B = 8 / 9 is the latency switch (zero-copy outputs up to 8 egos).  16 x 8 x 8 candidates make the cost table of 8 egos exactly 64 KiB
(the largest array of the small window), 17 x 8 x 8 is the next lattice above it.  The obstacle tables take the inputs of an
8-ego call to 249.5 KiB in all (everything below the 256 KiB the kernels may read from the pinned block), to a 250 KiB table (still one
array of the window, but 300 KiB in all) and to a 257.5 KiB table (its own copy in every regime).  17 egos make the in/out flag table
of the boundary mask larger than the window takes."""
import functools

import numpy as np
import pytest

import boundary_ref as R
from fiss_plus_planner_amd import _abi, synth

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
