"""GPU: oracle parity at every compiled-in limit and packed-field width, on both sides of it.

The kernels change code path at the limits of include/frenet_gpu.h and at the widths of the fused kernel's packed fields
(csrc/frenet_lattice_fused.hip fused_shape / lattice_group_fit).  Each row runs the value AT the limit (the fast path must be taken - a
forced `lattice_kernel = 2` succeeds, a launch counter moves - and agree with the oracle: flag words incl. N and M, best_idx, Stats exact,
costs within 1e-9 of the oracle's and, at tick 0.1, within 1e-12 relative of the exact cost of tests/exact_cost.py) and the value just
PAST it (the fallback gives the oracle's answer while a forced fused kernel fails, or the call is refused with FP_ELIMIT naming the limit).
"""
import math

import numpy as np
import pytest

import exact_cost as X
import lattice_paths as L
from conftest import assert_series_close
from fiss_plus_planner_amd import _abi, synth
from fiss_plus_planner_amd.batch import ProblemBatch
from fiss_plus_planner_amd.engine import make_params

pytestmark = pytest.mark.gpu


def horizon(N, tick=0.1):
    """A T with len(np.arange(0, T, tick)) == ceil(T / tick) == N (half a tick below N ticks)."""
    T = (N - 0.5) * tick
    assert math.ceil(T / tick) == N == len(np.arange(0.0, T, tick)), (N, T)
    return T


def horizon_below_integer(N, tick=0.1):
    """T = N * tick as a double (T / tick may round to either side of N) and ceil(T / tick), asserted equal to len(np.arange(0, T, tick))."""
    T = N * tick
    n = math.ceil(T / tick)
    assert n == len(np.arange(0.0, T, tick)), (N, T, n)
    return T, n


def with_horizons(batch, Ts, ego_kick=False, seed=0):
    """The batch with t_samples = Ts (its FISS sampling box follows) and, with ego_kick, large initial lateral speed / acceleration on
    every other ego (|d_d| ~ 3, |d_dd| ~ 2: where a monomial-basis lateral sum would cancel)."""
    Ts = np.asarray(Ts, dtype=np.float64)
    kw = {k: getattr(batch, k) for k in ("d_samples", "v_samples", "target_speed", "ego", "frame_of", "scene_of", "t_now", "nx", "knots", "coef",
                                          "obs_pose", "obs_dims", "final_time_step", "veh_l", "veh_w", "max_speed", "max_accel", "tick_t", "check_stride",
                                          "samp_min", "samp_max", "samp_res")}
    ego = kw["ego"].copy()
    if ego_kick:
        rng = np.random.default_rng(seed)
        k = np.arange(0, batch.B, 2)
        ego[k, 4] = rng.choice([-3.0, 3.0], len(k)) * rng.uniform(0.9, 1.0, len(k))
        ego[k, 5] = rng.choice([-2.0, 2.0], len(k)) * rng.uniform(0.9, 1.0, len(k))
    smin, smax, sres = kw["samp_min"].copy(), kw["samp_max"].copy(), kw["samp_res"].copy()
    smin[:, 2], smax[:, 2] = Ts.min(), Ts.max()
    sres[:, 2] = (Ts.max() - Ts.min()) / (len(Ts) - 1) if len(Ts) > 1 else 1.0
    kw.update(t_samples=Ts, ego=ego, samp_min=smin, samp_max=smax, samp_res=sres)
    if ego_kick:  # (such starts break the speed / acceleration limits everywhere: lift them, or no candidate would survive to be compared)
        kw.update(max_speed=1e3, max_accel=1e3)
    return ProblemBatch(**kw, meta=dict(batch.meta, horizons=[float(t) for t in Ts]))


def check_dense(out, ref, what):
    L.compare(out, ref, what, cost="relative")


def exact_costs(batch, egos=None, cands=None):
    """{(ego, cand): exact cost} of the lattice candidates (all, or `cands` per ego)."""
    out = {}
    for e in range(batch.B) if egos is None else egos:
        for c in range(batch.C) if cands is None else cands:
            iv, it, i_d = c % batch.nv, (c // batch.nv) % batch.nt, c // (batch.nv * batch.nt)
            out[e, c] = X.cost_total(batch.ego[e], batch.d_samples[i_d], batch.v_samples[e, iv], batch.t_samples[it], batch.tick_t, batch.target_speed[e])
    return out


def assert_exact(table, exact, what):
    worst = 0.0
    for (e, c), ex in exact.items():
        err = X.rel_err(table[e, c], ex)
        assert err <= X.REL_BAR, f"{what} ego {e} cand {c}: {table[e, c]!r} vs exact {float(ex)!r} (rel {err:.2e})"
        worst = max(worst, err)
    return worst


def series_check(oracle, batch, best_idx, best_traj, stride, what):
    n = 0
    for e, pr in enumerate(oracle.problems_from_batch(batch)):
        if best_idx[e] < 0:
            assert np.isnan(best_traj[e]).all()
            continue
        bi = int(best_idx[e])
        iv, it, i_d = bi % batch.nv, (bi // batch.nv) % batch.nt, bi // (batch.nv * batch.nt)
        t = pr.eval_traj(batch.d_samples[i_d], batch.v_samples[e, iv], batch.t_samples[it], dump=True, stride=stride)
        assert_series_close(best_traj[e], t.arrays, batch.tick_t, f"{what} ego {e}")
        n += 1
    return n


# ---------------------------------------------------------------------------------------------------- points per trajectory
POINT_SETS = [((1, 2, 64), "N <= 64"), ((65, 127, 128), "N up to FP_FAST_POINTS"), ((127, 128, 129), "N one past FP_FAST_POINTS"),
              ((129, 255, 256), "N up to FP_MAX_POINTS")]


@pytest.mark.parametrize("Ns,label", POINT_SETS, ids=[s[1] for s in POINT_SETS])
def test_points_per_trajectory_dense(oracle, engine, Ns, label):
    """Every lattice kernel instance (the five MODES), the lane-per-candidate kernel and the default at N = 1 .. 256; flag words (N, M
    included), best_idx, Stats and costs against the oracle, every cost of the fused and lane-per-candidate kernels within 1e-12 relative
    of the exact cost; the winners' series written inside the lattice kernel (lattice_winner = 1) and by winner_traj_kernel (= 2)."""
    Ts = [horizon(N) for N in Ns]
    batch = with_horizons(synth.make_batch(6, 5, 4, len(Ts), 8, 260, True, 3100 + Ns[-1]), Ts, ego_kick=True, seed=Ns[-1])
    assert batch.C == 60
    probs = oracle.problems_from_batch(batch)
    ref = [p.fop_plan() for p in probs]
    N_ref = np.stack([(r.flags >> 8) & 0xFFF for r in ref])
    assert sorted(set(N_ref.ravel().tolist())) == sorted(Ns)
    p = make_params(batch)
    assert p.points_max == (0 if max(Ns) <= _abi.FP_FAST_POINTS else max(Ns))   # which side of FP_FAST_POINTS the call is sized for
    exact = exact_costs(batch, egos=range(4))
    # the oracle meets the bar the kernels are held to
    assert_exact(np.stack([r.cost for r in ref]), exact, f"oracle ({label})")
    if min(Ns) > 2:  # (the absolute 1e-6 bar: one- and two-point trajectories cost ~1e10, checked relatively below)
        L.through_modes(ref, engine, batch, f"points {Ns}", L.EDGE_MODES, winner=False, cost="abs1e-6")
    for opts, what in (({"lattice_kernel": 2}, "fused"), ({"lattice_kernel": 2, "lattice_split": 1}, "fused, one workgroup per ego"),
                       ({"lattice_kernel": 1}, "lattice_percand"), ({}, "default")):
        with L.options(engine, opts):
            out = engine.plan_dense(batch)
        check_dense(out, ref, f"{what} {Ns}")
        w = assert_exact(out.cost, exact, f"{what} {Ns}")
        assert w <= X.REL_BAR
    stride = 256
    for lw in (1, 2):
        with L.options(engine, {"lattice_winner": lw}):
            wo = engine.plan_dense(batch, tables=False, winner=True, traj_stride=stride)
        assert np.array_equal(wo.best_idx, [r.best_idx for r in ref])
        assert series_check(oracle, batch, wo.best_idx, wo.best_traj, stride, f"winner series (lattice_winner {lw}) {Ns}") >= 1
    # eval_trajs: every candidate of two egos as explicit end states; costs exact to the bar, N / M / flags as the oracle's
    es = np.array([[[batch.d_samples[c // (batch.nv * batch.nt)], batch.v_samples[e, c % batch.nv], batch.t_samples[(c // batch.nv) % batch.nt]]
                    for c in range(batch.C)] for e in range(batch.B)])
    ev = engine.eval_trajs(batch, es, dump=True, traj_stride=stride)
    for e, r in enumerate(ref):
        np.testing.assert_array_equal(ev.flags[e], r.flags, err_msg=f"eval_trajs ego {e}")
        L.cost_close(ev.cost[e], r.cost, f"eval_trajs ego {e}")
    assert_exact(ev.cost, exact, f"eval_trajs {Ns}")
    for e in (0, 1):
        for c in range(0, batch.C, 7):
            t = probs[e].eval_traj(*es[e, c], dump=True, stride=stride)
            assert_series_close(ev.traj[e, c], t.arrays, batch.tick_t, f"eval_trajs series ego {e} cand {c}")
    # the materialiser (fast path: one chunk; beyond FP_FAST_POINTS: the chunked writer)
    sub = batch.take(np.array([0, 1]))
    m = engine.materialize_all(sub, traj_stride=stride)
    for e, pr in enumerate(probs[:2]):
        for c in range(sub.C):
            t = pr.eval_traj(*es[e, c], dump=True, stride=stride)
            assert ((m.flags[e, c] >> 8) & 0xFFF, m.flags[e, c] >> 20) == (t.N, t.M)
            assert_series_close(m.traj[e, c], t.arrays, batch.tick_t, f"materialize_all ego {e} cand {c}")


def test_points_a_horizon_just_below_an_integer_number_of_ticks(oracle, engine):
    """T = k * 0.1 (k <= 256) whose T / 0.1 lands just below k in double (ceil = k) and just above it (ceil = k + 1): N = ceil(T / tick) =
    len(np.arange(0, T, tick)) in the kernels as in the oracle (flag words carry N)."""
    picks = [horizon_below_integer(k) + (k,) for k in range(1, 256)]
    below = [(T, n) for T, n, k in picks if T / 0.1 < k]
    above = [(T, n) for T, n, k in picks if T / 0.1 > k]
    assert below and above and all(n == k for (T, n), k in zip(below, [k for T, n, k in picks if T / 0.1 < k]))
    assert all(n == round(T / 0.1) + 1 for T, n in above)
    Ts = sorted({below[0][0], below[-1][0], above[-1][0]})
    batch = with_horizons(synth.make_batch(3, 3, 3, len(Ts), 6, 260, True, 3200), Ts)
    ref = L.reference(oracle, batch)
    for T in Ts:
        assert math.ceil(T / 0.1) == len(np.arange(0.0, T, 0.1))
    for opts in ({"lattice_kernel": 2}, {"lattice_kernel": 1}):
        with L.options(engine, opts):
            check_dense(engine.plan_dense(batch), ref, f"T just below / above k ticks {opts}")


def test_points_past_the_limit_are_refused(engine):
    """N = 257 (T = 25.65 s at tick 0.1): FP_ELIMIT naming FP_MAX_POINTS from the dense pass and eval_trajs."""
    T = horizon(257)
    batch = with_horizons(synth.make_batch(2, 3, 3, 2, 4, 60, True, 3300), [horizon(256), T])
    with pytest.raises(_abi.FrenetGpuError, match="FP_MAX_POINTS") as ex:
        engine.plan_dense(batch)
    assert ex.value.code == -4
    ok = with_horizons(synth.make_batch(2, 3, 3, 2, 4, 60, True, 3300), [horizon(255), horizon(256)])
    es = np.array([[[0.0, 5.0, T]], [[0.0, 5.0, horizon(256)]]])
    with pytest.raises(_abi.FrenetGpuError, match="FP_MAX_POINTS") as ex:
        engine.eval_trajs(ok, es)
    assert ex.value.code == -4
    assert engine.plan_dense(ok).best_idx.shape == (2,)   # the ctx survives


def test_fiss_refinement_up_to_256_points(oracle, engine):
    """FISS / FISS+ on the device at tick 0.1 with horizons from 12.75 s (N = 128) to 25.55 s (N = 256): Stats, best_ijk, refined flag,
    end state and best cost against the oracle; the refined best cost within 1e-12 relative of the exact cost of its end state.  A sampling
    box whose upper T needs 257 points: FP_ELIMIT (a refinement probe there would silently come back as NaN)."""
    Ts = [horizon(128), horizon(129), horizon(192), horizon(256)]
    n_ref = 0
    for kind in ("FISS", "FISS+"):
        base = synth.make_batch(8, 5, 5, len(Ts), 8, 260, True, 3400, kind=kind)
        fb = with_horizons(base, Ts, ego_kick=True, seed=34)
        out = engine.plan_fiss(fb, kind, winner=True, traj_stride=256)
        for e, pr in enumerate(oracle.problems_from_batch(fb)):
            r = pr.fissplus_plan() if kind == "FISS+" else pr.fiss_plan()
            np.testing.assert_array_equal(out.stats[e], r.stats, err_msg=f"{kind} ego {e}")
            np.testing.assert_array_equal(out.best_ijk[e], r.best_ijk, err_msg=f"{kind} ego {e}")
            assert np.isnan(out.best_cost[e]) == np.isnan(r.best_cost)
            if np.isnan(r.best_cost):
                continue
            L.cost_close(out.best_cost[e], r.best_cost, f"{kind} ego {e}")
            es = out.end_state[e]
            ex = X.cost_total(fb.ego[e], es[0], es[1], es[2], fb.tick_t, fb.target_speed[e])
            assert X.rel_err(out.best_cost[e], ex) <= X.REL_BAR, (kind, e, out.best_cost[e], float(ex))
            assert X.rel_err(r.best_cost, ex) <= X.REL_BAR
            t = pr.eval_traj(*es, dump=True, stride=256)
            assert_series_close(out.best_traj[e], t.arrays, fb.tick_t, f"{kind} winner ego {e}")
            if kind == "FISS+":
                assert bool(out.refined[e]) == r.refined
                n_ref += int(r.refined)
    assert n_ref >= 1
    bad = with_horizons(synth.make_batch(2, 5, 5, 3, 8, 260, True, 3401, kind="FISS+"), [horizon(128), horizon(192), horizon(256)])
    bad.samp_max[:, 2] = horizon(257)
    with pytest.raises(_abi.FrenetGpuError, match="FP_MAX_POINTS") as ex:
        engine.plan_fiss(bad, "FISS+")
    assert ex.value.code == -4


# ---------------------------------------------------------------------------------------------------- dense-pass limits
def _fused_refuses(engine, batch):
    with L.options(engine, {"lattice_kernel": 2}), pytest.raises(_abi.FrenetGpuError):
        engine.plan_dense(batch)


def _fused_takes(oracle, engine, batch, ref, what, modes=L.EDGE_MODES):
    L.through_modes(ref, engine, batch, what, modes, winner=False, cost="abs1e-6")
    with L.options(engine, {"lattice_kernel": 2}):
        out = engine.plan_dense(batch)
    check_dense(out, ref, what)
    return out


def _fallback(oracle, engine, batch, ref, what):
    _fused_refuses(engine, batch)
    check_dense(engine.plan_dense(batch), ref, what)


def test_largest_dense_lattice(oracle, engine):
    """C = 64 x 16 x 16 = FP_MAX_CAND = 16384 (nd = 64: one lane per lateral sample), every mode; 16385 = 5 x 29 x 113: FP_ELIMIT."""
    batch = synth.make_batch(1, 64, 16, 16, 6, 50, True, 3500)
    assert batch.C == _abi.FP_MAX_CAND
    ref = L.reference(oracle, batch)
    _fused_takes(oracle, engine, batch, ref, "C = FP_MAX_CAND")
    past = synth.make_batch(1, 5, 29, 113, 6, 50, True, 3501)
    assert past.C == _abi.FP_MAX_CAND + 1
    with pytest.raises(_abi.FrenetGpuError, match="FP_MAX_CAND") as ex:
        engine.plan_dense(past)
    assert ex.value.code == -4


def test_lateral_samples_one_lane_each(oracle, engine):
    """nd = 64 (the fused kernel's lanes) on every instance; nd = 65: the fused kernel refuses, the default falls back."""
    at = synth.make_batch(3, 64, 2, 2, 8, 50, True, 3600)
    _fused_takes(oracle, engine, at, [p.fop_plan() for p in oracle.problems_from_batch(at)], "nd = 64")
    past = synth.make_batch(3, 65, 2, 2, 8, 50, True, 3601)
    _fallback(oracle, engine, past, [p.fop_plan() for p in oracle.problems_from_batch(past)], "nd = 65")


def test_speed_samples_8bit_profile_index(oracle, engine):
    """nv = 255 (the hit word's 8-bit profile index) on every instance; nv = 256: fallback."""
    at = synth.make_batch(2, 3, 255, 2, 8, 50, True, 3700)
    _fused_takes(oracle, engine, at, [p.fop_plan() for p in oracle.problems_from_batch(at)], "nv = 255")
    past = synth.make_batch(2, 3, 256, 2, 8, 50, True, 3701)
    _fallback(oracle, engine, past, [p.fop_plan() for p in oracle.problems_from_batch(past)], "nv = 256")


def test_grouped_slices_profile_index(oracle, engine):
    """lattice_group = 99: granted as g while g * nv <= 256 (group_fit) - nv = 128 gets two and with it the 1024-thread instance, nv = 129
    one and the plain instance; both through the fused kernel (it does not refuse: the group shrinks) and equal to the oracle."""
    for nv in (128, 129):
        batch = synth.make_batch(2, 3, nv, 4, 8, 50, True, 3800 + nv)
        ref = L.reference(oracle, batch)
        for opts in ({"lattice_kernel": 2, "lattice_group": 99}, {"lattice_kernel": 2, "lattice_group": 99, "lattice_split": 1}):
            with L.options(engine, opts):
                out = engine.plan_dense(batch)
            check_dense(out, ref, f"grouped nv = {nv} {opts}")


def _scene(B, n_obs, T_obs, seed, stride=2, Ts=None):
    b = synth.make_batch(B, 3, 3, 2, n_obs, T_obs, True, seed)
    b.check_stride = stride
    return with_horizons(b, Ts) if Ts is not None else b


def test_obstacle_count(oracle, engine):
    """n_obs = 4095 / 4096 (rows x n_obs kept <= 65535: 15 rows): the 12-bit obstacle field is not what binds - a 4095-obstacle scene
    does not fit the fused kernel's LDS layout either, so a forced fused launch fails on both sides and the default (lane-per-candidate)
    gives the oracle's answer."""
    for n_obs in (4095, 4096):
        batch = _scene(1, n_obs, 30, 3900 + n_obs)
        rows = min(math.ceil(128 / 2), math.ceil(batch.T_obs / 2))
        assert rows * n_obs <= 65535
        ref = L.reference(oracle, batch)
        assert any(((r.flags & 4) != 0).any() for r in ref)
        _fallback(oracle, engine, batch, ref, f"n_obs = {n_obs}")


def test_row_obstacle_pairs_16bit(oracle, engine):
    """rows x n_obs = 255 x 257 = 65535 (check stride 1, N = 256 so points_cap = 256, T_obs = 255 rows) on the fused kernel;
    256 x 256 = 65536: fallback.  rows = min(ceil(points_cap / stride), ceil(T_obs / stride)), fused_shape's own formula."""
    for rows_want, n_obs, fused in ((255, 257, True), (256, 256, False)):
        batch = _scene(1, n_obs, rows_want, 4000 + n_obs, stride=1, Ts=[horizon(200), horizon(256)])
        cap = make_params(batch).points_max
        assert cap == 256
        rows = min(math.ceil(cap / batch.check_stride), math.ceil(batch.T_obs / batch.check_stride))
        assert rows * n_obs == (65535 if fused else 65536)
        ref = L.reference(oracle, batch)
        if fused:
            _fused_takes(oracle, engine, batch, ref, f"rows x n_obs = {rows} x {n_obs}", modes=[L.MODES[0], L.MODES[4]])
        else:
            _fallback(oracle, engine, batch, ref, f"rows x n_obs = {rows} x {n_obs}")


def test_polygon_ring_vertices(oracle, engine):
    """Rings of 3, 4 and 128 = FP_MAX_POLY_VERTS vertices (poly_stride 128) against the oracle's polygon predicate on the fused and
    lane-per-candidate kernels; poly_stride 129: FP_ELIMIT naming FP_MAX_POLY_VERTS."""
    base = synth.make_batch(3, 5, 4, 3, 6, 60, True, 4100)
    rng = np.random.default_rng(41)

    def shaped(stride):
        S, n = base.S, base.n_obs
        poly = np.zeros((S, n, stride, 2))
        nvert = np.zeros((S, n), dtype=np.int32)
        dims = base.obs_dims.copy()
        for sc in range(S):
            for j, k in enumerate((3, 4, min(stride, 128), 0, 3, min(stride, 128))):
                if k == 0:
                    continue
                ring = synth.random_convex_ring(rng, k, 0.5 * dims[sc, j, 0], 0.5 * dims[sc, j, 1])
                ring = ring - 0.5 * (ring.min(axis=0) + ring.max(axis=0))
                poly[sc, j, :k] = ring
                nvert[sc, j] = k
                dims[sc, j] = 2.0 * np.abs(ring).max(axis=0)
        kw = {k: getattr(base, k) for k in ("d_samples", "t_samples", "v_samples", "target_speed", "ego", "frame_of", "scene_of", "t_now", "nx", "knots",
                                             "coef", "obs_pose", "final_time_step", "veh_l", "veh_w", "max_speed", "max_accel", "tick_t", "check_stride")}
        return ProblemBatch(**kw, obs_dims=dims, obs_poly=poly, obs_nvert=nvert)

    batch = shaped(128)
    assert batch.obs_poly.shape[2] == _abi.FP_MAX_POLY_VERTS and set(batch.obs_nvert.ravel().tolist()) == {0, 3, 4, 128}
    ref = L.reference(oracle, batch)
    assert any(((r.flags & 4) != 0).any() for r in ref)
    for opts in ({"lattice_kernel": 2}, {"lattice_kernel": 1}, {}):
        with L.options(engine, opts):
            check_dense(engine.plan_dense(batch), ref, f"poly rings {opts}")
    past = shaped(129)
    with pytest.raises(_abi.FrenetGpuError, match="FP_MAX_POLY_VERTS") as ex:
        engine.plan_dense(past)
    assert ex.value.code == -4


# ---------------------------------------------------------------------------------------------------- FISS search walk
def test_device_search_walk_at_its_limit(oracle, engine):
    """C = 16 x 16 x 16 = FP_MAX_CAND_SEARCH on the device walk, FISS and FISS+, Stats exact; C = 4100 (just past): fp_plan_fiss refuses
    naming the limit and the drop-in FissPlusPlanner takes the host walk."""
    from fiss_plus_planner_amd import planners as P
    from fiss_plus_planner_amd.vehicle import Vehicle

    for kind in ("FISS", "FISS+"):
        fb = synth.make_batch(2, 16, 16, 16, 10, 50, True, 4200, kind=kind)
        assert fb.C == _abi.FP_MAX_CAND_SEARCH
        out = engine.plan_fiss(fb, kind)
        for e, pr in enumerate(oracle.problems_from_batch(fb)):
            r = pr.fissplus_plan() if kind == "FISS+" else pr.fiss_plan()
            np.testing.assert_array_equal(out.stats[e], r.stats, err_msg=f"{kind} ego {e}")
            np.testing.assert_array_equal(out.best_ijk[e], r.best_ijk, err_msg=f"{kind} ego {e}")
            L.cost_close(out.best_cost[e], r.best_cost, f"{kind} ego {e}")
    assert P.FissPlusPlanner(P.FissPlusPlannerSettings(16, 16, 16), Vehicle(), None, engine=engine)._device_walk()
    past = synth.make_batch(1, 10, 10, 41, 10, 50, True, 4201, kind="FISS+")
    assert past.C > _abi.FP_MAX_CAND_SEARCH
    with pytest.raises(_abi.FrenetGpuError, match="FP_MAX_CAND_SEARCH") as ex:
        engine.plan_fiss(past, "FISS+")
    assert ex.value.code == -4
    assert not P.FissPlusPlanner(P.FissPlusPlannerSettings(10, 10, 41), Vehicle(), None, engine=engine)._device_walk()


# ---------------------------------------------------------------------------------------------------- device calls: points_max
def test_device_calls_size_themselves_from_points_max(oracle, engine):
    """FP_MEM_DEVICE calls cannot look at t_samples: fp_params.points_max = 0 holds N <= 128 and 200 holds N <= 200.  A trajectory that
    needs one point more (129 / 201) comes back as NaN cost + infeasible (include/frenet_gpu.h), from plan_dense_device and
    eval_trajs_device; the candidates that fit equal the oracle's."""
    import torch

    from fiss_plus_planner_amd.device_batch import DeviceBatch

    for pm, n_ok, n_past in ((0, 128, 129), (200, 200, 201)):
        batch = with_horizons(synth.make_batch(4, 3, 3, 2, 6, 260, True, 4300 + pm), [horizon(n_ok), horizon(n_past)])
        ref = L.reference(oracle, batch)
        db = DeviceBatch(batch, 0)
        params = make_params(batch)
        params.points_max = pm
        B, C = batch.B, batch.C
        bi, bc, st = db.empty(B, torch.int32), db.empty(B, torch.float64), db.empty((B, 4), torch.int32)
        ct, ft = db.empty((B, C), torch.float64), db.empty((B, C), torch.int32)
        engine.plan_dense_device(params, db.fb, bi.data_ptr(), bc.data_ptr(), st.data_ptr(), ct.data_ptr(), ft.data_ptr())
        torch.cuda.synchronize()
        cost, flags = ct.cpu().numpy(), ft.cpu().numpy().view(np.uint32)
        it = (np.arange(C) // batch.nv) % batch.nt
        for e, r in enumerate(ref):
            fit = it == 0
            np.testing.assert_array_equal(flags[e, fit], r.flags[fit], err_msg=f"points_max {pm} ego {e}")
            L.cost_close(cost[e, fit], r.cost[fit], f"points_max {pm} ego {e}")
            assert np.isnan(cost[e, ~fit]).all(), (pm, e)
            assert ((flags[e, ~fit] & _abi.FLAG_INFEASIBLE) != 0).all(), (pm, e)
        es = torch.tensor([[[0.0, 5.0, horizon(n_ok)], [0.0, 5.0, horizon(n_past)]]] * B, dtype=torch.float64, device=db.dev)
        ec, ef = db.empty((B, 2), torch.float64), db.empty((B, 2), torch.int32)
        engine.eval_trajs_device(params, db.fb, 2, es.data_ptr(), ec.data_ptr(), ef.data_ptr())
        torch.cuda.synchronize()
        ec, ef = ec.cpu().numpy(), ef.cpu().numpy().view(np.uint32)
        for e, pr in enumerate(oracle.problems_from_batch(batch)):
            t = pr.eval_traj(0.0, 5.0, horizon(n_ok))
            assert (ef[e, 0] & 0xFF) == t.flags and ((ef[e, 0] >> 8) & 0xFFF, ef[e, 0] >> 20) == (t.N, t.M) and abs(ec[e, 0] - t.cost) <= 1e-9 * max(1.0, abs(t.cost))
            assert np.isnan(ec[e, 1]) and (ef[e, 1] & _abi.FLAG_INFEASIBLE) != 0
