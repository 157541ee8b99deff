"""GPU: fp_speed_envelope (position-dependent speed limits and stop lines behind the dense pass) against its numpy + oracle restatement
(tests/envelope_ref.py): flag words exact on every candidate the reference decides by more than 1e-9, bits only ever added, every other
bit and the cost table untouched, the argmin and the violation count exact, through both memory spaces, with a launch order and a
skipped ego; idempotence, the stop line on the winner's own series, the entry points that take its outputs, graph capture, a ctx that
never asks, the planner class and the error codes."""
import dataclasses

import numpy as np
import pytest

import envelope_ref as R
import rule_pass as RP
from fiss_plus_planner_amd import _abi, synth
from rule_pass import same_bits

pytestmark = pytest.mark.gpu
RULE = "envelope"
SPEED, ACCEL = np.uint32(R.FLAG_SPEED), np.uint32(R.FLAG_ACCEL)
BOTH = SPEED | ACCEL


def dense_and_envelope(engine, batch):
    return RP.dense_and_pass(engine, RULE, batch)


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("name", list(R.CASES))
def test_parity_host(engine, oracle, name):
    batch, refs, out, got = RP.host_parity(engine, oracle, RULE, name, skip_ego=2 if name in ("base", "both") else None)
    if name == "unlimited":  # no bit may change, the winner is the dense call's
        assert np.array_equal(got[0], out.flags) and np.array_equal(got[1], out.best_idx) and same_bits(got[2], out.best_cost) and (got[3] == 0).all()
    if name == "line_ends":  # past the end: M <= 1, nothing is checked, no bit
        assert (out.flags[3] >> 20 <= 1).all() and np.array_equal(got[0][3], out.flags[3]) and got[3][3] == 0


@pytest.mark.parametrize("name", ["base", "both"])
def test_parity_device_with_order_and_skip(engine, oracle, name):
    RP.device_parity(engine, oracle, RULE, name)


def test_idempotence(engine, oracle):
    assert len(list(RP.idempotence(engine, oracle, RULE, ("both", "stop")))) == 2


# ---------------------------------------------------------------- the stop line, on the winner's own series
def test_winners_stop_before_the_line(engine, oracle):
    batch, refs = R.case(oracle, "stop")
    egos = R.stop_egos(oracle)
    assert len(egos) >= 2
    _, start = R.stop_limit(R.plain_batch())
    out, (flags, bi, bc, nl) = dense_and_envelope(engine, batch)
    w = engine.winner_trajs(batch, bi)
    for b in egos:
        assert out.best_idx[b] == refs[b].best_in and bi[b] == refs[b].best_idx != refs[b].best_in  # the unmasked winner ran the light
        M = int(w.best_flags[b]) >> 20
        s, s_d = w.best_traj[b, R.S, 1:M], w.best_traj[b, R.S_D, 1:M]
        on = s + batch.limit_front >= start[b]
        assert M > 1 and (s_d[on] <= batch.limit_tol).all(), b
        u = engine.winner_trajs(batch, out.best_idx)  # ... and the unmasked one did not stop
        Mu = int(u.best_flags[b]) >> 20
        su, sdu = u.best_traj[b, R.S, 1:Mu], u.best_traj[b, R.S_D, 1:Mu]
        assert (sdu[su + batch.limit_front >= start[b]] > batch.limit_tol).any(), b


# ---------------------------------------------------------------- composition
CORRIDOR_WIDEN = 0.2


def with_corridor(batch):
    """The envelope batch with the boundary tests' corridor (tests/boundary_ref.py) on top, both edges CORRIDOR_WIDEN further out: on the
    reference that leaves four egos of the `both` batch a survivor and moves two of their winners."""
    import boundary_ref

    left, right = boundary_ref.wavy_corridor(batch.knots)
    return dataclasses.replace(batch, bound_left=left + CORRIDOR_WIDEN, bound_right=right - CORRIDOR_WIDEN, bound_margin=0.05)


def test_rank_boundary_and_plan_dense_compose(engine, oracle):
    import boundary_ref

    batch, refs = R.case(oracle, "both")
    out = engine.plan_dense(batch, tables=True)
    flags, bi, bc, nl = engine.speed_envelope(batch, out.cost, out.flags)
    K = 4
    ri, rc, nf = engine.rank_feasible(batch, out.cost, flags, K)
    assert np.array_equal(ri[0], bi) and same_bits(np.where(bi < 0, 0.0, rc[0]), np.where(bi < 0, 0.0, bc)) and np.array_equal(np.isnan(rc[0]), bi < 0)
    for b in range(batch.B):
        idx = ri[:, b][ri[:, b] >= 0]
        assert not (flags[b, idx] & BOTH).any()
        assert nf[b] == np.count_nonzero(((flags[b] & _abi.FLAG_INFEASIBLE) == 0) & ~np.isnan(out.cost[b]))
    one = engine.plan_dense(batch, tables=True, winner=True, top_k=K, envelope=True)
    w = engine.winner_trajs(batch, bi)
    assert np.array_equal(one.flags, flags) and same_bits(one.cost, out.cost) and np.array_equal(one.best_idx, bi) and same_bits(one.best_cost, bc)
    assert np.array_equal(one.n_limited, nl) and np.array_equal(one.rank_idx, ri) and same_bits(one.rank_cost, rc) and np.array_equal(one.n_feasible, nf)
    assert same_bits(one.best_traj, w.best_traj) and np.array_equal(one.best_flags, w.best_flags)
    lean = engine.plan_dense(batch, tables=False, envelope=True)
    assert lean.cost is None and lean.flags is None and np.array_equal(lean.best_idx, bi) and np.array_equal(lean.n_limited, nl)
    with pytest.raises(ValueError):
        engine.plan_dense(R.plain_batch(), envelope=True)
    # the envelope, then the road boundary: the reference's combined argmin
    cb = with_corridor(batch)
    combined = [boundary_ref.ego_mask(oracle, cb, b, (refs[b].cost, refs[b].flags)) for b in range(cb.B)]
    flags2, bi2, bc2, nm2 = engine.boundary_mask(cb, out.cost, flags)
    assert sum(r.n_masked for r in combined) > 0 and [r.best_idx for r in combined] != [r.best_idx for r in refs]  # (the corridor decides something too)
    for b, (r, e) in enumerate(zip(combined, refs)):
        ok = ~(r.undecided | e.undecided)
        assert np.array_equal(flags2[b][ok], r.flags[ok]), b
        if ok.all():
            assert bi2[b] == r.best_idx and nm2[b] == r.n_masked, (b, int(bi2[b]), r.best_idx)
        if bi2[b] >= 0:
            assert same_bits(bc2[b:b + 1], out.cost[b, bi2[b]:bi2[b] + 1])
    two = engine.plan_dense(cb, tables=True, top_k=K, envelope=True, boundary=True, margins=True)
    assert np.array_equal(two.flags, flags2) and np.array_equal(two.best_idx, bi2) and same_bits(two.best_cost, bc2)
    assert np.array_equal(two.n_limited, nl) and np.array_equal(two.n_masked, nm2) and np.array_equal(two.rank_idx[0], bi2)
    md, ms, mo = engine.traj_margins(cb, best_idx=two.rank_idx)
    assert same_bits(two.margin_dist, md) and np.array_equal(two.margin_step, ms) and np.array_equal(two.margin_obs, mo)


# ---------------------------------------------------------------- capture
def test_dense_and_envelope_replay_from_a_graph(engine, oracle):
    RP.graph_replay(engine, oracle, RULE, "both")


# ---------------------------------------------------------------- off unless called
def test_a_ctx_that_never_asks_pays_nothing(oracle):
    RP.never_asks(oracle, RULE, "both")


# ---------------------------------------------------------------- the planner class
def test_planner_class(engine, oracle):
    from fiss_plus_planner_amd import planners as P
    from fiss_plus_planner_amd.frenet import FrenetState

    batch, refs = R.case(oracle, "both")
    b = next(i for i, r in enumerate(refs) if r.best_idx >= 0 and r.best_idx != r.best_in and not r.undecided.any())
    st = P.FrenetOptimalPlannerSettings(batch.nd, batch.nv, batch.nt)
    planner = P.FrenetOptimalPlanner(st, synth.Vehicle(), engine=engine, frame_on="host")
    # the ego's own centre line: rebuilt from its spline's knot values (coefficient a of every segment)
    planner.generate_frenet_frame(np.column_stack((batch.coef[b, 0], batch.coef[b, 4])))
    assert np.allclose(planner.cubic_spline.knots, batch.knots[b], atol=1e-9)
    e = batch.ego[b]
    fs = FrenetState(t=0.0, s=e[0], s_d=e[1], s_dd=e[2], d=e[3], d_d=e[4], d_dd=e[5])
    speed = float(batch.target_speed[b])
    before = planner.plan(fs, speed, None)
    assert before.lattice_index == refs[b].best_in
    planner.set_speed_profile(batch.speed_limit[b], tol=batch.limit_tol, max_lat_accel=batch.max_lat_accel)  # front=None: vehicle.l / 2
    assert planner._speed_profile[1] == batch.limit_front
    obeys = planner.plan(fs, speed, None)
    assert obeys.lattice_index == refs[b].best_idx and np.array_equal(planner.last_tables[1], refs[b].flags)
    w = engine.winner_trajs(batch, np.array([r.best_idx for r in refs], dtype=np.int32))
    M = int(w.best_flags[b]) >> 20
    assert np.array_equal(np.asarray(obeys.s)[:M], w.best_traj[b, R.S, :M]) and np.array_equal(np.asarray(obeys.s_d)[:M], w.best_traj[b, R.S_D, :M])
    planner.set_speed_profile(None)
    off = planner.plan(fs, speed, None)
    assert off.lattice_index == refs[b].best_in and np.array_equal(planner.last_tables[1], refs[b].flags_in)
    with pytest.raises(ValueError):
        P.FissPlusPlanner(P.FissPlusPlannerSettings(), synth.Vehicle(), engine=engine).set_speed_profile(batch.speed_limit[b])


# ---------------------------------------------------------------- errors
def test_host_errors_and_ignored_entries(engine, oracle):
    batch, _ = R.case(oracle, "both")
    lim = batch.speed_limit.copy()
    good = lambda v=lim, front=2.0, tol=0.05, lat=0.1: _abi.FpSpeedProfile(v.ctypes.data if v is not None else None, front, tol, lat)  # noqa: E731
    call = RP.host_error_codes(engine, RULE, batch, [good(v=None), good(front=-1.0), good(front=float("nan")), good(front=float("inf")), good(tol=-1e-9),
                                                     good(tol=float("inf")), good(lat=-0.1), good(lat=float("nan")), good(lat=float("inf"))])
    n1, masked = RP.launches(engine, RULE), call.flags.copy()
    nocoef = _abi.FpBatch.from_buffer_copy(call.fb)
    nocoef.coef = None
    assert call(good(), fb=nocoef) == -1 and b"coef" in engine._lib.fp_last_error()
    for value in (np.nan, -0.5):
        bad = lim.copy()
        bad[1, 7] = value
        assert call(good(v=bad)) == -1 and b"frame 1, knot 7" in engine._lib.fp_last_error()
    assert RP.launches(engine, RULE) == n1 and np.array_equal(call.flags, masked)  # (a refused call launched and wrote nothing)
    assert call(good(lat=0.0), fb=nocoef) == 0 and RP.launches(engine, RULE) == n1 + 1  # (coef is read only by the lateral check)
    # entries k >= nx[f] - 1 are ignored: a frame table with padding, NaN in the padded entries and at the last knot
    small = R.with_profile(synth.make_batch(2, 5, 4, 3, 0, 20, False, R.SEED, n_knots=61), max_lat_accel=R.MAX_LAT_ACCEL)
    NX = 64
    kn = np.full((2, NX), np.inf); kn[:, :61] = small.knots
    co = np.zeros((2, 8, NX)); co[:, :, :61] = small.coef
    li = np.full((2, NX), np.nan); li[:, :60] = small.speed_limit[:, :60]
    pad = dataclasses.replace(small, knots=kn, coef=co, speed_limit=li)
    a, b = dense_and_envelope(engine, small)[1], dense_and_envelope(engine, pad)[1]
    for x, y in zip(a, b):
        assert same_bits(x, y)
    assert 0 < a[3].sum() < 2 * small.C


def test_device_error_codes(engine, oracle):
    batch, _ = R.case(oracle, "both")
    RP.device_error_codes(engine, RULE, batch, [dict(v_limit=0), dict(front=-1.0), dict(front=float("nan")), dict(tol=-1.0), dict(tol=float("inf")),
                                                dict(max_lat_accel=-1.0), dict(max_lat_accel=float("nan"))])
