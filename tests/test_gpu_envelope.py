"""GPU: fp_speed_envelope (position-dependent speed limits and stop lines behind the dense pass) against its numpy + oracle restatement
(tests/envelope_ref.py): flag words exact on every candidate the reference decides by more than 1e-9, bits only ever added, every other
bit and the cost table untouched, the argmin and the violation count exact, through both memory spaces, with a launch order and a
skipped ego; idempotence, the stop line on the winner's own series, the entry points that take its outputs, graph capture, a ctx that
never asks, the planner class and the error codes."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import envelope_ref as R
from fiss_plus_planner_amd import _abi, synth
from fiss_plus_planner_amd.engine import FrenetEngine, host_structs

pytestmark = pytest.mark.gpu
SPEED, ACCEL = np.uint32(R.FLAG_SPEED), np.uint32(R.FLAG_ACCEL)
BOTH = SPEED | ACCEL


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def check_against(refs, dense, got, what, skip=None):
    """got = (flags, best_idx, best_cost, n_limited) of an envelope call over the tables of `dense` (cost, flags)."""
    flags, bi, bc, nl = got
    cost_in, flags_in = dense
    R.check_caps(refs, what)
    for b, r in enumerate(refs):
        if skip is not None and skip[b]:
            assert bi[b] == -1 and np.isnan(bc[b]) and nl[b] == 0, (what, b)
            assert np.array_equal(flags[b], flags_in[b]), (what, b)  # rows neither read nor written
            continue
        assert np.array_equal(flags_in[b], r.flags_in), (what, b)  # (the dense call's own parity with the oracle)
        assert np.array_equal(flags[b] & ~BOTH, flags_in[b] & ~BOTH), (what, b)
        assert np.array_equal(flags[b] & flags_in[b], flags_in[b]), (what, b)  # bits are only ever added
        ok = ~r.undecided
        assert np.array_equal(flags[b][ok], r.flags[ok]), (what, b, np.nonzero(flags[b] != r.flags)[0][:8].tolist())
        added = np.count_nonzero(flags[b] != flags_in[b])
        assert added <= nl[b] <= np.count_nonzero(flags[b] & BOTH), (what, b)  # (a violating candidate may have carried its bits already)
        if not r.undecided.any():
            assert nl[b] == r.n_limited and bi[b] == r.best_idx, (what, b, int(bi[b]), r.best_idx, int(nl[b]), r.n_limited)
        if bi[b] >= 0:
            assert same_bits(bc[b:b + 1], cost_in[b, bi[b]:bi[b] + 1]) and not (flags[b, bi[b]] & _abi.FLAG_INFEASIBLE), (what, b)
        else:
            assert np.isnan(bc[b]), (what, b)


def dense_and_envelope(engine, batch, skip=None):
    out = engine.plan_dense(batch, tables=True)
    cost0, flags0 = out.cost.copy(), out.flags.copy()
    got = engine.speed_envelope(batch, out.cost, out.flags, skip=skip)
    assert same_bits(out.cost, cost0) and np.array_equal(out.flags, flags0)  # the caller's tables are copies here; cost is never written
    return out, got


class Resident:
    """A batch and its limits in device memory, the dense call and the envelope behind it on one stream."""

    def __init__(self, engine, batch, order=None, skip=None, poison=None):
        import torch

        from fiss_plus_planner_amd.device_batch import DeviceBatch

        self.torch, self.engine, self.db, self.batch = torch, engine, DeviceBatch(batch, 0, order_hint=False), batch
        db, B, Cn = self.db, batch.B, batch.C
        self.fb = _abi.FpBatch.from_buffer_copy(db.fb)
        if order is not None:
            self.order = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(db.dev)
            self.fb.launch_order = self.order.data_ptr()
        if skip is not None:
            self.skip = torch.from_numpy(np.ascontiguousarray(skip, dtype=np.int32)).to(db.dev)
            self.fb.skip = self.skip.data_ptr()
        self.bi0, self.bc0 = db.empty(B, torch.int32), db.empty(B, torch.float64)
        self.bi, self.bc, self.nl = db.empty(B, torch.int32), db.empty(B, torch.float64), db.empty(B, torch.int32)
        self.cost, self.flags = torch.zeros((B, Cn), dtype=torch.float64, device=db.dev), torch.zeros((B, Cn), dtype=torch.int32, device=db.dev)
        if poison is not None:
            self.flags[poison] = -1  # 0xFFFFFFFF: a row that WOULD count (M = 4095, every bit set) if it were read

    def dense(self, stream=0):
        db = self.db
        self.engine.plan_dense_device(db.params, self.fb, self.bi0.data_ptr(), self.bc0.data_ptr(), cost_tbl=self.cost.data_ptr(), flag_tbl=self.flags.data_ptr(), stream=stream)

    def envelope(self, stream=0, **kw):
        db, b = self.db, self.batch
        a = dict(v_limit=db.t["speed_limit"].data_ptr(), front=b.limit_front, tol=b.limit_tol, max_lat_accel=b.max_lat_accel, cost_tbl=self.cost.data_ptr(),
                 flag_tbl=self.flags.data_ptr(), best_idx=self.bi.data_ptr(), best_cost=self.bc.data_ptr(), n_limited=self.nl.data_ptr())
        a.update(kw)
        self.engine.speed_envelope_device(db.params, self.fb, stream=stream, **a)

    def pair(self, stream=0):
        self.dense(stream)
        self.envelope(stream)

    def fetch(self):
        self.torch.cuda.synchronize(self.db.dev)
        return self.flags.cpu().numpy().view(np.uint32), self.bi.cpu().numpy(), self.bc.cpu().numpy(), self.nl.cpu().numpy()


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("name", list(R.CASES))
def test_parity_host(engine, oracle, name):
    batch, refs = R.case(oracle, name)
    n0 = engine.get_option("envelope_launches")
    out, got = dense_and_envelope(engine, batch)
    assert engine.get_option("envelope_launches") == n0 + 1  # one launch
    check_against(refs, (out.cost, out.flags), got, name)
    if name == "unlimited":  # no bit may change, the winner is the dense call's
        assert np.array_equal(got[0], out.flags) and np.array_equal(got[1], out.best_idx) and same_bits(got[2], out.best_cost) and (got[3] == 0).all()
    if name == "line_ends":  # past the end: M <= 1, nothing is checked, no bit
        assert (out.flags[3] >> 20 <= 1).all() and np.array_equal(got[0][3], out.flags[3]) and got[3][3] == 0
    if name in ("base", "both"):  # a skipped ego: -1 / NaN / 0, its rows untouched
        skip = np.zeros(batch.B, dtype=np.int32)
        skip[2] = 1
        out.flags[2] = 0xFFFFFFFF  # (a row that WOULD count if it were read)
        got = engine.speed_envelope(batch, out.cost, out.flags, skip=skip)
        assert (got[0][2] == 0xFFFFFFFF).all()
        out.flags[2] = refs[2].flags_in
        got[0][2] = refs[2].flags_in
        check_against(refs, (out.cost, out.flags), got, name + " skip", skip)


@pytest.mark.parametrize("name", ["base", "both"])
def test_parity_device_with_order_and_skip(engine, oracle, name):
    batch, refs = R.case(oracle, name)
    host = engine.plan_dense(batch, tables=True)
    res = Resident(engine, batch)
    res.pair()
    plain = res.fetch()
    check_against(refs, (host.cost, host.flags), plain, name + " device")
    skip = np.zeros(batch.B, dtype=np.int32)
    skip[2] = 1
    res = Resident(engine, batch, order=np.arange(batch.B)[::-1], skip=skip, poison=2)
    res.pair()
    got = res.fetch()
    assert (got[0][2] == 0xFFFFFFFF).all()  # the poisoned rows of the skipped ego come back untouched
    tables = (host.cost.copy(), host.flags.copy())
    tables[1][2] = 0xFFFFFFFF
    check_against(refs, tables, got, name + " device, reversed order, skip", skip)
    keep = skip == 0
    for a, b in zip(got, plain):
        assert same_bits(a[keep], b[keep])


def test_idempotence(engine, oracle):
    for name in ("both", "stop"):
        batch, _ = R.case(oracle, name)
        out, first = dense_and_envelope(engine, batch)
        second = engine.speed_envelope(batch, out.cost, first[0])
        for a, b in zip(first, second):
            assert same_bits(a, b), name
        assert first[3].sum() > 0


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
    import torch

    batch, refs = R.case(oracle, "both")
    res = Resident(engine, batch)
    dev = res.db.dev
    n0 = engine.get_option("envelope_launches")
    res.pair(torch.cuda.current_stream(dev).cuda_stream)  # eager (also the warm-up of the capture)
    eager = res.fetch()
    assert engine.get_option("envelope_launches") == n0 + 1
    free = torch.cuda.mem_get_info()[0]
    res.pair(torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert torch.cuda.mem_get_info()[0] == free  # enqueue only: a second call allocates nothing
    side = torch.cuda.Stream(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        res.pair(side.cuda_stream)  # a linear chain on one stream: the envelope directly behind the dense call
    torch.cuda.synchronize(dev)
    assert engine.get_option("envelope_launches") == n0 + 3
    for step in range(2):
        res.flags.zero_(); res.bi.fill_(-9); res.bc.fill_(-9.0); res.nl.fill_(-9)
        graph.replay()
        replay = res.fetch()
        for a, b in zip(eager, replay):
            assert same_bits(a, b), step
    host = engine.plan_dense(batch, tables=True)
    check_against(refs, (host.cost, host.flags), replay, "replay")
    assert engine.get_option("envelope_launches") == n0 + 3  # a replay is not a call


# ---------------------------------------------------------------- off unless called
def test_a_ctx_that_never_asks_pays_nothing(oracle):
    batch, refs = R.case(oracle, "both")
    with FrenetEngine(0) as other:
        o = other.plan_dense(batch, tables=True)
        assert other.get_option("envelope_launches") == 0 and other.get_option("lattice_launches") == 1
        for b, r in enumerate(refs):  # the bits of the dense call alone: the oracle's tables
            assert np.array_equal(o.flags[b], r.flags_in) and o.best_idx[b] == r.best_in


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
    out = engine.plan_dense(batch, tables=True)
    p, fb = host_structs(batch)
    B = batch.B
    bi, bc, nl = np.empty(B, dtype=np.int32), np.empty(B), np.empty(B, dtype=np.int32)
    flags = out.flags.copy()
    lim = batch.speed_limit.copy()

    def call(prof, params=p, cost=out.cost, idx=bi, batch_struct=fb):
        return engine._lib.fp_speed_envelope(engine._ctx, C.byref(params), C.byref(batch_struct), C.byref(prof) if prof is not None else None,
                                             cost.ctypes.data if cost is not None else None, flags.ctypes.data, idx.ctypes.data if idx is not None else None,
                                             bc.ctypes.data, nl.ctypes.data, _abi.FP_MEM_HOST, None)

    good = lambda v=lim, front=2.0, tol=0.05, lat=0.1: _abi.FpSpeedProfile(v.ctypes.data if v is not None else None, front, tol, lat)  # noqa: E731
    n0 = engine.get_option("envelope_launches")
    for prof in (None, good(v=None), good(front=-1.0), good(front=float("nan")), good(front=float("inf")), good(tol=-1e-9), good(tol=float("inf")),
                 good(lat=-0.1), good(lat=float("nan")), good(lat=float("inf"))):
        assert call(prof) == -1
    assert call(good(), cost=None) == -1 and call(good(), idx=None) == -1
    nocoef = _abi.FpBatch.from_buffer_copy(fb)
    nocoef.coef = None
    assert call(good(), batch_struct=nocoef) == -1 and b"coef" in engine._lib.fp_last_error()
    assert call(good(lat=0.0), batch_struct=nocoef) == 0  # (coef is read only by the lateral check)
    flags[...] = out.flags
    for value in (np.nan, -0.5):
        bad = lim.copy()
        bad[1, 7] = value
        assert call(good(v=bad)) == -1 and b"frame 1, knot 7" in engine._lib.fp_last_error()
    big = _abi.FpParams.from_buffer_copy(p)
    big.nd, big.nv, big.nt = 129, 128, 1  # C = 16 512 > FP_MAX_CAND
    assert call(good(), params=big) == -4
    assert engine.get_option("envelope_launches") == n0 + 1 and np.array_equal(flags, out.flags)  # (a refused call launched and wrote nothing)
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
    res = Resident(engine, batch)
    res.pair()
    first = res.fetch()
    n0 = engine.get_option("envelope_launches")
    for kw in (dict(v_limit=0), dict(cost_tbl=0), dict(flag_tbl=0), dict(best_idx=0), dict(best_cost=0), dict(front=-1.0), dict(front=float("nan")),
               dict(tol=-1.0), dict(tol=float("inf")), dict(max_lat_accel=-1.0), dict(max_lat_accel=float("nan"))):
        with pytest.raises(_abi.FrenetGpuError) as err:
            res.envelope(**kw)
        assert err.value.code == -1, kw
    big = _abi.FpParams.from_buffer_copy(res.db.params)
    big.nd, big.nv, big.nt = 129, 128, 1
    prof = _abi.FpSpeedProfile(res.db.t["speed_limit"].data_ptr(), 1.0, 0.05, 0.0)
    rc = engine._lib.fp_speed_envelope(engine._ctx, C.byref(big), C.byref(res.fb), C.byref(prof), res.cost.data_ptr(), res.flags.data_ptr(), res.bi.data_ptr(),
                                       res.bc.data_ptr(), None, _abi.FP_MEM_DEVICE, None)
    assert rc == -4
    assert engine.get_option("envelope_launches") == n0
    res.envelope(n_limited=0)  # n_limited is optional
    again = res.fetch()
    for a, b in zip(first, again):
        assert same_bits(a, b)
    assert engine.get_option("envelope_launches") == n0 + 1
