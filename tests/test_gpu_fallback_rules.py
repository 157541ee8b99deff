"""GPU: fp_fallback_stop_rules (the stopping manoeuvre that obeys the road rules) against its restatement (tests/fallback_rules_ref.py)
on the fixtures of tests/fallback_rules_cases.py - every output exact on every counted ego, hit_speed within 1e-9
(tests/test_fallback_rules_cpu.py shows that the fixtures reach their paths and that no ego is left out); then the memory modes, the
launch order and a second call bit for bit, cand_rules against fp_eval_trajs + fp_rules_eval, the equivalence with fp_fallback_stop
under a rule set that cannot speak, the edge shapes and counters, every error, plan_dense / plan_fiss(fallback=), the closed-loop scenario
eagerly and from a graph, and the drop-in classes.

On the code before fp_fallback_stop_rules the analytic fixture fails (the symbol is missing; the rule-blind call picks T = 6) and so does
the loop scenario's "never over the closed line"."""
import ctypes as C
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

import fallback_cases as FC
import fallback_ref as FR
import fallback_rules_cases as RC
import fallback_rules_ref as FRR
import gates_ref as GR
from fiss_plus_planner_amd import _abi, rules, synth
from fiss_plus_planner_amd.engine import host_structs
from fiss_plus_planner_amd.fallback import FallbackStop

pytestmark = pytest.mark.gpu

SHARED = ("end_state", "status", "fb_idx", "hit_step", "hit_obs", "hit_speed", "cand", "counts")  # the outputs fp_fallback_stop has too
OUTS = SHARED + ("rule_bits", "cand_rules", "rule_counts")


def stop_of(c, obey=None):
    return FallbackStop(c.stop_T, c.d_targets, c.max_decel, obey=c.obey if obey is None else obey)


def host(engine, c, obey=None, **kw):
    """engine.fallback_stop (FP_MEM_HOST) on a fixture."""
    kw.setdefault("best_idx", c.best_idx)
    return engine.fallback_stop(c.batch, stop_of(c, obey), cand=True, skip=c.skip, **kw)


def device(engine, c, order=None, obey=None):
    """fp_fallback_stop_rules(FP_MEM_DEVICE) on a fixture: resident batch and arrays, one launch, read back.  order: fp_batch.launch_order."""
    import torch

    from fiss_plus_planner_amd.device_batch import DeviceBatch

    db = DeviceBatch(c.batch, order_hint=False)
    dev, B = db.dev, c.batch.B
    fs = stop_of(c, obey)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    held = {}

    def addr(name, a):
        held[name] = up(a)
        return held[name].data_ptr()

    st = fs.struct(c.batch, addr)
    rs, structs = rules.rule_set(c.batch, lambda k: db.t[k].data_ptr(), fs.rules_for(c.batch))
    F = st.n_d * st.n_stop
    p = _abi.FpParams.from_buffer_copy(db.params)
    pts = max(fs.points_max(c.batch.tick_t), int(p.points_max))
    p.points_max = min(pts, _abi.FP_MAX_POINTS) if pts > _abi.FP_FAST_POINTS else 0
    fb = _abi.FpBatch.from_buffer_copy(db.fb)
    if c.skip is not None:
        held["skip"] = up(c.skip)
        fb.skip = held["skip"].data_ptr()
    if order is not None:
        held["order"] = up(np.asarray(order, dtype=np.int32))
        fb.launch_order = held["order"].data_ptr()
    i32 = np.int32
    t = dict(end_state=up(np.full((B, 3), np.nan)), status=up(np.full(B, -7, dtype=i32)), fb_idx=up(np.full(B, -7, dtype=i32)), hit_step=up(np.full(B, -7, dtype=i32)),
             hit_obs=up(np.full(B, -7, dtype=i32)), hit_speed=up(np.full(B, -7.0)), cand=up(np.full((B, F), -3, dtype=i32)), counts=up(np.zeros((B, 4), dtype=i32)),
             rule_bits=up(np.full(B, -7, dtype=i32)), cand_rules=up(np.zeros((B, F), dtype=i32)), rule_counts=up(np.zeros((B, 5), dtype=i32)))
    bi = up(c.best_idx)
    engine.fallback_stop_rules_device(p, fb, st, rs, t["end_state"].data_ptr(), t["status"].data_ptr(), t["fb_idx"].data_ptr(), t["hit_step"].data_ptr(),
                                      t["hit_obs"].data_ptr(), t["hit_speed"].data_ptr(), t["rule_bits"].data_ptr(), best_idx=bi.data_ptr(), cand=t["cand"].data_ptr(),
                                      cand_rules=t["cand_rules"].data_ptr(), counts=t["counts"].data_ptr(), rule_counts=t["rule_counts"].data_ptr(),
                                      stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    out = SimpleNamespace(**{k: v.cpu().numpy() for k, v in t.items()})
    out.rule_bits, out.cand_rules = out.rule_bits.view(np.uint32), out.cand_rules.view(np.uint32)
    return out


def same_bits(a, b, what, keys=OUTS):
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


def assert_matches(got, ref, what):
    """Every output exact on the counted egos (hit_speed within SPEED_TOL); the egos that need none are always compared."""
    ok = ref.counted
    assert (ref.need & ~ok).sum() <= FRR.MAX_LEFT_OUT, what
    print(f"{what}: status {got.status.tolist()} fb_idx {got.fb_idx.tolist()} hit_step {got.hit_step.tolist()} rule_bits {got.rule_bits.tolist()}, "
          f"{int((ref.need & ok).sum())} of {int(ref.need.sum())} fallback egos compared")
    for k in ("status", "fb_idx", "hit_step", "hit_obs", "cand", "counts", "rule_bits", "cand_rules", "rule_counts"):
        assert np.array_equal(getattr(got, k)[ok], getattr(ref, k)[ok]), (what, k, getattr(got, k)[ok].tolist(), getattr(ref, k)[ok].tolist())
    assert np.array_equal(got.end_state[ok], ref.end_state[ok], equal_nan=True), (what, got.end_state, ref.end_state)
    assert np.array_equal(np.isnan(got.hit_speed[ok]), np.isnan(ref.hit_speed[ok])), what
    hit = ok & ~np.isnan(ref.hit_speed)
    err = np.abs(got.hit_speed[hit] - ref.hit_speed[hit])
    print(f"{what}: max |hit_speed - ref| = {err.max() if err.size else 0.0:.3e}")
    assert (err <= FR.SPEED_TOL).all(), (what, err)


@pytest.mark.parametrize("name", sorted(RC.FIXTURES))
def test_fixtures_against_the_reference(engine, oracle, name):
    c, ref = RC.case(name), RC.reference(oracle, name)
    got = host(engine, c)
    assert_matches(got, ref, name)
    assert (got.cand[~ref.need] == -3).all() and (got.cand_rules[~ref.need] == 0).all() and (got.rule_bits[~ref.need] == 0).all()


def test_analytic_fixture_obeys_the_gate(engine, oracle):
    """The hand-computed answers on the device: rule-blind T = 6 across the line, obeying T = 3 and clean; T = 4.5 with FP_RULE_GATE when
    the harder stops are inadmissible; the waived ego chooses as the rule-blind call does."""
    assert hasattr(engine._lib, "fp_fallback_stop_rules")
    c = RC.case("analytic")
    blind, obey = host(engine, c, obey=()), host(engine, c)
    assert blind.end_state[:, 2].tolist() == [6.0, 6.0] and not hasattr(blind, "rule_bits")
    assert obey.end_state[0].tolist() == [0.0, 0.0, 3.0] and obey.rule_bits.tolist() == [0, 0] and obey.status.tolist() == [1, 1]
    assert obey.end_state[1].tobytes() == blind.end_state[1].tobytes()
    soft = host(engine, RC.case("analytic soft"))
    assert soft.end_state[:, 2].tolist() == [4.5, 6.0] and soft.rule_bits.tolist() == [_abi.RULE_GATE, 0] and soft.rule_counts[0].tolist() == [0, 0, 1, 0, 0]


@pytest.mark.parametrize("name", ["base", "many poses", "off LDS", "rings", "analytic", "time gap"])
def test_memory_modes_launch_order_and_a_second_call_give_the_same_bits(engine, name):
    c = RC.case(name)
    h = host(engine, c)
    d = device(engine, c)
    same_bits(h, d, f"{name}: host / device")
    same_bits(d, device(engine, c, order=np.arange(c.batch.B)[::-1]), f"{name}: reversed launch order")
    same_bits(d, device(engine, c), f"{name}: second call")


def family(c):
    """[B, F, 3]: the end states of the fixture's family, as the header defines them."""
    b = c.batch
    d = np.where(np.isnan(c.d_targets)[None, :], b.ego[:, 3:4], np.asarray(c.d_targets)[None, :])  # [B, n_d]
    es = np.zeros((b.B, len(c.d_targets), len(c.stop_T), 3))
    es[..., 0] = d[:, :, None]
    es[..., 2] = np.asarray(c.stop_T)[None, None, :]
    return es.reshape(b.B, -1, 3)


@pytest.mark.parametrize("name", ["base", "rings", "ties", "fewest rules", "time gap", "zero limit"])
def test_cand_rules_against_the_public_calls(engine, name):
    """fp_eval_trajs on the family, the FP_FLAG_INFEASIBLE bits cleared, fp_rules_eval(rule_bits=): equal to cand_rules on every admissible,
    clear candidate; cand_rules is 0 on every other candidate."""
    c = RC.case(name)
    got = host(engine, c)
    es = family(c)
    words = engine.eval_trajs(c.batch, es).flags & np.uint32(~_abi.FLAG_INFEASIBLE & 0xFFFFFFFF)
    ev = engine.rules_eval(c.batch, es, flags=words, rules=c.obey, skip=c.skip)
    clear = got.cand == -1
    assert clear.any() and np.array_equal(got.cand_rules[clear], ev.rule_bits[clear]), name
    assert (got.cand_rules[~clear] == 0).all()
    assert (got.cand_rules != 0).any()


def silenced(c):
    """The fixture with a rule set that cannot speak (RC.silent) and obey = its three table rules."""
    return SimpleNamespace(**{**vars(c), "batch": RC.silent(c.batch), "obey": ("envelope", "gates", "boundary")})


@pytest.mark.parametrize("name", sorted(FC.FIXTURES))
def test_a_silent_rule_set_gives_the_rule_blind_call_bit_for_bit(engine, name):
    c = FC.case(name)
    c = SimpleNamespace(**vars(c), obey=())
    plain = host(engine, c)
    s = silenced(c)
    got = host(engine, s)
    same_bits(plain, got, f"{name}: silent set", SHARED)
    assert (got.rule_bits == 0).all() and (got.cand_rules == 0).all() and (got.rule_counts == 0).all()
    same_bits(got, device(engine, s), f"{name}: silent set, device")
    if name == "no obstacles":  # lags with no obstacle near: all four rules
        s.batch = dataclasses.replace(s.batch, gap_follow=20, gap_lead=10, gap_first=1)
        s.obey = RC.ALL
        same_bits(plain, host(engine, s), f"{name}: silent set with lags", SHARED)


def test_largest_family(engine, oracle):
    """F = FP_MAX_FALLBACK = 64 lateral targets x 4 stop times against the reference (F = 1: the "no obstacles" fixture); one more is FP_ELIMIT."""
    b = RC.case("ties").batch
    c = SimpleNamespace(batch=b, stop_T=FC.STOP_T, d_targets=np.linspace(-0.8, 0.8, 64), max_decel=np.inf, best_idx=np.full(b.B, -1, dtype=np.int32), skip=None,
                        obey=RC.ALL)
    ref = FRR.fallback_rules(oracle, b, c.stop_T, c.d_targets, c.max_decel, c.obey, best_idx=c.best_idx)
    got = host(engine, c)
    assert got.cand_rules.shape == (b.B, _abi.FP_MAX_FALLBACK) and RC.case("no obstacles").d_targets.size * RC.case("no obstacles").stop_T.size == 1
    assert_matches(got, ref, "F = 256")
    same_bits(got, device(engine, c), "F = 256: host / device")
    assert raw(engine, b, n_d=257, n_stop=1)[0] == -4


def test_egos_that_need_none(engine):
    """Every ego has a plan: the early return - rule_bits 0, cand and cand_rules keep their sentinels, end_state is the decoded sample."""
    b = RC.with_rules(synth.make_batch(8, 3, 3, 2, 10, 60, True, 7111))
    bi = np.full(8, 4, dtype=np.int32)
    c = SimpleNamespace(batch=b, stop_T=FC.STOP_T, d_targets=FC.D3, max_decel=np.inf, best_idx=bi, skip=None, obey=RC.ALL)
    plain = host(engine, c, obey=())
    for got in (host(engine, c), device(engine, c)):
        assert (got.status == 0).all() and (got.rule_bits == 0).all() and (got.cand == -3).all() and (got.cand_rules == 0).all() and (got.rule_counts == 0).all()
        assert np.array_equal(got.counts, np.tile([1, 0, 0, 0], (b.B, 1)))
        same_bits(plain, got, "no ego needs one", ("end_state", "status", "fb_idx", "hit_step", "hit_obs", "hit_speed"))


@pytest.mark.parametrize("obey", [("envelope",), ("gates",), ("boundary",), ("gaps",), ("gates", "gaps"), RC.ALL])
def test_each_rule_alone_and_all_together(engine, oracle, obey):
    c = RC.case("base")
    assert_matches(host(engine, c, obey=obey), RC.reference(oracle, "base", obey), f"base, obey={obey}")


def test_rule_counts_accumulate_over_two_calls(engine, oracle):
    c, ref = RC.case("analytic soft"), RC.reference(oracle, "analytic soft")
    one = host(engine, c)
    two = host(engine, c, counts=one.counts, rule_counts=one.rule_counts)
    assert ref.rule_counts.any() and np.array_equal(one.rule_counts, ref.rule_counts)
    assert np.array_equal(two.rule_counts, 2 * ref.rule_counts) and np.array_equal(two.counts, 2 * ref.counts)
    start = np.arange(10, dtype=np.int32).reshape(2, 5)
    assert np.array_equal(host(engine, c, rule_counts=start).rule_counts, start + ref.rule_counts)


def raw(engine, batch, n_d=1, n_stop=1, max_decel=np.inf, null=(), mem=_abi.FP_MEM_HOST, rule_set="gates", edit=None):
    """fp_fallback_stop_rules through ctypes with every argument in the caller's hands -> (rc, message).  rule_set: names, None (a NULL
    set) or () (a set whose members are all NULL); edit(structs) may spoil a rule's struct."""
    B = batch.B
    d, t = np.zeros(n_d), np.arange(1, n_stop + 1, dtype=np.float64)
    st = _abi.FpFallback(n_d, n_stop, None if "d_targets" in null else d.ctypes.data, None if "stop_T" in null else t.ctypes.data, max_decel)
    bi = np.full(B, -1, dtype=np.int32)
    a = dict(end_state=np.full((B, 3), np.nan), status=np.zeros(B, dtype=np.int32), fb_idx=np.zeros(B, dtype=np.int32), hit_step=np.zeros(B, dtype=np.int32),
             hit_obs=np.zeros(B, dtype=np.int32), hit_speed=np.zeros(B), rule_bits=np.zeros(B, dtype=np.uint32))
    ptr = lambda k: None if k in null else a[k].ctypes.data  # noqa: E731
    held = {}

    def addr(name):
        held[name] = np.ascontiguousarray(rules.array(batch, name))
        return held[name].ctypes.data

    rs, structs = (_abi.FpRuleSet(), {}) if not rule_set else rules.rule_set(batch, addr, rule_set)
    if edit:
        edit(structs)
    p, fb = host_structs(batch)
    rc = engine._lib.fp_fallback_stop_rules(engine._ctx, C.byref(p), C.byref(fb), C.byref(st), None if rule_set is None else C.byref(rs), bi.ctypes.data,
                                            ptr("end_state"), ptr("status"), ptr("fb_idx"), ptr("hit_step"), ptr("hit_obs"), ptr("hit_speed"), None, None,
                                            ptr("rule_bits"), None, None, mem, None)
    return rc, engine._lib.fp_last_error().decode(errors="replace")


def test_every_error_and_the_launch_counters(engine):
    b = RC.case("ties").batch
    before, before_plain = engine.get_option("fallback_rules_launches"), engine.get_option("fallback_launches")
    EINVAL, ELIMIT = -1, -4
    # fp_fallback_stop's own
    for k in ("d_targets", "stop_T", "end_state", "status", "fb_idx", "hit_step", "hit_obs", "hit_speed"):
        assert raw(engine, b, null=(k,))[0] == EINVAL, k
    assert raw(engine, b, n_d=0)[0] == EINVAL and raw(engine, b, n_d=16, n_stop=17)[0] == ELIMIT
    for md in (0.0, -1.0, np.nan):
        assert raw(engine, b, max_decel=md)[0] == EINVAL, md
    # the rule set
    rc, msg = raw(engine, b, rule_set=None)
    assert rc == EINVAL and "rules" in msg
    rc, msg = raw(engine, b, rule_set=())
    assert rc == EINVAL and "every rule of the set is NULL" in msg
    rc, msg = raw(engine, b, null=("rule_bits",))
    assert rc == EINVAL and "rule_bits" in msg
    # every rule that is on raises its own pass' errors, with that pass' messages
    for names, spoil, want in ((("gates",), lambda s: setattr(s["gates"], "gate_stride", 33), "fp_gate_mask: gate_stride"),
                               (("gates",), lambda s: setattr(s["gates"], "T_gate", 0), "fp_gate_mask: T_gate"),
                               (("envelope",), lambda s: setattr(s["envelope"], "tol", -1.0), "fp_speed_envelope: tol"),
                               (("boundary",), lambda s: setattr(s["boundary"], "margin", np.nan), "fp_boundary_mask: margin"),
                               (("gaps",), lambda s: setattr(s["gaps"], "first", 0), "fp_gap_mask: first"),
                               (RC.ALL, lambda s: setattr(s["gaps"], "lag_follow", 257), "fp_gap_mask: lag_follow")):
        for mem in (_abi.FP_MEM_HOST, _abi.FP_MEM_DEVICE):
            rc, msg = raw(engine, b, rule_set=names, edit=spoil, mem=mem)
            assert rc == EINVAL and want in msg, (names, msg)
    bad = dataclasses.replace(b, bound_left=np.where(np.arange(b.NX)[None, :] == 3, np.nan, b.bound_left))
    rc, msg = raw(engine, bad, rule_set=("boundary",))
    assert rc == EINVAL and "corridor has a NaN" in msg
    assert engine.get_option("fallback_rules_launches") == before
    # one launch per call; fp_fallback_stop's counter does not move
    assert raw(engine, b)[0] == 0 and engine.get_option("fallback_rules_launches") == before + 1
    c = RC.case("ties")
    host(engine, c)
    device(engine, c)
    assert engine.get_option("fallback_rules_launches") == before + 3 and engine.get_option("fallback_launches") == before_plain
    host(engine, c, obey=())
    assert engine.get_option("fallback_rules_launches") == before + 3 and engine.get_option("fallback_launches") == before_plain + 1
    with pytest.raises(ValueError, match="carries no data for the gates pass"):
        engine.fallback_stop(FC.case("ties").batch, FallbackStop(FC.STOP_T, obey=("gates",)), best_idx=c.best_idx)


# ---------------------------------------------------------------------------
# plan_dense / plan_fiss (fallback=)
# ---------------------------------------------------------------------------
def _compare(got, ref):
    ok = ref.counted
    assert (ref.need & ~ok).sum() <= FRR.MAX_LEFT_OUT and ref.need.any()
    for k in ("status", "fb_idx", "hit_step", "hit_obs", "counts", "rule_bits"):
        assert np.array_equal(getattr(got, k)[ok], getattr(ref, k)[ok]), (k, getattr(got, k).tolist(), getattr(ref, k).tolist())
    assert np.array_equal(got.end_state[ok], ref.end_state[ok], equal_nan=True)


def test_plan_dense_fallback_obeys_the_gates(engine, oracle):
    """Gates 10 m ahead, closed for ever, in front of egos 0, 2 and 5: the egos among them whose every candidate is flagged have best_idx
    -1, and exactly they get a fallback - one that the gates rank; obey is independent of the passes the call switched on."""
    b = synth.make_batch(8, 3, 3, 2, 6, 60, True, 7112)
    closed = np.zeros((b.F, 4, 1), dtype=bool)
    closed[[0, 2, 5]] = True
    b = GR.with_gates(b, ahead=(10.0,), T_gate=4, closed=closed)
    fs = FallbackStop(FC.STOP_T, FC.D3, obey=("gates",))
    plain = engine.plan_dense(b, gates=True)
    out = engine.plan_dense(b, gates=True, fallback=fs)
    need = out.best_idx < 0
    assert np.array_equal(out.best_idx, plain.best_idx) and need.sum() >= 2 and not need[[1, 3, 4, 6, 7]].any() and (out.n_gated[need] > 0).all()
    ref = FRR.fallback_rules(oracle, b, FC.STOP_T, FC.D3, np.inf, ("gates",), best_idx=out.best_idx)
    _compare(out.fallback, ref)
    blind = engine.plan_dense(b, gates=True, fallback=FallbackStop(FC.STOP_T, FC.D3)).fallback
    assert not hasattr(blind, "rule_bits") and (blind.end_state[need, 2] != out.fallback.end_state[need, 2]).any()
    with pytest.raises(ValueError, match="boundary"):
        engine.plan_dense(b, gates=True, fallback=FallbackStop(FC.STOP_T, FC.D3, obey=("boundary",)))
    # obey does not depend on the passes the call switched on: without the gate pass everybody has a plan, and nobody needs the gates
    out2 = engine.plan_dense(b, fallback=fs)
    need2 = out2.best_idx < 0
    assert (out2.fallback.rule_bits[~need2] == 0).all() and np.array_equal(out2.fallback.status != 0, need2)


def test_plan_fiss_enforce_and_fallback(engine, oracle):
    """FISS+ obeying a gate 10 m ahead of ego 0 that is closed for ever: its end state is NaN, the fallback that obeys the gate fills it."""
    b = synth.make_batch(4, 5, 5, 5, 6, 110, True, 7113, kind="FISS+")
    closed = np.zeros((b.F, 4, 1), dtype=bool)
    closed[0] = True
    b = GR.with_gates(b, ahead=(10.0,), T_gate=4, closed=closed)
    fs = FallbackStop(FC.STOP_T, FC.D3, obey=("gates",))
    plain = engine.plan_fiss(b, "FISS+", enforce=("gates",))
    out = engine.plan_fiss(b, "FISS+", enforce=("gates",), fallback=fs)
    assert np.array_equal(out.end_state, plain.end_state, equal_nan=True) and np.isnan(out.end_state[0]).all()
    ref = FRR.fallback_rules(oracle, b, FC.STOP_T, FC.D3, np.inf, ("gates",), end_state=out.end_state)
    assert ref.counted[0]
    _compare(out.fallback, ref)
    keep = ~np.isnan(out.end_state[:, 0])
    assert out.fallback.end_state[keep].tobytes() == out.end_state[keep].tobytes() and (out.fallback.rule_bits[keep] == 0).all()


# ---------------------------------------------------------------------------
# the closed-loop scenario
# ---------------------------------------------------------------------------
def _runner(engine, fallback, planner="FOP", **kw):
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch

    batch, goal_xy = RC.loop_scenario()
    return batch, ClosedLoopRunner(engine, DeviceBatch(batch), goal_xy, planner, fallback=fallback, **kw)


def _closed_steps(rows):
    step = np.arange(len(rows)) + 1  # row r is the ego at step r + 1
    return (step >= RC.K_CLOSE) & (step < RC.K_OPEN)


def test_loop_scenario_never_over_the_closed_line(engine, oracle):
    ref = RC.loop_reference(oracle, True)
    batch, blind = _runner(engine, FallbackStop(RC.LOOP_STOP_T), rules=("gates",))
    out0 = blind.run(RC.LOOP_CYCLES, record=True)
    front = 0.5 * batch.veh_l
    over = [bool((out0.log.ego_rows(b)[_closed_steps(out0.log.ego_rows(b)), _abi.LOG_X] + front > RC.LOOP_LINE).any()) for b in range(batch.B)]
    assert any(over)  # the need: rule-blind, a front bumper is beyond the line while the gate is closed
    fs = FallbackStop(RC.LOOP_STOP_T, obey=("gates",))
    _, run = _runner(engine, fs, rules=("gates",))
    out = run.run(RC.LOOP_CYCLES, record=True)
    assert np.isin(out.done, (_abi.DONE_GOAL, _abi.DONE_END_OF_LINE)).all() and np.array_equal(out.done, ref.done) and np.array_equal(out.cycles, ref.cycles)
    assert np.array_equal(out.fallback_counts[:, 1:], ref.counts[:, 1:]) and out.fallback_rule_counts.shape == (batch.B, 5)
    assert np.array_equal(out.fallback_rule_counts, ref.rule_counts)
    worst = 0.0
    for b in range(batch.B):
        rows = out.log.ego_rows(b)
        assert len(rows) == ref.cycles[b]
        got = rows[:, [_abi.LOG_S, _abi.LOG_VELOCITY, _abi.LOG_S_DD, _abi.LOG_D, _abi.LOG_VELOCITY_Y, _abi.LOG_D_DD]]
        worst = max(worst, float(np.abs(got - ref.states[1:ref.cycles[b] + 1, b]).max()))
        closed = _closed_steps(rows)
        assert closed.any() and (rows[closed, _abi.LOG_X] + front <= RC.LOOP_LINE).all()  # never over the closed line
        assert rows[-1, _abi.LOG_X] > RC.LOOP_LINE  # ... and on after it opens
    print(f"loop: driven states within {worst:.3e} of the CPU reference loop, cycles {out.cycles.tolist()}, fallback counts {out.fallback_counts[:, 1:].tolist()}")
    assert worst <= 1e-8
    # the graph replays the same cycle: bit for bit
    _, g = _runner(engine, fs, rules=("gates",))
    outg = g.run_graph(RC.LOOP_CYCLES, record=True)
    for k in ("done", "cycles", "ego", "t_now", "cart"):
        assert getattr(outg, k).tobytes() == getattr(out, k).tobytes(), k
    assert np.array_equal(outg.fallback_counts[:, 1:], out.fallback_counts[:, 1:]) and np.array_equal(outg.fallback_rule_counts, out.fallback_rule_counts)
    for b in range(batch.B):
        assert outg.log.ego_rows(b).tobytes() == out.log.ego_rows(b).tobytes()


STATE_COLS = [_abi.LOG_S, _abi.LOG_VELOCITY, _abi.LOG_S_DD, _abi.LOG_D, _abi.LOG_VELOCITY_Y, _abi.LOG_D_DD]


def test_loop_fiss_plus_enforce_with_an_obeying_fallback(engine, oracle):
    """The scenario under FISS+ with enforce=("gates",) and the fallback that obeys them, eagerly and from a graph, against the CPU
    reference loop (fiss_rules_ref.plan, fallback_rules_ref, advance_ref): the driven states within 1e-8, the fallback's counts equal, every
    ego on fallback stops while the gate is closed and none beyond the line; then the runner's refusals.  The states are compared up to
    the first cycle the reference could not decide for the ego (near-tied costs of refined candidates: the loops may part there, as in
    tests/test_gpu_fiss_rules.py) - tests/test_fallback_rules_cpu.py shows that it lies behind the opening and the last fallback cycle."""
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch

    ref = RC.fiss_loop_reference(oracle)
    batch, goal = RC.fiss_loop_scenario()
    fs = FallbackStop(RC.LOOP_STOP_T, obey=("gates",))
    front = 0.5 * batch.veh_l
    fresh = lambda: DeviceBatch(RC.fiss_loop_scenario()[0])  # noqa: E731
    blind = ClosedLoopRunner(engine, fresh(), goal, "FISS+", enforce=("gates",), fallback=FallbackStop(RC.LOOP_STOP_T)).run(RC.LOOP_CYCLES, record=True)
    over = [bool((blind.log.ego_rows(b)[_closed_steps(blind.log.ego_rows(b)), _abi.LOG_X] + front > RC.LOOP_LINE).any()) for b in range(batch.B)]
    assert any(over)  # the need: with the rule-blind fallback a front bumper is beyond the line while the gate is closed
    out = ClosedLoopRunner(engine, fresh(), goal, "FISS+", enforce=("gates",), fallback=fs).run(RC.LOOP_CYCLES, record=True)
    assert np.isin(out.done, (_abi.DONE_GOAL, _abi.DONE_END_OF_LINE)).all() and np.array_equal(out.done, ref.done)
    assert (out.fallback_counts[:, 1] > 0).all() and np.array_equal(out.fallback_counts[:, 1:], ref.counts[:, 1:])
    assert np.array_equal(out.fallback_rule_counts, ref.rule_counts)
    worst = 0.0
    for b in range(batch.B):
        rows = out.log.ego_rows(b)
        n = min(int(ref.first_undecided[b]), int(ref.cycles[b]))  # rows 0 .. n - 1 are the cycles before the first undecided one
        assert n > RC.K_OPEN and len(rows) >= n
        if ref.first_undecided[b] > ref.cycles[b]:
            assert len(rows) == ref.cycles[b] == out.cycles[b]
        worst = max(worst, float(np.abs(rows[:n, STATE_COLS] - ref.states[1:n + 1, b]).max()))
        closed = _closed_steps(rows)
        assert closed.any() and (rows[closed, _abi.LOG_X] + front <= RC.LOOP_LINE).all()  # never over the closed line
        assert rows[-1, _abi.LOG_X] > RC.LOOP_LINE  # ... and on after it opens
    print(f"FISS+ loop: driven states within {worst:.3e} of the CPU reference loop up to cycles {np.minimum(ref.first_undecided, ref.cycles).tolist()}, "
          f"cycles {out.cycles.tolist()} (reference {ref.cycles.tolist()}), fallback counts {out.fallback_counts[:, 1:].tolist()}")
    assert worst <= 1e-8
    # the graph replays the same cycle: bit for bit
    outg = ClosedLoopRunner(engine, fresh(), goal, "FISS+", enforce=("gates",), fallback=fs).run_graph(RC.LOOP_CYCLES, record=True)
    for k in ("done", "cycles", "ego", "t_now", "cart"):
        assert getattr(outg, k).tobytes() == getattr(out, k).tobytes(), k
    assert np.array_equal(outg.fallback_counts[:, 1:], out.fallback_counts[:, 1:]) and np.array_equal(outg.fallback_rule_counts, out.fallback_rule_counts)
    for b in range(batch.B):
        assert outg.log.ego_rows(b).tobytes() == out.log.ego_rows(b).tobytes()
    with pytest.raises(ValueError, match="not done"):
        ClosedLoopRunner(engine, fresh(), goal, "FISS+", audit=("gates",), fallback=fs)
    with pytest.raises(ValueError, match="carries no data for the boundary pass"):
        ClosedLoopRunner(engine, fresh(), goal, "FISS+", fallback=FallbackStop(FC.STOP_T, obey=("boundary",)))


# ---------------------------------------------------------------------------
# the drop-in classes
# ---------------------------------------------------------------------------
def test_drop_in_class_obeys_the_gate(engine):
    """FrenetOptimalPlanner behind a gate 0.5 m in front of its bumper that is closed for ever: plan() finds nothing; the rule-blind
    fallback takes the gentlest stop, the obeying one the hardest brake - every stop crosses - and says so in fallback_info.rule_bits."""
    from test_gpu_planners import _inputs, _planner

    c = RC.case("analytic")
    b = c.batch
    pts, fs, obs = _inputs(b, 0)
    pl = _planner("FOP", b, engine)
    pl.generate_frenet_frame(pts)
    front = 0.5 * b.veh_l
    pl.set_gates([b.ego[0, 0] + front + 0.5], np.ones((4, 1), dtype=bool), front=front)
    assert pl.plan(fs, 8.0, obs, 0) is None
    got = {}
    for name, stop in (("blind", FallbackStop(c.stop_T, c.d_targets)), ("obey", FallbackStop(c.stop_T, c.d_targets, obey=("gates",)))):
        pl.set_fallback(stop)
        tr = pl.plan(fs, 8.0, obs, 0)
        assert tr is not None and tr.is_fallback
        got[name] = (tr.end_state.t, pl.fallback_info.rule_bits, pl.fallback_info.status)
    assert got["blind"] == (6.0, 0, _abi.FALLBACK_CLEAR) and got["obey"] == (2.0, _abi.RULE_GATE, _abi.FALLBACK_CLEAR)


@pytest.mark.parametrize("kind", ["FOP+", "FISS", "FISS+"])
def test_drop_in_classes_that_carry_no_rule_data(engine, kind):
    """FOP+, FISS and FISS+ take the object too, but none of them can be given rule data (set_gates, set_road_boundary, set_speed_profile
    and set_time_gap are FrenetOptimalPlanner's alone): when plan() needs the fallback, an obeyed rule is refused at that call through
    rules.missing, and obey=() plans the rule-blind stop with fallback_info.rule_bits 0."""
    from test_gpu_planners import _inputs, _planner

    b = synth.make_batch(2, 5, 5, 5, 6, 110, True, 7113, kind="FISS+" if kind.startswith("FISS") else "FOP")
    b.ego[0] = (30.0, 9.0, 0.0, 0.1, 0.0, 0.0)
    b.obs_pose[0, :, :, 3] = 0.0
    FC.place(b, 0, 0, 30.0 + 12.0 + 0.5 * b.veh_l + 1.0, 0.0, 2.0, 9.0)
    pts, fs, obs = _inputs(b, 0)
    pl = _planner(kind, b, engine)
    pl.generate_frenet_frame(pts)
    with pytest.raises(ValueError, match="FrenetOptimalPlanner only"):
        pl.set_gates([50.0], np.ones((4, 1), dtype=bool))
    assert pl.plan(fs, float(b.target_speed[0]), obs, 0) is None
    pl.set_fallback(FallbackStop(FC.STOP_T, FC.D3, obey=("gates",)))
    with pytest.raises(ValueError, match="carries no data for the gates pass"):
        pl.plan(fs, float(b.target_speed[0]), obs, 0)
    pl.set_fallback(FallbackStop(FC.STOP_T, FC.D3, obey=None))
    tr = pl.plan(fs, float(b.target_speed[0]), obs, 0)
    assert tr is not None and tr.is_fallback and pl.fallback_info.rule_bits == 0 and pl.fallback_info.status == _abi.FALLBACK_CLEAR
