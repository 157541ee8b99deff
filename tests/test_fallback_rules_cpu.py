"""CPU: what makes the GPU suite of fp_fallback_stop_rules (tests/test_gpu_fallback_rules.py) meaningful, shown without a device.  The
restatement (tests/fallback_rules_ref.py) leaves out at most MAX_LEFT_OUT egos of every fixture; every fixture reaches the path it is named
after; the analytic fixture's hand-computed answers hold; the closed-loop scenario has the two facts the GPU test relies on; FallbackStop
validates obey without a device and obey=() builds exactly the calls of today; the header declares the call the binding mirrors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fallback_cases as FC
import fallback_ref as FR
import fallback_rules_cases as RC
import fallback_rules_ref as FRR
import gates_ref as GR
import rules_eval_ref as RR
from conftest import ROOT
from fiss_plus_planner_amd import _abi, rules
from fiss_plus_planner_amd.fallback import FallbackStop


@pytest.mark.parametrize("name", sorted(RC.FIXTURES))
def test_reference_stays_within_the_cap(oracle, name):
    c, r = RC.case(name), RC.reference(oracle, name)
    left_out = int((r.need & ~r.counted).sum())
    print(f"{name}: {int(r.need.sum())} egos need a fallback, {left_out} left out, smallest slack {r.slack[r.need].min():.3e}, smallest rule slack "
          f"{r.rule_slack.min():.3e}, status {r.status.tolist()}, rule_bits {r.rule_bits.tolist()}")
    assert left_out <= FRR.MAX_LEFT_OUT
    assert r.need.sum() - left_out >= 1
    assert r.cand_rules.shape == r.cand.shape == (c.batch.B, len(np.atleast_1d(c.d_targets)) * len(c.stop_T))
    # verdicts exist only for admissible, clear candidates; the unchanged parts are the rule-blind call's
    bl = RC.blind(oracle, name)
    assert (r.cand_rules[r.cand != -1] == 0).all() and np.array_equal(r.cand, bl.cand) and np.array_equal(r.need, bl.need)
    assert np.array_equal(r.rule_counts, (r.rule_bits[:, None] >> np.arange(5)[None, :]) & 1)


def test_no_ego_is_left_out_at_all(oracle):
    """The aim, as test_fallback_cpu.py achieves it for the rule-blind fixtures: zero."""
    assert sum(int((RC.reference(oracle, n).need & ~RC.reference(oracle, n).counted).sum()) for n in RC.FIXTURES) == 0


def test_analytic_fixture_by_hand(oracle):
    c, r, bl = RC.case("analytic"), RC.reference(oracle, "analytic"), RC.blind(oracle, "analytic")
    b, n_stop = c.batch, len(c.stop_T)
    front, line = b.gate_front, b.gate_s[0, 0]
    assert front == 0.5 * b.veh_l and abs(line - (b.ego[0, 0] + front) - 14.0) < 1e-12 and abs(line - (b.ego[1, 0] + front) - 5.0) < 1e-12
    travel = 0.5 * b.ego[0, 1] * c.stop_T
    assert travel.tolist() == [8.0, 12.0, 18.0, 24.0]
    prob = oracle.problems_from_batch(b, egos=[0])[0]
    for T, want in zip(c.stop_T, travel):  # a stop (d, 0, T) travels v0 T / 2 (the last series point is one tick before T)
        s = prob.eval_traj(0.0, 0.0, float(T), dump=True, stride=256).arrays[1]
        assert abs(np.nanmax(s) - b.ego[0, 0] - want) < 1e-2
    # the stopping distance at the gates' own max_decel: 8 m < 14 m (not waived), 8 m > 5 m (waived)
    assert b.ego[0, 1] ** 2 / (2 * b.gate_max_decel) == 8.0
    assert GR.waived_gates(b, 0)[0].tolist() == [False] and GR.waived_gates(b, 1)[0].tolist() == [True]
    # rule-blind: T = 6 for both, across the line for ego 0.  Obeying: T = 3 (2 m short of the line; T = 4.5 would end 4 m beyond it)
    assert (bl.fb_idx % n_stop).tolist() == [3, 3] and (bl.status == FR.CLEAR).all()
    assert r.fb_idx.tolist() == [1, 3] and r.rule_bits.tolist() == [0, 0] and (r.status == FR.CLEAR).all()
    assert r.end_state[0].tolist() == [0.0, 0.0, 3.0] and np.allclose((b.ego[0, 0] + front + 12.0, b.ego[0, 0] + front + 18.0), (line - 2.0, line + 4.0), rtol=0, atol=1e-12)
    assert r.cand_rules[0].reshape(3, n_stop).tolist() == [[0, 0, RC.RULE_GATE, RC.RULE_GATE]] * 3 and (r.cand_rules[1] == 0).all()
    assert np.array_equal(r.end_state[1], bl.end_state[1])  # the waived ego chooses as the rule-blind call does
    # the fallback's max_decel = 3 admits T = 4.5 and T = 6 only (peak deceleration 1.5 v0 / T): the hardest brake with FP_RULE_GATE
    assert (1.5 * b.ego[0, 1] / c.stop_T).round(3).tolist() == [6.0, 4.0, 2.667, 2.0]
    soft, soft_bl = RC.reference(oracle, "analytic soft"), RC.blind(oracle, "analytic soft")
    assert soft.cand[0].reshape(3, n_stop).tolist() == [[-2, -2, -1, -1]] * 3
    assert soft.fb_idx.tolist() == [2, 3] and soft.rule_bits.tolist() == [RC.RULE_GATE, 0] and soft.rule_counts[0].tolist() == [0, 0, 1, 0, 0]
    assert soft_bl.fb_idx.tolist() == [3, 3]


def test_each_rule_decides_its_fixture(oracle):
    for name, bit in (("corridor", RC.RULE_BOUNDARY), ("zero limit", RC.RULE_LIMIT), ("time gap", RC.RULE_GAP)):
        r, bl = RC.reference(oracle, name), RC.blind(oracle, name)
        assert (r.cand[0] == -1).all(), name  # every stop is admissible and clear: the rule alone decides
        assert r.cand_rules[0, bl.fb_idx[0]] == bit and r.fb_idx[0] != bl.fb_idx[0] and r.rule_bits[0] == 0, name
        assert set(r.cand_rules[0].tolist()) == {0, bit}, name
    r = RC.reference(oracle, "corridor")
    assert r.end_state[0, 0] == -0.6 and RC.blind(oracle, "corridor").end_state[0, 0] == 0.9  # the outer target is cut off
    r = RC.reference(oracle, "time gap")
    assert r.end_state[0, 2] == 4.5 and RC.blind(oracle, "time gap").end_state[0, 2] == 6.0


def test_contact_on_every_candidate_consults_no_rule(oracle):
    r, bl = RC.reference(oracle, "all contact"), RC.blind(oracle, "all contact")
    assert (r.cand[0] >= 0).all() and (r.cand_rules == 0).all() and r.status[0] == FR.CONTACT and r.rule_bits[0] == 0
    for k in ("fb_idx", "hit_step", "hit_obs", "end_state"):
        assert np.array_equal(getattr(r, k), getattr(bl, k)), k
    # ... although the first stop alone would cross the closed line 3 m ahead
    c = RC.case("all contact")
    assert abs(c.batch.gate_s[0, 0] - (c.batch.ego[0, 0] + c.batch.gate_front) - 3.0) < 1e-12


def test_carried_fixtures_reach_their_paths(oracle):
    seen = set()
    for name in FC.FIXTURES:
        c, r = RC.case(name), RC.reference(oracle, name)
        assert RR.carried(c.batch) == RC.ALL == r.obey
        seen |= {int(v) for v in r.cand_rules[r.cand == -1]}
        if name == "off LDS":  # the rules' tables only take from the budget: the rows stay in the scene table
            assert not FC.rows_in_lds(c.batch, FR.points_cap(c.batch, c.stop_T))[1]
    # clean and violating verdicts, single rules and several at once (the popcount key), every rule
    assert 0 in seen and any(FRR.popcount(v) >= 2 for v in seen)
    assert all(any(v & bit for v in seen) for bit in (RC.RULE_LIMIT, RC.RULE_LATERAL, RC.RULE_GATE, RC.RULE_BOUNDARY))
    base = RC.reference(oracle, "base")
    assert base.status.tolist() == RC.blind(oracle, "base").status.tolist() and (base.rule_bits[[2, 3, 4, 5]] == 0).all()  # CONTACT, NONE, NOT_NEEDED, skipped
    chosen_violating = [(n, b) for n in FC.FIXTURES for b in np.nonzero(RC.reference(oracle, n).rule_bits)[0]]
    chosen_clean = [(n, b) for n in FC.FIXTURES for b in np.nonzero((RC.reference(oracle, n).status == FR.CLEAR) & (RC.reference(oracle, n).rule_bits == 0))[0]]
    assert chosen_violating and chosen_clean


def test_fewest_rules_broken_decides(oracle):
    r, n_stop = RC.reference(oracle, "fewest rules"), len(RC.STOP_T)
    both = RC.RULE_GATE | RC.RULE_BOUNDARY
    assert (r.cand[0] == -1).all() and r.cand_rules[0].reshape(2, n_stop).tolist() == [[both] * n_stop, [RC.RULE_GATE] * n_stop]
    assert r.fb_idx[0] == n_stop and r.rule_bits[0] == RC.RULE_GATE and r.end_state[0].tolist() == [-0.6, 0.0, 2.0]  # one rule, then the hardest brake
    assert r.rule_counts[0].tolist() == [0, 0, 1, 0, 0]
    c = RC.case("fewest rules")
    assert abs(0.9 - c.batch.ego[0, 3]) < abs(-0.6 - c.batch.ego[0, 3])  # (the lateral key alone would take 0.9)


def test_loop_scenario_facts(oracle):
    """Rule-blind, the fallback rolls at least one front bumper over the line while the gate is closed; obeying the gates none does, no
    chosen stop violates, and every ego drives on to the end of the line after the gate opens.  No cycle is undecided."""
    batch, _ = RC.loop_scenario()
    front = batch.gate_front
    assert (batch.obs_pose[..., 3] == 0).all() and batch.gate_max_decel == 0.0
    blind, obey = RC.loop_reference(oracle, False), RC.loop_reference(oracle, True)
    assert blind.undecided == 0 and obey.undecided == 0
    assert (blind.crossed_closed > 0).any()
    assert (obey.crossed_closed == 0).all() and (obey.rule_counts == 0).all()
    assert np.nanmax(obey.states[RC.K_CLOSE:RC.K_OPEN, :, 0]) + front <= RC.LOOP_LINE  # (state k is the ego at step k; closed: K_CLOSE .. K_OPEN - 1)
    assert np.nanmax(blind.states[RC.K_CLOSE:RC.K_OPEN, :, 0]) + front > RC.LOOP_LINE
    assert (obey.done == 2).all() and (obey.cycles > RC.K_OPEN).all() and (obey.counts[:, FR.CLEAR] > 0).all() and (obey.counts[:, 2:] == 0).all()
    for b in range(batch.B):  # plan, brake on fallbacks while the gate is closed, plan again
        st = obey.status[:obey.cycles[b], b]
        fb = np.nonzero(st == FR.CLEAR)[0]
        assert (st[:fb[0]] == 0).all() and (st[fb[-1] + 1:] == 0).all() and fb[0] > 0 and fb[-1] < RC.K_OPEN and fb[-1] + 1 < len(st)


def test_fiss_loop_scenario_facts(oracle):
    """The same scenario under FISS+ with the gates enforced and the fallback that obeys them: every ego spends cycles on clean
    fallback stops while the gate is closed, none has its bumper beyond the closed line, all drive on to the end of the line.  What the
    reference cannot decide (near-tied costs of refined candidates) comes only after the gate has opened and the last fallback cycle."""
    batch, _ = RC.fiss_loop_scenario()
    r = RC.fiss_loop_reference(oracle)
    assert batch.samp_min is not None and (r.crossed_closed == 0).all() and (r.rule_counts == 0).all()
    assert np.nanmax(r.states[RC.K_CLOSE:RC.K_OPEN, :, 0]) + batch.gate_front <= RC.LOOP_LINE
    assert (r.done == 2).all() and (r.cycles > RC.K_OPEN).all() and (r.counts[:, FR.CLEAR] > 0).all() and (r.counts[:, 2:] == 0).all()
    for b in range(batch.B):
        fb = np.nonzero(r.status[:r.cycles[b], b] == FR.CLEAR)[0]
        assert fb[0] > 0 and fb[-1] < RC.K_OPEN
        assert r.first_undecided[b] > RC.K_OPEN and r.first_undecided[b] > fb[-1] + 1, (b, r.first_undecided[b])


def test_obey_validation_needs_no_device():
    with pytest.raises(ValueError, match="unknown rule 'lights'"):
        FallbackStop([1.0], obey=("gates", "lights"))
    assert FallbackStop([1.0]).obey == () and FallbackStop([1.0], obey=None).obey == () and FallbackStop([1.0], obey="gates").obey == ("gates",)
    assert FallbackStop([1.0], obey=("gaps", "envelope")).obey == ("envelope", "gaps")  # (the order the rules run in)
    fs = FallbackStop([1.0, 2.0], obey=("gates", "boundary"))
    plain = FC.case("base").batch
    with pytest.raises(ValueError, match="carries no data for the gates pass"):
        fs.rules_for(plain, "fallback_stop")
    assert fs.rules_for(RC.case("base").batch) == ("gates", "boundary")
    with pytest.raises(ValueError, match="boundary"):
        fs.rules_for(RC.case("analytic").batch)  # gates only
    # the struct of the family does not depend on obey
    a, b = FallbackStop([1.0, 2.5], max_decel=6.0), FallbackStop([1.0, 2.5], max_decel=6.0, obey=("gates",))
    sa, sb = (f.struct(plain, lambda name, arr: 0) for f in (a, b))
    assert bytes(sa) == bytes(sb)


class _Lib:
    """Stands in for the loaded library: records which entry points are called (no device, nothing computed)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, len(args)))
            return 0
        return fn


def _engine_without_device():
    from fiss_plus_planner_amd.engine import FrenetEngine

    eng = FrenetEngine.__new__(FrenetEngine)
    eng._lib, eng._ctx = _Lib(), None
    return eng


def test_obey_empty_builds_exactly_the_calls_of_today():
    eng = _engine_without_device()
    c = FC.case("base")
    eng.fallback_stop(c.batch, FallbackStop(c.stop_T, c.d_targets), best_idx=c.best_idx, skip=c.skip, cand=True)
    assert eng._lib.calls == [("fp_fallback_stop", 15)]
    out = eng.fallback_stop(c.batch, FallbackStop(c.stop_T, c.d_targets), best_idx=c.best_idx)
    assert not hasattr(out, "rule_bits") and not hasattr(out, "cand_rules")
    eng = _engine_without_device()
    rc = RC.case("base")
    out = eng.fallback_stop(rc.batch, FallbackStop(rc.stop_T, rc.d_targets, obey=("gates",)), best_idx=rc.best_idx, skip=rc.skip, cand=True)
    assert eng._lib.calls == [("fp_fallback_stop_rules", 19)]
    assert out.rule_bits.shape == (8,) and out.cand_rules.shape == (8, 12) and out.rule_counts.shape == (8, 5) and out.cand_rules.dtype == np.uint32
    eng = _engine_without_device()
    with pytest.raises(ValueError, match="carries no data for the gates pass"):
        eng.fallback_stop(c.batch, FallbackStop(c.stop_T, c.d_targets, obey=("gates",)), best_idx=c.best_idx)
    with pytest.raises(ValueError, match="rule_counts needs"):
        eng.fallback_stop(c.batch, FallbackStop(c.stop_T, c.d_targets), best_idx=c.best_idx, rule_counts=np.zeros((8, 5), dtype=np.int32))
    with pytest.raises(ValueError, match="rule_counts must be"):
        eng.fallback_stop(rc.batch, FallbackStop(rc.stop_T, rc.d_targets, obey=("gates",)), best_idx=rc.best_idx, rule_counts=np.zeros((8, 4), dtype=np.int32))
    assert eng._lib.calls == []


def test_header_declares_the_call_and_the_binding_mirrors_it():
    hdr = open(os.path.join(ROOT, "include", "frenet_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = re.search(r"\bint\s+fp_fallback_stop_rules\s*\(([^)]*)\)", code).group(1)
    args = [a.strip() for a in decl.split(",")]
    assert len(args) == 19 and "fp_rule_set" in args[4] and args[13] == "uint32_t* cand_rules" and args[14] == "uint32_t* rule_bits" and args[16] == "int32_t* rule_counts"
    assert "fp_fallback_stop_rules" in _abi.EXPORTED_SYMBOLS and "#define FP_ABI_VERSION 18" in hdr and _abi.FP_ABI_VERSION == 18
    lib = _abi.load()
    at = lib.fp_fallback_stop_rules.argtypes
    assert len(at) == 19 and at[3] is C.POINTER(_abi.FpFallback) and at[4] is C.POINTER(_abi.FpRuleSet)
    # fp_fallback_stop's own text no longer lists the stop line among what is not done: it points to the new call
    old = hdr[hdr.index("a stopping manoeuvre for the egos without a plan"):hdr.index("#define FP_MAX_FALLBACK")]
    assert "obeys no rule pass" not in old.split("Deliberately not done")[1] and "fp_fallback_stop_rules" in old
    assert tuple(rules.by_name) == RC.ALL
