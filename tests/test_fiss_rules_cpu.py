"""fp_plan_fiss_rules without a GPU: the reference (tests/fiss_rules_ref.py) against the oracle's own FISS / FISS+ planners under a rule
set that cannot speak, its caps on every case the GPU test compares with it, the paths those cases exist for, the argument errors of the Python layers (raised before any device is touched), the binding of
the new entry point and the rule set it takes."""
import ctypes as C
import dataclasses
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import fiss_rules_ref as FR
import gaps_ref as PR
import gates_ref as GR
import rules_eval_ref as R
from fiss_plus_planner_amd import _abi, rules
from fiss_plus_planner_amd.engine import FrenetEngine
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", ["FISS", "FISS+"])
@pytest.mark.parametrize("name", ["silent", "silent_long"])
def test_reference_with_a_silent_rule_set_is_the_oracles_planner(name, kind):
    """Indices, Stats and `refined` exactly; the refined end state within the project's 1e-9 (the oracle takes its gradient step in C, the
    reference through search.refine_step); the cost of an unrefined plan exactly."""
    batch = FR.case(name)
    refs = FR.batch_plan(O, batch, kind, FR.NAMES, key=name)
    found = 0
    for r, p in zip(refs, O.problems_from_batch(batch)):
        w = p.fiss_plan(None) if kind == "FISS" else p.fissplus_plan(None)
        assert np.array_equal(r.stats, w.stats) and r.rejected == 0
        if np.isnan(w.best_cost):
            assert (r.best_ijk == -1).all() and np.isnan(r.best_cost)
            continue
        found += 1
        assert np.array_equal(r.best_ijk, w.best_ijk) and np.array_equal(r.prev_best_idx, w.prev_best_idx)
        if kind == "FISS+":
            assert r.refined == w.refined and np.abs(r.end_state - w.end_state).max() <= 1e-9 and abs(r.best_cost - w.best_cost) <= 1e-9 * abs(w.best_cost)
        else:
            assert r.best_cost == w.best_cost
    assert found > 0


def case_refs(name, names, kind):
    return FR.batch_plan(O, FR.case(name), kind, names, key=name)


@pytest.mark.parametrize("name,names,kind", FR.CASES, ids=[f"{n}-{'+'.join(r)}-{k}" for n, r, k in FR.CASES])
def test_every_case_stays_within_the_cap(name, names, kind):
    refs = case_refs(name, names, kind)
    FR.check_caps(refs, name)
    assert any(r.best_ijk[0] >= 0 for r in refs)  # somebody plans


def test_cases_reach_the_paths_they_exist_for():
    """Proven on the reference alone (undecided egos do not count)."""
    ok = lambda refs: [r for r in refs if not r.undecided]  # noqa: E731
    full = ok(case_refs("small", FR.NAMES, "FISS+"))
    # the unenforced coarse winner carries a rule bit (the enforced walk did not take it) and the enforced one is another sample
    assert any(r.best_ijk[0] >= 0 and r.coarse_ijk_free[0] >= 0 and (r.best_ijk != r.coarse_ijk_free).any() for r in full)
    assert any(r.best_ijk[0] < 0 and r.stats.tolist()[:3] == [126, 125, 125] for r in full)  # no rule-clean sample: the closed-form Stats
    assert any(r.popped_boundary_only for r in full)  # a sample whose only bit is 128, popped before the winner
    later = ok(case_refs("small", ("gates", "boundary"), "FISS+"))
    assert any(r.rejected > 0 and r.refined for r in later)  # a rule rejects refined candidates, a later one wins
    back = ok(case_refs("small", ("envelope",), "FISS+"))
    assert any(r.rejected > 0 and not r.refined and r.best_ijk[0] >= 0 for r in back)  # ... or none does: the coarse winner stands
    assert any(r.rejected > 0 for r in ok(case_refs("long", ("envelope",), "FISS+")))  # the four-points-per-lane instance rejects too
    assert any(r.best_ijk[0] >= 0 for r in ok(case_refs("wide", ("gates", "boundary"), "FISS+")))


def test_the_loop_at_the_red_light_waits_and_drives_on():
    """The scenario of the GPU test on the reference alone: a plan in every cycle, the bumper crosses only into an open step, within 40
    cycles of the opening - for all four egos; the rules reject refined candidates on the way; no cycle is undecided."""
    batch, loops = FR.loop_case(O)
    for b, rows in enumerate(loops):
        assert len(rows) == GR.LOOP_CYCLES and not any(r.undecided for r in rows), b
        GR.check_loop_invariants(batch, b, np.array([r.t_now for r in rows]), np.where([r.planned for r in rows], 0, -1),
                                 np.array([r.q_before for r in rows]), np.array([r.q_after for r in rows]), GR.OPEN_STEPS[b])
    assert sum(r.rejected for rows in loops for r in rows) > 0


class NoEngine:
    """Stands where a FrenetEngine would: touching anything of it is a test failure."""

    def __getattr__(self, name):
        raise AssertionError(f"plan_fiss touched the engine ({name}) before it checked its arguments")


def test_plan_fiss_enforce_argument_errors_need_no_device():
    batch, plain = R.all_rules_batch(), PR.moving_batch()
    for b, names in ((batch, ("gate",)),                    # unknown rule
                     (plain, ("gates",)), (plain, "boundary"),  # rule without data
                     (dataclasses.replace(batch, gap_follow=0, gap_lead=0), ("gaps",))):
        with pytest.raises(ValueError):
            FrenetEngine.plan_fiss(NoEngine(), b, enforce=names)
    with pytest.raises(ValueError, match="enforce"):
        FrenetEngine.plan_fiss(NoEngine(), plain, rules=(), enforce=("envelope",))


def test_closed_loop_runner_enforce_argument_errors_need_no_device():
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner

    batch, plain = R.all_rules_batch(), PR.moving_batch()
    goal = np.zeros((batch.B, 2))
    for b, kw in ((batch, dict(enforce=("nope",), planner="FISS+")),                  # unknown rule
                  (plain, dict(enforce=("gates",), planner="FISS+")),                 # rule without data
                  (plain, dict(enforce="gaps", planner="FISS")),
                  (batch, dict(enforce=("gates",), planner="FOP")),                   # FOP enforces with rules=
                  (batch, dict(enforce=("gates",), rules=("gates",), planner="FOP")),  # the two do not combine
                  (batch, dict(enforce=("gates",), rules=("gates",), planner="FISS+"))):  # (rules= with FISS+ keeps raising)
        with pytest.raises(ValueError):
            ClosedLoopRunner(None, SimpleNamespace(host=b), goal, **kw)
    with pytest.raises(ValueError, match="rules="):  # the refusal points to the keyword that does enforce for FOP
        ClosedLoopRunner(None, SimpleNamespace(host=batch), goal, enforce=("gates",), planner="FOP")
    assert ClosedLoopRunner._check_enforce(("gaps", "envelope"), "FISS+", batch, ()) == ("envelope", "gaps")  # (the order the rules run in)
    assert ClosedLoopRunner._check_enforce((), "FOP", plain, ("gates",)) == ()


def test_binding_and_header_agree():
    lib = _abi.load()
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frenet_gpu.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+fp_plan_fiss_rules\s*\(([^)]*)\)", code).group(1)
    args = [a.strip() for a in decl.split(",")]
    assert len(args) == 10 and "fp_rule_set" in args[5] and "fp_loop_io" in args[6] and args[7] == "int32_t* rejected"
    assert "fp_plan_fiss_rules" in _abi.EXPORTED_SYMBOLS and lib.fp_abi_version() == 18  # one new symbol, the version stays
    at = lib.fp_plan_fiss_rules.argtypes
    assert len(at) == 10 and at[5] is C.POINTER(_abi.FpRuleSet) and at[6] is C.POINTER(_abi.FpLoopIo) and at[4] is C.POINTER(_abi.FpFissIo)


def test_rule_set_round_trip_for_the_new_binding():
    """The set a caller of plan_fiss_rules_device builds: the enforced rules only, pointing at the structs it is returned with."""
    batch = R.all_rules_batch()
    addr = {}

    def at(name):
        addr.setdefault(name, 0x1000 * (len(addr) + 1))
        return addr[name]

    names = rules.check_names(("boundary", "gates"), batch, "test")
    assert names == ("gates", "boundary")
    rs, structs = rules.rule_set(batch, at, names)
    assert tuple(structs) == names and not rs.envelope and not rs.gaps
    for n in names:
        assert C.addressof(getattr(rs, n).contents) == C.addressof(structs[n])
    g, c = structs["gates"], structs["boundary"]
    assert (g.gate_s, g.closed, g.gate_stride, g.T_gate) == (addr["gate_s"], addr["gate_closed"], 2, GR.T_GATE)
    assert (c.left, c.right, c.margin) == (addr["bound_left"], addr["bound_right"], batch.bound_margin)
    assert set(addr) == {"gate_s", "gate_closed", "bound_left", "bound_right"}  # no other rule's arrays are asked for
