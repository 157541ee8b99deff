"""fp_rules_eval without a GPU: the reference (tests/rules_eval_ref.py) against its four siblings on the lattice's own end states, its
caps on the off-lattice inputs of the GPU test, the argument errors of the Python layers (raised before any device is touched) and
rules.rule_set."""
import ctypes as C
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

import boundary_ref as BR
import envelope_ref as ER
import gaps_ref as PR
import gates_ref as GR
import rules_eval_ref as R
from fiss_plus_planner_amd import _abi, rules
from fiss_plus_planner_amd.engine import FrenetEngine
from oracle import oracle as O

# sibling module, its rule, what its per-ego reference calls the verdict(s), and the RULE_* bit of each
SIBLINGS = {
    "envelope": (ER, (("bit_a", R.RULE_LIMIT), ("bit_b", R.RULE_LATERAL))),
    "gates": (GR, (("gated", R.RULE_GATE),)),
    "boundary": (BR, (("bit", R.RULE_BOUNDARY),)),
    "gaps": (PR, (("close", R.RULE_GAP),)),
}
CASES = [(rule, name) for rule, (mod, _) in SIBLINGS.items() for name in mod.CASES]


@pytest.mark.parametrize("rule,name", CASES, ids=[f"{r}-{n}" for r, n in CASES])
def test_reference_equals_its_sibling_on_the_lattice(rule, name):
    """Both are oracle-based restatements of one definition: on the lattice's end states the bits are exactly the sibling's."""
    mod, verdicts = SIBLINGS[rule]
    batch, refs = mod.case(O, name)
    flags_in = np.stack([r.flags_in for r in refs])
    got = R.batch_rules(O, batch, R.lattice_end_states(batch), flags_in, names=(rule,))
    assert np.array_equal(got.flags_in, flags_in)
    assert np.array_equal(got.flags, np.stack([r.flags for r in refs]))
    want_bits = np.zeros(flags_in.shape, dtype=np.uint32)
    for field, bit in verdicts:
        want_bits |= np.where(np.stack([getattr(r, field) for r in refs]), bit, 0).astype(np.uint32)
    assert np.array_equal(got.rule_bits, want_bits)
    assert np.array_equal(got.undecided, np.stack([r.undecided for r in refs]))
    for i in range(5):
        assert np.array_equal(got.counts[:, i], ((want_bits >> i) & 1).sum(axis=1))


def test_off_lattice_inputs_stay_within_the_caps():
    """The caps are conditions on the inputs, checked here on the reference alone; the inputs do something: every rule speaks at least
    once, and the NaN / short / skipped trajectories are where the GPU test expects them."""
    batch = R.all_rules_batch()
    assert R.carried(batch) == R.RULE_NAMES == tuple(r.name for r in rules.TABLE if r.carried(batch))
    es, skip = R.off_lattice(batch), R.off_skip(batch)
    assert es.shape == (5, R.OFF_K, 3) and np.isnan(es[R.OFF_NAN]).any() and es[R.OFF_SHORT][2] < 2 * batch.tick_t
    keep = ~np.isnan(es).any(axis=2)
    keep[R.OFF_SHORT] = False  # (below samp_min's T on purpose)
    lo, hi = (np.broadcast_to(v[:, None, :], es.shape)[keep] for v in (batch.samp_min, batch.samp_max))
    assert (es[keep] >= lo).all() and (es[keep] <= hi).all()
    off_grid = np.abs(es[..., 2] / batch.tick_t - np.round(es[..., 2] / batch.tick_t))
    assert (off_grid[keep] > 1e-3).all()
    ref = R.batch_rules(O, batch, es, skip=skip)
    R.check_caps(ref, "off-lattice")
    assert ref.rule_bits[R.OFF_SKIP].sum() == 0 and ref.rule_bits[R.OFF_NAN] == 0 and ref.counts[R.OFF_SKIP].sum() == 0
    assert ref.flags_in[R.OFF_SHORT] >> 20 == 2  # two points: point 1 alone is checked
    seen = int(np.bitwise_or.reduce(ref.rule_bits.ravel()))
    assert seen & R.RULE_LIMIT and seen & R.RULE_GATE and seen & R.RULE_BOUNDARY, hex(seen)
    # the lattice end states of the same batch, all four rules at once (the GPU test's "all four" case)
    lat = R.batch_rules(O, batch, R.lattice_end_states(batch))
    R.check_caps(lat, "all four")
    assert int(np.bitwise_or.reduce(lat.rule_bits.ravel())) == 31  # every rule speaks, the gaps on what the others leave


class NoEngine:
    """Stands where a FrenetEngine would: an argument error must be raised before anything of it is touched."""


def test_rules_eval_argument_errors_need_no_device():
    batch, plain = R.all_rules_batch(), PR.moving_batch()
    es = R.off_lattice(batch)
    call = lambda *a, **kw: FrenetEngine.rules_eval(NoEngine(), *a, **kw)  # noqa: E731
    for b, a, kw in ((batch, (es[:, :, :2],), {}), (batch, (es[:3],), {}), (batch, (es[:, :0],), {}), (batch, (es,), dict(rules=("gate",))), (batch, (es,), dict(rules=())),
                     (plain, (es,), {}), (plain, (es,), dict(rules=("gaps",))), (batch, (es,), dict(flags=np.zeros((5, 3), dtype=np.uint32))),
                     (batch, (es,), dict(counts=np.zeros((5, 4), dtype=np.int32))), (dataclasses.replace(batch, gate_s=None, gate_closed=None), (es,), dict(rules="gates"))):
        with pytest.raises(ValueError):
            call(b, *a, **kw)
    with pytest.raises(ValueError, match="carries no data for the gaps pass"):
        call(plain, es, rules=("gaps",))


def test_plan_fiss_rules_argument_errors_need_no_device():
    batch, plain = R.all_rules_batch(), PR.moving_batch()
    for b, r in ((batch, ("gate",)), (plain, ("gates",)), (plain, "boundary"), (dataclasses.replace(batch, gap_follow=0, gap_lead=0), ("gaps",))):
        with pytest.raises(ValueError):
            FrenetEngine.plan_fiss(NoEngine(), b, rules=r)


def test_closed_loop_runner_audit_argument_errors_need_no_device():
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner

    batch, plain = R.all_rules_batch(), PR.moving_batch()
    goal = np.zeros((batch.B, 2))
    for b, kw in ((batch, dict(audit=("gates",))), (batch, dict(audit=("gates",), planner="FOP")), (batch, dict(audit=("gate",), planner="FISS+")),
                  (plain, dict(audit=("gates",), planner="FISS+")), (plain, dict(audit="gaps", planner="FISS")),
                  (dataclasses.replace(batch, bound_left=None, bound_right=None), dict(audit=("gates", "boundary"), planner="FISS+"))):
        with pytest.raises(ValueError):
            ClosedLoopRunner(None, SimpleNamespace(host=b), goal, **kw)
    assert ClosedLoopRunner._check_audit(("gaps", "envelope"), "FISS+", batch) == ("envelope", "gaps")  # (the order the rules run in)
    assert ClosedLoopRunner._check_audit((), "FOP", plain) == ()


def test_rule_set_builds_the_structs():
    batch = R.all_rules_batch()
    addr = {}

    def at(name):
        addr[name] = 0x1000 * (len(addr) + 1)
        return addr[name]

    rs, structs = rules.rule_set(batch, at)
    assert tuple(structs) == R.RULE_NAMES and tuple(rules.BITS) == R.RULE_NAMES
    assert [rules.BITS[n] for n in R.RULE_NAMES] == [R.RULE_LIMIT | R.RULE_LATERAL, R.RULE_GATE, R.RULE_BOUNDARY, R.RULE_GAP]
    assert (_abi.RULE_LIMIT, _abi.RULE_LATERAL, _abi.RULE_GATE, _abi.RULE_BOUNDARY, _abi.RULE_GAP, _abi.FP_RULE_COUNT) == (1, 2, 4, 8, 16, 5)
    for n in R.RULE_NAMES:  # the set points at the very structs it is returned with
        assert C.addressof(getattr(rs, n).contents) == C.addressof(structs[n])
    e, g, c, t = (structs[n] for n in R.RULE_NAMES)
    assert (e.v_limit, e.front, e.tol, e.max_lat_accel) == (addr["speed_limit"], batch.limit_front, batch.limit_tol, batch.max_lat_accel)
    assert (g.gate_s, g.closed, g.gate_stride, g.T_gate, g.front, g.max_decel) == (addr["gate_s"], addr["gate_closed"], 2, GR.T_GATE, batch.gate_front, 0.0)
    assert (c.left, c.right, c.margin) == (addr["bound_left"], addr["bound_right"], batch.bound_margin)
    assert (t.lag_follow, t.lag_lead, t.first) == (20, 10, 2)
    rs, structs = rules.rule_set(batch, at, ("gaps", "gates"))
    assert tuple(structs) == ("gates", "gaps") and not rs.envelope and not rs.boundary and rs.gates and rs.gaps
    with pytest.raises(ValueError):
        rules.rule_set(PR.moving_batch(), at, ("gates",))
    assert C.sizeof(_abi.FpRuleSet) == 4 * C.sizeof(C.c_void_p)
    assert "fp_rules_eval" in _abi.EXPORTED_SYMBOLS
