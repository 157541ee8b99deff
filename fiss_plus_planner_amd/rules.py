"""The rule passes behind the dense pass, described once.

Every pass reads the dense call's [B][C] tables, ORs bits into flag_tbl, returns the argmin among what is left and writes a count per
ego (fp::TablePassArgs on the C side).  TABLE lists them in the order they run - every argmin honours the bits set before it, so the
order decides results - and carries what differs between them; FrenetEngine.plan_dense, DeviceBatch / ClosedLoopRunner and the planner
classes loop over it.  A new pass is one entry here and one public method pair on FrenetEngine.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import numpy as np

from . import _abi


class Rule(NamedTuple):
    name: str         # the plan_dense keyword and the ClosedLoopRunner(rules=...) word
    fn: str           # the ABI entry point
    count: str        # the per-ego count in plan_dense's result
    carried: Callable  # (batch) -> bool: the batch has the data the pass needs (fields a batch lacks altogether count as unset)
    needs: tuple      # the ProblemBatch fields named when it has not
    arrays: tuple     # the batch arrays the pass reads (array() below): DeviceBatch uploads these
    struct: Callable  # (batch, addr) -> the pass' ctypes struct; addr(name) = the address of array(batch, name) in the caller's memory space


def array(batch, name: str) -> np.ndarray:
    """A batch array as a pass reads it.  An envelope without speed_limit (a lateral bound alone) reads "no limit anywhere"; the uint32
    words of gate_closed travel as their int32 bit patterns (the same memory on the host)."""
    a = getattr(batch, name, None)
    if a is None and name == "speed_limit":
        return np.full((batch.F, batch.NX), np.inf)
    return a.view(np.int32) if name == "gate_closed" else a


def _has_speed_profile(batch) -> bool:
    return getattr(batch, "speed_limit", None) is not None or float(getattr(batch, "max_lat_accel", 0.0) or 0.0) > 0.0


def _has_time_gap(batch) -> bool:
    """A batch with both lags 0 carries no time gap."""
    return int(getattr(batch, "gap_follow", 0) or 0) > 0 or int(getattr(batch, "gap_lead", 0) or 0) > 0


def _time_gap(follow, lead, first, who: str) -> "_abi.FpTimeGap":
    """fp_time_gap of three Python ints; a value outside the struct's range raises here (a ctypes field would wrap it silently)."""
    follow, lead, first = int(follow), int(lead), int(first)
    if not (0 <= follow <= _abi.FP_MAX_POINTS and 0 <= lead <= _abi.FP_MAX_POINTS):
        raise ValueError(f"{who}: follow = {follow} / lead = {lead} outside 0 .. FP_MAX_POINTS ({_abi.FP_MAX_POINTS}) steps")
    if not 1 <= first <= 2**31 - 1:
        raise ValueError(f"{who}: first = {first} outside 1 .. INT32_MAX")
    return _abi.FpTimeGap(follow, lead, first, 0)


TABLE = (
    Rule("envelope", "fp_speed_envelope", "n_limited", _has_speed_profile, ("speed_limit", "max_lat_accel"), ("speed_limit",),
         lambda b, addr: _abi.FpSpeedProfile(addr("speed_limit"), float(b.limit_front), float(b.limit_tol), float(b.max_lat_accel))),
    Rule("gates", "fp_gate_mask", "n_gated", lambda b: getattr(b, "gate_s", None) is not None, ("gate_s", "gate_closed"), ("gate_s", "gate_closed"),
         lambda b, addr: _abi.FpGates(addr("gate_s"), addr("gate_closed"), int(b.gate_s.shape[1]), int(b.gate_closed.shape[1]), float(b.gate_front),
                                      float(b.gate_max_decel))),
    Rule("boundary", "fp_boundary_mask", "n_masked", lambda b: getattr(b, "bound_left", None) is not None, ("bound_left", "bound_right"),
         ("bound_left", "bound_right"), lambda b, addr: _abi.FpCorridor(addr("bound_left"), addr("bound_right"), float(b.bound_margin))),
    # (last: it does geometry against the obstacle table, and the cheaper passes leave it fewer survivors)
    Rule("gaps", "fp_gap_mask", "n_close", _has_time_gap, ("gap_follow", "gap_lead"), (),
         lambda b, addr: _time_gap(b.gap_follow, b.gap_lead, b.gap_first, "gaps")),
)
by_name = {r.name: r for r in TABLE}
# fp_rules_eval: the FP_RULE_* bits each rule can report for an explicit end state (rule_bits), and the fp_rule_set field it fills
BITS = {"envelope": _abi.RULE_LIMIT | _abi.RULE_LATERAL, "gates": _abi.RULE_GATE, "boundary": _abi.RULE_BOUNDARY, "gaps": _abi.RULE_GAP}
assert tuple(BITS) == tuple(by_name) == tuple(n for n, _ in _abi.FpRuleSet._fields_)


def carried_names(batch) -> tuple:
    """The rules the batch carries data for, in the order they run."""
    return tuple(r.name for r in TABLE if r.carried(batch))


def check_names(names, batch, who: str) -> tuple:
    """`names` (a rule name or an iterable of them) in the order the rules run; ValueError for an unknown name or a rule the batch
    carries no data for."""
    asked = (names,) if isinstance(names, str) else tuple(names)
    for n in asked:
        if n not in by_name:
            raise ValueError(f"{who}: unknown rule {n!r} (rules are a subset of {tuple(by_name)})")
    for n in asked:
        if not by_name[n].carried(batch):
            raise missing(by_name[n], f"{who}, rule {n!r}")
    return tuple(n for n in by_name if n in asked)


def rule_set(batch, addr, names=None):
    """The fp_rule_set of `names` (None: every rule the batch carries) from TABLE's struct builders -> (FpRuleSet, {name: struct}).  The
    set holds pointers into the structs: keep the dict alive as long as the set is used.  addr(name) = the address of array(batch, name)
    in the caller's memory space."""
    import ctypes as C

    names = carried_names(batch) if names is None else check_names(names, batch, "rule_set")
    structs = {n: by_name[n].struct(batch, addr) for n in names}
    rs = _abi.FpRuleSet()
    for n, st in structs.items():
        setattr(rs, n, C.pointer(st))
    return rs, structs


def missing(rule: Rule, who: str) -> ValueError:
    """The error of a caller that asks for a pass the batch carries no data for."""
    return ValueError(f"{who}: the batch carries no data for the {rule.name} pass (ProblemBatch.{' / '.join(rule.needs)})")
