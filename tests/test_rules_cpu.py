"""CPU: the table of rule passes (fiss_plus_planner_amd/rules.py) - names, order and ABI entry points, the has-data predicate of every
pass on batches that carry one rule each, and the struct builders: every pointer field the address of the right array, every scalar the
batch's, the same struct through a host-resolving and a fake address function but for the pointers.  No library, no GPU."""
import ctypes as C
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

import gaps_ref
import gates_ref
from fiss_plus_planner_amd import _abi, rules
from fiss_plus_planner_amd.device_batch import OBSTACLE_RULES, RULES

NAMES = ("envelope", "gates", "boundary", "gaps")


def one_rule_batches():
    plain = gates_ref.plain_batch()
    shape = plain.knots.shape
    return dict(gates=[gates_ref.CASES["base"]()], gaps=[gaps_ref.CASES["base"]()],
                envelope=[dataclasses.replace(plain, max_lat_accel=0.5), dataclasses.replace(plain, speed_limit=np.full(shape, 9.0))],
                boundary=[dataclasses.replace(plain, bound_left=np.full(shape, 2.0), bound_right=np.full(shape, -2.0))])


def full_batch():
    b = gates_ref.CASES["base"]()
    shape = b.knots.shape
    return dataclasses.replace(b, speed_limit=np.full(shape, 9.0), limit_front=1.25, limit_tol=0.05, max_lat_accel=0.5, bound_left=np.full(shape, 2.0),
                               bound_right=np.full(shape, -2.0), bound_margin=0.07, gap_follow=20, gap_lead=10, gap_first=2)


class Recorder:
    """addr(name) -> a distinct fake address per name; remembers what was asked for."""

    def __init__(self, base):
        self.base, self.asked = base, []

    def __call__(self, name):
        if name not in self.asked:
            self.asked.append(name)
        return self.base + 0x100 * self.asked.index(name)

    def of(self, name):
        return self.base + 0x100 * self.asked.index(name)


def fields(st):
    return {n: getattr(st, n) for n, _ in st._fields_}


def pointer_fields(st):
    return {n for n, t in st._fields_ if t is C.c_void_p}


def test_names_order_and_entry_points():
    assert tuple(r.name for r in rules.TABLE) == NAMES and tuple(rules.by_name) == NAMES
    assert [r.fn for r in rules.TABLE] == ["fp_speed_envelope", "fp_gate_mask", "fp_boundary_mask", "fp_gap_mask"]
    assert [r.count for r in rules.TABLE] == ["n_limited", "n_gated", "n_masked", "n_close"]
    assert RULES + OBSTACLE_RULES == NAMES
    assert all(rules.by_name[r.name] is r for r in rules.TABLE)
    import types

    assert {v.__name__ for v in vars(rules).values() if isinstance(v, types.ModuleType)} == {"numpy", "fiss_plus_planner_amd._abi"}  # (no torch, no engine)
    with pytest.raises(AttributeError):
        rules.TABLE[0].name = "other"  # (immutable records)


def test_carried_is_true_for_the_rule_the_batch_carries_and_no_other():
    assert not any(r.carried(gates_ref.plain_batch()) for r in rules.TABLE)
    assert not any(r.carried(SimpleNamespace()) for r in rules.TABLE)  # (an object without the fields: the tolerant form)
    for name, batches in one_rule_batches().items():
        for batch in batches:
            assert [r.name for r in rules.TABLE if r.carried(batch)] == [name], name
    assert all(r.carried(full_batch()) for r in rules.TABLE)
    for r in rules.TABLE:  # what the error of a missing rule names: fields of the batch
        assert r.needs and all(f in gates_ref.plain_batch().__dataclass_fields__ for f in r.needs + r.arrays)


def test_structs_hold_the_right_addresses_and_the_batch_scalars():
    b, addr = full_batch(), Recorder(0x10000)
    env = rules.by_name["envelope"].struct(b, addr)
    assert isinstance(env, _abi.FpSpeedProfile) and fields(env) == dict(v_limit=addr.of("speed_limit"), front=1.25, tol=0.05, max_lat_accel=0.5)
    g = rules.by_name["gates"].struct(b, addr)
    assert isinstance(g, _abi.FpGates)
    assert fields(g) == dict(gate_s=addr.of("gate_s"), closed=addr.of("gate_closed"), gate_stride=b.gate_s.shape[1], T_gate=b.gate_closed.shape[1],
                             front=b.gate_front, max_decel=b.gate_max_decel)
    cor = rules.by_name["boundary"].struct(b, addr)
    assert isinstance(cor, _abi.FpCorridor) and fields(cor) == dict(left=addr.of("bound_left"), right=addr.of("bound_right"), margin=0.07)
    gap = rules.by_name["gaps"].struct(b, addr)
    assert isinstance(gap, _abi.FpTimeGap) and fields(gap) == dict(lag_follow=20, lag_lead=10, first=2, reserved0=0)
    assert len({addr.of(n) for n in addr.asked}) == len(addr.asked) == 5
    for r in rules.TABLE:  # a pass asks for the arrays it lists, and for nothing else
        one = Recorder(0x20000)
        r.struct(b, one)
        assert tuple(one.asked) == r.arrays, r.name


def test_the_two_special_cases_exist_once():
    lat_only = dataclasses.replace(gates_ref.plain_batch(), max_lat_accel=0.5)
    addr = Recorder(0x30000)
    env = rules.by_name["envelope"].struct(lat_only, addr)  # no speed_limit on the batch: the pass asks for the default by the same name
    assert addr.asked == ["speed_limit"] and env.v_limit == addr.of("speed_limit") and env.max_lat_accel == 0.5
    default = rules.array(lat_only, "speed_limit")
    assert default.shape == (lat_only.F, lat_only.NX) and default.dtype == np.float64 and np.isposinf(default).all() and default.flags.c_contiguous
    b = full_batch()
    assert rules.array(b, "speed_limit") is b.speed_limit and rules.array(b, "bound_left") is b.bound_left and rules.array(b, "gate_s") is b.gate_s
    words = rules.array(b, "gate_closed")  # the uint32 words as their int32 bit patterns: the same memory
    assert words.dtype == np.int32 and np.shares_memory(words, b.gate_closed) and np.array_equal(words.view(np.uint32), b.gate_closed)
    assert words.__array_interface__["data"][0] == b.gate_closed.__array_interface__["data"][0]


def test_gaps_refuses_what_the_struct_cannot_hold():
    b, gaps = full_batch(), rules.by_name["gaps"]
    for bad in (dict(gap_follow=_abi.FP_MAX_POINTS + 1), dict(gap_lead=_abi.FP_MAX_POINTS + 1), dict(gap_first=0), dict(gap_first=2**31)):
        ns = SimpleNamespace(**dict(dict(gap_follow=b.gap_follow, gap_lead=b.gap_lead, gap_first=b.gap_first), **bad))  # (ProblemBatch itself refuses these)
        with pytest.raises(ValueError):
            gaps.struct(ns, Recorder(0))
    from fiss_plus_planner_amd import engine

    assert engine._time_gap is rules._time_gap


def test_host_and_device_addresses_give_the_same_struct_but_for_the_pointers():
    b = full_batch()
    held = []

    def host(name):  # what the engine's host path does: the address of the array itself
        held.append(rules.array(b, name))
        return held[-1].__array_interface__["data"][0]

    fake = Recorder(0x40000)
    for r in rules.TABLE:
        h, d = r.struct(b, host), r.struct(b, fake)
        assert type(h) is type(d)
        ptrs = pointer_fields(h)
        assert len(ptrs) == len(r.arrays), r.name
        fh, fd = fields(h), fields(d)
        assert {n for n in fh if fh[n] != fd[n]} == ptrs, r.name
    assert rules.by_name["boundary"].struct(b, host).left == b.bound_left.__array_interface__["data"][0]
    assert rules.by_name["gates"].struct(b, host).closed == b.gate_closed.__array_interface__["data"][0]
