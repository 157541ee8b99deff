"""CPU: the gates (fp_gate_mask) without a GPU - the reference restatement (tests/gates_ref.py) on a case with a closed form, on every
batch the GPU tests use (caps on undecided candidates, shares, survivors, the per-profile observation the kernel rests on: all asserted
on the reference alone) and through the closed-loop scenario; gate_bits, ProblemBatch.take / shard / digest, the header against the
binding, and the argument checks that need no device."""
import ctypes as C
import dataclasses
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import gates_ref as R
from conftest import ROOT
from fiss_plus_planner_amd import _abi, synth
from fiss_plus_planner_amd.batch import ProblemBatch
from fiss_plus_planner_amd.spline import gate_bits


def straight_batch(gate_s, closed, t_now=0, front=2.25, max_decel=0.0, s0=10.0, v0=5.0):
    """One ego on a straight 200 m line at constant speed v0 (one speed sample = v0, s_dd = 0): s_i = s0 + v0 i / 10, the bumper at
    q_i = 12.25 + 0.5 i.  C = 4, c = i_d * 2 + i_T: T = 8 s drives to q_79 = 51.75, T = 10 s to q_99 = 61.75.  closed: [T_gate, G]."""
    pts = np.zeros((1, 41, 2))
    pts[0, :, 0] = np.linspace(0.0, 200.0, 41)
    knots, coef = synth.build_frames(pts)
    return ProblemBatch(d_samples=[0.0, 0.5], t_samples=[8.0, 10.0], v_samples=[[v0]], target_speed=[v0], ego=[[s0, v0, 0.0, 0.0, 0.0, 0.0]],
                        frame_of=[0], scene_of=[-1], t_now=[t_now], nx=[41], knots=knots, coef=coef, obs_pose=np.zeros((0, 1, 0, 4)), obs_dims=np.zeros((0, 0, 2)),
                        final_time_step=np.zeros(0, dtype=np.int32), veh_l=4.5, veh_w=1.8, max_speed=30.0, max_accel=10.0,
                        gate_s=np.atleast_2d(np.asarray(gate_s, dtype=np.float64)), gate_closed=gate_bits(np.asarray(closed)[None]), gate_front=front,
                        gate_max_decel=max_decel)


def only(T, *steps, G=1, g=0):
    c = np.zeros((T, G), dtype=bool)
    c[list(steps), g] = True
    return c


def test_reference_on_a_closed_form(oracle):
    """Constant speed 5 m/s: the bumper moves over a line at s = 40.1 between the points 55 (39.75) and 56 (40.25)."""
    verdict = lambda *a, **kw: R.ego_gates(oracle, straight_batch(*a, **kw), 0)  # noqa: E731
    r = verdict([40.1], only(128, 56))
    assert r.gated.all() and (r.step == 56).all() and r.n_gated == 4 and r.best_idx == -1 and np.allclose(r.slack, 0.15)
    assert np.array_equal(r.flags & ~np.uint32(R.FLAG_SPEED), r.flags_in) and not (r.flags_in & R.FLAG_SPEED).any()
    for step in (55, 57):  # the state of exactly the arrival step decides
        r = verdict([40.1], only(128, step))
        assert not r.gated.any() and r.best_idx == r.best_in >= 0 and np.array_equal(r.flags, r.flags_in)
    assert verdict([40.1], ~only(128, 56)).n_gated == 0
    # the ego's own clock
    assert verdict([40.1], only(128, 66), t_now=10).gated.all() and not verdict([40.1], only(128, 56), t_now=10).gated.any()
    # the two clamps of the time index: the last known state holds, and so does the first before step 0
    assert verdict([40.1], only(20, 19)).gated.all() and not verdict([40.1], ~only(20, 19)).gated.any()
    assert verdict([40.1], only(20, 0), t_now=-100).gated.all() and not verdict([40.1], ~only(20, 0), t_now=-100).gated.any()
    assert verdict([40.1], only(128, 1), t_now=-55).gated.all() and not verdict([40.1], only(128, 0), t_now=-55).gated.any()  # (arrival at step 1: no clamp)
    # a line at 55.1: only the T = 10 s profile gets there (point 86)
    r = verdict([55.1], np.ones((128, 1), dtype=bool))
    assert r.gated.tolist() == [False, True, False, True] and r.step.tolist() == [-1, 86, -1, 86]
    # the bumper exactly on the line crosses it with its first move; past the line it never does; a NaN slot is no gate
    r = verdict([12.25], only(128, 1))
    assert r.gated.all() and (r.step == 1).all()
    assert not verdict([12.25], ~only(128, 1)).gated.any()
    assert not verdict([12.0], np.ones((128, 1), dtype=bool)).gated.any()
    assert not verdict([np.nan, 40.1], np.ones((128, 2), dtype=bool) & np.array([True, False])).gated.any()
    assert verdict([np.nan, 40.1], np.ones((128, 2), dtype=bool) & np.array([False, True])).gated.all()
    # the waiver: 12.25 + 25 / (2 a) against 40.1, a micrometre either side
    closed = np.ones((128, 1), dtype=bool)
    for reach, want in ((40.1 + 1e-6, False), (40.1 - 1e-6, True)):
        r = verdict([40.1], closed, max_decel=12.5 / (reach - 12.25))
        assert r.gated.tolist() == [want] * 4 and r.waived.tolist() == [not want] and np.allclose(r.slack, 1e-6, rtol=1e-3)
    assert not verdict([40.1], closed, max_decel=0.3).gated.any() and verdict([40.1], closed, max_decel=0.3, v0=0.0).M.max() <= 100
    r = verdict([12.0], closed, max_decel=0.3)  # (past the line: nothing to waive, nothing to cross)
    assert not r.waived.any() and not r.gated.any()


@pytest.mark.parametrize("name", list(R.CASES))
def test_caps_hold_on_every_gpu_batch(oracle, name):
    """At most 0.5 % of a batch's candidates within 1e-9 of a line or of the waiver's threshold, at most one ego excluded for having one."""
    batch, refs = R.case(oracle, name)
    R.check_caps(refs, name)
    assert len(refs) == batch.B


@pytest.mark.parametrize("name", list(R.CASES))
def test_verdicts_are_shared_by_the_candidates_of_a_profile(oracle, name):
    """What the kernel rests on: the oracle's M and the reference's verdict (and its step) are equal across i_d within a profile."""
    batch, refs = R.case(oracle, name)
    P = batch.nv * batch.nt
    for r in refs:
        for arr in (r.M, r.N, r.gated, r.step):
            a = np.asarray(arr).reshape(batch.nd, P)
            assert (a == a[0]).all(), name


def test_gpu_batches_gate_some_and_not_all(oracle):
    """A batch where all or none violate tests nothing: 10 % .. 90 % on the base batches, at least three egos keep a survivor, at least two
    winners change; the waiver decides a different set."""
    for name in R.BASE_CASES + ("waiver",):
        batch, refs = R.case(oracle, name)
        assert 0.10 <= R.gated_share(refs) <= 0.90, (name, R.gated_share(refs))
        assert sum(r.best_idx >= 0 for r in refs) >= 3, name
        assert sum(r.best_idx != r.best_in for r in refs) >= 2, name
        c = (batch.gate_closed[:, :, None] >> np.arange(2, dtype=np.uint32)) & 1
        assert c.any(axis=1).all() and not c.all(axis=1).any()  # every line closes at some step and opens at another ...
        assert (c[:, :, 0] != c[:, :, 1]).any(axis=1).all() and len({tuple(w) for w in batch.gate_closed}) == batch.F  # ... out of step with its neighbour, and the frames differ
    _, base = R.case(oracle, "base")
    wb, waiver = R.case(oracle, "waiver")
    assert any(r.waived.any() for r in waiver) and not any(r.waived.any() for r in base) and wb.gate_max_decel == R.MAX_DECEL
    assert [r.gated.tolist() for r in waiver] != [r.gated.tolist() for r in base] and [r.best_idx for r in waiver] != [r.best_idx for r in base]
    # the shapes the cases exist for
    N = lambda refs: np.concatenate([r.N for r in refs])  # noqa: E731
    M = lambda refs: np.concatenate([r.M for r in refs])  # noqa: E731
    assert 64 < N(base).min() and N(base).max() <= 128                       # two lane rounds
    assert N(R.case(oracle, "tick005")[1]).max() == 200                      # four
    tb, _ = R.case(oracle, "t_now")
    assert (tb.t_now > 0).all() and len(set(tb.t_now.tolist())) == tb.B
    hb, hold = R.case(oracle, "hold_last")
    assert hb.gate_closed.shape[1] < N(hold).min() and [r.gated.tolist() for r in hold] != [r.gated.tolist() for r in base]
    zb, zero = R.case(oracle, "before_zero")
    assert (zb.t_now < 0).all() and (zb.t_now + 1 < 0).any() and [r.gated.tolist() for r in zero] != [r.gated.tolist() for r in base]
    ends = R.case(oracle, "line_ends")[1]
    assert ((M(ends) < N(ends)) & (M(ends) > 1)).any() and (ends[3].M <= 1).all() and not ends[3].gated.any()
    cb, chunks = R.case(oracle, "chunks")
    assert cb.B == 2 and cb.C == 567 and any(r.gated.any() for r in chunks) and any(r.best_idx >= 0 for r in chunks)
    sb, s32 = R.case(oracle, "stride32")
    assert sb.gate_s.shape == (5, _abi.FP_MAX_GATES) and not np.isnan(sb.gate_s).any() and any(r.best_idx >= 0 for r in s32) and 0 < R.gated_share(s32) < 1
    ob, opened = R.case(oracle, "open")
    assert not ob.gate_closed.any()
    for r in opened:
        assert not r.gated.any() and np.array_equal(r.flags, r.flags_in) and r.best_idx == r.best_in


OPEN_AT, LOOP_CYCLES, check_loop_invariants = R.OPEN_STEPS, R.LOOP_CYCLES, R.check_loop_invariants


def test_closed_loop_scenario_on_the_reference(oracle):
    batch, loops = R.loop_case(oracle, OPEN_AT, LOOP_CYCLES)
    arrivals = []
    for b, rows in enumerate(loops):
        assert len(rows) == LOOP_CYCLES and not any(r.undecided for r in rows)
        s_after = np.array([r.ego[0] for r in rows])
        s_before = np.concatenate(([batch.ego[b, 0]], s_after[:-1]))
        arrivals.append(check_loop_invariants(batch, b, [r.t_now for r in rows], [r.best_idx for r in rows], s_before + batch.gate_front,
                                              s_after + batch.gate_front, OPEN_AT[b]))
        assert [r.crossed for r in rows].count(True) == 1
    assert arrivals[0] == 80 and arrivals[2] == 120  # the first open step: the ego waited at the line
    held = [r.n_gated for r in loops[0] if r.n_gated]  # (in the last cycles before the opening every candidate arrives at an open step)
    assert 70 <= len(held) < 80 and min(held) == 6 and max(held) == 33 and not any(r.n_gated for r in loops[0][80:])
    assert 1.5 < min(r.ego[1] for r in loops[0]) < 2.5  # (it slows to about 1.8 m/s)
    # without the gates the lattice drives over the line while it is closed: the gate, not the lattice, holds the ego
    _, free = R.loop_case(oracle, OPEN_AT, 70, gates=False)
    for b in (0, 2, 3):
        cross = [r.t_now + 1 for r in free[b] if r.crossed]
        assert len(cross) == 1 and cross[0] < OPEN_AT[b], (b, cross)


def test_gate_bits():
    c = np.zeros((2, 3, 4), dtype=bool)
    c[0, 1, 0] = c[0, 1, 3] = c[1, 2, 2] = True
    out = gate_bits(c)
    assert out.dtype == np.uint32 and out.shape == (2, 3) and out.tolist() == [[0, 9, 0], [0, 0, 4]]
    assert gate_bits(c[0]).tolist() == [0, 9, 0]
    assert gate_bits(np.ones((1, 1, 32))).tolist() == [[0xFFFFFFFF]] and gate_bits(np.array([[[0, 2.5]]])).tolist() == [[2]]
    for bad in (np.ones((1, 1, 33)), np.ones(4), np.ones((1, 1, 0))):
        with pytest.raises(ValueError):
            gate_bits(bad)


def test_take_and_shard_keep_the_gates():
    b = R.CASES["waiver"]()
    sub = b.take([3, 1])
    assert np.array_equal(sub.gate_s[sub.frame_of], b.gate_s[[3, 1]]) and np.array_equal(sub.gate_closed[sub.frame_of], b.gate_closed[[3, 1]])
    assert sub.gate_closed.dtype == np.uint32 and (sub.gate_front, sub.gate_max_decel) == (b.gate_front, b.gate_max_decel) == (0.5 * b.veh_l, R.MAX_DECEL)
    sh = b.shard(1, 2)
    assert sh.B == 3 and np.array_equal(sh.gate_s[sh.frame_of], b.gate_s[2:5]) and np.array_equal(sh.gate_closed[sh.frame_of], b.gate_closed[2:5])
    plain = R.plain_batch()
    assert plain.take([0]).gate_s is None and plain.shard(0, 2).gate_closed is None and plain.take([0]).gate_max_decel == 0.0
    for bad in (dict(gate_s=np.ones((4, 2)), gate_closed=np.ones((5, 8))), dict(gate_s=np.ones((5, 33)), gate_closed=np.ones((5, 8))),
                dict(gate_s=np.ones((5, 2)), gate_closed=np.ones((5, 0))), dict(gate_s=np.ones((5, 2))), dict(gate_closed=np.ones((5, 8)))):
        with pytest.raises(AssertionError):
            dataclasses.replace(plain, **bad)


def test_a_batch_without_gates_keeps_its_digest():
    """Pinned on the commit before the gate fields existed (the same batch and digest as tests/test_envelope_cpu.py)."""
    plain = R.plain_batch()
    assert plain.gate_s is None and plain.gate_closed is None and (plain.gate_front, plain.gate_max_decel) == (0.0, 0.0)
    assert plain.digest() == "48c26a8ddc9898b2a4dcadda741a0e6d07287e10d0a8bb7f63f8f6bdefc926e1"
    g = R.with_gates(plain)
    digests = {plain.digest(), g.digest(), R.with_gates(plain, max_decel=1.0).digest(), R.with_gates(plain, front=0.0).digest(),
               R.with_gates(plain, T_gate=64).digest(), dataclasses.replace(g, gate_s=g.gate_s + 1.0).digest()}
    assert len(digests) == 6


def test_header_and_binding_agree(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "frenet_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+fp_gate_mask\s*\(", code) and "fp_gate_mask" in _abi.EXPORTED_SYMBOLS
    assert sorted(set(re.findall(r"\b(fp_\w+)\s*\(", code))) == sorted(_abi.EXPORTED_SYMBOLS)
    assert int(re.search(r"#define FP_MAX_GATES (\d+)", hdr).group(1)) == _abi.FP_MAX_GATES == 32
    assert int(re.search(r"#define FP_FLAG_SPEED (\d+)u", hdr).group(1)) == _abi.FLAG_SPEED == R.FLAG_SPEED and _abi.FLAG_INFEASIBLE == R.FLAG_INFEASIBLE
    assert float(re.search(r"#define FP_AUDIT_GAP_TOL (\S+)", hdr).group(1)) == R.UNDECIDED_TOL
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "frenet_gpu.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(fp_gates));']
    for fname, _ in _abi.FpGates._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(fp_gates, {fname}));')
    lines += ['  printf("version %d\\n", FP_ABI_VERSION);', '  return 0;', '}']
    src = tmp_path / "gates.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "gates"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_abi.FpGates) == 40
    for fname, _ in _abi.FpGates._fields_:
        assert int(got[fname]) == getattr(_abi.FpGates, fname).offset, fname
    assert int(got["version"]) == 18 == _abi.FP_ABI_VERSION


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "fiss_plus_planner_amd", "csrc"), "-s"])
    return _abi.load()


def test_library_exports_the_symbol_within_abi_18(lib):
    assert hasattr(lib, "fp_gate_mask") and lib.fp_abi_version() == 18
    assert lib.fp_gate_mask.argtypes is not None and len(lib.fp_gate_mask.argtypes) == 11


def test_null_ctx_fails_loudly(lib):
    """No GPU needed: the argument checks come first."""
    assert lib.fp_gate_mask(None, None, None, None, None, None, None, None, None, _abi.FP_MEM_HOST, None) == -1
    assert b"ctx is NULL" in lib.fp_last_error()


def test_planner_classes_accept_or_refuse_gates():
    """No GPU: set_gates only records (FOP) or raises (the planners that order candidates before validation)."""
    from fiss_plus_planner_amd import planners as P

    class NoEngine:
        pass

    veh = synth.Vehicle()
    fop = P.FrenetOptimalPlanner(P.FrenetOptimalPlannerSettings(), veh, engine=NoEngine())
    fop.set_gates([60.0, np.nan], [[True, False], [False, True], [True, True]])
    assert fop._gates[0].tolist()[0] == 60.0 and np.isnan(fop._gates[0][1]) and fop._gates[1].tolist() == [1, 2, 3] and fop._gates[1].dtype == np.uint32
    assert fop._gates[2:] == (veh.l / 2, 0.0)
    fop.set_gates([60.0], np.array([1, 0, 1], dtype=np.uint32), front=0.0, max_decel=2.5)  # words already packed
    assert fop._gates[1].tolist() == [1, 0, 1] and fop._gates[2:] == (0.0, 2.5)
    fop.set_gates(None, None)
    assert fop._gates is None
    for bad in (dict(gate_s=[1.0], closed=[[True]], front=-1.0), dict(gate_s=[1.0], closed=[[True]], max_decel=np.inf), dict(gate_s=[1.0], closed=[[True]], max_decel=np.nan),
                dict(gate_s=[], closed=[[True]]), dict(gate_s=np.zeros(33), closed=np.zeros(4, dtype=np.uint32)), dict(gate_s=[1.0, 2.0], closed=[[True]]),
                dict(gate_s=[1.0], closed=np.zeros(0, dtype=np.uint32)), dict(gate_s=[1.0], closed=np.zeros((2, 2, 1)))):
        with pytest.raises(ValueError):
            fop.set_gates(**bad)
    for cls, st in ((P.FopPlusPlanner, P.FrenetOptimalPlannerSettings()), (P.FissPlanner, P.FissPlannerSettings()), (P.FissPlusPlanner, P.FissPlusPlannerSettings())):
        with pytest.raises(ValueError):
            cls(st, veh, engine=NoEngine()).set_gates([1.0], [[True]])


def test_closed_loop_runner_refuses_rules_it_cannot_run():
    """No GPU: the rules are checked before the runner touches the device."""
    from fiss_plus_planner_amd.device_batch import RULES, ClosedLoopRunner

    assert RULES == ("envelope", "gates", "boundary")
    gated = R.CASES["base"]()
    goal = np.zeros((gated.B, 2))
    for batch, kw in ((gated, dict(rules=("gates",), planner="FISS")), (gated, dict(rules=("gates",), planner="FISS+")), (gated, dict(rules=("lights",))),
                      (gated, dict(rules=("envelope",))), (gated, dict(rules=("gates", "boundary"))), (R.plain_batch(), dict(rules=("gates",))),
                      (R.plain_batch(), dict(rules="gates"))):
        with pytest.raises(ValueError):
            ClosedLoopRunner(None, SimpleNamespace(host=batch), goal, **kw)
    both = dataclasses.replace(gated, max_lat_accel=0.5, bound_left=np.full(gated.knots.shape, 2.0), bound_right=np.full(gated.knots.shape, -2.0))
    assert ClosedLoopRunner._check_rules(("boundary", "gates", "envelope"), "FOP", both) == RULES  # (they run in one order, whatever the caller's)
    assert ClosedLoopRunner._check_rules((), "FISS+", R.plain_batch()) == () and ClosedLoopRunner._check_rules("gates", "FOP", gated) == ("gates",)
