"""CPU: what makes the GPU suite of fp_fallback_stop (tests/test_gpu_fallback.py) meaningful, shown without a device.  The restatement
(tests/fallback_ref.py) leaves out at most MAX_LEFT_OUT egos of every fixture; every fixture reaches the path it is named after; the
closed-loop scenario reaches its three phases with no undecided cycle; FallbackStop refuses bad arguments and the binding's struct
matches the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fallback_cases as FC
import fallback_ref as FR
from conftest import ROOT
from fiss_plus_planner_amd import _abi
from fiss_plus_planner_amd.fallback import FallbackStop


@pytest.mark.parametrize("name", sorted(FC.FIXTURES))
def test_reference_stays_within_the_cap(oracle, name):
    c, r = FC.case(name), FC.reference(oracle, name)
    left_out = int((r.need & ~r.counted).sum())
    print(f"{name}: {int(r.need.sum())} egos need a fallback, {left_out} left out, smallest slack {r.slack[r.need].min():.3e}, status {r.status.tolist()}")
    assert left_out <= FR.MAX_LEFT_OUT
    assert r.need.sum() - left_out >= 1
    assert r.cand.shape == (c.batch.B, len(np.atleast_1d(c.d_targets)) * len(c.stop_T))


def test_base_reaches_its_paths(oracle):
    c, r = FC.case("base"), FC.reference(oracle, "base")
    b, n_stop = c.batch, len(c.stop_T)
    assert r.counted.all()
    # ego 0: the longer stops leave the line, and stay admissible (M >= 2)
    assert (r.M[0] < r.N[0]).any() and (r.M[0] == r.N[0]).any() and (r.cand[0] != -2).all()
    # ego 1: a clear stop that is not the longest T, because the longer ones reverse (v0 = 5, a0 = -4: the header's example)
    assert r.status[1] == FR.CLEAR and r.fb_idx[1] % n_stop < n_stop - 1
    assert (r.cand[1].reshape(-1, n_stop)[:, r.fb_idx[1] % n_stop + 1:] == -2).all() and (r.cand[1].reshape(-1, n_stop)[:, :r.fb_idx[1] % n_stop + 1] == -1).all()
    prob = oracle.problems_from_batch(b, egos=[1])[0]
    assert prob.eval_traj(0.2, 0.0, 6.0, dump=True).arrays[2, :60].min() < -0.4
    # ego 2: every candidate hits; the latest hit wins, and it is not candidate-independent
    assert r.status[2] == FR.CONTACT and (r.cand[2] >= 0).all() and r.hit_step[2] == r.cand[2].max() and len(set(r.cand[2].tolist())) > 1
    assert r.hit_obs[2] == 0 and r.hit_speed[2] > 1.0
    # ego 3: M = 1 for every candidate, nothing admissible
    assert r.status[3] == FR.NONE and (r.cand[3] == -2).all() and (r.M[3] == 1).all() and np.isnan(r.end_state[3]).all() and r.fb_idx[3] == -1
    # ego 4 has a plan, ego 5 is skipped: status 0, the decoded sample / NaN, cand untouched
    assert r.status[4] == 0 and np.array_equal(r.end_state[4], FR.decode(b, 4, 5)) and r.status[5] == 0 and np.isnan(r.end_state[5]).all()
    assert (r.cand[4:6] == -3).all() and r.counts[:, 0].tolist() == [0, 0, 0, 0, 1, 1, 0, 0]
    # ego 6: t_now > 0 among obstacles that move (the rows read are t_now + i)
    assert b.t_now[6] == 7 and r.need[6]
    # ego 7: the horizon cuts the poses before the wall; with the whole table in view the same family hits it
    assert r.status[7] == FR.CLEAR and (r.cand[7] == -1).all()
    fts = b.final_time_step.copy()
    try:
        b.final_time_step[7] = b.T_obs - 1
        full = FR.fallback(oracle, b, c.stop_T, c.d_targets, c.max_decel, best_idx=c.best_idx, skip=c.skip)
    finally:
        b.final_time_step[...] = fts
    assert (full.cand[7] >= 10).any() and full.cand[7][full.cand[7] >= 0].min() >= 9


def test_many_poses_hit_in_the_second_and_third_round(oracle):
    c, r = FC.case("many poses"), FC.reference(oracle, "many poses")
    assert FR.points_cap(c.batch, c.stop_T) == 160 and r.N.max() == 160 and c.batch.check_stride == 1
    assert ((r.cand[0] >= 64) & (r.cand[0] < 128)).any() and (r.cand[1] >= 128).any()
    assert r.counted.all()


def test_off_lds_rows_exceed_the_budget(oracle):
    """lds_layout_doubles restated: 81 knots x 9 + 48 x 4 + 128 rows x 48 x 4 doubles = 204 KB against 144 KB; every other fixture fits."""
    for name in FC.FIXTURES:
        c = FC.case(name)
        doubles, fits = FC.rows_in_lds(c.batch, FR.points_cap(c.batch, c.stop_T))
        assert fits == (name != "off LDS"), (name, doubles * 8)
    c, r = FC.case("off LDS"), FC.reference(oracle, "off LDS")
    assert FC.rows_in_lds(c.batch, 128)[0] == 81 * 9 + 48 * 4 + 128 * 48 * 4
    assert r.status[0] == FR.CONTACT and r.hit_obs[0] == 47 and r.counted.all()


def test_ties_and_deceleration_bound(oracle):
    c, r = FC.case("ties"), FC.reference(oracle, "ties")
    n_stop = len(c.stop_T)
    for e in (0, 1):  # both targets clear and equally far: the smaller i_d wins
        assert r.cand[e, r.fb_idx[e]] == -1 and r.cand[e, r.fb_idx[e] + n_stop] == -1 and r.fb_idx[e] // n_stop == 0
        assert abs(c.d_targets[0] - c.batch.ego[e, 3]) == abs(c.d_targets[1] - c.batch.ego[e, 3])
    assert c.batch.scene_of[0] == -1
    assert (r.cand == -2).any() and np.isfinite(c.max_decel)  # (the bound removes the short stops)
    unbounded = FR.fallback(oracle, c.batch, c.stop_T, c.d_targets, np.inf, best_idx=c.best_idx)
    assert (unbounded.cand != -2).all()


def test_no_obstacles_and_single_candidate(oracle):
    c, r = FC.case("no obstacles"), FC.reference(oracle, "no obstacles")
    assert c.batch.n_obs == 0 and (c.batch.scene_of == -1).all() and r.cand.shape[1] == 1
    assert (r.status == FR.CLEAR).all() and (r.fb_idx == 0).all() and np.array_equal(r.end_state[:, 0], c.batch.ego[:, 3])


def test_rings_decide_a_contact(oracle):
    c, r = FC.case("rings"), FC.reference(oracle, "rings")
    assert r.status[1] == FR.CONTACT and c.batch.obs_nvert[1, r.hit_obs[1]] == 6
    assert (r.cand[0] >= 0).any() and r.status[0] == FR.CLEAR and r.counted.all()


def test_loop_scenario_reaches_its_three_phases(oracle):
    """Driven through the oracle, the restatement and advance_ref: without a fallback every ego ends with DONE_NO_SOLUTION in front of
    the wall; with it every ego plans, then brakes on CLEAR fallbacks while the wall stands, then plans again and ends at the end of
    the line - never in contact, and no cycle's fallback is undecided."""
    batch, _ = FC.loop_scenario()
    assert batch.v_samples.min() > 0
    plain = FC.loop_reference(oracle, fallback=False)
    assert (plain.done == 3).all() and (plain.cycles < FC.K_OPEN).all()
    r = FC.loop_reference(oracle)
    assert r.undecided == 0
    assert (r.done == 2).all() and (r.counts[:, 1] > 0).all() and (r.counts[:, 2:] == 0).all()
    for b in range(batch.B):
        st = r.status[:r.cycles[b], b]
        fb = np.nonzero(st == FR.CLEAR)[0]
        assert (st[:fb[0]] == 0).all() and (st[fb[-1] + 1:] == 0).all() and fb[-1] + 1 < len(st) and fb[0] > 0  # plan, brake, plan again
        assert fb[-1] < FC.K_OPEN
    # the wall's rear face is at 45 - 1 m: no front bumper reaches it while it stands
    assert np.nanmax(r.states[:FC.K_OPEN, :, 0]) + 0.5 * batch.veh_l < 44.0  # (state k is the ego at step k; the wall is valid in rows 0 .. K_OPEN - 1)


def test_fallback_stop_argument_errors():
    for bad in ([], [1.0, 1.0], [2.0, 1.0], [0.0, 1.0], [-1.0], [np.nan], [np.inf], [[1.0, 2.0]]):
        with pytest.raises(ValueError, match="stop_times"):
            FallbackStop(bad)
    with pytest.raises(ValueError, match="max_decel"):
        FallbackStop([1.0], max_decel=0.0)
    with pytest.raises(ValueError, match="max_decel"):
        FallbackStop([1.0], max_decel=float("nan"))
    with pytest.raises(ValueError, match="d_targets"):
        FallbackStop([1.0], d_targets=[])
    with pytest.raises(ValueError, match="d_targets"):
        FallbackStop([1.0], d_targets=[np.inf])
    with pytest.raises(ValueError, match="FP_MAX_FALLBACK"):
        FallbackStop(np.arange(1, 130) * 0.01, d_targets=[0.0, 1.0])
    fs = FallbackStop([1.0, 2.5], max_decel=6.0)
    batch = FC.case("base").batch
    assert np.array_equal(fs.targets(batch)[1:], batch.d_samples) and np.isnan(fs.targets(batch)[0]) and fs.n_candidates(batch) == 2 * (batch.nd + 1)
    assert fs.points_max(0.1) == 25
    seen = {}
    st = fs.struct(batch, lambda name, a: seen.setdefault(name, a).ctypes.data)
    assert (st.n_d, st.n_stop, st.max_decel) == (batch.nd + 1, 2, 6.0) and st.d_targets == seen["fallback_d"].ctypes.data and st.stop_T == seen["fallback_T"].ctypes.data
    with pytest.raises(ValueError, match="FP_MAX_FALLBACK"):
        FallbackStop(np.arange(1, 101) * 0.01).targets(batch)  # (None resolves to nd + 1 = 4 targets: 400 candidates)


def test_struct_layout_and_constants_match_the_header(tmp_path):
    """fp_fallback against its ctypes mirror, and the constants, as gcc reads them from the header (a stand-alone C program)."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "frenet_gpu.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(fp_fallback));']
    for fname, _ in _abi.FpFallback._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(fp_fallback, {fname}));')
    lines += ['  printf("max %d\\n", FP_MAX_FALLBACK);', '  printf("tol %.17g\\n", FP_FALLBACK_REVERSE_TOL);',
              '  printf("status %d%d%d%d\\n", FP_FALLBACK_NOT_NEEDED, FP_FALLBACK_CLEAR, FP_FALLBACK_CONTACT, FP_FALLBACK_NONE);', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_abi.FpFallback)
    for fname, _ in _abi.FpFallback._fields_:
        assert int(got[fname]) == getattr(_abi.FpFallback, fname).offset, fname
    assert int(got["max"]) == _abi.FP_MAX_FALLBACK == FR.MAX_FALLBACK and float(got["tol"]) == _abi.FP_FALLBACK_REVERSE_TOL == FR.REVERSE_TOL
    assert got["status"] == "0123" and (_abi.FALLBACK_NOT_NEEDED, _abi.FALLBACK_CLEAR, _abi.FALLBACK_CONTACT, _abi.FALLBACK_NONE) == (0, 1, 2, 3)
    assert "fp_fallback_stop" in _abi.EXPORTED_SYMBOLS


def test_the_library_exports_the_symbol():
    assert hasattr(_abi.load(), "fp_fallback_stop")
