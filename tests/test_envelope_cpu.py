"""CPU: the speed envelope (fp_speed_envelope) without a GPU - the reference restatement (tests/envelope_ref.py) on a case with a closed
form and on every batch the GPU tests use (caps on undecided candidates, shares, survivors, the per-profile observation the kernel rests
on: all asserted on the reference alone), limits_from_path_column, ProblemBatch.take / shard / digest, the header against the binding,
and the argument checks that need no device."""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import envelope_ref as R
from conftest import ROOT
from fiss_plus_planner_amd import _abi, synth
from fiss_plus_planner_amd.batch import ProblemBatch
from fiss_plus_planner_amd.spline import limits_from_path_column


def straight_batch(limit, front, tol, v0=5.0):
    """One ego on a straight 200 m line at constant speed v0 (one speed sample = v0, s_dd = 0): s_d = v0 at every point."""
    pts = np.zeros((1, 41, 2))
    pts[0, :, 0] = np.linspace(0.0, 200.0, 41)
    knots, coef = synth.build_frames(pts)
    return ProblemBatch(d_samples=[0.0, 0.5], t_samples=[8.0, 10.0], v_samples=[[v0]], target_speed=[v0], ego=[[10.0, v0, 0.0, 0.0, 0.0, 0.0]],
                        frame_of=[0], scene_of=[-1], t_now=[0], nx=[41], knots=knots, coef=coef, obs_pose=np.zeros((0, 1, 0, 4)), obs_dims=np.zeros((0, 0, 2)),
                        final_time_step=np.zeros(0, dtype=np.int32), veh_l=4.5, veh_w=1.8, max_speed=30.0, max_accel=10.0,
                        speed_limit=np.broadcast_to(np.asarray(limit, dtype=np.float64), (1, 41)).copy(), limit_front=front, limit_tol=tol)


def test_reference_on_a_closed_form(oracle):
    """Constant speed 5 m/s: the verdict is 5 > lim + tol exactly, and a zero stretch counts from where s + front reaches it."""
    for lim, want in ((5.0 - 0.05 + 1e-6, False), (5.0 - 0.05 - 1e-6, True)):
        r = R.ego_envelope(oracle, straight_batch(lim, 2.25, 0.05), 0)
        assert r.bit_a.tolist() == [want] * 4 and not r.bit_b.any() and np.allclose(r.slack, 1e-6, rtol=1e-3)
        assert r.n_limited == (4 if want else 0) and (r.best_idx >= 0) == (not want)
        assert np.array_equal(r.flags & ~np.uint32(R.FLAG_SPEED), r.flags_in) and not (r.flags_in & R.FLAG_SPEED).any()
    # the ego drives 40 m (T = 8 s) or 50 m (T = 10 s) from s = 10: the last checked point is s = 49.5 / 59.5, the bumper 2.25 m ahead of it
    lim = np.full(41, np.inf)
    lim[11:] = 0.0  # knots are 5 m apart: the zero stretch starts at s = 55
    r = R.ego_envelope(oracle, straight_batch(lim, 2.25, 0.05), 0)
    assert r.bit_a.tolist() == [False, True, False, True]  # (c = i_d * nt + i_T with nv = 1: only the T = 10 s profile reaches 55 m)
    r = R.ego_envelope(oracle, straight_batch(lim, 0.0, 0.05), 0)  # read at s itself: 59.5 is on the stretch too
    assert r.bit_a.tolist() == [False, True, False, True]
    lim[10] = 0.0  # from s = 50: 49.5 + 2.25 reaches it, 49.5 does not
    assert R.ego_envelope(oracle, straight_batch(lim, 2.25, 0.05), 0).bit_a.all()
    assert R.ego_envelope(oracle, straight_batch(lim, 0.0, 0.05), 0).bit_a.tolist() == [False, True, False, True]


def test_reference_curvature_on_a_circle():
    """kappa_r of a circle of radius 50 m, sampled finely enough for the spline to follow it."""
    th = np.linspace(0.0, 1.5, 61)
    pts = np.stack([50.0 * np.sin(th), 50.0 * (1.0 - np.cos(th))], axis=1)[None]
    knots, coef = synth.build_frames(pts)
    s = np.linspace(knots[0, 5], knots[0, -6], 200)  # (away from the natural spline's free ends)
    assert np.allclose(R.line_curvature(knots[0], coef[0], s), 1.0 / 50.0, rtol=2e-3)


@pytest.mark.parametrize("name", list(R.CASES))
def test_caps_hold_on_every_gpu_batch(oracle, name):
    """At most 0.5 % of a batch's candidates within 1e-9 of a threshold or of a deciding knot, at most one ego excluded for having one."""
    batch, refs = R.case(oracle, name)
    R.check_caps(refs, name)
    assert len(refs) == batch.B


@pytest.mark.parametrize("name", list(R.CASES))
def test_verdicts_are_shared_by_the_candidates_of_a_profile(oracle, name):
    """What the kernel rests on: the oracle's M and the reference's two bits are equal across i_d within a longitudinal profile."""
    batch, refs = R.case(oracle, name)
    P = batch.nv * batch.nt
    for r in refs:
        for arr in (r.M, r.N, r.bit_a, r.bit_b):
            a = np.asarray(arr).reshape(batch.nd, P)
            assert (a == a[0]).all(), name


def test_gpu_batches_limit_some_and_not_all(oracle):
    """A batch where all or none violate tests nothing: 10 % .. 90 % on base, lat and both, at least three egos keep a survivor."""
    for name in ("base", "lat", "both"):
        batch, refs = R.case(oracle, name)
        assert 0.10 <= R.limited_share(refs) <= 0.90, (name, R.limited_share(refs))
        assert sum(r.best_idx >= 0 for r in refs) >= 3, name
    _, base = R.case(oracle, "base")
    _, lat = R.case(oracle, "lat")
    _, both = R.case(oracle, "both")
    assert any(r.bit_a.any() for r in base) and not any(r.bit_b.any() for r in base)
    assert any(r.bit_b.any() for r in lat) and not any(r.bit_a.any() for r in lat)
    assert any((r.bit_a & ~r.bit_b).any() for r in both) and any((r.bit_b & ~r.bit_a).any() for r in both)  # each check decides something alone
    assert [r.best_idx for r in both] != [r.best_idx for r in base]                                       # ... and the lateral one moves a winner
    # the shapes the cases exist for
    N = lambda refs: np.concatenate([r.N for r in refs])  # noqa: E731
    M = lambda refs: np.concatenate([r.M for r in refs])  # noqa: E731
    assert 64 < N(base).min() and N(base).max() <= 128                       # two lane rounds
    assert N(R.case(oracle, "tick005")[1]).max() == 200                      # four
    ends = R.case(oracle, "line_ends")[1]
    assert ((M(ends) < N(ends)) & (M(ends) > 1)).any() and (ends[3].M <= 1).all() and not ends[3].limited.any()
    cb, chunks = R.case(oracle, "chunks")
    assert cb.B == 2 and cb.C == 567 and any(r.limited.any() for r in chunks) and any(r.best_idx >= 0 for r in chunks)
    ub, unl = R.case(oracle, "unlimited")
    assert np.isinf(ub.speed_limit).all() and ub.max_lat_accel == 0.0
    for r in unl:
        assert not r.limited.any() and np.array_equal(r.flags, r.flags_in) and r.best_idx == r.best_in


def test_stop_line_moves_winners(oracle):
    batch, refs = R.case(oracle, "stop")
    egos = R.stop_egos(oracle)
    assert len(egos) >= 2
    lim, start = R.stop_limit(R.plain_batch())
    assert np.array_equal(lim, batch.speed_limit) and (start - batch.ego[:, 0] >= R.STOP_AHEAD).all() and (start - batch.ego[:, 0] < R.STOP_AHEAD + 6.0).all()
    prob = oracle.problems_from_batch(batch)
    for b in egos:
        r = refs[b]
        assert not r.bit_a[r.best_idx] and r.best_idx != r.best_in
        # restated once more for the winner alone: on the zero stretch only at rest
        c, nv, nt = r.best_idx, batch.nv, batch.nt
        t = prob[b].eval_traj(float(batch.d_samples[c // (nv * nt)]), float(batch.v_samples[b, c % nv]), float(batch.t_samples[(c // nv) % nt]), dump=True, stride=256)
        s, s_d = t.arrays[R.S, 1:t.M], t.arrays[R.S_D, 1:t.M]
        assert (s_d[s + batch.limit_front >= start[b]] <= batch.limit_tol).all()


def test_limits_from_path_column():
    col = [13.4, 1, 0, 0.0, 8.3, 1.0, 2]
    out = limits_from_path_column(col)
    assert out.dtype == np.float64 and out.tolist() == [13.4, np.inf, 0.0, 0.0, 8.3, np.inf, 2.0]
    assert limits_from_path_column(np.zeros((0,))).shape == (0,)
    for bad in ([1.0, np.nan], [-1.0, 3.0]):
        with pytest.raises(ValueError):
            limits_from_path_column(bad)


def test_take_and_shard_keep_the_profile():
    b = R.CASES["both"]()
    sub = b.take([3, 1])
    assert np.array_equal(sub.speed_limit[sub.frame_of], b.speed_limit[[3, 1]]) and np.array_equal(sub.knots[sub.frame_of], b.knots[[3, 1]])
    assert (sub.limit_front, sub.limit_tol, sub.max_lat_accel) == (b.limit_front, b.limit_tol, b.max_lat_accel) == (0.5 * b.veh_l, R.TOL, R.MAX_LAT_ACCEL)
    sh = b.shard(1, 2)
    assert sh.B == 3 and np.array_equal(sh.speed_limit[sh.frame_of], b.speed_limit[2:5]) and sh.max_lat_accel == b.max_lat_accel
    plain = R.plain_batch()
    assert plain.take([0]).speed_limit is None and plain.shard(0, 2).speed_limit is None and plain.take([0]).max_lat_accel == 0.0
    with pytest.raises(AssertionError):  # the shape is [F, NX]
        dataclasses.replace(plain, speed_limit=np.ones((5, 80)))


def test_a_batch_without_a_profile_keeps_its_digest():
    """Pinned on the commit before the profile fields existed (the same batch and digest as tests/test_boundary_cpu.py)."""
    plain = R.plain_batch()
    assert plain.speed_limit is None and (plain.limit_front, plain.limit_tol, plain.max_lat_accel) == (0.0, 0.0, 0.0)
    assert plain.digest() == "48c26a8ddc9898b2a4dcadda741a0e6d07287e10d0a8bb7f63f8f6bdefc926e1"
    digests = {plain.digest(), R.with_profile(plain).digest(), R.with_profile(plain, tol=0.1).digest(),
               R.with_profile(plain, limit=None, max_lat_accel=0.3).digest()}
    assert len(digests) == 4


def _header():
    return open(os.path.join(ROOT, "include", "frenet_gpu.h")).read()


def test_header_and_binding_agree(tmp_path):
    hdr = _header()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+fp_speed_envelope\s*\(", code) and "fp_speed_envelope" in _abi.EXPORTED_SYMBOLS
    declared = sorted(set(re.findall(r"\b(fp_\w+)\s*\(", code)))
    assert declared == sorted(_abi.EXPORTED_SYMBOLS)
    assert int(re.search(r"#define FP_FLAG_SPEED (\d+)u", hdr).group(1)) == _abi.FLAG_SPEED == R.FLAG_SPEED
    assert int(re.search(r"#define FP_FLAG_ACCEL (\d+)u", hdr).group(1)) == _abi.FLAG_ACCEL == R.FLAG_ACCEL
    assert _abi.FLAG_INFEASIBLE == R.FLAG_INFEASIBLE
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "frenet_gpu.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(fp_speed_profile));']
    for fname, _ in _abi.FpSpeedProfile._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(fp_speed_profile, {fname}));')
    lines += ['  printf("version %d\\n", FP_ABI_VERSION);', '  return 0;', '}']
    src = tmp_path / "profile.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "profile"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_abi.FpSpeedProfile) == 32
    for fname, _ in _abi.FpSpeedProfile._fields_:
        assert int(got[fname]) == getattr(_abi.FpSpeedProfile, fname).offset, fname
    assert int(got["version"]) == 18 == _abi.FP_ABI_VERSION


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "fiss_plus_planner_amd", "csrc"), "-s"])
    return _abi.load()


def test_library_exports_the_symbol_within_abi_18(lib):
    assert hasattr(lib, "fp_speed_envelope") and lib.fp_abi_version() == 18
    assert lib.fp_speed_envelope.argtypes is not None and len(lib.fp_speed_envelope.argtypes) == 11


def test_null_ctx_fails_loudly(lib):
    """No GPU needed: the argument checks come first."""
    assert lib.fp_speed_envelope(None, None, None, None, None, None, None, None, None, _abi.FP_MEM_HOST, None) == -1
    assert b"ctx is NULL" in lib.fp_last_error()


def test_planner_classes_accept_or_refuse_a_profile():
    """No GPU: set_speed_profile only records (FOP) or raises (the planners that order candidates before validation)."""
    from fiss_plus_planner_amd import planners as P

    class NoEngine:
        pass

    veh = synth.Vehicle()
    fop = P.FrenetOptimalPlanner(P.FrenetOptimalPlannerSettings(), veh, engine=NoEngine())
    fop.set_speed_profile([8.0, np.inf, 0.0])
    assert fop._speed_profile[1:] == (veh.l / 2, 0.05, 0.0) and fop._speed_profile[0].tolist() == [8.0, np.inf, 0.0]
    fop.set_speed_profile([8.0], front=0.0, tol=0.0, max_lat_accel=1.5)
    assert fop._speed_profile[1:] == (0.0, 0.0, 1.5)
    fop.set_speed_profile(None, max_lat_accel=1.0)
    assert fop._speed_profile[0] is None and fop._speed_profile[3] == 1.0
    fop.set_speed_profile(None)
    assert fop._speed_profile is None
    for bad in (dict(v_limit=[1.0, np.nan]), dict(v_limit=[-1.0]), dict(v_limit=[1.0], front=-1.0), dict(v_limit=[1.0], tol=np.inf),
                dict(v_limit=[1.0], max_lat_accel=-0.1), dict(v_limit=[1.0], max_lat_accel=np.nan)):
        with pytest.raises(ValueError):
            fop.set_speed_profile(**bad)
    for cls, st in ((P.FopPlusPlanner, P.FrenetOptimalPlannerSettings()), (P.FissPlanner, P.FissPlannerSettings()), (P.FissPlusPlanner, P.FissPlusPlannerSettings())):
        with pytest.raises(ValueError):
            cls(st, veh, engine=NoEngine()).set_speed_profile([1.0])
