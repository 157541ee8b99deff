"""CPU: the time gap to moving obstacles (fp_gap_mask) on its reference alone (tests/gaps_ref.py) - the caps on undecided candidates and
the floor on the violating share of every test batch the GPU suite compares against, the cases whose outcome follows from the
definition, the hand-built lead case, the closed-loop scenario - and the parts of the binding that need no GPU: header and binding
agree, the planner classes accept or refuse the rule, ClosedLoopRunner's rule list."""
import ctypes as C
import dataclasses
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import gaps_ref as R
from fiss_plus_planner_amd import _abi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the reference's own numbers
@pytest.mark.parametrize("name", list(R.CASES))
def test_caps_and_violating_share(oracle, name):
    batch, refs = R.case(oracle, name)
    R.check_caps(refs, name)
    assert R.close_share(refs) >= R.SHARE_FLOOR[name], (name, R.close_share(refs))
    for r in refs:  # only survivors are flagged, one bit, and the winner is a survivor that is left
        assert not (r.close & ((r.flags_in & R.FLAG_INFEASIBLE) != 0)).any()
        assert np.array_equal(r.flags ^ r.flags_in, np.where(r.close, R.FLAG_COLLISION, 0))
        assert r.best_idx < 0 or not r.close[r.best_idx]


def test_cases_reach_the_paths_they_are_named_after(oracle):
    assert R.lds_plan(R.CASES["base"]()) == (True, True)
    assert R.lds_plan(R.CASES["cull_only"]()) == (False, True) and R.lds_plan(R.CASES["no_lds"]()) == (False, False)
    assert R.CASES["chunks"]().C > R.CHUNK > R.CASES["lattice567"]().C
    assert R.CASES["polygons"]().obs_nvert is not None and (R.CASES["polygons"]().obs_nvert > 0).sum() >= 20
    batch, refs = R.case(oracle, "line_ends")
    assert (refs[3].M <= 1).all() and refs[3].n_close == 0           # past the end of the line: no pose, no bit
    assert ((refs[1].flags_in >> 8) & 0xFFF > refs[1].M).any()       # M < N
    batch, refs = R.case(oracle, "short_table")
    assert batch.T_obs < int(np.ceil(batch.t_samples.max() / batch.tick_t)) and (batch.final_time_step < batch.T_obs - 1).any()
    assert any(r.best_idx < 0 < r.survivors for r in refs)          # an ego whose survivors all violate
    batch, refs = R.case(oracle, "t_now")
    assert (batch.t_now > 0).all()
    assert sum(r.best_idx != r.best_in for r in R.case(oracle, "base")[1]) >= 2  # the rule moves winners


def test_outcomes_that_follow_from_the_definition(oracle):
    batch, refs = R.case(oracle, "base")
    horizon = int(np.ceil(batch.t_samples.max() / batch.tick_t))
    for b, r in enumerate(refs):
        off = R.ego_gaps(oracle, batch, b, follow=0, lead=0)
        late = R.ego_gaps(oracle, batch, b, first=horizon)
        never = R.ego_gaps(oracle, batch, b, first=2**31 - 1)
        for q in (off, late, never):  # both lags 0, or `first` beyond every pose: the tables and the argmin as the dense call left them
            assert q.n_close == 0 and np.array_equal(q.flags, r.flags_in) and q.best_idx == r.best_in
        full = R.ego_gaps(oracle, batch, b, follow=horizon, lead=horizon)
        more = R.ego_gaps(oracle, batch, b, follow=256, lead=256)
        assert np.array_equal(full.flags, more.flags) and full.best_idx == more.best_idx  # lags longer than the horizon
        assert not (r.close & ~full.close).any()                                          # a longer lag only adds
        again = R.ego_gaps(oracle, batch, b, tables=(r.cost, r.flags))                    # the violators are no longer evaluated
        assert again.n_close == 0 and np.array_equal(again.flags, r.flags) and again.best_idx == r.best_idx
    no_scene = dataclasses.replace(batch, scene_of=np.full(batch.B, -1))
    q = R.ego_gaps(oracle, no_scene, 0)
    assert q.n_close == 0 and np.array_equal(q.flags, q.flags_in)


def test_a_parked_obstacle_is_the_collision_checks_business(oracle):
    """A shape that does not move is overlapped at a lag exactly when it is overlapped at lag 0 - at a pose the collision check looked
    at, so no survivor is flagged."""
    batch = R.with_gap(synth.make_batch(5, 5, 4, 3, 12, 120, False, R.SEED), follow=40, lead=40, first=1)
    refs = R.batch_gaps(oracle, batch)
    assert sum(r.survivors for r in refs) > 50 and sum(r.n_close for r in refs) == 0


def test_lead_case_is_flagged_by_the_lead_direction_alone(oracle):
    batch, refs = R.case(oracle, "lead")
    assert batch.gap_follow == 0 and refs[0].n_close >= 1 and refs[0].best_idx >= 0
    assert R.ego_gaps(oracle, batch, 0, follow=20, lead=0).n_close == 0
    # the flagged candidates are the ones that pull out towards the obstacle's lane
    i_d = np.nonzero(refs[0].close)[0] // (batch.nv * batch.nt)
    assert (batch.d_samples[i_d] > 0).all()


def test_closed_loop_keeps_its_distance_on_the_reference(oracle):
    batch, rows = R.loop_case(oracle)
    _, free = R.loop_case(oracle, gaps=False)
    assert len(rows) == len(free) == R.LOOP_CYCLES
    assert all(r.best_idx >= 0 for r in rows) and not any(r.undecided for r in rows)  # every cycle has a plan, and a decided one
    assert sum(r.n_close > 0 for r in rows) > R.LOOP_CYCLES // 2
    steps = np.arange(1, R.LOOP_CYCLES + 1)
    kept = R.bumper_distance(batch, [r.ego[0] for r in rows], steps)
    came = R.bumper_distance(batch, [r.ego[0] for r in free], steps)
    # two seconds behind a car doing LEAD_V are 8.2 m; without the rule the ego closes in to within a car's length
    assert came < batch.veh_l < R.LOOP_FOLLOW * batch.tick_t * R.LEAD_V < kept, (came, kept)


# ---------------------------------------------------------------- header, binding, library
def test_header_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "frenet_gpu.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} fp_time_gap;", hdr).group(1)
    fields = re.findall(r"int32_t\s+(\w+);", body)
    assert fields == [f[0] for f in _abi.FpTimeGap._fields_] and C.sizeof(_abi.FpTimeGap) == 16
    assert all(f[1] is C.c_int32 for f in _abi.FpTimeGap._fields_)
    decl = re.search(r"int fp_gap_mask\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == 11 and "fp_gap_mask" in _abi.EXPORTED_SYMBOLS
    assert "#define FP_ABI_VERSION 18" in hdr and _abi.FP_ABI_VERSION == 18


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "fiss_plus_planner_amd", "csrc"), "-s"])
    return _abi.load()


def test_library_exports_the_symbol_within_abi_18(lib):
    assert hasattr(lib, "fp_gap_mask") and lib.fp_abi_version() == 18
    assert lib.fp_gap_mask.argtypes is not None and len(lib.fp_gap_mask.argtypes) == 11


def test_null_ctx_fails_loudly(lib):
    """No GPU needed: the argument checks come first."""
    assert lib.fp_gap_mask(None, None, None, None, None, None, None, None, None, _abi.FP_MEM_HOST, None) == -1
    assert b"ctx is NULL" in lib.fp_last_error()


# ---------------------------------------------------------------- the Python layers
def test_batches_without_a_gap_keep_their_digests():
    plain = R.moving_batch()
    assert (plain.gap_follow, plain.gap_lead, plain.gap_first) == (0, 0, 1)
    assert dataclasses.replace(plain, gap_first=3).digest() == plain.digest()  # (no lag: no rule, whatever the grace)
    gapped = R.with_gap(plain)
    assert gapped.digest() != plain.digest() and R.with_gap(plain, lead=11).digest() != gapped.digest()
    assert gapped.take([1, 3]).gap_follow == 20 and gapped.take([1, 3]).gap_first == 2
    assert dataclasses.replace(gapped, gap_follow=256, gap_lead=256, gap_first=2**31 - 1).gap_first == 2**31 - 1
    for bad in (dict(gap_follow=-1), dict(gap_lead=-2), dict(gap_first=0), dict(gap_follow=257), dict(gap_lead=2**32 + 10), dict(gap_first=2**31)):
        with pytest.raises(AssertionError):
            dataclasses.replace(plain, **bad)


def test_binding_refuses_what_the_struct_cannot_hold():
    """No GPU: the range check comes before the library is touched (a ctypes field would wrap 2**32 + 2 to 2 silently)."""
    from fiss_plus_planner_amd.engine import _time_gap

    g = _time_gap(20, 10, 2**31 - 1, "t")
    assert (g.lag_follow, g.lag_lead, g.first, g.reserved0) == (20, 10, 2**31 - 1, 0)
    assert _time_gap(0, _abi.FP_MAX_POINTS, 1, "t").lag_lead == _abi.FP_MAX_POINTS
    for bad in ((-1, 0, 1), (0, -1, 1), (_abi.FP_MAX_POINTS + 1, 0, 1), (0, 2**32 + 5, 1), (20, 10, 0), (20, 10, 2**31), (20, 10, 2**32 + 2)):
        with pytest.raises(ValueError):
            _time_gap(*bad, "t")


def test_planner_classes_accept_or_refuse_the_time_gap():
    """No GPU: set_time_gap only records (FOP) or raises (the planners that order candidates before validation)."""
    from fiss_plus_planner_amd import planners as P

    class NoEngine:
        pass

    veh = synth.Vehicle()
    fop = P.FrenetOptimalPlanner(P.FrenetOptimalPlannerSettings(), veh, engine=NoEngine())
    fop.set_time_gap(2.0)
    assert fop._time_gap == (2.0, 0.0, 0.0)
    fop.set_time_gap(1.5, lead_s=1.0, grace_s=0.4)
    assert fop._time_gap == (1.5, 1.0, 0.4)
    fop.set_time_gap(0.0)
    assert fop._time_gap is None
    for bad in (dict(follow_s=-1.0), dict(follow_s=np.nan), dict(follow_s=np.inf), dict(follow_s=1.0, lead_s=-0.5), dict(follow_s=1.0, grace_s=np.nan),
                dict(follow_s=(_abi.FP_MAX_POINTS + 1) * fop.settings.tick_t), dict(follow_s=1.0, grace_s=2.0**31 * fop.settings.tick_t)):
        with pytest.raises(ValueError):
            fop.set_time_gap(**bad)
    for cls, st in ((P.FopPlusPlanner, P.FrenetOptimalPlannerSettings()), (P.FissPlanner, P.FissPlannerSettings()), (P.FissPlusPlanner, P.FissPlusPlannerSettings())):
        with pytest.raises(ValueError):
            cls(st, veh, engine=NoEngine()).set_time_gap(2.0)


def test_closed_loop_runner_knows_the_rule():
    """No GPU: the rules are checked before the runner touches the device."""
    from fiss_plus_planner_amd.device_batch import OBSTACLE_RULES, RULES, ClosedLoopRunner

    assert RULES == ("envelope", "gates", "boundary") and OBSTACLE_RULES == ("gaps",)
    gapped, plain = R.CASES["base"](), R.moving_batch()
    goal = np.zeros((gapped.B, 2))
    for batch, kw in ((gapped, dict(rules=("gaps",), planner="FISS")), (gapped, dict(rules=("gaps",), planner="FISS+")), (gapped, dict(rules=("gap",))),
                      (gapped, dict(rules=("gaps", "gates"))), (plain, dict(rules=("gaps",))), (plain, dict(rules="gaps")),
                      (dataclasses.replace(gapped, gap_follow=0, gap_lead=0), dict(rules=("gaps",)))):  # both lags 0 carry no data for the rule
        with pytest.raises(ValueError):
            ClosedLoopRunner(None, SimpleNamespace(host=batch), goal, **kw)
    every = dataclasses.replace(gapped, max_lat_accel=0.5, bound_left=np.full(gapped.knots.shape, 2.0), bound_right=np.full(gapped.knots.shape, -2.0),
                                gate_s=np.full((gapped.F, 1), 50.0), gate_closed=np.zeros((gapped.F, 4), dtype=np.uint32))
    assert ClosedLoopRunner._check_rules(("gaps", "boundary", "gates", "envelope"), "FOP", every) == RULES + OBSTACLE_RULES  # (it runs last)
    assert ClosedLoopRunner._check_rules("gaps", "FOP", gapped) == ("gaps",) and ClosedLoopRunner._check_rules(("gaps", "boundary"), "FOP", every) == ("boundary", "gaps")
    assert ClosedLoopRunner._check_rules((), "FISS+", plain) == ()
