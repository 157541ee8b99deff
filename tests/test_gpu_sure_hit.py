"""GPU: the walk's stage S (csrc/frenet_lattice_fused.hip, `// [section S]`: a blocked lon profile ends on one sure hit, before prep, B
and N) on the inputs of tests/sure_hit_cases.py - a box across the line at an early row, at row 0 and at the last checked row; the fan's
ends on either side of thr by 1e-5 and 1e-3 m; veh_l < veh_w; egos far off the line; the sure item behind 64 survivors and in a later
chunk of the list; a line that ends inside the checked rows; t_now odd on a short table; a NaN lateral sample, poses without a state,
an obstacle of size 0, egos without a scene; a near miss; a tight bend.  The stage stands in the shaped rectangle instances that run
three and four per CU: the 9 x 9 x 7 cases take it there and run WITHOUT it two per CU (latency mode, one workgroup per ego) and
through the lane-per-candidate kernel; the 5 x 5 x 5 shape (its shaped instances run two per CU only) and a run-time 5 x 4 x 3 are
controls.  The boundary cases put a real candidate on the fan's outside end - even egos on E+, odd egos on E- - so that a stage that
tested one end alone, or either end, blocks a candidate the oracle keeps free.  tests/test_sure_hit_cpu.py shows with the oracle
alone what each case is.

Every case runs in latency mode and with one workgroup per ego, three and four per CU (each also with the tail split forced and
forbidden), through the lane-per-candidate kernel and through the device entry point into fresh arrays, and is compared with the
oracle: flag words, Stats and the selected index exact, cost within 1e-9.  Two cases run through the FISS+ twin instances, compared bit
for bit with the search in its own launch."""
import numpy as np
import pytest

import sure_hit_cases as S
from test_gpu_adversarial import MODES
from test_gpu_scalar_paths import RESET_ALL, TAIL, TWO_PER_CU, device_call
from test_gpu_walk_decode import COST_TOL, SHAPE_555, SHAPE_997, assert_compiled_in_shape, check

pytestmark = pytest.mark.gpu
SHAPE_NAMES = list(S.SHAPES)


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("name", list(S.CASES))
def test_sure_hit_case_through_every_path(oracle, engine, name, shape):
    batch, _ = S.build(name, shape)
    assert batch.B == 8
    if shape == SHAPE_NAMES[0]:
        assert_compiled_in_shape(batch, SHAPE_997)
    elif shape == SHAPE_NAMES[1]:
        assert_compiled_in_shape(batch, SHAPE_555)
    before4 = engine.get_option("lattice_launches_4")
    try:
        # (the 5 x 5 x 5 shape's 50 rows of frames do not fit a third of a CU's LDS: its shaped instances run two per CU)
        ref = check(oracle, engine, batch, f"{name} [{shape}]", TWO_PER_CU if shape == SHAPE_NAMES[1] else MODES + TAIL)
    finally:
        engine.set_option("lattice_tail", 0)
    if shape == SHAPE_NAMES[0]:
        assert engine.get_option("lattice_launches_4") > before4
    # the device entry point, into fresh arrays
    idx, cost1, stats, cost, flags = device_call(engine, batch, None, None)
    for e, r in enumerate(ref):
        what = f"{name} [{shape}; device entry point] ego {e}"
        np.testing.assert_array_equal(flags[e], r.flags, err_msg=what + ": flag words")
        np.testing.assert_array_equal(stats[e], r.stats, err_msg=what + ": Stats")
        np.testing.assert_allclose(cost[e], r.cost, rtol=0, atol=COST_TOL, err_msg=what)
        assert idx[e] == r.best_idx, what


@pytest.mark.parametrize("name", list(S.FISS_TWINS))
def test_fiss_twin_instances(oracle, engine, name):
    """fiss_fused = 1: the lattice launch carries the search workgroups (the FISS instances, three and four per CU); fiss_fused = 0: the
    plain instances and the search in its own launch.  Every output identical; Stats exact, the cost within 1e-9 of the oracle's."""
    from test_gpu_fiss_fused import _run, _same

    batch = S.fiss_twin(name)
    ref = [p.fissplus_plan() for p in oracle.problems_from_batch(batch)]
    try:
        for label, opts in (("three per CU", {"resident_groups": 2, "lattice_occupancy": 3}), ("four per CU", {"resident_groups": 2}),
                            ("four per CU, four egos cut in two", {"resident_groups": 2, "lattice_tail": 4})):
            for k, v in {**RESET_ALL, **opts}.items():
                engine.set_option(k, v)
            own = _run(engine, batch, 0, None)
            _same(_run(engine, batch, 1, None), own, f"{name} [{label}]")
            for e, r in enumerate(ref):
                np.testing.assert_array_equal(own.stats[e], r.stats, err_msg=f"{name} [{label}] ego {e}")
                assert np.isnan(own.best_cost[e]) == np.isnan(r.best_cost), (name, label, e)
                if not np.isnan(r.best_cost):
                    assert abs(own.best_cost[e] - r.best_cost) <= COST_TOL, (name, label, e)
    finally:
        for k, v in RESET_ALL.items():
            engine.set_option(k, v)
