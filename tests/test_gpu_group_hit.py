"""GPU: stage V of the lattice kernel (csrc/frenet_lattice_fused.hip, `// [section VCIRC]`, `// [section VTEST]`: a whole end-speed
group ends before the walk on one sure hit of its circle) on the inputs of tests/group_hit_cases.py - every group of an ego ended,
only the slow or only the fast end speeds, a real candidate of every group passing a box beside the line by 1e-3 and 1e-5 m, the
rearmost candidate of the slowest group passing a box AHEAD by as much (straight and on a 12 m bend), that group's circle 1e-5 inside
thr, a 12 m bend, rows the
group does not share (a short horizon in the middle of t_samples, poses without a state, t_now > 0, final_time_step), NaN samples, veh_l < veh_w, a vehicle with
thr <= 0, the deciding item in a later chunk of the list.  tests/test_group_hit_cpu.py shows with the oracle alone what each case is.

Every case runs in latency mode and with one workgroup per ego, three and four per CU (each with the tail split forced - two workgroups
judge their own slices - and forbidden), through the lane-per-candidate kernel and through the device entry point, and is compared with
the oracle: flag words, Stats and the selected index exact, cost within 1e-9.  The 5 x 5 x 5 shape and a run-time 5 x 4 x 3 are controls
without the stage.  One case runs on 220-knot lines (the instances with the coefficient window) and one through the FISS+ twins."""
import numpy as np
import pytest

import group_hit_cases as C
from test_gpu_adversarial import MODES
from test_gpu_scalar_paths import RESET_ALL, TAIL, TWO_PER_CU, device_call
from test_gpu_walk_decode import COST_TOL, SHAPE_555, SHAPE_997, assert_compiled_in_shape, check

pytestmark = pytest.mark.gpu
SHAPE_NAMES = list(C.SHAPES)


def _through_every_path(oracle, engine, batch, what, modes):
    try:
        ref = check(oracle, engine, batch, what, modes)
    finally:
        engine.set_option("lattice_tail", 0)
    idx, _, stats, cost, flags = device_call(engine, batch, None, None)
    for e, r in enumerate(ref):
        np.testing.assert_array_equal(flags[e], r.flags, err_msg=f"{what} [device entry point] ego {e}: flag words")
        np.testing.assert_array_equal(stats[e], r.stats, err_msg=f"{what} [device entry point] ego {e}: Stats")
        np.testing.assert_allclose(cost[e], r.cost, rtol=0, atol=COST_TOL, err_msg=what)
        assert idx[e] == r.best_idx, (what, e)


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("name", list(C.CASES))
def test_group_hit_case_through_every_path(oracle, engine, name, shape):
    batch, _ = C.build(name, shape)
    assert batch.B == 8
    if shape == SHAPE_NAMES[0]:
        assert_compiled_in_shape(batch, SHAPE_997)
    elif shape == SHAPE_NAMES[1]:
        assert_compiled_in_shape(batch, SHAPE_555)
    before4 = engine.get_option("lattice_launches_4")
    _through_every_path(oracle, engine, batch, f"{name} [{shape}]", TWO_PER_CU if shape == SHAPE_NAMES[1] else MODES + TAIL)
    if shape == SHAPE_NAMES[0]:
        assert engine.get_option("lattice_launches_4") > before4


def test_on_220_knot_lines(oracle, engine):
    batch = C.long_line()
    assert batch.NX >= 220
    _through_every_path(oracle, engine, batch, "a box over the first second [220-knot lines]", MODES + TAIL)


def test_fiss_twin_instances(oracle, engine):
    from test_gpu_fiss_fused import _run, _same

    batch = C.fiss_twin()
    ref = [p.fissplus_plan() for p in oracle.problems_from_batch(batch)]
    try:
        for label, opts in (("three per CU", {"resident_groups": 2, "lattice_occupancy": 3}), ("four per CU", {"resident_groups": 2}),
                            ("four per CU, four egos cut in two", {"resident_groups": 2, "lattice_tail": 4})):
            for k, v in {**RESET_ALL, **opts}.items():
                engine.set_option(k, v)
            own = _run(engine, batch, 0, None)
            _same(_run(engine, batch, 1, None), own, f"first second [{label}]")
            for e, r in enumerate(ref):
                np.testing.assert_array_equal(own.stats[e], r.stats, err_msg=f"first second [{label}] ego {e}")
                assert np.isnan(own.best_cost[e]) == np.isnan(r.best_cost), (label, e)
                if not np.isnan(r.best_cost):
                    assert abs(own.best_cost[e] - r.best_cost) <= COST_TOL, (label, e)
    finally:
        for k, v in RESET_ALL.items():
            engine.set_option(k, v)
