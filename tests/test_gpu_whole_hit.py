"""GPU: stage W of the lattice kernel (csrc/frenet_lattice_fused.hip, `// [section WEXIT]`: behind the walk, full collision masks of
all the workgroup's slices end the ego - no assembly and no argmin when no table is requested, no argmin with tables) on the inputs
of tests/whole_hit_cases.py - egos stage V ends whole (at row 0, at rows 8-10, on a bend, in a later item chunk, with t_now odd), egos
the walk fills, one free candidate among colliding ones (beside the line by 1e-3 and 1e-5 m, along it straight and on a 12 m bend), lon
profiles with one point at the line's end, a short horizon in the middle of t_samples (one half of a tail-split ego is blocked whole,
the other is not), final_time_step, poses without a state and NaN poses, NaN samples, thr <= 0, veh_l < veh_w.
tests/test_whole_hit_cpu.py shows with the oracle alone what each case is.

Every case runs with the tables requested through every path (latency mode and one workgroup per ego, three and four per CU, each with
the tail split forced and forbidden, the lane-per-candidate kernel) and through the device entry point three and four per CU: flag
words, Stats and the selected index exact, every cost within 1e-9.  Then WITHOUT tables - the headline's call, where the stage skips
the assembly - through the same paths: selected index and Stats exact, selected cost within 1e-9.  The 5 x 5 x 5 shape and a run-time
5 x 4 x 3 are controls without the stage; one case runs through the FISS+ twins (their tables are always written) and one through
a closed loop on the device."""
import numpy as np
import pytest

import lattice_paths as L
import lattice_quiet as Q
import whole_hit_cases as C

pytestmark = pytest.mark.gpu
SHAPE_NAMES = list(C.SHAPES)
ROUNDS3 = {**L.ROUNDS, "lattice_occupancy": 3}


def _case(oracle, engine, name, shape):
    batch, _ = C.build(name, shape)
    assert batch.B == 8
    what = f"{name} [{shape}]"
    compiled_in = dict(zip(SHAPE_NAMES, (L.SHAPE_997, L.SHAPE_555))).get(shape)
    ref = L.shaped_case(oracle, engine, batch, what, compiled_in, L.modes_for(batch), decides=False)
    for opts in ((L.ROUNDS, ROUNDS3) if compiled_in == L.SHAPE_997 else ({},)):
        with L.options(engine, opts):
            L.device_entry_matches(engine, batch, ref, what)
    Q.quiet_matches(engine, batch, ref, what, L.modes_for(batch))


@pytest.mark.parametrize("name", list(C.CASES))
def test_whole_hit_case_through_every_path(oracle, engine, name):
    _case(oracle, engine, name, SHAPE_NAMES[0])


@pytest.mark.parametrize("shape", SHAPE_NAMES[1:])
@pytest.mark.parametrize("name", C.CONTROLS)
def test_controls_without_the_stage(oracle, engine, name, shape):
    _case(oracle, engine, name, shape)


def test_fiss_twin_instances(oracle, engine):
    L.fiss_twins(oracle, engine, C.fiss_twin(), "first second", L.fiss_twin_modes())


def test_closed_loop_step_on_blocked_egos(engine):
    """Three closed-loop cycles on egos that are blocked whole: the hand-over (state, step counter, done flags) three and four per CU is
    that of the two-per-CU instance, which has no stage W and hands the egos over itself."""
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch

    outs = []
    for opts in ({"lattice_kernel": 2}, L.ROUNDS, ROUNDS3):
        batch, _ = C.build("a box over the first second", SHAPE_NAMES[0])
        goal = np.stack([batch.coef[batch.frame_of, 0, 40], batch.coef[batch.frame_of, 4, 40]], axis=1)
        with L.options(engine, opts):
            outs.append(ClosedLoopRunner(engine, DeviceBatch(batch, 0), goal, "FOP").run(3))
    for out in outs[1:]:
        for k in ("done", "cycles", "t_now"):
            np.testing.assert_array_equal(getattr(out, k), getattr(outs[0], k), err_msg=k)
        assert np.array_equal(out.ego, outs[0].ego, equal_nan=True)
