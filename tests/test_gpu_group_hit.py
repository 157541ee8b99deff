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
import pytest

import group_hit_cases as C
import lattice_paths as L

pytestmark = pytest.mark.gpu
SHAPE_NAMES = list(C.SHAPES)


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("name", list(C.CASES))
def test_group_hit_case_through_every_path(oracle, engine, name, shape):
    batch, _ = C.build(name, shape)
    assert batch.B == 8
    compiled_in = dict(zip(SHAPE_NAMES, (L.SHAPE_997, L.SHAPE_555))).get(shape)
    ref = L.shaped_case(oracle, engine, batch, f"{name} [{shape}]", compiled_in, L.modes_for(batch), decides=False)
    L.device_entry_matches(engine, batch, ref, f"{name} [{shape}]")


def test_on_220_knot_lines(oracle, engine):
    batch = C.long_line()
    assert batch.NX >= 220
    ref = L.through_modes(oracle, engine, batch, "a box over the first second [220-knot lines]", L.MODES + L.TAIL, winner=False)
    L.device_entry_matches(engine, batch, ref, "a box over the first second [220-knot lines]")


def test_fiss_twin_instances(oracle, engine):
    L.fiss_twins(oracle, engine, C.fiss_twin(), "first second", L.fiss_twin_modes())
