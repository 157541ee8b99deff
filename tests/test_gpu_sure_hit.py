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
import pytest

import lattice_paths as L
import sure_hit_cases as S

pytestmark = pytest.mark.gpu
SHAPE_NAMES = list(S.SHAPES)


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("name", list(S.CASES))
def test_sure_hit_case_through_every_path(oracle, engine, name, shape):
    batch, _ = S.build(name, shape)
    assert batch.B == 8
    compiled_in = dict(zip(SHAPE_NAMES, (L.SHAPE_997, L.SHAPE_555))).get(shape)
    ref = L.shaped_case(oracle, engine, batch, f"{name} [{shape}]", compiled_in, L.modes_for(batch), decides=False)
    L.device_entry_matches(engine, batch, ref, f"{name} [{shape}]")


@pytest.mark.parametrize("name", list(S.FISS_TWINS))
def test_fiss_twin_instances(oracle, engine, name):
    L.fiss_twins(oracle, engine, S.fiss_twin(name), name, L.fiss_twin_modes())
