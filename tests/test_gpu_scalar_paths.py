"""GPU: the fused lattice kernel's kernel-wide scalars (csrc/frenet_lattice_fused.hip) on the inputs of tests/scalar_cases.py - t_now odd,
a table shorter than the horizon (13 of 25 rows staged), final_time_step inside the table (11 rows checked), a line that ends inside
the checked rows, more survivors than the 256-entry list holds (item_base != 0), frame_of / scene_of permuted with an ego without a
scene, a 220-knot line behind a coefficient window, on both compiled-in shapes and a run-time shape with nv != nd.

Every case runs through
* the two-per-CU instances in latency mode (nsplit > 1: it_lo != 0) and with one workgroup per ego,
* the three- and four-per-CU instances (resident_groups = 2: eight egos are several rounds) with the tail split (the last four egos
  cut in two: nsplit 2 beside nsplit 1 in one launch) and without it (lattice_tail = 1),
* the same four under a caller's launch order that leaves no ego in its own slot, with an ego skipped between two live ones (the
  device entry point: fp_batch.launch_order / fp_batch.skip), into output arrays no earlier launch has written - the engine's own
  tables keep what the previous path left there, which would hide a candidate that is never written,
* the lane-per-candidate kernel as cross-check,
and is compared with the oracle: flag words, Stats and the selected index exact, cost within 1e-9.  The FISS+ cases run the twin
instances with the appended search (three and four per CU) against the search in its own launch, bit for bit, and against the oracle."""
import pytest

import lattice_paths as L
import scalar_cases as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(S.CASES))
def test_scalar_case_through_every_path(oracle, engine, name):
    batch = S.CASES[name]()
    assert batch.B <= 8
    shape = L.SHAPE_997 if name in S.SHAPED_997 else L.SHAPE_555 if name in S.SHAPED_555 else None
    L.shaped_case(oracle, engine, batch, name, shape, L.modes_for(batch))


@pytest.mark.parametrize("name", sorted(S.SHAPED_997) + [n for n in S.CASES if n.startswith("5 x 4 x 3")])
def test_scalar_case_under_a_callers_order_with_a_skipped_ego(oracle, engine, name):
    batch = S.CASES[name]()
    ref = L.reference(oracle, batch)
    for label, opts, counter in L.TAIL:
        with L.options(engine, {**opts, "lattice_order": 0}):  # (no learnt order: the caller's is the one that is used)
            for order, skip in ((S.ORDER, None), (S.ORDER, S.SKIP), (None, S.SKIP)):
                before = L.launches(engine, counter)
                L.device_entry_matches(engine, batch, ref, f"{name} [{label}]", order, skip)
                assert L.launches(engine, counter) > before, (name, label)


@pytest.mark.parametrize("name", list(S.FISS_CASES))
def test_fiss_twin_with_its_appended_search(oracle, engine, name):
    L.fiss_twins(oracle, engine, S.FISS_CASES[name](), name, L.fiss_twin_modes(no_tail_split=True), repetitions=2)
