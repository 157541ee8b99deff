"""GPU: the fused lattice kernel's row ranges and argmin (csrc/frenet_lattice_fused.hip, sections VENDS / RANGES and ARGMIN) on the
inputs of tests/range_argmin_cases.py.

* row ranges   the shaped instances take a row's arclength range from the lon profiles of the smallest and the largest end speed
               (found once per ego, any order of v_samples); the run-time-shape instances evaluate every sample.  v_samples ascending,
               descending, permuted with both extremes on middle indices, equal extremes, a negative and an infinite sample, a NaN in
               the middle and at an end, nv = 1, nv != nd; obstacles that exist at one late step and that only the fastest / only the
               slowest profile reaches (a range from the first and the last INDEX culls them: tests/test_range_argmin_cpu.py shows that
               the oracle's flags then differ); t_now odd; a windowed 220-knot line.
* argmin       one wavefront merges every lane's candidate.  Winners in every wavefront's share of the candidates and in the assembly
               loop's second trip (index >= 512), the only feasible candidate first and last, none feasible, fewer candidates than a
               wavefront has lanes, bit-exact ties between mirrored lateral samples inside one share and across two (the higher index
               wins), no obstacles (the smallest layout), the 1024-thread grouped instances.

Every case runs through the two-per-CU instances in latency mode (the partial argmins of several workgroups) and with one workgroup per
ego, the three- and four-per-CU instances in rounds with a split tail (tests/lattice_paths.py's MODES, launch counters asserted)
and the lane-per-candidate kernel, and is compared with the oracle: flag words, Stats and the selected index exact, cost within 1e-9
(lattice_paths.through_modes)."""
import pytest

import lattice_paths as L
import range_argmin_cases as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(R.RANGE_CASES))
def test_row_range_case_through_every_instance(oracle, engine, name):
    batch = R.RANGE_CASES[name]()
    shape = L.SHAPE_997 if name in R.SHAPED_997 else L.SHAPE_555 if name in R.SHAPED_555 else None
    L.shaped_case(oracle, engine, batch, name, shape, L.modes_for(batch, tail=False))


@pytest.mark.parametrize("name", list(R.ARGMIN_CASES))
def test_argmin_case_through_every_instance(oracle, engine, name):
    batch = R.ARGMIN_CASES[name]()
    ref = L.shaped_case(oracle, engine, batch, name, None, L.modes_for(batch, tail=False), decides=name not in R.NO_OBSTACLES)
    if name in R.NO_OBSTACLES:
        assert L.colliding(ref) == 0


@pytest.mark.parametrize("name", ["9 x 9 x 7, v_samples permuted", "mirror tie across two wavefronts' shares (9 x 9 x 7)",
                                  "winners in the share of lateral sample 8", "the only feasible candidate is index C - 1"])
def test_grouped_launch(oracle, engine, name):
    """lattice_group = 99: as many slices per 1024-thread workgroup as the shape allows (16 wavefronts leave their candidates in the
    pose table's 16 KB).  That such a launch takes a grouped instance is pinned where launches are decided: rows `grouped_997` and
    `grouped_runtime` of tests/test_lattice_plan_cpu.py (a batch without obstacles has the run-time shape)."""
    batch = {**R.RANGE_CASES, **R.ARGMIN_CASES}[name]()
    L.through_modes(oracle, engine, batch, name, L.GROUPED, winner=False)
