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
ego, the three- and four-per-CU instances in rounds with a split tail (tests/test_gpu_adversarial.py's MODES, launch counters asserted)
and the lane-per-candidate kernel, and is compared with the oracle: flag words, Stats and the selected index exact, cost within 1e-9
(test_gpu_walk_decode.check)."""
import pytest

import range_argmin_cases as R
from test_gpu_adversarial import MODES
from test_gpu_walk_decode import assert_compiled_in_shape, check, colliding

pytestmark = pytest.mark.gpu
# (the 5 x 5 x 5 shape's 50 rows of frames do not fit a third of a CU's LDS: its shaped instances run two per CU)
MODES_555 = [m for m in MODES if m[2] in ("lattice_launches_2", None)]
GROUPED = [("grouped, 1024 threads", {"lattice_kernel": 2, "lattice_group": 99}, "lattice_launches_2"),
           ("grouped, one workgroup per ego", {"lattice_kernel": 2, "lattice_group": 99, "lattice_split": 1}, "lattice_launches_2")]


@pytest.mark.parametrize("name", list(R.RANGE_CASES))
def test_row_range_case_through_every_instance(oracle, engine, name):
    batch = R.RANGE_CASES[name]()
    if name in R.SHAPED_997:
        assert_compiled_in_shape(batch, R.SHAPE_997)
    elif name in R.SHAPED_555:
        assert_compiled_in_shape(batch, R.SHAPE_555)
    before4 = engine.get_option("lattice_launches_4")
    ref = check(oracle, engine, batch, name, MODES_555 if name in R.SHAPED_555 else MODES)
    assert 0 < colliding(ref) < batch.B * batch.C
    if name in R.SHAPED_997:
        assert engine.get_option("lattice_launches_4") > before4


@pytest.mark.parametrize("name", list(R.ARGMIN_CASES))
def test_argmin_case_through_every_instance(oracle, engine, name):
    batch = R.ARGMIN_CASES[name]()
    ref = check(oracle, engine, batch, name, MODES_555 if batch.nd == 5 else MODES)
    if name in R.NO_OBSTACLES:
        assert colliding(ref) == 0
    else:
        assert 0 < colliding(ref) < batch.B * batch.C


@pytest.mark.parametrize("name", ["9 x 9 x 7, v_samples permuted", "mirror tie across two wavefronts' shares (9 x 9 x 7)",
                                  "winners in the share of lateral sample 8", "the only feasible candidate is index C - 1"])
def test_grouped_launch(oracle, engine, name):
    """lattice_group = 99: as many slices per 1024-thread workgroup as the shape allows (16 wavefronts leave their candidates in the
    pose table's 16 KB).  That such a launch takes a grouped instance is pinned where launches are decided: rows `grouped_997` and
    `grouped_runtime` of tests/test_lattice_plan_cpu.py (a batch without obstacles has the run-time shape)."""
    batch = {**R.RANGE_CASES, **R.ARGMIN_CASES}[name]()
    try:
        check(oracle, engine, batch, name, GROUPED)
    finally:
        engine.set_option("lattice_group", 0)
