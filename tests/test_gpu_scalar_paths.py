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
import numpy as np
import pytest

import scalar_cases as S
from test_gpu_adversarial import MODES, RESET
from test_gpu_walk_decode import COST_TOL, assert_compiled_in_shape, check, colliding

pytestmark = pytest.mark.gpu
ROUNDS = {"lattice_kernel": 2, "resident_groups": 2}
# (the automatic tail of a launch this small cuts no ego - an eighth or a quarter of a round of two CUs' worth - so the split is asked for:
# lattice_tail = 4 cuts the last four dispatch slots in two, 1 forbids it)
TAIL = [("three per CU, four egos cut in two", {**ROUNDS, "lattice_occupancy": 3, "lattice_tail": 4}, "lattice_launches_3"),
        ("four per CU, four egos cut in two", {**ROUNDS, "lattice_tail": 4}, "lattice_launches_4|lattice_launches_3"),
        ("three per CU, no tail split", {**ROUNDS, "lattice_occupancy": 3, "lattice_tail": 1}, "lattice_launches_3"),
        ("four per CU, no tail split", {**ROUNDS, "lattice_tail": 1}, "lattice_launches_4|lattice_launches_3")]
RESET_ALL = {**RESET, "lattice_tail": 0}
# (the 5 x 5 x 5 shape's 50 rows of frames do not fit a third of a CU's LDS: its shaped instances run two per CU)
TWO_PER_CU = [m for m in MODES if m[2] in ("lattice_launches_2", None)]


def modes_of(name):
    return TWO_PER_CU if name in S.SHAPED_555 else MODES + TAIL


@pytest.mark.parametrize("name", list(S.CASES))
def test_scalar_case_through_every_path(oracle, engine, name):
    batch = S.CASES[name]()
    assert batch.B <= 8
    if name in S.SHAPED_997:
        assert_compiled_in_shape(batch, S.SHAPE_997)
    elif name in S.SHAPED_555:
        assert_compiled_in_shape(batch, S.SHAPE_555)
    before4 = engine.get_option("lattice_launches_4")
    try:
        ref = check(oracle, engine, batch, name, modes_of(name))
    finally:
        engine.set_option("lattice_tail", 0)
    assert 0 < colliding(ref) < batch.B * batch.C
    if name in S.SHAPED_997:
        assert engine.get_option("lattice_launches_4") > before4


def device_call(engine, batch, order, skip):
    """fp_plan_dense on a resident batch with the tables asked for; order / skip: host int32 arrays or None."""
    import torch

    from fiss_plus_planner_amd.device_batch import DeviceBatch

    db = DeviceBatch(batch, 0, order_hint=False)
    held = {k: torch.from_numpy(v).to(db.dev) for k, v in (("order", order), ("skip", skip)) if v is not None}
    db.fb.launch_order = held["order"].data_ptr() if "order" in held else None
    db.fb.skip = held["skip"].data_ptr() if "skip" in held else None
    B, C = batch.B, batch.C
    idx, cost1 = torch.full((B,), -7, dtype=torch.int32, device=db.dev), torch.zeros(B, dtype=torch.float64, device=db.dev)
    stats = torch.zeros((B, 4), dtype=torch.int32, device=db.dev)
    cost, flags = torch.zeros((B, C), dtype=torch.float64, device=db.dev), torch.zeros((B, C), dtype=torch.int32, device=db.dev)
    engine.plan_dense_device(db.params, db.fb, idx.data_ptr(), cost1.data_ptr(), stats.data_ptr(), cost.data_ptr(), flags.data_ptr())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), cost1.cpu().numpy(), stats.cpu().numpy(), cost.cpu().numpy(), flags.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", sorted(S.SHAPED_997) + [n for n in S.CASES if n.startswith("5 x 4 x 3")])
def test_scalar_case_under_a_callers_order_with_a_skipped_ego(oracle, engine, name):
    batch = S.CASES[name]()
    ref = [p.fop_plan() for p in oracle.problems_from_batch(batch)]
    try:
        for label, opts, counter in TAIL:
            for k, v in {**RESET_ALL, **opts, "lattice_order": 0}.items():  # (no learnt order: the caller's is the one that is used)
                engine.set_option(k, v)
            for order, skip in ((S.ORDER, None), (S.ORDER, S.SKIP), (None, S.SKIP)):
                before = sum(engine.get_option(c) for c in counter.split("|"))
                idx, cost1, stats, cost, flags = device_call(engine, batch, order, skip)
                assert sum(engine.get_option(c) for c in counter.split("|")) > before, (name, label)
                for e, r in enumerate(ref):
                    what = f"{name} [{label}; order {order is not None}, skip {skip is not None}] ego {e}"
                    if skip is not None and skip[e]:
                        assert idx[e] == -1 and np.isnan(cost1[e]), what
                        continue
                    np.testing.assert_array_equal(flags[e], r.flags, err_msg=what + ": flag words")
                    np.testing.assert_array_equal(stats[e], r.stats, err_msg=what + ": Stats")
                    np.testing.assert_allclose(cost[e], r.cost, rtol=0, atol=COST_TOL, err_msg=what)
                    assert idx[e] == r.best_idx, what
                    assert (np.isnan(cost1[e]) and r.best_idx < 0) or abs(cost1[e] - r.cost[r.best_idx]) <= COST_TOL, what
    finally:
        for k, v in {**RESET_ALL, "lattice_order": 1}.items():
            engine.set_option(k, v)


@pytest.mark.parametrize("name", list(S.FISS_CASES))
def test_fiss_twin_with_its_appended_search(oracle, engine, name):
    """fiss_fused = 1: the lattice launch carries the search workgroups (the FISS instances, three and four per CU); fiss_fused = 0: the
    plain instances and the search in its own launch.  Every output identical; Stats exact and the cost within 1e-9 of the oracle's."""
    from test_gpu_fiss_fused import _run, _same

    batch = S.FISS_CASES[name]()
    ref = [p.fissplus_plan() for p in oracle.problems_from_batch(batch)]
    try:
        for label, opts in (("three per CU", {"resident_groups": 2, "lattice_occupancy": 3}), ("four per CU", {"resident_groups": 2}),
                            ("four per CU, four egos cut in two", {"resident_groups": 2, "lattice_tail": 4}),
                            ("four per CU, no tail split", {"resident_groups": 2, "lattice_tail": 1})):
            for k, v in {**RESET_ALL, **opts}.items():
                engine.set_option(k, v)
            own = _run(engine, batch, 0, None)
            for rep in range(2):
                _same(_run(engine, batch, 1, None), own, f"{name} [{label}] repetition {rep}")
            for e, r in enumerate(ref):
                np.testing.assert_array_equal(own.stats[e], r.stats, err_msg=f"{name} [{label}] ego {e}")
                assert np.isnan(own.best_cost[e]) == np.isnan(r.best_cost), (name, label, e)
                if not np.isnan(r.best_cost):
                    print(f"{name} [{label}] ego {e}: |cost - oracle| = {abs(own.best_cost[e] - r.best_cost):.3e}")
                    assert abs(own.best_cost[e] - r.best_cost) <= COST_TOL, (name, label, e)
    finally:
        for k, v in RESET_ALL.items():
            engine.set_option(k, v)
