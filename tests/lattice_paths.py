"""How the suites of the fused lattice kernel (fiss_plus_planner_amd/csrc/frenet_lattice_fused.hip) run a case and compare it, in one place.

A case module (prologue_cases, range_argmin_cases, scalar_cases, sure_hit_cases, group_hit_cases, adversarial) builds ProblemBatches and
a `_cpu` file proves with the oracle alone what each one is; this module takes a batch through the kernel's launch paths and holds it
against the oracle.  MODES .. fiss_twin_modes name the paths (label, ctx options, the launch counter that must move), `options` sets
them and puts every option back, `compare` is the one comparison with the oracle, `through_modes`, `shaped_case`,
`device_entry_matches` and `fiss_twins` are the test bodies tests/test_gpu_{adversarial,edges,walk_decode,prologue_paths,range_argmin,
scalar_paths,sure_hit,group_hit}.py call.  A new stage of the kernel brings a case module, its `_cpu` proof and a GPU file of a few
lines that parametrises over the cases and calls shaped_case / device_entry_matches.

A plain helper module: no fixture, no GPU import at module level (tests/test_lattice_paths_cpu.py runs it against a stub engine), and
not rewritten by pytest, so every assertion carries its message."""
import contextlib
import math

import numpy as np

from fiss_plus_planner_amd import _abi
from fiss_plus_planner_amd.engine import make_params

# ---------------------------------------------------------------- shapes and what a reference decides
# (nd, nv, nt, check stride, obstacles, checked rows) of the two shapes the kernel is instantiated for (kLatticeShapes)
SHAPE_997, SHAPE_555 = (9, 9, 7, 2, 50, 25), (5, 5, 5, 2, 10, 50)


def rows_of(batch):
    """Checked pose rows, by the host's own formula (fused_shape, frenet_lattice_plan.h)."""
    cap = make_params(batch).points_max or _abi.FP_FAST_POINTS  # (0: no trajectory of the batch has more than the fast path's points)
    return min(math.ceil(cap / batch.check_stride), math.ceil(batch.T_obs / batch.check_stride))


def shape_of(batch):
    return (batch.nd, batch.nv, batch.nt, batch.check_stride, batch.n_obs, rows_of(batch))


def assert_compiled_in_shape(batch, shape):
    """The batch has one of the two shapes the kernel is instantiated for: the launch planner then names the shaped instance of
    whichever family and occupancy it picks, and with it the packed item code."""
    assert shape_of(batch) == shape, f"shape {shape_of(batch)}, not the compiled-in {shape}"


def coll_of(ref):
    """[B][C]: the candidates the reference finds colliding."""
    return np.stack([(r.flags & 4) != 0 for r in ref])


def colliding(ref):
    return int(coll_of(ref).sum())


def reference(oracle, batch, planner="fop"):
    return [p.fissplus_plan() if planner == "fissplus" else p.fop_plan() for p in oracle.problems_from_batch(batch)]


# ---------------------------------------------------------------- the launch paths: (label, ctx options, the launch counter that must move)
# The multi-round instances (three / four workgroups per compute unit) only run on batches of more than 512 / 768 egos on a whole
# MI355X; "resident_groups" 2 models a one-CU device, so a handful of egos - what the oracle can check in seconds - takes them.
ROUNDS = {"lattice_kernel": 2, "resident_groups": 2}
MODES = [
    ("two per CU, latency split", {"lattice_kernel": 2}, "lattice_launches_2"),
    ("two per CU, one workgroup per ego", {"lattice_kernel": 2, "lattice_split": 1}, "lattice_launches_2"),
    ("three per CU", {**ROUNDS, "lattice_occupancy": 3}, "lattice_launches_3"),
    ("four per CU (slim layout; three when the 40 KB layout does not hold the shape)", ROUNDS, "lattice_launches_4|lattice_launches_3"),
    ("lane per candidate", {"lattice_kernel": 1}, None),
]
TWO_PER_CU = [m for m in MODES if m[2] in ("lattice_launches_2", None)]
# (the automatic tail of a launch this small cuts no ego - an eighth or a quarter of a round of two CUs' worth - so the split is asked for:
# lattice_tail = 4 cuts the last four dispatch slots in two, 1 forbids it)
TAIL = [("three per CU, four egos cut in two", {**ROUNDS, "lattice_occupancy": 3, "lattice_tail": 4}, "lattice_launches_3"),
        ("four per CU, four egos cut in two", {**ROUNDS, "lattice_tail": 4}, "lattice_launches_4|lattice_launches_3"),
        ("three per CU, no tail split", {**ROUNDS, "lattice_occupancy": 3, "lattice_tail": 1}, "lattice_launches_3"),
        ("four per CU, no tail split", {**ROUNDS, "lattice_tail": 1}, "lattice_launches_4|lattice_launches_3")]
GROUPED = [("grouped, 1024 threads", {"lattice_kernel": 2, "lattice_group": 99}, "lattice_launches_2"),
           ("grouped, one workgroup per ego", {"lattice_kernel": 2, "lattice_group": 99, "lattice_split": 1}, "lattice_launches_2")]
# with one ego, or a scene whose layout does not fit a third / quarter of the CU's LDS, the three- and four-per-CU requests run two per CU
# (their counters do not move): the rows of tests/test_gpu_edges.py use these three
EDGE_MODES = [MODES[0], MODES[1], MODES[4]]
# the four-per-CU instances have no polygon variant: a request without a cap runs three per CU
POLY_MODES = [m for m in MODES if "four per CU" not in m[0]] + [("three per CU (no cap)", ROUNDS, "lattice_launches_3")]


def fiss_twin_modes(no_tail_split=False):
    """The FISS+ twin instances (three and four per CU; no counter of their own); the fourth row on request."""
    rows = [("three per CU", {"resident_groups": 2, "lattice_occupancy": 3}, None), ("four per CU", {"resident_groups": 2}, None),
            ("four per CU, four egos cut in two", {"resident_groups": 2, "lattice_tail": 4}, None)]
    return rows + [("four per CU, no tail split", {"resident_groups": 2, "lattice_tail": 1}, None)] * no_tail_split


def modes_for(batch_or_shape, tail=True):
    """The paths a lattice of that size can take.  The 5 x 5 x 5 shape's 50 rows of frames do not fit a third of a CU's LDS: its
    shaped instances run two per CU only."""
    s = batch_or_shape if isinstance(batch_or_shape, tuple) else shape_of(batch_or_shape)
    return TWO_PER_CU if s[:3] == SHAPE_555[:3] else MODES + TAIL * tail


# ---------------------------------------------------------------- ctx options
# every option these suites set, with its default
DEFAULTS = {"lattice_kernel": 0, "lattice_split": 0, "resident_groups": 0, "lattice_occupancy": 0, "lattice_tail": 0, "lattice_group": 0,
            "lattice_winner": 0, "lattice_order": 1, "fiss_fused": 1}


@contextlib.contextmanager
def options(engine, opts):
    """DEFAULTS overlaid with opts inside the block; every option of DEFAULTS back at its default behind it, passed or raised."""
    try:
        for k, v in {**DEFAULTS, **opts}.items():
            engine.set_option(k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            engine.set_option(k, v)


def launches(engine, counter):
    """The sum of the launch counters `counter` names ("a|b": either may move); None names none."""
    return sum(engine.get_option(c) for c in counter.split("|")) if counter else 0


# ---------------------------------------------------------------- the comparison with the oracle
COST_MODES = {"abs1e-9": (1e-9, False), "abs1e-6": (1e-6, False), "relative": (1e-9, True)}  # (tolerance, relative beyond magnitude 1)


def _cost_within(got, want, what, tol, relative):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN where the oracle has a cost, or a cost where it has NaN"
    m = ~np.isnan(want)
    bad = np.abs(got[m] - want[m]) > tol * (np.maximum(1.0, np.abs(want[m])) if relative else 1.0)
    assert not bad.any(), f"{what}: {int(bad.sum())} costs beyond {tol:g}: {got[m][bad][:4]} vs {want[m][bad][:4]}, off by {np.abs(got[m] - want[m])[bad][:4]}"


def cost_close(got, want, what):
    """Costs within 1e-9 of the oracle's (relative beyond magnitude 1: a one-point trajectory's jerk term reaches 1e10); NaN where NaN."""
    _cost_within(got, want, what, *COST_MODES["relative"])


def compare(out, ref, what, *, stats=True, cost="abs1e-9", skip=None):
    """out: a plan_dense result or device_call's five arrays; ref: the oracle's plan per ego.  Flag words, Stats and the selected index
    exact, the cost table and the selected cost within `cost`; an ego of `skip` has idx -1 and cost NaN, whatever its rows hold."""
    idx, best, stats_got, table, flags = out if isinstance(out, tuple) else (out.best_idx, out.best_cost, out.stats, out.cost, out.flags)
    assert len(idx) == len(ref), f"{what}: {len(idx)} egos, the oracle has {len(ref)}"
    for e, r in enumerate(ref):
        w = f"{what} ego {e}"
        if skip is not None and skip[e]:
            assert idx[e] == -1 and np.isnan(best[e]), f"{w}: skipped, yet idx {idx[e]} and cost {best[e]} (not -1 and NaN)"
            continue
        assert flags[e].shape == r.flags.shape, f"{w}: {flags[e].shape} flag words, the oracle has {r.flags.shape}"
        bad = np.nonzero(flags[e] != r.flags)[0]
        if bad.size:
            raise AssertionError(f"{w}: {bad.size} flag words differ, first candidate {bad[0]}: got {flags[e][bad[0]]:#x} want {r.flags[bad[0]]:#x}")
        if stats:
            np.testing.assert_array_equal(stats_got[e], r.stats, err_msg=f"{w}: Stats")
        _cost_within(table[e], r.cost, w, *COST_MODES[cost])
        assert idx[e] == r.best_idx, f"{w}: best_idx {idx[e]}, the oracle's {r.best_idx}"
        _cost_within(best[e], r.cost[r.best_idx] if r.best_idx >= 0 else np.nan, w + ": selected cost", *COST_MODES[cost])


# ---------------------------------------------------------------- the test bodies
def through_modes(oracle_or_ref, engine, batch, what, modes, *, winner=True, planner="fop", stats=True, cost="abs1e-9"):
    """engine.plan_dense through every path of `modes`: each takes its instance (its launch counter moves) and gives the oracle's
    answer.  oracle_or_ref: the oracle, or the list of plans it gave for the batch.  -> that list."""
    ref = oracle_or_ref if isinstance(oracle_or_ref, (list, tuple)) else reference(oracle_or_ref, batch, planner)
    for label, opts, counter in modes:
        with options(engine, opts):
            before = launches(engine, counter)
            out = engine.plan_dense(batch, winner=winner)
            assert not counter or launches(engine, counter) > before, f"{what}: '{label}' did not take its instance"
            compare(out, ref, f"{what} [{label}]", stats=stats, cost=cost)
    return ref


def shaped_case(oracle, engine, batch, what, shape, modes, decides=True):
    """A case through `modes`: with `shape`, the batch has that compiled-in shape, and the 9 x 9 x 7 one takes the slim four-per-CU
    layout (also behind a coefficient window); with `decides`, the oracle finds a colliding and a free candidate.  -> the oracle's plans."""
    if shape is not None:
        assert_compiled_in_shape(batch, shape)
    before4 = engine.get_option("lattice_launches_4")
    ref = through_modes(oracle, engine, batch, what, modes, winner=False)
    if decides:
        assert 0 < colliding(ref) < batch.B * batch.C, f"{what}: {colliding(ref)} of {batch.B * batch.C} candidates collide"
    if shape == SHAPE_997:
        assert engine.get_option("lattice_launches_4") > before4, f"{what}: no four-per-CU launch"
    return ref


def device_call(engine, batch, order, skip):
    """fp_plan_dense on a resident batch with the tables asked for, into arrays no earlier launch has written (the engine's own tables
    keep what the previous path left there, which would hide a candidate that is never written); order / skip: host int32 arrays or
    None.  -> (idx, selected cost, Stats, cost table, flag words)."""
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


def device_entry_matches(engine, batch, ref, what, order=None, skip=None):
    """The device entry point under the options in force, a caller's launch order and skipped egos included, against the oracle."""
    compare(device_call(engine, batch, order, skip), ref, f"{what} [device entry point; order {order is not None}, skip {skip is not None}]", skip=skip)


# ---------------------------------------------------------------- the FISS+ twin instances
FISS_KEYS = ("best_ijk", "stats", "refined", "prev_best_idx", "best_flags")
FISS_FKEYS = ("best_cost", "end_state", "best_traj", "trace")


def fiss_run(engine, batch, fused, prev, **kw):
    """FISS+ with the search appended to the lattice launch (fused = 1) or in its own launch (0)."""
    engine.set_option("fiss_fused", fused)
    try:
        return engine.plan_fiss(batch, "FISS+", prev_best_idx=prev, winner=True, trace=True, **kw)
    finally:
        engine.set_option("fiss_fused", DEFAULTS["fiss_fused"])


def fiss_same(a, b, what):
    """Every output of two FISS+ calls identical."""
    for k in FISS_KEYS:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"{what}: {k}")
    found = ~np.isnan(b.best_cost)
    for k in FISS_FKEYS:
        x, y = getattr(a, k), getattr(b, k)
        if k == "trace":  # (the refinement trace of an ego without a coarse winner is not written)
            x, y = x[found], y[found]
        assert np.array_equal(x, y, equal_nan=True), f"{what}: {k}"


def fiss_twins(oracle, engine, batch, what, modes, repetitions=1):
    """fiss_fused = 1: the lattice launch carries the search workgroups (the FISS instances, three and four per CU); fiss_fused = 0: the
    plain instances and the search in its own launch.  Every output identical; Stats exact and the cost within 1e-9 of the oracle's."""
    ref = reference(oracle, batch, "fissplus")
    for label, opts, _ in modes:
        with options(engine, opts):
            own = fiss_run(engine, batch, 0, None)
            for rep in range(repetitions):
                fiss_same(fiss_run(engine, batch, 1, None), own, f"{what} [{label}] repetition {rep}")
        for e, r in enumerate(ref):
            w = f"{what} [{label}] ego {e}"
            np.testing.assert_array_equal(own.stats[e], r.stats, err_msg=w)
            print(f"{w}: |cost - oracle| = {abs(own.best_cost[e] - r.best_cost):.3e}")
            _cost_within(own.best_cost[e], r.best_cost, w, *COST_MODES["abs1e-9"])
    return ref
