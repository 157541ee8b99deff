"""The call WITHOUT tables through the launch paths of tests/lattice_paths.py, held against the oracle.

lattice_paths.compare needs the cost table and the flag words; fp_plan_dense with neither requested - what the headline workload asks
for, and the only call on which stage W of the lattice kernel skips the assembly - leaves the selected index, the selected cost and
Stats.  This module makes that call through the same rows of (label, ctx options, the launch counter that must move) and compares those
three.  A plain helper module like lattice_paths: no fixture, no GPU import at module level, every assertion carries its message."""
import numpy as np

import lattice_paths as L

TOL = L.COST_MODES["abs1e-9"][0]


def quiet_call(engine, batch):
    """fp_plan_dense on a resident batch with NO table requested, into arrays no earlier launch has written.
    -> (idx, selected cost, Stats)."""
    import torch

    from fiss_plus_planner_amd.device_batch import DeviceBatch

    db = DeviceBatch(batch, 0, order_hint=False)
    idx, cost = torch.full((batch.B,), -7, dtype=torch.int32, device=db.dev), torch.zeros(batch.B, dtype=torch.float64, device=db.dev)
    stats = torch.full((batch.B, 4), -7, dtype=torch.int32, device=db.dev)
    engine.plan_dense_device(db.params, db.fb, idx.data_ptr(), cost.data_ptr(), stats.data_ptr())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), cost.cpu().numpy(), stats.cpu().numpy()


def quiet_compare(out, ref, what):
    """out: quiet_call's three arrays; ref: the oracle's plan per ego.  The selected index and Stats exact, the selected cost within
    1e-9 of the oracle's, NaN where it has none."""
    idx, cost, stats = out
    assert len(idx) == len(ref), f"{what}: {len(idx)} egos, the oracle has {len(ref)}"
    for e, r in enumerate(ref):
        w = f"{what} ego {e}"
        assert idx[e] == r.best_idx, f"{w}: best_idx {idx[e]}, the oracle's {r.best_idx}"
        if r.best_idx < 0:
            assert np.isnan(cost[e]), f"{w}: selected cost {cost[e]} where the oracle has none"
        else:
            want = float(r.cost[r.best_idx])
            assert abs(cost[e] - want) <= TOL, f"{w}: selected cost {cost[e]} vs {want}, off by {abs(cost[e] - want):.3e} (beyond {TOL:g})"
        np.testing.assert_array_equal(stats[e], r.stats, err_msg=f"{w}: Stats")


def quiet_matches(engine, batch, ref, what, modes):
    """The call without tables through every path of `modes`: each takes its instance (its launch counter moves) and gives the oracle's
    selection."""
    for label, opts, counter in modes:
        with L.options(engine, opts):
            before = L.launches(engine, counter)
            out = quiet_call(engine, batch)
            assert not counter or L.launches(engine, counter) > before, f"{what}: '{label}' did not take its instance"
        quiet_compare(out, ref, f"{what} [{label}, no tables]")
