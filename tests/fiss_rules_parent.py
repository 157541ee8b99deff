"""The fp_plan_fiss_rules calls whose outputs tests/golden/fiss_rules_parent.npz pins: recorded on the commit before the refinement's
rule instance became a caller of frenet_rules.h (its own copy of the rule evaluation, the kernel body a twice-included header).  The
same function produced the recording and reproduces it (tests/test_gpu_fiss_rules.py compares the arrays exactly).

    python tests/fiss_rules_parent.py        # on a GPU, with the library to record: writes the file

Cases, all batches of tests/fiss_rules_ref.py: small with all four rules and with each rule alone, wide, long and silent_long (the
four-points-per-lane instance) with all four, small with all four on clocks t_now > 0 - each under FISS and FISS+, with a search history
and the trace; the winner's series where SERIES says so (unchanged code behind an end state that is compared anyway: three cases keep
the file small); and the closed loop at the red light, whose hand-over runs inside the rule instance.

While recording, a FISS+ case whose rules can speak must have an ego with rejected > 0, and with the gap rule a consumed candidate that
got FP_FLAG_COLLISION from it.  (FISS runs no refinement and silent_long's rules cannot speak: their `rejected` is all zero by
construction, and is recorded as that.)  With ALL FOUR rules on, no batch of the file gets there: the gaps run last and only on a word
the other three left feasible, and on these batches a consumed candidate that reaches them passes them (small, long, small on its
clocks: rejected > 0, no gap collision; wide: the rules move the coarse winners and then reject nothing).  Those four cases are recorded
as they are, named in ALL_FOUR_QUIET, and each batch has a companion with fewer rules in front of the gaps that meets both conditions."""
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (run as a script)
    sys.path.insert(0, ROOT)

import fiss_rules_ref as FR  # noqa: E402

NAMES = FR.NAMES
KEYS = ("best_ijk", "prev_best_idx", "end_state", "best_cost", "refined", "stats", "rejected")
T_NOW = (3, 17, 40, 8, 25, 0, 11, 33, 5, 21, 2, 14)  # small's twelve egos, each on its own clock
CASES = ([("small", names, 0) for names in (NAMES,) + tuple((n,) for n in NAMES)] +
         [("wide", NAMES, 0), ("long", NAMES, 0), ("silent_long", NAMES, 0), ("small", NAMES, 1)] +
         # the companions: the gaps speak behind other rules
         [("small", ("envelope", "gates", "gaps"), 0), ("small", ("envelope", "boundary", "gaps"), 0), ("small", ("gates", "boundary", "gaps"), 1),
          ("wide", ("gates", "boundary", "gaps"), 0), ("long", ("boundary", "gaps"), 0)])
ALL_FOUR_QUIET = {("small", 0): "rejected", ("long", 0): "rejected", ("small", 1): "rejected", ("wide", 0): None}  # what the all-four case still has
SERIES = {("small", NAMES, 0), ("long", NAMES, 0), ("small", NAMES, 1)}  # with FISS+: the winner's series and flag words too
LOOP_KEYS = ("ego", "t_now", "done", "cycles", "rejected")


def label(name, names, clock, kind):
    return f"{name}{' t_now' if clock else ''} {'+'.join(names)} {kind}"


def batch_of(name, clock):
    b = FR.case(name)
    return dataclasses.replace(b, t_now=np.array(T_NOW[:b.B], dtype=b.t_now.dtype)) if clock else b


def history(b, seed=5):
    rng = np.random.default_rng(seed)
    return np.where(rng.uniform(size=(b.B, 1)) < 0.5, -1, np.column_stack([rng.integers(0, b.nd, b.B), rng.integers(0, b.nv, b.B),
                                                                          rng.integers(0, b.nt, b.B)])).astype(np.int32)


def plan(engine, batch, kind, names, series):
    kw = dict(winner=True, traj_stride=256) if series else {}
    return engine.plan_fiss(batch, kind, prev_best_idx=history(batch), trace=True, enforce=names, **kw)


def run_all(engine):
    """-> {"<case>/<key>": array}"""
    import gates_ref as GR
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch

    out = {}
    for name, names, clock in CASES:
        for kind in ("FISS", "FISS+"):
            series = kind == "FISS+" and (name, names, clock) in SERIES
            got = plan(engine, batch_of(name, clock), kind, names, series)
            keys = KEYS + (("trace",) if kind == "FISS+" else ()) + (("best_flags", "best_traj") if series else ())
            for k in keys:
                out[f"{label(name, names, clock, kind)}/{k}"] = np.ascontiguousarray(getattr(got, k))
            if kind == "FISS+":  # (the call writes no trace for an ego without a coarse winner: whatever the buffer held)
                out[f"{label(name, names, clock, kind)}/trace"][got.best_ijk[:, 0] < 0] = np.nan
    batch = FR.loop_batch()
    res = ClosedLoopRunner(engine, DeviceBatch(batch, 0), np.full((batch.B, 2), 1e6), planner="FISS+", enforce=("gates",)).run(GR.LOOP_CYCLES)
    for k in LOOP_KEYS:
        out[f"loop gates FISS+/{k}"] = np.ascontiguousarray(getattr(res, k))
    return out


def gap_collisions_consumed(engine, batch, names, got):
    """Candidates of the call `got` that the refinement consumed, that are feasible by their own word and whose word after the rules
    carries FP_FLAG_COLLISION: only the gap rule gives that bit."""
    from fiss_plus_planner_amd import _abi

    found = got.best_ijk[:, 0] >= 0
    filler = np.column_stack([np.full(batch.B, batch.d_samples[0]), batch.v_samples[:, 0], np.full(batch.B, batch.t_samples[0])])[:, None, :]
    es = np.where(found[:, None, None] & ~np.isnan(got.trace[:, :, 3:4]), got.trace[:, :, :3], filler)
    base = engine.eval_trajs(batch, es).flags
    ruled = engine.rules_eval(batch, es, base, rules=names).flags
    still = dataclasses.replace(batch, samp_res=np.zeros_like(batch.samp_res))  # (every probe IS the coarse winner: row 0 prices it)
    coarse = engine.plan_fiss(still, "FISS+", prev_best_idx=history(batch), max_refine_iters=1, trace=True, enforce=names).trace[:, 0, 3]
    n = 0
    for e in np.flatnonzero(found):
        cost = got.trace[e, :, 3]
        for c in sorted(np.flatnonzero(~np.isnan(cost)), key=lambda c: (cost[c], c)):
            if cost[c] > coarse[e]:
                break
            word = ruled[e, c] if not base[e, c] & _abi.FLAG_INFEASIBLE else base[e, c]
            n += bool(not base[e, c] & _abi.FLAG_INFEASIBLE and ruled[e, c] & _abi.FLAG_COLLISION)
            if not word & _abi.FLAG_INFEASIBLE:
                break  # the winner
    return n


def record(engine, path):
    out = run_all(engine)
    missing = []
    for name, names, clock in CASES:
        if name.startswith("silent"):
            continue
        what = label(name, names, clock, "FISS+")
        rejected = out[f"{what}/rejected"]
        hits = None
        if "gaps" in names:
            batch = batch_of(name, clock)
            hits = gap_collisions_consumed(engine, batch, names, plan(engine, batch, "FISS+", names, False))
        print(f"{what}: rejected {int(rejected.sum())}, consumed candidates the gaps rejected {hits}")
        if names == NAMES:  # (see the module's text)
            assert hits == 0 and (rejected > 0).any() == (ALL_FOUR_QUIET[(name, clock)] == "rejected"), what
        elif not (rejected > 0).any() or hits == 0:
            missing.append(what)
    assert not missing, missing  # a case that does not reach the rule evaluation pins nothing: take another batch of the file for it
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    from fiss_plus_planner_amd.engine import FrenetEngine

    record(FrenetEngine(0), sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "fiss_rules_parent.npz"))
