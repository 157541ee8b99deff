#!/usr/bin/env python3
"""Cost of FISS+ that obeys the road rules (fp_plan_fiss_rules) on the headline FISS+ batch (2048 egos x 9x9x7 x 50 moving obstacles,
resident) with the rule data of tools/rules_eval_rate.py - a wavy speed limit with a lateral bound, two lights per frame, a wavy
corridor, a time gap of 20 / 10 / 2 steps.  Per 2048-ego step, hip events around each step, all in one process, the variants taking
turns within every repetition:
  (a) fp_plan_fiss with fiss_fused = 0 (the search in its own launch, as fp_plan_fiss_rules runs it): the yardstick;
  (b) (a) followed by the four pass launches alone, over a resident copy of the dense tables (the flag words restored before every step,
      outside the timed window: the passes only ever add bits);
  (c) fp_plan_fiss_rules with all four rules, and with the gates only;
  (d) the audited step, the alternative without the call: fp_plan_fiss (asking for best_flags, so with the winner's series) ->
      fp_rules_eval at K = 1.
And the share of egos with rejected > 0 after one enforced call, beside the share of egos whose result the rules changed.
One JSON line.  `--repeats` repetitions of `--steps` steps after `--warmup` (every variant is warmed up)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]


def spread(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--egos", type=int, default=2048)
    args = ap.parse_args()
    import torch

    from rules_eval_rate import with_all_rules

    from fiss_plus_planner_amd import _abi, rules, synth
    from fiss_plus_planner_amd.device_batch import DeviceBatch
    from fiss_plus_planner_amd.engine import FrenetEngine

    eng = FrenetEngine(0)
    eng.set_option("fiss_fused", 0)
    host = with_all_rules(synth.make_config(3, B=args.egos, kind="FISS+"))
    names = tuple(r.name for r in rules.TABLE)
    db = DeviceBatch(host, 0)
    B, Cn, dev = db.B, db.C, db.dev
    stream = torch.cuda.current_stream(dev).cuda_stream
    i32, f64 = torch.int32, torch.float64
    sets = {k: rules.rule_set(host, lambda n: db.t[n].data_ptr(), v) for k, v in (("all", names), ("gates", ("gates",)))}
    passes = [(r, r.struct(host, lambda n: db.t[n].data_ptr())) for r in rules.TABLE]

    prev = torch.full((B, 3), -1, dtype=i32, device=dev)
    o = dict(best_ijk=db.empty((B, 3), i32), best_cost=db.empty(B, f64), end_state=db.empty((B, 3), f64), refined=db.empty(B, i32),
             stats=db.empty((B, 4), i32))
    rejected = torch.zeros(B, dtype=i32, device=dev)
    opts = _abi.FpFissOpts(_abi.FP_FISS_PLUS, 3, 10.0, 0.5)

    def fiss_io(series):
        f = _abi.FpFissIo()
        f.samp_min, f.samp_max, f.samp_res = (db.t[k].data_ptr() for k in ("samp_min", "samp_max", "samp_res"))
        f.prev_best_idx = prev.data_ptr()
        for k, t in o.items():
            setattr(f, k, t.data_ptr())
        if series:
            f.best_flags, f.best_traj, f.traj_stride, f.traj_sparse = best_flags.data_ptr(), best_traj.data_ptr(), _abi.FP_DEFAULT_STRIDE, 1
        return f

    best_flags = torch.zeros(B, dtype=i32, device=dev)
    best_traj = db.empty((B, 16, _abi.FP_DEFAULT_STRIDE), f64)
    io, io_series = fiss_io(False), fiss_io(True)
    # the dense tables the pass launches of (b) run over, and the words they are restored to
    cost_tbl, flag_tbl, flag0 = db.empty((B, Cn), f64), db.empty((B, Cn), i32), db.empty((B, Cn), i32)
    pidx, pcost, pcount = db.empty(B, i32), db.empty(B, f64), db.empty(B, i32)
    eng.plan_dense_device(db.params, db.fb, pidx.data_ptr(), pcost.data_ptr(), cost_tbl=cost_tbl.data_ptr(), flag_tbl=flag0.data_ptr(), stream=stream)
    counts = torch.zeros((B, _abi.FP_RULE_COUNT), dtype=i32, device=dev)

    def plain():
        eng.plan_fiss_device(db.params, db.fb, opts, io, stream=stream)

    def plain_and_passes():
        plain()
        for rule, struct in passes:
            eng._table_pass_device(rule, db.params, db.fb, struct, cost_tbl.data_ptr(), flag_tbl.data_ptr(), pidx.data_ptr(), pcost.data_ptr(), pcount.data_ptr(), stream)

    def enforced(which):
        return lambda: eng.plan_fiss_rules_device(db.params, db.fb, opts, io, sets[which][0], None, rejected.data_ptr(), stream)

    def audited():
        eng.plan_fiss_device(db.params, db.fb, opts, io_series, stream=stream)
        eng.rules_eval_device(db.params, db.fb, sets["all"][0], 1, o["end_state"].data_ptr(), best_flags.data_ptr(), 0, counts.data_ptr(), stream)

    variants = dict(a_plan_fiss=plain, b_plan_fiss_and_passes=plain_and_passes, c_enforced_all=enforced("all"), c_enforced_gates=enforced("gates"),
                    d_audited=audited)
    us = {k: [] for k in variants}
    for rep in range(args.repeats + 1):  # (the first repetition is the warm-up of every variant)
        for name, call in variants.items():
            ev = []
            for _ in range(args.steps if rep else args.warmup):
                prev.fill_(-1)
                flag_tbl.copy_(flag0)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                b.record()
                ev.append((a, b))
            torch.cuda.synchronize(dev)
            if rep:
                us[name].append(float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3)
    out = dict(B=B, C=Cn, steps=args.steps, repeats=args.repeats, rules=names, us_per_step={k: spread(v) for k, v in us.items()})

    # what the rules changed, from one call of each kind on fresh history
    def one(call):
        prev.fill_(-1)
        rejected.zero_()
        call()
        torch.cuda.synchronize(dev)
        return {k: t.cpu().numpy().copy() for k, t in o.items()}, rejected.cpu().numpy().copy()

    free, _ = one(plain)
    for which in ("all", "gates"):
        got, rej = one(enforced(which))
        planned = got["best_ijk"][:, 0] >= 0
        out[f"enforced_{which}"] = dict(planned=int(planned.sum()), planned_unenforced=int((free["best_ijk"][:, 0] >= 0).sum()),
                                        share_rejected=float((rej > 0).mean()), rejected_total=int(rej.sum()),
                                        share_coarse_winner_moved=float((got["best_ijk"] != free["best_ijk"]).any(axis=1).mean()),
                                        share_end_state_changed=float((np.nan_to_num(got["end_state"], nan=-1.0) != np.nan_to_num(free["end_state"], nan=-1.0)).any(axis=1).mean()),
                                        refined=int(got["refined"].sum()))
    out["fiss_rules_calls"] = eng.get_option("fiss_rules_calls")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
