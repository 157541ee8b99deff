#!/usr/bin/env python3
"""Cost of the rule verdicts of explicit end states (fp_rules_eval) on the headline FISS+ batch (2048 egos x 9x9x7 x 50 moving
obstacles, resident) with all four rules on - a wavy speed limit with a lateral bound, two lights per frame, a wavy corridor, a time
gap of 20 / 10 / 2 steps:
  (a) the kernel per launch at K = 1 (fp_plan_fiss' winner: the first trajectory of every ego is the end state a FISS+ call returned)
      and at K = 22 (the winner plus a full refinement trace's worth of random end states inside the sampling box): hip events around
      each launch alone; the gaps' work is not idempotent (their violators are no longer evaluated), so every timed launch runs on
      fp_eval_trajs' own flag words, copied back on the device before it;
  (b) in the same process, the only way to the same answer without the call: fp_eval_trajs writing the K series (dump) and their
      read-back to the host, where the rules would then be evaluated - hip events around the kernel, a host clock around the copy;
  (c) the device-resident closed loop per cycle: ClosedLoopRunner(planner="FISS+", audit=all four) against the same unfused loop
      without audit, eager (wall clock over --cycles enqueued cycles) and replayed from a captured graph, each on a fresh resident batch.
One JSON line.  `--repeats` repetitions of `--steps` launches after `--warmup`; median and min / max."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def spread(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def with_all_rules(batch):
    """The batch with data for the four rules (the shapes of the test batches, on this batch's own lines)."""
    from fiss_plus_planner_amd.spline import gate_bits

    k = np.where(np.isfinite(batch.knots), batch.knots, 0.0)
    line = np.full((batch.F, 2), np.nan)
    line[np.asarray(batch.frame_of)] = batch.ego[:, :1] + np.array([25.0, 60.0])
    t = np.arange(128)[None, :, None] + 7 * np.arange(batch.F)[:, None, None]
    closed = ((t // np.array([23, 31])[None, None, :]) % 2) == np.arange(2)[None, None, :]
    return dataclasses.replace(batch, speed_limit=8.5 + 3.5 * np.sin(k / 31.0), limit_front=0.5 * batch.veh_l, limit_tol=0.05, max_lat_accel=0.1,
                               gate_s=line, gate_closed=gate_bits(closed), gate_front=0.5 * batch.veh_l, gate_max_decel=0.0,
                               bound_left=1.65 + 0.5 * np.sin(k / 17.0), bound_right=-(1.45 + 0.4 * np.cos(k / 23.0)), bound_margin=0.05,
                               gap_follow=20, gap_lead=10, gap_first=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cycles", type=int, default=40)
    ap.add_argument("--egos", type=int, default=2048)
    ap.add_argument("--ks", default="1,22")
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()
    import torch

    from fiss_plus_planner_amd import _abi, rules, synth
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch
    from fiss_plus_planner_amd.engine import TRAJ_STRIDE, FrenetEngine

    eng = FrenetEngine(0)
    make = lambda: with_all_rules(synth.make_config(3, B=args.egos, kind="FISS+"))  # noqa: E731
    host = make()
    names = tuple(r.name for r in rules.TABLE)
    db = DeviceBatch(host, 0)
    B, dev = db.B, db.dev
    stream = torch.cuda.current_stream(dev).cuda_stream
    rule_set, structs = rules.rule_set(host, lambda k: db.t[k].data_ptr(), names)
    winner = eng.plan_fiss(host, "FISS+").end_state
    rng = np.random.default_rng(1)
    out = dict(B=B, C=db.C, steps=args.steps, repeats=args.repeats, cycles=args.cycles, rules=names, planned=int((~np.isnan(winner[:, 0])).sum()), by_K={})

    for K in (int(v) for v in args.ks.split(",")):
        es_h = host.samp_min[:, None, :] + (host.samp_max - host.samp_min)[:, None, :] * rng.random((B, K, 3))
        es_h[:, 0] = winner
        es = torch.from_numpy(es_h).to(dev)
        cost = torch.empty((B, K), dtype=torch.float64, device=dev)
        flags0 = torch.empty((B, K), dtype=torch.int32, device=dev)
        traj = torch.empty((B, K, 16, TRAJ_STRIDE), dtype=torch.float64, device=dev)
        eng.eval_trajs_device(db.params, db.fb, K, es.data_ptr(), cost.data_ptr(), flags0.data_ptr(), stream=stream)
        torch.cuda.synchronize(dev)
        flags, bits = flags0.clone(), torch.empty((B, K), dtype=torch.int32, device=dev)
        counts = torch.zeros((B, _abi.FP_RULE_COUNT), dtype=torch.int32, device=dev)

        def verdict():
            eng.rules_eval_device(db.params, db.fb, rule_set, K, es.data_ptr(), flags.data_ptr(), bits.data_ptr(), counts.data_ptr(), stream)

        def series():
            eng.eval_trajs_device(db.params, db.fb, K, es.data_ptr(), cost.data_ptr(), flags.data_ptr(), traj.data_ptr(), stream=stream)

        def per_launch(call):
            us = []
            for rep in range(args.repeats + 1):  # (the first repetition is the warm-up)
                ev = []
                for _ in range(args.steps if rep else args.warmup):
                    flags.copy_(flags0)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    call()
                    b.record()
                    ev.append((a, b))
                torch.cuda.synchronize(dev)
                if rep:
                    us.append(float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3)
            return spread(us)

        row = dict(rules_eval_us_per_launch=per_launch(verdict))
        row["violating"] = {n: int(np.count_nonzero(bits.cpu().numpy().view(np.uint32) & rules.BITS[n])) for n in names}
        row["eval_trajs_dump_us_per_launch"] = per_launch(series)
        back = []
        pinned = torch.empty(traj.shape, dtype=traj.dtype, pin_memory=True)
        for _ in range(3):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            pinned.copy_(traj)
            torch.cuda.synchronize(dev)
            back.append((time.perf_counter() - t0) * 1e6)
        row["series_read_back_us"] = spread(back[1:])
        row["series_bytes"] = int(traj.numel() * 8)
        row["rules_eval_us_per_launch_again"] = per_launch(verdict)
        out["by_K"][str(K)] = row
        del traj, pinned

    if not args.no_loop:
        goal = np.full((B, 2), 1e9)  # never reached; egos that run out of solutions drop out
        loops = {}
        for name, kw in (("audit", dict(audit=names)), ("unfused", dict(fused=False)), ("fused", dict()), ("audit_again", dict(audit=names))):
            eager, graph, running = [], [], 0
            for _ in range(3):
                run = ClosedLoopRunner(eng, DeviceBatch(make(), 0), goal, planner="FISS+", **kw)
                run.run(2)  # warm-up of this runner
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                res = run.run(args.cycles)
                eager.append((time.perf_counter() - t0) / args.cycles * 1e6)
                running = int((res.done == 0).sum())
                run = ClosedLoopRunner(eng, DeviceBatch(make(), 0), goal, planner="FISS+", **kw)
                run.run(2)
                run.run_graph(args.cycles)
                graph.append(run.replay_seconds / max(args.cycles - 1, 1) * 1e6)
            loops[name] = dict(eager_us_per_cycle=spread(eager), graph_us_per_cycle=spread(graph), still_running_after_eager=running)
            if kw.get("audit"):
                loops[name]["violations"] = {n: int(v.sum()) for n, v in res.violations.items()}
        out["closed_loop"] = loops
    out["rules_eval_launches"] = eng.get_option("rules_eval_launches")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
