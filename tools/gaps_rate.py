#!/usr/bin/env python3
"""Cost of the time gap (fp_gap_mask) on the headline batch (2048 egos x 9x9x7 x 50 moving obstacles, resident), lag_follow 20,
lag_lead 10, first 2:
  (a) fp_gap_mask behind a dense call: the call is NOT idempotent in its work (its violators are no longer evaluated), so every timed
      launch runs on the dense call's own flag words, copied back on the device before it; hip events around each launch alone;
  (b) the dense call alone (w_obstacle = 0), hip events around `--steps` enqueued calls;
  (c) clearance_rescore_kernel on the same batch: the dense call with w_obstacle = 0.1, the same way, less (b);
  (d) --lags: (a) with other lags (the cull and the staging stay, the lag walk scales);
  (e) the device-resident closed loop of the same egos, per cycle: ClosedLoopRunner with rules=("gaps",) against rules=() - fused and
      unfused -, eager (wall clock over --cycles enqueued cycles) and replayed from a captured graph, each on a fresh resident batch.
One JSON line.  `--repeats` repetitions after `--warmup` launches; median and min / max."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=40)
    ap.add_argument("--egos", type=int, default=2048)
    ap.add_argument("--follow", type=int, default=20)
    ap.add_argument("--lead", type=int, default=10)
    ap.add_argument("--first", type=int, default=2)
    ap.add_argument("--lags", default="2:0,10:0,20:0,48:48", help="follow:lead pairs of (d)")
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()
    import torch

    from fiss_plus_planner_amd import synth
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch
    from fiss_plus_planner_amd.engine import FrenetEngine, make_params

    eng = FrenetEngine(0)
    make = lambda: dataclasses.replace(synth.make_config(3, B=args.egos), gap_follow=args.follow, gap_lead=args.lead, gap_first=args.first)  # noqa: E731
    host = make()
    db = DeviceBatch(host, 0)
    B, Cn, dev = db.B, db.C, db.dev
    i32, f64 = torch.int32, torch.float64
    best_idx, best_cost = torch.empty(B, dtype=i32, device=dev), torch.empty(B, dtype=f64, device=dev)
    cost, flags = torch.empty((B, Cn), dtype=f64, device=dev), torch.empty((B, Cn), dtype=i32, device=dev)
    m_idx, m_cost, count = torch.empty(B, dtype=i32, device=dev), torch.empty(B, dtype=f64, device=dev), torch.empty(B, dtype=i32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    priced = make_params(dataclasses.replace(host, w_obstacle=0.1))

    def dense(params=db.params):
        eng.plan_dense_device(params, db.fb, best_idx.data_ptr(), best_cost.data_ptr(), cost_tbl=cost.data_ptr(), flag_tbl=flags.data_ptr(), stream=stream)

    def gaps(follow=args.follow, lead=args.lead):
        eng.gap_mask_device(db.params, db.fb, follow, lead, args.first, cost.data_ptr(), flags.data_ptr(), m_idx.data_ptr(), m_cost.data_ptr(), count.data_ptr(), stream=stream)

    def timed_block(call):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize(dev)
        us = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                call()
            b.record()
            torch.cuda.synchronize(dev)
            us.append(a.elapsed_time(b) / args.steps * 1e3)
        return spread(us)

    def timed_gaps(**kw):
        dense()
        torch.cuda.synchronize(dev)
        flags0 = flags.clone()
        us = []
        for rep in range(args.repeats + 1):  # (the first repetition is the warm-up)
            ev = []
            for _ in range(args.steps if rep else args.warmup):
                flags.copy_(flags0)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                gaps(**kw)
                b.record()
                ev.append((a, b))
            torch.cuda.synchronize(dev)
            if rep:
                us.append(float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3)
        return spread(us)

    out = dict(B=B, C=Cn, steps=args.steps, repeats=args.repeats, cycles=args.cycles, follow=args.follow, lead=args.lead, first=args.first)
    out["gap_kernel_us_per_launch"] = timed_gaps()
    fl = flags.cpu().numpy().view(np.uint32)
    out["survivors_on_entry"] = int(B * Cn - np.count_nonzero(fl & 0xF7)) + int(count.cpu().numpy().sum())
    out["flagged"] = int(count.cpu().numpy().sum())
    out["egos_with_a_survivor"] = dict(before=int((best_idx.cpu().numpy() >= 0).sum()), after=int((m_idx.cpu().numpy() >= 0).sum()))
    out["dense_us_per_call"] = timed_block(dense)
    out["dense_with_clearance_us_per_call"] = timed_block(lambda: dense(priced))
    out["clearance_kernel_us_per_launch"] = out["dense_with_clearance_us_per_call"]["median"] - out["dense_us_per_call"]["median"]
    out["gap_kernel_us_per_launch_again"] = timed_gaps()
    out["by_lags"] = {}
    for pair in filter(None, args.lags.split(",")):
        f, l = (int(v) for v in pair.split(":"))
        out["by_lags"][pair] = timed_gaps(follow=f, lead=l)

    if not args.no_loop:
        goal = np.full((B, 2), 1e9)  # never reached; egos that run out of solutions drop out
        loops = {}
        for name, kw in (("rules_gaps", dict(rules=("gaps",))), ("rules_none_fused", dict()), ("rules_none_unfused", dict(fused=False)), ("rules_gaps_again", dict(rules=("gaps",)))):
            eager, graph, running = [], [], 0
            for _ in range(args.repeats):
                run = ClosedLoopRunner(eng, DeviceBatch(make(), 0), goal, **kw)
                run.run(2)  # warm-up of this runner
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                res = run.run(args.cycles)
                eager.append((time.perf_counter() - t0) / args.cycles * 1e6)
                running = int((res.done == 0).sum())
                run = ClosedLoopRunner(eng, DeviceBatch(make(), 0), goal, **kw)
                run.run(2)
                run.run_graph(args.cycles)
                graph.append(run.replay_seconds / max(args.cycles - 1, 1) * 1e6)
            loops[name] = dict(eager_us_per_cycle=spread(eager), graph_us_per_cycle=spread(graph), still_running_after_eager=running)
        out["closed_loop"] = loops
    out["gap_launches"] = eng.get_option("gap_launches")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
