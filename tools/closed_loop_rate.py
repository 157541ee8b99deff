#!/usr/bin/env python3
"""Plan cycles per second of the device-resident closed loop (eager launches vs one captured HIP graph replayed).

    python tools/closed_loop_rate.py [--egos 256] [--cycles 40] [--planner FOP] [--config 3] [--log]

--config N: the egos of BASELINE configs[N-1] (synth.make_config) instead of the 5 x 5 x 5 default.
--log: what the driven trajectory costs - per cycle, in one process: (a) the plain loop, (b) the loop with the device log
(run(record=True): fp_loop_record behind every step), (c) the host-traced loop (run(trace=True): five blocking read-backs per cycle),
then the captured graph with and without the log.  Every variant is warmed up and timed --repeat times; the median is printed.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fiss_plus_planner_amd import synth  # noqa: E402
from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch  # noqa: E402
from fiss_plus_planner_amd.engine import FrenetEngine  # noqa: E402


def make(args):
    if args.config:
        return synth.make_config(args.config, B=args.egos, kind=args.planner)
    return synth.make_batch(args.egos, 5, 5, 5, 10, 100, False, 99, kind=args.planner)


def log_cost(eng, args):
    goal = np.full((args.egos, 2), 1e9)  # never reached; egos that run out of solutions drop out the same way in every variant
    variants = (("a plain", dict()), ("b record", dict(record=True)), ("c trace", dict(trace=True)), ("a plain again", dict()))
    for name, kw in variants:
        us = []
        for _ in range(args.repeat):
            run = ClosedLoopRunner(eng, DeviceBatch(make(args), 0), goal, args.planner)
            run.run(2, **kw)  # warm-up of this runner (first-use allocations; with record: the log's too)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run.run(args.cycles, **kw)
            us.append((time.perf_counter() - t0) / args.cycles * 1e6)
        print(f"eager {name:14s} {args.planner} B={args.egos}: median {np.median(us):8.1f} us/cycle  (min {min(us):.1f}, max {max(us):.1f}; "
              f"{args.repeat} x {args.cycles} cycles, completed ego-cycles {int(out.cycles.sum())}, still running {int((out.done == 0).sum())})", flush=True)
    for name, kw in (("a plain", dict()), ("b record", dict(record=True))):
        us = []
        for _ in range(args.repeat):
            run = ClosedLoopRunner(eng, DeviceBatch(make(args), 0), goal, args.planner)
            run.run(2)
            run.run_graph(args.cycles, **kw)
            us.append(run.replay_seconds / max(args.cycles - 1, 1) * 1e6)
        print(f"graph {name:14s} {args.planner} B={args.egos}: median {np.median(us):8.1f} us/cycle  (min {min(us):.1f}, max {max(us):.1f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--egos", type=int, default=256)
    ap.add_argument("--cycles", type=int, default=40)
    ap.add_argument("--planner", default="FOP")
    ap.add_argument("--config", type=int, default=0)
    ap.add_argument("--log", action="store_true")
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    eng = FrenetEngine(0)
    if args.log:
        return log_cost(eng, args)
    for mode in ("eager", "graph"):
        batch = make(args)
        goal = np.full((args.egos, 2), 1e9)  # never reached: every ego runs all cycles
        run = ClosedLoopRunner(eng, DeviceBatch(batch, 0), goal, args.planner)
        run.run(2)  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run.run_graph(args.cycles) if mode == "graph" else run.run(args.cycles)
        dt = time.perf_counter() - t0
        if mode == "graph":
            dt = run.replay_seconds * args.cycles / max(args.cycles - 1, 1)  # replays only (capture + instantiate excluded)
        n = int(out.cycles.sum())
        print(f"{mode:6s} {args.planner} B={args.egos}: {args.cycles} cycles in {dt * 1e3:.2f} ms -> {dt / args.cycles * 1e6:.1f} us/cycle, "
              f"{args.egos * args.cycles / dt / 1e6:.2f} M ego-plans/s (completed cycles {n})")


if __name__ == "__main__":
    main()
