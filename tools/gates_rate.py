#!/usr/bin/env python3
"""Cost of the gates (fp_gate_mask) on the headline batch (2048 egos x 9x9x7 x 50 obstacles, resident), with two lines per frame 25 m and
60 m ahead of the frame's ego whose phases are out of step (closed while (t + 7 f) // 23 is even / (t + 7 f) // 31 is odd), front =
veh_l / 2, no waiver:
  (a) fp_gate_mask alone over tables that stay put (the call is idempotent): the kernel's launch time by events, and beside it
  (b) fp_speed_envelope alone over the same tables (limit = 8.5 + 3.5 sin(knots / 31) m/s, tol 0.05, lateral off), in the same process;
  (c) the device-resident closed loop of the same 2048 egos, per cycle: ClosedLoopRunner with rules=("gates",) (fp_plan_dense ->
      fp_gate_mask -> fp_advance) against rules=() - fused (fp_plan_step, the default) and unfused (fp_plan_dense -> fp_advance) -,
      eager (wall clock over --cycles enqueued cycles) and replayed from a captured graph (replays only), each on a fresh resident batch.
One JSON line.  (a), (b): hip events around `--steps` enqueued launches, `--repeats` times after `--warmup`; median and min / max.
(c): `--repeats` runs of `--cycles` cycles; median and min / max."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def with_gates(batch, ahead=(25.0, 60.0), T_gate=256):
    import dataclasses

    from fiss_plus_planner_amd.spline import gate_bits

    line = np.full((batch.F, len(ahead)), np.nan)
    line[batch.frame_of] = batch.ego[:, :1] + np.asarray(ahead)
    t = np.arange(T_gate)[None, :] + 7 * np.arange(batch.F)[:, None]
    closed = np.stack([(t // 23) % 2 == 0, (t // 31) % 2 == 1], axis=-1)
    return dataclasses.replace(batch, gate_s=line, gate_closed=gate_bits(closed), gate_front=0.5 * batch.veh_l)


def spread(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=40)
    ap.add_argument("--egos", type=int, default=2048)
    args = ap.parse_args()
    import torch

    from fiss_plus_planner_amd import synth
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch
    from fiss_plus_planner_amd.engine import FrenetEngine

    eng = FrenetEngine(0)
    make = lambda: with_gates(synth.make_config(3, B=args.egos))  # noqa: E731
    host = make()
    db = DeviceBatch(host, 0)
    B, Cn, dev = db.B, db.C, db.dev
    i32, f64 = torch.int32, torch.float64
    best_idx, best_cost = torch.empty(B, dtype=i32, device=dev), torch.empty(B, dtype=f64, device=dev)
    cost, flags = torch.empty((B, Cn), dtype=f64, device=dev), torch.empty((B, Cn), dtype=i32, device=dev)
    m_idx, m_cost, count = torch.empty(B, dtype=i32, device=dev), torch.empty(B, dtype=f64, device=dev), torch.empty(B, dtype=i32, device=dev)
    limit = torch.from_numpy(8.5 + 3.5 * np.sin(host.knots / 31.0)).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def dense():
        eng.plan_dense_device(db.params, db.fb, best_idx.data_ptr(), best_cost.data_ptr(), cost_tbl=cost.data_ptr(), flag_tbl=flags.data_ptr(), stream=stream)

    def gates():
        eng.gate_mask_device(db.params, db.fb, db.t["gate_s"].data_ptr(), db.t["gate_closed"].data_ptr(), host.gate_s.shape[1], host.gate_closed.shape[1],
                             host.gate_front, host.gate_max_decel, cost.data_ptr(), flags.data_ptr(), m_idx.data_ptr(), m_cost.data_ptr(), count.data_ptr(), stream=stream)

    def envelope():
        eng.speed_envelope_device(db.params, db.fb, limit.data_ptr(), 0.5 * host.veh_l, 0.05, 0.0, cost.data_ptr(), flags.data_ptr(), m_idx.data_ptr(),
                                  m_cost.data_ptr(), count.data_ptr(), stream=stream)

    def timed(call):
        dense()  # fresh tables (either pass only ORs bits in: running it again rewrites nothing)
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

    out = dict(B=B, C=Cn, steps=args.steps, repeats=args.repeats, cycles=args.cycles)
    out["gate_kernel_us_per_launch"] = timed(gates)
    out["gated_share"] = float(count.cpu().numpy().sum()) / (B * Cn)
    out["egos_with_a_survivor"] = dict(before=int((best_idx.cpu().numpy() >= 0).sum()), after=int((m_idx.cpu().numpy() >= 0).sum()))
    out["envelope_kernel_us_per_launch"] = timed(envelope)
    out["gate_kernel_us_per_launch_again"] = timed(gates)

    goal = np.full((B, 2), 1e9)  # never reached; egos that run out of solutions drop out
    loops = {}
    for name, kw in (("rules_gates", dict(rules=("gates",))), ("rules_none_fused", dict()), ("rules_none_unfused", dict(fused=False)), ("rules_gates_again", dict(rules=("gates",)))):
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
    out["gate_launches"] = eng.get_option("gate_launches")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
