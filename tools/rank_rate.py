#!/usr/bin/env python3
"""Cost of a ranked short list per plan step on the headline batch (2048 egos x 9x9x7 x 50 obstacles, resident, four batches cycled):
  (a) fp_plan_dense with tables                                  (--dense-only: nothing but this leg, runs on a checkout without the entry point)
  (b) the same + fp_rank_feasible, K = 8 and 64
  (c) what a caller did before: D2H of both tables + the numpy restatement (tests/rank_ref.py) on the host
One JSON line.  Timing: hip events around `--steps` enqueued steps, `--repeats` times after `--warmup` steps; median and min / max of
the repeats.  The kernel's own time comes from `rocprofv3 --kernel-trace --stats -- python tools/rank_rate.py --steps 50 --repeats 1`."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--dense-only", action="store_true")
    ap.add_argument("--host-steps", type=int, default=3)
    args = ap.parse_args()
    import torch

    from fiss_plus_planner_amd import synth
    from fiss_plus_planner_amd.device_batch import DeviceBatch
    from fiss_plus_planner_amd.engine import FrenetEngine

    eng = FrenetEngine(0)
    dbs = [DeviceBatch(synth.make_config(3, ego_offset=2048 * i), 0) for i in range(4)]
    B, Cn = dbs[0].B, dbs[0].C
    dev = dbs[0].dev
    i32, f64 = torch.int32, torch.float64
    best_idx, best_cost = torch.empty(B, dtype=i32, device=dev), torch.empty(B, dtype=f64, device=dev)
    cost, flags = torch.empty((B, Cn), dtype=f64, device=dev), torch.empty((B, Cn), dtype=i32, device=dev)
    ri, rc, nf = torch.empty((64, B), dtype=i32, device=dev), torch.empty((64, B), dtype=f64, device=dev), torch.empty(B, dtype=i32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def step(i, K):
        db = dbs[i % 4]
        eng.plan_dense_device(db.params, db.fb, best_idx.data_ptr(), best_cost.data_ptr(), cost_tbl=cost.data_ptr(), flag_tbl=flags.data_ptr(), stream=stream)
        if K:
            eng.rank_feasible_device(db.params, db.fb, cost.data_ptr(), flags.data_ptr(), K, ri.data_ptr(), rc.data_ptr(), nf.data_ptr(), stream=stream)

    def timed(K):
        for i in range(args.warmup):
            step(i, K)
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(args.steps):
                step(i, K)
            b.record()
            torch.cuda.synchronize(dev)
            ms.append(a.elapsed_time(b) / args.steps)
        return dict(median_ms=float(np.median(ms)), min_ms=min(ms), max_ms=max(ms))

    out = dict(B=B, C=Cn, steps=args.steps, repeats=args.repeats, table_bytes=B * Cn * 12, dense_tables=timed(0))
    if not args.dense_only:
        import rank_ref

        for K in (8, 64):
            out[f"dense_plus_rank_K{K}"] = timed(K)
        out["dense_tables_again"] = timed(0)  # (the spread of leg (a) within this process)
        out["rank_launches"] = eng.get_option("rank_launches")
        h_cost, h_flags = torch.empty((B, Cn), dtype=f64).pin_memory(), torch.empty((B, Cn), dtype=i32).pin_memory()
        for K in (8, 64):
            copy_ms, sort_ms = [], []
            for i in range(args.host_steps):
                step(i, 0)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                h_cost.copy_(cost, non_blocking=True); h_flags.copy_(flags, non_blocking=True)
                torch.cuda.synchronize(dev)
                t1 = time.perf_counter()
                want = rank_ref.rank_tables(h_cost.numpy(), h_flags.numpy().view(np.uint32), K)
                t2 = time.perf_counter()
                copy_ms.append((t1 - t0) * 1e3); sort_ms.append((t2 - t1) * 1e3)
            step(args.host_steps - 1, K)
            torch.cuda.synchronize(dev)
            same = np.array_equal(ri[:K].cpu().numpy(), want[0]) and np.array_equal(nf.cpu().numpy(), want[2])
            out[f"host_readback_K{K}"] = dict(d2h_ms=float(np.median(copy_ms)), numpy_rank_ms=float(np.median(sort_ms)), device_equals_host=bool(same))
        surv = nf.cpu().numpy()
        out["survivors_per_ego"] = dict(mean=float(surv.mean()), max=int(surv.max()), egos_with_any=int((surv > 0).sum()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
