#!/usr/bin/env python3
"""Cost of the plan margins on the headline batch (2048 egos x 9x9x7 x 50 obstacles, resident): for K = 1 and K = 8 planes of
fp_rank_feasible and pose_stride = check_stride and 1,
  (a) fp_traj_margins alone (the planes are ranked once, outside the timed region);
  (b) what a caller did before, in the same process: fp_winner_trajs on each of the K planes plus the copy of those series
      [K][B][16][128] to pinned host memory - before any host geometry.
One JSON line.  Timing: hip events around `--steps` enqueued calls, `--repeats` times after `--warmup` calls; median and min / max of
the repeats.  The kernel's own time comes from `rocprofv3 --kernel-trace --stats -- python tools/margins_rate.py --repeats 1`, taken in
a run of its own."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--readback-steps", type=int, default=5)
    args = ap.parse_args()
    import torch

    from fiss_plus_planner_amd import synth
    from fiss_plus_planner_amd.device_batch import DeviceBatch
    from fiss_plus_planner_amd.engine import FrenetEngine

    eng = FrenetEngine(0)
    db = DeviceBatch(synth.make_config(3), 0)
    B, Cn, dev = db.B, db.C, db.dev
    i32, f64 = torch.int32, torch.float64
    KMAX = 8
    best_idx, best_cost = torch.empty(B, dtype=i32, device=dev), torch.empty(B, dtype=f64, device=dev)
    cost, flags = torch.empty((B, Cn), dtype=f64, device=dev), torch.empty((B, Cn), dtype=i32, device=dev)
    ri, rc = torch.empty((KMAX, B), dtype=i32, device=dev), torch.empty((KMAX, B), dtype=f64, device=dev)
    md, ms, mo = torch.empty((KMAX, B), dtype=f64, device=dev), torch.empty((KMAX, B), dtype=i32, device=dev), torch.empty((KMAX, B), dtype=i32, device=dev)
    series, sflags = torch.empty((KMAX, B, 16, 128), dtype=f64, device=dev), torch.empty((KMAX, B), dtype=i32, device=dev)
    h_series = torch.empty((KMAX, B, 16, 128), dtype=f64).pin_memory()
    stream = torch.cuda.current_stream(dev).cuda_stream
    eng.plan_dense_device(db.params, db.fb, best_idx.data_ptr(), best_cost.data_ptr(), cost_tbl=cost.data_ptr(), flag_tbl=flags.data_ptr(), stream=stream)
    eng.rank_feasible_device(db.params, db.fb, cost.data_ptr(), flags.data_ptr(), KMAX, ri.data_ptr(), rc.data_ptr(), stream=stream)
    torch.cuda.synchronize(dev)

    def margins(K, stride):
        eng.traj_margins_device(db.params, db.fb, K, md.data_ptr(), ms.data_ptr(), mo.data_ptr(), best_idx=ri.data_ptr(), pose_stride=stride, stream=stream)

    def readback(K):
        for k in range(K):
            eng.winner_trajs_device(db.params, db.fb, ri.data_ptr() + 4 * k * B, sflags.data_ptr() + 4 * k * B, series.data_ptr() + 8 * k * B * 16 * 128, stream=stream)
        h_series[:K].copy_(series[:K], non_blocking=True)

    def timed(fn, steps):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize(dev)
        t = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                fn()
            b.record()
            torch.cuda.synchronize(dev)
            t.append(a.elapsed_time(b) / steps)
        return dict(median_ms=float(np.median(t)), min_ms=min(t), max_ms=max(t))

    cs = int(db.params.check_stride)
    out = dict(B=B, C=Cn, steps=args.steps, repeats=args.repeats, check_stride=cs)
    for K in (1, 8):
        for stride in (cs, 1):
            out[f"margins_K{K}_stride{stride}"] = timed(lambda K=K, stride=stride: margins(K, stride), args.steps)
        rb = timed(lambda K=K: readback(K), args.readback_steps)
        out[f"series_readback_K{K}"] = dict(rb, bytes=K * B * 16 * 128 * 8)
        out[f"readback_over_margins_K{K}"] = rb["median_ms"] / out[f"margins_K{K}_stride{cs}"]["median_ms"]
    margins(KMAX, cs)
    torch.cuda.synchronize(dev)
    d = md.cpu().numpy()
    out["plans"] = dict(with_trajectory=int((~np.isnan(d)).sum()), in_contact=int((d == 0).sum()), finite=int(np.isfinite(d).sum()),
                        median_margin_m=float(np.median(d[np.isfinite(d)])) if np.isfinite(d).any() else None)
    out["margin_launches"] = eng.get_option("margin_launches")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
