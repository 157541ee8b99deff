#!/usr/bin/env python3
"""Cost of the speed envelope per plan step on the headline batch (2048 egos x 9x9x7 x 50 obstacles, resident, four batches cycled), with
the profile of the tests (limit = 8.5 + 3.5 sin(knots / 31) m/s per segment, front = veh_l / 2, tol 0.05; --max-lat-accel > 0 adds the
lateral check):
  (a) fp_plan_dense with tables                 (--dense-only: nothing but this leg, runs on a checkout without the entry point)
  (b) the same + fp_speed_envelope behind it
  (c) fp_speed_envelope alone, over tables that stay put (the call is idempotent): the kernel's launch time by events
  (d) what the call replaces: both tables read back to the host and masked there with numpy (one step, wall clock, synchronised)
  (a) again: the spread of the dense leg within this process
One JSON line.  Timing: hip events around `--steps` enqueued steps, `--repeats` times after `--warmup` steps; median and min / max of
the repeats.  The kernel's own time comes from `rocprofv3 --kernel-trace --stats -- python tools/envelope_rate.py --steps 50 --repeats 1`."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--max-lat-accel", type=float, default=0.0)
    ap.add_argument("--dense-only", action="store_true")
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
    m_idx, m_cost, n_limited = torch.empty(B, dtype=i32, device=dev), torch.empty(B, dtype=f64, device=dev), torch.empty(B, dtype=i32, device=dev)
    limits = [torch.from_numpy(8.5 + 3.5 * np.sin(db.host.knots / 31.0)).to(dev) for db in dbs]
    front, tol = 0.5 * dbs[0].host.veh_l, 0.05
    stream = torch.cuda.current_stream(dev).cuda_stream

    def step(i, dense=True, envelope=False):
        db = dbs[i % 4]
        if dense:
            eng.plan_dense_device(db.params, db.fb, best_idx.data_ptr(), best_cost.data_ptr(), cost_tbl=cost.data_ptr(), flag_tbl=flags.data_ptr(), stream=stream)
        if envelope:
            eng.speed_envelope_device(db.params, db.fb, limits[i % 4].data_ptr(), front, tol, args.max_lat_accel, cost.data_ptr(), flags.data_ptr(),
                                      m_idx.data_ptr(), m_cost.data_ptr(), n_limited.data_ptr(), stream=stream)

    def timed(fixed=False, **kw):
        for i in range(args.warmup):
            step(0 if fixed else i, **kw)
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(args.steps):
                step(0 if fixed else i, **kw)
            b.record()
            torch.cuda.synchronize(dev)
            ms.append(a.elapsed_time(b) / args.steps)
        return dict(median_ms=float(np.median(ms)), min_ms=min(ms), max_ms=max(ms))

    out = dict(B=B, C=Cn, steps=args.steps, repeats=args.repeats, max_lat_accel=args.max_lat_accel, dense_tables=timed())
    out["lattice_launches_per_dense_step"] = eng.get_option("lattice_launches") / float((args.warmup + args.steps * args.repeats))
    if not args.dense_only:
        out["dense_plus_envelope"] = timed(envelope=True)
        step(0)  # tables of batch 0 that stay put (the call only ORs bits in: running it again rewrites nothing)
        torch.cuda.synchronize(dev)
        out["envelope_alone"] = timed(fixed=True, dense=False, envelope=True)
        out["dense_tables_again"] = timed()
        out["envelope_launches"] = eng.get_option("envelope_launches")
        # (d) the host's way: read both tables back, OR per-profile bits in with numpy (the verdicts taken as given: the lower bound of the
        # host path), argmin
        step(0, envelope=True)
        torch.cuda.synchronize(dev)
        fl_dev = flags.cpu().numpy().view(np.uint32)
        step(0)
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(5):
            t0 = time.perf_counter()
            c_h, f_h = cost.cpu().numpy(), flags.cpu().numpy().view(np.uint32)
            f_h = f_h | (fl_dev & 3)
            alive = ((f_h & (0xFF & ~8)) == 0) & ~np.isnan(c_h)
            np.where(alive, c_h, np.inf).argmin(axis=1)
            ms.append((time.perf_counter() - t0) * 1e3)
        out["host_readback_and_mask_ms"] = dict(median_ms=float(np.median(ms)), min_ms=min(ms), max_ms=max(ms))
        step(0, envelope=True)
        torch.cuda.synchronize(dev)
        nl = n_limited.cpu().numpy()
        out["limited_share"] = float(nl.sum()) / (B * Cn)
        out["egos_with_a_survivor"] = dict(before=int((best_idx.cpu().numpy() >= 0).sum()), after=int((m_idx.cpu().numpy() >= 0).sum()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
