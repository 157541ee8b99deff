#!/usr/bin/env python3
"""Cost of the road-boundary check per plan step on the headline batch (2048 egos x 9x9x7 x 50 obstacles, resident, four batches cycled),
with the corridor of the tests (left = 1.3 + 0.5 sin(knots / 17), right = -(1.1 + 0.4 cos(knots / 23)), margin 0.05; --widen moves both
edges outwards):
  (a) fp_plan_dense with tables                 (--dense-only: nothing but this leg, runs on a checkout without the entry point)
  (b) the same + fp_boundary_mask behind it
  (c) fp_boundary_mask alone, over tables that stay put
  (a) again: the spread of the dense leg within this process
One JSON line.  Timing: hip events around `--steps` enqueued steps, `--repeats` times after `--warmup` steps; median and min / max of
the repeats.  The kernel's own time comes from `rocprofv3 --kernel-trace --stats -- python tools/boundary_rate.py --steps 50 --repeats 1`."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--widen", type=float, default=0.0)
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
    m_idx, m_cost, n_masked = torch.empty(B, dtype=i32, device=dev), torch.empty(B, dtype=f64, device=dev), torch.empty(B, dtype=i32, device=dev)
    edges = []
    for db in dbs:
        k = db.host.knots
        edges.append((torch.from_numpy(1.3 + 0.5 * np.sin(k / 17.0) + args.widen).to(dev), torch.from_numpy(-(1.1 + 0.4 * np.cos(k / 23.0)) - args.widen).to(dev)))
    stream = torch.cuda.current_stream(dev).cuda_stream

    def step(i, dense=True, mask=False):
        db, (left, right) = dbs[i % 4], edges[i % 4]
        if dense:
            eng.plan_dense_device(db.params, db.fb, best_idx.data_ptr(), best_cost.data_ptr(), cost_tbl=cost.data_ptr(), flag_tbl=flags.data_ptr(), stream=stream)
        if mask:
            eng.boundary_mask_device(db.params, db.fb, left.data_ptr(), right.data_ptr(), 0.05, cost.data_ptr(), flags.data_ptr(), m_idx.data_ptr(),
                                     m_cost.data_ptr(), n_masked.data_ptr(), stream=stream)

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

    out = dict(B=B, C=Cn, steps=args.steps, repeats=args.repeats, widen=args.widen, dense_tables=timed())
    out["lattice_launches_per_dense_step"] = eng.get_option("lattice_launches") / float((args.warmup + args.steps * args.repeats))
    if not args.dense_only:
        out["dense_plus_mask"] = timed(mask=True)
        step(0)  # tables of batch 0 that stay put (masking them again rewrites the same bits)
        torch.cuda.synchronize(dev)
        out["mask_alone"] = timed(fixed=True, dense=False, mask=True)
        out["dense_tables_again"] = timed()
        out["boundary_launches"] = eng.get_option("boundary_launches")
        step(0, mask=True)
        torch.cuda.synchronize(dev)
        nm, fl = n_masked.cpu().numpy(), flags.cpu().numpy().view(np.uint32)
        out["masked_share"] = float(nm.sum()) / (B * Cn)
        out["egos_with_a_survivor"] = dict(before=int((best_idx.cpu().numpy() >= 0).sum()), after=int((m_idx.cpu().numpy() >= 0).sum()))
        alive = (fl & (0x7F & ~8)) == 0  # no constraint or collision bit (FP_FLAG_TRUNCATED alone is not infeasible)
        out["masked_among_otherwise_feasible"] = float(np.count_nonzero(alive & ((fl & 128) != 0))) / max(1, int(np.count_nonzero(alive)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
