#!/usr/bin/env python3
"""Cost of the fallback stop on the headline batch (config 3: 2048 egos x 9x9x7 x 50 obstacles, resident), a family of 5 d x 6 T:
  (a) fp_fallback_stop per launch on the dense pass' own best_idx (the egos without a winner need one), and what the library offered
      for the same answer before: fp_eval_trajs with K = 30 plus fp_traj_margins with K = 30 on those egos (the others skipped), plus
      the copy of both results to pinned host memory - before any host code chooses among them;
  (b) the launch alone on a healthy batch (every ego has a plan: every workgroup returns before it stages anything);
  (c) the unfused FOP closed-loop cycle of 2048 egos (fp_plan_dense + fp_advance) with and without fallback=, over the first cycles of a
      fresh loop (without a fallback the egos that find nothing leave after their first cycle and are skipped from then on; with one
      they stay and are planned every cycle: `running_after` says how many).
One JSON line.  Timing: hip events around `--steps` enqueued calls, `--repeats` times after `--warmup` calls; median and min / max of
the repeats, interleaved in one process."""
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
    ap.add_argument("--egos", type=int, default=2048)
    args = ap.parse_args()
    import torch

    from fiss_plus_planner_amd import _abi, synth
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch
    from fiss_plus_planner_amd.engine import FrenetEngine
    from fiss_plus_planner_amd.fallback import FallbackStop

    eng = FrenetEngine(0)
    batch = synth.make_config(3, B=args.egos)
    db = DeviceBatch(batch, 0)
    B, dev = db.B, db.dev
    i32, f64 = torch.int32, torch.float64
    stream = torch.cuda.current_stream(dev).cuda_stream
    fs = FallbackStop([2.0, 3.0, 4.0, 5.0, 6.0, 8.0], [np.nan, -1.0, -0.5, 0.5, 1.0])
    held = {}

    def addr(name, a):
        held[name] = torch.from_numpy(a).to(dev)
        return held[name].data_ptr()

    st = fs.struct(batch, addr)
    F = st.n_d * st.n_stop
    best_idx, best_cost = torch.empty(B, dtype=i32, device=dev), torch.empty(B, dtype=f64, device=dev)
    eng.plan_dense_device(db.params, db.fb, best_idx.data_ptr(), best_cost.data_ptr(), stream=stream)
    torch.cuda.synchronize(dev)
    bi = best_idx.cpu().numpy()
    healthy_idx = torch.from_numpy(np.where(bi >= 0, bi, 0).astype(np.int32)).to(dev)
    es = torch.full((B, 3), float("nan"), dtype=f64, device=dev)
    o_i = [torch.zeros(B, dtype=i32, device=dev) for _ in range(4)]
    o_v = torch.zeros(B, dtype=f64, device=dev)

    def fallback(idx):
        eng.fallback_stop_device(db.params, db.fb, st, es.data_ptr(), o_i[0].data_ptr(), o_i[1].data_ptr(), o_i[2].data_ptr(), o_i[3].data_ptr(), o_v.data_ptr(),
                                 best_idx=idx.data_ptr(), stream=stream)

    # the parent's route to the same answer: price and measure all F candidates of the egos without a winner, read both back
    d_t = fs.targets(batch)
    d_end = np.where(np.isnan(d_t)[None, :], batch.ego[:, 3:4], d_t[None, :])  # [B, n_d]
    fam = np.zeros((B, F, 3))
    fam[:, :, 0] = np.repeat(d_end, st.n_stop, axis=1)
    fam[:, :, 2] = np.tile(fs.stop_times, st.n_d)[None, :]
    fam_bk = torch.from_numpy(fam).to(dev)                                        # [B][K][3]: fp_eval_trajs
    fam_kb = torch.from_numpy(np.ascontiguousarray(fam.transpose(1, 0, 2))).to(dev)  # [K][B][3]: fp_traj_margins
    has_plan = torch.from_numpy((bi >= 0).astype(np.int32)).to(dev)
    fb_skip = _abi.FpBatch.from_buffer_copy(db.fb)
    fb_skip.skip = has_plan.data_ptr()
    cost, flags = torch.empty((B, F), dtype=f64, device=dev), torch.empty((B, F), dtype=i32, device=dev)
    md, ms, mo = torch.empty((F, B), dtype=f64, device=dev), torch.empty((F, B), dtype=i32, device=dev), torch.empty((F, B), dtype=i32, device=dev)
    h = [torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in (cost, flags, md, ms, mo)]

    def parent_route():
        eng.eval_trajs_device(db.params, fb_skip, F, fam_bk.data_ptr(), cost.data_ptr(), flags.data_ptr(), stream=stream)
        eng.traj_margins_device(db.params, fb_skip, F, md.data_ptr(), ms.data_ptr(), mo.data_ptr(), end_state=fam_kb.data_ptr(), stream=stream)
        for dst, src in zip(h, (cost, flags, md, ms, mo)):
            dst.copy_(src, non_blocking=True)

    def timed(fn, steps, warmup=None):
        for _ in range(args.warmup if warmup is None else warmup):
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

    out = dict(B=B, F=F, steps=args.steps, repeats=args.repeats, need=int((bi < 0).sum()))
    out["fallback_headline"] = timed(lambda: fallback(best_idx), args.steps)
    out["parent_eval_margins_readback"] = timed(parent_route, max(args.steps // 5, 1))
    out["fallback_healthy"] = timed(lambda: fallback(healthy_idx), args.steps)
    fallback(best_idx)
    torch.cuda.synchronize(dev)
    out["status_counts"] = np.bincount(o_i[0].cpu().numpy(), minlength=4).tolist()

    def cycle(fallback_stop):
        """The unfused FOP cycle over the first cycles of a fresh loop."""
        b2 = synth.make_config(3, B=args.egos)
        run = ClosedLoopRunner(eng, DeviceBatch(b2, 0), np.full((B, 2), 1e6), "FOP", fused=False, fallback=fallback_stop)
        ego0, t0 = run.db.t["ego"].clone(), run.db.t["t_now"].clone()

        def step():
            run.step(stream)

        r = timed(step, 5, warmup=1)
        run.db.t["ego"].copy_(ego0)
        run.db.t["t_now"].copy_(t0)
        r["running_after"] = int((run.done == 0).sum().item())
        return r

    out["loop_cycle_plain"] = cycle(None)
    out["loop_cycle_fallback"] = cycle(fs)
    out["fallback_launches"] = eng.get_option("fallback_launches")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
