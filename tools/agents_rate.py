#!/usr/bin/env python3
"""Cost of sharing plans on the device (fp_obstacles_from_plans) against the host route it replaces, on the headline batch (config 3:
2048 egos, 50 obstacles) attached in groups of 8 at n_rows = 64 (2048 x 8 x 64 x 32 B = 33.5 MB written per call):
  --part a   the new launch on the resident batch: time per launch and GB/s written (obstacles_predict_kernel: 3.4 TB/s, materialise
             mode: 5.2 TB/s)
  --part b   the route it replaces, per cycle: fp_eval_trajs with series on the device, the read-back of B x 16 x stride doubles, the
             numpy scatter into pose rows, the upload of the table from pinned memory (wall clock, it contains a host round trip)
  --part c   the closed-loop cycle (FOP, unfused, no fallback) on that batch with and without agents=, eager and from a graph
  --part d   the cycle without agents on the plain config-3 batch, fused and unfused, eager and from a graph - the part that also runs
             on a tree from before the feature (--root): what shows that the existing cycle did not move
One JSON line per part.  Timing: hip events around `--steps` enqueued calls, `--repeats` times after `--warmup`; median and min / max of
the repeats.  Run each part as its own process under its own time limit."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices="abcd", required=True)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--egos", type=int, default=2048)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--root", default=ROOT, help="the tree whose package is measured")
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.root)]
    import torch

    from fiss_plus_planner_amd import _abi, synth
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch
    from fiss_plus_planner_amd.engine import FrenetEngine

    eng = FrenetEngine(0)
    B, g, rows = args.egos, args.group, args.rows
    plain = synth.make_config(3, B=B)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def timed(fn, steps=args.steps):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                fn()
            b.record()
            torch.cuda.synchronize(dev)
            ms.append(a.elapsed_time(b) / steps)
        return dict(median_us=float(np.median(ms)) * 1e3, min_us=min(ms) * 1e3, max_us=max(ms) * 1e3)

    def cycles(make_runner):
        """us per cycle of a fresh runner: eager (events around --steps steps) and from a graph (replay wall clock)"""
        res = []
        for _ in range(args.repeats):
            r = make_runner()
            for _ in range(args.warmup):
                r.step(stream)
            torch.cuda.synchronize(dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                r.step(stream)
            b.record()
            torch.cuda.synchronize(dev)
            res.append(a.elapsed_time(b) / args.steps * 1e3)
        gr = []
        for _ in range(args.repeats):
            r = make_runner()
            r.run_graph(args.steps + 1)
            gr.append(r.replay_seconds / args.steps * 1e6)
        return dict(eager_us=dict(median=float(np.median(res)), min=min(res), max=max(res)), graph_us=dict(median=float(np.median(gr)), min=min(gr), max=max(gr)))

    goal = np.full((B, 2), 1e6)
    out = dict(part=args.part, egos=B, steps=args.steps, repeats=args.repeats, root=os.path.abspath(args.root))
    if args.part == "d":
        for fused in (True, False):
            out["fop_fused" if fused else "fop_unfused"] = cycles(lambda: ClosedLoopRunner(eng, DeviceBatch(synth.make_config(3, B=B)), goal, "FOP", fused=fused))
        print(json.dumps(out))
        return
    from fiss_plus_planner_amd.agents import AgentGroups

    ag = AgentGroups([list(range(i, min(i + g, B))) for i in range(0, B, g)], rows, "coast", col_base=plain.n_obs)
    T_obs = 96  # (rows t_now .. t_now + 63 of the cycles a measurement drives stay inside the table)

    def attached():
        return ag.attach(synth.make_config(3, B=B), T_obs)

    batch = attached()
    written = B * g * rows * 32
    out.update(group=g, n_rows=rows, T_obs=T_obs, n_obs=batch.n_obs, scenes=batch.S, written_mb=written / 1e6)
    if args.part in "ab":
        db = DeviceBatch(batch)
        bi = db.empty(B, torch.int32)
        bc = db.empty(B, torch.float64)
        eng.plan_dense_device(db.params, db.fb, bi.data_ptr(), bc.data_ptr(), stream=stream)
        torch.cuda.synchronize(dev)
        idx = bi.cpu().numpy()
        idx = np.where(idx < 0, 0, idx)  # (every ego shares some plan: the cost does not depend on which)
        bi.copy_(torch.from_numpy(idx))
        out["egos_with_a_plan"] = int((idx >= 0).sum())
    if args.part == "a":
        held = {}

        def addr(name, a):
            held[name] = torch.from_numpy(a).to(dev)
            return held[name].data_ptr()

        st = ag.struct(batch, addr)
        k = timed(lambda: eng.share_plans_device(db.params, db.fb, st, bi.data_ptr(), 0, db.t["obs_pose"].data_ptr(), db.t["final_time_step"].data_ptr(), stream), steps=50)
        k["gb_per_s_written"] = written / 1e9 / (k["median_us"] / 1e6)
        out["from_plans_kernel"] = k
        out["from_plans_launches"] = eng.get_option("from_plans_launches")
    if args.part == "b":
        stride = 128
        es = np.stack([batch.d_samples[idx // (batch.nv * batch.nt)], batch.v_samples[np.arange(B), idx % batch.nv], batch.t_samples[(idx // batch.nv) % batch.nt]], axis=1)
        d_es = torch.from_numpy(np.ascontiguousarray(es)).to(dev)
        cost, flags = db.empty(B, torch.float64), db.empty(B, torch.int32)
        traj = db.empty((B, 16, stride), torch.float64)
        S0 = plain.S  # the members' scenes are the ones behind the batch's own: only they travel
        table = np.array(batch.obs_pose[S0:])
        pinned = torch.from_numpy(table.copy()).pin_memory()
        members = ag.members.reshape(-1, g) if B % g == 0 else None
        assert members is not None, "--egos must be a multiple of --group"
        scenes = batch.scene_of[members] - S0  # [G, g]
        t_now = batch.t_now
        parts = dict(eval_ms=[], readback_ms=[], scatter_ms=[], upload_ms=[], total_ms=[])
        for it in range(args.warmup + args.repeats):
            torch.cuda.synchronize(dev)
            w0 = time.perf_counter()
            eng.eval_trajs_device(db.params, db.fb, 1, d_es.data_ptr(), cost.data_ptr(), flags.data_ptr(), traj.data_ptr(), stream=stream, traj_stride=stride)
            torch.cuda.synchronize(dev)
            w1 = time.perf_counter()
            series = traj.cpu().numpy()
            w2 = time.perf_counter()
            m = min(rows, stride, T_obs - int(t_now.max()))
            el = np.stack([series[:, 9, :m], series[:, 10, :m], series[:, 11, :m], np.ones((B, m))], axis=-1)  # [B, m, 4]
            el = np.nan_to_num(el, nan=0.0)
            for k in range(g):  # member k of every group -> column col_base + k of every scene of its group
                src = el[members[:, k]]  # [G, m, 4]
                for k2 in range(g):
                    table[scenes[:, k2], :m, ag.col_base + k] = 0.0 if k2 == k else src
            w3 = time.perf_counter()
            pinned.copy_(torch.from_numpy(table))
            db.t["obs_pose"][S0:].copy_(pinned, non_blocking=True)
            torch.cuda.synchronize(dev)
            w4 = time.perf_counter()
            if it >= args.warmup:
                for key, v in zip(parts, (w1 - w0, w2 - w1, w3 - w2, w4 - w3, w4 - w0)):
                    parts[key].append(v * 1e3)
        out["uploaded_mb"] = table.nbytes / 1e6
        out["host_route"] = {k: dict(median=float(np.median(v)), min=min(v), max=max(v)) for k, v in parts.items()}
    if args.part == "c":
        out["without_agents"] = cycles(lambda: ClosedLoopRunner(eng, DeviceBatch(attached()), goal, "FOP", fused=False))
        out["with_agents"] = cycles(lambda: ClosedLoopRunner(eng, DeviceBatch(attached()), goal, "FOP", agents=ag))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
