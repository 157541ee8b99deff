#!/usr/bin/env python3
"""Cost of predicting the obstacle pose table on the device (fp_obstacles_predict) against shipping it, on the 2048-scene config-3 table
(50 rows x 50 obstacles per scene, 164 MB written) and on one scene:
  (a) the kernel on the resident 2048-scene batch: time per launch and GB/s written (materialise mode's measured rate: 5.2 TB/s written)
  (b) the parent's way, in the same process: the host-to-device copy of the same table from pinned memory; the numpy build of the table
      (synth's own arithmetic on the same tracks) is reported separately
  (c) one scene: the FP_MEM_HOST call (stage the tracks, launch, copy 80 KB back, wait) against the host-to-device copy of one 80 KB table
One JSON line.  Timing: hip events around `--steps` enqueued launches / copies, `--repeats` times after `--warmup`; median and min / max
of the repeats; (c) is wall clock per call.  The kernel's own time comes from
`rocprofv3 --kernel-trace --stats -- python tools/predict_rate.py --steps 50 --repeats 1`."""
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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--scenes", type=int, default=2048)
    args = ap.parse_args()
    import dataclasses

    import torch

    from fiss_plus_planner_amd import synth
    from fiss_plus_planner_amd.device_batch import DeviceBatch
    from fiss_plus_planner_amd.engine import FrenetEngine

    eng = FrenetEngine(0)
    cfg = (args.scenes, 9, 9, 7, 50, 50, True, synth.CONFIG_SEEDS[3])
    batch = synth.make_batch(*cfg, layout="survey8d")
    tr = synth.make_tracks(*cfg, layout="survey8d")
    batch = dataclasses.replace(batch, track_model=tr.model, track_state=tr.state, track_frame=tr.frame_of_scene)
    db = DeviceBatch(batch, 0)
    dev = db.dev
    S, T, n = batch.S, batch.T_obs, batch.n_obs
    table_bytes = S * T * n * 32
    t0 = torch.zeros(S, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                fn()
            b.record()
            torch.cuda.synchronize(dev)
            ms.append(a.elapsed_time(b) / args.steps)
        return dict(median_ms=float(np.median(ms)), min_ms=min(ms), max_ms=max(ms))

    out = dict(scenes=S, T_obs=T, n_obs=n, table_mb=table_bytes / 1e6, steps=args.steps, repeats=args.repeats)
    # (a) the kernel, the tracks and the table resident
    k = timed(lambda: db.predict(eng, t0, T, stream=stream))
    k["gb_per_s_written"] = table_bytes / 1e9 / (k["median_ms"] / 1e3)
    out["predict_kernel"] = k
    torch.cuda.synchronize(dev)
    got = db.t["obs_pose"].cpu().numpy()
    out["max_abs_diff_to_numpy_table"] = float(np.abs(got - batch.obs_pose).max())
    # (b) the parent's way: the table built in numpy, copied from pinned memory
    t_build = []
    for _ in range(3):
        w = time.perf_counter()
        tt = np.arange(T) * batch.tick_t
        s_t = tr.state[:, None, :, 0] + tr.state[:, None, :, 2] * tt[None, :, None]
        px, py, yaw = synth.sample_frames(batch.knots, batch.coef, s_t)
        d = tr.state[:, None, :, 1]
        pose = np.stack([px - d * np.sin(yaw), py + d * np.cos(yaw), yaw, np.ones_like(px)], axis=-1)
        t_build.append((time.perf_counter() - w) * 1e3)
    assert np.array_equal(pose, batch.obs_pose)
    out["numpy_build_ms"] = dict(median_ms=float(np.median(t_build)), min_ms=min(t_build), max_ms=max(t_build))
    pinned = torch.from_numpy(batch.obs_pose).pin_memory()
    dst = torch.empty_like(db.t["obs_pose"])
    c = timed(lambda: dst.copy_(pinned, non_blocking=True))
    c["gb_per_s"] = table_bytes / 1e9 / (c["median_ms"] / 1e3)
    out["h2d_copy_pinned"] = c
    out["kernel_below_copy"] = bool(k["median_ms"] < c["median_ms"])
    # (c) one scene: the FP_MEM_HOST call against the copy of one 80 KB table
    one = batch.take([0])
    calls = max(args.steps * 4, 100)

    def wall(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize(dev)
        us = []
        for _ in range(args.repeats):
            w = time.perf_counter()
            for _ in range(calls):
                fn()
            us.append((time.perf_counter() - w) * 1e6 / calls)
        return dict(median_us=float(np.median(us)), min_us=min(us), max_us=max(us))

    table1 = np.zeros((1, T, n, 4))
    out["one_scene_host_call"] = wall(lambda: eng.predict_obstacles(one, one.track_model, one.track_state, one.track_frame, 0, T, out=table1))
    pinned1, dst1 = torch.from_numpy(one.obs_pose).pin_memory(), torch.empty((1, T, n, 4), dtype=torch.float64, device=dev)

    def copy_one():
        dst1.copy_(pinned1, non_blocking=True)
        torch.cuda.synchronize(dev)

    out["one_scene_h2d_copy_pinned"] = wall(copy_one)
    one_dev = DeviceBatch(one, 0)
    t01 = torch.zeros(1, dtype=torch.int32, device=dev)
    k1 = timed(lambda: one_dev.predict(eng, t01, T, stream=stream))
    out["one_scene_kernel"] = k1
    out["predict_launches"] = eng.get_option("predict_launches")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
