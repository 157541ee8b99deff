#!/usr/bin/env python3
"""Cost of the fallback stop that obeys the road rules (fp_fallback_stop_rules) on the headline batch (config 3: 2048 egos x 9x9x7 x 50
obstacles, resident) carrying all four rules, a family of 5 d x 6 T, on the dense pass' own best_idx (the egos without a winner need one):
  (a) fp_fallback_stop_rules per launch, with the gates only and with all four rules;
  (b) fp_fallback_stop per launch, in the same run;
  (c) what a caller needed for the same answer before: fp_fallback_stop(cand=), fp_eval_trajs and fp_rules_eval with K = 30 on the egos
      without a winner (the others skipped), the copy of cand, the flag words and the rule bits to pinned host memory, and the choice on
      the host (numpy, vectorised over the egos) - wall clock per round, with the device part (hip events) beside it;
  (d) both launches on a healthy batch (every ego has a plan: every workgroup returns before it stages anything).
One JSON line.  Timing: hip events around `--steps` enqueued calls, `--repeats` times after `--warmup` calls; median and min / max of
the repeats, interleaved in one process."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def with_rules(batch):
    """The batch with a wavy speed limit, one light 15 m ahead of the last ego of every frame that is closed half of the time, a wavy
    corridor and a time gap of 2 s / 1 s."""
    from fiss_plus_planner_amd.spline import gate_bits

    k = np.where(np.isfinite(batch.knots), batch.knots, 0.0)
    line = np.full((batch.F, 1), np.nan)
    line[np.asarray(batch.frame_of), 0] = batch.ego[:, 0] + 15.0
    closed = ((np.arange(256)[None, :, None] // 40) % 2 == 0) & np.ones((batch.F, 1, 1), dtype=bool)
    return dataclasses.replace(batch, speed_limit=np.where(np.isfinite(batch.knots), 8.5 + 3.5 * np.sin(k / 31.0), np.inf), limit_front=0.5 * batch.veh_l,
                               limit_tol=0.05, gate_s=line, gate_closed=gate_bits(closed), gate_front=0.5 * batch.veh_l, gate_max_decel=4.0,
                               bound_left=1.65 + 0.5 * np.sin(k / 17.0), bound_right=-(1.45 + 0.4 * np.cos(k / 23.0)), bound_margin=0.05,
                               gap_follow=20, gap_lead=10, gap_first=2)


def host_choice(cand, bits, d_end, d0, n_stop):
    """The definition's choice from cand [B, F] and the rule bits [B, F] (0 where cand != -1) -> fb_idx [B] (-1: none), vectorised."""
    B, F = cand.shape
    i_T = np.arange(F)[None, :] % n_stop
    adm = cand != -2
    contact = cand >= 0
    pop = np.zeros_like(bits)
    for i in range(5):
        pop += (bits >> i) & 1
    viol = (bits != 0) & ~contact
    k1 = np.where(contact, 2, np.where(viol, 1, 0)).astype(np.int64)
    k2 = np.where(contact, -cand, np.where(viol, pop * 65536 + i_T, -i_T)).astype(np.int64)
    k3 = np.where(contact, i_T, 0)
    lat = np.abs(d_end - d0[:, None])
    order = np.lexsort((np.broadcast_to(np.arange(F), (B, F)), lat, k3, k2, k1, ~adm), axis=1)[:, 0]
    return np.where(adm.any(axis=1), order, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--egos", type=int, default=2048)
    args = ap.parse_args()
    import torch

    from fiss_plus_planner_amd import _abi, rules, synth
    from fiss_plus_planner_amd.device_batch import DeviceBatch
    from fiss_plus_planner_amd.engine import FrenetEngine
    from fiss_plus_planner_amd.fallback import FallbackStop

    eng = FrenetEngine(0)
    batch = with_rules(synth.make_config(3, B=args.egos))
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
    sets = {names: rules.rule_set(batch, lambda k: db.t[k].data_ptr(), names) for names in (("gates",), tuple(rules.by_name))}
    best_idx, best_cost = torch.empty(B, dtype=i32, device=dev), torch.empty(B, dtype=f64, device=dev)
    eng.plan_dense_device(db.params, db.fb, best_idx.data_ptr(), best_cost.data_ptr(), stream=stream)
    torch.cuda.synchronize(dev)
    bi = best_idx.cpu().numpy()
    healthy_idx = torch.from_numpy(np.where(bi >= 0, bi, 0).astype(np.int32)).to(dev)
    es = torch.full((B, 3), float("nan"), dtype=f64, device=dev)
    o_i = [torch.zeros(B, dtype=i32, device=dev) for _ in range(5)]
    o_v = torch.zeros(B, dtype=f64, device=dev)
    cand = torch.full((B, F), -3, dtype=i32, device=dev)

    def fallback(idx, with_cand=False):
        eng.fallback_stop_device(db.params, db.fb, st, es.data_ptr(), o_i[0].data_ptr(), o_i[1].data_ptr(), o_i[2].data_ptr(), o_i[3].data_ptr(), o_v.data_ptr(),
                                 best_idx=idx.data_ptr(), cand=cand.data_ptr() if with_cand else 0, stream=stream)

    def fallback_rules(idx, names):
        eng.fallback_stop_rules_device(db.params, db.fb, st, sets[names][0], es.data_ptr(), o_i[0].data_ptr(), o_i[1].data_ptr(), o_i[2].data_ptr(), o_i[3].data_ptr(),
                                       o_v.data_ptr(), o_i[4].data_ptr(), best_idx=idx.data_ptr(), stream=stream)

    # the earlier route to the same answer: contact per candidate, the family's flag words, the rule bits, read back, chosen on the host
    d_t = fs.targets(batch)
    d_end = np.where(np.isnan(d_t)[None, :], batch.ego[:, 3:4], d_t[None, :])  # [B, n_d]
    fam = np.zeros((B, F, 3))
    fam[:, :, 0] = np.repeat(d_end, st.n_stop, axis=1)
    fam[:, :, 2] = np.tile(fs.stop_times, st.n_d)[None, :]
    fam_bk = torch.from_numpy(fam).to(dev)
    has_plan = torch.from_numpy((bi >= 0).astype(np.int32)).to(dev)
    fb_skip = _abi.FpBatch.from_buffer_copy(db.fb)
    fb_skip.skip = has_plan.data_ptr()
    cost, flags, bits = torch.empty((B, F), dtype=f64, device=dev), torch.empty((B, F), dtype=i32, device=dev), torch.zeros((B, F), dtype=i32, device=dev)
    h_cand, h_flags, h_bits = (torch.empty((B, F), dtype=i32).pin_memory() for _ in range(3))
    keep = ~_abi.FLAG_INFEASIBLE & 0x7FFFFFFF | -(1 << 31)  # (the words travel as int32 here)
    all_names = tuple(rules.by_name)

    def earlier_device():
        fallback(best_idx, with_cand=True)
        eng.eval_trajs_device(db.params, fb_skip, F, fam_bk.data_ptr(), cost.data_ptr(), flags.data_ptr(), stream=stream)
        flags.bitwise_and_(keep)
        eng.rules_eval_device(db.params, fb_skip, sets[all_names][0], F, fam_bk.data_ptr(), flags.data_ptr(), bits.data_ptr(), 0, stream)
        for dst, src in zip((h_cand, h_flags, h_bits), (cand, flags, bits)):
            dst.copy_(src, non_blocking=True)

    def earlier_round():
        earlier_device()
        torch.cuda.synchronize(dev)
        c = h_cand.numpy()
        return host_choice(c, np.where(c == -1, h_bits.numpy(), 0), fam[:, :, 0], batch.ego[:, 3], st.n_stop)

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

    def walled(fn, rounds):
        fn()
        t = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            for _ in range(rounds):
                fn()
            t.append((time.perf_counter() - t0) * 1e3 / rounds)
        return dict(median_ms=float(np.median(t)), min_ms=min(t), max_ms=max(t))

    out = dict(B=B, F=F, steps=args.steps, repeats=args.repeats, need=int((bi < 0).sum()))
    out["a_rules_gates"] = timed(lambda: fallback_rules(best_idx, ("gates",)), args.steps)
    out["a_rules_all_four"] = timed(lambda: fallback_rules(best_idx, all_names), args.steps)
    out["b_fallback_stop"] = timed(lambda: fallback(best_idx), args.steps)
    out["c_earlier_route_device"] = timed(earlier_device, max(args.steps // 5, 1))
    out["c_earlier_route_wall_with_host_choice"] = walled(earlier_round, max(args.steps // 10, 1))
    out["d_healthy_rules_all_four"] = timed(lambda: fallback_rules(healthy_idx, all_names), args.steps)
    out["d_healthy_fallback_stop"] = timed(lambda: fallback(healthy_idx), args.steps)
    out["d_healthy_rules_all_four_again"] = timed(lambda: fallback_rules(healthy_idx, all_names), args.steps)
    out["d_healthy_fallback_stop_again"] = timed(lambda: fallback(healthy_idx), args.steps)
    # the same answer both ways (the egos whose verdicts do not sit on a threshold: all but a few)
    fallback_rules(best_idx, all_names)
    torch.cuda.synchronize(dev)
    got = o_i[1].cpu().numpy()
    want = earlier_round()
    need = bi < 0
    out["same_choice"] = int((got[need] == want[need]).sum())
    out["status_counts"] = np.bincount(o_i[0].cpu().numpy(), minlength=4).tolist()
    out["rule_bits_set"] = int((o_i[4].cpu().numpy()[need] != 0).sum())
    out["launches"] = dict(fallback=eng.get_option("fallback_launches"), fallback_rules=eng.get_option("fallback_rules_launches"))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
