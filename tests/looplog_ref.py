"""numpy restatement of fp_loop_record's per-ego rule (include/frenet_gpu.h): the bookkeeping reference of the loop-log tests.

A snapshot is what a step left behind for the whole batch: ego [B, 6], t_now, done, cycles [B], cart [B, 3], best_cost [B], stats [B, 4]
and either best_idx [B] or end_state [B, 3].  For every ego with sealed == 0: stats_sum += stats; cycles > n_rows: row n_rows is written
when it is below max_rows, n_rows = cycles; done != 0: sealed = 1.  n_running = egos with done == 0.
"""
import numpy as np

COLS = 16
(TIME_STEP, X, Y, YAW, VELOCITY, VELOCITY_Y, S, S_DD, D, D_DD, COST, D_END, V_END, T_END, BEST_IDX, DONE) = range(COLS)


class LoopLogRef:
    def __init__(self, B, max_rows, done=None, n_rows=None):
        self.B, self.max_rows = B, max_rows
        self.rows = np.full((B, max_rows, COLS), np.nan)
        self.row_stats = np.zeros((B, max_rows, 4), dtype=np.int32)
        self.n_rows = np.zeros(B, dtype=np.int32) if n_rows is None else np.array(n_rows, dtype=np.int32)
        self.sealed = np.zeros(B, dtype=np.int32) if done is None else (np.asarray(done) != 0).astype(np.int32)  # whoever resets the log seals the finished
        self.stats_sum = np.zeros((B, 4), dtype=np.int64)
        self.n_running = -1

    def record(self, snap, d_samples=None, v_samples=None, t_samples=None):
        """snap: an object with ego, t_now, done, cycles, cart, best_cost, stats and best_idx or end_state (the other None / absent)."""
        best_idx = getattr(snap, "best_idx", None)
        end_state = getattr(snap, "end_state", None)
        assert (best_idx is None) != (end_state is None)
        for b in range(self.B):
            if self.sealed[b]:
                continue
            self.stats_sum[b] += snap.stats[b]
            if snap.cycles[b] > self.n_rows[b]:
                n = int(self.n_rows[b])
                if n < self.max_rows:
                    if end_state is not None:
                        idx, end = -1, end_state[b]
                    else:
                        idx = int(best_idx[b])
                        end = [np.nan] * 3
                        if idx >= 0:  # flat FOP index (i_d * nt + i_T) * nv + i_v, as fp_advance decodes it
                            nv, nt = v_samples.shape[1], len(t_samples)
                            end = [d_samples[idx // (nv * nt)], v_samples[b, idx % nv], t_samples[(idx // nv) % nt]]
                    e = snap.ego[b]
                    self.rows[b, n] = [snap.t_now[b] - 1, snap.cart[b, 0], snap.cart[b, 1], snap.cart[b, 2], e[1], e[4], e[0], e[2], e[3], e[5],
                                       snap.best_cost[b], end[0], end[1], end[2], idx, snap.done[b]]
                    self.row_stats[b, n] = snap.stats[b]
                self.n_rows[b] = snap.cycles[b]
            if snap.done[b] != 0:
                self.sealed[b] = 1
        self.n_running = int(np.sum(np.asarray(snap.done) == 0))
