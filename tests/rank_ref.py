"""Numpy restatement of fp_rank_feasible (include/frenet_gpu.h): the k cheapest survivors of every ego from the dense tables.
Survivor: no FP_FLAG_INFEASIBLE bit, cost not NaN.  Order: ascending cost, the higher flat index first among equal costs."""
import numpy as np

FLAG_INFEASIBLE = 1 | 2 | 4 | 16 | 32 | 64


def rank_tables(cost, flags, k, skip=None):
    """cost, flags [B, C] -> rank_idx [k, B] (-1 padded), rank_cost [k, B] (NaN padded), n_feasible [B]."""
    B = cost.shape[0]
    rank_idx, rank_cost, n = np.full((k, B), -1, dtype=np.int32), np.full((k, B), np.nan), np.zeros(B, dtype=np.int32)
    for b in range(B):
        if skip is not None and skip[b]:
            continue
        idx = np.nonzero(((flags[b] & FLAG_INFEASIBLE) == 0) & ~np.isnan(cost[b]))[0]
        order = idx[np.lexsort((-idx, cost[b, idx]))][:k]
        n[b] = len(idx)
        rank_idx[:len(order), b], rank_cost[:len(order), b] = order, cost[b, order]
    return rank_idx, rank_cost, n
