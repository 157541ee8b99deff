"""What the four rule-pass references (tests/envelope_ref.py, gates_ref.py, boundary_ref.py, gaps_ref.py) literally share: the argmin of
the definition, the caps on undecided candidates and two batch builders.  numpy only; nothing here calls the library under test.  The
four ego_<rule> computations are the independent restatements and stay in their own modules."""
import numpy as np

FLAG_INFEASIBLE = 1 | 2 | 4 | 16 | 32 | 64 | 128  # FP_FLAG_CONSTRAINTS | FP_FLAG_COLLISION | FP_FLAG_BOUNDARY
SEED = 33055                                      # the seed of every rule pass's test batches


def argmin(cost, flags):
    """`min_cost >= cost`: the last minimum wins; a NaN cost never does (frenet_optimal_planner.py:264-268)."""
    best_idx, best_cost = -1, np.nan
    for c in range(len(cost)):
        if not (int(flags[c]) & FLAG_INFEASIBLE) and cost[c] == cost[c] and (best_idx < 0 or best_cost >= cost[c]):
            best_idx, best_cost = c, float(cost[c])
    return best_idx, best_cost


def check_caps(refs, max_share, max_egos, what=""):
    """The caps the tests rely on: at most `max_share` of the batch's candidates undecided, at most `max_egos` egos excluded for having
    one.  -> (undecided candidates, egos with one)"""
    total = sum(len(r.undecided) for r in refs)
    und = sum(int(r.undecided.sum()) for r in refs)
    egos = sum(1 for r in refs if r.undecided.any())
    assert und <= max_share * total, (what, und, total)
    assert egos <= max_egos, (what, egos)
    return und, egos


def plain_batch(B=5, nd=5, nv=4, nt=3, seed=SEED):
    """The smallest shape that still exercises every loop: 5 egos x 5 x 4 x 3 (C = 60: no multiple of the wave or of the workgroup,
    12 profiles for 4 wavefronts), N = 80 .. 100 (two lane rounds), 81 knots, no obstacles."""
    from fiss_plus_planner_amd import synth

    return synth.make_batch(B, nd, nv, nt, 0, 20, False, seed)


def _line_ends(batch, carry):
    """The line_ends case of every rule: `batch` with ego 1 close to the end of its line and ego 3 past it; carry(batch, ego) -> the
    batch with those ego states and the rule's data."""
    ego = batch.ego.copy()
    ego[1, 0] = batch.knots[1, -1] - 40.0  # within 40 m of the end of its line: fast candidates leave it (M < N)
    ego[3, 0] = batch.knots[3, -1] + 5.0   # past the end: M = 0 for every candidate, nothing is checked
    return carry(batch, ego)
