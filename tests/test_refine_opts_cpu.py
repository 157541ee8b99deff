"""The FISS+ refinement off its defaults, without a GPU: the oracle's planner (orc_fissplus_plan, the C refinement loop) against the numpy
restatement (tests/fiss_rules_ref.py: the oracle's per-trajectory costs, search.refine_step, the pop loop) on every case of
tests/refine_cases.py, and the proof on the restatement alone that the cases reach the paths they exist for."""
from types import SimpleNamespace

import numpy as np
import pytest

import refine_cases as RC
from oracle import oracle as O


@pytest.mark.parametrize("cid", RC.IDS)
def test_oracle_equals_the_restatement(cid):
    """A step whose gradient is undefined ends the rounds: the oracle used to clip it first, which turned the NaN into samp_min, and went
    on refining from there (26 generated candidates where the contract gives 11, on base with samp_res[:, 1] = 0 and R = 3)."""
    c = RC.BY_ID[cid]
    batch, prev = RC.made(c)
    rows = []
    for e, p in enumerate(O.problems_from_batch(batch)):
        w = p.fissplus_plan(None if prev[e, 0] < 0 else prev[e], **RC.opts(c))
        rows.append(SimpleNamespace(best_ijk=w.best_ijk, prev_best_idx=w.prev_best_idx, stats=w.stats, refined=w.refined, end_state=w.end_state,
                                    best_cost=w.best_cost, trace=w.trace.reshape(-1, 4)))
    RC.check_batch(rows, RC.refs(O, c), cid)


def decided(c):
    return [r for r in RC.refs(O, c) if not r.undecided]


@pytest.mark.parametrize("on", ["base", "long"])
def test_nine_rounds_fill_the_wavefront(on):
    """63 candidates for every ego with a coarse winner, and an ego that consumes more than 40 of them: more than ten validation groups."""
    for name in ("R9", "R9-decay1"):
        c = RC.BY_ID[f"{on}-{name}"]
        planned = [r for r in decided(c) if r.best_ijk[0] >= 0]
        assert planned and all(len(r.trace) == 63 for r in planned), c.id
    assert max(RC.pops(O, RC.BY_ID[f"{on}-R9"])) > 40, on


@pytest.mark.parametrize("on", ["base", "long"])
def test_shrunk_box_consumes_candidates_and_keeps_the_coarse_winner(on):
    c = RC.BY_ID[f"{on}-box0.9"]
    assert any(n > 0 and not r.refined and not r.undecided for n, r in zip(RC.pops(O, c), RC.refs(O, c))), on


@pytest.mark.parametrize("cid", [c.id for c in RC.CASES if c.undefined])
def test_undefined_step_leaves_six_candidates(cid):
    planned = [r for r in decided(RC.BY_ID[cid]) if r.best_ijk[0] >= 0]
    assert planned and all(len(r.trace) == 6 for r in planned), cid


def test_history_weight_changes_a_walk():
    a, b = RC.refs(O, RC.BY_ID["base-w0"]), RC.refs(O, RC.BY_ID["base-w50"])
    assert any(not (x.undecided or y.undecided) and (not np.array_equal(x.stats, y.stats) or not np.array_equal(x.best_ijk, y.best_ijk)) for x, y in zip(a, b))
