"""CPU: every case of tests/whole_hit_cases.py is what its kind says - proved with the oracle and the numpy restatement of stage V's
circle (tools/group_hit_estimate.py, tools/whole_hit_estimate.py) alone, no kernel:

  * which egos reach stage W's verdict (every candidate collides and every lon profile has two points), and how: "V" - the kernel's
    circle ends all nv end-speed groups before the walk; "walk" - V leaves groups and S, B and N fill the masks; "open" - none;
  * the cases with one free candidate: it is free in the oracle by the distance the case states, every other lateral sample of its
    lon profile collides, and it is the oracle's winner's kind (a free one exists: best_idx >= 0);
  * the line's end: every candidate collides in the oracle although lon profiles with M = 1 exist - a verdict that took "every
    candidate collides" from the oracle's flags alone would be reached where the kernel's masks stay open;
  * the short horizon in the MIDDLE of t_samples: the first half of the horizons (the first workgroup of a tail-split ego) is blocked
    whole, the second half holds the free profiles - one half reaches the verdict, the other does not;
  * no candidate of any case stands within 1e-6 m of contact with an obstacle at a checked row (the cases built here: checked here;
    the others are cases of the V suite, seed for seed, checked there), so the GPU file compares every ego."""
import numpy as np
import pytest

import group_hit_cases as H
import whole_hit_cases as C

SHAPE = "9 x 9 x 7"
W = H.G  # tools/group_hit_estimate.py


@pytest.fixture(scope="module")
def plans(oracle):
    out = {}
    for name in C.CASES:
        batch, kind = C.build(name, SHAPE)
        out[name] = (batch, kind, [p.fop_plan() for p in oracle.problems_from_batch(batch)])
    return out


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_reaches_the_stage_its_kind_names(plans, name):
    batch, kind, ref = plans[name]
    reached = [C.reaches(r.flags) for r in ref]
    for b, r in enumerate(ref):
        assert not reached[b] or r.best_idx == -1, f"{name} ego {b}: blocked whole, yet the oracle selects {r.best_idx}"
    if kind in ("V", "walk"):
        assert all(reached), f"{name}: egos {[b for b, x in enumerate(reached) if not x]} do not reach the verdict"
        by_v = [len(H.ended_groups(batch, b)[0]) == batch.nv for b in range(batch.B)]
        if kind == "V":
            assert all(by_v), f"{name}: V leaves groups of egos {[b for b, x in enumerate(by_v) if not x]}"
        else:
            assert not any(by_v), f"{name}: V ends every group of egos {[b for b, x in enumerate(by_v) if x]}: nothing is left to the walk"
    elif kind == "open":
        assert not any(reached), f"{name}: egos {[b for b, x in enumerate(reached) if x]} reach the verdict"
    else:
        assert tuple(b for b, x in enumerate(reached) if x) == C.EGOS[name], (name, reached)


@pytest.mark.parametrize("name", [n for n in C.CASES if "passes by" in n])
def test_one_free_candidate_keeps_the_ego_open(plans, name):
    """Beside the line every lon profile keeps exactly its extreme lateral sample free; along the line the slowest group's rearmost
    candidate is free.  The oracle selects a free candidate: an ego ended whole would report none."""
    batch, _, ref = plans[name]
    for b, r in enumerate(ref):
        coll = ((r.flags & 4) != 0).reshape(batch.nd, batch.nt, batch.nv)
        assert r.best_idx >= 0 and not coll.reshape(-1)[r.best_idx], (name, b)
        if "lon profile" in name:
            at_end = int(np.argmax(batch.d_samples) if b % 2 == 0 else np.argmin(batch.d_samples))
            assert not coll[at_end].any() and coll[[i for i in range(batch.nd) if i != at_end]].all(), (name, b)
        else:
            assert coll.sum() >= coll.size - batch.nt, f"{name} ego {b}: more than one lateral sample's horizons are free"


@pytest.mark.parametrize("mixed", [False, True])
def test_line_end_blocks_every_candidate_through_profiles_with_one_point(plans, mixed):
    name = "the line ends between the second points (M = 1 and M >= 2)" if mixed else "the line ends before every second point (M = 1)"
    batch, _, ref = plans[name]
    for b, r in enumerate(ref):
        M = (r.flags >> 20).reshape(batch.nd, batch.nt, batch.nv)[0]
        assert ((r.flags & 4) != 0).all() and r.best_idx == -1, (name, b)
        assert (M == 1).any() and ((M >= 2).any() if mixed else (M == 1).all()), (name, b, np.unique(M))


def test_short_middle_horizon_blocks_one_half_of_a_split_ego(plans):
    batch, _, ref = plans["a short horizon among long ones"]
    mid = batch.nt // 2
    for b, r in enumerate(ref):
        coll = ((r.flags & 4) != 0).reshape(batch.nd, batch.nt, batch.nv)
        assert coll[:, :mid].all(), f"ego {b}: the slices of the first workgroup (horizons 0..{mid - 1}) are blocked whole"
        assert not coll[:, mid].any() and r.best_idx >= 0, f"ego {b}: the short profiles, in the second workgroup's slices, stay free"


def test_estimate_agrees_with_the_cases(plans):
    """tools/whole_hit_estimate.py's verdicts on two cases: all collide, reached and V's share as the kinds say; no unsound circle."""
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import whole_hit_estimate as WE

    for name, want in (("a box over the first second", (True, True, True)), ("a vehicle so small that thr <= 0", (True, True, False)),
                       ("the line ends before every second point (M = 1)", (True, False, False))):
        batch = plans[name][0]
        for b in (0, 5):
            got = WE.ego_verdicts(batch, b)
            assert got[:3] == want, (name, b, got)
            assert got[3] < 0 or got[0], f"{name} ego {b}: the one circle ends an ego with a free candidate"


def test_the_other_cases_are_proved_apart_in_their_own_suites():
    """Every case that is not built here is a case of the S or the V suite with the same builder and seed: tests/test_sure_hit_cpu.py
    and tests/test_group_hit_cpu.py prove that none of its candidates stands within 1e-6 m of contact."""
    for name in C.CASES:
        if name not in C.NEW:
            batch = C.build(name, SHAPE)[0]
            twins = [H.build(n, SHAPE)[0] for n in H.CASES]
            assert any(np.array_equal(batch.obs_pose, t.obs_pose, equal_nan=True) and np.array_equal(batch.ego, t.ego) and
                       np.array_equal(batch.t_samples, t.t_samples) and batch.veh_l == t.veh_l for t in twins), name


@pytest.mark.parametrize("name", C.NEW)
def test_no_candidate_within_a_micrometre_of_contact(oracle, name):
    """What the GPU file compares is decided by the stages, not by rounding: no ego box of any candidate of the cases built here is
    within 1e-6 m of contact with an obstacle at a checked row."""
    batch, _ = C.build(name, SHAPE)
    for b in range(batch.B):
        near = H.near_contacts(batch, b)
        assert not near, f"{name} ego {b}: (id, it, iv, k, obstacle) within 1e-6 m of contact: {near[:5]}"
