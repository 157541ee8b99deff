"""CPU: every case of tests/sure_hit_cases.py is what its name says - proved with the oracle and the numpy test of
tools/sure_hit_estimate.py alone (no kernel): where the sure item stands, that the silent cases have none, on which side of thr
the boundary cases lie and by how much, and that across all cases no lon profile with a sure hit has a free candidate.

The boundary cases put a real candidate on the fan's outside end (a symmetric fan on a straight line, the egos on the extreme lateral
sample): with that end outside thr by delta S is silent, N decides, that candidate is free and every other lateral sample collides;
with both ends inside, S fires and all collide.  Even egos have the outside end at E+, odd egos at E-: either end's test alone,
or `||` in place of `&&`, blocks a candidate the oracle keeps free."""
import numpy as np
import pytest

import range_argmin_cases as R
import sure_hit_cases as S

E = S.E
SHAPE_NAMES = list(S.SHAPES)


def report(batch):
    """Per ego: the rows of E.ego_report - (it, iv, blocked, any collision, first sure step with +-dm, with the true ends)."""
    return [E.ego_report(batch, b) for b in range(batch.B)]


def has_pose_at(batch, b, it, k):
    """Whether the profiles of slice `it` of ego b have a checked pose at step k (the line does not end: M = N = len(arange(0, T, tick)))."""
    n = len(np.arange(0.0, batch.t_samples[it], batch.tick_t))
    sc = int(batch.scene_of[b])
    return sc >= 0 and k < n and k + int(batch.t_now[b]) < min(batch.T_obs, int(batch.final_time_step[sc]))


@pytest.fixture(scope="module")
def reports(oracle):
    out = {}
    for shape in SHAPE_NAMES:
        for name in S.CASES:
            batch, kind = S.build(name, shape)
            out[shape, name] = (batch, kind, report(batch))
    return out


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("name", [n for n, (_, kind) in S.CASES.items() if kind == "sure"])
def test_sure_cases_have_a_sure_item_where_they_say(reports, shape, name):
    batch, _, rep = reports[shape, name]
    k_want, pos_want = S.EXPECT[name]
    k_want = S.k_last(batch) if k_want == "last" else k_want
    found = 0
    for b, rows in enumerate(rep):
        for it, iv, blocked, _, pm, ends in rows:
            if has_pose_at(batch, b, it, k_want):
                assert pm == k_want and ends == k_want and blocked, (shape, name, b, it, iv, pm, ends, blocked)
                found += 1
            else:
                assert pm < 0 and not blocked, (shape, name, b, it, iv)
    assert found >= batch.B, "a case table without a sure hit for this shape is a broken table, not a skip"
    if pos_want:  # items of the list in front of the sure one: the columns that ride alongside, at every checked step before it
        n_cols = 4 if pos_want == 64 else batch.n_obs - 1
        before = n_cols * (k_want // batch.check_stride)
        assert before >= (pos_want if shape != SHAPE_NAMES[2] else 64), (shape, name, before)
        for b in range(batch.B):  # ... and they do survive the group test: nearer than what its circle adds to the range
            assert S.ALONGSIDE + 0.5 < R.group_reach(batch, b, (1.0, 1.0))


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("name", [n for n, (_, kind) in S.CASES.items() if kind == "silent"])
def test_silent_cases_have_no_sure_item(reports, shape, name):
    batch, _, rep = reports[shape, name]
    rows = [r for ego in rep for r in ego]
    assert all(r[4] < 0 for r in rows), (shape, name)
    blocked, free = sum(r[2] for r in rows), sum(not r[3] for r in rows)
    if name.startswith("veh_l < veh_w") or name.startswith("the line ends") or name.startswith("a near miss"):
        assert blocked == 0 and free == len(rows)  # the oracle keeps every candidate free
    else:  # far off the line, a NaN lateral sample: blocked through N
        assert blocked == len(rows)
    if name.startswith("a near miss"):  # both ends 2 cm outside thr (+ the 1e-6 of thr itself): a thr 5 cm too large would fire
        prob = E.O.problems_from_batch(batch, [0])[0]
        k, signed = E.sure_table(batch, 0, prob, 0, 0)
        assert k[0] == 0 and abs(signed[0, 0, 0] - 0.02) < 2e-6 and abs(signed[1, 0, 0] - 0.02) < 2e-6
    if name.startswith("veh_l < veh_w"):  # with rho = the half WIDTH the stage would fire: the case is not vacuous
        wrong = 0.5 * batch.veh_w - E.threshold(batch)
        prob = E.O.problems_from_batch(batch, [0])[0]
        tabs = [E.sure_table(batch, 0, prob, it, iv)[1] for it in range(batch.nt) for iv in range(batch.nv)]
        assert any(E.first_sure(t[:2] - wrong) is not None for t in tabs) and all(E.first_sure(t[:2]) is None for t in tabs)


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("delta", [1e-5, 1e-3, -1e-5])
def test_boundary_cases_lie_where_they_say(oracle, reports, shape, delta):
    name = {1e-5: "boundary: one end outside thr by 1e-5", 1e-3: "boundary: one end outside thr by 1e-3", -1e-5: "boundary: both ends inside thr by 1e-5"}[delta]
    batch, _, rep = reports[shape, name]
    k = S.K_BOUNDARY
    for b in range(batch.B):
        prob = oracle.problems_from_batch(batch, [b])[0]
        coll = ((prob.fop_plan().flags & 4) != 0).reshape(batch.nd, batch.nt, batch.nv)
        at_end = int(np.argmax(batch.d_samples) if b % 2 == 0 else np.argmin(batch.d_samples))  # the lateral sample that stands on the outside end
        out_end = 1 if b % 2 == 0 else 0  # E+ for the even egos, E- for the odd ones (rows of sure_table: E-, E+, lo, hi)
        seen = 0
        for it in range(batch.nt):
            if not has_pose_at(batch, b, it, k):
                continue
            for iv in range(batch.nv):
                ks, signed = E.sure_table(batch, b, prob, it, iv)
                r = int(np.nonzero(ks == k)[0][0])
                far, near = signed[out_end, r, 0], signed[1 - out_end, r, 0]  # against the case's box, minus thr
                assert abs(far - delta) < 1e-9 and near < -0.1, (shape, b, it, iv, far, near)
                assert abs(signed[2 + out_end, r, 0] - delta) < 1e-9, "a real candidate's centre stands on the outside end"
                row = rep[b][it * batch.nv + iv]
                assert row[:2] == (it, iv) and (row[4] == k) == (delta < 0), row
                if delta > 0:  # S is silent and N decides: the candidate on the outside end is free, every other one collides
                    assert not coll[at_end, it, iv] and coll[np.arange(batch.nd) != at_end, it, iv].all(), (shape, b, it, iv, coll[:, it, iv])
                else:
                    assert coll[:, it, iv].all(), (shape, b, it, iv)
                seen += 1
        assert seen >= batch.nv


@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_mixed_cases(reports, shape):
    for name, egos_with in (("poses without a state", [3, 7]), ("egos without a scene", [0, 2, 3, 4, 6, 7]), ("an obstacle of size 0", None)):
        batch, _, rep = reports[shape, name]
        for b, rows in enumerate(rep):
            for it, iv, blocked, anyc, pm, _ in rows:
                live = has_pose_at(batch, b, it, S.K_EARLY) and (egos_with is None or b in egos_with)
                if name == "an obstacle of size 0":  # a point on the line: inside every candidate's disk while the fan is narrower than thr
                    assert blocked == live, (shape, name, b, it, iv)
                    assert (pm == S.K_EARLY) == live
                else:
                    assert (pm == S.K_EARLY) == live and blocked == live and anyc == live, (shape, name, b, it, iv)


def test_no_sure_profile_has_a_free_candidate(reports):
    sure = 0
    for (shape, name), (_, _, rep) in reports.items():
        for rows in rep:
            for it, iv, blocked, _, pm, ends in rows:
                if pm >= 0 or ends >= 0:
                    sure += 1
                    assert blocked, (shape, name, it, iv)
    assert sure > 1000
