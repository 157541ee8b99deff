"""CPU: the cases of tests/scalar_cases.py are what their names say, by the oracle alone - every one decides something (a colliding and a
free candidate), and on both sides of every boundary a case is about (the staged rows, the checked rows, the line's end, the list's
capacity, the egos with and without a scene) there is a colliding and a free candidate."""
import math

import numpy as np
import pytest

import prologue_cases as P
import scalar_cases as S
from lattice_paths import SHAPE_555, SHAPE_997, coll_of, rows_of, shape_of


@pytest.fixture(scope="module")
def plans(oracle):
    cache = {}

    def get(name, batch=None):
        if name not in cache:
            b = S.CASES[name]() if batch is None else batch
            cache[name] = (b, [p.fop_plan() for p in oracle.problems_from_batch(b)])
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(S.CASES))
def test_every_case_decides_something(plans, name):
    batch, ref = plans(name)
    assert batch.B == S.B <= 8
    coll = coll_of(ref)
    assert coll.any() and (~coll).any(), (name, int(coll.sum()), coll.size)
    assert any(r.best_idx >= 0 for r in ref), name
    want = SHAPE_997 if name in S.SHAPED_997 else SHAPE_555 if name in S.SHAPED_555 else None
    assert (shape_of(batch) == want) if want else (shape_of(batch) not in (SHAPE_997, SHAPE_555) and batch.nv != batch.nd)


def _staged(batch):
    return np.ceil((batch.T_obs - batch.t_now) / batch.check_stride).astype(int)


def _horizon_cap(batch):
    return batch.final_time_step[np.maximum(batch.scene_of, 0)] - batch.t_now


def test_t_now_is_odd_and_differs_per_ego():
    for name in ("t_now odd", "220 knots (coefficient window), t_now odd"):
        b = S.CASES[name]()
        assert (b.t_now % 2 == 1).all() and (b.t_now > 0).all() and len(set(b.t_now.tolist())) == b.B and b.check_stride == 2
    assert S.CASES["220 knots (coefficient window), t_now odd"]().NX == 220


@pytest.mark.parametrize("name", ["table shorter than the horizon (13 of 25 rows staged)", "5 x 4 x 3 (nv != nd): table shorter than the horizon"])
def test_the_short_table_stages_13_rows_and_its_collisions_lie_below_them(oracle, plans, name):
    """rows_stage 13 < rows 25, horizon_cap beyond both, t_now odd.  The obstacle rows the kernel must NOT read (steps >= T_obs - t_now of the
    horizon) do not exist; the collisions there are come from the 13 rows that do: with the parked obstacles' states removed from
    t_now on candidates turn free, and removing every state BEFORE t_now changes nothing."""
    batch, ref = plans(name)
    assert (batch.t_now == S.T_NOW_SHORT).all() and S.T_NOW_SHORT % 2 == 1
    assert (_staged(batch) == 13).all() and rows_of(batch) == 25 and (_horizon_cap(batch) > 2 * 25).all()
    coll = coll_of(ref)
    hit = [e for e in range(batch.B) if coll[e].any()]
    assert hit and (~coll).any()
    pose = batch.obs_pose.copy()
    pose[:, S.T_NOW_SHORT:, 0, 3] = 0.0  # the parked obstacle (column 0) has no state from t_now on
    _, gone = plans(name + " / parked obstacle removed from t_now on", S._keep(batch, obs_pose=pose))
    assert coll_of(gone).sum() < coll.sum()
    pose = batch.obs_pose.copy()
    pose[:, :S.T_NOW_SHORT, :, 3] = 0.0  # ... and no obstacle has a state before t_now: those steps are nobody's business
    _, after = plans(name + " / no states before t_now", S._keep(batch, obs_pose=pose))
    np.testing.assert_array_equal(coll_of(after), coll)


@pytest.mark.parametrize("name", ["final_time_step inside the table (11 rows checked)", "5 x 5 x 5: t_now odd, final_time_step inside the table",
                                  "5 x 4 x 3 (nv != nd): t_now odd, final_time_step inside the table"])
def test_the_early_final_step_checks_11_rows_and_both_sides_of_it_matter(plans, name):
    """horizon_cap 21 -> 11 rows checked (poses 0, 2 .. 20), fewer than the table holds from t_now on and fewer than its rows in all.  An
    obstacle that stands on the ego's line from pose 22 on alone collides with nothing; the same obstacle from pose 0 on does."""
    batch, ref = plans(name)
    cap = _horizon_cap(batch)
    assert (cap == S.HORIZON_CAP).all() and (batch.t_now == S.T_NOW_CAP).all() and S.T_NOW_CAP % 2 == 1
    rows = math.ceil(S.HORIZON_CAP / batch.check_stride)
    assert rows == 11 and (rows < _staged(batch)).all() and (_staged(batch) < rows_of(batch)).all() or rows_of(batch) == 25
    assert len({rows, int(_staged(batch)[0]), rows_of(batch), S.HORIZON_CAP, S.T_NOW_CAP}) == 5
    coll = coll_of(ref)
    pose = batch.obs_pose.copy()
    pose[:, :S.T_NOW_CAP + S.HORIZON_CAP + 1, :, 3] = 0.0  # every obstacle exists behind the collision horizon alone
    _, late = plans(name + " / obstacles behind the horizon only", S._keep(batch, obs_pose=pose))
    assert coll.any() and not coll_of(late).any()


def test_the_line_ends_inside_the_checked_rows(plans):
    batch, ref = plans("a line that ends inside the checked rows")
    flags = np.concatenate([r.flags for r in ref])
    M, N, coll = flags >> 20, (flags >> 8) & 0xFFF, (flags & 4) != 0
    k_last = (rows_of(batch) - 1) * batch.check_stride
    early, whole = (M >= 2) & (M <= k_last + 1), M == N
    assert early.any() and whole.any() and (M > k_last + 1).any()
    assert (coll & early).any() and (~coll & early).any() and (coll & whole).any() and (~coll & whole).any()


def test_the_crowded_scene_fills_more_than_the_list(plans):
    """Every (row, obstacle) pair of the convoy lies within the ego's half diagonal + the largest lateral sample of a point of the lon
    profiles' range (tests/test_prologue_paths_cpu.py shows why that puts it inside the group circle): 25 x 50 survivors against a list
    of 256, five whole rows per chunk - the walk runs per chunk and item_base grows past 0."""
    batch, ref = plans("more survivors than the 256-entry list holds")
    reach = 0.5 * math.hypot(batch.veh_l, batch.veh_w) + np.abs(batch.d_samples).max()
    assert math.hypot(P.CONVOY_DS, P.CONVOY_D) < 0.9 * reach
    assert rows_of(batch) * batch.n_obs > 4 * 256 and rows_of(batch) >= S.CONVOY_ROWS_MIN
    assert (batch.obs_pose[..., 3] == 1.0).all()
    coll = coll_of(ref)
    assert any(coll[e].any() and not coll[e].all() for e in range(batch.B))


@pytest.mark.parametrize("name", ["frame_of / scene_of permuted, one ego without a scene", "5 x 5 x 5: permuted, one ego without a scene"])
def test_the_permuted_case(plans, name):
    batch, ref = plans(name)
    ids = np.arange(batch.B)
    assert (batch.frame_of != ids).all() and sorted(batch.frame_of.tolist()) == ids.tolist()
    assert (batch.scene_of != ids).all() and (batch.scene_of == -1).sum() == 1
    coll = coll_of(ref)
    lone = int(np.flatnonzero(batch.scene_of == -1)[0])
    assert not coll[lone].any() and any(coll[e].any() for e in range(batch.B) if e != lone)
    assert 0 < lone < batch.B - 1 and coll[lone - 1].any() or coll[lone + 1].any()


def test_skip_and_order_are_not_the_identity():
    assert S.SKIP[3] == 1 and S.SKIP[2] == 0 and S.SKIP[4] == 0 and S.SKIP.sum() == 2
    assert sorted(S.ORDER.tolist()) == list(range(S.B)) and (S.ORDER != np.arange(S.B)).all()


@pytest.mark.parametrize("name", list(S.FISS_CASES))
def test_fiss_cases_find_plans_and_collisions(oracle, name):
    batch = S.FISS_CASES[name]()
    assert batch.B == S.B and batch.samp_min is not None
    ref = [p.fop_plan() for p in oracle.problems_from_batch(batch)]
    coll = coll_of(ref)
    assert coll.any() and (~coll).any()
    found = [not np.isnan(p.fissplus_plan().best_cost) for p in oracle.problems_from_batch(batch)]
    assert any(found)
