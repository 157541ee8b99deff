"""CPU: the cases of tests/prologue_cases.py decide something - by the oracle alone every one has a colliding and a free candidate - and
are what their names say (shape, t_now, missing states, the convoy inside every group circle)."""
import math

import numpy as np
import pytest

import prologue_cases as P
from lattice_paths import SHAPE_997, coll_of, rows_of, shape_of


@pytest.fixture(scope="module")
def plans(oracle):
    cache = {}

    def get(name):
        if name not in cache:
            batch = P.CASES[name]()
            cache[name] = (batch, [p.fop_plan() for p in oracle.problems_from_batch(batch)])
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(P.CASES))
def test_every_case_has_a_colliding_and_a_free_candidate(plans, name):
    batch, ref = plans(name)
    assert 8 <= batch.B <= 16
    coll = coll_of(ref)
    assert coll.any() and (~coll).any(), (name, int(coll.sum()), coll.size)
    assert any(r.best_idx >= 0 for r in ref), name


@pytest.mark.parametrize("name", sorted(P.SHAPED))
def test_shaped_cases_have_the_compiled_in_shape(name):
    batch = P.CASES[name]()
    assert shape_of(batch) == SHAPE_997


def test_run_time_tables_are_no_multiple_of_a_pass():
    b = P.CASES["13 rows x 7 obstacles"]()
    assert rows_of(b) == 13 and b.n_obs == 7 and (13 * 7) % 64 != 0
    assert P.CASES["one obstacle"]().n_obs == 1
    sums = {n: (lambda b: b.nt * (b.nv + b.nd))(P.CASES[n]()) for n in P.CASES if "sum lanes" in n}
    assert sorted(sums.values()) == [24, 98, 140] and P.CASES["9 x 5 x 7 (98 sum lanes)"]().nd != P.CASES["9 x 5 x 7 (98 sum lanes)"]().nv


def test_t_now_case_is_odd_and_cuts_the_table():
    b = P.CASES["t_now odd, tables shorter than the horizon"]()
    assert b.check_stride == 2 and (b.t_now % 2 == 1).all() and (b.t_now > 0).all()
    staged = np.ceil((b.T_obs - b.t_now) / b.check_stride)
    assert (staged < rows_of(b)).sum() >= 4 and staged.min() == 1 and (staged >= rows_of(b) - 1).any()


def test_missing_states_and_scenes():
    b = P.CASES["poses without a state"]()
    assert (b.obs_pose[..., 3] == 0).mean() > 0.2 and np.isnan(b.obs_pose[..., 0]).mean() > 0.05
    b = P.CASES["an ego without a scene"]()
    assert (b.scene_of == -1).sum() == 2 and (b.scene_of >= 0).sum() == b.B - 2
    b = P.CASES["d_samples descending"]()
    assert (np.diff(b.d_samples) < 0).all()
    assert np.isnan(P.CASES["d_samples with a NaN"]().d_samples).sum() == 1
    b = P.CASES["a line with all knots in one place"]()
    f = int(b.frame_of[0])
    assert np.ptp(b.knots[f]) == 0.0 and (np.ptp(b.knots[np.arange(b.knots.shape[0]) != f], axis=1) > 0).all()
    assert P.CASES["220 knots (coefficient window)"]().NX == 220
    b = P.CASES["veh_l == veh_w"]()
    assert b.veh_l == b.veh_w


def test_blocked_egos_collide_everywhere(plans):
    batch, ref = plans("blocked in the first round")
    for e, r in enumerate(ref):
        checked = (r.flags >> 20) >= 1  # candidates with at least one point on the line
        if e % 2 == 0:
            assert ((r.flags & 4) != 0)[checked].all(), e


def test_the_convoy_lies_inside_every_group_circle():
    """The circle of a row is centred on the line at the middle of the lon profiles' arclength range and reaches at least half the range
    along the line + the ego's half diagonal + the largest |d sample|: an obstacle on the line's normal through a point of that range,
    closer than the last two terms, is inside it.  All rows x obstacles then survive: 25 x 50 = 1250 > 512."""
    b = P.CASES["more survivors than the list holds"]()
    reach = 0.5 * math.hypot(b.veh_l, b.veh_w) + np.abs(b.d_samples).max()
    assert math.hypot(P.CONVOY_DS, P.CONVOY_D) < 0.9 * reach
    assert rows_of(b) * b.n_obs > 512
    for e in range(b.B):
        s = P.lon_positions(b, e)
        mean = np.nanmean(s, axis=0)
        assert (mean >= np.nanmin(s, axis=0) - 1e-9).all() and (mean <= np.nanmax(s, axis=0) + 1e-9).all()  # (equal at step 0, up to the mean's rounding)
        f = int(b.frame_of[e])
        assert mean.min() - P.CONVOY_DS > b.knots[f, 0] and mean.max() + P.CONVOY_DS < b.knots[f, int(b.nx[f]) - 1]
