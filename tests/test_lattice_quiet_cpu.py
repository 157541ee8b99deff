"""CPU: tests/lattice_quiet.py's comparison accepts the oracle's selection and refuses single corruptions of it (no engine, no GPU)."""
from types import SimpleNamespace

import numpy as np
import pytest

import lattice_quiet as Q

REF = [SimpleNamespace(best_idx=2, cost=np.array([3.0, np.nan, 1.5]), stats=np.array([0, 3, 3, 3])),
       SimpleNamespace(best_idx=-1, cost=np.array([np.nan, np.nan, np.nan]), stats=np.array([0, 3, 3, 3]))]


def _out(**kw):
    out = dict(idx=np.array([2, -1]), cost=np.array([1.5, np.nan]), stats=np.array([[0, 3, 3, 3], [0, 3, 3, 3]]))
    out.update(kw)
    return out["idx"], out["cost"], out["stats"]


def test_the_oracles_selection_passes():
    Q.quiet_compare(_out(), REF, "tiny")
    Q.quiet_compare(_out(cost=np.array([1.5 + 5e-10, np.nan])), REF, "tiny")


@pytest.mark.parametrize("what,kw", [
    ("an index where the oracle has none", dict(idx=np.array([2, 0]))),
    ("no index where the oracle has one", dict(idx=np.array([-1, -1]))),
    ("the selected cost moved by 2e-9", dict(cost=np.array([1.5 + 2e-9, np.nan]))),
    ("a NaN where the oracle has a cost", dict(cost=np.array([np.nan, np.nan]))),
    ("a cost where the oracle has none", dict(cost=np.array([1.5, 0.0]))),
    ("a Stats entry changed", dict(stats=np.array([[0, 3, 3, 3], [0, 3, 2, 3]]))),
    ("an ego missing", dict(idx=np.array([2]))),
])
def test_a_single_corruption_is_refused(what, kw):
    with pytest.raises(AssertionError):
        Q.quiet_compare(_out(**kw), REF, what)
