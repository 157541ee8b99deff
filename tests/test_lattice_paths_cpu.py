"""CPU: the harness of the lattice suites (tests/lattice_paths.py) against a stub engine that answers with the oracle's own plan of a
tiny batch (2 egos, 5 x 4 x 3, four obstacles, one ego without a feasible candidate) or with that plan and ONE corruption: the plan passes, every corruption is refused, the
ctx options are back at their defaults either way, and each plan_dense call ran under DEFAULTS overlaid with its mode's options."""
from types import SimpleNamespace

import numpy as np
import pytest

import lattice_paths as L
import prologue_cases as P
from fiss_plus_planner_amd import synth

SKIP = np.array([0, 1], dtype=np.int32)


@pytest.fixture(scope="module")
def tiny(oracle):
    batch = P.park(synth.make_batch(2, 5, 4, 3, 4, 40, True, 9900, layout="survey8d"), [0], ahead=6.0)  # (ego 0 is blocked, ego 1 is not)
    ref = L.reference(oracle, batch)
    assert ref[0].best_idx < 0 <= ref[1].best_idx and 0 < L.colliding(ref) < batch.B * batch.C
    return batch, ref


class Stub:
    """The engine as the harness sees it: options, launch counters, plan_dense; `spoil` edits the answer, `stuck` freezes the counters."""

    def __init__(self, ref, spoil=None, stuck=False):
        self.ref, self.spoil, self.stuck = ref, spoil, stuck
        self.opts, self.calls, self.seen = dict(L.DEFAULTS), 0, []

    def set_option(self, name, value):
        assert name in L.DEFAULTS, name
        self.opts[name] = value

    def get_option(self, name):
        return (0 if self.stuck else self.calls) if name.startswith("lattice_launches") else self.opts[name]

    def answer(self, skip=None):
        out = SimpleNamespace(best_idx=np.array([r.best_idx for r in self.ref], dtype=np.int32), best_cost=np.array([r.cost[r.best_idx] if r.best_idx >= 0 else np.nan for r in self.ref]),
                              stats=np.stack([r.stats for r in self.ref]), cost=np.stack([r.cost for r in self.ref]), flags=np.stack([r.flags for r in self.ref]))
        if skip is not None:  # (a skipped ego: -1 / NaN, its rows as the caller left them)
            for a, fill in ((out.best_idx, -1), (out.best_cost, np.nan), (out.stats, 0), (out.cost, 0.0), (out.flags, 0)):
                a[skip != 0] = fill
        if self.spoil:
            self.spoil(out)
        return out

    def plan_dense(self, batch, winner=False):
        self.calls += 1
        self.seen.append(dict(self.opts))
        return self.answer()

    def device_call(self, engine, batch, order, skip):
        assert engine is self
        self.calls += 1
        out = self.answer(skip)
        return out.best_idx, out.best_cost, out.stats, out.cost, out.flags


def finite(out, e):
    return int(np.nonzero(np.isfinite(out.cost[e]))[0][0])


def moved(delta, relative=False):
    def spoil(out):
        c = finite(out, 1)
        out.cost[1, c] += delta * (max(1.0, abs(out.cost[1, c])) if relative else 1.0)
    return spoil


def flag(out):
    out.flags[1, 7] ^= 4


def stat(out):
    out.stats[0, 2] += 1


def nan(out):
    out.cost[0, finite(out, 0)] = np.nan


def idx(out):
    out.best_idx[1] += 1


def selected(out):
    out.best_cost[1] += 2e-9


def woken(out):
    out.best_idx[1] = 0


CORRUPTIONS = {"a flag word flipped": flag, "a Stats entry changed": stat, "a cost moved by 2e-9": moved(2e-9), "a NaN cost": nan, "best_idx off by one": idx,
               "the selected cost moved by 2e-9": selected}
MOVES = {"abs1e-9": (moved(2e-9), moved(0.5e-9)), "abs1e-6": (moved(2e-6), moved(0.5e-6)), "relative": (moved(2e-9, True), moved(0.5e-9, True))}


def test_the_oracles_own_answer_passes_and_every_call_runs_under_its_modes_options(oracle, tiny, monkeypatch):
    batch, ref = tiny
    stub = Stub(ref)
    modes = L.MODES + L.TAIL + L.GROUPED
    assert L.through_modes(ref, stub, batch, "tiny", modes) is ref
    assert stub.seen == [{**L.DEFAULTS, **opts} for _, opts, _ in modes] and stub.opts == L.DEFAULTS
    monkeypatch.setattr(L, "device_call", stub.device_call)
    L.device_entry_matches(stub, batch, ref, "tiny")
    L.device_entry_matches(stub, batch, ref, "tiny", skip=SKIP)
    for cost in L.COST_MODES:
        L.compare(stub.answer(), ref, "tiny", cost=cost)
    L.shaped_case(oracle, stub, batch, "tiny", None, L.MODES)
    with pytest.raises(AssertionError, match="compiled-in"):
        L.shaped_case(oracle, stub, batch, "tiny", L.SHAPE_555, L.MODES)
    assert stub.opts == L.DEFAULTS


@pytest.mark.parametrize("what", list(CORRUPTIONS))
def test_a_single_corruption_is_refused(tiny, monkeypatch, what):
    batch, ref = tiny
    stub = Stub(ref, CORRUPTIONS[what])
    with pytest.raises(AssertionError, match="tiny"):
        L.through_modes(ref, stub, batch, "tiny", L.TAIL)
    assert len(stub.seen) == 1 and stub.seen[0] == {**L.DEFAULTS, **L.TAIL[0][1]} and stub.opts == L.DEFAULTS
    monkeypatch.setattr(L, "device_call", stub.device_call)
    with pytest.raises(AssertionError, match="device entry point"):
        L.device_entry_matches(stub, batch, ref, "tiny")
    for cost in L.COST_MODES:
        if "2e-9" not in what or cost == "abs1e-9":  # (the other modes' moves: the test below)
            with pytest.raises(AssertionError):
                L.compare(stub.answer(), ref, "tiny", cost=cost)


@pytest.mark.parametrize("cost", list(L.COST_MODES))
def test_a_cost_beyond_the_modes_tolerance_is_refused_and_one_inside_it_passes(tiny, cost):
    """Twice the tolerance is refused, half of it passes (relative: of max(1, |cost|))."""
    batch, ref = tiny
    beyond, inside = MOVES[cost]
    with pytest.raises(AssertionError, match="beyond"):
        L.through_modes(ref, Stub(ref, beyond), batch, "tiny", L.MODES, cost=cost)
    L.through_modes(ref, Stub(ref, inside), batch, "tiny", L.MODES, cost=cost)


def test_stats_are_compared_unless_the_caller_says_otherwise(tiny):
    batch, ref = tiny
    L.through_modes(ref, Stub(ref, stat), batch, "tiny", L.MODES, stats=False)


def test_a_skipped_ego_with_an_index_is_refused(tiny, monkeypatch):
    batch, ref = tiny
    stub = Stub(ref, woken)
    monkeypatch.setattr(L, "device_call", stub.device_call)
    with pytest.raises(AssertionError, match="skipped"):
        L.device_entry_matches(stub, batch, ref, "tiny", skip=SKIP)


def test_a_counter_that_does_not_move_is_refused(tiny):
    batch, ref = tiny
    stub = Stub(ref, stuck=True)
    with pytest.raises(AssertionError, match="did not take its instance"):
        L.through_modes(ref, stub, batch, "tiny", L.MODES)
    assert stub.opts == L.DEFAULTS
    L.through_modes(ref, stub, batch, "tiny", [L.MODES[4]])  # (the lane-per-candidate kernel has no counter)


def test_options_restores_every_default_when_the_body_raises():
    stub = Stub(None)
    with pytest.raises(KeyError):
        with L.options(stub, {"lattice_tail": 4, "lattice_order": 0, "fiss_fused": 0}):
            assert stub.opts == {**L.DEFAULTS, "lattice_tail": 4, "lattice_order": 0, "fiss_fused": 0}
            raise KeyError
    assert stub.opts == L.DEFAULTS
    assert L.DEFAULTS == {**dict.fromkeys(L.DEFAULTS, 0), "lattice_order": 1, "fiss_fused": 1}


def test_modes_for(tiny):
    assert L.modes_for(L.SHAPE_555) == L.TWO_PER_CU and L.modes_for(L.SHAPE_997) == L.MODES + L.TAIL
    assert L.modes_for(L.SHAPE_997, tail=False) == L.MODES and L.modes_for(tiny[0]) == L.MODES + L.TAIL
    assert [m[2] for m in L.TWO_PER_CU] == ["lattice_launches_2", "lattice_launches_2", None]
    assert len(L.fiss_twin_modes()) == 3 and len(L.fiss_twin_modes(no_tail_split=True)) == 4
    assert L.shape_of(tiny[0])[:3] == (5, 4, 3)
