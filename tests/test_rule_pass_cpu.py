"""CPU: the shared check_against of tests/rule_pass.py is as strict as the per-rule copies it replaced.  For one case per rule the answer
the reference itself would give is accepted, and every single corruption of it below is refused - which also shows that each rule's row
of rule_pass.PASSES (mask, flag law, count law, count field) is the one check_against applies."""
import numpy as np
import pytest

import rule_pass as RP
from fiss_plus_planner_amd import _abi

CASE = {"envelope": "both", "gates": "base", "boundary": "base", "gaps": "base"}
SKIPPED = 2     # the ego the skip corruptions skip
OUTSIDE = 1 << 31  # a bit no pass may touch (the top bit of M, clear in every word of the cases: flipping it adds a bit)


def answer(rule, refs, skip_ego=None):
    """-> (dense, got, skip): the tables the reference read and the outputs it would give, ego `skip_ego` skipped."""
    p = RP.PASSES[rule]
    dense = (np.stack([r.cost for r in refs]), np.stack([r.flags_in for r in refs]).astype(np.uint32))
    got = [np.stack([r.flags for r in refs]).astype(np.uint32), np.array([r.best_idx for r in refs], dtype=np.int32),
           np.array([r.best_cost for r in refs], dtype=np.float64), np.array([getattr(r, p.rule.count) for r in refs], dtype=np.int32)]
    if skip_ego is None:
        return dense, got, None
    got[0][skip_ego], got[1][skip_ego], got[2][skip_ego], got[3][skip_ego] = dense[1][skip_ego], -1, np.nan, 0
    return dense, got, (np.arange(len(refs)) == skip_ego).astype(np.int32)


def pick(refs, cond):
    """The first (ego, candidate) with cond(r)[candidate]."""
    for b, r in enumerate(refs):
        c = np.nonzero(cond(r))[0]
        if len(c):
            return b, int(c[0])
    raise AssertionError("the case has no such candidate")


def alive(r):
    return ((r.flags & np.uint32(_abi.FLAG_INFEASIBLE)) == 0) & ~np.isnan(r.cost)


def decided_ego(refs, cond=lambda r: True):
    return next(b for b, r in enumerate(refs) if not r.undecided.any() and cond(r))


# each: (p, refs, dense, got) -> None, one corruption of `got` in place
def bit_set(p, refs, dense, got):
    b, c = pick(refs, lambda r: ~r.undecided & ((r.flags & p.mask) == 0))
    got[0][b, c] |= np.uint32(int(p.mask) & -int(p.mask))  # (the lowest bit of the mask)


def bit_cleared(p, refs, dense, got):
    b, c = pick(refs, lambda r: ~r.undecided & (((r.flags ^ r.flags_in) & p.mask) != 0))
    got[0][b, c] &= ~((refs[b].flags[c] ^ refs[b].flags_in[c]) & p.mask)


def outside_flipped(p, refs, dense, got):
    got[0][0, 0] ^= np.uint32(OUTSIDE)


def input_bit_cleared(p, refs, dense, got):
    """A bit of the mask where a candidate carried one on entry, else (no candidate of the case does) the lowest bit it did carry."""
    if any(((r.flags_in & p.mask) != 0).any() for r in refs):
        b, c = pick(refs, lambda r: (r.flags_in & p.mask) != 0)
        got[0][b, c] &= ~p.mask
    else:
        word = int(dense[1][0, 0])
        got[0][0, 0] &= ~np.uint32(word & -word)


def count_over(p, refs, dense, got):
    """One more than the count law allows: envelope and gates bound the count by the marked words, boundary and gaps fix it."""
    b = decided_ego(refs)
    marked = np.count_nonzero(got[0][b] & p.mask)
    got[3][b] = marked + 1 if p.rule.name in ("envelope", "gates") else got[3][b] + 1


def count_under(p, refs, dense, got):
    """One fewer than the count law allows: envelope and gates bound the count by the words the call changed."""
    b = decided_ego(refs)
    added = np.count_nonzero(got[0][b] != dense[1][b])
    got[3][b] = added - 1 if p.rule.name in ("envelope", "gates") else got[3][b] - 1


def winner_moved(p, refs, dense, got):
    b = decided_ego(refs, lambda r: alive(r).sum() >= 2)
    c = next(int(c) for c in np.nonzero(alive(refs[b]))[0] if c != refs[b].best_idx)
    got[1][b], got[2][b] = c, dense[0][b, c]


def winner_infeasible(p, refs, dense, got):
    b, c = pick(refs, lambda r: (r.flags & np.uint32(_abi.FLAG_INFEASIBLE)) != 0)
    got[1][b], got[2][b] = c, dense[0][b, c]


def cost_one_ulp(p, refs, dense, got):
    b = next(b for b, r in enumerate(refs) if r.best_idx >= 0)
    got[2][b] = np.nextafter(got[2][b], np.inf)


def no_winner_with_a_cost(p, refs, dense, got):
    b = next(b for b, r in enumerate(refs) if r.best_idx >= 0)
    got[1][b] = -1


def skipped_winner(p, refs, dense, got):
    got[1][SKIPPED] = 0


def skipped_row_changed(p, refs, dense, got):
    got[0][SKIPPED, 0] ^= np.uint32(OUTSIDE)


def skipped_count(p, refs, dense, got):
    got[3][SKIPPED] = 1


CORRUPTIONS = (bit_set, bit_cleared, outside_flipped, input_bit_cleared, count_over, count_under, winner_moved, winner_infeasible, cost_one_ulp,
               no_winner_with_a_cost, skipped_winner, skipped_row_changed, skipped_count)


def corruptions(rule):
    """The corruptions that apply to the rule: a pass that writes its bit has no input bit to lose."""
    return [f for f in CORRUPTIONS if not (f is input_bit_cleared and RP.PASSES[rule].flag_law is RP._written)]


def corrupted(rule, refs, corrupt):
    """-> (dense, got, skip) with the one corruption applied."""
    dense, got, skip = answer(rule, refs, SKIPPED if corrupt.__name__.startswith("skipped") else None)
    before = [a.copy() for a in got]
    corrupt(RP.PASSES[rule], refs, dense, got)
    assert sum(not RP.same_bits(a, b) for a, b in zip(before, got)) >= 1, corrupt.__name__  # (it did change the answer)
    return dense, got, skip


@pytest.mark.parametrize("rule", list(CASE))
def test_the_references_own_answer_is_accepted(oracle, rule):
    refs = RP.PASSES[rule].ref.case(oracle, CASE[rule])[1]
    for skip_ego in (None, SKIPPED):
        dense, got, skip = answer(rule, refs, skip_ego)
        RP.check_against(rule, refs, dense, got, rule, skip)


@pytest.mark.parametrize("rule,corrupt", [(rule, f) for rule in CASE for f in corruptions(rule)], ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_a_single_corruption_is_refused(oracle, rule, corrupt):
    refs = RP.PASSES[rule].ref.case(oracle, CASE[rule])[1]
    dense, got, skip = corrupted(rule, refs, corrupt)
    with pytest.raises(AssertionError):
        RP.check_against(rule, refs, dense, got, corrupt.__name__, skip)
