"""CPU: the fixtures of tests/indirection.py proved on the references alone (numpy + the CPU oracle; nothing here calls the library).

1. every reference gives the same bits for a batch, for reindex(batch) and for expand(batch): the transformations change the addressing
   and nothing else (and the references do index through frame_of / scene_of / nx);
2. every reference's own caps hold on the shared and the ragged fixtures (the undecided counts are printed);
3. the fixtures reach what they exist for."""
import dataclasses
import functools

import numpy as np
import pytest

import boundary_ref as BR
import clearance_ref as CR
import envelope_ref as ER
import fallback_ref as FR
import fiss_rules_ref as FRR
import gaps_ref as PR
import gates_ref as GR
import indirection as IX
import margins_ref as MR
import rules_eval_ref as R


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def stacked(refs, fields):
    """{field: array} of a reference's result: a namespace, or one namespace per ego."""
    if isinstance(refs, (list, tuple)) and not isinstance(refs[0], np.ndarray):
        return {k: np.stack([np.asarray(getattr(r, k)) for r in refs]) for k in fields}
    return {k: np.asarray(getattr(refs, k)) for k in fields}


@functools.lru_cache(maxsize=None)
def rules_batch(sharing=2, nx=0, shapes=False):
    return IX.rules_batch(sharing, nx, shapes)


def shaped_batch():
    return IX.rules_batch(2, 0, True)


@functools.lru_cache(maxsize=None)
def lattice_rules(O, sharing=2, nx=0, shapes=False):
    b = rules_batch(sharing, nx, shapes)
    return R.batch_rules(O, b, R.lattice_end_states(b))


@functools.lru_cache(maxsize=None)
def fallback_of(O, name):
    c = IX.fallback_case(name)
    return c, FR.fallback(O, c.batch, c.stop_T, c.d_targets, c.max_decel, best_idx=c.best_idx, skip=c.skip)


# ---------------------------------------------------------------- 1. invariance
def _table_ref(mod, fn, fields):
    return lambda O, b: stacked(getattr(mod, fn)(O, b), fields)


def _rules(O, b):
    out = stacked(R.batch_rules(O, b, R.lattice_end_states(b)), ("flags_in", "flags", "rule_bits", "counts", "slack"))
    off = stacked(R.batch_rules(O, b, R.off_lattice(b), skip=R.off_skip(b)), ("flags_in", "flags", "rule_bits", "counts", "slack"))
    out.update({"off_" + k: v for k, v in off.items()})
    return out


def _margins(O, b):
    return stacked(MR.margins(O, b, best_idx=IX.margin_planes(b), pose_stride=b.check_stride), ("min_dist", "min_step", "min_obs", "gap", "n_pairs", "M"))


def _fiss(O, b):
    return stacked(FRR.batch_plan(O, b, "FISS+", FRR.NAMES), ("best_ijk", "end_state", "best_cost", "refined", "stats", "rejected", "slack", "cost_gap"))


def _clearance(O, b):
    cost, flags, bi, bc = CR.batch_tables(O, b, w_obstacle=IX.W_OBSTACLE)
    return dict(cost=cost, flags=flags, best_idx=bi, best_cost=bc)


def _fallback(name):
    def run(O, c):
        return stacked(FR.fallback(O, c.batch, c.stop_T, c.d_targets, c.max_decel, best_idx=c.best_idx, skip=c.skip),
                       ("end_state", "status", "fb_idx", "hit_step", "hit_obs", "hit_speed", "cand", "counts", "slack", "stable", "N", "M"))
    return run


REFS = {
    "envelope": (rules_batch, _table_ref(ER, "batch_envelope", ("cost", "flags_in", "flags", "bit_a", "bit_b", "slack", "best_idx"))),
    "gates": (rules_batch, _table_ref(GR, "batch_gates", ("flags", "gated", "step", "slack", "best_idx"))),
    "boundary": (rules_batch, _table_ref(BR, "batch_mask", ("flags", "bit", "slack", "best_idx"))),
    "gaps": (rules_batch, _table_ref(PR, "batch_gaps", ("flags", "close", "slack", "best_idx"))),
    "rules_eval": (rules_batch, _rules),
    "margins": (rules_batch, _margins),
    "clearance": (rules_batch, _clearance),
    "gaps, polygon columns": (shaped_batch, _table_ref(PR, "batch_gaps", ("flags", "close", "slack", "best_idx"))),
    "rules_eval, polygon columns": (shaped_batch, _rules),
    "margins, polygon columns": (shaped_batch, _margins),
    "clearance, polygon columns": (shaped_batch, _clearance),
    "fiss_rules": (IX.fiss_batch, _fiss),
    "fallback base": (lambda: IX.fallback_case("base"), _fallback("base")),
    "fallback rings": (lambda: IX.fallback_case("rings"), _fallback("rings")),
    "fallback ties": (lambda: IX.fallback_case("ties"), _fallback("ties")),
}


@pytest.mark.parametrize("name", list(REFS))
def test_reference_is_invariant_under_reindex_and_expand(oracle, name):
    make, run = REFS[name]
    x = make()
    batch_of = (lambda v: v.batch) if name.startswith("fallback") else (lambda v: v)
    with_batch = IX.with_batch if name.startswith("fallback") else (lambda v, b: b)
    base = run(oracle, x)
    b = batch_of(x)
    assert not np.array_equal(b.frame_of, np.arange(b.B)) and (b.nx < b.NX).any(), name  # the fixture itself is shared and ragged
    for what, twin in (("reindex", IX.reindex(b, IX.SEED)), ("expand", IX.expand(b))):
        if what == "reindex":  # no ego keeps its index as its row, in either table; the decoys are there
            assert (twin.frame_of != np.arange(b.B)).all() and (twin.scene_of != np.arange(b.B)).all(), name
            assert twin.F >= b.B + 2 and twin.NX == b.NX + IX.PAD and len(twin.meta["decoy_frames"]) >= 2, name
            assert twin.S == 0 or (twin.S >= b.B + 2 and len(twin.meta["decoy_scenes"]) >= 2), name
        else:
            assert np.array_equal(twin.frame_of, np.arange(b.B)) and twin.F == b.B, name
        got = run(oracle, with_batch(x, twin))
        diff = [k for k in base if not same(base[k], got[k])]
        print(f"{name}: {what}: {len(base)} outputs, {len(diff)} differ")
        assert not diff, (name, what, diff)


# ---------------------------------------------------------------- 2. the references' caps on the shared and the ragged fixtures
FIXTURES = [(s, n, False) for s in range(len(IX.SHARINGS)) for n in (None, 0, 1)] + [(2, 0, True)]


@pytest.mark.parametrize("sharing,nx,shapes", FIXTURES, ids=[f"sharing{s}-nx{n}{'-shapes' if p else ''}" for s, n, p in FIXTURES])
def test_rules_caps_hold(oracle, sharing, nx, shapes):
    b = rules_batch(sharing, nx, shapes)
    ref = lattice_rules(oracle, sharing, nx, shapes)
    und, egos = R.check_caps(ref, f"lattice {sharing} {nx}")
    off = R.batch_rules(oracle, b, R.off_lattice(b), skip=R.off_skip(b))
    und_off, egos_off = R.check_caps(off, f"off-lattice {sharing} {nx}")
    seen = int(np.bitwise_or.reduce(ref.rule_bits.ravel()))
    print(f"sharing {sharing}, nx {nx}: undecided {und} of {ref.undecided.size} lattice / {und_off} of {off.undecided.size} off-lattice trajectories, rule bits seen {seen}")
    assert seen == 31, (sharing, nx, seen)


@pytest.mark.parametrize("rule", ["envelope", "gates", "boundary", "gaps"])
def test_table_pass_caps_hold(oracle, rule):
    mod, fn = {"envelope": (ER, "batch_envelope"), "gates": (GR, "batch_gates"), "boundary": (BR, "batch_mask"), "gaps": (PR, "batch_gaps")}[rule]
    for sharing, nx, shapes in ((2, 0, False), (0, 1, False)) + (((2, 0, True),) if rule == "gaps" else ()):
        refs = getattr(mod, fn)(oracle, rules_batch(sharing, nx, shapes))
        und, egos = mod.check_caps(refs, f"{rule} {sharing} {nx} {shapes}")
        print(f"{rule}: sharing {sharing}, nx {nx}, polygon columns {shapes}: {und} undecided candidates, {egos} egos excluded")


@pytest.mark.parametrize("name", ["base", "rings", "ties"])
def test_fallback_caps_hold(oracle, name):
    c, ref = fallback_of(oracle, name)
    left_out = int((ref.need & ~ref.counted).sum())
    print(f"fallback {name}: {left_out} of {int(ref.need.sum())} fallback egos left out, status {ref.status.tolist()}")
    assert left_out <= FR.MAX_LEFT_OUT, (name, left_out)


def test_fiss_rules_and_margins_caps_hold(oracle):
    for kind, names in IX.FISS_CASES:
        refs = FRR.batch_plan(oracle, IX.fiss_batch(), kind, names, key="indirection")
        egos = FRR.check_caps(refs, "fiss_rules, shared and ragged")
        planned = sum(r.best_ijk[0] >= 0 for r in refs)
        print(f"fiss_rules {kind} {'+'.join(names)}: {egos} egos undecided, {planned} of {len(refs)} planned, {sum(r.refined for r in refs)} refined, rejected {[r.rejected for r in refs]}")
        assert 0 < planned and (kind == "FISS" or any(r.rejected for r in refs))
    for shapes in (False, True):
        b = rules_batch(2, 0, shapes)
        m = MR.margins(oracle, b, best_idx=IX.margin_planes(b), pose_stride=b.check_stride)
        ok, share = MR.decidable(m)
        print(f"margins, polygon columns {shapes}: no pair distance in (0, {MR.DECIDE_TOL}): {ok}; {share:.3f} of the plans with a pair count")
        assert ok and share >= MR.MIN_COUNTED


# ---------------------------------------------------------------- 3. the fixtures reach what they exist for
def test_a_truncated_line_ends_trajectories(oracle):
    cut, full = lattice_rules(oracle, 2, 0), lattice_rules(oracle, 2, None)
    N, M, M_full = (cut.flags_in >> 8) & 0xFFF, cut.flags_in >> 20, full.flags_in >> 20
    only_cut = (M < N) & (M_full == N)
    print(f"M < N only because of the cut: {only_cut.sum(axis=1).tolist()} candidates per ego; {int((cut.flags != full.flags).sum())} flag words differ")
    assert only_cut.any() and (cut.flags != full.flags).any()


def test_egos_on_one_frame_get_different_gate_verdicts(oracle):
    b, ref = rules_batch(), lattice_rules(oracle)
    gate = (ref.rule_bits & R.RULE_GATE) != 0
    pairs = [(i, j) for i in range(b.B) for j in range(i + 1, b.B) if b.frame_of[i] == b.frame_of[j]]
    differ = [(i, j) for i, j in pairs if gate[i].any() and gate[j].any() and not np.array_equal(gate[i], gate[j])]
    print(f"egos on one frame: {pairs}, with different non-empty gate verdicts: {differ}")
    assert differ


def test_egos_on_one_scene_depend_on_their_own_clock(oracle):
    """Two egos of one scene at different t_now: give the later one the earlier one's clock, and its gap or collision verdicts change."""
    b, ref = rules_batch(), lattice_rules(oracle)
    pairs = [(i, j) for i in range(b.B) for j in range(b.B) if i != j and b.scene_of[i] == b.scene_of[j] >= 0 and b.t_now[i] != b.t_now[j]]
    assert pairs
    changed = 0
    for i, j in pairs:
        t = b.t_now.copy()
        t[j] = t[i]
        other = R.batch_rules(oracle, dataclasses.replace(b, t_now=t), R.lattice_end_states(b), skip=np.arange(b.B) != j)
        mask = np.uint32(R.FLAG_COLLISION)
        changed += int(((other.flags[j] ^ ref.flags[j]) & mask).any() or ((other.rule_bits[j] ^ ref.rule_bits[j]) & R.RULE_GAP).any())
    print(f"{changed} of {len(pairs)} (ego, clock) swaps on a shared scene change a gap / collision verdict")
    assert changed


def test_fallback_fixtures_show_every_status_and_a_polygon_in_another_egos_scene(oracle):
    seen = set()
    for name in ("base", "rings", "ties"):
        seen |= set(fallback_of(oracle, name)[1].status.tolist())
    assert {FR.CLEAR, FR.CONTACT, FR.NONE} <= seen, seen
    c, ref = fallback_of(oracle, "rings")
    b = c.batch
    hits = [(e, int(b.scene_of[e]), int(ref.hit_obs[e])) for e in range(b.B)
            if ref.status[e] == FR.CONTACT and ref.counted[e] and b.scene_of[e] != e and b.obs_nvert[b.scene_of[e], ref.hit_obs[e]] > 0]
    print(f"rings: (ego, scene, polygon column hit) with scene != ego: {hits}")
    assert hits
    # ... and the ego's OWN index names a scene whose column of that number is another shape: reading it gives another verdict
    assert any(b.obs_nvert[e, j] != b.obs_nvert[sc, j] or not same(b.obs_poly[e, j], b.obs_poly[sc, j]) for e, sc, j in hits)


def test_a_decoy_row_changes_a_verdict_of_every_rule(oracle):
    b, ref = rules_batch(), lattice_rules(oracle)
    twin = IX.reindex(b, IX.SEED)
    es = R.lattice_end_states(b)
    df, ds = twin.meta["decoy_frames"], twin.meta["decoy_scenes"]
    wrong_frame = R.batch_rules(oracle, IX.misdirect(twin, egos_frame={e: df[e % len(df)] for e in range(b.B)}), es, names=("envelope", "gates", "boundary"))
    # the scene alone is wrong: the end states keep their own words (N, M and the collision verdict of the right scene)
    wrong_scene = R.batch_rules(oracle, IX.misdirect(twin, egos_scene={e: ds[e % len(ds)] for e in range(b.B) if b.scene_of[e] >= 0}), es, flags=ref.flags_in, names=("gaps",))
    right_gap = R.batch_rules(oracle, twin, es, flags=ref.flags_in, names=("gaps",))
    changed = {}
    for name, bit in (("limit", R.RULE_LIMIT), ("lateral", R.RULE_LATERAL), ("gate", R.RULE_GATE), ("boundary", R.RULE_BOUNDARY)):
        changed[name] = int((((wrong_frame.rule_bits ^ ref.rule_bits) & bit) != 0).sum())
    changed["gap"] = int((((wrong_scene.rule_bits ^ right_gap.rule_bits) & R.RULE_GAP) != 0).sum())
    print(f"verdicts a decoy row changes, per rule: {changed}")
    assert all(changed.values()), changed
