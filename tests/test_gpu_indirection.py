"""GPU: the rule, margin, fallback and rescoring kernels on shared, permuted, ragged frames (tests/indirection.py; the fixtures are proved
on the references alone by tests/test_indirection_cpu.py).

  1. twins: every entry point gives the same bits for a shared, ragged batch, for reindex(batch) - the same problems behind permuted
     frame and scene rows, hostile decoy rows and a wider NX - and for expand(batch), its one-frame-one-scene-per-ego form; in
     FP_MEM_HOST and on resident data (the sibling suites' Resident helpers);
  2. the same fixtures against the references, with each sibling suite's own comparison, tolerances and caps;
  3. closed loops of 6 cycles, eager and replayed from a graph, on the shared batch and its twins.

A kernel that addresses a per-frame table by the ego index reads a decoy in (1) and another ego's row in (2); one that addresses a
per-scene table that way likewise; one that takes NX for nx[f] reads the poison behind the cut.  The rule fixtures run twice, as drawn
(rectangle columns) and with some columns turned into polygons: obs_nvert / obs_poly are read only where a batch has polygon columns,
and a shape taken from a decoy row is a triangle one millimetre across."""
import dataclasses

import numpy as np
import pytest

import boundary_ref as BR
import envelope_ref as ER
import fallback_cases as FC
import fallback_ref as FR
import fiss_rules_ref as FRR
import gaps_ref as PR
import gates_ref as GR
import indirection as IX
import margins_ref as MR
import rule_pass as RP
import rules_eval_ref as R
import test_gpu_clearance as TC
import test_gpu_fallback as TF
import test_gpu_fiss_rules as TFR
import test_gpu_margins as TM
import test_gpu_rules_eval as TR
from fiss_plus_planner_amd import rules
from fiss_plus_planner_amd.fallback import FallbackStop

pytestmark = pytest.mark.gpu
NAMES = R.RULE_NAMES
PASSES = {"envelope": (ER, "batch_envelope"), "gates": (GR, "batch_gates"), "boundary": (BR, "batch_mask"), "gaps": (PR, "batch_gaps")}
LOOP_CYCLES = 6
SHAPES = pytest.mark.parametrize("shapes", [False, True], ids=["rectangles", "polygon columns"])  # (the fixture with_shapes() went over first)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def twins(batch):
    return {"batch": batch, "reindex": IX.reindex(batch, IX.SEED), "expand": IX.expand(batch)}


def assert_twins(run, variants, what):
    """run(variant) -> {name: array}, every array per ego: the same bits for every variant.  -> the first variant's outputs."""
    names = list(variants)
    want = run(variants[names[0]])
    for name in names[1:]:
        got = run(variants[name])
        diff = [k for k in want if not same_bits(want[k], got[k])]
        assert not diff, (what, name, diff)
    return want


def stop():
    return FallbackStop(FC.STOP_T, FC.D3)


def fields(ns, keys):
    return {k: getattr(ns, k) for k in keys}


# ---------------------------------------------------------------- 1. twins
@SHAPES
def test_twins_dense_chain_and_fallback_host(engine, shapes):
    def run(b):
        out = engine.plan_dense(b, tables=True, winner=True, envelope=True, gates=True, boundary=True, gaps=True, fallback=stop())
        got = fields(out, ("cost", "flags", "best_idx", "best_cost", "best_flags", "best_traj") + tuple(r.count for r in rules.TABLE))
        got.update({"fallback_" + k: getattr(out.fallback, k) for k in ("end_state", "status", "fb_idx", "hit_step", "hit_obs", "hit_speed", "counts")})
        return got

    out = assert_twins(run, twins(IX.rules_batch(shapes=shapes)), "plan_dense, four passes, fallback")
    assert all(out[r.count].any() for r in rules.TABLE)  # every pass flagged something


@SHAPES
@pytest.mark.parametrize("rule", list(PASSES))
def test_twins_one_pass_host_and_device(engine, rule, shapes):
    method = RP.PASSES[rule].method

    def run(b):
        dense = engine.plan_dense(b, tables=True)
        host = getattr(engine, method)(b, dense.cost, dense.flags)
        res = RP.Resident(engine, rule, b)
        res.pair()
        dev = res.fetch()
        for h, d in zip(host, dev):
            assert same_bits(h, d), rule  # FP_MEM_DEVICE equals FP_MEM_HOST
        return dict(zip(("flags", "best_idx", "best_cost", "count"), host), cost=dense.cost)

    out = assert_twins(run, twins(IX.rules_batch(shapes=shapes)), rule)
    assert out["count"].any()


@SHAPES
def test_twins_rules_eval_host_and_device(engine, shapes):
    base = IX.rules_batch(shapes=shapes)
    lat, off, skip = R.lattice_end_states(base), R.off_lattice(base), R.off_skip(base)

    def run(b):
        got = {}
        for what, es, sk in (("lattice", lat, None), ("off", off, skip)):
            words = engine.eval_trajs(b, es).flags
            h = engine.rules_eval(b, es, words, skip=sk)
            d = TR.Resident(engine, b, es, words, skip=sk)
            d.call()
            for x, y in zip((h.flags, h.rule_bits, h.counts), d.fetch()):
                assert same_bits(x, y), what
            got.update({f"{what}_{k}": v for k, v in (("words", words), ("flags", h.flags), ("rule_bits", h.rule_bits), ("counts", h.counts))})
        return got

    out = assert_twins(run, twins(base), "rules_eval")
    assert int(np.bitwise_or.reduce(out["lattice_rule_bits"].ravel())) == 31


def margins_device(engine, batch, planes):
    import torch

    from fiss_plus_planner_amd.device_batch import DeviceBatch

    db = DeviceBatch(batch, 0, order_hint=False)
    K, B = planes.shape
    bi = torch.from_numpy(np.ascontiguousarray(planes, dtype=np.int32)).to(db.dev)
    md, ms, mo = db.empty((K, B), torch.float64), db.empty((K, B), torch.int32), db.empty((K, B), torch.int32)
    engine.traj_margins_device(db.params, db.fb, K, md.data_ptr(), ms.data_ptr(), mo.data_ptr(), best_idx=bi.data_ptr(), pose_stride=int(batch.check_stride),
                               stream=torch.cuda.current_stream(db.dev).cuda_stream)
    torch.cuda.synchronize(db.dev)
    return md.cpu().numpy(), ms.cpu().numpy(), mo.cpu().numpy()


@SHAPES
def test_twins_traj_margins_host_and_device(engine, shapes):
    base = IX.rules_batch(shapes=shapes)
    planes = IX.margin_planes(base)

    def run(b):
        host = engine.traj_margins(b, best_idx=planes, pose_stride=b.check_stride)
        for h, d in zip(host, margins_device(engine, b, planes)):
            assert same_bits(h, d)
        return dict(zip(("min_dist", "min_step", "min_obs"), host))

    out = assert_twins(run, twins(base), "traj_margins")
    assert np.isfinite(out["min_dist"]).any()


@pytest.mark.parametrize("name", ["base", "rings", "ties"])
def test_twins_fallback_stop_host_and_device(engine, name):
    c = IX.fallback_case(name)

    def run(b):
        v = IX.with_batch(c, b)
        h = TF.host(engine, v)
        TF.same_bits(h, TF.device(engine, v), f"{name}: host / device")
        return fields(h, TF.OUTS)

    assert_twins(run, twins(c.batch), f"fallback_stop {name}")


@SHAPES
@pytest.mark.parametrize("kind,names", IX.FISS_CASES, ids=IX.FISS_IDS)
def test_twins_plan_fiss_enforce_host_and_device(engine, kind, names, shapes):
    def run(b):
        h = engine.plan_fiss(b, kind, enforce=names, winner=True)
        d = TFR.Resident(engine, b, kind, names)
        d.call()
        dev = d.fetch()
        for k in TFR.OUT_KEYS + ("rejected",):
            assert same_bits(getattr(h, k), dev[k]), (kind, k)
        return fields(h, TFR.OUT_KEYS + ("rejected", "best_flags", "best_traj"))

    out = assert_twins(run, twins(IX.fiss_batch(shapes)), f"plan_fiss {kind}")
    assert (out["best_ijk"][:, 0] >= 0).any()


def weighted(b):
    return dataclasses.replace(b, w_obstacle=IX.W_OBSTACLE)


@SHAPES
def test_twins_clearance_rescoring_host_and_device(engine, shapes):
    def run(b):
        b = weighted(b)
        n0 = engine.get_option("clearance_launches")
        h = engine.plan_dense(b, tables=True, winner=True)
        assert engine.get_option("clearance_launches") == n0 + 1
        res = RP.Resident(engine, "gaps", b)
        res.dense()
        flags = res.fetch()[0]
        assert same_bits(flags, h.flags) and same_bits(res.cost.cpu().numpy(), h.cost) and same_bits(res.bi0.cpu().numpy(), h.best_idx)
        assert same_bits(res.bc0.cpu().numpy(), h.best_cost)
        return fields(h, ("cost", "flags", "best_idx", "best_cost", "best_flags", "best_traj"))

    base = IX.rules_batch(shapes=shapes)
    out = assert_twins(run, twins(base), "clearance rescoring")
    plain = engine.plan_dense(base, tables=True)
    assert not same_bits(out["cost"], plain.cost)  # the term re-priced survivors


# ---------------------------------------------------------------- 2. against the references, on the shared and ragged fixture
@SHAPES
def test_chain_of_four_passes_against_the_reference(engine, oracle, shapes):
    batch = IX.rules_batch(shapes=shapes)
    es = R.lattice_end_states(batch)
    words = engine.eval_trajs(batch, es).flags
    table = engine.plan_dense(batch, tables=True, envelope=True, gates=True, boundary=True, gaps=True).flags
    ref = R.batch_rules(oracle, batch, es, words)
    und, egos = R.check_caps(ref, "chain, shared and ragged")
    print(f"chain of four passes: {und} undecided of {ref.undecided.size}")
    assert np.array_equal(words, ref_words(oracle, batch, es))  # (the words are the oracle's own)
    ok = ~ref.undecided
    assert np.array_equal(table[ok], ref.flags[ok])
    got = engine.rules_eval(batch, es, words)
    assert np.array_equal(got.flags[ok], ref.flags[ok]) and np.array_equal(got.rule_bits[ok], ref.rule_bits[ok])
    assert int(np.bitwise_or.reduce(got.rule_bits.ravel())) == 31
    for b in range(batch.B):
        if ok[b].all():
            assert np.array_equal(got.counts[b], ref.counts[b]), b


def ref_words(oracle, batch, es):
    return R.batch_rules(oracle, batch, es, names=()).flags_in


@pytest.mark.parametrize("rule", list(PASSES))
def test_one_pass_against_its_reference(engine, oracle, rule):
    (mod, fn), method = PASSES[rule], RP.PASSES[rule].method
    for sharing, nx, shapes in ((2, 0, False), (0, 1, False)) + (((2, 0, True),) if rule == "gaps" else ()):
        batch = IX.rules_batch(sharing, nx, shapes)
        refs = getattr(mod, fn)(oracle, batch)
        dense = engine.plan_dense(batch, tables=True)
        got = getattr(engine, method)(batch, dense.cost, dense.flags)
        RP.check_against(rule, refs, (dense.cost, dense.flags), got, f"{rule}, sharing {sharing}, nx list {nx}, polygon columns {shapes}")
        assert got[3].sum() > 0, rule


@SHAPES
def test_rules_eval_off_the_lattice_against_the_reference(engine, oracle, shapes):
    batch = IX.rules_batch(shapes=shapes)
    es, skip = R.off_lattice(batch), R.off_skip(batch)
    words = engine.eval_trajs(batch, es).flags
    ref = R.batch_rules(oracle, batch, es, words, skip=skip)
    R.check_caps(ref, "off-lattice, shared and ragged")
    acc = np.full((batch.B, 5), 3, dtype=np.int32)
    got = engine.rules_eval(batch, es, words, skip=skip, counts=acc)
    ok = ~ref.undecided
    assert np.array_equal(got.flags[ok], ref.flags[ok]) and np.array_equal(got.rule_bits[ok], ref.rule_bits[ok])
    assert np.array_equal(got.flags[R.OFF_SKIP], words[R.OFF_SKIP]) and not got.rule_bits[R.OFF_SKIP].any() and (got.counts[R.OFF_SKIP] == 3).all()
    assert got.flags[R.OFF_NAN] == words[R.OFF_NAN] and got.rule_bits[R.OFF_NAN] == 0
    for b in range(batch.B):
        if ok[b].all():
            assert np.array_equal(got.counts[b], ref.counts[b] + 3), b
    assert got.rule_bits.any()


@SHAPES
def test_traj_margins_against_the_reference(engine, oracle, shapes):
    batch = IX.rules_batch(shapes=shapes)
    planes = IX.margin_planes(batch)
    ref = MR.margins(oracle, batch, best_idx=planes, pose_stride=batch.check_stride)
    got = engine.traj_margins(batch, best_idx=planes, pose_stride=batch.check_stride)
    TM.assert_margins(got, ref, "margins, shared and ragged")
    assert np.isnan(got[0][1, batch.B - 1]) and np.isinf(got[0][:, batch.scene_of < 0]).all()  # no plan; no scene


@pytest.mark.parametrize("name", ["base", "rings"])
def test_fallback_stop_against_the_reference(engine, oracle, name):
    c = IX.fallback_case(name)
    ref = FR.fallback(oracle, c.batch, c.stop_T, c.d_targets, c.max_decel, best_idx=c.best_idx, skip=c.skip)
    got = TF.host(engine, c)
    TF.assert_matches(got, ref, f"{name}, shared and ragged")
    assert (got.cand[~ref.need] == -3).all()


@pytest.mark.parametrize("kind,names", IX.FISS_CASES, ids=IX.FISS_IDS)
def test_plan_fiss_enforce_against_the_reference(engine, oracle, kind, names):
    batch = IX.fiss_batch()
    refs = FRR.batch_plan(oracle, batch, kind, names, key="indirection")
    FRR.check_caps(refs, "shared and ragged")
    got = engine.plan_fiss(batch, kind, enforce=names)
    compared = 0
    for e, r in enumerate(refs):
        if r.undecided:
            continue
        compared += 1
        assert np.array_equal(got.best_ijk[e], r.best_ijk) and np.array_equal(got.stats[e], r.stats) and np.array_equal(got.prev_best_idx[e], r.prev_best_idx), (kind, e)
        assert bool(got.refined[e]) == r.refined and got.rejected[e] == r.rejected, (kind, e)
        if r.best_ijk[0] < 0:
            assert np.isnan(got.best_cost[e]) and np.isnan(got.end_state[e]).all()
            continue
        assert np.abs(got.end_state[e] - r.end_state).max() <= 1e-9 and abs(got.best_cost[e] - r.best_cost) <= 1e-6, (kind, e)
    assert compared >= batch.B - 1


@SHAPES
def test_clearance_rescoring_against_the_reference(engine, oracle, shapes):
    TC.check_against_restatement(engine, oracle, weighted(IX.rules_batch(shapes=shapes)), what="clearance, shared and ragged")


# ---------------------------------------------------------------- 3. closed loops
def run_loop(engine, batch, graph, **kw):
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch

    runner = ClosedLoopRunner(engine, DeviceBatch(batch, 0), np.full((batch.B, 2), 1e9), **kw)  # (nobody arrives)
    out = runner.run_graph(LOOP_CYCLES, record=True) if graph else runner.run(LOOP_CYCLES, record=True)
    got = fields(out, ("ego", "t_now", "done", "cycles", "cart") + tuple(k for k in ("violation_counts", "rejected", "fallback_counts") if hasattr(out, k)))
    got["log_n_rows"] = out.log.n_rows
    got["log_rows"] = np.stack([np.where(np.arange(out.log.rows.shape[1])[:, None] < out.log.n_rows[b], out.log.rows[b], np.nan) for b in range(batch.B)])
    return got


@SHAPES
@pytest.mark.parametrize("config", ["FOP, four passes, fallback", "FISS+, enforce, audit"])
def test_closed_loop_twins(engine, config, shapes):
    if config.startswith("FOP"):
        base, kw = IX.rules_batch(shapes=shapes), dict(planner="FOP", rules=NAMES, fallback=stop())
    else:
        base, kw = IX.fiss_batch(shapes), dict(planner="FISS+", enforce=NAMES, audit=NAMES)
    variants = twins(base)
    eager = assert_twins(lambda b: run_loop(engine, b, False, **kw), variants, config + ", eager")
    graph = assert_twins(lambda b: run_loop(engine, b, True, **kw), variants, config + ", graph")
    diff = [k for k in eager if not same_bits(eager[k], graph[k])]
    assert not diff, (config, "eager / graph", diff)
    assert (eager["cycles"] > 0).any() and (eager["log_n_rows"] > 0).any()
    if "fallback_counts" in eager:
        assert (eager["fallback_counts"].sum(axis=1) == LOOP_CYCLES).all()  # every cycle of every ego has a status
