"""GPU: the FISS+ refinement kernel (fiss_refine_kernel<NCH, Args>) off the defaults every other test calls it with - up to nine rounds
(63 candidates: every lane but one of the wavefront, 16 validation groups through the two-slot verdict buffers, the whole rank loop,
63 trace rows), decays up to 1.0, other history weights, a sampling box that is not the lattice's hull, resolutions that are not its
spacing, and steps whose gradient is undefined (a step with a NaN component before clipping ends the rounds; its probes stay candidates).

  1. every case of tests/refine_cases.py against the numpy restatement (tests/fiss_rules_ref.py; tests/test_refine_opts_cpu.py proves on
     the restatement alone that the cases reach their paths), with the bars of tests/test_gpu_fiss_batch.py;
  2. without the fp32 pair table: bit-identical; 3. the engine's cache of its option struct; 4. resident data: bit-identical;
  5. the rule instances under a rule set that cannot speak: bit-identical to the plain instances.

Not covered, on purpose: a box that reaches T <= 0 (samp_min[:, 2] = 0 with a large resolution: the oracle aborts the round after four
probes, the restatement raises, the kernel prices a NaN - the only way found into its unranked pop path; what the ABI should accept there
is undecided), and a box with samp_min == samp_max on an axis (NaN in the search estimate, search.py)."""
from types import SimpleNamespace

import numpy as np
import pytest

import fiss_rules_ref as FR
import refine_cases as RC
from fiss_rules_parent import history
from fiss_plus_planner_amd import _abi

pytestmark = pytest.mark.gpu
NAMES = FR.NAMES
UNDEFINED = [c.id for c in RC.CASES if c.undefined]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def rows_of(out, with_trace=True):
    return [SimpleNamespace(best_ijk=out.best_ijk[e], prev_best_idx=out.prev_best_idx[e], stats=out.stats[e], refined=out.refined[e], end_state=out.end_state[e],
                            best_cost=out.best_cost[e], trace=out.trace[e] if with_trace else None) for e in range(len(out.best_cost))]


def run(engine, c, **kw):
    batch, prev = RC.made(c)
    return engine.plan_fiss(batch, "FISS+", prev_best_idx=prev, trace=True, **RC.opts(c), **kw)


def assert_same_outputs(a, b, what):
    found = b.best_ijk[:, 0] >= 0
    for k in RC.OUT_KEYS:
        assert same_bits(getattr(a, k), getattr(b, k)), (what, k)
    assert same_bits(a.trace[found], b.trace[found]), (what, "trace")  # (an ego without a coarse winner: the call writes no row)


# ---------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("cid", RC.IDS)
def test_against_the_restatement(engine, oracle, cid):
    c = RC.BY_ID[cid]
    got = run(engine, c)
    assert got.trace.shape == (got.best_cost.shape[0], c.R * 7, 4)
    RC.check_batch(rows_of(got), RC.refs(oracle, c), cid)


# ---------------------------------------------------------------- 2. the pair table off
@pytest.mark.parametrize("cid", ["base-R9"] + UNDEFINED)
def test_without_the_pair_table(engine, cid):
    c = RC.BY_ID[cid]
    want = run(engine, c)
    engine.set_option("refine_table_kb", 0)
    try:
        got = run(engine, c)
    finally:
        engine.set_option("refine_table_kb", 96)
    assert (want.best_ijk[:, 0] >= 0).any()
    assert_same_outputs(got, want, cid)


# ---------------------------------------------------------------- 3. the engine's option cache
def test_option_struct_follows_the_arguments(engine, oracle):
    """One batch object, one reused `out`, the options alternating: plan_fiss keeps its fp_fiss_opts in `out` under (plus, R, w_heuristic,
    decaying_factor) - a call that found a stale one would plan with the other call's rounds, weight or decay."""
    ends = [RC.BY_ID["base-R9-decay1-w50"], RC.BY_ID["base-w0"]]
    batch, prev = RC.made(ends[0])
    assert RC.made(ends[1])[0] is batch
    out = engine.fiss_outputs(batch.B, 9)
    for c in ends * 2:
        got = engine.plan_fiss(batch, "FISS+", prev_best_idx=prev, out=out, **RC.opts(c))
        assert got is out
        RC.check_batch(rows_of(got, with_trace=False), RC.refs(oracle, c), c.id)


# ---------------------------------------------------------------- 4. resident data
def test_resident_call_equals_the_host_call(engine):
    import torch

    from fiss_plus_planner_amd.device_batch import DeviceBatch

    c = RC.BY_ID["base-R9"]
    batch, prev = RC.made(c)
    want = run(engine, c)
    db, B = DeviceBatch(batch, 0, order_hint=False), batch.B
    i32, f64 = torch.int32, torch.float64
    o = dict(prev_best_idx=torch.from_numpy(prev.copy()).to(db.dev), best_ijk=db.empty((B, 3), i32), best_cost=db.empty(B, f64), end_state=db.empty((B, 3), f64),
             refined=db.empty(B, i32), stats=db.empty((B, 4), i32), trace=torch.full((B, c.R * 7, 4), float("nan"), dtype=f64, device=db.dev))
    io = _abi.FpFissIo()
    io.samp_min, io.samp_max, io.samp_res = (db.t[k].data_ptr() for k in ("samp_min", "samp_max", "samp_res"))
    for k, t in o.items():
        setattr(io, k, t.data_ptr())
    engine.plan_fiss_device(db.params, db.fb, _abi.FpFissOpts(_abi.FP_FISS_PLUS, c.R, c.w, c.decay), io)
    torch.cuda.synchronize(db.dev)
    assert_same_outputs(SimpleNamespace(**{k: t.cpu().numpy() for k, t in o.items()}), want, c.id)


# ---------------------------------------------------------------- 5. the rule instances
@pytest.mark.parametrize("cid", ["base-R9-decay1", "base-res1-zero"])
@pytest.mark.parametrize("name", ["silent", "silent_long"])
def test_silent_rules_leave_every_output(engine, name, cid):
    """test_identity of tests/test_gpu_fiss_rules.py off the defaults: nine rounds at decay 1.0 and an undefined step through
    fiss_refine_kernel<NCH, FissRulesArgs>."""
    c = RC.BY_ID[cid]
    batch = FR.case(name) if c.change is None else c.change(FR.case(name))
    kw = dict(prev_best_idx=history(batch), trace=True, **RC.opts(c))
    plain = engine.plan_fiss(batch, "FISS+", **kw)
    got = engine.plan_fiss(batch, "FISS+", enforce=NAMES, **kw)
    found = plain.best_ijk[:, 0] >= 0
    assert found.any()
    n = (~np.isnan(plain.trace[found][:, :, 3])).sum(axis=1)
    assert (n == (6 if c.undefined else 63)).all(), (name, cid, n)
    assert_same_outputs(got, plain, (name, cid))
    assert not got.rejected.any()
