"""GPU: fp_rules_eval (the four road rules on explicit end states) - on the lattice's own end states against the table passes it
restates (fp_speed_envelope, fp_gate_mask, fp_boundary_mask, fp_gap_mask) and their references, one rule at a time and all four; off
the lattice against tests/rules_eval_ref.py; the counts, the two memory spaces, a launch order, a second call on its own output;
FrenetEngine.plan_fiss(rules=...), ClosedLoopRunner(audit=...) and the error codes of the C ABI; a rule's bad argument refused with
one code and one text by the rule's own pass, fp_rules_eval and fp_plan_fiss_rules, and a bad fp_loop_io by every closed-loop entry point."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import boundary_ref as BR
import envelope_ref as ER
import gaps_ref as PR
import gates_ref as GR
import rules_eval_ref as R
from fiss_plus_planner_amd import _abi, rules, synth
from fiss_plus_planner_amd.engine import host_structs

pytestmark = pytest.mark.gpu
LOW = np.uint32(0xFF)
GAP = np.uint32(R.RULE_GAP)
SIBLINGS = {
    "envelope": (ER, "speed_envelope", (("bit_a", R.RULE_LIMIT), ("bit_b", R.RULE_LATERAL))),
    "gates": (GR, "gate_mask", (("gated", R.RULE_GATE),)),
    "boundary": (BR, "boundary_mask", (("bit", R.RULE_BOUNDARY),)),
    "gaps": (PR, "gap_mask", (("close", R.RULE_GAP),)),
}
CASES = [(rule, name) for rule, (mod, _, _) in SIBLINGS.items() for name in mod.CASES]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def planning(batch):
    """The batch as a host PLANNING call takes it: those refuse a negative t_now (without obstacles nothing they compute depends on it)."""
    if (np.asarray(batch.t_now) >= 0).all():
        return batch
    assert batch.n_obs == 0
    return dataclasses.replace(batch, t_now=np.maximum(batch.t_now, 0))


def lattice_words(engine, batch):
    """(end states [B, C, 3], eval_trajs' flag words of them [B, C], the dense call's result)."""
    es = R.lattice_end_states(batch)
    words = engine.eval_trajs(planning(batch), es).flags
    dense = engine.plan_dense(planning(batch), tables=True)
    assert np.array_equal(words >> 8, dense.flags >> 8)  # N and M of an end state are those of the candidate it is
    return es, words, dense


# ---------------------------------------------------------------- 1. the lattice's own end states
@pytest.mark.parametrize("rule,name", CASES, ids=[f"{r}-{n}" for r, n in CASES])
def test_lattice_equivalence_one_rule(engine, oracle, rule, name):
    mod, method, verdicts = SIBLINGS[rule]
    batch, refs = mod.case(oracle, name)
    mod.check_caps(refs, name)
    es, words, dense = lattice_words(engine, batch)
    table = getattr(engine, method)(batch, dense.cost, dense.flags)[0]  # the pass over the dense call's table
    n0 = engine.get_option("rules_eval_launches")
    got = engine.rules_eval(batch, es, words, rules=(rule,))
    assert engine.get_option("rules_eval_launches") == n0 + 1  # one launch
    ok = ~np.stack([r.undecided for r in refs])
    assert np.array_equal((got.flags & LOW)[ok], (table & LOW)[ok]), (rule, name)
    assert np.array_equal(got.flags & ~LOW, words & ~LOW)  # N, M and everything above the low byte stay
    want = np.zeros(words.shape, dtype=np.uint32)
    for field, bit in verdicts:
        want |= np.where(np.stack([getattr(r, field) for r in refs]), bit, 0).astype(np.uint32)
    assert np.array_equal(got.rule_bits[ok], want[ok]), (rule, name)
    for b, r in enumerate(refs):
        if not r.undecided.any():
            assert np.array_equal(got.counts[b], [((want[b] >> i) & 1).sum() for i in range(5)]), (rule, name, b)
    if name not in ("unlimited", "open"):
        assert got.rule_bits.any(), (rule, name)


def test_lattice_equivalence_all_four(engine, oracle):
    batch = R.all_rules_batch()
    es, words, _ = lattice_words(engine, batch)
    table = engine.plan_dense(batch, tables=True, envelope=True, gates=True, boundary=True, gaps=True).flags  # the chain of the four passes
    ref = R.batch_rules(oracle, batch, es, words)
    R.check_caps(ref, "all four")
    got = engine.rules_eval(batch, es, words)  # rules=None: every rule the batch carries
    ok = ~ref.undecided
    assert np.array_equal(got.flags[ok], table[ok]) and np.array_equal(got.flags[ok], ref.flags[ok])
    assert np.array_equal(got.rule_bits[ok], ref.rule_bits[ok])
    assert int(np.bitwise_or.reduce(got.rule_bits.ravel())) == 31
    for b in range(batch.B):
        if ok[b].all():
            assert np.array_equal(got.counts[b], ref.counts[b]), b


# ---------------------------------------------------------------- 2. off the lattice
_off = {}


def off_inputs(engine, oracle):
    """(batch, end states, skip, eval_trajs' words, the reference) of the off-lattice inputs; computed once and shared (do not modify)."""
    if not _off:
        _off["v"] = _off_inputs(engine, oracle)
    return _off["v"]


def _off_inputs(engine, oracle):
    batch = R.all_rules_batch()
    es, skip = R.off_lattice(batch), R.off_skip(batch)
    words = engine.eval_trajs(batch, es).flags
    ref = R.batch_rules(oracle, batch, es, words, skip=skip)
    R.check_caps(ref, "off-lattice")
    return batch, es, skip, words, ref


def test_off_lattice(engine, oracle):
    batch, es, skip, words, ref = off_inputs(engine, oracle)
    got = engine.rules_eval(batch, es, words, skip=skip)
    ok = ~ref.undecided
    assert np.array_equal(got.flags[ok], ref.flags[ok]) and np.array_equal(got.rule_bits[ok], ref.rule_bits[ok])
    assert np.array_equal(got.flags[R.OFF_SKIP], words[R.OFF_SKIP]) and not got.rule_bits[R.OFF_SKIP].any() and not got.counts[R.OFF_SKIP].any()
    assert got.flags[R.OFF_NAN] == words[R.OFF_NAN] and got.rule_bits[R.OFF_NAN] == 0
    assert words[R.OFF_SHORT] >> 20 == 2
    for b in range(batch.B):
        if ok[b].all():
            assert np.array_equal(got.counts[b], ref.counts[b]), b
    # flags=None: eval_trajs runs first and supplies the same words
    auto = engine.rules_eval(batch, es, skip=skip)
    keep = np.ones(batch.B, dtype=bool)
    keep[R.OFF_SKIP] = False
    assert np.array_equal(auto.flags[keep], got.flags[keep]) and np.array_equal(auto.rule_bits, got.rule_bits) and np.array_equal(auto.counts, got.counts)


# ---------------------------------------------------------------- 3. K = 1 and the counts
def raw_call(engine, batch, names, K, es, flags, rule_bits, counts, mem=_abi.FP_MEM_HOST, rule_set=None):
    """fp_rules_eval through the C ABI with the pointers as given (None = NULL) -> the return code."""
    held = {}

    def addr(k):
        held[k] = np.ascontiguousarray(rules.array(batch, k))
        return held[k].ctypes.data

    rs = rule_set
    if rs is None:
        rs, structs = rules.rule_set(batch, addr, names)
    p, fb = host_structs(batch)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return engine._lib.fp_rules_eval(engine._ctx, C.byref(p), C.byref(fb), None if rs is False else C.byref(rs), K, ptr(es), ptr(flags), ptr(rule_bits), ptr(counts),
                                     mem, None)


def test_single_trajectory_and_counts(engine, oracle):
    batch, es, _, words, ref = off_inputs(engine, oracle)
    es1, words1 = np.ascontiguousarray(es[:, 2:3]), np.ascontiguousarray(words[:, 2:3])
    first = engine.rules_eval(batch, es1, words1)
    ok = ~ref.undecided[:, 2]
    ok[R.OFF_SKIP] = False  # (the shared reference skips that ego; this call does not)
    assert np.array_equal(first.flags[ok, 0], ref.flags[ok, 2]) and np.array_equal(first.rule_bits[ok, 0], ref.rule_bits[ok, 2])
    assert np.array_equal(first.counts, np.stack([(first.rule_bits[:, 0] >> i) & 1 for i in range(5)], axis=1)) and first.counts.any()
    acc = np.zeros((batch.B, 5), dtype=np.int32)
    for _ in range(3):
        acc = engine.rules_eval(batch, es1, words1, counts=acc).counts
    assert np.array_equal(acc, 3 * first.counts)
    # rule_bits and counts are optional
    w = words1.copy()
    assert raw_call(engine, batch, None, 1, es1, w, None, None) == 0
    assert np.array_equal(w, first.flags)


# ---------------------------------------------------------------- 4. invariance
class Resident:
    """The batch, the end states and the outputs in device memory."""

    def __init__(self, engine, batch, es, words, order=None, skip=None):
        import torch

        from fiss_plus_planner_amd.device_batch import DeviceBatch

        self.torch, self.engine, self.db = torch, engine, DeviceBatch(batch, 0, order_hint=False)
        db, B, K = self.db, es.shape[0], es.shape[1]
        self.K = K
        self.fb = _abi.FpBatch.from_buffer_copy(db.fb)
        if order is not None:
            self.order = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(db.dev)
            self.fb.launch_order = self.order.data_ptr()
        if skip is not None:
            self.skip = torch.from_numpy(np.ascontiguousarray(skip, dtype=np.int32)).to(db.dev)
            self.fb.skip = self.skip.data_ptr()
        self.es = torch.from_numpy(np.ascontiguousarray(es)).to(db.dev)
        self.flags = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(db.dev)
        self.bits = torch.full((B, K), -1, dtype=torch.int32, device=db.dev)
        self.counts = torch.zeros((B, 5), dtype=torch.int32, device=db.dev)
        self.rule_set, self.structs = rules.rule_set(batch, lambda k: db.t[k].data_ptr())

    def call(self, stream=0):
        self.engine.rules_eval_device(self.db.params, self.fb, self.rule_set, self.K, self.es.data_ptr(), self.flags.data_ptr(), self.bits.data_ptr(),
                                      self.counts.data_ptr(), stream)

    def fetch(self):
        self.torch.cuda.synchronize(self.db.dev)
        return self.flags.cpu().numpy().view(np.uint32), self.bits.cpu().numpy().view(np.uint32), self.counts.cpu().numpy()


def test_memory_space_launch_order_and_a_second_call(engine, oracle):
    batch, es, skip, words, _ = off_inputs(engine, oracle)
    host = engine.rules_eval(batch, es, words, skip=skip)
    n0 = engine.get_option("rules_eval_launches")
    for order in (None, np.arange(batch.B)[::-1]):
        dev = Resident(engine, batch, es, words, order=order, skip=skip)
        dev.call()
        flags, bits, counts = dev.fetch()
        assert np.array_equal(flags, host.flags) and np.array_equal(bits, host.rule_bits) and np.array_equal(counts, host.counts), order
    assert engine.get_option("rules_eval_launches") == n0 + 2
    # the lattice's end states too: K = 60 over four wavefronts, both memory spaces; here the gaps speak
    lat = R.lattice_end_states(batch)
    lw = engine.eval_trajs(batch, lat).flags
    h = engine.rules_eval(batch, lat, lw)
    d = Resident(engine, batch, lat, lw)
    d.call()
    flags, bits, counts = d.fetch()
    assert np.array_equal(flags, h.flags) and np.array_equal(bits, h.rule_bits) and np.array_equal(counts, h.counts) and (h.rule_bits & GAP).any()
    # a second call on the words the first one left: no word changes (the boundary bit is written to the same value, the OR bits stay);
    # the gaps no longer evaluate their own violators, so that call's rule_bits lack FP_RULE_GAP for them - and differ in nothing else
    d.call()
    flags2, bits2, counts2 = d.fetch()
    assert np.array_equal(flags2, h.flags)
    assert np.array_equal(bits2, h.rule_bits & ~GAP)
    assert np.array_equal(counts2[:, :4], 2 * h.counts[:, :4]) and np.array_equal(counts2[:, 4], h.counts[:, 4])
    again = engine.rules_eval(batch, lat, h.flags)
    assert np.array_equal(again.flags, h.flags) and np.array_equal(again.rule_bits, h.rule_bits & ~GAP)


# ---------------------------------------------------------------- 5. plan_fiss(rules=...)
def fiss_batch():
    """A FISS+ batch (its own lattice and sampling box) that carries gates and a corridor; ego 3 drives at three times max_speed: no plan."""
    b = synth.make_batch(5, 5, 4, 3, 6, 120, True, R.SEED, kind="FISS+")
    ego = b.ego.copy()
    ego[3, 1] = 3.0 * b.max_speed  # (every trajectory starts above max_speed: infeasible at point 0)
    b = GR.with_gates(b, ego=ego)
    dl, dr = BR.wavy_corridor(b.knots)
    return dataclasses.replace(b, bound_left=dl + BR.WIDEN, bound_right=dr - BR.WIDEN, bound_margin=0.05)


def test_plan_fiss_with_rules(engine):
    batch = fiss_batch()
    names = ("gates", "boundary")
    plain = engine.plan_fiss(batch, "FISS+")
    assert not hasattr(plain, "rule_bits")
    for winner in (False, True):
        out = engine.plan_fiss(batch, "FISS+", rules=names, winner=winner)
        for k in ("end_state", "best_cost", "stats", "best_ijk", "refined", "prev_best_idx"):
            assert same_bits(getattr(out, k), getattr(plain, k)), (winner, k)
        want = engine.rules_eval(batch, out.end_state[:, None, :], rules=names)
        assert out.rule_bits.shape == (batch.B,) and np.array_equal(out.rule_bits, want.rule_bits[:, 0]), winner
        none = out.best_ijk[:, 0] < 0
        assert none[3] and np.isnan(out.end_state[none]).all() and not out.rule_bits[none].any()
        assert (out.best_ijk[[0, 1, 2, 4], 0] >= 0).any()
        assert not (out.rule_bits & ~np.uint32(R.RULE_GATE | R.RULE_BOUNDARY)).any()


# ---------------------------------------------------------------- 6. ClosedLoopRunner(audit=...)
LOOP_CYCLES = 30


def loop_batch():
    """gates_ref.loop_batch() (one gate at s = 60, closed before step 80) for the four opening steps its own tests drive, with the FISS
    sampling box of its lattice."""
    b = GR.loop_batch(GR.OPEN_STEPS)
    d, t, v = np.asarray(b.d_samples), np.asarray(b.t_samples), np.asarray(b.v_samples)
    one = np.ones(b.B)
    return dataclasses.replace(b, samp_min=np.column_stack([one * d.min(), v.min(axis=1), one * t.min()]),
                               samp_max=np.column_stack([one * d.max(), v.max(axis=1), one * t.max()]),
                               samp_res=np.column_stack([one * (d[1] - d[0]), v[:, 1] - v[:, 0], one * (t[1] - t[0])]))


def runner_for(engine, batch, **kw):
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch

    goal = np.full((batch.B, 2), 1e6)  # (nobody arrives)
    return ClosedLoopRunner(engine, DeviceBatch(batch, 0), goal, planner="FISS+", **kw)


def test_closed_loop_audit(engine):
    batch = loop_batch()
    base = runner_for(engine, batch).run(LOOP_CYCLES)
    eager = runner_for(engine, batch, audit=("gates",)).run(LOOP_CYCLES)
    graph = runner_for(engine, batch, audit=("gates",)).run_graph(LOOP_CYCLES)
    for out in (eager, graph):
        assert set(out.violations) == {"gates"} and out.violations["gates"].shape == (batch.B,)
        assert np.array_equal(out.violation_counts[:, 2], out.violations["gates"]) and not out.violation_counts[:, [0, 1, 3, 4]].any()
        for k in ("ego", "t_now", "done", "cycles", "cart"):  # the audit changes no plan: the driven states are the loop's own
            assert same_bits(getattr(out, k), getattr(base, k)), k
    assert np.array_equal(eager.violations["gates"], graph.violations["gates"])
    # by hand: an unfused eager loop, the verdict of every cycle's end state through the host call
    r = runner_for(engine, batch, fused=False)
    torch, db = r.db.torch, r.db
    stream = torch.cuda.current_stream(db.dev).cuda_stream
    count = np.zeros(batch.B, dtype=np.int64)
    for _ in range(LOOP_CYCLES):
        engine.plan_fiss_device(db.params, r.fb, r.fopts, r.fio, stream=stream)
        torch.cuda.synchronize(db.dev)
        now = dataclasses.replace(batch, ego=db.t["ego"].cpu().numpy(), t_now=db.t["t_now"].cpu().numpy())
        v = engine.rules_eval(now, r.end_state.cpu().numpy()[:, None, :], rules=("gates",), skip=r.done.cpu().numpy())
        count += (v.rule_bits[:, 0] & R.RULE_GATE) != 0
        engine.advance_device(db.params, r.fb, r.io, end_state=r.end_state.data_ptr(), stream=stream)
    torch.cuda.synchronize(db.dev)
    assert same_bits(db.t["ego"].cpu().numpy(), base.ego)
    assert np.array_equal(eager.violations["gates"], count) and count.any()  # (the gate is closed when the first cycles' plans arrive)


# ---------------------------------------------------------------- 7. errors through the ABI
def test_errors(engine, oracle):
    batch, es, _, words, _ = off_inputs(engine, oracle)
    n0 = engine.get_option("rules_eval_launches")
    bits, counts = np.zeros(words.shape, dtype=np.uint32), np.zeros((batch.B, 5), dtype=np.int32)
    w = words.copy()
    assert raw_call(engine, batch, None, 0, es, w, bits, counts) == -1    # K = 0: FP_EINVAL
    assert raw_call(engine, batch, None, R.OFF_K, es, w, bits, counts, rule_set=_abi.FpRuleSet()) == -1  # every rule NULL
    assert raw_call(engine, batch, None, R.OFF_K, es, w, bits, counts, rule_set=False) == -1             # no rule set at all
    assert raw_call(engine, batch, None, R.OFF_K, es, None, bits, counts) == -1  # flags NULL
    assert raw_call(engine, batch, None, R.OFF_K, None, w, bits, counts) == -1   # end_states NULL
    long = es.copy()
    long[4, 1, 2] = (_abi.FP_MAX_POINTS + 0.5) * batch.tick_t
    assert raw_call(engine, batch, None, R.OFF_K, long, w, bits, counts) == -4   # FP_ELIMIT: more than FP_MAX_POINTS points
    assert b"FP_MAX_POINTS" in engine._lib.fp_last_error()
    # a rule's own argument error, with the pass' message
    with pytest.raises(_abi.FrenetGpuError, match="fp_boundary_mask: margin"):
        engine.rules_eval(dataclasses.replace(batch, bound_margin=-1.0), es, words, rules=("boundary",))
    assert engine.get_option("rules_eval_launches") == n0 and np.array_equal(w, words) and not bits.any() and not counts.any()  # nothing launched, nothing written
    assert raw_call(engine, batch, None, R.OFF_K, es, w, bits, counts) == 0 and engine.get_option("rules_eval_launches") == n0 + 1


# ---------------------------------------------------------------- 8. one refusal, whichever entry point carries the rule
NAN, INF = float("nan"), float("inf")
# (rule, what is wrong, the text of fp_last_error as the rule's checks in csrc/frenet_abi.hip word it); every row is FP_EINVAL.  "field"
# rows change the rule's struct, "array" rows an entry of the array the field points to (only a host call can look there)
BAD_ARGUMENTS = [
    ("envelope", ("field", "front", -1.0), "fp_speed_envelope: front must be finite and >= 0"),
    ("envelope", ("field", "tol", NAN), "fp_speed_envelope: tol must be finite and >= 0"),
    ("envelope", ("field", "max_lat_accel", INF), "fp_speed_envelope: max_lat_accel must be finite and >= 0 (0 = off)"),
    ("envelope", ("field", "v_limit", None), "fp_speed_envelope: profile / v_limit must not be NULL"),
    ("gates", ("field", "gate_stride", 0), "fp_gate_mask: gate_stride=0 outside 1..FP_MAX_GATES"),
    ("gates", ("field", "gate_stride", _abi.FP_MAX_GATES + 1), f"fp_gate_mask: gate_stride={_abi.FP_MAX_GATES + 1} outside 1..FP_MAX_GATES"),
    ("gates", ("field", "T_gate", 0), "fp_gate_mask: T_gate=0 must be >= 1"),
    ("gates", ("field", "max_decel", NAN), "fp_gate_mask: max_decel must be finite and >= 0 (0 = off)"),
    ("gates", ("field", "closed", None), "fp_gate_mask: gates / gate_s / closed must not be NULL"),
    ("boundary", ("field", "margin", NAN), "fp_boundary_mask: margin must be finite and >= 0"),
    ("boundary", ("field", "left", None), "fp_boundary_mask: corridor / left / right must not be NULL"),
    ("gaps", ("field", "lag_follow", -1), "fp_gap_mask: lag_follow=-1 outside 0..FP_MAX_POINTS"),
    ("gaps", ("field", "lag_lead", _abi.FP_MAX_POINTS + 1), f"fp_gap_mask: lag_lead={_abi.FP_MAX_POINTS + 1} outside 0..FP_MAX_POINTS"),
    ("gaps", ("field", "first", 0), "fp_gap_mask: first=0 must be >= 1"),
    ("envelope", ("array", "speed_limit", -1.0), 'fp_speed_envelope: v_limit is -1 at frame 0, knot 0 (+inf says "no limit", 0 "stop")'),
    ("boundary", ("array", "bound_right", NAN), 'fp_boundary_mask: corridor has a NaN at frame 0, knot 0 (+-inf says "no edge")'),
]
LAUNCH_COUNTERS = ("envelope_launches", "gate_launches", "boundary_launches", "gap_launches", "rules_eval_launches", "lattice_launches")


def last_error(engine):
    return engine._lib.fp_last_error().decode()


def test_one_refusal_in_the_pass_the_rules_kernel_and_the_fiss_call(engine):
    from test_gpu_fiss_rules import raw_call as fiss_raw_call

    batch = R.all_rules_batch()
    B, Cn = batch.B, batch.C
    p, fb = host_structs(batch)
    es = np.ascontiguousarray(R.lattice_end_states(batch)[:, :1])
    cost, words = np.zeros((B, Cn)), np.zeros((B, Cn), dtype=np.uint32)
    idx, best, count = np.zeros(B, dtype=np.int32), np.zeros(B), np.zeros(B, dtype=np.int32)
    w1, bits, counts = np.zeros((B, 1), dtype=np.uint32), np.zeros((B, 1), dtype=np.uint32), np.zeros((B, 5), dtype=np.int32)
    before = [engine.get_option(k) for k in LAUNCH_COUNTERS]

    def own_pass(rule, struct, tables=True):
        ptr = lambda a: a.ctypes.data if tables else None  # noqa: E731
        return getattr(engine._lib, rules.by_name[rule].fn)(engine._ctx, C.byref(p), C.byref(fb), C.byref(struct), ptr(cost), ptr(words), ptr(idx), ptr(best),
                                                            count.ctypes.data, _abi.FP_MEM_HOST, None)

    for rule, (kind, name, value), text in BAD_ARGUMENTS:
        held = {}

        def addr(k):
            held[k] = np.array(rules.array(batch, k), order="C", copy=True)
            return held[k].ctypes.data

        rs, structs = rules.rule_set(batch, addr, (rule,))
        if kind == "field":
            setattr(structs[rule], name, value)
        else:
            held[name][0, 0] = value  # (knot 0 of frame 0 is used: every line has two knots or more)
        got = [(own_pass(rule, structs[rule]), last_error(engine)),
               (raw_call(engine, batch, None, 1, es, w1, bits, counts, rule_set=rs), last_error(engine)),
               (fiss_raw_call(engine, batch, rs), last_error(engine))]
        assert got == [(-1, text)] * 3, (rule, name, value, got)
    # the empty set names the entry point it was handed to
    assert raw_call(engine, batch, None, 1, es, w1, bits, counts, rule_set=_abi.FpRuleSet()) == -1
    assert last_error(engine) == "fp_rules_eval: every rule of the set is NULL"
    assert fiss_raw_call(engine, batch, _abi.FpRuleSet()) == -1 and last_error(engine) == "fp_plan_fiss_rules: every rule of the set is NULL"
    # a pass looks at its tables before it looks at the rule's scalars
    held = {}
    rs, structs = rules.rule_set(batch, lambda k: held.setdefault(k, np.ascontiguousarray(rules.array(batch, k))).ctypes.data, ("boundary",))
    structs["boundary"].margin = NAN
    assert own_pass("boundary", structs["boundary"], tables=False) == -1
    assert last_error(engine) == "fp_boundary_mask: cost_tbl/flag_tbl/best_idx/best_cost must not be NULL"
    assert [engine.get_option(k) for k in LAUNCH_COUNTERS] == before and not words.any() and not w1.any() and not bits.any() and not counts.any()


def test_loop_io_refusals(engine):
    batch = R.all_rules_batch()
    B = batch.B
    p, fb = host_structs(batch)
    lib, ctx, HOST = engine._lib, engine._ctx, _abi.FP_MEM_HOST
    arr = dict(ego=np.array(batch.ego, dtype=np.float64), t_now=np.zeros(B, dtype=np.int32), done=np.zeros(B, dtype=np.int32), cycles=np.zeros(B, dtype=np.int32),
               goal_xy=np.full((B, 2), 1e6), cart_state=np.zeros((B, 3)), goal_poly=np.zeros((B, 4, 2)))
    idx, best = np.zeros(B, dtype=np.int32), np.zeros(B)
    res = _abi.FpResult()
    res.best_idx, res.best_cost = idx.ctypes.data, best.ctypes.data
    out = engine.fiss_outputs(B, 0)
    fio = _abi.FpFissIo()
    fio.samp_min, fio.samp_max, fio.samp_res = (np.ascontiguousarray(getattr(batch, k)).ctypes.data for k in ("samp_min", "samp_max", "samp_res"))
    for k in ("prev_best_idx", "best_ijk", "best_cost", "end_state", "refined", "stats"):
        setattr(fio, k, getattr(out, k).ctypes.data)
    opts = _abi.FpFissOpts(_abi.FP_FISS, 0, 10.0, 0.5)

    def loop_io(*names, goal_max_vertices=0):
        io = _abi.FpLoopIo()
        for k in names:
            setattr(io, k, arr[k].ctypes.data)
        io.goal_max_vertices = goal_max_vertices
        return io

    calls = {
        "fp_advance": lambda io: lib.fp_advance(ctx, C.byref(p), C.byref(fb), idx.ctypes.data, None, C.byref(io), HOST, None),
        "fp_plan_step": lambda io: lib.fp_plan_step(ctx, C.byref(p), C.byref(fb), C.byref(res), C.byref(io), HOST, None),
        "fp_plan_fiss_step": lambda io: lib.fp_plan_fiss_step(ctx, C.byref(p), C.byref(fb), C.byref(opts), C.byref(fio), C.byref(io), HOST, None),
        "fp_loop_record": lambda io: lib.fp_loop_record(ctx, C.byref(p), C.byref(fb), C.byref(io), idx.ctypes.data, None, best.ctypes.data, None, None, HOST, None),
    }
    n0 = engine.get_option("lattice_launches")
    no_ego = loop_io("t_now", "done", "cycles", "goal_xy", "cart_state")
    for fn, call in calls.items():
        assert call(no_ego) == -1 and last_error(engine) == "fp_loop_io has a NULL mandatory array", fn
    no_nv = loop_io("ego", "t_now", "done", "cycles", "goal_xy", "cart_state", "goal_poly", goal_max_vertices=4)
    for fn in ("fp_advance", "fp_plan_step", "fp_plan_fiss_step"):
        assert calls[fn](no_nv) == -1 and last_error(engine) == "fp_loop_io.goal_poly needs goal_nv and goal_max_vertices >= 3", fn
    assert engine.get_option("lattice_launches") == n0 and (arr["t_now"] == 0).all() and (arr["cycles"] == 0).all()
