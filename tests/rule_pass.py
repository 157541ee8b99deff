"""The contract of the rule passes behind the dense pass (fiss_plus_planner_amd/rules.py, include/frenet_gpu.h), tested from one place.

Every pass reads the dense call's [B][C] tables, puts bits into flag_tbl, returns the argmin among what is left and a count per ego,
honours skip and launch_order, is one launch, replays from a captured graph and costs nothing on a ctx that never asks.  PASSES carries
per rule what rules.TABLE does not know and the tests need; check_against, dense_and_pass, Resident and the test bodies below take the
rule's name and are what tests/test_gpu_{envelope,gates,boundary,gaps}.py call.  A new pass brings one row here and one thin test file.

A plain helper module: no fixture, no GPU import at module level (tests/test_rule_pass_cpu.py runs check_against without one)."""
import ctypes as C
import dataclasses
from typing import Callable, NamedTuple

import numpy as np
import pytest

import boundary_ref
import envelope_ref
import gaps_ref
import gates_ref
from fiss_plus_planner_amd import _abi, rules
from fiss_plus_planner_amd.engine import FrenetEngine, host_structs

POISON = 0xFFFFFFFF  # a flag row that WOULD count (M = 4095, every bit set) if it were read


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---------------------------------------------------------------- what differs between the passes
def _ored(p, flags, flags_in, want, ok, note):
    """The pass ORs: every other bit as it was, bits only ever added, the words the reference's where it decides."""
    assert np.array_equal(flags & ~p.mask, flags_in & ~p.mask), note
    assert np.array_equal(flags & flags_in, flags_in), note
    assert np.array_equal(flags[ok], want[ok]), note + (np.nonzero(flags != want)[0][:8].tolist(),)


def _written(p, flags, flags_in, want, ok, note):
    """The pass writes its bit (set / cleared): every other bit as it was, the bit the reference's verdict where it decides."""
    assert np.array_equal(flags & ~p.mask, flags_in), note
    bit = flags & p.mask != 0
    assert np.array_equal(bit[ok], want[ok]), note + (np.nonzero(bit != want)[0][:8].tolist(),)


def _plan_dense(engine, batch):
    return engine.plan_dense(batch, tables=True)


def _plan_dense_gates(engine, batch):
    """(a host planning call refuses a negative t_now; without obstacles its tables do not depend on t_now)"""
    assert batch.n_obs == 0
    return engine.plan_dense(dataclasses.replace(batch, t_now=np.maximum(batch.t_now, 0)), tables=True)


class Pass(NamedTuple):
    rule: rules.Rule     # the product's row: name, entry point, and `count`, which is also the reference's count field
    ref: object          # the rule's reference module
    method: str          # FrenetEngine.<method> (host tables) and <method>_device
    launches: str        # the launch counter (fp_ctx_get_option)
    mask: np.uint32      # the flag bits the pass may touch
    flag_law: Callable   # _ored / _written
    field: str           # the reference's verdict the flag law reads: the words (flags) or truth values (bit)
    count_law: Callable  # (n, added, marked) -> bool; added = words the call changed, marked = words that carry a bit of the mask
    recounts: bool       # a second run over its own output counts the same violators again (False: it evaluates survivors only, so 0)
    dense: Callable      # (engine, batch) -> the dense call's result with tables
    device_kw: Callable  # (batch, t) -> the rule's own keyword arguments of <method>_device; t[name] = the device array (DeviceBatch.t)


PASSES = {p.rule.name: p for p in (
    Pass(rules.by_name["envelope"], envelope_ref, "speed_envelope", "envelope_launches", np.uint32(envelope_ref.FLAG_SPEED | envelope_ref.FLAG_ACCEL), _ored, "flags",
         lambda n, added, marked: added <= n <= marked, True, _plan_dense,  # (a violating candidate may have carried its bits already)
         lambda b, t: dict(v_limit=t["speed_limit"].data_ptr(), front=b.limit_front, tol=b.limit_tol, max_lat_accel=b.max_lat_accel)),
    Pass(rules.by_name["gates"], gates_ref, "gate_mask", "gate_launches", np.uint32(gates_ref.FLAG_SPEED), _ored, "flags",
         lambda n, added, marked: added <= n <= marked, True, _plan_dense_gates,
         lambda b, t: dict(gate_s=t["gate_s"].data_ptr(), closed=t["gate_closed"].data_ptr(), gate_stride=b.gate_s.shape[1], T_gate=b.gate_closed.shape[1],
                           front=b.gate_front, max_decel=b.gate_max_decel)),
    Pass(rules.by_name["boundary"], boundary_ref, "boundary_mask", "boundary_launches", np.uint32(boundary_ref.FLAG_BOUNDARY), _written, "bit",
         lambda n, added, marked: n == marked, True, _plan_dense,
         lambda b, t: dict(left=t["bound_left"].data_ptr(), right=t["bound_right"].data_ptr(), margin=float(b.bound_margin))),
    Pass(rules.by_name["gaps"], gaps_ref, "gap_mask", "gap_launches", np.uint32(gaps_ref.FLAG_COLLISION), _ored, "flags",
         lambda n, added, marked: n == added, False, _plan_dense,  # violators are survivors: every one of them gains the bit
         lambda b, t: dict(follow=b.gap_follow, lead=b.gap_lead, first=b.gap_first)),
)}
assert tuple(PASSES) == tuple(rules.by_name)


def launches(engine, rule):
    return engine.get_option(PASSES[rule].launches)


# ---------------------------------------------------------------- the common checks
def check_against(rule, refs, dense, got, what, skip=None):
    """got = (flags, best_idx, best_cost, count) of a call of the pass over the tables of `dense` (cost, flags)."""
    p = PASSES[rule]
    flags, bi, bc, n = got
    cost_in, flags_in = dense
    p.ref.check_caps(refs, what)
    for b, r in enumerate(refs):
        if skip is not None and skip[b]:
            assert bi[b] == -1 and np.isnan(bc[b]) and n[b] == 0, (what, b)
            assert np.array_equal(flags[b], flags_in[b]), (what, b)  # rows neither read nor written
            continue
        assert np.array_equal(flags_in[b], r.flags_in), (what, b)  # (the dense call's own parity with the oracle)
        p.flag_law(p, flags[b], flags_in[b], getattr(r, p.field), ~r.undecided, (what, b))
        added, marked = np.count_nonzero(flags[b] != flags_in[b]), np.count_nonzero(flags[b] & p.mask)
        assert p.count_law(int(n[b]), added, marked), (what, b, int(n[b]), added, marked)
        if not r.undecided.any():
            want = getattr(r, p.rule.count)
            assert n[b] == want and bi[b] == r.best_idx, (what, b, int(bi[b]), r.best_idx, int(n[b]), want)
        if bi[b] >= 0:
            assert same_bits(bc[b:b + 1], cost_in[b, bi[b]:bi[b] + 1]) and not (flags[b, bi[b]] & _abi.FLAG_INFEASIBLE), (what, b)
        else:
            assert np.isnan(bc[b]), (what, b)


def dense_and_pass(engine, rule, batch, skip=None, **kw):
    """The dense call and the pass over its tables, both through host memory -> (the dense result, the pass's four outputs)."""
    p = PASSES[rule]
    out = p.dense(engine, batch)
    cost0, flags0 = out.cost.copy(), out.flags.copy()
    got = getattr(engine, p.method)(batch, out.cost, out.flags, skip=skip, **kw)
    assert same_bits(out.cost, cost0) and np.array_equal(out.flags, flags0)  # the caller's tables are copies here; cost is never written
    return out, got


def skip_only(batch, ego):
    skip = np.zeros(batch.B, dtype=np.int32)
    skip[ego] = 1
    return skip


class Resident:
    """A batch and its rule data in device memory, the dense call and the pass behind it on one stream."""

    def __init__(self, engine, rule, batch, order=None, skip=None, poison=None):
        import torch

        from fiss_plus_planner_amd.device_batch import DeviceBatch

        self.torch, self.engine, self.p, self.db, self.batch = torch, engine, PASSES[rule], DeviceBatch(batch, 0, order_hint=False), batch
        db, B, Cn = self.db, batch.B, batch.C
        self.fb = _abi.FpBatch.from_buffer_copy(db.fb)
        if order is not None:
            self.order = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(db.dev)
            self.fb.launch_order = self.order.data_ptr()
        if skip is not None:
            self.skip = torch.from_numpy(np.ascontiguousarray(skip, dtype=np.int32)).to(db.dev)
            self.fb.skip = self.skip.data_ptr()
        self.bi0, self.bc0 = db.empty(B, torch.int32), db.empty(B, torch.float64)
        self.bi, self.bc, self.n = db.empty(B, torch.int32), db.empty(B, torch.float64), db.empty(B, torch.int32)
        self.cost, self.flags = torch.zeros((B, Cn), dtype=torch.float64, device=db.dev), torch.zeros((B, Cn), dtype=torch.int32, device=db.dev)
        if poison is not None:
            self.flags[poison] = -1  # POISON

    def dense(self, stream=0):
        db = self.db
        self.engine.plan_dense_device(db.params, self.fb, self.bi0.data_ptr(), self.bc0.data_ptr(), cost_tbl=self.cost.data_ptr(), flag_tbl=self.flags.data_ptr(), stream=stream)

    def call(self, stream=0, **kw):
        """The rule's public <method>_device over the resident tables; kw replaces any of its keyword arguments."""
        a = self.p.device_kw(self.batch, self.db.t)
        a.update(cost_tbl=self.cost.data_ptr(), flag_tbl=self.flags.data_ptr(), best_idx=self.bi.data_ptr(), best_cost=self.bc.data_ptr())
        a[self.p.rule.count] = self.n.data_ptr()
        a.update(kw)
        getattr(self.engine, self.p.method + "_device")(self.db.params, self.fb, stream=stream, **a)

    def pair(self, stream=0):
        self.dense(stream)
        self.call(stream)

    def clobber(self):
        self.flags.zero_(); self.bi.fill_(-9); self.bc.fill_(-9.0); self.n.fill_(-9)

    def fetch(self):
        self.torch.cuda.synchronize(self.db.dev)
        return self.flags.cpu().numpy().view(np.uint32), self.bi.cpu().numpy(), self.bc.cpu().numpy(), self.n.cpu().numpy()


def run_loop(engine, batch, cycles, graph, rules):
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch

    runner = ClosedLoopRunner(engine, DeviceBatch(batch, 0), np.full((batch.B, 2), 1e9), rules=rules)
    out = runner.run_graph(cycles, record=True) if graph else runner.run(cycles, record=True)
    return runner, out


# ---------------------------------------------------------------- the test bodies every pass shares
def host_parity(engine, oracle, rule, name, skip_ego=None):
    """One host call is one launch and the reference's answer; with skip_ego, that ego skipped: -1 / NaN / 0, its poisoned rows untouched.
    -> (batch, refs, the dense result, the pass's outputs) for the rule's own assertions."""
    p = PASSES[rule]
    batch, refs = p.ref.case(oracle, name)
    n0 = launches(engine, rule)
    out, got = dense_and_pass(engine, rule, batch)
    assert launches(engine, rule) == n0 + 1  # one launch
    check_against(rule, refs, (out.cost, out.flags), got, name)
    if skip_ego is not None:
        skip = skip_only(batch, skip_ego)
        out.flags[skip_ego] = POISON
        skipped = getattr(engine, p.method)(batch, out.cost, out.flags, skip=skip)
        assert (skipped[0][skip_ego] == POISON).all()
        out.flags[skip_ego] = refs[skip_ego].flags_in
        skipped[0][skip_ego] = refs[skip_ego].flags_in
        check_against(rule, refs, (out.cost, out.flags), skipped, name + " skip", skip)
    return batch, refs, out, got


def device_parity(engine, oracle, rule, name, skip_ego=2):
    """HOST and DEVICE give the same bits, and so do two runs; a launch order and a skipped ego are honoured."""
    batch, refs = PASSES[rule].ref.case(oracle, name)
    host_out, host = dense_and_pass(engine, rule, batch)
    res = Resident(engine, rule, batch)
    res.pair()
    plain = res.fetch()
    check_against(rule, refs, (host_out.cost, host_out.flags), plain, name + " device")
    for a, b in zip(host, plain):
        assert same_bits(a, b), name
    res = Resident(engine, rule, batch)
    res.pair()
    for a, b in zip(plain, res.fetch()):
        assert same_bits(a, b), name  # two runs, identical bits
    skip = skip_only(batch, skip_ego)
    res = Resident(engine, rule, batch, order=np.arange(batch.B)[::-1], skip=skip, poison=skip_ego)
    res.pair()
    got = res.fetch()
    assert (got[0][skip_ego] == POISON).all()  # the poisoned rows of the skipped ego come back untouched
    tables = (host_out.cost.copy(), host_out.flags.copy())
    tables[1][skip_ego] = POISON
    check_against(rule, refs, tables, got, name + " device, reversed order, skip", skip)
    keep = skip == 0
    for a, b in zip(got, plain):
        assert same_bits(a[keep], b[keep])


def idempotence(engine, oracle, rule, names):
    """The pass over its own output: the same words and the same winner.  Yields (batch, the dense result, the first run's outputs) per
    case for the rule's own assertions."""
    p = PASSES[rule]
    for name in names:
        batch, _ = p.ref.case(oracle, name)
        out, first = dense_and_pass(engine, rule, batch)
        second = getattr(engine, p.method)(batch, out.cost, first[0])
        assert first[3].sum() > 0, name
        for a, b in zip(first[:3], second[:3]):
            assert same_bits(a, b), name
        assert same_bits(second[3], first[3] if p.recounts else np.zeros_like(first[3])), name
        yield batch, out, first


def graph_replay(engine, oracle, rule, name):
    """The dense call and the pass on one stream: eager, eager again without an allocation, captured, replayed twice.
    -> (the resident batch, the graph, the host dense result, the launch counter before) for the rule's own replays."""
    import torch

    batch, refs = PASSES[rule].ref.case(oracle, name)
    res = Resident(engine, rule, batch)
    dev = res.db.dev
    n0 = launches(engine, rule)
    res.pair(torch.cuda.current_stream(dev).cuda_stream)  # eager (also the warm-up of the capture)
    eager = res.fetch()
    assert launches(engine, rule) == n0 + 1
    free = torch.cuda.mem_get_info()[0]
    res.pair(torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert torch.cuda.mem_get_info()[0] == free  # enqueue only: a second call allocates nothing
    side = torch.cuda.Stream(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        res.pair(side.cuda_stream)  # a linear chain on one stream: the pass directly behind the dense call
    torch.cuda.synchronize(dev)
    assert launches(engine, rule) == n0 + 3
    for step in range(2):
        res.clobber()
        graph.replay()
        replay = res.fetch()
        for a, b in zip(eager, replay):
            assert same_bits(a, b), step
    host = PASSES[rule].dense(engine, batch)
    check_against(rule, refs, (host.cost, host.flags), replay, "replay")
    assert launches(engine, rule) == n0 + 3  # a replay is not a call
    return res, graph, host, n0


def never_asks(oracle, rule, name):
    """A ctx that never asks pays nothing: the dense call alone launches no pass and leaves the oracle's tables; then the pass, once, is
    one launch of its own kernel and of nothing else.  -> the dense result."""
    p = PASSES[rule]
    batch, refs = p.ref.case(oracle, name)
    assert batch.w_obstacle == 0.0
    with FrenetEngine(0) as other:
        o = p.dense(other, batch)
        assert other.get_option("lattice_launches") == 1 and other.get_option("rank_launches") == 0
        assert all(other.get_option(q.launches) == 0 for q in PASSES.values())
        for b, r in enumerate(refs):  # the bits of the dense call alone: the oracle's tables
            assert np.array_equal(o.flags[b], r.flags_in) and o.best_idx[b] == r.best_in
        getattr(other, p.method)(batch, o.cost, o.flags)
        assert all(other.get_option(q.launches) == (q is p) for q in PASSES.values())
        assert other.get_option("lattice_launches") == 1 and other.get_option("clearance_launches") == 0
    return o


def _oversized(params):
    big = _abi.FpParams.from_buffer_copy(params)
    big.nd, big.nv, big.nt = 129, 128, 1  # C = 16 512 > FP_MAX_CAND
    return big


class HostCall:
    """The rule's C entry point over host arrays with every argument replaceable; `good` is the struct the product builds from the batch."""

    def __init__(self, engine, rule, batch):
        self.engine, self.p, self.batch, self.held = engine, PASSES[rule], batch, {}
        self.out = self.p.dense(engine, batch)
        self.params, self.fb = host_structs(batch)
        self.flags = self.out.flags.copy()
        self.idx, self.best, self.count = np.empty(batch.B, dtype=np.int32), np.empty(batch.B), np.empty(batch.B, dtype=np.int32)
        self.good = self.p.rule.struct(batch, self._addr)

    def _addr(self, name):
        self.held[name] = rules.array(self.batch, name)  # (kept alive over the calls)
        return self.held[name].ctypes.data

    def __call__(self, struct, **kw):
        a = dict(params=self.params, fb=self.fb, cost=self.out.cost, flags=self.flags, idx=self.idx, best=self.best)
        a.update(kw)
        ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return getattr(self.engine._lib, self.p.rule.fn)(self.engine._ctx, C.byref(a["params"]), C.byref(a["fb"]), None if struct is None else C.byref(struct),
                                                         ptr(a["cost"]), ptr(a["flags"]), ptr(a["idx"]), ptr(a["best"]), self.count.ctypes.data, _abi.FP_MEM_HOST, None)


def host_error_codes(engine, rule, batch, bad):
    """The refusals every pass shares, through host memory: no struct, the rule's `bad` structs and every NULL table give -1, a lattice
    beyond FP_MAX_CAND -4; a refused call launched and wrote nothing; the good call then is one launch and the Python method's answer.
    -> the HostCall for the rule's own cases."""
    p = PASSES[rule]
    call = HostCall(engine, rule, batch)
    n0 = launches(engine, rule)
    for struct in (None, *bad):
        assert call(struct) == -1
    for table in ("cost", "flags", "idx", "best"):
        assert call(call.good, **{table: None}) == -1, table
    assert call(call.good, params=_oversized(call.params)) == -4
    assert launches(engine, rule) == n0 and np.array_equal(call.flags, call.out.flags)  # (a refused call launched and wrote nothing)
    assert call(call.good) == 0 and launches(engine, rule) == n0 + 1
    want = getattr(engine, p.method)(batch, call.out.cost, call.out.flags)
    assert np.array_equal(call.flags, want[0]) and np.array_equal(call.idx, want[1]) and np.array_equal(call.count, want[3])
    return call


def device_error_codes(engine, rule, batch, refused):
    """The same through device memory: every NULL table and the rule's `refused` keyword arguments raise -1, a lattice beyond FP_MAX_CAND
    gives -4, none of them launches; the count pointer is optional.  -> (the resident batch, the launch counter) for the rule's own cases."""
    p = PASSES[rule]
    res = Resident(engine, rule, batch)
    res.pair()
    first = res.fetch()
    n0 = launches(engine, rule)
    for kw in (dict(cost_tbl=0), dict(flag_tbl=0), dict(best_idx=0), dict(best_cost=0), *refused):
        with pytest.raises(_abi.FrenetGpuError) as err:
            res.call(**kw)
        assert err.value.code == -1, kw
    struct = p.rule.struct(batch, lambda name: res.db.t[name].data_ptr())
    rc = getattr(engine._lib, p.rule.fn)(engine._ctx, C.byref(_oversized(res.db.params)), C.byref(res.fb), C.byref(struct), res.cost.data_ptr(), res.flags.data_ptr(),
                                         res.bi.data_ptr(), res.bc.data_ptr(), None, _abi.FP_MEM_DEVICE, None)
    assert rc == -4
    assert launches(engine, rule) == n0
    res.call(**{p.rule.count: 0})  # the count is optional; the pass over its own output leaves every word and the winner
    for a, b in zip(first, res.fetch()):
        assert same_bits(a, b)
    assert launches(engine, rule) == n0 + 1
    return res, n0 + 1
