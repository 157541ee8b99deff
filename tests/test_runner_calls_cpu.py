"""ClosedLoopRunner's cycle, call for call: what one step() / record() hands to the C ABI in every valid configuration, against the
recording of tests/golden/runner_calls.json.

No device and no library: the engine is a FrenetEngine without a context whose `_lib` records (name, args) and returns 0, the DeviceBatch
holds CPU tensors.  Every argument is normalised to something that does not depend on an address: a struct passed by reference is its
name among the runner's structs (or "temp") plus its fields, an address is the name of the tensor it belongs to.  An address that
belongs to no known tensor fails the test.

`python tests/test_runner_calls_cpu.py` writes the fixture.  It was written once, from the runner as it stood before its cycle was
described by cycle_plan(), and is not to be regenerated along with a change of the runner: it is what such a change is held against.
"""
import ctypes as C
import dataclasses
import itertools
import json
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(ROOT, "tests", "golden", "runner_calls.json")
N_VALID, N_SEQUENCES = 80, 28  # of the 288 combinations below; the distinct sequences of call names
MIN_ADDRESS = 1 << 16  # a positional integer from here on is an address (the scalars of these calls are counts, strides and enums)


class RecordingLib:
    """Every fp_* entry point appends (name, args) and reports success."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("fp_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0

        return call


def recording_engine():
    from fiss_plus_planner_amd.engine import FrenetEngine

    eng = FrenetEngine.__new__(FrenetEngine)
    eng._lib, eng._ctx = RecordingLib(), None
    return eng


def cpu_device_batch(batch):
    """A DeviceBatch of CPU tensors: the arrays DeviceBatch.__init__ uploads, without a device."""
    import torch

    from fiss_plus_planner_amd import device_batch as DB
    from fiss_plus_planner_amd import rules
    from fiss_plus_planner_amd.engine import device_batch, make_params

    db = DB.DeviceBatch.__new__(DB.DeviceBatch)
    db.torch, db.host, db.dev = torch, batch, torch.device("cpu")
    db.t = {k: torch.from_numpy(np.ascontiguousarray(getattr(batch, k))) for k in DB._NAMES}
    for k in ("samp_min", "samp_max", "samp_res"):
        db.t[k] = torch.from_numpy(getattr(batch, k))
    for rule in rules.TABLE:
        if rule.carried(batch):
            db.t.update((k, torch.from_numpy(rules.array(batch, k))) for k in rule.arrays)
    db.params = make_params(batch)
    db.fb = device_batch(batch, {k: (v.data_ptr() if v.numel() else 0) for k, v in db.t.items() if k in DB._NAMES})
    return db


def configurations():
    """(key, planner, the runner's keyword arguments as a function of the batch) for the whole product; the batch per configuration."""
    import rules_eval_ref as RR

    from fiss_plus_planner_amd.agents import AgentGroups
    from fiss_plus_planner_amd.fallback import FallbackStop

    base = RR.all_rules_batch()
    assert base.B == 5
    groups = AgentGroups([[0, 1], [2, 3, 4]], 30, "hold", col_base=int(base.n_obs))
    for planner in ("FOP", "FISS", "FISS+"):
        for fused, rules, audit, enforce, fallback, obey, agents in itertools.product(
                (True, False), ((), ("gates", "gaps")), ((), ("envelope",)), ((), ("gates",)), (False, True), (False, True), (False, True)):
            if obey and not fallback:
                continue
            batch = dataclasses.replace(base, ego=base.ego.copy(), t_now=base.t_now.copy())
            if agents:
                batch = groups.attach(batch, int(base.T_obs))
            kw = dict(fused=fused, rules=rules, audit=audit, enforce=enforce, agents=groups if agents else None,
                      fallback=FallbackStop([2.0, 4.0], obey=("gates",) if obey else ()) if fallback else None)
            words = [planner, "fused" if fused else "unfused"] + [w for w, on in (("rules", rules), ("audit", audit), ("enforce", enforce), ("fallback", fallback),
                                                                                 ("obey", obey), ("agents", agents)) if on]
            yield " ".join(words), planner, batch, kw


class Names:
    """The runner's structs by identity and its tensors by address."""

    def __init__(self, run):
        import torch

        self.structs, self.tensors = [(run.db.params, "db.params")], {}
        for k, v in run.db.t.items():
            self._tensor(v, "t." + k)
        for attr, v in vars(run).items():
            if isinstance(v, C.Structure):
                self.structs.append((v, attr))
            elif isinstance(v, torch.Tensor):
                self._tensor(v, attr)
            elif isinstance(v, dict):  # (n_flagged by rule; the uploaded fallback / agents arrays by their own names)
                for k, t in v.items():
                    if isinstance(t, torch.Tensor):
                        self._tensor(t, f"upload.{k}" if attr.startswith("_") else f"{attr}.{k}")
        for rule, struct, _ in getattr(run, "passes", ()):
            self.structs.append((struct, "pass." + rule.name))

    def _tensor(self, t, name):
        if t.numel():
            assert self.tensors.setdefault(t.data_ptr(), name) == name, (name, self.tensors[t.data_ptr()])

    def address(self, value, where):
        if not value:
            return None
        assert value in self.tensors, f"{where}: the address {value:#x} belongs to no tensor of the runner or its batch"
        return self.tensors[value]

    def fields(self, struct, where):
        out = {}
        for name, ctype in struct._fields_:
            v = getattr(struct, name)
            if ctype is C.c_void_p:
                out[name] = self.address(v, f"{where}.{name}")
            elif isinstance(v, C._Pointer):  # (fp_rule_set: a pointer per rule)
                out[name] = self.fields(v.contents, f"{where}.{name}") if v else None
            else:
                out[name] = scalar(v)
        return out

    def arg(self, a, where):
        if a is None:
            return None
        if hasattr(a, "_obj"):  # byref
            label = next((n for s, n in self.structs if s is a._obj), "temp")
            return {"struct": label, "type": type(a._obj).__name__, "fields": self.fields(a._obj, f"{where} ({label})")}
        if isinstance(a, int) and not isinstance(a, bool) and (a in self.tensors or a >= MIN_ADDRESS):
            return {"tensor": self.address(a, where)}
        return scalar(a)


def scalar(v):
    if isinstance(v, float) and not math.isfinite(v):
        return repr(v)
    assert isinstance(v, (int, float, str, bool)), v
    return v


def normalised(run, calls):
    names = Names(run)
    return [[name, [names.arg(a, f"{name} argument {i}") for i, a in enumerate(args)]] for name, args in calls]


def record_all():
    """{key: {"step": calls, "record": calls}} for every valid configuration, plus the invalid keys; one configuration also records
    with poll=True."""
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner

    eng = recording_engine()
    out, invalid, runners = {}, [], {}
    for key, planner, batch, kw in configurations():
        try:
            run = ClosedLoopRunner(eng, cpu_device_batch(batch), np.full((batch.B, 2), 1e6), planner, **kw)
        except ValueError:
            invalid.append(key)
            continue
        assert not eng._lib.calls, key  # (the constructor calls nothing)
        run.step(0)
        first = normalised(run, eng._lib.calls)
        eng._lib.calls.clear()
        run.step(0)
        assert normalised(run, eng._lib.calls) == first, f"{key}: the second step differs from the first"
        eng._lib.calls.clear()
        run.log_reset(4, poll=False)
        run.record(0)
        out[key] = {"step": first, "record": normalised(run, eng._lib.calls)}
        eng._lib.calls.clear()
        if key == "FISS+ unfused fallback agents":
            run.log_reset(4, poll=True)
            run.record(0)
            out[key]["record_poll"] = normalised(run, eng._lib.calls)
            eng._lib.calls.clear()
        runners[key] = run
    return out, invalid, runners


def packed(record):
    """The record with every struct dump stored once: {"structs": [...], "configurations": {key: ...}} - eighty configurations pass the
    same few structs."""
    table, index = [], {}

    def pack(x):
        if isinstance(x, list):
            return [pack(y) for y in x]
        if isinstance(x, dict) and "struct" in x:
            k = json.dumps(x, sort_keys=True)
            if k not in index:
                index[k] = len(table)
                table.append(x)
            return {"$": index[k]}
        return x

    return {"configurations": {key: {part: pack(calls) for part, calls in parts.items()} for key, parts in record.items()}, "structs": table}


def unpacked(fixture):
    table = fixture["structs"]

    def unpack(x):
        if isinstance(x, list):
            return [unpack(y) for y in x]
        return table[x["$"]] if isinstance(x, dict) and "$" in x else x

    return {key: {part: unpack(calls) for part, calls in parts.items()} for key, parts in fixture["configurations"].items()}


def predicted_names(plan, kw):
    """The call names of one step() + record() as cycle_plan's record says them."""
    from fiss_plus_planner_amd import rules

    stage_calls = {"plan": [plan.plan_call], "rules": [rules.by_name[r].fn for r in rules.by_name if r in kw["rules"]], "audit": ["fp_rules_eval"],
                   "fallback": [plan.fallback_call], "share": ["fp_obstacles_from_plans"], "advance": ["fp_advance"]}
    assert tuple(s for s in stage_calls if s in plan.stages) == tuple(plan.stages)  # (the fixed order)
    assert ("advance" in plan.stages) == (not plan.handover_inside)
    return [n for s in plan.stages for n in stage_calls[s]] + ["fp_loop_record"]


@pytest.fixture(scope="module")
def recorded():
    return record_all()


def test_the_valid_configurations_and_their_sequences(recorded):
    record, invalid, _ = recorded
    assert len(record) == N_VALID and len(record) + len(invalid) == 288
    sequences = {tuple(c[0] for c in parts["step"] + parts["record"]) for parts in record.values()}
    assert len(sequences) == N_SEQUENCES


def test_cycle_plan_predicts_the_call_names(recorded):
    from fiss_plus_planner_amd.device_batch import cycle_plan

    record, _, runners = recorded
    kws = {key: (planner, kw) for key, planner, _, kw in configurations()}
    for key, parts in record.items():
        planner, kw = kws[key]
        plan = cycle_plan(planner, kw["fused"], kw["rules"], kw["audit"], kw["enforce"], kw["fallback"] is not None,
                          kw["fallback"].obey if kw["fallback"] is not None else (), kw["agents"] is not None)
        assert [c[0] for c in parts["step"] + parts["record"]] == predicted_names(plan, kw), key
        drives = parts["record"][0][1][4:6]  # fp_loop_record's best_idx / end_state
        assert (drives[0] is not None, drives[1] is not None) == (plan.drives == "best_idx", plan.drives == "end_state"), key
        assert parts["record"][0][1][1]["struct"] == ("fb_params" if plan.later_params == "fb_params" else "db.params"), key


def test_the_calls_equal_the_recording(recorded):
    record, _, _ = recorded
    with open(FIXTURE) as f:
        want = unpacked(json.load(f))
    assert list(record) == list(want)
    for key in want:
        for part in want[key]:
            got = json.loads(json.dumps(record[key][part]))  # (tuples -> lists, as the fixture went through)
            assert [c[0] for c in got] == [c[0] for c in want[key][part]], (key, part)
            for g, w in zip(got, want[key][part]):
                assert g == w, (key, part, g[0], [i for i, (x, y) in enumerate(zip(g[1], w[1])) if x != y])
        assert set(record[key]) == set(want[key]), key


def test_a_dropped_runner_is_freed_at_once():
    """The chain holds no reference to the runner: without a cycle the runner, its tensors and its batch go when the last name does,
    not when the cycle collector gets to them (a loop over fresh runners would pile up device memory until then)."""
    import gc
    import weakref

    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner

    eng = recording_engine()
    for key, planner, batch, kw in configurations():
        if key in ("FOP fused", "FOP unfused rules fallback obey agents", "FISS+ unfused audit enforce", "FISS+ fused enforce"):
            gc.collect()
            gc.disable()
            try:
                run = ClosedLoopRunner(eng, cpu_device_batch(batch), np.full((batch.B, 2), 1e6), planner, **kw)
                run.step(0)
                run.log_reset(4)
                run.record(0)
                ref = weakref.ref(run)
                del run
                assert ref() is None, key
            finally:
                gc.enable()


if __name__ == "__main__":
    rec = record_all()[0]
    with open(FIXTURE, "w") as f:
        json.dump(packed(rec), f, indent=None, separators=(",", ":"), sort_keys=False)
        f.write("\n")
    print(len(rec), "configurations,", os.path.getsize(FIXTURE), "bytes")
