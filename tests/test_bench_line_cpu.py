"""bench.py's ONE stdout line: the compact contract line built from a full run record (no GPU: the builder is pure Python).

The driver parses the last stdout line; round 5's 24.7 KB line did not parse and the round went unmeasured.  These tests pin:
the line built from a real full record (profiles/r05_bench.json, the last record the old format printed) is < 4096 bytes,
strict JSON, has exactly the contract key set, scalars only below the second level, and carries the record's numbers.
"""
import json
import math
import os

import pytest

import bench
from conftest import ROOT


@pytest.fixture(scope="module")
def full():
    rec = json.load(open(os.path.join(ROOT, "profiles", "r05_bench.json")))
    rec = bench._finite(rec)
    rec["extras_file"] = bench.EXTRAS_FILE
    return rec


def _strict(text):
    return json.loads(text, parse_constant=lambda c: pytest.fail(f"non-strict JSON constant {c}"))


def test_line_is_small_strict_and_has_exactly_the_contract_keys(full):
    text = bench.dump_line(bench.contract_line(full))
    assert len(text.encode()) < bench.LINE_LIMIT == 4096 and "\n" not in text
    line = _strict(text)
    assert tuple(line) == bench.CONTRACT_KEYS
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in line
    assert line["metric"] == json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"]
    assert line["vs_baseline"] is None and line["dtype"] == "f64" and line["higher_is_better"] is True


def test_line_carries_the_records_numbers(full):
    line = bench.contract_line(full)
    assert line["value"] == pytest.approx(full["value"], rel=1e-8) and line["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-6)
    r = line["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-4) and r["traffic"] == pytest.approx(full["roofline"]["traffic"], rel=1e-8)
    assert r["binding"] == "valu_fp64" and r["valu_fp64_frac"] == pytest.approx(full["roofline"]["valu_fp64"]["frac"], rel=1e-5)
    c = line["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == full["cpu_baseline"]["cores"] and c["value"] == pytest.approx(full["cpu_baseline"]["value"], rel=1e-5)
    assert line["parity"]["index_exact"] is True and line["parity"]["max_abs_cost_err"] <= 1e-6
    assert line["legs"]["config4"]["ms_per_step"] == pytest.approx(full["config4"]["ms_per_step"], rel=1e-5) and line["legs"]["config4"]["parity_ok"] is True
    assert line["legs"]["closed_loop_FISS+"]["us_per_cycle"] == pytest.approx(full["closed_loop"]["FISS+"]["us_per_cycle"], rel=1e-5)


def test_line_has_scalars_only_below_the_second_level_and_short_strings(full):
    line = bench.contract_line(full)

    def walk(o, depth):
        if isinstance(o, dict):
            assert depth < 3, "the driver's reader keeps scalars of nested objects only"
            for v in o.values():
                walk(v, depth + 1)
        else:
            assert not isinstance(o, (list, tuple))
            if isinstance(o, str):
                assert len(o) <= 200
            if isinstance(o, float):
                assert math.isfinite(o)

    walk(line, 0)
    for k in ("config", "roofline", "cpu_baseline", "parity"):
        assert all(not isinstance(v, dict) for v in line[k].values()), k


def test_a_failed_parity_or_a_nan_cannot_hide(full):
    bad = json.loads(json.dumps(full))
    bad["config4"]["parity"]["stats_exact"] = False
    bad["config2"]["parity"]["max_abs_cost_err"] = 1e-3
    line = bench.contract_line(bad)
    assert line["legs"]["config4"]["parity_ok"] is False and line["legs"]["config2"]["parity_ok"] is False
    bad["parity"]["batches"][1]["index_exact"] = False
    assert bench.contract_line(bad)["parity"]["index_exact"] is False
    nan = bench._finite({"a": float("nan"), "b": [float("inf"), 1.0]})
    assert nan == {"a": None, "b": [None, 1.0]}
    with pytest.raises(ValueError):
        bench.dump_line({"x": float("nan")})


def test_an_oversized_line_is_refused(full):
    line = bench.contract_line(full)
    line["config"]["workload"] = "x" * 5000
    with pytest.raises(SystemExit):
        bench.dump_line(line)


def test_multi_gpu_record_without_the_single_gpu_legs(full):
    rec = {k: full[k] for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                                "roofline")}
    rec.update(n_gpus=8, cpu_baseline=None, parity=None, extras_file="bench_extras.json")
    line = _strict(bench.dump_line(bench.contract_line(rec)))
    assert line["n_gpus"] == 8 and line["cpu_baseline"] is None and line["legs"] is None and line["parity"] is None


def test_emit_prints_one_line_and_writes_the_side_file(full, tmp_path, capsys, monkeypatch):
    monkeypatch.setenv("BENCH_EXTRAS_FILE", str(tmp_path / "x.json"))
    bench.emit(dict(full))
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and out.endswith("}\n")
    assert _strict(out)["extras_file"] == "x.json"
    side = json.load(open(tmp_path / "x.json"))
    assert side["config4"]["stage_ms"] and side["closed_loop"]["FOP"]["value"] > 0


def test_line_from_the_current_rounds_full_record():
    """The same on round 6's own full record (profiles/r06_bench_extras.json: the side file of the run behind profiles/r06_bench.json):
    the line bench.py printed equals the line built again from the record."""
    rec = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_extras.json")))
    printed = _strict(open(os.path.join(ROOT, "profiles", "r06_bench.json")).read())
    built = _strict(bench.dump_line(bench.contract_line(rec)))
    assert tuple(printed) == bench.CONTRACT_KEYS
    assert built == printed
    assert printed["legs"]["overlap"]["parity_ok"] is True and printed["legs"]["config4"]["ms_per_step"] < 0.21
    assert printed["roofline"]["traffic"] < 1.2 * printed["roofline"]["algorithmic_bytes_per_launch"]


def test_dump_outputs_are_float64_and_a_fixed_sample_beyond_the_limit(tmp_path):
    """--dump-outputs: every output as <name>.npy in float64 (exact for int32 / uint32 words); over the limit the same seeded sample
    of egos from every array, named by sample_rows.npy, and the same sample on every run."""
    import numpy as np

    rng = np.random.default_rng(1)
    arrays = {"best_idx": rng.integers(-1, 567, 1000).astype(np.int32), "best_flags": rng.integers(0, 2**32, 1000, dtype=np.uint64).astype(np.uint32),
              "best_traj": rng.standard_normal((1000, 16, 8))}
    assert bench.write_outputs(str(tmp_path / "all"), arrays) == 1000 * (8 + 8 + 16 * 8 * 8)
    for k, v in arrays.items():
        got = np.load(tmp_path / "all" / f"{k}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, v.astype(np.float64))
    assert not (tmp_path / "all" / "sample_rows.npy").exists()
    limit = 100_000
    n = bench.write_outputs(str(tmp_path / "a"), arrays, limit, "_rank1")
    assert n <= limit
    rows = np.load(tmp_path / "a" / "sample_rows_rank1.npy").astype(np.int64)
    assert 0 < len(rows) < 1000 and np.array_equal(rows, np.unique(rows))
    for k, v in arrays.items():
        assert np.array_equal(np.load(tmp_path / "a" / f"{k}_rank1.npy"), v[rows].astype(np.float64))
    bench.write_outputs(str(tmp_path / "b"), arrays, limit, "_rank1")
    assert np.array_equal(np.load(tmp_path / "b" / "sample_rows_rank1.npy"), rows)


def test_dump_zeroes_exactly_what_the_abi_marks_absent(oracle):
    """absent_to_zero: NaN where include/frenet_gpu.h says a value does not exist becomes 0 - the series past each row's length (the
    region is the oracle's own non-NaN pattern of the winner's series, exactly), everything of an ego without a result (FOP: best_idx
    -1; FISS+: best_ijk -1 and not refined) - and any other non-finite value stays, so a defect still shows."""
    import numpy as np

    from fiss_plus_planner_amd import synth

    b = synth.make_config(3, B=48)
    probs = oracle.problems_from_batch(b, list(range(b.B)))
    idx, _ = oracle.fop_plan_batch(probs, threads=4)
    winners = np.nonzero(idx >= 0)[0][:16]
    assert len(winners) >= 8
    for e in winners:
        bi = int(idx[e])
        t = probs[e].eval_traj(b.d_samples[bi // (b.nv * b.nt)], b.v_samples[e, bi % b.nv], b.t_samples[(bi // b.nv) % b.nt], dump=True, stride=112)
        fl = np.array([t.N << 8 | t.M << 20], dtype=np.uint32)
        out = bench.absent_to_zero({"best_idx": np.array([bi]), "best_cost": np.array([np.nan]), "best_flags": fl,
                                    "best_traj": np.full((1, 16, 112), np.nan)}, fiss=False)
        assert np.array_equal(np.isnan(out["best_traj"][0]), ~np.isnan(t.arrays)), (e, t.N, t.M)
        assert np.isnan(out["best_cost"][0])  # a winner's cost is never zeroed
    none = bench.absent_to_zero({"best_idx": np.array([-1]), "best_cost": np.array([np.nan]), "best_flags": np.zeros(1, np.uint32),
                                 "best_traj": np.full((1, 16, 112), np.nan)}, fiss=False)
    assert none["best_cost"][0] == 0 and (none["best_traj"] == 0).all()
    inf = bench.absent_to_zero({"best_idx": np.array([-1]), "best_cost": np.array([np.inf]), "best_flags": np.zeros(1, np.uint32),
                                "best_traj": np.full((1, 16, 112), np.inf)}, fiss=False)
    assert np.isinf(inf["best_cost"][0]) and np.isinf(inf["best_traj"]).all()
    # FISS+: none = best_ijk -1 and refined 0; a refined result has best_ijk -1 too, and keeps its values
    f = bench.absent_to_zero({"best_ijk": np.array([[-1, -1, -1], [-1, -1, -1], [2, 3, 4]]), "refined": np.array([0, 1, 0]),
                              "best_cost": np.array([np.nan, np.nan, np.nan]), "end_state": np.full((3, 3), np.nan),
                              "best_flags": np.zeros(3, np.uint32), "best_traj": np.full((3, 16, 16), np.nan)}, fiss=True)
    assert f["best_cost"][0] == 0 and (f["end_state"][0] == 0).all()
    assert np.isnan(f["best_cost"][1:]).all() and np.isnan(f["end_state"][1:]).all()
