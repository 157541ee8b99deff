"""CPU: the loop log (fp_loop_record / fp_loop_log, ABI 17) as far as it can be checked without a device - header against binding,
closed_loop.result_from_log on a hand-built log, the loud failure without a GPU, and the numpy bookkeeping reference the GPU tests
compare the kernel with (tests/looplog_ref.py) against a hand-written expected log."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import looplog_ref as R
from conftest import ROOT
from fiss_plus_planner_amd import _abi


def _header():
    return open(os.path.join(ROOT, "include", "frenet_gpu.h")).read()


def test_header_declares_the_log_and_the_binding_mirrors_it(tmp_path):
    hdr = _header()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+fp_loop_record\s*\(", code) and "fp_loop_record" in _abi.EXPORTED_SYMBOLS
    assert re.search(r"}\s*fp_loop_log\s*;", code)
    assert int(re.search(r"#define FP_LOG_COLS (\d+)", hdr).group(1)) == 16 == _abi.FP_LOG_COLS == R.COLS
    assert int(re.search(r"#define FP_ABI_VERSION (\d+)", hdr).group(1)) == _abi.FP_ABI_VERSION >= 17
    # field order: the struct body's member names, in the order the header declares them
    body = re.search(r"typedef struct \{([^}]*)\}\s*fp_loop_log\s*;", code).group(1)
    names = re.findall(r"(\w+)\s*;", body)
    assert names == [f[0] for f in _abi.FpLoopLog._fields_] == ["max_rows", "reserved0", "rows", "row_stats", "n_rows", "sealed", "stats_sum", "n_running"]
    # sizes, offsets and the column enum as the C compiler sees them
    cols = ("TIME_STEP", "X", "Y", "YAW", "VELOCITY", "VELOCITY_Y", "S", "S_DD", "D", "D_DD", "COST", "D_END", "V_END", "T_END", "BEST_IDX", "DONE")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "frenet_gpu.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(fp_loop_log));']
    lines += [f'  printf("{n} %zu\\n", offsetof(fp_loop_log, {n}));' for n in names]
    lines += [f'  printf("FP_LOG_{c} %d\\n", (int)FP_LOG_{c});' for c in cols]
    lines += ['  return 0;', '}']
    src = tmp_path / "log_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "log_layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_abi.FpLoopLog)
    for n in names:
        assert int(got[n]) == getattr(_abi.FpLoopLog, n).offset, n
    for i, c in enumerate(cols):
        assert int(got[f"FP_LOG_{c}"]) == i == getattr(_abi, f"LOG_{c}") == getattr(R, c), c
    # the stub INTEGRATION.md shows carries the same struct
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    ns = {"C": C}
    exec(txt[txt.index("class FpLoopLog(C.Structure):"):txt.index("FP_ABI_VERSION =")], ns)
    assert [(f[0], C.sizeof(f[1])) for f in ns["FpLoopLog"]._fields_] == [(f[0], C.sizeof(f[1])) for f in _abi.FpLoopLog._fields_]
    assert ns["FP_LOG_COLS"] == 16


def _row(t, x, y, yaw, fr, cost, end, idx, done):
    s, s_d, s_dd, d, d_d, d_dd = fr
    return [t, x, y, yaw, s_d, d_d, s, s_dd, d, d_dd, cost, end[0], end[1], end[2], idx, done]


def test_result_from_log_on_a_hand_built_log():
    """Three egos: one reaches the goal after 3 rows, one finds no solution in its first cycle (0 rows, Stats counted), one drove more
    cycles than the log holds rows."""
    from fiss_plus_planner_amd.closed_loop import ClosedLoopResult, LoopLog, result_from_log

    max_rows = 4
    rows = np.full((3, max_rows, 16), np.nan)
    row_stats = np.zeros((3, max_rows, 4), dtype=np.int32)
    fr = [[10.0 + i, 5.0, 0.1 * i, -0.5, 0.01 * i, 0.0] for i in range(6)]
    for i in range(3):
        rows[0, i] = _row(i, 100.0 + i, 50.0 - i, 0.25 * i, fr[i + 1], 7.5 + i, (0.5, 9.0, 8.5), 37 + i, _abi.DONE_GOAL if i == 2 else _abi.RUNNING)
        row_stats[0, i] = [125, 125, 10 + i, 20 + i]
    for i in range(max_rows):
        rows[2, i] = _row(i, 1.0 * i, 2.0 * i, 0.0, fr[i + 1], 3.0, (np.nan, np.nan, np.nan) if i == 1 else (0.0, 5.0, 9.0), -1, _abi.RUNNING)
        row_stats[2, i] = [1, 2, 3, 4]
    log = LoopLog(rows=rows, n_rows=np.array([3, 0, 9], dtype=np.int32), row_stats=row_stats,
                  stats_sum=np.array([[375, 375, 33, 63], [125, 125, 125, 0], [9, 18, 27, 36]], dtype=np.int64))
    a = result_from_log(log, 0, start=fr[0])
    assert isinstance(a, ClosedLoopResult) and a.goal_reached and len(a.cycles) == 3
    np.testing.assert_array_equal(np.array(a.states), [[100.0, 50.0, 0.0], [101.0, 49.0, 0.25], [102.0, 48.0, 0.5]])
    np.testing.assert_array_equal(log.states(0), np.array(a.states))
    assert [c.start for c in a.cycles] == [fr[0], fr[1], fr[2]]            # the caller's initial state, then the previous row's
    assert [c.cost for c in a.cycles] == [7.5, 8.5, 9.5] and [c.stats for c in a.cycles] == [(125, 125, 10, 20), (125, 125, 11, 21), (125, 125, 12, 22)]
    assert a.cycles[1].end == [0.5, 9.0, 8.5] and int(a.cycles[1].idx[0]) == 38 and all(np.isnan(c.seconds) for c in a.cycles)
    assert np.isnan(a.plan_seconds).all()
    assert (a.stats.num_iter, a.stats.num_trajs_generated, a.stats.num_trajs_validated, a.stats.num_collison_checks) == (375, 375, 33, 63)
    assert all(np.isnan(v) for v in result_from_log(log, 0).cycles[0].start)  # no initial state given
    b = result_from_log(log, 1)
    assert b.cycles == [] and b.states == [] and not b.goal_reached and log.states(1).shape == (0, 3)
    assert (b.stats.num_iter, b.stats.num_trajs_validated) == (125, 125)    # the plan that found nothing still counts (planning.py:129)
    c = result_from_log(log, 2)
    assert len(c.cycles) == max_rows == len(c.states) and not c.goal_reached  # 9 cycles driven, 4 rows kept
    assert int(c.cycles[0].idx[0]) == -1 and np.isnan(c.cycles[1].end).all() and c.stats.num_collison_checks == 36


def test_fp_loop_record_fails_loudly_without_a_device():
    """No CPU path: without a GPU no ctx exists, and the entry point reports the missing ctx through the binding like every other one."""
    import torch

    lib = _abi.load()
    lg, io, p, fb = _abi.FpLoopLog(), _abi.FpLoopIo(), _abi.FpParams(), _abi.FpBatch()
    rc = lib.fp_loop_record(None, C.byref(p), C.byref(fb), C.byref(io), None, None, None, None, C.byref(lg), _abi.FP_MEM_HOST, None)
    assert rc == -1
    with pytest.raises(_abi.FrenetGpuError, match="ctx is NULL"):
        _abi.check(rc)
    if not torch.cuda.is_available():
        from fiss_plus_planner_amd.engine import FrenetEngine

        with pytest.raises(_abi.FrenetGpuError):
            FrenetEngine(0)


def test_bookkeeping_reference_on_a_hand_written_sequence():
    """tests/looplog_ref.py against an expected log written out by hand.  Four egos, max_rows = 2, four steps:
    ego 0 drives three cycles and reaches the goal in the third (the third row does not fit: counted, not written);
    ego 1 finds no solution in its first cycle (Stats counted, no row, sealed);
    ego 2 was finished before the log started (sealed by the reset: its stale Stats never count);
    ego 3 drives every cycle (lattice index decoded into its end state)."""
    d_s, t_s = np.array([-1.0, 0.0, 1.0]), np.array([8.0, 10.0])
    v_s = np.arange(8.0).reshape(4, 2)                       # nv = 2, nt = 2: flat = (i_d * 2 + i_T) * 2 + i_v
    ref = R.LoopLogRef(4, 2, done=[0, 0, 1, 0])
    np.testing.assert_array_equal(ref.sealed, [0, 0, 1, 0])
    ego = np.zeros((4, 6)); cart = np.full((4, 3), np.nan)
    t_now = np.zeros(4, dtype=np.int32); cycles = np.zeros(4, dtype=np.int32); done = np.array([0, 0, 1, 0], dtype=np.int32)
    stats = np.tile(np.array([8, 8, 3, 5], dtype=np.int32), (4, 1))
    want_running = [2, 2, 1, 1]
    for k in range(4):
        for b in (0, 3):
            if done[b] == 0:
                ego[b] = [10.0 * b + k + 1, 2.0, 0.5, 0.1 * k, 0.01, 0.0]
                cart[b] = [b + 0.5 * k, -b, 0.125 * k]
                t_now[b] += 1; cycles[b] += 1
        if k == 0:
            done[1] = 3
        if k == 2:
            done[0] = 1
        best_idx = np.array([5, -1, 7, 2 + k], dtype=np.int32)
        cost = np.array([1.5 + k, np.nan, 9.0, 2.5 + k])
        ref.record(SimpleNamespace(ego=ego.copy(), t_now=t_now.copy(), done=done.copy(), cycles=cycles.copy(), cart=cart.copy(),
                                   best_idx=best_idx, best_cost=cost, stats=stats), d_s, v_s, t_s)
        assert ref.n_running == want_running[k], k
    np.testing.assert_array_equal(ref.n_rows, [3, 0, 0, 4])
    np.testing.assert_array_equal(ref.sealed, [1, 1, 1, 0])
    np.testing.assert_array_equal(ref.stats_sum, [[24, 24, 9, 15], [8, 8, 3, 5], [0, 0, 0, 0], [32, 32, 12, 20]])
    # index 5 = (i_d 1, i_T 0, i_v 1): d 0, v of ego 0 = v_s[0, 1] = 1, T 8;  ego 3: index 2 = (0, 1, 0) -> d -1, v 6, T 10; 3 = (0, 1, 1) -> v 7
    want0 = [_row(0, 0.0, 0.0, 0.0, [1.0, 2.0, 0.5, 0.0, 0.01, 0.0], 1.5, (0.0, 1.0, 8.0), 5, 0),
             _row(1, 0.5, 0.0, 0.125, [2.0, 2.0, 0.5, 0.1, 0.01, 0.0], 2.5, (0.0, 1.0, 8.0), 5, 0)]
    want3 = [_row(0, 3.0, -3.0, 0.0, [31.0, 2.0, 0.5, 0.0, 0.01, 0.0], 2.5, (-1.0, 6.0, 10.0), 2, 0),
             _row(1, 3.5, -3.0, 0.125, [32.0, 2.0, 0.5, 0.1, 0.01, 0.0], 3.5, (-1.0, 7.0, 10.0), 3, 0)]
    np.testing.assert_array_equal(ref.rows[0], want0)
    np.testing.assert_array_equal(ref.rows[3], want3)
    assert np.isnan(ref.rows[1]).all() and np.isnan(ref.rows[2]).all()
    np.testing.assert_array_equal(ref.row_stats[0], [[8, 8, 3, 5]] * 2)
    np.testing.assert_array_equal(ref.row_stats[1], np.zeros((2, 4)))
    # an explicit end state instead of an index: BEST_IDX = -1, the end state copied
    ref2 = R.LoopLogRef(1, 1)
    ref2.record(SimpleNamespace(ego=np.array([[1.0, 2, 3, 4, 5, 6]]), t_now=[7], done=[4], cycles=[1], cart=np.array([[8.0, 9, 10]]),
                                end_state=np.array([[0.25, 11.0, 9.5]]), best_cost=[12.0], stats=np.array([[1, 2, 3, 4]])))
    np.testing.assert_array_equal(ref2.rows[0, 0], [6, 8, 9, 10, 2, 5, 1, 3, 4, 6, 12, 0.25, 11, 9.5, -1, 4])
    assert ref2.sealed[0] == 1 and ref2.n_running == 0
