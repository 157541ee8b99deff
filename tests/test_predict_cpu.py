"""CPU: the reference of the obstacle prediction (predict_ref.py) against an independent integration and against synth.make_batch, the
inputs of the GPU tests, the Python layers that need no device, and the binding of fp_obstacles_predict."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import predict_cases as PC
import predict_ref as R
import pytest

from conftest import ROOT
from fiss_plus_planner_amd import _abi, synth
from fiss_plus_planner_amd.obstacles import TRACK_ARC, TRACK_LANE, TRACK_NONE, ObstacleTable, ObstacleTracks


@pytest.mark.parametrize("kappa", [0.0, 1e-7, 0.02, 0.2])
def test_arc_reference_against_rk4(kappa):
    """The closed form is the truth; RK4 over x' = v cos(yaw), y' = v sin(yaw), yaw' = kappa v, v' = a (v clamped at 0) with 1000
    substeps per tick is the cross-check, so the bar is RK4's own error: per step about (kappa v)^4 v h^5 / 120 with h = 1e-4 s, over
    41 000 steps far below 1e-12 m - what is left is the rounding of 41 000 additions.  Asserted: 1e-8 m.  Observed maximum over 41 rows,
    braking from 5 m/s at 2 m/s^2 to a stop at 2.5 s inside the 4 s horizon: 1.0e-13 (x / y / yaw together)."""
    q = np.array([3.0, -7.0, 0.4, 5.0, -2.0, kappa])
    rows = R.rk4_arc_rows(q, 0.1, 41, 1000)
    worst = 0.0
    for r, got in enumerate(rows):
        (x, y, yaw, valid), undecided = R.arc_pose(q, r * 0.1)
        assert valid == 1.0 and not undecided
        worst = max(worst, abs(got[0] - x), abs(got[1] - y), abs(got[2] - yaw))
    print(f"kappa={kappa}: max |closed form - RK4| = {worst:.3e}")
    assert worst < 1e-8
    assert R.arc_pose(q, 2.6)[0] == R.arc_pose(q, 4.0)[0]  # after the stop (2.5 s) nothing moves


@pytest.mark.parametrize("args", [(4, 9, 9, 7, 50, 50, True, synth.CONFIG_SEEDS[3]), (2, 5, 5, 5, 10, 100, False, synth.CONFIG_SEEDS[2])], ids=["config3", "config2"])
def test_lane_reference_reproduces_make_batch(args):
    """predict_ref on make_tracks(...) against make_batch(...).obs_pose: `valid` exact; x, y, yaw within 1e-12 (the arithmetic is the
    same up to d * n against d * (-sin, cos)(yaw) and the summation order of the cubic).  Observed: 2.8e-14 m, 0 rad."""
    kw = dict(layout="survey8d")
    batch = synth.make_batch(*args, **kw)
    tr = synth.make_tracks(*args, **kw)
    assert tr.model.shape == (batch.S, batch.n_obs) and np.all(tr.model == TRACK_LANE) and np.array_equal(tr.frame_of_scene, np.arange(batch.B))
    assert np.array_equal(tr.dims, batch.obs_dims) and not tr.state[..., 3:].any()
    pose, written, fts, undecided = R.predict(tr.model, tr.state, tr.frame_of_scene, 0, batch.T_obs, batch.T_obs, batch.tick_t, batch.nx, batch.knots, batch.coef)
    R.check_caps(undecided, "make_tracks")
    assert written.all() and np.all(fts == batch.T_obs)
    assert np.array_equal(pose[..., 3], batch.obs_pose[..., 3])
    err = np.abs(pose[..., :3] - batch.obs_pose[..., :3]).max(axis=(0, 1, 2))
    print("max |ref - make_batch| x, y, yaw:", err)
    assert err.max() <= 1e-12


def test_make_tracks_does_not_disturb_make_batch():
    """Same draws, same arrays: digest() of configs 2 and 3 at B = 4 before and after make_tracks, against the arrays built by a draw loop
    restated here is not needed - the committed SHA fixtures of the configs guard the values; this guards the RNG streams' independence."""
    for cfg in (2, 3):
        a = synth.make_config(cfg, B=4).digest()
        args = {2: (4, 5, 5, 5, 10, 100, False, synth.CONFIG_SEEDS[2]), 3: (4, 9, 9, 7, 50, 50, True, synth.CONFIG_SEEDS[3])}[cfg]
        synth.make_tracks(*args, layout="survey8d")
        assert synth.make_config(cfg, B=4).digest() == a
        assert synth.make_batch(*args, layout="survey8d").digest() == a
    golden = os.path.join(ROOT, "BASELINE.json")
    assert os.path.exists(golden)


def test_batch_digest_and_take_with_tracks():
    args = (4, 5, 5, 5, 10, 100, True, 11)
    plain = synth.make_batch(*args)
    tr = synth.make_tracks(*args)
    import dataclasses

    with_tr = dataclasses.replace(plain, track_model=tr.model, track_state=tr.state, track_frame=tr.frame_of_scene)
    assert dataclasses.replace(plain).digest() == plain.digest() != with_tr.digest()
    sub = with_tr.take([3, 1])
    assert np.array_equal(sub.track_model, tr.model[[1, 3]]) and np.array_equal(sub.track_state, tr.state[[1, 3]])
    assert np.array_equal(sub.knots[sub.track_frame], plain.knots[[1, 3]])  # the scenes still follow their own lines
    sh = with_tr.shard(1, 2)
    assert np.array_equal(sh.track_state, tr.state[2:]) and np.array_equal(sh.knots[sh.track_frame], plain.knots[2:])
    assert plain.take([0]).track_model is None
    with pytest.raises(AssertionError):
        dataclasses.replace(plain, track_model=tr.model)  # model and state come together
    with pytest.raises(AssertionError):
        dataclasses.replace(plain, track_model=tr.model[:, :3], track_state=tr.state)


@pytest.mark.parametrize("name", PC.CASE_NAMES)
def test_no_gpu_input_is_undecided(name):
    case = dict(PC.all_cases_lazy())[name]()
    R.check_caps(case["ref"].undecided, name)
    ref = case["ref"]
    assert np.all(np.isfinite(ref.pose[ref.written])) and np.all(np.isnan(ref.pose[~ref.written]))
    assert np.abs(ref.pose[ref.written][..., :2]).max(initial=0.0) <= 1e3  # (the GPU bar's reasoning: coordinates of at most 1e3 m)


def test_cases_cover_what_they_claim():
    valid = lambda c: c["ref"].pose[0, :, :, 3]
    le = PC.line_ends()
    v = valid(le)
    assert v[0, 0] == 1 and v[-1, 0] == 0 and np.all(np.diff(v[:, 0]) <= 0)       # runs off the last knot mid-horizon
    assert v[0, 1] == 0 and v[-1, 1] == 1 and np.all(np.diff(v[:, 1]) >= 0)       # enters over the first knot
    assert not v[:, 2].any() and v[:, 3].all()
    st = PC.stops()["ref"].pose[0]
    for j in (0, 4):  # stops at 0.25 s: rows 3 .. are identical, row 2 is not yet there
        assert np.array_equal(st[3], st[3]) and all(np.array_equal(st[r, j], st[3, j]) for r in range(3, 12)) and not np.array_equal(st[2, j], st[3, j])
    for j in (1, 5):  # stops exactly on row 2
        assert all(np.array_equal(st[r, j], st[2, j]) for r in range(2, 12)) and not np.array_equal(st[1, j], st[2, j])
    assert np.array_equal(st[:, 2], st[:, 3]) and np.array_equal(st[:, 6], st[:, 7])  # v < 0 behaves as v = 0
    assert all(np.array_equal(st[r, 8], st[0, 8]) for r in range(12)) and all(np.array_equal(st[r, 9], st[0, 9]) for r in range(12))
    ab = PC.arc_branch()
    u_end = ab["state"][0, :, 5] * 11.0 / 2
    assert np.sum(np.abs(u_end) < 1e-4) >= 4 and np.sum(np.abs(u_end) > 1e-4) >= 4 and (ab["state"][0, :, 5] == 0).any() and (ab["state"][0, :, 5] < 0).any()
    for key in PC.SWEEP:
        m = PC.sweep(*key)["model"]
        if key[0] >= 3:
            assert all(set(m[s]) == {0, 1, 2} for s in range(3))
    oor, null = dict(PC.all_cases_lazy())["frames_out_of_range"](), dict(PC.all_cases_lazy())["frames_null"]()
    for c in (oor, null):
        lane, arc = c["model"] == R.LANE, c["model"] == R.ARC
        vv = c["ref"].pose[..., 3]
        assert arc.any() and np.all(vv[:, :, :][np.broadcast_to(arc[:, None, :], vv.shape)] == 1)
    assert not null["ref"].pose[..., 3][np.broadcast_to((null["model"] == R.LANE)[:, None, :], null["ref"].pose[..., 3].shape)].any()
    assert oor["ref"].pose[0, :, :, 3][:, oor["model"][0] == R.LANE].any() and not oor["ref"].pose[1:, :, :, 3][np.broadcast_to((oor["model"][1:] == R.LANE)[:, None, :], (2, 20, 6))].any()


def test_row_range_rule():
    for k, t0 in enumerate((0, 3, -2, 22, 27)):
        ref = PC.row_range(k)["ref"]
        assert ref.fts[1] == min(23, t0 + 32) and ref.fts[0] == 23 and ref.fts[2] == 6
        assert np.array_equal(np.nonzero(ref.written[1])[0], np.arange(max(t0, 0), 23)[: max(0, 23 - max(t0, 0))])
        assert np.array_equal(np.nonzero(ref.written[2])[0], np.arange(0, 6))


# ---------------------------------------------------------------------------------------------------------------- ObstacleTracks
def _tracks(n=4):
    return ObstacleTracks(model=[TRACK_LANE, TRACK_ARC, TRACK_NONE, TRACK_LANE][:n], state=np.arange(6.0 * n).reshape(n, 6), dims=np.full((n, 2), 2.0))


def test_obstacle_tracks_validate_and_update():
    t = _tracks()
    assert t.model.dtype == np.int32 and t.state.shape == (4, 6) and t.version == 0
    for bad in (dict(model=[0, 1, 3, 1]), dict(model=[0, 1, -1, 1]), dict(state=np.zeros((4, 5))), dict(dims=np.zeros((3, 2))), dict(model=[[0, 1, 2, 1]])):
        kw = dict(model=[1, 2, 0, 1], state=np.zeros((4, 6)), dims=np.ones((4, 2)))
        kw.update(bad)
        with pytest.raises(ValueError):
            ObstacleTracks(**kw)
    with pytest.raises(ValueError):
        ObstacleTracks(model=[1], state=np.zeros((1, 6)), dims=np.ones((1, 2)), poly=np.zeros((1, 4, 2)))  # poly and nvert come together
    new_state = t.state + 1.0
    assert t.update(state=new_state) is t and t.version == 1 and np.array_equal(t.state, new_state) and t.state is not new_state
    with pytest.raises(ValueError):
        t.update(model=[1, 2])  # another column count without the other arrays
    assert t.version == 1 and t.model.shape == (4,)  # a refused update changes nothing
    with pytest.raises(ValueError):
        t.update(poly=np.zeros((4, 3, 2)))
    t.update(model=[2, 2], state=np.zeros((2, 6)), dims=np.ones((2, 2)))
    assert t.version == 2 and len(t.model) == 2
    t.freeze()
    with pytest.raises(ValueError):
        t.state[0, 0] = 1.0
    t.update(state=np.ones((2, 6)))  # replaces the frozen array
    t.state[0, 0] = 2.0
    assert t.version == 3
    ring = np.array([[[1, 1], [-1, 1], [-1, -1.5], [1, -1]]], dtype=float)
    p = ObstacleTracks(model=[2], state=np.zeros((1, 6)), dims=[[2, 3]], poly=ring, nvert=[4])
    assert p.nvert.dtype == np.int32 and p.poly.shape == (1, 4, 2)


# ---------------------------------------------------------------------------------------------------------------- the binding
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "fiss_plus_planner_amd", "csrc"), "-s"])
    return _abi.load()


def test_header_and_binding_agree(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "frenet_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+fp_obstacles_predict\s*\(", code) and "fp_obstacles_predict" in _abi.EXPORTED_SYMBOLS
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "frenet_gpu.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(fp_tracks));']
    for fname, _ in _abi.FpTracks._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(fp_tracks, {fname}));')
    lines += ['  printf("consts %d %d %d\\n", FP_TRACK_NONE, FP_TRACK_LANE, FP_TRACK_ARC);', '  printf("version %d\\n", FP_ABI_VERSION);', '  return 0;', '}']
    src = tmp_path / "tracks.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "tracks"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = {l.split()[0]: l.split()[1:] for l in subprocess.check_output([str(exe)], text=True).splitlines()}
    assert int(got["size"][0]) == C.sizeof(_abi.FpTracks) and int(got["version"][0]) == 18 == _abi.FP_ABI_VERSION
    for fname, _ in _abi.FpTracks._fields_:
        assert int(got[fname][0]) == getattr(_abi.FpTracks, fname).offset, fname
    assert [int(v) for v in got["consts"]] == [_abi.FP_TRACK_NONE, _abi.FP_TRACK_LANE, _abi.FP_TRACK_ARC] == [TRACK_NONE, TRACK_LANE, TRACK_ARC] == [R.NONE, R.LANE, R.ARC]


def test_library_exports_the_symbol_and_checks_arguments_first(lib):
    assert hasattr(lib, "fp_obstacles_predict") and lib.fp_abi_version() == 18
    assert lib.fp_obstacles_predict(None, None, None, None, None, None, _abi.FP_MEM_HOST, None) == -1
    assert b"ctx is NULL" in lib.fp_last_error()


def test_without_a_gpu_every_new_entry_point_fails_like_the_others():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from fiss_plus_planner_amd.engine import FrenetEngine
    from fiss_plus_planner_amd.planners import FrenetOptimalPlanner, FrenetOptimalPlannerSettings
    from fiss_plus_planner_amd.vehicle import Vehicle

    with pytest.raises(_abi.FrenetGpuError):
        FrenetEngine(0)  # predict_obstacles / predict_obstacles_device live on an engine: there is none to call them on
    t = _tracks()
    with pytest.raises(_abi.FrenetGpuError):
        t.table(FrenetEngine(0), np.arange(5.0), np.zeros((8, 5)), 0.1, 10)
    with pytest.raises(_abi.FrenetGpuError):  # the planner classes open their engine when they are built, tracks or no tracks
        FrenetOptimalPlanner(FrenetOptimalPlannerSettings(), Vehicle())
    assert isinstance(ObstacleTable(np.zeros((2, 1, 4)), np.ones((1, 2)), 2), ObstacleTable)
