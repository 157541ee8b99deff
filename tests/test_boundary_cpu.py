"""CPU: the road-boundary check (fp_boundary_mask) without a GPU - the reference restatement (tests/boundary_ref.py) on a case with a
closed form and on every batch the GPU tests use (the caps on undecided candidates, asserted on the reference alone), the header
against the binding, the corridor of the demo scenarios, ProblemBatch.take / shard / digest, and the loud failure without a device."""
import ctypes as C
import glob
import lzma
import os
import re
import subprocess

import numpy as np
import pytest

import boundary_ref as R
from conftest import GOLDEN, ROOT
from fiss_plus_planner_amd import _abi, synth
from fiss_plus_planner_amd.batch import ProblemBatch

# the smallest lane half-width (distance of a bound vertex from its centre vertex) on the five demo scenarios: DEU_Lohmar-15_1_T-1
MIN_HALF_WIDTH = 1.7339573


def straight_batch(d0, left, right, margin):
    """One ego on a straight 200 m line, d_d = d_dd = 0 and one lateral sample equal to d0: d is constant, h = veh_w / 2."""
    pts = np.zeros((1, 41, 2))
    pts[0, :, 0] = np.linspace(0.0, 200.0, 41)
    knots, coef = synth.build_frames(pts)
    return ProblemBatch(d_samples=[d0], t_samples=[8.0, 10.0], v_samples=[[3.0, 6.0]], target_speed=[6.0], ego=[[10.0, 5.0, 0.0, d0, 0.0, 0.0]],
                        frame_of=[0], scene_of=[-1], t_now=[0], nx=[41], knots=knots, coef=coef, obs_pose=np.zeros((0, 1, 0, 4)), obs_dims=np.zeros((0, 0, 2)),
                        final_time_step=np.zeros(0, dtype=np.int32), veh_l=4.5, veh_w=1.8, max_speed=30.0, max_accel=10.0,
                        bound_left=np.full((1, 41), left), bound_right=np.full((1, 41), right), bound_margin=margin)


@pytest.mark.parametrize("side", ["left", "right"])
def test_reference_on_a_closed_form(oracle, side):
    """d constant and the heading along the line: the verdict is d0 + w/2 + margin > L (d0 - w/2 - margin < R) exactly."""
    d0, margin, w = (0.3, 0.05, 1.8) if side == "left" else (-0.2, 0.1, 1.8)
    edge = d0 + w / 2 + margin if side == "left" else d0 - w / 2 - margin
    for eps, want in ((1e-6, False), (-1e-6, True)):  # the edge 1 um outside / inside the footprint's reach
        e = edge + eps if side == "left" else edge - eps
        b = straight_batch(d0, e if side == "left" else 50.0, -50.0 if side == "left" else e, margin)
        r = R.ego_mask(oracle, b, 0)
        assert r.bit.tolist() == [want] * b.C, (side, eps, r.bit)
        assert np.allclose(r.hi, d0 + w / 2, atol=1e-12) and np.allclose(r.lo, d0 - w / 2, atol=1e-12)
        assert np.allclose(r.slack, 1e-6, rtol=1e-3)
        assert r.n_masked == (b.C if want else 0) and (r.best_idx >= 0) == (not want)
        assert np.array_equal(r.flags & ~np.uint32(R.FLAG_BOUNDARY), r.flags_in) and not (r.flags_in & R.FLAG_BOUNDARY).any()


@pytest.mark.parametrize("name", list(R.CASES))
def test_caps_hold_on_every_gpu_batch(oracle, name):
    """At most 0.5 % of a batch's candidates within 1e-9 m of an edge, at most one ego excluded for having one."""
    batch, refs = R.case(oracle, name)
    R.check_caps(refs, name)
    assert len(refs) == batch.B


def test_gpu_batches_mask_some_and_not_all(oracle):
    """A batch where all or none are masked tests nothing.  The issue's corridor against the default 1.84 m vehicle masks 93 % of the
    base batch at the best of 40 000 seeds (see boundary_ref.SEED): at least three egos keep a survivor there, and the 10 % .. 90 %
    window is asserted on its widened twin, which every GPU test runs on as well."""
    _, base = R.case(oracle, "base")
    assert sum(r.best_idx >= 0 for r in base) >= 3
    share = sum(r.n_masked for r in base) / sum(len(r.bit) for r in base)
    assert 0.10 <= share < 1.0, share
    for name in ("wide", "tick005_wide", "line_ends", "unbounded", "obstacles", "chunks", "unstaged"):
        batch, refs = R.case(oracle, name)
        share = sum(r.n_masked for r in refs) / sum(len(r.bit) for r in refs)
        assert 0.10 <= share <= 0.90, (name, share)
        assert sum(r.best_idx >= 0 for r in refs) >= min(3, batch.B), name
    # the shapes the cases exist for
    N = lambda refs: np.concatenate([(r.flags_in >> 8) & 0xFFF for r in refs])   # noqa: E731
    M = lambda refs: np.concatenate([r.flags_in >> 20 for r in refs])            # noqa: E731
    assert 64 < N(base).min() and N(base).max() <= 128                           # two lane rounds
    assert N(R.case(oracle, "tick005")[1]).max() == 200                          # four
    ends = R.case(oracle, "line_ends")[1]
    assert ((M(ends) < N(ends)) & (M(ends) > 1)).any() and (M(ends[3:4]) <= 1).all() and not ends[3].bit.any()
    unb, (bb, _) = R.case(oracle, "unbounded")[1], R.case(oracle, "unbounded")
    assert np.isinf(bb.bound_left[:, 20:41]).all() and np.isinf(bb.bound_right).all() and any(r.bit.any() for r in unb)


def _header():
    return open(os.path.join(ROOT, "include", "frenet_gpu.h")).read()


def test_header_and_binding_agree(tmp_path):
    hdr = _header()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+fp_boundary_mask\s*\(", code) and "fp_boundary_mask" in _abi.EXPORTED_SYMBOLS
    assert int(re.search(r"#define FP_FLAG_BOUNDARY (\d+)u", hdr).group(1)) == 128 == _abi.FLAG_BOUNDARY
    infeasible = re.search(r"#define FP_FLAG_INFEASIBLE \((.*?)\)", hdr).group(1)
    assert "FP_FLAG_BOUNDARY" in infeasible and _abi.FLAG_INFEASIBLE & _abi.FLAG_BOUNDARY
    assert _abi.FLAG_INFEASIBLE == R.FLAG_INFEASIBLE
    assert "WITHIN ABI 18" in hdr and "looking the symbol up" in hdr
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "frenet_gpu.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(fp_corridor));']
    for fname, _ in _abi.FpCorridor._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(fp_corridor, {fname}));')
    lines += ['  printf("infeasible %u\\n", FP_FLAG_INFEASIBLE);', '  printf("version %d\\n", FP_ABI_VERSION);', '  return 0;', '}']
    src = tmp_path / "corridor.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "corridor"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_abi.FpCorridor)
    for fname, _ in _abi.FpCorridor._fields_:
        assert int(got[fname]) == getattr(_abi.FpCorridor, fname).offset, fname
    assert int(got["infeasible"]) == _abi.FLAG_INFEASIBLE and int(got["version"]) == 18


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "fiss_plus_planner_amd", "csrc"), "-s"])
    return _abi.load()


def test_library_exports_the_symbol_within_abi_18(lib):
    assert hasattr(lib, "fp_boundary_mask") and lib.fp_abi_version() == 18


def test_null_ctx_fails_loudly(lib):
    """No GPU needed: the argument checks come first."""
    assert lib.fp_boundary_mask(None, None, None, None, None, None, None, None, None, _abi.FP_MEM_HOST, None) == -1
    assert b"ctx is NULL" in lib.fp_last_error()


def test_demo_scenarios_carry_their_corridor(tmp_path):
    from fiss_plus_planner_amd.commonroad_xml import load_scenario

    files = sorted(glob.glob(os.path.join(GOLDEN, "demo", "*.xml.xz")))
    assert len(files) == 5
    smallest = np.inf
    for f in files:
        xml = tmp_path / os.path.basename(f)[:-3]
        xml.write_bytes(lzma.open(f).read())
        sc = load_scenario(str(xml))
        cor = sc.corridor
        assert cor.shape == (len(sc.centerline), 2), f
        assert (cor[:, 0] > 0).all() and (cor[:, 1] < 0).all(), f
        assert (cor[:, 0] - cor[:, 1] >= 2 * MIN_HALF_WIDTH).all(), f
        smallest = min(smallest, cor[:, 0].min(), -cor[:, 1].max())
    assert MIN_HALF_WIDTH <= smallest < MIN_HALF_WIDTH + 1e-6  # (the recorded value IS the smallest one seen)


def test_take_and_shard_keep_the_corridor_rows():
    b = R.base_batch()
    sub = b.take([3, 1])
    assert np.array_equal(sub.bound_left[sub.frame_of], b.bound_left[[3, 1]]) and np.array_equal(sub.bound_right[sub.frame_of], b.bound_right[[3, 1]])
    assert np.array_equal(sub.knots[sub.frame_of], b.knots[[3, 1]]) and sub.bound_margin == b.bound_margin
    sh = b.shard(1, 2)
    assert sh.B == 3 and np.array_equal(sh.bound_left[sh.frame_of], b.bound_left[2:5]) and np.array_equal(sh.bound_right[sh.frame_of], b.bound_right[2:5])
    plain = synth.make_batch(5, 5, 4, 3, 0, 20, False, R.SEED)
    assert plain.take([0]).bound_left is None and plain.shard(0, 2).bound_right is None
    kw = {k: getattr(plain, k) for k in ("d_samples", "t_samples", "v_samples", "target_speed", "ego", "frame_of", "scene_of", "t_now", "nx",
                                          "knots", "coef", "obs_pose", "obs_dims", "final_time_step", "veh_l", "veh_w", "max_speed", "max_accel")}
    with pytest.raises(AssertionError):  # shapes are [F, NX]
        ProblemBatch(**kw, bound_left=np.ones((5, 80)), bound_right=-np.ones((5, 80)))
    with pytest.raises(AssertionError):  # the two sides come together
        ProblemBatch(**{k: getattr(plain, k) for k in ("d_samples", "t_samples", "v_samples", "target_speed", "ego", "frame_of", "scene_of", "t_now", "nx",
                                                         "knots", "coef", "obs_pose", "obs_dims", "final_time_step", "veh_l", "veh_w", "max_speed", "max_accel")},
                     bound_left=np.ones((5, 81)))


def test_a_batch_without_a_corridor_keeps_its_digest():
    """Pinned on the commit before the corridor fields existed."""
    plain = synth.make_batch(5, 5, 4, 3, 0, 20, False, R.SEED)
    assert plain.bound_left is None and plain.bound_right is None and plain.bound_margin == 0.0
    assert plain.digest() == "48c26a8ddc9898b2a4dcadda741a0e6d07287e10d0a8bb7f63f8f6bdefc926e1"
    assert R.base_batch().digest() != plain.digest()


def test_planner_classes_accept_or_refuse_a_boundary():
    """No GPU: set_road_boundary only records (FOP) or raises (the planners that order candidates before validation)."""
    from fiss_plus_planner_amd import planners as P

    class NoEngine:
        pass

    veh = synth.Vehicle()
    fop = P.FrenetOptimalPlanner(P.FrenetOptimalPlannerSettings(), veh, engine=NoEngine())
    fop.set_road_boundary([1.5, 1.5], [-1.5, -np.inf], 0.1)
    assert fop._boundary[2] == 0.1
    fop.set_road_boundary(None, None)
    assert fop._boundary is None
    for bad in (([1.0, np.nan], [-1.0, -1.0], 0.0), ([1.0], [-1.0, -1.0], 0.0), ([1.0], [-1.0], -1.0), ([1.0], [-1.0], np.inf)):
        with pytest.raises(ValueError):
            fop.set_road_boundary(*bad)
    for cls, st in ((P.FopPlusPlanner, P.FrenetOptimalPlannerSettings()), (P.FissPlanner, P.FissPlannerSettings()), (P.FissPlusPlanner, P.FissPlusPlannerSettings())):
        with pytest.raises(ValueError):
            cls(st, veh, engine=NoEngine()).set_road_boundary([1.0], [-1.0])
