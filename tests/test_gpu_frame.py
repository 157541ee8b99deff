"""GPU: Frenet frame construction (fp_frames_build) and Cartesian->Frenet projection (fp_from_state) against the
reference goldens (G2 spline coefficients, G7 from_state) and the oracle on ragged batches."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import load_golden
from fiss_plus_planner_amd import _abi

import frame_ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["flens", "sinus"])
def test_frames_build_matches_reference(engine, name):
    g = load_golden("g2_spline.npz")
    pts = g[f"{name}_pts"]
    knots, coef = engine.build_frames(pts[None])
    np.testing.assert_allclose(knots[0], g[f"{name}_knots"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(coef[0], g[f"{name}_coef"], rtol=1e-9, atol=1e-11)


def test_frames_build_ragged_batch_vs_oracle(oracle, engine):
    rng = np.random.default_rng(5)
    F, NX = 9, 96
    n = rng.integers(3, NX + 1, F).astype(np.int32)
    n[0], n[1] = 2, NX
    pts = np.zeros((F, NX, 2))
    for f in range(F):
        x = np.cumsum(rng.uniform(0.5, 9.0, n[f]))
        pts[f, : n[f], 0] = x
        pts[f, : n[f], 1] = rng.uniform(0, 6) * np.sin(x / rng.uniform(20, 70)) + rng.uniform(-50, 50)
    knots, coef = engine.build_frames(pts, n)
    for f in range(F):
        k, cx, cy = oracle.spline2d_build(pts[f, : n[f], 0], pts[f, : n[f], 1])
        np.testing.assert_allclose(knots[f, : n[f]], k, rtol=0, atol=1e-10)
        assert np.isinf(knots[f, n[f]:]).all()
        np.testing.assert_allclose(coef[f, 0:4, : n[f]], cx, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(coef[f, 4:8, : n[f]], cy, rtol=1e-8, atol=1e-10)
        assert (coef[f, :, n[f]:] == 0).all()


def test_from_state_matches_reference(engine):
    g5 = load_golden("g5_closed_loop.npz")
    g7 = load_golden("g7_from_state.npz")
    knots, coef = engine.build_frames(g5["centerline"][None])
    n = np.array([len(g5["centerline"])], dtype=np.int32)
    B = len(g7["poses"])
    ego = engine.from_state(knots, coef, n, np.zeros(B, dtype=np.int32), g7["poses"])
    np.testing.assert_allclose(ego, g7["frenet"], rtol=0, atol=1e-8)
    # the planning problem's initial state (SURVEY 8d config 1 anchor)
    np.testing.assert_allclose(ego[0, [0, 3, 1, 4]], [51.5936, 0.3687, 14.6660, -0.1639], atol=5e-4)


# ---------------------------------------------------------------------------------------------------------------------------------
# fp_from_state against tests/frame_ref.py (the reference's resampling + the oracle's from_state), under frame_ref's comparison rules
def _report(name, r):
    print(f"{name}: {r.n} poses, undecidable {r.undecidable * r.n:.0f}, max err s {r.err_s:.2e} s_d {r.err_sd:.2e} d {r.err_d:.2e} d_d {r.err_dd:.2e}")


@pytest.fixture(scope="module")
def ragged(engine):
    """F = 7 rotated, shifted lines of 2 .. 96 knots (tables built on the GPU), frame 4 referenced by nobody; 200 random poses and the
    two clamp poses per referenced frame, shuffled."""
    pts, n = frame_ref.ragged_frames()
    knots, coef = engine.build_frames(pts, n)
    used = [f for f in range(len(n)) if f != 4]
    fo, poses = frame_ref.random_poses(knots, coef, n, used)
    fc, pc = frame_ref.clamp_poses(knots, coef, n, used)
    fo, poses = np.concatenate([fo, fc]), np.concatenate([poses, pc])
    perm = np.random.default_rng(13).permutation(len(fo))
    return SimpleNamespace(pts=pts, n=n, knots=knots, coef=coef, frame_of=fo[perm], poses=poses[perm])


@pytest.fixture(scope="module")
def ragged_ref(oracle, ragged):
    return frame_ref.reference_rows(oracle, ragged.knots, ragged.coef, ragged.n, ragged.frame_of, ragged.poses)


def test_from_state_ragged_multi_frame_batch(engine, ragged, ragged_ref):
    r = ragged
    ref, dec, _ = ragged_ref
    assert r.n[0] == 2 and r.n[1] == r.knots.shape[1] == 96 and len(set(r.n.tolist())) > 3 and 4 not in r.frame_of
    assert (np.diff(r.frame_of) < 0).any() and len(np.unique(r.frame_of)) == 6  # shuffled, several frames
    assert (frame_ref.point_count_margin(r.knots, r.n) >= 1e-3).all()  # kernel and reference agree on the point counts
    ahead = np.array([d.angle <= math.pi / 2 for d in dec])
    assert 0.2 < ahead.mean() < 0.8  # both sides of pi/2
    assert any(d.raw_next < 1 for d in dec) and any(d.raw_next >= d.n for d in dec)  # both clamps
    got = engine.from_state(r.knots, r.coef, r.n, r.frame_of, r.poses)
    _report("ragged batch", frame_ref.assert_projection(got, ref, dec, what="ragged batch"))


def test_from_state_line_shorter_than_the_workgroup(oracle, engine):
    """A two-knot line of 0.25 m: 3 resampled points for 256 threads, every pose within one step of both clamps."""
    pts = frame_ref.rotate_shift(np.array([[0.0, 0.0], [0.25, 0.0]]), 0.7, (120.0, -45.0))
    knots, coef = engine.build_frames(pts[None])
    n = np.array([2], dtype=np.int32)
    fo, poses = frame_ref.random_poses(knots, coef, n, [0], per_frame=60, seed=14)
    fc, pc = frame_ref.clamp_poses(knots, coef, n, [0])
    fo, poses = np.concatenate([fo, fc]), np.concatenate([poses, pc])
    ref, dec, pls = frame_ref.reference_rows(oracle, knots, coef, n, fo, poses)
    assert len(pls[0]) == 3
    assert {d.nearest for d in dec} == {0, 1, 2} and any(d.raw_next < 1 for d in dec) and any(d.raw_next >= 3 for d in dec)
    got = engine.from_state(knots, coef, n, fo, poses)
    _report("0.25 m line", frame_ref.assert_projection(got, ref, dec, what="0.25 m line"))


@pytest.fixture(scope="module")
def straight(engine):
    """The line through (0,0), (1,0) .. (64,0): tables exactly b = 1, c = d = 0, y = 0, resampled points exactly x = i * 0.1."""
    pts = np.column_stack([np.arange(65.0), np.zeros(65)])
    knots, coef = engine.build_frames(pts[None])
    assert (knots[0] == np.arange(65.0)).all() and (coef[0, 0] == np.arange(65.0)).all()
    assert (coef[0, 1, :64] == 1).all() and (coef[0, 2:] == 0).all() and coef[0, 1, 64] == 0
    pl = frame_ref.resample(knots[0], coef[0])
    assert len(pl) == 640 and (pl[:, 0] == np.arange(640) * 0.1).all() and (pl[:, 1:] == 0).all()
    return knots, coef, pl


def test_from_state_exact_ties_resolve_to_the_first_minimum(oracle, engine, straight):
    """Poses exactly equidistant from two resampled points: np.argmin takes the first.  With yaw = pi the two choices give s values
    0.2 m apart (the nearest point lies ahead of the ego for one, behind it for the other).  Ties at 63 | 64 cross a wavefront boundary,
    at 255 | 256 the wrap of the thread stride, at 10 | 11 stay inside a wavefront."""
    knots, coef, pl = straight
    x = pl[:, 0]
    mid = (x[:-1] + x[1:]) / 2
    ties = [i for i in range(639) if mid[i] - x[i] == x[i + 1] - mid[i] and math.hypot(x[i] - mid[i], 1.5) == math.hypot(x[i + 1] - mid[i], 1.5)]
    assert len(ties) == 213 and {10, 63, 191, 255} <= set(ties)
    poses = np.array([[mid[i], 1.5, math.pi, 4.0] for i in ties] + [[x[100], 0.0, math.pi, 4.0]])  # the last one ON a point: dd == 0
    fo, n = np.zeros(len(poses), dtype=np.int32), np.array([65], dtype=np.int32)
    ref = np.stack([frame_ref.project(oracle, pl, p) for p in poses])
    for k, i in enumerate(ties):  # the reference itself: first minimum, and what the other choice would have cost
        assert frame_ref.decide(pl, poses[k]).nearest == i and frame_ref.decide(pl, poses[k]).gap == 0.0
        lo = frame_ref.project(oracle, pl, poses[k] - [1e-6, 0, 0, 0])[0]
        hi = frame_ref.project(oracle, pl, poses[k] + [1e-6, 0, 0, 0])[0]
        assert ref[k, 0] == lo and abs(hi - lo - (0.2 if 0 < i < 638 else 0.1)) < 1e-9, (i, lo, hi)  # (0.1 where a clamp holds one choice back)
    got = engine.from_state(knots, coef, n, fo, poses)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-8)  # every tie: the first minimum won (the other one is 0.2 m away)
    # Bit for bit where the kernel's summation tree is exact: up to prev = 256 every thread holds ONE segment length and the tree adds
    # aligned blocks of 2^k neighbours, whose sums x[a + 2^k] - x[a] are representable; beyond it a thread adds lengths 25.6 m apart
    # and rounds (25 of the 213 ties differ from the sequential sum in the last bit, on any machine).
    exact = [k for k, i in enumerate(ties) if i <= 256] + [len(ties)]
    assert {10, 63, 191, 255} <= {ties[k] for k in exact[:-1]}
    assert (got[exact][:, [0, 3]] == ref[exact][:, [0, 3]]).all(), np.abs(got[exact] - ref[exact]).max(axis=0)
    assert got[-1, 0] == x[100] and got[-1, 3] == 0
    print(f"exact ties: {len(ties)} ties, {len(exact) - 1} compared bit for bit, max err s {np.abs(got - ref)[:, 0].max():.2e}")


def _device_batch(torch, dev, r, frame_of):
    t = SimpleNamespace(n=torch.from_numpy(r.n).to(dev), fo=torch.from_numpy(np.ascontiguousarray(frame_of, dtype=np.int32)).to(dev))
    fb = _abi.FpBatch()
    fb.B, fb.F, fb.NX = len(frame_of), r.knots.shape[0], r.knots.shape[1]
    return t, fb


def test_frames_and_projection_on_the_device_path(engine, ragged):
    """FP_MEM_DEVICE: the ragged batch's frames built on the device, the egos projected from those tables without a host round trip
    (torch tensors, one stream) - bit-equal to the FP_MEM_HOST calls."""
    import torch

    r = ragged
    dev = torch.device("cuda", 0)
    F, NX = r.knots.shape
    t, fb = _device_batch(torch, dev, r, r.frame_of)
    pts = torch.from_numpy(r.pts).to(dev)
    knots = torch.full((F, NX), 7.0, dtype=torch.float64, device=dev)
    coef = torch.full((F, 8, NX), 7.0, dtype=torch.float64, device=dev)
    states = torch.from_numpy(r.poses).to(dev)
    ego = torch.full((len(r.poses), 6), 7.0, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n0 = engine.get_option("from_state_launches")
    engine.build_frames_device(F, NX, t.n.data_ptr(), pts.data_ptr(), knots.data_ptr(), coef.data_ptr(), stream)
    fb.frame_of, fb.nx, fb.knots, fb.coef = t.fo.data_ptr(), t.n.data_ptr(), knots.data_ptr(), coef.data_ptr()
    engine.from_state_device(fb, states.data_ptr(), ego.data_ptr(), stream)
    torch.cuda.synchronize(dev)
    assert engine.get_option("from_state_launches") == n0 + 1
    assert np.array_equal(knots.cpu().numpy(), r.knots) and np.array_equal(coef.cpu().numpy(), r.coef)
    assert np.array_equal(ego.cpu().numpy(), engine.from_state(r.knots, r.coef, r.n, r.frame_of, r.poses))


def test_from_state_refusals_and_nan_rows(engine, ragged):
    """FP_MEM_HOST names what it cannot project and launches nothing; FP_MEM_DEVICE answers such an ego with a NaN row and leaves the
    others alone.  (NaN only: the infinite yaw is proven on the CPU, tests/test_project_cpu.py, and never sent to a GPU kernel - the host
    path refuses it before any launch.)"""
    import torch

    r = ragged
    sel = np.nonzero(r.frame_of == 1)[0][:8]
    fo, poses = r.frame_of[sel], r.poses[sel]
    n0 = engine.get_option("from_state_launches")
    for k, col, val, text in ((3, 0, math.nan, r"ego 3: x=-?nan is not finite"), (5, 2, math.inf, r"ego 5: yaw=inf is not finite"), (0, 3, math.nan, r"ego 0: v=-?nan is not finite")):
        bad = poses.copy()
        bad[k, col] = val
        with pytest.raises(_abi.FrenetGpuError, match=text) as ei:
            engine.from_state(r.knots, r.coef, r.n, fo, bad)
        assert ei.value.code == -1  # FP_EINVAL
    # a 0.05 m line: one resampled point
    pts = r.pts.copy()
    pts[4, :2] = [[10.0, 10.0], [10.03, 10.04]]
    n = r.n.copy()
    n[4] = 2
    knots, coef = engine.build_frames(pts, n)
    assert abs(knots[4, 1] - 0.05) < 1e-12
    fo4 = fo.copy()
    fo4[6] = 4
    with pytest.raises(_abi.FrenetGpuError, match=r"ego 6 sits on frame 4, whose line of length 0\.05 has fewer than two resampled points") as ei:
        engine.from_state(knots, coef, n, fo4, poses)
    assert ei.value.code == -1  # FP_EINVAL
    assert engine.get_option("from_state_launches") == n0  # nothing was launched
    good = engine.from_state(knots, coef, n, fo, poses)      # the same line, referenced by nobody: accepted
    assert engine.get_option("from_state_launches") == n0 + 1
    assert np.array_equal(good, engine.from_state(r.knots, r.coef, r.n, fo, poses))
    # device path: egos 2 (NaN x) and 5 (NaN yaw) among valid ones, all on frame 1
    dev = torch.device("cuda", 0)
    bad = poses.copy()
    bad[2, 0] = math.nan
    bad[5, 2] = math.nan
    t, fb = _device_batch(torch, dev, r, fo)
    kd, cd = torch.from_numpy(r.knots).to(dev), torch.from_numpy(r.coef).to(dev)
    fb.frame_of, fb.nx, fb.knots, fb.coef = t.fo.data_ptr(), t.n.data_ptr(), kd.data_ptr(), cd.data_ptr()
    states = torch.from_numpy(bad).to(dev)
    ego = torch.full((len(bad), 6), 7.0, dtype=torch.float64, device=dev)
    engine.from_state_device(fb, states.data_ptr(), ego.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    got = ego.cpu().numpy()
    assert np.isnan(got[[2, 5]]).all()
    keep = [0, 1, 3, 4, 6, 7]
    assert np.array_equal(got[keep], good[keep])


# ---------------------------------------------------------------------------------------------------------------------------------
# fp_frames_build
KNOT_ATOL, COEF_RTOL, COEF_ATOL = 1e-10, 1e-8, 1e-10  # the tolerances of test_frames_build_ragged_batch_vs_oracle


def _assert_tables(oracle, pts, n, knots, coef, what=""):
    worst = np.zeros(2)
    for f in range(len(n)):
        k, cx, cy = oracle.spline2d_build(pts[f, : n[f], 0], pts[f, : n[f], 1])
        want = np.concatenate([cx, cy])
        np.testing.assert_allclose(knots[f, : n[f]], k, rtol=0, atol=KNOT_ATOL, err_msg=f"{what} frame {f}")
        np.testing.assert_allclose(coef[f, :, : n[f]], want, rtol=COEF_RTOL, atol=COEF_ATOL, err_msg=f"{what} frame {f}")
        assert np.isinf(knots[f, n[f]:]).all() and (knots[f, n[f]:] > 0).all() and (coef[f, :, n[f]:] == 0).all(), (what, f)
        worst = np.maximum(worst, [np.abs(knots[f, : n[f]] - k).max(), (np.abs(coef[f, :, : n[f]] - want) / (COEF_ATOL + COEF_RTOL * np.abs(want))).max()])
    return worst


def _spline_residuals(knots, coef):
    """What any correct natural spline satisfies, from ONE frame's tables alone (used rows), in np.longdouble: the segment i polynomial
    ends on vertex i + 1, first and second derivatives continuous at the interior knots.  -> the largest residual of each kind."""
    L = np.longdouble
    h = np.diff(knots.astype(L))
    res = np.zeros(3)
    for ax in (0, 4):
        a, b, c, d = (coef[ax + k].astype(L) for k in range(4))
        end = a[:-1] + b[:-1] * h + c[:-1] * h ** 2 + d[:-1] * h ** 3
        d1 = b[:-1] + 2 * c[:-1] * h + 3 * d[:-1] * h ** 2
        d2 = 2 * c[:-1] + 6 * d[:-1] * h
        res[0] = max(res[0], float(np.abs(end - a[1:]).max()))
        if len(a) > 2:
            res[1] = max(res[1], float(np.abs(d1[:-1] - b[1:-1]).max()))
        res[2] = max(res[2], float(np.abs(d2 - 2 * c[1:]).max()))
    return res


def _geometry_lines():
    """frame_ref.ragged_frames with offsets up to +-5000 m; frame 0: n = 2, 2: n = 3, 3: knot steps alternating 0.05 m and 5 m,
    5: collinear."""
    pts, n = frame_ref.ragged_frames(seed=21, shift=5000.0)
    rng = np.random.default_rng(22)
    n[2] = 3
    pts[2, 3:] = 0
    n[3] = 80
    x = np.cumsum(np.tile([0.05, 5.0], 40))
    pts[3] = 0
    pts[3, :80] = frame_ref.rotate_shift(np.column_stack([x, 3.0 * np.sin(x / 40.0)]), rng.uniform(-3, 3), rng.uniform(-5000, 5000, 2))
    t = np.cumsum(rng.uniform(0.5, 3.0, n[5]))
    pts[5] = 0
    pts[5, : n[5]] = frame_ref.rotate_shift(np.column_stack([t, np.zeros_like(t)]), rng.uniform(-3, 3), rng.uniform(-5000, 5000, 2))
    return pts, n


def test_frames_build_geometry(oracle, engine):
    pts, n = _geometry_lines()
    assert n[0] == 2 and n[2] == 3 and np.abs(pts).max() > 2000
    knots, coef = engine.build_frames(pts, n)
    worst = _assert_tables(oracle, pts, n, knots, coef, "geometry")
    got, ref = np.zeros(3), np.zeros(3)
    for f in range(len(n)):
        assert (coef[f, 0, : n[f]] == pts[f, : n[f], 0]).all() and (coef[f, 4, : n[f]] == pts[f, : n[f], 1]).all()  # through every vertex
        assert coef[f, 2, 0] == 0 and coef[f, 2, n[f] - 1] == 0 and coef[f, 6, 0] == 0 and coef[f, 6, n[f] - 1] == 0  # natural ends
        k, cx, cy = oracle.spline2d_build(pts[f, : n[f], 0], pts[f, : n[f], 1])
        got = np.maximum(got, _spline_residuals(knots[f, : n[f]], coef[f, :, : n[f]]))
        ref = np.maximum(ref, _spline_residuals(k, np.concatenate([cx, cy])))
    print(f"geometry: knots max err {worst[0]:.2e}, coef max err / tolerance {worst[1]:.2e}; residuals (end point, 1st, 2nd derivative) "
          f"kernel {got} oracle {ref}")
    # two correct solvers of the same tridiagonal system differ by a few units of its conditioning: x 4 on the oracle's own residuals
    assert (got <= 4 * ref).all(), (got, ref)


@pytest.mark.parametrize("NX,n", [(2, 2), (127, 127), (128, 128), (129, 129), (129, 128)])
def test_frames_build_either_side_of_the_thread_stride(oracle, engine, NX, n):
    """128 threads: NX below, at and above the stride (a second trip of every strided loop), and n one short of NX."""
    rng = np.random.default_rng(100 + NX + n)
    F = 3
    pts = np.zeros((F, NX, 2))
    for f in range(F):
        x = np.cumsum(rng.uniform(0.5, 3.0, n))
        pts[f, :n] = frame_ref.rotate_shift(np.column_stack([x, rng.uniform(0, 6) * np.sin(x / rng.uniform(20, 70))]), rng.uniform(-3, 3), rng.uniform(-500, 500, 2))
    nn = np.full(F, n, dtype=np.int32)
    knots, coef = engine.build_frames(pts, nn)
    worst = _assert_tables(oracle, pts, nn, knots, coef, f"NX={NX} n={n}")
    print(f"NX={NX} n={n}: knots max err {worst[0]:.2e}, coef max err / tolerance {worst[1]:.2e}")


def test_frames_build_ignores_the_rows_beyond_n(engine, ragged):
    """Rows >= n[f] of `points` hold NaN and 1e300 instead of zeros: the same tables bit for bit, +inf / 0 padding."""
    r = ragged
    dirty = r.pts.copy()
    for f in range(len(r.n)):
        dirty[f, r.n[f]:, 0] = np.nan
        dirty[f, r.n[f]:, 1] = 1e300
    knots, coef = engine.build_frames(dirty, r.n)
    assert np.array_equal(knots, r.knots) and np.array_equal(coef, r.coef)
    for f in range(len(r.n)):
        assert (knots[f, r.n[f]:] == np.inf).all() and (coef[f, :, r.n[f]:] == 0).all() and np.isfinite(coef[f, :, : r.n[f]]).all()
