"""GPU: the walk's per-profile shortcuts (csrc/frenet_lattice_fused.hip, "WALK"), each on the inputs at which it switches.

* item codes   the shaped instances pack a survivor as row << bits | obstacle (item_shift, frenet_lattice_plan.h); the run-time-shape
               instances keep the table index row * n_obs + obstacle and take it apart by division.  Both, at obstacle counts around the
               powers of two, with check strides 1, 2, 3, a single checked row and the most rows strides 2 and 3 allow (with as
               many obstacles as the 16-bit table index then holds).  item_shift itself - 25 x 50 -> 6 bits, 50 x 10 -> 4, a code that
               leaves 16 bits -> 0, one obstacle -> 0 - is checked where it is defined (static_asserts in frenet_lattice_plan.h): no
               compiled-in shape overflows, so no launch can take that branch.  (Stride 1 at the most rows is tests/test_gpu_edges.py's
               test_row_obstacle_pairs_16bit.  The compiled-in maximum of 4095 obstacles cannot reach the walk at all: such a scene does
               not fit the fused kernel's LDS and goes to the lane-per-candidate kernel, which is what test_obstacle_count there shows;
               762 is the largest count exercised on the walk.)
* last point   a pose on its profile's LAST point takes the previous step's heading.  Only a profile whose reference line ends inside
               the checked rows can have one: those take the compare and the selects, the others do not - lines that end after 2, 3,
               an even and an odd number of points, an obstacle standing on the line's end, and in the same launch (and the same
               wavefront's share of the profiles) lines that do not end.
* segment hint one step from the bucket's hint when every knot spacing exceeds a bucket (lut_segment_step), the loops otherwise:
               uniform lines, lines with several knots inside one bucket, the ego exactly on a knot and exactly on a bucket edge, and
               arclengths so large (1e10 m) that the spacing margin no longer covers their rounding: those take the loops too.

Every case runs through the two-, three- and four-per-CU instances (tests/lattice_paths.py's MODES: "resident_groups" 2 models
a one-CU device, so a dozen egos take them; asserted through the launch counters) and is compared with the oracle: flag words, Stats and
the selected index exact, cost within 1e-9."""
import numpy as np
import pytest

import math

import adversarial as A
import lattice_paths as L
from fiss_plus_planner_amd import synth
from fiss_plus_planner_amd.engine import make_params
from fiss_plus_planner_amd.spline import build_frames

pytestmark = pytest.mark.gpu


def check(oracle, engine, batch, what, modes=L.MODES):
    return L.through_modes(oracle, engine, batch, what, modes, winner=False)


# ---------------------------------------------------------------- item codes
@pytest.mark.parametrize("shape", ["997", "555"])
def test_packed_item_codes_of_the_shaped_instances(oracle, engine, shape):
    """BASELINE's two compiled-in shapes: 25 rows x 50 obstacles (6 bits of obstacle) and 50 rows x 10 obstacles (4 bits)."""
    batch = (synth.make_batch(12, 9, 9, 7, 50, 50, True, 8101, layout="survey8d") if shape == "997" else
             synth.make_batch(12, 5, 5, 5, 10, 100, True, 8102))
    L.shaped_case(oracle, engine, batch, f"shaped {shape}", L.SHAPE_997 if shape == "997" else L.SHAPE_555, L.modes_for(batch, tail=False))


@pytest.mark.parametrize("n_obs,stride", [(1, 2), (31, 1), (32, 2), (33, 3), (63, 1), (64, 2), (65, 3)])
def test_item_codes_around_the_powers_of_two(oracle, engine, n_obs, stride):
    base = synth.make_batch(8, 5, 4, 3, n_obs, 40, True, 8200 + n_obs, layout="survey8d")
    batch = A._copy(base, check_stride=stride)
    ref = check(oracle, engine, batch, f"{n_obs} obstacles, stride {stride}")
    if n_obs > 1:
        assert L.colliding(ref) > 0


@pytest.mark.parametrize("stride", [1, 2, 3])
def test_a_single_checked_row(oracle, engine, stride):
    """final_time_step = 1: the collision horizon is the first pose row alone (row 0 decides everything there is to decide)."""
    base = synth.make_batch(8, 5, 4, 3, 33, 40, True, 8300 + stride, layout="survey8d")
    pose = base.obs_pose.copy()
    for b in range(base.B):  # half of the obstacles onto the ego's own position, so that row 0 has something to say
        f = int(base.frame_of[b])
        px, py, yaw = synth.sample_frames(base.knots[f:f + 1], base.coef[f:f + 1], np.array([[base.ego[b, 0] + 1.0]]))
        pose[int(base.scene_of[b]), :, ::2, 0], pose[int(base.scene_of[b]), :, ::2, 1], pose[int(base.scene_of[b]), :, ::2, 2] = px[0, 0], py[0, 0], yaw[0, 0]
    batch = A._copy(base, check_stride=stride, obs_pose=pose, final_time_step=np.full(len(base.final_time_step), 1, dtype=np.int32))
    ref = check(oracle, engine, batch, f"one row, stride {stride}")
    assert L.colliding(ref) > 0


@pytest.mark.parametrize("stride", [2, 3])
def test_the_most_rows_a_stride_allows(oracle, engine, stride):
    """256 points per trajectory and a 256-step pose table: 128 rows at stride 2, 86 at stride 3, with 511 / 762 obstacles - the row x
    obstacle table within a row of its 65535 entries.  One ego, a layout of ~100 KB: two per CU and the lane-per-candidate kernel."""
    from test_gpu_edges import _scene, horizon

    rows_want = math.ceil(256 / stride)
    n_obs = 65535 // rows_want
    batch = _scene(1, n_obs, 256, 8350 + stride, stride=stride, Ts=[horizon(200), horizon(256)])
    assert make_params(batch).points_max == 256 and L.rows_of(batch) == rows_want and 65535 - rows_want < rows_want * n_obs <= 65535
    ref = check(oracle, engine, batch, f"{rows_want} rows x {n_obs} obstacles, stride {stride}", L.EDGE_MODES)
    assert L.colliding(ref) > 0


# ---------------------------------------------------------------- last point
@pytest.mark.parametrize("shaped,stride", [(True, 2), (False, 1), (False, 2)])
def test_an_obstacle_on_the_last_point_of_a_line_that_ends_early(oracle, engine, shaped, stride):
    """Egos 2, 3, 6, 7, 21 and ~44 points before the end of their reference line (every other ego stays where it was: its profiles do not
    end early), an obstacle across the end of the line: the truncated trajectories' last existing pose is inside it.  The last of them
    is placed so that its fast profiles leave the line inside the checked rows and its slow ones behind them: one workgroup, and every
    wavefront's share of its profiles (dealt round-robin over the end speeds), walks profiles of both kinds."""
    base = (synth.make_batch(12, 9, 9, 7, 50, 50, True, 8401, layout="survey8d") if shaped else
            synth.make_batch(12, 5, 6, 3, 12, 40, True, 8402, layout="survey8d"))
    ego, pose, dims = base.ego.copy(), base.obs_pose.copy(), base.obs_dims.copy()
    points = [2, 3, 6, 7, 21, 44]  # points on the line: the ego covers ~ s_d * tick per point in its first seconds, whatever the profile
    for b in range(0, base.B, 2):
        f, sc = int(base.frame_of[b]), int(base.scene_of[b])
        k_last = float(base.knots[f, int(base.nx[f]) - 1])
        ego[b, 2] = 0.0
        ego[b, 0] = k_last - (points[(b // 2) % len(points)] - 0.5) * ego[b, 1] * base.tick_t
        px, py, yaw = synth.sample_frames(base.knots[f:f + 1], base.coef[f:f + 1], np.array([[k_last - 0.5]]))
        pose[sc, :, 0, 0], pose[sc, :, 0, 1], pose[sc, :, 0, 2], pose[sc, :, 0, 3] = px[0, 0], py[0, 0], yaw[0, 0], 1.0
        dims[sc, 0] = (3.0, 6.0)  # across the road
    batch = A._copy(base, ego=ego, obs_pose=pose, obs_dims=dims, check_stride=stride)
    ref = check(oracle, engine, batch, f"line ends early ({'shaped' if shaped else 'run-time shape'}, stride {stride})")
    flags = np.concatenate([r.flags for r in ref])
    M, N, coll = flags >> 20, (flags >> 8) & 0xFFF, (flags & 4) != 0
    assert (M == 2).any() and (M == 3).any() and ((M > 3) & (M < N) & (M % 2 == 0)).any() and ((M > 3) & (M < N) & (M % 2 == 1)).any() and (M == N).any()
    assert (coll & (M >= 2) & (M < N)).any() and (~coll & (M == N)).any()
    if shaped:
        L.assert_compiled_in_shape(batch, L.SHAPE_997)
    k_last = (L.rows_of(batch) - 1) * batch.check_stride  # a profile with M <= k_last + 1 can have a checked pose on its last point
    mixed = [e for e, r in enumerate(ref) if ((r.flags >> 20 >= 2) & (r.flags >> 20 <= k_last + 1)).any() and (r.flags >> 20 > k_last + 1).any()]
    assert mixed, "no ego whose profiles end both inside and behind the checked rows"
    for e in mixed:  # ... spread over the end speeds, so that each of the 8 wavefronts (profile pq = slice * nv + end speed, dealt pq % 8) gets both
        Me = (ref[e].flags >> 20).reshape(batch.nd, batch.nt, batch.nv)[0]  # [slice][end speed] (flat index = (id * nt + it) * nv + iv)
        early = (Me <= k_last + 1).ravel()
        shares = [early[w::8] for w in range(min(8, early.size))]
        if any(s.any() and not s.all() for s in shares):
            break
    else:
        raise AssertionError("no wavefront's share of an ego's profiles holds both kinds")


# ---------------------------------------------------------------- segment hint
def _with_knots_at(base, xs_of):
    """`base` on reference lines through the same road, sampled at xs_of(b) instead of every 5 m (the obstacles stay where they are)."""
    pts = np.empty((base.B, base.NX, 2))
    for b in range(base.B):
        f = int(base.frame_of[b])
        xs = xs_of(b)
        s = np.interp(xs, base.coef[f, 0, :int(base.nx[f])], base.knots[f, :int(base.nx[f])])
        px, py, _ = synth.sample_frames(base.knots[f:f + 1], base.coef[f:f + 1], s[None])
        pts[b, :, 0], pts[b, :, 1] = px[0], py[0]
    knots, coef = build_frames(pts)
    return A._copy(base, knots=knots, coef=coef, frame_of=np.arange(base.B))


@pytest.mark.parametrize("shaped", [True, False])
@pytest.mark.parametrize("knots", ["uniform", "clustered", "mixed"])
def test_segment_hint_on_uniform_and_on_crowded_knots(oracle, engine, shaped, knots):
    """uniform: every spacing is 2 nx / (nx - 1) buckets, one step; clustered: runs of knots 0.4 m apart inside one ~2.5 m bucket, the
    loops; mixed: every other ego of the launch the one, the others the other (the flag is per ego).  Four egos stand exactly on a knot,
    four exactly on a bucket edge.  (The run-time-shape instances take the loops on every line: there this is their regression test.)"""
    base = (synth.make_batch(12, 9, 9, 7, 50, 50, True, 8501, layout="survey8d") if shaped else
            synth.make_batch(12, 5, 6, 3, 12, 40, True, 8502, layout="survey8d"))
    if shaped:
        L.assert_compiled_in_shape(base, L.SHAPE_997)
    NX = base.NX
    uniform = np.linspace(0.0, 400.0, NX)
    rng = np.random.default_rng(8503)
    clustered = np.sort(np.concatenate([np.linspace(0.0, 400.0, NX - 30), (rng.uniform(20.0, 140.0, 6)[:, None] + 0.4 * np.arange(1, 6)[None, :]).ravel()]))
    assert np.diff(clustered).min() > 1e-3
    batch = _with_knots_at(base, lambda b: uniform if knots == "uniform" or (knots == "mixed" and b % 2) else clustered)
    ego = batch.ego.copy()
    for b in range(8):
        f = int(batch.frame_of[b])
        nx = int(batch.nx[f])
        k0, k1 = float(batch.knots[f, 0]), float(batch.knots[f, nx - 1])
        if b < 4:
            ego[b, 0] = batch.knots[f, np.searchsorted(batch.knots[f, :nx], ego[b, 0])]  # exactly a knot
        else:
            w = (k1 - k0) / (2 * nx)
            ego[b, 0] = k0 + float(np.ceil((ego[b, 0] - k0) / w)) * w  # exactly a bucket's first arclength, as the kernel forms it
    batch = A._copy(batch, ego=ego)
    w_b = (batch.knots[:, -1] - batch.knots[:, 0]) / (2 * NX)
    crowded = (np.diff(batch.knots, axis=1) < w_b[:, None]).any(axis=1)
    assert crowded.all() == (knots == "clustered") and crowded.any() == (knots != "uniform")
    ref = check(oracle, engine, batch, f"{knots} knots ({'shaped' if shaped else 'run-time shape'})")
    assert 0 < L.colliding(ref) < batch.B * batch.C


@pytest.mark.parametrize("shaped", [True, False])
def test_segment_hint_far_from_the_arclength_origin(oracle, engine, shaped):
    """Every other ego's line starts at arclength 1e10 m (knots and the ego's s0 moved together; uniform spacing, so only the
    |knot| 2^-50 guard of s_cnt[4] sends them to the loops - the roundings of (s - knot0) / width and of a bucket's start, 2e-6 m here,
    exceed the 1e-6 of a 2.5 m bucket the one-step lookup allows for).  The others stay at the origin and take one step."""
    base = (synth.make_batch(12, 9, 9, 7, 50, 50, True, 8601, layout="survey8d") if shaped else
            synth.make_batch(12, 5, 6, 3, 12, 40, True, 8602, layout="survey8d"))
    if shaped:
        L.assert_compiled_in_shape(base, L.SHAPE_997)
    knots, ego = base.knots.copy(), base.ego.copy()
    far = np.arange(base.B) % 2 == 0
    knots[base.frame_of[far]] += 1e10
    ego[far, 0] += 1e10
    batch = A._copy(base, knots=knots, ego=ego)
    w_b = (batch.knots[:, -1] - batch.knots[:, 0]) / (2 * batch.NX)
    assert (np.abs(batch.knots[base.frame_of[far]]).max(axis=1) * 2.0 ** -50 > 1e-6 * w_b[base.frame_of[far]]).all()
    assert (np.abs(batch.knots[base.frame_of[~far]]).max(axis=1) * 2.0 ** -50 < 1e-6 * w_b[base.frame_of[~far]]).all()
    ref = check(oracle, engine, batch, f"arclength offset 1e10 ({'shaped' if shaped else 'run-time shape'})")
    assert any(((r.flags & 4) != 0).any() for r, f in zip(ref, far) if f) and 0 < L.colliding(ref) < batch.B * batch.C
