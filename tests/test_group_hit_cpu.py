"""CPU: every case of tests/group_hit_cases.py is what its name says - proved with the oracle and the numpy restatement of the kernel's
group circle (tools/group_hit_estimate.py) alone, no kernel:

  * which end-speed groups the kernel's circle and the tight circle of the true fan ends finish, per case kind, and that no finished
    group has a candidate the oracle keeps free;
  * the boundary cases: with a real candidate of every group passing the box by delta - 1e-6 the circle is silent, and at the early
    row it is NOT silent with thr + 0.05 - the case would catch that mistake on the flag word;
  * the boundary ALONG the line (straight and on the bend): the rearmost candidate of the slowest group is free in the oracle and the
    kernel's circle is silent, while a circle of HALF the radius ends the group for the egos the test names - that mistake shows on
    the candidate's flag word; a short horizon in the MIDDLE of t_samples: a stage that judged a group from its first and last
    horizon alone would end groups whose short profiles the oracle keeps free;
  * no candidate of any case, in any shape, stands within 1e-6 m of contact with an obstacle at a compared row (the boundary candidates
    pass by delta - 1e-6 >= 9e-6 or overlap by 1e-6 - delta >= 1.1e-5: there is no exception to list);
  * a line of 12 m radius (the tightest bend the generator draws is gentler): all nt x nd candidate centres of every group at every
    checked row lie inside the kernel's circle, by brute force over the oracle's dumps - the curvature and normal-turning bound."""
import numpy as np
import pytest

import group_hit_cases as C

G, E, S = C.G, C.G.E, C.S
SHAPE_NAMES = list(C.SHAPES)


@pytest.fixture(scope="module")
def ended(oracle):
    out = {}
    for shape in SHAPE_NAMES:
        for name in C.CASES:
            batch, kind = C.build(name, shape)
            out[shape, name] = (batch, kind, [C.ended_groups(batch, b) for b in range(batch.B)])
    return out


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("name", list(C.CASES))
def test_case_is_what_it_says(ended, shape, name):
    batch, kind, sets = ended[shape, name]
    everyone = set(range(batch.nv))
    for b, (kern, tight, coll) in enumerate(sets):
        assert kern <= coll and tight <= coll, f"{name} [{shape}] ego {b}: a finished group has a free candidate"
        if kind == "all":
            assert kern == everyone and coll == everyone, (name, shape, b, kern)
        elif kind == "silent":
            assert not kern and not tight, (name, shape, b, kern, tight)
    if kind == "some" and shape == SHAPE_NAMES[0]:
        n_kern, n_free = sum(len(k) for k, _, _ in sets), sum(batch.nv - len(k) for k, _, _ in sets)
        assert n_kern > 0 and n_free > 0, (name, shape, n_kern, n_free)


@pytest.mark.parametrize("slow", [True, False])
def test_speed_split_ends_the_groups_the_box_covers(ended, slow):
    """The tight circle ends groups at the covered end of the end speeds (a neighbour of the covered half within thr of the box
    included); the far end - metres beyond the box - is free, and what lies between is blocked through S, B and N."""
    batch, _, sets = ended[SHAPE_NAMES[0], "a box the slow end speeds reach" if slow else "a box the fast end speeds reach"]
    for b, (kern, tight, coll) in enumerate(sets):
        order = [int(i) for i in np.argsort(batch.v_samples[b])]
        far = set(order[-2:] if slow else order[:2])  # the two end speeds farthest from the box
        assert tight and not (tight & far) and not (coll & far), (b, tight, coll, far)
        assert coll - kern, f"ego {b}: no blocked group is left to S, B and N"
        assert len(coll) < batch.nv, f"ego {b}: no group stays free"


@pytest.mark.parametrize("delta", [1e-3, 1e-5])
def test_boundary_outside_is_silent_and_would_catch_a_wrong_threshold(oracle, delta):
    """The outermost candidate of every group is free in the oracle and inside the kernel's circle, which is silent; a threshold of
    thr + 0.05 would end the group - a mistake that shows on that candidate's flag word."""
    batch, _ = C.build(f"boundary at an early row: passes by {'1e-3' if delta == 1e-3 else '1e-5'}", SHAPE_NAMES[0])
    k_box = C.K_NEAR
    thr = E.threshold(batch)
    for b in range(batch.B):
        prob = oracle.problems_from_batch(batch, [b])[0]
        coll = ((prob.fop_plan().flags & 4) != 0).reshape(batch.nd, batch.nt, batch.nv)
        at_end = int(np.argmax(batch.d_samples) if b % 2 == 0 else np.argmin(batch.d_samples))
        sc = int(batch.scene_of[b])
        for iv in range(batch.nv):
            k, s, d, xy = G.group_rows(batch, b, prob, iv)
            r = int(np.nonzero(k == k_box)[0][0])
            assert not coll[at_end, :, iv].any(), (b, iv)
            pose = batch.obs_pose[sc, k[r:r + 1] + int(batch.t_now[b])]
            centre, rad = G.kernel_circle(batch, b, s[:, r], d[:, :, r])
            dist = float(E.box_distance(centre[None], pose, batch.obs_dims[sc])[0, 0])
            ends = np.array([E.box_distance(xy[it, w, r][None], pose, batch.obs_dims[sc])[0, 0] for it in range(batch.nt) for w in range(2)])
            assert abs(ends.max() - (thr + delta)) < 1e-9, (b, iv, ends.max() - thr)
            assert dist + rad > thr, "the kernel's circle is silent"
            assert dist + rad <= thr + 0.05, "thr + 0.05 would fire: the case catches it"


def test_tight_bend_every_centre_lies_inside_the_kernels_circle(oracle):
    batch, _ = C.build("a tight bend", SHAPE_NAMES[0])
    d_all = [float(x) for x in batch.d_samples]
    lo, hi = int(np.argmin(batch.d_samples)), int(np.argmax(batch.d_samples))
    worst = 0.0
    for b in (0, 5):
        prob = oracle.problems_from_batch(batch, [b])[0]
        for iv in range(batch.nv):
            k, s, d, xy = G.group_rows(batch, b, prob, iv, d_all)
            assert len(k) >= 20
            for r in range(len(k)):
                circ = G.kernel_circle(batch, b, s[:, r], d[:, [lo, hi], r])
                if circ is None:  # (g - A2 hs <= 0: the kernel is silent there)
                    continue
                far = float(np.hypot(*(xy[:, :, r].reshape(-1, 2) - circ[0]).T).max())
                assert far <= circ[1], (b, iv, int(k[r]), far, circ[1])
                worst = max(worst, far / circ[1])
    assert worst > 0.3, "the bound is not vacuous: some centre uses a third of its circle"


@pytest.mark.parametrize("bend", [False, True])
@pytest.mark.parametrize("delta", [1e-3, 1e-5])
def test_boundary_along_the_line_is_silent_and_would_catch_half_the_radius(oracle, delta, bend):
    name = f"boundary along {'the bend' if bend else 'a straight line'}: the rearmost candidate passes by {'1e-3' if delta == 1e-3 else '1e-5'}"
    batch, _ = C.build(name, SHAPE_NAMES[0])
    k_box = C.K_BEND if bend else C.K_AHEAD
    thr = E.threshold(batch)
    i_d = int(np.argmin(batch.d_samples))
    caught = []
    for b in range(batch.B):
        iv, it, d_end, _ = C.ahead_target(batch, b, k_box)
        prob = oracle.problems_from_batch(batch, [b])[0]
        coll = ((prob.fop_plan().flags & 4) != 0).reshape(batch.nd, batch.nt, batch.nv)
        assert d_end == batch.d_samples[i_d] and not coll[i_d, it, iv], f"ego {b}: the rearmost candidate is free"
        assert coll[:, :, iv].sum() >= coll[:, :, iv].size - batch.nt, f"ego {b}: the rest of the group collides (the other horizons of the same lateral sample may pass)"
        k, s, d, xy = G.group_rows(batch, b, prob, iv)
        r = int(np.nonzero(k == k_box)[0][0])
        sc = int(batch.scene_of[b])
        pose = batch.obs_pose[sc, k[r:r + 1] + int(batch.t_now[b])]
        # the candidate's centre is rho + delta - 1e-6 from the face: thr + delta, to the rounding of thr's own 1e-9 rho
        gap = float(E.box_distance(xy[it, 0, r][None], pose, batch.obs_dims[sc])[0, 0])
        assert abs(gap - (0.5 * C.SQUARE + delta - 1e-6)) < 1e-9, (b, gap)
        centre, rad = G.kernel_circle(batch, b, s[:, r], d[:, :, r])
        dist = float(E.box_distance(centre[None], pose, batch.obs_dims[sc])[0, 0])
        assert dist + rad > thr, f"ego {b}: the kernel's circle is silent"
        if dist + 0.5 * rad <= thr:
            caught.append(b)
    assert len(caught) >= 2, f"half the radius ends the group of egos {caught}: fewer than two"


def test_just_inside_the_circle_fires_with_1e_5_to_spare(oracle):
    batch, _ = C.build("the slowest group's circle inside thr by 1e-5", SHAPE_NAMES[0])
    for b in range(batch.B):
        prob = oracle.problems_from_batch(batch, [b])[0]
        iv = int(np.argmin(batch.v_samples[b]))
        k, kern, _ = G.group_table(batch, b, prob, iv)
        r = int(np.nonzero(k == C.K_AHEAD)[0][0])
        assert abs(kern[r, 0] + 1e-5) < 1e-9, (b, kern[r, 0])  # dist + rad - thr = -1e-5 at the box's step
        assert not (kern[:r] <= 0).any(), f"ego {b}: no earlier row ends the group"
        coll = ((prob.fop_plan().flags & 4) != 0).reshape(batch.nd, batch.nt, batch.nv)
        assert coll[:, :, iv].all()


def test_short_middle_horizon_would_catch_a_group_judged_from_its_first_and_last_horizon(oracle):
    import adversarial as A

    batch, _ = C.build("a short horizon among long ones", SHAPE_NAMES[0])
    mid = batch.nt // 2
    assert batch.t_samples[mid] == 1.0 and batch.t_samples[0] > 1.3 and batch.t_samples[-1] > 1.3
    ends_only = A._copy(batch, t_samples=batch.t_samples[[0, batch.nt - 1]].copy())
    fired = 0
    for b in range(batch.B):
        prob = oracle.problems_from_batch(batch, [b])[0]
        coll = ((prob.fop_plan().flags & 4) != 0).reshape(batch.nd, batch.nt, batch.nv)
        assert not coll[:, mid, :].any(), f"ego {b}: the short profiles have no pose at the box's step and stay free"
        fired += sum(1 for g in G.ego_groups(ends_only, b) if g[2] >= 0)
    assert fired >= batch.B, "judged from the first and the last horizon alone, groups would end on the box"


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("name", list(C.CASES))
def test_no_candidate_within_a_micrometre_of_contact(oracle, shape, name):
    """What the GPU file compares is decided by the stages, not by rounding: no ego box of any candidate is within 1e-6 m of contact with
    an obstacle at a checked row.  The candidates placed at a boundary on purpose pass by delta - 1e-6 >= 9e-6 m or overlap by
    1e-6 - delta >= 1.1e-5 m, so they are not exceptions either."""
    batch, _ = C.build(name, shape)
    for b in range(batch.B):
        near = C.near_contacts(batch, b)
        assert not near, f"{name} [{shape}] ego {b}: (id, it, iv, k, obstacle) within 1e-6 m of contact: {near[:5]}"
