"""Case factories and CPU proofs for the kernel paths of the obstacle-clearance term (clearance_rescore_kernel) that the config-2 /
config-3 cases of tests/test_clearance_cpu.py never take: more than one chunk of 1024 candidates, obstacle rows read from the scene
table instead of LDS, t_now > 0, frames of different knot counts in one launch, the broad-phase skip and a 220-knot line.

Every case names the egos that are compared with the restatement (tests/clearance_ref.py) - two to four, because the restatement
walks survivors in Python - and carries a proof, run on the CPU by tests/test_clearance_cpu.py::test_path_cases_recorded, that
  1. every compared ego is decidable: R.margin > 1e-6, so "best_idx exact" is a fair demand at a 1e-9 cost bar;
  2. the batch really reaches the path the case is named after (asserted from the batch alone, the LDS budget by restating
     ego_lds_bytes / lds_layout_doubles of csrc/frenet_ego.h) and the term matters there (moved winners, survivors with clearance).
reference(oracle, name) computes the restatement once per process; the GPU tests and the CPU proofs share it and leave it unchanged."""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np

import clearance_ref as R
from fiss_plus_planner_amd import synth

W = 100.0              # = test_clearance_cpu.W_TEST (the weight at which the term moves winners, see there)
CHUNK = 1024           # kClearThreads: candidates per pass of the kernel's chunk loop
LDS_BUDGET = 144 * 1024  # bytes launch_clearance_rescore hands ego_lds_bytes
POINTS_CAP = 128       # points_cap() at tick_t = 0.1 (FP_FAST_POINTS)
CLEAR_SKIP = 48.0      # kClearSkip


# ---------------------------------------------------------------------------
# csrc/frenet_ego.h restated: what the launch reserves and what stage_ego decides per ego
# ---------------------------------------------------------------------------
def launch_lds_doubles(batch):
    """(doubles of dynamic LDS the launch reserves, True when that includes the obstacle rows): ego_lds_bytes."""
    assert batch.tick_t == 0.1
    cs = int(batch.check_stride)
    rows = min(-(-POINTS_CAP // cs), -(-batch.T_obs // cs))
    base = batch.NX * 9 + batch.n_obs * 4
    full = base + rows * batch.n_obs * 4
    return (full, True) if full * 8 <= LDS_BUDGET else (base, False)


def ego_rows(batch, e):
    """Rows of its scene's table that stage_ego would stage for ego e."""
    cs, sc, t_now = int(batch.check_stride), int(batch.scene_of[e]), int(batch.t_now[e])
    hmax = max(min(int(batch.final_time_step[sc]) - t_now, POINTS_CAP), 0)
    in_table = batch.T_obs - t_now
    return min(-(-hmax // cs), -(-in_table // cs) if in_table > 0 else 0)


def ego_staged(batch, e):
    """True when ego e's obstacle rows are in LDS during the launch of `batch` (lds_layout_doubles <= the launch's doubles)."""
    n = batch.n_obs
    return int(batch.nx[batch.frame_of[e]]) * 9 + n * 4 + ego_rows(batch, e) * n * 4 <= launch_lds_doubles(batch)[0]


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
def weighted(batch, w=W):
    batch.w_obstacle = w
    return batch


def _chunks(nd, nv, nt, seed):
    return lambda: weighted(synth.make_batch(8, nd, nv, nt, 10, 100, True, seed))


def _silence(batch, alive):
    """Every obstacle column outside `alive` without a state at any step (its poses stay in the table: a reader that ignores the
    validity word sums them)."""
    dead = np.setdiff1d(np.arange(batch.n_obs), alive)
    batch.obs_pose[:, :, dead, 3] = 0.0
    return batch


def scene_table_100():
    """100 obstacles x 100 rows at check_stride 1: 320 KB of rows, read from the scene table.  Some rows without a state and one
    obstacle whose prediction ends early, as in test_check_stride_invalid_rows_and_no_scene."""
    b = synth.make_batch(6, 5, 5, 5, 100, 100, True, 104)
    b.check_stride = 1
    b.obs_pose[:, 7::9, ::2, 3] = 0.0
    b.obs_pose[:, 30:, 1, 3] = 0.0
    return weighted(b)


def staged_40(pad=0):
    """40 obstacles x 100 rows at check_stride 1 are staged (125 KB of rows); padded with 30 rows in which no column is valid, beyond
    final_time_step and never looked at, the same table is past the budget and is read in place (the margins suite's device)."""
    b = synth.make_batch(5, 5, 5, 5, 40, 100, True, 4008)
    b.check_stride = 1
    b.obs_pose[:, 5::11, 1::3, 3] = 0.0
    if pad:
        b.obs_pose = np.ascontiguousarray(np.concatenate([b.obs_pose, np.zeros((b.S, pad, b.n_obs, 4))], axis=1))
    return weighted(b)


# per-ego (t_now, final_time_step) of the t_now cases; T_obs is 100 (rows in LDS) or 128 (rows from the table)
T_NOW = {
    0: (60, 99),    # 0 < final_time_step - t_now = 39 < M: the horizon cuts the poses
    1: (50, 150),   # final_time_step > T_obs and t_now + i runs past the table: rows beyond it hold no state
    2: (99, 99),    # final_time_step - t_now = 0: no pose at all
    3: (7, 99),     # odd t_now at check_stride 2: row i / stride, time step i + t_now
    4: (120, 99),   # final_time_step - t_now < 0
}
T_NOW_ALIVE = np.r_[0:2, 11:23]  # the columns that keep their states in the 72-column scenes (2 in the ego's lane, 12 beside it)


def t_now_lds(t_zero=False):
    b = synth.make_batch(5, 5, 5, 5, 10, 100, True, 111)
    for e, (t, fts) in T_NOW.items():
        b.t_now[e], b.final_time_step[e] = (0 if t_zero else t), fts
    return weighted(b)


def t_now_table(t_zero=False):
    """72 columns x 64 rows (T_obs 128 at check_stride 2) are 18432 doubles: past the budget with the spline beside them.  58 of the
    columns never have a state, so that the restatement stays cheap and the scene keeps survivors."""
    b = _silence(synth.make_batch(5, 5, 5, 5, 72, 128, True, 111), T_NOW_ALIVE)
    for e, (t, fts) in T_NOW.items():
        b.t_now[e], b.final_time_step[e] = (0 if t_zero else t), fts
    return weighted(b)


MIXED_ALIVE = np.r_[9:24]  # (beside the lane: the static columns in it would leave the egos at t_now 0 no survivor)


def mixed_knots():
    """Egos 0, 1 on 400-knot lines, egos 2 .. 4 on 81-knot lines, 60 static obstacle columns x 128 rows at check_stride 2.  NX = 400
    sizes the launch: 3600 + 240 + 64 * 240 doubles are past the budget, so it reserves 3840 doubles and no rows.  The short lines
    need 729 + 240: egos 3 and 4 (t_now 110 / 113 of final_time_step 127: 9 and 7 rows of 240 doubles) stage their rows in what the
    long lines' knots leave free, ego 2 (t_now 0, 64 rows) cannot and reads the table like egos 0 and 1."""
    long_ = synth.make_batch(2, 5, 5, 5, 60, 128, False, 733, n_knots=400)
    short = synth.make_batch(5, 5, 5, 5, 60, 128, False, 733)
    F, NX = 5, 400
    knots, coef = np.full((F, NX), np.inf), np.zeros((F, 8, NX))
    knots[:2], coef[:2] = long_.knots, long_.coef
    knots[2:, :81], coef[2:, :, :81] = short.knots[2:], short.coef[2:]
    b = dataclasses.replace(short, knots=knots, coef=coef, nx=np.array([400, 400, 81, 81, 81], dtype=np.int32))
    b.obs_pose[:2], b.obs_dims[:2] = long_.obs_pose, long_.obs_dims  # (drawn alike; sampled on their own lines)
    b.t_now[3], b.t_now[4] = 110, 113
    return weighted(_silence(b, MIXED_ALIVE))


def alone(batch, e):
    """Ego e of `batch` as a batch of its own, its line no wider than its own knots (so NX is what the ego needs, not what the widest
    line of the batch it came from needed)."""
    sub = batch.take([e])
    n = int(sub.nx.max())
    return dataclasses.replace(sub, knots=sub.knots[:, :n], coef=sub.coef[:, :, :n])


FAR_MOVED = (2, 4, 5, 7, 8)  # columns of scene 0 moved away from the road; scene 1 has every column there


def _far_offsets(n, rng):
    """Lateral offsets of 40 .. 60 m, both signs: on both sides of r_e + r_obs + 48 for poses abreast, beyond it for all others."""
    return rng.uniform(40.0, 60.0, n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)


def broad_phase():
    """Scene 0: five of ten obstacles moved 40 .. 60 m to the side of where they stood; scene 1: all ten.  Scenes 2, 3 as drawn."""
    b = synth.make_batch(4, 5, 5, 5, 10, 100, True, 101)
    rng = np.random.default_rng(48)
    for sc, cols in ((0, FAR_MOVED), (1, tuple(range(10)))):
        off = _far_offsets(len(cols), rng)
        for j, d in zip(cols, off):
            yaw = b.obs_pose[sc, :, j, 2]
            b.obs_pose[sc, :, j, 0] -= d * np.sin(yaw)
            b.obs_pose[sc, :, j, 1] += d * np.cos(yaw)
    return weighted(b)


def short_table(n_knots=81):
    """Config 2 with a 50-row table: 25 staged rows leave the lattice pass's layout within a third / a quarter of a CU's LDS, which the
    three- and four-per-CU instances need (with config 2's own 100 rows a multi-round launch stays at two per CU); final_time_step 49
    cuts every candidate's poses.  On 220- / 400-knot lines the whole spline no longer fits that share beside the table, and a launch
    at four / three per CU is a windowed (WIN) one."""
    return weighted(synth.make_batch(24, 5, 5, 5, 10, 50, True, 101, n_knots=n_knots))


# The lattice launch underneath three of the cases, under the ctx options the GPU test sets: (options, launch counter that must move,
# row of tests/test_lattice_plan_cpu.py whose plan_lattice dump says which instance that launch is).  prove_lattice_row ties the
# batch to the row's numbers.
LATTICE_UNDERNEATH = {
    "short table": [({"lattice_kernel": 2, "resident_groups": 2, "lattice_occupancy": 3}, "lattice_launches_3", "clearance_short_table_occ3"),
                    ({"lattice_kernel": 2, "resident_groups": 2}, "lattice_launches_4", "clearance_short_table")],
    "knots 220": [({"lattice_kernel": 2, "resident_groups": 2}, "lattice_launches_4", "clearance_knots220")],
    "knots 400": [({"lattice_kernel": 2, "resident_groups": 2, "lattice_occupancy": 3}, "lattice_launches_3", "clearance_knots400_occ3")],
}

@functools.lru_cache(maxsize=None)
def reference(oracle, name):
    """The restatement of a case, once per process: batch, egos, cost / flags / best_idx / best_cost over the egos, the winners
    without the weight and the survivors' {candidate: (clearance, poses, pairs)}."""
    make, egos = PATH_CASES[name][:2]
    batch = make()
    rows = [R.ego_table(oracle, batch, e, details=True) for e in egos]
    plain = np.array([R.ego_table(oracle, batch, e, 0.0)[2] for e in egos], dtype=np.int32)
    ref = SimpleNamespace(batch=batch, egos=list(egos), cost=np.stack([r[0] for r in rows]), flags=np.stack([r[1] for r in rows]),
                          idx=np.array([r[2] for r in rows], dtype=np.int32), best=np.array([r[3] for r in rows]), plain=plain,
                          info=[r[4] for r in rows])
    for a in (ref.cost, ref.flags, ref.idx, ref.best, ref.plain):
        a.setflags(write=False)
    return ref


def tables(ref):
    """The tuple check_against_restatement takes in place of its own R.batch_tables call."""
    return ref.cost, ref.flags, ref.idx, ref.best


def survivors(ref, k):
    return np.nonzero((ref.flags[k] & R.FLAG_INFEASIBLE) == 0)[0]


def record(ref):
    """The recorded numbers of a case (printed by the CPU test, quoted in EXPERIMENTS.md)."""
    per_chunk = [np.bincount(survivors(ref, k) // CHUNK, minlength=-(-ref.batch.C // CHUNK)).tolist() for k in range(len(ref.egos))]
    with_clear = [sum(1 for v in info.values() if v[0] > 0.0) for info in ref.info]
    poses = [sorted({v[1] for v in info.values()}) for info in ref.info]
    return dict(egos=ref.egos, plain=ref.plain.tolist(), winners=ref.idx.tolist(), moved=int(np.sum((ref.idx != ref.plain) & (ref.plain >= 0))),
                margin=[float(R.margin(ref.cost[k], ref.flags[k])) for k in range(len(ref.egos))], survivors_per_chunk=per_chunk,
                survivors_with_clearance=with_clear, pose_counts=[(p[0], p[-1]) if p else () for p in poses],
                staged=[bool(ego_staged(ref.batch, e)) for e in ref.egos], launch_has_rows=launch_lds_doubles(ref.batch)[1])


# ---------------------------------------------------------------------------
# the proofs: what each case must show on the CPU before the GPU is asked anything
# ---------------------------------------------------------------------------
def pose_total(ref, k, only=None):
    """Sum of the pose counts over ego k's survivors (only: restricted to these candidates)."""
    return sum(v[1] for c, v in ref.info[k].items() if only is None or c in only)


def far_pairs(oracle, ref, k, cols):
    """(pairs inside, pairs beyond) the broad phase's radius r_e + r_obs + kClearSkip among the checked poses of ego k's reference
    winner and the columns `cols` of its scene."""
    b, e = ref.batch, ref.egos[k]
    w = R.winner_series(oracle, b, e, int(ref.idx[k]))
    m = int(np.sum(~np.isnan(w[9])))
    i = np.arange(0, min(m, int(b.final_time_step[b.scene_of[e]]) - int(b.t_now[e])), int(b.check_stride))
    sc = int(b.scene_of[e])
    inside = beyond = 0
    for j in cols:
        rad = 0.5 * np.hypot(b.veh_l, b.veh_w) + 0.5 * np.hypot(*b.obs_dims[sc, j]) + CLEAR_SKIP
        d = np.hypot(b.obs_pose[sc, i, j, 0] - w[9, i], b.obs_pose[sc, i, j, 1] - w[10, i])
        inside, beyond = inside + int(np.sum(d < rad)), beyond + int(np.sum(d >= rad))
    return inside, beyond


def prove_lattice_row(batch, opts, row, family, per_cu):
    """The plan_lattice dump of tests/test_lattice_plan_cpu.py has a row for exactly this batch under exactly these options (a dense
    call with the weight: tables, a provisional argmin, the tail offered), and the row is a `family` instance at `per_cu` per CU -
    windowed ones with a window narrower than the line.  test_lattice_plans_match_the_table holds the row to plan_lattice itself."""
    import test_lattice_plan_cpu as P

    spec = dict(P.CASES)[row].split()
    want = {"B": batch.B, "res2": opts["resident_groups"], "nd": batch.nd, "nv": batch.nv, "nt": batch.nt, "obs": batch.n_obs, "T_obs": batch.T_obs,
            "NX": batch.NX, "tail": -(opts["resident_groups"] // 2)}
    if opts.get("lattice_occupancy"):
        want["occ"] = opts["lattice_occupancy"]
    if batch.NX == 81:
        del want["NX"]  # (the driver's default)
    assert {t.split("=")[0]: int(t.split("=")[1]) for t in spec if "=" in t} == want and {t for t in spec if "=" not in t} == {"tables", "parts"}
    assert batch.check_stride == 2 and batch.obs_nvert is None  # (the driver's stride; rectangle columns)
    line = [l for l in P.EXPECTED.strip().splitlines() if l.split()[0] == row][0].split()
    wcap = int([t for t in line if t.startswith("wcap=")][0][5:])
    assert line[1].split("/")[:2] == [family, str(per_cu)], line
    assert (wcap < batch.NX) == (family == "window") and (family != "window" or wcap >= 32)
    return " ".join(line[1:2] + [f"wcap={wcap}"])


def prove_chunks(oracle, ref, rec, name):
    b = ref.batch
    assert -(-b.C // CHUNK) == {"chunk 1024": 1, "chunk 1025": 2, "chunk 2197": 3}[name] and rec["launch_has_rows"] and all(rec["staged"])
    assert rec["moved"] >= 1 and sum(rec["survivors_with_clearance"]) >= 400
    if name == "chunk 1025":
        # The second chunk is the single candidate 1024 = (widest d, longest T, fastest v).  "Survivors in every chunk" therefore
        # needs an ego that keeps every candidate of the corner (here ego 1, all 1025 alive; ego 4 is the cheap companion whose
        # winner moves), and "a reference winner >= 1024" would need that corner to be the cheapest candidate, which no seed of the
        # generator gives: the demand for winners on both sides of 1024 is met by chunk 2197 below.  What must hold here is that the
        # second pass of the loop has work whose result the cost table shows: candidate 1024 alive, all its poses checked, a sum > 0.
        full = [k for k, pc in enumerate(rec["survivors_per_chunk"]) if min(pc) >= 1]
        assert full and all(ref.info[k][CHUNK][0] > 0.0 and ref.info[k][CHUNK][1] >= 40 for k in full)
    else:
        assert all(min(pc) >= 1 for pc in rec["survivors_per_chunk"])  # every compared ego has survivors in every chunk
    if name == "chunk 2197":
        assert (ref.idx >= CHUNK).any() and (ref.idx < CHUNK).any()
        assert (ref.idx // CHUNK != ref.plain // CHUNK).any()  # the weight moves a winner into another chunk


def prove_table_rows(oracle, ref, rec, name):
    b = ref.batch
    assert b.check_stride == 1 and not rec["launch_has_rows"] and not any(rec["staged"])
    assert (b.n_obs * 4 * min(POINTS_CAP, b.T_obs) + b.NX * 9 + b.n_obs * 4) * 8 > LDS_BUDGET
    assert (b.obs_pose[b.scene_of[ref.egos]][..., 3] == 0.0).any(axis=(1, 2)).all()  # rows without a state in every compared scene
    assert rec["moved"] >= 1 and min(rec["survivors_with_clearance"]) >= 20
    if name == "scene table":
        assert (b.obs_pose[:, 30:, 1, 3] == 0.0).all() and (b.obs_pose[:, :30, 1, 3] == 1.0).any()  # a prediction that ends early
    else:  # the padded table: the same batch without the padding is staged
        short = staged_40()
        assert launch_lds_doubles(short)[1] and all(ego_staged(short, e) for e in range(short.B))
        assert short.T_obs * 40 * 32 < LDS_BUDGET - 9 * 81 * 8 - 40 * 32 < LDS_BUDGET < 128 * 40 * 32 and b.T_obs == 130
        assert np.array_equal(b.obs_pose[:, :100], short.obs_pose) and (b.obs_pose[:, 100:] == 0.0).all()
        assert (b.final_time_step == 99).all()  # the padding lies beyond every horizon


def prove_t_now(oracle, ref, rec, name):
    b, table = ref.batch, name == "t_now table"
    assert b.check_stride == 2 and rec["launch_has_rows"] == (not table)
    zero = SimpleNamespace(batch=(t_now_table if table else t_now_lds)(True), egos=ref.egos)
    zero.info = [R.ego_table(oracle, zero.batch, e, details=True)[4] for e in ref.egos]
    rec["pose_counts_at_t_now_0"] = []
    kinds, with_poses = set(), 0
    for k, e in enumerate(ref.egos):
        t, fts = int(b.t_now[e]), int(b.final_time_step[b.scene_of[e]])
        assert (t, fts) == T_NOW[e] and t > 0
        assert ego_staged(b, e) == (not table or fts - t <= 0)  # (no rows at all fit any launch)
        M = ref.flags[k][survivors(ref, k)] >> 20
        both = set(ref.info[k]) & set(zero.info[k])
        assert len(both) >= 10 and pose_total(ref, k, both) != pose_total(zero, k, both)  # the offset changes the poses that are checked
        rec["pose_counts_at_t_now_0"].append((min(v[1] for v in zero.info[k].values()), max(v[1] for v in zero.info[k].values())))
        if 0 < fts - t < M.min():
            kinds.add("horizon cuts")
            assert all(v[1] == -(-(fts - t) // 2) for v in ref.info[k].values())
        if fts > b.T_obs and t + M.max() > b.T_obs:
            kinds.add("beyond the table")
            assert all(v[1] == -(-(b.T_obs - t) // 2) for v in ref.info[k].values())
        if fts - t <= 0:
            kinds.add("no pose")
            assert all(v == (0.0, 0, 0) for v in ref.info[k].values())
            assert np.array_equal(ref.cost[k], R.ego_table(oracle, b, e, 0.0)[0], equal_nan=True)
        else:  # the term at work: every survivor of an ego that has poses carries clearance, at least 50 of them per ego
            with_poses += 1
            assert rec["survivors_with_clearance"][k] == len(ref.info[k]) >= 50
        if t % 2 == 1:
            kinds.add("odd t_now")
    assert kinds == {"horizon cuts", "beyond the table", "no pose", "odd t_now"} and with_poses == 3 and rec["moved"] >= 1, kinds


def prove_mixed_knots(oracle, ref, rec, name):
    b = ref.batch
    full = b.NX * 9 + b.n_obs * 4 + 64 * b.n_obs * 4
    assert b.NX >= 200 and full * 8 > LDS_BUDGET and launch_lds_doubles(b) == (b.NX * 9 + b.n_obs * 4, False)
    assert b.nx[b.frame_of[ref.egos]].tolist() == [400, 81, 81, 81] and rec["staged"] == [False, False, True, True]
    for e in (3, 4):  # the short lines' rows fit what the long lines' knots leave free (alone, an 81-knot launch reserves all 64 rows)
        assert 0 < ego_rows(b, e) * b.n_obs * 4 <= (b.NX - 81) * 9 and launch_lds_doubles(alone(b, e))[1]
    assert ego_rows(b, 2) == 64 and rec["moved"] >= 1 and min(rec["survivors_with_clearance"]) >= 100


def prove_broad_phase(oracle, ref, rec, name):
    b = ref.batch
    near = [j for j in range(b.n_obs) if j not in FAR_MOVED]
    rec["far_pairs_inside_beyond"] = [far_pairs(oracle, ref, 0, FAR_MOVED), far_pairs(oracle, ref, 1, range(b.n_obs))]
    for inside, beyond in rec["far_pairs_inside_beyond"]:
        assert inside >= 10 and beyond >= 10
    assert far_pairs(oracle, ref, 0, near)[0] >= 100 and rec["moved"] >= 1
    # scene 1 holds far obstacles only: every pair is 30 m apart or more, a candidate's whole sum stays below 1e-12 and the plain winner wins
    assert ref.idx[1] == ref.plain[1] and 0.0 < max(v[0] for v in ref.info[1].values()) < 1e-12


def prove_short_table(oracle, ref, rec, name):
    b = ref.batch
    assert b.B == 24 and b.T_obs == 50 and (b.final_time_step == 49).all() and all(p == (25, 25) for p in rec["pose_counts"]) and rec["moved"] >= 2
    assert (b.nx == {"short table": 81, "knots 220": 220, "knots 400": 400}[name]).all()
    rec["lattice_underneath"] = [prove_lattice_row(b, opts, row, "plain" if name == "short table" else "window", int(counter[-1]))
                                 for opts, counter, row in LATTICE_UNDERNEATH[name]]


# name -> (factory, compared egos, proof of the case's own path)
PATH_CASES = {
    "chunk 1024": (_chunks(16, 8, 8, 311), (2, 6), prove_chunks),
    "chunk 1025": (_chunks(5, 5, 41, 411), (1, 4), prove_chunks),
    "chunk 2197": (_chunks(13, 13, 13, 410), (4, 6), prove_chunks),
    "scene table": (scene_table_100, (1, 3), prove_table_rows),
    "padded table": (lambda: staged_40(30), (0, 2), prove_table_rows),
    "t_now lds": (t_now_lds, (0, 1, 2, 3), prove_t_now),
    "t_now table": (t_now_table, (0, 1, 3, 4), prove_t_now),
    "mixed knots": (mixed_knots, (0, 2, 3, 4), prove_mixed_knots),
    "broad phase": (broad_phase, (0, 1, 2), prove_broad_phase),
    "short table": (short_table, (1, 7, 10, 14), prove_short_table),
    "knots 220": (lambda: short_table(220), (1, 7, 10, 14), prove_short_table),
    "knots 400": (lambda: short_table(400), (1, 7, 10, 14), prove_short_table),
}


def prove(oracle, name):
    """Assert the two rules for a case - every compared ego has a winner and is decidable, then the case's own proof that it reaches
    its path and that the term matters there - and return its recorded numbers."""
    ref = reference(oracle, name)
    rec = record(ref)
    assert 2 <= len(ref.egos) <= 4
    for k, e in enumerate(ref.egos):
        assert ref.idx[k] >= 0 and ref.plain[k] >= 0 and rec["margin"][k] > 1e-6, (name, e)
    PATH_CASES[name][2](oracle, ref, rec, name)
    return rec


# ---------------------------------------------------------------------------
# the closed loop: three cycles of the config-2 batch, simulated with the restatement
# ---------------------------------------------------------------------------
LOOP_EGOS = (0, 1, 2)
LOOP_CYCLES = 3


def loop_batch():
    return weighted(synth.make_batch(6, 5, 5, 5, 10, 100, True, 101))


def with_state(batch, ego, t_now):
    """`batch` at the start states and time steps a closed loop has reached."""
    batch.ego[:] = ego
    batch.t_now[:] = t_now
    return batch


@functools.lru_cache(maxsize=None)
def loop_reference(oracle):
    """[(ego states [3, 6], best_idx [3], best_cost [3], margins [3])] per cycle for LOOP_EGOS: every cycle the restatement's winner,
    then the hand-over to its point 1 (s, s_d, s_dd, d, d_d, d_dd: rows 1 - 3 and 5 - 7 of its series) one time step later."""
    b = loop_batch()
    out = []
    for cycle in range(LOOP_CYCLES):
        b.t_now[:] = cycle
        rows = [R.ego_table(oracle, b, e) for e in LOOP_EGOS]
        out.append((b.ego[list(LOOP_EGOS)].copy(), [r[2] for r in rows], [r[3] for r in rows], [float(R.margin(r[0], r[1])) for r in rows]))
        for e, r in zip(LOOP_EGOS, rows):
            w = R.winner_series(oracle, b, e, r[2])
            b.ego[e] = [w[1, 1], w[2, 1], w[3, 1], w[5, 1], w[6, 1], w[7, 1]]
    return out
