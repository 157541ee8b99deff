"""Independent restatement of the gates (fp_gate_mask), numpy + the CPU oracle only.

For one ego of a ProblemBatch everything about a candidate comes from the ORACLE - its flag word, its cost (dense_tables), its dumped
S series and N / M (eval_traj) - and the rule is restated from its definition (include/frenet_gpu.h), point by point:

    points      q_0 = ego s + front;  q_i = s_i + front, i = 1 .. M-1 (M <= 1: nothing is checked, no bit)
    crossing    of gate g at i (1 <= i <= M-1):  q_{i-1} <= gate_s[f, g] < q_i  (a NaN slot compares false)
    state       w = gate_closed[f, clip(t_now + i, 0, T_gate - 1)]
    waiver      (gate_max_decel > 0)  v0 > 0 and q_0 <= gate_s and q_0 + v0 * v0 / (2 * max_decel) > gate_s
    violation   a crossing at i of a gate that is not waived and whose bit is set in w
    bit         a violating candidate gets FLAG_SPEED ORed in; nothing is ever cleared, no other bit touched
    winner      minimum cost over candidates without an infeasible bit and a non-NaN cost, the LAST one in FOP index order on exact ties

Per candidate it also returns the SLACK: the smallest |q_i - gate_s| over i = 1 .. M-1 and the frame's used gates and, when the waiver
is on, |q_0 + v0^2 / (2 max_decel) - gate_s| (q_0 itself is computed the same way on both sides and is not part of it).  The kernel
evaluates the series by fma Horner, the oracle point by point: a candidate with slack < UNDECIDED_TOL (the project's FP_AUDIT_GAP_TOL)
may be decided either way and is excluded from exact comparisons; the tests cap how many there may be.

ref_loop drives one ego through the closed loop [oracle dense tables -> this rule -> argmin -> tests/advance_ref.py hand-over].

Nothing here calls the library under test."""
import dataclasses
from types import SimpleNamespace

import numpy as np

import rule_ref_common as common
from rule_ref_common import argmin, plain_batch  # noqa: F401  (the tests reach plain_batch through this module too)

FLAG_SPEED = 1
FLAG_INFEASIBLE = 1 | 2 | 4 | 16 | 32 | 64 | 128  # FP_FLAG_CONSTRAINTS | FP_FLAG_COLLISION | FP_FLAG_BOUNDARY
UNDECIDED_TOL = 1e-9                              # FP_AUDIT_GAP_TOL (include/frenet_gpu.h)
MAX_UNDECIDED_SHARE = 0.005                       # of the candidates of a test batch
MAX_EXCLUDED_EGOS = 1                             # per test batch
S = 1                                             # row of a [16, stride] dump (FP_ARR_S)

SEED = 33055  # the seed of every test batch (the envelope's and the boundary check's batches use the same one)


def waived_gates(batch, b):
    """[G] bool: the gates of ego b's frame the dilemma-zone rule waives, and the rule's distance from its threshold per gate."""
    g = batch.gate_s[int(batch.frame_of[b])]
    q0, v0, md = batch.ego[b, 0] + batch.gate_front, batch.ego[b, 1], float(batch.gate_max_decel)
    if not md > 0.0:
        return np.zeros(len(g), dtype=bool), np.full(len(g), np.inf)
    with np.errstate(invalid="ignore"):
        reach = q0 + v0 * v0 / (2.0 * md)
        return (v0 > 0) & (q0 <= g) & (reach > g), np.where(np.isnan(g), np.inf, np.abs(reach - g))


def ego_gates(O, batch, b, tables=None):
    """The rule for ego b of a batch that carries gates.  tables = (cost [C], flags [C]) to mask (default: the oracle's dense tables).
    Returns a namespace: cost [C], flags_in [C], flags [C] (bit ORed in), gated [C], step [C] (the first violating point, -1 = none),
    slack [C], undecided [C], M [C], N [C], waived [G], best_idx, best_cost (the masked winner), best_in (the winner of flags_in),
    n_gated."""
    # (the oracle's tables do not depend on t_now without obstacles; a negative one is the gates' business alone)
    prob = O.problems_from_batch(dataclasses.replace(batch, t_now=np.maximum(batch.t_now, 0)), egos=[b])[0]
    cost, flags_in = prob.dense_tables() if tables is None else (np.asarray(tables[0], dtype=np.float64), np.asarray(tables[1], dtype=np.uint32))
    f = int(batch.frame_of[b])
    line, words = batch.gate_s[f], batch.gate_closed[f]
    T_gate, t_now, front = len(words), int(batch.t_now[b]), float(batch.gate_front)
    waived, waiver_gap = waived_gates(batch, b)
    used = np.nonzero(~np.isnan(line))[0]
    Cn, nv, nt = batch.C, batch.nv, batch.nt
    gated, step = np.zeros(Cn, dtype=bool), np.full(Cn, -1, dtype=np.int64)
    slack = np.full(Cn, np.inf)
    Ms, Ns = np.zeros(Cn, dtype=np.int64), np.zeros(Cn, dtype=np.int64)
    for c in range(Cn):
        iv, it, i_d = c % nv, (c // nv) % nt, c // (nv * nt)
        r = prob.eval_traj(float(batch.d_samples[i_d]), float(batch.v_samples[b, iv]), float(batch.t_samples[it]), dump=True, stride=256)
        N, M = r.N, r.M
        assert N == (int(flags_in[c]) >> 8) & 0xFFF and M == int(flags_in[c]) >> 20, (b, c, N, M, hex(int(flags_in[c])))
        Ns[c], Ms[c] = N, M
        slack[c] = waiver_gap.min() if len(used) else np.inf
        if M <= 1:
            continue
        q = np.concatenate(([batch.ego[b, 0] + front], r.arrays[S, 1:M] + front))
        for i in range(1, M):
            w = int(words[min(max(t_now + i, 0), T_gate - 1)])
            for g in used:
                slack[c] = min(slack[c], abs(q[i] - line[g]))
                if q[i - 1] <= line[g] < q[i] and not waived[g] and (w >> int(g)) & 1 and step[c] < 0:
                    gated[c], step[c] = True, i
    flags = flags_in | np.where(gated, FLAG_SPEED, 0).astype(np.uint32)
    return SimpleNamespace(cost=cost, flags_in=flags_in, flags=flags, gated=gated, step=step, slack=slack, undecided=slack < UNDECIDED_TOL, M=Ms, N=Ns,
                           waived=waived, best_idx=argmin(cost, flags)[0], best_cost=argmin(cost, flags)[1], best_in=argmin(cost, flags_in)[0],
                           n_gated=int(gated.sum()))


def batch_gates(O, batch, tables=None, egos=None):
    """ego_gates for the egos asked for (all by default) -> list; tables = (cost [B, C], flags [B, C]) or None."""
    egos = range(batch.B) if egos is None else egos
    return [ego_gates(O, batch, b, None if tables is None else (tables[0][b], tables[1][b])) for b in egos]


def check_caps(refs, what=""):
    """The caps the tests rely on: at most 0.5 % of the batch's candidates undecided, at most one ego excluded for having one."""
    return common.check_caps(refs, MAX_UNDECIDED_SHARE, MAX_EXCLUDED_EGOS, what)


def gated_share(refs):
    return sum(r.n_gated for r in refs) / sum(len(r.slack) for r in refs)


# ---------------------------------------------------------------------------
# the test batches (shared by tests/test_gates_cpu.py, which checks caps and shares on the reference alone, and tests/test_gpu_gates.py)
# ---------------------------------------------------------------------------
AHEAD = (25.0, 60.0)  # m: the two lines of every frame, ahead of the frame's ego
T_GATE = 128          # steps of the phase tables (the base batches' horizon is N <= 100)
MAX_DECEL = 2.0       # m/s^2 of the waiver case: the egos faster than ~9.5 m/s cannot stop in front of the line 25 m ahead


def phases(F, T, G, period=(23, 31), offset=7):
    """[F, T, G] truth values: gate g of frame f is closed while ((t + offset f) // period_g) is even (g even) / odd (g odd): lights with
    two phase lengths, shifted from frame to frame, so that the two lines of a frame are never in step."""
    t = np.arange(T)[None, :, None] + offset * np.arange(F)[:, None, None]
    g = np.arange(G)[None, None, :]
    per = np.asarray(period)[g % len(period)] + g // len(period)
    return ((t // per) % 2) == (g % 2)


def with_gates(batch, ahead=AHEAD, T_gate=T_GATE, closed=None, front=None, max_decel=0.0, **kw):
    """A copy of `batch` that carries gates: the lines `ahead` metres in front of each ego's s (one frame per ego, synth.make_batch),
    closed [F, T, G] truth values (None: phases), front None = veh_l / 2; kw overrides any other ProblemBatch field."""
    from fiss_plus_planner_amd.spline import gate_bits

    ego = np.asarray(kw.get("ego", batch.ego))
    line = np.full((batch.F, len(ahead)), np.nan)
    for b in range(batch.B):
        line[int(batch.frame_of[b])] = ego[b, 0] + np.asarray(ahead)
    if closed is None:
        closed = phases(batch.F, T_gate, len(ahead))
    return dataclasses.replace(batch, gate_s=line, gate_closed=gate_bits(closed), gate_front=0.5 * batch.veh_l if front is None else front,
                               gate_max_decel=max_decel, **kw)


def _stride32():
    ahead = tuple(4.0 + 2.5 * g for g in range(32))  # a line every 2.5 m from 4 m to 81.5 m ahead, every slot used
    b = plain_batch()
    return with_gates(b, ahead=ahead, closed=phases(b.F, T_GATE, 32, period=(5, 9, 14)) & (np.arange(32) % 3 == 0)[None, None, :])


CASES = {
    "base": lambda: with_gates(plain_batch()),                                                          # two lights per frame, out of step
    "t_now": lambda: with_gates(plain_batch(), t_now=[3, 17, 40, 8, 25]),                               # every ego on its own clock
    "hold_last": lambda: with_gates(plain_batch(), T_gate=30),                                          # the table ends before the horizon
    "before_zero": lambda: with_gates(plain_batch(), t_now=[-50, -5, -120, -1, -30]),                   # t_now + i < 0: row 0 holds
    "tick005": lambda: with_gates(plain_batch(), tick_t=0.05, T_gate=2 * T_GATE),                       # N up to 200 (needs points_max)
    "line_ends": lambda: common._line_ends(plain_batch(), lambda b, ego: with_gates(b, ahead=(10.0, 25.0), ego=ego)),  # M < N and M <= 1
    "chunks": lambda: with_gates(plain_batch(2, 9, 9, 7)),                                              # C = 567: three chunks, 63 profiles
    "stride32": _stride32,                                                                              # gate_stride = 32, every slot used
    "open": lambda: with_gates(plain_batch(), closed=np.zeros((5, T_GATE, 2), dtype=bool)),             # no bit closed: nothing may change
    "waiver": lambda: with_gates(plain_batch(), max_decel=MAX_DECEL),                                   # base with the dilemma-zone rule
}
BASE_CASES = ("base", "t_now")
_cache = {}


def case(O, name):
    """(batch, refs) of a named test batch; the reference is computed once per process and shared (do not modify it)."""
    if name not in _cache:
        batch = CASES[name]()
        _cache[name] = (batch, batch_gates(O, batch))
    return _cache[name]


# ---------------------------------------------------------------------------
# the closed loop on the reference
# ---------------------------------------------------------------------------
GATE_S, OPEN_AT = 60.0, 80  # the scenario's one line and the first step it is open at


def loop_batch(open_at=(OPEN_AT,), T_gate=256):
    """The closed-loop scenario, one ego per opening step: a straight 400 m line of 81 knots, d_samples -0.5 / 0 / 0.5, t_samples 3 / 5 /
    7 s, v_samples 0 / 3 / 6 / 9, ego s = 10, s_d = 8, one gate at s = 60, front 2.25, closed at the steps < open_at, no obstacles."""
    from fiss_plus_planner_amd import synth
    from fiss_plus_planner_amd.batch import ProblemBatch
    from fiss_plus_planner_amd.spline import gate_bits

    B = len(open_at)
    pts = np.zeros((B, 81, 2))
    pts[:, :, 0] = np.linspace(0.0, 400.0, 81)
    knots, coef = synth.build_frames(pts)
    closed = np.arange(T_gate)[None, :, None] < np.asarray(open_at)[:, None, None]
    return ProblemBatch(d_samples=[-0.5, 0.0, 0.5], t_samples=[3.0, 5.0, 7.0], v_samples=np.tile([0.0, 3.0, 6.0, 9.0], (B, 1)), target_speed=np.full(B, 9.0),
                        ego=np.tile([10.0, 8.0, 0.0, 0.0, 0.0, 0.0], (B, 1)), frame_of=np.arange(B), scene_of=np.full(B, -1), t_now=np.zeros(B), nx=np.full(B, 81),
                        knots=knots, coef=coef, obs_pose=np.zeros((0, 1, 0, 4)), obs_dims=np.zeros((0, 0, 2)), final_time_step=np.zeros(0, dtype=np.int32),
                        veh_l=4.5, veh_w=1.8, max_speed=30.0, max_accel=10.0, gate_s=np.full((B, 1), GATE_S), gate_closed=gate_bits(closed), gate_front=2.25)


def ref_loop(O, batch, b, cycles, gates=True):
    """Ego b of `batch` through `cycles` cycles of [dense tables -> gates -> argmin -> hand-over] on the reference (gates=False: the
    lattice's own winner).  -> list of rows, one per cycle driven: t_now (on entry), best_idx, n_gated, undecided (any candidate), ego [6]
    (after the hand-over), done, crossed (the bumper moved over the line in this cycle)."""
    import advance_ref

    f = int(batch.frame_of[b])
    nx = int(batch.nx[f])
    ego, t_now, done, n_cycles = batch.ego[b].copy(), int(batch.t_now[b]), 0, 0
    rows = []
    for _ in range(cycles):
        if done:
            break
        e2 = batch.ego.copy()
        e2[b] = ego
        tn = batch.t_now.copy()
        tn[b] = t_now
        now = dataclasses.replace(batch, ego=e2, t_now=tn)
        r = ego_gates(O, now, b)
        best = r.best_idx if gates else r.best_in
        a = advance_ref.advance(O, tick_t=batch.tick_t, veh_l=batch.veh_l, knots=batch.knots[f, :nx], coef=batch.coef[f][:, :nx], ego=ego, t_now=t_now,
                                cycles=n_cycles, best_idx=best, d_samples=batch.d_samples, v_samples=batch.v_samples[b], t_samples=batch.t_samples)
        q_before, q_after = ego[0] + batch.gate_front, a.ego[0] + batch.gate_front
        line = batch.gate_s[f, 0]
        rows.append(SimpleNamespace(t_now=t_now, best_idx=best, n_gated=r.n_gated, undecided=bool(r.undecided.any()), ego=a.ego.copy(), done=a.done,
                                    crossed=bool(a.moved and q_before <= line < q_after)))
        ego, t_now, done, n_cycles = a.ego, a.t_now, a.done, a.cycles
    return rows


OPEN_STEPS = (80, 40, 120, 61)  # the opening step per ego of the four-ego scenario the tests drive
LOOP_CYCLES = 130


def check_loop_invariants(batch, b, t_entry, best_idx, q_before, q_after, open_at):
    """The two invariants of the scenario on one ego's driven cycles (arrays over the cycles): every cycle has a plan, the bumper moves
    over the line only into an open step, and it does so within 40 cycles of the opening."""
    line = batch.gate_s[int(batch.frame_of[b]), 0]
    assert (np.asarray(best_idx) >= 0).all(), b
    crossed = (np.asarray(q_before) <= line) & (line < np.asarray(q_after))
    arrival = np.asarray(t_entry)[crossed] + 1
    assert len(arrival) == 1 and open_at <= arrival[0] <= max(open_at, 0) + 40, (b, arrival.tolist(), open_at)
    return int(arrival[0])


_loops = {}


def loop_case(O, open_at, cycles, gates=True):
    """(batch, [rows of ego b]) of the scenario; computed once per process and shared (do not modify it)."""
    key = (tuple(open_at), cycles, gates)
    if key not in _loops:
        batch = loop_batch(open_at)
        _loops[key] = (batch, [ref_loop(O, batch, b, cycles, gates) for b in range(batch.B)])
    return _loops[key]
