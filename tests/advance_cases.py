"""One deterministic table of hand-over cases (one ego each) for tests/test_advance_ref_cpu.py and tests/test_gpu_advance.py.

build(O, lattice) -> Table: the arrays of one launch (egos share a few frames: F < B, nx < NX, +inf padded knots), every case's
name, and the expected result of tests/advance_ref.py per case.  Goals are placed around the point the REFERENCE lands on (never
around a result of the code under test).  Offsets of "1e-6" are 1.001e-6, so that the computed margin cannot round below the
decidability bound of 1e-6 the CPU test asserts.
"""
from types import SimpleNamespace

import numpy as np

import advance_ref as R

TICK = 0.1
VEH_L = 4.5          # l / 2 = 2.25: a multiple of the ulp of every coordinate below 2^52 * 2^-2 (the exact-equality test relies on it)
V = 6                # goal_max_vertices
FAR = 1e9
LATTICES = {"A": (3, 4, 5), "B": (5, 3, 2)}  # nd, nt, nv
EPS = (-1e-3, -1.001e-6, 1.001e-6, 1e-3)     # threshold offsets (m): inside by 1 mm / 1 um, outside by 1 um / 1 mm
ULP_LENGTHS = (0.30000000000000004, 2.9000000000000004, 203.10000000000002)


def straight_frame(s_knots, x0, y0, theta):
    """Tables of a straight line written directly: knots as given (bit for bit), position (x0, y0) + s (cos, sin)(theta)"""
    k = np.array(s_knots, dtype=np.float64)
    c = np.zeros((8, len(k)))
    c[0], c[4] = x0 + np.cos(theta) * k, y0 + np.sin(theta) * k
    c[1, :-1], c[5, :-1] = np.cos(theta), np.sin(theta)
    return k, c


def curved_frame(n, length, amp, lam, x0=0.0, y0=0.0):
    """n points of y = amp sin(x / lam), the synthetic road of the benchmarks, through the package's host spline (spline.build_frames)"""
    from fiss_plus_planner_amd.spline import build_frames

    x = np.linspace(0.0, length, n)
    knots, coef = build_frames(np.column_stack([x0 + x, y0 + amp * np.sin(x / lam)])[None])
    return knots[0], coef[0]


def frames():
    """name -> (knots [nx], coef [8, nx])"""
    f = {
        "curve200": curved_frame(41, 200.0, 6.0, 40.0, 50.0, -20.0),
        "curve120": curved_frame(25, 120.0, 3.0, 55.0, -300.0, 410.0),
        "line30": straight_frame([0.0, 10.0, 20.0, 30.0], 100.0, -50.0, 0.6),
        "line100w": straight_frame(np.linspace(0.0, 100.0, 11), 40.0, 7.0, np.pi - 1e-3),   # heads west: yaw next to +pi
        "line015": straight_frame([0.0, 0.15], 10.0, 20.0, 0.3),                              # two resampled points (0, 0.1)
        "line008": straight_frame([0.0, 0.08], 10.0, 30.0, 0.3),                              # one resampled point: no end of map
    }
    for s_last in ULP_LENGTHS:
        f[f"ulp{s_last:.1f}"] = straight_frame([0.0, s_last / 4.0, s_last / 2.0, s_last], 64.0, 32.0, 0.25)
    for name, (k, _) in f.items():
        assert np.all(np.diff(k) > 0), name
    assert [f[f"ulp{s:.1f}"][0][-1] for s in ULP_LENGTHS] == list(ULP_LENGTHS) and f["line30"][0][-1] == 30.0
    return f


def _case(name, frame, ego, end=None, idx=None, t_now=0, cycles=0, done=R.RUNNING, goal=None, **kw):
    return SimpleNamespace(name=name, frame=frame, ego=list(ego), end=end, idx=idx, t_now=int(t_now), cycles=int(cycles),
                           done=int(done), goal=goal or {}, generic=kw.get("generic", False))


def _specs(lattice, rng):
    """The cases as specifications: goals are given relative to the landing point (resolved by build)."""
    nd, nt, nv = LATTICES[lattice]
    C = nd * nt * nv
    out = []
    slow = lambda s: [s, 0.2, 0.0, 0.0, 0.0, 0.0]  # creeps along a short line: point 1 at s + 0.02
    gen_ego = lambda fr: [rng.uniform(5, 90 if fr == "curve120" else 150), rng.uniform(2, 13), rng.uniform(-1, 1), rng.uniform(-0.8, 0.8),
                          rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2)]
    gen_end = lambda: (rng.uniform(-1, 1), rng.uniform(0, 13.5), rng.uniform(2, 10))
    if lattice == "B":  # the second index decode: every flat index once
        for i in range(C):
            out.append(_case(f"decode {i}", "curve200" if i % 2 else "curve120", gen_ego("curve120"), idx=i, t_now=rng.integers(0, 41), cycles=rng.integers(0, 41)))
        return out
    # ---- points
    ego0 = [40.0, 9.0, 0.4, 0.3, -0.2, 0.1]
    for name, T in (("N=1", 0.05), ("N=2", 0.15), ("N=3", 0.25), ("N=4 T=3*0.1", 0.30000000000000004)):
        out.append(_case(f"points {name}", "curve200", ego0, end=(-0.4, 7.0, T), t_now=3, cycles=5))
        out.append(_case(f"points {name} heading", "curve120", [30.0, 12.0, -0.5, -0.6, 0.8, 0.0], end=(0.9, 3.0, T), t_now=11, cycles=2,
                         goal=dict(region=1.0, iv=dict(orientation=(-0.25, 0.25)))))
    L = "curve200"
    out.append(_case("points point 2 beyond the last knot", L, ["L-1.5", 10.0, 0.0, 0.2, 0.1, 0.0], end=(0.0, 10.0, 5.0), t_now=1))
    out.append(_case("points point 1 beyond the last knot", L, ["L-0.5", 10.0, 0.0, 0.2, 0.1, 0.0], end=(0.0, 10.0, 5.0), t_now=1))
    out.append(_case("points s at the last knot", L, ["L", 10.0, 0.0, 0.2, 0.1, 0.0], end=(0.0, 10.0, 5.0)))
    out.append(_case("points s beyond the last knot", L, ["L+1", 10.0, 0.0, 0.2, 0.1, 0.0], end=(0.0, 10.0, 5.0)))
    out.append(_case("points s below the first knot", L, [-0.5, 10.0, 0.0, 0.2, 0.1, 0.0], end=(0.0, 10.0, 5.0)))
    out.append(_case("points at rest", L, [60.0, 0.0, 0.0, 0.25, 0.0, 0.0], end=(0.25, 0.0, 5.0), t_now=9, cycles=9))
    # ---- no plan / already done
    out.append(_case("no plan best_idx -1", L, ego0, idx=-1, t_now=4, cycles=6))
    for k, nm in enumerate(("d", "v", "T")):
        e = [0.1, 5.0, 6.0]; e[k] = np.nan
        out.append(_case(f"no plan NaN {nm}", L, ego0, end=tuple(e), t_now=4, cycles=6))
    for code in (R.DONE_GOAL, R.DONE_END_OF_LINE, R.DONE_NO_SOLUTION, R.DONE_GOAL_REGION):
        out.append(_case(f"already done {code}", L, ego0, end=(0.1, 5.0, 6.0), t_now=12, cycles=13, done=code, goal=dict(centre=(0.0, 0.0))))
        out.append(_case(f"already done {code} idx", L, ego0, idx=7, t_now=12, cycles=13, done=code, goal=dict(region=1.0)))
    # ---- goal centre: l/2 from either side, several directions
    for k, eps in enumerate(EPS):
        for j, ang in enumerate((0.0, 2.0, -2.6, 0.9)):
            fr = "curve120" if j % 2 else "curve200"
            out.append(_case(f"centre {eps:+.0e} dir {ang}", fr, gen_ego(fr), end=gen_end(), t_now=rng.integers(0, 41), cycles=rng.integers(0, 41),
                             goal=dict(centre=(VEH_L / 2 + eps, ang))))
    # ---- end of map: 3.0 from either side (the ego's s is solved for), the exact lengths, the short lines
    for eps in EPS:
        out.append(_case(f"end of map {eps:+.0e} line30", "line30", [26.0, 5.0, 0.0, 0.0, 0.0, 0.0], end=(0.0, 5.0, 4.0), t_now=2, goal=dict(eom=eps)))
        out.append(_case(f"end of map {eps:+.0e} curve", "curve120", [100.0, 8.0, 0.3, 0.5, -0.1, 0.0], end=(-0.3, 6.0, 5.0), t_now=2, goal=dict(eom=eps)))
    out.append(_case("end of map length 30.0 near", "line30", [28.0, 3.0, 0.0, 0.1, 0.0, 0.0], end=(0.1, 3.0, 3.0)))
    out.append(_case("end of map length 30.0 far", "line30", [5.0, 3.0, 0.0, 0.1, 0.0, 0.0], end=(0.1, 3.0, 3.0)))
    out.append(_case("end of map ulp length 0.3", "ulp0.3", slow(0.05), end=(0.0, 0.2, 1.0), t_now=5))
    out.append(_case("end of map ulp length 2.9", "ulp2.9", slow(1.0), end=(0.05, 0.2, 1.0), t_now=5))
    out.append(_case("end of map ulp length 203.1", "ulp203.1", [201.0, 2.0, 0.0, 0.2, 0.0, 0.0], end=(0.0, 2.0, 3.0), t_now=5))
    out.append(_case("end of map ulp length 203.1 far", "ulp203.1", [150.0, 2.0, 0.0, 0.2, 0.0, 0.0], end=(0.0, 2.0, 3.0), t_now=5))
    out.append(_case("end of map line of two points", "line015", slow(0.01), end=(0.0, 0.2, 1.0)))
    out.append(_case("end of map line of one point: rule off", "line008", slow(0.01), end=(0.0, 0.2, 1.0)))
    out.append(_case("end of map line of one point: centre still applies", "line008", slow(0.01), end=(0.0, 0.2, 1.0), goal=dict(centre=(1.0, 0.5))))
    # ---- order of the rules (line30, landing within 3 m of its last point)
    near = [28.0, 3.0, 0.0, 0.1, 0.0, 0.0]
    out.append(_case("order region + centre + end of map", "line30", near, end=(0.1, 3.0, 3.0), goal=dict(region=1.0, centre=(0.5, 1.0))))
    out.append(_case("order centre + end of map", "line30", near, end=(0.1, 3.0, 3.0), goal=dict(centre=(0.5, 1.0))))
    out.append(_case("order polygon but interval false + centre", "line30", near, end=(0.1, 3.0, 3.0), t_now=7,
                     goal=dict(region=1.0, iv=dict(time_step=(8, 9)), centre=(0.5, 1.0))))
    out.append(_case("order polygon but interval false + end of map", "line30", near, end=(0.1, 3.0, 3.0), t_now=7, goal=dict(region=1.0, iv=dict(velocity=(1.0, 2.0)))))
    # ---- goal region: orientation, time step, velocity, goal_nv
    g = lambda: dict(frame="curve200", ego=gen_ego("curve200"), end=gen_end(), cycles=rng.integers(0, 41))
    for nm, rel in (("contains", (-0.5, 0.5)), ("misses low by 1e-3", (1e-3, 0.5)), ("misses high by 1e-3", (-0.5, -1e-3)), ("contains by 1e-3", (-1e-3, 1e-3))):
        out.append(_case(f"region orientation {nm}", **g(), t_now=rng.integers(0, 41), goal=dict(region=2.0, iv=dict(orientation=rel))))
    west = lambda: [rng.uniform(10, 80), rng.uniform(3, 10), 0.0, rng.uniform(-0.3, 0.3), 0.0, 0.0]  # (d_d = 0: the heading stays next to +pi)
    for k in range(3):
        e = west()
        out.append(_case(f"region heading +pi, interval at -pi {k}", "line100w", e, end=(e[3], e[1], 5.0), goal=dict(region=2.0, iv=dict(orientation_abs=(-np.pi, -np.pi + 0.01)))))
        out.append(_case(f"region heading +pi, interval at +pi {k}", "line100w", e, end=(e[3], e[1], 5.0), goal=dict(region=2.0, iv=dict(orientation_abs=(np.pi - 0.01, np.pi)))))
    for nm, iv in (("[7, 7]", (7, 7)), ("[6, 7]", (6, 7)), ("[7, 9]", (7, 9)), ("[8, 9]", (8, 9)), ("[0, 6]", (0, 6)), ("[8, nan]", (8, np.nan))):
        out.append(_case(f"region time step {nm} at t_now 7", **g(), t_now=7, goal=dict(region=0.5, iv=dict(time_step=iv))))
    for nm, rel in (("contains", (-0.5, 0.5)), ("below", (1e-3, 1.0)), ("above", (-1.0, -1e-3))):
        out.append(_case(f"region velocity {nm}", **g(), t_now=rng.integers(0, 41), goal=dict(region=4.0, iv=dict(velocity=rel))))
    # (all V slots hold a ring around the landing point; the slot BEHIND the ring of "goal_nv V + 1" - the next ego's first vertex - lies on
    # that ring's closing edge, so a kernel that does not skip the rule reads a 7-vertex ring that contains the point, whatever the order of the table)
    for nv_ in (0, 2, V + 1):
        out.append(_case(f"region goal_nv {nv_}", **g(), t_now=3, goal=dict(region=1.0, nv=nv_, shape="hexagon")))
        out.append(_case(f"region goal_nv {nv_} + centre", **g(), t_now=3, goal=dict(region=1.0, nv=nv_, shape="hexagon", centre=(1.0, -1.0), closes_previous=True)))
    for k, shape in enumerate(("beside", "triangle", "nonconvex")):  # (a point ON the boundary is not decidable from outside: tests/test_gpu_closed_loop_device.py has it)
        out.append(_case(f"region polygon {shape}", **g(), t_now=k, goal=dict(region=1.0, shape=shape)))
    # ---- index decode: every flat index once, per-ego v_samples
    for i in range(C):
        fr = "curve120" if i % 3 == 0 else "curve200"
        out.append(_case(f"decode {i}", fr, gen_ego(fr), idx=i, t_now=rng.integers(0, 41), cycles=rng.integers(0, 41)))
    # ---- generic: random states, end states on and off the lattice, some with a region or a centre around the landing point
    k = 0
    while len(out) < 300:
        fr = "curve120" if k % 3 == 0 else "curve200"
        goal = {}
        if k % 7 == 1: goal = dict(region=2.0, iv=dict(time_step=(0, 20)))
        if k % 7 == 3: goal = dict(centre=(rng.uniform(0.0, 4.5), rng.uniform(-3, 3)))
        kw = dict(idx=int(rng.integers(0, C))) if k % 2 else dict(end=gen_end())
        out.append(_case(f"generic {k}", fr, gen_ego(fr), t_now=rng.integers(0, 41), cycles=rng.integers(0, 41), goal=goal, generic=True, **kw))
        k += 1
    return out


def lattice_samples(lattice, B, rng):
    nd, nt, nv = LATTICES[lattice]
    d = np.linspace(-0.7, 0.6, nd)
    t = np.array([0.15, 0.25, 4.0, 7.5])[:nt] if nt == 4 else np.linspace(3.0, 8.0, nt)   # (lattice A: N = 2 and N = 3 through best_idx too)
    v = np.stack([np.linspace(0.0, hi, nv) for hi in rng.uniform(6.0, 13.5, B)])
    return d, t, v


def _ring(shape, x, y, w):
    if shape == "around":    return [[x - w, y - w], [x + w, y - w], [x + w, y + w], [x - w, y + w]]
    if shape == "beside":    return [[x + w, y - w], [x + 3 * w, y - w], [x + 3 * w, y + w], [x + w, y + w]]
    if shape == "hexagon":   return [[x - w, y - w], [x, y - 2 * w], [x + w, y - w], [x + w, y + w], [x, y + 2 * w], [x - w, y + w]]
    if shape == "triangle":  return [[x - w, y - w], [x + w, y - w], [x + w, y + 2 * w]]
    if shape == "nonconvex": return [[x - w, y - w], [x + w, y - w], [x + w, y + w], [x, y + w], [x, y + w / 2], [x - w, y + w / 2]]
    raise ValueError(shape)


NO_IDX = -(2 ** 31)  # best_idx of a case that is given by its end state only


def _advance(O, T, b, ego=None, goal=False, variant="full", state=None, goal_xy=None, series_tol=None):
    f = T.frame_of[b]
    n = T.nx[f]
    st = state or T
    kw = {}
    if goal:
        kw = dict(goal_xy=T.goal_xy[b] if goal_xy is None else goal_xy[b])
        if variant != "no_poly":
            kw.update(goal_poly=T.goal_poly[b], goal_nv=T.goal_nv[b], goal_max_vertices=T.goal_max_vertices,
                      goal_intervals=None if variant == "no_intervals" else T.goal_intervals[b])
    return R.advance(O, tick_t=T.tick_t, veh_l=T.veh_l, knots=T.knots[f, :n], coef=T.coef[f, :, :n], ego=st.ego[b] if ego is None else ego,
                     t_now=st.t_now[b], cycles=st.cycles[b], done=st.done[b] if goal else R.RUNNING, end_state=T.end_state[b], series_tol=series_tol, **kw)


def reference(O, T, variant="full", state=None, goal_xy=None, series_tol=None):
    """advance_ref for every ego of the table.  variant: "full", "no_intervals" (goal_intervals = NULL), "no_poly" (goal_poly = NULL);
    state: another loop state (ego, t_now, cycles, done) than the table's; goal_xy: other goal centres."""
    return [_advance(O, T, b, goal=True, variant=variant, state=state, goal_xy=goal_xy, series_tol=series_tol) for b in range(T.B)]


def build(O, lattice="A"):
    """-> Table: B, lattice (nd, nt, nv), names, generic [B] bool; frames nx [F], knots [F, NX], coef [F, 8, NX]; per ego frame_of, ego,
    t_now, cycles, done, end_state [B, 3] (the decoded sample for cases given by index), best_idx [B] (NO_IDX = the case has none),
    d_samples, t_samples, v_samples [B, nv], goal_xy, goal_poly [B, V, 2], goal_nv, goal_intervals [B, 6], goal_max_vertices."""
    rng = np.random.default_rng(20240 + ord(lattice))
    specs = _specs(lattice, rng)
    B = len(specs)
    fr = frames()
    fnames = list(fr)
    NX = max(len(k) for k, _ in fr.values())
    F = len(fnames)
    knots = np.full((F, NX), np.inf); coef = np.zeros((F, 8, NX)); nx = np.zeros(F, dtype=np.int32)
    for f, nm in enumerate(fnames):
        k, c = fr[nm]
        nx[f] = len(k); knots[f, :len(k)] = k; coef[f, :, :len(k)] = c
    d_s, t_s, v_s = lattice_samples(lattice, B, rng)
    T = SimpleNamespace(B=B, lattice=LATTICES[lattice], names=[c.name for c in specs], generic=np.array([c.generic for c in specs]), tick_t=TICK, veh_l=VEH_L,
                        nx=nx, knots=knots, coef=coef, frame_of=np.array([fnames.index(c.frame) for c in specs], dtype=np.int32),
                        ego=np.zeros((B, 6)), t_now=np.array([c.t_now for c in specs], dtype=np.int32), cycles=np.array([c.cycles for c in specs], dtype=np.int32),
                        done=np.array([c.done for c in specs], dtype=np.int32), end_state=np.full((B, 3), np.nan), best_idx=np.full(B, NO_IDX, dtype=np.int32),
                        d_samples=d_s, t_samples=t_s, v_samples=v_s, goal_xy=np.full((B, 2), FAR), goal_poly=np.zeros((B, V, 2)), goal_nv=np.zeros(B, dtype=np.int32),
                        goal_intervals=np.full((B, 6), np.nan), goal_max_vertices=V)
    nd, nt, nv = T.lattice
    for b, c in enumerate(specs):
        ego = list(c.ego)
        if isinstance(ego[0], str):  # "L-1.5": relative to the line's last knot
            ego[0] = fr[c.frame][0][-1] + float(ego[0][1:] or 0.0)
        T.ego[b] = ego
        if c.idx is not None:
            T.best_idx[b] = c.idx
            if c.idx >= 0:
                idd, it, iv = R.decode_index(c.idx, nd, nt, nv)
                T.end_state[b] = [d_s[idd], v_s[b, iv], t_s[it]]
        else:
            T.end_state[b] = c.end
    # goals, relative to where the reference lands
    for b, c in enumerate(specs):
        g = c.goal
        if not g:
            continue
        if "eom" in g:  # the ego's arclength that puts the landing point at 3.0 + eps from the line's last point (secant on the margin)
            f = lambda s: _advance(O, T, b, ego=np.concatenate([[s], T.ego[b, 1:]])).margins["end_of_map"] - g["eom"]
            s_a, s_b = T.ego[b, 0], T.ego[b, 0] + 0.25
            f_a, f_b = f(s_a), f(s_b)
            for _ in range(40):
                if abs(f_b) < 1e-10:
                    break
                s_a, s_b, f_a = s_b, s_b - f_b * (s_b - s_a) / (f_b - f_a), f_b
                f_b = f(s_b)
            assert abs(f_b) < 1e-10, (c.name, f_b)
            T.ego[b, 0] = s_b
        land = _advance(O, T, b)
        if not land.moved:
            continue
        x, y, yaw = land.cart
        if "centre" in g:
            r, ang = g["centre"]
            T.goal_xy[b] = [x + r * np.cos(ang), y + r * np.sin(ang)]
        if "region" in g:
            ring = _ring(g.get("shape", "around"), x, y, g["region"])
            T.goal_poly[b, :len(ring)] = ring
            if g.get("closes_previous"):  # (this ego's ring is never evaluated: its goal_nv is outside 3 .. V)
                T.goal_poly[b, 0] = 0.5 * (T.goal_poly[b - 1, V - 1] + T.goal_poly[b - 1, 0])
            T.goal_nv[b] = g.get("nv", len(ring))
            iv = g.get("iv", {})
            if "time_step" in iv: T.goal_intervals[b, 0:2] = iv["time_step"]
            if "velocity" in iv: T.goal_intervals[b, 2:4] = land.ego[1] + np.array(iv["velocity"])
            if "orientation" in iv: T.goal_intervals[b, 4:6] = yaw + np.array(iv["orientation"])
            if "orientation_abs" in iv: T.goal_intervals[b, 4:6] = iv["orientation_abs"]
    T.has_idx = T.best_idx != NO_IDX
    return T


def take(T, sel):
    """The sub-table of the egos `sel` (index array, slice or bool mask); the frames stay"""
    out = SimpleNamespace(**vars(T))
    idx = np.arange(T.B)[sel]
    for k in ("generic", "frame_of", "ego", "t_now", "cycles", "done", "end_state", "best_idx", "v_samples", "goal_xy", "goal_poly", "goal_nv", "goal_intervals", "has_idx"):
        setattr(out, k, np.ascontiguousarray(getattr(T, k)[idx]))
    out.names = [T.names[i] for i in idx]
    out.B = len(idx)
    return out


def exact_end_of_map_table(T0, n=24, s_last=30.0):
    """n egos, each on a straight line of its own with knots 0, 20, (n_pts - 1) * 0.1, s_last: the line's last resampled point IS the
    third knot, so the kernel evaluates it with dx == 0 and gets that knot's `a` coefficients bit for bit.  Those coefficients are free
    (the tables are written directly, the egos drive on the first segment): end_point_at() puts the point anywhere."""
    rng = np.random.default_rng(77)
    s_ref = (R.end_point_count(s_last) - 1) * R.STEP
    assert 20.0 < s_ref < s_last and s_ref == np.arange(0, s_last, R.STEP)[R.end_point_count(s_last) - 1]
    T = take(T0, slice(0, 0))
    T.B, T.names, T.generic = n, [f"exact end of map {b}" for b in range(n)], np.zeros(n, dtype=bool)
    T.nx, T.knots, T.coef = np.full(n, 4, dtype=np.int32), np.zeros((n, 4)), np.zeros((n, 8, 4))
    for b in range(n):
        T.knots[b], T.coef[b] = straight_frame([0.0, 20.0, s_ref, s_last], rng.uniform(64.0, 120.0), rng.uniform(-100.0, 100.0), 0.0)
    T.frame_of = np.arange(n, dtype=np.int32)
    T.ego = np.column_stack([rng.uniform(1, 8, n), rng.uniform(2, 10, n), rng.uniform(-1, 1, n), rng.uniform(-0.8, 0.8, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-0.2, 0.2, n)])
    T.end_state = np.column_stack([rng.uniform(-1, 1, n), rng.uniform(2, 10, n), rng.uniform(3, 8, n)])
    T.t_now, T.cycles, T.done = (np.zeros(n, dtype=np.int32) for _ in range(3))
    T.best_idx, T.has_idx = np.full(n, NO_IDX, dtype=np.int32), np.zeros(n, dtype=bool)
    T.v_samples = np.tile(np.linspace(0.0, 10.0, T.lattice[2]), (n, 1))
    T.goal_xy, T.goal_poly, T.goal_nv, T.goal_intervals = np.full((n, 2), FAR), np.zeros((n, V, 2)), np.zeros(n, dtype=np.int32), np.full((n, 6), np.nan)
    return T


def end_point_at(T, x, y):
    """The table with every line's last resampled point moved to (x[b], y[b])"""
    out = SimpleNamespace(**vars(T))
    out.coef = T.coef.copy()
    out.coef[:, 0, 2], out.coef[:, 4, 2] = x, y
    return out


def exact_end_of_map_goals(T, x1, y1):
    """-> (on, off): the end points exactly 3.0 m from the landing points (x1, y1), and one ulp further away.  x1 > 3 and the offset
    points towards 0, so x1 - 3.0 is exact (3.0 is a multiple of the ulp of x1, the exponent cannot grow)."""
    assert (x1 > 4.0).all()
    px = x1 - R.END_OF_MAP
    assert (x1 - px == R.END_OF_MAP).all() and (np.hypot(x1 - px, y1 - y1) == R.END_OF_MAP).all()  # the construction, not a skip
    px2 = np.nextafter(px, -np.inf)
    assert (x1 - px2 > R.END_OF_MAP).all() and (np.hypot(x1 - px2, 0.0) > R.END_OF_MAP).all()
    return end_point_at(T, px, y1), end_point_at(T, px2, y1)
