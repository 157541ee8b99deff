"""numpy restatement of fp_obstacles_predict's definition (include/frenet_gpu.h), element by element, sharing no code with the product.

predict(...) -> (pose [S, T_obs, n_obs, 4], written [S, T_obs] bool, final_time_step [S], undecided [S, T_obs, n_obs] bool).
`pose` holds the definition's value in the written rows and NaN elsewhere.  `undecided` marks the elements a last-bit difference of
another correct implementation could flip: LANE elements whose s lies within 1e-6 m of either end of the line, and ARC elements whose
|u| lies within 1e-9 of the 1e-4 branch point.  check_caps asserts that an input has none."""
import numpy as np

NONE, LANE, ARC = 0, 1, 2
END_BAND = 1e-6      # m around knots[0] / knots[nx - 1]
BRANCH_BAND = 1e-9   # around |u| = 1e-4


def bisect_right(a, x):
    lo, hi = 0, len(a)
    while lo < hi:
        mid = (lo + hi) // 2
        if x < a[mid]:
            hi = mid
        else:
            lo = mid + 1
    return lo


def travelled(v, a, tau):
    """l(tau): v0 = (v < 0) ? 0 : v, the clock stopped at v0 / (-a) for a braking obstacle."""
    v0 = 0.0 if v < 0 else v
    tau_e = tau
    if a < 0:
        ts = v0 / (-a)
        if ts < tau:
            tau_e = ts
    return v0 * tau_e + 0.5 * a * tau_e * tau_e


def arc_pose(q, tau):
    x0, y0, yaw0, v, a, kappa = (float(c) for c in q)
    if not np.all(np.isfinite(q)):
        return (0.0, 0.0, 0.0, 0.0), False
    with np.errstate(all="ignore"):
        l = travelled(v, a, tau)
        u = kappa * l / 2
        sinc = 1 - u * u / 6 if abs(u) < 1e-4 else np.sin(u) / u
        pose = (x0 + l * sinc * np.cos(yaw0 + u), y0 + l * sinc * np.sin(yaw0 + u), yaw0 + kappa * l, 1.0)
    return pose, bool(abs(abs(u) - 1e-4) < BRANCH_BAND)


def lane_pose(q, tau, knots, coef):
    """knots [nx], coef [8, nx] of the scene's frame, or None when the scene has no usable frame."""
    s0, d, v, a = (float(c) for c in q[:4])
    invalid = (0.0, 0.0, 0.0, 0.0)
    with np.errstate(all="ignore"):
        s = s0 + travelled(v, a, tau)
    if knots is None or not np.isfinite(s) or not np.isfinite(d):
        return invalid, False
    near_end = bool(abs(s - knots[0]) < END_BAND or abs(s - knots[-1]) < END_BAND)
    if s < knots[0] or s >= knots[-1]:
        return invalid, near_end
    k = bisect_right(list(knots), s) - 1
    dx = s - knots[k]
    ax, bx, cx, dx3, ay, by, cy, dy3 = (float(coef[r, k]) for r in range(8))
    px = ax + bx * dx + cx * dx ** 2 + dx3 * dx ** 3
    py = ay + by * dx + cy * dx ** 2 + dy3 * dx ** 3
    gx = bx + 2 * cx * dx + 3 * dx3 * dx ** 2
    gy = by + 2 * cy * dx + 3 * dy3 * dx ** 2
    g = np.hypot(gx, gy)
    return (px + d * (-gy / g), py + d * (gx / g), float(np.arctan2(gy, gx)), 1.0), near_end


def predict(model, state, frame_of_scene, t0, n_rows, T_obs, tick_t, nx=None, knots=None, coef=None):
    model, state = np.asarray(model), np.asarray(state, dtype=np.float64)
    S, n = model.shape
    t0 = np.broadcast_to(np.asarray(t0, dtype=np.int64), (S,))
    pose = np.full((S, T_obs, n, 4), np.nan)
    written = np.zeros((S, T_obs), dtype=bool)
    undecided = np.zeros((S, T_obs, n), dtype=bool)
    fts = np.zeros(S, dtype=np.int32)
    F = 0 if knots is None else len(knots)
    for s in range(S):
        lo, hi = max(int(t0[s]), 0), min(T_obs, int(t0[s]) + int(n_rows))
        fts[s] = max(hi, 0)
        fk = fc = None
        if frame_of_scene is not None and 0 <= int(frame_of_scene[s]) < F:
            f = int(frame_of_scene[s])
            fk, fc = np.asarray(knots[f][:int(nx[f])], dtype=np.float64), np.asarray(coef[f], dtype=np.float64)
        for r in range(lo, hi):
            written[s, r] = True
            tau = (r - int(t0[s])) * tick_t
            for j in range(n):
                m = int(model[s, j])
                if m == LANE:
                    pose[s, r, j], undecided[s, r, j] = lane_pose(state[s, j], tau, fk, fc)
                elif m == ARC:
                    pose[s, r, j], undecided[s, r, j] = arc_pose(state[s, j], tau)
                else:
                    pose[s, r, j] = 0.0
    return pose, written, fts, undecided


def check_caps(undecided, what=""):
    assert not undecided.any(), f"{what}: {int(undecided.sum())} elements sit on a decision a last bit could flip, first {np.argwhere(undecided)[:3].tolist()}"


def rk4_arc_rows(q, tick_t, n_rows, substeps):
    """x' = v cos(yaw), y' = v sin(yaw), yaw' = kappa v, v' = a with v clamped at 0: classical RK4, `substeps` steps per tick, carried
    from row to row -> [(x, y, yaw)] at tau = r * tick_t, r = 0 .. n_rows - 1.  A step that straddles the stop (the right-hand side has
    a kink there) is cut in two at it."""
    import math

    x, y, yaw, v0, a, kappa = (float(c) for c in q)
    v0 = max(v0, 0.0)
    t_stop = v0 / (-a) if a < 0 else math.inf
    speed = lambda t: v0 + a * t if t < t_stop else 0.0

    def step(t, h, x, y, yaw):
        va, vm, vb = speed(t), speed(t + h / 2), speed(min(t + h, t_stop) if t < t_stop else t + h)
        k1 = (va * math.cos(yaw), va * math.sin(yaw), kappa * va)
        y2 = yaw + h / 2 * k1[2]
        k2 = (vm * math.cos(y2), vm * math.sin(y2), kappa * vm)
        y3 = yaw + h / 2 * k2[2]
        k3 = (vm * math.cos(y3), vm * math.sin(y3), kappa * vm)
        y4 = yaw + h * k3[2]
        k4 = (vb * math.cos(y4), vb * math.sin(y4), kappa * vb)
        return (x + h / 6 * (k1[0] + 2 * k2[0] + 2 * k3[0] + k4[0]), y + h / 6 * (k1[1] + 2 * k2[1] + 2 * k3[1] + k4[1]),
                yaw + h / 6 * (k1[2] + 2 * k2[2] + 2 * k3[2] + k4[2]))

    rows = [(x, y, yaw)]
    for r in range(1, n_rows):
        t_a, t_b = (r - 1) * tick_t, r * tick_t
        h = (t_b - t_a) / substeps
        for i in range(substeps):
            t = t_a + i * h
            if t < t_stop < t + h:
                x, y, yaw = step(t, t_stop - t, x, y, yaw)
                x, y, yaw = step(t_stop, t + h - t_stop, x, y, yaw)
            else:
                x, y, yaw = step(t, h, x, y, yaw)
        rows.append((x, y, yaw))
    return rows
