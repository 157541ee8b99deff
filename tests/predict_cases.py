"""The inputs of the obstacle-prediction tests (test_predict_cpu.py checks on the CPU that none of them sits on a decision a last bit
could flip; test_gpu_predict.py runs them).  Every case: a dict of fp_obstacles_predict's arguments + `ref`, predict_ref.predict of them."""
import functools
from types import SimpleNamespace

import numpy as np
import predict_ref as R

from fiss_plus_planner_amd.spline import build_frames

TICK = 0.1
SWEEP = [(n, T, nx) for n in (1, 5, 64, 67) for T in (7, 50, 130) for nx in (81, 220)]


def frames(nx: int, seed: int = 0):
    """Two reference lines over the same 400 m road: one of nx knots, one of nx - 13 (its rows +inf padded as ProblemBatch pads them)."""
    rng = np.random.default_rng([77, nx, seed])
    knots = np.full((2, nx), np.inf)
    coef = np.zeros((2, 8, nx))
    n_of = np.array([nx, nx - 13], dtype=np.int32)
    for f in range(2):
        xs = np.linspace(0.0, 400.0, int(n_of[f]))
        pts = np.stack([xs, rng.uniform(2, 8) * np.sin(xs / rng.uniform(30, 80))], axis=1)
        k, c = build_frames(pts[None])
        knots[f, :n_of[f]] = k[0]
        coef[f, :, :n_of[f]] = c[0]
    return n_of, knots, coef


def shape_of(case):
    """What FrenetEngine.predict_obstacles reads of a batch."""
    return SimpleNamespace(S=case["model"].shape[0], T_obs=case["T_obs"], n_obs=case["model"].shape[1], nx=case["nx"], knots=case["knots"], coef=case["coef"],
                           tick_t=case["tick_t"])


def finish(model, state, frame_of_scene, t0, n_rows, T_obs, nx, knots, coef, tick_t=TICK):
    case = dict(model=np.ascontiguousarray(model, dtype=np.int32), state=np.ascontiguousarray(state, dtype=np.float64),
                frame_of_scene=None if frame_of_scene is None else np.ascontiguousarray(frame_of_scene, dtype=np.int32),
                t0=np.ascontiguousarray(np.broadcast_to(np.asarray(t0, dtype=np.int32), (np.shape(model)[0],))), n_rows=int(n_rows), T_obs=int(T_obs), nx=nx, knots=knots,
                coef=coef, tick_t=tick_t)
    pose, written, fts, undecided = R.predict(case["model"], case["state"], case["frame_of_scene"], case["t0"], n_rows, T_obs, tick_t, nx, knots, coef)
    case["ref"] = SimpleNamespace(pose=pose, written=written, fts=fts, undecided=undecided)
    return case


def random_tracks(rng, S, n):
    """All three models mixed inside every scene (n >= 3), LANE along the line with some running off its end, ARC of every curvature class."""
    model = rng.integers(0, 3, size=(S, n)).astype(np.int32)
    for s in range(S):
        if n >= 3:
            model[s, rng.permutation(n)[:3]] = (R.NONE, R.LANE, R.ARC)
        else:
            model[s, 0] = (R.LANE, R.ARC, R.NONE)[s % 3]
    state = np.zeros((S, n, 6))
    lane = np.stack([rng.uniform(10, 200, (S, n)), rng.uniform(-4, 4, (S, n)), rng.uniform(-1, 12, (S, n)), rng.uniform(-2, 1, (S, n)),
                     rng.uniform(-9, 9, (S, n)), rng.uniform(-9, 9, (S, n))], axis=-1)  # (the last two are not read)
    kappa = np.where(rng.uniform(size=(S, n)) < 0.5, rng.choice([0.0, 1e-7, -1e-7, 0.02, -0.02, 0.2, -0.2], size=(S, n)), rng.uniform(-0.1, 0.1, (S, n)))
    arc = np.stack([rng.uniform(-100, 100, (S, n)), rng.uniform(-100, 100, (S, n)), rng.uniform(-np.pi, np.pi, (S, n)), rng.uniform(-1, 15, (S, n)),
                    rng.uniform(-3, 2, (S, n)), kappa], axis=-1)
    state[model == R.LANE] = lane[model == R.LANE]
    state[model == R.ARC] = arc[model == R.ARC]
    state[model == R.NONE] = rng.uniform(-5, 5, (S, n, 6))[model == R.NONE]
    return model, state


@functools.lru_cache(maxsize=None)
def sweep(n, T, nx):
    rng = np.random.default_rng([4242, n, T, nx])
    model, state = random_tracks(rng, 3, n)
    return finish(model, state, [0, 1, 0], [0, 2, -1], T, T, *frames(nx))


@functools.lru_cache(maxsize=None)
def row_range(t0_kind: int):
    """t0 in {0, 3, -2, T_obs - 1, T_obs + 4} with n_rows that runs past T_obs (scene 1 carries the t0 under test, scenes 0 / 2 others)."""
    T = 23
    t0 = (0, 3, -2, T - 1, T + 4)[t0_kind]
    rng = np.random.default_rng([99, t0_kind])
    model, state = random_tracks(rng, 3, 5)
    return finish(model, state, [1, 0, 0], [1, t0, -T - 3], T + 9, T, *frames(81))


@functools.lru_cache(maxsize=None)
def stops():
    """Braking to a stop strictly between two rows (v / -a = 0.25 s) and on a row (exactly 2 ticks: 0.5 / 2.5 = 0.2 = 2 * 0.1 in
    doubles), both models; v < 0 next to its v = 0 twin."""
    assert 0.5 / 2.5 == 2 * TICK
    lane = lambda s0, d, v, a: [s0, d, v, a, 0, 0]
    arc = lambda v, a, k: [3.0, -4.0, 0.7, v, a, k]
    state = np.array([[lane(50, 1.5, 0.5, -2.0), lane(50, 1.5, 0.5, -2.5), lane(60, -2, -3.0, 0.5), lane(60, -2, 0.0, 0.5),
                       arc(0.5, -2.0, 0.05), arc(0.5, -2.5, 0.05), arc(-3.0, 0.5, -0.1), arc(0.0, 0.5, -0.1), arc(-2.0, -1.0, 0.1), lane(70, 0, -2.0, -1.0)]])
    model = np.array([[1, 1, 1, 1, 2, 2, 2, 2, 2, 1]])
    return finish(model, state, [0], [0], 12, 12, *frames(81))


@functools.lru_cache(maxsize=None)
def line_ends():
    """A LANE track that runs off the last knot mid-horizon, one that starts before the first knot and enters, one off the line throughout;
    s stays at least 1e-3 m from either end at every row (v = 7.3 m/s: 0.73 m per row)."""
    nx, knots, coef = frames(81)
    last = float(knots[0, nx[0] - 1])
    state = np.zeros((1, 4, 6))
    state[0, 0, :4] = (last - 10.0 - 0.211, 1.0, 7.3, 0.0)
    state[0, 1, :4] = (-10.0 - 0.211, -1.0, 7.3, 0.0)
    state[0, 2, :4] = (last + 5.0, 0.0, 1.0, 0.0)
    state[0, 3, :4] = (100.0, 2.0, 7.3, 0.0)
    return finish(np.ones((1, 4), dtype=np.int32), state, [0], [0], 40, 40, nx, knots, coef)


@functools.lru_cache(maxsize=None)
def arc_branch():
    """u = kappa l / 2 either side of 1e-4 by a factor 2 and by 1e-3 of it (at the last row, l = 11 m: no earlier row lands on the
    branch point), kappa = 0 exactly, negative kappa."""
    k_of = lambda u_end: 2.0 * u_end / 11.0
    kap = [k_of(5e-5), k_of(2e-4), k_of(-5e-5), k_of(-2e-4), 0.0, -0.3, 0.3, k_of(1e-4 * 0.999), k_of(1e-4 * 1.001)]
    state = np.array([[[1.0, 2.0, 0.3, 10.0, 0.0, k] for k in kap]])
    return finish(np.full((1, len(kap)), 2, dtype=np.int32), state, None, [0], 12, 12, *frames(81))


@functools.lru_cache(maxsize=None)
def frames_shared(frame_of_scene=(0, 0, 1)):
    rng = np.random.default_rng(5150)
    model, state = random_tracks(rng, 3, 6)
    return finish(model, state, None if frame_of_scene is None else list(frame_of_scene), [0, 0, 0], 20, 20, *frames(81))


def all_cases_lazy():
    """(name, thunk) of every input the GPU tests feed to the kernel."""
    out = [(f"sweep{key}", functools.partial(sweep, *key)) for key in SWEEP]
    out += [(f"row_range[{k}]", functools.partial(row_range, k)) for k in range(5)]
    out += [("stops", stops), ("line_ends", line_ends), ("arc_branch", arc_branch), ("frames_shared", frames_shared),
            ("frames_out_of_range", functools.partial(frames_shared, (0, 7, -1))), ("frames_null", functools.partial(frames_shared, None))]
    return out


CASE_NAMES = [name for name, _ in all_cases_lazy()]
