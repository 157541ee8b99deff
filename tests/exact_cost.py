"""Exact reference of CostFunction.cost_total (reference planners/common/cost/cost_function.py:29-50) in rational arithmetic.

The inputs are the doubles a planner hands over (start state, end state, horizon, tick); from there on nothing is rounded:

* the quintic / quartic boundary-value problems (planners/common/geometry/polynomial.py:5-19, 45-62) are solved exactly;
* the time samples are the doubles np.arange(0.0, T, tick) produces (0.0 + i * tick, rounded once), so N = len(np.arange(...)) and
  `cost_time = 10.0 - t[-1]` use the same t[-1] as the reference;
* every sum of squares is sum_i p(t_i)^2 = sum_k (p * p)_k S_k with the exact power sums S_k = sum_i t_i^k - equal, as rationals, to the
  reference's point-by-point sums taken without rounding; the terms are combined in the reference's grouping.

A helper module for the tests (test_exact_cost_cpu.py, test_gpu_edges.py), not a conftest.
"""
from __future__ import annotations

import math
from fractions import Fraction
from functools import lru_cache

import numpy as np

# CostFunction("WX1") weights as the doubles the reference multiplies by (cost_function.py:6-12) and the 10.0 of cost_time (:42)
W_V, W_A, W_J, W_LC, HORIZON = (Fraction(w) for w in (1.0, 0.1, 0.1, 10.0, 10.0))


def arange_len(T: float, tick: float) -> int:
    """len(np.arange(0.0, T, tick)) = ceil(T / tick) evaluated in double (what the kernels and the oracle use)."""
    n = math.ceil(float(T) / float(tick))
    return max(n, 0)


def quintic(xs, vxs, axs, xe, vxe, axe, T):
    """Exact a0..a5 of QuinticPolynomial (polynomial.py:45-62) for double inputs."""
    xs, vxs, axs, xe, vxe, axe, T = (Fraction(float(v)) for v in (xs, vxs, axs, xe, vxe, axe, T))
    a0, a1, a2 = xs, vxs, axs / 2
    D = xe - a0 - a1 * T - a2 * T ** 2
    V = vxe - a1 - 2 * a2 * T
    A = axe - 2 * a2
    # the 3x3 system [[T^3, T^4, T^5], [3T^2, 4T^3, 5T^4], [6T, 12T^2, 20T^3]] a = (D, V, A), solved in closed form
    a3 = (20 * D - 8 * V * T + A * T ** 2) / (2 * T ** 3)
    a4 = (-30 * D + 14 * V * T - 2 * A * T ** 2) / (2 * T ** 4)
    a5 = (12 * D - 6 * V * T + A * T ** 2) / (2 * T ** 5)
    assert a3 * T ** 3 + a4 * T ** 4 + a5 * T ** 5 == D and 3 * a3 * T ** 2 + 4 * a4 * T ** 3 + 5 * a5 * T ** 4 == V
    assert 6 * a3 * T + 12 * a4 * T ** 2 + 20 * a5 * T ** 3 == A
    return [a0, a1, a2, a3, a4, a5]


def quartic(xs, vxs, axs, vxe, axe, T):
    """Exact a0..a4 of QuarticPolynomial (polynomial.py:5-19) for double inputs."""
    xs, vxs, axs, vxe, axe, T = (Fraction(float(v)) for v in (xs, vxs, axs, vxe, axe, T))
    a0, a1, a2 = xs, vxs, axs / 2
    V = vxe - a1 - 2 * a2 * T
    A = axe - 2 * a2
    a3 = (3 * V - A * T) / (3 * T ** 2)
    a4 = (A * T - 2 * V) / (4 * T ** 3)
    assert 3 * a3 * T ** 2 + 4 * a4 * T ** 3 == V and 6 * a3 * T + 12 * a4 * T ** 2 == A
    return [a0, a1, a2, a3, a4]


def derivative(c):
    return [k * c[k] for k in range(1, len(c))]


def _square(c):
    out = [Fraction(0)] * (2 * len(c) - 1)
    for i, a in enumerate(c):
        for j, b in enumerate(c):
            out[i + j] += a * b
    return out


@lru_cache(maxsize=64)
def time_samples(N: int, tick: float):
    """The N doubles np.arange(0.0, T, tick) holds (0.0 + i * tick, one rounding) as exact rationals."""
    return tuple(Fraction(v) for v in np.arange(N, dtype=np.float64) * float(tick))


@lru_cache(maxsize=64)
def power_sums(N: int, tick: float):
    """S_k = sum_{i<N} t_i^k, k = 0..10, exactly."""
    ts = time_samples(N, tick)
    S = []
    for k in range(11):
        S.append(sum((t ** k for t in ts), Fraction(0)))
    return tuple(S)


def sum_of_squares(c, S) -> Fraction:
    """sum_i p(t_i)^2 for the polynomial with coefficients c (a0 first)."""
    return sum((q * S[k] for k, q in enumerate(_square(c))), Fraction(0))


def cost_terms(ego, d_end, v_end, T, tick, target_speed):
    """(N, dict of the six sums) of one Frenet candidate: lateral quintic (d, d_d, d_dd) -> (d_end, 0, 0), longitudinal quartic
    (s, s_d, s_dd) -> (v_end, 0), both over T (frenet_optimal_planner.py:79-99, fiss_planner.py:113-130)."""
    N = arange_len(T, tick)
    S = power_sums(N, float(tick))
    lat = quintic(ego[3], ego[4], ego[5], d_end, 0.0, 0.0, T)
    lon = quartic(ego[0], ego[1], ego[2], v_end, 0.0, T)
    lon_v = derivative(lon)
    lon_v[0] -= Fraction(float(target_speed))
    sums = dict(speed=sum_of_squares(lon_v, S), acc_s=sum_of_squares(derivative(derivative(lon)), S),
                acc_d=sum_of_squares(derivative(derivative(lat)), S), jerk_s=sum_of_squares(derivative(derivative(derivative(lon))), S),
                jerk_d=sum_of_squares(derivative(derivative(derivative(lat))), S), offset=sum_of_squares(lat, S))
    return N, sums


def cost_total(ego, d_end, v_end, T, tick, target_speed) -> Fraction:
    """CostFunction.cost_total of the candidate, exactly (cost_function.py:41-50)."""
    N, s = cost_terms(ego, d_end, v_end, T, tick, target_speed)
    if N == 0:
        raise ValueError("empty trajectory (T <= 0)")
    cost_time = HORIZON - time_samples(N, float(tick))[-1]
    cost_obstacle = Fraction(0)
    cost_speed = W_V * s["speed"]
    cost_accel = W_A * s["acc_s"] + W_A * s["acc_d"]
    cost_jerk = W_J * s["jerk_s"] + W_J * s["jerk_d"]
    cost_offset = W_LC * s["offset"]
    return (cost_time + cost_obstacle + cost_speed + cost_accel + cost_jerk + cost_offset) / N


def rel_err(got, exact: Fraction) -> float:
    """|got - exact| / max(1, |exact|) in exact arithmetic (inf for a non-finite `got`)."""
    got = float(got)
    if not math.isfinite(got):
        return math.inf
    return float(abs(Fraction(got) - exact) / max(Fraction(1), abs(exact)))


REL_BAR = 1e-12  # |cost - exact| <= REL_BAR * max(1, |exact|)
