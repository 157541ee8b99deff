"""CPU: tests/exact_cost.py (CostFunction.cost_total in exact rational arithmetic) against the reference's own values in the golden
fixtures and against the CPU oracle, under the relative bar the GPU edge tests hold the kernels to (|cost - exact| <= 1e-12 max(1, |exact|)).
A reference that does not meet its own bar would make the GPU comparisons meaningless."""
from fractions import Fraction

import numpy as np

import exact_cost as X
from conftest import batch_from_golden, load_golden


def test_time_samples_are_numpys():
    for T, tick in ((8.0, 0.1), (10.0, 0.05), (12.8, 0.1), (12.85, 0.1), (25.6, 0.1), (25.55, 0.1), (0.1, 0.1), (0.3, 0.1)):
        want = np.arange(0.0, T, tick)
        N = X.arange_len(T, tick)
        assert N == len(want), (T, tick)
        assert [Fraction(v) for v in want] == list(X.time_samples(N, tick))


def test_power_sums_match_point_by_point_sums():
    ts = X.time_samples(7, 0.1)
    for k, S in enumerate(X.power_sums(7, 0.1)):
        assert S == sum(t ** k for t in ts)


def test_boundary_value_coefficients_g1(oracle):
    """Exact BVP solutions vs np.linalg.solve (the fixture) and the oracle's closed forms: every term a_k T^k within the bar."""
    g = load_golden("g1_poly.npz")
    for row, ref in zip(g["quintic_in"], g["quintic_coef"]):
        ex, T = X.quintic(*row), Fraction(float(row[6]))
        for got in (ref, oracle.quintic_coefs(*row)):
            for k in range(6):
                term = ex[k] * T ** k
                assert abs(Fraction(float(got[k])) * T ** k - term) <= Fraction(X.REL_BAR) * max(1, abs(term)), (row, k)
    for row, ref in zip(g["quartic_in"], g["quartic_coef"]):
        ex, T = X.quartic(*row), Fraction(float(row[5]))
        for got in (ref, oracle.quartic_coefs(*row)):
            for k in range(5):
                term = ex[k] * T ** k
                assert abs(Fraction(float(got[k])) * T ** k - term) <= Fraction(X.REL_BAR) * max(1, abs(term)), (row, k)


def test_cost_of_g1_polynomials(oracle):
    """Candidates built from G1's boundary data (lateral start + end offset + horizon of a quintic row, longitudinal start + end speed of a
    quartic row): the oracle's point-by-point cost within the bar of the exact one, at tick 0.1 and 0.05."""
    g = load_golden("g1_poly.npz")
    n = 0
    for qi, qa in zip(g["quintic_in"], g["quartic_in"]):
        ego = [qa[0], qa[1], qa[2], qi[0], qi[1], qi[2]]
        d_end, v_end, T = float(qi[3]), float(qa[3]), float(qi[6])
        for tick in (0.1, 0.05):
            ex = X.cost_total(ego, d_end, v_end, T, tick, 13.4112)
            pr = oracle.Problem(d_samples=[d_end], v_samples=[v_end], t_samples=[T], tick_t=tick, target_speed=13.4112, veh_l=5.0, veh_w=2.0,
                                max_speed=1e3, max_accel=1e3, ego=ego, knots=np.linspace(0.0, 1e4, 5), coef_x=np.zeros((4, 5)), coef_y=np.zeros((4, 5)))
            r = pr.eval_traj(d_end, v_end, T, collision=False)
            assert r.N == X.arange_len(T, tick)
            assert X.rel_err(r.cost, ex) <= X.REL_BAR, (ego, d_end, v_end, T, tick, r.cost, float(ex))
            n += 1
    assert n == 2 * len(g["quintic_in"])


def test_cost_table_g13(oracle):
    """G13 (tick 0.05, 160-200 points): the reference's cost of every candidate (the fixture) and the oracle's, within the bar of the
    exact cost."""
    g = load_golden("g13_tick005.npz")
    batch = batch_from_golden(g, "tick005_in_")
    ref = g["tick005_cost"]
    for e, pr in enumerate(oracle.problems_from_batch(batch)):
        o = pr.fop_plan().cost
        for c in range(batch.C):
            iv, it, i_d = c % batch.nv, (c // batch.nv) % batch.nt, c // (batch.nv * batch.nt)
            ex = X.cost_total(batch.ego[e], batch.d_samples[i_d], batch.v_samples[e, iv], batch.t_samples[it], batch.tick_t, batch.target_speed[e])
            assert X.rel_err(ref[e, c], ex) <= X.REL_BAR, (e, c, ref[e, c], float(ex))
            assert X.rel_err(o[c], ex) <= X.REL_BAR, (e, c, o[c], float(ex))
