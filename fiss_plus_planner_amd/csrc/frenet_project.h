// frenet_project.h - the per-ego scalar rules of the Cartesian -> Frenet projection (FrenetState.from_state, reference
// common/scenario/frenet.py:32-99), shared by from_state_kernel (frenet_frame.hip) and the host checks of fp_from_state
// (frenet_abi.hip).  Plain C++ and <cmath> only: a host compiler builds it without any HIP header (tests/test_project_cpu.py runs
// every rule on a machine without a GPU, under the sanitizers too).
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define FP_PROJECT_HD __host__ __device__
#else
#define FP_PROJECT_HD
#endif

namespace fp {

constexpr double kProjectPi = 3.141592653589793;
constexpr double kProjectStep = 0.1;  // generate_frenet_frame resamples the line every 0.1 m (frenet_optimal_planner.py:274)
// project_unify_angle walks at most this far (3979 turns): a larger difference is not a heading any more
constexpr double kProjectUnifyMax = 25000.0;

FP_PROJECT_HD inline double project_nan() { return __builtin_nan(""); }

// The library's one "finite" (NaN and +-inf both fail the comparison): the kernels and the host checks of frenet_abi.hip use it too
constexpr double kF64Max = 1.7976931348623157e308;
FP_PROJECT_HD inline bool finite_f64(double v) { return std::fabs(v) <= kF64Max; }

// The state check: x, y, yaw, v all finite.  A NaN position makes every distance comparison false (no nearest point), an infinite
// yaw never leaves the reference's unification loops.
FP_PROJECT_HD inline bool project_state_ok(double x, double y, double yaw, double v)
{
    return finite_f64(x) && finite_f64(y) && finite_f64(yaw) && finite_f64(v);
}

// Number of resampled points of a line of arclength s_last: len(np.arange(0, s_last, 0.1)) = ceil(s_last / 0.1), reduced while the
// last sampled arclength (n - 1) * 0.1 would reach s_last - the quotient rounds up across an integer when s_last is within an ulp of
// a multiple of 0.1 (3 * 0.1 = 0.30000000000000004: ceil gives 4 and 3 * 0.1 == s_last), and the spline has no segment at s_last
// (the reference raises IndexError there; here the line loses that one point).  Every sampled arclength i * 0.1, i < n, is < s_last.
// 0 = unusable: s_last is not finite, the count does not fit an int, or fewer than two points remain (s_last <= 0.1: the reference
// indexes past its one-point polyline).
FP_PROJECT_HD inline int project_point_count(double s_last)
{
    if (!finite_f64(s_last) || !(s_last > 0.0)) return 0;
    const double c = std::ceil(s_last / kProjectStep);
    if (!(c < 2147483647.0)) return 0;
    int n = (int)c;
    while (n > 0 && (double)(n - 1) * kProjectStep >= s_last) --n;  // (one step at the most: the quotient is off by an ulp)
    return n >= 2 ? n : 0;
}

// find_next_point_idx (frenet.py:38-56): the angle between the ego's yaw and the direction to the nearest point, folded to
// [.., pi] ...
FP_PROJECT_HD inline double project_fold_angle(double yaw, double heading)
{
    const double angle = std::fabs(yaw - heading);
    return std::fmin(2.0 * kProjectPi - angle, angle);
}

// ... the nearest point lies behind the ego (angle > pi/2): the next waypoint is the one after it.  Clamped to 1 .. n - 1 (n >= 2).
FP_PROJECT_HD inline int project_next_idx(int nearest, int n, double angle)
{
    int next = angle > kProjectPi / 2.0 ? nearest + 1 : nearest;
    if (next < 1) next = 1;
    else if (next >= n) next = n - 1;
    return next;
}

FP_PROJECT_HD inline int project_prev_idx(int next) { return next - 1 > 0 ? next - 1 : 0; }

// unifyAngleRange (math_utils.py:28-34): the reference's two loops, bit for bit, for |angle| <= kProjectUnifyMax (they end within
// 3979 steps).  Beyond that, and for NaN and +-inf (where the reference never returns), the result is NaN at once.
FP_PROJECT_HD inline double project_unify_angle(double angle)
{
    if (!(std::fabs(angle) <= kProjectUnifyMax)) return project_nan();
    while (angle > kProjectPi) angle -= 2.0 * kProjectPi;
    while (angle < -kProjectPi) angle += 2.0 * kProjectPi;
    return angle;
}

// Projection of the state on the segment prev -> next and the sign rule (frenet.py:58-99): out = s_d, d, d_d.
// (p_x, p_y, p_yaw): the previous waypoint and the line's yaw there; (q_x, q_y): the next waypoint.
FP_PROJECT_HD inline void project_on_segment(double x, double y, double yaw, double v, double p_x, double p_y, double p_yaw, double q_x, double q_y,
                                             double* s_d, double* d_out, double* d_d)
{
    const double n_x = q_x - p_x, n_y = q_y - p_y;
    const double x_x = x - p_x, x_y = y - p_y;
    const double x_yaw = std::atan2(x_y, x_x);
    const double proj = (x_x * n_x + x_y * n_y) / (n_x * n_x + n_y * n_y);
    double d = std::hypot(x_x - proj * n_x, x_y - proj * n_y);
    const double delta = project_unify_angle(yaw - p_yaw);
    if (p_yaw <= x_yaw) d = -d;  // :82-83
    *s_d = v * std::cos(delta);
    *d_out = d;
    *d_d = v * std::sin(delta);
}

}  // namespace fp
