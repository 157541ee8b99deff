// frenet_rules.h - the per-point predicates of the four rule passes (fp_speed_envelope, fp_gate_mask, fp_boundary_mask, fp_gap_mask),
// shared by the table kernels that run them over a dense call's candidates and by rules_eval_kernel (frenet_rules_eval.hip), which runs
// them over explicit end states.  Each function is the text its pass kernel held inline: one definition, one arithmetic, the same bits
// on both sides.  The definitions: include/frenet_gpu.h.
#pragma once

#include "frenet_device.h"
#include "frenet_kernels.h"
#include "frenet_ego.h"
#include "frenet_project.h"

namespace fp {

// ---- fp_speed_envelope: point t of the longitudinal profile `lon`.  sp = the line's knots (and, for the lateral check, its
// coefficient columns [8][nx]), lim[k] = the limit of the segment that starts at knot k.  fast = violation A, lat = violation B.
__device__ __forceinline__ void envelope_point(const SplineLds& sp, const double* lim, double guess_scale, const Quartic& lon, double t, double front,
                                               double tol, int lateral, double max_lat, bool& fast, bool& lat)
{
    double s, s_d, unused_a, unused_j;
    quartic_eval(lon, t, s, s_d, unused_a, unused_j);
    const double s_q = s + front;
    int k = spline_segment_clamped(sp, s_q, guess_scale);
    fast = s_d > lim[k] + tol;  // (+inf, and a NaN, compare false: no limit there)
    if (lateral) {
        const int nx = sp.nx;
        k = spline_segment_clamped(sp, s, guess_scale);
        const double dx = s - sp.knots[k];
        const double* c = sp.coef + k;
        const double bx = c[nx], cx = c[2 * nx], dx3 = c[3 * nx], by = c[5 * nx], cy = c[6 * nx], dy3 = c[7 * nx];
        const double gx = fma(fma(3.0 * dx3, dx, 2.0 * cx), dx, bx), gy = fma(fma(3.0 * dy3, dx, 2.0 * cy), dx, by);
        const double hx = fma(6.0 * dx3, dx, 2.0 * cx), hy = fma(6.0 * dy3, dx, 2.0 * cy);
        const double g2 = fma(gx, gx, gy * gy);
        const double kappa = fma(gx, hy, -(gy * hx)) / (g2 * sqrt(g2));
        lat = s_d * s_d * fabs(kappa) > max_lat;
    }
}

// ---- fp_gate_mask
// the dilemma zone: the ego (bumper at q0, speed s_d0) is in front of the line g and cannot stop there any more
__device__ __forceinline__ bool gate_waived(double max_decel, double s_d0, double q0, double g)
{
    return max_decel > 0.0 && s_d0 > 0.0 && q0 <= g && q0 + s_d0 * s_d0 / (2.0 * max_decel) > g;
}
// the closed word of absolute step t (before step 0 the first, at or after T_gate the last known state holds)
__device__ __forceinline__ uint32_t gate_word(const uint32_t* closed, long long t, int t_last)
{
    return closed[t < 0 ? 0 : (t > t_last ? t_last : (int)t)];
}
// point i >= 1 of the profile against the gates whose bit is set in w (live and closed at the arrival step); line[g] = the gate's
// arclength, NaN for a slot that is unused or waived
__device__ __forceinline__ bool gate_point(const Quartic& lon, int i, double tick, double front, double q0, uint32_t w, const double* line)
{
    bool hit = false;
    const double q_prev = i == 1 ? q0 : quartic_pos(lon, (double)(i - 1) * tick) + front;
    const double q = quartic_pos(lon, (double)i * tick) + front;
    while (w) {
        const double g = line[__builtin_ctz(w)];
        w &= w - 1u;
        hit = hit || (q_prev <= g && g < q);
    }
    return hit;
}

// ---- fp_boundary_mask
// the corridor of one frame as the kernels hold it: per segment the edge at the segment's first knot and its slope in s, for both
// sides (a segment with a knot value that is not finite: +-inf with slope 0, it cannot be violated)
__device__ __forceinline__ void stage_corridor(const double* gk, const double* gl, const double* gr, int nx, double* knots, double* l0, double* l1,
                                               double* r0, double* r1, int tid, int nth)
{
    for (int i = tid; i < nx; i += nth) {
        const double k0 = gk[i];
        if (knots) knots[i] = k0;
        if (i + 1 < nx) {
            const double inv = 1.0 / (gk[i + 1] - k0);
            const double la = gl[i], lb = gl[i + 1], ra = gr[i], rb = gr[i + 1];
            const bool lfin = finite_f64(la) && finite_f64(lb), rfin = finite_f64(ra) && finite_f64(rb);
            l0[i] = lfin ? la : __builtin_inf();
            l1[i] = lfin ? (lb - la) * inv : 0.0;
            r0[i] = rfin ? ra : -__builtin_inf();
            r1[i] = rfin ? (rb - ra) * inv : 0.0;
        }
    }
}
// point t of the candidate (lon, lat): does the lateral extent of its footprint cross an edge
__device__ __forceinline__ bool boundary_point(const SplineLds& sp, const double* l0, const double* l1, const double* r0, const double* r1,
                                               double guess_scale, const Quartic& lon, const Quintic& lat, double t, double hw, double hl, double margin)
{
    double s, s_d, d, d_d, unused_a, unused_j;
    quartic_eval(lon, t, s, s_d, unused_a, unused_j);
    quintic_eval(lat, t, d, d_d, unused_a, unused_j);
    const int k = spline_segment_clamped(sp, s, guess_scale);  // (a point below M lies on the line)
    const double ds = s - sp.knots[k];
    const double L = fma(l1[k], ds, l0[k]), R = fma(r1[k], ds, r0[k]);
    const double r = hypot(s_d, d_d);
    const double h = r == 0.0 ? hw : (hw * fabs(s_d) + hl * fabs(d_d)) / r;
    return (d + h) + margin > L || (d - h) - margin < R;
}

// ---- fp_gap_mask
// centre distance beyond which an ego box of circumradius r_e and column j cannot touch, widened past any rounding of the compare
__device__ __forceinline__ double gap_reach(const EgoCtx& e, double r_e, int j) { return (r_e + e.obs_dim[4 * j + 2]) * (1.0 + 1e-9) + 1e-9; }
// grid poses q = i / cs the ego's horizon and table hold (stage_ego's row count): q < G <=> q cs < final_time_step - t_now, the call's
// points and T_obs - t_now
__device__ __forceinline__ int gap_grid_poses(const fp_params& p, const EgoCtx& e)
{
    int G = 0;
    if (e.n_obs > 0) {
        const int cs = p.check_stride;
        int hmax = e.horizon_cap < points_cap(p) ? e.horizon_cap : points_cap(p);
        if (hmax < 0) hmax = 0;
        G = (hmax + cs - 1) / cs;
        const int in_table = e.T_obs - e.t_now;
        const int rows_tab = in_table > 0 ? (in_table + cs - 1) / cs : 0;
        if (rows_tab < G) G = rows_tab;
    }
    return G;
}
// the ego footprint `ego` at grid pose q (point q cs) of a plan with n_pose grid poses: does it overlap a column at a paired row
// (q - Lf .. q + Ll, q itself left out: lag 0 is the collision check's).  The lane takes the columns sub, sub + split, ...; bound = the
// cull table [G][n_obs] or nullptr.
__device__ __forceinline__ bool gap_pose_hit(const KernelArgs& ka, const EgoCtx& e, const Obb& ego, int q, int n_pose, int Lf, int Ll, int sub, int split,
                                             const float4* bound, double r_e, int cs, int n_obs)
{
    bool hit = false;
    const int lo = q - Lf > 0 ? q - Lf : 0, hi = q + Ll < n_pose - 1 ? q + Ll : n_pose - 1;
    for (int j = sub; j < n_obs && !hit; j += split) {
        if (bound) {
            const float4 bb = bound[q * n_obs + j];
            if (!(ego.x >= (double)bb.x && ego.x <= (double)bb.z && ego.y >= (double)bb.y && ego.y <= (double)bb.w)) continue;
        }
        const double R = gap_reach(e, r_e, j);
        for (int qr = lo; qr <= hi; ++qr) {
            if (qr == q) continue;  // lag 0 is the collision check's
            const double* row = obs_row(e, qr * cs, cs);
            double ox, oy, oc, os;
            if (!row || !obs_centre(e, row, j, ox, oy)) continue;
            const double dx = ox - ego.x, dy = oy - ego.y;
            if (!(fma(dx, dx, dy * dy) <= R * R)) continue;
            obs_heading(e, row, j, oc, os);
            const int nvert = obs_nvert(ka, e, j);
            hit = nvert > 0 ? poly_overlap(ego, ox, oy, oc, os, obs_ring(ka, e, j), nvert)
                            : obb_overlap(ego, Obb{ox, oy, oc, os, e.obs_dim[4 * j], e.obs_dim[4 * j + 1]});
            if (hit) break;
        }
    }
    return hit;
}

}  // namespace fp
