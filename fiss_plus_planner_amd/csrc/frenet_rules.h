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

// ---- the four rules on one explicit trajectory, evaluated by a whole wavefront (rules_eval_kernel per end state, the fallback
// kernel's rule instance per candidate, the FISS+ refinement's rule instance per popped candidate): the tables a workgroup stages once
// per ego, the call's constants, and the evaluation.
constexpr int kRulesSplit = 8;  // at most this many lanes share one pose's columns (the gaps)

// The rules' own tables in LDS, behind stage_ego's layout at a.off_lim / off_edge / off_gate (doubles): limits [NX] | l0, l1, r0, r1
// [NX] each | gate lines [FP_MAX_GATES], closed words [points_cap].  closed = the frame's words in global memory (a point beyond the cap).
struct RuleTables {
    double *lim, *l0, *l1, *r0, *r1, *line;
    uint32_t* word;
    const uint32_t* closed;
};
// doubles the tables of the rules in `on` take
__host__ __device__ inline long rule_table_doubles(uint32_t on, const fp_params& p, int NX)
{
    long own = 0;
    if (on & FP_RULE_LIMIT) own += NX;
    if (on & FP_RULE_BOUNDARY) own += 4L * NX;
    if (on & FP_RULE_GATE) own += FP_MAX_GATES + (points_cap(p) + 1) / 2;
    return own;
}
// where each table starts when the layout before them ends at `off` doubles
inline void rule_table_offsets(RulesEvalArgs& a, int off, int NX)
{
    a.off_lim = off;
    if (a.on & FP_RULE_LIMIT) off += NX;
    a.off_edge = off;
    if (a.on & FP_RULE_BOUNDARY) off += 4 * NX;
    a.off_gate = off;
}
// the tables of ego b in the layout that starts at lds (every wavefront of the workgroup: the addresses alone)
__device__ __forceinline__ RuleTables rule_tables(const KernelArgs& ka, const RulesEvalArgs& a, int b, double* lds)
{
    const int NX = ka.b.NX;
    RuleTables t;
    t.lim = lds + a.off_lim;
    t.l0 = lds + a.off_edge;
    t.l1 = t.l0 + NX;
    t.r0 = t.l1 + NX;
    t.r1 = t.r0 + NX;
    t.line = lds + a.off_gate;
    t.word = (uint32_t*)(t.line + FP_MAX_GATES);
    t.closed = (a.on & FP_RULE_GATE) ? a.closed + (size_t)ka.b.frame_of[b] * a.T_gate : nullptr;
    return t;
}
// Stage them with nth threads of the workgroup, numbered tid = wave * kWave + lane (after stage_ego; the caller's barrier follows): the
// limit of every segment, the corridor (stage_corridor), the gate lines with the waiver folded in - taken from the ego's present state -,
// the mask of the live slots (*s_live, one LDS word, written by wavefront 0) and the closed words of the steps t_now + 1 .. t_now + points_cap.
__device__ __forceinline__ RuleTables stage_rule_tables(const KernelArgs& ka, const RulesEvalArgs& a, int b, const EgoCtx& e, double* lds, uint32_t* s_live,
                                                        int tid, int wave, int lane, int nth)
{
    const int f = ka.b.frame_of[b], nx = e.sp.nx, NX = ka.b.NX;
    const int cap = points_cap(ka.p), t_last = a.T_gate - 1;
    const long long tn = e.t_now;
    const RuleTables t = rule_tables(ka, a, b, lds);
    if (a.on & FP_RULE_LIMIT) {
        const double* gl = a.v_limit + (size_t)f * NX;
        for (int i = tid; i < nx; i += nth) t.lim[i] = i + 1 < nx ? gl[i] : __builtin_inf();  // (the last knot starts no segment)
    }
    if (a.on & FP_RULE_BOUNDARY) stage_corridor(ka.b.knots + (size_t)f * NX, a.left + (size_t)f * NX, a.right + (size_t)f * NX, nx, nullptr, t.l0, t.l1, t.r0, t.r1, tid, nth);
    if (a.on & FP_RULE_GATE) {
        if (wave == 0) {
            double g = __builtin_nan("");
            if (lane < a.gate_stride) {
                g = a.gate_s[(size_t)f * a.gate_stride + lane];
                if (gate_waived(a.max_decel, e.s_d0, e.s0 + a.gate_front, g)) g = __builtin_nan("");
            }
            if (lane < FP_MAX_GATES) t.line[lane] = g;
            const unsigned long long live = __ballot(g == g);
            if (lane == 0) *s_live = (uint32_t)live;
        }
        for (int i = tid; i < cap; i += nth) t.word[i] = gate_word(t.closed, tn + 1 + i, t_last);
    }
    return t;
}

// What the evaluation needs beside the tables and does not depend on the trajectory (after the barrier behind stage_rule_tables)
struct RuleConsts {
    uint32_t live, env_want;
    double guess_scale, hl, hw, r_e, q0;
    int lateral, cap, t_last, cs, Lf, Ll, G, q_first;
    bool gaps_active;
};
__device__ __forceinline__ RuleConsts rule_consts(const KernelArgs& ka, const RulesEvalArgs& a, const EgoCtx& e, const uint32_t* s_live)
{
    const fp_params& p = ka.p;
    RuleConsts c;
    const int nx = e.sp.nx;
    c.live = (a.on & FP_RULE_GATE) ? *s_live : 0u;
    c.lateral = (a.on & FP_RULE_LATERAL) ? 1 : 0;
    c.env_want = FP_FLAG_SPEED | (c.lateral ? FP_FLAG_ACCEL : 0u);
    c.guess_scale = (double)(nx - 1) / (e.sp.knots[nx - 1] - e.sp.knots[0]);
    c.hl = 0.5 * p.veh_l; c.hw = 0.5 * p.veh_w;
    c.r_e = sqrt(fma(c.hl, c.hl, c.hw * c.hw));
    c.q0 = e.s0 + a.gate_front;
    c.cap = points_cap(p); c.t_last = a.T_gate - 1;
    c.cs = p.check_stride;
    c.Lf = a.lag_follow / c.cs; c.Ll = a.lag_lead / c.cs;  // the lags in grid steps: only pairs on the grid exist
    c.G = (a.on & FP_RULE_GAP) ? gap_grid_poses(p, e) : 0;
    c.gaps_active = c.G > 0 && (c.Lf > 0 || c.Ll > 0);
    c.q_first = (a.first - 1) / c.cs + 1 < c.G ? (a.first - 1) / c.cs + 1 : c.G;
    return c;
}

// The trajectory (lon, lat) with points 1 .. M - 1 (2 <= M <= N <= points_cap) and flag word word_in -> the word the rules leave;
// spoke = the FP_RULE_* bits violated.  The rules run in the passes' order; every rule gives the lanes the points 1 + lane, 65 + lane,
// ... < M (the gaps: the grid poses, split like gap_mask_kernel's), __ballot is the verdict and a rule ends on its first hit; the gaps
// run only when the word carries no FP_FLAG_INFEASIBLE bit after the three rules before them.  Wave-uniform in, wave-uniform out.
__device__ __forceinline__ uint32_t wave_rules_eval(const KernelArgs& ka, const RulesEvalArgs& a, const EgoCtx& e, const RuleTables& t, const RuleConsts& c,
                                                    const Quartic& lon, const Quintic& lat, int M, uint32_t word_in, int lane, uint32_t& spoke)
{
    const fp_params& p = ka.p;
    const double tick = p.tick_t;
    const long long tn = e.t_now;
    uint32_t word_new = word_in;
    spoke = 0u;
    if (a.on & FP_RULE_LIMIT) {
        uint32_t bits = 0u;
        for (int i0 = 1; i0 < M; i0 += kWave) {
            const int i = i0 + lane;
            bool fast = false, lat_v = false;
            if (i < M) envelope_point(e.sp, t.lim, c.guess_scale, lon, (double)i * tick, a.env_front, a.env_tol, c.lateral, a.max_lat_accel, fast, lat_v);
            if (__ballot(fast)) bits |= FP_FLAG_SPEED;
            if (__ballot(lat_v)) bits |= FP_FLAG_ACCEL;
            if (bits == c.env_want) break;  // every bit the rule can give is found
        }
        word_new |= bits;
        if (bits & FP_FLAG_SPEED) spoke |= FP_RULE_LIMIT;
        if (bits & FP_FLAG_ACCEL) spoke |= FP_RULE_LATERAL;
    }
    if ((a.on & FP_RULE_GATE) && c.live != 0u) {
        for (int i0 = 1; i0 < M; i0 += kWave) {
            const int i = i0 + lane;
            bool hit = false;
            if (i < M) {
                const uint32_t w = (i <= c.cap ? t.word[i - 1] : gate_word(t.closed, tn + i, c.t_last)) & c.live;
                if (w) hit = gate_point(lon, i, tick, a.gate_front, c.q0, w, t.line);
            }
            if (__ballot(hit)) {
                word_new |= FP_FLAG_SPEED;
                spoke |= FP_RULE_GATE;
                break;
            }
        }
    }
    if (a.on & FP_RULE_BOUNDARY) {
        bool out = false;
        for (int i0 = 1; i0 < M; i0 += kWave) {
            const int i = i0 + lane;
            bool viol = false;
            if (i < M) viol = boundary_point(e.sp, t.l0, t.l1, t.r0, t.r1, c.guess_scale, lon, lat, (double)i * tick, c.hw, c.hl, a.margin);
            if (__ballot(viol)) {  // one violation decides the trajectory
                out = true;
                break;
            }
        }
        word_new = (word_new & ~FP_FLAG_BOUNDARY) | (out ? FP_FLAG_BOUNDARY : 0u);
        if (out) spoke |= FP_RULE_BOUNDARY;
    }
    if (c.gaps_active && !(word_new & FP_FLAG_INFEASIBLE)) {
        // poses i = 0, cs, 2 cs, ... < min(M, final_time_step - t_now) inside the table: grid poses q < n_pose
        const int cs = c.cs;
        const int limit = M < e.horizon_cap ? M : e.horizon_cap;
        int n_pose = limit > 0 ? (limit + cs - 1) / cs : 0;
        if (c.G < n_pose) n_pose = c.G;
        if (c.q_first < n_pose) {
            int split = 1;
            while (split < kRulesSplit && (n_pose - c.q_first) * split * 2 <= kWave) split *= 2;
            const int per_round = kWave / split, sub = lane & (split - 1);
            for (int qb = c.q_first; qb < n_pose; qb += per_round) {
                const int q = qb + lane / split, i = q * cs;
                bool hit = false;
                Obb ego;
                if (q < n_pose && i + e.t_now >= 0 && checked_pose(p, e.sp, c.guess_scale, lon, lat, i, M, ego))
                    hit = gap_pose_hit(ka, e, ego, q, n_pose, c.Lf, c.Ll, sub, split, nullptr, c.r_e, cs, e.n_obs);
                if (__ballot(hit)) {
                    word_new |= FP_FLAG_COLLISION;
                    spoke |= FP_RULE_GAP;
                    break;  // the one bit the rule can give is found
                }
            }
        }
    }
    return word_new;
}

}  // namespace fp
