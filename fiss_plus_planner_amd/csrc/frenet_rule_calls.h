// frenet_rule_calls.h - how a road rule's C struct (fp_speed_profile, fp_gates, fp_corridor, fp_time_gap) becomes kernel arguments and
// staged arrays.  Three host paths carry the rules - each rule's own table pass, fp_rules_eval, and fp_plan_fiss_rules, which runs the
// table passes and the refinement's rule instances - and all of them build their blocks here.  Host-side arithmetic and pointer
// assignments only: no HIP call, no allocation (tests/test_rule_calls_cpu.py prints the blocks on a machine without a GPU).
// A new rule: its fields in RulesEvalArgs and rule_args, its arrays in stage_rule_arrays, a filler for its pass block.
#pragma once

#include "frenet_kernels.h"
#include "frenet_stage_plan.h"

namespace fp {

// The rule set as the rules kernel and the refinement's rule instances take it; a rule that is off leaves its fields unset.  The table
// passes fill their blocks from it too (a set of one rule), so every scalar is read from its struct here and nowhere else.
inline RulesEvalArgs rule_args(const fp_rule_set& rules)
{
    RulesEvalArgs a;
    if (const fp_speed_profile* e = rules.envelope) {
        a.on |= FP_RULE_LIMIT | (e->max_lat_accel > 0 ? FP_RULE_LATERAL : 0u);
        a.env_front = e->front; a.env_tol = e->tol; a.max_lat_accel = e->max_lat_accel; a.v_limit = e->v_limit;
    }
    if (const fp_gates* g = rules.gates) {
        a.on |= FP_RULE_GATE;
        a.gate_front = g->front; a.max_decel = g->max_decel; a.gate_stride = g->gate_stride; a.T_gate = g->T_gate;
        a.gate_s = g->gate_s; a.closed = g->closed;
    }
    if (const fp_corridor* c = rules.boundary) {
        a.on |= FP_RULE_BOUNDARY;
        a.margin = c->margin; a.left = c->left; a.right = c->right;
    }
    if (const fp_time_gap* t = rules.gaps) {
        a.on |= FP_RULE_GAP;
        a.lag_follow = t->lag_follow; a.lag_lead = t->lag_lead;
        a.first = t->first < FP_MAX_POINTS ? t->first : FP_MAX_POINTS;  // (points are 0 .. FP_MAX_POINTS - 1: anything above is "beyond every pose")
    }
    return a;
}

// The arrays of the rules that are on, declared in the call's list in the passes' order ([F][NX] limits; [F][gate_stride] lines,
// [F][T_gate] words; [F][NX] edges): a host call's get their device addresses at commit, a device call's keep the caller's
inline void stage_rule_arrays(StageList& sl, RulesEvalArgs* a, int F, int NX)
{
    const size_t fn = (size_t)F * NX;
    if (a->on & FP_RULE_LIMIT) sl.in(a->v_limit, fn, &a->v_limit);
    if (a->on & FP_RULE_GATE) {
        sl.in(a->gate_s, (size_t)F * a->gate_stride, &a->gate_s);
        sl.in(a->closed, (size_t)F * a->T_gate, &a->closed);
    }
    if (a->on & FP_RULE_BOUNDARY) {
        sl.in(a->left, fn, &a->left);
        sl.in(a->right, fn, &a->right);
    }
}

// The points a trajectory of the call can have, as two passes size themselves.  A device caller announces them in fp_params.points_max; a
// host call has looked at its time samples (`host_points`: what host_points_max made of them, 0 when the fast paths' FP_FAST_POINTS
// hold them).  The gap pass takes the number as its KernelArgs' points_max; the gate pass stages that many closed words per ego, and
// never fewer than the fast paths' points.
inline int gap_points_max(const fp_params& p, bool host, int host_points) { return host ? host_points : p.points_max; }
inline int gate_points_cap(const fp_params& p, bool host, int host_points)
{
    const int n = gap_points_max(p, host, host_points);
    return n > FP_FAST_POINTS ? n : FP_FAST_POINTS;
}

// The rule's own fields of each pass block (the TablePassArgs part is table_pass_declare's, frenet_abi.hip).  coef, t_now, d_samples: the
// batch's arrays as the launch addresses them; coef is read by the lateral check alone.
inline void envelope_args(EnvelopeArgs* a, const RulesEvalArgs& r, const double* coef)
{
    a->front = r.env_front; a->tol = r.env_tol; a->max_lat_accel = r.max_lat_accel;
    a->coef = (r.on & FP_RULE_LATERAL) ? coef : nullptr; a->v_limit = r.v_limit;
}
inline void gate_args(GateArgs* a, const RulesEvalArgs& r, const int32_t* t_now, int points_cap)
{
    a->front = r.gate_front; a->max_decel = r.max_decel; a->gate_stride = r.gate_stride; a->T_gate = r.T_gate;
    a->t_now = t_now; a->gate_s = r.gate_s; a->closed = r.closed;
    a->points_cap = points_cap;
}
inline void boundary_args(BoundaryArgs* a, const RulesEvalArgs& r, const fp_params& p, const double* d_samples)
{
    a->veh_l = p.veh_l; a->veh_w = p.veh_w; a->margin = r.margin;
    a->d_samples = d_samples; a->left = r.left; a->right = r.right;
}
inline GapArgs gap_args(const RulesEvalArgs& r, const int32_t* perm, int32_t* count)
{
    GapArgs g;
    g.lag_follow = r.lag_follow; g.lag_lead = r.lag_lead; g.first = r.first;
    g.perm = perm; g.count = count;
    return g;
}

}  // namespace fp
