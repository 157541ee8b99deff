// frenet_rules_eval.hip - the four road rules on explicit end states (fp_rules_eval, added within ABI 18).
//
// fp_speed_envelope, fp_gate_mask, fp_boundary_mask and fp_gap_mask are table passes: a trajectory has a verdict only as a lattice
// candidate of a dense call.  What fp_plan_fiss returns - an end state (d, v, T) that refinement has moved off the lattice - and what a
// caller makes itself has none.  rules_eval_kernel evaluates the same four definitions (include/frenet_gpu.h) on K end states per ego,
// in the order the passes run, with the passes' own predicates (frenet_rules.h): on the lattice's end states it leaves the words the
// chain of the four passes leaves in the table.
//
// One 256-thread workgroup per ego, honouring perm and skip like the passes.
//   - LDS, staged once per ego: stage_ego's layout (spline, obstacle sizes and - when they fit - the obstacle rows of the pose grid;
//     else the rows are read from the scene table: obs_row, frenet_ego.h), then what the rules that are on add: the limit of every
//     segment; the corridor's edge and slope per segment and side (stage_corridor); the gate lines with the waiver folded in, the mask
//     of the live slots and the closed words of the steps t_now + 1 .. t_now + points_cap, as gate_mask_kernel stages them;
//   - the four wavefronts take the K trajectories round-robin (K has no cap: the kernel loops).  N and M come from the trajectory's
//     flag word; a NaN end state, M <= 1 or a T the call is not sized for: nothing is evaluated, the word stays;
//   - wave_rules_eval (frenet_rules.h, shared with the fallback kernel's rule instance): every rule gives the lanes the points
//     1 + lane, 65 + lane, ... < M (the gaps: the grid poses, split like gap_mask_kernel's); __ballot is the verdict and a rule ends on
//     its first hit.  The gaps run only when the word carries no FP_FLAG_INFEASIBLE bit after the three rules before them;
//   - lane 0 stores the word (only when it changes) and the rule bits; the wavefronts' violation counts meet in LDS and one lane per
//     rule adds them to the ego's row of `counts` (read, add, vector store: the row is this workgroup's alone).
// No atomics, no scratch, every verdict a ballot: two runs give the same bits, whatever order workgroups and lanes finish in.
#include "frenet_device.h"
#include "frenet_kernels.h"
#include "frenet_ego.h"
#include "frenet_rules.h"

namespace fp {

constexpr int kRulesThreads = 256;
constexpr int kRulesWaves = kRulesThreads / kWave;
constexpr int kRulesLdsBytes = 144 * 1024;  // stage_ego's layout and the rules' tables together

__global__ __launch_bounds__(kRulesThreads) void rules_eval_kernel(KernelArgs ka, RulesEvalArgs a, int lds_doubles)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ uint32_t s_live;
    __shared__ int s_cnt[kRulesWaves][FP_RULE_COUNT];
    const int b = a.perm ? a.perm[blockIdx.x] : (int)blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const fp_params& p = ka.p;
    const int K = a.K;
    uint32_t* flags = a.flags + (size_t)b * K;
    uint32_t* rule_bits = a.rule_bits ? a.rule_bits + (size_t)b * K : nullptr;
    if (ka.b.skip && ka.b.skip[b]) {  // not planned: the words stay, no rule spoke, nothing is counted
        if (rule_bits)
            for (int k = tid; k < K; k += kRulesThreads) rule_bits[k] = 0u;
        return;
    }
    EgoCtx e;
    stage_ego(ka, b, lds, e, lds_doubles);  // (ends with a barrier)
    // the rules' own tables behind stage_ego's layout, and what the evaluation needs beside them (frenet_rules.h)
    const RuleTables tabs = stage_rule_tables(ka, a, b, e, lds, &s_live, tid, wave, lane, kRulesThreads);
    __syncthreads();
    const RuleConsts rc = rule_consts(ka, a, e, &s_live);
    const int cap = rc.cap;
    const double tick = p.tick_t;
    int n_limit = 0, n_lateral = 0, n_gate = 0, n_bound = 0, n_gap = 0;  // (wave-uniform: this wavefront's violators per rule)
    for (int k = wave; k < K; k += kRulesWaves) {  // (wave-uniform from here to the trajectory's stores)
        const double* es = a.end_states + ((size_t)b * K + k) * 3;
        const double d_end = es[0], v_end = es[1], T = es[2];
        const uint32_t fl = (uint32_t)__builtin_amdgcn_readfirstlane((int)flags[k]);
        int M = (int)(fl >> FP_FLAG_M_SHIFT);
        const int N = (T == T) ? arange_len(T, tick) : 0;
        if (N <= 0 || N > cap || !(d_end == d_end) || !(v_end == v_end) || M <= 1) {  // no trajectory, or nothing to check
            if (lane == 0 && rule_bits) rule_bits[k] = 0u;
            continue;
        }
        if (M > N) M = N;  // (a word that is the trajectory's own never says so)
        const Quintic lat = quintic_bvp(e.d0, e.d_d0, e.d_dd0, d_end, 0.0, 0.0, T);
        const Quartic lon = quartic_bvp(e.s0, e.s_d0, e.s_dd0, v_end, 0.0, T);
        uint32_t spoke;
        const uint32_t word_new = wave_rules_eval(ka, a, e, tabs, rc, lon, lat, M, fl, lane, spoke);
        n_limit += (int)(spoke & FP_RULE_LIMIT ? 1 : 0); n_lateral += (int)(spoke & FP_RULE_LATERAL ? 1 : 0); n_gate += (int)(spoke & FP_RULE_GATE ? 1 : 0);
        n_bound += (int)(spoke & FP_RULE_BOUNDARY ? 1 : 0); n_gap += (int)(spoke & FP_RULE_GAP ? 1 : 0);
        if (lane == 0) {
            if (word_new != fl) flags[k] = word_new;
            if (rule_bits) rule_bits[k] = spoke;
        }
    }
    if (!a.counts) return;  // (kernel argument: the whole workgroup leaves)
    if (lane == 0) {
        s_cnt[wave][0] = n_limit; s_cnt[wave][1] = n_lateral; s_cnt[wave][2] = n_gate; s_cnt[wave][3] = n_bound; s_cnt[wave][4] = n_gap;
    }
    __syncthreads();
    if (tid < FP_RULE_COUNT) {
        int n = 0;
        for (int w = 0; w < kRulesWaves; ++w) n += s_cnt[w][tid];
        int32_t* row = a.counts + (size_t)b * FP_RULE_COUNT;
        if (n != 0) row[tid] = row[tid] + n;
    }
}

hipError_t launch_rules_eval(const KernelArgs& ka, RulesEvalArgs a, hipStream_t stream)
{
    const uint32_t all = FP_RULE_LIMIT | FP_RULE_LATERAL | FP_RULE_GATE | FP_RULE_BOUNDARY | FP_RULE_GAP;
    if (ka.b.B < 1 || a.K < 1 || !(a.on & all) || (a.on & ~all) || ((a.on & FP_RULE_LATERAL) && !(a.on & FP_RULE_LIMIT)) || !a.end_states || !a.flags ||
        ka.b.NX < 2 || ka.b.NX > FP_MAX_KNOTS || ka.p.check_stride < 1 || ((a.on & FP_RULE_LIMIT) && !a.v_limit) ||
        ((a.on & FP_RULE_GATE) && (!a.gate_s || !a.closed || a.gate_stride < 1 || a.gate_stride > FP_MAX_GATES || a.T_gate < 1)) ||
        ((a.on & FP_RULE_BOUNDARY) && (!a.left || !a.right)) || ((a.on & FP_RULE_GAP) && (a.lag_follow < 0 || a.lag_lead < 0 || a.first < 1)))
        return hipErrorInvalidValue;  // (internal: fp_rules_eval has checked its arguments)
    if (a.first > FP_MAX_POINTS) a.first = FP_MAX_POINTS;  // (no trajectory has a point FP_MAX_POINTS: beyond every pose either way)
    // the rules' tables go behind what stage_ego lays out; the obstacle rows get what is left of the budget, and stay in the scene
    // table when that is too little
    const long own = rule_table_doubles(a.on, ka.p, ka.b.NX);  // doubles
    int lds_doubles = 0;
    ego_lds_bytes(ka.p, ka.b, (int)(kRulesLdsBytes - own * 8), &lds_doubles);
    rule_table_offsets(a, lds_doubles, ka.b.NX);
    const int bytes = (int)((lds_doubles + own) * 8);
    return launch_with_lds<rules_eval_kernel>(dim3(ka.b.B), dim3(kRulesThreads), bytes, stream, ka, a, lds_doubles);
}

}  // namespace fp
