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
//   - every rule gives the lanes the points 1 + lane, 65 + lane, ... < M (the gaps: the grid poses, split like gap_mask_kernel's);
//     __ballot is the verdict and a rule ends on its first hit.  The gaps run only when the word carries no FP_FLAG_INFEASIBLE bit
//     after the three rules before them;
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
constexpr int kRulesSplit = 8;             // at most this many lanes share one pose's columns (the gaps)
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
    const bool envelope = a.on & FP_RULE_LIMIT, gates = a.on & FP_RULE_GATE, boundary = a.on & FP_RULE_BOUNDARY, gaps = a.on & FP_RULE_GAP;
    const int lateral = (a.on & FP_RULE_LATERAL) ? 1 : 0;
    const int f = ka.b.frame_of[b], nx = e.sp.nx, NX = ka.b.NX;
    const int cap = points_cap(p), t_last = a.T_gate - 1;
    const long long tn = e.t_now;
    const double tick = p.tick_t;
    const double q0 = e.s0 + a.gate_front;
    // ---- stage the rules' own tables: limits [NX] | l0, l1, r0, r1 [NX] each | gate lines [FP_MAX_GATES], closed words [cap]
    double* lim = lds + a.off_lim;
    double* l0 = lds + a.off_edge;
    double* l1 = l0 + NX;
    double* r0 = l1 + NX;
    double* r1 = r0 + NX;
    double* line = lds + a.off_gate;
    uint32_t* word = (uint32_t*)(line + FP_MAX_GATES);
    const uint32_t* closed = gates ? a.closed + (size_t)f * a.T_gate : nullptr;
    if (envelope) {
        const double* gl = a.v_limit + (size_t)f * NX;
        for (int i = tid; i < nx; i += kRulesThreads) lim[i] = i + 1 < nx ? gl[i] : __builtin_inf();  // (the last knot starts no segment)
    }
    if (boundary) stage_corridor(ka.b.knots + (size_t)f * NX, a.left + (size_t)f * NX, a.right + (size_t)f * NX, nx, nullptr, l0, l1, r0, r1, tid, kRulesThreads);
    if (gates) {
        if (wave == 0) {
            double g = __builtin_nan("");
            if (lane < a.gate_stride) {
                g = a.gate_s[(size_t)f * a.gate_stride + lane];
                if (gate_waived(a.max_decel, e.s_d0, q0, g)) g = __builtin_nan("");
            }
            if (lane < FP_MAX_GATES) line[lane] = g;
            const unsigned long long live = __ballot(g == g);
            if (lane == 0) s_live = (uint32_t)live;
        }
        for (int i = tid; i < cap; i += kRulesThreads) word[i] = gate_word(closed, tn + 1 + i, t_last);
    }
    __syncthreads();
    const uint32_t live = gates ? s_live : 0u;
    const double guess_scale = (double)(nx - 1) / (e.sp.knots[nx - 1] - e.sp.knots[0]);
    const double hl = 0.5 * p.veh_l, hw = 0.5 * p.veh_w;
    const double r_e = sqrt(fma(hl, hl, hw * hw));
    const int cs = p.check_stride;
    const int Lf = a.lag_follow / cs, Ll = a.lag_lead / cs;  // the lags in grid steps: only pairs on the grid exist
    const int G = gaps ? gap_grid_poses(p, e) : 0;
    const bool gaps_active = G > 0 && (Lf > 0 || Ll > 0);
    const int q_first = (a.first - 1) / cs + 1 < G ? (a.first - 1) / cs + 1 : G;
    const uint32_t env_want = FP_FLAG_SPEED | (lateral ? FP_FLAG_ACCEL : 0u);
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
        uint32_t word_new = fl, spoke = 0u;
        if (envelope) {
            uint32_t bits = 0u;
            for (int i0 = 1; i0 < M; i0 += kWave) {
                const int i = i0 + lane;
                bool fast = false, lat_v = false;
                if (i < M) envelope_point(e.sp, lim, guess_scale, lon, (double)i * tick, a.env_front, a.env_tol, lateral, a.max_lat_accel, fast, lat_v);
                if (__ballot(fast)) bits |= FP_FLAG_SPEED;
                if (__ballot(lat_v)) bits |= FP_FLAG_ACCEL;
                if (bits == env_want) break;  // every bit the rule can give is found
            }
            word_new |= bits;
            if (bits & FP_FLAG_SPEED) { spoke |= FP_RULE_LIMIT; ++n_limit; }
            if (bits & FP_FLAG_ACCEL) { spoke |= FP_RULE_LATERAL; ++n_lateral; }
        }
        if (gates && live != 0u) {
            for (int i0 = 1; i0 < M; i0 += kWave) {
                const int i = i0 + lane;
                bool hit = false;
                if (i < M) {
                    const uint32_t w = (i <= cap ? word[i - 1] : gate_word(closed, tn + i, t_last)) & live;
                    if (w) hit = gate_point(lon, i, tick, a.gate_front, q0, w, line);
                }
                if (__ballot(hit)) {
                    word_new |= FP_FLAG_SPEED;
                    spoke |= FP_RULE_GATE;
                    ++n_gate;
                    break;
                }
            }
        }
        if (boundary) {
            bool out = false;
            for (int i0 = 1; i0 < M; i0 += kWave) {
                const int i = i0 + lane;
                bool viol = false;
                if (i < M) viol = boundary_point(e.sp, l0, l1, r0, r1, guess_scale, lon, lat, (double)i * tick, hw, hl, a.margin);
                if (__ballot(viol)) {  // one violation decides the trajectory
                    out = true;
                    break;
                }
            }
            word_new = (word_new & ~FP_FLAG_BOUNDARY) | (out ? FP_FLAG_BOUNDARY : 0u);
            if (out) { spoke |= FP_RULE_BOUNDARY; ++n_bound; }
        }
        if (gaps_active && !(word_new & FP_FLAG_INFEASIBLE)) {
            // poses i = 0, cs, 2 cs, ... < min(M, final_time_step - t_now) inside the table: grid poses q < n_pose
            const int limit = M < e.horizon_cap ? M : e.horizon_cap;
            int n_pose = limit > 0 ? (limit + cs - 1) / cs : 0;
            if (G < n_pose) n_pose = G;
            if (q_first < n_pose) {
                int split = 1;
                while (split < kRulesSplit && (n_pose - q_first) * split * 2 <= kWave) split *= 2;
                const int per_round = kWave / split, sub = lane & (split - 1);
                for (int qb = q_first; qb < n_pose; qb += per_round) {
                    const int q = qb + lane / split, i = q * cs;
                    bool hit = false;
                    Obb ego;
                    if (q < n_pose && i + e.t_now >= 0 && checked_pose(p, e.sp, guess_scale, lon, lat, i, M, ego))
                        hit = gap_pose_hit(ka, e, ego, q, n_pose, Lf, Ll, sub, split, nullptr, r_e, cs, e.n_obs);
                    if (__ballot(hit)) {
                        word_new |= FP_FLAG_COLLISION;
                        spoke |= FP_RULE_GAP;
                        ++n_gap;
                        break;  // the one bit the rule can give is found
                    }
                }
            }
        }
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
    long own = 0;  // doubles
    if (a.on & FP_RULE_LIMIT) own += ka.b.NX;
    if (a.on & FP_RULE_BOUNDARY) own += 4L * ka.b.NX;
    if (a.on & FP_RULE_GATE) own += FP_MAX_GATES + (points_cap(ka.p) + 1) / 2;
    int lds_doubles = 0;
    ego_lds_bytes(ka.p, ka.b, (int)(kRulesLdsBytes - own * 8), &lds_doubles);
    int off = lds_doubles;
    a.off_lim = off;
    if (a.on & FP_RULE_LIMIT) off += ka.b.NX;
    a.off_edge = off;
    if (a.on & FP_RULE_BOUNDARY) off += 4 * ka.b.NX;
    a.off_gate = off;
    const int bytes = (int)((lds_doubles + own) * 8);
    return launch_with_lds<rules_eval_kernel>(dim3(ka.b.B), dim3(kRulesThreads), bytes, stream, ka, a, lds_doubles);
}

}  // namespace fp
