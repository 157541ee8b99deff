// frenet_fallback.hip - a stopping manoeuvre for the egos whose planner found nothing (fp_fallback_stop, added within ABI 18).
//
// An ego needs a fallback when its plan call left "no solution" (best_idx < 0, or a NaN end state).  For such an ego the kernel looks at
// a small family of explicit end states (d, v = 0, T) - n_d lateral offsets x n_stop stop times, exactly the trajectories fp_eval_trajs
// builds for them - and picks one by a "least harm" order instead of "feasible or nothing": a stop without contact before one with,
// the gentlest clear stop, the latest contact (the definition: include/frenet_gpu.h).  Every other ego gets its own plan's end state
// written beside it, so that one array describes what every ego drives.
//
// fallback_kernel<false>: one 512-thread workgroup per ego.
//   - A workgroup whose ego needs no fallback returns before anything is staged: thread 0 decodes the lattice index and writes the
//     "none" values.  In a healthy loop that is nearly every workgroup.
//   - stage_ego (frenet_ego.h) once for all F candidates: spline, obstacle sizes and - when they fit kFallbackLdsBytes - the rows the
//     pose set can touch; else obs_row reads the scene table.
//   - Per stop time (a wavefront takes one at a time): the longitudinal quartic, N, M (the first point off the line) and the two
//     admissibility ballots over the series points, 64 points per round; one packed word per stop time in LDS.  Nothing of this depends
//     on the lateral target, so F candidates share n_stop of these passes.
//   - Per candidate (a wavefront takes one at a time): the lanes are the checked poses in ascending order, 64 per round; a lane walks the
//     columns in ascending order behind the collision check's circumradius broad phase and stops at its first overlap.  The first round
//     with a non-zero ballot decides: its lowest lane is hit_step, that lane's column is hit_obs (the lane's own walk ascends, so its
//     first overlap is the pose's smallest column).  The candidate's key is wave-uniform: no reduction inside the wavefront.
//   - The key is three integers compared lexicographically (smaller wins): [contact | 0xffff - i_T or 0xffff - hit_step | 0 or i_T],
//     the bit pattern of the non-negative double fabs(d_end - d0), and f (equal leading words imply equal i_T, so f orders as i_d).
//     Each wavefront keeps the smallest key of its candidates; thread 0 merges the wavefronts' keys from LDS in a plain loop and writes
//     the ego's outputs.
// fallback_kernel<true> (fp_fallback_stop_rules): the same kernel with kRules = true.  The rules' tables are staged behind stage_ego's
// layout (stage_rule_tables, frenet_rules.h: they share the 144 KB budget, so the pose rows go to the scene table a little earlier); a
// wavefront whose candidate is admissible and clear evaluates the four rules on it (wave_rules_eval: fp_rules_eval's verdict of the end
// state (d, 0, T) on a word that carries M alone) and the verdict ranks the candidate inside the order word - clean before violating,
// then fewer rules broken, then the harder brake.  A candidate with contact or without admissibility is never shown to the rules.
// Plain C++ FP64, no atomics, nothing depends on the order workgroups run in: two runs give the same bits.
#include <type_traits>

#include "frenet_device.h"
#include "frenet_kernels.h"
#include "frenet_ego.h"
#include "frenet_rules.h"

namespace fp {

constexpr int kFallbackThreads = 512;
constexpr int kFallbackWaves = kFallbackThreads / kWave;
// LDS budget of stage_ego's tables (the kernel's static LDS is 1.3 KB): as the plan-margin kernel's, one workgroup per CU at the most
constexpr int kFallbackLdsBytes = 144 * 1024;

struct FallbackKey {
    unsigned long long order, lateral;  // smaller wins; order == ~0: no admissible candidate
    int f, hit_step, hit_obs;
};
// the rule instance's key: the order word carries the verdict's rank, `rules` the verdict itself (FP_RULE_*, 0 = clean or not evaluated)
struct FallbackRulesKey {
    unsigned long long order, lateral;
    int f, hit_step, hit_obs;
    uint32_t rules;
};
struct FallbackRuleState {
    RuleTables tabs;
    RuleConsts rc;
    uint32_t* live;
};
struct NoRules {};
// where the contact bit of the order word sits: above the 16-bit i_T / hit_step field, and in the rule instance above the verdict's
// rank too - [contact | violates | popcount(verdict) : 3 | 0xffff - i_T (clean), i_T (violating), 0xffff - hit_step (contact) | 0 or i_T]
constexpr int kContactBit = 32, kRulesContactBit = 36, kViolatesBit = 35;
template <class Key>
__device__ __forceinline__ bool fallback_before(const Key& a, const Key& b)
{
    return a.order < b.order || (a.order == b.order && (a.lateral < b.lateral || (a.lateral == b.lateral && a.f < b.f)));
}

// is the footprint `ego` at checked pose i in contact with a valid column?  -> the smallest such column, or -1 (has_collision's predicate)
__device__ __forceinline__ int first_overlap(const KernelArgs& ka, const EgoCtx& e, const Obb& ego, const double* row, double r_e)
{
    for (int j = 0; j < e.n_obs; ++j) {
        double ox, oy, oc, os;
        if (!obs_centre(e, row, j, ox, oy)) continue;
        const double R = (r_e + e.obs_dim[4 * j + 2]) * (1.0 + 1e-12);
        const double dx = ox - ego.x, dy = oy - ego.y;
        if (!(fma(dx, dx, dy * dy) <= R * R)) continue;
        obs_heading(e, row, j, oc, os);
        const Obb ob{ox, oy, oc, os, e.obs_dim[4 * j], e.obs_dim[4 * j + 1]};
        if (shape_overlap(ego, ob, ka.b.obs_nvert, ka.b.obs_poly, ka.b.poly_stride, e.col0 + j)) return j;
    }
    return -1;
}

// kRules = false: fp_fallback_stop's kernel (its arguments are FallbackArgs; the instance compiles to what the kernel was before it became
// a template).  kRules = true: fp_fallback_stop_rules' (FallbackRulesArgs) - a wavefront whose candidate is admissible and clear asks
// wave_rules_eval (frenet_rules.h) for its verdict, and the verdict ranks the candidate between the contact bit and i_T.
template <bool kRules>
__global__ __launch_bounds__(kFallbackThreads) void fallback_kernel(KernelArgs ka, std::conditional_t<kRules, FallbackRulesArgs, FallbackArgs> a, int lds_doubles)
{
    using Key = std::conditional_t<kRules, FallbackRulesKey, FallbackKey>;
    constexpr int contact_bit = kRules ? kRulesContactBit : kContactBit;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ int s_stop[FP_MAX_FALLBACK];  // per stop time: M | admissible << 16
    __shared__ Key s_key[kFallbackWaves];
    // what only the rule instance has: the staged tables, the call's constants and one LDS word for the gates that are live for this ego
    // (NoRules for kRules = false: that instance declares none of it)
    std::conditional_t<kRules, FallbackRuleState, NoRules> rs;
    if constexpr (kRules) {
        __shared__ uint32_t s_live;
        rs.live = &s_live;
    }
    const int b = a.perm ? a.perm[blockIdx.x] : (int)blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const fp_params& p = ka.p;
    const double nan = __builtin_nan("");
    const int F = a.n_d * a.n_stop;
    double* es = a.end_state + (size_t)b * 3;
    const bool skipped = ka.b.skip && ka.b.skip[b];
    const int c = a.best_idx ? a.best_idx[b] : 0;
    const bool need = !skipped && (a.best_idx ? c < 0 : !(es[0] == es[0]));
    if (!need) {  // (block-uniform: nothing is staged, no barrier is met)
        if (tid == 0) {
            if (a.best_idx) {
                double d_end = nan, v_end = nan, T = nan;
                if (!skipped && c < p.nd * p.nv * p.nt) {  // (an index beyond the lattice reads nothing)
                    const int iv = c % p.nv, it = (c / p.nv) % p.nt, id = c / (p.nv * p.nt);
                    d_end = ka.b.d_samples[id]; v_end = ka.b.v_samples[(size_t)b * p.nv + iv]; T = ka.b.t_samples[it];
                }
                es[0] = d_end; es[1] = v_end; es[2] = T;
            }
            a.status[b] = FP_FALLBACK_NOT_NEEDED; a.fb_idx[b] = -1;
            a.hit_step[b] = -1; a.hit_obs[b] = -1; a.hit_speed[b] = nan;
            if (a.counts) a.counts[(size_t)b * 4 + FP_FALLBACK_NOT_NEEDED] += 1;
            if constexpr (kRules) a.rule_bits[b] = 0u;
        }
        return;
    }
    EgoCtx e;
    stage_ego(ka, b, lds, e, lds_doubles);  // (ends with a barrier)
    if constexpr (kRules) rs.tabs = stage_rule_tables(ka, a.rules, b, e, lds, rs.live, tid, wave, lane, kFallbackThreads);  // (read behind the next barrier)
    const int cs = p.check_stride;
    const double k0 = e.sp.knots[0], kl = e.sp.knots[e.sp.nx - 1];
    const double guess_scale = (double)(e.sp.nx - 1) / (kl - k0);
    const double hl = 0.5 * p.veh_l, hw = 0.5 * p.veh_w;
    const double r_e = sqrt(fma(hl, hl, hw * hw));

    // per stop time: N, M and the admissibility of the longitudinal profile
    for (int it = wave; it < a.n_stop; it += kFallbackWaves) {
        const double T = a.stop_T[it];
        const int N = (T == T) ? arange_len(T, p.tick_t) : 0;
        int M = 0, ok = 0;
        if (N > 0 && N <= points_cap(p)) {
            const Quartic lon = quartic_bvp(e.s0, e.s_d0, e.s_dd0, 0.0, 0.0, T);
            M = N;
            ok = 1;
            for (int i0 = 0; i0 < N; i0 += kWave) {
                const int i = i0 + lane;
                double sv, sd, sdd, sddd;
                quartic_eval(lon, (double)i * p.tick_t, sv, sd, sdd, sddd);
                const bool in = i < N;
                const unsigned long long off = __ballot(in && M == N && (!(sv >= k0) || !(sv < kl)));
                if (off) M = i0 + __ffsll((long long)off) - 1;
                if (__ballot(in && (!(sd >= -FP_FALLBACK_REVERSE_TOL) || !(-sdd <= a.max_decel)))) ok = 0;
            }
            if (M < 2) ok = 0;
        }
        if (lane == 0) s_stop[it] = M | (ok << 16);
    }
    __syncthreads();

    // per candidate: the first contact over the collision check's pose set, and the key
    if constexpr (kRules) rs.rc = rule_consts(ka, a.rules, e, rs.live);
    Key mine;
    mine.order = ~0ull; mine.lateral = ~0ull; mine.f = 0x7fffffff; mine.hit_step = -1; mine.hit_obs = -1;
    if constexpr (kRules) mine.rules = 0u;
    for (int f = wave; f < F; f += kFallbackWaves) {
        const int id = f / a.n_stop, it = f - id * a.n_stop;
        const int word = s_stop[it], M = word & 0xffff;
        if (!(word >> 16)) {
            if (a.cand && lane == 0) a.cand[(size_t)b * F + f] = -2;
            if constexpr (kRules) {
                if (a.cand_rules && lane == 0) a.cand_rules[(size_t)b * F + f] = 0u;
            }
            continue;
        }
        const double T = a.stop_T[it], dt = a.d_targets[id];
        const double d_end = dt == dt ? dt : e.d0;
        const Quartic lon = quartic_bvp(e.s0, e.s_d0, e.s_dd0, 0.0, 0.0, T);
        const Quintic lat = quintic_bvp(e.d0, e.d_d0, e.d_dd0, d_end, 0.0, 0.0, T);
        const int limit = M < e.horizon_cap ? M : e.horizon_cap;
        const int n_pose = e.n_obs > 0 && limit > 0 ? (limit + cs - 1) / cs : 0;
        int hit_step = -1, hit_obs = -1;
        for (int q0 = 0; q0 < n_pose; q0 += kWave) {
            const int q = q0 + lane, i = q * cs;
            int j = -1;
            if (q < n_pose) {
                const double* row = obs_row(e, i, cs);
                Obb ego;
                if (row && checked_pose(p, e.sp, guess_scale, lon, lat, i, M, ego)) j = first_overlap(ka, e, ego, row, r_e);
            }
            const unsigned long long hits = __ballot(j >= 0);
            if (hits) {
                const int first = __ffsll((long long)hits) - 1;
                hit_step = (q0 + first) * cs;
                hit_obs = __shfl(j, first, kWave);
                break;
            }
        }
        if (a.cand && lane == 0) a.cand[(size_t)b * F + f] = hit_step;  // (-1: clear)
        Key k;
        if constexpr (kRules) {
            // the verdict of an admissible, clear candidate: fp_rules_eval's rule_bits for (d_end, 0, T) on a word that carries M alone
            uint32_t verdict = 0u;
            if (hit_step < 0) wave_rules_eval(ka, a.rules, e, rs.tabs, rs.rc, lon, lat, M, (uint32_t)M << FP_FLAG_M_SHIFT, lane, verdict);
            if (a.cand_rules && lane == 0) a.cand_rules[(size_t)b * F + f] = verdict;
            k.rules = verdict;
            if (hit_step >= 0)
                k.order = 1ull << kRulesContactBit | (unsigned long long)(0xffff - hit_step) << 16 | (unsigned long long)it;
            else if (verdict != 0u)  // fewest rules broken, then the hardest brake
                k.order = 1ull << kViolatesBit | (unsigned long long)__popc(verdict) << 32 | (unsigned long long)it << 16;
            else
                k.order = (unsigned long long)(0xffff - it) << 16;
        } else {
            k.order = hit_step < 0 ? (unsigned long long)(0xffff - it) << 16 : 1ull << 32 | (unsigned long long)(0xffff - hit_step) << 16 | (unsigned long long)it;
        }
        k.lateral = (unsigned long long)__double_as_longlong(fabs(d_end - e.d0));
        k.f = f; k.hit_step = hit_step; k.hit_obs = hit_obs;
        if (fallback_before(k, mine)) mine = k;
    }
    if (lane == 0) s_key[wave] = mine;
    __syncthreads();
    if (tid == 0) {
        Key best = s_key[0];
        for (int w = 1; w < kFallbackWaves; ++w)
            if (fallback_before(s_key[w], best)) best = s_key[w];
        int status = FP_FALLBACK_NONE, fb = -1;
        double d_end = nan, v_end = nan, T = nan, speed = nan;
        if (best.order != ~0ull) {
            fb = best.f;
            const int id = fb / a.n_stop, it = fb - id * a.n_stop;
            const double dt = a.d_targets[id];
            d_end = dt == dt ? dt : e.d0; v_end = 0.0; T = a.stop_T[it];
            // (the contact bit of the order word, by arithmetic: written as a select on best.hit_step beside the select on dt above, this
            // compiler's scalar select took the OTHER select's condition - status followed "d_targets is NaN", seen in the .s and on the GPU)
            static_assert(FP_FALLBACK_CONTACT == FP_FALLBACK_CLEAR + 1, "status = CLEAR + the contact bit");
            status = FP_FALLBACK_CLEAR + (int)((best.order >> contact_bit) & 1ull);
            if (best.hit_step >= 0) {
                double sv, sdd, sddd;
                quartic_eval(quartic_bvp(e.s0, e.s_d0, e.s_dd0, 0.0, 0.0, T), (double)best.hit_step * p.tick_t, sv, speed, sdd, sddd);
            }
        }
        es[0] = d_end; es[1] = v_end; es[2] = T;
        a.status[b] = status; a.fb_idx[b] = fb;
        a.hit_step[b] = best.hit_step; a.hit_obs[b] = best.hit_obs; a.hit_speed[b] = speed;
        if (a.counts) a.counts[(size_t)b * 4 + status] += 1;
        if constexpr (kRules) {
            // (the winning key's own verdict: 0 in the initial key, for a clean winner and for one with contact - no select beside the above)
            const uint32_t bits = best.rules;
            a.rule_bits[b] = bits;
            if (a.rule_counts) {
                int32_t* row = a.rule_counts + (size_t)b * FP_RULE_COUNT;
                for (int i = 0; i < FP_RULE_COUNT; ++i) row[i] = row[i] + (int32_t)((bits >> i) & 1u);  // (the row is this workgroup's alone)
            }
        }
    }
}

hipError_t launch_fallback_stop(const KernelArgs& ka, const FallbackArgs& a, hipStream_t stream)
{
    if (ka.b.B < 1 || a.n_d < 1 || a.n_stop < 1 || a.n_d * a.n_stop > FP_MAX_FALLBACK || ka.p.check_stride < 1 || !a.d_targets || !a.stop_T || !a.end_state ||
        !a.status || !a.fb_idx || !a.hit_step || !a.hit_obs || !a.hit_speed)
        return hipErrorInvalidValue;  // (internal: fp_fallback_stop has checked its arguments)
    int lds_doubles = 0;
    const int bytes = ego_lds_bytes(ka.p, ka.b, kFallbackLdsBytes, &lds_doubles);
    return launch_with_lds<fallback_kernel<false>>(dim3(ka.b.B), dim3(kFallbackThreads), bytes, stream, ka, a, lds_doubles);
}

hipError_t launch_fallback_stop_rules(const KernelArgs& ka, FallbackRulesArgs a, hipStream_t stream)
{
    const uint32_t all = FP_RULE_LIMIT | FP_RULE_LATERAL | FP_RULE_GATE | FP_RULE_BOUNDARY | FP_RULE_GAP;
    RulesEvalArgs& r = a.rules;
    if (ka.b.B < 1 || a.n_d < 1 || a.n_stop < 1 || a.n_d * a.n_stop > FP_MAX_FALLBACK || ka.p.check_stride < 1 || !a.d_targets || !a.stop_T || !a.end_state ||
        !a.status || !a.fb_idx || !a.hit_step || !a.hit_obs || !a.hit_speed || !a.rule_bits || !(r.on & all) || (r.on & ~all) ||
        ((r.on & FP_RULE_LATERAL) && !(r.on & FP_RULE_LIMIT)) || ka.b.NX < 2 || ka.b.NX > FP_MAX_KNOTS || ((r.on & FP_RULE_LIMIT) && !r.v_limit) ||
        ((r.on & FP_RULE_GATE) && (!r.gate_s || !r.closed || r.gate_stride < 1 || r.gate_stride > FP_MAX_GATES || r.T_gate < 1)) ||
        ((r.on & FP_RULE_BOUNDARY) && (!r.left || !r.right)) || ((r.on & FP_RULE_GAP) && (r.lag_follow < 0 || r.lag_lead < 0 || r.first < 1)))
        return hipErrorInvalidValue;  // (internal: fp_fallback_stop_rules has checked its arguments)
    if (r.first > FP_MAX_POINTS) r.first = FP_MAX_POINTS;  // (no trajectory has a point FP_MAX_POINTS: beyond every pose either way)
    // the rules' tables go behind stage_ego's layout and come out of the same budget, as launch_rules_eval lays them out
    const long own = rule_table_doubles(r.on, ka.p, ka.b.NX);  // doubles
    int lds_doubles = 0;
    ego_lds_bytes(ka.p, ka.b, (int)(kFallbackLdsBytes - own * 8), &lds_doubles);
    rule_table_offsets(r, lds_doubles, ka.b.NX);
    const int bytes = (int)((lds_doubles + own) * 8);
    return launch_with_lds<fallback_kernel<true>>(dim3(ka.b.B), dim3(kFallbackThreads), bytes, stream, ka, a, lds_doubles);
}

}  // namespace fp
