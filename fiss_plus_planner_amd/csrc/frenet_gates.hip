// frenet_gates.hip - stop lines that open and close behind the dense FOP pass (fp_gate_mask, added within ABI 18).
//
// fp_speed_envelope models a red light as a stretch of zero speed limit: a function of s alone, so a light never turns green and an ego
// that obeys it in a closed loop waits for ever.  A GATE is a stop line at an arclength of a reference line with a state per absolute
// time step - a traffic light with phases, a crossing while a pedestrian is predicted on it, a barrier.  A candidate violates when its
// front bumper (s + front) moves over the line of a gate that is closed at the step it arrives there; a gate the ego can no longer stop
// in front of is waived (the dilemma zone).  The definition: include/frenet_gpu.h.
//
// The verdict depends on the candidate's longitudinal series, its M and the ego alone: the nd candidates of a longitudinal profile
// (i_v, i_T) share it - what speed_envelope_kernel rests on, and gate_mask_kernel has its shape: one 256-thread workgroup per ego.
//   - LDS: the frame's gate_stride line positions with the waiver folded in (a waived slot becomes NaN, like an unused one) and the mask
//     of the slots that are left (wavefront 0, one gate per lane, one ballot); the closed words of the steps t_now + 1 .. t_now +
//     points_cap, the time index clamped once here; one byte per profile for its verdict;
//   - profile pass: the wavefronts take the profiles round-robin, the lanes the points 1 + lane, 65 + lane, ... < M.  A lane whose step
//     has no live gate closed is done; the others evaluate q_i and q_{i-1} (quartic_bvp / quartic_pos, the arithmetic of every series
//     dump; q_0 from the ego) and walk the set bits of the word.  __ballot gives the verdict, the profile ends on the first hit.  An
//     ego without a live closed gate anywhere in its window therefore costs one LDS read per point and no arithmetic;
//   - row pass, after a barrier: the envelope's - OR the profile's bit in (a vector store, and only when the word changes), keep the
//     argmin among the own candidates, count the violating ones by ballot; see finish_ego for the rest.
// No atomics, no scratch, every reduction a fixed tree or a ballot: two runs give the same bits.
#include "frenet_device.h"
#include "frenet_kernels.h"
#include "frenet_rules.h"

namespace fp {

constexpr int kGateThreads = 256;
constexpr int kGateWaves = kGateThreads / kWave;

__global__ __launch_bounds__(kGateThreads) void gate_mask_kernel(GateArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ uint32_t s_live;
    const int b = a.perm ? a.perm[blockIdx.x] : (int)blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    if (a.skip && a.skip[b]) {  // not planned: the dense pass wrote no rows for this ego
        skip_ego(b, a.best_idx, a.best_cost, a.count);
        return;
    }
    const int nv = a.nv, P = a.nv * a.nt, C = a.nd * P;
    const int f = a.frame_of[b];
    const int cap = a.points_cap, t_last = a.T_gate - 1;
    const long long tn = a.t_now[b];
    const double* eg = a.ego + (size_t)b * 6;
    const double s0 = eg[0], s_d0 = eg[1], s_dd0 = eg[2];
    const double tick = a.tick_t, front = a.front;
    const double q0 = s0 + front;
    // ---- stage: line positions [FP_MAX_GATES] | closed words of the steps t_now + 1 .. t_now + cap | verdicts [P]
    double* line = lds;
    uint32_t* word = (uint32_t*)(line + FP_MAX_GATES);
    uint8_t* verdict = (uint8_t*)(word + cap);
    const uint32_t* closed = a.closed + (size_t)f * a.T_gate;
    if (wave == 0) {
        double g = __builtin_nan("");
        if (lane < a.gate_stride) {
            g = a.gate_s[(size_t)f * a.gate_stride + lane];
            // the dilemma zone: the ego is in front of the line and cannot stop there any more
            if (gate_waived(a.max_decel, s_d0, q0, g)) g = __builtin_nan("");
        }
        if (lane < FP_MAX_GATES) line[lane] = g;
        const unsigned long long live = __ballot(g == g);
        if (lane == 0) s_live = (uint32_t)live;
    }
    for (int i = tid; i < cap; i += kGateThreads) {
        word[i] = gate_word(closed, tn + 1 + i, t_last);  // (the first / the last known state holds)
    }
    __syncthreads();
    const uint32_t live = s_live;
    const double* vs = a.v_samples + (size_t)b * nv;
    const double* cost = a.cost_tbl + (size_t)b * C;
    uint32_t* flag = a.flag_tbl + (size_t)b * C;
    // ---- profile pass: profile p = i_T nv + i_v is candidate p of the ego (i_d = 0), whose flag word carries the profile's M
    for (int p = wave; p < P; p += kGateWaves) {
        const int M = (int)(flag[p] >> FP_FLAG_M_SHIFT);
        uint32_t bits = 0u;
        if (M > 1 && live != 0u) {
            const Quartic lon = quartic_bvp(s0, s_d0, s_dd0, vs[p % nv], 0.0, a.t_samples[p / nv]);
            for (int i0 = 1; i0 < M; i0 += kWave) {
                const int i = i0 + lane;
                bool hit = false;
                if (i < M) {
                    uint32_t w;
                    if (i <= cap) {
                        w = word[i - 1];
                    } else {  // (a caller that announced fewer points than its flag words carry: the same word, from memory)
                        w = gate_word(closed, tn + i, t_last);
                    }
                    w &= live;
                    if (w) hit = gate_point(lon, i, tick, front, q0, w, line);
                }
                if (__ballot(hit)) {
                    bits = FP_FLAG_SPEED;
                    break;  // the one bit the profile can get is found
                }
            }
        }
        if (lane == 0) verdict[p] = (uint8_t)bits;
    }
    __syncthreads();
    // ---- row pass: one candidate per thread
    Best mine{0.0, -1};  // (per lane: the best of the candidates this lane owned)
    int gated = 0;       // (wave-uniform: candidates of this wavefront that violate in this call)
    for (int c0 = 0; c0 < C; c0 += kGateThreads) {
        const int c = c0 + tid;
        uint32_t bits = 0u;
        if (c < C) {
            bits = verdict[c % P];
            const uint32_t fl_own = flag[c], fl_new = fl_own | bits;
            const double cost_own = cost[c];
            if (fl_new != fl_own) flag[c] = fl_new;
            if (!(fl_new & FP_FLAG_INFEASIBLE) && cost_own == cost_own) mine = best_merge(mine, Best{cost_own, c});  // (a NaN cost can never win, :266)
        }
        gated += __popcll(__ballot(bits != 0u));
    }
    finish_ego<kGateWaves>(mine, gated, b, a.best_idx, a.best_cost, a.count);
}

hipError_t launch_gate_mask(const GateArgs& a, hipStream_t stream)
{
    if (a.B < 1 || a.nd < 1 || a.nv < 1 || a.nt < 1 || (long)a.nd * a.nv * a.nt > FP_MAX_CAND || !a.cost_tbl || !a.flag_tbl || !a.best_idx ||
        !a.best_cost || !a.gate_s || !a.closed || !a.t_now || a.gate_stride < 1 || a.gate_stride > FP_MAX_GATES || a.T_gate < 1 || a.points_cap < 1 ||
        a.points_cap > FP_MAX_POINTS)
        return hipErrorInvalidValue;  // (internal: fp_gate_mask has checked its arguments)
    const int bytes = FP_MAX_GATES * 8 + a.points_cap * 4 + ((a.nv * a.nt + 15) & ~15);  // <= 256 B + 1 KB + 16 KB
    return launch_with_lds<gate_mask_kernel>(dim3(a.B), dim3(kGateThreads), bytes, stream, a);
}

}  // namespace fp
