// frenet_envelope.hip - position-dependent speed limits and stop lines behind the dense FOP pass (fp_speed_envelope, added within
// ABI 18).
//
// The planner's one speed limit is fp_params.max_speed.  The reference's own data carries more: the last column of the reference path
// its second caller receives holds, per point, "0 is red light, 1 is crosswalk, other is speed_limi[t]"
// (planners/waymo_interface/waymo_interface.py:160-189) - and that caller hands the planner the largest value on the path.  Finished
// here: a limit per reference-line segment (+inf = none, 0 = stop line / red light), read at the front bumper (s + front), and an
// optional bound on s_d^2 |kappa_r(s)|, the lateral acceleration on the reference line (the definition: include/frenet_gpu.h).
//
// Both verdicts depend on the candidate's longitudinal series alone, and so does M (the series is cut at the first s off the line): the
// nd candidates of a longitudinal profile (i_v, i_T) share them.  speed_envelope_kernel therefore evaluates nv x nt profiles per ego,
// not nd x nv x nt candidates: one 256-thread workgroup per ego.
//   - LDS: the ego's knots, the limit of every segment and - only when the lateral check is on - the eight coefficient columns of the
//     line ((2 + 8) nx doubles, at most 80 KB at FP_MAX_KNOTS), then one byte per profile for its verdict;
//   - profile pass: the wavefronts take the profiles round-robin.  Every lane solves the profile's quartic (quartic_bvp: a division and
//     a dozen multiplications, cheaper than a staging pass with a barrier of its own, and a lattice of any size needs no fallback); the
//     lanes take the points 1 + lane, 65 + lane, ... < M: quartic_eval (the arithmetic of every series dump), the segment look-up (see
//     spline_segment_clamped) for s + front - and for s when the lateral check is on -, the compares.  __ballot gives the two verdicts; a
//     profile ends once every bit it can get is found;
//   - row pass, after a barrier: one coalesced pass over the ego's C flag words, one candidate per thread - OR the profile's bits in (a
//     vector store, and only when the word changes), keep the argmin among the own candidates, count the violating ones by ballot;
//     see finish_ego for the rest.
// No atomics, no scratch, every reduction a fixed tree or a ballot: two runs give the same bits.
#include "frenet_device.h"
#include "frenet_kernels.h"
#include "frenet_rules.h"

namespace fp {

constexpr int kEnvThreads = 256;
constexpr int kEnvWaves = kEnvThreads / kWave;

__global__ __launch_bounds__(kEnvThreads) void speed_envelope_kernel(EnvelopeArgs a, int lateral)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int b = a.perm ? a.perm[blockIdx.x] : (int)blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    if (a.skip && a.skip[b]) {  // not planned: the dense pass wrote no rows for this ego
        skip_ego(b, a.best_idx, a.best_cost, a.count);
        return;
    }
    const int nv = a.nv, P = a.nv * a.nt, C = a.nd * P;
    const int f = a.frame_of[b];
    const int nx = a.nx[f];
    // ---- stage: knots | the limit of the segment that starts at the knot | coefficient columns [8][nx] (lateral check) | verdicts [P]
    double* knots = lds;
    double* lim = knots + nx;
    double* coef = lim + nx;
    uint8_t* verdict = (uint8_t*)(coef + (lateral ? 8 * nx : 0));
    const double* gk = a.knots + (size_t)f * a.NX;
    const double* gl = a.v_limit + (size_t)f * a.NX;
    for (int i = tid; i < nx; i += kEnvThreads) {
        knots[i] = gk[i];
        lim[i] = i + 1 < nx ? gl[i] : __builtin_inf();  // (the last knot starts no segment)
    }
    if (lateral) {
        const double* gc = a.coef + (size_t)f * 8 * a.NX;
        for (int i = tid; i < 8 * nx; i += kEnvThreads) {
            const int r = i / nx, c = i - r * nx;
            coef[i] = gc[(size_t)r * a.NX + c];
        }
    }
    __syncthreads();
    const SplineLds sp{knots, coef, nx, nx};
    const double guess_scale = (double)(nx - 1) / (knots[nx - 1] - knots[0]);
    const double tick = a.tick_t, front = a.front, tol = a.tol, max_lat = a.max_lat_accel;
    const double* eg = a.ego + (size_t)b * 6;
    const double s0 = eg[0], s_d0 = eg[1], s_dd0 = eg[2];
    const double* vs = a.v_samples + (size_t)b * nv;
    const double* cost = a.cost_tbl + (size_t)b * C;
    uint32_t* flag = a.flag_tbl + (size_t)b * C;
    const uint32_t want = FP_FLAG_SPEED | (lateral ? FP_FLAG_ACCEL : 0u);
    // ---- profile pass: profile p = i_T nv + i_v is candidate p of the ego (i_d = 0), whose flag word carries the profile's M
    for (int p = wave; p < P; p += kEnvWaves) {
        const int M = (int)(flag[p] >> FP_FLAG_M_SHIFT);
        uint32_t bits = 0u;
        if (M > 1) {
            const Quartic lon = quartic_bvp(s0, s_d0, s_dd0, vs[p % nv], 0.0, a.t_samples[p / nv]);
            for (int i0 = 1; i0 < M; i0 += kWave) {
                const int i = i0 + lane;
                bool fast = false, lat = false;
                if (i < M) envelope_point(sp, lim, guess_scale, lon, (double)i * tick, front, tol, lateral, max_lat, fast, lat);
                if (__ballot(fast)) bits |= FP_FLAG_SPEED;
                if (__ballot(lat)) bits |= FP_FLAG_ACCEL;
                if (bits == want) break;  // every bit the profile can get is found
            }
        }
        if (lane == 0) verdict[p] = (uint8_t)bits;
    }
    __syncthreads();
    // ---- row pass: one candidate per thread
    Best mine{0.0, -1};  // (per lane: the best of the candidates this lane owned)
    int limited = 0;     // (wave-uniform: candidates of this wavefront that violate in this call)
    for (int c0 = 0; c0 < C; c0 += kEnvThreads) {
        const int c = c0 + tid;
        uint32_t bits = 0u;
        if (c < C) {
            bits = verdict[c % P];
            const uint32_t fl_own = flag[c], fl_new = fl_own | bits;
            const double cost_own = cost[c];
            if (fl_new != fl_own) flag[c] = fl_new;
            if (!(fl_new & FP_FLAG_INFEASIBLE) && cost_own == cost_own) mine = best_merge(mine, Best{cost_own, c});  // (a NaN cost can never win, :266)
        }
        limited += __popcll(__ballot(bits != 0u));
    }
    finish_ego<kEnvWaves>(mine, limited, b, a.best_idx, a.best_cost, a.count);
}

hipError_t launch_speed_envelope(const EnvelopeArgs& a, hipStream_t stream)
{
    const int lateral = a.max_lat_accel > 0.0 ? 1 : 0;
    if (a.B < 1 || a.NX < 2 || a.NX > FP_MAX_KNOTS || a.nd < 1 || a.nv < 1 || a.nt < 1 || (long)a.nd * a.nv * a.nt > FP_MAX_CAND || !a.cost_tbl ||
        !a.flag_tbl || !a.best_idx || !a.best_cost || !a.v_limit || (lateral && !a.coef))
        return hipErrorInvalidValue;  // (internal: fp_speed_envelope has checked its arguments)
    const int bytes = (2 + (lateral ? 8 : 0)) * a.NX * 8 + ((a.nv * a.nt + 15) & ~15);  // <= 80 KB + 16 KB
    return launch_with_lds<speed_envelope_kernel>(dim3(a.B), dim3(kEnvThreads), bytes, stream, a, lateral);
}

}  // namespace fp
