// frenet_boundary.hip - the road-boundary check of the dense FOP pass (fp_boundary_mask, added within ABI 18).
//
// The reference declares the check (`check_boundary = True  # True if check collison with road boundaries`,
// frenet_optimal_planner.py:56) and never reads the setting: the lattice confines only the END offset of a candidate, nothing stops
// a candidate from swinging over the road edge on the way there.  Finished here, in Frenet coordinates alone: the corridor is a pair
// of lateral offsets per reference-line knot (left, right), linear in s between the knots, and a candidate violates it when the
// lateral extent of its footprint,  d +- (h + margin),  h = (veh_w / 2 |s_d| + veh_l / 2 |d_d|) / hypot(s_d, d_d),  crosses an edge
// at any of its points 1 .. M - 1 (the definition: include/frenet_gpu.h).
//
// boundary_mask_kernel runs behind the dense pass, over its tables: one 256-thread workgroup per ego.
//   - LDS: the ego's knots, and per segment the edge at the segment's first knot and its slope in s, for both sides (5 nx doubles; a
//     segment with a knot value that is not finite is staged as +-inf with slope 0: it cannot be violated), then - when they fit
//     kBoundProfBytes - the nd x nt lateral quintics and nv x nt longitudinal quartics of the lattice, one lane per profile;
//   - the flag / cost rows are read in chunks of one candidate per thread, wavefront w holding candidates c0 + 4 lane + w, so that
//     every lattice size keeps all four wavefronts busy;
//   - a wavefront then takes its 64 candidates one at a time (the candidate's flag word and profile indices come out of the owning
//     lane's registers), its lanes the points 1 + lane, 65 + lane, ... < M: two fma Horner chains per series (quintic_eval /
//     quartic_eval, the arithmetic of every series dump), the segment look-up (see spline_segment_clamped), one hypot, one division,
//     two compares.  __ballot is the verdict; a round that finds a violation ends the candidate;
//   - the owning lane rewrites the bit in its flag word (a vector store, and only when the word changes) and keeps the ego's argmin
//     among its own candidates; see finish_ego for the rest.
// No atomics, no scratch, every reduction a fixed tree or a ballot: two runs give the same bits.
#include "frenet_device.h"
#include "frenet_kernels.h"
#include "frenet_project.h"
#include "frenet_rules.h"

namespace fp {

constexpr int kBoundThreads = 256;
constexpr int kBoundWaves = kBoundThreads / kWave;
// LDS budget of the staged profiles: (6 nd + 5 nv) nt doubles.  A 9 x 9 x 7 lattice takes 5.4 KB; a lattice beyond the budget (e.g.
// 40 x 1 x 40) solves the two boundary-value problems per candidate instead - same arithmetic, same bits.
constexpr int kBoundProfBytes = 64 * 1024;

__global__ __launch_bounds__(kBoundThreads) void boundary_mask_kernel(BoundaryArgs a, int staged)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int b = a.perm ? a.perm[blockIdx.x] : (int)blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    if (a.skip && a.skip[b]) {  // not planned: the dense pass wrote no rows for this ego
        skip_ego(b, a.best_idx, a.best_cost, a.count);
        return;
    }
    const int nd = a.nd, nv = a.nv, nt = a.nt, C = nd * nv * nt;
    const int f = a.frame_of[b];
    const int nx = a.nx[f];
    // ---- stage: knots | left edge at the knot, its slope | right edge, slope | quintics [nd][nt] | quartics [nv][nt]
    double* knots = lds;
    double* l0 = knots + nx;
    double* l1 = l0 + nx;
    double* r0 = l1 + nx;
    double* r1 = r0 + nx;
    double* s_lat = r1 + nx;
    double* s_lon = s_lat + 6 * nd * nt;
    const double* gk = a.knots + (size_t)f * a.NX;
    const double* gl = a.left + (size_t)f * a.NX;
    const double* gr = a.right + (size_t)f * a.NX;
    stage_corridor(gk, gl, gr, nx, knots, l0, l1, r0, r1, tid, kBoundThreads);
    const double* eg = a.ego + (size_t)b * 6;
    const double s0 = eg[0], s_d0 = eg[1], s_dd0 = eg[2], d0 = eg[3], d_d0 = eg[4], d_dd0 = eg[5];
    const double* vs = a.v_samples + (size_t)b * nv;
    if (staged) {
        for (int i = tid; i < nd * nt; i += kBoundThreads) {
            const Quintic q = quintic_bvp(d0, d_d0, d_dd0, a.d_samples[i / nt], 0.0, 0.0, a.t_samples[i % nt]);
            double* o = s_lat + 6 * i;
            o[0] = q.a0; o[1] = q.a1; o[2] = q.a2; o[3] = q.a3; o[4] = q.a4; o[5] = q.a5;
        }
        for (int i = tid; i < nv * nt; i += kBoundThreads) {
            const Quartic q = quartic_bvp(s0, s_d0, s_dd0, vs[i / nt], 0.0, a.t_samples[i % nt]);
            double* o = s_lon + 5 * i;
            o[0] = q.a0; o[1] = q.a1; o[2] = q.a2; o[3] = q.a3; o[4] = q.a4;
        }
    }
    __syncthreads();
    const SplineLds sp{knots, nullptr, nx, nx};
    const double guess_scale = (double)(nx - 1) / (knots[nx - 1] - knots[0]);
    const double hw = 0.5 * a.veh_w, hl = 0.5 * a.veh_l, margin = a.margin, tick = a.tick_t;
    const double* cost = a.cost_tbl + (size_t)b * C;
    uint32_t* flag = a.flag_tbl + (size_t)b * C;
    Best mine{0.0, -1};  // (per lane: the best of the candidates this lane owned)
    int masked = 0;      // (wave-uniform: candidates of this wavefront that carry the bit)
    for (int c0 = 0; c0 < C; c0 += kBoundThreads) {
        const int c = c0 + lane * kBoundWaves + wave;
        const bool valid = c < C;
        uint32_t fl_own = 0u;
        double cost_own = 0.0;
        int id_own = 0, it_own = 0, iv_own = 0;
        if (valid) {
            fl_own = flag[c];
            cost_own = cost[c];
            iv_own = c % nv;
            it_own = (c / nv) % nt;
            id_own = c / (nv * nt);
        }
        bool bit_own = false;
        const int left_in_chunk = C - c0 - wave;  // candidates c0 + wave + 4 j < C
        const int n_own = left_in_chunk <= 0 ? 0 : (left_in_chunk + kBoundWaves - 1) / kBoundWaves;
        for (int j = 0; j < kWave && j < n_own; ++j) {
            const uint32_t fl = (uint32_t)__builtin_amdgcn_readlane((int)fl_own, j);
            const int M = (int)(fl >> FP_FLAG_M_SHIFT);
            if (M <= 1) continue;  // nothing is checked: no bit
            const int id = __builtin_amdgcn_readlane(id_own, j), it = __builtin_amdgcn_readlane(it_own, j), iv = __builtin_amdgcn_readlane(iv_own, j);
            Quintic lat;
            Quartic lon;
            if (staged) {
                const double* q = s_lat + 6 * (id * nt + it);
                lat = Quintic{q[0], q[1], q[2], q[3], q[4], q[5]};
                const double* g = s_lon + 5 * (iv * nt + it);
                lon = Quartic{g[0], g[1], g[2], g[3], g[4]};
            } else {
                const double T_end = a.t_samples[it];
                lat = quintic_bvp(d0, d_d0, d_dd0, a.d_samples[id], 0.0, 0.0, T_end);
                lon = quartic_bvp(s0, s_d0, s_dd0, vs[iv], 0.0, T_end);
            }
            bool out = false;
            for (int i0 = 1; i0 < M; i0 += kWave) {
                const int i = i0 + lane;
                bool viol = false;
                if (i < M) viol = boundary_point(sp, l0, l1, r0, r1, guess_scale, lon, lat, (double)i * tick, hw, hl, margin);
                if (__ballot(viol)) {  // one violation decides the candidate
                    out = true;
                    break;
                }
            }
            if (out) {
                ++masked;
                if (lane == j) bit_own = true;
            }
        }
        if (valid) {
            const uint32_t fl_new = (fl_own & ~FP_FLAG_BOUNDARY) | (bit_own ? FP_FLAG_BOUNDARY : 0u);
            if (fl_new != fl_own) flag[c] = fl_new;
            if (!(fl_new & FP_FLAG_INFEASIBLE) && cost_own == cost_own) mine = best_merge(mine, Best{cost_own, c});  // (a NaN cost can never win, :266)
        }
    }
    finish_ego<kBoundWaves>(mine, masked, b, a.best_idx, a.best_cost, a.count);
}

hipError_t launch_boundary_mask(const BoundaryArgs& a, hipStream_t stream)
{
    if (a.B < 1 || a.NX < 2 || a.NX > FP_MAX_KNOTS || a.nd < 1 || a.nv < 1 || a.nt < 1 || (long)a.nd * a.nv * a.nt > FP_MAX_CAND || !a.cost_tbl ||
        !a.flag_tbl || !a.best_idx || !a.best_cost || !a.left || !a.right)
        return hipErrorInvalidValue;  // (internal: fp_boundary_mask has checked its arguments)
    const long prof = (6L * a.nd + 5L * a.nv) * a.nt * 8;
    const int staged = prof <= kBoundProfBytes ? 1 : 0;
    const int bytes = 5 * a.NX * 8 + (staged ? (int)prof : 0);  // <= 40 KB + 64 KB
    return launch_with_lds<boundary_mask_kernel>(dim3(a.B), dim3(kBoundThreads), bytes, stream, a, staged);
}

}  // namespace fp
