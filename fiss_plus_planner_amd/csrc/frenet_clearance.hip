// frenet_clearance.hip - the obstacle-clearance cost term of the dense FOP pass (fp_params.w_obstacle > 0).
//
// The reference keeps the term as a stub: cost_function.py:9 defines w_D, :21-27 sketches cost_dist_obstacle
// (`Xis = np.exp(-dists); return w_D * sum(Xis)`), :43 holds its slot in cost_total (`cost_obstacle = 0.0`).  Finished here as
//     clearance  = sum over has_collision's poses i (frenet_optimal_planner.py:168-195) and the obstacles j valid at step i + t_now
//                  of exp(-dist(i, j)),  dist = Euclidean distance of the ego footprint to the obstacle's shape (obb_distance /
//                  poly_distance, frenet_device.h)
//     cost_final = (base_sum + w_obstacle * clearance) / N
// for the candidates that survived the checks; every other candidate keeps its cost.
//
// clearance_rescore_kernel runs behind the lattice pass, over its tables: one workgroup per ego, staged like the lane-per-candidate
// kernel (stage_ego: spline, obstacle sizes and - when they fit - the obstacle rows in LDS; see frenet_ego.h).  The flag table is
// walked in chunks of one candidate per thread, the survivors of a chunk compacted by ballot + popcount; then every wavefront takes
// one survivor at a time, its lanes the checked poses (lane, lane + 64, ...; see checked_pose), each lane looping over the obstacles of
// its row.  A candidate's sum is its lanes' sums (poses ascending, obstacles ascending) reduced by wave_sum_f64: one fixed tree, no
// atomics - two runs give the same bits.  The ego's argmin over the new costs (see finish_ego) replaces the lattice pass's.
#include "frenet_device.h"
#include "frenet_kernels.h"
#include "frenet_ego.h"

namespace fp {

constexpr int kClearThreads = 1024;  // 16 wavefronts: with the obstacle rows in LDS (~86 KB for 50 obstacles x 50 rows) one workgroup per CU
constexpr int kClearWaves = kClearThreads / kWave;
// Broad phase: a pair whose centres are further apart than the two bounding radii + kClearSkip is at least kClearSkip metres apart and
// is not summed.  With at most FP_MAX_POINTS x 4095 = 1.05e6 pairs per candidate everything skipped sums to less than
// exp(-48) * 1.05e6 < 2e-15, far below the 1e-12 the definition allows.
constexpr double kClearSkip = 48.0;

// exp(-dist) of the ego box at checked pose i against every obstacle present at that pose's row (obs_row, frenet_ego.h), obstacles in
// column order
__device__ __forceinline__ double pose_clearance(const KernelArgs& ka, const EgoCtx& e, int i, const Obb& ego)
{
    const double r_e = sqrt(fma(ego.hl, ego.hl, ego.hw * ego.hw)) + kClearSkip;
    const double* row = obs_row(e, i, ka.p.check_stride);
    if (!row) return 0.0;  // state_at_time() is None for every obstacle
    double acc = 0.0;
    for (int j = 0; j < e.n_obs; ++j) {
        double ox, oy, oc, os;
        if (!obs_centre(e, row, j, ox, oy, /*nan_ok=*/true)) continue;
        const double R = r_e + e.obs_dim[4 * j + 2];
        const double dx = ox - ego.x, dy = oy - ego.y;
        if (!(fma(dx, dx, dy * dy) < R * R)) continue;  // kClearSkip; also skips NaN (no state in an LDS row)
        obs_heading(e, row, j, oc, os);
        acc += exp(-shape_distance(ka, e, ego, j, ox, oy, oc, os));
    }
    return acc;
}

__global__ __launch_bounds__(kClearThreads) void clearance_rescore_kernel(KernelArgs ka, int lds_doubles, const int* perm)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ int s_list[kClearThreads];  // survivors of the current chunk, in index order
    __shared__ int s_count[kClearWaves];
    const int b = perm ? perm[blockIdx.x] : blockIdx.x;
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
    const fp_params& p = ka.p;
    const int C = p.nd * p.nv * p.nt;
    if (ka.b.skip && ka.b.skip[b]) return;  // not planned: the lattice pass left best_idx = -1 and wrote no table rows
    EgoCtx e;
    stage_ego(ka, b, lds, e, lds_doubles);  // (ends with a barrier)
    double* cost = ka.r.cost_tbl + (size_t)b * C;
    const uint32_t* flag = ka.r.flag_tbl + (size_t)b * C;
    const double* vs = ka.b.v_samples + (size_t)b * p.nv;
    const int cs = p.check_stride;
    const double guess_scale = (double)(e.sp.nx - 1) / (e.sp.knots[e.sp.nx - 1] - e.sp.knots[0]);
    Best mine{0.0, -1};  // (wave-uniform: the best of the survivors this wavefront priced)
    for (int c0 = 0; c0 < C; c0 += kClearThreads) {
        // survivors of the chunk, compacted in index order
        const int cc = c0 + tid;
        const bool alive = cc < C && !(flag[cc] & FP_FLAG_INFEASIBLE);
        const unsigned long long m = __ballot(alive);
        if (lane == 0) s_count[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < kClearWaves; ++w) {
            const int n = s_count[w];
            before += w < wave ? n : 0;
            total += n;
        }
        if (alive) s_list[before + __popcll(m & ((1ull << lane) - 1ull))] = cc;
        __syncthreads();
        for (int k = wave; k < total; k += kClearWaves) {
            const int c = s_list[k];
            const uint32_t fl = flag[c];
            const int N = (int)((fl >> FP_FLAG_N_SHIFT) & 0xfffu), M = (int)(fl >> FP_FLAG_M_SHIFT);
            const double base = cost[c];
            double sum = 0.0;
            if (e.n_obs > 0 && M >= 2) {
                const int iv = c % p.nv, it = (c / p.nv) % p.nt, id = c / (p.nv * p.nt);
                const double T_end = ka.b.t_samples[it];
                const Quintic lat = quintic_bvp(e.d0, e.d_d0, e.d_dd0, ka.b.d_samples[id], 0.0, 0.0, T_end);
                const Quartic lon = quartic_bvp(e.s0, e.s_d0, e.s_dd0, vs[iv], 0.0, T_end);
                const int limit = M < e.horizon_cap ? M : e.horizon_cap;  // poses i = 0, cs, 2 cs, ... < min(M, final_time_step - t_now)
                for (int i = lane * cs; i < limit; i += kWave * cs) {
                    Obb ego;
                    if (checked_pose(p, e.sp, guess_scale, lon, lat, i, M, ego)) sum += pose_clearance(ka, e, i, ego);
                }
            }
            sum = wave_sum_f64(sum);
            // (base_sum + w clearance) / N with base = base_sum / N from the table; no clearance at all leaves the cost's bits alone
            const double priced = sum > 0.0 ? base + p.w_obstacle * sum / (double)N : base;
            if (lane == 0 && sum > 0.0) cost[c] = priced;
            if (priced == priced) mine = best_merge(mine, Best{priced, c});  // (a NaN cost can never win, :266)
        }
        __syncthreads();  // s_list is rewritten by the next chunk
    }
    finish_ego<kClearWaves>(mine, 0, b, ka.r.best_idx, ka.r.best_cost, nullptr, ka.idx_shadow);
}

hipError_t launch_clearance_rescore(const KernelArgs& ka, const int* perm, hipStream_t stream)
{
    if (!ka.r.cost_tbl || !ka.r.flag_tbl || !ka.r.best_idx || !ka.r.best_cost) return hipErrorInvalidValue;  // (internal: the caller provides the tables)
    int lds_doubles = 0;
    // the static tables of the kernel (survivor list, counts, argmins) come out of the same 160 KB
    const int bytes = ego_lds_bytes(ka.p, ka.b, 144 * 1024, &lds_doubles);
    return launch_with_lds<clearance_rescore_kernel>(dim3(ka.b.B), dim3(kClearThreads), bytes, stream, ka, lds_doubles, perm);
}

}  // namespace fp
