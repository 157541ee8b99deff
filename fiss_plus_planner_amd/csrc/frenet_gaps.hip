// frenet_gaps.hip - a time gap to moving obstacles behind the dense FOP pass (fp_gap_mask, added within ABI 18).
//
// has_collision asks whether the ego at pose i overlaps an obstacle at step i.  The time gap asks the same question with the two time
// indices apart: the ego at pose a against the obstacles at step r, 0 < a - r <= lag_follow (the ego arrives where an obstacle was: it
// follows too closely) or 0 < r - a <= lag_lead (an obstacle arrives where the ego was: the ego cut in front of it).  That is the
// post-encroachment time on the candidate's own path; a parked obstacle is overlapped at a lag exactly when it is overlapped at lag 0,
// so the rule is silent for it.  A violating survivor gets FP_FLAG_COLLISION.  The definition: include/frenet_gpu.h.
//
// gap_mask_kernel has the shape of clearance_rescore_kernel: one 768-thread workgroup per ego, staged by stage_ego (spline, obstacle
// sizes and - when they fit - the obstacle rows of the pose grid in LDS; else the rows are read from the scene table: obs_row,
// frenet_ego.h).  a and r are both on the pose grid 0, cs, 2 cs, ..., so those rows are all the rule reads.
//   - cull table, once per ego, when it fits LDS: per (grid pose a, column j) the box of the column's centres over the rows a can pair
//     with (a - lag_follow .. a + lag_lead, a itself left out), grown by the two circumradii and stored as four floats rounded outwards.
//     An ego centre outside that box can overlap the column at none of those rows;
//   - the flag table is walked in chunks of one candidate per thread, the survivors compacted by ballot + popcount;
//   - a wavefront takes one survivor at a time, its lanes the ego poses a >= first (a plan of few poses gives every pose 2, 4 or
//     kGapSplit lanes, which share the pose's columns round-robin).  A lane evaluates its pose once (checked_pose: the arithmetic of the
//     collision check), rejects a column with the cull table's one test and walks the lags only for the columns that remain: a circle
//     test per pair, then the collision check's own predicate (obb_overlap / poly_overlap).  A ballot after every round of poses ends
//     the candidate on the first violation;
//   - the argmin over the survivors that are left: finish_ego.
// An ego without obstacles, or a call with both lags below one grid step, takes neither table nor survivor loop: its argmin is one pass
// over the tables.  No atomics, every verdict a ballot: two runs give the same bits, whatever order workgroups and lanes finish in.
#include "frenet_device.h"
#include "frenet_kernels.h"
#include "frenet_ego.h"
#include "frenet_rules.h"

namespace fp {

// 12 wavefronts, three per SIMD: the narrow phases with a pose's polynomials live need 142 VGPRs, which 16 wavefronts (128) would spill;
// rows and cull table of 50 obstacles x 25 grid poses take ~60 KB of LDS.  tests/gaps_ref.py reads kGapThreads and kGapLdsBytes from
// this file (one integer expression each) to prove that its cases reach the chunk loop's second pass and the paths without LDS tables
constexpr int kGapThreads = 768;
constexpr int kGapWaves = kGapThreads / kWave;
constexpr int kGapSplit = 8;       // at most this many lanes share one pose's columns
constexpr int kGapLdsBytes = 144 * 1024;  // the static tables (survivor list, counts, argmins) come out of the same 160 KB

// a double as the nearest float at or below / at or above it
__device__ __forceinline__ float f32_down(double v)
{
    const float f = (float)v;
    return (double)f > v ? nextafterf(f, -__builtin_inff()) : f;
}
__device__ __forceinline__ float f32_up(double v)
{
    const float f = (float)v;
    return (double)f < v ? nextafterf(f, __builtin_inff()) : f;
}
__global__ __launch_bounds__(kGapThreads) void gap_mask_kernel(KernelArgs ka, GapArgs g, int lds_doubles)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ int s_list[kGapThreads];  // survivors of the current chunk, in index order
    __shared__ int s_count[kGapWaves];
    const int b = g.perm ? g.perm[blockIdx.x] : (int)blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const fp_params& p = ka.p;
    const int C = p.nd * p.nv * p.nt;
    if (ka.b.skip && ka.b.skip[b]) {  // not planned: the dense pass wrote no rows for this ego
        skip_ego(b, ka.r.best_idx, ka.r.best_cost, g.count);
        return;
    }
    EgoCtx e;
    stage_ego(ka, b, lds, e, lds_doubles);  // (ends with a barrier)
    const double* cost = ka.r.cost_tbl + (size_t)b * C;
    uint32_t* flag = ka.r.flag_tbl + (size_t)b * C;
    const double* vs = ka.b.v_samples + (size_t)b * p.nv;
    const int cs = p.check_stride, n_obs = e.n_obs;
    const int Lf = g.lag_follow / cs, Ll = g.lag_lead / cs;  // the lags in grid steps: only pairs on the grid exist
    const double inf = __builtin_inf();
    const double hl = 0.5 * p.veh_l, hw = 0.5 * p.veh_w;
    const double r_e = sqrt(fma(hl, hl, hw * hw));
    const int G = gap_grid_poses(p, e);  // grid poses q = i / cs the ego's horizon and table hold
    const bool active = G > 0 && (Lf > 0 || Ll > 0);  // (block-uniform)
    // ---- cull table [G][n_obs]: x_min, y_min, x_max, y_max of where the ego's centre can be and still reach the column at a paired row
    const float4* bound = nullptr;
    if (active && G <= g.grid_cap) {
        float4* bw = (float4*)(lds + g.bound_off);
        for (int k = tid; k < G * n_obs; k += kGapThreads) {
            const int qa = k / n_obs, j = k - qa * n_obs;
            const int lo = qa - Lf > 0 ? qa - Lf : 0, hi = qa + Ll < G - 1 ? qa + Ll : G - 1;
            double x0 = inf, y0 = inf, x1 = -inf, y1 = -inf;
            for (int qr = lo; qr <= hi; ++qr) {
                if (qr == qa) continue;
                const double* row = obs_row(e, qr * cs, cs);
                double ox, oy;
                if (!row || !obs_centre(e, row, j, ox, oy)) continue;
                x0 = fmin(x0, ox); x1 = fmax(x1, ox);
                y0 = fmin(y0, oy); y1 = fmax(y1, oy);
            }
            const double R = gap_reach(e, r_e, j);
            const float finf = __builtin_inff();
            bw[k] = x1 >= x0 ? make_float4(f32_down(x0 - R), f32_down(y0 - R), f32_up(x1 + R), f32_up(y1 + R)) : make_float4(finf, finf, -finf, -finf);
        }
        bound = bw;
        __syncthreads();
    }
    const double guess_scale = (double)(e.sp.nx - 1) / (e.sp.knots[e.sp.nx - 1] - e.sp.knots[0]);
    // the first grid pose at or behind `first` (>= 1, as large as the caller likes: no sum that could overflow), G when there is none
    const int q_first = (g.first - 1) / cs + 1 < G ? (g.first - 1) / cs + 1 : G;
    Best mine{0.0, -1};  // (active: wave-uniform, the best of the survivors this wavefront cleared; else per lane)
    int close = 0;       // (wave-uniform: survivors of this wavefront that violate)
    for (int c0 = 0; c0 < C; c0 += kGapThreads) {
        const int cc = c0 + tid;
        const bool alive = cc < C && !(flag[cc] & FP_FLAG_INFEASIBLE);
        if (!active) {  // nothing can be flagged: the argmin of the tables as they are
            if (alive) {
                const double own = cost[cc];
                if (own == own) mine = best_merge(mine, Best{own, cc});  // (a NaN cost can never win, :266)
            }
            continue;
        }
        // survivors of the chunk, compacted in index order
        const unsigned long long m = __ballot(alive);
        if (lane == 0) s_count[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < kGapWaves; ++w) {
            const int n = s_count[w];
            before += w < wave ? n : 0;
            total += n;
        }
        if (alive) s_list[before + __popcll(m & ((1ull << lane) - 1ull))] = cc;
        __syncthreads();
        for (int k = wave; k < total; k += kGapWaves) {  // (wave-uniform from here to the candidate's store)
            const int c = s_list[k];
            const uint32_t fl = flag[c];
            const int M = (int)(fl >> FP_FLAG_M_SHIFT);
            // poses i = 0, cs, 2 cs, ... < min(M, final_time_step - t_now) inside the table: grid poses q < n_pose
            const int limit = M < e.horizon_cap ? M : e.horizon_cap;
            int n_pose = limit > 0 ? (limit + cs - 1) / cs : 0;
            if (G < n_pose) n_pose = G;
            bool flagged = false;
            if (M >= 2 && q_first < n_pose) {
                const int iv = c % p.nv, it = (c / p.nv) % p.nt, id = c / (p.nv * p.nt);
                const double T_end = ka.b.t_samples[it];
                const Quintic lat = quintic_bvp(e.d0, e.d_d0, e.d_dd0, ka.b.d_samples[id], 0.0, 0.0, T_end);
                const Quartic lon = quartic_bvp(e.s0, e.s_d0, e.s_dd0, vs[iv], 0.0, T_end);
                int split = 1;
                while (split < kGapSplit && (n_pose - q_first) * split * 2 <= kWave) split *= 2;
                const int per_round = kWave / split, sub = lane & (split - 1);
                for (int qb = q_first; qb < n_pose; qb += per_round) {
                    const int q = qb + lane / split, a = q * cs;
                    bool hit = false;
                    Obb ego;
                    if (q < n_pose && a + e.t_now >= 0 && checked_pose(p, e.sp, guess_scale, lon, lat, a, M, ego)) {
                        hit = gap_pose_hit(ka, e, ego, q, n_pose, Lf, Ll, sub, split, bound, r_e, cs, n_obs);
                    }
                    if (__ballot(hit)) {
                        flagged = true;
                        break;  // the one bit the candidate can get is found
                    }
                }
            }
            if (flagged) {
                if (lane == 0) flag[c] = fl | FP_FLAG_COLLISION;
                ++close;
            } else {
                const double own = cost[c];
                if (own == own) mine = best_merge(mine, Best{own, c});  // (a NaN cost can never win, :266)
            }
        }
        __syncthreads();  // s_list is rewritten by the next chunk
    }
    finish_ego<kGapWaves>(mine, close, b, ka.r.best_idx, ka.r.best_cost, g.count);
}

hipError_t launch_gap_mask(const KernelArgs& ka, GapArgs g, hipStream_t stream)
{
    if (ka.b.B < 1 || !ka.r.cost_tbl || !ka.r.flag_tbl || !ka.r.best_idx || !ka.r.best_cost || g.lag_follow < 0 || g.lag_lead < 0 || g.first < 1 ||
        ka.p.check_stride < 1)
        return hipErrorInvalidValue;  // (internal: fp_gap_mask has checked its arguments)
    // the cull table has one entry of 16 bytes per grid pose and column (ego_lds_bytes' own row count); it goes behind what stage_ego
    // lays out, and comes first when LDS cannot hold both: the rows then stay in the scene table
    const int cs = ka.p.check_stride;
    long rows = (points_cap(ka.p) + cs - 1) / cs;
    const long rows_tab = ((long)ka.b.T_obs + cs - 1) / cs;
    if (rows_tab < rows) rows = rows_tab;
    const long bound_bytes = ka.b.n_obs > 0 && rows > 0 ? rows * ka.b.n_obs * 16 : 0;
    if (g.first > FP_MAX_POINTS) g.first = FP_MAX_POINTS;  // (no trajectory has a point FP_MAX_POINTS: beyond every pose either way)
    const long base_bytes = ((long)ka.b.NX * 9 + (long)ka.b.n_obs * 4) * 8;
    int lds_doubles = 0, bytes = 0;
    if (bound_bytes > 0 && base_bytes + bound_bytes + 8 <= kGapLdsBytes) {
        ego_lds_bytes(ka.p, ka.b, (int)(kGapLdsBytes - bound_bytes - 8), &lds_doubles);
        g.bound_off = (lds_doubles + 1) & ~1;  // (16-byte aligned)
        g.grid_cap = (int)rows;
        bytes = g.bound_off * 8 + (int)bound_bytes;
    } else {
        bytes = ego_lds_bytes(ka.p, ka.b, kGapLdsBytes, &lds_doubles);
        g.bound_off = 0;
        g.grid_cap = 0;
    }
    return launch_with_lds<gap_mask_kernel>(dim3(ka.b.B), dim3(kGapThreads), bytes, stream, ka, g, lds_doubles);
}

}  // namespace fp
