// frenet_margins.hip - the obstacle margin of a handful of chosen plans per ego (fp_traj_margins, added within ABI 18).
//
// For plane k and ego b the plan is lattice candidate best_idx[k][b] or the explicit end state end_state[k][b]; its margin is the
// smallest Euclidean distance between the ego footprint at a checked pose and an obstacle valid at that pose's row, with the pose and
// the column where it occurs (the definition: include/frenet_gpu.h).  Nothing is priced and nothing is decided here: the kernel reads
// the batch and writes three numbers per plan.
//
// margins_kernel: one 512-thread workgroup per ego, staged by stage_ego like the clearance rescoring kernel (spline, obstacle sizes
// and - when they fit kMarginLdsBytes - the rows the pose set can touch in LDS, once for all K planes; else the rows are read from the
// scene table: see obs_row, frenet_ego.h).  A wavefront takes one plane at a time:
//   - M, the first point off the reference line, by a ballot over the longitudinal quartic (64 points per round, any N up to
//     FP_MAX_POINTS: no series is written, so the 128-point chunks of the series writers do not apply);
//   - the lanes are the checked poses (i = 0, pose_stride, ... < min(M, final_time_step - t_now)); a plan with at most 32 poses gives
//     every pose 2, 4 or kMarginSplit lanes, which share the pose's columns round-robin.  A lane evaluates its pose from the
//     polynomials (see checked_pose: the arithmetic of the collision check and of the clearance term) and keeps it in registers;
//   - broad phase: a pair is skipped only when (centre distance) > (lane's minimum + both circumradii), the right-hand side widened by
//     1e-9 relative + 1e-9 absolute - the true distance is at least centre distance - circumradii, so a skipped pair is strictly
//     further away than what the lane already holds and can neither win nor tie; a lane that holds a contact (distance 0) is done:
//     its later pairs come later in the tie order;
//   - the lexicographic minimum of (dist, i, j) over the lanes by six __shfl_xor steps; lane 0 writes the plane's three outputs.
// No atomics, no VGPR spill, nothing depends on the order workgroups run in: two runs give the same bits.
#include "frenet_device.h"
#include "frenet_kernels.h"
#include "frenet_ego.h"

namespace fp {

constexpr int kMarginThreads = 512;  // 8 wavefronts: the K = 8 planes of a typical call, one each
constexpr int kMarginWaves = kMarginThreads / kWave;
constexpr int kMarginSplit = 8;      // at most this many lanes share one pose's columns
// LDS budget of the staged tables (the kernel's static LDS is nothing): config 3 (50 obstacles, T_obs = 50: 25 rows = 40 KB at stride
// 2, 50 rows = 80 KB at stride 1, + the spline) fits with one workgroup per CU; 128 rows x 40 obstacles (160 KB) do not and take the
// scene-table path.
constexpr int kMarginLdsBytes = 144 * 1024;

struct MarginMin {
    double d;
    int i, j;
};
__device__ __forceinline__ MarginMin margin_merge(MarginMin a, MarginMin b)
{
    const bool take_b = b.d < a.d || (b.d == a.d && (b.i < a.i || (b.i == a.i && b.j < a.j)));
    return take_b ? b : a;
}

__global__ __launch_bounds__(kMarginThreads) void margins_kernel(KernelArgs ka, MarginArgs m, int lds_doubles)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int b = m.perm ? m.perm[blockIdx.x] : (int)blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const fp_params& p = ka.p;
    const int B = ka.b.B, K = m.K;
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    if (ka.b.skip && ka.b.skip[b]) {  // not planned: no trajectory on any plane, and none of the ego's rows is read
        for (int k = tid; k < K; k += kMarginThreads) {
            const size_t o = (size_t)k * B + b;
            m.min_dist[o] = nan; m.min_step[o] = -1; m.min_obs[o] = -1;
        }
        return;
    }
    EgoCtx e;
    stage_ego(ka, b, lds, e, lds_doubles);  // (ends with a barrier; p.check_stride is the call's pose_stride)
    const int C = p.nd * p.nv * p.nt, cs = p.check_stride, n_obs = e.n_obs;
    const double k0 = e.sp.knots[0], kl = e.sp.knots[e.sp.nx - 1];
    const double guess_scale = (double)(e.sp.nx - 1) / (kl - k0);
    const double hl = 0.5 * p.veh_l, hw = 0.5 * p.veh_w;
    const double r_e = sqrt(fma(hl, hl, hw * hw));
    for (int k = wave; k < K; k += kMarginWaves) {  // (wave-uniform from here to the plane's store)
        const size_t o = (size_t)k * B + b;
        double d_end = nan, v_end = nan, T = nan;
        if (m.end_state) {
            const double* es = m.end_state + o * 3;
            d_end = es[0]; v_end = es[1]; T = es[2];
        } else {
            const int c = m.best_idx[o];
            if (c >= 0 && c < C) {  // (an index beyond the lattice is "no trajectory" for a device caller)
                const int iv = c % p.nv, it = (c / p.nv) % p.nt, id = c / (p.nv * p.nt);
                d_end = ka.b.d_samples[id]; v_end = ka.b.v_samples[(size_t)b * p.nv + iv]; T = ka.b.t_samples[it];
            }
        }
        const int N = (T == T) ? arange_len(T, p.tick_t) : 0;
        if (N <= 0 || N > points_cap(p) || !(d_end == d_end) || !(v_end == v_end)) {
            if (lane == 0) { m.min_dist[o] = nan; m.min_step[o] = -1; m.min_obs[o] = -1; }
            continue;
        }
        const Quintic lat = quintic_bvp(e.d0, e.d_d0, e.d_dd0, d_end, 0.0, 0.0, T);
        const Quartic lon = quartic_bvp(e.s0, e.s_d0, e.s_dd0, v_end, 0.0, T);
        // M: the first point whose s is outside [first knot, last knot) (spline_segment's range test)
        int M = N;
        for (int i0 = 0; i0 < N; i0 += kWave) {
            const int i = i0 + lane;
            const double t = (double)i * p.tick_t;
            const double sv = quartic_pos(lon, t);
            const unsigned long long off = __ballot(i < N && (!(sv >= k0) || !(sv < kl)));
            if (off) { M = i0 + __ffsll((long long)off) - 1; break; }
        }
        MarginMin mine{inf, 0x7fffffff, 0x7fffffff};
        // poses i = 0, cs, 2 cs, ... < min(M, final_time_step - t_now); a series of fewer than two points has no heading: no pose
        const int limit = M < e.horizon_cap ? M : e.horizon_cap;
        if (n_obs > 0 && M >= 2 && limit > 0) {
            const int n_pose = (limit + cs - 1) / cs;
            int split = 1;
            while (split < kMarginSplit && n_pose * split * 2 <= kWave) split *= 2;
            const int per_round = kWave / split, sub = lane & (split - 1);
            for (int q = lane / split; q < n_pose; q += per_round) {
                if (mine.d == 0.0) break;  // a contact: every later pair of this lane loses the tie
                const int i = q * cs;
                const double* row = obs_row(e, i, cs);
                Obb ego;
                if (!row || !checked_pose(p, e.sp, guess_scale, lon, lat, i, M, ego)) continue;  // no obstacle has a state there / off the line
                for (int j = sub; j < n_obs; j += split) {
                    if (mine.d == 0.0) break;
                    double ox, oy, oc, os;
                    if (!obs_centre(e, row, j, ox, oy)) continue;
                    const double reach = (mine.d + (r_e + e.obs_dim[4 * j + 2])) * (1.0 + 1e-9) + 1e-9;
                    const double dx = ox - ego.x, dy = oy - ego.y;
                    if (fma(dx, dx, dy * dy) > reach * reach) continue;  // strictly further than the lane's minimum
                    obs_heading(e, row, j, oc, os);
                    const double dist = shape_distance(ka, e, ego, j, ox, oy, oc, os);
                    if (dist < mine.d) mine = MarginMin{dist, i, j};  // (poses and columns ascending: the first of equal distances stays)
                }
            }
        }
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            MarginMin other;
            other.d = __shfl_xor(mine.d, off, kWave);
            other.i = __shfl_xor(mine.i, off, kWave);
            other.j = __shfl_xor(mine.j, off, kWave);
            mine = margin_merge(mine, other);
        }
        if (lane == 0) {
            const bool none = !(mine.d < inf);
            m.min_dist[o] = none ? inf : mine.d;
            m.min_step[o] = none ? -1 : mine.i;
            m.min_obs[o] = none ? -1 : mine.j;
        }
    }
}

hipError_t launch_traj_margins(const KernelArgs& ka, const MarginArgs& m, hipStream_t stream)
{
    if (ka.b.B < 1 || m.K < 1 || m.K > FP_MAX_RANK || ka.p.check_stride < 1 || (m.best_idx == nullptr) == (m.end_state == nullptr) || !m.min_dist || !m.min_step ||
        !m.min_obs)
        return hipErrorInvalidValue;  // (internal: fp_traj_margins has checked its arguments)
    int lds_doubles = 0;
    const int bytes = ego_lds_bytes(ka.p, ka.b, kMarginLdsBytes, &lds_doubles);
    return launch_with_lds<margins_kernel>(dim3(ka.b.B), dim3(kMarginThreads), bytes, stream, ka, m, lds_doubles);
}

}  // namespace fp
