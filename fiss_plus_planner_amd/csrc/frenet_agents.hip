// frenet_agents.hip - the chosen plans of grouped egos as obstacle columns of each other's scenes (fp_obstacles_from_plans, added
// within ABI 18).
//
// Member k of a group owns column col_base + k of the scene of every member of its group; rows t_now[a] .. t_now[a] + n_rows - 1 of
// that column get the poses of ego a's plan (lattice candidate best_idx[a] or end state end_state[a]): the series' own x, y, yaw up to
// its last point, the tail rule behind it, (0, 0, 0, 0) where there is no pose - and in a's own scene, where an ego never sees itself
// (the definition: include/frenet_gpu.h).
//
// agents_kernel: one 256-thread workgroup per DESTINATION member - row r of its scene holds the group's columns side by side, so the
// lanes of one row write one contiguous run.  The sources of the group are taken in rounds of kAgentChunk:
//   1. a wavefront per source builds the source's quartic / quintic from its ego row and finds M, the first point off its reference
//      line, by margins_kernel's ballot loop; polynomials, M, frame and clock go to LDS (a source without a plan: M = 0);
//   2. behind a barrier the lanes run over (row, source): a lane evaluates its pose - two Cartesian points and the heading of the step
//      between them, the arithmetic of checked_pose and of every series dump - and writes its element as two 16-byte stores.
// Members of one group may follow different frames: a lane reads its source's knots and coefficients from global memory (L2) with
// spline_segment's uniform-spacing guess.  Every destination recomputes its sources (g x g x n_rows poses per group): nothing next to
// the g x g x n_rows x 32 bytes written.
// An element is a function of its source's state, plan, row and frame alone - not of the grid, the rounds or where the table lives:
// two runs, and the two memory spaces, give the same bits.  Plain FP64, no atomics, no scratch.
#include "frenet_device.h"
#include "frenet_kernels.h"
#include "frenet_project.h"

namespace fp {

constexpr int kAgentThreads = 256;
constexpr int kAgentWaves = kAgentThreads / kWave;
constexpr int kAgentChunk = 64;  // sources per round (7 KB of LDS); a workgroup's lanes cover at least four rows of a round at a time

struct AgentPlan {
    Quartic lon;
    Quintic lat;
    double guess_scale;
    int src;    // the ego, or -1: not an ego of the batch (nothing of its column is written)
    int M;      // points of the Cartesian series, 0: no plan
    int frame, nx;
    int t_now;
    int pad;
};

__global__ __launch_bounds__(kAgentThreads) void agents_kernel(KernelArgs ka, AgentArgs a)
{
    __shared__ AgentPlan s_plan[kAgentChunk];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const fp_params& p = ka.p;
    const fp_batch& bt = ka.b;
    const int m = (int)blockIdx.x;
    // the group of member m: bisect_right(group_ptr, m) - 1 (an empty group owns no member)
    int lo = 0, hi = a.G + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (m < a.group_ptr[mid]) hi = mid; else lo = mid + 1;
    }
    const int g = lo - 1;
    if (g < 0 || g >= a.G) return;  // (every test up to the first barrier is the same for the whole workgroup)
    const int g0 = a.group_ptr[g], g1 = a.group_ptr[g + 1];
    if (g0 < 0 || g1 > a.n_members || m < g0 || m >= g1) return;
    const int gs = g1 - g0;
    const int dest = a.members[m];
    if (dest < 0 || dest >= bt.B) return;
    const int sd = bt.scene_of[dest];
    if (sd < 0 || sd >= bt.S || a.col_base < 0 || (long)a.col_base + gs > bt.n_obs) return;
    const long T_obs = bt.T_obs;
    if (tid == 0 && a.final_time_step) {
        long end = (long)bt.t_now[dest] + a.n_rows;
        end = end < 0 ? 0 : (end > T_obs ? T_obs : end);
        a.final_time_step[sd] = (int32_t)end;
    }
    const int C = p.nd * p.nv * p.nt;
    double* scene = a.obs_pose + (size_t)sd * (size_t)T_obs * bt.n_obs * 4;
    for (int c0 = 0; c0 < gs; c0 += kAgentChunk) {
        const int cn = gs - c0 < kAgentChunk ? gs - c0 : kAgentChunk;
        // ---- 1. a wavefront per source: polynomials and M (wave-uniform up to the store)
        for (int k = wave; k < cn; k += kAgentWaves) {
            AgentPlan pl;
            pl.lon = Quartic{0.0, 0.0, 0.0, 0.0, 0.0};
            pl.lat = Quintic{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            pl.guess_scale = 0.0;
            pl.src = a.members[g0 + c0 + k];
            pl.M = 0; pl.frame = 0; pl.nx = 0; pl.t_now = 0; pl.pad = 0;
            if (pl.src < 0 || pl.src >= bt.B) {
                pl.src = -1;
            } else {
                const int b = pl.src;
                pl.t_now = bt.t_now[b];
                const int f = bt.frame_of[b];
                const int nx = f >= 0 && f < bt.F ? bt.nx[f] : 0;
                double d_end = __builtin_nan(""), v_end = d_end, T = d_end;
                if (!(bt.skip && bt.skip[b]) && nx >= 2 && nx <= bt.NX && b != dest) {  // (its own plan is of no use to the destination)
                    if (a.end_state) {
                        const double* es = a.end_state + (size_t)b * 3;
                        if (finite_f64(es[0]) && finite_f64(es[1]) && finite_f64(es[2])) { d_end = es[0]; v_end = es[1]; T = es[2]; }
                    } else {
                        const int c = a.best_idx[b];
                        if (c >= 0 && c < C) {  // (decoded as margins_kernel does)
                            const int iv = c % p.nv, it = (c / p.nv) % p.nt, id = c / (p.nv * p.nt);
                            d_end = bt.d_samples[id]; v_end = bt.v_samples[(size_t)b * p.nv + iv]; T = bt.t_samples[it];
                        }
                    }
                }
                const int N = (T == T) ? arange_len(T, p.tick_t) : 0;
                if (N >= 1 && N <= points_cap(p) && d_end == d_end && v_end == v_end) {
                    const double* eg = bt.ego + (size_t)b * 6;
                    pl.lon = quartic_bvp(eg[0], eg[1], eg[2], v_end, 0.0, T);
                    pl.lat = quintic_bvp(eg[3], eg[4], eg[5], d_end, 0.0, 0.0, T);
                    const double* kn = bt.knots + (size_t)f * bt.NX;
                    const double k0 = kn[0], kl = kn[nx - 1];
                    int M = N;  // the first point whose s is outside [first knot, last knot) (spline_segment's range test)
                    for (int i0 = 0; i0 < N; i0 += kWave) {
                        const int i = i0 + lane;
                        const double sv = quartic_pos(pl.lon, (double)i * p.tick_t);
                        const unsigned long long off = __ballot(i < N && (!(sv >= k0) || !(sv < kl)));
                        if (off) { M = i0 + __ffsll((long long)off) - 1; break; }
                    }
                    if (M >= 2) {  // (a series of fewer than two points has no heading: no pose)
                        pl.M = M; pl.frame = f; pl.nx = nx;
                        const double gsc = (double)(nx - 1) / (kl - k0);
                        pl.guess_scale = gsc < 1e300 ? gsc : 0.0;  // (NaN / inf: spline_segment divides per point instead)
                    }
                }
            }
            if (lane == 0) s_plan[k] = pl;
        }
        __syncthreads();
        // ---- 2. the lanes over (row, source): lane's source k = tid % cn, its rows i = tid / cn, + rows_per_pass, ...
        int ilo = 0x7fffffff, ihi = 0;  // the steps some source of the round has a row of the table for
        for (int k = 0; k < cn; ++k) {
            if (s_plan[k].src < 0) continue;
            const long t = s_plan[k].t_now;
            const long l = t < 0 ? -t : 0, h = T_obs - t < a.n_rows ? T_obs - t : a.n_rows;
            if (l < ilo) ilo = (int)l;
            if (h > ihi) ihi = (int)h;
        }
        const int rows_per_pass = kAgentThreads / cn, k = tid % cn;
        if (tid < rows_per_pass * cn && s_plan[k].src >= 0) {
            const AgentPlan pl = s_plan[k];
            const SplineLds sp{bt.knots + (size_t)pl.frame * bt.NX, bt.coef + (size_t)pl.frame * 8 * bt.NX, pl.nx, bt.NX};
            const int M = pl.M;
            double2* col = (double2*)(scene + (size_t)(a.col_base + c0 + k) * 4);
            for (int i = ilo + tid / cn; i < ihi; i += rows_per_pass) {
                const long r = (long)pl.t_now + i;
                if (r < 0 || r >= T_obs) continue;
                double x = 0.0, y = 0.0, yaw = 0.0, valid = 0.0;
                if (M >= 2 && (i < M || a.tail != FP_TAIL_NONE)) {
                    const int i0 = i + 1 < M ? i : M - 2;
                    double x0, y0, x1, y1;
                    if (traj_point(p, sp, pl.guess_scale, pl.lon, pl.lat, i0, x0, y0) && traj_point(p, sp, pl.guess_scale, pl.lon, pl.lat, i0 + 1, x1, y1)) {
                        const double sx = x1 - x0, sy = y1 - y0;
                        x = i0 == i ? x0 : x1;
                        y = i0 == i ? y0 : y1;
                        if (i >= M && a.tail == FP_TAIL_COAST) {
                            const double n = (double)(i - M + 1);
                            x = fma(n, sx, x1);
                            y = fma(n, sy, y1);
                        }
                        yaw = atan2(sy, sx);
                        valid = 1.0;
                    }
                }
                double2* out = col + (size_t)r * bt.n_obs * 2;
                out[0] = make_double2(x, y);
                out[1] = make_double2(yaw, valid);
            }
        }
        __syncthreads();  // (the next round rewrites s_plan)
    }
}

hipError_t launch_obstacles_from_plans(const KernelArgs& ka, const AgentArgs& a, hipStream_t stream)
{
    if (a.G < 0 || a.n_members < 0 || a.n_rows < 1 || a.tail < FP_TAIL_NONE || a.tail > FP_TAIL_COAST || (a.best_idx == nullptr) == (a.end_state == nullptr) ||
        !a.obs_pose || ((uintptr_t)a.obs_pose & 15u))
        return hipErrorInvalidValue;  // (internal: fp_obstacles_from_plans has checked its arguments)
    if (a.G == 0 || a.n_members == 0) return hipSuccess;
    if (!a.group_ptr || !a.members) return hipErrorInvalidValue;
    hipLaunchKernelGGL(agents_kernel, dim3((unsigned)a.n_members), dim3(kAgentThreads), 0, stream, ka, a);
    return hipGetLastError();
}

}  // namespace fp
