// frenet_predict.hip - the obstacle pose table built on the device from tracks (fp_obstacles_predict, added within ABI 18).
//
// The reference has no predictor: it reads CommonRoad's recorded trajectories through `state_at_time` and skips an obstacle that has no
// state at a step (frenet_optimal_planner.py:187-188).  A caller fed by a tracker has a few numbers per obstacle instead; this kernel
// writes rows of obs_pose [S][T_obs][n_obs][4] from them (the definition: include/frenet_gpu.h):
//   FP_TRACK_LANE  the obstacle follows the scene's reference line at a fixed lateral offset: P(s) + d n(s), yaw = the line's heading;
//   FP_TRACK_ARC   a circular arc in Cartesian coordinates, by its exact chord: x0 + l sinc(u) cos(yaw0 + u), u = kappa l / 2;
//   both           travelled distance l = v0 tau_e + a tau_e^2 / 2 with the clock stopped where a braking obstacle stands still.
//
// obstacles_predict_kernel: one 256-thread workgroup per (scene, slab of rows).  The rows a scene gets are
// [max(t0, 0), min(T_obs, t0 + n_rows)) with t0 read on the device, so the grid is cut over the at most min(T_obs, n_rows) rows behind
// max(t0, 0) and a workgroup whose slab turns out empty leaves at once.  A slab x n_obs x 4 doubles is one contiguous run of memory: the
// flat element index runs along it, a lane writes its element's 32 bytes as two 16-byte vector stores and a wavefront whole 128-byte
// lines.  Staged once per workgroup in LDS: the scene's tracks (6 doubles + the model per column, up to kPredictStagedCols columns;
// beyond that they are read from global memory), and - when the scene has a LANE column and a usable frame - the frame's knots and
// coefficients for spline_segment / spline_frame.
// An element's value is a function of its track, its row and the frame alone - not of the grid, the slab cut or where the output
// lives: two runs, and the two memory spaces, give the same bits.  Plain FP64, no atomics, no scratch.
#include "frenet_device.h"
#include "frenet_kernels.h"
#include "frenet_project.h"

namespace fp {

constexpr int kPredictThreads = 256;
constexpr int kPredictStagedCols = 1024;         // tracks staged in LDS up to this many columns (52 KB; with 1024 knots: 124 KB)
constexpr int kPredictTargetGroups = 2048;       // workgroups a launch aims at (8 per compute unit)
constexpr long kPredictSlabElems = 1L << 24;     // elements per slab at most (the flat index stays far inside 32 bits)

__global__ __launch_bounds__(kPredictThreads) void obstacles_predict_kernel(PredictArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int s = (int)(blockIdx.x / (unsigned)a.n_slabs), slab = (int)(blockIdx.x % (unsigned)a.n_slabs);
    const long t0 = a.t0[s];
    const long rlo = t0 > 0 ? t0 : 0;
    long rhi = t0 + a.n_rows;
    if (rhi > a.T_obs) rhi = a.T_obs;
    if (slab == 0 && tid == 0 && a.final_time_step) a.final_time_step[s] = (int32_t)(rhi < 0 ? 0 : rhi);
    const long r0 = rlo + (long)slab * a.rows_per_slab;
    const long r1 = r0 + a.rows_per_slab < rhi ? r0 + a.rows_per_slab : rhi;
    if (r0 >= r1) return;  // (the whole workgroup: nothing of this slab is inside the scene's rows)
    const int n = a.n_obs;
    // ---- stage: tracks [n][6] | models [n] (as doubles' worth of ints) | knots [nx] | coef [8][nx]
    const double* g_state = a.state + (size_t)s * n * 6;
    const int32_t* g_model = a.model + (size_t)s * n;
    const double* st = g_state;
    const int32_t* model = g_model;
    double* frame_lds = lds;
    int has_lane = 0;
    if (a.stage_tracks) {
        double* l_state = lds;
        int32_t* l_model = (int32_t*)(lds + 6 * (size_t)n);
        for (int i = tid; i < 6 * n; i += kPredictThreads) l_state[i] = g_state[i];
        for (int i = tid; i < n; i += kPredictThreads) {
            const int32_t m = g_model[i];
            l_model[i] = m;
            has_lane |= m == FP_TRACK_LANE;
        }
        st = l_state;
        model = l_model;
        frame_lds = lds + 6 * (size_t)n + (n + 1) / 2;
    } else {
        for (int i = tid; i < n; i += kPredictThreads) has_lane |= g_model[i] == FP_TRACK_LANE;
    }
    has_lane = __syncthreads_or(has_lane);
    // the frame LANE tracks of this scene follow; without a usable one they have no pose
    int nx = 0;
    if (has_lane && a.frame_of_scene && a.nx && a.knots && a.coef) {
        const int f = a.frame_of_scene[s];
        if (f >= 0 && f < a.F) {
            const int nxf = a.nx[f];
            if (nxf >= 2 && nxf <= a.NX) {
                nx = nxf;
                const double* gk = a.knots + (size_t)f * a.NX;
                const double* gc = a.coef + (size_t)f * 8 * a.NX;
                for (int i = tid; i < nx; i += kPredictThreads) frame_lds[i] = gk[i];
                for (int row = 0; row < 8; ++row)
                    for (int i = tid; i < nx; i += kPredictThreads) frame_lds[nx + row * nx + i] = gc[(size_t)row * a.NX + i];
            }
        }
    }
    __syncthreads();
    const SplineLds sp{frame_lds, frame_lds + nx, nx, nx};
    double guess_scale = 0.0;
    if (nx >= 2) {
        guess_scale = (double)(nx - 1) / (frame_lds[nx - 1] - frame_lds[0]);
        if (!(guess_scale < 1e300)) guess_scale = 0.0;  // (NaN / inf: spline_segment divides per point instead)
    }
    const double tick = a.tick_t;
    const unsigned total = (unsigned)(r1 - r0) * (unsigned)n;
    const size_t row_out = a.compact ? (size_t)s * a.span + (size_t)(r0 - rlo) : (size_t)s * a.T_obs + (size_t)r0;
    double2* out = (double2*)(a.obs_pose + row_out * n * 4);
    for (unsigned e = tid; e < total; e += kPredictThreads) {
        const unsigned ri = e / (unsigned)n;
        const int j = (int)(e - ri * (unsigned)n);
        const double tau = (double)(r0 + (long)ri - t0) * tick;
        const int m = model[j];
        const double* q = st + 6 * (size_t)j;
        double x = 0.0, y = 0.0, yaw = 0.0, valid = 0.0;
        if (m == FP_TRACK_LANE || m == FP_TRACK_ARC) {
            const bool arc = m == FP_TRACK_ARC;
            const double v = arc ? q[3] : q[2], acc = arc ? q[4] : q[3];
            // travelled distance: the clock stops where a braking obstacle stands still (a NaN speed stays NaN)
            const double v0 = v < 0.0 ? 0.0 : v;
            double tau_e = tau;
            if (acc < 0.0) {
                const double t_stop = v0 / (-acc);
                if (t_stop < tau) tau_e = t_stop;
            }
            const double l = v0 * tau_e + 0.5 * acc * tau_e * tau_e;
            if (arc) {
                const double x0 = q[0], y0 = q[1], yaw0 = q[2], kappa = q[5];
                if (finite_f64(x0) && finite_f64(y0) && finite_f64(yaw0) && finite_f64(v) && finite_f64(acc) && finite_f64(kappa)) {
                    const double u = kappa * l / 2.0;
                    const double sinc = fabs(u) < 1e-4 ? 1.0 - u * u / 6.0 : sin(u) / u;
                    double sn, cs;
                    sincos(yaw0 + u, &sn, &cs);
                    x = x0 + l * sinc * cs;
                    y = y0 + l * sinc * sn;
                    yaw = yaw0 + kappa * l;
                    valid = 1.0;
                }
            } else {
                const double sv = q[0] + l, d = q[1];
                const int seg = nx >= 2 && finite_f64(d) ? spline_segment(sp, sv, -1, guess_scale) : -1;  // (-1: s is NaN or off the line)
                if (seg >= 0) {
                    double px, py, tx, ty;
                    spline_frame(sp, seg, sv - sp.knots[seg], px, py, tx, ty);
                    frenet_to_cartesian(px, py, tx, ty, d, x, y);
                    yaw = atan2(ty, tx);
                    valid = 1.0;
                }
            }
        }
        out[2 * (size_t)e] = make_double2(x, y);
        out[2 * (size_t)e + 1] = make_double2(yaw, valid);
    }
}

hipError_t launch_obstacles_predict(PredictArgs a, hipStream_t stream)
{
    if (a.S < 1 || a.T_obs < 1 || a.n_obs < 1 || a.n_rows < 1 || a.F < 0 || a.NX < 0 || a.NX > FP_MAX_KNOTS || !a.model || !a.state || !a.t0 || !a.obs_pose ||
        ((uintptr_t)a.obs_pose & 15u))
        return hipErrorInvalidValue;  // (internal: fp_obstacles_predict has checked its arguments)
    // the slab cut: a function of the sizes alone (t0 lives on the device).  span = the most rows a scene can get
    a.span = a.n_rows < a.T_obs ? a.n_rows : a.T_obs;
    long slabs = (kPredictTargetGroups + (long)a.S - 1) / a.S;
    if (slabs > a.span) slabs = a.span;
    long rps = (a.span + slabs - 1) / slabs;
    const long cap = kPredictSlabElems / a.n_obs;
    if (rps > (cap < 1 ? 1 : cap)) rps = cap < 1 ? 1 : cap;
    slabs = (a.span + rps - 1) / rps;
    if ((long)a.S * slabs > 0x7fffffffL) return hipErrorInvalidValue;
    a.rows_per_slab = (int)rps;
    a.n_slabs = (int)slabs;
    a.stage_tracks = a.n_obs <= kPredictStagedCols ? 1 : 0;
    const bool frames = a.F > 0 && a.NX >= 2 && a.frame_of_scene && a.nx && a.knots && a.coef;
    const int bytes = (a.stage_tracks ? (6 * a.n_obs + (a.n_obs + 1) / 2) * 8 : 0) + (frames ? 9 * a.NX * 8 : 0);  // <= 52 KB + 72 KB
    return launch_with_lds<obstacles_predict_kernel>(dim3((unsigned)(a.S * slabs)), dim3(kPredictThreads), bytes, stream, a);
}

}  // namespace fp
