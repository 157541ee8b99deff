// frenet_ego.h - the per-ego staging the one-workgroup-per-ego kernels share (lane-per-candidate lattice, explicit end states, audit,
// clearance rescoring): the ego's start state, its reference-line spline and the rows of its obstacle table that the collision
// horizon can touch, in LDS.
#pragma once

#include "frenet_device.h"
#include "frenet_kernels.h"

namespace fp {

// ---------------------------------------------------------------------------
// per-workgroup shared state
// ---------------------------------------------------------------------------
struct EgoCtx {
    // start state
    double s0, s_d0, s_dd0, d0, d_d0, d_dd0;
    double target_speed;
    // spline in LDS
    SplineLds sp;
    // obstacles
    const double* obs_lds;   // [rows][n_obs][4] = x, y, cos, sin (x = NaN: no state) or nullptr
    const double* obs_dim;   // [n_obs][4] = hl, hw, bounding radius, unused
    const double* obs_glb;   // global pose table of the scene (fallback when LDS is too small)
    int n_obs, T_obs, rows, t_now, horizon_cap;  // horizon_cap = final_time_step - t_now
    size_t col0;             // first obstacle column of the ego's scene (scene * n_obs): index base of obs_nvert / obs_poly
};

__device__ __forceinline__ int lds_layout_doubles(int nx, int n_obs, int rows)
{
    return nx * 9 + n_obs * 4 + rows * n_obs * 4;
}

// Stage spline + obstacle rows of ego `b` into LDS.  All threads of the block take part.
__device__ inline void stage_ego(const KernelArgs& ka, int b, double* lds, EgoCtx& e, int lds_doubles)
{
    const fp_batch& bt = ka.b;
    const int tid = threadIdx.x, nth = blockDim.x;
    const double* eg = bt.ego + (size_t)b * 6;
    e.s0 = eg[0]; e.s_d0 = eg[1]; e.s_dd0 = eg[2]; e.d0 = eg[3]; e.d_d0 = eg[4]; e.d_dd0 = eg[5];
    e.target_speed = bt.target_speed[b];
    const int f = bt.frame_of[b];
    const int nx = bt.nx[f];
    const int NX = bt.NX;
    double* knots = lds;
    double* coef = lds + nx;
    const double* gk = bt.knots + (size_t)f * NX;
    const double* gc = bt.coef + (size_t)f * 8 * NX;
    for (int i = tid; i < nx; i += nth) knots[i] = gk[i];
    for (int i = tid; i < 8 * nx; i += nth) {
        const int r = i / nx, c = i - r * nx;
        coef[r * nx + c] = gc[(size_t)r * NX + c];
    }
    e.sp.knots = knots;
    e.sp.coef = coef;
    e.sp.nx = nx;
    e.sp.ld = nx;

    const int sc = bt.scene_of[b];
    e.t_now = bt.t_now[b];
    e.n_obs = (sc >= 0) ? bt.n_obs : 0;
    e.T_obs = bt.T_obs;
    e.obs_lds = nullptr;
    e.obs_dim = nullptr;
    e.obs_glb = nullptr;
    e.rows = 0;
    e.horizon_cap = 0;
    e.col0 = (size_t)(sc >= 0 ? sc : 0) * bt.n_obs;
    if (e.n_obs > 0) {
        const int n = e.n_obs;
        e.horizon_cap = bt.final_time_step[sc] - e.t_now;
        const int stride = ka.p.check_stride;
        int hmax = e.horizon_cap < points_cap(ka.p) ? e.horizon_cap : points_cap(ka.p);
        if (hmax < 0) hmax = 0;
        int rows = (hmax + stride - 1) / stride;  // poses 0, stride, 2*stride, ... < hmax
        // rows past the end of the table hold no state at all: do not stage them
        const int in_table = bt.T_obs - e.t_now;
        const int rows_tab = in_table > 0 ? (in_table + stride - 1) / stride : 0;
        if (rows_tab < rows) rows = rows_tab;
        double* dim = coef + 8 * nx;
        const double* gd = bt.obs_dims + (size_t)sc * n * 2;
        for (int j = tid; j < n; j += nth) {
            const double hl = 0.5 * gd[2 * j], hw = 0.5 * gd[2 * j + 1];
            dim[4 * j] = hl;
            dim[4 * j + 1] = hw;
            dim[4 * j + 2] = sqrt(fma(hl, hl, hw * hw));
            dim[4 * j + 3] = 0.0;
        }
        e.obs_dim = dim;
        e.obs_glb = bt.obs_pose + (size_t)sc * bt.T_obs * n * 4;
        if (lds_layout_doubles(nx, n, rows) <= lds_doubles) {
            double* tab = dim + 4 * n;
            for (int i = tid; i < rows * n; i += nth) {
                const int r = i / n, j = i - r * n;
                const int ts = r * stride + e.t_now;
                double x = __builtin_nan(""), y = 0.0, c = 1.0, s = 0.0;
                if (ts >= 0 && ts < bt.T_obs) {
                    const double* ps = e.obs_glb + ((size_t)ts * n + j) * 4;
                    if (ps[3] != 0.0) {
                        x = ps[0];
                        y = ps[1];
                        sincos_snapped(ps[2], s, c);
                    }
                }
                tab[4 * i] = x; tab[4 * i + 1] = y; tab[4 * i + 2] = c; tab[4 * i + 3] = s;
            }
            e.obs_lds = tab;
            e.rows = rows;
        }
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------
// The reader of the obstacle rows stage_ego leaves: LDS rows are x, y, cos, sin with x = NaN for "no state", one row per checked pose
// (row i / check_stride); scene-table rows are x, y, yaw, valid with valid == 0.0 for "no state", one row per time step (row i + t_now).
// Column j of either is obstacle e.col0 + j of obs_nvert / obs_poly.  A caller keeps its own broad phase between obs_centre and
// obs_heading: the trigonometry of a table row is paid only for the pairs that pass it.
// ---------------------------------------------------------------------------
// the row of checked pose i, or nullptr: the pose lies outside the table, where no obstacle has a state
__device__ __forceinline__ const double* obs_row(const EgoCtx& e, int i, int stride)
{
    if (e.obs_lds) return i / stride < e.rows ? e.obs_lds + (size_t)(i / stride) * e.n_obs * 4 : nullptr;
    const int ts = i + e.t_now;
    return ts >= 0 && ts < e.T_obs ? e.obs_glb + (size_t)ts * e.n_obs * 4 : nullptr;
}
// centre of column j in that row; false: the obstacle has no state there.  nan_ok: the caller's next test is false for a NaN centre
// anyway (a broad phase written as !(d2 < R2)) and takes an LDS row's "no state" as that NaN - one compare less per pair
__device__ __forceinline__ bool obs_centre(const EgoCtx& e, const double* row, int j, double& ox, double& oy, bool nan_ok = false)
{
    ox = row[4 * j];
    oy = row[4 * j + 1];
    return e.obs_lds ? nan_ok || ox == ox : row[4 * j + 3] != 0.0;
}
// cos / sin of the column's orientation: stored in LDS, sincos_snapped from the table
__device__ __forceinline__ void obs_heading(const EgoCtx& e, const double* row, int j, double& oc, double& os)
{
    oc = row[4 * j + 2];
    os = row[4 * j + 3];
    if (!e.obs_lds) sincos_snapped(row[4 * j + 2], os, oc);
}
// vertices of the column's polygon (0: a rectangle of the staged sizes) and its ring
__device__ __forceinline__ int obs_nvert(const KernelArgs& ka, const EgoCtx& e, int j) { return ka.b.obs_nvert ? ka.b.obs_nvert[e.col0 + j] : 0; }
__device__ __forceinline__ const double* obs_ring(const KernelArgs& ka, const EgoCtx& e, int j) { return ka.b.obs_poly + (e.col0 + j) * 2 * (size_t)ka.b.poly_stride; }
// Euclidean distance of the ego footprint to column j at pose (ox, oy, oc, os), whatever the column's shape
__device__ __forceinline__ double shape_distance(const KernelArgs& ka, const EgoCtx& e, const Obb& ego, int j, double ox, double oy, double oc, double os)
{
    const int nvert = obs_nvert(ka, e, j);
    return nvert > 0 ? poly_distance(ego, ox, oy, oc, os, obs_ring(ka, e, j), nvert) : obb_distance(ego, Obb{ox, oy, oc, os, e.obs_dim[4 * j], e.obs_dim[4 * j + 1]});
}

// dynamic LDS of a kernel that calls stage_ego: the spline and the obstacle sizes always, the pose rows when they fit max_bytes
inline int ego_lds_bytes(const fp_params& p, const fp_batch& b, int max_bytes, int* lds_doubles)
{
    int hmax = points_cap(p);
    const int rows = (hmax + p.check_stride - 1) / p.check_stride;
    const long base = (long)b.NX * 9 + (long)b.n_obs * 4;
    long full = base + (long)rows * b.n_obs * 4;
    // never more rows than the table has
    const long rows_tab = ((long)b.T_obs + p.check_stride - 1) / p.check_stride;
    if (rows_tab < rows) full = base + rows_tab * b.n_obs * 4;
    long use = full * 8 <= max_bytes ? full : base;  // obstacle rows stay in HBM/L2 when they do not fit
    *lds_doubles = (int)use;
    return (int)(use * 8);
}

}  // namespace fp
