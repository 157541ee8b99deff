// frenet_lattice_plan.h - how a launch of the fused lattice kernel (frenet_lattice_fused.hip) is shaped: the LDS carve-up of its
// instances and plan_lattice, the one function that decides a launch (does it fit, instance, workgroups per CU, coefficient window,
// appended workgroups, LDS, tail split, grid).  Host-side arithmetic only: no HIP call, no allocation (tests/test_lattice_plan_cpu.py
// prints plans on a machine without a GPU).
#pragma once

#include "frenet_device.h"
#include "frenet_fissplus.h"
#include "frenet_kernels.h"

namespace fp {

constexpr int kThreads = 512;
#ifndef FP_GROUP_THREADS
#define FP_GROUP_THREADS 1024  // threads per workgroup of the grouped instances
#endif
// block-wide list of (row, obstacle) items that pass the group test (+ their poses, 32 B each).  Two kernel variants: OCC = 4 waves per
// SIMD (two workgroups per CU, up to 128 VGPRs, winner epilogue inside) and OCC = 6 (THREE workgroups per CU: 80 VGPRs - a few spill
// - and at most 53 KB of LDS, so a shorter list; no winner epilogue, the batches it serves get theirs from winner_traj_kernel or from the
// appended epilogue workgroups) and, for BASELINE.json's dense shape, OCC = 8 (FOUR per CU: 64 VGPRs, none spilled, and the 40 KB "slim"
// layout of make_layout with a 256-entry list - the largest ego of the headline workload keeps 221; longer lists take the chunked redo)
__host__ __device__ constexpr int item_cap(int occ) { return occ > 6 ? 256 : occ > 4 ? 320 : 512; }
constexpr int kItemCapMax = 512;
// bits of the obstacle index in a packed walk item (row << bits | obstacle), or 0 where such a code does not fit the list's 16 bits
constexpr int item_shift(int n_obs, int rows)
{
    int s = 0;
    while ((1 << s) < n_obs) ++s;
    return s > 0 && ((long long)(rows > 0 ? rows - 1 : 0) << s) + (n_obs - 1) <= 0xFFFF ? s : 0;
}
static_assert(item_shift(50, 25) == 6 && item_shift(10, 50) == 4, "the two compiled-in shapes pack their items");
static_assert(item_shift(64, 1024) == 6 && item_shift(65, 1024) == 0 && item_shift(64, 1025) == 0, "(1023 << 6 | 63 is the last code that fits 16 bits)");
static_assert(item_shift(1, 25) == 0 && item_shift(2, 25) == 1 && item_shift(4095, 16) == 12 && item_shift(4095, 17) == 0, "one obstacle has no bits to pack");

// LDS carve-up (all offsets in bytes, 16-byte aligned)
struct Layout {
    int knots, coef, lut, dim, pose, frames, dmax, ddmax, wfat, grp, iqueue, pows, samples, lon_sum, lat_sum, lon_meta, qlon, qlat, box, coll, queue, cnt, nslice, best, konst, nvert, poly, total;
};

__host__ __device__ inline int align16(int v) { return (v + 15) & ~15; }

// The collision stages are a WALK: every wavefront takes one lon profile (T, v) at a time and does everything for it by itself - frames,
// fan half-widths, broad phase, narrow phase - with NO workgroup barrier.  So the per-profile tables (frames, half-widths, hit list) are
// per WAVEFRONT (nwaves of each); the lateral bounds and coefficients of all slices are computed once per ego.
// Polygon columns (POLY instances): the vertex counts always sit in LDS, the rings when they are small (kPolyLdsMax: a few KB keep the
// three-workgroups-per-CU instance inside its 52 KB; 9.6 KB of 12-gons pushed config-3-sized scenes to two per CU: 208 -> 234 us) - a
// narrow-phase lane reads another obstacle than its neighbour, and from global memory a ring costs it two dependent L2 round trips
// (count, then vertices) per round.  Measured on config-3 sizes, half of the columns rings (same box): rectangle-only scene on its
// shaped instance 138.7 us; the run-time-shape POLY instance with no polygon at all 162.5; 4-vertex rings that ARE their rectangles
// 177.6 (185.9 with counts and rings in global memory).
constexpr int kPolyLdsMax = 4 * 1024;
__host__ __device__ inline int poly_lds_verts(int n_obs, int poly_stride) { return poly_stride > 0 && n_obs * poly_stride * 16 <= kPolyLdsMax ? n_obs * poly_stride : 0; }

// coef_cols: columns (segments) of the spline's coefficient rows the workgroup keeps in LDS: all nx_max of them (default), or a WINDOW
// of that many segments placed at the ego's position (the kernel's `wcap`): 64 of the 76 bytes a knot costs.  Long reference lines
// (200+ knots) then still fit the three- / four-per-CU layouts; a point whose segment lies outside the window reads global memory.
__host__ __device__ inline Layout make_layout(int nx_max, int n_obs, int rows, int hp, int nd, int nv, int nt, int kItemCap, int nwaves, int poly_stride = 0, bool slim = false,
                                              int coef_cols = -1)
{
    // slim (the four-per-CU instance, no polygon columns): the same tables in 40 KB - no inner radii, fp16 fan bounds, 16-bit
    // hit codes, the row boxes inside the power sums' / hit lists' bytes (they are read for the last time before the first hit is written)
    Layout L;
    int o = 0;
    L.dim = o;      o = align16(o + (slim ? 24 : 32) * n_obs);
    L.pose = o;     o = align16(o + 32 * kItemCap);  // poses of the group test's survivors (x, y, cos, sin), in list order
    L.frames = o;   o = align16(o + 32 * nwaves * hp);   // [wavefront][point]: the profile the wavefront is working on
    L.dmax = o;     o = align16(o + (slim ? 2 : 4) * nt * hp);   // [slice][point] float (slim: half), rounded up: max |d| over the lateral samples
    L.ddmax = o;    o = align16(o + (slim ? 2 : 4) * nt * hp);   // max |d(i + 1) - d(i)|
    L.wfat = o;     o = align16(o + 4 * nwaves * (rows > 0 ? rows : 1));  // [wavefront][row] float, rounded up
    L.grp = o;      o =align16(o + 32 * (rows > 0 ? rows : 1));       // per checked pose row: circle enclosing all lon profiles' points
    L.iqueue = o;   o = align16(o + 2 * kItemCap);                           // (row, obstacle) items that pass the group test
    L.samples = o;  o = align16(o + 8 * (nt + nv + nd));  // t / v / d sample grids (read all over the kernel: keep them out of HBM latency)
    L.lon_sum = o;  o = align16(o + 24 * nt * nv);   // sum_v, sum_as, sum_js
    L.lat_sum = o;  o = align16(o + 24 * nd * nt);   // sum_ad, sum_jd, sum_d
    L.lon_meta = o; o = align16(o + 8 * nt * nv);    // int M, uint flags
    L.qlon = o;     o = align16(o + 16 * nt * nv);   // a3, a4 of every lon profile (a0..a2 are the ego state)
    L.qlat = o;     o = align16(o + 24 * nt * nd);   // a3, a4, a5 of the lat profiles of every slice
    L.box = o;      if (!slim) o = align16(o + 16 * (rows > 0 ? rows : 1));  // per checked pose row: bounding box of the row's reference points (ordered-uint fp32)
    L.coll = o;     o = align16(o + 8 * nt * nv);  // one bit per lateral sample, a 64-bit word per lon profile
    // per-wavefront hit lists; before the walk the same bytes hold the power sums S_k(N) = sum_i (i*tick - c)^k, k = 0..10, per slice
    L.queue = o;    L.pows = o;
    {
        const int q = (slim ? 2 : 4) * 64 * nwaves;
        int pw = align16(88 * nt);
        if (slim) { L.box = o + pw; pw += 16 * (rows > 0 ? rows : 1); }
        o = align16(o + (q > pw ? q : pw));
    }
    L.cnt = o;      o = align16(o + 32);  // list counters (monotone) + scan mask + ticket + two fp32 bounds
    L.nslice = o;   o = align16(o + 4 * nt);  // points per slice, len(np.arange(0, T, tick))
    L.best = o;     o = align16(o + 16 * (slim ? 8 : 16));  // (up to 16 wavefronts; slim: 8)
    L.konst = o;    o = align16(o + 96);  // per-ego constants the collision stages re-read (instead of registers held through the kernel)
    L.nvert = o;    o = align16(o + (poly_stride > 0 ? 4 * n_obs : 0));                              // polygon columns: vertices per obstacle
    L.poly = o;     o = align16(o + 16 * poly_lds_verts(n_obs, poly_stride));                        // ... and the rings, when they fit
    // the spline tables last: theirs is the one size no instance of the kernel knows at compile time, so every other offset folds
    L.knots = o;    o = align16(o + 8 * nx_max);
    L.coef = o;     o = align16(o + 64 * (coef_cols >= 0 && coef_cols < nx_max ? coef_cols : nx_max));
    L.lut = o;      o = align16(o + 2 * (2 * nx_max + 1));  // uint16 segment hint per arclength bucket
    L.total = o;
    return L;
}

// LDS of an epilogue workgroup (kThreads / 128 trajectories): [4][FP_FAST_POINTS] doubles of difference-chain scratch per trajectory,
// {first point off the spline} x 2, the argmin and the "had to wait" flag per trajectory; then, for reference lines of at most
// kEpiSplineNX knots, room for one spline copy per trajectory
constexpr int kEpiPairsC = 512 / (2 * kWave);
constexpr int kEpiLdsBytes = kEpiPairsC * 4 * FP_FAST_POINTS * 8 + kEpiPairsC * 4 * 4 + 16;
constexpr int kEpiSplineNX = 96;

// LDS budget of one workgroup (the CU has 160 KB; beyond ~82 KB only one workgroup fits per CU)
constexpr int kLdsLimit = 150 * 1024;
constexpr int kLdsThird = 52 * 1024;          // (a margin below 160 KB / 3 for the allocation granule)
constexpr int kLdsQuarter = 40 * 1024 - 512;  // (a margin below 160 KB / 4 for the allocation granule)
// Coefficient window (the kernel's wcap): below this many segments too many points would read global memory
constexpr int kWinMin = 32;
// buckets of the FISS+ ranking in the appended search workgroups (a multiple of 64 x their 8 wavefronts)
constexpr int kAppendedSearchNB = 512;

// Checked pose rows and the time points they span; false when the problem does not fit the kernel's index widths.
inline bool fused_shape(const fp_params& p, const fp_batch& b, int* rows_out, int* hp_out)
{
    if (p.nd > kWave || p.nv > 255 || b.n_obs > 4095) return false;
    const int stride = p.check_stride;
    int rows = 0, hp = 0;
    if (b.n_obs > 0) {
        rows = (points_cap(p) + stride - 1) / stride;
        const int rows_tab = (b.T_obs + stride - 1) / stride;
        if (rows_tab < rows) rows = rows_tab;
        hp = rows * stride + 1;
        if (hp > points_cap(p)) hp = points_cap(p);
        if (rows > 4095 || (long)rows * b.n_obs > 65535) return false;
    }
    *rows_out = rows;
    *hp_out = hp;
    return true;
}

// The largest "lattice_group" a problem gets: nt, capped at 256 / nv; 0 when the problem does not fit the fused kernel or the layout
// of a 1024-thread workgroup does not fit the LDS budget.  Above 1 the launch takes a grouped instance (plan_lattice, step 2).  The
// cap g * nv <= 256 was the 8-bit profile index of a kernel organisation that is gone (several slices per barrier interval); it is
// kept because it still decides which launches get the 1024-thread instances - tests/test_gpu_edges.py pins nv = 128 (two: grouped)
// against nv = 129 (one: plain) - and a refactor does not move that line.
inline int group_fit(const fp_params& p, const fp_batch& b)
{
    int rows = 0, hp = 0;
    if (!fused_shape(p, b, &rows, &hp)) return 0;
    if (make_layout(b.NX, b.n_obs, rows, hp, p.nd, p.nv, p.nt, item_cap(4), FP_GROUP_THREADS / kWave, b.obs_nvert ? b.poly_stride : 0).total > kLdsLimit) return 0;
    const int by_index = 256 / p.nv;  // (lattice sizes are at least 1: the ABI refuses anything else)
    return p.nt < by_index ? p.nt : by_index;
}

// The instances of lattice_fused_kernel - family (grouped: 1024 threads; poly: POLY; search: FISS; window: WIN) x workgroups per CU x compile-time
// shape (BASELINE.json's two; else run-time sizes).  frenet_lattice_fused.hip instantiates exactly these; a plan names one by index.
enum LatticeFamily { kPlain, kGrouped, kPoly, kPolyGrouped, kSearch, kWindow, kPolyWindow };
enum LatticeShape { kShapeRuntime, kShape997, kShape555 };
struct LatticeShapeDims { int nd, nv, nt, stride, n_obs, rows; };
constexpr LatticeShapeDims kLatticeShapes[3] = {{0, 0, 0, 0, 0, 0}, {9, 9, 7, 2, 50, 25}, {5, 5, 5, 2, 10, 50}};
struct LatticeKey { LatticeFamily family; int per_cu; LatticeShape shape; };
constexpr LatticeKey kLatticeInstances[] = {
    {kPlain, 2, kShapeRuntime}, {kPlain, 2, kShape997}, {kPlain, 2, kShape555}, {kPlain, 3, kShapeRuntime}, {kPlain, 3, kShape997}, {kPlain, 3, kShape555},
    {kPlain, 4, kShapeRuntime}, {kPlain, 4, kShape997}, {kGrouped, 2, kShapeRuntime}, {kGrouped, 2, kShape997}, {kGrouped, 2, kShape555},
    {kPoly, 2, kShapeRuntime}, {kPoly, 3, kShapeRuntime}, {kPoly, 3, kShape997}, {kPolyGrouped, 2, kShapeRuntime},
    {kSearch, 3, kShapeRuntime}, {kSearch, 3, kShape997}, {kSearch, 4, kShapeRuntime}, {kSearch, 4, kShape997},
    {kWindow, 3, kShapeRuntime}, {kWindow, 3, kShape997}, {kWindow, 4, kShapeRuntime}, {kWindow, 4, kShape997},
    {kPolyWindow, 3, kShapeRuntime}, {kPolyWindow, 3, kShape997},
};
constexpr int kLatticeInstanceCount = sizeof(kLatticeInstances) / sizeof(kLatticeInstances[0]);

// The index of the instance (family, per_cu, shape), or of its run-time-shape sibling when that shape has no instance of its own.
inline int lattice_instance(LatticeFamily family, int per_cu, LatticeShape shape)
{
    for (int i = 0; i < kLatticeInstanceCount; ++i)
        if (kLatticeInstances[i].family == family && kLatticeInstances[i].per_cu == per_cu && kLatticeInstances[i].shape == shape) return i;
    return shape == kShapeRuntime ? -1 : lattice_instance(family, per_cu, kShapeRuntime);
}

struct LatticePlan {
    bool fits = false;       // false: the problem does not fit the fused kernel (index widths, LDS budget) - nothing below is set
    int rows = 0, hp = 0;    // checked pose rows, the time points they span
    int gs = 1;              // "lattice_group" as granted (group_fit); > 1: a grouped instance - 1024-thread workgroups, two per CU, no window, no tail
    int nsplit = 1;          // workgroups per ego (latency mode)
    int per_cu = 2;          // lattice workgroups per CU the instance is built for (2 / 3 / 4)
    int wcap = 0;            // spline coefficient columns in LDS: NX (the whole table) unless the instance keeps a window
    bool epilogue = false;   // winner-series epilogue workgroups appended to the grid
    bool search = false;     // FISS+ search workgroups appended to the grid
    bool series = false;     // the launch writes the winner's series (inside its lattice workgroups or by the epilogue)
    int tail_from = -1;      // first dispatch slot of the tail split (-1: none)
    int epi_from = -1;       // first appended workgroup (-1: none)
    unsigned grid = 0;
    int lds = 0;             // dynamic LDS bytes of every workgroup of the launch
    int threads = 0;
    int instance = -1;       // index into kLatticeInstances
};

// The launch plan.  Decided in dependency order - shape, grouped or not, the window of each occupancy, occupancy and offers, LDS,
// tail, grid - and nothing is undone later: a launch whose plan comes out windowed is planned as if no search had been offered (no
// instance has both; the search then follows in its own launch, and neither the occupancy nor the LDS is gated on it).
inline LatticePlan plan_lattice(const KernelArgs& ka, const LatticeRequest& rq)
{
    // Diagnostic builds, all in one place: FP_PHASE_STAMPS / FP_COUNTERS leave their stamps in the series block (no epilogue workgroups,
    // series asked of the kernel do not pin it to two per CU, no tail); FP_NO_OCC6 / FP_NO_OCC8: at most two / three per CU;
    // FP_NO_SHAPES: the run-time-shape polygon instances for every shape, two per CU.
    enum : unsigned { kStamps = 1, kNoOcc6 = 2, kNoOcc8 = 4, kNoShapes = 8 };
    constexpr unsigned diag = 0
#if defined(FP_PHASE_STAMPS) || defined(FP_COUNTERS)
        | kStamps
#endif
#if defined(FP_NO_OCC6)
        | kNoOcc6
#endif
#if defined(FP_NO_OCC8)
        | kNoOcc8
#endif
#if defined(FP_NO_SHAPES)
        | kNoShapes | kNoOcc6
#endif
        ;
    constexpr bool stamps = diag & kStamps, no_occ6 = diag & kNoOcc6, no_occ8 = diag & kNoOcc8, no_shapes = diag & kNoShapes;
    const fp_params& p = ka.p;
    const fp_batch& b = ka.b;
    if (rq.provisional && (ka.r.best_traj || ka.epi_flag || ka.has_loop)) {  // the winner is decided behind this launch: plan it without the offers
        KernelArgs plain = ka;
        plain.r.best_traj = nullptr; plain.epi_flag = nullptr; plain.has_loop = 0;
        return plan_lattice(plain, rq);
    }
    LatticePlan pl;
    // 1. shape
    if (!fused_shape(p, b, &pl.rows, &pl.hp)) return pl;
    const int rows = pl.rows, hp = pl.hp;
    const bool poly = b.obs_nvert && b.n_obs > 0;
    const int pstride = poly ? b.poly_stride : 0;  // (polygon columns: their counts - and rings, when they fit - live in LDS)
    const bool inl = rq.inl && rq.inl->on;
    pl.nsplit = !rq.part_scratch || rq.nsplit < 1 ? 1 : rq.nsplit > p.nt ? p.nt : rq.nsplit;
    // 2. grouped or not: "lattice_group" as asked for, clamped to [1, group_fit].  Its value only matters as 1 / more than 1: above 1 the
    // launch takes a grouped instance - workgroups of 1024 threads (twice the wavefronts walking an ego's lon profiles: the latency
    // instances, for batches that leave every ego a CU to itself) - never three or four per CU, never a coefficient window, never a
    // tail split (all gated on gs == 1 below).  The host's automatic choice asks for it together with one workgroup per ego (no split).
    int gs = rq.group < 1 ? 1 : (rq.group > p.nt ? p.nt : rq.group);
    if (gs > 1) {
        const int fit = group_fit(p, b);
        gs = fit < 1 ? 1 : (gs > fit ? fit : gs);
    }
    pl.gs = gs;
    pl.threads = gs > 1 ? FP_GROUP_THREADS : kThreads;
    // 3. the coefficient window of each occupancy: when the whole spline does not fit a residency's LDS share, the largest window that
    // does - if it is at least kWinMin segments (0: not even a useful window fits); no grouped instance has a window
    auto window_for = [&](int cap_bytes, int occ, int ps, bool slim) {
        const int base = make_layout(b.NX, b.n_obs, rows, hp, p.nd, p.nv, p.nt, item_cap(occ), kThreads / kWave, ps, slim, 0).total;
        const int w = (cap_bytes - base - 16) / 64;
        if (w >= b.NX) return b.NX;
        return gs == 1 && w >= kWinMin ? w : b.NX;
    };
    const int w6 = window_for(kLdsThird, 6, pstride, false), w8 = window_for(kLdsQuarter, 8, 0, true);
    const Layout L6 = make_layout(b.NX, b.n_obs, rows, hp, p.nd, p.nv, p.nt, item_cap(6), kThreads / kWave, pstride, false, w6);
    const Layout L8 = make_layout(b.NX, b.n_obs, rows, hp, p.nd, p.nv, p.nt, item_cap(8), kThreads / kWave, 0, true, w8);
    // 4. occupancy and the offers.  Three workgroups per CU (OCC = 6) when the launch has more egos than two per CU hold at once,
    // nobody needs the series from this kernel (series asked of it pin it to two per CU; series offered to the epilogue workgroups do
    // not) and a workgroup's LDS fits a third of the CU; never for inline inputs (read by the two-per-CU instances only) or a CU with
    // less than gfx950's 160 KB of LDS; "lattice_occupancy" 2 keeps two.
    const bool three = gs == 1 && pl.nsplit == 1 && (stamps || !ka.r.best_traj || ka.epi_flag) && b.B > ka.resident2 && L6.total <= kLdsThird &&
                       ka.lds_cu_kb >= 160 && !inl && !no_occ6 && ka.occ_cap != 2;
    // the series of a three-per-CU launch: by epilogue workgroups appended to the grid (ka.epi_flag + ka.idx_shadow from the caller);
    // else the caller launches winner_traj_kernel behind this launch
    pl.epilogue = three && !stamps && ka.r.best_traj && ka.epi_flag && ka.idx_shadow && !ka.has_loop;
    const int epi_lds = kEpiLdsBytes + (b.NX <= kEpiSplineNX ? kEpiPairsC * 9 * b.NX * 8 : 0);
    // the FISS+ search in appended workgroups: three-per-CU launches that write their tables, lattices the 1024-sample search instance holds
    const int C_all = p.nd * p.nv * p.nt;
    pl.search = three && rq.ft && rq.ft->flag && ka.r.cost_tbl && ka.r.flag_tbl && !ka.r.best_traj && !ka.has_loop &&
                C_all > 4 * kWave && C_all <= 1024 && rq.ft->opts.kind == FP_FISS_PLUS && !poly;
    const int search_lds = pl.search ? fsp::fissplus_lds_bytes(C_all, kAppendedSearchNB) : 0;
    // FOUR workgroups per CU when the slim layout and the appended workgroups' LDS fit a quarter of the CU (BASELINE.json's dense shape:
    // reference lines of up to ~80 knots) and the launch has more egos than three per CU hold.  Not for a closed-loop batch (its
    // finished egos leave at once, what runs rarely fills three per CU - measured 68 -> 71-75 us per cycle with four) unless
    // "lattice_occupancy" 4 asks for it; "lattice_occupancy" 2 / 3 keep fewer.
    const bool four = three && !poly && L8.total <= kLdsQuarter && (!pl.epilogue || epi_lds <= kLdsQuarter) && (!pl.search || search_lds <= kLdsQuarter) &&
                      (long)b.B * 2 > (long)ka.resident2 * 3 && (!b.skip || ka.occ_cap == 4) && !no_occ8 && ka.occ_cap != 2 && ka.occ_cap != 3;
    pl.per_cu = four ? 4 : three ? 3 : 2;
    pl.wcap = four ? w8 : three ? w6 : b.NX;  // (two per CU: the whole table)
    pl.series = ka.r.best_traj && (pl.epilogue || (!three && !ka.epi_flag));
    // 5. LDS, tail, grid
    const Layout L = four ? L8 : three ? L6 : make_layout(b.NX, b.n_obs, rows, hp, p.nd, p.nv, p.nt, item_cap(4), pl.threads / kWave, pstride);
    if (L.total > kLdsLimit) return LatticePlan{};
    pl.lds = L.total;
    if (pl.epilogue && pl.lds < epi_lds) pl.lds = epi_lds;  // (every workgroup of a launch gets the same dynamic LDS)
    if (pl.search && pl.lds < search_lds) pl.lds = search_lds;
    // Tail split: a launch of several rounds of workgroups (one per ego) ends on the egos that happened to start last - with ~50 us
    // per ego and the last workgroup starting ~40 us before the end, a fifth of the launch runs on a draining chip.  The last `tail`
    // dispatch slots are cut in two (time-horizon slices it_lo .. it_hi per part, ticket + merge like the latency mode): each half
    // repeats the ego's prologue, so only a quarter of a round's worth of slots is cut (tail < 0: auto).  Results do not depend on it.
    if (!stamps && rq.tail != 0 && pl.nsplit == 1 && gs == 1 && rq.part_scratch && p.nt >= 2 && b.S > 0 && b.n_obs > 0 && (size_t)b.B * 4 <= kTicketBytes) {
        const int resident = pl.per_cu * (rq.tail < 0 ? -rq.tail : 0);  // workgroups the device holds at once (auto: tail = -compute units)
        // (three per CU: 128 ... 384 of 768 slots measured within 1 %; 576: no gain; 768: slower.  Four per CU, launch order = the batch's own
        // history, round 6: 96-192 of 1024 within 1 % of each other and of no cut at all, 512: 4 % slower - an eighth of a round, which also
        // halves the inputs staged twice)
        int n_tail = rq.tail > 0 ? rq.tail : (b.B > resident ? resident / (four ? 8 : 4) : 0);
        if (n_tail > b.B - resident && rq.tail < 0) n_tail = b.B - resident;
        if (n_tail > b.B) n_tail = b.B;
        if (n_tail > 0) pl.tail_from = b.B - n_tail;
    }
    const unsigned lattice_grid = pl.tail_from >= 0 ? (unsigned)(2 * b.B - pl.tail_from) : (unsigned)(b.B * pl.nsplit);
    pl.epi_from = pl.epilogue || pl.search ? (int)lattice_grid : -1;
    pl.grid = lattice_grid + (pl.epilogue ? (unsigned)((b.B + kEpiPairsC - 1) / kEpiPairsC) : 0u) + (pl.search ? (unsigned)b.B : 0u);
    // the instance: windowed exactly when wcap < NX; the compile-time shape when this problem has it
    const bool windowed = pl.wcap < b.NX;
    if (windowed && pl.search) {
        LatticeRequest no_search = rq;
        no_search.ft = nullptr;
        return plan_lattice(ka, no_search);
    }
    const LatticeFamily family = poly ? (gs > 1 ? kPolyGrouped : windowed ? kPolyWindow : kPoly)
                                      : gs > 1 ? kGrouped : pl.search ? kSearch : windowed ? kWindow : kPlain;
    LatticeShape shape = kShapeRuntime;
    for (int s = 1; s < 3 && !no_shapes; ++s) {
        const LatticeShapeDims& d = kLatticeShapes[s];
        if (p.nd == d.nd && p.nv == d.nv && p.nt == d.nt && p.check_stride == d.stride && b.n_obs == d.n_obs && rows == d.rows) shape = (LatticeShape)s;
    }
    pl.instance = lattice_instance(family, pl.per_cu, shape);
    pl.fits = pl.instance >= 0;
    return pl;
}

}  // namespace fp
