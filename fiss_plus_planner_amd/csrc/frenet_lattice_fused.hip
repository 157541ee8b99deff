// frenet_lattice_fused.hip - the production dense-lattice kernel (gfx950).
//
// One workgroup per ego problem.  The lattice is separable, and the kernel is built around that:
//
//   * the longitudinal polynomial s(t) depends on (T, v) only  -> nt*nv "lon profiles"
//   * the lateral polynomial d(t) depends on (d_end, T) only    -> nd*nt "lat profiles"
//   * the reference-line frame (position + unit tangent at s(t)) belongs to the lon profile, so the
//     spline is evaluated nt*nv*N times per ego, not nd*nv*nt*N times (9x fewer at 9x9x7)
//   * cost_final = (time + lon sums + lat sums) / N recombines per candidate with the reference's grouping
//
// Once per ego (phase A0): one lane per lon profile solves the boundary-value problem and tries to PROVE the profile clean from
// the extrema of its polynomials (speed / acceleration limits, inside the spline's range); only slices with an unproven profile
// run the reference's point-by-point scan (lane per (profile, point), LDS atomics).  The cost sums of every profile follow in
// closed form from the per-slice power sums (centred, power_sums_closed) - no per-point work.
// Once per ego, collision stage G: for every checked pose row the arclength range of the reference points of ALL lon profiles of
// ALL slices (a polynomial evaluation each) becomes a circle - centre on the line at the middle of the range, radius = half the
// range x an upper bound of the spline's parametric speed + ego reach + a closed-form bound of the lateral offsets - and one lane
// per (row, obstacle) item tests the obstacle against it: ~7 % survive, and only their orientations are turned into (cos, sin).
// Per lon profile (T, v) - the WALK: one wavefront does everything for the profile by itself, with no workgroup barrier:
//   frames   one lane per time point the collision horizon can touch: spline frame -> the wavefront's LDS table
//   prep     one lane per pose row: the half-width of the fan of lateral samples along the reference normal
//   B        one lane per surviving item: circle fattened by the largest lateral offset of the slice, separating axes along the
//            reference normal and tangent
//   N        one lane per (hit, lateral sample): exact ego centre + heading, exact circle test, 4-axis separating-axis test
//            (closed: touching collides).  Survivors of G are appended to a block-wide LDS list with ballot / popcount + one atomic
//            per wavefront; those of B are compacted into the wavefront's own hit list.
// Finally one lane per candidate assembles cost + flag word, a wave/LDS argmin with FOP's "last minimum wins" rule picks the
// winner, and - when the caller asked for it - one wavefront of the same workgroup writes the winner's series (frenet_winner.h).
//
// Semantics restated from the reference (paths relative to its checkout):
//   lattice + cost      planners/frenet_optimal_planner.py:69-104, planners/common/cost/cost_function.py:41-50
//   Frenet->Cartesian   planners/frenet_optimal_planner.py:106-138 (truncation at the spline end :112-113)
//   constraints         planners/frenet_optimal_planner.py:140-160
//   collision           planners/frenet_optimal_planner.py:168-208 (stride 2, horizon from obstacles[0], M==1 -> collision)
//   argmin              planners/frenet_optimal_planner.py:263-268
#include <atomic>
#include <type_traits>
#include <utility>

#include "frenet_device.h"
#include "frenet_kernels.h"
#include "frenet_winner.h"
#include "frenet_advance.h"
#include "frenet_fissplus.h"
#include "frenet_lattice_plan.h"

namespace fp {

namespace {

// fp64 -> fp32 that never rounds below the argument (x >= 0): to nearest, then one part in 2^22 up.  Replaces the software
// emulation of the directed-rounding conversion (~15 instructions) where only a conservative bound is needed.
__device__ __forceinline__ float float_above(double x) { return (float)x * 1.00000024f; }

// the counterpart of frenet_device.h's vmin_f64: v_max_f64 without the canonicalising instruction in front of each fmax operand
__device__ __forceinline__ double vmax_f64(double a, double b) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

// monotone map fp32 -> uint32 (and back), so that LDS integer atomic min / max order floats of either sign
__device__ __forceinline__ uint32_t f32_ordered(float f)
{
    const uint32_t u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float f32_from_ordered(uint32_t u) { return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }
constexpr uint32_t kOrdPosInf = 0xFF800000u, kOrdNegInf = 0x007FFFFFu;  // f32_ordered(+inf), f32_ordered(-inf)

// e / d for 0 <= e, e + d < 2^22 with inv_d = 1.0f / d: (e + 0.5) / d lies at least 0.5 / d away from an integer and the two fp32
// roundings move it by less than (e / d + 1) 2^-23, so the truncation is exact.  Four full-rate instructions instead of the
// ~20 of an integer division; the remainder uses the 24-bit multiplier (full rate; v_mul_lo_u32 is quarter rate).
__device__ __forceinline__ int div_small(int e, float inv_d) { return (int)(((float)e + 0.5f) * inv_d); }
__device__ __forceinline__ int mul24(int a, int b) { return __mul24(a, b); }
// e / D for a divisor known at compile time (the specialised instances of the kernel): one 24-bit multiply and a shift.
// Exact for 0 <= e <= MAXE: with M = ceil(2^20 / D) the error term e (M D - 2^20) / (D 2^20) stays below 1 / D, and e M < 2^32.
// D = 0: the divisor is a run-time value, div_small with its reciprocal.
template <int D, int MAXE>
__device__ __forceinline__ int div_by(int e, float inv_d)
{
    if constexpr (D > 0) {
        constexpr unsigned long long M = ((1ull << 20) + D - 1) / D;
        static_assert(M < (1ull << 24) && (unsigned long long)MAXE < (1ull << 24), "24-bit multiplier");
        static_assert((unsigned long long)MAXE * M < (1ull << 32), "product overflows");
        static_assert((unsigned long long)MAXE * (M * D - (1ull << 20)) < (1ull << 20), "not exact over the whole range");
        return (int)(__umul24((unsigned int)e, (unsigned int)M) >> 20);
    } else {
        return div_small(e, inv_d);
    }
}

// bits of a ballot below the calling lane: __popcll(m & ((1ull << lane) - 1)) as the hardware counts it (v_mbcnt_lo / v_mbcnt_hi)
__device__ __forceinline__ int lanes_below(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Hand-over wait of the workgroups appended to a launch (winner-series epilogue, FISS+ search): spin on the ego's flag - set by the
// lattice workgroup that published the ego's results - for at most kHandoverTimeout ticks of the 100 MHz wall clock.  A wait that
// runs out (only possible if the workgroup distributors did NOT start this XCD's lattice workgroups before this one, see the kernel)
// does not trap - a trap aborts the queue and with it the ctx: it leaves `code` in the ctx's error word (device-mapped host memory,
// system scope: the host sees it without a synchronisation) and the workgroup returns without output; the slot falls free, the
// launch completes, and the next call on the ctx reports the failure, resets the flags and stops using appended workgroups.
constexpr long long kHandoverTimeout = 200000000ll;  // 2 s
__device__ __forceinline__ bool handover_wait(const int32_t* flag, int32_t* err_word, int code, int timeout_us = 0)
{
    const long long t0 = wall_clock64();
    const long long limit = timeout_us > 0 ? (long long)timeout_us * 100ll : kHandoverTimeout;  // (100 MHz wall clock; timeout_us: KernelArgs::handover_timeout_us, tests only)
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
        __builtin_amdgcn_s_sleep(2);
        if (wall_clock64() - t0 > limit) {
            if (err_word) __hip_atomic_store(err_word, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return false;
        }
    }
    return true;
}

struct __attribute__((aligned(16))) Frame {  // reference-line frame of one lon-profile point
    double px, py, tx, ty;
};
struct __attribute__((aligned(16))) ObsPose {
    double x, y, c, s;
};
struct __attribute__((aligned(16))) ObsDim {
    double hl, hw, r, pad;
};
// A table of 32-byte records {a, b, c, d} kept as two arrays of 16-byte halves.  Consecutive lanes reading consecutive records as two
// ds_read_b128 at a 32-byte stride touch only half of the LDS banks per instruction (every fourth lane lands on the same banks: a 2-way
// conflict on every read of a frame or a survivor's pose); at a 16-byte stride the same reads are conflict free.  Same bytes in total.
template <typename T>
struct SplitTab {
    double2* lo;
    double2* hi;
    __device__ __forceinline__ T get(int i) const { const double2 a = lo[i], b = hi[i]; return T{a.x, a.y, b.x, b.y}; }
    __device__ __forceinline__ void set(int i, double a, double b, double c, double d) const { lo[i] = make_double2(a, b); hi[i] = make_double2(c, d); }
    __device__ __forceinline__ SplitTab at(int off) const { return SplitTab{lo + off, hi + off}; }
};



// the walk's fan bounds in LDS: fp32, or (slim layout) fp16 that is never below the fp32 value: x (1 + 2^-10) survives the rounding to
// 11 bits (relative error <= 2^-11), the offset keeps the result a normal half (no dependence on the denormal mode), NaN stays NaN
template <bool SLIM> struct FanType { using type = float; static __device__ __forceinline__ float above(float x) { return x; } };
template <> struct FanType<true> { using type = _Float16; static __device__ __forceinline__ _Float16 above(float x) { return (_Float16)(x * 1.001f + 6.2e-5f); } };


}  // namespace

__device__ __forceinline__ double gk_first(const fp_batch& bt, int f) { return bt.knots[(size_t)f * bt.NX]; }
__device__ __forceinline__ double gk_last(const fp_batch& bt, int f, int nx) { return bt.knots[(size_t)f * bt.NX + nx - 1]; }

// segment of s (known to be inside [knot0, knot_last)) from the bucket table + walk
__device__ __forceinline__ int lut_segment(const double* knots, const unsigned short* lut, int nx, double s, double knot0,
                                           double inv_bucket_w, int n_buckets)
{
    int bkt = (int)((s - knot0) * inv_bucket_w);
    bkt = bkt < 0 ? 0 : (bkt > n_buckets ? n_buckets : bkt);
    int seg = lut[bkt];
    while (seg > 0 && s < knots[seg]) --seg;            // rounding at a bucket edge
    while (seg < nx - 2 && s >= knots[seg + 1]) ++seg;  // knots inside the bucket
    return seg;
}

// The same segment in ONE step, for lines whose knots are all further apart than a bucket is wide (the walk's `lut_crowded` == 0): the bucket
// index is off by rounding at most at a bucket edge, so s lies within a hair of [sb, sb + width], sb the bucket's start, and that stretch
// holds at most one knot.  lut[bkt] is the last knot at or below sb: the segment of s is that one, or the one before it (the knot sits
// at sb and s a hair below it), or the one after it (the knot lies between sb and s) - one compare each, against knots the hint names.
__device__ __forceinline__ int lut_segment_step(const double* knots, const unsigned short* lut, int nx, double s, double knot0,
                                                double inv_bucket_w, int n_buckets)
{
    int bkt = (int)((s - knot0) * inv_bucket_w);
    bkt = bkt < 0 ? 0 : (bkt > n_buckets ? n_buckets : bkt);
    const int seg = lut[bkt];  // (<= nx - 2: knots[seg + 1] exists)
    const double k_lo = knots[seg], k_hi = knots[seg + 1];
    return seg - (int)(seg > 0 && s < k_lo) + (int)(seg < nx - 2 && s >= k_hi);
}

// nsplit > 1 (latency mode for small batches): the time-horizon slices of one ego are spread over nsplit workgroups, each
// writes its partial argmin to part_best[ego * nsplit + part]; the last one to arrive (ticket counter) merges them.
//
// Template parameters = the problem shape when it is known at compile time (0 = run-time value from the arguments): lattice sizes,
// collision check stride, obstacles per scene, checked pose rows.  BASELINE.json has two shapes (9 x 9 x 7 with 50 obstacles over
// 25 rows, 5 x 5 x 5 with 10 obstacles over 50 rows); in their instances every index decode is a constant multiply-shift, the LDS
// carve-up folds to immediates and the loop bounds are known.  The <0, ...> instance is the same source with everything read from
// the arguments.
//
// NTH: threads per workgroup, 512 or - the grouped instances (kGrouped / kPolyGrouped, "lattice_group") - 1024: twice the wavefronts
// walking the ego's lon profiles, for small batches in which every ego can have a CU to itself.  Small lattices with few obstacles
// are bound by latency, not by arithmetic: with all slices in one such workgroup an ego needs no split over workgroups (no ticket, no
// merge).  Nothing else distinguishes a grouped instance from a plain one.
//
// The kernel's parameters as one struct: where InlineIn::bytes sits in the argument segment.
// `reserved` is a slot nothing reads (it held the slices per barrier interval of an organisation that is gone); the launcher passes 0.
// It stays because the layout of the argument segment is part of the generated code: without it tail_from, epi_from and wcap move by
// 4 bytes, and the register allocator then came out differently in 14 of the 25 instances (SGPR spills of the four-per-CU instances
// 38 -> 41, 26 -> 21, 95 -> 104; instruction counts -0.4 % ... +4 %; one three-per-CU instance gained 36 B of scratch).
struct LatticeKernarg {
    KernelArgs ka; int rows_max_arg, hp_max_arg, nsplit; Best* part_best; int* part_count; const int* perm; int* dur; int reserved, tail_from, epi_from, wcap; FissTail ft; InlineIn inl;
};
constexpr size_t kInlineOffset = offsetof(LatticeKernarg, inl) + offsetof(InlineIn, bytes);

// POLY: the scene may hold convex-polygon obstacle columns (fp_batch.obs_nvert != NULL).  Only the run-time-shape instances exist with
// POLY = true: the polygon branch in the narrow phase costs the rectangle-only instances 26 more spilled SGPRs and 2 % of the headline
// step (same-box A/B), and scenes with polygons are not what the shaped instances were made for.
// FISS: the launch carries one appended workgroup per ego that runs the FISS+ search (frenet_fissplus.h) on the ego's dense tables as
// soon as the ego's lattice workgroup has written them - inside the launch's drain instead of in a launch of its own (a launch that is
// one round of 4-wavefront workgroups as long as its slowest ego, behind a kernel boundary).  The tables travel between workgroups of
// ONE launch, possibly on different XCDs whose L2s are not coherent with each other: they are written with agent-scope stores and read
// with agent-scope loads; the flag follows the stores of ALL threads of the writing workgroup (s_waitcnt + barrier).
// WIN: the instance can keep a WINDOW of the spline's coefficient columns in LDS (wcap < NX, see make_layout) - reference lines too long
// for a residency's LDS share.  Its own instances: the window's bookkeeping costs the others 10-35 spilled SGPRs each (v_writelane /
// v_readlane pairs in a kernel that is VALU-issue bound), so the instances without it are exactly what they were.
template <int ND, int NV, int NT, int STRIDE, int NOBS, int ROWS, int OCC, int NTH, bool POLY = false, bool FISS = false, bool WIN = false>
__global__ __launch_bounds__(NTH, OCC) void lattice_fused_kernel(KernelArgs ka, int rows_max_arg, int hp_max_arg, int nsplit_arg, Best* part_best, int* part_count, const int* perm,
                                                                   int* dur, int reserved, int tail_from, int epi_from, int wcap, FissTail ft, InlineIn inl)
{
    // [section APPSEARCH]
    if constexpr (FISS) {
        if (epi_from >= 0 && (int)blockIdx.x >= epi_from) {  // ---- appended search workgroup: one ego, in launch order
            extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
            const int eslot = (int)blockIdx.x - epi_from;
            const int eb = perm ? perm[eslot] : eslot;
#if defined(FP_TL)  // timeline diagnostic (tools/fused_timeline.py, -DFP_TL): the FISS+ outputs carry clock ticks instead of results
            const long long tl0 = wall_clock64();
            long long tl1 = 0;
#endif
            int timed_out = 0;
            if (threadIdx.x == 0) {
                timed_out = !handover_wait(&ft.flag[eb], ka.err_word, 2, ka.handover_timeout_us);
                if (!timed_out) __hip_atomic_store(&ft.flag[eb], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
#if defined(FP_TL)
                tl1 = wall_clock64();
#endif
            }
            if (__syncthreads_or(timed_out)) return;  // (timed out: reported through the ctx's error word, see handover_wait)
            __atomic_signal_fence(__ATOMIC_SEQ_CST);  // the tables are read after the flag
            FissArgs fa;
            fa.ka = ka;
            fa.opts = ft.opts;
            fa.io = ft.io;
            fa.cost_tbl = ka.r.cost_tbl;
            fa.flag_tbl = ka.r.flag_tbl;
            fa.walk_jump = ft.walk_jump;
            fsp::fissplus_search_ego<NTH / kWave, 1, 1024, true>(fa, ft.NB, eb, fsm);
#if defined(FP_TL)
            if (threadIdx.x == 0) {  // (the lattice workgroup left its start / end in the dense call's best_idx / best_cost)
                const long long tl2 = wall_clock64();
                const double lat_end = __longlong_as_double((long long)__hip_atomic_load((const unsigned long long*)&ka.r.best_cost[eb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                const int lat_start = __hip_atomic_load(&ka.r.best_idx[eb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __builtin_amdgcn_s_waitcnt(0);
                double* es = ft.io.end_state + (size_t)eb * 3;
                es[0] = (double)(tl0 & 0xFFFFFFFFFFll); es[1] = (double)(tl1 & 0xFFFFFFFFFFll); es[2] = (double)(tl2 & 0xFFFFFFFFFFll);
                ft.io.best_cost[eb] = lat_end;
                ft.io.refined[eb] = lat_start;
            }
#endif
            return;
        }
    }
    // [/section APPSEARCH]
    // ---------------------------------------------------------------- appended epilogue workgroups (blockIdx >= epi_from)
    // The three-workgroups-per-CU instances cannot write the winner's series themselves (the slot time of a one-wavefront dependent
    // chain, and 125 registers), and a winner_traj_kernel behind the launch costs ~9.5 us of a ~155 us step in which the last ~25 us
    // run on a draining chip.  So the series are written INSIDE the drain: the grid carries B / 4 more workgroups at its end - the
    // hardware dispatches workgroups in index order, so they become resident when every lattice workgroup has been dispatched and
    // slots fall free - each of which takes four dispatch slots (in launch order: the egos that started first), waits for their argmins
    // (flag per ego, set by the workgroup that published it; relaxed agent-scope atomics, see the ticket's ordering argument below)
    // and writes the four series, two wavefronts per trajectory (winner_series_pair: one point per lane, 80 registers).
    // No deadlock: an epilogue workgroup only ever waits for lattice workgroups, and a workgroup distributor (one per XCD, each
    // taking every eighth workgroup) starts its workgroups in index order: when an epilogue workgroup holds a slot, every lattice
    // workgroup of the same XCD has been started, and those of the other XCDs do not depend on this XCD's slots.  That order is
    // observed, not documented: the host offers appended workgroups only on the architectures it was verified on (gfx942 / gfx950,
    // fp_ctx_create), and should it ever not hold the wait gives up after 2 s WITHOUT a trap (handover_wait): the slot falls free,
    // the launch completes, and the next call on the ctx reports the failed hand-over and falls back to winner_traj_kernel.
    // [section APPSERIES]
    if constexpr (OCC > 4) {
        if (epi_from >= 0 && (int)blockIdx.x >= epi_from) {
            extern __shared__ __attribute__((aligned(16))) unsigned char esm[];
            constexpr int kPairs = NTH / (2 * kWave);  // trajectories per workgroup
            double* scratch = (double*)esm;                         // [kPairs][4][FP_FAST_POINTS]
            int* s_m = (int*)(esm + kPairs * 4 * FP_FAST_POINTS * 8);  // [kPairs][2] first point off the spline per wavefront
            int* s_idx = s_m + 2 * kPairs;                           // [kPairs] the egos' argmins
            const int pair = (int)threadIdx.x / (2 * kWave), i = (int)threadIdx.x - pair * 2 * kWave;
            const int eslot = ((int)blockIdx.x - epi_from) * kPairs + pair;
            const bool have = eslot < ka.b.B;
            const int eb = have ? (perm ? perm[eslot] : eslot) : 0;
            const fp_params& pp = ka.p;
            const fp_batch& bb = ka.b;
            const int ef = bb.frame_of[eb];
            const double* gk = bb.knots + (size_t)ef * bb.NX;
            const double* gc = bb.coef + (size_t)ef * 8 * bb.NX;
            // A pair that finds its ego's argmin not published yet is one of the launch's last: the launch ends when IT is done.  It spends
            // the wait copying the ego's spline to LDS (9 NX doubles, when four copies fit), so that the segment searches and coefficient
            // reads of the series - three to four dependent L2 round trips after the flag - become LDS reads.  Pairs whose argmin is
            // already there (the many that run inside the drain) read the few segments they touch from global memory as before.
            int* s_wait = s_idx + kPairs;
            double* s_spl = (double*)(esm + kEpiLdsBytes) + (size_t)pair * 9 * bb.NX;
            const bool can_copy = bb.NX <= kEpiSplineNX;
            if (have && i == 0) s_wait[pair] = can_copy && __hip_atomic_load(&ka.epi_flag[eb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
            __syncthreads();
            const bool in_lds = have && s_wait[pair] != 0;
            if (in_lds)
                for (int k = i; k < 9 * bb.NX; k += 2 * kWave) s_spl[k] = k < bb.NX ? gk[k] : gc[k - bb.NX];
            if (have && i == 0) {
                if (handover_wait(&ka.epi_flag[eb], ka.err_word, 1, ka.handover_timeout_us)) {
                    __atomic_signal_fence(__ATOMIC_SEQ_CST);  // the index is read after the flag
                    s_idx[pair] = __hip_atomic_load(&ka.idx_shadow[eb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&ka.epi_flag[eb], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
                } else {
                    s_idx[pair] = -2;  // timed out: nothing is written for this ego (reported through the ctx's error word)
                }
            }
            __syncthreads();
            const int win = have ? s_idx[pair] : -1;
            const bool handed = have && win != -2;
            double d_end = __builtin_nan(""), v_end = d_end, T_end = d_end;
            if (win >= 0) {
                const int iv = win % pp.nv, it = (win / pp.nv) % pp.nt, id = win / (pp.nv * pp.nt);
                d_end = bb.d_samples[id]; v_end = bb.v_samples[(size_t)eb * pp.nv + iv]; T_end = bb.t_samples[it];
            }
            // (a pair beyond the batch still runs the barriers; it writes nothing)
            const SplineLds sp = in_lds ? SplineLds{s_spl, s_spl + bb.NX, bb.nx[ef], bb.NX} : SplineLds{gk, gc, bb.nx[ef], bb.NX};
            winner_series_pair(ka, eb, eb, win >= 0, d_end, v_end, T_end, i, sp, scratch + pair * 4 * FP_FAST_POINTS, s_m + 2 * pair, handed);
            return;
        }
    }
    // [/section APPSERIES]
    // [section ENTRY]
    // Dispatch slot -> (ego, part).  Uniform split (latency mode): slot = blockIdx / nsplit.  Tail split (tail_from >= 0, nsplit_arg
    // == 1): the slots from tail_from on - the workgroups that start when the launch's last round is already draining - are cut in
    // two like a latency-mode ego, so the launch does not end on whole egos that started last (see launch_lattice_fused).
    const bool in_tail = tail_from >= 0 && (int)blockIdx.x >= tail_from;
    // Three and four per CU are only ever launched with ONE workgroup per ego outside the tail (plan_lattice grants them to launches with
    // nsplit == 1 alone; launch_lattice_fused refuses anything else): nsplit is 1 or 2 there, and the three scalar divisions of the
    // uniform split - blockIdx / nsplit here, part nt / nsplit twice below, five vector instructions each on every wavefront for the
    // reciprocal - are a shift by nsplit - 1.  Three instances keep the divisions: the two shaped polygon instances (80 VGPRs, all in
    // use) spill two VGPRs without them, and the plain run-time-shape four-per-CU instance comes out LARGER (4595 -> 4673 vector
    // instructions, 94 -> 111 spilled SGPRs: another register assignment, not less work).
    constexpr bool kOnePart = OCC > 4 && !(ND > 0 && POLY) && !(ND == 0 && OCC > 6 && !POLY && !FISS && !WIN);
    const int nsplit = in_tail ? 2 : (kOnePart ? 1 : nsplit_arg);
    const int slot = in_tail ? tail_from + (((int)blockIdx.x - tail_from) >> 1) : (kOnePart ? (int)blockIdx.x : (int)blockIdx.x / nsplit_arg);
    const int part_of_slot = in_tail ? (((int)blockIdx.x - tail_from) & 1) : (kOnePart ? 0 : (int)blockIdx.x - slot * nsplit_arg);
    constexpr bool kShape = ND > 0;  // (all six are set together)
    // The run-time-shape three-per-CU instances have no register to spare (80 VGPRs, run-time sizes in place of immediates): from the
    // prologue's second barrier on they re-read the ego's start state from LDS (s_k[5..10]) where it is used instead of holding twelve
    // VGPRs through the kernel.  NOT an optimisation: this build of the compiler places VGPR spill stores in the exit block of a
    // divergent loop BEFORE the exec mask is restored (exec = 0: nothing is stored, the reload returns whatever the scratch slot held -
    // zeros in a launch's first round of workgroups, another workgroup's values later), so no instance may spill a VGPR at all
    // (tools/resource_usage.py must show 0 in "VGPRs Spill" for every kernel; tests/test_abi_cpu.py checks it).
    constexpr bool kEgoLds = (ND == 0 && OCC > 4) || OCC > 6;
    constexpr bool kEgoEarly = OCC > 6;  // four per CU (64 VGPRs): from the FIRST barrier on
    constexpr int kThreads = NTH, kWaves = NTH / kWave;  // (shadow the file-scope defaults)
    constexpr int kItemCap = item_cap(OCC);
    constexpr bool kSlim = OCC > 6;  // four workgroups per CU: the 40 KB layout (make_layout)
    static_assert(!kSlim || (!POLY && NTH <= 512 && item_cap(OCC) <= 256), "slim layout: boxes only, 8 wavefronts, 8-bit survivor index");
    const int rows_max = kShape ? ROWS : rows_max_arg;
    const int hp_max = kShape ? (ROWS > 0 ? (ROWS * STRIDE + 1 > FP_MAX_POINTS ? FP_MAX_POINTS : ROWS * STRIDE + 1) : 0) : hp_max_arg;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#if defined(FP_PHASE_STAMPS)
    const long long t_begin = wall_clock64();
#elif defined(FP_TL)
    const long long t_begin = wall_clock64();
#else
    const long long t_begin = dur ? wall_clock64() : 0;
#endif
    // Timing diagnostic (tools/phase_stamps.py, -DFP_PHASE_STAMPS): thread 0 leaves the time since the workgroup started (10 ns
    // ticks) at the phase boundaries in columns 112.. of the last row of its best_traj block (free with traj_stride = 128, sparse, T <= 11 s).
#if defined(FP_PHASE_STAMPS)
#define FP_STAMP(k) do { if (threadIdx.x == 0 && ka.r.best_traj && (perm || blockIdx.x % nsplit == 0)) ka.r.best_traj[((size_t)(perm ? perm[blockIdx.x] : blockIdx.x / nsplit) * FP_ARR_COUNT + 15) * (ka.r.traj_stride > 0 ? ka.r.traj_stride : FP_DEFAULT_STRIDE) + 112 + (k)] = (double)(wall_clock64() - t_begin); } while (0)
// (the one workgroup of an ego that is left after the ticket - whichever part it is - stamps columns 5, 6 and 10)
#define FP_STAMP_LAST(k) do { if (threadIdx.x == 0 && ka.r.best_traj) ka.r.best_traj[((size_t)b * FP_ARR_COUNT + 15) * (ka.r.traj_stride > 0 ? ka.r.traj_stride : FP_DEFAULT_STRIDE) + 112 + (k)] = (double)(wall_clock64() - t_begin); } while (0)
#else
#define FP_STAMP(k) do { } while (0)
#define FP_STAMP_LAST(k) do { } while (0)
#endif
#if defined(FP_PHASE_STAMPS)
    __shared__ unsigned int s_walk_t[2];  // when the first / the last wavefront of the workgroup finished its profiles
#endif
#if defined(FP_COUNTERS)  // work statistics (tools/work_counters.py): LDS counters, left in row 14, columns 112.. of the winner block
    __shared__ int s_dbg[22];  // (16..19: stage V's groups ended, profiles that entered the walk, S rounds no lane's first end passed, the ended groups' bits; 20, 21: stage W - workgroups that took WEXIT, and those of them whose assembly was skipped too)
    if (threadIdx.x < 22) s_dbg[threadIdx.x] = 0;
#define FP_COUNT(k, v) atomicAdd(&s_dbg[k], (int)(v))
#else
#define FP_COUNT(k, v) do { } while (0)
#endif
    const fp_params& p = ka.p;
    const fp_batch& bt = ka.b;
    // launch order: longest egos first when the host has an order for this batch (perm; nsplit == 1 then)
    const int b = perm ? perm[slot] : slot, part = part_of_slot;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid / kWave;
    // The prologue's cuts: phases entered on a scalar test of the wavefront's number, the cost sums dealt by kind, one boundary-value solve
    // per lat profile, the ends of d_samples found once, G with a column per lane - each described where it stands.  In the shaped
    // rectangle instances only: the run-time-shape instances have no scalar register to spare and came out larger with them, and the two
    // shaped polygon instances (80 VGPRs, all in use) spill a VGPR with them; both keep the statements they had.
    // (Also kCut: the appends' lane count by v_mbcnt - lanes_below - and the fold of an N round's hits by halving, both in the walk.)
    // Every statement of the kernel stands in a `// [section NAME]` pair - the bodies, and since the last census also the entry, the glue
    // between sections, the profile loop's own statements and the appended workgroups - so that tools/nonwalk_census.py can weigh all of it.
    constexpr bool kCut = kShape && !POLY;
    // The walk's stage S (a blocked profile ends on one SURE hit, before prep, B and N - see the walk): kCut instances, three and four per CU.  Never a
    // POLY instance: a ring lies inside its box, so a sure hit on the box proves nothing about the ring.
    // -DFP_ABL_NO_SURE compiles the stage out: one source gives both sides of an A/B.
#if defined(FP_ABL_NO_SURE)
    constexpr bool kSure = false;
#else
    // (the four-per-CU instances with the appended search or the coefficient window - 63 of 64 VGPRs before - spill one VGPR with
    // the stage and keep the statements they had; the plain four-per-CU instance, the headline's, holds it in 64)
    // The two-per-CU instances (OCC 4: small batches, latency mode, the grouped 1024-thread launches) do not get it either: their
    // launches leave the device underfilled and last as long as one profile's dependent chain, which S lengthens for every profile
    // it does not end, while the issue slots it saves are not what bounds them - config 2 (5 x 5 x 5, 256 egos) measured 6 % slower
    // with it although S ended three in four of its profiles (EXPERIMENTS.md).  S stands where launches run in rounds: three and four per CU.
    constexpr bool kSure = kCut && OCC > 4 && !(OCC > 6 && (FISS || WIN));
#endif
    // Stage V (whole end-speed GROUPS end on a sure hit before the walk - see VCIRC and VTEST): the instances with stage S.  It needs
    // S's threshold and the speed bound of VBOUND.  -DFP_ABL_NO_GROUP compiles it out.
    // Not the instance with the coefficient window (three per CU; the four-per-CU one has no S): with the stage its FRAMES - the path of
    // a profile V does NOT end - came out ten vector instructions larger (75 > 85) and it spilled 16 SGPRs where it spilled none, so
    // it keeps the statements it had.
    // The same rule was knowingly NOT applied to the plain four-per-CU instance, the headline's, which also came out larger there
    // (FRAMES 62 > 65, PREP 47 > 51, the loop's own statements +5, spilled SGPRs 15 > 31: about 12 vector instructions per walked
    // profile, 0.3 k per ego) - it is the instance the stage was made for, V takes 38 of its 63 profiles out of the walk, and with
    // that cost included it measured 15.8 % fewer vector instructions and 8 % less time (profiles/group_hit_valu_count.txt).  The
    // cause is another register assignment around the mask read at the loop's head; reading only the mask's low word where nd <= 32
    // was tried to shorten it (EXPERIMENTS.md).
#if defined(FP_ABL_NO_GROUP) || defined(FP_ABL_NO_VMAX)
    constexpr bool kGroup = false;
#else
    constexpr bool kGroup = kSure && !WIN;
#endif
    // Stage W (a WHOLE ego ends: every candidate of the workgroup's slices collides - see WEXIT): the instances with stage V, whose full
    // masks are the verdict, less the one with the appended search.  -DFP_ABL_NO_WHOLE compiles it out.
    // Not a FISS instance: W skips the argmin WITH its workgroup barrier, and in those instances that barrier is part of the hand-over
    // to the ego's search workgroup - every thread's table stores are acknowledged (s_waitcnt) BEFORE it, thread 0 raises the flag
    // BEHIND it (see the template's comment).  Without it thread 0 could raise the flag while other wavefronts still store their rows.
    // Those instances always write the tables, so W could only ever take the argmin off them; they keep the parent's statements.
    // (In the other instances the tables are read by later kernels or the host, behind the kernel's end.)
#if defined(FP_ABL_NO_WHOLE)
    constexpr bool kWhole = false;
#else
    constexpr bool kWhole = kGroup && !FISS;
#endif
    // The argmin by one wavefront (ARGMIN below): every instance comes out smaller with it but the shaped polygon instance without a
    // window (80 VGPRs, all in use), which spills two VGPRs with it and keeps the statements it had.
    constexpr bool kArgWave = !(kShape && POLY && !WIN);
    // the same number in a scalar register (kCut): a phase that belongs to some of the wavefronts is entered on a scalar
    // compare and a branch - on `wave` every wavefront pays the vector compare and the EXEC round trip of a phase that is not its own
    const int wave_s = kCut ? __builtin_amdgcn_readfirstlane(wave) : wave;
    const int nd = kShape ? ND : p.nd, nv = kShape ? NV : p.nv, nt = kShape ? NT : p.nt;
    const int C = nd * nv * nt;
    // this workgroup's slices (kOnePart: nsplit is 1 or 2 and the products are not negative - the same quotients)
    const int it_lo = kOnePart ? (part * nt) >> (nsplit - 1) : part * nt / nsplit, it_hi = kOnePart ? ((part + 1) * nt) >> (nsplit - 1) : (part + 1) * nt / nsplit;
    const int n_it = it_hi - it_lo;
    const int stride = kShape ? STRIDE : p.check_stride;
    const int n_obs_tab = kShape ? NOBS : bt.n_obs;  // obstacles per scene of the table
    const double tick = p.tick_t;

    // wcap < NX: the coefficient rows in LDS are a WINDOW of wcap segments (make_layout's coef_cols) that starts one segment behind the ego
    const bool windowed = WIN && wcap < bt.NX;
    const int ld = windowed ? wcap : bt.NX;  // row stride of the LDS coefficient table
    const Layout L = make_layout(bt.NX, n_obs_tab, rows_max, hp_max, nd, nv, nt, kItemCap, kWaves, POLY ? bt.poly_stride : 0, kSlim, wcap);
    double* s_knots = (double*)(smem + L.knots);
    double* s_coef = (double*)(smem + L.coef);
    unsigned short* s_lut = (unsigned short*)(smem + L.lut);
    // obstacle sizes: (half length, half width) pairs and the bounding radii in their own array (a lane reads another obstacle's record
    // than its neighbour: 24 useful bytes per lane instead of a 32-byte record)
    struct DimTab {
        double2* hlw;
        double* rad;
        double* rin;  // polygon columns: radius of the disk about the rotation centre inside the ring (poly_inner_radius); else 0
        __device__ __forceinline__ ObsDim get(int j) const { const double2 a = hlw[j]; return ObsDim{a.x, a.y, rad[j], 0.0}; }
    };
    const DimTab s_dim{(double2*)(smem + L.dim), (double*)(smem + L.dim) + 2 * n_obs_tab, (double*)(smem + L.dim) + 3 * n_obs_tab};
    // polygon rings of the ego's scene: the LDS copy when it exists (indexed by obstacle), else the global table (indexed by column)
    const bool rings_in_lds = POLY && poly_lds_verts(n_obs_tab, ka.b.poly_stride) > 0;
    // poses of the (row, obstacle) items that survive the group test, in the order of the item list: the table itself is read from
    // global memory exactly once (registers -> group test), only the ~7 % the slices can touch are kept
    const SplitTab<ObsPose> s_spose{(double2*)(smem + L.pose), (double2*)(smem + L.pose) + kItemCap};
    const int n_frames = mul24(kWaves, hp_max);  // records of the frame table: [wavefront][point]
    const SplitTab<Frame> s_frames{(double2*)(smem + L.frames), (double2*)(smem + L.frames) + n_frames};
    using fan_t = typename FanType<kSlim>::type;  // the lateral fan bounds: [slice][hp_max]
    fan_t* s_fan_d = (fan_t*)(smem + L.dmax);
    fan_t* s_fan_dd = (fan_t*)(smem + L.ddmax);
    float* s_wfat = (float*)(smem + L.wfat);  // [wavefront][rows_max]
    ObsDim* s_grp = (ObsDim*)(smem + L.grp);  // reused as {cx, cy, radius, -}
    unsigned short* s_items = (unsigned short*)(smem + L.iqueue);  // item (row r, obstacle j), see kItemShift
    // A survivor's item in the list: the shaped instances pack it as r << kItemShift | j (kItemShift = bits of NOBS - 1), so that
    // B and N take it apart with a shift and a mask; where the shape is a run-time value, or the packed code would not fit the list's
    // 16 bits, it is the table index mul24(r, n_obs) + j and a division takes it apart (kItemShift = 0).
    constexpr int kItemShift = kShape ? item_shift(NOBS, ROWS) : 0;
    double* s_pows = (double*)(smem + L.pows);
    double* s_ts = (double*)(smem + L.samples);
    double* s_vs = s_ts + nt;
    double* s_ds = s_vs + nv;
    double* s_lon_sum = (double*)(smem + L.lon_sum);
    double* s_lat_sum = (double*)(smem + L.lat_sum);
    int2* s_lon_meta = (int2*)(smem + L.lon_meta);
    double* s_qlon = (double*)(smem + L.qlon);  // [nt][nv][2]
    double* s_qlat = (double*)(smem + L.qlat);  // [nt][nd][3]
    uint4* s_box = (uint4*)(smem + L.box);      // [rows] {min x, max x, min y, max y} relative to the first knot
    uint32_t* s_collmask = (uint32_t*)(smem + L.coll);  // [lon profile][2], bit id = lateral sample id of the profile collides
    using hit_t = typename std::conditional<kSlim, uint16_t, uint32_t>::type;  // (point k, survivor index) codes
    hit_t* s_hits = (hit_t*)(smem + L.queue);  // [wavefront][kWave]
    int* s_cnt = (int*)(smem + L.cnt);
    int* s_nslice = (int*)(smem + L.nslice);
    Best* s_best = (Best*)(smem + L.best);
    // Stage V's tables.  The group circles [end speed][row]{cx, cy, (thr - rad)^2, -} stand in the walk's frame tables, which are dead until
    // the walk's barrier and again from its last barrier to the next item chunk's walk: VCIRC rebuilds them for every item chunk.
    // The bound of |P''| (fp32 bits, a wave maximum like s_cnt[5]) stands in s_best[1]: s_cnt's eight words are taken, and a kArgWave
    // instance - every kGroup instance is one - writes s_best[0] alone, after the last walk.
    double* s_vcirc = (double*)(smem + L.frames);
    uint32_t* s_vword = (uint32_t*)&s_best[1];
    if constexpr (kGroup) {
        constexpr int kHpMaxC = ROWS * STRIDE + 1 > FP_MAX_POINTS ? FP_MAX_POINTS : ROWS * STRIDE + 1;
        static_assert(kArgWave && 32 * NV * ROWS <= 32 * kWaves * kHpMaxC && ND <= 64, "stage V: s_best[1] is free and the circles fit the frame tables");
    }
    // {first knot, bucket width reciprocal, ego half length, half width, half diagonal; [5..10] ego start state, [11] d_dd0 / 2}: uniform FP64 values live in VECTOR registers
    // (the scalar unit has no FP64); kept in registers from the prologue to the last slice they cost the three-workgroup variant spills
    double* s_k = (double*)(smem + L.konst);

    // the ego's scalars: independent global reads, all issued before the first one is waited for (a read costs ~1-2 us)
    // the per-ego arrays: at the addresses in the batch, or (InlineIn, latency instances only) inside this kernel's own argument block
    const double *in_d = bt.d_samples, *in_t = bt.t_samples, *in_v = bt.v_samples, *in_ts = bt.target_speed, *in_ego = bt.ego;
    const int32_t *in_frame = bt.frame_of, *in_scene = bt.scene_of, *in_tnow = bt.t_now;
    if constexpr (OCC <= 4) {
        if (inl.on) {
            // (the blob's place in this kernel's own argument segment: taking the address of the by-value parameter itself would
            // make the compiler keep a private copy of it)
            const unsigned char* base = (const unsigned char*)__builtin_amdgcn_kernarg_segment_ptr() + kInlineOffset;
            in_d = (const double*)(base + (size_t)bt.d_samples); in_t = (const double*)(base + (size_t)bt.t_samples);
            in_v = (const double*)(base + (size_t)bt.v_samples); in_ts = (const double*)(base + (size_t)bt.target_speed);
            in_ego = (const double*)(base + (size_t)bt.ego); in_frame = (const int32_t*)(base + (size_t)bt.frame_of);
            in_scene = (const int32_t*)(base + (size_t)bt.scene_of); in_tnow = (const int32_t*)(base + (size_t)bt.t_now);
            if (inl.publish && blockIdx.x == 0)  // (InlineIn::publish: the following kernels of the call read the arrays from device memory)
                for (int i = threadIdx.x; i < inl.n8; i += kThreads) ((unsigned long long*)inl.publish)[i] = ((const unsigned long long*)base)[i];
        }
    }
    const int skip_flag = bt.skip ? bt.skip[b] : 0;
    const int f = in_frame[b];
    const int sc = in_scene[b];
    const double* ring_base = rings_in_lds ? (const double*)(smem + L.poly) : ka.b.obs_poly;
    const size_t ring_col0 = rings_in_lds ? (size_t)0 : (size_t)(sc >= 0 ? sc : 0) * (size_t)ka.b.n_obs;
    const int t_now = in_tnow[b];
    const double target_speed = in_ts[b];
    const double* eg = in_ego + (size_t)b * 6;
    const double s0 = eg[0], s_d0 = eg[1], s_dd0 = eg[2], d0 = eg[3], d_d0 = eg[4], d_dd0 = eg[5];
    // [section SKIPPED]
    if (skip_flag) {  // finished ego of a closed-loop batch (block-uniform exit)
        if (part == 0) {
            if (tid == 0 && dur) dur[b] = 0;
            if (tid == 0) { ka.r.best_idx[b] = -1; ka.r.best_cost[b] = __builtin_nan(""); }
            if constexpr (OCC > 4) {
                if (ka.epi_flag) {  // (the appended epilogue workgroups write the NaN series / the zero flag word of a skipped ego too)
                    if (tid == 0) {
                        __atomic_signal_fence(__ATOMIC_SEQ_CST);
                        __hip_atomic_store(&ka.idx_shadow[b], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __atomic_signal_fence(__ATOMIC_SEQ_CST);
                        __builtin_amdgcn_s_waitcnt(0);
                        __atomic_signal_fence(__ATOMIC_SEQ_CST);
                        __hip_atomic_store(&ka.epi_flag[b], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    return;
                }
            }
            if (tid == 0 && ka.idx_shadow) ka.idx_shadow[b] = -1;
            if constexpr (FISS) {
                if (tid == 0 && ft.flag) __hip_atomic_store(&ft.flag[b], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (its search workgroup writes the "none" outputs)
            }
            if (ka.r.best_traj) {  // NaN series, flag word 0 (returns before it touches the spline or the scratch)
                const double nan = __builtin_nan("");
                if (wave == 0) winner_series_wave(ka, b, b, false, nan, nan, nan, lane, SplineLds{nullptr, nullptr, 0, 0});
            }
        }
        return;
    }
    // [/section SKIPPED]
    // [/section ENTRY]
    // [section STAGE]
    // ---------------------------------------------------------------- stage: ego, spline, obstacle rows
    // Global reads cost 1-2 us each, so everything that depends only on the scalars above is requested at once.  The obstacle
    // table is NOT staged: the group test reads it once, straight from global memory, and keeps the poses of its survivors
    // (rows_stage = the rows the table holds from t_now on).
    const int NX = bt.NX;
    const int n_obs = sc >= 0 ? n_obs_tab : 0;
    const float inv_nobs_s = 1.0f / (float)(n_obs > 0 ? n_obs : 1);
    int rows_stage = 0;  // obstacle rows of the table from t_now on: poses k = r*stride, k + t_now < T_obs
    if (n_obs > 0) {
        const int in_table = bt.T_obs - t_now;
        rows_stage = in_table > 0 ? (in_table + stride - 1) / stride : 0;
        if (rows_stage > rows_max) rows_stage = rows_max;
    }
    const double* gp = bt.obs_pose + (size_t)(sc >= 0 ? sc : 0) * bt.T_obs * n_obs_tab * 4;
#ifndef FP_POSE_FLIGHT
#define FP_POSE_FLIGHT 2
#endif
    // pose reads in flight per lane in the group test.  The four-per-CU instances take three (512 x 3 items: the 1250 of config 3 in ONE pass;
    // same-box A/B 130.7-131.2 against 131.6-132.2 us per step); three in the three-per-CU shaped instance spill two VGPRs.
    constexpr int kPoseFlight = OCC > 6 ? FP_POSE_FLIGHT + 1 : FP_POSE_FLIGHT;
    auto fetch_poses = [&](int i0, double4* ps) {
#pragma unroll
        for (int u = 0; u < kPoseFlight; ++u) {
            const int i = i0 + u * kThreads + tid;
            ps[u] = make_double4(0.0, 0.0, 0.0, 0.0);
            if (i < rows_stage * n_obs) {
                const int r = div_by<NOBS, ROWS * NOBS>(i, inv_nobs_s), j = i - mul24(r, n_obs);
                ps[u] = *(const double4*)(gp + ((size_t)(mul24(r, stride) + t_now) * n_obs + j) * 4);
            }
        }
    };
    const int nx = bt.nx[f];
    const int fts = n_obs > 0 ? bt.final_time_step[sc] : 0;
    int w0 = 0;  // first segment of the coefficient window (windowed), else 0
    {
        const double* gk = bt.knots + (size_t)f * NX;
        const double* gc = bt.coef + (size_t)f * 8 * NX;
        // [0]: counter of the item list; [1]: kCut instances: the ends of d_samples, packed (see the cost sums); [2]: slices whose lon profiles need the point-by-point scan; [3]: ticket; [4]: knots closer than a
        // bucket (the segment hint needs its loops); [5], [6]: fp32 bit patterns of the spline's speed bound and of the largest lateral offset;
        // [7]: kCut instances: the ends of the ego's v_samples, packed like [1] (see the row ranges)
        if (tid < 8) s_cnt[tid] = 0;
        if (kGroup && tid == 8) s_vword[0] = 0u;
#if defined(FP_PHASE_STAMPS)
        if (tid == 0) { s_walk_t[0] = 0xFFFFFFFFu; s_walk_t[1] = 0u; }
#endif
        // all NX columns (the copy does not wait for nx; columns >= nx hold the +inf padding / are never addressed)
        for (int i = tid; i < NX; i += kThreads) s_knots[i] = gk[i];
        for (int i = tid; i < nt + nv + nd; i += kThreads)
            s_ts[i] = i < nt ? in_t[i] : (i < nt + nv ? in_v[(size_t)b * nv + (i - nt)] : in_d[i - nt - nv]);
        if (windowed) {
            // Coefficient WINDOW: the segment the ego stands on = (knots <= s0) - 1, counted by the threads that hold a knot each (one more
            // barrier and one more dependent round trip than the whole-table copy: only lines too long for the layout pay it); the window
            // starts one segment behind it.  Whatever a trajectory point needs outside the window is read from global memory (rare: the
            // window is sized by the host for the residency it buys, not for a guarantee).
            int below = 0;
            for (int i0 = 0; i0 < NX; i0 += kThreads) below += __syncthreads_count(i0 + tid < nx && gk[i0 + tid] <= s0);
            w0 = below - 2;  // (the ego's segment - 1)
            w0 = w0 > nx - 1 - wcap ? nx - 1 - wcap : w0;
            w0 = __builtin_amdgcn_readfirstlane(w0 < 0 ? 0 : w0);
            for (int i = tid; i < 8 * wcap; i += kThreads) {
                const int r = i / wcap, c = i - r * wcap;
                s_coef[i] = w0 + c < NX ? gc[(size_t)r * NX + w0 + c] : 0.0;
            }
        } else if constexpr (OCC > 6) {
            // [8][NX], same layout; the four-per-CU instances in 16-byte pieces (8 NX doubles are an even count; a global load needs no more
            // than the doubles' own alignment) - one trip instead of two; in the polygon three-per-CU instance the same change spills two VGPRs
            for (int i = tid; i < 4 * NX; i += kThreads) ((double2*)s_coef)[i] = ((const double2*)gc)[i];
        } else {
            for (int i = tid; i < 8 * NX; i += kThreads) s_coef[i] = gc[i];
        }
        if (n_obs > 0) {
            const double* gd = bt.obs_dims + (size_t)sc * n_obs * 2;
            if constexpr (POLY) {  // the scene's rings, when they fit (same layout as in global memory: [obstacle][poly_stride] vertex pairs)
                const int nv2 = poly_lds_verts(n_obs_tab, bt.poly_stride);
                const double2* gr = (const double2*)bt.obs_poly + (size_t)sc * n_obs * bt.poly_stride;
                for (int i = tid; i < nv2; i += kThreads) ((double2*)(smem + L.poly))[i] = gr[i];
            }
            for (int j = tid; j < n_obs; j += kThreads) {
                const double hl = 0.5 * gd[2 * j], hw = 0.5 * gd[2 * j + 1];
                s_dim.hlw[j] = make_double2(hl, hw);
                s_dim.rad[j] = sqrt(fma(hl, hl, hw * hw));
                if constexpr (POLY) {
                    const size_t col = (size_t)sc * n_obs + j;
                    const int nvx = bt.obs_nvert[col];
                    s_dim.rin[j] = nvx > 0 ? poly_inner_radius(bt.obs_poly + col * 2 * (size_t)bt.poly_stride, nvx) : 0.0;
                    ((int32_t*)(smem + L.nvert))[j] = nvx;
                }
            }
        }
    }
    // the LDS spline: every knot, and the coefficient columns of segments [w0, w0 + ld) addressed by their ABSOLUTE segment index
    SplineLds sp{s_knots, s_coef - w0, nx, ld};
    // frame of (segment, offset): from the LDS table, or - a segment outside the coefficient window - from the batch's table in global memory
    auto frame_at = [&](int seg, double dxs, double& px, double& py, double& tx, double& ty) {
        if (!windowed || (unsigned)(seg - w0) < (unsigned)wcap) {
            spline_frame(sp, seg, dxs, px, py, tx, ty);
        } else {
            const int fg = in_frame[b];
            spline_frame(SplineLds{bt.knots + (size_t)fg * bt.NX, bt.coef + (size_t)fg * 8 * bt.NX, nx, bt.NX}, seg, dxs, px, py, tx, ty);
        }
    };
    // [/section STAGE]
    // [section GLUE]
    if (kEgoEarly && tid == 8) { s_k[5] = s0; s_k[6] = s_d0; s_k[7] = s_dd0; s_k[8] = d0; s_k[9] = d_d0; s_k[10] = d_dd0; s_k[11] = d_dd0 * 0.5; }
    __syncthreads();
    FP_STAMP(0);
    // the ego's start state as the prologue's solves read it (kEgoEarly: from LDS already)
    auto pS0 = [&]() -> double { if constexpr (kEgoEarly) return s_k[5]; else return s0; };
    auto pSd0 = [&]() -> double { if constexpr (kEgoEarly) return s_k[6]; else return s_d0; };
    auto pSdd0 = [&]() -> double { if constexpr (kEgoEarly) return s_k[7]; else return s_dd0; };
    auto pD0 = [&]() -> double { if constexpr (kEgoEarly) return s_k[8]; else return d0; };
    auto pDd0 = [&]() -> double { if constexpr (kEgoEarly) return s_k[9]; else return d_d0; };
    auto pDdd0 = [&]() -> double { if constexpr (kEgoEarly) return s_k[10]; else return d_dd0; };
    // [/section GLUE]
    // [section LUT]
    // Arclength buckets -> segment hint: lut[b] = bisect_right(knots, k0 + b*width) - 1, 2*nx buckets.  A point then
    // needs one table read plus a short walk instead of a log2(nx) search (knots may be non-uniform: the walk fixes it).
    const int n_buckets = 2 * nx;
    const double knot0 = s_knots[0], knot_last = s_knots[nx - 1];
    // The bucket width and its reciprocal are two fp64 divisions.  They are read by the wavefronts that fill the table, by those that
    // check the knot spacing below (fewer: nx - 1 segments against 2 nx + 1 buckets) and by thread 0 (s_k[1]): in the kCut instances
    // the others branch around them on a scalar test.
    double bucket_w = 0.0, inv_bucket_w = 0.0;
    if (!kCut || wave_s * kWave <= n_buckets) {
        bucket_w = (knot_last - knot0) / (double)n_buckets;
        inv_bucket_w = bucket_w > 0.0 ? 1.0 / bucket_w : 0.0;
    }
    for (int bkt = tid; bkt <= n_buckets; bkt += kThreads) {
        const double sb = knot0 + (double)bkt * bucket_w;
        int lo = 0, hi = nx;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sb < s_knots[mid]) hi = mid; else lo = mid + 1;
        }
        int seg = lo - 1;
        seg = seg < 0 ? 0 : (seg > nx - 2 ? nx - 2 : seg);
        s_lut[bkt] = (unsigned short)seg;
    }
    // [/section LUT]
    // [section VBOUND]
#if defined(FP_ABL_NO_VMAX)
    if (tid == 0) s_cnt[4] = 1;  // (the knot spacing is checked in the loop below)
    if (false) {
#else
    if (n_obs > 0) {
#endif
        // upper bound of the spline's parametric speed |P'(s)| (the arclength parameter is the cumulative CHORD length, so it is a
        // little above 1 in bends): per segment the exact maxima of the two quadratic derivative components (ends + vertex).  The
        // once-per-ego group test turns an arclength interval into a circle with it.  Wave maximum of fp32 bit patterns, one LDS
        // atomic per wavefront (a NaN coefficient is the largest pattern: the circle then keeps every obstacle).
        // (coefficient window: over its segments only - a row whose arclength range leaves the window gets an infinite circle below)
        // In the same pass, s_cnt[4] != 0: some knots are no further apart than a bucket is wide (or the line is degenerate, or only its
        // window was looked at) - a point's segment can then lie several knots from its bucket's hint, and the walk's frames take
        // lut_segment's loops instead of lut_segment_step.  (A uniform line's knots are 2 nx / (nx - 1) buckets apart.)
        const int seg_end = windowed ? (w0 + wcap < nx - 1 ? w0 + wcap : nx - 1) : nx - 1;
        // The 1e-6 of slack below has to cover the rounding of (s - knot0) / width and of a bucket's start, which grow with the
        // arclengths themselves (2^-52 |knot| each), not with the bucket: a line whose |knot| 2^-50 exceeds it (arclengths of 1e9 m with
        // metre-sized buckets) takes the loops too.
        if (tid == 0 && (windowed || !(inv_bucket_w > 0.0) || !(fmax(fabs(s_knots[0]), fabs(s_knots[nx - 1])) * inv_bucket_w < 1e-6 * 0x1p50))) s_cnt[4] = 1;
        for (int i0 = w0 + wave * kWave; i0 < seg_end; i0 += kThreads) {
            const int i = i0 + lane;
            uint32_t bits = 0u, bits2 = 0u;
            if (i < seg_end) {
                const double h = s_knots[i + 1] - s_knots[i];
                if (!(h * inv_bucket_w >= 1.0 + 1e-6)) atomicOr((unsigned int*)&s_cnt[4], 1u);
                double m2 = 0.0, w2 = 0.0;
#pragma unroll
                for (int ax = 0; ax < 2; ++ax) {
                    const double b1 = sp.coef[(4 * ax + 1) * ld + i], c2 = 2.0 * sp.coef[(4 * ax + 2) * ld + i], d3 = 3.0 * sp.coef[(4 * ax + 3) * ld + i];
                    double m = fmax(fabs(b1), fabs(fma(fma(d3, h, c2), h, b1)));  // g(u) = b1 + c2 u + d3 u^2 at u = 0, h
                    const double uv = -c2 / (2.0 * d3);
                    if (uv > 0.0 && uv < h) m = fmax(m, fabs(fma(fma(d3, uv, c2), uv, b1)));
                    if (!(m == m) || !(h == h)) m = __builtin_nan("");
                    m2 = fma(m, m, m2);
                    if constexpr (kGroup) {  // stage V: |P''| - g'(u) = c2 + 2 d3 u is linear, extreme at the segment's ends
                        double w = fmax(fabs(c2), fabs(fma(2.0 * d3, h, c2)));
                        if (!(c2 == c2) || !(d3 == d3) || !(h == h)) w = __builtin_nan("");
                        w2 = fma(w, w, w2);
                    }
                }
                bits = __float_as_uint(float_above(sqrt(m2)) * 1.0000005f);
                if constexpr (kGroup) bits2 = __float_as_uint(float_above(sqrt(w2)) * 1.0000005f);
            }
            if constexpr (kGroup) {  // (a NaN is the largest pattern: VCIRC then leaves every circle silent)
#pragma unroll
                for (int off = kWave / 2; off > 0; off >>= 1) {
                    const uint32_t o2 = (uint32_t)__shfl_xor((int)bits2, off, kWave);
                    bits2 = o2 > bits2 ? o2 : bits2;
                }
                if (lane == 0) atomicMax(&s_vword[0], bits2);
            }
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1) {
                const uint32_t o2 = (uint32_t)__shfl_xor((int)bits, off, kWave);
                bits = o2 > bits ? o2 : bits;
            }
            if (lane == 0) atomicMax((unsigned int*)&s_cnt[5], bits);
        }
    }
    // [/section VBOUND]
    // [section GLUE]
    int horizon_cap = 0;  // final_time_step - time_step_now (:173-174)
    int rows = 0;         // obstacle rows the collision horizon can touch: rows of the table below final_time_step
    if (n_obs > 0) {
        horizon_cap = fts - t_now;
        int h = horizon_cap < points_cap(p) ? horizon_cap : points_cap(p);
        if (h < 0) h = 0;
        rows = (h + stride - 1) / stride;
        if (rows_stage < rows) rows = rows_stage;
    }
    for (int c = tid; c < 2 * nt * nv; c += kThreads) s_collmask[c] = 0u;
    for (int r = tid; r < rows; r += kThreads) {
        s_box[r] = make_uint4(kOrdPosInf, kOrdNegInf, kOrdPosInf, kOrdNegInf);  // empty
        // stage V: the row's range of lateral offsets over every slice and lateral sample, two ordered fp32 words in the unused fourth
        // word of the row's circle record (FAN fills them; row 0's word holds S's threshold, and at t = 0 every offset is d0)
        if (kGroup && r >= 1) *(uint2*)&s_grp[r].pad = make_uint2(kOrdPosInf, kOrdNegInf);
    }
    // points whose frame the collision stage can touch: 0 .. hp-1 (pose k needs point k+1 for its heading)
    const int pose_limit = rows * stride < horizon_cap ? rows * stride : horizon_cap;  // poses k < pose_limit (and k < M)
    int hp = pose_limit > 0 ? pose_limit + 1 : 0;
    if (hp > hp_max) hp = hp_max;
    // (thread 0 leaves them in s_k below: in the kCut instances the other wavefronts branch around the square root)
    double veh_hl = 0.0, veh_hw = 0.0, r_ego = 0.0;
    if (!kCut || wave_s == 0) {
        veh_hl = 0.5 * p.veh_l; veh_hw = 0.5 * p.veh_w;
        r_ego = sqrt(fma(veh_hl, veh_hl, veh_hw * veh_hw));
    }
    // (no barrier: phase A0 below needs only what the staging barrier made visible - the LUT / speed bound above and the solves below
    // are independent and share one barrier interval; the solves go to the LAST threads, the LUT to the first)
    FP_STAMP(1);

    const double* v_samples = s_vs;
    int item_base = 0;  // the item list's counter at the start of the current chunk (block-uniform)

    // ---------------------------------------------------------------- phase A0 (once): masks / M / cost sums of every profile
    // (0) lane per lon profile: the boundary-value solve (two divisions), kept for the whole kernel; meta = {N, no flags}.
    // (1) lane per (lon profile, time point): speed / acceleration masks by LDS atomic OR, the truncation index M (first point
    //     off the spline, a pure range test) by LDS atomic MIN - the same brute force over every point as the reference, with
    //     every lane busy (a wavefront per profile would idle a third of its lanes and all of its second half);
    //     one lane per slice: the power sums S_k = sum_{i<N} (t_i - c)^k (k = 0..10) about the samples' centre in closed form (power_sums_closed).
    // (2) lane per profile: the six cost sums in closed form.  Each summand is the square of a polynomial in t
    //     (s_d - v_target: cubic, s_dd: quadratic, s_ddd: linear, d: quintic, d_dd: cubic, d_ddd: quadratic), so
    //     sum_i p(t_i)^2 = sum_k c_k S_k with c = p (*) p (coefficient convolution) - no per-point work and no reductions.
    //     Conditioning is benign on t in [0, 10] (terms ~1e2..1e4 against sums ~1e1..1e3: ~1e-12 absolute), far inside the
    //     1e-6 cost bar, and the expressions are even in the lateral boundary data, so mirrored candidates still tie bit-exactly.
    // [/section GLUE]
    // [section SOLVE]
    // (kCut instances: the wavefronts that hold no solve branch around the loop on a scalar test; likewise DALL, POWS and CIRCLES below)
    if (!kCut || (wave_s + 1) * kWave + n_it * nv > kThreads)
    for (int e = kThreads - 1 - tid; e < n_it * nv; e += kThreads) {
        const int eq = div_by<NV, NT * NV>(e, 1.0f / (float)nv);
        const int it = it_lo + eq, iv = e - mul24(eq, nv);
        const double T = s_ts[it];
        const Quartic q = quartic_bvp(pS0(), pSd0(), pSdd0(), v_samples[iv], 0.0, T);
        s_qlon[2 * (mul24(it, nv) + iv)] = q.a3;
        s_qlon[2 * (mul24(it, nv) + iv) + 1] = q.a4;
        const int N = arange_len(T, tick);
        s_lon_meta[mul24(it, nv) + iv] = make_int2(N, 0);
        if (iv == 0) s_nslice[it] = N;
        // Proof that the profile violates nothing, from the extrema of the polynomials over the continuous interval [0, t_last]
        // (a superset of the grid): |s_dd| (quadratic: ends + vertex), s_d (cubic: ends + the roots of s_dd), and s inside the
        // spline's range (s_d >= 0 makes s monotone: its ends suffice).  Margins of 1e-9 dwarf the rounding of the Horner
        // evaluations the point-by-point scan would do; anything not proven (including NaNs) falls back to that scan, so the
        // outcome is the scan's outcome either way.
        if (N > 0) {
            const double a2 = pSdd0() * 0.5, tl = (double)(N - 1) * tick;
            auto acc = [&](double t) { return fma(fma(12.0 * q.a4, t, 6.0 * q.a3), t, 2.0 * a2); };
            auto vel = [&](double t) { return fma(fma(fma(4.0 * q.a4, t, 3.0 * q.a3), t, 2.0 * a2), t, pSd0()); };
            const double qa = 12.0 * q.a4, qb = 6.0 * q.a3, qc = 2.0 * a2;  // s_dd = qa t^2 + qb t + qc
            double amax = fmax(fabs(acc(0.0)), fabs(acc(tl)));
            const double tv = -qb / (2.0 * qa);
            if (tv > 0.0 && tv < tl) amax = fmax(amax, fabs(acc(tv)));
            bool proven = amax <= p.max_accel * (1.0 - 1e-9) - 1e-12;
            double vmax = fmax(vel(0.0), vel(tl)), vmin = fmin(vel(0.0), vel(tl));
            const double disc = fma(qb, qb, -4.0 * qa * qc);
            if (disc >= 0.0) {  // stable quadratic roots; a root that is NaN / inf / outside (0, t_last) is not an interior extremum
                const double sq = sqrt(disc), qq = -0.5 * (qb + (qb >= 0.0 ? sq : -sq));
                const double r1 = qq / qa, r2 = qc / qq;
                if (r1 > 0.0 && r1 < tl) { vmax = fmax(vmax, vel(r1)); vmin = fmin(vmin, vel(r1)); }
                if (r2 > 0.0 && r2 < tl) { vmax = fmax(vmax, vel(r2)); vmin = fmin(vmin, vel(r2)); }
            } else if (!(disc < 0.0)) proven = false;  // NaN
            const double pad = amax * 1e-6;  // |s_d(t) - s_d(r)| <= max|s_dd| |t - r|: covers a root off by a microsecond
            proven = proven && vmax + pad <= p.max_speed * (1.0 - 1e-9) - 1e-12 && vmin - pad >= 0.0;
            const double s_end = fma(fma(fma(fma(q.a4, tl, q.a3), tl, a2), tl, pSd0()), tl, pS0());
            const double eps = 1e-9 * (1.0 + fabs(knot_last) + fabs(knot0));
            proven = proven && pS0() >= knot0 + eps && s_end < knot_last - eps;
            if (!proven) atomicOr((unsigned int*)&s_cnt[2], 1u << ((it - it_lo) & 31));
        }
    }
    // [/section SOLVE]
    // [section DALL]
    // bound of |d(t)| over ALL slices and lateral samples (the once-per-ego group test needs it), by the wavefronts the solves above
    // leave idle.  In the Hermite form of the quintic with a resting end state,
    //   d(t) = d_end + (d0 - d_end) h0 + d_d0 T h1 + d_dd0 T^2 h2  (tau = t / T),  h0 = 1 - 10 tau^3 + 15 tau^4 - 6 tau^5 in [0, 1],
    //   |h1| = |tau - 6 tau^3 + 8 tau^4 - 3 tau^5| <= 16/81,  h2 = tau^2 (1 - tau)^3 / 2 <= 54/3125:
    //   |d| <= max(|d0|, |d_end|) + 0.1976 |d_d0| T + 0.01729 |d_dd0| T^2.
    // Wave maximum of the fp32 bit patterns (a NaN is the largest pattern and keeps every obstacle), ONE LDS atomic per wavefront -
    // same-address LDS atomics of many lanes serialise badly.
#if defined(FP_ABL_NO_DALL)
    if (false) {
#else
    if (n_obs > 0 && wave_s >= 1) {
#endif
        for (int e0 = (wave_s - 1) * kWave; e0 < n_it * nd; e0 += (kWaves - 1) * kWave) {
            const int e = e0 + lane;
            uint32_t bits = 0u;
            if (e < n_it * nd) {
                const int eq = div_by<ND, NT * ND + kWave>(e < n_it * nd ? e : 0, 1.0f / (float)nd);
                const double T = s_ts[it_lo + eq], de = s_ds[e - mul24(eq, nd)];
                const double d0e = pD0();
                double bd = (fabs(d0e) > fabs(de) ? fabs(d0e) : fabs(de)) + 0.1976 * fabs(pDd0()) * T + 0.01729 * fabs(pDdd0()) * T * T;
                if (!(d0e == d0e) || !(de == de)) bd = __builtin_nan("");
                bits = __float_as_uint(float_above(bd) * 1.0000005f);
            }
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1) {
                const uint32_t o2 = (uint32_t)__shfl_xor((int)bits, off, kWave);
                bits = o2 > bits ? o2 : bits;
            }
            if (lane == 0 && bits) atomicMax((unsigned int*)&s_cnt[6], bits);
        }
    }
    // [/section DALL]
    // [section GLUE]
    if (tid == 0) { s_k[0] = knot0; s_k[1] = inv_bucket_w; s_k[2] = veh_hl; s_k[3] = veh_hw; s_k[4] = r_ego; }
    if constexpr (kSure) {
        // stage S's threshold, squared: thr = rho (1 - 1e-9) - 1e-6 with rho = min(half length, half width), the radius of the disk
        // inside the ego box at any heading (see the walk).  It stands in the unused fourth word of the first row circle (s_grp[0].pad:
        // CIRCLES writes the other three, G reads past it; the row exists also with no rows) - s_k's twelve words are taken and one more
        // would move every table behind it.  A thr that is not > 0 (a NaN size included) leaves -1: no squared distance is <= -1, S is silent.
        // (entered on the scalar test, like the square root above: the other wavefronts pay no vector compare for it)
        if (wave_s == 0 && tid == 0) {
            const double thr = (veh_hl < veh_hw ? veh_hl : veh_hw) * (1.0 - 1e-9) - 1e-6, both = veh_hl + veh_hw;  // (fmin would drop a NaN)
            s_grp[0].pad = thr > 0.0 && both == both ? thr * thr : -1.0;
        }
    }
    if (kEgoLds && !kEgoEarly && tid == 1) { s_k[5] = s0; s_k[6] = s_d0; s_k[7] = s_dd0; s_k[8] = d0; s_k[9] = d_d0; s_k[10] = d_dd0; s_k[11] = d_dd0 * 0.5; }
    // [/section GLUE]
    // [section POWS]
    {   // power sums of every slice (they need nothing but the time samples): a few threads of the middle
        const int i = tid - kThreads / 2;
        if ((!kCut || wave_s == kWaves / 2) && i >= 0 && i < n_it) power_sums_closed(arange_len(s_ts[it_lo + i], tick), tick, s_pows + (it_lo + i) * 11);
    }
    // [/section POWS]
    // [section VENDS]
    // kCut instances: the ends of the ego's v_samples for the row ranges below (s_cnt[7] = iv_lo | iv_hi << 8 | NaN << 16; nv <= 255),
    // found once by a wavefront that has nothing else in this interval (the solves take the last one, the power sums the middle one,
    // the LUT, the speed bound and the lateral bound the first ones).  Any order of v_samples, as for d_samples below.
    if constexpr (kCut) {
        if (wave_s == kWaves - 2) {
            int iv_lo = 0, iv_hi = 0;
            for (int iv = 1; iv < nv; ++iv) {
                iv_lo = s_vs[iv] < s_vs[iv_lo] ? iv : iv_lo;
                iv_hi = s_vs[iv] > s_vs[iv_hi] ? iv : iv_hi;
            }
            bool v_nan = false;
            for (int iv = 0; iv < nv; ++iv) v_nan = v_nan || !(s_vs[iv] == s_vs[iv]);
            if (lane == 0) s_cnt[7] = iv_lo | (iv_hi << 8) | ((int)v_nan << 16);
        }
    }
    // [/section VENDS]
    // [section GLUE]
    __syncthreads();
    FP_STAMP(2);
    auto eS0 = [&]() -> double { if constexpr (kEgoLds) return s_k[5]; else return s0; };
    auto eSd0 = [&]() -> double { if constexpr (kEgoLds) return s_k[6]; else return s_d0; };
    auto eSdd0 = [&]() -> double { if constexpr (kEgoLds) return s_k[7]; else return s_dd0; };
    auto eD0 = [&]() -> double { if constexpr (kEgoLds) return s_k[8]; else return d0; };
    auto eDd0 = [&]() -> double { if constexpr (kEgoLds) return s_k[9]; else return d_d0; };
    auto eDdd0 = [&]() -> double { if constexpr (kEgoLds) return s_k[10]; else return d_dd0; };
    auto eDdd0Half = [&]() -> double { if constexpr (kEgoLds) return s_k[11]; else return d_dd0 * 0.5; };  // (the walk's N: the product, ready)
    // [/section GLUE]
    // [section RANGES]
    if (n_obs > 0 && pose_limit > 0) {
        // ---- arclength range of every checked pose row over the lon profiles of ALL slices of this workgroup: lane = (row, slice),
        // loop over the end-speed samples, then LDS atomic min / max on order-preserving fp32 bit patterns (relative to the first knot).
        // (The truncation index M is still being reduced in this phase: poses off the spline count too, the circle clamps the range.)
        const float inv_rows = 1.0f / (float)(rows > 0 ? rows : 1);
        if constexpr (kCut) {
            // kCut instances: TWO profiles instead of nv.  quartic_bvp makes a3 and a4 affine in the end speed v:
            //   s(t; v) = base(t) + v g(t),  g(t) = t^3 / T^2 (1 - t / (2 T)) >= 0 for 0 <= t <= 2 T
            // (every point looked at has k < s_nslice[it], t <= T), so s is monotone in v and its ends over the samples sit at the
            // smallest and the largest sample (s_cnt[7], found once per ego).  Those two are the parent's expressions on the parent's
            // operands, bit for bit; what is gone is the comparison with the samples between them.  How far can the COMPUTED s of a
            // middle sample - the number the walk's frames use - lie outside the two computed ends?  With u = 2^-53, X = |v| + |s_d0|,
            // Y = |a2| T, |V| <= X + 2 Y:  a3 carries at most u (9 X + 20 Y) / T^2 of absolute rounding (the operations of quartic_bvp,
            // one by one, cancellation in V and in 3 V - A T included), a4 at most u (8 X + 16 Y) / T^3, so a3 t^3 + a4 t^4 is off
            // by at most 36 u (X + Y) t; the Horner chain's four roundings add 4 u sum|term|, sum|term| <= |s0| + |s_d0| t + |a2| t^2
            // + |a3| t^3 + |a4| t^4 <= 5.2 Q with  Q = |s0| + t (|s_d0| + max|v| + |a2| T).  Each value is within 60 u Q of the
            // exact affine one, two values within 120 u Q < 2^-46 Q of their exact order.  That is NOT inside the slack of CIRCLES
            // at any magnitude (its absolute part is 1e-6: an |s0| of 1e9 m uses it up), so the range is widened HERE, where Q is
            // known, by E = 2^-44 Q on each side (four times the bound; 6e-11 m at s0 = 1 km); the subtraction of knot0 is monotone,
            // its rounding and that of lo - E are relative to the ends (2^-53, inside the 6e-8 the relative slack has to spare).
            // max|v| is at an end.  A NaN sample, a NaN end or an E that is not finite (an infinite sample makes its own end NaN
            // already: inf t - inf) keeps everything, as a NaN did before.
            const int ends = __builtin_amdgcn_readfirstlane(s_cnt[7]);
            const int iv_lo = ends & 0xFF, iv_hi = (ends >> 8) & 0xFF;
            const bool v_nan = (ends >> 16) != 0;
            const double v_abs = fmax(fabs(s_vs[iv_lo]), fabs(s_vs[iv_hi]));
            for (int e = tid; e < mul24(n_it, rows); e += kThreads) {
                const int itl = div_small(e, inv_rows), r = e - mul24(itl, rows);
                const int it = it_lo + itl;
                const int k = mul24(r, stride);
                if (k >= pose_limit || k >= s_nslice[it]) continue;
                const double t = (double)k * tick;
                const double* qa = s_qlon + 2 * (mul24(it, nv) + iv_lo);
                const double* qb = s_qlon + 2 * (mul24(it, nv) + iv_hi);
                const double sa = fma(fma(fma(fma(qa[1], t, qa[0]), t, eSdd0() * 0.5), t, eSd0()), t, eS0()) - knot0;
                const double sb = fma(fma(fma(fma(qb[1], t, qb[0]), t, eSdd0() * 0.5), t, eSd0()), t, eS0()) - knot0;
                const double E = fma(t, fabs(eSd0()) + v_abs + fabs(eSdd0() * 0.5) * s_ts[it], fabs(eS0())) * 0x1p-44;
                const bool bad = v_nan || !(sa == sa) || !(sb == sb) || !(E < __builtin_inf());
                uint32_t* bx = (uint32_t*)&s_box[r];
                if (bad) { atomicMin(bx + 0, kOrdNegInf); atomicMax(bx + 1, kOrdPosInf); }  // NaN: keep everything
                else { atomicMin(bx + 0, f32_ordered((float)(fmin(sa, sb) - E))); atomicMax(bx + 1, f32_ordered((float)(fmax(sa, sb) + E))); }
            }
        } else
        for (int e = tid; e < mul24(n_it, rows); e += kThreads) {
            const int itl = div_small(e, inv_rows), r = e - mul24(itl, rows);
            const int it = it_lo + itl;
            const int k = mul24(r, stride);
            if (k >= pose_limit || k >= s_nslice[it]) continue;
            const double t = (double)k * tick;
            double lo = __builtin_inf(), hi = -__builtin_inf();
            bool bad = false;
            for (int iv = 0; iv < nv; ++iv) {
                const double a3 = s_qlon[2 * (mul24(it, nv) + iv)], a4 = s_qlon[2 * (mul24(it, nv) + iv) + 1];
                const double sv = fma(fma(fma(fma(a4, t, a3), t, eSdd0() * 0.5), t, eSd0()), t, eS0()) - knot0;
                bad = bad || !(sv == sv);
                lo = fmin(lo, sv); hi = fmax(hi, sv);
            }
            uint32_t* bx = (uint32_t*)&s_box[r];
            if (bad) { atomicMin(bx + 0, kOrdNegInf); atomicMax(bx + 1, kOrdPosInf); }  // NaN: keep everything
            else if (lo <= hi) { atomicMin(bx + 0, f32_ordered((float)lo)); atomicMax(bx + 1, f32_ordered((float)hi)); }
        }
    }
    // [/section RANGES]
    // [section MASKS]
#if defined(FP_ABL_NO_SCAN)  // timing ablation: no point-by-point mask scan (results are wrong)
    const uint32_t scan_mask = 0u;
#else
    const uint32_t scan_mask = (uint32_t)s_cnt[2];
#endif
    if (tid == 0) FP_COUNT(9, __popc(scan_mask));
    for (int it = it_lo; it < it_hi; ++it) {
        if (!((scan_mask >> ((it - it_lo) & 31)) & 1u)) continue;  // every lon profile of the slice is proven clean
        const int N = arange_len(s_ts[it], tick);
        const float inv_n = 1.0f / (float)N;
        for (int e = tid; e < nv * N; e += kThreads) {
            const int iv = div_small(e, inv_n), i = e - mul24(iv, N);
            const double a3 = s_qlon[2 * (mul24(it, nv) + iv)], a4 = s_qlon[2 * (mul24(it, nv) + iv) + 1];
            const double a2 = eSdd0() * 0.5;
            const double t = (double)i * tick;
            const double s = fma(fma(fma(fma(a4, t, a3), t, a2), t, eSd0()), t, eS0());
            const double s_d = fma(fma(fma(4.0 * a4, t, 3.0 * a3), t, 2.0 * a2), t, eSd0());
            const double s_dd = fma(fma(12.0 * a4, t, 6.0 * a3), t, 2.0 * a2);
            const uint32_t bad = (s_d > p.max_speed ? FP_FLAG_SPEED : 0u) | (fabs(s_dd) > p.max_accel ? FP_FLAG_ACCEL : 0u);
            if (bad) atomicOr((unsigned int*)&s_lon_meta[mul24(it, nv) + iv].y, bad);
            if (!(s >= knot0) || !(s < knot_last)) atomicMin(&s_lon_meta[mul24(it, nv) + iv].x, i);  // calc_position -> None (cubic_spline.py:56-59)
        }
    }
    // [/section MASKS]
    // [section SUMS]
    if constexpr (kCut) {
        // kCut instances: the lon profiles go to the last wavefront and the lat profiles to the one before it, each entered on a scalar
        // test - dealt nv + nd lanes per slice as in the loop below, both wavefronts execute both branches.  The lat lane also keeps the
        // coefficients of its boundary-value solve for the fan bounds and the walk (QLAT below solves every one a second time), and the
        // wavefront before those two finds the ends of d_samples ONCE (s_cnt[1] = id_lo | id_hi << 8 | NaN << 16; nd <= 64) instead of
        // all eight in front of the fan bounds.  Every value is the expression it was; only the lane that evaluates it changed.
        for (int e0 = (kWaves - 1 - wave_s) * kWave; e0 < n_it * nv; e0 += kThreads) {
            const int e = e0 + lane;
            if (e < n_it * nv) {
                const int eq = div_by<NV, NT * NV>(e, 0.0f);
                const int it = it_lo + eq, iv = e - mul24(eq, nv);
                const Quartic q{eS0(), eSd0(), eSdd0() * 0.5, s_qlon[2 * (mul24(it, nv) + iv)], s_qlon[2 * (mul24(it, nv) + iv) + 1]};
                double lon[3];
                lon_cost_sums(q, target_speed, s_pows + it * 11, lon);
                double* o = s_lon_sum + 3 * (mul24(it, nv) + iv);
                o[0] = lon[0]; o[1] = lon[1]; o[2] = lon[2];
            }
        }
        for (int e0 = ((kWaves - 2 - wave_s) & (kWaves - 1)) * kWave; e0 < n_it * nd; e0 += kThreads) {
            const int e = e0 + lane;
            if (e < n_it * nd) {
                const int eq = div_by<ND, NT * ND>(e, 0.0f);
                const int it = it_lo + eq, id = e - mul24(eq, nd);
                const Quintic q = quintic_bvp(eD0(), eDd0(), eDdd0(), s_ds[id], 0.0, 0.0, s_ts[it]);
                double lat[3];
                lat_cost_sums(q, s_pows + it * 11, lat);
                double* o = s_lat_sum + 3 * (mul24(id, nt) + it);
                o[0] = lat[0]; o[1] = lat[1]; o[2] = lat[2];
                double* oq = s_qlat + 3 * (mul24(it, nd) + id);
                oq[0] = q.a3; oq[1] = q.a4; oq[2] = q.a5;
            }
        }
        if (wave_s == kWaves - 3) {
            int id_lo = 0, id_hi = 0;  // (the loops of the run-time-shape instances' fan bounds)
            for (int id = 1; id < nd; ++id) {
                id_lo = s_ds[id] < s_ds[id_lo] ? id : id_lo;
                id_hi = s_ds[id] > s_ds[id_hi] ? id : id_hi;
            }
            bool d_nan = false;
            for (int id = 0; id < nd; ++id) d_nan = d_nan || !(s_ds[id] == s_ds[id]);
            if (lane == 0) s_cnt[1] = id_lo | (id_hi << 8) | ((int)d_nan << 16);
        }
    } else {
        for (int e0 = (kWaves - 1 - wave) * kWave; e0 < n_it * (nv + nd); e0 += kThreads) {  // (the last wavefronts: the ranges above keep the first busy)  // (whole wavefronts: the row maxima below are wave reductions)
            const int e = e0 + lane;
            const bool live = e < n_it * (nv + nd);
            const int eq = live ? div_by<NV + ND, NT * (NV + ND)>(e, 1.0f / (float)(nv + nd)) : 0;
            const int it = it_lo + eq, sub = live ? e - mul24(eq, nv + nd) : 0;
            const double T = s_ts[it];
            const double* S = s_pows + it * 11;
            if (!live) {
            } else if (sub < nv) {
                const Quartic q{eS0(), eSd0(), eSdd0() * 0.5, s_qlon[2 * (mul24(it, nv) + sub)], s_qlon[2 * (mul24(it, nv) + sub) + 1]};
                double lon[3];
                lon_cost_sums(q, target_speed, S, lon);
                double* o = s_lon_sum + 3 * (mul24(it, nv) + sub);
                o[0] = lon[0]; o[1] = lon[1]; o[2] = lon[2];
            } else {
                const int id = sub - nv;
                const Quintic q = quintic_bvp(eD0(), eDd0(), eDdd0(), s_ds[id], 0.0, 0.0, T);
                double lat[3];
                lat_cost_sums(q, S, lat);
                double* o = s_lat_sum + 3 * (mul24(id, nt) + it);
                o[0] = lat[0]; o[1] = lat[1]; o[2] = lat[2];
            }
        }
    }
    // [/section SUMS]
    // [section QLAT]
    // lat polynomial coefficients of every slice of this workgroup, [slice][lateral sample] (absolute slice index): a boundary-value
    // solve costs two divisions - nd threads per slice (the last ones) instead of once per trajectory point
    // (A plain loop, in a lambda that is called on the spot: written without the lambda, the same statements come out of the compiler
    // with other register assignments and SGPR spills (38 600 lines of the 25 instances' assembly differ; with it, none) - and the
    // instances are to stay exactly as validated.)
    const float inv_nd = 1.0f / (float)nd;
    // (kCut instances: written by the lat lanes of the sums above)
    if constexpr (!kCut) [&] {
        for (int e = kThreads - 1 - tid; e < mul24(n_it, nd); e += kThreads) {
            const int itl = div_small(e, inv_nd), id = e - mul24(itl, nd);
            const Quintic q = quintic_bvp(eD0(), eDd0(), eDdd0(), s_ds[id], 0.0, 0.0, s_ts[it_lo + itl]);
            double* o = s_qlat + 3 * (mul24(it_lo + itl, nd) + id);
            o[0] = q.a3; o[1] = q.a4; o[2] = q.a5;
        }
    }();
    // [/section QLAT]
    // [section GLUE]
    __syncthreads();
    FP_STAMP(3);
    // [/section GLUE]
    // [section FAN]
    // ---- lateral fan bounds of EVERY slice: lane = (slice, point inside the collision horizon): fan half-width max|d| and
    // largest lateral step max|d(i + 1) - d(i)| over the lateral samples, float_above: never below the fp64 value.  For a fixed
    // horizon the quintic is AFFINE in its end offset (Hermite form, see the lateral bound above): d(t; d_end) = b(t) + d_end g(t),
    // so |d| and |d(i + 1) - d(i)| are convex in d_end and their maxima over the samples sit at the smallest and the largest
    // sample - two profiles are evaluated instead of nd (the rounding of the other samples' own evaluations, ~1e-16 relative,
    // is far inside float_above's 2^-22).  (The first threads: the circles below take the last ones.)
    if (n_obs > 0 && hp > 0) {
        int id_lo = 0, id_hi = 0;
        bool d_nan = false;
        if constexpr (kCut) {  // (found once per ego, see the sums above)
            const int ends = __builtin_amdgcn_readfirstlane(s_cnt[1]);
            id_lo = ends & 0xFF; id_hi = (ends >> 8) & 0xFF; d_nan = (ends >> 16) != 0;
        } else {  // (any order of d_samples: the reference passes np.linspace, the ABI does not require it)
            for (int id = 1; id < nd; ++id) {
                id_lo = s_ds[id] < s_ds[id_lo] ? id : id_lo;
                id_hi = s_ds[id] > s_ds[id_hi] ? id : id_hi;
            }
            for (int id = 0; id < nd; ++id) d_nan = d_nan || !(s_ds[id] == s_ds[id]);
        }
        const float inv_hp = 1.0f / (float)hp;
        for (int e = tid; e < mul24(n_it, hp); e += kThreads) {
            const int itl = div_small(e, inv_hp), i = e - mul24(itl, hp);
            const int it = it_lo + itl;
            const int np_i = hp < s_nslice[it] ? hp : s_nslice[it];
            if (i >= np_i) continue;
            const double t = (double)i * tick, tn = (double)(i + 1) * tick;
            float dm = 0.0f, ddm = 0.0f;
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const double* ql = s_qlat + 3 * (mul24(it, nd) + (side ? id_hi : id_lo));
                const double a3 = ql[0], a4 = ql[1], a5 = ql[2];
                const double d = fma(fma(fma(fma(fma(a5, t, a4), t, a3), t, eDdd0() * 0.5), t, eDd0()), t, eD0());
                const double dn = fma(fma(fma(fma(fma(a5, tn, a4), tn, a3), tn, eDdd0() * 0.5), tn, eDd0()), tn, eD0());
                // (a NaN offset poisons the bound: as an unsigned bit pattern NaN is the largest)
                const float fd = float_above(fabs(d)), fdd = float_above(fabs(dn - d));
                if constexpr (kGroup) {  // stage V: the signed range at the checked rows (to nearest: VCIRC adds the half ulp back; a NaN stays one)
                    const int r_i = div_by<STRIDE, FP_MAX_POINTS>(i, 0.0f);
                    if (i > 0 && i == mul24(r_i, STRIDE) && r_i < rows) {
                        uint32_t* w = (uint32_t*)&s_grp[r_i].pad;
                        atomicMin(w, f32_ordered((float)d)); atomicMax(w + 1, f32_ordered((float)d));
                    }
                }
                dm = __float_as_uint(fd) > __float_as_uint(dm) ? fd : dm;
                ddm = __float_as_uint(fdd) > __float_as_uint(ddm) ? fdd : ddm;
            }
            if (d_nan) dm = ddm = __builtin_nanf("");  // a NaN sample: its own profile is NaN everywhere -> every pair passes
            s_fan_d[mul24(it, hp_max) + i] = FanType<kSlim>::above(dm);
            s_fan_dd[mul24(it, hp_max) + i] = i + 1 < np_i ? FanType<kSlim>::above(ddm) : (fan_t)0.0f;
        }
    }
    // [/section FAN]
    // [section CIRCLES]
    // ---- ranges -> circles: every reference point of the row lies within  v_max * (half the range)  of the line's point at
    // the middle of the range (v_max >= |P'(s)| everywhere); + ego reach + the largest lateral offset.  One test per
    // (row, obstacle) item then prunes the item for every profile of every slice at once.
    if (n_obs > 0 && (!kCut || (wave_s * kWave <= kThreads - 1 - nd && wave_s * kWave + kWave - 1 >= kThreads - nd - rows)) && kThreads - 1 - nd - tid >= 0 &&
        kThreads - 1 - nd - tid < rows) {  // (the threads next to the lat coefficients' first)
        const int r = kThreads - 1 - nd - tid;
        const uint4 bx = s_box[r];
        const double knot0 = s_knots[0], knot_last = s_knots[nx - 1];  // (fresh reads: the prologue's copies need not live this long)
        const float lo_f = f32_from_ordered(bx.x), hi_f = f32_from_ordered(bx.y);
        const double v_max = (double)__uint_as_float((uint32_t)s_cnt[5]), d_all = (double)__uint_as_float((uint32_t)s_cnt[6]);
        // empty row (no valid pose): radius -1 rejects every obstacle; an infinite range or a NaN bound keeps every obstacle
        double rad = -1.0, cx = sp.coef[w0], cy = sp.coef[4 * ld + w0];  // a knot: fallback centre of an empty row circle
        if (hi_f >= lo_f) {
            // the ends were rounded to nearest fp32: half an ulp each, covered by slack; points off the spline do not exist
            const double slack = ((double)fabsf(lo_f) + (double)fabsf(hi_f)) * 1.2e-7 + 1e-6;
            double s_lo = knot0 + (double)lo_f - slack, s_hi = knot0 + (double)hi_f + slack;
            s_lo = fmax(s_lo, knot0); s_hi = fmin(s_hi, knot_last);
            if (!(s_hi >= s_lo)) s_hi = s_lo = fmin(fmax(knot0 + (double)lo_f, knot0), knot_last);  // (a range that only grazes the end)
            double s_mid = 0.5 * (s_lo + s_hi);
            if (!(s_mid < knot_last)) s_mid = knot0 + 0.5 * (knot_last - knot0);  // infinite range: any centre will do
            const int seg = lut_segment(s_knots, s_lut, nx, s_mid, s_k[0], s_k[1], n_buckets);
            double tx, ty;
            frame_at(seg, s_mid - s_knots[seg], cx, cy, tx, ty);
            rad = (v_max * (0.5 * (s_hi - s_lo)) * (1.0 + 1e-9) + s_k[4] + d_all) * (1.0 + 1e-9) + 1e-6;
            if (!(hi_f <= 3.0e38f) || !(lo_f >= -3.0e38f)) rad = __builtin_inf();
            // (coefficient window: v_max bounds |P'| over the window's segments only - a range that leaves them keeps every obstacle)
            if (windowed && (!(s_lo >= s_knots[w0]) || !(s_hi <= s_knots[w0 + wcap < nx - 1 ? w0 + wcap : nx - 1]))) rad = __builtin_inf();
        }
        // (field by field, never the whole record: with stage S the fourth word of row 0, s_grp[0].pad, holds S's squared threshold -
        // written once per ego beside s_k - and a store of the whole ObsDim here would wipe it)
        static_assert(sizeof(ObsDim) == 4 * sizeof(double) && offsetof(ObsDim, pad) == 3 * sizeof(double), "s_grp[0].pad is the record's fourth word (stage S's threshold)");
        s_grp[r].hl = cx;
        s_grp[r].hw = cy;
        s_grp[r].r = rad;
    }
    // [/section CIRCLES]
    // [section GLUE]
    __syncthreads();  // the final assembly reads the sums (with no obstacles there is no other barrier in between)
    FP_STAMP(4);

    // ---------------------------------------------------------------- collision
    // Once per ego:   G  lane = (row, obstacle) item against the circle that encloses the row's reference points of ALL lon
    //                    profiles of ALL slices of this workgroup (+ ego reach + the largest lateral offset)     -> s_items
    // Per lon profile (one wavefront each, no workgroup barrier - see WALK below):
    //                 frames, prep  the profile's reference-line frames and fan half-widths       -> the wavefront's s_frames, s_wfat
    //                 B  lane = surviving item: fattened circle around the reference point + separating axes
    //                    n_k and t_k of the lateral fan                                            -> the wavefront's s_hits
    //                 N  lane = (hit, lateral sample): exact circle + 4-axis separating-axis test -> s_collmask
    // The time horizon T moves a profile's first seconds only a little (the end speed spreads them by tens of metres), so one
    // group test per ego keeps about as few items as one per slice would - at a seventh of the work.
    // The item list is appended with one LDS atomic per wavefront (ballot + popcount); its counter only ever grows, a chunk works
    // on [base, counter) and every thread tracks the base itself, so nothing is reset between chunks.  Capacity: the item list is
    // filled optimistically by the whole table; if the survivors do not fit (rare) the table is cut into chunks of kItemCap items
    // and the profiles are walked once per chunk.  A wavefront's hit list holds one B round (kWave items): it cannot overflow.
#if defined(FP_ABL_NO_COLL)
    const bool collide = false;
#else
    const bool collide = n_obs > 0 && hp > 0;
#endif
    if (collide) {
#if defined(FP_ABL_NO_GBN)   // timing ablations (tools/variants.sh): results are wrong, only the clock is read
        const int n_items = 0;
#else
        const int n_items = rows * n_obs;
#endif
        const float inv_nobs = 1.0f / (float)n_obs, inv_nvf = 1.0f / (float)nv, inv_ndf = 1.0f / (float)nd;
        // items of a chunk of the redo: at most kItemCap, so that its survivors always fit; kCut instances: whole rows (see G)
        constexpr int kChunk = kCut ? kItemCap / (NOBS > 0 ? NOBS : 1) * NOBS : kItemCap;
        static_assert(kChunk > 0 && (!kCut || NOBS <= kThreads), "a chunk of the redo and a pass of the workgroup hold at least one row");
        int chunk = n_items;
        for (int i0 = 0; i0 < n_items;) {
            // ---- G (once per ego and item chunk): the poses come straight from the scene table (L2 for all but the first ego of a
            // scene), kPoseFlight reads in flight per lane.  x = NaN / valid = 0: no state at this step (state_at_time -> None).
            // A survivor's pose goes to the list with its orientation still an angle.
    // [/section GLUE]
    // [section VCIRC]
            // ---- V, first half (once per ego and item chunk): one circle per (end speed iv, checked row r) that encloses the ego CENTRES of
            // the whole end-speed GROUP at pose k = r stride - the lon profiles (it, iv) of every slice `it` of this workgroup, times every
            // lateral sample.  VTEST (behind SINCOS) then tests each survivor of G against the nv circles of its row: a circle that lies
            // within S's sure-hit distance `thr` of an obstacle's box ends the n_it profiles of the group before any frame of theirs.
            // The horizon T moves a profile's first seconds by centimetres, the end speed by metres: the group is the tight unit.
            //   Centre of candidate (it, iv, id), as N computes it:  C = P(s) + d n(s),  s = s_it(t_k),  d = d_{it,id}(t_k),  n = (-ty, tx).
            //   [s_lo, s_hi]: range of the n_it values s - the expression FRAMES evaluates, operand for operand - with middle s_m and
            //   half width hs;  [d_lo, d_hi]: range of d over the slices and the two EXTREME lateral samples (d is affine in its end offset
            //   for a fixed horizon, see FAN), middle d_m, half width hd - the same for every end speed, so FAN, which evaluates those
            //   offsets anyway, leaves it once per ego and row in s_grp[r].pad.  Circle centre  C0 = P(s_m) + d_m n(s_m).
            //   C - C0 = (P(s) - P(s_m)) + (d - d_m) n(s) + d_m (n(s) - n(s_m)), hence
            //   |C - C0| <= v_max hs + hd + |d_m| |n(s) - n(s_m)|          (v_max >= |P'| everywhere, VBOUND)
            //   |n(s) - n(s_m)| = |T(s) - T(s_m)| <= |P'(s) - P'(s_m)| / min(|P'(s)|, |P'(s_m)|) <= A2 hs / (g - A2 hs)
            //   with T = P' / |P'|, A2 >= |P''| everywhere (VBOUND; P' is continuous across knots), g = |P'(s_m)|: |u/|u| - v/|v|| <=
            //   2 |u - v| / (|u| + |v|) for any two vectors, and |P'(s)| >= g - A2 hs.  A group whose g - A2 hs is not > 0 stays silent.
            // Rounding: the middle samples' computed d can leave [d_lo, d_hi] by ~1e-15 m, FAN's fp32 ends are widened by their half ulp
            // here, the frames are good to ~1e-12 m, v_max, A2 and the fp32 reciprocal of g - A2 hs are rounded up; the factors 1 + 1e-9 and the 1e-6 m below cover it as they do in CIRCLES, and thr carries S's own 1e-6.
            // The row must be a pose of EVERY profile of the group: k < pose_limit (final_time_step, the table's rows) and k < the
            // smallest M of the group, which must be >= 2 (a profile with M < 2 is never walked and must not be marked).  Every comparison
            // fails on a NaN (a NaN sample, state, coefficient or size): the word stays -1 and VTEST is silent.  (No instance with a coefficient
            // window has the stage - see kGroup; one that gets it must keep a range that leaves the window silent, as CIRCLES does.)
            if constexpr (kGroup) {
                const int n_circ = mul24(nv, rows);
                if (wave_s * kWave < n_circ) {
                    const int ends = s_cnt[1];
                    const float inv_rows_v = 1.0f / (float)(rows > 0 ? rows : 1);
                    // (the opaque copies of tid keep the lanes' addresses INSIDE the chunk loop, as in G: hoisted out of it they live through
                    // the walk and spill four VGPRs of the four-per-CU instance)
                    int tv = tid;
                    asm volatile("" : "+v"(tv));
                    for (int e = tv; e < n_circ; e += kThreads) {
                        const int iv = div_small(e, inv_rows_v), r = e - mul24(iv, rows);
                        const int k = mul24(r, stride);
                        const double t = (double)k * tick;
                        double s_lo = __builtin_inf(), s_hi = -__builtin_inf();
                        int m_min = 0x7FFFFFFF;
                        bool ok = (ends >> 16) == 0 && k < pose_limit;
#pragma unroll 1
                        for (int it = it_lo; it < it_hi; ++it) {
                            const int qg = mul24(it, nv) + iv;
                            const int Mq = s_lon_meta[qg].x;
                            m_min = Mq < m_min ? Mq : m_min;
                            const double a3 = s_qlon[2 * qg], a4 = s_qlon[2 * qg + 1];
                            const double s = fma(fma(fma(fma(a4, t, a3), t, eSdd0() * 0.5), t, eSd0()), t, eS0());
                            ok = ok && s == s;  // (fmin / fmax drop a NaN)
                            s_lo = vmin_f64(s_lo, s); s_hi = vmax_f64(s_hi, s);
                        }
                        // the lateral range of the row: FAN's two words (rounded to nearest fp32: half an ulp each, covered by the slack)
                        double d_lo = eD0(), d_hi = d_lo;
                        if (r > 0) {
                            const uint2 w = *(const uint2*)&s_grp[r].pad;
                            const float lo_f = f32_from_ordered(w.x), hi_f = f32_from_ordered(w.y);
                            const double slack = ((double)fabsf(lo_f) + (double)fabsf(hi_f)) * 1.2e-7 + 1e-9;
                            d_lo = (double)lo_f - slack; d_hi = (double)hi_f + slack;
                        }
                        ok = ok && d_hi >= d_lo && d_hi - d_lo < 1e30;  // (an empty or a NaN range fails)
                        ok = ok && m_min >= 2 && k < m_min;
                        // (the ranges go through the circle's own record and the frame is a second pass of the same lane over it: held in
                        // registers across the frame's coefficient reads they spill four VGPRs of the four-per-CU instance)
                        const double s_m = 0.5 * (s_lo + s_hi), d_m = 0.5 * (d_lo + d_hi);
                        double* o = s_vcirc + 4 * (mul24(iv, rows_max) + r);
                        o[0] = s_m; o[1] = ok ? fmax(s_hi - s_m, s_m - s_lo) : -1.0; o[2] = d_m; o[3] = fmax(d_hi - d_m, d_m - d_lo);
                    }
                    wave_lds_sync();
                    asm volatile("" : "+v"(tv));
                    for (int e = tv; e < n_circ; e += kThreads) {
                        const int iv = div_small(e, inv_rows_v), r = e - mul24(iv, rows);
                        double* o = s_vcirc + 4 * (mul24(iv, rows_max) + r);
                        const double s_m = o[0], hs = o[1];
                        double cx = 0.0, cy = 0.0, t2 = -1.0;
                        if (hs >= 0.0) {
                            const int seg = s_cnt[4] == 0 ? lut_segment_step(s_knots, s_lut, nx, s_m, s_k[0], s_k[1], n_buckets)
                                                          : lut_segment(s_knots, s_lut, nx, s_m, s_k[0], s_k[1], n_buckets);
                            {
                                const double u = s_m - s_knots[seg];
                                const double* c = sp.coef + seg;
                                // (spline_frame's expressions; the derivative's length g is needed beside the unit tangent)
                                const double gx = fma(fma(3.0 * c[3 * ld], u, 2.0 * c[2 * ld]), u, c[ld]), gy = fma(fma(3.0 * c[7 * ld], u, 2.0 * c[6 * ld]), u, c[5 * ld]);
                                const double g2 = fma(gx, gx, gy * gy), inv = rsqrt_nr(g2);
                                const double v_max = (double)__uint_as_float((uint32_t)s_cnt[5]), A2 = (double)__uint_as_float(s_vword[0]);
                                const double g = g2 * inv * (1.0 - 1e-9);
                                const double bend = A2 * hs * (1.0 + 1e-9), m = g - bend;
                                const double d_m = o[2], hd = o[3];
                                // (1 / m from above in fp32, as PREP's sigma: v_rcp_f32 is good to 1 ulp, the factor covers it and the rounding of m)
                                const double turn = bend * (double)(__builtin_amdgcn_rcpf((float)m) * (1.0f + 4e-6f));
                                const double rad = (v_max * hs * (1.0 + 1e-9) + hd + fabs(d_m) * turn) * (1.0 + 1e-9) + 1e-6;
                                const double thr = (s_k[2] < s_k[3] ? s_k[2] : s_k[3]) * (1.0 - 1e-9) - 1e-6;  // S's threshold (fmin would drop a NaN)
                                const double room = thr - rad;
                                cx = fma(-d_m, gy * inv, fma(fma(fma(c[3 * ld], u, c[2 * ld]), u, c[ld]), u, c[0]));
                                cy = fma(d_m, gx * inv, fma(fma(fma(c[7 * ld], u, c[6 * ld]), u, c[5 * ld]), u, c[4 * ld]));
                                if (m > 1e-30 && room > 0.0 && s_k[2] + s_k[3] == s_k[2] + s_k[3] && cx == cx && cy == cy) t2 = room * room;
                            }
                        }
                        o[0] = cx; o[1] = cy; o[2] = t2;
                    }
                }
            }
    // [/section VCIRC]
    // [section G]
            const int i1 = i0 + chunk < n_items ? i0 + chunk : n_items;
            if constexpr (kCut) {
                // kCut instances: a lane keeps ONE obstacle column and steps through the rows - a pass of the workgroup is kRowsPass whole
                // rows, a lane's items of one trip are kRowsPass rows apart.  One division per lane and chunk (item = pass * kThreads +
                // tid cost two per item, and a third for a survivor's code).  Pass u still covers the band of rows it covered -
                // [u kRowsPass, (u + 1) kRowsPass) against items [u kThreads, (u + 1) kThreads) - so the list stays in time order pass by
                // pass, which is what ends a blocked profile's walk early.  A chunk of the redo is whole rows (kChunk).
                // A lane without an item (the kThreads % NOBS last threads hold no column; rows behind the chunk) reads the chunk's LAST row
                // instead - a valid address, its neighbours' cache lines - and its pose is never looked at: no zeroed registers, no
                // branch around the reads.
                // (The opaque copy of tid keeps the lane's row and column INSIDE the chunk loop: hoisted out of it they would live
                // through the walk, in an instance with one VGPR to spare.)
                constexpr int kRowsPass = kThreads / NOBS;
                int tl = tid;
                asm volatile("" : "+v"(tl));
                const int r0 = div_by<NOBS, kThreads>(tl, 0.0f), j = tl - mul24(r0, NOBS);  // (j < NOBS for every thread)
                const int r_end = div_by<NOBS, ROWS * NOBS>(i1, 0.0f);  // (uniform; i0 and i1 are multiples of NOBS; 0 <= i0 < i1: r_end >= 1)
                for (int rb = div_by<NOBS, ROWS * NOBS>(i0, 0.0f); rb < r_end; rb += kPoseFlight * kRowsPass) {
                    double4 ps[kPoseFlight];
#pragma unroll
                    for (int u = 0; u < kPoseFlight; ++u) {
                        const int r = rb + u * kRowsPass + r0, r_ld = r < r_end ? r : r_end - 1;  // (r_end <= rows <= rows_stage: inside the table)
                        ps[u] = *(const double4*)(gp + ((size_t)(mul24(r_ld, STRIDE) + t_now) * NOBS + j) * 4);
                    }
#pragma unroll
                    for (int u = 0; u < kPoseFlight; ++u) {
                        const int r = rb + u * kRowsPass + r0;
                        bool keep = false;
                        if (r0 < kRowsPass && r < r_end) {
                            const int k = mul24(r, STRIDE);
                            const ObsDim g = s_grp[r];
                            const double dx = ps[u].x - g.hl, dy = ps[u].y - g.hw, R = g.r + s_dim.rad[j];
                            keep = k < pose_limit && ps[u].w != 0.0 && (ps[u].x == ps[u].x) && !(g.r < 0.0) && !(fma(dx, dx, dy * dy) > R * R);
                        }
                        const unsigned long long m = __ballot(keep);
                        if (m) {
                            const int first = __ffsll((long long)m) - 1;
                            int base = 0;
                            if (lane == first) base = atomicAdd(&s_cnt[0], __popcll(m));
                            // (the survivors in the lanes below this one: v_mbcnt counts them in two instructions - the mask (1 << lane) - 1,
                            // two ands and two popcounts were eight)
                            const int pos = __builtin_amdgcn_readlane(base, first) - item_base + lanes_below(m);
                            if (keep && pos < kItemCap) {
                                s_items[pos] = (unsigned short)(kItemShift > 0 ? (r << kItemShift) | j : mul24(r, NOBS) + j);
                                s_spose.set(pos, ps[u].x, ps[u].y, ps[u].z, 0.0);
                            }
                        }
                    }
                }
            } else {
                for (int b0 = i0; b0 < i1; b0 += kPoseFlight * kThreads) {
                    double4 ps[kPoseFlight];
                    fetch_poses(b0, ps);
#pragma unroll
                    for (int u = 0; u < kPoseFlight; ++u) {
                        const int e = b0 + u * kThreads + tid;
                        bool keep = false;
                        if (e < i1) {
                            const int r = div_by<NOBS, ROWS * NOBS>(e, inv_nobs), j = e - mul24(r, n_obs);
                            const int k = mul24(r, stride);
                            const ObsDim g = s_grp[r];
                            const double dx = ps[u].x - g.hl, dy = ps[u].y - g.hw, R = g.r + s_dim.rad[j];
                            keep = k < pose_limit && ps[u].w != 0.0 && (ps[u].x == ps[u].x) && !(g.r < 0.0) && !(fma(dx, dx, dy * dy) > R * R);
                        }
                        const unsigned long long m = __ballot(keep);
                        if (m) {
                            const int first = __ffsll((long long)m) - 1;
                            int base = 0;
                            if (lane == first) base = atomicAdd(&s_cnt[0], __popcll(m));
                            const int pos = __builtin_amdgcn_readlane(base, first) - item_base + __popcll(m & ((1ull << lane) - 1ull));
                            if (keep && pos < kItemCap) {
                                if constexpr (kItemShift > 0) {  // (taken apart again here: a survivor is rare, a register held across the ballot is not free)
                                    const int r_e = div_by<NOBS, ROWS * NOBS>(e, inv_nobs);
                                    s_items[pos] = (unsigned short)((r_e << kItemShift) | (e - mul24(r_e, n_obs)));
                                } else {
                                    s_items[pos] = (unsigned short)e;
                                }
                                s_spose.set(pos, ps[u].x, ps[u].y, ps[u].z, 0.0);
                            }
                        }
                    }
                }
            }
    // [/section G]
    // [section GLUE]
            __syncthreads();
    FP_STAMP(7);
            const int item_end = s_cnt[0];
            const int n_surv = item_end - item_base;
            item_base = item_end;
            if (tid == 0) FP_COUNT(0, n_surv);
            if (n_surv > kItemCap) {  // block-uniform: does not fit, redo [i0, ...) in chunks whose survivors always fit
                chunk = kChunk;
                __syncthreads();  // every thread has read s_cnt[0] before the redone pass adds to it again
                continue;
            }
    // [/section GLUE]
    // [section SINCOS]
            // the survivors' orientations -> (cos, sin), with shapely's snap (frenet_device.h); every item belongs to one chunk
            for (int si = tid; si < n_surv; si += kThreads) {
                double sn, cs;
                sincos_snapped(s_spose.hi[si].x, sn, cs);
                s_spose.hi[si] = make_double2(cs, sn);
    // [/section SINCOS]
    // [section VTEST]
                // ---- V, second half: the lane that snapped a survivor's orientation tests its box against the nv group circles of its row -
                // the squared point-to-box distance of the circle's centre exactly as S computes it for a fan end (same pose, same
                // half extents, same snapped (cos, sin)), against (thr - rad)^2.  dist(C0, box) <= thr - rad puts every ego centre of the
                // group within thr < rho of the box: all n_it x nd candidates of the group collide at this pose (S's argument (a)).
                // A survivor is a pose the table holds at a row below pose_limit; the circle is silent (-1) unless the row is a pose of
                // every profile of the group.  Every comparison fails on a NaN.  A passing lane fills the collision masks of the group's
                // profiles (the same words from every passing lane); the profile loop skips a full mask at its head.  No extra
                // barrier: the circles were written before G's, the masks are read behind the walk's.  With item chunks the masks accumulate.
                if constexpr (kGroup) {
                    const int item = s_items[si];
                    const int r = kItemShift > 0 ? item >> kItemShift : div_by<NOBS, ROWS * NOBS>(item, 1.0f / (float)n_obs);
                    const int j = kItemShift > 0 ? item & ((1 << kItemShift) - 1) : item - mul24(r, n_obs);
                    const double2 oxy = s_spose.lo[si], ohw = s_dim.hlw[j];
                    const unsigned long long full_v = nd >= 64 ? ~0ull : ((1ull << nd) - 1ull);
#pragma unroll 1
                    for (int iv = 0; iv < nv; ++iv) {
                        const double* c = s_vcirc + 4 * (mul24(iv, rows_max) + r);
                        const double dx = c[0] - oxy.x, dy = c[1] - oxy.y;
                        const double a = fabs(fma(dx, cs, dy * sn)) - ohw.x, bq = fabs(fma(dy, cs, -dx * sn)) - ohw.y;
                        const double qx = fmax(a, 0.0), qy = fmax(bq, 0.0);
                        const double fin = a + bq;
                        if (fma(qx, qx, qy * qy) <= c[2] && fin == fin) {
#if defined(FP_COUNTERS)  // (slot 19: one bit per end speed V ended, whichever chunk and however many lanes - slot 16 reports their number)
                            atomicOr((unsigned int*)&s_dbg[19], 1u << (iv & 31));
#endif
                            for (int it = it_lo; it < it_hi; ++it) {
                                const int qg = mul24(it, nv) + iv;
                                s_collmask[2 * qg] = (uint32_t)full_v; s_collmask[2 * qg + 1] = (uint32_t)(full_v >> 32);
                            }
                        }
                    }
                }
            }
    // [/section VTEST]
    // [section WSETUP]
            // (the walk's barrier below orders these writes before stage B reads them)
            // No survivor (block-uniform: empty surroundings, obstacles out of reach): nothing can collide, the walk is skipped.
            // (Skipping only the rows without a survivor was tried: a lane that skips its point saves nothing while its wavefront's
            // other lanes work, and the bookkeeping cost 3 % on dense scenes.)
            // ---- WALK: every wavefront takes lon profiles (slice, end speed) round-robin and handles each one on its own, in four
            // wave-local steps with no workgroup barrier between them (a wavefront's LDS accesses execute in program order):
            //   frames   lane = trajectory point inside the collision horizon: reference-line frame -> the wavefront's frame table
            //   prep     lane = checked pose row: the fan's half-width along the reference normal (fp32, rounded outwards)
            //   B        lane = surviving item, in list (= time) order, 64 at a time: fattened circle + separating axes n_k, t_k;
            //            the passing items are compacted into the wavefront's hit list (ballot + popcount, no atomics)
            //   N        lane = (hit, lateral sample), floor(64 / nd) hits per round: exact circle + 4-axis separating-axis test.
            // The collision state of the profile's nd candidates is ONE wave-uniform bit mask: a lane skips candidates that have
            // collided, and the walk of a profile ENDS when all nd have (later items cannot change anything) - items are in time
            // order, so a blocked profile ends after its first hits instead of testing every pose of the horizon.
            if (n_surv > 0) {
                __syncthreads();  // the survivors' (cos, sin), the item list and the lateral bounds are visible to every wavefront
                const SplitTab<Frame> wfr = s_frames.at(mul24(wave, hp_max));
                float* wwf = s_wfat + mul24(wave, rows_max > 0 ? rows_max : 1);
                hit_t* wh = s_hits + wave * kWave;
                constexpr int kHpwC = ND > 0 ? kWave / ND : 1;
                const int hpw = kShape ? kHpwC : kWave / nd;  // hits per narrow-phase round
                const int hh_l = div_by<ND, kWave>(lane, inv_ndf), id_l = lane - mul24(hh_l, nd);
                const unsigned long long full = nd >= 64 ? ~0ull : ((1ull << nd) - 1ull);
                const unsigned long long lt_mask = (1ull << lane) - 1ull;
                const int n_prof = mul24(n_it, nv);
                const float inv_stride = 1.0f / (float)stride;
                // wave-uniform, in scalar registers across the profile loop: whether the segment hint is exact to one step (s_cnt[4], see
                // the LUT build), and prep's fp32 ego sizes (the bits of float_above(s_k[4]), (s_k[2]), (s_k[3]))
                // (the builtin would not do: the compiler knows these values to be uniform, drops it and keeps them in VECTOR registers
                // through the whole walk - this instance has none to spare.  The compiler's hazard recogniser does not look into an asm:
                // of gfx950's VALU-writes-SGPR hazards (VMEM reading it as an address: 5 wait states; v_readlane / v_writelane taking it as
                // the lane select: 4) neither use exists - the four values only ever feed s_cmp and the constant operand of v_min_f32 /
                // v_mul_f32 / v_add_f32, which need none - and the first reader is behind the profile loop's header, LDS waits included.
                // Whoever gives them another use pads it.  tools/resource_usage.py after this change: the four-per-CU instances 63 VGPRs
                // (shaped) / 64 (run-time shape), 62 - 64 with the appended search, 0 spilled in all 25.)
                auto in_sgpr = [](int v) { int r; asm volatile("v_readfirstlane_b32 %0, %1" : "=s"(r) : "v"(v)); return r; };
                const int lut_crowded = kShape ? in_sgpr(s_cnt[4]) : 1;  // (run-time shape: the loops, see FRAMES)
                // (shaped instances only: the run-time-shape ones have no scalar register left either - held there, the four cost more
                // lane operations on spilled SGPRs than they save - and convert per profile as before)
                const float r_ego_s = kShape ? __int_as_float(in_sgpr(__float_as_int(float_above(s_k[4])))) : 0.0f;
                const float hl_s = kShape ? __int_as_float(in_sgpr(__float_as_int(float_above(s_k[2])))) : 0.0f;
                const float hw_s = kShape ? __int_as_float(in_sgpr(__float_as_int(float_above(s_k[3])))) : 0.0f;
                // the last pose row a lane can hold: a profile with more points than that has no hit on its own last point
                const int k_last = kShape ? mul24(rows - 1, stride) : 0;
                // Profiles are dealt to the wavefronts round-robin (wave w takes w, w + 8, ...: a mix of end speeds each); the first
                // wavefront to run out waits ~3 of the walk's 24 us for the last one.  Dealing them from a shared LDS counter instead was
                // built and measured: no difference (153.1 / 154.4 against 155.1 / 154.1 us per step in same-box runs) - the waiting
                // wavefronts cost no issue slots and the CU's other workgroups fill them.  (Its C++ spelling, `if (lane == 0) t =
                // atomicAdd(...)` + readfirstlane inside a loop whose only exit is a break, was restructured by the compiler so that lanes
                // 1..63 spun on their own - a hang; it took an inline-asm block with EXEC narrowed by hand.)  The loop below has a
                // wave-uniform scalar trip count and no divergent branch around a cross-lane operation.
    // [/section WSETUP]
    // [section PQ]
                for (int pq = __builtin_amdgcn_readfirstlane(wave); pq < n_prof; pq += kWaves) {
    // [section PQDEC]
                    const int itl = div_by<NV, NT * NV>(pq, inv_nvf), iv = pq - mul24(itl, nv);
                    const int it = it_lo + itl, qg = mul24(it, nv) + iv;
    // [/section PQDEC]
    // [section PQFETCH]
                    // candidates of this profile that collided in an earlier item chunk (crowded scenes only; else 0) - or, stage V, whose
                    // whole end-speed group VTEST ended: the mask is full and the profile is skipped here, on a scalar test, before its
                    // frames.  (Profiles are dealt pq = wave, wave + kWaves, ... with iv = pq mod nv: an ended end speed thins every
                    // wavefront's share alike.)
                    auto coll_so_far = [&]() {
                        return ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)s_collmask[2 * qg + 1]) << 32) |
                               (uint32_t)__builtin_amdgcn_readfirstlane((int)s_collmask[2 * qg]);
                    };
                    unsigned long long coll = 0;
                    if constexpr (kGroup) {
                        coll = coll_so_far();
                        if (coll == full) continue;
                        if (lane == 0) FP_COUNT(17, 1);
                    }
                    const int M = __builtin_amdgcn_readfirstlane(s_lon_meta[qg].x);  // (M <= N; wave-uniform -> scalar registers)
                    // a trajectory of fewer than two points has no heading: no pair (M == 1 is the assembly's business)
                    if (M < 2) continue;
                    const int n_pts = __builtin_amdgcn_readfirstlane(s_nslice[it]);
                    const int np = hp < n_pts ? hp : n_pts;
                    const int npm = np < M ? np : M;
                    const double a3 = s_qlon[2 * qg], a4 = s_qlon[2 * qg + 1];
    // [/section PQFETCH]
    // [section FRAMES]
                    for (int i = lane; i < npm; i += kWave) {
                        const double t = (double)i * tick;
                        const double s = fma(fma(fma(fma(a4, t, a3), t, eSdd0() * 0.5), t, eSd0()), t, eS0());
                        int seg;
                        if (kShape && lut_crowded == 0) {  // (the run-time-shape instances keep the loops alone: both lookups in one instance make it larger than it was)
                            seg = lut_segment_step(s_knots, s_lut, nx, s, s_k[0], s_k[1], n_buckets);
                        } else {
    // [section LUTWALK]
                            seg = lut_segment(s_knots, s_lut, nx, s, s_k[0], s_k[1], n_buckets);
    // [/section LUTWALK]
                        }
                        Frame fr;
                        frame_at(seg, s - s_knots[seg], fr.px, fr.py, fr.tx, fr.ty);
                        wfr.set(i, fr.px, fr.py, fr.tx, fr.ty);
                    }
    // [/section FRAMES]
    // [section PQPTR]
                    wave_lds_sync();
                    const fan_t* dm = s_fan_d + mul24(it, hp_max);
                    const fan_t* ddm = s_fan_dd + mul24(it, hp_max);
    // [/section PQPTR]
    // [section PQFETCH]
                    // (the mask of the earlier item chunks is read here by the instances with stage S, which may end the profile at once -
                    // those with stage V have it from the loop's head - and by the others behind prep, as before)
#if defined(FP_ABL_NO_BN)
                    const int n_walk = 0;
#else
                    const int n_walk = n_surv;
#endif
                    // ---- S: a SURE hit ends a blocked profile before prep, B and N.  lane = surviving item, in list (= time) order, 64 at a
                    // time.  Three in four lon profiles of the headline batches are blocked - all nd lateral samples collide - and paid
                    // prep, a B round and an N round (two quintics, two Frenet-to-Cartesian conversions, a heading and a 4-axis test per
                    // (hit, lateral sample)) to learn it.  The proof here needs no heading, no quintic and no separating axis:
                    //   (a) A box of half extents (hl, hw) contains, at ANY heading, the disk of radius rho = min(hl, hw) about its centre.
                    //   (b) At pose k every one of the profile's nd ego centres is P_k + d n_k with |d| <= dm[k] (the fan bound B reads: the
                    //       largest |d| over the lateral samples, rounded UP to fp32 / fp16, which only lengthens the segment), n_k = (-ty, tx):
                    //       they lie on the segment between E- = P_k - dm n_k and E+ = P_k + dm n_k.
                    //   (c) The distance from a point to a convex set - the obstacle's box - is a convex function of the point, so on a
                    //       segment it is largest at an end.
                    //   So if dist(E-, box) and dist(E+, box) are both <= thr = rho (1 - 1e-9) - 1e-6, then every centre of the fan is closer
                    //   than rho to the box: its disk, hence its ego box, whatever its heading, meets the obstacle's box - the profile's nd
                    //   candidates all collide at pose k, which is what N would find one pair at a time (its circle test holds a fortiori:
                    //   the centres are closer than rho + the obstacle's radius).  coll = full, and the profile goes to PQEND as it does
                    //   when N fills the mask.
                    // |n_k| = 1 up to the frame's own rounding (spline_frame normalises the tangent: a few ulp), and N builds its centres from
                    // the same frame.  What the 1e-6 m absorbs: the reference's and the kernel's centres differ by less than 1e-12 m; the
                    // rounding of this stage's own dozen operations on coordinates of 1e3..1e5 m (below 1e-10 m); the relative 1e-9 is for
                    // rho's.  The obstacle's (cos, sin) are the snapped ones N uses (SINCOS), its box the one N tests.
                    // Every comparison fails on a NaN: the squared distances (frame, fan - d_nan -, pose) and the sum `fin` (sizes: max(NaN, 0)
                    // would be 0) leave `sure` false, thr <= 0 or NaN is -1 in LDS.  Poses k >= M are never judged (their frames are stale).
                    // A profile S does not end takes prep, B and N exactly as before.  The trip count is wave-uniform (scalar n_walk, coll)
                    // and the ballot stands under no divergent branch (see WSETUP on the hang).
                    if constexpr (kSure) {
                        if constexpr (!kGroup) coll = coll_so_far();
    // [/section PQFETCH]
    // [section ROUNDS]
                        for (int c0 = 0; c0 < n_walk && coll != full; c0 += kWave) {
                            const int si = c0 + lane;
                            bool sure = false;
#if defined(FP_COUNTERS)
                            bool first_end = false;  // (the E- end alone: a round in which no lane passes it skips the second end's instructions)
#endif
    // [/section ROUNDS]
    // [section S]
                            if (si < n_walk) {
                                const int item = s_items[si];
                                const int r = kItemShift > 0 ? item >> kItemShift : div_by<NOBS, ROWS * NOBS>(item, 1.0f / (float)n_obs);
                                const int j = kItemShift > 0 ? item & ((1 << kItemShift) - 1) : item - mul24(r, n_obs);
                                const int k = mul24(r, stride);
                                const ObsPose op = s_spose.get(si);
                                const double2 ohw = s_dim.hlw[j];
                                const Frame fr = wfr.get(k);  // (stale beyond the profile's M: the test below excludes those poses)
                                const double dmk = (double)dm[k], thr2 = s_grp[0].pad;
                                const double ex = dmk * fr.ty, ey = dmk * fr.tx;  // E+- = (px -+ ex, py +- ey)
                                const double dxp = (fr.px - ex) - op.x, dyp = (fr.py + ey) - op.y;
                                const double dxm = (fr.px + ex) - op.x, dym = (fr.py - ey) - op.y;
                                // in the obstacle's axes: u along its length, w along its width; q = the part of each outside the box
                                const double ap = fabs(fma(dxp, op.c, dyp * op.s)) - ohw.x, bp = fabs(fma(dyp, op.c, -dxp * op.s)) - ohw.y;
                                const double am = fabs(fma(dxm, op.c, dym * op.s)) - ohw.x, bm = fabs(fma(dym, op.c, -dxm * op.s)) - ohw.y;
                                const double qxp = fmax(ap, 0.0), qyp = fmax(bp, 0.0), qxm = fmax(am, 0.0), qym = fmax(bm, 0.0);
                                const double fin = ap + bp;  // (NaN if any input is: the frame, the fan and the pose enter both ends)
                                sure = k < M && fma(qxp, qxp, qyp * qyp) <= thr2 && fma(qxm, qxm, qym * qym) <= thr2 && fin == fin;
#if defined(FP_COUNTERS)
                                first_end = k < M && fma(qxp, qxp, qyp * qyp) <= thr2;
#endif
                            }
    // [/section S]
    // [section ROUNDS]
                            if (lane == 0) FP_COUNT(4, 1);
#if defined(FP_COUNTERS)
                            if (!__ballot(first_end) && lane == 0) FP_COUNT(18, 1);
#endif
                            if (__ballot(sure)) {
                                coll = full;
                                if (lane == 0) FP_COUNT(8, 1);
                            }
                        }
    // [/section ROUNDS]
                    }
                    // ---- prep: wfat = lateral half-width of the whole fan along the reference normal n_k, per checked pose row r of this
                    // profile: every ego centre is P_k + d n_k with |d| <= dm[k];  the ego box, whose heading deviates from the
                    // reference tangent by alpha, reaches hw cos(alpha) + hl |sin(alpha)| <= min(r_ego, hw + hl sigma) along n_k, where
                    // sigma >= |sin(alpha)| for every lateral sample follows from the heading vector
                    //   h = (P_{k+1} - P_k) + d_{k+1} n_{k+1} - d_k n_k:  |h.n_k| <= |dP.n_k| + max|d_{k+1} - d_k| + max|d_{k+1}| |1 - n_{k+1}.n_k|,
                    //   |h| >= |h.t_k| >= |dP.t_k| - max|d_{k+1}| |n_{k+1}.t_k|.   n_k then serves as a (conservative) separating axis.
                    // A conservative bound, so it is computed in fp32 (the ratio is a reciprocal instead of an fp64 division).
                    {
                        const float r_ego_f = kShape ? r_ego_s : float_above(s_k[4]), hl_f = kShape ? hl_s : float_above(s_k[2]), hw_f = kShape ? hw_s : float_above(s_k[3]);
    // [section PREP]
                        // (a profile S ended - or one that an earlier chunk blocked - needs no half-widths: a scalar test)
                        if (!kSure || coll != full)
                        for (int r = lane; r < rows; r += kWave) {
                            const int k = mul24(r, stride);
                            const bool row_ok = k < n_pts && k < hp;
                            float wl = r_ego_f;
                            if (k + 1 < M && k + 1 < hp) {
                                const Frame f0 = wfr.get(k), f1 = wfr.get(k + 1);
                                const double dpx = f1.px - f0.px, dpy = f1.py - f0.py;
                                const double a_n = fma(dpy, f0.tx, -dpx * f0.ty);     // dP . n_k,  n_k = (-ty, tx)
                                const double a_t = fma(dpx, f0.tx, dpy * f0.ty);      // dP . t_k
                                const double nn = fma(f1.tx, f0.tx, f1.ty * f0.ty);   // n_{k+1} . n_k
                                const double nt_ = fma(f1.tx, f0.ty, -f1.ty * f0.tx); // n_{k+1} . t_k
                                const double dm1 = (double)dm[k + 1];
                                const float num = (float)(fabs(a_n) + (double)ddm[k] + dm1 * fabs(1.0 - nn));
                                const float den = (float)(fabs(a_t) - dm1 * fabs(nt_));
                                if (den > 1e-30f) {  // v_rcp_f32: 1 ulp; the factor covers it and the two roundings to nearest
                                    const float sigma = vmin_f32(1.0f, num * __builtin_amdgcn_rcpf(den) * (1.0f + 4e-6f) + 1e-9f);
                                    wl = vmin_f32(r_ego_f, (hl_f * sigma + hw_f) * (1.0f + 1e-6f));
                                }
                            }
                            wwf[r] = row_ok ? ((float)dm[k] + wl) * (1.0f + 1e-6f) + 1e-9f : 0.0f;
                        }
    // [/section PREP]
    // [section PQFETCH]
                    }
                    wave_lds_sync();
                    if constexpr (!kSure) coll = coll_so_far();
                    const double* qlat = s_qlat + 3 * mul24(it, nd);
    // [/section PQFETCH]
    // [section ROUNDB]
                    for (int c0 = 0; c0 < n_walk && coll != full; c0 += kWave) {
                        const int si = c0 + lane;
                        bool pass = false;
                        uint32_t code = 0;
    // [/section ROUNDB]
    // [section B]
                        if (si < n_walk) {
                            const int item = s_items[si];
                            const int r = kItemShift > 0 ? item >> kItemShift : div_by<NOBS, ROWS * NOBS>(item, inv_nobs);
                            const int j = kItemShift > 0 ? item & ((1 << kItemShift) - 1) : item - mul24(r, n_obs);
                            const int k = mul24(r, stride);
                            const ObsPose op = s_spose.get(si);
                            const ObsDim od = s_dim.get(j);
                            const Frame fr = wfr.get(k);  // (stale beyond the profile's M: the test below excludes those poses)
                            const double r_ego_b = s_k[4];
                            const double fat = (r_ego_b + od.r + (double)dm[k]) * (1.0 + 1e-12);
                            const double dx = op.x - fr.px, dy = op.y - fr.py;
                            // (1) circle around the reference point; (2) separating axis n_k: lateral offset of the obstacle centre
                            // vs the fan half-width + the obstacle's own reach along n_k; (3) separating axis t_k: every ego centre
                            // of the fan lies ON the normal line, so along t_k the fan reaches no further than the ego box's
                            // half-diagonal.  A NaN pose passes all three (-> "collision").
                            const double w = fma(dy, fr.tx, -dx * fr.ty), u = fma(dx, fr.tx, dy * fr.ty);
                            const double a_n = fabs(fma(op.s, fr.tx, -op.c * fr.ty)), a_t = fabs(fma(op.c, fr.tx, op.s * fr.ty));
                            const double reach = fma(od.hl, a_n, od.hw * a_t), reach_t = fma(od.hl, a_t, od.hw * a_n);
                            pass = k < M && !(fma(dx, dx, dy * dy) > fat * fat) && !(fabs(w) > (double)wwf[r] + reach) &&
                                   !(fabs(u) > r_ego_b * (1.0 + 1e-12) + reach_t);
                            code = (uint32_t)k | ((uint32_t)si << 8);  // k < 128, si < 512 (slim: si < 256, 16 bits)
                        }
    // [/section B]
    // [section ROUNDB]
                        const unsigned long long m = __ballot(pass);
                        if (lane == 0) { FP_COUNT(1, 1); FP_COUNT(2, __popcll(m)); }
                        if (!m) continue;
                        const int n_hits = __popcll(m);
                        if (pass) wh[kCut ? lanes_below(m) : __popcll(m & lt_mask)] = (hit_t)code;
                        wave_lds_sync();
                        // ---- N: exact narrow phase, hpw hits x nd lateral samples per round
#if defined(FP_ABL_NO_N)
                        const int n_exact = 0;
#else
                        const int n_exact = n_hits;
#endif
    // [/section ROUNDB]
    // [section ROUNDN]
                        for (int h0 = 0; h0 < n_exact; h0 += hpw) {
                            const int h = h0 + hh_l;
                            bool hit = false;
    // [/section ROUNDN]
    // [section N]
                            if (hh_l < hpw && h < n_exact && !((coll >> id_l) & 1ull)) {
                                const uint32_t hc = wh[h];
                                const int k = hc & 0xFF, si2 = hc >> 8;
                                const int j = kItemShift > 0 ? (int)s_items[si2] & ((1 << kItemShift) - 1)
                                                             : (int)s_items[si2] - mul24(div_by<STRIDE, FP_MAX_POINTS>(k, inv_stride), n_obs);  // (table index: row * n_obs + obstacle)
                                FP_COUNT(3, 1);
                                // heading of pose k: forward difference, or the previous one for the last point (:127-129)
                                // (only a profile whose line ends inside the checked rows has such a point: the others take k without the compare and the selects)
                                int ka_ = k;
                                unsigned long long on_last = 0;  // the round's lanes that stand on their profile's last point
                                // (run-time shape: every profile takes the block - one more scalar held through the walk costs those instances more
                                // lane operations on spilled SGPRs than the block has instructions)
                                if (!kShape || M <= k_last + 1) {  // (scalar: the line ends inside the checked rows)
    // [section NLAST]
                                    asm volatile("");  // (nothing is emitted: it keeps this a wave-uniform BRANCH - without it the compiler folds the block into selects that every profile pays)
                                    on_last = __builtin_amdgcn_ballot_w64(k + 1 >= M);
                                    ka_ = (k + 1 < M) ? k : k - 1;
    // [/section NLAST]
                                }
                                const Frame f0 = wfr.get(ka_), f1 = wfr.get(ka_ + 1);
                                const double* ql = qlat + mul24(id_l, 3);
                                const double b3 = ql[0], b4 = ql[1], b5 = ql[2];
                                const double ta = (double)ka_ * tick, tb = (double)(ka_ + 1) * tick;
                                const double da = fma(fma(fma(fma(fma(b5, ta, b4), ta, b3), ta, eDdd0Half()), ta, eDd0()), ta, eD0());
                                const double db = fma(fma(fma(fma(fma(b5, tb, b4), tb, b3), tb, eDdd0Half()), tb, eDd0()), tb, eD0());
                                double xa, ya, xb, yb;
                                frenet_to_cartesian(f0.px, f0.py, f0.tx, f0.ty, da, xa, ya);
                                frenet_to_cartesian(f1.px, f1.py, f1.tx, f1.ty, db, xb, yb);
                                Obb ego;
                                step_heading(xb - xa, yb - ya, ego.c, ego.s);
                                ego.x = xa;
                                ego.y = ya;
                                if (on_last) {
    // [section NLAST]
                                    asm volatile("");
                                    const bool mine = __builtin_amdgcn_inverse_ballot_w64(on_last);
                                    ego.x = mine ? xb : xa;
                                    ego.y = mine ? yb : ya;
    // [/section NLAST]
                                }
                                ego.hl = s_k[2];
                                ego.hw = s_k[3];
                                const ObsPose op = s_spose.get(si2);
                                const ObsDim od = s_dim.get(j);
                                if (!(ego.x == ego.x) || !(ego.y == ego.y) || !(ego.c == ego.c)) {
                                    hit = true;  // polygon construction fails in the reference -> collision (:178-182)
                                } else {
                                    const double R = (s_k[4] + od.r) * (1.0 + 1e-12);
                                    const double dx = op.x - ego.x, dy = op.y - ego.y;
                                    hit = fma(dx, dx, dy * dy) <= R * R && obb_overlap(ego, Obb{op.x, op.y, op.c, op.s, od.hl, od.hw});
                                    if constexpr (POLY) {
                                        if (hit) {  // a polygon column: its box was a necessary condition, the ring decides
                                            const int nvx = ((const int32_t*)(smem + L.nvert))[j];
                                            if (nvx > 0) hit = ring_overlap(ego, Obb{op.x, op.y, op.c, op.s, od.hl, od.hw}, ring_base + (ring_col0 + j) * 2 * (size_t)bt.poly_stride, nvx, s_dim.rin[j]);
                                        }
                                    }
                                }
                                if (hit) FP_COUNT(5, 1);
                            }
    // [/section N]
    // [section ROUNDN]
                            if (lane == 0) FP_COUNT(6, 1);
                            unsigned long long hm = __ballot(hit);
                            // fold the round's hits onto the nd lateral samples (scalar arithmetic on the ballot)
                            // (kCut instances: the round's kHpwC groups of nd bits are ORed onto the first by halving - three or four
                            // scalar shift / or pairs.  The loop's test `hm != 0` of a 64-bit scalar has no scalar compare: it came out as
                            // v_mov_b64 + v_cmp_gt_u64 per trip, up to seven trips per round, which no static count weighs.  The shaped
                            // polygon instances come out seven instructions larger with it and keep the loop.)
                            if (nd >= kWave) coll |= hm;
                            else if constexpr (kCut) {
#pragma unroll
                                for (int g = 32; g >= 1; g >>= 1)
                                    if (g < kHpwC) hm |= hm >> (g * ND);
                                coll |= hm & full;
                            } else
                                for (; hm; hm >>= nd) coll |= hm & full;
                            if (coll == full) {
#if defined(FP_COUNTERS)  // when a blocked profile dies: the pose index of the last hit of the deciding round, in bins of 8 steps (slots 10..15)
                                if (lane == 0) {
                                    FP_COUNT(7, 1);
                                    const int hl = (h0 + hpw < n_exact ? h0 + hpw : n_exact) - 1;
                                    const int kd = (int)(wh[hl] & 0xFF) >> 3;
                                    FP_COUNT(10 + (kd > 5 ? 5 : kd), 1);
                                }
#endif
                                break;
                            }
                        }
                    }
    // [/section ROUNDN]
    // [section PQEND]
                    if (lane == 0) { s_collmask[2 * qg] = (uint32_t)coll; s_collmask[2 * qg + 1] = (uint32_t)(coll >> 32); }
                }
    // [/section PQEND]
    // [/section PQ]
    // [section POSTWALK]
#if defined(FP_PHASE_STAMPS)  // when the first and the last wavefront finished their profiles (columns 11, 12): the walk's imbalance
                if (lane == 0) { atomicMin(&s_walk_t[0], (unsigned int)(wall_clock64() - t_begin)); atomicMax(&s_walk_t[1], (unsigned int)(wall_clock64() - t_begin)); }
#endif
                // every wavefront's collision masks are visible to the assembly (and every wavefront is done with this chunk's item
                // list before G overwrites it: crowded scenes walk the profiles again over the next chunk's survivors)
                __syncthreads();
#if defined(FP_PHASE_STAMPS)
                if (threadIdx.x == 0 && ka.r.best_traj && (perm || blockIdx.x % nsplit == 0)) {
                    double* row = ka.r.best_traj + ((size_t)(perm ? perm[blockIdx.x] : blockIdx.x / nsplit) * FP_ARR_COUNT + 15) * (ka.r.traj_stride > 0 ? ka.r.traj_stride : FP_DEFAULT_STRIDE) + 112;
                    row[11] = (double)s_walk_t[0]; row[12] = (double)s_walk_t[1];
                }
#endif
            }
            i0 = i1;
        }
    }
    // [/section POSTWALK]
    // [section WEXIT]
    // ---- W: a WHOLE ego has its answer when every collision mask of the workgroup's slices is full - VTEST ended all nv end-speed groups,
    // or S and N filled what it left.  The assembly flags every candidate of these slices as colliding whatever else it finds, none can
    // reach the argmin: this workgroup's answer is "none", Best{., -1}.  Each wavefront reads the n_it nv mask words for itself, one
    // lane per lon profile (contiguous: qg = it_lo nv + pq), behind the last walk's closing barrier - nothing stores a mask after it,
    // so the verdict is the same in every wavefront, the branches on it are block-uniform and no barrier is added.  An ego with no
    // survivor of G, or a profile V never marks (M < 2) and the walk never enters, has an open mask and goes the way it went.
    bool whole = false;
    if constexpr (kWhole) {
        if (collide) {
            const unsigned long long full_w = nd >= 64 ? ~0ull : ((1ull << nd) - 1ull);
            const int n_prof_w = mul24(n_it, nv);
            bool open = false;  // some profile of the slices has a candidate that is not known to collide
            for (int e0 = 0; e0 < n_prof_w; e0 += kWave) {
                const int e = e0 + lane;
                bool lane_open = false;
                if (e < n_prof_w) {
                    const uint2 m = ((const uint2*)s_collmask)[mul24(it_lo, nv) + e];
                    lane_open = m.x != (uint32_t)full_w || m.y != (uint32_t)(full_w >> 32);
                }
                open = open || __ballot(lane_open) != 0ull;
            }
            whole = !open;
#if defined(FP_COUNTERS)
            if (tid == 0 && whole) { FP_COUNT(20, 1); FP_COUNT(21, !ka.r.cost_tbl && !ka.r.flag_tbl); }
#endif
        }
    }
    // [/section WEXIT]
    // [section POSTWALK]

    FP_STAMP(8);
#if defined(FP_COUNTERS)
    __syncthreads();
    if (tid < 16 && ka.r.best_traj) ka.r.best_traj[((size_t)b * FP_ARR_COUNT + 14) * (ka.r.traj_stride > 0 ? ka.r.traj_stride : FP_DEFAULT_STRIDE) + 112 + tid] = (double)s_dbg[tid];
    if (tid >= 16 && tid < 22 && ka.r.best_traj) ka.r.best_traj[((size_t)b * FP_ARR_COUNT + 13) * (ka.r.traj_stride > 0 ? ka.r.traj_stride : FP_DEFAULT_STRIDE) + 112 + tid - 16] = (double)(tid == 16 ? __popc((unsigned int)s_dbg[19]) : s_dbg[tid]);  // (row 13: row 14 is full; 16 = groups ended by V, counted from slot 19's bits)
#endif
    // ---------------------------------------------------------------- per-candidate assembly + argmin
    // From here on the kernel's arguments are read through `la`: for the four-per-CU instances (80 SGPRs) a view of the argument segment the
    // compiler cannot fold into the loads at the kernel's start - result pointers, cost weights and ticket buffers are then scalar loads HERE
    // instead of values carried through the walk in spilled SGPRs (each spill is a v_writelane / v_readlane pair: VALU issue slots); for
    // the other instances the same loads as before.
    int la_off = 0;
    if constexpr (OCC > 6) asm volatile("" : "+s"(la_off));
    const LatticeKernarg& la = *(const LatticeKernarg*)((const unsigned char*)__builtin_amdgcn_kernarg_segment_ptr() + la_off);
    const KernelArgs& kb = la.ka;
    const fp_params& pa = la.ka.p;
    Best mine{0.0, -1};
    const float inv_nv_a = 1.0f / (float)nv, inv_nt_a = 1.0f / (float)nt;
    // [/section POSTWALK]
    // [section WEXIT]
    // A whole-blocked ego (the verdict above) with no table requested: the assembly's only outputs would be the tables, and no
    // candidate of these slices can reach the argmin - both are skipped and RESULTS is entered with Best{., -1}, this workgroup's
    // "none" (the tail split's ticket and merge, the hand-over flags, Stats and `dur` are RESULTS' as before).  With tables the
    // assembly runs as it is - its flag words and costs are outputs - and only the argmin, which has nothing to reduce, is skipped:
    // with it goes its workgroup barrier, which orders nothing in a kWhole instance (no search workgroup reads the tables inside
    // the launch, RESULTS' thread 0 reads its own `mine`, a split ego's ticket has barriers of its own).
    // (`whole` is false wherever kWhole is.)
    const bool whole_quiet = whole && !kb.r.cost_tbl && !kb.r.flag_tbl;
    // [/section WEXIT]
    // [section ASM]
    if (!whole_quiet)
    for (int c = tid; c < C; c += kThreads) {
        // c = (id * nt + it) * nv + iv
        const int q1 = div_by<NV, ND * NV * NT>(c, inv_nv_a), iv = c - mul24(q1, nv);
        const int id = div_by<NT, ND * NT>(q1, inv_nt_a), it = q1 - mul24(id, nt);
        if (it < it_lo || it >= it_hi) continue;  // another workgroup's slice (latency mode)
        const int N = s_nslice[it];
        const double* ls = s_lon_sum + mul24(3, mul24(it, nv) + iv);
        const double* ds = s_lat_sum + mul24(3, mul24(id, nt) + it);
        const int2 meta = s_lon_meta[mul24(it, nv) + iv];
        const int M = meta.x;
        uint32_t flags = (uint32_t)meta.y;
        bool hit = (s_collmask[2 * (mul24(it, nv) + iv) + (id >> 5)] >> (id & 31)) & 1u;
        if (n_obs > 0 && M == 1 && horizon_cap >= 1) hit = true;  // traj.yaw is empty -> IndexError -> collision (:178-182)
        if (hit) flags |= FP_FLAG_COLLISION;
        if (M < N) flags |= FP_FLAG_TRUNCATED;
        if (kb.curv_tbl) flags |= kb.curv_tbl[(size_t)b * C + c];  // optional curvature checks, computed by curvature_flags_kernel
        double cost = combine_cost(pa, N, ls, ds);  // cost_function.py:41-50, same grouping as the reference
        uint32_t word = flags | ((uint32_t)N << FP_FLAG_N_SHIFT) | ((uint32_t)M << FP_FLAG_M_SHIFT);
        if (N <= 0 || N > points_cap(pa)) {  // a time sample the ABI's limits exclude (unvalidated in FP_MEM_DEVICE mode): no trajectory,
            cost = __builtin_nan("");        // exactly what the lane-per-candidate kernel reports (traj_eval)
            word = flags = FP_FLAG_SPEED | FP_FLAG_ACCEL | FP_FLAG_COLLISION;
        }
        if constexpr (FISS) {  // (read by the ego's search workgroup in THIS launch: agent-scope stores, see the template's comment)
            __hip_atomic_store((unsigned long long*)&kb.r.cost_tbl[(size_t)b * C + c], (unsigned long long)__double_as_longlong(cost), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&kb.r.flag_tbl[(size_t)b * C + c], word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (kb.r.cost_tbl) kb.r.cost_tbl[(size_t)b * C + c] = cost;
            if (kb.r.flag_tbl) kb.r.flag_tbl[(size_t)b * C + c] = word;
        }
        if (!(flags & FP_FLAG_INFEASIBLE) && cost == cost) mine = best_merge(mine, Best{cost, c});
    }
    if constexpr (FISS) {  // every thread's table stores are acknowledged before the barrier below - and so before the ticket / the flag
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        __builtin_amdgcn_s_waitcnt(0);
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
    }
    // [/section ASM]
    // [section ARGMIN]
    // (a whole-blocked ego - block-uniform - has nothing to reduce: every thread's `mine` is Best{., -1} still, thread 0's is what RESULTS reads)
    if (!whole) {
    if constexpr (kArgWave) {
        // ONE wavefront reduces the workgroup: every lane leaves its `mine` in LDS, the first wavefront merges kWaves of them per lane
        // and runs the exchange chain once (it ran on all kWaves, and thread 0 merged their partials).  best_merge is a total order
        // on (cost, index) among feasible candidates with a cost that is a number - all ASM lets through - so any reduction tree
        // ends on the same winner.  The bytes are the survivors' pose table: nothing reads it after the walk's last barrier (the
        // series of the two-per-CU instances read the spline, the sample grids and s_best), and it exists in every layout.
        static_assert(sizeof(Best) == 16 && 32 * kItemCap >= (int)sizeof(Best) * kThreads, "every thread's partial argmin fits the pose table");
        Best* s_arg = (Best*)(smem + L.pose);
        s_arg[tid] = mine;
        __syncthreads();
        if (wave == 0) {  // (not wave_s: a scalar held through the walk costs the four-per-CU instances spilled SGPRs at the kernel's entry)
            mine = s_arg[lane];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) mine = best_merge(mine, s_arg[w * kWave + lane]);
            mine = wave_best(mine);
        }
    } else {
        mine = wave_best(mine);
        if (lane == 0) s_best[wave] = mine;
        __syncthreads();
    }
    }
    FP_STAMP(9);
    // [/section ARGMIN]
    // [section RESULTS]
    if (nsplit > 1) {
        // Latency mode: this workgroup holds the argmin of its slices.  The LAST workgroup of the ego to arrive (ticket counter;
        // the partial argmins travel as device-coherent atomic stores / loads) merges the partial argmins in part order - the result does not depend on
        // the arrival order - and carries on as the ego's only workgroup: results, epilogue.  No merge launch.
        if (tid == 0) {
            Best r = mine;  // (kArgWave: the workgroup's argmin already)
            if constexpr (!kArgWave) {
                r = s_best[0];
                for (int w = 1; w < kWaves; ++w) r = best_merge(r, s_best[w]);
            }
            // device-coherent (agent scope) stores, acknowledged before the ticket is taken: no whole-L2 write-back fence
            // Ordering: relaxed agent-scope atomics go to the device-coherent L2 in program order per wavefront; s_waitcnt(0) holds
            // the ticket back until both stores are acknowledged by L2, and the merging workgroup reads the partials with
            // agent-scope atomic loads (served by L2, never by a stale L1 / scalar cache line).  That is a hardware argument
            // (gfx950: one coherent L2 per agent for atomics with agent scope), not a C++ memory-model one - a release / acquire
            // pair would be the portable spelling, but on this chip it writes back the whole L2 per workgroup (measured: 15-35 %
            // of the launch).  The signal fences pin the COMPILER to the same order (no motion of the stores, the wait, the ticket
            // or the loads across each other).  A kernel that faults leaves the ticket counters non-zero, but a GPU fault ends
            // the process on this stack, and with it the ctx that owns the counters.
            Best* mine = la.part_best + blockIdx.x;
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            __hip_atomic_store(&mine->cost, r.cost, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&mine->idx, r.idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            __builtin_amdgcn_s_waitcnt(0);
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            const int ticket = __hip_atomic_fetch_add(&la.part_count[b], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            s_cnt[3] = ticket;
        }
        __syncthreads();
        if (s_cnt[3] != nsplit - 1) return;
        FP_STAMP_LAST(5);
        if (tid == 0) {
            la.part_count[b] = 0;  // ready for the next launch
            __atomic_signal_fence(__ATOMIC_SEQ_CST);  // the loads below stay behind the ticket
            Best* pb = la.part_best + ((size_t)blockIdx.x - part);  // the ego's first workgroup
            auto part = [&](int w) {
                return Best{__hip_atomic_load(&pb[w].cost, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                            __hip_atomic_load(&pb[w].idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)};
            };
            Best r = part(0);
            for (int w = 1; w < nsplit; ++w) r = best_merge(r, part(w));
            s_best[0] = r;
        }
        __syncthreads();
    } else if (tid == 0) {
        Best r = mine;
        if constexpr (!kArgWave) {
            r = s_best[0];
            for (int w = 1; w < kWaves; ++w) r = best_merge(r, s_best[w]);
        }
        s_best[0] = r;
    }
    if (tid == 0) {
        const Best r = s_best[0];
        // (the hand-over first: its s_waitcnt would otherwise also wait for the stores below, and best_idx / best_cost may be
        // device-mapped HOST memory - a link round trip in front of every flag)
        if constexpr (OCC > 4) {
            if (kb.epi_flag) {  // hand the ego to the appended epilogue workgroups: index first, acknowledged by L2, then the flag
                __atomic_signal_fence(__ATOMIC_SEQ_CST);
                __hip_atomic_store(&kb.idx_shadow[b], r.idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __atomic_signal_fence(__ATOMIC_SEQ_CST);
                __builtin_amdgcn_s_waitcnt(0);
                __atomic_signal_fence(__ATOMIC_SEQ_CST);
                __hip_atomic_store(&kb.epi_flag[b], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __atomic_signal_fence(__ATOMIC_SEQ_CST);
            } else if (kb.idx_shadow) kb.idx_shadow[b] = r.idx;
        } else if (kb.idx_shadow) kb.idx_shadow[b] = r.idx;
#if defined(FP_TL)
        __hip_atomic_store((unsigned long long*)&kb.r.best_cost[b], (unsigned long long)__double_as_longlong((double)(wall_clock64() & 0xFFFFFFFFFFll)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&kb.r.best_idx[b], (int)(t_begin & 0x7FFFFFFFll), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_s_waitcnt(0);
#endif
        if constexpr (FISS) {
            if (la.ft.flag) {  // the ego's rows of the tables are complete (both halves of a tail-split ego: the ticket came after theirs)
                __atomic_signal_fence(__ATOMIC_SEQ_CST);
                __hip_atomic_store(&la.ft.flag[b], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __atomic_signal_fence(__ATOMIC_SEQ_CST);
            }
        }
#if !defined(FP_TL)
        kb.r.best_idx[b] = r.idx;
        kb.r.best_cost[b] = r.idx >= 0 ? r.cost : __builtin_nan("");
#endif
        if (kb.r.stats) {
            int32_t* st = kb.r.stats + (size_t)b * 4;
            st[0] = 0; st[1] = C; st[2] = C; st[3] = C;
        }
    }
    // 10 ns ticks: feeds the next launches' order (a tail ego leaves twice its last part's time: about what it would take whole)
    if (tid == 0 && la.dur && (nsplit == 1 || in_tail)) la.dur[b] = (int)(wall_clock64() - t_begin) * nsplit;
    // [/section RESULTS]
    // [section SERIES]
    if (nsplit > 1) FP_STAMP_LAST(10); else FP_STAMP(10);
#if defined(FP_PHASE_STAMPS)  // column 15: the workgroup's absolute start (10 ns ticks, low 40 bits) - the launch's occupancy over time
    if (threadIdx.x == 0 && ka.r.best_traj && (perm || blockIdx.x % nsplit == 0)) ka.r.best_traj[((size_t)b * FP_ARR_COUNT + 15) * (ka.r.traj_stride > 0 ? ka.r.traj_stride : FP_DEFAULT_STRIDE) + 112 + 15] = (double)(t_begin & 0xFFFFFFFFFFll);
#endif
    // ---------------------------------------------------------------- winner epilogue (what plan() returns), on request
    // The workgroup that found the argmin writes its series itself: no second launch, no re-staging of the ego's tables, and the
    // stores hide behind the other workgroups' arithmetic.  ONE wavefront does it (two time points per lane, neighbours by lane
    // shuffles: no barrier, no scratch); the other seven are done and leave - their issue slots go to the CU's other workgroup.
#if defined(FP_ABL_NO_WINNER)
    return;
#endif
    // fp_plan_step: the ego's hand-over to its next state (point 1 of the winner, stop rules) by the thread that published the argmin -
    // after the series below where this workgroup writes them (they describe the trajectory from the OLD state).  Every other
    // workgroup of the ego (latency mode, tail split) has read the state before it posted its partial argmin.
    // (The three-workgroup instances never do it: the hand-over needs ~110 registers - atan2, hypot, the spline search through global
    // memory - against their 80, and an instance that spills there also changes its code elsewhere; their launcher reports it and
    // advance_kernel follows the launch.)
    if constexpr (OCC > 4) return;  // (this variant is only launched when the series come from winner_traj_kernel)
    if (!ka.r.best_traj) {
        if (ka.has_loop && tid == 0) advance_ego(ka, b, s_best[0].idx, nullptr, ka.loop);
        return;
    }
    __syncthreads();
    if (wave != 0) return;
    const int win = s_best[0].idx;
    double d_end = __builtin_nan(""), v_end = d_end, T_end = d_end;
    if (win >= 0) {
        const int q1 = div_by<NV, ND * NV * NT>(win, inv_nv_a), iv = win - mul24(q1, nv);
        const int id = div_by<NT, ND * NT>(q1, inv_nt_a), it = q1 - mul24(id, nt);
        d_end = s_ds[id]; v_end = s_vs[iv]; T_end = s_ts[it];
    }
    if (ld != NX) {  // (coefficient window: the series run over the WHOLE horizon - straight from the batch's table)
        const int fg = in_frame[b];
        winner_series_wave(ka, b, b, win >= 0, d_end, v_end, T_end, lane, SplineLds{bt.knots + (size_t)fg * NX, bt.coef + (size_t)fg * 8 * NX, nx, NX}, eg);
    } else {
        winner_series_wave(ka, b, b, win >= 0, d_end, v_end, T_end, lane, sp, eg);
    }
    FP_STAMP_LAST(6);
    if (ka.has_loop && tid == 0) advance_ego(ka, b, win, nullptr, ka.loop);
    // [/section SERIES]
}


int lattice_group_fit(const fp_params& p, const fp_batch& b) { return group_fit(p, b); }

static std::atomic<long> g_launches_per_cu[3];
long lattice_launches_per_cu(int which) { return which >= 0 && which < 3 ? g_launches_per_cu[which].load(std::memory_order_relaxed) : 0; }

// The instances of kLatticeInstances, in its order: kernel and its LDS-attribute slot (see ensure_dynamic_lds).
using LatticeFn = void (*)(KernelArgs, int, int, int, Best*, int*, const int*, int*, int, int, int, int, FissTail, InlineIn);
template <int I>
constexpr LatticeFn lattice_kernel_of()
{
    constexpr LatticeKey k = kLatticeInstances[I];
    constexpr LatticeShapeDims d = kLatticeShapes[k.shape];
    constexpr bool grouped = k.family == kGrouped || k.family == kPolyGrouped;
    constexpr bool poly = k.family == kPoly || k.family == kPolyGrouped || k.family == kPolyWindow;
    constexpr bool win = k.family == kWindow || k.family == kPolyWindow;
    return lattice_fused_kernel<d.nd, d.nv, d.nt, d.stride, d.n_obs, d.rows, 2 * k.per_cu, grouped ? FP_GROUP_THREADS : kThreads, poly,
                                k.family == kSearch, win>;
}
struct LatticeInstance {
    LatticeFn kernel;
    LdsSlots lds_slot;
};
template <size_t... I>
static LatticeInstance& lattice_instance_at(int i, std::index_sequence<I...>)
{
    static LatticeInstance table[] = {{lattice_kernel_of<I>(), {}}...};
    return table[i];
}

static hipError_t launch_lattice_fused(const KernelArgs& ka, hipStream_t stream, const LatticeRequest& rq, const LatticePlan& pl, LatticeResult* res)
{
    if (ka.p.curvature_mask) {  // optional curvature checks: their own launch, ORed into the flag words by the assembly stage
        if (!ka.curv_tbl) return hipErrorInvalidValue;  // (internal: the caller provides the table)
        const hipError_t e = launch_curvature_flags(ka, const_cast<uint8_t*>(ka.curv_tbl), stream);
        if (e != hipSuccess) return e;
    }
    // the kernel's arguments, one variable per parameter
    KernelArgs kx = ka;  // (epilogue workgroups offered but not taken: the caller's winner_traj_kernel writes the series)
    if (ka.epi_flag && !pl.epilogue) { kx.r.best_traj = nullptr; kx.epi_flag = nullptr; }
    if (rq.provisional) { kx.r.best_traj = nullptr; kx.epi_flag = nullptr; kx.has_loop = 0; }  // (as planned: tables and a provisional argmin only)
    if (pl.per_cu > 2 && pl.nsplit != 1) return hipErrorInvalidValue;  // (internal: those instances read nsplit as 1, see kOnePart)
    int rows = pl.rows, hp = pl.hp, nsplit = pl.nsplit, reserved = 0, tail_from = pl.tail_from, epi_from = pl.epi_from, wcap = pl.wcap;
    // part_scratch: [ticket counters: kTicketBytes, zero between launches][partial argmins: Best x B x nsplit]
    int* part_count = (int*)rq.part_scratch;
    Best* part_best = rq.part_scratch ? (Best*)((char*)rq.part_scratch + kTicketBytes) : nullptr;
    const int* perm = pl.nsplit == 1 ? rq.perm : nullptr;
    int* dur = rq.dur;
    FissTail fx{};
    if (pl.search) { fx = *rq.ft; fx.NB = kAppendedSearchNB; }
    static const InlineIn kNoInline{};
    const InlineIn* in = rq.inl ? rq.inl : &kNoInline;
    void* args[] = {&kx, &rows, &hp, &nsplit, &part_best, &part_count, &perm, &dur, &reserved, &tail_from, &epi_from, &wcap, &fx, (void*)in};
    LatticeInstance& inst = lattice_instance_at(pl.instance, std::make_index_sequence<kLatticeInstanceCount>());
    hipError_t e = ensure_dynamic_lds((const void*)inst.kernel, pl.lds, inst.lds_slot);
    if (e != hipSuccess) return e;
    e = hipLaunchKernel((const void*)inst.kernel, dim3(pl.grid), dim3(pl.threads), args, pl.lds, stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return e;
    g_launches_per_cu[pl.per_cu - 2].fetch_add(1, std::memory_order_relaxed);
    *res = LatticeResult{pl.series, kx.has_loop != 0 && pl.per_cu == 2, pl.search};  // (the two-per-CU instances hand the egos over themselves)
    return hipSuccess;
}

hipError_t launch_lattice(const KernelArgs& ka, hipStream_t stream, int which, const LatticeRequest& rq, LatticeResult* res)
{
    *res = LatticeResult{};
    const LatticePlan pl = which == 1 ? LatticePlan{} : plan_lattice(ka, rq);
    if (pl.fits) return launch_lattice_fused(ka, stream, rq, pl, res);
    if (which == 2 || (rq.inl && rq.inl->on)) return hipErrorInvalidValue;  // (the fused kernel or nothing)
    return launch_lattice_percand(ka, stream);
}

}  // namespace fp
