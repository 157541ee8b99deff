/*
 * frenet_gpu.h - C ABI of libfrenetgpu.so, the MI355X (gfx950) Frenet trajectory
 * sampling-and-scoring engine.
 *
 * This is the drop-in boundary for the candidate-generation hot path of
 * SS47816/fiss_plus_planner.  The reference is pure Python and has no FFI of its
 * own; each entry point below names the reference code it replaces (paths relative
 * to the reference checkout).  Bindings: ctypes (fiss_plus_planner_amd/_abi.py);
 * the stub a maintainer of the reference would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success, a negative FP_E* code on failure;
 *     fp_last_error() returns a thread-local description.  Nothing throws.
 *   - all arrays are contiguous, little-endian, float64 / int32 / uint32.
 *   - `mem` says where EVERY pointer of the call lives: FP_MEM_HOST (the library
 *     stages through device buffers it owns inside the ctx, runs, copies back and
 *     synchronises before returning) or FP_MEM_DEVICE (pointers are device
 *     addresses on the ctx's GPU; the call only enqueues work on `stream` and
 *     returns; no synchronisation and no allocation once the ctx's scratch buffers
 *     have reached the size the batch needs, i.e. after the first call of that size).
 *     FP_MEM_DEVICE calls cannot look at the arrays: frame_of / scene_of / nx / t_now / best_idx are NOT range-checked (an
 *     out-of-range index is a GPU memory fault, not FP_EINVAL - unless fp_ctx_set_option("validate", 1) is on), and a time sample that needs more than FP_MAX_POINTS points
 *     yields NaN cost + FP_FLAG_INFEASIBLE for its candidates instead of FP_ELIMIT.  Validate on the host, or use FP_MEM_HOST.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *   - a ctx is bound to one device; calls on one ctx must not overlap in time, and the work they enqueue must not either: use
 *     one stream per ctx at a time (the ctx keeps scratch buffers - partial results, launch order - that successive calls reuse
 *     in stream order).  FP_MEM_DEVICE calls may allocate or grow such a scratch buffer on first use (never inside a stream capture
 *     after a warm-up call of the same size).  A captured graph holds the addresses of those buffers: a later call on the same ctx
 *     with a LARGER batch may reallocate them - capture again after such a call.
 */
#ifndef FRENET_GPU_H
#define FRENET_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FP_ABI_VERSION 18

/* error codes */
#define FP_OK 0
#define FP_EINVAL (-1)  /* bad argument */
#define FP_EHIP (-2)    /* HIP runtime error (see fp_last_error) */
#define FP_ENOMEM (-3)
#define FP_ELIMIT (-4)  /* problem exceeds a compiled-in limit (FP_MAX_*) */
#define FP_ENODEV (-5)  /* no usable gfx950 device */

/* memory space of the pointers of a call */
#define FP_MEM_HOST 0
#define FP_MEM_DEVICE 1

/* compiled-in limits */
#define FP_MAX_POINTS 256   /* N = ceil(T / tick_t) per trajectory (T = 10 s at tick_t = 0.05 s: 200).  Up to FP_FAST_POINTS every
                               kernel runs its two-points-per-lane fast path; beyond it the series come from a chunked writer, the
                               epilogue workgroups and the per-profile materialiser give way to winner_traj_kernel, and the FISS+
                               refinement runs its four-points-per-lane instance (two workgroups per CU instead of three) */
#define FP_FAST_POINTS 128
#define FP_DEFAULT_STRIDE 128 /* columns of a series row when traj_stride = 0 */
#define FP_MAX_KNOTS 1024   /* reference-line knots per frame (72 bytes of LDS each in every kernel that walks the line) */
#define FP_MAX_CAND 16384   /* nd*nv*nt of the dense pass (fp_plan_dense and everything built on its tables) */
#define FP_MAX_CAND_SEARCH 4096 /* nd*nv*nt of the device-side FISS / FISS+ walks (fp_plan_fiss: rank bit sets of 64 x 64 bits); above
                                   it FP_ELIMIT - walk the dense tables on the host (fiss_plus_planner_amd/search.py), as the drop-in
                                   planner classes then do by themselves */
#define FP_MAX_POLY_VERTS 128 /* vertices of one convex-polygon obstacle column (shapely's buffer() circle has 64) */
#define FP_MAX_RANK 64      /* K of fp_rank_feasible */
#define FP_MAX_GATES 32     /* gates per frame of fp_gate_mask (one bit each of a `closed` word) */

/* candidate flag word: low bits = why a candidate is infeasible, then N and M */
#define FP_FLAG_SPEED 1u      /* any(s_d > max_speed)       frenet_optimal_planner.py:152 */
#define FP_FLAG_ACCEL 2u      /* any(|s_dd| > max_accel)    frenet_optimal_planner.py:155 */
#define FP_FLAG_COLLISION 4u  /* has_collision()            frenet_optimal_planner.py:168-195 */
#define FP_FLAG_TRUNCATED 8u  /* M < N: left the spline     frenet_optimal_planner.py:112-113 */
/* the three checks check_constraints carries commented out (frenet_optimal_planner.py:145-150); set only when
 * fp_params.curvature_mask != 0 */
#define FP_FLAG_CURVATURE 16u /* any(|c| > max_curvature)    :145-146 */
#define FP_FLAG_KAPPA_D 32u   /* any(|c_d| > max_kappa_d)    :147-148 */
#define FP_FLAG_KAPPA_DD 64u  /* any(|c_dd| > max_kappa_dd)  :149-150 */
#define FP_FLAG_CONSTRAINTS (FP_FLAG_SPEED | FP_FLAG_ACCEL | FP_FLAG_CURVATURE | FP_FLAG_KAPPA_D | FP_FLAG_KAPPA_DD) /* check_constraints */
#define FP_FLAG_BOUNDARY 128u  /* the candidate leaves the road corridor; written by fp_boundary_mask only (no other entry point sets it) */
#define FP_FLAG_INFEASIBLE (FP_FLAG_CONSTRAINTS | FP_FLAG_COLLISION | FP_FLAG_BOUNDARY)
#define FP_FLAG_N_SHIFT 8     /* bits 8..19  N = len(t) */
#define FP_FLAG_M_SHIFT 20    /* bits 20..31 M = len(x) */

/* rows of a [16][stride] trajectory dump = FrenetTrajectory series, frenet.py:129-146 */
enum {
    FP_ARR_T = 0, FP_ARR_S, FP_ARR_S_D, FP_ARR_S_DD, FP_ARR_S_DDD, FP_ARR_D, FP_ARR_D_D, FP_ARR_D_DD, FP_ARR_D_DDD,
    FP_ARR_X, FP_ARR_Y, FP_ARR_YAW, FP_ARR_DS, FP_ARR_C, FP_ARR_C_D, FP_ARR_C_DD, FP_ARR_COUNT
};

typedef struct fp_ctx fp_ctx;

/* Settings + vehicle + cost weights.
 * Replaces: FrenetOptimalPlannerSettings (frenet_optimal_planner.py:38-56), Vehicle
 * (common/vehicle/vehicle.py:15-46), CostFunction("WX1") weights (common/cost/cost_function.py:6-12). */
typedef struct {
    int32_t nd, nv, nt;     /* num_width, num_speed, num_t */
    int32_t check_stride;   /* check_res of has_collision (2)              :202 */
    double tick_t;          /* 0.1 */
    double cost_horizon;    /* the 10.0 of `cost_time = 10.0 - t[-1]`      cost_function.py:42 */
    double w_speed, w_accel, w_jerk, w_offset; /* w_V=1, w_A=0.1, w_J=0.1, w_LC=10 */
    double veh_l, veh_w;    /* ego footprint */
    double max_speed, max_accel;
    /* Optional curvature checks: the reference has them in check_constraints but commented out (:145-150), so 0 = off is the
     * reference's behaviour.  != 0: a candidate whose Cartesian series has any |c| > max_curvature, |c_d| > max_kappa_d or
     * |c_dd| > max_kappa_dd (c = diff(yaw)/ds, c_d = diff(c)/tick_t, c_dd = diff(c_d)/tick_t, :131-134) fails the constraints
     * like a speed / acceleration violation does.  Limits: Vehicle.max_curvature / max_kappa_d / max_kappa_dd (vehicle.py:44-46). */
    int32_t curvature_mask;
    /* FP_MEM_DEVICE calls only (FP_MEM_HOST calls look at t_samples / samp_max themselves): an upper bound of the points per trajectory,
     * ceil(T / tick_t) over every time sample the call can generate.  0 = at most FP_FAST_POINTS (128); a caller whose batch needs
     * more says so here (<= FP_MAX_POINTS) and gets the kernels that can do it.  A device batch that needs more points than announced
     * yields NaN cost + FP_FLAG_INFEASIBLE for those candidates, as beyond FP_MAX_POINTS. */
    int32_t points_max;
    double max_curvature, max_kappa_d, max_kappa_dd;
    /* Optional obstacle-clearance cost term (ABI 16).  The reference defines the weight (w_D = 0.1, cost_function.py:9), sketches the
     * term (cost_dist_obstacle, :21-27: `Xis = np.exp(-dists); return w_D * sum(Xis)`) and keeps its slot in cost_total at zero
     * (`cost_obstacle = 0.0`, :43), so 0 = off is the reference's behaviour, bit for bit and launch for launch.  > 0: fp_plan_dense and
     * fp_plan_step price every candidate that SURVIVED the checks (no FP_FLAG_INFEASIBLE bit) as
     *     cost_final = (base_sum + w_obstacle * clearance) / N,   clearance = sum_i sum_j exp(-dist(i, j)),
     * base_sum / N being the cost_final without the term: i runs over has_collision's poses (frenet_optimal_planner.py:168-195:
     * i = 0, check_stride, 2 check_stride, ... < min(M, final_time_step - t_now), the veh_l x veh_w footprint at x[i], y[i], yaw[i]), j over
     * the obstacle columns with a valid pose at step i + t_now, and dist is the Euclidean distance in metres between the two closed
     * convex shapes (rectangle against rectangle, or against the column's ring when obs_nvert > 0; 0 when they touch - which a survivor
     * never does).  Pairs at least 48 m apart are not summed (together below 2e-15 per candidate).  cost_tbl holds the new value for
     * the survivors and the old one for every other candidate; best_idx / best_cost / best_traj belong to the argmin of the new costs
     * (last minimum in FOP order on exact ties, :264-268); Stats do not change.  A second kernel behind the lattice pass does it (over
     * the call's tables, or tables of [B][C] in the ctx's scratch when the caller passed none).
     * FopPlusPlanner, FissPlanner and FissPlusPlanner order candidates by cost BEFORE a trajectory has Cartesian points
     * (fop_plus_planner.py:16-41, fiss_planner.py:101-138), so the term has no defined place there yet: result.fopplus, result.audit,
     * fp_plan_fiss and fp_plan_fiss_step return FP_EINVAL when it is non-zero.  fp_eval_trajs prices arbitrary end states and ignores it.
     * < 0 or not finite: FP_EINVAL. */
    double w_obstacle;
} fp_params;

/* A batch of B independent ego planning problems (layout: DESIGN.md "problem batch"). */
typedef struct {
    int32_t B, F, NX, S, T_obs, n_obs;
    const double* d_samples;     /* [nd]        np.linspace(-sw/2, sw/2, nd)      :75 */
    const double* t_samples;     /* [nt]        np.linspace(min_t, max_t, nt)     :78 */
    const double* v_samples;     /* [B][nv]     np.linspace(lowest, highest, nv)  :89 */
    const double* target_speed;  /* [B]         settings.highest_speed            :250 */
    const double* ego;           /* [B][6]      s, s_d, s_dd, d, d_d, d_dd        frenet.py:15-27 */
    const int32_t* frame_of;     /* [B]         index into the frame table */
    const int32_t* scene_of;     /* [B]         index into the scene table, -1 = no obstacles */
    const int32_t* t_now;        /* [B]         time_step_now */
    const int32_t* nx;           /* [F]         knots per frame */
    const double* knots;         /* [F][NX]     cumulative chord length, +inf padded   cubic_spline.py:162-168 */
    const double* coef;          /* [F][8][NX]  ax bx cx dx ay by cy dy                cubic_spline.py:30-43 */
    const double* obs_pose;      /* [S][T_obs][n_obs][4]  x, y, yaw, valid(0/1) */
    const double* obs_dims;      /* [S][n_obs][2]         length, width (a polygon column: the centred box that contains it, see obs_poly) */
    const int32_t* final_time_step; /* [S]      obstacles[0].prediction.final_time_step :173 */
    const int32_t* skip;         /* NULL or [B]: egos with skip[b] != 0 are not planned (best_idx = -1, no table rows written);
                                    the closed-loop driver passes its `done` array here */
    /* FP_MEM_HOST only, 0 = off.  A non-zero tag is the caller's promise that the frame and scene tables of this call (nx, knots,
     * coef, obs_pose, obs_dims, final_time_step - with F, NX, S, T_obs, n_obs) are byte for byte those of the previous
     * FP_MEM_HOST call on this ctx that carried the same tag: the library then keeps them on the device and uploads only the
     * per-ego arrays (a planner re-plans against the same centerline and obstacle predictions cycle after cycle; for one ego that
     * is ~100 KB per call that need not travel, ~12 us of a ~43 us call).  A new tag (or changed sizes) uploads again; a ctx keeps
     * the tables of its four most recently used tags.  Ignored by FP_MEM_DEVICE calls. */
    int32_t tables_tag;
    /* Obstacle shapes other than rectangles (ABI 12).  has_collision hands `obstacle.obstacle_shape.shapely_object` - ANY polygon - to
     * construct_polygon and Polygon.intersects (frenet_optimal_planner.py:162-166, :189-191).  obs_nvert == NULL: every column is the
     * rectangle of obs_dims.  Else obs_nvert[s][j] = 0 for a rectangle, or the number of vertices (3 .. poly_stride) of a CONVEX
     * polygon whose ring is obs_poly[s][j][0 .. nvert): (x, y) relative to the column's rotation centre - the centre of the shape's
     * bounding box, about which affinity.rotate(origin='center') turns it; the column's poses carry that centre - in COUNTER-CLOCKWISE
     * order, closing vertex not repeated.  At a pose (x, y, yaw) vertex i sits at (x, y) + R(yaw) (u_x, u_y).  obs_dims of such a column
     * MUST be (2 max|u_x|, 2 max|u_y|) or larger (the broad phases test that box; FP_MEM_HOST calls check it).  A circle is the polygon
     * shapely's buffer() makes of it; a non-convex shape or a group of shapes is several columns with the same poses, one convex piece
     * each, every piece relative to the WHOLE shape's centre (fiss_plus_planner_amd/obstacles.py does all of this).  Part of the
     * scene tables as far as tables_tag is concerned.
     * The narrow phase tests a ring as the intersection of its edge half-planes: a ring that is NOT convex, NOT counter-clockwise or
     * that reaches outside obs_dims is tested as a smaller shape than it is (missed collisions; a clockwise ring never collides).
     * FP_MEM_HOST calls reject such columns with FP_EINVAL; FP_MEM_DEVICE calls do so only with fp_ctx_set_option("validate", 1) -
     * rings handed over in device memory without it are the caller's responsibility, and the result for a bad ring is undefined. */
    int32_t poly_stride;          /* vertices per column of obs_poly (<= FP_MAX_POLY_VERTS); ignored when obs_nvert == NULL */
    const double* obs_poly;       /* NULL or [S][n_obs][poly_stride][2] */
    const int32_t* obs_nvert;     /* NULL or [S][n_obs] */
    /* Launch-order hint (ABI 14), FP_MEM_DEVICE calls: NULL, or a permutation of 0 .. B-1 in device memory - the egos in the order their
     * workgroups should START when the batch has more egos than the device holds workgroups at once (the launch ends on the egos that
     * start last: put the ones expected to take longest first; ego speed, descending, is a good stand-in - a faster ego reaches more
     * obstacle rows - and is what fiss_plus_planner_amd.device_batch.DeviceBatch passes, computed once at upload).  Results do not
     * depend on it; entries outside 0 .. B-1 or repeated entries are the caller's responsibility (fp_ctx_set_option("validate", 1)
     * checks them).  NULL: the library orders a launch by the durations an earlier launch of the ctx left behind ("lattice_order").
     * Ignored by FP_MEM_HOST calls. */
    const int32_t* launch_order;
} fp_batch;

/* Outputs of the dense lattice pass; any pointer except best_idx/best_cost may be NULL.
 * best_traj requires best_flags. */
typedef struct {
    int32_t* best_idx;   /* [B]     flat FOP index (i_d*nt+i_T)*nv+i_v of the argmin, -1 = no survivor  :263-268 */
    double* best_cost;   /* [B]     its cost_final (NaN when -1) */
    double* cost_tbl;    /* [B][C]  cost_final of every candidate                                       :99 */
    uint32_t* flag_tbl;  /* [B][C]  FP_FLAG_* | N << 8 | M << 20 */
    int32_t* stats;      /* [B][4]  num_iter, generated, validated, collision_checks                    :254-256 */
    uint32_t* best_flags; /* [B]    flag word (N, M) of the argmin, 0 when best_idx = -1 */
    double* best_traj;   /* [B][16][traj_stride]  winner epilogue: the argmin's full FrenetTrajectory series (NaN padded;
                            all NaN when best_idx = -1) = what plan() returns                           :264-270 */
    int32_t* fopplus;    /* NULL or [B][2]: FopPlusPlanner.plan for every ego (fop_plus_planner.py:16-41: candidates validated lazily in
                            cost order, the first feasible one wins).  [b][0] = candidates popped up to and including the winner
                            (all C when nothing is feasible) = num_iter = validated = collision checks, also written to stats;
                            [b][1] = 1 when an exact cost tie (or a NaN cost) at the decision point leaves the outcome to the
                            reference's heap order - replay that ego on the host (fiss_plus_planner_amd/search.py:fopplus_search) -
                            else 0: best_idx / best_cost ARE FopPlusPlanner's answer */
    uint32_t* audit;     /* NULL or [B]: how thin the margins under this ego's answer are (FP_AUDIT_* bits, see below).  Asking for it
                            adds a pass over the ego's tables (one more launch) and, where FP_AUDIT_NEAR_TIE is found, settles the
                            choice among the tied candidates by the reference's own point-by-point sums. */
    int32_t traj_stride; /* columns per series row; 0 = FP_DEFAULT_STRIDE.  Must be >= the largest N = ceil(T / tick_t) of the batch
                            (e.g. 100 for T <= 10 s at 0.1 s): a smaller stride is FP_EINVAL (host) / truncates the rows (device) */
    int32_t traj_sparse; /* 0: every element of the [16][traj_stride] block is written (NaN where a row has no element).
                            1: only the rows' leading elements are written - row r gets its len(r) elements (N for the Frenet rows,
                            M / M-1 / M-2 / M-3 for x y yaw / ds c / c_d / c_dd) plus NaN up to the next multiple of 16 columns (so
                            that, with a stride that is a multiple of 16, only whole 128-byte lines are stored); the rest of the
                            block and the blocks of egos without a winner (best_flags = 0) are left untouched.  Bytes written =
                            the algorithmic bytes rounded up to lines: ~6 % more at N ~ 90.  Use traj_stride = 112 for T <= 10 s */
} fp_result;

/* fp_result.audit bits.  The kernels sum the cost terms in closed form (~1e-12 from the reference's point-by-point sums) and decide box
 * overlaps in fp64 (they can differ from shapely / GEOS's exact predicates for boxes closer than ~1e-13 m to touching), so "the
 * selected index is exact" holds with a margin.  These bits say when the margin is gone:
 *   FP_AUDIT_NEAR_TIE    another FEASIBLE candidate's cost lies within FP_AUDIT_COST_TOL of the winner's.  The tied candidates (and
 *                        the winner) were then re-priced with the reference's summation (one term per trajectory point, in order)
 *                        and the argmin rule (:263-268, last minimum wins) applied to those sums; best_idx / best_cost are the outcome.
 *   FP_AUDIT_REORDERED   ... and that changed the winner.
 *   FP_AUDIT_CONTACT     the collision verdict of the winner, or of a candidate at most as expensive that was rejected ONLY for
 *                        colliding, hangs on a pair of boxes within FP_AUDIT_GAP_TOL metres of touching (their deepest overlap over
 *                        all checked poses and obstacles is shallower than that, or their closest miss nearer): a different
 *                        rounding of the same geometry - GEOS, another compiler - could decide this ego differently.
 *   FP_AUDIT_TIES_OVERFLOW  more than 63 candidates were within the tolerance: the first 63 in index order (and the winner) were
 *                        re-priced, the others were not - the outcome is deterministic but not settled among all of them.
 * best_cost of an ego whose FP_AUDIT_NEAR_TIE bit is set is the POINT-BY-POINT sum of its (possibly new) winner; every other ego keeps
 * the closed-form sum (the two differ by ~1e-12: one output array, two summation orders - compare against cost_tbl with that in mind).
 * No bit set: every comparison behind best_idx was decided by more than the tolerances. */
#define FP_AUDIT_NEAR_TIE 1u
#define FP_AUDIT_CONTACT 2u
#define FP_AUDIT_REORDERED 4u
#define FP_AUDIT_TIES_OVERFLOW 8u
#define FP_AUDIT_COST_TOL 1e-9
#define FP_AUDIT_GAP_TOL 1e-9

int fp_abi_version(void);
const char* fp_last_error(void);

/* Build identity.  fp_build_flags: the diagnostic macros the library was compiled with (the Makefile's EXTRA and every FP_ABL_* /
 * FP_NO_* / stamp / counter switch of the sources) - "" for a production build; the timing ablations produce WRONG results by design,
 * so the Python binding refuses a library whose string is not empty (FP_ALLOW_DIAGNOSTIC_BUILD=1 overrides, for the profiling tools).
 * fp_build_compiler: the compiler's version string (the kernels are validated on one toolchain, see csrc/Makefile). */
const char* fp_build_flags(void);
const char* fp_build_compiler(void);

/* Number of visible HIP devices / name+arch of one (buf may be NULL). */
int fp_device_count(int* count);
int fp_device_info(int device, char* buf, int buflen, int* compute_units, int64_t* hbm_bytes);

int fp_ctx_create(int device, fp_ctx** out);
int fp_ctx_destroy(fp_ctx* ctx);

/* Diagnostic knobs.  "lattice_kernel": 0 = auto (default), 1 = lane-per-candidate kernel, 2 = fused
 * profile-sharing kernel only (fails with FP_EHIP if the problem does not fit it).  Results are identical
 * (flags / indices exactly, costs to ~1e-13); used by the A/B parity tests and by profiling.
 * "lattice_split": 0 = auto (default: an ego's time-horizon slices are spread over as many workgroups - at most one per
 * slice - as keep ALL workgroups of the launch resident at once, 2 per compute unit: latency mode for small batches), 1 = never,
 * 2 = always one workgroup per slice.  Identical results either way.
 * "lattice_group": whether an ego's workgroups have 1024 threads instead of 512 (twice the wavefronts working through its lon
 * profiles).  0 = auto (default: 512, except for batches of at most one ego per compute unit that "lattice_split" could only cut in
 * two: one 1024-thread workgroup per ego then takes all nt slices, when its tables fit the LDS), 1 = always 512, n >= 2 = 1024
 * where its tables fit and the lattice has at least two slices of at most 128 end speeds each; n beyond 2 changes nothing.
 * Identical results.
 * "lattice_tail": 0 = auto (default: a launch with more one-workgroup egos than stay resident cuts the LAST quarter round of its
 * dispatch slots in two workgroups each - slices split, ticket + merge as in latency mode - so that it does not end on whole egos
 * that started last), 1 = never, n >= 2 = the last n slots.  Identical results.
 * "lattice_occupancy": 0 = auto (default: batches of more egos than stay resident run three lattice workgroups per compute unit - four
 * when a workgroup's tables fit a quarter of the unit's LDS: rectangle scenes, e.g. a 9 x 9 x 7 lattice against 50 obstacles on
 * reference lines of up to ~80 knots - instead of two), 2 / 3 / 4 = at most that many.  Identical results.
 * "overlap": 0 (default) = every call is ordered on the caller's stream like a kernel launch.  1 = FP_MEM_DEVICE fp_plan_dense calls
 * alternate between two INTERNAL streams of the ctx, so that two consecutive independent calls run side by side on the device: the
 * draining tail of one launch (a fifth of a 2048-ego launch runs on a chip that is emptying) overlaps the ramp of the next.  Ordering
 * with "overlap" on: (1) a call starts after everything enqueued on the caller's `stream` before it; (2) when fp_plan_dense returns,
 * `stream` is ordered after the results of the PREVIOUS dense call on the ctx (and of every older one), not yet after this call's - at
 * most two calls are in flight; (3) fp_ctx_join(ctx, stream), or any other entry point of the ctx, orders `stream` after all of them;
 * (4) a call that writes an array its predecessor writes (any fp_result member equal) is not independent: it waits for the predecessor.
 * The inputs of a call must not be outputs of the call before it (dense outputs are not dense inputs; fp_plan_step / fp_plan_fiss, which
 * do feed themselves, never overlap).  Calls inside a stream capture are never overlapped.  Identical results.
 * "resident_groups": lattice workgroups the device holds at once at two per compute unit.  0 / default = 2 x the device's compute units.
 * The latency-mode split, the tail split, the three- / four-per-unit instances and the launch order key on it: set it to 2 x the units the
 * process really has when it runs under a CU mask (HSA_CU_MASK / ROC_GLOBAL_CU_MASK - the runtime still reports every unit), or lower to
 * model a smaller device (the tests run the multi-round instances on a handful of egos that way).  Even, >= 2.  Identical results.
 * "lattice_order": 1 (default) = launches with more egos than resident workgroups dispatch the egos longest-first, from the
 * durations earlier launches left behind (fetched asynchronously, sorted on the host); 0 = index order.  Identical results.
 * "refine_table_kb": LDS budget (KiB, default 96, 0 = off) of the FISS+ refinement kernel's per-ego pose-obstacle pair
 * table; scenes whose table does not fit are checked straight from the scene table.  Identical results either way.
 * "lattice_winner": who writes fp_plan_dense's best_traj: 0 = auto (the lattice workgroups themselves while one round of them
 * holds the batch; for bigger batches epilogue workgroups appended to the lattice launch, which become resident in the slots the
 * draining launch leaves empty and wait for their egos' argmins - one launch per call), 1 = always the lattice workgroups, 2 = always
 * winner_traj_kernel behind the lattice launch.  Identical results.
 * "validate": 1 = FP_MEM_DEVICE calls first run a one-lane-per-ego range check of frame_of / scene_of / t_now / nx / t_samples on the
 * device and return FP_EINVAL / FP_ELIMIT (with the offending index in fp_last_error) instead of faulting the GPU; the call then
 * WAITS for the stream (one small kernel + an 8-byte copy).  0 (default) = no check, nothing waits.
 * "fiss_jump": 1 (default) = the FISS+ search walk runs its first iteration, then jumps to the state the reference's walk has
 * when the first feasible sample becomes reachable (minimax cost level, computed in parallel) and resumes there; 0 = every
 * iteration one after the other.  Identical results and Stats.
 * "stage_kernel" (1 default), "inline_inputs" (1 default), "zero_copy_in" (0 default): how an FP_MEM_HOST call of at most 8 egos
 * moves its inputs.  stage_kernel: the pinned staging block goes to the device by one copy KERNEL instead of copy commands (a
 * copy command plus the cross-engine dependency behind it costs ~15 us of a single-ego call).  inline_inputs: fp_plan_dense and
 * fp_plan_fiss with fp_batch.tables_tag set pass the per-ego arrays inside the lattice kernel's argument block - nothing is copied at
 * all (fp_plan_fiss: the lattice kernel leaves them in device memory for the kernels behind it).
 * zero_copy_in: the kernels read inputs from the pinned host block over the link (1: the per-ego arrays of a tagged call, 2:
 * everything) - measured slower than the copy kernel, kept for experiments.  Identical results in every combination.
 * "fiss_fused": 1 (default) = a FISS+ call of more egos than stay resident runs its search walk in workgroups APPENDED to the lattice
 * launch (one per ego; they become resident in the slots the draining launch leaves empty, wait for their ego's dense tables and walk
 * them - two launches per call instead of three); 0 = the search kernel always follows in its own launch.  Identical results.
 * "fiss_stages": timing diagnostic of fp_plan_fiss, 3 (default) = the whole pipeline, 2 = stop after the search walk (no
 * refinement), 1 = stop after the dense lattice pass; with 1 or 2 the outputs of the skipped stages are NOT produced. */
int fp_ctx_set_option(fp_ctx* ctx, const char* name, int value);
/* Reads an option back, or one of the read-only counters "clearance_launches" (launches of the clearance rescoring kernel,
 * fp_params.w_obstacle > 0, of this ctx so far), "looplog_launches" (launches of fp_loop_record's kernel), "rank_launches" (launches of
 * fp_rank_feasible's kernel), "boundary_launches" (launches of fp_boundary_mask's kernel), "envelope_launches" (launches of fp_speed_envelope's kernel), "gate_launches" (launches of fp_gate_mask's kernel), "margin_launches" (launches of fp_traj_margins' kernel), "fallback_launches" (launches of fp_fallback_stop's kernel), "fallback_rules_launches" (launches of fp_fallback_stop_rules' kernel), "rules_eval_launches" (launches of fp_rules_eval's kernel), "predict_launches" (launches of
 * fp_obstacles_predict's kernel), "from_plans_launches" (launches of fp_obstacles_from_plans' kernel), "from_state_launches" (launches of fp_from_state's kernel), "lattice_launches" (dense lattice launches of this ctx so far) and
 * "lattice_ordered_launches" (those dispatched in a feedback order or in the order of fp_batch.launch_order) - bench.py reports when an
 * order took effect -, "lattice_launches_2" / "_3" / "_4" (PROCESS-wide: fused lattice launches so far by workgroups per compute unit). */
int fp_ctx_get_option(fp_ctx* ctx, const char* name, int* value);
/* "overlap" = 1: orders `stream` (a hipStream_t, NULL = the default stream) after every dense call of the ctx that is still in flight on
 * its internal streams.  A no-op otherwise.  Also read-only: "overlapped_calls" = dense calls that started beside their predecessor. */
int fp_ctx_join(fp_ctx* ctx, void* stream);

/* Dense lattice pass = FrenetOptimalPlanner.plan() for B egos at once:
 *   calc_frenet_paths (:69-104) + CostFunction.cost_total (cost_function.py:41-50)
 *   + calc_global_paths (:106-138) + check_constraints (:140-160)
 *   + check_collisions/has_collision (:168-208) + argmin with the `>=` tie rule (:263-268).
 * The tables also feed the FOP+/FISS/FISS+ drop-ins (cost-ordered validation and
 * the index walks read them instead of generating candidates one by one). */
int fp_plan_dense(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_result* result, int mem,
                  void* stream);

/* Winner epilogue on its own: full series of lattice candidate best_idx[b] for every ego -> best_flags [B],
 * best_traj [B][16][traj_stride] (traj_stride / traj_sparse as in fp_result).  fp_plan_dense produces the same output inside its own launch when result.best_traj is set
 * (the workgroup that finds the argmin writes the series); exported separately for callers that pick the trajectory
 * themselves.  Replaces the object hand-back of plan() (:264-270). */
int fp_winner_trajs(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const int32_t* best_idx, uint32_t* best_flags,
                    double* best_traj, int32_t traj_stride, int32_t traj_sparse, int mem, void* stream);

/* ---- the K cheapest feasible candidates of every ego (ABI 18) ------------------------------------------------------
 * fp_plan_dense returns one index per ego, the argmin; whoever wants the runner-up (a behaviour layer that picks among the cheapest
 * survivors, a fallback when the winner is vetoed downstream, a visualiser that draws the best handful) would otherwise read back
 * both tables.  fp_rank_feasible ranks them on the device: cost_tbl / flag_tbl are [B][C] (C = nd*nv*nt) as fp_plan_dense wrote them.
 *   survivor   a candidate with no FP_FLAG_INFEASIBLE bit and a cost that is not NaN (`min_cost >= cost_final`,
 *              frenet_optimal_planner.py:266, never selects a NaN either).
 *   order      ascending cost; among equal costs the HIGHER flat index first - the order in which the "last minimum wins" loop
 *              (:263-268) would hand out winners if each winner were removed in turn.
 *   rank_idx   [K][B]  flat FOP index of the k-th cheapest survivor, -1 past the last one.
 *   rank_cost  [K][B]  its cost_tbl entry, bit for bit; NaN where rank_idx = -1.
 *   n_feasible NULL or [B]: the number of survivors of the ego (can exceed K).
 * Plane 0 is bit for bit best_idx / best_cost of the fp_plan_dense call that wrote the tables - with w_obstacle > 0 too (the tables then
 * hold the re-priced costs).  The one exception: an ego whose FP_AUDIT_NEAR_TIE bit is set when result.audit was requested, because
 * that path re-prices the tied candidates point by point and best_idx / best_cost are the outcome of those sums, not of the tables.
 * The layout is rank-major on purpose: rank_idx + k*B is a valid best_idx argument of fp_winner_trajs and fp_advance - the k-th
 * alternatives' series or hand-over need no new code and no gather.
 * An ego with batch->skip[b] != 0 has no table rows: its planes are -1 / NaN, its count 0, and its rows are not read.
 * FP_MEM_DEVICE: one kernel is enqueued (one workgroup per ego, in the order of batch->launch_order when there is one) - no
 * allocation, no wait; it can be captured behind a dense call.  FP_MEM_HOST stages the tables through the ctx and waits, like
 * fp_winner_trajs.  Of the batch only B and skip are used.  K < 1, K > FP_MAX_RANK or a NULL mandatory pointer: FP_EINVAL;
 * nd*nv*nt > FP_MAX_CAND: FP_ELIMIT.  Two calls on the same tables give the same bits.
 * Also read-only in fp_ctx_get_option: "rank_launches" = launches of the kernel on this ctx so far (0 for a caller that never asks). */
int fp_rank_feasible(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const double* cost_tbl, const uint32_t* flag_tbl,
                     int32_t K, int32_t* rank_idx, double* rank_cost, int32_t* n_feasible, int mem, void* stream);

/* ---- the road-boundary check (added WITHIN ABI 18: detect it by looking the symbol up, e.g. dlsym) --------------------
 * The reference declares the check - `check_boundary = True  # True if check collison with road boundaries`,
 * frenet_optimal_planner.py:56 - and never reads the setting.  The lattice confines only the END offset of a candidate to the road
 * width; nothing stops a candidate from swinging over the road edge on the way there (a large d_d or d at the start, a road narrower
 * than max_road_width).  fp_boundary_mask finishes it, behind fp_plan_dense and over its tables: cost_tbl / flag_tbl are [B][C]
 * (C = nd*nv*nt) as fp_plan_dense wrote them.  The road is a corridor in Frenet coordinates: one lateral offset per reference-line
 * knot and side (CommonRoad gives one bound vertex per centre vertex).
 *
 * Definition, for every candidate c of every ego b that is not skipped, N and M taken from the candidate's flag word:
 *   checked points   i = 1 .. M-1 of the trajectory.  Point 0 is the ego's present state, common to all candidates: it selects
 *                    nothing.  Points at or after M are off the reference line and have no frame.  M <= 1: nothing is checked, no bit.
 *   at point i       s, s_d, d, d_d = the candidate's series values at t = i * tick_t;
 *                    k = the segment index the Cartesian conversion uses for that s (bisect(knots, s) - 1), clamped to nx - 2;
 *                    u = (s - knots[k]) / (knots[k+1] - knots[k]).
 *   edges            L = left[k] + (left[k+1] - left[k]) * u, and R likewise from `right`.  A side whose two knot values are not both
 *                    finite is unbounded on that segment and cannot be violated there: +-inf is how a caller says "no edge here".
 *   half extent      r = hypot(s_d, d_d);  h = (veh_w / 2) |s_d| / r + (veh_l / 2) |d_d| / r, or veh_w / 2 when r == 0: the reach of
 *                    the veh_l x veh_w rectangle along the frame normal, its heading taken relative to the line as atan2(d_d, s_d).
 *                    The (1 - kappa d) factor of the exact heading is deliberately NOT applied.
 *   violation        d + h + margin > L   or   d - h - margin < R.
 *   the bit          FP_FLAG_BOUNDARY of the candidate's flag word is WRITTEN: set when any checked point violates, cleared otherwise
 *                    (two calls with two corridors leave the second one's verdicts).  No other bit of the word changes and cost_tbl is
 *                    never written.  The bit is independent of the other bits: it is evaluated for candidates that are already
 *                    infeasible too, like the constraint bits.
 *   best_idx / best_cost  [B] the argmin of cost_tbl over the candidates with no FP_FLAG_INFEASIBLE bit (which includes
 *                    FP_FLAG_BOUNDARY) and a cost that is not NaN; the last minimum in FOP order wins exact ties (:263-268); -1 / NaN when
 *                    there is none.  With w_obstacle > 0 the tables already hold the re-priced costs.  Bit for bit plane 0 of an
 *                    fp_rank_feasible call on the masked tables (which honours the bit through FP_FLAG_INFEASIBLE).
 *   n_masked         NULL or [B]: the candidates of the ego that carry the bit.
 *   Stats            do not change (FOP counts every candidate regardless).
 *   skipped egos     batch->skip[b] != 0: -1 / NaN / 0, the ego's rows are neither read nor written.
 * The kernel's series arithmetic (fma Horner) rounds differently from a point-by-point restatement: a candidate whose footprint comes
 * within ~FP_AUDIT_GAP_TOL of an edge may be decided either way by another rounding of the same numbers.
 *
 * FP_MEM_DEVICE: one kernel is enqueued (one workgroup per ego, in the order of batch->launch_order when there is one) - no
 * allocation, no wait; it can be captured directly behind a dense call in a linear chain.  FP_MEM_HOST stages the tables and the
 * corridor through the ctx and waits, like fp_rank_feasible.  Batch fields used: B, F, NX, nx, knots, frame_of, ego, d_samples,
 * t_samples, v_samples, skip, launch_order.  Rows k >= nx[f] of left / right are ignored.
 * Errors: a NULL mandatory pointer, margin negative or not finite, or (FP_MEM_HOST only) a NaN in a used row of left / right:
 * FP_EINVAL; nd*nv*nt > FP_MAX_CAND: FP_ELIMIT.  (A NaN a FP_MEM_DEVICE caller leaves in a used row makes its segments unbounded.)
 * Two calls on the same tables and corridor give the same bits.
 * Also read-only in fp_ctx_get_option: "boundary_launches" = launches of the kernel on this ctx so far (0 for a caller that never asks:
 * such a caller gets the bits and the launch counts it got before the symbol existed).
 *
 * Deliberately not done:
 *   - fp_plan_step and the FISS entry points take no corridor.  A closed loop that wants the check enqueues fp_plan_dense ->
 *     fp_boundary_mask -> fp_advance: the best_idx array is a valid argument of fp_advance (and fp_winner_trajs) as it stands.  FISS and
 *     FISS+ order candidates by cost BEFORE validation; where a boundary verdict belongs in those walks is a separate decision.
 *   - fp_shard_call has no slot for it. */
typedef struct {
    const double* left;    /* [F][NX] lateral offset (m, positive to the left) of the left road edge at every knot of the frame */
    const double* right;   /* [F][NX] the right edge (normally negative) */
    double margin;         /* extra distance kept from both edges, finite, >= 0 */
} fp_corridor;

int fp_boundary_mask(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_corridor* corridor, const double* cost_tbl,
                     uint32_t* flag_tbl, int32_t* best_idx, double* best_cost, int32_t* n_masked, int mem, void* stream);

/* ---- position-dependent speed limits and stop lines (added WITHIN ABI 18: detect it by looking the symbol up, e.g. dlsym) ----
 * The planner knows one speed limit, fp_params.max_speed: one number for the whole batch, line and horizon (`any(s_d > max_speed)`,
 * frenet_optimal_planner.py:152).  The reference's second caller receives more - the last column of its reference path holds, per
 * point, "0 is red light, 1 is crosswalk, other is speed_limi[t]" (planners/waymo_interface/waymo_interface.py:160-189) - and hands the
 * planner `np.amax(ref_path[:, -1])`, the largest value anywhere on the path: a 30 km/h zone, a red light 60 m ahead and a bend that
 * cannot be taken at 13 m/s all look the same to the lattice.  fp_speed_envelope finishes it, behind fp_plan_dense and over its tables:
 * cost_tbl / flag_tbl are [B][C] (C = nd*nv*nt) as fp_plan_dense wrote them.
 *
 * Definition, for every candidate c of every ego b that is not skipped, N and M taken from the candidate's flag word:
 *   checked points   i = 1 .. M-1 of the trajectory.  Point 0 is the ego's present state, common to all candidates: it selects
 *                    nothing.  M <= 1: nothing is checked, no bit is set.
 *   at point i       s, s_d = the candidate's longitudinal series values at t = i * tick_t (rows FP_ARR_S, FP_ARR_S_D); f = frame_of[b].
 *   speed limit      s_q = s + front;  k_q = bisect_right(knots, s_q) - 1, clamped to 0 .. nx-2;  lim = v_limit[f][k_q].
 *                    Violation A: s_d > lim + tol (never for lim = +inf).  A stop line or a red light is a stretch of segments with
 *                    lim = 0: a candidate that is at rest (s_d <= tol) before s + front reaches the stretch survives, every other one
 *                    violates.
 *   lateral accel.   only when max_lat_accel > 0:  k = the segment index the Cartesian conversion uses for s, clamped to nx-2 (as in
 *                    fp_boundary_mask);  dx = s - knots[k];  x' = bx + 2 cx dx + 3 dx_ dx^2,  x'' = 2 cx + 6 dx_ dx, and y', y''
 *                    likewise (bx, cx, dx_ = rows 1, 2, 3 of coef; rows 5, 6, 7 for y);
 *                    kappa_r = (x' y'' - y' x'') / (x'^2 + y'^2)^1.5, the curvature of the REFERENCE LINE at s.
 *                    Violation B: s_d * s_d * |kappa_r| > max_lat_accel.  The (1 - kappa d) factor and d_dd are deliberately NOT
 *                    applied - the same choice fp_boundary_mask made for its heading.
 *   the bits         violation A at any checked point ORs FP_FLAG_SPEED into the candidate's flag word, violation B FP_FLAG_ACCEL.  The
 *                    low byte of the flag word is full, and these two bits already mean "too fast somewhere" and "too much acceleration
 *                    somewhere": the envelope refines what is allowed.  The call NEVER CLEARS a bit - the lattice's own verdict lives in
 *                    the same bits - so it is idempotent; a caller who wants another envelope runs the dense call again or keeps a copy
 *                    of flag_tbl.  No other bit changes and cost_tbl is never written.  Candidates that are already infeasible are
 *                    evaluated too.
 *   best_idx / best_cost  [B] the argmin of cost_tbl over the candidates with no FP_FLAG_INFEASIBLE bit and a cost that is not NaN; the
 *                    last minimum in FOP order wins exact ties (:263-268); -1 / NaN when there is none.  Bit for bit plane 0 of an
 *                    fp_rank_feasible call on the masked tables, and a valid argument of fp_advance, fp_winner_trajs, fp_traj_margins;
 *                    the masked tables are valid arguments of fp_boundary_mask.
 *   n_limited        NULL or [B]: the candidates of the ego with violation A or B in THIS call, whatever bits they carried before.
 *   Stats            do not change (FOP counts every candidate regardless).
 *   skipped egos     batch->skip[b] != 0: -1 / NaN / 0, the ego's rows are neither read nor written.
 * s, s_d and M depend on the candidate's longitudinal profile (i_v, i_T) alone (calc_global_paths stops at the first s off the line,
 * :112-113), so the nd candidates of a profile share one verdict; the kernel evaluates nv*nt profiles per ego, not nd*nv*nt candidates.
 * Its series arithmetic (fma Horner) rounds differently from a point-by-point restatement: a point with s_d within ~FP_AUDIT_GAP_TOL
 * of its threshold may be decided either way by another rounding of the same numbers, and so may a point with s_q within that of a
 * knot where the limit changes.
 *
 * FP_MEM_DEVICE: one kernel is enqueued (one workgroup per ego, in the order of batch->launch_order when there is one) - no
 * allocation, no wait; it can be captured directly behind a dense call in a linear chain.  FP_MEM_HOST stages the tables and the
 * profile through the ctx and waits, like fp_boundary_mask.  Batch fields used: B, F, NX, nx, knots, coef (only when
 * max_lat_accel > 0), frame_of, ego, t_samples, v_samples, skip, launch_order.
 * Errors: a NULL mandatory pointer (profile, v_limit, cost_tbl, flag_tbl, best_idx, best_cost; coef when max_lat_accel > 0), front /
 * tol negative or not finite, max_lat_accel negative or not finite: FP_EINVAL; (FP_MEM_HOST only) a NaN or a negative value in a used
 * entry of v_limit: FP_EINVAL, the message names frame and knot; nd*nv*nt > FP_MAX_CAND: FP_ELIMIT.  A NaN a FP_MEM_DEVICE caller
 * leaves in a used entry compares false: it means "no limit there" (a negative entry violates at every speed above it).
 * Also read-only in fp_ctx_get_option: "envelope_launches" = launches of the kernel on this ctx so far (0 for a caller that never asks:
 * such a caller gets the bits and the launch counts it got before the symbol existed).
 *
 * Deliberately not done:
 *   - fp_plan_step and the FISS entry points take no profile.  A closed loop that wants the envelope enqueues fp_plan_dense ->
 *     fp_speed_envelope -> fp_advance.
 *   - fp_shard_call has no slot for it.
 * The profile is a function of s alone; a stop line that opens and closes with time (a light that turns green) is a gate: fp_gate_mask
 * below. */
typedef struct {
    const double* v_limit;  /* [F][NX] speed limit (m/s) of the SEGMENT that starts at knot k: it holds on knots[k] <= s < knots[k+1].
                               +inf = no limit there.  Entries k >= nx[f] - 1 are ignored. */
    double front;           /* >= 0, finite: the limit is read at s + front (veh_l / 2 = the front bumper obeys the sign / stop line) */
    double tol;             /* >= 0, finite: a point violates when s_d > limit + tol */
    double max_lat_accel;   /* 0 = off; > 0 finite: a point violates when s_d^2 |kappa_r(s)| > max_lat_accel, kappa_r = curvature of the reference line */
} fp_speed_profile;

int fp_speed_envelope(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_speed_profile* profile,
                      const double* cost_tbl, uint32_t* flag_tbl, int32_t* best_idx, double* best_cost, int32_t* n_limited,
                      int mem, void* stream);

/* ---- stop lines that open and close: gates (added WITHIN ABI 18: detect it by looking the symbol up, e.g. dlsym) ------------------
 * fp_speed_envelope models a red light as a stretch of zero speed limit, a function of s alone: the light never turns green, and an ego
 * that obeys it in a closed loop waits for ever.  The reference's data says what kind of line it is - "0 is red light, 1 is crosswalk"
 * (planners/waymo_interface/waymo_interface.py:160-189) - and not when it holds.  A GATE is a stop line at an arclength of a reference
 * line with a state per absolute time step: a traffic light with phases, a crossing while a pedestrian is predicted on it, a barrier.
 * The time index is the obstacle table's own clock, t_now[b] + i.  fp_gate_mask runs behind fp_plan_dense and over its tables: cost_tbl /
 * flag_tbl are [B][C] (C = nd*nv*nt) as fp_plan_dense wrote them.
 *
 * Definition, for every candidate c of every ego b that is not skipped, N and M taken from the candidate's flag word, f = frame_of[b]:
 *   points           q_0 = ego[b][0] + front, computed exactly so (not from the series);  q_i = s_i + front for i = 1 .. M-1, s_i = the
 *                    candidate's longitudinal series value (row FP_ARR_S) at t = i * tick_t.  M <= 1: nothing is checked, no bit is set.
 *   crossing         the candidate crosses gate g at point i (1 <= i <= M-1) when  q_{i-1} <= gate_s[f][g]  &&  gate_s[f][g] < q_i.
 *                    A NaN slot compares false.  An ego whose bumper is already past the line (q_0 > gate_s) never crosses it: it is in
 *                    the junction and must clear it.
 *   gate state       read at the arrival step:  w = closed[f][clamp(t_now[b] + i, 0, T_gate - 1)]  (before step 0 the first, at or
 *                    after T_gate the last known state holds).
 *   waiver           only when max_decel > 0.  Gate g is waived for ego b when, with v0 = ego[b][1]:  v0 > 0,  q_0 <= gate_s[f][g]  and
 *                    q_0 + v0 * v0 / (2 * max_decel) > gate_s[f][g]:  the ego cannot stop in front of the line any more (the dilemma
 *                    zone: without the rule such an ego would be left without a plan).
 *   violation        a crossing at i of a gate that is not waived and whose bit g is set in w.
 *   the bit          a violating candidate gets FP_FLAG_SPEED ORed into its flag word - the bit fp_speed_envelope gives a candidate
 *                    that runs its static red light; the low byte of the flag word is full.  The call NEVER CLEARS a bit and changes
 *                    no other bit, so it is idempotent; cost_tbl is never written.  Candidates that are already infeasible are
 *                    evaluated too.
 *   best_idx / best_cost  [B] the argmin of cost_tbl over the candidates with no FP_FLAG_INFEASIBLE bit and a cost that is not NaN; the
 *                    last minimum in FOP order wins exact ties (:263-268); -1 / NaN when there is none.  Bit for bit plane 0 of an
 *                    fp_rank_feasible call on the masked tables, and a valid argument of fp_advance, fp_winner_trajs, fp_traj_margins;
 *                    the masked tables are valid arguments of fp_boundary_mask and fp_speed_envelope.
 *   n_gated          NULL or [B]: the candidates of the ego that violate in THIS call, whatever bits they carried before.
 *   Stats            do not change (FOP counts every candidate regardless).
 *   skipped egos     batch->skip[b] != 0: -1 / NaN / 0, the ego's rows are neither read nor written.
 * s_i and M depend on the candidate's longitudinal profile (i_v, i_T) alone, so the nd candidates of a profile share one verdict; the
 * kernel evaluates nv*nt profiles per ego.  Its series arithmetic (fma Horner) rounds differently from a point-by-point restatement: a
 * point with q_i within ~FP_AUDIT_GAP_TOL of a line may be decided either way by another rounding of the same numbers (q_0 and the
 * waiver's left side are computed as written above on every side).
 *
 * FP_MEM_DEVICE: one kernel is enqueued (one workgroup per ego, in the order of batch->launch_order when there is one) - no
 * allocation, no wait; it can be captured directly behind a dense call in a linear chain.  t_now, ego, closed and gate_s are read when
 * the kernel runs: a replayed graph follows a loop whose t_now advances on the device (fp_advance), and a caller may rewrite the
 * phases in place between cycles.  params->points_max announces the points per trajectory as for every FP_MEM_DEVICE call.
 * FP_MEM_HOST stages the tables and the gates through the ctx and waits, like fp_speed_envelope.  Batch fields used: B, F, frame_of,
 * ego, t_now, t_samples, v_samples, skip, launch_order (NX, nx, knots travel with a host call and are not read).
 * Errors: a NULL mandatory pointer (gates, gate_s, closed, cost_tbl, flag_tbl, best_idx, best_cost), gate_stride outside
 * 1 .. FP_MAX_GATES, T_gate < 1, front or max_decel negative or not finite: FP_EINVAL; nd*nv*nt > FP_MAX_CAND: FP_ELIMIT.  Bits of a
 * closed word at or above gate_stride are ignored.
 * Also read-only in fp_ctx_get_option: "gate_launches" = launches of the kernel on this ctx so far (0 for a caller that never asks: such
 * a caller gets the bits and the launch counts it got before the symbol existed).
 *
 * Deliberately not done:
 *   - fp_plan_step, the FISS entry points and fp_shard_call take no gates.  A closed loop enqueues fp_plan_dense -> fp_gate_mask ->
 *     fp_advance (ClosedLoopRunner(rules=...) of the Python package does, eagerly or from a graph).
 *   - the waiver looks at the ego's present speed alone; a yellow phase is the caller's: it closes the gate's bit from the step the
 *     light turns red and sets max_decel to the braking it asks of a driver. */
typedef struct {
    const double*   gate_s;   /* [F][gate_stride]  arclength of the stop line on the frame; NaN = unused slot */
    const uint32_t* closed;   /* [F][T_gate]       bit g set = gate g of the frame is closed at absolute time step t */
    int32_t gate_stride;      /* 1 .. FP_MAX_GATES */
    int32_t T_gate;           /* >= 1; steps before 0 read row 0, steps at or after T_gate read row T_gate-1 (the last known state holds) */
    double  front;            /* >= 0, finite: the line is crossed by s + front (veh_l / 2 = the front bumper) */
    double  max_decel;        /* 0 = off; > 0 finite: a gate the ego can no longer stop in front of is waived (above) */
} fp_gates;

int fp_gate_mask(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_gates* gates, const double* cost_tbl,
                 uint32_t* flag_tbl, int32_t* best_idx, double* best_cost, int32_t* n_gated, int mem, void* stream);

/* ---- a time gap to moving obstacles (added WITHIN ABI 18: detect it by looking the symbol up, e.g. dlsym) -------------------------
 * What decides how close an ego gets to another vehicle is has_collision alone: a plan that passes a hand's width behind a car doing
 * 12 m/s is as feasible as one 40 m back, and so is one that pulls out just in front of a faster car.  The reference has no such rule;
 * like the gates and the envelope this finishes what its planner leaves to luck.  A time gap of tau seconds means: the ego does not
 * occupy a place an obstacle occupied less than tau seconds earlier (FOLLOW), and no obstacle reaches a place the ego occupied less
 * than tau seconds earlier (LEAD: the ego does not cut in front of it).  That is the post-encroachment time on the candidate's own
 * path - it bends with the road, scales with speed, works for crossing traffic - and it is the collision check with the two time
 * indices apart.  It is silent for parked obstacles: a shape that does not move is overlapped at a lag exactly when it is overlapped at
 * lag 0, which is the collision check's business.  fp_gap_mask runs behind fp_plan_dense (or another pass) and over its tables:
 * cost_tbl / flag_tbl are [B][C] (C = nd*nv*nt).
 *
 * Definition, for every ego b that is not skipped and every candidate c of it that carries NO FP_FLAG_INFEASIBLE bit on entry
 * (candidates that are already infeasible are not evaluated and keep their words); N and M from the flag word, cs = check_stride:
 *   pose set P       { i = 0, cs, 2 cs, ... : i < min(M, final_time_step[scene] - t_now[b]) and 0 <= i + t_now[b] < T_obs }:
 *                    has_collision's own pose set, as in the clearance term and fp_traj_margins.  M < 2: no pose, no bit.
 *   pairs            (a, r) with a, r in P and a >= first, and either 0 < a - r <= lag_follow (the ego at point a against the
 *                    obstacles at step r: the ego arrives later) or 0 < r - a <= lag_lead (the obstacle arrives later).  Both lags are
 *                    in steps of tick_t; only pairs on the check grid exist.  first >= 1 is the grace: an ego that is already too
 *                    close gets `first` steps to open the gap (point 0 selects nothing anyway).  Any value up to INT32_MAX is legal:
 *                    `first` >= FP_MAX_POINTS lies beyond every pose and flags nothing (it is read as FP_MAX_POINTS).
 *   ego shape        the veh_l x veh_w rectangle at x[a], y[a], yaw[a] of the candidate's series.
 *   obstacle shape   the columns j of the ego's scene with valid != 0 at row r + t_now[b]; the rectangle of obs_dims, or the column's
 *                    ring (obs_poly / obs_nvert), at that row's pose.
 *   violation        the two closed shapes intersect for any such pair and column - the collision check's own predicates, so touching
 *                    counts.
 *   the bit          a violating candidate gets FP_FLAG_COLLISION ORed into its flag word: the low byte is full, and the bit already
 *                    means "too close to an obstacle" (the choice the gates made with FP_FLAG_SPEED).  The call NEVER CLEARS a bit and
 *                    touches no other bit; cost_tbl is never written; Stats do not change.  A second call on the masked tables changes
 *                    nothing and reports n_close = 0: its violators are no longer evaluated.
 *   best_idx / best_cost  [B] the argmin of cost_tbl over the candidates with no FP_FLAG_INFEASIBLE bit and a cost that is not NaN; the
 *                    last minimum in FOP order wins exact ties (:263-268); -1 / NaN when there is none.  Bit for bit plane 0 of an
 *                    fp_rank_feasible call on the masked tables, and a valid argument of fp_advance, fp_winner_trajs, fp_traj_margins.
 *   n_close          NULL or [B]: the candidates of the ego that violate in THIS call.
 *   skipped egos     batch->skip[b] != 0: -1 / NaN / 0, the ego's rows are neither read nor written.
 *   no scene         an ego with scene_of < 0, or a batch with n_obs == 0: nothing is flagged, the argmin is that of the tables as they are.
 * Both lags 0 is legal and flags nothing; so does a lag below check_stride.
 * Rounding: the kernel's pose arithmetic rounds differently from a point-by-point restatement: a pair within ~FP_AUDIT_GAP_TOL of
 * touching may be decided either way.
 * Sampling: pairs exist on the check grid only, so the lag is sampled every cs * tick_t seconds.  That leaves no hole while the ego moves
 * less than veh_l per grid step - with cs = 2 and tick_t = 0.1 s that is 22 m/s for a 4.5 m car; a faster ego can step over a place an
 * obstacle held between two samples.
 *
 * FP_MEM_DEVICE: one kernel is enqueued (one workgroup per ego, in the order of batch->launch_order when there is one) - no
 * allocation, no wait; it can be captured directly behind a dense call or another pass in a linear chain.  t_now, ego and the obstacle
 * table are read when the kernel runs: a replayed graph follows a loop whose state advances on the device (fp_advance).
 * params->points_max announces the points per trajectory as for every FP_MEM_DEVICE call.  FP_MEM_HOST stages the batch and the tables
 * through the ctx and waits, like fp_gate_mask.  The result depends neither on launch_order nor on the memory space; two calls on the
 * same tables give the same bits.
 * Errors: a NULL mandatory pointer (gap, cost_tbl, flag_tbl, best_idx, best_cost), a negative lag, a lag above FP_MAX_POINTS, first < 1:
 * FP_EINVAL; nd*nv*nt > FP_MAX_CAND: FP_ELIMIT.
 * Also read-only in fp_ctx_get_option: "gap_launches" = launches of the kernel on this ctx so far (0 for a caller that never asks).
 *
 * Deliberately not done: fp_plan_step does not call it, the FISS entry points do not call it, and fp_shard_call has no slot for it.  A
 * closed loop enqueues fp_plan_dense -> (other passes) -> fp_gap_mask -> fp_advance (ClosedLoopRunner(rules=("gaps",)) of the Python
 * package does, eagerly or from a graph). */
typedef struct {
    int32_t lag_follow;  /* >= 0 steps: the ego may not be where an obstacle was up to this many steps earlier */
    int32_t lag_lead;    /* >= 0 steps: an obstacle may not be where the ego was up to this many steps earlier */
    int32_t first;       /* >= 1: ego points before this one are not checked (>= FP_MAX_POINTS: none is) */
    int32_t reserved0;
} fp_time_gap;

int fp_gap_mask(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_time_gap* gap, const double* cost_tbl,
                uint32_t* flag_tbl, int32_t* best_idx, double* best_cost, int32_t* n_close, int mem, void* stream);

/* ---- the rules on explicit end states (added WITHIN ABI 18: detect it by looking the symbol up, e.g. dlsym) -------------------------
 * fp_speed_envelope, fp_gate_mask, fp_boundary_mask and fp_gap_mask are table passes: a trajectory has a rule verdict only as a lattice
 * candidate of a dense call.  What fp_plan_fiss hands back - an end state (d, v, T) that refinement has moved off the lattice - and
 * every trajectory a caller makes itself (fp_eval_trajs, fp_traj_margins, fp_advance take them) has none.  fp_rules_eval evaluates the
 * same four definitions on K explicit end states per ego.  It prices nothing and chooses nothing.
 *
 * Definition, for every ego b that is not skipped and every trajectory k < K:
 *   trajectory       the one fp_eval_trajs builds for end_states[b][k] = (d, v, T).
 *   N, M             from flags[b][k] ON ENTRY - fp_eval_trajs' flag word of the same end state (or fp_plan_fiss' best_flags, K = 1) -,
 *                    as the passes take them from the table's flag word.
 *   rules            the rules whose pointer in fp_rule_set is not NULL, in the passes' order: envelope, gates, boundary, gaps.  Each
 *                    is its own pass' definition above, word for word (checked points, thresholds, the gates' waiver from the ego's
 *                    present state, the gaps' pose set and pairs), with "candidate" read as "trajectory".
 *   the bits         envelope: ORs FP_FLAG_SPEED (violation A) / FP_FLAG_ACCEL (violation B).  gates: OR FP_FLAG_SPEED.  boundary:
 *                    WRITES FP_FLAG_BOUNDARY, set or cleared.  gaps: OR FP_FLAG_COLLISION, and only a trajectory whose word carries no
 *                    FP_FLAG_INFEASIBLE bit after the rules before it IN THIS CALL is evaluated (fp_gap_mask's entry condition behind
 *                    the other passes).  No other bit changes.
 *   equivalence      on the lattice's own end states (d_samples[i_d], v_samples[b][i_v], t_samples[i_t]) and their flag words the call
 *                    leaves the words the chain fp_speed_envelope -> fp_gate_mask -> fp_boundary_mask -> fp_gap_mask leaves in a
 *                    dense call's table: the kernels share the predicates (same arithmetic, same bits).
 *   rule_bits        NULL or [B][K] out: the FP_RULE_* of the rules the trajectory violates in THIS call, whatever bits it carried
 *                    before.  The flag bits are shared - FP_FLAG_SPEED comes from the envelope or from a gate -: a report needs the rule.
 *   counts           NULL or [B][FP_RULE_COUNT] in/out: entry log2(FP_RULE_x) of row b grows by the trajectories of ego b that violate
 *                    rule x in this call.  A loop that passes the same array every cycle accumulates violations per ego and rule.
 *   nothing checked  a NaN in the end state, M <= 1, or batch->skip[b] != 0: the word is unchanged, rule_bits is 0, nothing is counted.
 * A second call on the words the first one left changes no word: the boundary bit is written to the same value, the OR bits stay; the
 * gaps no longer evaluate their own violators, so that call's rule_bits lack FP_RULE_GAP for them.  Two calls on the same inputs give
 * the same bits; the result depends neither on batch->launch_order nor on the memory space.  The rounding notes of the four passes hold
 * here too.
 *
 * FP_MEM_DEVICE: one kernel is enqueued (one workgroup per ego, in the order of batch->launch_order when there is one) - no
 * allocation, no wait; it can be captured behind fp_plan_fiss in a linear chain (fp_plan_fiss -> fp_rules_eval -> fp_advance: the
 * verdict is taken before the hand-over moves ego / t_now).  t_now, ego, the gate phases and the obstacle table are read when the kernel
 * runs.  A row of `counts` is read, added to and stored by the ego's workgroup alone (no atomics).  K has no compiled-in cap.
 * params->points_max announces the points per trajectory as for every FP_MEM_DEVICE call.
 * FP_MEM_HOST stages the batch, the arrays of the rules that are on, end_states, flags (in/out), rule_bits (out) and counts (in/out)
 * through the ctx and waits, like fp_gap_mask.
 * Errors: K < 1, a NULL rules / end_states / flags, or all four rules NULL: FP_EINVAL; for every rule that is on, its own pass' argument
 * errors with the pass' messages; (FP_MEM_HOST only) an end state of an ego that is not skipped whose T needs more than FP_MAX_POINTS
 * points: FP_ELIMIT - FP_MEM_DEVICE treats such a trajectory (and one that needs more points than the call is sized for) as having
 * none: nothing is checked.
 * Also read-only in fp_ctx_get_option: "rules_eval_launches" = launches of the kernel on this ctx so far (0 for a caller that never asks).
 *
 * Deliberately not done: fp_plan_fiss does not call it - where a verdict belongs INSIDE the FISS walks remains the separate decision the
 * passes name, and this call is what it needs first -; fp_shard_call has no slot for it; there is no lattice-index input (an index has
 * no flag word outside a table: a caller with tables runs the passes). */
#define FP_RULE_LIMIT    1u   /* fp_speed_envelope violation A */
#define FP_RULE_LATERAL  2u   /* fp_speed_envelope violation B */
#define FP_RULE_GATE     4u
#define FP_RULE_BOUNDARY 8u
#define FP_RULE_GAP      16u
#define FP_RULE_COUNT    5

typedef struct {              /* each NULL = that rule is off; all four NULL: FP_EINVAL */
    const fp_speed_profile* envelope;
    const fp_gates*         gates;
    const fp_corridor*      boundary;
    const fp_time_gap*      gaps;
} fp_rule_set;

int fp_rules_eval(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_rule_set* rules, int32_t K,
                  const double* end_states,  /* [B][K][3] = (d, v, T): fp_eval_trajs' layout */
                  uint32_t* flags,           /* [B][K] in/out: fp_eval_trajs' flag words (N, M and the bits so far) */
                  uint32_t* rule_bits,       /* NULL or [B][K] out: FP_RULE_* violated in THIS call */
                  int32_t* counts,           /* NULL or [B][FP_RULE_COUNT] in/out */
                  int mem, void* stream);

/* ---- the obstacle margin of chosen plans (added WITHIN ABI 18: detect it by looking the symbol up, e.g. dlsym) ------------
 * fp_rank_feasible hands a behaviour layer K alternatives per ego as an index and a cost.  How close each of them comes to anything,
 * when, and to what, is not in either number: a plan without FP_FLAG_COLLISION may pass 2 cm from a truck or 6 m from it, and it may
 * even touch an obstacle at a pose has_collision never looks at (it checks every check_stride-th pose).  fp_traj_margins answers on
 * the device, for K chosen plans per ego, against the obstacle table that is already resident.  It prices nothing and changes nothing.
 *
 * Definition, for plane k < K and ego b:
 *   trajectory   the series fp_winner_trajs would write for best_idx[k][b] (a flat FOP index), or fp_eval_trajs for the end state
 *                end_state[k][b] = (d, v, T); its points are 0 .. M-1, with x, y and yaw from the series.  M < 2: the series has no
 *                heading, hence no pose.
 *   poses        i = 0, pose_stride, 2 pose_stride, ... < min(M, final_time_step[scene] - t_now[b]) with 0 <= i + t_now[b] < T_obs;
 *                each pose is the veh_l x veh_w rectangle at point i.  pose_stride = params->check_stride reproduces has_collision's
 *                pose set (and the clearance term's), 1 looks at every pose.  params->check_stride itself is not used.
 *   obstacles    the columns j of the ego's scene with a valid pose (valid != 0) at row i + t_now[b]; the shape is the rectangle of
 *                obs_dims, or the column's ring (obs_poly / obs_nvert).
 *   dist(i, j)   the Euclidean distance between the two shapes, 0 on contact (touching counts): the clearance term's distance.
 *   min_dist     [K][B] the minimum of dist over all pairs; +inf when there is no pair (scene_of < 0, n_obs == 0, no pose in the
 *                horizon, no valid column); NaN when there is no trajectory (index < 0, a NaN in the end state, more points than the
 *                call is sized for - what makes fp_winner_trajs write a NaN series -, or batch->skip[b] != 0: such an ego's rows are
 *                not read).
 *   min_step, min_obs  [K][B] the point index i and the column j of the minimum.  Among equal distances the smallest i wins, then the
 *                smallest j: for a plan in contact this is the first contact.  -1, -1 when min_dist is +inf or NaN.
 * The layout is rank-major like fp_rank_feasible's: its rank_idx array is a valid best_idx argument with the same K, and the best_idx
 * array of fp_plan_dense / fp_boundary_mask with K = 1.  end_state takes what fp_advance takes: the refined winners of fp_plan_fiss.
 * Two calls give the same bits; the result depends neither on batch->launch_order nor on the memory space.  The kernel's arithmetic
 * rounds differently from a restatement of the definition: distances agree to ~1e-12 m, and a contact within ~FP_AUDIT_GAP_TOL may be
 * decided either way.  With pose_stride = check_stride the contact verdicts are the collision check's own (same arithmetic).
 *
 * FP_MEM_DEVICE: one kernel is enqueued (one workgroup per ego, in the order of batch->launch_order when there is one) - no
 * allocation, no wait; it can be captured behind fp_plan_dense -> fp_rank_feasible.  FP_MEM_HOST stages the batch through the ctx
 * and waits, like fp_winner_trajs.
 * Errors: K < 1, K > FP_MAX_RANK, pose_stride < 1, both or neither of best_idx / end_state, a NULL output: FP_EINVAL.  The compiled-in
 * limits answer as they do for fp_winner_trajs (FP_ELIMIT).  FP_MEM_HOST refuses an index >= nd*nv*nt of an ego that is not skipped
 * (FP_EINVAL, naming ego and plane) and an end state whose T needs more than FP_MAX_POINTS points (FP_ELIMIT); FP_MEM_DEVICE treats
 * both as "no trajectory".
 * Also read-only in fp_ctx_get_option: "margin_launches" = launches of the kernel on this ctx so far (0 for a caller that never asks).
 * Deliberately not done: no fp_shard_call slot, no loop-log columns, nothing inside fp_plan_step (a loop enqueues the call behind its
 * plan call). */
int fp_traj_margins(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, int32_t K,
                    const int32_t* best_idx,     /* NULL or [K][B] */
                    const double* end_state,     /* NULL or [K][B][3] */
                    int32_t pose_stride,         /* >= 1 */
                    double* min_dist,            /* [K][B] */
                    int32_t* min_step,           /* [K][B] */
                    int32_t* min_obs,            /* [K][B] */
                    int mem, void* stream);

/* ---- a stopping manoeuvre for the egos without a plan (added WITHIN ABI 18: detect it by looking the symbol up, e.g. dlsym) ------
 * Every planner here answers "no solution" with best_idx = -1 / a NaN end state, and fp_advance then ends the ego with
 * FP_DONE_NO_SOLUTION: its next state is never computed.  Every rule pass removes more candidates, so in a resident closed loop an
 * ego whose candidates are all flagged leaves the simulation at full speed.  fp_fallback_stop gives such an ego a degraded answer: it
 * brakes to a stop along the lane; if contact can no longer be avoided the contact comes as late as possible; and it keeps planning,
 * so the ego drives on when the road clears.  The egos that have a plan pay one early return.
 *
 * need(b)      batch->skip[b] == 0 and: best_idx given and best_idx[b] < 0; or best_idx NULL and end_state[b][0] is NaN (what
 *              fp_plan_fiss leaves for an ego without a trajectory).
 * family       candidate f = i_d * n_stop + i_T is the explicit end state (d_targets[i_d], or the ego's own d0 when that entry is NaN;
 *              v = 0; stop_T[i_T]) - exactly the trajectory fp_eval_trajs builds for it: a longitudinal quartic to v = 0, s_dd = 0 at T,
 *              a lateral quintic to the offset with zero end derivatives, N = len(arange(0, T, tick_t)) series points, M = the first
 *              point off the reference line.
 * admissible   N <= the points the call is sized for (FP_FAST_POINTS, or params->points_max) and M >= 2 and, at every series point
 *              i < N, s_d[i] >= -FP_FALLBACK_REVERSE_TOL (the ego never reverses: v0 = 5, a0 = -4, T = 6 passes through -0.5 m/s) and
 *              -s_dd[i] <= max_decel.
 * first contact  over the collision check's own pose set, i = 0, check_stride, ... < min(M, final_time_step - t_now) with
 *              0 <= i + t_now < T_obs: hit_step = the smallest i at which the footprint intersects a valid column, hit_obs = the smallest
 *              such column at that pose, hit_speed = s_d[hit_step]; -1, -1, NaN without contact.  The predicate is the collision check's
 *              own: fp_traj_margins(end_state, pose_stride = check_stride) has min_dist == 0 exactly when there is a hit, and names the
 *              same step and column; fp_eval_trajs sets FP_FLAG_COLLISION exactly then.
 * choice       among the admissible candidates only; every key is an integer or one exact IEEE operation on inputs, so two
 *              implementations of the definition agree bit for bit:
 *                1. a candidate without contact beats one with contact;
 *                2. among candidates without contact the larger i_T wins (the gentlest stop);
 *                3. among candidates with contact the larger hit_step wins (the latest contact), then the smaller i_T (brake hardest);
 *                4. then the smaller fabs(d_end - d0);  5. then the smaller i_d.
 * outputs, need(b):  status[b] = FP_FALLBACK_CLEAR / _CONTACT / _NONE (no admissible candidate); fb_idx[b] = f, or -1 for NONE;
 *              end_state[b] = the chosen (d, 0, T), or three NaN for NONE; hit_step / hit_obs / hit_speed as above;
 *              cand[b][f] = -2 inadmissible, -1 clear, else the candidate's first hit step; counts[b][status] += 1.
 * outputs, no need:  status 0, fb_idx -1, hit_step / hit_obs / hit_speed -1, -1, NaN, cand untouched, counts[b][0] += 1.  With best_idx
 *              given, end_state[b] becomes the lattice sample's (d_samples[i_d], v_samples[b][i_v], t_samples[i_T]), decoded as
 *              fp_advance decodes it; with best_idx NULL it is untouched.
 * outputs, skipped ego:  status 0 and the "none" values (counts[b][0] += 1); end_state becomes NaN when best_idx is given and is
 *              untouched otherwise.  None of its rows is read.
 * After the call end_state is "the plan every ego drives": a valid argument of fp_advance, fp_loop_record, fp_eval_trajs,
 * fp_traj_margins and fp_rules_eval.
 *
 * FP_MEM_DEVICE: one kernel is enqueued (one workgroup per ego, in the order of batch->launch_order when there is one) - nothing is
 * allocated, nothing waited for, the call can be captured.  The result does not depend on launch_order, and two runs give the same
 * bits.  FP_MEM_HOST stages the batch and the call's arrays through the ctx and waits, like fp_traj_margins.
 * Errors, all before any launch: a NULL fallback / d_targets / stop_T / end_state / status / fb_idx / hit_step / hit_obs / hit_speed,
 * n_d < 1, n_stop < 1: FP_EINVAL; n_d * n_stop > FP_MAX_FALLBACK: FP_ELIMIT; max_decel not positive or NaN: FP_EINVAL.  FP_MEM_HOST
 * also refuses a stop_T entry that is not finite, not positive or not above its predecessor (FP_EINVAL, the entry named), one that
 * needs more than FP_MAX_POINTS points (FP_ELIMIT; on the device such a candidate is inadmissible) and a best_idx >= nd*nv*nt of an
 * ego that is not skipped (FP_EINVAL, as fp_advance answers; on the device such an ego gets a NaN end state).
 * Also read-only in fp_ctx_get_option: "fallback_launches" = launches of the kernel on this ctx so far (0 for a caller that never asks).
 * The rules: fp_fallback_stop itself looks at no rule pass - a stop may end across a stop line.  fp_fallback_stop_rules (below) is the
 * call that ranks the clear stops by the rule set.
 * Deliberately not done:
 *   - the footprint's heading is the series' own yaw, the difference quotient of calc_global_paths: an ego that stands from the first
 *     point has yaw 0, as every lattice candidate at v = 0 already has in every entry point - changing that is a change to all of them;
 *   - no fp_shard_call slot, nothing inside fp_plan_step / fp_plan_fiss_step (a loop enqueues plan, fp_fallback_stop, fp_advance),
 *     no per-row marker in the loop log. */
#define FP_MAX_FALLBACK 256          /* n_d * n_stop */
#define FP_FALLBACK_REVERSE_TOL 1e-6 /* m/s */
enum { FP_FALLBACK_NOT_NEEDED = 0, FP_FALLBACK_CLEAR = 1, FP_FALLBACK_CONTACT = 2, FP_FALLBACK_NONE = 3 };

typedef struct {
    int32_t n_d, n_stop;
    const double* d_targets;  /* [n_d]    lateral end offsets; a NaN entry = the ego's own d0 (stay where you are) */
    const double* stop_T;     /* [n_stop] stop times in seconds, strictly ascending, > 0 */
    double max_decel;         /* > 0, +inf = no limit */
} fp_fallback;

int fp_fallback_stop(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_fallback* fallback,
                     const int32_t* best_idx,   /* NULL or [B] */
                     double* end_state,         /* [B][3] in/out */
                     int32_t* status,           /* [B] */
                     int32_t* fb_idx,           /* [B] */
                     int32_t* hit_step, int32_t* hit_obs, double* hit_speed,   /* [B] each */
                     int32_t* cand,             /* NULL or [B][n_d * n_stop] */
                     int32_t* counts,           /* NULL or [B][4] in/out */
                     int mem, void* stream);

/* ---- the stopping manoeuvre that obeys the road rules (added WITHIN ABI 18: detect it by looking the symbol up, e.g. dlsym) ----------
 * The rule passes are the main producer of egos without a plan: an ego whose every candidate is flagged by fp_speed_envelope,
 * fp_gate_mask, fp_boundary_mask, fp_gap_mask or the enforced FISS walks gets best_idx = -1, and fp_fallback_stop then prefers the
 * gentlest clear stop - the one most likely to roll over the line the gate has just closed.  fp_fallback_stop_rules is
 * fp_fallback_stop with one more key in its choice: the verdict of the rule set on every clear candidate.
 *
 * Unchanged: need(b), the family, admissibility and the first contact are fp_fallback_stop's, word for word.
 * rule verdict  of a candidate, taken only for an admissible candidate without contact: the rule_bits fp_rules_eval defines for the
 *              end state (d, 0, T) when the flag word on entry carries the candidate's M (M << FP_FLAG_M_SHIFT) and no FP_FLAG_* bit.
 *              The rules are those whose pointer in `rules` is not NULL; they run in the passes' order, the gaps only if the three
 *              rules before them left the word feasible; the gates' waiver is taken from the ego's present state with the gates' own
 *              max_decel.  An inadmissible candidate and a candidate with contact have verdict 0: no rule is evaluated for them.
 *              cand_rules[b][f] = that verdict.
 * choice       among the admissible candidates only, smaller first; every key is an integer or one exact IEEE operation on inputs:
 *                1. a candidate without contact beats one with contact;
 *                2. among candidates without contact a clean verdict (0) beats a violating one;
 *                3. among clean candidates the larger i_T wins (the gentlest stop);
 *                4. among violating candidates the smaller number of FP_RULE_* bits set wins, then the smaller i_T (it brakes hardest
 *                   and overshoots least);
 *                5. among candidates with contact the larger hit_step wins, then the smaller i_T;
 *                6. then the smaller fabs(d_end - d0), then the smaller i_d.
 * outputs      status keeps its four values (FP_FALLBACK_CLEAR still says "no contact").  rule_bits[b] = the chosen candidate's verdict: 0
 *              = clean; 0 also for NOT_NEEDED, NONE, CONTACT and skipped egos.  rule_counts[b][log2 bit] += 1 for every bit of
 *              rule_bits[b] (accumulated by the ego's own workgroup without atomics, like fp_rules_eval's counts).  Everything else is
 *              as fp_fallback_stop writes it, end_state of the egos that have a plan included; cand_rules, like cand, is untouched in
 *              the rows of the egos that need no fallback.
 * Equivalence: with a rule set that cannot speak on the batch - limits +inf, gates never closed, a corridor wider than any footprint,
 * lags with no obstacle near - every output shared with fp_fallback_stop equals that call's bit for bit.
 *
 * FP_MEM_DEVICE: one kernel (the fallback kernel's rule instance), nothing allocated, nothing waited for, capturable.  FP_MEM_HOST
 * stages the batch, the family and the rule arrays through the ctx and waits, as fp_rules_eval's host call does.  The rules' tables
 * share the kernel's LDS budget with the obstacle rows: a batch whose rows just fit fp_fallback_stop's launch reads them from the scene
 * table here - the result is the same.
 * Errors, all before any launch: fp_fallback_stop's own; a NULL rules, a set whose four members are all NULL, a NULL rule_bits:
 * FP_EINVAL; every rule that is on raises its own pass' argument errors with that pass' messages (FP_MEM_HOST: also what the pass
 * finds in its arrays).
 * Also read-only in fp_ctx_get_option: "fallback_rules_launches" = launches of the rule instance on this ctx so far;
 * "fallback_launches" does not move for this call.
 * Deliberately not done: no fp_shard_call slot; nothing inside fp_plan_step / fp_plan_fiss_step (a loop enqueues plan,
 * fp_fallback_stop_rules, fp_advance); no per-row marker in the loop log; a closed loop that audits (fp_rules_eval on the planner's own
 * end state) beside a fallback stays refused by the Python runner. */
int fp_fallback_stop_rules(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_fallback* fallback,
                           const fp_rule_set* rules,
                           const int32_t* best_idx,   /* NULL or [B] */
                           double* end_state,         /* [B][3] in/out */
                           int32_t* status, int32_t* fb_idx,
                           int32_t* hit_step, int32_t* hit_obs, double* hit_speed,   /* [B] each */
                           int32_t* cand,             /* NULL or [B][n_d * n_stop], as fp_fallback_stop */
                           uint32_t* cand_rules,      /* NULL or [B][n_d * n_stop] out */
                           uint32_t* rule_bits,       /* [B] out: FP_RULE_* the chosen stop violates, 0 = clean */
                           int32_t* counts,           /* NULL or [B][4] in/out, as fp_fallback_stop */
                           int32_t* rule_counts,      /* NULL or [B][FP_RULE_COUNT] in/out */
                           int mem, void* stream);

/* ---- obstacle pose tables from tracks (added WITHIN ABI 18: detect it by looking the symbol up, e.g. dlsym) --------------
 * The reference has no predictor: it reads CommonRoad's recorded trajectories through `state_at_time` and skips an obstacle that has no
 * state at a step (frenet_optimal_planner.py:187-188).  A caller fed by a tracker has a few numbers per obstacle - position, heading,
 * speed, acceleration, path curvature - and a prediction that changes every cycle; fp_obstacles_predict writes the rows of
 * obs_pose [S][T_obs][n_obs][4] (x, y, yaw, valid) from those numbers on the device, so the table never crosses the link.
 *
 * The call reads params->tick_t and, from `batch`, S, T_obs, n_obs, F, NX, nx, knots, coef - nothing else; batch->obs_pose is NOT read
 * (a caller normally passes the same address as `obs_pose`).
 *
 * Definition.  For scene s the rows r = max(t0[s], 0) .. min(T_obs, t0[s] + n_rows) - 1 are written, all n_obs columns, four doubles
 * each; every other row of the scene is neither read nor written.
 *   tau              = (r - t0[s]) * tick_t, computed as that product (the way the lattice forms t_i = i * tick_t).
 *   final_time_step  [s] = min(T_obs, t0[s] + n_rows), clamped to 0 below; written when the pointer is not NULL.
 *   travelled distance (both models)
 *                    v0 = (v < 0) ? 0 : v  (a NaN speed stays NaN);   tau_e = (a < 0 and v0 / (-a) < tau) ? v0 / (-a) : tau  - a braking
 *                    obstacle stops and never reverses -;   l = v0 * tau_e + 0.5 * a * tau_e * tau_e.
 *   FP_TRACK_LANE    state = s0, d, v, a, -, -.   s = s0 + l;  k = bisect_right(knots, s) - 1 on frame frame_of_scene[scene], the segment
 *                    the Cartesian conversion uses;  pose = P(s) + d * n(s),  n = (-P'_y, P'_x) / |P'|;  yaw = atan2(P'_y, P'_x);  valid = 1.
 *                    The column is invalid at this row when s < knots[0], s >= knots[nx - 1], s or d is not finite, frame_of_scene is
 *                    NULL, the frame index is outside 0 .. F - 1 (or the frame's tables are NULL / its nx outside 2 .. NX).
 *   FP_TRACK_ARC     state = x0, y0, yaw0, v, a, kappa.   u = kappa * l / 2;  sinc = (|u| < 1e-4) ? 1 - u * u / 6 : sin(u) / u  (the
 *                    truncation error is below 1e-17);  x = x0 + l * sinc * cos(yaw0 + u);  y = y0 + l * sinc * sin(yaw0 + u);
 *                    yaw = yaw0 + kappa * l, not wrapped;  valid = 1.  This is the exact chord of a circular arc of length l, for any
 *                    speed profile.  Any state entry that is not finite makes the column invalid.
 *   invalid element  written as 0, 0, 0, 0 - what "no state at that step" means to every kernel.  FP_TRACK_NONE is invalid in every
 *                    row; on FP_MEM_DEVICE so is a model value outside 0 .. 2.
 * An element is a function of its track, its row and the frame alone: two runs, and the two memory spaces, give the same bits.
 *
 * FP_MEM_DEVICE: one kernel is enqueued - nothing is allocated and nothing waited for.  model, state, t0 (and the frames) are read on
 * the device when the kernel runs, so a captured call replays against new tracks.  obs_pose must be 16-byte aligned.
 * FP_MEM_HOST stages the inputs through the ctx like fp_winner_trajs, waits, and copies back only the written rows.
 * Errors: FP_EINVAL for a NULL tracks / model / state / t0 / obs_pose, n_rows <= 0, tick_t not finite or not positive; on FP_MEM_HOST
 * also - with a message that names the scene and the column - for a model outside 0 .. 2 and for a LANE track whose scene has no
 * frame (frame_of_scene NULL or its entry outside 0 .. F - 1).  S, T_obs or n_obs of 0: nothing is written, FP_OK.
 * Also read-only in fp_ctx_get_option: "predict_launches" = launches of the kernel on this ctx so far (0 for a caller that never
 * asks: such a caller gets the bits and the launch counts it got before the symbol existed).
 *
 * Deliberately not done: fp_shard_call has no slot for it; the closed-loop entry points do not call it (a loop that re-perceives
 * updates state / t0 on the device and enqueues this call in front of its plan step); a scene follows ONE line - there is no frame
 * index per track. */
#define FP_TRACK_NONE 0   /* the column has no pose in any written row */
#define FP_TRACK_LANE 1   /* follows a reference line at a fixed lateral offset */
#define FP_TRACK_ARC  2   /* Cartesian, constant path curvature, constant acceleration */

typedef struct {
    const int32_t* model;           /* [S][n_obs]     FP_TRACK_* */
    const double*  state;           /* [S][n_obs][6]  LANE: s0, d, v, a, -, -    ARC: x, y, yaw, v, a, kappa */
    const int32_t* frame_of_scene;  /* NULL or [S]    the frame LANE tracks of the scene follow */
    const int32_t* t0;              /* [S]            absolute time step the states are valid at */
    int32_t n_rows;                 /* rows written per scene, starting at row max(t0, 0) */
} fp_tracks;

int fp_obstacles_predict(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_tracks* tracks,
                         double* obs_pose, int32_t* final_time_step, int mem, void* stream);

/* ---- obstacle pose columns from the egos' own plans (added WITHIN ABI 18: detect it by looking the symbol up, e.g. dlsym) ----
 * A batch is B egos that cannot see one another: every ego plans against the obstacle table of its scene.  fp_obstacles_from_plans
 * makes the egos each other's traffic: it writes the plan every member of a group has just chosen into the obstacle tables of the
 * other members of its group, on the device, so that ego a's committed plan is what ego b avoids in the next cycle.
 *
 * The call reads params (lattice sizes, tick_t, points_max) and, from `batch`, the sizes, d_samples, t_samples, v_samples, ego,
 * frame_of, scene_of, t_now, skip, nx, knots, coef - nothing else; batch->obs_pose is NOT read (a caller normally passes the same
 * address as `obs_pose`).  obs_dims is the caller's to fill: an agent column has the footprint veh_l x veh_w.
 *
 * Definition.  Member k of group g is ego a = members[group_ptr[g] + k]; its column is c = col_base + k.  Every member has a scene of
 * its own: scene_of[a] >= 0, distinct among all members.
 *   a has a plan     when skip[a] == 0 (or skip is NULL); its lattice index best_idx[a] lies in 0 .. nd*nv*nt - 1 (decoded as
 *                    i_v = idx % nv, i_T = (idx / nv) % nt, i_d = idx / (nv * nt): d_samples[i_d], v_samples[a][i_v], t_samples[i_T]) or
 *                    its end state end_state[a] = (d, v, T) is three finite numbers; N = len(arange(0, T, tick_t)) lies in
 *                    1 .. the points the call is sized for (fp_params.points_max); and the plan's series has M >= 2 Cartesian points
 *                    (M = the first point whose s leaves [knots[0], knots[nx - 1]) of frame frame_of[a], else N).
 *   pose at step i   i < M: the series' own FP_ARR_X / FP_ARR_Y / FP_ARR_YAW element - point i of the plan from ego[a], and
 *                    yaw[i] = atan2 of the step from point i to point i + 1, the last point repeating yaw[M - 2];
 *                    i >= M: by `tail` - FP_TAIL_NONE no pose, FP_TAIL_HOLD pose M - 1 again, FP_TAIL_COAST
 *                    p[i] = p[M-1] + (i - M + 1) * (p[M-1] - p[M-2]) with yaw[M - 1].
 *   written          for i = 0 .. n_rows - 1 and r = t_now[a] + i with 0 <= r < T_obs: element [scene_of[b']][r][c] of every OTHER
 *                    member b' of g becomes (x, y, yaw, 1) - or (0, 0, 0, 0) when a has no plan or the tail gives no pose -, and
 *                    element [scene_of[a]][r][c], a's own column in its own scene, becomes (0, 0, 0, 0): an ego never sees itself.
 *                    Every other element of the table - other columns, other rows, the scenes of non-members - is neither read
 *                    nor written.
 *   final_time_step  [scene_of[a]] = min(T_obs, max(t_now[a] + n_rows, 0)) for every member a, when the pointer is not NULL.
 * An element is a function of its source ego's state, plan, row and frame alone: two runs, and the two memory spaces, give the same
 * bits, whatever the order of the members.
 *
 * Call order.  The call goes between the plan (fp_plan_dense and its rule passes, fp_plan_fiss, or the fallback behind them) and
 * fp_advance: `ego` and `t_now` are then still the plan's start, and plan point 1 lands on row t_now + 1 - the row pose 0 of the next
 * cycle's collision check reads.  n_rows must be at least the longest N + 1 for the next cycle's whole check horizon to be covered by
 * freshly written rows.  The table is what fp_gap_mask reads, so agents keep a time gap to each other with no further code.
 *
 * FP_MEM_DEVICE: one kernel is enqueued - nothing is allocated and nothing waited for.  The groups, the plans, ego and t_now are read
 * on the device when the kernel runs, so a captured call replays.  obs_pose must be 16-byte aligned.  What a host call reports as an
 * error is decided silently here: a member outside 0 .. B-1, or one without a scene, writes nothing and gets nothing.
 * FP_MEM_HOST stages the arrays through the ctx's declared list, obs_pose and final_time_step as in/out arrays, and waits.  All checks
 * run before any launch, each FP_EINVAL with the group, member or ego named: NULL pointers; both or neither of best_idx / end_state;
 * n_rows <= 0; tail outside 0 .. 2; a member outside 0 .. B-1; an ego in two groups; a member with scene_of < 0; two members sharing a
 * scene; col_base < 0 or col_base + group size > n_obs; a non-ascending group_ptr; n_members != group_ptr[G]; a best_idx >= nd*nv*nt
 * of an ego that is not skipped (as fp_advance).  G == 0 or n_members == 0: nothing is written, FP_OK.
 * Also read-only in fp_ctx_get_option: "from_plans_launches" = launches of the kernel on this ctx so far (0 for a caller that never
 * asks: such a caller gets the bits and the launch counts it got before the symbol existed).
 *
 * Deliberately not done: fp_shard_call has no slot for it; fp_plan_step / fp_plan_fiss_step do not call it (their hand-over moves the
 * ego inside the plan launch); no priorities or right-of-way between agents; one footprint (veh_l x veh_w) for every agent. */
#define FP_TAIL_NONE  0   /* beyond the plan's last point the column has no pose */
#define FP_TAIL_HOLD  1   /* ... the last pose is repeated */
#define FP_TAIL_COAST 2   /* ... the last step is repeated: p[i] = p[M-1] + (i-M+1) * (p[M-1] - p[M-2]), yaw = yaw[M-1] */

typedef struct {
    int32_t G, n_members;        /* groups; n_members = group_ptr[G] (host-known: the grid is a function of sizes alone) */
    const int32_t* group_ptr;    /* [G+1]        ascending, group_ptr[0] = 0 */
    const int32_t* members;      /* [n_members]  ego indices; an ego is a member of at most one group */
    int32_t col_base;            /* member k of a group owns column col_base + k of every scene of its group */
    int32_t n_rows;              /* rows written per member, from row t_now[a] */
    int32_t tail;                /* FP_TAIL_* */
    int32_t reserved0;
} fp_agents;

int fp_obstacles_from_plans(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_agents* agents,
                            const int32_t* best_idx, const double* end_state,   /* exactly one non-NULL, as fp_advance */
                            double* obs_pose, int32_t* final_time_step, int mem, void* stream);

/* Materialise the whole lattice: the full series of EVERY candidate of every ego, in FOP order
 *   traj [B][C][16][traj_stride] (traj_stride / traj_sparse as in fp_result), flags [B][C] (N << 8 | M << 20 | FP_FLAG_TRUNCATED; the feasibility bits
 *   come from fp_plan_dense's flag_tbl).
 * = what calc_frenet_paths + calc_global_paths leave in `all_trajs` for the visualisation (frenet_optimal_planner.py:102,
 * planners/benchmark/planning.py:336-357).  This is the one mode of the path that is HBM bound: 128 B per trajectory point. */
int fp_materialize_all(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, uint32_t* flags, double* traj, int32_t traj_stride,
                       int32_t traj_sparse, int mem, void* stream);

/* Explicit end states: K trajectories per ego with end state (d_end, v_end, T_end)
 *   = generate_trajectory_by_end_state (fiss_plus_planner.py:172-205) / generate_trajectory
 *   (fiss_planner.py:101-138) + calc_global_paths + check_constraints + has_collision.
 * end_states [B][K][3]; cost [B][K]; flags [B][K]; traj NULL or [B][K][16][traj_stride] (traj_stride / traj_sparse as in fp_result),
 * the full FrenetTrajectory series of every requested trajectory (winner epilogue,
 * FISS+ refinement, all_trajs visualisation payload).  One difference to the other entry points: with traj_sparse = 1 this one
 * writes exactly the elements that exist and NO padding up to the 16-column boundary (one lane walks a trajectory point by point);
 * a trajectory that needs more points than traj_stride gets NaN cost + FP_FLAG_INFEASIBLE. */
int fp_eval_trajs(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, int32_t K, const double* end_states,
                  double* cost, uint32_t* flags, double* traj, int32_t traj_stride, int32_t traj_sparse, int mem, void* stream);

/* ---- FISS / FISS+ for a whole batch, entirely on the device --------------------------------------------------
 * fp_plan_fiss = FissPlanner.plan (fiss_planner.py:190-270) or FissPlusPlanner.plan (fiss_plus_planner.py:61-170)
 * for B egos: dense lattice tables (fp_plan_dense kernels) -> one wavefront per ego replays the reference's
 * visiting order over the tables (initial guess :140-150, gradient walk :152-188 / frontier search
 * fiss_plus_planner.py:30-59,106-116, cost-ordered validation :229-258) -> FISS+ only: refinement
 * (gradient_decent :207-277, refine_solution :279-326; 6 probes + 1 step per round, all rounds in one launch).
 * Tie rule: exact cost ties resolve to the lower (i_d, i_v, i_t) raster index (the reference raises ValueError).
 * The wall-clock `time_limit` of refine_solution (:152-158, :293-299) is the CALLER's business: this entry point runs max_refine_iters
 * rounds; the drop-in FissPlusPlanner turns a budget that is already spent into 0 rounds (has_time_limit) or 1 (fixture G14). */
#define FP_FISS 0
#define FP_FISS_PLUS 1

typedef struct {
    int32_t kind;              /* FP_FISS or FP_FISS_PLUS */
    int32_t max_refine_iters;  /* FissPlusPlannerSettings.max_refine_iters (3); 0 = no refinement */
    double w_heuristic;        /* FissPlannerSettings.w_heuristic (10.0)          fiss_planner.py:16 */
    double decaying_factor;    /* FissPlusPlannerSettings.decaying_factor (0.5)   fiss_plus_planner.py:22 */
} fp_fiss_opts;

typedef struct {
    /* inputs, order (d, v, t): sampling_min / sampling_max / np.linspace retstep   fiss_planner.py:45-47,57-59,67-69 */
    const double* samp_min;    /* [B][3] */
    const double* samp_max;    /* [B][3] */
    const double* samp_res;    /* [B][3] */
    int32_t* prev_best_idx;    /* [B][3] in/out, -1 = None; updated to the coarse winner           :30,:252 / :140 */
    /* outputs */
    int32_t* best_ijk;         /* [B][3] coarse winner (i_d, i_v, i_t), -1 = none */
    double* best_cost;         /* [B]    cost_final of the returned trajectory (NaN = none) */
    double* end_state;         /* [B][3] (d, v, T) of the returned trajectory (refined or lattice) */
    int32_t* refined;          /* [B]    1 when a refined trajectory replaced the coarse winner (its idx is [-1,-1,-1]) */
    int32_t* stats;            /* [B][4] num_iter, generated, validated, collision_checks (incl. refinement) */
    double* trace;             /* NULL or [B][max_refine_iters*7][4] = d, v, T, cost of every refinement trajectory */
    uint32_t* best_flags;      /* NULL or [B] flag word (N, M) of the returned trajectory */
    double* best_traj;         /* NULL or [B][16][traj_stride] its full series (requires best_flags) */
    int32_t traj_stride;       /* as in fp_result (0 = FP_DEFAULT_STRIDE) */
    int32_t traj_sparse;       /* as in fp_result */
} fp_fiss_io;

/* In FP_MEM_DEVICE mode the ctx grows an internal scratch arena (dense tables, B*C*12 bytes) on first use. */
int fp_plan_fiss(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_fiss_opts* opts, const fp_fiss_io* io,
                 int mem, void* stream);

/* ---- Frenet frame construction on the device ------------------------------------------------------------------
 * fp_frames_build = CubicSpline2D.__init__ for F centerlines at once (common/geometry/cubic_spline.py:157-168 arclength
 * knots, :19-43 natural cubic spline per axis; the reference solves the dense system with np.linalg.solve, here a
 * tridiagonal Thomas sweep - same solution to ~1e-12).
 * points [F][NX][2] (rows >= n[f] ignored), n [F]  ->  knots [F][NX] (+inf padded), coef [F][8][NX]. */
int fp_frames_build(fp_ctx* ctx, int32_t F, int32_t NX, const int32_t* n, const double* points, double* knots, double* coef, int mem,
                    void* stream);

/* fp_from_state = FrenetState.from_state (common/scenario/frenet.py:32-99) for B egos: projection of a Cartesian state
 * (x, y, yaw, v) on the 0.1 m-resampled reference line of its frame (generate_frenet_frame, frenet_optimal_planner.py:272-278):
 * nearest point (first minimum), next-waypoint rule by heading, projection on the segment, sign from `wp_yaw <= x_yaw`,
 * s = polyline length up to the previous waypoint.  states [B][4]  ->  ego [B][6] = s, s_d, 0, d, d_d, 0.
 * Uses batch->F, NX, nx, knots, coef, frame_of (the other batch fields may be NULL).
 * The number of resampled points of a line is len(np.arange(0, s_last, 0.1)) = ceil(s_last / 0.1), MINUS ONE when the last of them
 * would lie at s_last itself (s_last within an ulp of a multiple of 0.1, e.g. 3 * 0.1): the spline has no segment there.  A deviation
 * from the reference, which raises IndexError on such a line; here the line loses that point (both memory modes).
 * What cannot be projected - a state with a NaN or infinite x, y, yaw or v (the reference's angle unification never returns for an
 * infinite yaw), or a frame whose line has fewer than two resampled points (s_last <= 0.1 m, or not finite) -
 *   FP_MEM_HOST:   is refused with FP_EINVAL before anything is launched; the message names the ego, the entry or the frame, and the
 *                  value.  Only frames that some frame_of[b] references are looked at.
 *   FP_MEM_DEVICE: gives that ego a row of six NaN (so does a frame_of[b] outside 0 .. F-1 or an nx outside 2 .. NX); the other
 *                  egos of the call are not affected.
 * A finite yaw whose difference to the line's yaw exceeds 25000 rad (3979 turns) gives NaN in s_d and d_d; s and d are valid.
 * Also read-only in fp_ctx_get_option: "from_state_launches" = launches of the kernel on this ctx so far. */
int fp_from_state(fp_ctx* ctx, const fp_batch* batch, const double* states, double* ego, int mem, void* stream);

/* ---- closed-loop stepping on the device ---------------------------------------------------------------------
 * fp_advance = the bookkeeping between two plan() calls of the reference's simulation loop
 * (planners/benchmark/planning.py:131-162): next FrenetState = point 1 of the returned trajectory
 * (frenet.py:185-196), time_step_now += 1, stop when there is no solution (:131-133), when the new position is within
 * l/2 of the goal-lanelet centre (:154-157) or within 3 m of the end of the 0.1 m-resampled reference line (:158-161).
 * goal_region.is_reached() (:150-153) is evaluated when the caller supplies the goal geometry (goal_poly below); commonroad itself is
 * not a dependency: the rule is restated from commonroad-io's GoalRegion.is_reached / Shape.contains_point (closed point-in-polygon
 * test + the optional time-step / velocity / orientation intervals of the goal state).
 * The chosen trajectory is given either as a lattice index (best_idx, FOP order) or as explicit end states
 * (end_state [B][3] = d, v, T; NaN = no solution) - exactly one of the two pointers is non-NULL.
 * Plan + advance can be enqueued back to back on one stream for as many cycles as wanted: no host round trip; fp_plan_step does
 * both in ONE launch.
 * FP_DONE_END_OF_LINE: the resampled line's last point is point n - 1 at arclength (n - 1) * 0.1, n = the point count fp_from_state uses
 * (len(np.arange(0, s_last, 0.1)), less one when that last sample would reach s_last itself, where the spline has no segment).  A line
 * of fewer than two such points (s_last <= 0.1 m) has no end-of-map point: the rule is off for its egos, the other rules apply.
 * best_idx: a negative index = no solution.  FP_MEM_HOST: an index >= nd*nv*nt of a running ego is refused with FP_EINVAL (ego and
 * value named) before anything is staged.  FP_MEM_DEVICE: the caller guarantees best_idx[b] < nd*nv*nt for every running ego - the
 * kernel decodes the index and reads d_samples / t_samples / v_samples with it unchecked. */
#define FP_RUNNING 0
#define FP_DONE_GOAL 1
#define FP_DONE_END_OF_LINE 2
#define FP_DONE_NO_SOLUTION 3
#define FP_DONE_GOAL_REGION 4   /* goal_region.is_reached(state)                                      planning.py:150-153 */

typedef struct {
    double* ego;            /* [B][6] in/out  (aliases fp_batch.ego) */
    int32_t* t_now;         /* [B]    in/out  (aliases fp_batch.t_now) */
    int32_t* done;          /* [B]    in/out  FP_RUNNING / FP_DONE_*  (pass it as fp_batch.skip to the plan calls) */
    int32_t* cycles;        /* [B]    in/out  number of completed plan cycles */
    const double* goal_xy;  /* [B][2] centre vertex of the goal lanelet                      planning.py:54-58 */
    double* cart_state;     /* NULL or [B][3] out: x, y, yaw of the new state                planning.py:135 */
    /* Optional goal region (NULL = the rule is skipped, as before ABI 11).  One goal state per ego: its position is a simple polygon
     * (a lanelet's left bound + reversed right bound, a rectangle's corners, ...; either orientation, closing vertex not repeated),
     * reached when the new position lies inside or ON the boundary (commonroad's Shape.contains_point is shapely's `intersects`).
     * goal_intervals (NULL or [B][6]) = the goal state's time_step / velocity / orientation intervals as lo, hi pairs; a NaN bound
     * means the goal state does not define that attribute.  time_step is compared with the cycle index i = t_now BEFORE the
     * increment (state.time_step = i, planning.py:138), velocity with s_d, orientation with yaw[1] (closed intervals). */
    const double* goal_poly;       /* NULL or [B][goal_max_vertices][2] */
    const int32_t* goal_nv;        /* [B] vertices of the ego's polygon (< 3: this ego has no goal region) */
    const double* goal_intervals;  /* NULL or [B][6] */
    int32_t goal_max_vertices;
    int32_t reserved0;
} fp_loop_io;

int fp_advance(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const int32_t* best_idx, const double* end_state,
               const fp_loop_io* io, int mem, void* stream);

/* fp_plan_step = one cycle of the simulation loop for B egos (planning.py:120-162): fp_plan_dense (FrenetOptimalPlanner.plan) and
 * fp_advance in ONE launch - the workgroup that finds an ego's argmin hands the ego over to its next state itself (io->ego / t_now /
 * done / cycles / cart_state updated in place; egos with done != FP_RUNNING are skipped: batch->skip is ignored, io->done is used).
 * result: as for fp_plan_dense (best_idx / best_cost mandatory; the tables and the winner's series optional - the series describe the
 * trajectory the ego just left behind).  A problem that does not fit the fused lattice kernel, or a multi-round launch that also asks
 * for the series, takes the two-launch path (same results).  Identical to fp_plan_dense + fp_advance in every output. */
int fp_plan_step(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_result* result, const fp_loop_io* io, int mem,
                 void* stream);

/* fp_plan_fiss_step = one cycle of the same loop with FissPlanner / FissPlusPlanner planning it: fp_plan_fiss followed by the hand-over of
 * fp_advance (the returned trajectory's end state decides; loop->done is used as batch->skip).  With refinement rounds (FP_FISS_PLUS,
 * max_refine_iters > 0) the refinement workgroup that settles an ego's trajectory hands the ego over itself - no advance launch behind
 * the pipeline; otherwise the advance kernel follows.  Identical to fp_plan_fiss + fp_advance in every output. */
int fp_plan_fiss_step(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_fiss_opts* opts, const fp_fiss_io* io,
                      const fp_loop_io* loop, int mem, void* stream);

/* ---- FISS / FISS+ that obey the road rules: fp_plan_fiss_rules (added within ABI 18: one new symbol, found by looking it up) -------
 * fp_plan_fiss (loop = NULL) or fp_plan_fiss_step (loop set, FP_MEM_DEVICE only) whose cost-ordered VALIDATION sees the verdicts of the
 * rules in `rules` (as fp_rules_eval: a NULL member = that rule is off, all four NULL = FP_EINVAL).  The visiting order, the frontier and
 * the gradient rounds stay cost-only (fiss_planner.py:229-258, fiss_plus_planner.py:120-146, :301-323 are the only places either walk
 * consults feasibility).
 *  1. Lattice stage.  The call's dense tables (ctx scratch) are masked by the table passes of the rules that are on, in the order
 *     fp_speed_envelope, fp_gate_mask, fp_boundary_mask, fp_gap_mask - the launches a dense call's caller makes behind it, so the table
 *     the search reads is bit for bit the one that chain leaves.  The search runs in its own launch (no appended search, no inline inputs).
 *  2. Search.  The unchanged walk, with FP_FLAG_BOUNDARY counting as a constraint bit (the stand-alone search kernels test
 *     FP_FLAG_CONSTRAINTS | FP_FLAG_BOUNDARY; no other entry point puts bit 128 into their table).  Stats keep their meaning on the masked
 *     words: validated = pops, collision_checks = pops without a constraint or boundary bit; "nothing feasible" is C + 1, C, C,
 *     pass_constraints.
 *  3. Refinement (FP_FISS_PLUS, max_refine_iters > 0).  Rounds, candidate list, pop order (cost, then generation index) and the end test
 *     `cost > coarse cost` are unchanged.  A popped candidate's word is the trajectory's own; if it has no FP_FLAG_INFEASIBLE bit the
 *     enforced rules are evaluated on it in the order above, exactly as fp_rules_eval defines them for an end state whose word on entry is
 *     that word (the gaps only when the word is still feasible after the other three), and the loop consumes the result - again with
 *     FP_FLAG_BOUNDARY as a constraint bit.  rejected [B] (in / out, or NULL) is increased by the number of CONSUMED pops that were feasible
 *     by their own word and got a rule bit.  If no refined candidate survives, the coarse winner - rule-clean by 1 - stands.
 *  4. Everything else - skipped egos, egos without a coarse winner, prev_best_idx, trace, best_flags / best_traj (the trajectory's own
 *     word: it is feasible, the rules add nothing), the refusals, the hand-over with `loop` - is fp_plan_fiss' / fp_plan_fiss_step's.
 *     FP_MEM_HOST stages the rule arrays as fp_rules_eval's host call does and checks them the same way (a clock before step 0 stays
 *     refused: the lattice stage plans from it).  FP_MEM_DEVICE is a linear chain of launches on the caller's stream: it waits for
 *     nothing, allocates nothing after the first call of a size, and can be captured into a graph.
 *  5. With a rule set that cannot speak on the batch (limits +inf, a corridor wider than any footprint, gates never closed, lags with no
 *     obstacle near) every output equals fp_plan_fiss' bit for bit, Stats included.
 * Limit: the refinement's rule instances hold the rules' tables in LDS beside the refinement's own layout - NX doubles (limits), 4 NX
 * (corridor), FP_MAX_GATES + points / 2 (gates), 4 n_obs (gaps).  A call with refinement rounds whose total exceeds 160 KB is refused
 * with FP_ELIMIT in both memory modes (the message names the sizes).
 * fp_ctx_get_option("fiss_rules_calls") counts the calls that passed their argument checks. */
int fp_plan_fiss_rules(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_fiss_opts* opts, const fp_fiss_io* io,
                       const fp_rule_set* rules, const fp_loop_io* loop, int32_t* rejected, int mem, void* stream);

/* ---- the driven trajectory of a device-resident loop (ABI 17) ---------------------------------------------------
 * The reference's loop returns `state_list` - one row per driven cycle: time step, position, orientation, velocity, velocity_y
 * (planners/benchmark/planning.py:135-148) - beside the summed Stats and goal_reached (:129, :150-161).  fp_loop_record keeps that
 * record ON THE DEVICE: enqueue it directly behind a step (fp_plan_step, fp_plan_fiss_step, or a plan call + fp_advance) on the same
 * stream, with the step's own fp_loop_io and result arrays; one small kernel, one lane per ego, copies the ego's new state into the
 * ego's next free row.  For every ego with sealed[b] == 0:
 *   - stats_sum[b] += stats[b] (the loop's `stats += planner.stats`, :129 - also for the plan that found no solution);
 *   - io->cycles[b] > n_rows[b]: the ego moved in this step.  Row n_rows[b] is written when it is below max_rows (the columns:
 *     FP_LOG_* below; row_stats gets the stats row) and n_rows[b] = io->cycles[b];
 *   - io->done[b] != FP_RUNNING: sealed[b] = 1.  An ego that ends with FP_DONE_NO_SOLUTION adds Stats but no row (the reference
 *     breaks before state_list.append, :131-133).
 * Whoever resets a log (n_rows = cycles so far, usually 0) seals the egos that are already finished: their stats rows are stale.
 * n_running: an exact count of the egos with done == FP_RUNNING after the step (the call zeroes the word on the stream first) - what a
 * host loop polls, now and then, to stop enqueueing.
 * The row index lives on the device and every pointer is fixed, so a captured [step, record] pair replays for any number of cycles:
 * no allocation, no synchronisation (FP_MEM_DEVICE).  FP_MEM_HOST stages every array through the ctx and waits, like fp_advance.
 * Exactly one of best_idx / end_state is non-NULL, as for fp_advance (end_state: FP_LOG_BEST_IDX = -1; best_idx: the end state is
 * decoded from the index as fp_advance decodes it).  io->cart_state, best_cost, log->rows / n_rows / sealed are mandatory; stats is
 * mandatory when row_stats or stats_sum is set; rows must be 16-byte aligned (a lane stores its 128-byte row as eight 16-byte words).
 * Violations: FP_EINVAL.  The rows hold copies: every value is bit for bit what the step left in its arrays. */
#define FP_LOG_COLS 16
enum { FP_LOG_TIME_STEP = 0, FP_LOG_X, FP_LOG_Y, FP_LOG_YAW, FP_LOG_VELOCITY /* s_d */, FP_LOG_VELOCITY_Y /* d_d */,
       FP_LOG_S, FP_LOG_S_DD, FP_LOG_D, FP_LOG_D_DD, FP_LOG_COST, FP_LOG_D_END, FP_LOG_V_END, FP_LOG_T_END,
       FP_LOG_BEST_IDX /* flat FOP index, -1 when the trajectory is not a lattice sample */, FP_LOG_DONE /* FP_RUNNING / FP_DONE_* after the cycle */ };

typedef struct {
    int32_t max_rows;     /* rows per ego the arrays below hold */
    int32_t reserved0;
    double*  rows;        /* [B][max_rows][FP_LOG_COLS] */
    int32_t* row_stats;   /* NULL or [B][max_rows][4]: Stats of the plan() that produced the row */
    int32_t* n_rows;      /* [B] in/out: cycles recorded so far (can exceed max_rows: such rows are counted, not written) */
    int32_t* sealed;      /* [B] in/out: 0 = still recording; set when the ego is seen finished */
    int64_t* stats_sum;   /* NULL or [B][4] in/out: the loop's `stats += planner.stats` (planning.py:129), incl. the plan that found no solution */
    int32_t* n_running;   /* NULL or [1] out: egos with done == FP_RUNNING after this step */
} fp_loop_log;

/* Also read-only in fp_ctx_get_option: "looplog_launches" = launches of the record kernel of this ctx so far (a loop that does not ask
 * for a log pays nothing: 0). */
int fp_loop_record(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_loop_io* io, const int32_t* best_idx,
                   const double* end_state, const double* best_cost, const int32_t* stats, const fp_loop_log* log, int mem, void* stream);

/* ---- several devices from one host thread ----------------------------------------------------------------------
 * The path shards over independent egos, one shard per GPU, no collective (planning.py:120-162 plans its scenarios one after the
 * other; nothing is exchanged).  An 8-GPU node running 0.15 ms plan steps - or 0.07 ms closed-loop cycles - per device needs
 * 50 000-120 000 enqueued calls per second: more than one host thread issues when every call crosses an FFI.  A group owns one
 * PERSISTENT worker thread per ctx (a mailbox per worker: it spins for a few tens of microseconds after its last call, then sleeps on
 * a condition variable); fp_group_submit posts one call per ctx and returns, fp_group_wait returns when every worker has ENQUEUED its
 * call (not when the GPUs are done: synchronise the streams for that) with the first error.  FP_MEM_DEVICE calls only; the structs a
 * call points to are copied at submit time.  One submitter at a time per group; a ctx of a group must not be used from other
 * threads while the group has work in flight. */
typedef struct fp_group fp_group;

typedef struct {
    void* dst;        /* host (pinned) or device address */
    const void* src;  /* device address */
    size_t bytes;
} fp_copy;            /* hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault) on the call's stream, behind its kernels */

/* One shard's call.  Which entry point runs follows from the pointers that are set:
 *   result                        fp_plan_dense(ctx, params, batch, result, FP_MEM_DEVICE, stream)
 *   result + loop                 fp_plan_step (..., result, loop, ...)
 *   fiss_opts + fiss_io           fp_plan_fiss (..., fiss_opts, fiss_io, ...)
 *   fiss_opts + fiss_io + loop    fp_plan_fiss_step(..., fiss_opts, fiss_io, loop, ...)
 * params == NULL: nothing for this ctx in this round. */
typedef struct {
    const fp_params* params;
    const fp_batch* batch;
    const fp_result* result;
    const fp_loop_io* loop;
    const fp_fiss_opts* fiss_opts;
    const fp_fiss_io* fiss_io;
    void* stream;
    const fp_copy* copies;   /* NULL or [n_copies] (at most 8) */
    int32_t n_copies;
    int32_t reserved0;
} fp_shard_call;

int fp_group_create(fp_ctx* const* ctxs, int32_t n, fp_group** out);
int fp_group_destroy(fp_group* group);
/* calls [n], calls[i] runs on ctxs[i].  A worker that is still busy with the previous round is waited for first. */
int fp_group_submit(fp_group* group, const fp_shard_call* calls);
/* FP_OK, or the first failing worker's code (fp_last_error() then carries its message, prefixed with the shard index). */
int fp_group_wait(fp_group* group);

#ifdef __cplusplus
}
#endif
#endif /* FRENET_GPU_H */
