// frenet_kernels.h - host-visible launch interface of the gfx950 kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/frenet_gpu.h"

namespace fp {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device and not free: remember the largest size configured per
// (kernel, device).  `slot` is a static LdsSlots of the kernel: per device the configured bytes + 1, so that the zeroes a static
// object starts with say "nothing configured yet".  Several host threads may launch on one device (ShardedEngine(shards_per_device >
// 1), two contexts on two streams): the check-and-set is serialised, so the recorded size is always the size the runtime was last
// told (a smaller request can never land after a larger one).
constexpr int kMaxDevices = 64;
struct LdsSlots {
    int bytes1[kMaxDevices];
};
inline std::mutex& dynamic_lds_mutex()
{
    static std::mutex m;
    return m;
}
inline hipError_t ensure_dynamic_lds(const void* kernel, int bytes, LdsSlots& slot)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(dynamic_lds_mutex());
    if (dev < 0 || dev >= kMaxDevices) return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (bytes >= slot.bytes1[dev]) {
        e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return e;
        slot.bytes1[dev] = bytes + 1;
    }
    return hipSuccess;
}
// The launch of a kernel that has one instance: its slots, the LDS attribute, the launch, the launch's error
template <auto Kernel, typename... Args>
hipError_t launch_with_lds(dim3 grid, dim3 block, int bytes, hipStream_t stream, const Args&... args)
{
    static LdsSlots configured;
    hipError_t err = ensure_dynamic_lds((const void*)Kernel, bytes, configured);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(Kernel, grid, block, bytes, stream, args...);
    return hipGetLastError();
}

// Everything a kernel needs, passed by value as the kernel argument block.
// All pointers are device addresses.
struct KernelArgs {
    fp_params p;
    fp_batch b;
    fp_result r;
    // [B][C] FP_FLAG_CURVATURE / KAPPA_D / KAPPA_DD of every lattice candidate (flat FOP order), written by
    // launch_curvature_flags ahead of the fused lattice kernel when p.curvature_mask is set; nullptr otherwise
    const uint8_t* curv_tbl = nullptr;
    // device copy of r.best_idx, written by the lattice kernels beside it and read by winner_traj_kernel (optional): the caller's
    // best_idx may be device-mapped HOST memory (bench.py's results need no copy that way), where the epilogue's first read costs
    // the link's round trip (winner kernel 10.9 -> 9.2 us on BASELINE configs[2])
    int32_t* idx_shadow = nullptr;
    // fp_plan_step (fused lattice kernel only): the workgroup that finds an ego's argmin also hands the ego over to its next state
    // (advance_ego, frenet_advance.h) - has_loop != 0: `loop` holds the caller's fp_loop_io (device addresses), b.skip = loop.done
    fp_loop_io loop = {};
    int has_loop = 0;
    // Epilogue workgroups appended to a multi-round fused lattice launch (three workgroups per CU): [B] ints, zero between launches.
    // The workgroup that publishes an ego's argmin sets its flag; the appended workgroups - dispatched last, i.e. into the slots the
    // draining launch leaves empty - wait for it, write the winner's series (r.best_traj) and clear it.  Needs idx_shadow.
    int32_t* epi_flag = nullptr;
    // The ctx's hand-over error word (device-mapped pinned host memory, or nullptr): an appended workgroup whose wait for its ego's flag
    // runs out leaves a code here instead of trapping (1: winner-series epilogue, 2: FISS+ search); the host reads it at the next call.
    int32_t* err_word = nullptr;
    // host-side launch hint (fp_ctx_set_option("lattice_occupancy")): 0 = auto, 2 / 3 = at most that many lattice workgroups per CU
    int occ_cap = 0;
    // host-side launch hints from the ctx: lattice workgroups the device holds at once at TWO per CU (fp_ctx: resident_groups = 2 x compute
    // units, or what fp_ctx_set_option("resident_groups") says - a process under a CU mask, a test that models a smaller device) and the
    // LDS of one CU in KB.  A launch takes the three- / four-per-CU instances when it has more egos than resident2 / 1.5 x resident2 and
    // the CU's LDS holds three / four of their layouts.
    int resident2 = 512;
    int lds_cu_kb = 160;
    // test hook (fp_ctx_set_option("handover_timeout_us"), FP_TEST_HOOKS only): how long an appended workgroup waits for its ego's flag
    // before it gives up; 0 = the production value (2 s).  A microsecond makes REAL waits run out, which is how the tests drive the
    // device side of the time-out path (error word, workgroup leaves without output, the launch completes) instead of injecting its result.
    int handover_timeout_us = 0;
};

// Inline inputs (latency regime of the FP_MEM_HOST entry, fused lattice kernel only): the per-ego arrays of a tiny batch travel
// INSIDE the kernel argument block - kernel arguments live in device memory on this platform (the host writes them through the
// BAR), so the kernel reads them like any other HBM data and no copy, copy kernel or dependency is enqueued for them.  on != 0:
// the fields d_samples, t_samples, v_samples, target_speed, ego, frame_of, scene_of, t_now of KernelArgs.b hold byte OFFSETS into
// bytes[] instead of addresses (skip must be NULL).
// publish != nullptr: the lattice kernel's first workgroup also copies the first n8 8-byte words of bytes[] to that device address -
// the later kernels of a multi-kernel call (fp_plan_fiss: search, refinement) read the same arrays from there, stream-ordered behind
// the lattice kernel, and the call enqueues no copy of any kind.
constexpr int kInlineMax = 1024;
struct InlineIn {
    int on = 0;
    int n8 = 0;
    void* publish = nullptr;
    unsigned char bytes[kInlineMax];
};

// Arguments of the FISS / FISS+ batch kernels: the lattice arguments plus the dense tables and the fp_fiss_io arrays.
struct FissArgs {
    KernelArgs ka;
    fp_fiss_opts opts;
    fp_fiss_io io;
    const double* cost_tbl;    // [B][C] flat FOP order
    const uint32_t* flag_tbl;  // [B][C]
    int walk_jump = 1;         // FISS+ walk: skip the iterations below the first feasible sample's minimax level (frenet_fissplus.hip)
};

// The FISS+ search as workgroups appended to the fused lattice launch (lattice_fused_kernel's FISS instances): what the search needs
// beside the lattice's KernelArgs.  flag: [B] ints, zero between launches - an ego's lattice workgroup sets its flag when the ego's
// rows of the dense tables are written (agent-scope stores), the ego's search workgroup waits for it and clears it.
struct FissTail {
    fp_fiss_opts opts;
    fp_fiss_io io;
    int NB = 0;          // buckets of the ranking (fsp::fissplus_search_ego)
    int walk_jump = 1;
    int32_t* flag = nullptr;
};

// One wavefront per ego: coarse FISS / FISS+ search over the dense tables.
hipError_t launch_fiss_search(const FissArgs& fa, hipStream_t stream);
// The FISS+ walk in rank space (frenet_fissplus.hip); launch_fiss_search dispatches to it for FP_FISS_PLUS.
hipError_t launch_fissplus_search(const FissArgs& fa, hipStream_t stream);
// One workgroup per ego: FISS+ refinement rounds + cost-ordered validation of the refined trajectories.  table_kb = LDS budget
// of the per-ego fp32 pose-obstacle pair table (0: no table, pairs are read from the scene table).
// perm / dur: launch order and duration feedback, like LatticeRequest.
hipError_t launch_fiss_refine(const FissArgs& fa, hipStream_t stream, int table_kb, const int* perm = nullptr, int* dur = nullptr);

// part_scratch: device buffer of kTicketBytes (ticket counters, int per ego, ZERO before the first launch; the kernel leaves
// them zero) + B * nsplit * 16 bytes (partial argmins), or nullptr; nsplit > 1 = latency mode (B <= kTicketBytes / 4).
constexpr size_t kTicketBytes = 64 * 1024;
// What a caller asks of a lattice launch beside the offers its KernelArgs carry (series inside: r.best_traj; epilogue workgroups:
// epi_flag + idx_shadow; loop hand-over: has_loop + loop).  plan_lattice (frenet_lattice_plan.h) takes what fits.
struct LatticeRequest {
    void* part_scratch = nullptr;  // see kTicketBytes
    int nsplit = 1;
    const int* perm = nullptr;     // (nsplit == 1) workgroup i works on ego perm[i]: the launch order
    int* dur = nullptr;            // every workgroup leaves its ego's duration there (10 ns ticks)
    int group = 1;                 // "lattice_group", granted up to lattice_group_fit; above 1: a grouped instance (1024-thread workgroups)
    int tail = 0;                  // (needs part_scratch) cut the last `tail` slots of a multi-round launch in two; < 0: auto for -tail CUs
    const InlineIn* inl = nullptr;  // inline inputs: the fused kernel or nothing
    const FissTail* ft = nullptr;   // the FISS+ search in workgroups appended to the launch (three- / four-per-CU launches)
    // a pass behind the launch decides the winner (the clearance rescoring, fp_params.w_obstacle > 0): the launch writes its tables and
    // a provisional argmin - no series from its workgroups, no epilogue workgroups, no loop hand-over, whatever the KernelArgs offer
    bool provisional = false;
};
// What the launch did: wrote the winner's series (else winner_traj_kernel follows), handed the egos over (else advance_kernel),
// ran the FISS+ search (else the search kernel).
struct LatticeResult {
    bool winner_done = false, step_done = false, search_done = false;
};
int lattice_group_fit(const fp_params& p, const fp_batch& b);
// launches of the fused lattice kernel by workgroups per CU ([0] two, [1] three, [2] four) since the library was loaded: process-wide
// counters behind fp_ctx_get_option("lattice_launches_2 / _3 / _4") - what the tests use to know which instance family they ran
long lattice_launches_per_cu(int which);
hipError_t launch_lattice_percand(const KernelArgs& ka, hipStream_t stream);
// The clearance cost term (frenet_clearance.hip): re-prices the survivors in ka.r.cost_tbl (ka.r.flag_tbl says who survived), rewrites
// ka.r.best_idx / best_cost (+ idx_shadow) with the argmin of the new costs.  One workgroup per ego, in the order of perm (optional).
hipError_t launch_clearance_rescore(const KernelArgs& ka, const int* perm, hipStream_t stream);
// Curvature flags of every lattice candidate -> out [B][C] (one workgroup per ego, one lane per candidate, spline in LDS).
hipError_t launch_curvature_flags(const KernelArgs& ka, uint8_t* out, hipStream_t stream);
// The lattice pass of a dense, FISS or closed-loop call.  which: 0 = auto (the fused kernel when the problem fits it, else the
// lane-per-candidate kernel), 1 = lane-per-candidate, 2 = fused only (hipErrorInvalidValue when it does not fit; so do inline inputs).
// Every other error is the runtime's.
hipError_t launch_lattice(const KernelArgs& ka, hipStream_t stream, int which, const LatticeRequest& rq, LatticeResult* res);
// Winner epilogue: recompute the full series of trajectory best_idx[b] for every ego (one lane per time point).
// end_states = nullptr: series of lattice candidate ka.r.best_idx[b]; else [B][3] explicit (d, v, T) end states (NaN = none).
hipError_t launch_winner_traj(const KernelArgs& ka, const double* end_states, hipStream_t stream);
// FopPlusPlanner.plan from the dense tables + the FOP argmin (one wavefront per ego): out [B][2] = {popped, tie}, stats [B][4].
// skip (optional, fp_batch.skip): egos the lattice kernel did not plan get out = {0, 0} and keep their Stats.
hipError_t launch_fopplus_count(int B, int C, const double* cost_tbl, const uint32_t* flag_tbl, const int32_t* best_idx, const double* best_cost,
                                int32_t* out, int32_t* stats, const int32_t* skip, hipStream_t stream);
// fp_result.audit: near-tie / thin-contact bits of every ego from its dense tables (ka.r.cost_tbl / flag_tbl / best_idx / best_cost must be
// set; best_idx / best_cost are rewritten where a near tie is settled by point-by-point sums).  One workgroup per ego.
hipError_t launch_audit(const KernelArgs& ka, uint32_t* audit, hipStream_t stream);
// Frenet frame construction / Cartesian -> Frenet projection (frenet_frame.hip).
hipError_t launch_frames_build(int F, int NX, const int32_t* n, const double* points, double* knots, double* coef, hipStream_t stream);
hipError_t launch_from_state(const fp_batch& bt, const double* states, double* ego, hipStream_t stream);
// Closed-loop bookkeeping between two plan cycles (one lane per ego).
hipError_t launch_advance(const KernelArgs& ka, const int32_t* best_idx, const double* end_state, const fp_loop_io& io, hipStream_t stream);
// The driven-trajectory log of a resident loop (frenet_looplog.hip, fp_loop_record): behind a step, one lane per ego copies the ego's
// new state into its next free row.  Device addresses; exactly one of best_idx / end_state set; stats may be nullptr when the log
// asks for none.  log.n_running (optional) must be zero on the stream before the launch.
struct LoopLogArgs {
    int B = 0, nv = 1, nt = 1;
    const double* d_samples = nullptr;
    const double* v_samples = nullptr;
    const double* t_samples = nullptr;
    fp_loop_io io = {};
    const int32_t* best_idx = nullptr;
    const double* end_state = nullptr;
    const double* best_cost = nullptr;
    const int32_t* stats = nullptr;
    fp_loop_log log = {};
};
hipError_t launch_loop_record(const LoopLogArgs& a, hipStream_t stream);
// The K cheapest survivors of every ego from the dense tables (frenet_rank.hip, fp_rank_feasible): one workgroup per ego, in the order
// of perm (optional).  Device addresses; rank_idx / rank_cost are [K][B], n_feasible (optional) [B].
struct RankArgs {
    int B = 0, C = 0, K = 0;
    const double* cost_tbl = nullptr;
    const uint32_t* flag_tbl = nullptr;
    const int32_t* skip = nullptr;
    const int32_t* perm = nullptr;
    int32_t* rank_idx = nullptr;
    double* rank_cost = nullptr;
    int32_t* n_feasible = nullptr;
};
hipError_t launch_rank_feasible(const RankArgs& a, hipStream_t stream);
// What the table passes behind the dense pass share (frenet_boundary.hip, frenet_envelope.hip, frenet_gates.hip): one workgroup per ego, in the order of
// perm (optional), over the ego's rows of cost_tbl / flag_tbl [B][C]; each rewrites bits of the flag words and writes the ego's argmin
// over what is still feasible, and - optionally - how many candidates it flagged (count [B]).  Device addresses.
struct TablePassArgs {
    int B = 0, NX = 0, nd = 1, nv = 1, nt = 1;
    double tick_t = 0.0;
    const double* t_samples = nullptr;
    const double* v_samples = nullptr;
    const double* ego = nullptr;
    const int32_t* frame_of = nullptr;
    const int32_t* nx = nullptr;
    const double* knots = nullptr;
    const int32_t* skip = nullptr;
    const int32_t* perm = nullptr;
    const double* cost_tbl = nullptr;
    uint32_t* flag_tbl = nullptr;
    int32_t* best_idx = nullptr;
    double* best_cost = nullptr;
    int32_t* count = nullptr;
};
// The road-boundary check (fp_boundary_mask): FP_FLAG_BOUNDARY of every candidate.  left / right are [F][NX] lateral offsets of the road
// edges at the knots; count = n_masked.
struct BoundaryArgs : TablePassArgs {
    double veh_l = 0.0, veh_w = 0.0, margin = 0.0;
    const double* d_samples = nullptr;
    const double* left = nullptr;
    const double* right = nullptr;
};
hipError_t launch_boundary_mask(const BoundaryArgs& a, hipStream_t stream);
// Position-dependent speed limits (fp_speed_envelope): ORs FP_FLAG_SPEED / FP_FLAG_ACCEL into the flag words.  v_limit is [F][NX] (the
// limit of the segment that starts at the knot); coef is read only when max_lat_accel > 0; count = n_limited.
struct EnvelopeArgs : TablePassArgs {
    double front = 0.0, tol = 0.0, max_lat_accel = 0.0;
    const double* coef = nullptr;
    const double* v_limit = nullptr;
};
hipError_t launch_speed_envelope(const EnvelopeArgs& a, hipStream_t stream);
// Stop lines that open and close (frenet_gates.hip, fp_gate_mask): ORs FP_FLAG_SPEED into the flag word of a candidate that crosses a
// closed gate.  gate_s is [F][gate_stride] (NaN = unused slot), closed [F][T_gate] (bit g = gate g closed at that absolute step), t_now
// [B] the egos' clocks; points_cap = the points a trajectory of the call can have (the closed words staged per ego); count = n_gated.
struct GateArgs : TablePassArgs {
    double front = 0.0, max_decel = 0.0;
    int gate_stride = 0, T_gate = 0, points_cap = 0;
    const int32_t* t_now = nullptr;
    const double* gate_s = nullptr;
    const uint32_t* closed = nullptr;
};
hipError_t launch_gate_mask(const GateArgs& a, hipStream_t stream);
// A time gap to moving obstacles (frenet_gaps.hip, fp_gap_mask): ORs FP_FLAG_COLLISION into the flag word of a survivor in ka.r.flag_tbl
// whose footprint overlaps an obstacle's with the two time indices up to lag_follow / lag_lead steps apart, and writes the argmin of
// ka.r.cost_tbl over the survivors that are left to ka.r.best_idx / best_cost.  One workgroup per ego, in the order of perm (optional);
// count = n_close (optional).  Device addresses.  grid_cap and bound_off are filled in by the launcher: the grid poses its LDS cull
// table holds (0: none) and where the table starts, in doubles.
struct GapArgs {
    int lag_follow = 0, lag_lead = 0, first = 1;
    int grid_cap = 0, bound_off = 0;
    const int32_t* perm = nullptr;
    int32_t* count = nullptr;
};
hipError_t launch_gap_mask(const KernelArgs& ka, GapArgs g, hipStream_t stream);
// The four rules on K explicit end states per ego (frenet_rules_eval.hip, fp_rules_eval): one workgroup per ego, in the order of perm
// (optional).  on = the FP_RULE_* bits of the rules that run (FP_RULE_LATERAL only beside FP_RULE_LIMIT); each rule's scalars and
// arrays as its own pass takes them (a rule that is off leaves them unset).  Device addresses; end_states [B][K][3], flags [B][K]
// in/out, rule_bits [B][K] or nullptr, counts [B][FP_RULE_COUNT] or nullptr.  The off_* fields are filled in by the launcher: where
// the rules' own tables start in LDS behind stage_ego's layout, in doubles.
struct RulesEvalArgs {
    int K = 0;
    uint32_t on = 0u;
    double env_front = 0.0, env_tol = 0.0, max_lat_accel = 0.0;
    const double* v_limit = nullptr;
    double gate_front = 0.0, max_decel = 0.0;
    int gate_stride = 0, T_gate = 0;
    const double* gate_s = nullptr;
    const uint32_t* closed = nullptr;
    double margin = 0.0;
    const double* left = nullptr;
    const double* right = nullptr;
    int lag_follow = 0, lag_lead = 0, first = 1;
    int off_lim = 0, off_edge = 0, off_gate = 0;
    const double* end_states = nullptr;
    uint32_t* flags = nullptr;
    uint32_t* rule_bits = nullptr;
    int32_t* counts = nullptr;
    const int32_t* perm = nullptr;
};
hipError_t launch_rules_eval(const KernelArgs& ka, RulesEvalArgs a, hipStream_t stream);
// fp_plan_fiss_rules: the refinement whose popped candidates are also checked against the enforced rules (fiss_refine_kernel<NCH, FissRulesArgs>,
// frenet_fiss.hip).  rules = the rule set as launch_rules_eval takes it (K, end_states, flags, rule_bits, counts and perm
// are not read); rejected [B] in/out or nullptr; rules_off = where the rules' tables start in LDS, in bytes, the off_* fields relative to
// it (both filled in by the launcher).
struct FissRulesArgs : FissArgs {
    RulesEvalArgs rules;
    int32_t* rejected = nullptr;
    int rules_off = 0;
};
// LDS of one workgroup of that launch: the refinement's own layout (*base_bytes) and the rules' tables behind it (*rule_bytes) - the limit
// per segment, the corridor's edge and slope per segment and side, the gate lines and closed words, the obstacle sizes (the gaps).
// kRefineRulesLdsMax is what a workgroup may use; a call that needs more is refused (FP_ELIMIT).
constexpr int kRefineRulesLdsMax = 160 * 1024;
void fiss_refine_rules_lds(const FissArgs& fa, uint32_t on, int table_kb, int* base_bytes, int* rule_bytes);
hipError_t launch_fiss_refine_rules(const FissArgs& fa, const RulesEvalArgs& rules, int32_t* rejected, hipStream_t stream, int table_kb,
                                    const int* perm = nullptr, int* dur = nullptr);
// The obstacle margin of K chosen plans per ego (frenet_margins.hip, fp_traj_margins): one workgroup per ego, in the order of perm
// (optional).  ka.p.check_stride is the call's pose_stride; ka.r is not read.  Device addresses; exactly one of best_idx [K][B] /
// end_state [K][B][3] set; the outputs are [K][B].
struct MarginArgs {
    int K = 0;
    const int32_t* best_idx = nullptr;
    const double* end_state = nullptr;
    const int32_t* perm = nullptr;
    double* min_dist = nullptr;
    int32_t* min_step = nullptr;
    int32_t* min_obs = nullptr;
};
hipError_t launch_traj_margins(const KernelArgs& ka, const MarginArgs& m, hipStream_t stream);
// A stopping manoeuvre for the egos without a plan (frenet_fallback.hip, fp_fallback_stop): one workgroup per ego, in the order of perm
// (optional).  Device addresses; best_idx [B] or nullptr, end_state [B][3] in/out, cand [B][n_d * n_stop] or nullptr, counts [B][4]
// in/out or nullptr, the other outputs [B].
struct FallbackArgs {
    int n_d = 0, n_stop = 0;
    const double* d_targets = nullptr;
    const double* stop_T = nullptr;
    double max_decel = 0.0;
    const int32_t* best_idx = nullptr;
    double* end_state = nullptr;
    int32_t* status = nullptr;
    int32_t* fb_idx = nullptr;
    int32_t* hit_step = nullptr;
    int32_t* hit_obs = nullptr;
    double* hit_speed = nullptr;
    int32_t* cand = nullptr;
    int32_t* counts = nullptr;
    const int32_t* perm = nullptr;
};
hipError_t launch_fallback_stop(const KernelArgs& ka, const FallbackArgs& a, hipStream_t stream);
// fp_fallback_stop_rules: the fallback whose clear candidates are also ranked by the rule set (fallback_kernel<true>, frenet_fallback.hip).
// rules = the rule set as launch_rules_eval takes it (K, end_states, flags, rule_bits, counts and perm are not read; the off_* fields are
// filled in by the launcher); cand_rules [B][F] or nullptr, rule_bits [B], rule_counts [B][FP_RULE_COUNT] in/out or nullptr.
struct FallbackRulesArgs : FallbackArgs {
    RulesEvalArgs rules;
    uint32_t* cand_rules = nullptr;
    uint32_t* rule_bits = nullptr;
    int32_t* rule_counts = nullptr;
};
hipError_t launch_fallback_stop_rules(const KernelArgs& ka, FallbackRulesArgs a, hipStream_t stream);
// The obstacle pose table from tracks (frenet_predict.hip, fp_obstacles_predict): rows max(t0, 0) .. min(T_obs, t0 + n_rows) - 1 of
// every scene of obs_pose [S][T_obs][n_obs][4].  Device addresses; nx / knots / coef / frame_of_scene may be NULL (LANE columns then
// have no pose).  compact: the output is [S][span][n_obs][4], span = min(T_obs, n_rows), and a scene's first written row lands in
// its row 0 (what a host call reads back).  span, rows_per_slab, n_slabs and stage_tracks are filled in by the launcher.
struct PredictArgs {
    int S = 0, T_obs = 0, n_obs = 0, F = 0, NX = 0, n_rows = 0, compact = 0;
    int span = 0, rows_per_slab = 0, n_slabs = 0, stage_tracks = 0;
    double tick_t = 0.0;
    const int32_t* nx = nullptr;
    const double* knots = nullptr;
    const double* coef = nullptr;
    const int32_t* model = nullptr;
    const double* state = nullptr;
    const int32_t* frame_of_scene = nullptr;
    const int32_t* t0 = nullptr;
    double* obs_pose = nullptr;
    int32_t* final_time_step = nullptr;
};
hipError_t launch_obstacles_predict(PredictArgs a, hipStream_t stream);
// The chosen plans of grouped egos as obstacle columns of each other's scenes (frenet_agents.hip, fp_obstacles_from_plans): one
// workgroup per destination member.  ka.b.obs_pose and ka.r are not read.  Device addresses; exactly one of best_idx [B] / end_state
// [B][3] set; final_time_step [S] or nullptr.
struct AgentArgs {
    int G = 0, n_members = 0, col_base = 0, n_rows = 0, tail = 0;
    const int32_t* group_ptr = nullptr;
    const int32_t* members = nullptr;
    const int32_t* best_idx = nullptr;
    const double* end_state = nullptr;
    double* obs_pose = nullptr;
    int32_t* final_time_step = nullptr;
};
hipError_t launch_obstacles_from_plans(const KernelArgs& ka, const AgentArgs& a, hipStream_t stream);
// Series of EVERY lattice candidate: ka.r.best_traj [B*C][16][traj_stride], ka.r.best_flags [B*C] (N, M, truncated).
hipError_t launch_materialize_all(const KernelArgs& ka, hipStream_t stream);
hipError_t launch_eval_trajs(const KernelArgs& ka, int K, const double* end_states, double* cost, uint32_t* flags, double* traj,
                             int stride, int sparse, hipStream_t stream);

}  // namespace fp
