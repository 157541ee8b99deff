// frenet_abi.hip - the C ABI of libfrenetgpu.so (include/frenet_gpu.h).
//
// Host-side responsibilities only: argument validation, the per-ctx staging used by FP_MEM_HOST calls, error
// strings.  No planning arithmetic happens on the host: if there is no usable GPU every entry point fails with
// FP_ENODEV / FP_EHIP.
//
// One body per entry point, whatever the memory space (CallStage below): the argument checks; under `if (call.host())` the checks that
// look into the arrays and the points_max a host call derives itself; the arrays, declared once in the call's StageList
// (frenet_stage_plan.h) - an FP_MEM_DEVICE call's list hands the caller's addresses through, an FP_MEM_HOST call's stages them -;
// commit; one launch on call.stream(); one counter; `return call.finish()`.  What else differs between the spaces stands at one place
// each: launch_order_of (the caller's launch order: device calls only), stage_batch's DeviceView, a device call's alignment checks.
//
// FP_MEM_HOST staging (latency matters for the B = 1 drop-in planners): small arrays are packed into ONE pinned host
// block that mirrors the head of the device arena, so a call costs one H2D copy, the kernels, one D2H copy - instead of
// one transfer per array.  Arrays above kSmallMax bytes are copied directly (no extra host pass over big batches).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "frenet_kernels.h"
#include "frenet_project.h"
#include "frenet_rule_calls.h"
#include "frenet_stage_plan.h"

// Toolchain pin.  The kernels were validated on ROCm 7.2.0's clang 22 (AMD clang 22.0.0git roc-7.2.0): no kernel may spill a VGPR
// (tests/test_abi_cpu.py:test_no_kernel_spills_a_vgpr - this compiler's spill placement in divergent loop exits is wrong), the build
// needs -mllvm -disable-machine-licm, and the four-per-CU instances sit exactly on their 64-VGPR / 80-SGPR budgets.  Another major
// version is another code generator: rebuild with -DFP_ANY_COMPILER only together with tools/resource_usage.py and the GPU test suite.
#if !defined(FP_ANY_COMPILER) && defined(__clang_major__) && __clang_major__ != 22
#error "libfrenetgpu was validated on ROCm 7.2.0 (clang 22); build with EXTRA=-DFP_ANY_COMPILER after re-checking spills (tools/resource_usage.py) and the GPU tests"
#endif

namespace {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) return fail(FP_EHIP, "%s failed: %s", #expr, hipGetErrorString(_e));     \
    } while (0)
#define FP_TRY(expr)                  \
    do {                              \
        int _rc = (expr);             \
        if (_rc != FP_OK) return _rc; \
    } while (0)
#define LAUNCH_TRY(expr, what)                                                                          \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess) return fail(FP_EHIP, what " launch failed: %s", hipGetErrorString(_e));   \
    } while (0)

using fp::align_up;
using fp::kAlign;
using fp::kSmallRegion;
using fp::StageList;
using fp::StageRegime;

// grow-only device buffer
struct DeviceBuf {
    char* base = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return FP_OK;
        if (base) {
            hipError_t e = hipFree(base);
            base = nullptr;
            cap = 0;
            if (e != hipSuccess) return fail(FP_EHIP, "hipFree failed: %s", hipGetErrorString(e));
        }
        const size_t want = bytes + bytes / 4 + (1u << 20);
        hipError_t e = hipMalloc((void**)&base, want);
        if (e != hipSuccess) return fail(FP_ENOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        cap = want;
        return FP_OK;
    }
};

}  // namespace

// launches between two fetches of the duration table: 8 while a batch's order is young, doubling with every order that lands up to 64 -
// a fetch and the upload of the order it yields are two copy commands on the launch stream (~13 us of stream time each: a copy engine
// hand-over), 2.5 % of a 2048-ego step at one pair per 8 launches; a resident batch's durations drift slowly
constexpr int kOrderRefresh = 8, kOrderRefreshMax = 64;

// State of one kernel's feedback-directed launch order (see lattice_order_before).
struct LaunchOrder {
    DeviceBuf buf;              // [dur: int x cap][perm: int x cap]
    int* host = nullptr;        // pinned: [dur x cap][perm x cap]
    int cap = 0;                // egos the buffers hold
    int valid_B = 0;            // the uploaded order is a permutation of [0, valid_B)
    int dur_B = 0;              // batch size of the durations in flight / on the device
    int since = 0;              // launches since the last fetch was enqueued
    int interval = 8;           // launches between two fetches: kOrderRefresh at first, doubled after every order that landed (up to kOrderRefreshMax)
    bool pending = false;       // a fetch is in flight (event)
    hipEvent_t event = nullptr;
    void release()
    {
        if (buf.base) (void)hipFree(buf.base);
        if (host) (void)hipHostFree(host);
        if (event) (void)hipEventDestroy(event);
    }
};

// The feedback orders of one kernel, one per RESIDENT BATCH (keyed by the address of the batch's ego-state array): an order is only ever
// applied to the batch it was learnt on.  (Until round 6 there was one order per kernel and batch SIZE: a caller cycling through
// several resident batches of one size dispatched each in the order another one had left behind - for the refinement kernel, whose
// launch is one round of workgroups with only the egos that found a trajectory doing work, a foreign order is worse than none:
// rocprofv3 82 us per launch against 55 with its own.)  kOrderSlots batches, least recently used one replaced.
constexpr int kOrderSlots = 8;
struct OrderSet {
    LaunchOrder slot[kOrderSlots];
    const void* key[kOrderSlots] = {};
    unsigned long used[kOrderSlots] = {};
    unsigned long tick = 0;
    LaunchOrder& of(const void* k)
    {
        int lru = 0;
        for (int i = 0; i < kOrderSlots; ++i) {
            if (key[i] == k && used[i]) { used[i] = ++tick; return slot[i]; }
            if (used[i] < used[lru]) lru = i;
        }
        LaunchOrder& o = slot[lru];
        if (o.pending) { (void)hipEventSynchronize(o.event); o.pending = false; }  // (the fetch in flight belongs to the batch that leaves)
        o.valid_B = o.dur_B = 0;
        o.since = 0;
        o.interval = kOrderRefresh;
        key[lru] = k;
        used[lru] = ++tick;
        return o;
    }
    void forget() { for (auto& o : slot) o.valid_B = 0; }
    void release() { for (auto& o : slot) o.release(); }
};

struct fp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;  // used by FP_MEM_HOST calls
    DeviceBuf arena;               // [ small region (kSmallRegion) | large region ] staging of FP_MEM_HOST calls
    char* pinned = nullptr;        // kSmallRegion bytes of pinned host memory mirroring the small region
    DeviceBuf scratch;             // intermediate tables of multi-kernel entry points (fp_plan_fiss)
    // frame + scene tables of tagged FP_MEM_HOST calls (fp_batch.tables_tag): a few sets, least recently used one replaced - two
    // planners that take turns on one ctx (FOP and FISS+ on the same scenario, say) both keep theirs
    struct TableSet {
        DeviceBuf buf;
        int key[7] = {0, 0, 0, 0, 0, 0, 0};    // {tag, F, NX, S, T_obs, n_obs, poly_stride (0: rectangles only)} of what buf holds (tag 0: nothing)
        size_t off[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // nx, knots, coef, obs_pose, obs_dims, final_time_step, obs_poly, obs_nvert
        unsigned long used = 0;                // tick of the last call that read it
    };
    static constexpr int kTableSets = 4;
    TableSet tables[kTableSets];
    unsigned long tables_tick = 0;
    DeviceBuf parts;               // latency-mode lattice launch: [ticket counters, fixed-size region][partial argmins]
    int lattice_kernel = 0;        // fp_ctx_set_option("lattice_kernel")
    int lattice_split = 0;         // fp_ctx_set_option("lattice_split"): 0 auto, 1 never, 2 always
    int inline_inputs = 1;         // fp_ctx_set_option("inline_inputs"): fp_plan_dense(FP_MEM_HOST) of a tiny batch with cached tables passes the per-ego arrays inside the lattice kernel's argument block
    int stage_kernel = 1;          // fp_ctx_set_option("stage_kernel"): the latency regime's inputs reach the device by a copy kernel instead of a copy command
    int zero_copy_in = 0;          // fp_ctx_set_option("zero_copy_in"): FP_MEM_HOST calls of a handful of egos read inputs from pinned host memory: 0 never (default: even a few hundred bytes read over the link cost every kernel of the call a round trip - measured slower than the copy kernel), 1 the per-ego arrays of a call whose tables are cached (tables_tag), 2 everything
    int lattice_occupancy = 0;     // fp_ctx_set_option("lattice_occupancy"): 0 auto, 2 / 3: at most that many lattice workgroups per CU
    int lattice_tail = 0;          // fp_ctx_set_option("lattice_tail"): 0 auto, 1 never, n >= 2: the last n dispatch slots of a multi-round launch are cut in two workgroups
    int lattice_group = 0;         // fp_ctx_set_option("lattice_group"): 0 auto, 1 never, n >= 2: the 1024-thread (grouped) instances where they fit
    int refine_table_kb = 96;      // fp_ctx_set_option("refine_table_kb")
    int fiss_stages = 3;           // fp_ctx_set_option("fiss_stages"): timing diagnostic, 3 = the whole pipeline
    int fiss_jump = 1;             // fp_ctx_set_option("fiss_jump"): FISS+ walk skips ahead to the first feasible sample's level
    int validate = 0;              // fp_ctx_set_option("validate"): FP_MEM_DEVICE calls range-check the batch's index arrays first
    DeviceBuf validate_buf;        // two ints on the device: first failing check, index
    int* validate_host = nullptr;  // ... and their pinned mirror
    int lattice_winner = 0;        // fp_ctx_set_option("lattice_winner"): 0 auto, 1 inside the lattice kernel, 2 its own launch
    int fiss_fused = 1;            // fp_ctx_set_option("fiss_fused"): 1 = the FISS+ search of a multi-round batch runs in workgroups appended to the lattice launch; 0 = always its own launch
    int resident_groups = 512;     // lattice workgroups the device holds at once: 2 per CU (128-VGPR budget, 512 threads each); fp_ctx_set_option("resident_groups")
    int lds_cu_kb = 160;           // LDS of one compute unit (hipDeviceProp_t::maxSharedMemoryPerMultiProcessor)
    // feedback-directed launch order of the multi-round lattice launch (fp_ctx_set_option("lattice_order")): every workgroup
    // leaves its ego's duration in dur_dev; now and then the host fetches them (async copy + event, never a wait), sorts the egos
    // longest-first and uploads the order the following launches dispatch in.  A stale or missing order only costs speed.
    int lattice_order = 1;
    int lattice_launches = 0, lattice_ordered_launches = 0;  // fp_ctx_get_option counters
    int clearance_launches = 0;    // fp_ctx_get_option("clearance_launches"): launches of the clearance rescoring kernel (fp_params.w_obstacle > 0)
    int looplog_launches = 0;      // fp_ctx_get_option("looplog_launches"): launches of the loop-log kernel (fp_loop_record)
    int rank_launches = 0;         // fp_ctx_get_option("rank_launches"): launches of the ranking kernel (fp_rank_feasible)
    int boundary_launches = 0;     // fp_ctx_get_option("boundary_launches"): launches of the road-boundary kernel (fp_boundary_mask)
    int envelope_launches = 0;     // fp_ctx_get_option("envelope_launches"): launches of the speed-envelope kernel (fp_speed_envelope)
    int gate_launches = 0;         // fp_ctx_get_option("gate_launches"): launches of the gate kernel (fp_gate_mask)
    int gap_launches = 0;          // fp_ctx_get_option("gap_launches"): launches of the time-gap kernel (fp_gap_mask)
    int rules_eval_launches = 0;   // fp_ctx_get_option("rules_eval_launches"): launches of the rules kernel (fp_rules_eval)
    int margin_launches = 0;       // fp_ctx_get_option("margin_launches"): launches of the plan-margin kernel (fp_traj_margins)
    int fallback_launches = 0;     // fp_ctx_get_option("fallback_launches"): launches of the fallback kernel (fp_fallback_stop)
    int fallback_rules_launches = 0;  // fp_ctx_get_option("fallback_rules_launches"): launches of its rule instance (fp_fallback_stop_rules)
    int from_plans_launches = 0;   // fp_ctx_get_option("from_plans_launches"): launches of the shared-plans kernel (fp_obstacles_from_plans)
    int predict_launches = 0;      // fp_ctx_get_option("predict_launches"): launches of the obstacle prediction kernel (fp_obstacles_predict)
    int from_state_launches = 0;   // fp_ctx_get_option("from_state_launches"): launches of the projection kernel (fp_from_state)
    int fiss_rules_calls = 0;      // fp_ctx_get_option("fiss_rules_calls"): calls of fp_plan_fiss_rules that passed their argument checks
    OrderSet order_lattice, order_refine, order_refine_rules;  // (the rule instances of the refinement learn their own order: two workgroups per CU, other durations)
    DeviceBuf idx_shadow;          // [B] device copy of best_idx for the winner kernel of a dense call (KernelArgs::idx_shadow)
    DeviceBuf epi_flags;           // [B] hand-over flags of the epilogue workgroups appended to a multi-round lattice launch (KernelArgs::epi_flag); zero between launches
    DeviceBuf curv_buf;            // [B][C] curvature flag bytes of the lattice (fp_params.curvature_mask), written ahead of the fused kernel
    // Workgroups appended to a lattice launch (winner-series epilogue, FISS+ search) wait for flags that other workgroups of the SAME
    // launch set; that they cannot starve rests on the workgroup distributors starting workgroups in index order - observed on gfx942 /
    // gfx950, documented nowhere.  appended_ok: the device is one of those architectures and no hand-over of this ctx ever timed out.
    // hand_err: one int of device-mapped, coherent host memory; a wait that runs out leaves a code there instead of trapping
    // (KernelArgs::err_word), and the next call on the ctx reports it, resets the flags and stops offering appended workgroups.
    bool appended_ok = false;
    int32_t* hand_err = nullptr;
    int handover_timeout_us = 0;   // fp_ctx_set_option("handover_timeout_us") (FP_TEST_HOOKS): KernelArgs::handover_timeout_us
    // fp_ctx_set_option("overlap"): consecutive INDEPENDENT FP_MEM_DEVICE dense calls alternate between two internal streams (this ctx's
    // and a twin ctx's, each with its own scratch: tickets, hand-over flags, launch order), so the draining tail of one launch runs beside
    // the ramp of the next.  See fp_plan_dense / fp_ctx_join in include/frenet_gpu.h for what the caller's stream is ordered after.
    int overlap = 0;
    bool is_twin = false;
    fp_ctx* twin = nullptr;
    hipEvent_t ov_fork = nullptr, ov_done[2] = {nullptr, nullptr};
    bool ov_pending[2] = {false, false};
    int ov_next = 0;
    const void* ov_last_p[12] = {};  // the output arrays of the call in flight on the OTHER internal stream (independence check)
    int overlapped_calls = 0;      // fp_ctx_get_option("overlapped_calls"): dense calls that started without waiting for their predecessor
};

namespace {

// Latency regime: the pinned window goes to the arena by a copy KERNEL (16 bytes per lane, read straight from the pinned host block)
// instead of a copy command: for ~100 KB the copy engine takes ~9 us and the kernel behind it starts ~8 us after the copy ends
// (cross-engine dependency); a kernel-to-kernel dependency on the same queue costs ~2-3 us and the copy itself ~4 us.
__global__ __launch_bounds__(256) void stage_copy_kernel(uint4* __restrict__ dst, const uint4* __restrict__ src, int n16)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

// One call of an entry point, in either memory space.  The entry point declares its arrays once, in list() (frenet_stage_plan.h);
// commit() makes the declarations good, the kernels are launched on stream(), finish() ends the call.
// FP_MEM_HOST: the list stages - commit() places the arrays, sizes the arena from them and brings the inputs over on the ctx's stream,
// finish() brings the outputs back and waits for them.  FP_MEM_DEVICE: the list passes the caller's addresses through, the stream is the
// caller's, commit() and finish() have nothing to do: no arena, no pinned block, no copy, no synchronisation.
// What differs between the two spaces beyond that - checks that look into the arrays, points_max, the launch order - an entry point
// says under host().
class CallStage {
  public:
    CallStage(fp_ctx* ctx, int mem, void* stream) : ctx_(ctx), host_(mem != FP_MEM_DEVICE), stream_(host_ ? ctx->stream : (hipStream_t)stream), list_(!host_) {}

    bool host() const { return host_; }
    hipStream_t stream() const { return stream_; }
    StageList& list() { return list_; }

    // The stream sees: the large inputs, one copy each in declaration order; then the window's flush.  Inputs the kernels address in the
    // pinned block itself need neither.  The default regime is the throughput one: no zero copy.
    int commit(const StageRegime& rg = StageRegime())
    {
        if (!host_) return FP_OK;
        if (list_.overflow()) return fail(FP_EHIP, "internal: a call staged %d arrays, the staging list holds %d", list_.n, fp::kStageCap);
        plan_ = fp::plan_stage(list_, rg);
        zero_copy_out_ = rg.zero_copy_out;
        if (!fp::stage_plan_inside(list_, plan_)) return fail(FP_EHIP, "internal: the staging plan places an array outside the arena it sized");
        FP_TRY(ctx_->arena.reserve(plan_.arena_bytes));
        for (int i = 0; i < list_.n; ++i) {
            const fp::StageItem& it = list_.item[i];
            *it.dev = addr(i);
            if ((it.kind != fp::StageKind::IN && it.kind != fp::StageKind::IN_MUT) || it.bytes == 0) continue;
            if (plan_.region[i] == fp::StageRegion::LARGE) HIP_TRY(hipMemcpyAsync(*it.dev, it.host, it.bytes, hipMemcpyHostToDevice, stream_));
            else memcpy(ctx_->pinned + plan_.offset[i], it.host, it.bytes);
        }
        if (plan_.flush) {  // the arena's copy of the window has to be brought up to date
            // Latency regime: by a copy kernel, see stage_copy_kernel
            if (zero_copy_out_ && ctx_->stage_kernel) {
                const int n16 = (int)((plan_.small_in + 15) / 16);  // (both blocks are 256-byte aligned and kSmallRegion long)
                const int blocks = (n16 + 255) / 256;
                hipLaunchKernelGGL(stage_copy_kernel, dim3(blocks < 512 ? blocks : 512), dim3(256), 0, stream_, (uint4*)ctx_->arena.base, (const uint4*)ctx_->pinned, n16);
                HIP_TRY(hipGetLastError());
            } else {
                HIP_TRY(hipMemcpyAsync(ctx_->arena.base, ctx_->pinned, plan_.small_in, hipMemcpyHostToDevice, stream_));
            }
        }
        return FP_OK;
    }
    // One D2H copy for the output window (none when the kernels wrote the pinned block itself), one per output outside it, the
    // stream's synchronisation, then the host's copies out of the pinned block.
    int finish()
    {
        if (!host_) return FP_OK;
        if (plan_.small_out_hi > plan_.small_out_lo && !zero_copy_out_)
            HIP_TRY(hipMemcpyAsync(ctx_->pinned + plan_.small_out_lo, ctx_->arena.base + plan_.small_out_lo, plan_.small_out_hi - plan_.small_out_lo,
                                   hipMemcpyDeviceToHost, stream_));
        for (int i = 0; i < list_.n; ++i)
            if (returns(i) && !via_pinned(i)) HIP_TRY(hipMemcpyAsync(list_.item[i].host, addr(i), list_.item[i].bytes, hipMemcpyDeviceToHost, stream_));
        HIP_TRY(hipStreamSynchronize(stream_));
        for (int i = 0; i < list_.n; ++i)
            if (returns(i) && via_pinned(i)) memcpy(list_.item[i].host, ctx_->pinned + plan_.offset[i], list_.item[i].bytes);
        return FP_OK;
    }

  private:
    char* addr(int i) const
    {
        if (plan_.region[i] == fp::StageRegion::NONE) return nullptr;
        return (plan_.region[i] == fp::StageRegion::PINNED ? ctx_->pinned : ctx_->arena.base) + plan_.offset[i];
    }
    bool returns(int i) const { return list_.item[i].kind == fp::StageKind::IN_MUT || (list_.item[i].kind == fp::StageKind::OUT && plan_.region[i] != fp::StageRegion::NONE); }
    // (an in/out array of the window was copied in with it, but comes back by a copy of its own)
    bool via_pinned(int i) const { return plan_.region[i] == fp::StageRegion::PINNED || (plan_.region[i] == fp::StageRegion::WINDOW && list_.item[i].kind == fp::StageKind::OUT); }

    fp_ctx* ctx_;
    const bool host_;
    const hipStream_t stream_;
    StageList list_;
    fp::StagePlan plan_;
    bool zero_copy_out_ = false;
};

// "finite and >= 0" / "finite and > 0" of a caller's scalar (a NaN fails both)
bool finite_nonneg(double v) { return v >= 0 && v <= fp::kF64Max; }
bool finite_pos(double v) { return v > 0 && v <= fp::kF64Max; }

int check_params(const fp_params* p)
{
    if (!p) return fail(FP_EINVAL, "params is NULL");
    if (p->nd < 1 || p->nv < 1 || p->nt < 1) return fail(FP_EINVAL, "lattice sizes must be >= 1 (got %d,%d,%d)", p->nd, p->nv, p->nt);
    if ((long)p->nd * p->nv * p->nt > FP_MAX_CAND) return fail(FP_ELIMIT, "nd*nv*nt = %ld exceeds FP_MAX_CAND", (long)p->nd * p->nv * p->nt);
    if (p->check_stride < 1) return fail(FP_EINVAL, "check_stride must be >= 1");
    if (!(p->tick_t > 0)) return fail(FP_EINVAL, "tick_t must be > 0");
    if (p->points_max < 0 || p->points_max > FP_MAX_POINTS) return fail(FP_ELIMIT, "points_max=%d outside 0..FP_MAX_POINTS", p->points_max);
    if (p->curvature_mask && (!(p->max_curvature >= 0) || !(p->max_kappa_d >= 0) || !(p->max_kappa_dd >= 0)))
        return fail(FP_EINVAL, "curvature_mask is set but max_curvature / max_kappa_d / max_kappa_dd are not all >= 0");
    if (!finite_nonneg(p->w_obstacle)) return fail(FP_EINVAL, "w_obstacle must be finite and >= 0");
    return FP_OK;
}

// Series layout of a call: columns per row (0 = FP_DEFAULT_STRIDE).  Host calls can check it against the batch's time samples.
int traj_stride_of(int32_t requested, int* stride)
{
    if (requested < 0) return fail(FP_EINVAL, "traj_stride must be >= 0");
    *stride = requested > 0 ? requested : FP_DEFAULT_STRIDE;
    return FP_OK;
}
int check_stride_host(const fp_params* p, const fp_batch* b, int stride)
{
    for (int k = 0; k < p->nt; ++k)
        if (ceil(b->t_samples[k] / p->tick_t) > stride)
            return fail(FP_EINVAL, "traj_stride=%d is smaller than the %g points of t_samples[%d]=%g", stride, ceil(b->t_samples[k] / p->tick_t), k, b->t_samples[k]);
    return FP_OK;
}

// Points per trajectory of a FP_MEM_HOST call (fp_params.points_max is the device callers' announcement; host calls look themselves):
// the largest ceil(T / tick_t) over the time samples (+ `extra_T`: explicit end states / refinement bounds of the call), 0 when the
// fast paths' FP_FAST_POINTS hold it.
int host_points_max(const fp_params* p, const fp_batch* b, const double* extra_T, size_t n_extra, size_t extra_step)
{
    double n = 0.0;
    for (int k = 0; k < p->nt; ++k) n = fmax(n, ceil(b->t_samples[k] / p->tick_t));
    for (size_t i = 0; i < n_extra; ++i) {
        const double v = ceil(extra_T[i * extra_step] / p->tick_t);
        if (v == v) n = fmax(n, v);
    }
    return n > FP_FAST_POINTS ? (n > FP_MAX_POINTS ? FP_MAX_POINTS : (int)n) : 0;
}
bool big_points(const fp_params& p) { return p.points_max > FP_FAST_POINTS; }

int check_batch(const fp_batch* b, bool need_coef = true)  // (need_coef = false: the caller decides itself whether it reads coef)
{
    if (!b) return fail(FP_EINVAL, "batch is NULL");
    if (b->B < 0 || b->F < 1 || b->NX < 2) return fail(FP_EINVAL, "bad batch sizes B=%d F=%d NX=%d", b->B, b->F, b->NX);
    if (b->NX > FP_MAX_KNOTS) return fail(FP_ELIMIT, "NX=%d exceeds FP_MAX_KNOTS", b->NX);
    if (!b->d_samples || !b->t_samples || !b->v_samples || !b->target_speed || !b->ego || !b->frame_of || !b->scene_of ||
        !b->t_now || !b->nx || !b->knots || (need_coef && !b->coef))
        return fail(FP_EINVAL, "batch has a NULL array");
    if (b->S > 0 && b->n_obs > 0 && (!b->obs_pose || !b->obs_dims || !b->final_time_step))
        return fail(FP_EINVAL, "batch has obstacles but a NULL obstacle array");
    if (b->S > 0 && b->n_obs > 0 && b->obs_nvert) {
        if (!b->obs_poly) return fail(FP_EINVAL, "obs_nvert is set but obs_poly is NULL");
        if (b->poly_stride < 3 || b->poly_stride > FP_MAX_POLY_VERTS) return fail(FP_ELIMIT, "poly_stride=%d outside 3..FP_MAX_POLY_VERTS", b->poly_stride);
    }
    return FP_OK;
}

// Host-side validation of the index arrays (only possible for FP_MEM_HOST calls): the frames the egos sit on ...
int check_frames_host(const fp_batch* b)
{
    for (int i = 0; i < b->B; ++i)
        if (b->frame_of[i] < 0 || b->frame_of[i] >= b->F) return fail(FP_EINVAL, "frame_of[%d]=%d out of range", i, b->frame_of[i]);
    for (int f = 0; f < b->F; ++f)
        if (b->nx[f] < 2 || b->nx[f] > b->NX) return fail(FP_EINVAL, "nx[%d]=%d out of range", f, b->nx[f]);
    return FP_OK;
}

// ... and everything else a planning call reads
int check_batch_host(const fp_params* p, const fp_batch* b, bool past_ok = false)  // (past_ok: the call reads a clock before step 0 like fp_gate_mask)
{
    FP_TRY(check_frames_host(b));
    for (int i = 0; i < b->B; ++i) {
        if (b->scene_of[i] >= b->S) return fail(FP_EINVAL, "scene_of[%d]=%d out of range", i, b->scene_of[i]);
        if (b->t_now[i] < 0 && !past_ok) return fail(FP_EINVAL, "t_now[%d]=%d is negative", i, b->t_now[i]);
    }
    for (int k = 0; k < p->nt; ++k) {
        const double n = b->t_samples[k] / p->tick_t;
        if (!(n > 0) || n > FP_MAX_POINTS) return fail(FP_ELIMIT, "t_samples[%d]=%g needs more than FP_MAX_POINTS points", k, b->t_samples[k]);
    }
    if (b->S > 0 && b->n_obs > 0 && b->obs_nvert) {  // polygon columns: vertex count, ring orientation, and the box the broad phases test
        for (long c = 0; c < (long)b->S * b->n_obs; ++c) {
            const int n = b->obs_nvert[c];
            if (n == 0) continue;
            if (n < 3 || n > b->poly_stride) return fail(FP_EINVAL, "obs_nvert[%ld]=%d outside 3..poly_stride=%d", c, n, b->poly_stride);
            const double* v = b->obs_poly + (size_t)c * 2 * b->poly_stride;
            double mx = 0.0, my = 0.0, area2 = 0.0;
            for (int i = 0; i < n; ++i) {
                const double* a = v + 2 * i;
                const double* q = v + 2 * ((i + 1) % n);
                if (!(a[0] == a[0]) || !(a[1] == a[1])) return fail(FP_EINVAL, "obs_poly column %ld has a NaN vertex", c);
                mx = fmax(mx, fabs(a[0])); my = fmax(my, fabs(a[1]));
                area2 += a[0] * q[1] - a[1] * q[0];
            }
            if (!(area2 > 0.0)) return fail(FP_EINVAL, "obs_poly column %ld is not counter-clockwise (twice its signed area = %g)", c, area2);
            // convex: the narrow phase treats the ring as the intersection of its edge half-planes - a reflex vertex would silently shrink
            // the obstacle to its kernel (missed collisions).  Every turn must be to the left; collinear vertices pass (the tolerance
            // covers the rounding of a cross product of coordinates ~ mx, my).
            const double turn_tol = 64.0 * 2.220446049250313e-16 * (mx + my) * (mx + my);
            for (int i = 0; i < n; ++i) {
                const double* a = v + 2 * i;
                const double* q = v + 2 * ((i + 1) % n);
                const double* r = v + 2 * ((i + 2) % n);
                const double cr = (q[0] - a[0]) * (r[1] - q[1]) - (q[1] - a[1]) * (r[0] - q[0]);
                if (!(cr >= -turn_tol)) return fail(FP_EINVAL, "obs_poly column %ld is not convex (right turn at vertex %d, cross product %g): cut it into convex pieces (obstacles.shape_columns)", c, (i + 1) % n, cr);
            }
            if (!(b->obs_dims[2 * c] >= 2.0 * mx) || !(b->obs_dims[2 * c + 1] >= 2.0 * my))
                return fail(FP_EINVAL, "obs_dims of polygon column %ld (%g x %g) does not contain its vertices (needs %g x %g)", c, b->obs_dims[2 * c], b->obs_dims[2 * c + 1], 2.0 * mx, 2.0 * my);
        }
    }
    return FP_OK;
}

// The lattice's sample arrays, as every kernel that walks the lattice reads them
void stage_samples(StageList& sl, const fp_params* p, const fp_batch* b, const double** d_samples, const double** t_samples, const double** v_samples)
{
    sl.in(b->d_samples, (size_t)p->nd, d_samples);
    sl.in(b->t_samples, (size_t)p->nt, t_samples);
    sl.in(b->v_samples, (size_t)b->B * p->nv, v_samples);
}

// The argument checks of the four rules, shared by each rule's own pass and fp_rules_eval: the same conditions, the same messages.
// The *_host halves look into the arrays, which only a FP_MEM_HOST call can.
int check_corridor(const fp_corridor* corridor)
{
    if (!corridor || !corridor->left || !corridor->right) return fail(FP_EINVAL, "fp_boundary_mask: corridor / left / right must not be NULL");
    if (!finite_nonneg(corridor->margin)) return fail(FP_EINVAL, "fp_boundary_mask: margin must be finite and >= 0");
    return FP_OK;
}
int check_corridor_host(const fp_corridor* corridor, const fp_batch* batch)
{
    for (int f = 0; f < batch->F; ++f)
        for (int k = 0; k < batch->nx[f]; ++k) {
            const double l = corridor->left[(size_t)f * batch->NX + k], r = corridor->right[(size_t)f * batch->NX + k];
            if (!(l == l) || !(r == r)) return fail(FP_EINVAL, "fp_boundary_mask: corridor has a NaN at frame %d, knot %d (+-inf says \"no edge\")", f, k);
        }
    return FP_OK;
}
int check_speed_profile(const fp_speed_profile* profile, const fp_batch* batch)
{
    if (!profile || !profile->v_limit) return fail(FP_EINVAL, "fp_speed_envelope: profile / v_limit must not be NULL");
    if (!finite_nonneg(profile->front)) return fail(FP_EINVAL, "fp_speed_envelope: front must be finite and >= 0");
    if (!finite_nonneg(profile->tol)) return fail(FP_EINVAL, "fp_speed_envelope: tol must be finite and >= 0");
    if (!finite_nonneg(profile->max_lat_accel)) return fail(FP_EINVAL, "fp_speed_envelope: max_lat_accel must be finite and >= 0 (0 = off)");
    if (profile->max_lat_accel > 0 && !batch->coef) return fail(FP_EINVAL, "fp_speed_envelope: max_lat_accel > 0 needs batch->coef");
    return FP_OK;
}
int check_speed_profile_host(const fp_speed_profile* profile, const fp_batch* batch)
{
    for (int f = 0; f < batch->F; ++f)
        for (int k = 0; k + 1 < batch->nx[f]; ++k) {
            const double l = profile->v_limit[(size_t)f * batch->NX + k];
            if (!(l >= 0)) return fail(FP_EINVAL, "fp_speed_envelope: v_limit is %g at frame %d, knot %d (+inf says \"no limit\", 0 \"stop\")", l, f, k);
        }
    return FP_OK;
}
int check_gates(const fp_gates* gates)
{
    if (!gates || !gates->gate_s || !gates->closed) return fail(FP_EINVAL, "fp_gate_mask: gates / gate_s / closed must not be NULL");
    if (gates->gate_stride < 1 || gates->gate_stride > FP_MAX_GATES) return fail(FP_EINVAL, "fp_gate_mask: gate_stride=%d outside 1..FP_MAX_GATES", gates->gate_stride);
    if (gates->T_gate < 1) return fail(FP_EINVAL, "fp_gate_mask: T_gate=%d must be >= 1", gates->T_gate);
    if (!finite_nonneg(gates->front)) return fail(FP_EINVAL, "fp_gate_mask: front must be finite and >= 0");
    if (!finite_nonneg(gates->max_decel)) return fail(FP_EINVAL, "fp_gate_mask: max_decel must be finite and >= 0 (0 = off)");
    return FP_OK;
}
int check_time_gap(const fp_time_gap* gap)
{
    if (!gap) return fail(FP_EINVAL, "fp_gap_mask: gap must not be NULL");
    if (gap->lag_follow < 0 || gap->lag_follow > FP_MAX_POINTS) return fail(FP_EINVAL, "fp_gap_mask: lag_follow=%d outside 0..FP_MAX_POINTS", gap->lag_follow);
    if (gap->lag_lead < 0 || gap->lag_lead > FP_MAX_POINTS) return fail(FP_EINVAL, "fp_gap_mask: lag_lead=%d outside 0..FP_MAX_POINTS", gap->lag_lead);
    if (gap->first < 1) return fail(FP_EINVAL, "fp_gap_mask: first=%d must be >= 1", gap->first);
    return FP_OK;
}
// A rule set (fp_rules_eval, fp_plan_fiss_rules: `fn` names the entry point): some rule is on, and every rule that is on passes its checks
int check_rule_set(const char* fn, const fp_rule_set* rules, const fp_batch* batch)
{
    if (!rules->envelope && !rules->gates && !rules->boundary && !rules->gaps) return fail(FP_EINVAL, "%s: every rule of the set is NULL", fn);
    if (rules->envelope) FP_TRY(check_speed_profile(rules->envelope, batch));
    if (rules->gates) FP_TRY(check_gates(rules->gates));
    if (rules->boundary) FP_TRY(check_corridor(rules->boundary));
    return rules->gaps ? check_time_gap(rules->gaps) : FP_OK;
}
int check_rule_set_host(const fp_rule_set* rules, const fp_batch* batch)
{
    if (rules->envelope) FP_TRY(check_speed_profile_host(rules->envelope, batch));
    return rules->boundary ? check_corridor_host(rules->boundary, batch) : FP_OK;
}

// The loop state of a closed-loop call.  need_goal: the call decides arrivals (fp_loop_record only copies the states).
int check_loop_io(const fp_loop_io* io, bool need_goal)
{
    if (!io || !io->ego || !io->t_now || !io->done || !io->cycles || (need_goal && !io->goal_xy)) return fail(FP_EINVAL, "fp_loop_io has a NULL mandatory array");
    if (need_goal && io->goal_poly && (!io->goal_nv || io->goal_max_vertices < 3)) return fail(FP_EINVAL, "fp_loop_io.goal_poly needs goal_nv and goal_max_vertices >= 3");
    return FP_OK;
}

// The batch as the kernels of an FP_MEM_DEVICE call see it: a batch without scenes or obstacle columns has no obstacles
fp_batch device_batch(const fp_batch* batch)
{
    fp_batch b = *batch;
    if (!(batch->S > 0 && batch->n_obs > 0)) b.n_obs = 0;
    return b;
}

// What differs between the memory spaces in every call that has a batch.  The launch order: an FP_MEM_DEVICE call hands the caller's
// fp_batch.launch_order to its kernel, a host call has none.
const int32_t* launch_order_of(const CallStage& call, const fp_batch* b) { return call.host() ? nullptr : b->launch_order; }

// The argument block the table passes behind the dense pass share (fp::TablePassArgs), declared in the call's list: its scalars, and
// of the arrays only what the kernels read (the lattice samples, the ego states, the knots, the two tables).  `own` declares the entry
// point's own arrays where they have always stood in its list, behind the knots: the order of a list decides the arena's layout
// (plan_stage).  plan_fiss_impl, whose batch and tables are on the device in either space, declares its blocks in a pass-through list.
template <typename Own>
void table_pass_declare(StageList& sl, fp::TablePassArgs* a, const fp_params* p, const fp_batch* b, const int32_t* perm, const double* cost_tbl, uint32_t* flag_tbl,
                        int32_t* best_idx, double* best_cost, int32_t* count, Own own)
{
    const size_t B = (size_t)b->B, C = (size_t)p->nd * p->nv * p->nt;
    a->B = b->B; a->NX = b->NX; a->nd = p->nd; a->nv = p->nv; a->nt = p->nt;
    a->tick_t = p->tick_t;
    a->perm = perm;
    sl.in(b->t_samples, (size_t)p->nt, &a->t_samples);
    sl.in(b->v_samples, B * p->nv, &a->v_samples);
    sl.in(b->ego, B * 6, &a->ego);
    sl.in(b->frame_of, B, &a->frame_of);
    sl.in(b->nx, (size_t)b->F, &a->nx);
    sl.in(b->knots, (size_t)b->F * b->NX, &a->knots);
    own(sl);
    if (b->skip) sl.in(b->skip, B, &a->skip);
    sl.in(cost_tbl, B * C, &a->cost_tbl);
    sl.in_mut(flag_tbl, B * C, &a->flag_tbl);
    sl.out(best_idx, B, &a->best_idx);
    sl.out(best_cost, B, &a->best_cost);
    sl.out(count, B, &a->count);
}

// Inline inputs of a multi-kernel call (fp::InlineIn::publish): besides the eight per-ego arrays of the batch the blob carries
// the call's other small inputs (`extra`), the lattice kernel copies it to a device mirror, and `dev_pub` / the extras' `dev`
// get the mirror's addresses - what the kernels behind the lattice kernel read.  The mirror is an item of the call's list like any
// other: until commit() has placed it (InlineIn::publish), they hold offsets into it and inline_publish() turns them into addresses.
struct InlineExtra { const void* src; size_t bytes; const void** dev; };
template <typename T>
void mirror_address(const T** field, const unsigned char* mirror) { *field = (const T*)(mirror + (size_t)*field); }
void inline_publish(const fp::InlineIn& inl, fp_batch* dev_pub, const InlineExtra* extra, int n_extra)
{
    const unsigned char* mirror = (const unsigned char*)inl.publish;
    mirror_address(&dev_pub->d_samples, mirror); mirror_address(&dev_pub->t_samples, mirror); mirror_address(&dev_pub->v_samples, mirror);
    mirror_address(&dev_pub->target_speed, mirror); mirror_address(&dev_pub->ego, mirror); mirror_address(&dev_pub->frame_of, mirror);
    mirror_address(&dev_pub->scene_of, mirror); mirror_address(&dev_pub->t_now, mirror);
    for (int i = 0; i < n_extra; ++i) mirror_address(extra[i].dev, mirror);
}

// FP_MEM_HOST: appends the batch's arrays to the call's list (`dev` gets their device addresses at commit).  The tables of a tagged batch do not
// use the arena: their upload, if one is due, is enqueued here - ahead of the call's other copies.
int stage_batch(fp_ctx* ctx, StageList& sl, StageRegime& rg, const fp_params* p, const fp_batch* b, fp_batch* dev, fp::InlineIn* inl = nullptr,
                fp_batch* dev_pub = nullptr, const InlineExtra* extra = nullptr, int n_extra = 0)
{
    *dev = *b;
    const bool has_obs = b->S > 0 && b->n_obs > 0;
    const bool has_poly = has_obs && b->obs_nvert != nullptr;
    if (!has_poly) { dev->obs_poly = nullptr; dev->obs_nvert = nullptr; dev->poly_stride = 0; }
    bool tables_resident = false;
    if (b->tables_tag != 0) {
        // the frame / scene tables of a tagged call live in their own device buffer across calls (fp_batch.tables_tag)
        const int key[7] = {b->tables_tag, b->F, b->NX, b->S, b->T_obs, has_obs ? b->n_obs : 0, has_poly ? b->poly_stride : 0};
        const void* src[8] = {b->nx, b->knots, b->coef, b->obs_pose, b->obs_dims, b->final_time_step, b->obs_poly, b->obs_nvert};
        const size_t bytes[8] = {sizeof(int32_t) * (size_t)b->F, sizeof(double) * (size_t)b->F * b->NX, sizeof(double) * (size_t)b->F * 8 * b->NX,
                                 has_obs ? sizeof(double) * (size_t)b->S * b->T_obs * b->n_obs * 4 : 0, has_obs ? sizeof(double) * (size_t)b->S * b->n_obs * 2 : 0,
                                 has_obs ? sizeof(int32_t) * (size_t)b->S : 0, has_poly ? sizeof(double) * (size_t)b->S * b->n_obs * 2 * b->poly_stride : 0,
                                 has_poly ? sizeof(int32_t) * (size_t)b->S * b->n_obs : 0};
        fp_ctx::TableSet* ts = nullptr;
        fp_ctx::TableSet* lru = &ctx->tables[0];
        for (auto& t : ctx->tables) {
            if (memcmp(key, t.key, sizeof(key)) == 0) { ts = &t; break; }
            if (t.used < lru->used) lru = &t;
        }
        if (!ts) {  // upload into the least recently used set
            ts = lru;
            size_t total = 0;
            for (int i = 0; i < 8; ++i) { ts->off[i] = total; total += align_up(bytes[i]); }
            ts->key[0] = 0;  // (nothing valid while the upload is being set up)
            if (total + kAlign > ts->buf.cap) {
                HIP_TRY(hipStreamSynchronize(ctx->stream));
                FP_TRY(ts->buf.reserve(total + kAlign));
            }
            for (int i = 0; i < 8; ++i)
                if (bytes[i]) HIP_TRY(hipMemcpyAsync(ts->buf.base + ts->off[i], src[i], bytes[i], hipMemcpyHostToDevice, ctx->stream));
            memcpy(ts->key, key, sizeof(key));
        }
        ts->used = ++ctx->tables_tick;
        char* tb = ts->buf.base;
        dev->nx = (const int32_t*)(tb + ts->off[0]);
        dev->knots = (const double*)(tb + ts->off[1]);
        dev->coef = (const double*)(tb + ts->off[2]);
        dev->obs_pose = (const double*)(tb + ts->off[3]);
        dev->obs_dims = (const double*)(tb + ts->off[4]);
        dev->final_time_step = (const int32_t*)(tb + ts->off[5]);
        if (has_poly) { dev->obs_poly = (const double*)(tb + ts->off[6]); dev->obs_nvert = (const int32_t*)(tb + ts->off[7]); }
        tables_resident = true;
        rg.small_inputs_only = true;
    }
#define PUSH(field, count) sl.in(b->field, (size_t)(count), &dev->field)
    // Inline inputs (fp::InlineIn): with the tables resident, what is left of a tiny batch fits the kernel's argument block
    bool inlined = false;
    if (inl && tables_resident && rg.zero_copy_out && !b->skip) {
        const void* src[8] = {b->d_samples, b->t_samples, b->v_samples, b->target_speed, b->ego, b->frame_of, b->scene_of, b->t_now};
        const size_t bytes[8] = {sizeof(double) * (size_t)p->nd, sizeof(double) * (size_t)p->nt, sizeof(double) * (size_t)b->B * p->nv, sizeof(double) * (size_t)b->B,
                                 sizeof(double) * (size_t)b->B * 6, sizeof(int32_t) * (size_t)b->B, sizeof(int32_t) * (size_t)b->B, sizeof(int32_t) * (size_t)b->B};
        size_t off[8], total = 0;
        for (int i = 0; i < 8; ++i) { off[i] = total; total += (bytes[i] + 7) & ~(size_t)7; }
        size_t total_x = total;
        for (int i = 0; i < n_extra; ++i) total_x += (extra[i].bytes + 7) & ~(size_t)7;
        if ((dev_pub ? total_x : total) <= (size_t)fp::kInlineMax) {
            for (int i = 0; i < 8; ++i) memcpy(inl->bytes + off[i], src[i], bytes[i]);
            dev->d_samples = (const double*)off[0]; dev->t_samples = (const double*)off[1]; dev->v_samples = (const double*)off[2];
            dev->target_speed = (const double*)off[3]; dev->ego = (const double*)off[4]; dev->frame_of = (const int32_t*)off[5];
            dev->scene_of = (const int32_t*)off[6]; dev->t_now = (const int32_t*)off[7];
            inl->on = 1;
            inlined = true;
            if (dev_pub) {  // the device mirror the lattice kernel fills for the kernels behind it (addresses: inline_publish)
                sl.temp(fp::kInlineMax, (unsigned char**)&inl->publish);
                *dev_pub = *dev;
                size_t o = total;
                for (int i = 0; i < n_extra; ++i) {
                    memcpy(inl->bytes + o, extra[i].src, extra[i].bytes);
                    *extra[i].dev = (const void*)o;
                    o += (extra[i].bytes + 7) & ~(size_t)7;
                }
                inl->n8 = (int)((total_x + 7) / 8);
            }
        }
    }
    if (!inlined) {
        stage_samples(sl, p, b, &dev->d_samples, &dev->t_samples, &dev->v_samples);
        PUSH(target_speed, b->B);
        PUSH(ego, (size_t)b->B * 6);
        PUSH(frame_of, b->B);
        PUSH(scene_of, b->B);
        PUSH(t_now, b->B);
    }
    if (!tables_resident) {
        PUSH(nx, b->F);
        PUSH(knots, (size_t)b->F * b->NX);
        PUSH(coef, (size_t)b->F * 8 * b->NX);
        PUSH(obs_pose, has_obs ? (size_t)b->S * b->T_obs * b->n_obs * 4 : 0);
        PUSH(obs_dims, has_obs ? (size_t)b->S * b->n_obs * 2 : 0);
        PUSH(final_time_step, has_obs ? b->S : 0);
        if (has_poly) {
            PUSH(obs_poly, (size_t)b->S * b->n_obs * 2 * b->poly_stride);
            PUSH(obs_nvert, (size_t)b->S * b->n_obs);
        }
    }
    if (b->skip) PUSH(skip, b->B);
#undef PUSH
    if (!has_obs) dev->n_obs = 0;
    if (!has_obs && dev_pub && inlined) dev_pub->n_obs = 0;
    return FP_OK;
}

// The batch of a call in either space.  FP_MEM_HOST: stage_batch.  FP_MEM_DEVICE: the caller's struct - as it stands (AS_GIVEN), or as
// device_batch sees it (NO_OBS_WITHOUT_SCENES) for the kernels that walk obstacle columns; nothing is enqueued.
enum class DeviceView { AS_GIVEN, NO_OBS_WITHOUT_SCENES };
int stage_batch(fp_ctx* ctx, CallStage& call, StageRegime& rg, const fp_params* p, const fp_batch* b, fp_batch* dev, DeviceView view)
{
    if (call.host()) return stage_batch(ctx, call.list(), rg, p, b, dev);
    *dev = view == DeviceView::AS_GIVEN ? *b : device_batch(b);
    return FP_OK;
}

// Launch order of a multi-round lattice launch (more egos than resident workgroups, one workgroup per ego).  Called right before
// the launch: hands out the permutation to dispatch in (nullptr = index order) and the array the workgroups leave their durations
// in.  Host work happens only when a fetched duration table has arrived (hipEventQuery, no wait): an argsort of B ints.
int launch_order_before(fp_ctx* ctx, OrderSet& set, int resident, const fp_batch* b, int nsplit, hipStream_t stream, const int** perm, int** dur,
                        const int* hint = nullptr, LaunchOrder** slot = nullptr)
{
    *perm = nullptr;
    *dur = nullptr;
    if (slot) *slot = nullptr;
    const bool lattice = &set == &ctx->order_lattice;
    if (lattice) ++ctx->lattice_launches;
    if (nsplit != 1 || b->B <= resident) return FP_OK;
    // Priority: the order learnt on THIS batch (exact history) > fp_batch.launch_order (the caller's input-only hint) > index order.
    // Durations are collected under a hint too, so a hinted batch moves on to its own order once it has one.
    if (!ctx->lattice_order) {
        if (hint) { *perm = hint; if (lattice) ++ctx->lattice_ordered_launches; }
        return FP_OK;
    }
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess) (void)hipGetLastError();
    const bool capturing = cap != hipStreamCaptureStatusNone;
    LaunchOrder& o = set.of(b->ego);
    if (slot) *slot = &o;
    if (b->B > o.cap) {
        if (capturing) {  // no (re)allocation inside a capture: the hint, or index order
            if (hint) { *perm = hint; if (lattice) ++ctx->lattice_ordered_launches; }
            if (slot) *slot = nullptr;
            return FP_OK;
        }
        if (o.pending) { HIP_TRY(hipEventSynchronize(o.event)); o.pending = false; }
        HIP_TRY(hipStreamSynchronize(stream));
        const int cap_new = b->B + b->B / 4;
        FP_TRY(o.buf.reserve((size_t)cap_new * 2 * sizeof(int)));
        if (o.host) (void)hipHostFree(o.host);
        o.host = nullptr;
        HIP_TRY(hipHostMalloc((void**)&o.host, (size_t)cap_new * 2 * sizeof(int), hipHostMallocDefault));
        if (!o.event) HIP_TRY(hipEventCreateWithFlags(&o.event, hipEventDisableTiming));
        o.cap = cap_new;
        o.valid_B = o.dur_B = 0;
        o.since = 0;
    }
    int* d_dur = (int*)o.buf.base;
    int* d_perm = d_dur + o.cap;
    if (!capturing && o.pending && hipEventQuery(o.event) == hipSuccess) {
        o.pending = false;
        const int n = o.dur_B;
        if (n == b->B) {  // longest first; ties in index order (std::stable_sort keeps the result deterministic)
            const int* h_dur = o.host;
            int* h_perm = o.host + o.cap;
            for (int i = 0; i < n; ++i) h_perm[i] = i;
            std::stable_sort(h_perm, h_perm + n, [h_dur](int x, int y) { return h_dur[x] > h_dur[y]; });
            HIP_TRY(hipMemcpyAsync(d_perm, h_perm, (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream));
            if (o.valid_B == n) o.interval = o.interval * 2 < kOrderRefreshMax ? o.interval * 2 : kOrderRefreshMax;
            o.valid_B = n;
        }
    } else if (o.pending) {
        (void)hipGetLastError();  // hipErrorNotReady is not an error
    }
    if (o.valid_B == b->B) *perm = d_perm;
    else if (hint) *perm = hint;
    *dur = d_dur;
    if (lattice && *perm) ++ctx->lattice_ordered_launches;
    return FP_OK;
}

// Right after the launch: every kOrderRefresh launches enqueue the fetch of the durations this launch leaves behind.
int launch_order_after(LaunchOrder* op, const fp_batch* b, const int* dur, hipStream_t stream)
{
    if (!dur || !op) return FP_OK;
    LaunchOrder& o = *op;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess) (void)hipGetLastError();
    if (cap != hipStreamCaptureStatusNone || o.pending) return FP_OK;
    const bool first = o.valid_B != b->B;  // no order for this batch size yet: fetch at once
    if (first) o.interval = kOrderRefresh;
    if (!first && ++o.since < o.interval) return FP_OK;
    o.since = 0;
    HIP_TRY(hipMemcpyAsync(o.host, dur, (size_t)b->B * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(o.event, stream));
    o.dur_B = b->B;
    o.pending = true;
    return FP_OK;
}

// Latency mode: a small batch cannot fill 256 CUs with one workgroup per ego, so the time-horizon slices of every ego are
// spread over nt workgroups.  Returns the split factor and makes sure the partial-argmin buffer exists.
int lattice_split_for(fp_ctx* ctx, const fp_params* p, const fp_batch* b, hipStream_t stream, int* nsplit, void** parts, int* group, int* tail)
{
    *nsplit = 1;
    *parts = nullptr;
    *group = 1;
    *tail = 0;
    // auto: as many workgroups per ego as keep ALL workgroups resident at once (measured on MI355X: 1.6-2.5x faster up to that
    // point, slower beyond it - a second round of workgroups costs more than the shorter critical path saves); at most one
    // workgroup per slice
    int parts_per_ego = p->nt;
    if (ctx->lattice_split == 0) {
        const long fit = b->B > 0 ? ctx->resident_groups / (long)b->B : 0;
        parts_per_ego = (int)(fit < p->nt ? fit : p->nt);
        // without obstacles the slices carry no work: one workgroup per ego
        if (parts_per_ego < p->nt && !(b->S > 0 && b->n_obs > 0)) parts_per_ego = 1;
    } else if (ctx->lattice_split == 1) {
        parts_per_ego = 1;
    }
    // Grouped instances (launch_lattice_fused, `group`): when the batch leaves room for no more than TWO workgroups per ego but every
    // ego can have a CU to itself, one 1024-thread workgroup per ego takes all its slices - twice the wavefronts on its lon
    // profiles, one prologue instead of two, no ticket and no merge.  Measured on MI355X (BASELINE configs[1], 5 x 5 x 5,
    // 10 obstacles; with the kernel organisation of the time): 256 egos 36.3 us against 37.9 split in two; 128 egos (split in
    // four) 34.5 against 31.3 - so only in that regime.  Needs lattice_group_fit to grant all nt slices.
    const bool obstacles = b->S > 0 && b->n_obs > 0;
    if (ctx->lattice_group >= 2) {
        *group = ctx->lattice_group;
    } else if (ctx->lattice_group == 0 && ctx->lattice_split == 0 && obstacles && p->nt > 2 && parts_per_ego == 2 &&
               (long)b->B * 2 <= ctx->resident_groups && fp::lattice_group_fit(*p, *b) >= p->nt) {
        *group = p->nt;
        parts_per_ego = 1;
    }
    // Tail split (launch_lattice_fused, `tail`): a launch of several rounds of one-workgroup egos cuts its last slots in two
    const bool want_tail = parts_per_ego < 2 && *group == 1 && ctx->lattice_tail != 1 && obstacles && p->nt >= 2 &&
                           (ctx->lattice_tail >= 2 || b->B > ctx->resident_groups);
    if ((parts_per_ego < 2 && !want_tail) || p->nt < 2) return FP_OK;
    // want implies a small batch or an explicit request: the counters get a fixed region in front (kTicketBytes) so that they
    // never share bytes with the partial argmins of a call with another B
    if ((size_t)b->B * 4 > fp::kTicketBytes) return FP_OK;  // (an explicitly requested split of a huge batch: not worth it)
    const size_t need = fp::kTicketBytes + (size_t)b->B * p->nt * 16 + kAlign;
    if (need > ctx->parts.cap) {
        if (want_tail) {  // an optimisation only: never (re)allocate inside a stream capture for it
            hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(stream, &cap) != hipSuccess) (void)hipGetLastError();
            if (cap != hipStreamCaptureStatusNone) return FP_OK;
        }
        HIP_TRY(hipStreamSynchronize(stream));  // the buffer is reallocated: drain its users
        FP_TRY(ctx->parts.reserve(need));
        // ticket counters start at zero; every launch leaves them at zero
        HIP_TRY(hipMemsetAsync(ctx->parts.base, 0, fp::kTicketBytes, stream));
    }
    *nsplit = parts_per_ego < 2 ? 1 : parts_per_ego;
    *parts = ctx->parts.base;
    if (want_tail) *tail = ctx->lattice_tail >= 2 ? ctx->lattice_tail : -(ctx->resident_groups / 2);  // (auto: the launcher knows the residency)
    return FP_OK;
}

// Device copy of best_idx for a dense call whose winner series come from winner_traj_kernel (KernelArgs::idx_shadow); nullptr
// when the buffer would have to grow inside a stream capture (the epilogue then reads the caller's array).
int32_t* idx_shadow_for(fp_ctx* ctx, size_t B, hipStream_t stream)
{
    if (B * sizeof(int32_t) > ctx->idx_shadow.cap) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cap) != hipSuccess) (void)hipGetLastError();
        if (cap != hipStreamCaptureStatusNone) return nullptr;
        if (hipStreamSynchronize(stream) != hipSuccess || ctx->idx_shadow.reserve(B * sizeof(int32_t)) != FP_OK) {
            (void)hipGetLastError();
            return nullptr;
        }
    }
    return (int32_t*)ctx->idx_shadow.base;
}

// Hand-over flags for the epilogue workgroups a multi-round fused lattice launch appends to its grid (KernelArgs::epi_flag): zero when
// allocated, and every launch leaves them zero.  nullptr when the buffer would have to grow inside a stream capture (the series then
// come from winner_traj_kernel).
int32_t* epi_flags_for(fp_ctx* ctx, size_t B, hipStream_t stream)
{
    if (B * sizeof(int32_t) > ctx->epi_flags.cap) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cap) != hipSuccess) (void)hipGetLastError();
        if (cap != hipStreamCaptureStatusNone) return nullptr;
        if (hipStreamSynchronize(stream) != hipSuccess || ctx->epi_flags.reserve(B * sizeof(int32_t)) != FP_OK ||
            hipMemsetAsync(ctx->epi_flags.base, 0, ctx->epi_flags.cap, stream) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
    }
    return (int32_t*)ctx->epi_flags.base;
}

// A hand-over of an earlier launch on this ctx timed out (fp_ctx::hand_err): the flags are reset in stream order, appended workgroups
// are not offered again on this ctx (winner_traj_kernel / the search kernel take over), and the caller learns that the outputs of that
// earlier call were incomplete.  FP_OK when nothing happened.
bool handover_failed(const fp_ctx* ctx) { return ctx->hand_err && *(volatile int32_t*)ctx->hand_err != 0; }
int handover_recover(fp_ctx* ctx, hipStream_t stream)
{
    const int code = *(volatile int32_t*)ctx->hand_err;
    ctx->appended_ok = false;
    // Inside a stream capture nothing may synchronise (and nothing runs): appended workgroups are off from here on, the word stays set,
    // and the first call outside a capture reports and clears it.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess) (void)hipGetLastError();
    if (cap != hipStreamCaptureStatusNone) return FP_OK;
    // (the launch that timed out may still hold workgroups about to give up too: drain the stream before the word is cleared, or one of
    // them would set it again and a later, healthy call would report a failure of its own)
    (void)hipStreamSynchronize(stream);
    *(volatile int32_t*)ctx->hand_err = 0;
    if (ctx->epi_flags.base) HIP_TRY(hipMemsetAsync(ctx->epi_flags.base, 0, ctx->epi_flags.cap, stream));
    return fail(FP_EHIP, "a %s workgroup appended to an earlier lattice launch on this ctx waited 2 s for its ego's results and gave up: that call's "
                         "%s incomplete; the ctx now runs them in their own launches (call again)",
                code == 2 ? "FISS+ search" : "winner-series", code == 2 ? "FISS+ outputs are" : "series are");
}
int handover_check(fp_ctx* ctx, hipStream_t stream) { return handover_failed(ctx) ? handover_recover(ctx, stream) : FP_OK; }

// The ctx's launch hints and hand-over error word, in the KernelArgs of a call that launches the lattice kernel.
void ctx_lattice_args(const fp_ctx* ctx, fp::KernelArgs* ka)
{
    ka->err_word = ctx->hand_err;
    ka->occ_cap = ctx->lattice_occupancy; ka->resident2 = ctx->resident_groups; ka->lds_cu_kb = ctx->lds_cu_kb; ka->handover_timeout_us = ctx->handover_timeout_us;
}

// The lattice pass of a call: curvature table, split, launch order, the launch of kl and the order's feedback.  kl carries the
// offers of the KernelArgs (the series inside, epilogue workgroups, the loop hand-over); inl / ft offer inline inputs and the
// appended FISS+ search (either may be nullptr); *res says what the launch took.
int lattice_step(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, fp::KernelArgs kl, hipStream_t stream, int which, const int* hint,
                 const fp::InlineIn* inl, const fp::FissTail* ft, fp::LatticeResult* res, bool provisional = false)
{
    if (params->curvature_mask) {  // optional curvature checks: the fused lattice kernel reads them from a [B][C] byte table it fills first
        const size_t need = (size_t)batch->B * params->nd * params->nv * params->nt + kAlign;
        if (need > ctx->curv_buf.cap) {
            HIP_TRY(hipStreamSynchronize(stream));  // the buffer is reallocated: drain its users
            FP_TRY(ctx->curv_buf.reserve(need));
        }
        kl.curv_tbl = (const uint8_t*)ctx->curv_buf.base;
    }
    fp::LatticeRequest rq;
    FP_TRY(lattice_split_for(ctx, params, batch, stream, &rq.nsplit, &rq.part_scratch, &rq.group, &rq.tail));
    LaunchOrder* oslot = nullptr;
    FP_TRY(launch_order_before(ctx, ctx->order_lattice, ctx->resident_groups, batch, rq.nsplit, stream, &rq.perm, &rq.dur, hint, &oslot));
    rq.inl = inl; rq.ft = ft; rq.provisional = provisional;
    LAUNCH_TRY(fp::launch_lattice(kl, stream, which, rq, res), "lattice kernel");
    return launch_order_after(oslot, batch, rq.dur, stream);
}

// Where the winner's series is written: by the lattice kernel's own workgroup (no second launch: what a single plan() call wants)
// or by winner_traj_kernel right behind it.  In a multi-round launch (more egos than resident workgroups) the epilogue - one
// wavefront's dependent chain of ~4 us - holds the workgroup's slot while the next ego waits for it; as its own launch the same
// work runs on idle SIMDs next to nothing else.
bool winner_inside_lattice(const fp_ctx* ctx, const fp_batch* b)
{
    if (ctx->lattice_winner == 1) return true;
    if (ctx->lattice_winner == 2) return false;
    return b->B <= ctx->resident_groups;
}

// The clearance cost term (fp_params.w_obstacle > 0) behind the lattice pass of a dense call: survivors re-priced in ka's tables, the
// ego's argmin over the new costs in best_idx / best_cost (and the shadow the winner kernel reads).
int clearance_step(fp_ctx* ctx, const fp::KernelArgs& ka, const int32_t* launch_order, hipStream_t stream)
{
    LAUNCH_TRY(fp::launch_clearance_rescore(ka, launch_order, stream), "clearance rescoring kernel");
    ++ctx->clearance_launches;
    return FP_OK;
}

// The launch of each rule's table pass and its counter: the pass's entry point (both memory modes) and plan_fiss_impl go through here
int envelope_pass(fp_ctx* ctx, const fp::EnvelopeArgs& a, hipStream_t stream)
{
    LAUNCH_TRY(fp::launch_speed_envelope(a, stream), "speed-envelope kernel");
    ++ctx->envelope_launches;
    return FP_OK;
}
int gate_pass(fp_ctx* ctx, const fp::GateArgs& a, hipStream_t stream)
{
    LAUNCH_TRY(fp::launch_gate_mask(a, stream), "gate kernel");
    ++ctx->gate_launches;
    return FP_OK;
}
int boundary_pass(fp_ctx* ctx, const fp::BoundaryArgs& a, hipStream_t stream)
{
    LAUNCH_TRY(fp::launch_boundary_mask(a, stream), "road-boundary kernel");
    ++ctx->boundary_launches;
    return FP_OK;
}
int gap_pass(fp_ctx* ctx, const fp::KernelArgs& ka, const fp::GapArgs& g, hipStream_t stream)
{
    LAUNCH_TRY(fp::launch_gap_mask(ka, g, stream), "time-gap kernel");
    ++ctx->gap_launches;
    return FP_OK;
}

fp_result no_result() { return fp_result{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0}; }

// FopPlusPlanner counts pops over the dense tables, the audit and the clearance rescoring walk them: when the caller did not ask
// for them they live in the ctx's scratch buffer.
int fopplus_tables(fp_ctx* ctx, size_t B, size_t C, fp_result* r, hipStream_t stream)
{
    const size_t need = align_up(sizeof(double) * B * C) + align_up(sizeof(uint32_t) * B * C);
    if (need > ctx->scratch.cap) {  // growing the buffer frees the old one: not inside a stream capture, and not under its users
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cap) != hipSuccess) (void)hipGetLastError();
        if (cap != hipStreamCaptureStatusNone) return fail(FP_EINVAL, "result.fopplus / result.audit / w_obstacle: the ctx's table scratch must grow - run one call of this size outside the stream capture first");
        HIP_TRY(hipStreamSynchronize(stream));
    }
    FP_TRY(ctx->scratch.reserve(need));
    char* sp = (char*)ctx->scratch.base;
    if (!r->cost_tbl) r->cost_tbl = (double*)sp;
    if (!r->flag_tbl) r->flag_tbl = (uint32_t*)(sp + align_up(sizeof(double) * B * C));
    return FP_OK;
}

// The checks of check_batch_host on arrays that live in device memory (fp_ctx_set_option("validate", 1)): one lane per ego / frame /
// time sample, the first failing check wins.  err[0] = 0: clean.
__global__ void validate_batch_kernel(fp_params p, fp_batch b, int* err)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int code = 0;
    if (i < b.B) {
        const int f = b.frame_of[i], sc = b.scene_of[i];
        if (f < 0 || f >= b.F) code = 1;
        else if (sc >= b.S) code = 2;
        else if (b.t_now[i] < 0) code = 3;
    }
    if (!code && i < b.F && (b.nx[i] < 2 || b.nx[i] > b.NX)) code = 4;
    if (!code && i < p.nt) {
        const double n = b.t_samples[i] / p.tick_t;
        if (!(n > 0) || n > FP_MAX_POINTS) code = 5;
    }
    // the launch-order hint: a permutation of 0 .. B-1 (an entry out of range would be read as an ego; a repeated one plans an ego twice and
    // another not at all).  marks: [B] zeros behind the error words.
    if (!code && b.launch_order && i < b.B) {
        const int e = b.launch_order[i];
        if (e < 0 || e >= b.B) code = 11;
        else if (atomicAdd(&err[2 + e], 1) != 0) code = 12;
    }
    // polygon columns, one lane per column: a vertex count outside {0} u [3, poly_stride] would walk off the ring table; a ring that is
    // not counter-clockwise and convex, or that reaches outside the box of obs_dims, would be tested as a smaller shape than it is
    // (check_batch_host's checks, same tolerances)
    if (!code && b.obs_nvert && b.S > 0 && b.n_obs > 0) {
        const long cols = (long)b.S * b.n_obs;
        for (long c = i; c < cols && !code; c += (long)gridDim.x * blockDim.x) {
            const int n = b.obs_nvert[c];
            if (n == 0) continue;
            if (n < 3 || n > b.poly_stride) code = 6;
            else {
                const double* v = b.obs_poly + (size_t)c * 2 * b.poly_stride;
                double mx = 0.0, my = 0.0, area2 = 0.0;
                bool nan = false;
                for (int k = 0; k < n; ++k) {
                    const double* a = v + 2 * k;
                    const double* q = v + 2 * ((k + 1) % n);
                    nan = nan || !(a[0] == a[0]) || !(a[1] == a[1]);
                    mx = fmax(mx, fabs(a[0])); my = fmax(my, fabs(a[1]));
                    area2 += a[0] * q[1] - a[1] * q[0];
                }
                const double turn_tol = 64.0 * 2.220446049250313e-16 * (mx + my) * (mx + my);
                bool convex = true;
                for (int k = 0; k < n; ++k) {
                    const double* a = v + 2 * k;
                    const double* q = v + 2 * ((k + 1) % n);
                    const double* r = v + 2 * ((k + 2) % n);
                    convex = convex && ((q[0] - a[0]) * (r[1] - q[1]) - (q[1] - a[1]) * (r[0] - q[0]) >= -turn_tol);
                }
                if (nan) code = 7;
                else if (!(area2 > 0.0)) code = 8;
                else if (!convex) code = 9;
                else if (!(b.obs_dims[2 * c] >= 2.0 * mx) || !(b.obs_dims[2 * c + 1] >= 2.0 * my)) code = 10;
            }
            if (code) { if (atomicCAS(&err[0], 0, code) == 0) err[1] = (int)c; return; }
        }
    }
    if (code && atomicCAS(&err[0], 0, code) == 0) err[1] = i;
}

static size_t batch_marks(const fp_batch* b) { return b->launch_order && b->B > 0 ? (size_t)b->B : 0; }

int device_validate(fp_ctx* ctx, const fp_params* p, const fp_batch* b, hipStream_t stream)
{
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t marks = batch_marks(b);
    FP_TRY(ctx->validate_buf.reserve((2 + marks) * sizeof(int)));
    if (!ctx->validate_host) HIP_TRY(hipHostMalloc((void**)&ctx->validate_host, 2 * sizeof(int), hipHostMallocDefault));
    int* d_err = (int*)ctx->validate_buf.base;
    HIP_TRY(hipMemsetAsync(d_err, 0, (2 + marks) * sizeof(int), stream));
    int n = b->B > b->F ? b->B : b->F;
    if (p->nt > n) n = p->nt;
    if (b->obs_nvert && b->S > 0 && b->n_obs > 0) {  // (polygon columns: a lane per column, grid-stride beyond 64 K lanes)
        const long cols = (long)b->S * b->n_obs;
        const int want = (int)(cols < 65536 ? cols : 65536);
        if (want > n) n = want;
    }
    hipLaunchKernelGGL(validate_batch_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, *p, *b, d_err);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ctx->validate_host, d_err, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));  // the price of the option: the call waits for the stream
    const int code = ctx->validate_host[0], at = ctx->validate_host[1];
    switch (code) {
        case 0: return FP_OK;
        case 1: return fail(FP_EINVAL, "frame_of[%d] out of range (device batch, F=%d)", at, b->F);
        case 2: return fail(FP_EINVAL, "scene_of[%d] out of range (device batch, S=%d)", at, b->S);
        case 3: return fail(FP_EINVAL, "t_now[%d] is negative (device batch)", at);
        case 4: return fail(FP_EINVAL, "nx[%d] out of range (device batch, NX=%d)", at, b->NX);
        case 6: return fail(FP_EINVAL, "obs_nvert[%d] outside {0} and 3..poly_stride=%d (device batch)", at, b->poly_stride);
        case 7: return fail(FP_EINVAL, "obs_poly column %d has a NaN vertex (device batch)", at);
        case 8: return fail(FP_EINVAL, "obs_poly column %d is not counter-clockwise (device batch)", at);
        case 9: return fail(FP_EINVAL, "obs_poly column %d is not convex (device batch): cut it into convex pieces (obstacles.shape_columns)", at);
        case 10: return fail(FP_EINVAL, "obs_dims of polygon column %d does not contain its vertices (device batch)", at);
        case 11: return fail(FP_EINVAL, "launch_order[%d] is outside 0 .. B-1 (device batch, B=%d)", at, b->B);
        case 12: return fail(FP_EINVAL, "launch_order[%d] repeats an ego: not a permutation (device batch)", at);
        default: return fail(FP_ELIMIT, "t_samples[%d] needs more than FP_MAX_POINTS points (device batch)", at);
    }
}

// Orders `stream` after every overlapped dense call still in flight on the ctx's internal streams ("overlap").
int overlap_join(fp_ctx* ctx, hipStream_t stream)
{
    for (int k = 0; k < 2; ++k)
        if (ctx->ov_pending[k]) {
            HIP_TRY(hipStreamWaitEvent(stream, ctx->ov_done[k], 0));
            ctx->ov_pending[k] = false;
        }
    return FP_OK;
}

int common_checks(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, int mem, void* stream = nullptr, bool need_coef = true)
{
    if (!ctx) return fail(FP_EINVAL, "ctx is NULL");
    // any entry point but the overlapped dense path itself first joins what that path left in flight: its inputs may be those calls' outputs
    if (ctx->ov_pending[0] || ctx->ov_pending[1]) FP_TRY(overlap_join(ctx, mem == FP_MEM_DEVICE ? (hipStream_t)stream : ctx->stream));
    FP_TRY(check_params(params));
    FP_TRY(check_batch(batch, need_coef));
    if (mem != FP_MEM_HOST && mem != FP_MEM_DEVICE) return fail(FP_EINVAL, "mem must be FP_MEM_HOST or FP_MEM_DEVICE");
    if (mem == FP_MEM_DEVICE && ctx->validate && batch->B > 0) FP_TRY(device_validate(ctx, params, batch, (hipStream_t)stream));
    return FP_OK;
}

// "overlap": the options the twin ctx must share with its owner (everything a dense call reads)
void overlap_sync_options(fp_ctx* twin, const fp_ctx* ctx)
{
    twin->lattice_kernel = ctx->lattice_kernel; twin->lattice_split = ctx->lattice_split; twin->lattice_occupancy = ctx->lattice_occupancy;
    twin->lattice_tail = ctx->lattice_tail; twin->lattice_group = ctx->lattice_group; twin->lattice_winner = ctx->lattice_winner;
    twin->lattice_order = ctx->lattice_order; twin->resident_groups = ctx->resident_groups; twin->lds_cu_kb = ctx->lds_cu_kb;
    twin->validate = ctx->validate;
    twin->refine_table_kb = ctx->refine_table_kb; twin->fiss_stages = ctx->fiss_stages; twin->fiss_jump = ctx->fiss_jump; twin->fiss_fused = ctx->fiss_fused;
    twin->handover_timeout_us = ctx->handover_timeout_us;
    if (!ctx->appended_ok) twin->appended_ok = false;
}

// The arrays a call writes (NULL entries write nothing), for the independence check of "overlap"
struct OverlapOuts {
    const void* p[12] = {};
    bool disjoint(const void* const (&o)[12]) const
    {
        for (const void* x : p)
            for (const void* y : o)
                if (x && x == y) return false;
        return true;
    }
};
OverlapOuts overlap_outs(const fp_result& a)
{
    OverlapOuts o;
    const void* v[] = {a.best_idx, a.best_cost, a.cost_tbl, a.flag_tbl, a.stats, a.best_flags, a.best_traj, a.fopplus, a.audit};
    for (int i = 0; i < 9; ++i) o.p[i] = v[i];
    return o;
}
OverlapOuts overlap_outs(const fp_fiss_io& a)
{
    OverlapOuts o;
    const void* v[] = {a.prev_best_idx, a.best_ijk, a.best_cost, a.end_state, a.refined, a.stats, a.trace, a.best_flags, a.best_traj};
    for (int i = 0; i < 9; ++i) o.p[i] = v[i];
    return o;
}

// "overlap": runs `impl(target ctx, its internal stream)` on the internal stream the previous overlapped call did NOT use.  The internal
// stream is ordered after everything the caller has enqueued on `stream` so far; `stream` is ordered after the call BEFORE this one (the
// deferred join: two calls in flight at most).  A call that writes an array its predecessor writes is not independent: it joins first
// and runs behind it.
template <class Impl>
int overlapped_call(fp_ctx* ctx, hipStream_t stream, const OverlapOuts& outs, Impl&& impl)
{
    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->twin) {
        fp_ctx* tw = nullptr;
        FP_TRY(fp_ctx_create(ctx->device, &tw));
        tw->is_twin = true;
        ctx->twin = tw;
        for (hipEvent_t* e : {&ctx->ov_fork, &ctx->ov_done[0], &ctx->ov_done[1]}) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    const int k = ctx->ov_next;
    fp_ctx* target = k ? ctx->twin : ctx;
    if (k) overlap_sync_options(ctx->twin, ctx);
    const bool independent = !ctx->ov_pending[k ^ 1] || outs.disjoint(ctx->ov_last_p);
    if (!independent) FP_TRY(overlap_join(ctx, stream));
    else if (ctx->ov_pending[k ^ 1]) ++ctx->overlapped_calls;
    HIP_TRY(hipEventRecord(ctx->ov_fork, stream));
    HIP_TRY(hipStreamWaitEvent(target->stream, ctx->ov_fork, 0));
    const bool keep[2] = {ctx->ov_pending[0], ctx->ov_pending[1]};
    ctx->ov_pending[0] = ctx->ov_pending[1] = false;  // (the implementation's common_checks must not join: that is this function's business)
    const int rc = impl(target, target->stream);
    ctx->ov_pending[0] = keep[0]; ctx->ov_pending[1] = keep[1];
    if (rc != FP_OK) {  // nothing (or not everything) was enqueued: leave the caller's stream ordered after whatever is in flight
        (void)overlap_join(ctx, stream);
        return rc;
    }
    HIP_TRY(hipEventRecord(ctx->ov_done[k], target->stream));
    if (ctx->ov_pending[k ^ 1]) {  // the deferred join of the predecessor
        HIP_TRY(hipStreamWaitEvent(stream, ctx->ov_done[k ^ 1], 0));
        ctx->ov_pending[k ^ 1] = false;
    }
    ctx->ov_pending[k] = true;
    memcpy(ctx->ov_last_p, outs.p, sizeof(outs.p));
    ctx->ov_next = k ^ 1;
    return FP_OK;
}

// Is this call one the "overlap" option applies to?  (FP_MEM_DEVICE, on the owner ctx, not inside a stream capture: nothing forks there.)
bool overlap_applies(fp_ctx* ctx, int mem, const fp_batch* batch, void* stream)
{
    if (!ctx->overlap || mem != FP_MEM_DEVICE || ctx->is_twin || !batch || batch->B <= 0) return false;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess) (void)hipGetLastError();
    return cap == hipStreamCaptureStatusNone;
}

}  // namespace

extern "C" {

int fp_abi_version(void) { return FP_ABI_VERSION; }

// The diagnostic macros this library was compiled with: "" for a production build.  The timing ablations (FP_ABL_*: results are
// WRONG by design), the instance switches (FP_NO_*, ...) and the stamp / counter builds (FP_PHASE_STAMPS, FP_COUNTERS,
// FP_TL: series blocks carry clock ticks) all live in the production sources behind #if and build into the same file name under the same
// ABI version; this is how a caller tells them apart.  Two sources: the Makefile's EXTRA verbatim, and - however the macro got onto the
// command line - the list below.
const char* fp_build_flags(void)
{
    static const std::string flags = [] {
        std::string o;
#if defined(FP_BUILD_EXTRA)
        o = FP_BUILD_EXTRA;
#endif
        auto add = [&o](const char* n) {
            if (o.find(n) == std::string::npos) { if (!o.empty()) o += " "; o += "-D"; o += n; }
        };
        (void)add;
#define FP_FLAG_IF(m) add(#m);
#if defined(FP_PHASE_STAMPS)
        FP_FLAG_IF(FP_PHASE_STAMPS)
#endif
#if defined(FP_TL)
        FP_FLAG_IF(FP_TL)
#endif
#if defined(FP_RABL)
        FP_FLAG_IF(FP_RABL)
#endif
#if defined(FP_COUNTERS)
        FP_FLAG_IF(FP_COUNTERS)
#endif
#if defined(FP_ABL_MAT_NO_STORE)
        FP_FLAG_IF(FP_ABL_MAT_NO_STORE)
#endif
#if defined(FP_ABL_MAT_STORE_ONLY)
        FP_FLAG_IF(FP_ABL_MAT_STORE_ONLY)
#endif
#if defined(FP_ABL_MAT_NO_MATH)
        FP_FLAG_IF(FP_ABL_MAT_NO_MATH)
#endif
#if defined(FP_ABL_SEARCH_NOWALK)
        FP_FLAG_IF(FP_ABL_SEARCH_NOWALK)
#endif
#if defined(FP_ABL_SEARCH_NOSORT)
        FP_FLAG_IF(FP_ABL_SEARCH_NOSORT)
#endif
#if defined(FP_ABL_NO_N)
        FP_FLAG_IF(FP_ABL_NO_N)
#endif
#if defined(FP_ABL_NO_BN)
        FP_FLAG_IF(FP_ABL_NO_BN)
#endif
#if defined(FP_ABL_NO_SURE)
        FP_FLAG_IF(FP_ABL_NO_SURE)
#endif
#if defined(FP_ABL_NO_GROUP)
        FP_FLAG_IF(FP_ABL_NO_GROUP)
#endif
#if defined(FP_ABL_NO_WHOLE)
        FP_FLAG_IF(FP_ABL_NO_WHOLE)
#endif
#if defined(FP_ABL_NO_GBN)
        FP_FLAG_IF(FP_ABL_NO_GBN)
#endif
#if defined(FP_ABL_NO_COLL)
        FP_FLAG_IF(FP_ABL_NO_COLL)
#endif
#if defined(FP_ABL_NO_WINNER)
        FP_FLAG_IF(FP_ABL_NO_WINNER)
#endif
#if defined(FP_ABL_NO_VMAX)
        FP_FLAG_IF(FP_ABL_NO_VMAX)
#endif
#if defined(FP_ABL_NO_SPLINE_COPY)
        FP_FLAG_IF(FP_ABL_NO_SPLINE_COPY)
#endif
#if defined(FP_ABL_NO_SCAN)
        FP_FLAG_IF(FP_ABL_NO_SCAN)
#endif
#if defined(FP_ABL_NO_DALL)
        FP_FLAG_IF(FP_ABL_NO_DALL)
#endif
#if defined(FP_NO_SHAPES)
        FP_FLAG_IF(FP_NO_SHAPES)
#endif
#if defined(FP_NO_OCC6)
        FP_FLAG_IF(FP_NO_OCC6)
#endif
#if defined(FP_NO_OCC8)
        FP_FLAG_IF(FP_NO_OCC8)
#endif
#if defined(FP_MAT_PER_CANDIDATE)
        FP_FLAG_IF(FP_MAT_PER_CANDIDATE)
#endif
#if defined(FP_MAT_NO_XCD)
        FP_FLAG_IF(FP_MAT_NO_XCD)
#endif
#if defined(FP_MAT_OCC)
        FP_FLAG_IF(FP_MAT_OCC)
#endif
#if defined(FP_WINNER_OCC)
        FP_FLAG_IF(FP_WINNER_OCC)
#endif
#if defined(FP_REFINE_OCC)
        FP_FLAG_IF(FP_REFINE_OCC)
#endif
#if defined(FP_SEARCH_WAVES)
        FP_FLAG_IF(FP_SEARCH_WAVES)
#endif
#if defined(FP_SEARCH_SMALL)
        FP_FLAG_IF(FP_SEARCH_SMALL)
#endif
#if defined(FP_SEARCH_NB)
        FP_FLAG_IF(FP_SEARCH_NB)
#endif
#if defined(FP_POSE_FLIGHT)
        FP_FLAG_IF(FP_POSE_FLIGHT)
#endif
#if defined(FP_GROUP_THREADS)
        FP_FLAG_IF(FP_GROUP_THREADS)
#endif
#if defined(FP_TEST_HOOKS)
        FP_FLAG_IF(FP_TEST_HOOKS)
#endif
#undef FP_FLAG_IF
        return o;
    }();
    return flags.c_str();
}

// The compiler this library was built with (the kernels depend on properties of ONE validated toolchain: no VGPR spill in any kernel -
// this compiler places spill stores before the exec restore of a divergent loop's exit -, -disable-machine-licm, the SGPR budgets).
const char* fp_build_compiler(void) { return __clang_version__; }

const char* fp_last_error(void) { return g_last_error.c_str(); }

int fp_device_count(int* count)
{
    if (!count) return fail(FP_EINVAL, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(FP_ENODEV, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
    }
    *count = n;
    return FP_OK;
}

int fp_device_info(int device, char* buf, int buflen, int* compute_units, int64_t* hbm_bytes)
{
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (buf && buflen > 0) snprintf(buf, (size_t)buflen, "%s (%s)", prop.name, prop.gcnArchName);
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    return FP_OK;
}

int fp_ctx_create(int device, fp_ctx** out)
{
    if (!out) return fail(FP_EINVAL, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(FP_ENODEV, "no HIP device visible: the engine has no CPU fallback");
    if (device < 0 || device >= n) return fail(FP_EINVAL, "device %d out of range (0..%d)", device, n - 1);
    HIP_TRY(hipSetDevice(device));
    fp_ctx* ctx = new (std::nothrow) fp_ctx();
    if (!ctx) return fail(FP_ENOMEM, "out of host memory");
    ctx->device = device;
    hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipHostMalloc((void**)&ctx->pinned, kSmallRegion, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&ctx->hand_err, 64, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) memset(ctx->hand_err, 0, 64);
    if (e != hipSuccess) {
        if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
        if (ctx->pinned) (void)hipHostFree(ctx->pinned);
        if (ctx->hand_err) (void)hipHostFree(ctx->hand_err);
        delete ctx;
        return fail(FP_EHIP, "ctx resources: %s", hipGetErrorString(e));
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        if (prop.multiProcessorCount > 0) ctx->resident_groups = 2 * prop.multiProcessorCount;
        if (prop.maxSharedMemoryPerMultiProcessor > 0) ctx->lds_cu_kb = (int)(prop.maxSharedMemoryPerMultiProcessor / 1024);
        // (in-order workgroup dispatch per XCD was verified on these two; anything else gets the series / the search in their own launches)
        ctx->appended_ok = strncmp(prop.gcnArchName, "gfx950", 6) == 0 || strncmp(prop.gcnArchName, "gfx942", 6) == 0;
    }
    *out = ctx;
    return FP_OK;
}

int fp_ctx_destroy(fp_ctx* ctx)
{
    if (!ctx) return FP_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->twin) {  // ("overlap": drain both internal streams before anything they use is freed)
        (void)hipStreamSynchronize(ctx->twin->stream);
        (void)hipStreamSynchronize(ctx->stream);
        (void)fp_ctx_destroy(ctx->twin);
        for (hipEvent_t e : {ctx->ov_fork, ctx->ov_done[0], ctx->ov_done[1]})
            if (e) (void)hipEventDestroy(e);
    }
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->arena.base) (void)hipFree(ctx->arena.base);
    if (ctx->scratch.base) (void)hipFree(ctx->scratch.base);
    if (ctx->parts.base) (void)hipFree(ctx->parts.base);
    for (auto& t : ctx->tables)
        if (t.buf.base) (void)hipFree(t.buf.base);
    if (ctx->curv_buf.base) (void)hipFree(ctx->curv_buf.base);
    if (ctx->idx_shadow.base) (void)hipFree(ctx->idx_shadow.base);
    if (ctx->epi_flags.base) (void)hipFree(ctx->epi_flags.base);
    ctx->order_lattice.release();
    ctx->order_refine.release();
    ctx->order_refine_rules.release();
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->hand_err) (void)hipHostFree(ctx->hand_err);
    if (ctx->validate_host) (void)hipHostFree(ctx->validate_host);
    delete ctx;
    return FP_OK;
}

int fp_ctx_set_option(fp_ctx* ctx, const char* name, int value)
{
    if (!ctx || !name) return fail(FP_EINVAL, "ctx/name is NULL");
    if (strcmp(name, "lattice_kernel") == 0) {
        if (value < 0 || value > 2) return fail(FP_EINVAL, "lattice_kernel must be 0 (auto), 1 (per-candidate) or 2 (fused)");
        ctx->lattice_kernel = value;
        return FP_OK;
    }
    if (strcmp(name, "lattice_order") == 0) {
        if (value < 0 || value > 1) return fail(FP_EINVAL, "lattice_order must be 0 or 1");
        ctx->lattice_order = value;
        ctx->order_lattice.forget(); ctx->order_refine.forget(); ctx->order_refine_rules.forget();
        return FP_OK;
    }
    if (strcmp(name, "refine_table_kb") == 0) {
        if (value < 0 || value > 96) return fail(FP_EINVAL, "refine_table_kb must be in [0, 96]");
        ctx->refine_table_kb = value;
        return FP_OK;
    }
    if (strcmp(name, "lattice_winner") == 0) {
        if (value < 0 || value > 2) return fail(FP_EINVAL, "lattice_winner must be 0 (auto), 1 (inside the lattice kernel) or 2 (own launch)");
        ctx->lattice_winner = value;
        return FP_OK;
    }
    if (strcmp(name, "fiss_fused") == 0) {
        if (value < 0 || value > 1) return fail(FP_EINVAL, "fiss_fused must be 0 or 1");
        ctx->fiss_fused = value;
        return FP_OK;
    }
    if (strcmp(name, "appended_workgroups") == 0) {  // 0: never offer appended workgroups on this ctx (what a timed-out hand-over sets)
        if (value < 0 || value > 1) return fail(FP_EINVAL, "appended_workgroups must be 0 or 1");
        ctx->appended_ok = value != 0;
        return FP_OK;
    }
    if (strcmp(name, "handover_timeout_us") == 0) {  // test hook: appended workgroups give up after this many microseconds (0 = 2 s)
        if (!getenv("FP_TEST_HOOKS")) return fail(FP_EINVAL, "handover_timeout_us is a test hook: set FP_TEST_HOOKS=1 in the environment to use it");
        if (value < 0 || value > 10000000) return fail(FP_EINVAL, "handover_timeout_us must be in 0..10^7");
        ctx->handover_timeout_us = value;
        return FP_OK;
    }
    if (strcmp(name, "handover_inject") == 0) {  // test hook: what a timed-out hand-over leaves in the ctx's error word (1 series, 2 search)
        if (!getenv("FP_TEST_HOOKS")) return fail(FP_EINVAL, "handover_inject is a test hook: set FP_TEST_HOOKS=1 in the environment to use it");
        if (value < 1 || value > 2 || !ctx->hand_err) return fail(FP_EINVAL, "handover_inject must be 1 or 2");
        *(volatile int32_t*)ctx->hand_err = value;
        return FP_OK;
    }
    if (strcmp(name, "fiss_stages") == 0) {
        if (value < 1 || value > 3) return fail(FP_EINVAL, "fiss_stages must be 1 (lattice only), 2 (+ search) or 3 (all)");
        ctx->fiss_stages = value;
        return FP_OK;
    }
    if (strcmp(name, "validate") == 0) {
        if (value < 0 || value > 1) return fail(FP_EINVAL, "validate must be 0 or 1");
        ctx->validate = value;
        return FP_OK;
    }
    if (strcmp(name, "fiss_jump") == 0) {
        if (value < 0 || value > 1) return fail(FP_EINVAL, "fiss_jump must be 0 or 1");
        ctx->fiss_jump = value;
        return FP_OK;
    }
    if (strcmp(name, "inline_inputs") == 0) {
        if (value < 0 || value > 1) return fail(FP_EINVAL, "inline_inputs must be 0 or 1");
        ctx->inline_inputs = value;
        return FP_OK;
    }
    if (strcmp(name, "stage_kernel") == 0) {
        if (value < 0 || value > 1) return fail(FP_EINVAL, "stage_kernel must be 0 or 1");
        ctx->stage_kernel = value;
        return FP_OK;
    }
    if (strcmp(name, "zero_copy_in") == 0) {
        if (value < 0 || value > 2) return fail(FP_EINVAL, "zero_copy_in must be 0, 1 or 2");
        ctx->zero_copy_in = value;
        return FP_OK;
    }
    if (strcmp(name, "lattice_group") == 0) {
        if (value < 0) return fail(FP_EINVAL, "lattice_group must be 0 (auto), 1 (never) or the number of slices per group");
        ctx->lattice_group = value;
        return FP_OK;
    }
    if (strcmp(name, "lattice_occupancy") == 0) {
        if (value != 0 && (value < 2 || value > 4)) return fail(FP_EINVAL, "lattice_occupancy must be 0 (auto), 2, 3 or 4 (workgroups per compute unit at most)");
        ctx->lattice_occupancy = value;
        return FP_OK;
    }
    if (strcmp(name, "overlap") == 0) {
        if (value < 0 || value > 1) return fail(FP_EINVAL, "overlap must be 0 or 1");
        if (ctx->is_twin) return fail(FP_EINVAL, "overlap: not on a twin ctx");
        ctx->overlap = value;  // (calls in flight stay in flight: fp_ctx_join / the next entry point joins them)
        return FP_OK;
    }
    if (strcmp(name, "resident_groups") == 0) {
        // lattice workgroups the device holds at once at two per CU (default: 2 x the device's compute units).  Lower it when the process
        // runs under a CU mask (HSA_CU_MASK / ROC_GLOBAL_CU_MASK: the runtime still reports every CU), or to model a smaller device: the
        // latency-mode split, the tail split, the three- / four-per-CU instances and the launch order all key on it.  0 = the device's value.
        if (value < 0 || (value & 1)) return fail(FP_EINVAL, "resident_groups must be 0 (the device's 2 x compute units) or an even number >= 2");
        if (value == 0) {
            hipDeviceProp_t prop;
            HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
            value = 2 * prop.multiProcessorCount;
        }
        ctx->resident_groups = value;
        return FP_OK;
    }
    if (strcmp(name, "lattice_tail") == 0) {
        if (value < 0) return fail(FP_EINVAL, "lattice_tail must be 0 (auto), 1 (never) or the number of egos cut in two");
        ctx->lattice_tail = value;
        return FP_OK;
    }
    if (strcmp(name, "lattice_split") == 0) {
        if (value < 0 || value > 2) return fail(FP_EINVAL, "lattice_split must be 0 (auto), 1 (never) or 2 (always)");
        ctx->lattice_split = value;
        return FP_OK;
    }
    return fail(FP_EINVAL, "unknown option '%s'", name);
}

int fp_ctx_get_option(fp_ctx* ctx, const char* name, int* value)
{
    if (!ctx || !name || !value) return fail(FP_EINVAL, "ctx/name/value is NULL");
    const struct { const char* n; int v; } tab[] = {
        {"lattice_kernel", ctx->lattice_kernel}, {"lattice_split", ctx->lattice_split}, {"lattice_group", ctx->lattice_group}, {"lattice_tail", ctx->lattice_tail}, {"lattice_occupancy", ctx->lattice_occupancy}, {"resident_groups", ctx->resident_groups}, {"zero_copy_in", ctx->zero_copy_in}, {"stage_kernel", ctx->stage_kernel}, {"inline_inputs", ctx->inline_inputs}, {"lattice_order", ctx->lattice_order},
        {"refine_table_kb", ctx->refine_table_kb}, {"fiss_stages", ctx->fiss_stages}, {"fiss_jump", ctx->fiss_jump}, {"validate", ctx->validate}, {"lattice_winner", ctx->lattice_winner}, {"fiss_fused", ctx->fiss_fused}, {"appended_workgroups", ctx->appended_ok ? 1 : 0}, {"handover_failed", ctx->hand_err ? *(volatile int32_t*)ctx->hand_err : 0}, {"overlap", ctx->overlap}, {"overlapped_calls", ctx->overlapped_calls}, {"clearance_launches", ctx->clearance_launches + (ctx->twin ? ctx->twin->clearance_launches : 0)}, {"lattice_launches", ctx->lattice_launches + (ctx->twin ? ctx->twin->lattice_launches : 0)},
        {"looplog_launches", ctx->looplog_launches}, {"rank_launches", ctx->rank_launches}, {"boundary_launches", ctx->boundary_launches}, {"envelope_launches", ctx->envelope_launches}, {"gate_launches", ctx->gate_launches}, {"gap_launches", ctx->gap_launches}, {"margin_launches", ctx->margin_launches}, {"fallback_launches", ctx->fallback_launches}, {"fallback_rules_launches", ctx->fallback_rules_launches}, {"rules_eval_launches", ctx->rules_eval_launches}, {"fiss_rules_calls", ctx->fiss_rules_calls}, {"predict_launches", ctx->predict_launches}, {"from_plans_launches", ctx->from_plans_launches}, {"from_state_launches", ctx->from_state_launches}, {"lattice_ordered_launches", ctx->lattice_ordered_launches + (ctx->twin ? ctx->twin->lattice_ordered_launches : 0)},
        {"lattice_launches_2", (int)fp::lattice_launches_per_cu(0)}, {"lattice_launches_3", (int)fp::lattice_launches_per_cu(1)}, {"lattice_launches_4", (int)fp::lattice_launches_per_cu(2)}};
    for (const auto& t : tab)
        if (strcmp(name, t.n) == 0) { *value = t.v; return FP_OK; }
    return fail(FP_EINVAL, "unknown option '%s'", name);
}

static int plan_dense_impl(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_result* result, int mem, void* stream);

int fp_ctx_join(fp_ctx* ctx, void* stream)
{
    if (!ctx) return fail(FP_EINVAL, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return overlap_join(ctx, (hipStream_t)stream);
}

int fp_plan_dense(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_result* result, int mem, void* stream)
{
    if (!ctx) return fail(FP_EINVAL, "ctx is NULL");
    if (!result || !overlap_applies(ctx, mem, batch, stream)) return plan_dense_impl(ctx, params, batch, result, mem, stream);
    return overlapped_call(ctx, (hipStream_t)stream, overlap_outs(*result),
                           [&](fp_ctx* target, hipStream_t is) { return plan_dense_impl(target, params, batch, result, FP_MEM_DEVICE, is); });
}

static int plan_dense_impl(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_result* result, int mem, void* stream)
{
    FP_TRY(common_checks(ctx, params, batch, mem, stream));
    if (!result || !result->best_idx || !result->best_cost) return fail(FP_EINVAL, "result.best_idx/best_cost must not be NULL");
    if (result->best_traj && !result->best_flags) return fail(FP_EINVAL, "result.best_traj requires result.best_flags");
    if (result->audit && result->fopplus) return fail(FP_EINVAL, "result.audit settles FrenetOptimalPlanner's argmin: not together with result.fopplus");
    const bool clearance = params->w_obstacle > 0;
    if (clearance && (result->fopplus || result->audit))
        return fail(FP_EINVAL, "w_obstacle > 0: the clearance term is defined for FrenetOptimalPlanner's dense pass only - result.fopplus / result.audit must be NULL");
    if (batch->B == 0) return FP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    CallStage call(ctx, mem, stream);
    const hipStream_t st = call.stream();
    FP_TRY(handover_check(ctx, st));
    const size_t C = (size_t)params->nd * params->nv * params->nt, B = (size_t)batch->B;
    int stride;
    FP_TRY(traj_stride_of(result->traj_stride, &stride));
    fp::KernelArgs ka;
    ka.p = *params;
    ctx_lattice_args(ctx, &ka);
    int32_t* fopplus = result->fopplus;
    uint32_t* audit = result->audit;
    StageList& sl = call.list();
    fp::InlineIn inl;
    if (mem == FP_MEM_DEVICE) {
        ka.b = device_batch(batch);
        ka.r = *result;
    } else {  // host buffers: checked, staged into device buffers, fetched below
        FP_TRY(check_batch_host(params, batch));
        if (result->best_traj) FP_TRY(check_stride_host(params, batch, stride));
        ka.p.points_max = host_points_max(params, batch, nullptr, 0, 0);
        const size_t traj_doubles = result->best_traj ? B * FP_ARR_COUNT * (size_t)stride : 0;
        StageRegime rg{/*zero_copy_out=*/B <= 8, ctx->zero_copy_in};
        // (inline inputs need the fused kernel with the winner's series inside it: no other kernel of this call may read the batch)
        const bool try_inline = ctx->inline_inputs && B <= 8 && !params->curvature_mask && ctx->lattice_kernel != 1 && !big_points(ka.p) && !clearance &&
                                (!result->best_traj || winner_inside_lattice(ctx, batch)) && !result->audit && fp::lattice_group_fit(*params, *batch) >= 1;
        FP_TRY(stage_batch(ctx, sl, rg, params, batch, &ka.b, try_inline ? &inl : nullptr));
        sl.out(result->best_idx, B, &ka.r.best_idx);
        sl.out(result->best_cost, B, &ka.r.best_cost);
        sl.out(result->stats, B * 4, &ka.r.stats);
        sl.out(result->cost_tbl, B * C, &ka.r.cost_tbl);
        sl.out(result->flag_tbl, B * C, &ka.r.flag_tbl);
        sl.out(result->best_flags, B, &ka.r.best_flags);
        sl.out(result->best_traj, traj_doubles, &ka.r.best_traj);
        ka.r.traj_stride = result->traj_stride;
        ka.r.traj_sparse = result->traj_sparse;
        sl.out(result->fopplus, B * 2, &fopplus);
        sl.out(result->audit, B, &audit);
        FP_TRY(call.commit(rg));
        // sparse rows are only partly written by the kernels: the host block comes back with the caller's own bytes elsewhere
        if (result->traj_sparse && ka.r.best_traj) HIP_TRY(hipMemcpyAsync(ka.r.best_traj, result->best_traj, traj_doubles * sizeof(double), hipMemcpyDefault, st));
    }
    if ((result->fopplus || result->audit || clearance) && (!ka.r.cost_tbl || !ka.r.flag_tbl)) FP_TRY(fopplus_tables(ctx, B, C, &ka.r, st));
    // the series: inside the lattice workgroups, else by the epilogue workgroups appended to the launch or by winner_traj_kernel behind
    // it (the audit pass and the clearance rescoring may move the winner: its series are written after them, by their own launch)
    const bool big = big_points(ka.p);
    const bool inside = winner_inside_lattice(ctx, batch) && !result->audit && !big && !clearance;
    if (result->best_traj && !inside) ka.idx_shadow = idx_shadow_for(ctx, B, st);
    fp::KernelArgs kl = ka;
    if (!inside) kl.r.best_traj = nullptr;
    if (!inside && !result->audit && !big && !clearance && ctx->lattice_winner == 0 && ctx->appended_ok && ka.r.best_traj && ka.idx_shadow) {  // ("lattice_winner" 0: auto)
        if (int32_t* flags = epi_flags_for(ctx, B, st)) { kl.r.best_traj = ka.r.best_traj; kl.epi_flag = flags; }  // (taken by three-per-CU launches)
    }
    fp::LatticeResult lr;
    FP_TRY(lattice_step(ctx, params, batch, kl, st, ctx->lattice_kernel, mem == FP_MEM_DEVICE ? batch->launch_order : nullptr, inl.on ? &inl : nullptr, nullptr, &lr, clearance));
    if (clearance) FP_TRY(clearance_step(ctx, ka, mem == FP_MEM_DEVICE ? batch->launch_order : nullptr, st));
    if (audit) LAUNCH_TRY(fp::launch_audit(ka, audit, st), "audit kernel");
    if (result->best_traj && !lr.winner_done) {
        if (inl.on) return fail(FP_EHIP, "internal: inline inputs without the series inside the lattice kernel");
        LAUNCH_TRY(fp::launch_winner_traj(ka, nullptr, st), "winner epilogue");
    }
    if (fopplus)
        LAUNCH_TRY(fp::launch_fopplus_count((int)B, (int)C, ka.r.cost_tbl, ka.r.flag_tbl, ka.r.best_idx, ka.r.best_cost, fopplus, ka.r.stats, ka.b.skip, st),
                   "FOP+ count kernel");
    if (mem == FP_MEM_DEVICE) return FP_OK;
    FP_TRY(call.finish());
    if (handover_failed(ctx)) {  // (the call has synchronised: a timed-out hand-over of ITS launch is known now - run it again without appended workgroups)
        (void)handover_recover(ctx, ctx->stream);
        return fp_plan_dense(ctx, params, batch, result, mem, stream);
    }
    return FP_OK;
}

int fp_winner_trajs(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const int32_t* best_idx, uint32_t* best_flags,
                    double* best_traj, int32_t traj_stride, int32_t traj_sparse, int mem, void* stream)
{
    FP_TRY(common_checks(ctx, params, batch, mem, stream));
    if (!best_idx || !best_flags || !best_traj) return fail(FP_EINVAL, "best_idx/best_flags/best_traj must not be NULL");
    if (batch->B == 0) return FP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    int stride;
    FP_TRY(traj_stride_of(traj_stride, &stride));
    const size_t B = (size_t)batch->B, traj_doubles = B * FP_ARR_COUNT * (size_t)stride;
    fp::KernelArgs ka;
    ka.p = *params;
    ka.r = no_result();
    ka.r.traj_stride = traj_stride;
    ka.r.traj_sparse = traj_sparse;
    CallStage call(ctx, mem, stream);
    if (call.host()) {
        FP_TRY(check_batch_host(params, batch));
        FP_TRY(check_stride_host(params, batch, stride));
        ka.p.points_max = host_points_max(params, batch, nullptr, 0, 0);
        const int C = params->nd * params->nv * params->nt;
        for (size_t i = 0; i < B; ++i)
            if (best_idx[i] >= C) return fail(FP_EINVAL, "best_idx[%zu]=%d out of range", i, best_idx[i]);
    }
    StageList& sl = call.list();
    StageRegime rg;  // (throughput)
    FP_TRY(stage_batch(ctx, call, rg, params, batch, &ka.b, DeviceView::AS_GIVEN));
    sl.in(best_idx, B, &ka.r.best_idx);
    sl.out(best_flags, B, &ka.r.best_flags);
    sl.out(best_traj, traj_doubles, &ka.r.best_traj);
    FP_TRY(call.commit(rg));
    // (sparse rows are only partly written by the kernels: a host array comes back with the caller's own bytes elsewhere)
    if (call.host() && traj_sparse) HIP_TRY(hipMemcpyAsync(ka.r.best_traj, best_traj, traj_doubles * sizeof(double), hipMemcpyDefault, call.stream()));
    LAUNCH_TRY(fp::launch_winner_traj(ka, nullptr, call.stream()), "winner epilogue");
    return call.finish();
}

int fp_rank_feasible(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const double* cost_tbl, const uint32_t* flag_tbl,
                     int32_t K, int32_t* rank_idx, double* rank_cost, int32_t* n_feasible, int mem, void* stream)
{
    FP_TRY(common_checks(ctx, params, batch, mem, stream));
    if (!cost_tbl || !flag_tbl || !rank_idx || !rank_cost) return fail(FP_EINVAL, "fp_rank_feasible: cost_tbl/flag_tbl/rank_idx/rank_cost must not be NULL");
    if (K < 1 || K > FP_MAX_RANK) return fail(FP_EINVAL, "fp_rank_feasible: K=%d outside 1..FP_MAX_RANK", K);
    if (batch->B == 0) return FP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t B = (size_t)batch->B, C = (size_t)params->nd * params->nv * params->nt;
    CallStage call(ctx, mem, stream);
    fp::RankArgs a;
    a.B = batch->B; a.C = (int)C; a.K = K;
    a.perm = launch_order_of(call, batch);
    // only what the kernel reads travels (the two tables and skip)
    StageList& sl = call.list();
    sl.in(cost_tbl, B * C, &a.cost_tbl);
    sl.in(flag_tbl, B * C, &a.flag_tbl);
    if (batch->skip) sl.in(batch->skip, B, &a.skip);
    sl.out(rank_idx, B * K, &a.rank_idx);
    sl.out(rank_cost, B * K, &a.rank_cost);
    sl.out(n_feasible, B, &a.n_feasible);
    FP_TRY(call.commit());
    LAUNCH_TRY(fp::launch_rank_feasible(a, call.stream()), "ranking kernel");
    ++ctx->rank_launches;
    return call.finish();
}

int fp_boundary_mask(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_corridor* corridor, const double* cost_tbl,
                     uint32_t* flag_tbl, int32_t* best_idx, double* best_cost, int32_t* n_masked, int mem, void* stream)
{
    FP_TRY(common_checks(ctx, params, batch, mem, stream));
    if (!corridor || !corridor->left || !corridor->right) return check_corridor(corridor);
    if (!cost_tbl || !flag_tbl || !best_idx || !best_cost) return fail(FP_EINVAL, "fp_boundary_mask: cost_tbl/flag_tbl/best_idx/best_cost must not be NULL");
    FP_TRY(check_corridor(corridor));
    if (batch->B == 0) return FP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    CallStage call(ctx, mem, stream);
    if (call.host()) {
        FP_TRY(check_frames_host(batch));
        FP_TRY(check_corridor_host(corridor, batch));
    }
    const size_t fn = (size_t)batch->F * batch->NX;
    fp::BoundaryArgs a;
    fp::boundary_args(&a, fp::rule_args(fp_rule_set{nullptr, nullptr, corridor, nullptr}), *params, batch->d_samples);
    StageList& sl = call.list();
    sl.in(a.d_samples, (size_t)params->nd, &a.d_samples);
    table_pass_declare(sl, &a, params, batch, launch_order_of(call, batch), cost_tbl, flag_tbl, best_idx, best_cost, n_masked, [&](StageList& l) {
        l.in(a.left, fn, &a.left);
        l.in(a.right, fn, &a.right);
    });
    FP_TRY(call.commit());
    FP_TRY(boundary_pass(ctx, a, call.stream()));
    return call.finish();
}

int fp_speed_envelope(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_speed_profile* profile, const double* cost_tbl,
                      uint32_t* flag_tbl, int32_t* best_idx, double* best_cost, int32_t* n_limited, int mem, void* stream)
{
    FP_TRY(common_checks(ctx, params, batch, mem, stream, /*need_coef=*/false));  // (coef is read by the lateral check alone: see below)
    if (!profile || !profile->v_limit) return check_speed_profile(profile, batch);
    if (!cost_tbl || !flag_tbl || !best_idx || !best_cost) return fail(FP_EINVAL, "fp_speed_envelope: cost_tbl/flag_tbl/best_idx/best_cost must not be NULL");
    FP_TRY(check_speed_profile(profile, batch));
    if (batch->B == 0) return FP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    CallStage call(ctx, mem, stream);
    if (call.host()) {
        FP_TRY(check_frames_host(batch));
        FP_TRY(check_speed_profile_host(profile, batch));
    }
    const size_t fn = (size_t)batch->F * batch->NX;
    fp::EnvelopeArgs a;
    fp::envelope_args(&a, fp::rule_args(fp_rule_set{profile, nullptr, nullptr, nullptr}), batch->coef);
    table_pass_declare(call.list(), &a, params, batch, launch_order_of(call, batch), cost_tbl, flag_tbl, best_idx, best_cost, n_limited, [&](StageList& l) {
        if (a.coef) l.in(a.coef, fn * 8, &a.coef);  // (set when the lateral bound is on: check_speed_profile has seen batch->coef then)
        l.in(a.v_limit, fn, &a.v_limit);
    });
    FP_TRY(call.commit());
    FP_TRY(envelope_pass(ctx, a, call.stream()));
    return call.finish();
}

int fp_gate_mask(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_gates* gates, const double* cost_tbl, uint32_t* flag_tbl,
                 int32_t* best_idx, double* best_cost, int32_t* n_gated, int mem, void* stream)
{
    FP_TRY(common_checks(ctx, params, batch, mem, stream, /*need_coef=*/false));  // (the line's coefficients are not read)
    if (!gates || !gates->gate_s || !gates->closed) return check_gates(gates);
    if (!cost_tbl || !flag_tbl || !best_idx || !best_cost) return fail(FP_EINVAL, "fp_gate_mask: cost_tbl/flag_tbl/best_idx/best_cost must not be NULL");
    FP_TRY(check_gates(gates));
    if (batch->B == 0) return FP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    CallStage call(ctx, mem, stream);
    int host_points = 0;  // (a device caller announces its points in fp_params.points_max; host calls look at their time samples themselves)
    if (call.host()) {
        FP_TRY(check_frames_host(batch));
        host_points = host_points_max(params, batch, nullptr, 0, 0);
    }
    const size_t F = (size_t)batch->F;
    fp::GateArgs a;
    fp::gate_args(&a, fp::rule_args(fp_rule_set{nullptr, gates, nullptr, nullptr}), batch->t_now, fp::gate_points_cap(*params, call.host(), host_points));
    table_pass_declare(call.list(), &a, params, batch, launch_order_of(call, batch), cost_tbl, flag_tbl, best_idx, best_cost, n_gated, [&](StageList& l) {
        l.in(a.t_now, (size_t)a.B, &a.t_now);
        l.in(a.gate_s, F * a.gate_stride, &a.gate_s);
        l.in(a.closed, F * a.T_gate, &a.closed);
    });
    FP_TRY(call.commit());
    FP_TRY(gate_pass(ctx, a, call.stream()));
    return call.finish();
}

int fp_gap_mask(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_time_gap* gap, const double* cost_tbl, uint32_t* flag_tbl,
                int32_t* best_idx, double* best_cost, int32_t* n_close, int mem, void* stream)
{
    FP_TRY(common_checks(ctx, params, batch, mem, stream));
    if (!gap) return check_time_gap(gap);
    if (!cost_tbl || !flag_tbl || !best_idx || !best_cost) return fail(FP_EINVAL, "fp_gap_mask: cost_tbl/flag_tbl/best_idx/best_cost must not be NULL");
    FP_TRY(check_time_gap(gap));
    if (batch->B == 0) return FP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t B = (size_t)batch->B, C = (size_t)params->nd * params->nv * params->nt;
    fp::KernelArgs ka;
    ka.p = *params;
    ka.r = no_result();
    CallStage call(ctx, mem, stream);
    if (call.host()) {
        FP_TRY(check_batch_host(params, batch));
        ka.p.points_max = fp::gap_points_max(*params, true, host_points_max(params, batch, nullptr, 0, 0));  // (host calls look at their time samples themselves)
    }
    fp::GapArgs g = fp::gap_args(fp::rule_args(fp_rule_set{nullptr, nullptr, nullptr, gap}), launch_order_of(call, batch), nullptr);
    StageList& sl = call.list();
    StageRegime rg;  // (throughput)
    FP_TRY(stage_batch(ctx, call, rg, params, batch, &ka.b, DeviceView::NO_OBS_WITHOUT_SCENES));
    sl.in(cost_tbl, B * C, &ka.r.cost_tbl);
    sl.in_mut(flag_tbl, B * C, &ka.r.flag_tbl);
    sl.out(best_idx, B, &ka.r.best_idx);
    sl.out(best_cost, B, &ka.r.best_cost);
    sl.out(n_close, B, &g.count);
    FP_TRY(call.commit(rg));
    FP_TRY(gap_pass(ctx, ka, g, call.stream()));
    return call.finish();
}

int fp_rules_eval(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_rule_set* rules, int32_t K, const double* end_states,
                  uint32_t* flags, uint32_t* rule_bits, int32_t* counts, int mem, void* stream)
{
    FP_TRY(common_checks(ctx, params, batch, mem, stream));
    if (K < 1) return fail(FP_EINVAL, "fp_rules_eval: K=%d must be >= 1", K);
    if (!rules || !end_states || !flags) return fail(FP_EINVAL, "fp_rules_eval: rules / end_states / flags must not be NULL");
    FP_TRY(check_rule_set("fp_rules_eval", rules, batch));
    if (batch->B == 0) return FP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t B = (size_t)batch->B, BK = B * (size_t)K;
    fp::KernelArgs ka;
    ka.p = *params;
    ka.r = no_result();
    CallStage call(ctx, mem, stream);
    fp::RulesEvalArgs a = fp::rule_args(*rules);
    a.K = K;
    a.perm = launch_order_of(call, batch);
    if (call.host()) {
        FP_TRY(check_batch_host(params, batch, /*past_ok=*/true));  // (a negative t_now reads the gates' first state; no obstacle has a state before step 0)
        FP_TRY(check_rule_set_host(rules, batch));
        for (size_t i = 0; i < BK; ++i) {
            const double n = end_states[3 * i + 2] / params->tick_t;
            if (n != n || (batch->skip && batch->skip[i / (size_t)K])) continue;  // NaN end state = "no trajectory"
            if (!(n > 0) || n > FP_MAX_POINTS)
                return fail(FP_ELIMIT, "fp_rules_eval: end_states of ego %zu, trajectory %zu: T=%g needs 1..FP_MAX_POINTS points", i / (size_t)K, i % (size_t)K, end_states[3 * i + 2]);
        }
        ka.p.points_max = host_points_max(params, batch, end_states + 2, BK, 3);
    }
    StageList& sl = call.list();
    StageRegime rg;  // (throughput)
    FP_TRY(stage_batch(ctx, call, rg, params, batch, &ka.b, DeviceView::NO_OBS_WITHOUT_SCENES));
    fp::stage_rule_arrays(sl, &a, batch->F, batch->NX);
    sl.in(end_states, BK * 3, &a.end_states);
    sl.in_mut(flags, BK, &a.flags);
    sl.out(rule_bits, BK, &a.rule_bits);
    if (counts) sl.in_mut(counts, B * FP_RULE_COUNT, &a.counts);
    FP_TRY(call.commit(rg));
    LAUNCH_TRY(fp::launch_rules_eval(ka, a, call.stream()), "rules kernel");
    ++ctx->rules_eval_launches;
    return call.finish();
}

int fp_traj_margins(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, int32_t K, const int32_t* best_idx, const double* end_state,
                    int32_t pose_stride, double* min_dist, int32_t* min_step, int32_t* min_obs, int mem, void* stream)
{
    FP_TRY(common_checks(ctx, params, batch, mem, stream));
    if (K < 1 || K > FP_MAX_RANK) return fail(FP_EINVAL, "fp_traj_margins: K=%d outside 1..FP_MAX_RANK", K);
    if (pose_stride < 1) return fail(FP_EINVAL, "fp_traj_margins: pose_stride=%d must be >= 1", pose_stride);
    if ((best_idx == nullptr) == (end_state == nullptr)) return fail(FP_EINVAL, "fp_traj_margins: exactly one of best_idx / end_state must be given");
    if (!min_dist || !min_step || !min_obs) return fail(FP_EINVAL, "fp_traj_margins: min_dist/min_step/min_obs must not be NULL");
    if (batch->B == 0) return FP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t KB = (size_t)K * batch->B;
    fp::KernelArgs ka;
    ka.p = *params;
    ka.p.check_stride = pose_stride;  // (the kernel's staging and pose set read it there; the caller's own check_stride is not used)
    ka.r = no_result();
    CallStage call(ctx, mem, stream);
    fp::MarginArgs m;
    m.K = K;
    m.perm = launch_order_of(call, batch);
    if (call.host()) {
        FP_TRY(check_batch_host(params, batch));
        if (best_idx) {
            const int C = params->nd * params->nv * params->nt;
            for (size_t i = 0; i < KB; ++i) {
                const size_t b = i % (size_t)batch->B;
                if (best_idx[i] >= C && !(batch->skip && batch->skip[b]))
                    return fail(FP_EINVAL, "fp_traj_margins: best_idx of ego %zu, plane %zu = %d is outside the lattice (nd*nv*nt = %d)", b, i / (size_t)batch->B, best_idx[i], C);
            }
            ka.p.points_max = host_points_max(params, batch, nullptr, 0, 0);
        } else {
            for (size_t i = 0; i < KB; ++i) {
                const double n = end_state[3 * i + 2] / params->tick_t;
                if (n != n || (batch->skip && batch->skip[i % (size_t)batch->B])) continue;  // NaN end state = "no trajectory"
                if (!(n > 0) || n > FP_MAX_POINTS)
                    return fail(FP_ELIMIT, "fp_traj_margins: end_state of ego %zu, plane %zu: T=%g needs 1..FP_MAX_POINTS points", i % (size_t)batch->B, i / (size_t)batch->B, end_state[3 * i + 2]);
            }
            ka.p.points_max = host_points_max(params, batch, end_state + 2, KB, 3);
        }
    }
    StageList& sl = call.list();
    StageRegime rg;  // (throughput)
    FP_TRY(stage_batch(ctx, call, rg, params, batch, &ka.b, DeviceView::NO_OBS_WITHOUT_SCENES));
    if (best_idx) sl.in(best_idx, KB, &m.best_idx); else sl.in(end_state, KB * 3, &m.end_state);
    sl.out(min_dist, KB, &m.min_dist);
    sl.out(min_step, KB, &m.min_step);
    sl.out(min_obs, KB, &m.min_obs);
    FP_TRY(call.commit(rg));
    LAUNCH_TRY(fp::launch_traj_margins(ka, m, call.stream()), "plan-margin kernel");
    ++ctx->margin_launches;
    return call.finish();
}

// fp_fallback_stop and fp_fallback_stop_rules: one body.  fn names the entry point in the messages; with_rules: the rule instance
// (rules, rule_bits mandatory; cand_rules, rule_counts optional), else the three are not read.
static int fallback_call(const char* fn, bool with_rules, fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_fallback* fallback,
                         const fp_rule_set* rules, const int32_t* best_idx, double* end_state, int32_t* status, int32_t* fb_idx, int32_t* hit_step,
                         int32_t* hit_obs, double* hit_speed, int32_t* cand, uint32_t* cand_rules, uint32_t* rule_bits, int32_t* counts, int32_t* rule_counts,
                         int mem, void* stream)
{
    FP_TRY(common_checks(ctx, params, batch, mem, stream));
    if (!fallback || !fallback->d_targets || !fallback->stop_T) return fail(FP_EINVAL, "%s: fallback / d_targets / stop_T must not be NULL", fn);
    if (!end_state || !status || !fb_idx || !hit_step || !hit_obs || !hit_speed)
        return fail(FP_EINVAL, "%s: end_state/status/fb_idx/hit_step/hit_obs/hit_speed must not be NULL", fn);
    if (fallback->n_d < 1 || fallback->n_stop < 1) return fail(FP_EINVAL, "%s: n_d=%d, n_stop=%d must be >= 1", fn, fallback->n_d, fallback->n_stop);
    if ((long long)fallback->n_d * fallback->n_stop > FP_MAX_FALLBACK)
        return fail(FP_ELIMIT, "%s: n_d * n_stop = %lld exceeds FP_MAX_FALLBACK (%d)", fn, (long long)fallback->n_d * fallback->n_stop, FP_MAX_FALLBACK);
    if (!(fallback->max_decel > 0)) return fail(FP_EINVAL, "%s: max_decel=%g must be > 0 (+inf = no limit)", fn, fallback->max_decel);
    if (with_rules) {
        if (!rules || !rule_bits) return fail(FP_EINVAL, "%s: rules / rule_bits must not be NULL", fn);
        FP_TRY(check_rule_set(fn, rules, batch));
    }
    if (batch->B == 0) return FP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t B = (size_t)batch->B, F = (size_t)fallback->n_d * fallback->n_stop;
    fp::KernelArgs ka;
    ka.p = *params;
    ka.r = no_result();
    CallStage call(ctx, mem, stream);
    fp::FallbackRulesArgs a;  // (fp_fallback_stop launches with its FallbackArgs part)
    a.n_d = fallback->n_d; a.n_stop = fallback->n_stop; a.max_decel = fallback->max_decel;
    if (with_rules) a.rules = fp::rule_args(*rules);
    a.perm = launch_order_of(call, batch);
    if (call.host()) {
        FP_TRY(check_batch_host(params, batch));
        if (with_rules) FP_TRY(check_rule_set_host(rules, batch));
        for (int i = 0; i < fallback->n_stop; ++i) {
            const double T = fallback->stop_T[i];
            if (!finite_pos(T) || (i > 0 && !(T > fallback->stop_T[i - 1])))
                return fail(FP_EINVAL, "%s: stop_T[%d]=%g must be finite, > 0 and above stop_T[%d]", fn, i, T, i - 1);
            if (ceil(T / params->tick_t) > FP_MAX_POINTS) return fail(FP_ELIMIT, "%s: stop_T[%d]=%g needs more than FP_MAX_POINTS points", fn, i, T);
        }
        if (best_idx) {
            const int C = params->nd * params->nv * params->nt;
            for (size_t b = 0; b < B; ++b)
                if (best_idx[b] >= C && !(batch->skip && batch->skip[b]))
                    return fail(FP_EINVAL, "%s: best_idx of ego %zu = %d is outside the lattice (nd*nv*nt = %d)", fn, b, best_idx[b], C);
        }
        ka.p.points_max = host_points_max(params, batch, fallback->stop_T, (size_t)fallback->n_stop, 1);
    }
    StageList& sl = call.list();
    StageRegime rg;  // (throughput)
    FP_TRY(stage_batch(ctx, call, rg, params, batch, &ka.b, DeviceView::NO_OBS_WITHOUT_SCENES));
    if (with_rules) fp::stage_rule_arrays(sl, &a.rules, batch->F, batch->NX);
    sl.in(fallback->d_targets, (size_t)fallback->n_d, &a.d_targets);
    sl.in(fallback->stop_T, (size_t)fallback->n_stop, &a.stop_T);
    if (best_idx) sl.in(best_idx, B, &a.best_idx);
    sl.in_mut(end_state, B * 3, &a.end_state);
    sl.out(status, B, &a.status);
    sl.out(fb_idx, B, &a.fb_idx);
    sl.out(hit_step, B, &a.hit_step);
    sl.out(hit_obs, B, &a.hit_obs);
    sl.out(hit_speed, B, &a.hit_speed);
    if (cand) sl.in_mut(cand, B * F, &a.cand);
    if (counts) sl.in_mut(counts, B * 4, &a.counts);
    if (with_rules) {
        if (cand_rules) sl.in_mut(cand_rules, B * F, &a.cand_rules);
        sl.out(rule_bits, B, &a.rule_bits);
        if (rule_counts) sl.in_mut(rule_counts, B * FP_RULE_COUNT, &a.rule_counts);
    }
    FP_TRY(call.commit(rg));
    if (with_rules) {
        LAUNCH_TRY(fp::launch_fallback_stop_rules(ka, a, call.stream()), "fallback rules kernel");
        ++ctx->fallback_rules_launches;
    } else {
        LAUNCH_TRY(fp::launch_fallback_stop(ka, a, call.stream()), "fallback kernel");
        ++ctx->fallback_launches;
    }
    return call.finish();
}

int fp_fallback_stop(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_fallback* fallback, const int32_t* best_idx, double* end_state,
                     int32_t* status, int32_t* fb_idx, int32_t* hit_step, int32_t* hit_obs, double* hit_speed, int32_t* cand, int32_t* counts, int mem,
                     void* stream)
{
    return fallback_call("fp_fallback_stop", false, ctx, params, batch, fallback, nullptr, best_idx, end_state, status, fb_idx, hit_step, hit_obs, hit_speed, cand,
                         nullptr, nullptr, counts, nullptr, mem, stream);
}

int fp_fallback_stop_rules(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_fallback* fallback, const fp_rule_set* rules,
                           const int32_t* best_idx, double* end_state, int32_t* status, int32_t* fb_idx, int32_t* hit_step, int32_t* hit_obs, double* hit_speed,
                           int32_t* cand, uint32_t* cand_rules, uint32_t* rule_bits, int32_t* counts, int32_t* rule_counts, int mem, void* stream)
{
    return fallback_call("fp_fallback_stop_rules", true, ctx, params, batch, fallback, rules, best_idx, end_state, status, fb_idx, hit_step, hit_obs, hit_speed, cand,
                         cand_rules, rule_bits, counts, rule_counts, mem, stream);
}

int fp_obstacles_predict(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_tracks* tracks, double* obs_pose,
                         int32_t* final_time_step, int mem, void* stream)
{
    if (!ctx) return fail(FP_EINVAL, "ctx is NULL");
    if (!params || !batch) return fail(FP_EINVAL, "fp_obstacles_predict: params / batch must not be NULL");
    if (mem != FP_MEM_HOST && mem != FP_MEM_DEVICE) return fail(FP_EINVAL, "mem must be FP_MEM_HOST or FP_MEM_DEVICE");
    if (!tracks || !tracks->model || !tracks->state || !tracks->t0 || !obs_pose)
        return fail(FP_EINVAL, "fp_obstacles_predict: tracks / model / state / t0 / obs_pose must not be NULL");
    if (tracks->n_rows <= 0) return fail(FP_EINVAL, "fp_obstacles_predict: n_rows=%d must be > 0", tracks->n_rows);
    if (!finite_pos(params->tick_t)) return fail(FP_EINVAL, "fp_obstacles_predict: tick_t must be finite and > 0");
    if (batch->S < 0 || batch->T_obs < 0 || batch->n_obs < 0 || batch->F < 0 || batch->NX < 0 || batch->NX > FP_MAX_KNOTS)
        return fail(FP_EINVAL, "fp_obstacles_predict: bad batch sizes S=%d T_obs=%d n_obs=%d F=%d NX=%d", batch->S, batch->T_obs, batch->n_obs, batch->F, batch->NX);
    // (the table may be an input of overlapped dense calls still in flight on the ctx's internal streams)
    if (ctx->ov_pending[0] || ctx->ov_pending[1]) FP_TRY(overlap_join(ctx, mem == FP_MEM_DEVICE ? (hipStream_t)stream : ctx->stream));
    if (batch->S == 0 || batch->T_obs == 0 || batch->n_obs == 0) return FP_OK;  // no element to write
    HIP_TRY(hipSetDevice(ctx->device));
    fp::PredictArgs a;
    a.S = batch->S; a.T_obs = batch->T_obs; a.n_obs = batch->n_obs; a.F = batch->F; a.NX = batch->NX; a.n_rows = tracks->n_rows;
    a.tick_t = params->tick_t;
    CallStage call(ctx, mem, stream);
    const size_t S = (size_t)batch->S, n = (size_t)batch->n_obs, fn = (size_t)batch->F * batch->NX;
    bool frames_read = !call.host();  // (a device call hands the frames on as they are; a host call stages them when a LANE track reads them)
    if (!call.host()) {
        if ((uintptr_t)obs_pose & 15u) return fail(FP_EINVAL, "fp_obstacles_predict: obs_pose must be 16-byte aligned");
    } else {
        // host arrays: what the device path decides silently (such a column has no pose) is an error the host path can name
        for (size_t s = 0; s < S; ++s)
            for (size_t j = 0; j < n; ++j) {
                const int32_t m = tracks->model[s * n + j];
                if (m < FP_TRACK_NONE || m > FP_TRACK_ARC) return fail(FP_EINVAL, "fp_obstacles_predict: model of scene %zu, column %zu is %d, not one of FP_TRACK_*", s, j, m);
                if (m != FP_TRACK_LANE) continue;
                frames_read = true;
                if (!tracks->frame_of_scene || !batch->nx || !batch->knots || !batch->coef)
                    return fail(FP_EINVAL, "fp_obstacles_predict: scene %zu, column %zu is a LANE track but frame_of_scene / nx / knots / coef is NULL", s, j);
                const int32_t f = tracks->frame_of_scene[s];
                if (f < 0 || f >= batch->F) return fail(FP_EINVAL, "fp_obstacles_predict: scene %zu, column %zu is a LANE track on frame %d, outside 0 .. F-1 (F=%d)", s, j, f, batch->F);
                if (batch->nx[f] < 2 || batch->nx[f] > batch->NX) return fail(FP_EINVAL, "fp_obstacles_predict: scene %zu, column %zu: nx[%d]=%d out of range", s, j, f, batch->nx[f]);
            }
    }
    const size_t span = (size_t)(tracks->n_rows < batch->T_obs ? tracks->n_rows : batch->T_obs);
    StageList& sl = call.list();
    sl.in(tracks->model, S * n, &a.model);
    sl.in(tracks->state, S * n * 6, &a.state);
    sl.in(tracks->t0, S, &a.t0);
    if (frames_read) {
        sl.in(tracks->frame_of_scene, S, &a.frame_of_scene);
        sl.in(batch->nx, (size_t)batch->F, &a.nx);
        sl.in(batch->knots, fn, &a.knots);
        sl.in(batch->coef, fn * 8, &a.coef);
    }
    sl.out(final_time_step, S, &a.final_time_step);
    // a host call predicts into a compact temporary, [S][span][n_obs][4]: a scene's written rows from its row 0 on; a device call into the table
    if (call.host()) { sl.temp(S * span * n * 4, &a.obs_pose); a.compact = 1; }
    else a.obs_pose = obs_pose;
    FP_TRY(call.commit());
    LAUNCH_TRY(fp::launch_obstacles_predict(a, call.stream()), "obstacle prediction kernel");
    ++ctx->predict_launches;
    if (!call.host()) return FP_OK;
    // only the written rows travel back; runs that are contiguous on both sides (whole tables) go as one copy
    const double* src = nullptr;
    double* dst = nullptr;
    size_t run = 0;
    for (size_t s = 0; s < S; ++s) {
        const long t0 = tracks->t0[s];
        const long rlo = t0 > 0 ? t0 : 0;
        long rhi = t0 + tracks->n_rows;
        if (rhi > batch->T_obs) rhi = batch->T_obs;
        if (rhi <= rlo) continue;
        const double* sc_src = a.obs_pose + s * span * n * 4;
        double* sc_dst = obs_pose + (s * (size_t)batch->T_obs + (size_t)rlo) * n * 4;
        const size_t count = (size_t)(rhi - rlo) * n * 4;
        if (run && sc_src == src + run && sc_dst == dst + run) {
            run += count;
            continue;
        }
        if (run) HIP_TRY(hipMemcpyAsync(dst, src, run * sizeof(double), hipMemcpyDeviceToHost, call.stream()));
        src = sc_src; dst = sc_dst; run = count;
    }
    if (run) HIP_TRY(hipMemcpyAsync(dst, src, run * sizeof(double), hipMemcpyDeviceToHost, call.stream()));
    return call.finish();
}

int fp_obstacles_from_plans(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_agents* agents, const int32_t* best_idx,
                            const double* end_state, double* obs_pose, int32_t* final_time_step, int mem, void* stream)
{
    if (!ctx) return fail(FP_EINVAL, "ctx is NULL");
    if (mem != FP_MEM_HOST && mem != FP_MEM_DEVICE) return fail(FP_EINVAL, "mem must be FP_MEM_HOST or FP_MEM_DEVICE");
    if (!params || !batch || !agents || !obs_pose) return fail(FP_EINVAL, "fp_obstacles_from_plans: params / batch / agents / obs_pose must not be NULL");
    // (the table may be an input of overlapped dense calls still in flight on the ctx's internal streams)
    if (ctx->ov_pending[0] || ctx->ov_pending[1]) FP_TRY(overlap_join(ctx, mem == FP_MEM_DEVICE ? (hipStream_t)stream : ctx->stream));
    FP_TRY(check_params(params));
    if (batch->B < 0 || batch->F < 1 || batch->NX < 2 || batch->S < 0 || batch->T_obs < 0 || batch->n_obs < 0)
        return fail(FP_EINVAL, "fp_obstacles_from_plans: bad batch sizes B=%d F=%d NX=%d S=%d T_obs=%d n_obs=%d", batch->B, batch->F, batch->NX, batch->S, batch->T_obs, batch->n_obs);
    if (batch->NX > FP_MAX_KNOTS) return fail(FP_ELIMIT, "NX=%d exceeds FP_MAX_KNOTS", batch->NX);
    if (!batch->d_samples || !batch->t_samples || !batch->v_samples || !batch->ego || !batch->frame_of || !batch->scene_of || !batch->t_now || !batch->nx ||
        !batch->knots || !batch->coef)
        return fail(FP_EINVAL, "fp_obstacles_from_plans: batch has a NULL array");
    if ((best_idx == nullptr) == (end_state == nullptr)) return fail(FP_EINVAL, "fp_obstacles_from_plans: exactly one of best_idx / end_state must be given");
    if (agents->n_rows <= 0) return fail(FP_EINVAL, "fp_obstacles_from_plans: n_rows=%d must be > 0", agents->n_rows);
    if (agents->tail < FP_TAIL_NONE || agents->tail > FP_TAIL_COAST) return fail(FP_EINVAL, "fp_obstacles_from_plans: tail=%d is not one of FP_TAIL_*", agents->tail);
    if (agents->G < 0 || agents->n_members < 0) return fail(FP_EINVAL, "fp_obstacles_from_plans: G=%d, n_members=%d must be >= 0", agents->G, agents->n_members);
    if (agents->G == 0 || agents->n_members == 0) return FP_OK;  // no element to write
    if (!agents->group_ptr || !agents->members) return fail(FP_EINVAL, "fp_obstacles_from_plans: group_ptr / members must not be NULL");
    if (agents->col_base < 0) return fail(FP_EINVAL, "fp_obstacles_from_plans: col_base=%d must be >= 0", agents->col_base);
    HIP_TRY(hipSetDevice(ctx->device));
    fp::KernelArgs ka;
    ka.p = *params;
    ka.r = no_result();
    fp::AgentArgs a;
    a.G = agents->G; a.n_members = agents->n_members; a.col_base = agents->col_base; a.n_rows = agents->n_rows; a.tail = agents->tail;
    CallStage call(ctx, mem, stream);
    const int G = agents->G, B = batch->B;
    const size_t nB = (size_t)B, S = (size_t)batch->S, fn = (size_t)batch->F * batch->NX;
    ka.b = *batch;
    if (!call.host()) {
        if ((uintptr_t)obs_pose & 15u) return fail(FP_EINVAL, "fp_obstacles_from_plans: obs_pose must be 16-byte aligned");
    } else {
        // host arrays: what the device path decides silently is an error the host path can name
        if (agents->group_ptr[0] != 0) return fail(FP_EINVAL, "fp_obstacles_from_plans: group_ptr[0]=%d must be 0", agents->group_ptr[0]);
        for (int g = 0; g < G; ++g) {
            const int lo = agents->group_ptr[g], hi = agents->group_ptr[g + 1];
            if (hi < lo) return fail(FP_EINVAL, "fp_obstacles_from_plans: group_ptr is not ascending at group %d (%d > %d)", g, lo, hi);
            if ((long)agents->col_base + (hi - lo) > batch->n_obs)
                return fail(FP_EINVAL, "fp_obstacles_from_plans: group %d: col_base + group size = %d + %d exceeds n_obs = %d", g, agents->col_base, hi - lo, batch->n_obs);
        }
        if (agents->group_ptr[G] != agents->n_members)
            return fail(FP_EINVAL, "fp_obstacles_from_plans: n_members=%d is not group_ptr[G]=%d", agents->n_members, agents->group_ptr[G]);
        FP_TRY(check_frames_host(batch));
        {
            std::vector<int32_t> group_of(nB, -1), member_of((size_t)(batch->S > 0 ? batch->S : 0), -1);
            for (int g = 0; g < G; ++g)
                for (int k = agents->group_ptr[g]; k < agents->group_ptr[g + 1]; ++k) {
                    const int e = agents->members[k];
                    if (e < 0 || e >= B) return fail(FP_EINVAL, "fp_obstacles_from_plans: member %d of group %d is ego %d, outside 0 .. B-1 (B=%d)", k - agents->group_ptr[g], g, e, B);
                    if (group_of[e] >= 0) return fail(FP_EINVAL, "fp_obstacles_from_plans: ego %d is a member of group %d and of group %d", e, group_of[e], g);
                    group_of[e] = g;
                    const int sc = batch->scene_of[e];
                    if (sc < 0) return fail(FP_EINVAL, "fp_obstacles_from_plans: member %d of group %d (ego %d) has no scene (scene_of = %d)", k - agents->group_ptr[g], g, e, sc);
                    if (sc >= batch->S) return fail(FP_EINVAL, "scene_of[%d]=%d out of range", e, sc);
                    if (member_of[sc] >= 0) return fail(FP_EINVAL, "fp_obstacles_from_plans: ego %d and ego %d share scene %d (every member needs a scene of its own)", member_of[sc], e, sc);
                    member_of[sc] = e;
                }
        }
        if (best_idx) {
            const long n_cand = (long)params->nd * params->nv * params->nt;
            for (int i = 0; i < B; ++i)
                if (best_idx[i] >= n_cand && !(batch->skip && batch->skip[i]))
                    return fail(FP_EINVAL, "fp_obstacles_from_plans: best_idx of ego %d = %d is outside the lattice (nd*nv*nt = %ld)", i, best_idx[i], n_cand);
            ka.p.points_max = host_points_max(params, batch, nullptr, 0, 0);
        } else {
            ka.p.points_max = host_points_max(params, batch, end_state + 2, nB, 3);
        }
        // (of the batch only what the kernel reads travels; the table itself is the call's in / out array)
        ka.b.obs_pose = nullptr; ka.b.obs_dims = nullptr; ka.b.final_time_step = nullptr; ka.b.obs_poly = nullptr; ka.b.obs_nvert = nullptr; ka.b.launch_order = nullptr;
    }
    StageList& sl = call.list();
    stage_samples(sl, params, batch, &ka.b.d_samples, &ka.b.t_samples, &ka.b.v_samples);
    sl.in(batch->ego, nB * 6, &ka.b.ego);
    sl.in(batch->frame_of, nB, &ka.b.frame_of);
    sl.in(batch->scene_of, nB, &ka.b.scene_of);
    sl.in(batch->t_now, nB, &ka.b.t_now);
    sl.in(batch->nx, (size_t)batch->F, &ka.b.nx);
    sl.in(batch->knots, fn, &ka.b.knots);
    sl.in(batch->coef, fn * 8, &ka.b.coef);
    if (batch->skip) sl.in(batch->skip, nB, &ka.b.skip);
    sl.in(agents->group_ptr, (size_t)G + 1, &a.group_ptr);
    sl.in(agents->members, (size_t)agents->n_members, &a.members);
    if (best_idx) sl.in(best_idx, nB, &a.best_idx); else sl.in(end_state, nB * 3, &a.end_state);
    sl.in_mut(obs_pose, S * (size_t)batch->T_obs * batch->n_obs * 4, &a.obs_pose);
    if (final_time_step) sl.in_mut(final_time_step, S, &a.final_time_step);
    FP_TRY(call.commit());
    LAUNCH_TRY(fp::launch_obstacles_from_plans(ka, a, call.stream()), "shared-plans kernel");
    ++ctx->from_plans_launches;
    return call.finish();
}

int fp_materialize_all(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, uint32_t* flags, double* traj, int32_t traj_stride,
                       int32_t traj_sparse, int mem, void* stream)
{
    FP_TRY(common_checks(ctx, params, batch, mem, stream));
    if (!flags || !traj) return fail(FP_EINVAL, "flags/traj must not be NULL");
    if (batch->B == 0) return FP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    int stride;
    FP_TRY(traj_stride_of(traj_stride, &stride));
    const size_t BC = (size_t)batch->B * params->nd * params->nv * params->nt, traj_doubles = BC * FP_ARR_COUNT * (size_t)stride;
    if (BC > 0x7fffffffu) return fail(FP_ELIMIT, "B*C = %zu exceeds the grid size limit", BC);
    fp::KernelArgs ka;
    ka.p = *params;
    ka.r = no_result();
    ka.r.traj_stride = traj_stride;
    ka.r.traj_sparse = traj_sparse;
    CallStage call(ctx, mem, stream);
    if (call.host()) {
        FP_TRY(check_batch_host(params, batch));
        FP_TRY(check_stride_host(params, batch, stride));
        ka.p.points_max = host_points_max(params, batch, nullptr, 0, 0);
    }
    StageList& sl = call.list();
    StageRegime rg;  // (throughput)
    FP_TRY(stage_batch(ctx, call, rg, params, batch, &ka.b, DeviceView::AS_GIVEN));
    sl.out(flags, BC, &ka.r.best_flags);
    sl.out(traj, traj_doubles, &ka.r.best_traj);
    FP_TRY(call.commit(rg));
    if (call.host() && traj_sparse) HIP_TRY(hipMemcpyAsync(ka.r.best_traj, traj, traj_doubles * sizeof(double), hipMemcpyDefault, call.stream()));  // (see fp_winner_trajs)
    LAUNCH_TRY(fp::launch_materialize_all(ka, call.stream()), "materialise kernel");
    return call.finish();
}

}  // extern "C"

namespace {

// fp_plan_fiss, and - with `loop` (FP_MEM_DEVICE only) - fp_plan_fiss_step: the pipeline plus the egos' hand-over to their next states.
// rules (fp_plan_fiss_rules, its arguments checked there): the dense tables are masked by the table passes of the rules that are on before
// the search reads them, and the refinement runs its rule instances; rejected [B] in / out or nullptr.
int plan_fiss_impl(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_fiss_opts* opts, const fp_fiss_io* io, const fp_loop_io* loop,
                   int mem, void* stream_v, const fp_rule_set* rules = nullptr, int32_t* rejected = nullptr)
{
    FP_TRY(common_checks(ctx, params, batch, mem, stream_v));
    if (!opts || !io) return fail(FP_EINVAL, "opts/io is NULL");
    if (params->w_obstacle > 0)
        return fail(FP_EINVAL, "w_obstacle > 0: FISS / FISS+ order candidates by cost before they have Cartesian points - the clearance term is defined for fp_plan_dense / fp_plan_step only");
    if (opts->kind != FP_FISS && opts->kind != FP_FISS_PLUS) return fail(FP_EINVAL, "opts.kind must be FP_FISS or FP_FISS_PLUS");
    if (opts->max_refine_iters < 0 || opts->max_refine_iters * 7 > 64) return fail(FP_ELIMIT, "max_refine_iters must be in 0..9");
    if ((long)params->nd * params->nv * params->nt > FP_MAX_CAND_SEARCH)
        return fail(FP_ELIMIT, "nd*nv*nt = %ld exceeds FP_MAX_CAND_SEARCH (the device-side search walk): use fp_plan_dense's tables and a host walk", (long)params->nd * params->nv * params->nt);
    if (!io->samp_min || !io->samp_max || !io->samp_res || !io->prev_best_idx || !io->best_ijk || !io->best_cost || !io->end_state ||
        !io->refined || !io->stats)
        return fail(FP_EINVAL, "fp_fiss_io has a NULL mandatory array");
    if (io->best_traj && !io->best_flags) return fail(FP_EINVAL, "io.best_traj requires io.best_flags");
    if (batch->B == 0) return FP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t B = (size_t)batch->B, C = (size_t)params->nd * params->nv * params->nt;
    const int R = opts->kind == FP_FISS_PLUS ? opts->max_refine_iters : 0;
    CallStage call(ctx, mem, stream_v);
    hipStream_t stream = call.stream();
    FP_TRY(handover_check(ctx, stream));
    // (host entry: prev_best_idx is in / out - should the appended search of this call time out, the call is repeated from the caller's values)
    std::vector<int32_t> prev_in;
    if (mem == FP_MEM_HOST && ctx->appended_ok && ctx->fiss_fused && B > (size_t)ctx->resident_groups) prev_in.assign(io->prev_best_idx, io->prev_best_idx + B * 3);

    // dense tables + per-ego dense results live in the scratch buffer in both modes
    // (with rules: the passes' best_idx / best_cost / count outputs behind them)
    const size_t scratch_need = align_up(sizeof(double) * B * C) + align_up(sizeof(uint32_t) * B * C) + align_up(sizeof(int32_t) * B) +
                                align_up(sizeof(double) * B) + 4 * kAlign +
                                (rules ? 2 * align_up(sizeof(int32_t) * B) + align_up(sizeof(double) * B) + 3 * kAlign : 0);
    if (scratch_need > ctx->scratch.cap) HIP_TRY(hipStreamSynchronize(stream));  // the buffer may be reallocated: drain its users
    FP_TRY(ctx->scratch.reserve(scratch_need));
    char* sp = ctx->scratch.base;
    fp::FissArgs fa;
    fa.ka.p = *params;
    ctx_lattice_args(ctx, &fa.ka);
    fa.opts = *opts;
    fa.opts.max_refine_iters = R;
    fa.ka.r = no_result();
    fa.ka.r.cost_tbl = (double*)sp;
    sp += align_up(sizeof(double) * B * C);
    fa.ka.r.flag_tbl = (uint32_t*)sp;
    sp += align_up(sizeof(uint32_t) * B * C);
    fa.ka.r.best_idx = (int32_t*)sp;
    sp += align_up(sizeof(int32_t) * B);
    fa.ka.r.best_cost = (double*)sp;
    sp += align_up(sizeof(double) * B);
    int32_t* pass_idx = (int32_t*)sp;
    sp += rules ? align_up(sizeof(int32_t) * B) : 0;
    double* pass_cost = (double*)sp;
    sp += rules ? align_up(sizeof(double) * B) : 0;
    int32_t* pass_count = (int32_t*)sp;
    int32_t* rejected_dev = rejected;  // (a host call: the staged copy's address at commit)
    // the rule set as the rules kernel takes it; a host call's arrays get their device addresses at commit
    fp::RulesEvalArgs ra = fp::rule_args(rules ? *rules : fp_rule_set{});
    const bool host = mem == FP_MEM_HOST;
    int pass_points = 0;  // (a host call: what the host calls of the passes work out from the time samples)
    // the rule instances of the refinement hold the rules' tables in LDS beside the refinement's own: a call that does not fit is refused
    auto refine_fits = [&](const fp_params& p_sized) -> int {
        if (!rules || R <= 0) return FP_OK;
        fp::FissArgs probe;
        probe.ka.p = p_sized;
        probe.ka.b = device_batch(batch);
        int base = 0, own = 0;
        fp::fiss_refine_rules_lds(probe, ra.on, ctx->refine_table_kb, &base, &own);
        if (base + own > fp::kRefineRulesLdsMax)
            return fail(FP_ELIMIT, "fp_plan_fiss_rules: the refinement needs %d bytes of LDS and the rules' tables %d (NX=%d, %d gate slots, %d points, n_obs=%d): more than the %d a workgroup has",
                        base, own, batch->NX, (ra.on & FP_RULE_GATE) ? FP_MAX_GATES : 0, p_sized.points_max > FP_FAST_POINTS ? (p_sized.points_max < FP_MAX_POINTS ? p_sized.points_max : FP_MAX_POINTS) : FP_FAST_POINTS, probe.ka.b.n_obs, fp::kRefineRulesLdsMax);
        return FP_OK;
    };
    fa.cost_tbl = fa.ka.r.cost_tbl;
    fa.flag_tbl = fa.ka.r.flag_tbl;
    int stride;
    FP_TRY(traj_stride_of(io->traj_stride, &stride));
    const size_t traj_doubles = io->best_traj ? B * FP_ARR_COUNT * (size_t)stride : 0;
    const size_t trace_doubles = (io->trace && R > 0) ? B * (size_t)R * 7 * 4 : 0;
    StageList& sl = call.list();
    fp::InlineIn inl;   // (host entry, latency regime: see below)
    fp_batch lat_b;     // the batch as the lattice kernel addresses it (byte offsets into inl.bytes when inl.on)
    if (mem == FP_MEM_DEVICE) {
        fa.ka.b = device_batch(batch);
        if (loop) fa.ka.b.skip = loop->done;
        fa.io = *io;
        if (!trace_doubles) fa.io.trace = nullptr;
        FP_TRY(refine_fits(fa.ka.p));
    } else {
        FP_TRY(check_batch_host(params, batch));
        if (rules) FP_TRY(check_rule_set_host(rules, batch));
        for (size_t i = 0; R > 0 && i < B; ++i)  // (a refinement probe beyond FP_MAX_POINTS would come back as NaN cost: a silently different walk)
            if (ceil(io->samp_max[3 * i + 2] / params->tick_t) > FP_MAX_POINTS)
                return fail(FP_ELIMIT, "samp_max[%zu].T=%g needs more than FP_MAX_POINTS points (FISS+ refinement)", i, io->samp_max[3 * i + 2]);
        fa.ka.p.points_max = host_points_max(params, batch, R > 0 ? io->samp_max + 2 : nullptr, R > 0 ? B : 0, 3);  // (refined trajectories reach T = samp_max)
        FP_TRY(refine_fits(fa.ka.p));
        if (rules) pass_points = host_points_max(params, batch, nullptr, 0, 0);
        if (io->best_traj) {
            for (size_t i = 0; i < B; ++i)  // refined trajectories reach T = samp_max of their ego
                if (ceil(io->samp_max[3 * i + 2] / params->tick_t) > stride) return fail(FP_EINVAL, "traj_stride=%d is smaller than the points of samp_max[%zu].T=%g", stride, i, io->samp_max[3 * i + 2]);
            FP_TRY(check_stride_host(params, batch, stride));
        }
        StageRegime rg{/*zero_copy_out=*/B <= 8, ctx->zero_copy_in};
        // Latency regime with the tables resident (fp_batch.tables_tag): the per-ego arrays and the three sampling-range arrays ride
        // inside the lattice kernel's argument block, which also leaves them in a device mirror for the search and refinement
        // kernels - no copy kernel, no dependency in front of the lattice kernel (a single-ego FISS+ cycle: ~5 us of ~80).
        fa.io = *io;
        const bool try_inline = !rules && ctx->inline_inputs && B <= 8 && !params->curvature_mask && ctx->lattice_kernel != 1 && !big_points(fa.ka.p) &&
                                fp::lattice_group_fit(*params, *batch) >= 1;
        const InlineExtra ex[3] = {{io->samp_min, sizeof(double) * B * 3, (const void**)&fa.io.samp_min},
                                   {io->samp_max, sizeof(double) * B * 3, (const void**)&fa.io.samp_max},
                                   {io->samp_res, sizeof(double) * B * 3, (const void**)&fa.io.samp_res}};
        FP_TRY(stage_batch(ctx, sl, rg, params, batch, &lat_b, try_inline ? &inl : nullptr, &fa.ka.b, ex, 3));
        if (!inl.on) {
            sl.in(io->samp_min, B * 3, &fa.io.samp_min);
            sl.in(io->samp_max, B * 3, &fa.io.samp_max);
            sl.in(io->samp_res, B * 3, &fa.io.samp_res);
        }
        fp::stage_rule_arrays(sl, &ra, batch->F, batch->NX);
        if (rules && rejected) sl.in_mut(rejected, B, &rejected_dev);
        sl.in_mut(io->prev_best_idx, B * 3, &fa.io.prev_best_idx);
        sl.out(io->best_ijk, B * 3, &fa.io.best_ijk);
        sl.out(io->best_cost, B, &fa.io.best_cost);
        sl.out(io->end_state, B * 3, &fa.io.end_state);
        sl.out(io->refined, B, &fa.io.refined);
        sl.out(io->stats, B * 4, &fa.io.stats);
        sl.out(io->trace, trace_doubles, &fa.io.trace);
        sl.out(io->best_flags, B, &fa.io.best_flags);
        sl.out(io->best_traj, traj_doubles, &fa.io.best_traj);
        FP_TRY(call.commit(rg));
        if (inl.on) inline_publish(inl, &fa.ka.b, ex, 3);
        else fa.ka.b = lat_b;
        if (io->traj_sparse && fa.io.best_traj) HIP_TRY(hipMemcpyAsync(fa.io.best_traj, io->best_traj, traj_doubles * sizeof(double), hipMemcpyDefault, ctx->stream));
    }
    // inline inputs: the lattice kernel reads the batch from its argument block (lat_b) - the fused kernel or nothing.  Else the FISS+
    // search is offered as workgroups appended to the lattice launch (taken by three-per-CU launches; "fiss_fused" 0, the stage-timing
    // diagnostic and every other shape: the search kernel follows in its own launch)
    fp::KernelArgs kl = fa.ka;
    if (inl.on) kl.b = lat_b;
    fp::FissTail ft;
    ft.opts = fa.opts; ft.io = fa.io; ft.walk_jump = ctx->fiss_jump;
    ft.flag = (!rules && !inl.on && ctx->fiss_fused && ctx->appended_ok && ctx->fiss_stages >= 3 && opts->kind == FP_FISS_PLUS) ? epi_flags_for(ctx, B, stream) : nullptr;
    fp::LatticeResult lr;
    FP_TRY(lattice_step(ctx, params, batch, kl, stream, inl.on ? 2 : ctx->lattice_kernel, mem == FP_MEM_DEVICE ? batch->launch_order : nullptr,
                        inl.on ? &inl : nullptr, ft.flag ? &ft : nullptr, &lr));
    if (ctx->fiss_stages < 2) return call.finish();  // timing diagnostic: outputs are not produced
    fa.walk_jump = ctx->fiss_jump;
    if (rules) {
        // the table passes of the rules that are on, in the order they run (rules.TABLE): the launches a dense call's caller makes behind
        // it, over the same tables - the search reads the words the FOP chain leaves
        const fp_batch& db = fa.ka.b;
        const int32_t* perm = host ? nullptr : batch->launch_order;
        StageList on_device(/*pass_through=*/true);  // (the call's batch and the scratch tables: device addresses in either space)
        auto pass_args = [&](fp::TablePassArgs* a) {
            table_pass_declare(on_device, a, params, &db, perm, fa.cost_tbl, fa.ka.r.flag_tbl, pass_idx, pass_cost, pass_count, [](StageList&) {});
        };
        if (ra.on & FP_RULE_LIMIT) {
            fp::EnvelopeArgs a;
            pass_args(&a);
            fp::envelope_args(&a, ra, db.coef);
            FP_TRY(envelope_pass(ctx, a, stream));
        }
        if (ra.on & FP_RULE_GATE) {
            fp::GateArgs a;
            pass_args(&a);
            fp::gate_args(&a, ra, db.t_now, fp::gate_points_cap(*params, host, pass_points));
            FP_TRY(gate_pass(ctx, a, stream));
        }
        if (ra.on & FP_RULE_BOUNDARY) {
            fp::BoundaryArgs a;
            pass_args(&a);
            fp::boundary_args(&a, ra, *params, db.d_samples);
            FP_TRY(boundary_pass(ctx, a, stream));
        }
        if (ra.on & FP_RULE_GAP) {
            fp::KernelArgs kg;
            kg.p = *params;
            kg.p.points_max = fp::gap_points_max(*params, host, pass_points);
            kg.b = db;
            kg.r = no_result();
            kg.r.cost_tbl = fa.ka.r.cost_tbl; kg.r.flag_tbl = fa.ka.r.flag_tbl; kg.r.best_idx = pass_idx; kg.r.best_cost = pass_cost;
            FP_TRY(gap_pass(ctx, kg, fp::gap_args(ra, perm, pass_count), stream));
        }
    }
    if (!lr.search_done) LAUNCH_TRY(fp::launch_fiss_search(fa, stream), "search kernel");
    bool handed_over = false;
    if (R > 0 && ctx->fiss_stages >= 3) {
        // three refinement workgroups per CU are resident at once (fiss_refine_kernel: 168 VGPRs, ~52 KB LDS)
        const int* rperm; int* rdur;
        LaunchOrder* oslot_r = nullptr;
        if (rules) FP_TRY(launch_order_before(ctx, ctx->order_refine_rules, ctx->resident_groups, batch, 1, stream, &rperm, &rdur, nullptr, &oslot_r));  // (two per CU)
        else FP_TRY(launch_order_before(ctx, ctx->order_refine, ctx->resident_groups / 2 * 3, batch, 1, stream, &rperm, &rdur, nullptr, &oslot_r));
        fp::FissArgs fr = fa;
        if (loop) {  // fp_plan_fiss_step: the refinement workgroup that settles an ego's trajectory hands the ego over itself
            fr.ka.loop = *loop;
            fr.ka.has_loop = 1;
            handed_over = true;
        }
        if (rules) LAUNCH_TRY(fp::launch_fiss_refine_rules(fr, ra, rejected_dev, stream, ctx->refine_table_kb, rperm, rdur), "refinement kernel (rule instance)");
        else LAUNCH_TRY(fp::launch_fiss_refine(fr, stream, ctx->refine_table_kb, rperm, rdur), "refinement kernel");
        FP_TRY(launch_order_after(oslot_r, batch, rdur, stream));
    }
    if (fa.io.best_traj && R <= 0) {  // with refinement rounds the refinement kernel writes the series itself
        fp::KernelArgs kw = fa.ka;
        kw.r.best_flags = fa.io.best_flags;
        kw.r.best_traj = fa.io.best_traj;
        kw.r.traj_stride = fa.io.traj_stride;
        kw.r.traj_sparse = fa.io.traj_sparse;
        LAUNCH_TRY(fp::launch_winner_traj(kw, fa.io.end_state, stream), "winner epilogue");
    }
    if (loop && !handed_over) LAUNCH_TRY(fp::launch_advance(fa.ka, nullptr, fa.io.end_state, *loop, stream), "advance kernel");  // (FISS, or no refinement rounds)
    if (mem != FP_MEM_HOST) return FP_OK;
    FP_TRY(call.finish());
    if (handover_failed(ctx)) {  // (see fp_plan_dense)
        (void)handover_recover(ctx, ctx->stream);
        if (!prev_in.empty()) memcpy(io->prev_best_idx, prev_in.data(), prev_in.size() * sizeof(int32_t));
        return plan_fiss_impl(ctx, params, batch, opts, io, loop, mem, stream_v, rules, rejected);
    }
    return FP_OK;
}

}  // namespace

extern "C" {

int fp_plan_fiss(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_fiss_opts* opts, const fp_fiss_io* io, int mem,
                 void* stream_v)
{
    if (!ctx) return fail(FP_EINVAL, "ctx is NULL");
    if (!io || !overlap_applies(ctx, mem, batch, stream_v)) return plan_fiss_impl(ctx, params, batch, opts, io, nullptr, mem, stream_v);
    // ("overlap": two FISS / FISS+ pipelines of independent batches side by side - the one-round search and refinement launches of one
    // run beside the other's lattice kernel; prev_best_idx is in/out, so calls that share it run one behind the other)
    return overlapped_call(ctx, (hipStream_t)stream_v, overlap_outs(*io),
                           [&](fp_ctx* target, hipStream_t is) { return plan_fiss_impl(target, params, batch, opts, io, nullptr, FP_MEM_DEVICE, is); });
}

int fp_plan_fiss_step(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_fiss_opts* opts, const fp_fiss_io* io,
                      const fp_loop_io* loop, int mem, void* stream)
{
    FP_TRY(check_loop_io(loop, /*need_goal=*/true));
    if (mem != FP_MEM_DEVICE) {  // host buffers: the two staged calls (every array travels anyway)
        if (!batch || !io) return fail(FP_EINVAL, "batch/io is NULL");
        fp_batch bb = *batch;
        bb.skip = loop->done;
        FP_TRY(plan_fiss_impl(ctx, params, &bb, opts, io, nullptr, mem, stream));
        return fp_advance(ctx, params, batch, nullptr, io->end_state, loop, mem, stream);
    }
    return plan_fiss_impl(ctx, params, batch, opts, io, loop, mem, stream);
}

int fp_plan_fiss_rules(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_fiss_opts* opts, const fp_fiss_io* io,
                       const fp_rule_set* rules, const fp_loop_io* loop, int32_t* rejected, int mem, void* stream)
{
    FP_TRY(common_checks(ctx, params, batch, mem, stream));
    if (!rules) return fail(FP_EINVAL, "fp_plan_fiss_rules: rules must not be NULL");
    FP_TRY(check_rule_set("fp_plan_fiss_rules", rules, batch));
    if (loop) {
        if (mem != FP_MEM_DEVICE) return fail(FP_EINVAL, "fp_plan_fiss_rules: loop needs FP_MEM_DEVICE (a host caller plans with loop = NULL and calls fp_advance)");
        FP_TRY(check_loop_io(loop, /*need_goal=*/true));
    }
    ++ctx->fiss_rules_calls;
    return plan_fiss_impl(ctx, params, batch, opts, io, loop, mem, stream, rules, rejected);
}

int fp_advance(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const int32_t* best_idx, const double* end_state,
               const fp_loop_io* io, int mem, void* stream)
{
    FP_TRY(common_checks(ctx, params, batch, mem, stream));
    if ((best_idx == nullptr) == (end_state == nullptr)) return fail(FP_EINVAL, "exactly one of best_idx / end_state must be given");
    FP_TRY(check_loop_io(io, /*need_goal=*/true));
    if (batch->B == 0) return FP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t B = (size_t)batch->B;
    fp::KernelArgs ka;
    ka.p = *params;
    ka.r = no_result();
    CallStage call(ctx, mem, stream);
    if (call.host()) {
        FP_TRY(check_batch_host(params, batch));
        if (best_idx) {  // (the kernel decodes the index of every running ego and reads d_samples / t_samples / v_samples with it; negative = no solution)
            const long n_cand = (long)params->nd * params->nv * params->nt;
            for (int i = 0; i < batch->B; ++i)
                if (io->done[i] == FP_RUNNING && best_idx[i] >= n_cand)
                    return fail(FP_EINVAL, "fp_advance: best_idx[%d]=%d is not below nd*nv*nt=%ld", i, best_idx[i], n_cand);
        }
    }
    StageList& sl = call.list();
    StageRegime rg;  // (throughput)
    FP_TRY(stage_batch(ctx, call, rg, params, batch, &ka.b, DeviceView::AS_GIVEN));
    fp_loop_io dio = *io;
    sl.in_mut(io->ego, B * 6, &dio.ego);
    sl.in_mut(io->t_now, B, &dio.t_now);
    sl.in_mut(io->done, B, &dio.done);
    sl.in_mut(io->cycles, B, &dio.cycles);
    sl.in(io->goal_xy, B * 2, &dio.goal_xy);
    if (io->goal_poly && io->goal_nv && io->goal_max_vertices >= 3) {
        sl.in(io->goal_poly, B * (size_t)io->goal_max_vertices * 2, &dio.goal_poly);
        sl.in(io->goal_nv, B, &dio.goal_nv);
        if (io->goal_intervals) sl.in(io->goal_intervals, B * 6, &dio.goal_intervals);
    } else {
        dio.goal_poly = nullptr;  // (check_loop_io: a polygon without its counts never gets here)
    }
    const int32_t* d_idx = nullptr;
    const double* d_es = nullptr;
    if (best_idx) sl.in(best_idx, B, &d_idx);
    if (end_state) sl.in(end_state, B * 3, &d_es);
    sl.out(io->cart_state, B * 3, &dio.cart_state);
    FP_TRY(call.commit(rg));
    if (call.host() && dio.cart_state) HIP_TRY(hipMemsetAsync(dio.cart_state, 0xFF, sizeof(double) * B * 3, call.stream()));  // NaN for egos that do not move
    LAUNCH_TRY(fp::launch_advance(ka, d_idx, d_es, dio, call.stream()), "advance kernel");
    return call.finish();
}

int fp_loop_record(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_loop_io* io, const int32_t* best_idx,
                   const double* end_state, const double* best_cost, const int32_t* stats, const fp_loop_log* log, int mem, void* stream)
{
    FP_TRY(common_checks(ctx, params, batch, mem, stream));
    if ((best_idx == nullptr) == (end_state == nullptr)) return fail(FP_EINVAL, "exactly one of best_idx / end_state must be given");
    FP_TRY(check_loop_io(io, /*need_goal=*/false));
    if (!io->cart_state) return fail(FP_EINVAL, "fp_loop_record: fp_loop_io.cart_state is mandatory (the rows' x, y, yaw)");
    if (!best_cost) return fail(FP_EINVAL, "fp_loop_record: best_cost is NULL");
    if (!log || !log->rows || !log->n_rows || !log->sealed) return fail(FP_EINVAL, "fp_loop_log has a NULL mandatory array (rows / n_rows / sealed)");
    if (log->max_rows < 0) return fail(FP_EINVAL, "fp_loop_log.max_rows=%d is negative", log->max_rows);
    if (!stats && (log->row_stats || log->stats_sum)) return fail(FP_EINVAL, "fp_loop_record: stats is NULL but the log asks for row_stats / stats_sum");
    if (batch->B == 0) return FP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t B = (size_t)batch->B;
    fp::LoopLogArgs a;
    a.B = batch->B; a.nv = params->nv; a.nt = params->nt;
    CallStage call(ctx, mem, stream);
    // (a lane stores its row as 16-byte words and moves a Stats row as one: a device caller's arrays have to allow it)
    if (!call.host() && (((uintptr_t)log->rows | (uintptr_t)stats | (uintptr_t)log->row_stats) & 15u))
        return fail(FP_EINVAL, "fp_loop_record: rows / stats / row_stats must be 16-byte aligned");
    // only what the kernel reads travels (the three sample arrays of the batch, the loop state, the step's results, the log)
    const size_t R = (size_t)log->max_rows;
    StageList& sl = call.list();
    stage_samples(sl, params, batch, &a.d_samples, &a.t_samples, &a.v_samples);
    a.io = *io;  // (the kernel only reads the loop state)
    a.log = *log;
    sl.in(io->ego, B * 6, &a.io.ego);
    sl.in(io->cart_state, B * 3, &a.io.cart_state);
    sl.in(io->t_now, B, &a.io.t_now);
    sl.in(io->done, B, &a.io.done);
    sl.in(io->cycles, B, &a.io.cycles);
    if (best_idx) sl.in(best_idx, B, &a.best_idx);
    if (end_state) sl.in(end_state, B * 3, &a.end_state);
    sl.in(best_cost, B, &a.best_cost);
    if (stats) sl.in(stats, B * 4, &a.stats);
    sl.in_mut(log->rows, B * R * FP_LOG_COLS, &a.log.rows);
    if (log->row_stats) sl.in_mut(log->row_stats, B * R * 4, &a.log.row_stats);
    sl.in_mut(log->n_rows, B, &a.log.n_rows);
    sl.in_mut(log->sealed, B, &a.log.sealed);
    if (log->stats_sum) sl.in_mut(log->stats_sum, B * 4, &a.log.stats_sum);
    sl.out(log->n_running, 1, &a.log.n_running);
    FP_TRY(call.commit());
    if (a.log.n_running) HIP_TRY(hipMemsetAsync(a.log.n_running, 0, sizeof(int32_t), call.stream()));
    LAUNCH_TRY(fp::launch_loop_record(a, call.stream()), "loop-log kernel");
    ++ctx->looplog_launches;
    return call.finish();
}

int fp_plan_step(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, const fp_result* result, const fp_loop_io* io, int mem, void* stream)
{
    FP_TRY(common_checks(ctx, params, batch, mem, stream));
    if (!result || !result->best_idx || !result->best_cost) return fail(FP_EINVAL, "result.best_idx/best_cost must not be NULL");
    if (result->best_traj && !result->best_flags) return fail(FP_EINVAL, "result.best_traj requires result.best_flags");
    if (result->fopplus || result->audit) return fail(FP_EINVAL, "fp_plan_step: result.fopplus / result.audit must be NULL (use fp_plan_dense + fp_advance)");
    FP_TRY(check_loop_io(io, /*need_goal=*/true));
    if (batch->B == 0) return FP_OK;
    if (mem != FP_MEM_DEVICE) {
        // host buffers: the two staged calls (every array travels anyway; the fused launch is for resident loops)
        fp_batch bb = *batch;
        bb.skip = io->done;
        FP_TRY(fp_plan_dense(ctx, params, &bb, result, mem, stream));
        return fp_advance(ctx, params, batch, result->best_idx, nullptr, io, mem, stream);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    FP_TRY(handover_check(ctx, (hipStream_t)stream));
    const size_t B = (size_t)batch->B;
    fp::KernelArgs ka;
    ka.p = *params;
    ctx_lattice_args(ctx, &ka);
    ka.b = device_batch(batch);
    ka.b.skip = io->done;
    ka.r = *result;
    // the hand-over is offered to the lattice launch unless that launch cannot write the series it is asked for itself (the standalone
    // epilogue reads the ego's state, so it has to run BEFORE the state moves on)
    // (nor when the clearance rescoring decides the winner behind the launch: series and hand-over follow it)
    const bool clearance = params->w_obstacle > 0;
    if (clearance && (!ka.r.cost_tbl || !ka.r.flag_tbl)) FP_TRY(fopplus_tables(ctx, B, (size_t)params->nd * params->nv * params->nt, &ka.r, (hipStream_t)stream));
    const bool series_elsewhere = result->best_traj && (!winner_inside_lattice(ctx, batch) || big_points(ka.p) || clearance);
    if (series_elsewhere) ka.idx_shadow = idx_shadow_for(ctx, B, (hipStream_t)stream);
    fp::KernelArgs kl = ka;
    if (series_elsewhere) kl.r.best_traj = nullptr;
    else if (!clearance) { kl.loop = *io; kl.has_loop = 1; }
    fp::LatticeResult lr;
    FP_TRY(lattice_step(ctx, params, batch, kl, (hipStream_t)stream, ctx->lattice_kernel, batch->launch_order, nullptr, nullptr, &lr, clearance));
    if (clearance) FP_TRY(clearance_step(ctx, ka, batch->launch_order, (hipStream_t)stream));
    if (result->best_traj && !lr.winner_done) LAUNCH_TRY(fp::launch_winner_traj(ka, nullptr, (hipStream_t)stream), "winner epilogue");
    if (!lr.step_done) LAUNCH_TRY(fp::launch_advance(ka, ka.r.best_idx, nullptr, *io, (hipStream_t)stream), "advance kernel");
    return FP_OK;
}

int fp_frames_build(fp_ctx* ctx, int32_t F, int32_t NX, const int32_t* n, const double* points, double* knots, double* coef, int mem,
                    void* stream)
{
    if (!ctx) return fail(FP_EINVAL, "ctx is NULL");
    if (F < 0 || NX < 2 || NX > FP_MAX_KNOTS) return fail(FP_EINVAL, "bad sizes F=%d NX=%d", F, NX);
    if (!n || !points || !knots || !coef) return fail(FP_EINVAL, "NULL array");
    if (mem != FP_MEM_HOST && mem != FP_MEM_DEVICE) return fail(FP_EINVAL, "mem must be FP_MEM_HOST or FP_MEM_DEVICE");
    if (F == 0) return FP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    CallStage call(ctx, mem, stream);
    if (call.host())
        for (int f = 0; f < F; ++f)
            if (n[f] < 2 || n[f] > NX) return fail(FP_EINVAL, "n[%d]=%d out of range", f, n[f]);
    const size_t fn = (size_t)F * NX;
    StageList& sl = call.list();
    const int32_t* d_n = nullptr;
    const double* d_pts = nullptr;
    double* d_k = nullptr;
    double* d_c = nullptr;
    sl.in(n, (size_t)F, &d_n);
    sl.in(points, fn * 2, &d_pts);
    sl.out(knots, fn, &d_k);
    sl.out(coef, fn * 8, &d_c);
    FP_TRY(call.commit());
    LAUNCH_TRY(fp::launch_frames_build(F, NX, d_n, d_pts, d_k, d_c, call.stream()), "frame build");
    return call.finish();
}

int fp_from_state(fp_ctx* ctx, const fp_batch* batch, const double* states, double* ego, int mem, void* stream)
{
    if (!ctx) return fail(FP_EINVAL, "ctx is NULL");
    if (!batch || !states || !ego) return fail(FP_EINVAL, "NULL argument");
    if (batch->B < 0 || batch->F < 1 || batch->NX < 2 || batch->NX > FP_MAX_KNOTS) return fail(FP_EINVAL, "bad batch sizes");
    if (!batch->frame_of || !batch->nx || !batch->knots || !batch->coef) return fail(FP_EINVAL, "batch frame arrays must not be NULL");
    if (mem != FP_MEM_HOST && mem != FP_MEM_DEVICE) return fail(FP_EINVAL, "mem must be FP_MEM_HOST or FP_MEM_DEVICE");
    if (batch->B == 0) return FP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    CallStage call(ctx, mem, stream);
    const size_t B = (size_t)batch->B, fn = (size_t)batch->F * batch->NX;
    if (call.host()) {
        FP_TRY(check_frames_host(batch));
        // host arrays: what the device path answers with a NaN row is an error the host path can name, before anything is launched
        // (only the frames some ego sits on are looked at, as fp_obstacles_predict does for its LANE tracks)
        for (size_t b = 0; b < B; ++b) {
            static const char* const kName[4] = {"x", "y", "yaw", "v"};
            for (int k = 0; k < 4; ++k)
                if (!fp::finite_f64(states[b * 4 + k])) return fail(FP_EINVAL, "fp_from_state: ego %zu: %s=%g is not finite", b, kName[k], states[b * 4 + k]);
            const int32_t f = batch->frame_of[b];
            const double s_last = batch->knots[(size_t)f * batch->NX + batch->nx[f] - 1];
            if (fp::project_point_count(s_last) == 0)
                return fail(FP_EINVAL, "fp_from_state: ego %zu sits on frame %d, whose line of length %g has fewer than two resampled points (0.1 m apart)", b, f, s_last);
        }
    }
    StageList& sl = call.list();
    fp_batch db = *batch;
    sl.in(batch->frame_of, B, &db.frame_of);
    sl.in(batch->nx, (size_t)batch->F, &db.nx);
    sl.in(batch->knots, fn, &db.knots);
    sl.in(batch->coef, fn * 8, &db.coef);
    const double* d_states = nullptr;
    double* d_ego = nullptr;
    sl.in(states, B * 4, &d_states);
    sl.out(ego, B * 6, &d_ego);
    FP_TRY(call.commit());
    LAUNCH_TRY(fp::launch_from_state(db, d_states, d_ego, call.stream()), "from_state");
    ++ctx->from_state_launches;
    return call.finish();
}

int fp_eval_trajs(fp_ctx* ctx, const fp_params* params, const fp_batch* batch, int32_t K, const double* end_states, double* cost,
                  uint32_t* flags, double* traj, int32_t traj_stride, int32_t traj_sparse, int mem, void* stream)
{
    FP_TRY(common_checks(ctx, params, batch, mem, stream));
    if (K < 1 || !end_states) return fail(FP_EINVAL, "K must be >= 1 and end_states non-NULL");
    int stride;
    FP_TRY(traj_stride_of(traj_stride, &stride));
    if (batch->B == 0) return FP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t BK = (size_t)batch->B * K;
    fp::KernelArgs ka;
    ka.p = *params;
    ka.r = no_result();
    CallStage call(ctx, mem, stream);
    if (call.host()) {
        FP_TRY(check_batch_host(params, batch));
        for (size_t i = 0; i < BK; ++i) {
            const double n = end_states[3 * i + 2] / params->tick_t;
            if (n != n) continue;  // NaN end state = "no trajectory": the kernels emit NaN cost / all-NaN series
            if (!(n > 0) || n > FP_MAX_POINTS) return fail(FP_ELIMIT, "end_states[%zu].T=%g needs 1..FP_MAX_POINTS points", i, end_states[3 * i + 2]);
            if (traj && ceil(n) > stride) return fail(FP_EINVAL, "traj_stride=%d is smaller than the %g points of end_states[%zu].T=%g", stride, ceil(n), i, end_states[3 * i + 2]);
        }
        ka.p.points_max = host_points_max(params, batch, end_states + 2, BK, 3);
    }
    const size_t traj_doubles = traj ? BK * FP_ARR_COUNT * (size_t)stride : 0;
    StageList& sl = call.list();
    StageRegime rg;  // (throughput)
    FP_TRY(stage_batch(ctx, call, rg, params, batch, &ka.b, DeviceView::NO_OBS_WITHOUT_SCENES));
    const double* d_end = nullptr;
    double* d_cost = nullptr;
    uint32_t* d_flags = nullptr;
    double* d_traj = nullptr;
    sl.in(end_states, BK * 3, &d_end);
    // (the kernel writes both on a host call whether or not the caller wants them; a device call's temporaries are NULL: what the caller passed)
    if (cost) sl.out(cost, BK, &d_cost); else sl.temp(BK, &d_cost);
    if (flags) sl.out(flags, BK, &d_flags); else sl.temp(BK, &d_flags);
    sl.out(traj, traj_doubles, &d_traj);
    FP_TRY(call.commit(rg));
    if (call.host() && traj_sparse && d_traj) HIP_TRY(hipMemcpyAsync(d_traj, traj, traj_doubles * sizeof(double), hipMemcpyDefault, call.stream()));  // (see fp_winner_trajs)
    LAUNCH_TRY(fp::launch_eval_trajs(ka, K, d_end, d_cost, d_flags, d_traj, stride, traj_sparse, call.stream()), "eval kernel");
    return call.finish();
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------- fp_group
// One persistent host thread per ctx, fed through a one-deep mailbox (include/frenet_gpu.h).  posted / done are sequence numbers:
// the submitter copies a call into the worker's slot and increments `posted`; the worker runs it and sets `done` = the number it
// ran.  A worker spins on `posted` for kSpinRounds pause instructions after its last call (~50 us: the next step of a running loop
// arrives well inside that), then sleeps on a condition variable; the submitter notifies only when it finds the worker asleep.
namespace {

inline void cpu_pause()
{
#if !defined(__HIP_DEVICE_COMPILE__) && (defined(__x86_64__) || defined(__i386__))
    __builtin_ia32_pause();
#endif
}

constexpr int kSpinRounds = 4000;
constexpr int kMaxCopies = 8;

struct GroupWorker {
    fp_ctx* ctx = nullptr;
    std::thread th;
    // the mailbox (written by the submitter while done == posted, read by the worker after it saw posted move)
    int kind = 0;  // 1 dense, 2 step, 3 fiss, 4 fiss + advance
    fp_params params;
    fp_batch batch;
    fp_result result;
    fp_loop_io loop;
    fp_fiss_opts fopts;
    fp_fiss_io fio;
    void* stream = nullptr;
    fp_copy copies[kMaxCopies];
    int n_copies = 0;
    std::atomic<unsigned long long> posted{0}, done{0};
    std::atomic<bool> asleep{false}, stop{false};
    std::mutex m;
    std::condition_variable cv;
    int rc = FP_OK;        // of the last call (read by fp_group_wait after done == posted)
    std::string err;
};

void group_worker_main(GroupWorker* w)
{
    (void)hipSetDevice(w->ctx->device);
    unsigned long long seen = 0;
    for (;;) {
        int spins = 0;
        while (w->posted.load(std::memory_order_acquire) == seen && !w->stop.load(std::memory_order_relaxed)) {
            if (++spins < kSpinRounds) { cpu_pause(); continue; }
            std::unique_lock<std::mutex> lk(w->m);
            w->asleep.store(true, std::memory_order_seq_cst);
            w->cv.wait(lk, [&] { return w->posted.load(std::memory_order_seq_cst) != seen || w->stop.load(std::memory_order_seq_cst); });
            w->asleep.store(false, std::memory_order_seq_cst);
            spins = 0;
        }
        if (w->stop.load(std::memory_order_relaxed) && w->posted.load(std::memory_order_acquire) == seen) return;
        seen = w->posted.load(std::memory_order_acquire);
        int rc = FP_OK;
        switch (w->kind) {
            case 1: rc = fp_plan_dense(w->ctx, &w->params, &w->batch, &w->result, FP_MEM_DEVICE, w->stream); break;
            case 2: rc = fp_plan_step(w->ctx, &w->params, &w->batch, &w->result, &w->loop, FP_MEM_DEVICE, w->stream); break;
            case 3: rc = fp_plan_fiss(w->ctx, &w->params, &w->batch, &w->fopts, &w->fio, FP_MEM_DEVICE, w->stream); break;
            case 4: rc = fp_plan_fiss_step(w->ctx, &w->params, &w->batch, &w->fopts, &w->fio, &w->loop, FP_MEM_DEVICE, w->stream); break;
            default: break;
        }
        for (int i = 0; rc == FP_OK && i < w->n_copies; ++i) {
            const hipError_t e = hipMemcpyAsync(w->copies[i].dst, w->copies[i].src, w->copies[i].bytes, hipMemcpyDefault, (hipStream_t)w->stream);
            if (e != hipSuccess) rc = fail(FP_EHIP, "fp_group copy %d failed: %s", i, hipGetErrorString(e));
        }
        w->rc = rc;
        if (rc != FP_OK) w->err = g_last_error;  // (thread-local: the worker's own)
        w->done.store(seen, std::memory_order_release);
    }
}

void group_wait_worker(GroupWorker& w)
{
    const unsigned long long want = w.posted.load(std::memory_order_relaxed);
    while (w.done.load(std::memory_order_acquire) != want) cpu_pause();
}

}  // namespace

struct fp_group {
    std::vector<GroupWorker*> workers;
};

extern "C" {

int fp_group_create(fp_ctx* const* ctxs, int32_t n, fp_group** out)
{
    if (!out) return fail(FP_EINVAL, "out is NULL");
    *out = nullptr;
    if (!ctxs || n < 1 || n > 1024) return fail(FP_EINVAL, "fp_group_create: need 1..1024 contexts");
    for (int i = 0; i < n; ++i) {
        if (!ctxs[i]) return fail(FP_EINVAL, "fp_group_create: ctxs[%d] is NULL", i);
        for (int j = 0; j < i; ++j)
            if (ctxs[j] == ctxs[i]) return fail(FP_EINVAL, "fp_group_create: ctxs[%d] and ctxs[%d] are the same ctx (one worker per ctx)", j, i);
    }
    fp_group* g = new (std::nothrow) fp_group();
    if (!g) return fail(FP_ENOMEM, "out of host memory");
    for (int i = 0; i < n; ++i) {
        GroupWorker* w = new (std::nothrow) GroupWorker();
        if (!w) { fp_group_destroy(g); return fail(FP_ENOMEM, "out of host memory"); }
        w->ctx = ctxs[i];
        try {  // (no exception may leave an extern "C" function: vector growth and thread creation both can throw)
            g->workers.push_back(w);
        } catch (...) {
            delete w;
            fp_group_destroy(g);
            return fail(FP_ENOMEM, "out of host memory");
        }
        try {
            w->th = std::thread(group_worker_main, w);
        } catch (const std::exception& ex) {  // std::system_error: the process is out of threads
            fp_group_destroy(g);  // (joins the workers that did start; this one is not joinable)
            return fail(FP_EHIP, "fp_group_create: worker thread %d could not be started: %s", i, ex.what());
        }
    }
    *out = g;
    return FP_OK;
}

int fp_group_destroy(fp_group* g)
{
    if (!g) return FP_OK;
    for (GroupWorker* w : g->workers) {
        {
            std::lock_guard<std::mutex> lk(w->m);
            w->stop.store(true, std::memory_order_seq_cst);
        }
        w->cv.notify_one();
        if (w->th.joinable()) w->th.join();
        delete w;
    }
    delete g;
    return FP_OK;
}

int fp_group_submit(fp_group* g, const fp_shard_call* calls)
{
    if (!g || !calls) return fail(FP_EINVAL, "group/calls is NULL");
    const int n = (int)g->workers.size();
    for (int i = 0; i < n; ++i) {  // validate the whole round before any of it is posted
        const fp_shard_call& c = calls[i];
        if (!c.params) continue;
        if (!c.batch) return fail(FP_EINVAL, "fp_group_submit: calls[%d].batch is NULL", i);
        if (!c.result && !(c.fiss_opts && c.fiss_io)) return fail(FP_EINVAL, "fp_group_submit: calls[%d] needs result or fiss_opts + fiss_io", i);
        if (c.result && (c.fiss_opts || c.fiss_io)) return fail(FP_EINVAL, "fp_group_submit: calls[%d] sets both result and the FISS structs", i);
        if (c.n_copies < 0 || c.n_copies > kMaxCopies || (c.n_copies > 0 && !c.copies)) return fail(FP_EINVAL, "fp_group_submit: calls[%d].n_copies must be 0..%d", i, kMaxCopies);
    }
    // A shard whose earlier call failed takes no new work until fp_group_wait has reported (and cleared) the failure - and the round is
    // refused as a whole, before any of it is posted: the other shards must not run ahead of a shard that silently skipped its call.
    for (int i = 0; i < n; ++i) {
        if (!calls[i].params) continue;
        GroupWorker& w = *g->workers[i];
        group_wait_worker(w);  // the mailbox is one deep
        if (w.rc != FP_OK) return fail(w.rc, "fp_group_submit: shard %d still holds the error of an earlier call (%s); nothing of this round was posted - fp_group_wait reports and clears it", i, w.err.c_str());
    }
    for (int i = 0; i < n; ++i) {
        const fp_shard_call& c = calls[i];
        if (!c.params) continue;
        GroupWorker& w = *g->workers[i];
        w.params = *c.params;
        w.batch = *c.batch;
        if (c.result) w.result = *c.result;
        if (c.loop) w.loop = *c.loop;
        if (c.fiss_opts) { w.fopts = *c.fiss_opts; w.fio = *c.fiss_io; }
        w.kind = c.result ? (c.loop ? 2 : 1) : (c.loop ? 4 : 3);
        w.stream = c.stream;
        w.n_copies = c.n_copies;
        for (int k = 0; k < c.n_copies; ++k) w.copies[k] = c.copies[k];
        w.posted.fetch_add(1, std::memory_order_seq_cst);
        if (w.asleep.load(std::memory_order_seq_cst)) {
            std::lock_guard<std::mutex> lk(w.m);
            w.cv.notify_one();
        }
    }
    return FP_OK;
}

int fp_group_wait(fp_group* g)
{
    if (!g) return fail(FP_EINVAL, "group is NULL");
    int rc = FP_OK;
    for (size_t i = 0; i < g->workers.size(); ++i) {
        GroupWorker& w = *g->workers[i];
        group_wait_worker(w);
        if (w.rc != FP_OK) {
            if (rc == FP_OK) rc = fail(w.rc, "shard %zu: %s", i, w.err.c_str());
            w.rc = FP_OK;
            w.err.clear();
        }
    }
    return rc;
}

}  // extern "C"
