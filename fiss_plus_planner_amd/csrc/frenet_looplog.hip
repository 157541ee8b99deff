// frenet_looplog.hip - the driven trajectory of a device-resident closed loop (fp_loop_record, ABI 17).
//
// The reference's simulation loop returns `state_list`: one row per driven cycle (planners/benchmark/planning.py:135-148), the summed
// Stats (:129) and goal_reached.  A resident loop keeps its egos' states in HBM and moves them in place; loop_record_kernel, enqueued
// behind a step, copies what the step left there into the ego's next free row - the row index (n_rows) lives on the device, so a
// captured [step, record] pair replays for any number of cycles.
//
// One lane per ego.  A row is FP_LOG_COLS = 16 doubles = one 128-byte line of the [B][max_rows][16] layout: neighbouring egos' rows
// lie max_rows lines apart, so no two lanes ever share a line - the best the layout allows is that every lane writes its own line
// completely (eight 16-byte vector stores back to back, no partial line left behind).  The inputs ([B] / [B][3] / [B][4] / [B][6]
// arrays indexed by the lane) coalesce as they are.
// n_running: ballot + popcount per wavefront, one relaxed agent-scope atomic add per wavefront into a word the host call zeroed on the
// stream.  No LDS, no scratch.
#include "frenet_device.h"
#include "frenet_kernels.h"

namespace fp {

constexpr int kLogThreads = kWave;  // like advance_kernel: a 2048-ego batch spreads over 32 compute units

__global__ __launch_bounds__(kLogThreads) void loop_record_kernel(LoopLogArgs a)
{
    const int b = blockIdx.x * kLogThreads + (int)threadIdx.x;
    const fp_loop_io& io = a.io;
    const fp_loop_log& lg = a.log;
    bool running = false;
    if (b < a.B) {
        const int done = io.done[b];
        running = done == FP_RUNNING;
        if (lg.sealed[b] == 0) {
            const int4 st = a.stats ? *(const int4*)(a.stats + (size_t)b * 4) : make_int4(0, 0, 0, 0);
            if (lg.stats_sum) {
                int64_t* sum = lg.stats_sum + (size_t)b * 4;
                sum[0] += st.x; sum[1] += st.y; sum[2] += st.z; sum[3] += st.w;
            }
            const int cyc = io.cycles[b], n = lg.n_rows[b];
            if (cyc > n) {  // the ego moved in this step
                if (n < lg.max_rows) {
                    const double nan = __builtin_nan("");
                    double d_end = nan, v_end = nan, T = nan;
                    int best = -1;
                    if (a.end_state) {
                        d_end = a.end_state[(size_t)b * 3]; v_end = a.end_state[(size_t)b * 3 + 1]; T = a.end_state[(size_t)b * 3 + 2];
                    } else {
                        best = a.best_idx[b];
                        if (best >= 0) {  // as advance_ego (frenet_advance.h) decodes it
                            const int iv = best % a.nv, it = (best / a.nv) % a.nt, id = best / (a.nv * a.nt);
                            d_end = a.d_samples[id]; v_end = a.v_samples[(size_t)b * a.nv + iv]; T = a.t_samples[it];
                        }
                    }
                    const double* eg = io.ego + (size_t)b * 6;
                    const double* cs = io.cart_state + (size_t)b * 3;
                    const double s = eg[0], s_d = eg[1], s_dd = eg[2], d = eg[3], d_d = eg[4], d_dd = eg[5];
                    double2* row = (double2*)(lg.rows + ((size_t)b * lg.max_rows + n) * FP_LOG_COLS);
                    row[0] = make_double2((double)(io.t_now[b] - 1), cs[0]);  // TIME_STEP = the loop index i (:139), X
                    row[1] = make_double2(cs[1], cs[2]);                      // Y, YAW
                    row[2] = make_double2(s_d, d_d);                          // VELOCITY, VELOCITY_Y
                    row[3] = make_double2(s, s_dd);
                    row[4] = make_double2(d, d_dd);
                    row[5] = make_double2(a.best_cost[b], d_end);
                    row[6] = make_double2(v_end, T);
                    row[7] = make_double2((double)best, (double)done);
                    if (lg.row_stats) *(int4*)(lg.row_stats + ((size_t)b * lg.max_rows + n) * 4) = st;
                }
                lg.n_rows[b] = cyc;
            }
            if (!running) lg.sealed[b] = 1;
        }
    }
    if (lg.n_running) {
        const unsigned long long m = __ballot(running);
        if ((threadIdx.x & (kWave - 1)) == 0 && m != 0ull)
            __hip_atomic_fetch_add(lg.n_running, __popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

hipError_t launch_loop_record(const LoopLogArgs& a, hipStream_t stream)
{
    hipLaunchKernelGGL(loop_record_kernel, dim3((a.B + kLogThreads - 1) / kLogThreads), dim3(kLogThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fp
