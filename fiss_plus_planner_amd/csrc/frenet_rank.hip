// frenet_rank.hip - the K cheapest feasible candidates of every ego, ranked on the device (fp_rank_feasible, ABI 18).
//
// The dense pass leaves cost_tbl / flag_tbl [B][C] in HBM and one index per ego, the argmin.  rank_feasible_kernel turns an ego's rows
// into a short list: the survivors (no FP_FLAG_INFEASIBLE bit, cost not NaN) in ascending cost, among equal costs the HIGHER flat index
// first - the order in which FOP's "last minimum wins" loop (frenet_optimal_planner.py:263-268) would hand out winners if each winner
// were removed in turn.  Plane 0 is therefore best_idx / best_cost of the call that wrote the tables.
//
// One workgroup per ego, one pass over the ego's rows (4 + 8 bytes per candidate, one candidate per lane: coalesced), select before
// stage:
//   - a chunk's survivors are compacted by ballot + popcount into an LDS buffer of kRankCap (key, tie) pairs.  key = the cost's bits
//     mapped so that unsigned order is numeric order (-0.0 folded onto +0.0, which compare equal); tie = kRankTieMax - index, so that
//     ascending (key, tie) IS the order above, and it is total: no two candidates compare equal;
//   - when the next chunk might not fit, the buffer is sorted (bitonic, in LDS) and cut to its K smallest pairs; the K-th becomes the
//     threshold, and from then on only survivors below it are staged at all.  "All 16 384 survive" takes ten such cuts; the headline
//     scenes (~100-140 survivors of 567) take none;
//   - one last sort of the next power of two above what is left, then lanes 0 .. K-1 write the planes.  rank_cost is read back from
//     the table (a line this workgroup has just read: L2), so it is the entry's bits whatever the key folded.
// What is kept at a cut is a function of the SET of pairs in the buffer, and every order decision is a comparison of distinct pairs:
// the planes are a function of the tables alone, two runs give the same bits.  No atomics, no scratch; 20.6 KB of LDS.
#include "frenet_device.h"
#include "frenet_kernels.h"

namespace fp {

constexpr int kRankThreads = 256;
constexpr int kRankWaves = kRankThreads / kWave;
constexpr int kRankCap = 2048;           // pairs the LDS buffer holds: 16 KB of keys + 4 KB of ties
constexpr unsigned kRankTieMax = 0xffffu;  // tie = kRankTieMax - index (FP_MAX_CAND - 1 < 65 536)
static_assert(FP_MAX_CAND - 1 <= (int)kRankTieMax, "a flat index must fit the 16-bit tie word");
static_assert(FP_MAX_RANK <= kRankThreads && FP_MAX_RANK + kRankThreads <= kRankCap, "a cut must leave room for the next chunk");
static_assert((kRankCap & (kRankCap - 1)) == 0, "the bitonic network sorts powers of two");

// cost bits -> unsigned key: a < b (numbers, not NaN)  <=>  key(a) < key(b); -0.0 and +0.0 share a key
__device__ __forceinline__ unsigned long long rank_key(double cost)
{
    const unsigned long long u = cost == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(cost);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ bool rank_less(unsigned long long ka, unsigned ta, unsigned long long kb, unsigned tb)
{
    return ka < kb || (ka == kb && ta < tb);
}

// ascending bitonic sort of s_key / s_tie [0, n), n a power of two <= kRankCap; ends with a barrier
__device__ __forceinline__ void rank_sort(unsigned long long* s_key, unsigned short* s_tie, int n, int tid)
{
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n >> 1); t += kRankThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long ki = s_key[i], kl = s_key[l];
                const unsigned ti = s_tie[i], tl = s_tie[l];
                const bool up = (i & k) == 0;
                if (rank_less(kl, tl, ki, ti) == up) {
                    s_key[i] = kl; s_key[l] = ki;
                    s_tie[i] = (unsigned short)tl; s_tie[l] = (unsigned short)ti;
                }
            }
            __syncthreads();
        }
    }
}

// sorts the `cnt` pairs of the buffer (padded to a power of two with pairs above every real one); ends with a barrier
__device__ __forceinline__ void rank_sort_first(unsigned long long* s_key, unsigned short* s_tie, int cnt, int tid)
{
    int n = 1;
    while (n < cnt) n <<= 1;
    for (int i = cnt + tid; i < n; i += kRankThreads) {
        s_key[i] = ~0ull;  // (above +inf's key; NaN costs never get here)
        s_tie[i] = (unsigned short)kRankTieMax;
    }
    __syncthreads();
    rank_sort(s_key, s_tie, n, tid);
}

__global__ __launch_bounds__(kRankThreads) void rank_feasible_kernel(RankArgs a)
{
    __shared__ unsigned long long s_key[kRankCap];
    __shared__ unsigned short s_tie[kRankCap];
    __shared__ int s_count[2][kRankWaves][2];  // [chunk parity][wave]{survivors, staged}: one barrier per chunk
    const int b = a.perm ? a.perm[blockIdx.x] : (int)blockIdx.x;
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
    const int B = a.B, C = a.C, K = a.K;
    if (a.skip && a.skip[b]) {  // not planned: the dense pass wrote no rows for this ego
        if (tid < K) {
            a.rank_idx[(size_t)tid * B + b] = -1;
            a.rank_cost[(size_t)tid * B + b] = __builtin_nan("");
        }
        if (tid == 0 && a.n_feasible) a.n_feasible[b] = 0;
        return;
    }
    const double* cost = a.cost_tbl + (size_t)b * C;
    const uint32_t* flag = a.flag_tbl + (size_t)b * C;
    int cnt = 0, total = 0;  // pairs in the buffer, survivors so far (both workgroup-uniform)
    bool have_thr = false;   // the buffer was cut: only pairs below (thr_key, thr_tie) can still make the list
    unsigned long long thr_key = 0ull;
    unsigned thr_tie = 0u;
    int par = 0;
    for (int c0 = 0; c0 < C; c0 += kRankThreads, par ^= 1) {
        if (cnt + kRankThreads > kRankCap) {  // the chunk might not fit: keep the K smallest (cnt > kRankCap - kRankThreads >= K here)
            rank_sort_first(s_key, s_tie, cnt, tid);
            thr_key = s_key[K - 1];
            thr_tie = s_tie[K - 1];
            have_thr = true;
            cnt = K;  // (the chunks that follow are staged behind the K pairs kept: the threshold's slot is not rewritten)
        }
        const int c = c0 + tid;
        bool alive = false;
        unsigned long long key = 0ull;
        const unsigned tie = kRankTieMax - (unsigned)c;
        if (c < C) {
            const uint32_t fl = flag[c];
            const double v = cost[c];
            alive = !(fl & FP_FLAG_INFEASIBLE) && v == v;
            key = rank_key(v);
        }
        const bool keep = alive && (!have_thr || rank_less(key, tie, thr_key, thr_tie));
        const unsigned long long m_alive = __ballot(alive), m_keep = __ballot(keep);
        if (lane == 0) {
            s_count[par][wave][0] = __popcll(m_alive);
            s_count[par][wave][1] = __popcll(m_keep);
        }
        __syncthreads();
        int before = 0, staged = 0;
        for (int w = 0; w < kRankWaves; ++w) {
            const int n = s_count[par][w][1];
            before += w < wave ? n : 0;
            staged += n;
            total += s_count[par][w][0];
        }
        if (keep) {
            const int at = cnt + before + __popcll(m_keep & ((1ull << lane) - 1ull));  // < cnt + kRankThreads <= kRankCap
            s_key[at] = key;
            s_tie[at] = (unsigned short)tie;
        }
        cnt += staged;
    }
    rank_sort_first(s_key, s_tie, cnt, tid);
    if (tid < K) {
        int idx = -1;
        double v = __builtin_nan("");
        if (tid < cnt) {
            idx = (int)(kRankTieMax - (unsigned)s_tie[tid]);
            v = cost[idx];
        }
        a.rank_idx[(size_t)tid * B + b] = idx;
        a.rank_cost[(size_t)tid * B + b] = v;
    }
    if (tid == 0 && a.n_feasible) a.n_feasible[b] = total;
}

hipError_t launch_rank_feasible(const RankArgs& a, hipStream_t stream)
{
    if (a.B < 1 || a.C < 1 || a.C > FP_MAX_CAND || a.K < 1 || a.K > FP_MAX_RANK || !a.cost_tbl || !a.flag_tbl || !a.rank_idx || !a.rank_cost)
        return hipErrorInvalidValue;  // (internal: fp_rank_feasible has checked its arguments)
    hipLaunchKernelGGL(rank_feasible_kernel, dim3(a.B), dim3(kRankThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fp
