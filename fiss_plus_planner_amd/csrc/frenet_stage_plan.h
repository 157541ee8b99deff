// frenet_stage_plan.h - where the arrays of one call go.  An entry point declares its arrays once, as a StageList, whatever the call's
// memory space.  FP_MEM_HOST: the list stages - plan_stage decides region and offset of every array, the output window and the arena's
// size, and CallStage::commit (frenet_abi.hip) is the one executor.  FP_MEM_DEVICE: the list passes through - every declaration hands the
// caller's address to the kernel's argument at once and nothing is recorded.  Host-side arithmetic only: no HIP call, no allocation
// (tests/test_stage_plan_cpu.py prints plans on a machine without a GPU).
#pragma once

#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace fp {

constexpr size_t kAlign = 256;
constexpr size_t kSmallRegion = 4u << 20;      // device bytes mirrored by the pinned host block
constexpr size_t kSmallMax = 64u << 10;        // arrays up to this size travel through the pinned block
constexpr size_t kZeroCopyInMax = 256u << 10;  // latency regime: inputs the kernels read straight from the pinned block (all of a call's arrays together)

inline size_t align_up(size_t v) { return (v + kAlign - 1) & ~(kAlign - 1); }

enum class StageKind : uint8_t { IN, IN_MUT, OUT, TEMP };  // IN_MUT: in/out array, staged in and copied straight back; TEMP: device-only scratch
// Where an item lives.  PINNED: the kernels address the pinned host block itself (no copy either way); WINDOW: the head of the arena,
// mirrored by the pinned block (one copy for all of them); LARGE: the arena behind the window (a copy of its own).  NONE: an output
// nobody asked for (NULL device pointer).
enum class StageRegion : uint8_t { NONE, PINNED, WINDOW, LARGE };

struct StageItem {
    StageKind kind;
    void* host;    // NULL for TEMP
    size_t bytes;
    void** dev;    // the device pointer commit fills
};

// The longest list of the library is fp_plan_fiss's (17 batch arrays, 4 sampling arrays, 8 outputs); the headroom also lets
// tests/test_stage_plan_cpu.py fill the whole window with 64 KiB arrays.  A list lives on its call's stack: nothing is allocated.
constexpr int kStageCap = 72;

struct StageList {
    StageItem item[kStageCap];
    int n = 0;  // items declared; beyond kStageCap nothing is stored and commit refuses the list
    // Pass-through (an FP_MEM_DEVICE call: the arrays are where the kernels read them): in / in_mut / out store the given address in
    // *dev - NULL for NULL, what plan_stage gives an output nobody asked for -, temp stores NULL (such a call has no arena), and no
    // item is recorded: n stays 0.
    const bool pass_through;

    explicit StageList(bool pass_through_ = false) : pass_through(pass_through_) {}
    void add(StageKind kind, const void* host, size_t bytes, void** dev)
    {
        if (pass_through) { *dev = const_cast<void*>(host); return; }
        if (n < kStageCap) item[n] = StageItem{kind, const_cast<void*>(host), bytes, dev};
        ++n;
    }
    bool overflow() const { return n > kStageCap; }
    template <typename T, typename D>  // (D: T or const T - a struct shared with the device path may hold the pointer as mutable)
    void in(const T* host, size_t count, D** dev)
    {
        static_assert(std::is_same<const T, const D>::value, "the device pointer's element type is the host array's");
        add(StageKind::IN, host, sizeof(T) * count, (void**)dev);
    }
    template <typename T>
    void in_mut(T* host, size_t count, T** dev) { add(StageKind::IN_MUT, host, sizeof(T) * count, (void**)dev); }
    template <typename T>
    void out(T* host, size_t count, T** dev) { add(StageKind::OUT, host, sizeof(T) * count, (void**)dev); }
    template <typename T>
    void temp(size_t count, T** dev) { add(StageKind::TEMP, nullptr, sizeof(T) * count, (void**)dev); }
};

// zero_copy_out (latency regime, a handful of egos): small outputs are written by the kernels straight into the pinned host block (it
// is device-visible) - no D2H command at all after the launch, only the stream synchronisation.  Larger batches keep the outputs in HBM
// (kernels of the same call read each other's outputs) and fetch them with one copy.
// The same regime can read its INPUTS from the pinned block too (fp_ctx_set_option("zero_copy_in"): 2 always, 1 when
// small_inputs_only): the host's memcpy into the block is the whole transfer, the kernels fetch what they touch over the link - no copy
// command, no blit kernel.  Only while the inputs of the call stay below kZeroCopyInMax bytes in total (a kernel re-reads parts of them;
// beyond that the copy engine wins).
struct StageRegime {
    bool zero_copy_out = false;
    int zero_copy_in = 0;
    bool small_inputs_only = false;  // the big tables are resident on the device (fp_batch.tables_tag): a few hundred bytes of per-ego arrays are left
};

struct StagePlan {
    StageRegion region[kStageCap];
    size_t offset[kStageCap];  // PINNED / WINDOW: into the pinned block and the arena's head alike; LARGE: into the arena (>= kSmallRegion)
    size_t small_in = 0;       // bytes of the window the inputs take
    bool flush = false;        // ... and whether the arena's copy of them has to be brought up to date (some input is WINDOW)
    size_t small_out_lo = 0, small_out_hi = 0;  // the output window
    size_t arena_bytes = 0;    // the arena the call needs, window included: every WINDOW / LARGE item ends at or below it
};

inline bool stage_zero_copy_in(const StageRegime& rg) { return rg.zero_copy_out && (rg.zero_copy_in == 2 || (rg.small_inputs_only && rg.zero_copy_in != 0)); }

// Inputs take the small window first, in declaration order, the outputs follow them; what does not fit the window (or is too big for
// it) goes to the large region in declaration order, TEMPs among them.  Every placement starts on a multiple of kAlign.  An input of
// zero bytes is not placed: it gets the large region's cursor as it stands ("any valid address").
inline StagePlan plan_stage(const StageList& l, const StageRegime& rg)
{
    StagePlan pl;
    const int n = l.n < kStageCap ? l.n : kStageCap;
    const bool zco = rg.zero_copy_out, zci = stage_zero_copy_in(rg);
    size_t small = 0;
    for (int i = 0; i < n; ++i) {
        const StageItem& it = l.item[i];
        pl.region[i] = it.kind == StageKind::OUT && (!it.host || it.bytes == 0) ? StageRegion::NONE : StageRegion::LARGE;
        pl.offset[i] = 0;
        if ((it.kind != StageKind::IN && it.kind != StageKind::IN_MUT) || it.bytes == 0) continue;
        const size_t at = align_up(small);
        if (it.kind == StageKind::IN_MUT && zco && it.bytes <= kSmallMax && at + it.bytes <= kSmallRegion) {
            pl.region[i] = StageRegion::PINNED;  // read and updated in place
        } else if (zci) {
            if (at + it.bytes <= kZeroCopyInMax) pl.region[i] = StageRegion::PINNED;
        } else if (it.bytes <= (zco ? kZeroCopyInMax : kSmallMax) && at + it.bytes <= kSmallRegion) {
            // (latency regime: bigger arrays too - one transfer for the whole call instead of one more copy command per array)
            pl.region[i] = StageRegion::WINDOW;
            pl.flush = true;
        }
        if (pl.region[i] == StageRegion::LARGE) continue;
        pl.offset[i] = at;
        small = at + it.bytes;
    }
    pl.small_in = small;
    pl.small_out_lo = pl.small_out_hi = align_up(small);
    size_t large = kSmallRegion;
    for (int i = 0; i < n; ++i) {
        const StageItem& it = l.item[i];
        if (pl.region[i] != StageRegion::LARGE) continue;
        if (it.kind == StageKind::OUT && it.bytes <= kSmallMax && align_up(pl.small_out_hi) + it.bytes <= kSmallRegion) {
            pl.region[i] = zco ? StageRegion::PINNED : StageRegion::WINDOW;
            pl.offset[i] = align_up(pl.small_out_hi);
            pl.small_out_hi = pl.offset[i] + it.bytes;
            continue;
        }
        if (it.bytes > 0 || it.kind == StageKind::TEMP) large = align_up(large);
        pl.offset[i] = large;
        large += it.bytes;
    }
    pl.arena_bytes = large;
    return pl;
}

// Every placed item inside its region and the arena (CallStage::commit refuses a plan that fails this: a planner bug is an error code,
// never an overrun).
inline bool stage_plan_inside(const StageList& l, const StagePlan& pl)
{
    const int n = l.n < kStageCap ? l.n : kStageCap;
    for (int i = 0; i < n; ++i) {
        const size_t lo = pl.offset[i], hi = lo + l.item[i].bytes;
        if (pl.region[i] == StageRegion::LARGE ? (lo < kSmallRegion || hi > pl.arena_bytes) : (pl.region[i] != StageRegion::NONE && hi > kSmallRegion)) return false;
    }
    return pl.arena_bytes >= kSmallRegion;
}

}  // namespace fp
