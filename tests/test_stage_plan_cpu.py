"""CPU: plan_stage (fiss_plus_planner_amd/csrc/frenet_stage_plan.h), the host function that places every array of a FP_MEM_HOST call
(pinned block, mirrored window, large arena) and sizes the arena, printed for a fixed list of cases by a small host program and compared
with the table below.

The rows are what HostStage's reserve / in / in_mut / flush_in / out / temp gave for the same sequence of calls before the placement was
one function (the old class, its HIP calls stubbed, printed them once).  Every case runs in four regimes: thr (throughput: no zero copy),
lat0 / lat1 / lat2 (latency: zero_copy_out with fp_ctx_set_option("zero_copy_in") 0, 1, 2).  `resident` cases have the big tables on the
device (fp_batch.tables_tag: StageRegime::small_inputs_only).  An item reads REGION:OFFSET - P the pinned block addressed directly,
W the window mirrored into the arena, L the large arena (offsets from the arena's base), - an output nobody asked for."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "fiss_plus_planner_amd", "csrc")

ALIGN, SMALL_REGION, SMALL_MAX, ZC_IN_MAX, STAGE_CAP = 256, 4 << 20, 64 << 10, 256 << 10, 72
REGIMES = ("thr", "lat0", "lat1", "lat2")

# per-ego arrays of a B = 1 planner batch (5 x 5 x 5): d_samples, t_samples, v_samples, target_speed, ego, frame_of, scene_of, t_now
_EGO1 = "in:40 in:40 in:40 in:8 in:48 in:4 in:4 in:4"
# ... and its tables when they travel: nx, knots, coef (81 knots), obs_pose, obs_dims, final_time_step (10 obstacles, 100 steps)
_TABLES1 = "in:4 in:648 in:5184 in:32000 in:160 in:4"
# fp_plan_dense's outputs (B = 1, C = 125, series of 16 x 128 doubles): best_idx, best_cost, stats, cost_tbl, flag_tbl, best_flags,
# best_traj, fopplus (NULL), audit (NULL)
_DENSE_OUT1 = "out:4 out:8 out:16 out:1000 out:500 out:4 out:16384 null:8 null:4"
# fp_plan_fiss: samp_min / samp_max / samp_res, prev_best_idx (in/out); best_ijk, best_cost, end_state, refined, stats, trace (3 rounds),
# best_flags, best_traj
_FISS_IN1 = "in:24 in:24 in:24 mut:12"
_FISS_OUT1 = "out:12 out:8 out:24 out:4 out:16 out:672 out:4 out:16384"

# name, "resident" or "-" ("through": a pass-through list, see the tests at the end), the declared list: in / mut (IN_MUT) / out / null (OUT with a NULL host pointer) / temp : bytes
CASES = [
    ("small_max", "-", f"in:{SMALL_MAX} in:{SMALL_MAX + 1} out:{SMALL_MAX} out:{SMALL_MAX + 1}"),
    ("latency_in_max", "-", f"in:{ZC_IN_MAX} in:{ZC_IN_MAX + 1} out:8"),
    ("zero_copy_exact", "-", " ".join([f"in:{SMALL_MAX}"] * 4) + " out:8"),
    ("zero_copy_over", "-", " ".join([f"in:{SMALL_MAX}"] * 4) + " in:256 out:8"),
    ("zero_copy_exact_resident", "resident", " ".join([f"in:{SMALL_MAX}"] * 4) + " out:8"),
    ("zero_copy_over_resident", "resident", " ".join([f"in:{SMALL_MAX}"] * 4) + " in:256 in:8 out:8"),
    ("fill_in", "-", " ".join([f"in:{SMALL_MAX}"] * 65) + " in:256 out:8"),
    ("fill_in_odd", "-", " ".join(["in:65000"] * 65) + " out:100"),
    ("fill_out", "-", "in:100 " + " ".join([f"out:{SMALL_MAX}"] * 64) + " out:8"),
    ("fill_out_odd", "-", "in:100 " + " ".join(["out:65000"] * 65) + " out:8"),
    ("odds_and_ends", "-", f"in:0 in:24 mut:4096 mut:{SMALL_MAX + 1} mut:0 in:0 in:7 null:64 out:0 out:40 temp:1000 out:8 out:70000 temp:3 out:16"),
    ("odds_and_ends_resident", "resident", f"in:0 in:24 mut:4096 mut:{SMALL_MAX + 1} mut:0 in:0 in:7 null:64 out:0 out:40 temp:1000 out:8 out:70000 temp:3 out:16"),
    ("dense_b1", "resident", f"{_EGO1} {_DENSE_OUT1}"),
    ("dense_b1_tables_travel", "-", f"{_EGO1} {_TABLES1} {_DENSE_OUT1}"),
    ("fiss_b1", "resident", f"{_EGO1} {_FISS_IN1} {_FISS_OUT1}"),
    ("fiss_b1_inline", "resident", f"temp:1024 mut:12 {_FISS_OUT1}"),  # inline inputs accepted: the mirror and what is left
    ("fiss_b1_tables_travel", "-", f"{_EGO1} {_TABLES1} {_FISS_IN1} {_FISS_OUT1}"),
]

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "frenet_stage_plan.h"
using namespace fp;
int main()
{
    static char line[1 << 16];
    static unsigned char dummy[1024], poison;
    static void* dev[1024];
    static const char* kRegime[] = {"thr", "lat0", "lat1", "lat2"};
    static const char kRegion[] = {'-', 'P', 'W', 'L'};
    while (fgets(line, sizeof line, stdin)) {
        char* save;
        const char* name = strtok_r(line, " \n", &save);
        if (!name) continue;
        const char* flag = strtok_r(nullptr, " \n", &save);
        const bool resident = strcmp(flag, "resident") == 0, through = strcmp(flag, "through") == 0;
        StageList l(through);
        if (through) std::printf("%s through", name);
        int k = 0;
        for (char* t; (t = strtok_r(nullptr, " \n", &save)); ++k) {
            char* c = strchr(t, ':');
            *c = 0;
            const size_t bytes = strtoull(c + 1, nullptr, 10);
            void** d = &dev[k % 1024];
            void* host = &dummy[k % 1024];  // (every declaration its own address)
            *d = &poison;
            if (strcmp(t, "in") == 0) l.add(StageKind::IN, host, bytes, d);
            else if (strcmp(t, "mut") == 0) l.add(StageKind::IN_MUT, host, bytes, d);
            else if (strcmp(t, "out") == 0) l.add(StageKind::OUT, host, bytes, d);
            else if (strcmp(t, "null") == 0) l.add(StageKind::OUT, nullptr, bytes, d);
            else if (strcmp(t, "temp") == 0) l.add(StageKind::TEMP, nullptr, bytes, d);
            else return 1;
            // pass-through: what the declaration stored - the given address, NULL, or nothing / something else
            if (through) std::printf(" %c", *d == host ? '=' : *d == nullptr ? '0' : '?');
        }
        if (through) { std::printf(" n=%d overflow=%d\n", l.n, (int)l.overflow()); continue; }
        if (l.overflow()) { std::printf("%s overflow n=%d\n", name, l.n); continue; }
        for (int r = 0; r < 4; ++r) {
            StageRegime rg;
            rg.zero_copy_out = r > 0;
            rg.zero_copy_in = r > 0 ? r - 1 : 2;  // (the throughput regime ignores the option)
            rg.small_inputs_only = resident;
            const StagePlan pl = plan_stage(l, rg);
            std::printf("%s %s", name, kRegime[r]);
            for (int i = 0; i < l.n; ++i) std::printf(" %c:%zu", kRegion[(int)pl.region[i]], pl.offset[i]);
            std::printf(" in=%zu%s out=[%zu,%zu) total=%zu%s\n", pl.small_in, pl.flush ? "+flush" : "", pl.small_out_lo, pl.small_out_hi, pl.arena_bytes,
                        stage_plan_inside(l, pl) ? "" : " OUTSIDE");
        }
    }
    return 0;
}
"""

EXPECTED = """
small_max thr W:0 L:4194304 W:65536 L:4260096 in=65536+flush out=[65536,131072) total=4325633
small_max lat0 W:0 W:65536 P:131328 L:4194304 in=131073+flush out=[131328,196864) total=4259841
small_max lat1 W:0 W:65536 P:131328 L:4194304 in=131073+flush out=[131328,196864) total=4259841
small_max lat2 P:0 P:65536 P:131328 L:4194304 in=131073 out=[131328,196864) total=4259841
latency_in_max thr L:4194304 L:4456448 W:0 in=0 out=[0,8) total=4718593
latency_in_max lat0 W:0 L:4194304 P:262144 in=262144+flush out=[262144,262152) total=4456449
latency_in_max lat1 W:0 L:4194304 P:262144 in=262144+flush out=[262144,262152) total=4456449
latency_in_max lat2 P:0 L:4194304 P:262144 in=262144 out=[262144,262152) total=4456449
zero_copy_exact thr W:0 W:65536 W:131072 W:196608 W:262144 in=262144+flush out=[262144,262152) total=4194304
zero_copy_exact lat0 W:0 W:65536 W:131072 W:196608 P:262144 in=262144+flush out=[262144,262152) total=4194304
zero_copy_exact lat1 W:0 W:65536 W:131072 W:196608 P:262144 in=262144+flush out=[262144,262152) total=4194304
zero_copy_exact lat2 P:0 P:65536 P:131072 P:196608 P:262144 in=262144 out=[262144,262152) total=4194304
zero_copy_over thr W:0 W:65536 W:131072 W:196608 W:262144 W:262400 in=262400+flush out=[262400,262408) total=4194304
zero_copy_over lat0 W:0 W:65536 W:131072 W:196608 W:262144 P:262400 in=262400+flush out=[262400,262408) total=4194304
zero_copy_over lat1 W:0 W:65536 W:131072 W:196608 W:262144 P:262400 in=262400+flush out=[262400,262408) total=4194304
zero_copy_over lat2 P:0 P:65536 P:131072 P:196608 L:4194304 P:262144 in=262144 out=[262144,262152) total=4194560
zero_copy_exact_resident thr W:0 W:65536 W:131072 W:196608 W:262144 in=262144+flush out=[262144,262152) total=4194304
zero_copy_exact_resident lat0 W:0 W:65536 W:131072 W:196608 P:262144 in=262144+flush out=[262144,262152) total=4194304
zero_copy_exact_resident lat1 P:0 P:65536 P:131072 P:196608 P:262144 in=262144 out=[262144,262152) total=4194304
zero_copy_exact_resident lat2 P:0 P:65536 P:131072 P:196608 P:262144 in=262144 out=[262144,262152) total=4194304
zero_copy_over_resident thr W:0 W:65536 W:131072 W:196608 W:262144 W:262400 W:262656 in=262408+flush out=[262656,262664) total=4194304
zero_copy_over_resident lat0 W:0 W:65536 W:131072 W:196608 W:262144 W:262400 P:262656 in=262408+flush out=[262656,262664) total=4194304
zero_copy_over_resident lat1 P:0 P:65536 P:131072 P:196608 L:4194304 L:4194560 P:262144 in=262144 out=[262144,262152) total=4194568
zero_copy_over_resident lat2 P:0 P:65536 P:131072 P:196608 L:4194304 L:4194560 P:262144 in=262144 out=[262144,262152) total=4194568
fill_in thr W:0 W:65536 W:131072 W:196608 W:262144 W:327680 W:393216 W:458752 W:524288 W:589824 W:655360 W:720896 W:786432 W:851968 W:917504 W:983040 W:1048576 W:1114112 W:1179648 W:1245184 W:1310720 W:1376256 W:1441792 W:1507328 W:1572864 W:1638400 W:1703936 W:1769472 W:1835008 W:1900544 W:1966080 W:2031616 W:2097152 W:2162688 W:2228224 W:2293760 W:2359296 W:2424832 W:2490368 W:2555904 W:2621440 W:2686976 W:2752512 W:2818048 W:2883584 W:2949120 W:3014656 W:3080192 W:3145728 W:3211264 W:3276800 W:3342336 W:3407872 W:3473408 W:3538944 W:3604480 W:3670016 W:3735552 W:3801088 W:3866624 W:3932160 W:3997696 W:4063232 W:4128768 L:4194304 L:4259840 L:4260096 in=4194304+flush out=[4194304,4194304) total=4260104
fill_in lat0 W:0 W:65536 W:131072 W:196608 W:262144 W:327680 W:393216 W:458752 W:524288 W:589824 W:655360 W:720896 W:786432 W:851968 W:917504 W:983040 W:1048576 W:1114112 W:1179648 W:1245184 W:1310720 W:1376256 W:1441792 W:1507328 W:1572864 W:1638400 W:1703936 W:1769472 W:1835008 W:1900544 W:1966080 W:2031616 W:2097152 W:2162688 W:2228224 W:2293760 W:2359296 W:2424832 W:2490368 W:2555904 W:2621440 W:2686976 W:2752512 W:2818048 W:2883584 W:2949120 W:3014656 W:3080192 W:3145728 W:3211264 W:3276800 W:3342336 W:3407872 W:3473408 W:3538944 W:3604480 W:3670016 W:3735552 W:3801088 W:3866624 W:3932160 W:3997696 W:4063232 W:4128768 L:4194304 L:4259840 L:4260096 in=4194304+flush out=[4194304,4194304) total=4260104
fill_in lat1 W:0 W:65536 W:131072 W:196608 W:262144 W:327680 W:393216 W:458752 W:524288 W:589824 W:655360 W:720896 W:786432 W:851968 W:917504 W:983040 W:1048576 W:1114112 W:1179648 W:1245184 W:1310720 W:1376256 W:1441792 W:1507328 W:1572864 W:1638400 W:1703936 W:1769472 W:1835008 W:1900544 W:1966080 W:2031616 W:2097152 W:2162688 W:2228224 W:2293760 W:2359296 W:2424832 W:2490368 W:2555904 W:2621440 W:2686976 W:2752512 W:2818048 W:2883584 W:2949120 W:3014656 W:3080192 W:3145728 W:3211264 W:3276800 W:3342336 W:3407872 W:3473408 W:3538944 W:3604480 W:3670016 W:3735552 W:3801088 W:3866624 W:3932160 W:3997696 W:4063232 W:4128768 L:4194304 L:4259840 L:4260096 in=4194304+flush out=[4194304,4194304) total=4260104
fill_in lat2 P:0 P:65536 P:131072 P:196608 L:4194304 L:4259840 L:4325376 L:4390912 L:4456448 L:4521984 L:4587520 L:4653056 L:4718592 L:4784128 L:4849664 L:4915200 L:4980736 L:5046272 L:5111808 L:5177344 L:5242880 L:5308416 L:5373952 L:5439488 L:5505024 L:5570560 L:5636096 L:5701632 L:5767168 L:5832704 L:5898240 L:5963776 L:6029312 L:6094848 L:6160384 L:6225920 L:6291456 L:6356992 L:6422528 L:6488064 L:6553600 L:6619136 L:6684672 L:6750208 L:6815744 L:6881280 L:6946816 L:7012352 L:7077888 L:7143424 L:7208960 L:7274496 L:7340032 L:7405568 L:7471104 L:7536640 L:7602176 L:7667712 L:7733248 L:7798784 L:7864320 L:7929856 L:7995392 L:8060928 L:8126464 L:8192000 P:262144 in=262144 out=[262144,262152) total=8192256
fill_in_odd thr W:0 W:65024 W:130048 W:195072 W:260096 W:325120 W:390144 W:455168 W:520192 W:585216 W:650240 W:715264 W:780288 W:845312 W:910336 W:975360 W:1040384 W:1105408 W:1170432 W:1235456 W:1300480 W:1365504 W:1430528 W:1495552 W:1560576 W:1625600 W:1690624 W:1755648 W:1820672 W:1885696 W:1950720 W:2015744 W:2080768 W:2145792 W:2210816 W:2275840 W:2340864 W:2405888 W:2470912 W:2535936 W:2600960 W:2665984 W:2731008 W:2796032 W:2861056 W:2926080 W:2991104 W:3056128 W:3121152 W:3186176 W:3251200 W:3316224 W:3381248 W:3446272 W:3511296 W:3576320 W:3641344 W:3706368 W:3771392 W:3836416 W:3901440 W:3966464 W:4031488 W:4096512 L:4194304 W:4161536 in=4161512+flush out=[4161536,4161636) total=4259304
fill_in_odd lat0 W:0 W:65024 W:130048 W:195072 W:260096 W:325120 W:390144 W:455168 W:520192 W:585216 W:650240 W:715264 W:780288 W:845312 W:910336 W:975360 W:1040384 W:1105408 W:1170432 W:1235456 W:1300480 W:1365504 W:1430528 W:1495552 W:1560576 W:1625600 W:1690624 W:1755648 W:1820672 W:1885696 W:1950720 W:2015744 W:2080768 W:2145792 W:2210816 W:2275840 W:2340864 W:2405888 W:2470912 W:2535936 W:2600960 W:2665984 W:2731008 W:2796032 W:2861056 W:2926080 W:2991104 W:3056128 W:3121152 W:3186176 W:3251200 W:3316224 W:3381248 W:3446272 W:3511296 W:3576320 W:3641344 W:3706368 W:3771392 W:3836416 W:3901440 W:3966464 W:4031488 W:4096512 L:4194304 P:4161536 in=4161512+flush out=[4161536,4161636) total=4259304
fill_in_odd lat1 W:0 W:65024 W:130048 W:195072 W:260096 W:325120 W:390144 W:455168 W:520192 W:585216 W:650240 W:715264 W:780288 W:845312 W:910336 W:975360 W:1040384 W:1105408 W:1170432 W:1235456 W:1300480 W:1365504 W:1430528 W:1495552 W:1560576 W:1625600 W:1690624 W:1755648 W:1820672 W:1885696 W:1950720 W:2015744 W:2080768 W:2145792 W:2210816 W:2275840 W:2340864 W:2405888 W:2470912 W:2535936 W:2600960 W:2665984 W:2731008 W:2796032 W:2861056 W:2926080 W:2991104 W:3056128 W:3121152 W:3186176 W:3251200 W:3316224 W:3381248 W:3446272 W:3511296 W:3576320 W:3641344 W:3706368 W:3771392 W:3836416 W:3901440 W:3966464 W:4031488 W:4096512 L:4194304 P:4161536 in=4161512+flush out=[4161536,4161636) total=4259304
fill_in_odd lat2 P:0 P:65024 P:130048 P:195072 L:4194304 L:4259328 L:4324352 L:4389376 L:4454400 L:4519424 L:4584448 L:4649472 L:4714496 L:4779520 L:4844544 L:4909568 L:4974592 L:5039616 L:5104640 L:5169664 L:5234688 L:5299712 L:5364736 L:5429760 L:5494784 L:5559808 L:5624832 L:5689856 L:5754880 L:5819904 L:5884928 L:5949952 L:6014976 L:6080000 L:6145024 L:6210048 L:6275072 L:6340096 L:6405120 L:6470144 L:6535168 L:6600192 L:6665216 L:6730240 L:6795264 L:6860288 L:6925312 L:6990336 L:7055360 L:7120384 L:7185408 L:7250432 L:7315456 L:7380480 L:7445504 L:7510528 L:7575552 L:7640576 L:7705600 L:7770624 L:7835648 L:7900672 L:7965696 L:8030720 L:8095744 P:260096 in=260072 out=[260096,260196) total=8160744
fill_out thr W:0 W:256 W:65792 W:131328 W:196864 W:262400 W:327936 W:393472 W:459008 W:524544 W:590080 W:655616 W:721152 W:786688 W:852224 W:917760 W:983296 W:1048832 W:1114368 W:1179904 W:1245440 W:1310976 W:1376512 W:1442048 W:1507584 W:1573120 W:1638656 W:1704192 W:1769728 W:1835264 W:1900800 W:1966336 W:2031872 W:2097408 W:2162944 W:2228480 W:2294016 W:2359552 W:2425088 W:2490624 W:2556160 W:2621696 W:2687232 W:2752768 W:2818304 W:2883840 W:2949376 W:3014912 W:3080448 W:3145984 W:3211520 W:3277056 W:3342592 W:3408128 W:3473664 W:3539200 W:3604736 W:3670272 W:3735808 W:3801344 W:3866880 W:3932416 W:3997952 W:4063488 L:4194304 W:4129024 in=100+flush out=[256,4129032) total=4259840
fill_out lat0 W:0 P:256 P:65792 P:131328 P:196864 P:262400 P:327936 P:393472 P:459008 P:524544 P:590080 P:655616 P:721152 P:786688 P:852224 P:917760 P:983296 P:1048832 P:1114368 P:1179904 P:1245440 P:1310976 P:1376512 P:1442048 P:1507584 P:1573120 P:1638656 P:1704192 P:1769728 P:1835264 P:1900800 P:1966336 P:2031872 P:2097408 P:2162944 P:2228480 P:2294016 P:2359552 P:2425088 P:2490624 P:2556160 P:2621696 P:2687232 P:2752768 P:2818304 P:2883840 P:2949376 P:3014912 P:3080448 P:3145984 P:3211520 P:3277056 P:3342592 P:3408128 P:3473664 P:3539200 P:3604736 P:3670272 P:3735808 P:3801344 P:3866880 P:3932416 P:3997952 P:4063488 L:4194304 P:4129024 in=100+flush out=[256,4129032) total=4259840
fill_out lat1 W:0 P:256 P:65792 P:131328 P:196864 P:262400 P:327936 P:393472 P:459008 P:524544 P:590080 P:655616 P:721152 P:786688 P:852224 P:917760 P:983296 P:1048832 P:1114368 P:1179904 P:1245440 P:1310976 P:1376512 P:1442048 P:1507584 P:1573120 P:1638656 P:1704192 P:1769728 P:1835264 P:1900800 P:1966336 P:2031872 P:2097408 P:2162944 P:2228480 P:2294016 P:2359552 P:2425088 P:2490624 P:2556160 P:2621696 P:2687232 P:2752768 P:2818304 P:2883840 P:2949376 P:3014912 P:3080448 P:3145984 P:3211520 P:3277056 P:3342592 P:3408128 P:3473664 P:3539200 P:3604736 P:3670272 P:3735808 P:3801344 P:3866880 P:3932416 P:3997952 P:4063488 L:4194304 P:4129024 in=100+flush out=[256,4129032) total=4259840
fill_out lat2 P:0 P:256 P:65792 P:131328 P:196864 P:262400 P:327936 P:393472 P:459008 P:524544 P:590080 P:655616 P:721152 P:786688 P:852224 P:917760 P:983296 P:1048832 P:1114368 P:1179904 P:1245440 P:1310976 P:1376512 P:1442048 P:1507584 P:1573120 P:1638656 P:1704192 P:1769728 P:1835264 P:1900800 P:1966336 P:2031872 P:2097408 P:2162944 P:2228480 P:2294016 P:2359552 P:2425088 P:2490624 P:2556160 P:2621696 P:2687232 P:2752768 P:2818304 P:2883840 P:2949376 P:3014912 P:3080448 P:3145984 P:3211520 P:3277056 P:3342592 P:3408128 P:3473664 P:3539200 P:3604736 P:3670272 P:3735808 P:3801344 P:3866880 P:3932416 P:3997952 P:4063488 L:4194304 P:4129024 in=100 out=[256,4129032) total=4259840
fill_out_odd thr W:0 W:256 W:65280 W:130304 W:195328 W:260352 W:325376 W:390400 W:455424 W:520448 W:585472 W:650496 W:715520 W:780544 W:845568 W:910592 W:975616 W:1040640 W:1105664 W:1170688 W:1235712 W:1300736 W:1365760 W:1430784 W:1495808 W:1560832 W:1625856 W:1690880 W:1755904 W:1820928 W:1885952 W:1950976 W:2016000 W:2081024 W:2146048 W:2211072 W:2276096 W:2341120 W:2406144 W:2471168 W:2536192 W:2601216 W:2666240 W:2731264 W:2796288 W:2861312 W:2926336 W:2991360 W:3056384 W:3121408 W:3186432 W:3251456 W:3316480 W:3381504 W:3446528 W:3511552 W:3576576 W:3641600 W:3706624 W:3771648 W:3836672 W:3901696 W:3966720 W:4031744 W:4096768 L:4194304 W:4161792 in=100+flush out=[256,4161800) total=4259304
fill_out_odd lat0 W:0 P:256 P:65280 P:130304 P:195328 P:260352 P:325376 P:390400 P:455424 P:520448 P:585472 P:650496 P:715520 P:780544 P:845568 P:910592 P:975616 P:1040640 P:1105664 P:1170688 P:1235712 P:1300736 P:1365760 P:1430784 P:1495808 P:1560832 P:1625856 P:1690880 P:1755904 P:1820928 P:1885952 P:1950976 P:2016000 P:2081024 P:2146048 P:2211072 P:2276096 P:2341120 P:2406144 P:2471168 P:2536192 P:2601216 P:2666240 P:2731264 P:2796288 P:2861312 P:2926336 P:2991360 P:3056384 P:3121408 P:3186432 P:3251456 P:3316480 P:3381504 P:3446528 P:3511552 P:3576576 P:3641600 P:3706624 P:3771648 P:3836672 P:3901696 P:3966720 P:4031744 P:4096768 L:4194304 P:4161792 in=100+flush out=[256,4161800) total=4259304
fill_out_odd lat1 W:0 P:256 P:65280 P:130304 P:195328 P:260352 P:325376 P:390400 P:455424 P:520448 P:585472 P:650496 P:715520 P:780544 P:845568 P:910592 P:975616 P:1040640 P:1105664 P:1170688 P:1235712 P:1300736 P:1365760 P:1430784 P:1495808 P:1560832 P:1625856 P:1690880 P:1755904 P:1820928 P:1885952 P:1950976 P:2016000 P:2081024 P:2146048 P:2211072 P:2276096 P:2341120 P:2406144 P:2471168 P:2536192 P:2601216 P:2666240 P:2731264 P:2796288 P:2861312 P:2926336 P:2991360 P:3056384 P:3121408 P:3186432 P:3251456 P:3316480 P:3381504 P:3446528 P:3511552 P:3576576 P:3641600 P:3706624 P:3771648 P:3836672 P:3901696 P:3966720 P:4031744 P:4096768 L:4194304 P:4161792 in=100+flush out=[256,4161800) total=4259304
fill_out_odd lat2 P:0 P:256 P:65280 P:130304 P:195328 P:260352 P:325376 P:390400 P:455424 P:520448 P:585472 P:650496 P:715520 P:780544 P:845568 P:910592 P:975616 P:1040640 P:1105664 P:1170688 P:1235712 P:1300736 P:1365760 P:1430784 P:1495808 P:1560832 P:1625856 P:1690880 P:1755904 P:1820928 P:1885952 P:1950976 P:2016000 P:2081024 P:2146048 P:2211072 P:2276096 P:2341120 P:2406144 P:2471168 P:2536192 P:2601216 P:2666240 P:2731264 P:2796288 P:2861312 P:2926336 P:2991360 P:3056384 P:3121408 P:3186432 P:3251456 P:3316480 P:3381504 P:3446528 P:3511552 P:3576576 P:3641600 P:3706624 P:3771648 P:3836672 P:3901696 P:3966720 P:4031744 P:4096768 L:4194304 P:4161792 in=100 out=[256,4161800) total=4259304
odds_and_ends thr L:4194304 W:0 W:256 L:4194304 L:4259841 L:4259841 W:4352 -:0 -:0 W:4608 L:4260096 W:4864 L:4261120 L:4331264 W:5120 in=4359+flush out=[4608,5136) total=4331267
odds_and_ends lat0 L:4194304 W:0 P:256 W:4352 L:4194304 L:4194304 W:70144 -:0 -:0 P:70400 L:4194304 P:70656 L:4195328 L:4265472 P:70912 in=70151+flush out=[70400,70928) total=4265475
odds_and_ends lat1 L:4194304 W:0 P:256 W:4352 L:4194304 L:4194304 W:70144 -:0 -:0 P:70400 L:4194304 P:70656 L:4195328 L:4265472 P:70912 in=70151+flush out=[70400,70928) total=4265475
odds_and_ends lat2 L:4194304 P:0 P:256 P:4352 L:4194304 L:4194304 P:70144 -:0 -:0 P:70400 L:4194304 P:70656 L:4195328 L:4265472 P:70912 in=70151 out=[70400,70928) total=4265475
odds_and_ends_resident thr L:4194304 W:0 W:256 L:4194304 L:4259841 L:4259841 W:4352 -:0 -:0 W:4608 L:4260096 W:4864 L:4261120 L:4331264 W:5120 in=4359+flush out=[4608,5136) total=4331267
odds_and_ends_resident lat0 L:4194304 W:0 P:256 W:4352 L:4194304 L:4194304 W:70144 -:0 -:0 P:70400 L:4194304 P:70656 L:4195328 L:4265472 P:70912 in=70151+flush out=[70400,70928) total=4265475
odds_and_ends_resident lat1 L:4194304 P:0 P:256 P:4352 L:4194304 L:4194304 P:70144 -:0 -:0 P:70400 L:4194304 P:70656 L:4195328 L:4265472 P:70912 in=70151 out=[70400,70928) total=4265475
odds_and_ends_resident lat2 L:4194304 P:0 P:256 P:4352 L:4194304 L:4194304 P:70144 -:0 -:0 P:70400 L:4194304 P:70656 L:4195328 L:4265472 P:70912 in=70151 out=[70400,70928) total=4265475
dense_b1 thr W:0 W:256 W:512 W:768 W:1024 W:1280 W:1536 W:1792 W:2048 W:2304 W:2560 W:2816 W:3840 W:4352 W:4608 -:0 -:0 in=1796+flush out=[2048,20992) total=4194304
dense_b1 lat0 W:0 W:256 W:512 W:768 W:1024 W:1280 W:1536 W:1792 P:2048 P:2304 P:2560 P:2816 P:3840 P:4352 P:4608 -:0 -:0 in=1796+flush out=[2048,20992) total=4194304
dense_b1 lat1 P:0 P:256 P:512 P:768 P:1024 P:1280 P:1536 P:1792 P:2048 P:2304 P:2560 P:2816 P:3840 P:4352 P:4608 -:0 -:0 in=1796 out=[2048,20992) total=4194304
dense_b1 lat2 P:0 P:256 P:512 P:768 P:1024 P:1280 P:1536 P:1792 P:2048 P:2304 P:2560 P:2816 P:3840 P:4352 P:4608 -:0 -:0 in=1796 out=[2048,20992) total=4194304
dense_b1_tables_travel thr W:0 W:256 W:512 W:768 W:1024 W:1280 W:1536 W:1792 W:2048 W:2304 W:3072 W:8448 W:40448 W:40704 W:40960 W:41216 W:41472 W:41728 W:42752 W:43264 W:43520 -:0 -:0 in=40708+flush out=[40960,59904) total=4194304
dense_b1_tables_travel lat0 W:0 W:256 W:512 W:768 W:1024 W:1280 W:1536 W:1792 W:2048 W:2304 W:3072 W:8448 W:40448 W:40704 P:40960 P:41216 P:41472 P:41728 P:42752 P:43264 P:43520 -:0 -:0 in=40708+flush out=[40960,59904) total=4194304
dense_b1_tables_travel lat1 W:0 W:256 W:512 W:768 W:1024 W:1280 W:1536 W:1792 W:2048 W:2304 W:3072 W:8448 W:40448 W:40704 P:40960 P:41216 P:41472 P:41728 P:42752 P:43264 P:43520 -:0 -:0 in=40708+flush out=[40960,59904) total=4194304
dense_b1_tables_travel lat2 P:0 P:256 P:512 P:768 P:1024 P:1280 P:1536 P:1792 P:2048 P:2304 P:3072 P:8448 P:40448 P:40704 P:40960 P:41216 P:41472 P:41728 P:42752 P:43264 P:43520 -:0 -:0 in=40708 out=[40960,59904) total=4194304
fiss_b1 thr W:0 W:256 W:512 W:768 W:1024 W:1280 W:1536 W:1792 W:2048 W:2304 W:2560 W:2816 W:3072 W:3328 W:3584 W:3840 W:4096 W:4352 W:5120 W:5376 in=2828+flush out=[3072,21760) total=4194304
fiss_b1 lat0 W:0 W:256 W:512 W:768 W:1024 W:1280 W:1536 W:1792 W:2048 W:2304 W:2560 P:2816 P:3072 P:3328 P:3584 P:3840 P:4096 P:4352 P:5120 P:5376 in=2828+flush out=[3072,21760) total=4194304
fiss_b1 lat1 P:0 P:256 P:512 P:768 P:1024 P:1280 P:1536 P:1792 P:2048 P:2304 P:2560 P:2816 P:3072 P:3328 P:3584 P:3840 P:4096 P:4352 P:5120 P:5376 in=2828 out=[3072,21760) total=4194304
fiss_b1 lat2 P:0 P:256 P:512 P:768 P:1024 P:1280 P:1536 P:1792 P:2048 P:2304 P:2560 P:2816 P:3072 P:3328 P:3584 P:3840 P:4096 P:4352 P:5120 P:5376 in=2828 out=[3072,21760) total=4194304
fiss_b1_inline thr L:4194304 W:0 W:256 W:512 W:768 W:1024 W:1280 W:1536 W:2304 W:2560 in=12+flush out=[256,18944) total=4195328
fiss_b1_inline lat0 L:4194304 P:0 P:256 P:512 P:768 P:1024 P:1280 P:1536 P:2304 P:2560 in=12 out=[256,18944) total=4195328
fiss_b1_inline lat1 L:4194304 P:0 P:256 P:512 P:768 P:1024 P:1280 P:1536 P:2304 P:2560 in=12 out=[256,18944) total=4195328
fiss_b1_inline lat2 L:4194304 P:0 P:256 P:512 P:768 P:1024 P:1280 P:1536 P:2304 P:2560 in=12 out=[256,18944) total=4195328
fiss_b1_tables_travel thr W:0 W:256 W:512 W:768 W:1024 W:1280 W:1536 W:1792 W:2048 W:2304 W:3072 W:8448 W:40448 W:40704 W:40960 W:41216 W:41472 W:41728 W:41984 W:42240 W:42496 W:42752 W:43008 W:43264 W:44032 W:44288 in=41740+flush out=[41984,60672) total=4194304
fiss_b1_tables_travel lat0 W:0 W:256 W:512 W:768 W:1024 W:1280 W:1536 W:1792 W:2048 W:2304 W:3072 W:8448 W:40448 W:40704 W:40960 W:41216 W:41472 P:41728 P:41984 P:42240 P:42496 P:42752 P:43008 P:43264 P:44032 P:44288 in=41740+flush out=[41984,60672) total=4194304
fiss_b1_tables_travel lat1 W:0 W:256 W:512 W:768 W:1024 W:1280 W:1536 W:1792 W:2048 W:2304 W:3072 W:8448 W:40448 W:40704 W:40960 W:41216 W:41472 P:41728 P:41984 P:42240 P:42496 P:42752 P:43008 P:43264 P:44032 P:44288 in=41740+flush out=[41984,60672) total=4194304
fiss_b1_tables_travel lat2 P:0 P:256 P:512 P:768 P:1024 P:1280 P:1536 P:1792 P:2048 P:2304 P:3072 P:8448 P:40448 P:40704 P:40960 P:41216 P:41472 P:41728 P:41984 P:42240 P:42496 P:42752 P:43008 P:43264 P:44032 P:44288 in=41740 out=[41984,60672) total=4194304
"""


def _hipcc():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stage_plan")
    src = tmp / "stage_driver.hip"
    src.write_text(DRIVER)
    exe = tmp / "stage_driver"
    subprocess.check_call([_hipcc(), "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", CSRC, "-o", str(exe), str(src)])
    return str(exe)


def _rows(driver, cases):
    text = "".join(f"{name} {flag} {ops}\n" for name, flag, ops in cases)
    return subprocess.check_output([driver], input=text, text=True).splitlines()


def test_stage_plans_match_the_table(driver):
    got = _rows(driver, CASES)
    want = EXPECTED.strip().splitlines()
    assert [tuple(l.split()[:2]) for l in got] == [(c[0], r) for c in CASES for r in REGIMES]
    for g, w in zip(got, want):
        assert g == w, (g, w)
    assert len(got) == len(want)


def _parse(row, ops):
    tok = row.split()
    items = []
    for t, op in zip(tok[2:2 + len(ops)], ops):
        kind, nbytes = op.split(":")
        region, off = t.split(":")
        items.append((kind, int(nbytes), region, int(off)))
    tail = dict(t.split("=") for t in tok[2 + len(ops):])
    lo, hi = (int(v) for v in tail["out"].strip("[)").split(","))
    return items, int(tail["in"].split("+")[0]), tail["in"].endswith("+flush"), lo, hi, int(tail["total"])


def test_stage_plan_invariants(driver):
    """Recomputed from the printed rows: alignment, no overlap within a region, everything inside the total, inputs before outputs in the
    small window, the zero-copy limit, the window's size.  (An input of zero bytes is not placed - it gets the large region's cursor as
    it stands, "any valid address", which follows an array of any length: it has no extent to align or to overlap.)"""
    rows = _rows(driver, CASES)
    assert len(rows) == len(CASES) * len(REGIMES)
    for k, row in enumerate(rows):
        name, flag, spec = CASES[k // len(REGIMES)]
        regime = REGIMES[k % len(REGIMES)]
        assert "OUTSIDE" not in row, row
        ops = spec.split()
        items, small_in, flush, lo, hi, total = _parse(row, ops)
        assert len(items) == len(ops)
        zero_copy_in = regime == "lat2" or (regime == "lat1" and flag == "resident")
        spans = {"small": [], "L": []}
        for kind, nbytes, region, off in items:
            if region == "-":
                assert kind in ("null", "out") and (kind == "null" or nbytes == 0), row
                continue
            if nbytes == 0 and kind in ("in", "mut"):
                assert region == "L" and SMALL_REGION <= off <= total, row
                continue
            assert off % ALIGN == 0, row
            if region == "L":
                assert off >= SMALL_REGION and off + nbytes <= total, row
                spans["L"].append((off, off + nbytes))
            else:  # the pinned block and the window are the same offsets of two mirrors: one address space
                assert off + nbytes <= SMALL_REGION and off + nbytes <= total, row
                spans["small"].append((off, off + nbytes))
                if kind in ("in", "mut"):
                    assert off + nbytes <= small_in <= lo, row
                else:
                    assert lo <= off and off + nbytes <= hi, row
                if kind == "in" and region == "P":
                    assert zero_copy_in and off + nbytes <= ZC_IN_MAX, row
                if kind == "in" and region == "W":
                    assert not zero_copy_in and flush and nbytes <= (SMALL_MAX if regime == "thr" else ZC_IN_MAX), row
                if kind == "out":
                    assert nbytes <= SMALL_MAX and region == ("W" if regime == "thr" else "P"), row
                if kind == "mut" and region == "P":
                    assert regime != "thr" and (nbytes <= SMALL_MAX or (zero_copy_in and off + nbytes <= ZC_IN_MAX)), row
            assert kind != "temp" or region == "L", row
        for name_, s in spans.items():
            s.sort()
            for (a0, a1), (b0, b1) in zip(s, s[1:]):
                assert a1 <= b0, (name_, row)
        assert lo % ALIGN == 0 and small_in <= lo <= hi <= SMALL_REGION and total >= SMALL_REGION, row
        if zero_copy_in:
            assert not flush, row


def test_stage_list_overflow_is_reported(driver):
    rows = _rows(driver, [("fits", "-", " ".join(["in:8"] * STAGE_CAP)), ("too_long", "-", " ".join(["in:8"] * (STAGE_CAP + 1)))])
    assert len(rows) == len(REGIMES) + 1 and rows[0].startswith("fits thr") and rows[-1] == f"too_long overflow n={STAGE_CAP + 1}"


_ODDS = next(ops for name, _, ops in CASES if name == "odds_and_ends")


def test_pass_through_list_hands_the_addresses_on(driver):
    """A pass-through list (an FP_MEM_DEVICE call) over the odds_and_ends sequence: every in / mut / out stores the address it was given,
    whatever its length; the output nobody asked for and every temp store NULL; nothing is recorded."""
    row, = _rows(driver, [("odds", "through", _ODDS)])
    want = ["0" if op.split(":")[0] in ("null", "temp") else "=" for op in _ODDS.split()]
    assert want.count("0") == 3 and row.split() == ["odds", "through"] + want + ["n=0", "overflow=0"]


def test_pass_through_list_never_overflows(driver):
    row, = _rows(driver, [("long", "through", " ".join([_ODDS] * 6))])
    tok = row.split()
    assert len(tok) - 4 == 6 * len(_ODDS.split()) > STAGE_CAP and "?" not in tok[2:-2] and tok[-2:] == ["n=0", "overflow=0"]
