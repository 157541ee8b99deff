"""CPU: plan_lattice (fiss_plus_planner_amd/csrc/frenet_lattice_plan.h), the host function that decides every launch of the fused
lattice kernel, printed for a fixed list of cases by a small host program and compared with the table below.

The rows are the decisions the launcher made before the plan was one function.  One rule changed: a launch that comes out windowed
(long reference lines at three or four per CU) is planned as if the appended FISS+ search had not been offered, where the search used
to be dropped only after it could have raised the LDS size or kept the launch from four per CU.  No row differs even so (knots*_fissplus):
the search's LDS - at most ~35 KB for 1024 samples - stays below a quarter of the CU and below a windowed layout, which fills its share."""
import os
import shutil
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "fiss_plus_planner_amd", "csrc")

# name: settings on top of BASELINE.json configs[2] (2048 egos, 9 x 9 x 7, 50 obstacles over 5 s, 81-knot lines, a 256-CU device)
# flags: series (r.best_traj), epi (epilogue workgroups offered), tables (cost / flag tables), search (FISS+ search offered),
# parts (partial-argmin scratch), skip (closed-loop batch), loop (hand-over offered), inl (inline inputs), poly (polygon columns)
CASES = [
    ("c2", ""),
    ("c2_series", "series"),
    ("c2_series_epi", "series epi"),
    ("c2_tables", "tables"),
    ("c2_tail", "parts tail=-256"),
    ("c2_step_series", "series loop"),
    ("c3_fissplus", "tables search parts tail=-256"),
    ("c3_fissplus_short", "tables search B=1024"),
    ("c1_555", "B=256 nd=5 nv=5 nt=5 obs=10 T_obs=100"),
    ("c1_555_many", "B=1024 nd=5 nv=5 nt=5 obs=10 T_obs=100"),
    ("c1_555_series", "B=1024 nd=5 nv=5 nt=5 obs=10 T_obs=100 series"),
    ("c4_shard", "B=2048 series epi parts tail=-256"),
    ("c4_shard_big", "B=16384 tables"),
    ("loop_skip", "skip loop"),
    ("loop_skip_occ4", "skip loop occ=4"),
    ("loop_skip_series", "skip loop series"),
    ("occ2", "occ=2"),
    ("occ3", "occ=3"),
    ("occ4", "occ=4"),
    ("multi_round_small_device", "B=300 res2=64 parts tail=-32"),
    ("multi_round_small_device_four", "B=300 res2=64 nd=5 nv=5 nt=5 obs=10"),
    ("lds_cu_64", "lds_kb=64"),
    ("inline", "B=4 inl series"),
    ("inline_too_big", "B=4 inl NX=1024 obs=500"),
    ("latency_split", "B=8 parts nsplit=7"),
    ("latency_split_clamped", "B=8 parts nsplit=9"),
    ("grouped", "B=256 nd=5 nv=5 nt=5 obs=10 T_obs=100 group=5"),
    ("grouped_997", "B=256 group=7"),
    ("grouped_runtime", "B=256 nd=5 nv=5 nt=5 obs=12 T_obs=100 group=5"),
    # lattice_group = 99 takes the 1024-thread instance while two slices' lon profiles number at most 256 (nv = 128 against 129, as in
    # tests/test_gpu_edges.py) and that instance's layout fits a workgroup's LDS
    ("grouped_nv128", "B=2 nd=3 nv=128 nt=4 obs=8 group=99"),
    ("grouped_nv129", "B=2 nd=3 nv=129 nt=4 obs=8 group=99"),
    ("grouped_lds", "B=256 NX=1250 group=99"),
    ("no_obstacles", "obs=0 S=0"),
    ("no_obstacles_tail", "obs=0 S=0 parts tail=-256"),
    ("knots200", "NX=200"),
    ("knots400", "NX=400"),
    ("knots1000", "NX=1000"),
    ("knots200_fissplus", "NX=200 tables search"),
    ("knots400_fissplus", "NX=400 tables search"),
    ("knots1000_fissplus", "NX=1000 tables search"),
    ("knots200_fissplus_c972", "NX=200 nt=12 tables search"),
    ("knots400_fissplus_c972", "NX=400 nt=12 tables search"),
    ("fissplus_c972", "nt=12 tables search"),
    ("knots200_series_epi", "NX=200 series epi"),
    ("poly_short", "poly pstride=8"),
    ("poly_short_few", "poly pstride=8 B=256"),
    ("poly_long", "poly pstride=8 NX=400"),
    ("poly_grouped", "poly pstride=8 B=256 nd=5 nv=5 nt=5 obs=10 T_obs=100 group=5"),
    ("poly_fissplus", "poly pstride=8 tables search"),
    ("runtime_shape", "nd=7 nv=7 nt=6 obs=20"),
    ("long_horizon", "pmax=256 T_obs=100"),
    ("nofit_nd65", "nd=65 nv=2 nt=2"),
    ("nofit_nobs4096", "obs=4096 T_obs=2"),
    ("nofit_nobs4095_lds", "obs=4095 T_obs=2"),
    ("nofit_rows_x_obs", "obs=3000"),
    # the lattice launch under the clearance term in tests/clearance_cases.py (24 egos on a modelled one-CU device: resident_groups = 2)
    ("clearance_config2", "B=24 res2=2 nd=5 nv=5 nt=5 obs=10 T_obs=100 tables parts tail=-1"),
    ("clearance_short_table", "B=24 res2=2 nd=5 nv=5 nt=5 obs=10 T_obs=50 tables parts tail=-1"),
    ("clearance_short_table_occ3", "B=24 res2=2 nd=5 nv=5 nt=5 obs=10 T_obs=50 occ=3 tables parts tail=-1"),
    ("clearance_knots220", "B=24 res2=2 nd=5 nv=5 nt=5 obs=10 T_obs=50 NX=220 tables parts tail=-1"),
    ("clearance_knots400_occ3", "B=24 res2=2 nd=5 nv=5 nt=5 obs=10 T_obs=50 NX=400 occ=3 tables parts tail=-1"),
]

FLAGS = {
    "series": "ka.r.best_traj = (double*)kDummy;",
    "epi": "ka.epi_flag = (int32_t*)kDummy; ka.idx_shadow = (int32_t*)kDummy;",
    "tables": "ka.r.cost_tbl = (double*)kDummy; ka.r.flag_tbl = (uint32_t*)kDummy;",
    "search": "rq.ft = &ft;",
    "parts": "rq.part_scratch = kDummy;",
    "skip": "ka.b.skip = (const int32_t*)kDummy;",
    "loop": "ka.has_loop = 1;",
    "inl": "rq.inl = &inl;",
    "poly": "ka.b.obs_nvert = (const int32_t*)kDummy;",
}
FIELDS = {"B": "ka.b.B", "S": "ka.b.S", "NX": "ka.b.NX", "obs": "ka.b.n_obs", "T_obs": "ka.b.T_obs", "pstride": "ka.b.poly_stride",
          "nd": "ka.p.nd", "nv": "ka.p.nv", "nt": "ka.p.nt", "pmax": "ka.p.points_max", "occ": "ka.occ_cap", "res2": "ka.resident2",
          "lds_kb": "ka.lds_cu_kb", "nsplit": "rq.nsplit", "group": "rq.group", "tail": "rq.tail"}

DRIVER = r"""
#include <cstdio>
#include "frenet_lattice_plan.h"
using namespace fp;
static void* const kDummy = (void*)0x1000;
static const char* kFamily[] = {"plain", "grouped", "poly", "poly+grouped", "search", "window", "poly+window"};
static const char* kShape[] = {"rt", "997", "555"};
static void show(const char* name, const KernelArgs& ka, const LatticeRequest& rq)
{
    const LatticePlan pl = plan_lattice(ka, rq);
    if (!pl.fits) { std::printf("%s nofit\n", name); return; }
    const LatticeKey& k = kLatticeInstances[pl.instance];
    std::printf("%s %s/%d/%s rows=%d hp=%d gs=%d nsplit=%d wcap=%d epi=%d search=%d series=%d tail_from=%d epi_from=%d grid=%u lds=%d threads=%d\n",
                name, kFamily[k.family], k.per_cu, kShape[k.shape], pl.rows, pl.hp, pl.gs, pl.nsplit, pl.wcap, pl.epilogue, pl.search, pl.series,
                pl.tail_from, pl.epi_from, pl.grid, pl.lds, pl.threads);
}
int main()
{
    FissTail ft;
    ft.flag = (int32_t*)kDummy;
    ft.opts.kind = FP_FISS_PLUS;
    static InlineIn inl;
    inl.on = 1;
"""


def _driver_source():
    lines = [DRIVER]
    for name, spec in CASES:
        body = ["KernelArgs ka{}; LatticeRequest rq;", "ka.p.nd = 9; ka.p.nv = 9; ka.p.nt = 7; ka.p.check_stride = 2;",
                "ka.b.B = 2048; ka.b.S = 2048; ka.b.NX = 81; ka.b.n_obs = 50; ka.b.T_obs = 50; ka.resident2 = 512; ka.lds_cu_kb = 160;"]
        for tok in spec.split():
            if "=" in tok:
                k, v = tok.split("=")
                body.append(f"{FIELDS[k]} = {int(v)};")
            else:
                body.append(FLAGS[tok])
        lines.append("    { " + " ".join(body) + f' show("{name}", ka, rq); }}')
    lines.append("    return 0;\n}\n")
    return "\n".join(lines)


EXPECTED = """
c2 plain/4/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=40288 threads=512
c2_series plain/2/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=1 tail_from=-1 epi_from=-1 grid=2048 lds=52384 threads=512
c2_series_epi plain/4/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=1 search=0 series=1 tail_from=-1 epi_from=2048 grid=2560 lds=40288 threads=512
c2_tables plain/4/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=40288 threads=512
c2_tail plain/4/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=1920 epi_from=-1 grid=2176 lds=40288 threads=512
c2_step_series plain/2/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=1 tail_from=-1 epi_from=-1 grid=2048 lds=52384 threads=512
c3_fissplus search/4/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=1 series=0 tail_from=1920 epi_from=2176 grid=4224 lds=40288 threads=512
c3_fissplus_short search/4/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=1 series=0 tail_from=-1 epi_from=1024 grid=2048 lds=40288 threads=512
c1_555 plain/2/555 rows=50 hp=101 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=256 lds=63056 threads=512
c1_555_many plain/2/555 rows=50 hp=101 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=1024 lds=63056 threads=512
c1_555_series plain/2/555 rows=50 hp=101 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=1 tail_from=-1 epi_from=-1 grid=1024 lds=63056 threads=512
c4_shard plain/4/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=1 search=0 series=1 tail_from=1920 epi_from=2176 grid=2688 lds=40288 threads=512
c4_shard_big plain/4/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=16384 lds=40288 threads=512
loop_skip plain/3/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=45856 threads=512
loop_skip_occ4 plain/4/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=40288 threads=512
loop_skip_series plain/2/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=1 tail_from=-1 epi_from=-1 grid=2048 lds=52384 threads=512
occ2 plain/2/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=52384 threads=512
occ3 plain/3/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=45856 threads=512
occ4 plain/4/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=40288 threads=512
multi_round_small_device plain/4/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=284 epi_from=-1 grid=316 lds=40288 threads=512
multi_round_small_device_four plain/4/rt rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=300 lds=34880 threads=512
lds_cu_64 plain/2/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=52384 threads=512
inline plain/2/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=1 tail_from=-1 epi_from=-1 grid=4 lds=52384 threads=512
inline_too_big plain/2/rt rows=25 hp=51 gs=1 nsplit=1 wcap=1024 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=4 lds=138448 threads=512
latency_split plain/2/997 rows=25 hp=51 gs=1 nsplit=7 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=56 lds=52384 threads=512
latency_split_clamped plain/2/997 rows=25 hp=51 gs=1 nsplit=7 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=56 lds=52384 threads=512
grouped grouped/2/555 rows=50 hp=101 gs=5 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=256 lds=92560 threads=1024
grouped_997 grouped/2/997 rows=25 hp=51 gs=7 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=256 lds=68288 threads=1024
grouped_runtime grouped/2/rt rows=50 hp=101 gs=5 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=256 lds=92624 threads=1024
grouped_nv128 grouped/2/rt rows=25 hp=51 gs=2 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2 lds=89216 threads=1024
grouped_nv129 plain/2/rt rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2 lds=73536 threads=512
grouped_lds plain/2/997 rows=25 hp=51 gs=1 nsplit=1 wcap=1250 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=256 lds=141216 threads=512
no_obstacles plain/4/rt rows=0 hp=0 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=23056 threads=512
no_obstacles_tail plain/4/rt rows=0 hp=0 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=23056 threads=512
knots200 window/4/997 rows=25 hp=51 gs=1 nsplit=1 wcap=61 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=40432 threads=512
knots400 window/3/997 rows=25 hp=51 gs=1 nsplit=1 wcap=136 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=53200 threads=512
knots1000 plain/2/997 rows=25 hp=51 gs=1 nsplit=1 wcap=1000 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=122224 threads=512
knots200_fissplus window/4/997 rows=25 hp=51 gs=1 nsplit=1 wcap=61 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=40432 threads=512
knots400_fissplus window/3/997 rows=25 hp=51 gs=1 nsplit=1 wcap=136 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=53200 threads=512
knots1000_fissplus plain/2/997 rows=25 hp=51 gs=1 nsplit=1 wcap=1000 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=122224 threads=512
knots200_fissplus_c972 window/3/rt rows=25 hp=51 gs=1 nsplit=1 wcap=69 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=53216 threads=512
knots400_fissplus_c972 plain/2/rt rows=25 hp=51 gs=1 nsplit=1 wcap=400 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=83328 threads=512
fissplus_c972 search/3/rt rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=1 series=0 tail_from=-1 epi_from=2048 grid=4096 lds=52560 threads=512
knots200_series_epi window/4/997 rows=25 hp=51 gs=1 nsplit=1 wcap=61 epi=1 search=0 series=1 tail_from=-1 epi_from=2048 grid=2560 lds=40432 threads=512
poly_short poly/3/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=46064 threads=512
poly_short_few poly/2/rt rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=256 lds=52592 threads=512
poly_long poly+window/3/997 rows=25 hp=51 gs=1 nsplit=1 wcap=133 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=53216 threads=512
poly_grouped poly+grouped/2/rt rows=50 hp=101 gs=5 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=256 lds=93888 threads=1024
poly_fissplus poly/3/997 rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=46064 threads=512
runtime_shape plain/4/rt rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=37104 threads=512
long_horizon plain/2/rt rows=50 hp=101 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=2048 lds=69968 threads=512
nofit_nd65 nofit
nofit_nobs4096 nofit
nofit_nobs4095_lds nofit
nofit_rows_x_obs nofit
clearance_config2 plain/2/555 rows=50 hp=101 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=24 lds=63056 threads=512
clearance_short_table plain/4/rt rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=24 lds=34880 threads=512
clearance_short_table_occ3 plain/3/rt rows=25 hp=51 gs=1 nsplit=1 wcap=81 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=24 lds=39712 threads=512
clearance_knots220 window/4/rt rows=25 hp=51 gs=1 nsplit=1 wcap=141 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=24 lds=40384 threads=512
clearance_knots400_occ3 window/3/rt rows=25 hp=51 gs=1 nsplit=1 wcap=232 epi=0 search=0 series=0 tail_from=-1 epi_from=-1 grid=24 lds=53200 threads=512
"""


def _hipcc():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_lattice_plans_match_the_table(tmp_path):
    src = tmp_path / "plan_driver.hip"
    src.write_text(_driver_source())
    exe = tmp_path / "plan_driver"
    subprocess.check_call([_hipcc(), "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", CSRC, "-o", str(exe), str(src)])
    got = subprocess.check_output([str(exe)], text=True).splitlines()
    want = EXPECTED.strip().splitlines()
    assert [l.split()[0] for l in got] == [c[0] for c in CASES]
    for g, w in zip(got, want):
        assert g == w, (g, w)
    assert len(got) == len(want)
