#!/usr/bin/env python3
"""Executed VALU instructions per ego of one lattice_fused_kernel instance, estimated section by section, beside the counter.

  python tools/nonwalk_census.py <file.s> <instance key> [--src FILE] [shape and work options] [--counter SQ_INSTS_VALU --egos B]

<file.s> and the key are what tools/isa_lines.py takes (a -gline-tables-only -S build; the template arguments as they stand in the
mangled name).  For every `// [section NAME]` of the source the static VALU count of the section is multiplied by how many wavefronts
execute it and how often - a closed form in the shape (nd, nv, nt, rows, n_obs, nx, hp, threads) and in the means of
tools/work_counters.py (survivors of G, B rounds, N rounds) that is printed beside the number.  The walk and the tail split's second
prologue are added, and the total stands beside SQ_INSTS_VALU / egos of a counter run of the same build (`rocprofv3 --pmc
SQ_INSTS_VALU` in a run of its own on `bench.py --steps 3 --warmup 1`) with the remainder it does not explain: the appended series
workgroups are not modelled and are part of that remainder, and so is whatever code a source without the whole-kernel marks (below)
leaves outside its sections.

What the model is and is not.  A section's static count is taken as ONE execution of it by a wavefront that does its work; a loop
inside a section counts once (the bisection of LUT and the end-speed loop of RANGES carry their trip counts below, as a factor on
the whole section - an over-estimate of their headers; --unrolled names the sections whose loop the compiler unrolled, so that the
static count is every trip already: RANGES wherever nv is a template argument).  A wavefront that only tests and skips a section is charged SKIP
instructions when the test is a vector compare, none when it is scalar (--scalar-skip names those sections: the kCut instances
enter LUT's divisions, the square root of `r_ego`, the cost sums, the ends of d_samples and of v_samples (VENDS) and the one-wavefront
argmin on a scalar test).  --two-ends names the sections that have the form of the instances with the two-profile RANGES and the
one-wavefront ARGMIN: RANGES then has no end-speed loop, ARGMIN runs once and only its store (--uniform ARGMIN=9) on every wavefront.  MASKS runs only for slices with an
unproven profile (0.05 of 7 on the headline workload) and is charged its share.  --whole is the share of the egos stage W ends with no
table requested: they skip ASM and ARGMIN and are not charged them (WEXIT, the mask read behind the walk, is charged to every ego).

The whole kernel is weighed when the source carries the marks for it: ENTRY (slot decode, the ego's scalars), GLUE (what stands between
the prologue's sections), WSETUP (the block in front of the profile loop) and POSTWALK on all wavefronts; the profile loop's own
statements (PQ, PQDEC, PQFETCH, PQPTR, PQEND) once per lon profile, S and ROUNDS (the sure-hit stage and its loop) once per S round
(--s-rounds), FRAMES once per profile that entered the walk
(--walked: stage V skips the others at the loop's head), PREP once per walked profile that S did not end (--s-ended), ROUNDB once per B round, ROUNDN once per N round (--fold-trips: the
trips of the loop that folds a round's hits onto the lateral samples, two vector instructions each in the builds that have the loop -
a static count holds one); SKIPPED (an ego that is finished: none in the headline), SERIES (two per CU only) and APPSEARCH are not
executed by a lattice workgroup of the headline and count 0; APPSERIES (the appended series workgroups, two wavefronts per ego on
paths that depend on what they find) is printed with its static count and left in the remainder.  A source without those marks gets
the earlier model: 28 instructions per profile for everything outside the walk's sections.  The `spill` column is the section's lane
operations on spilled SGPRs (tools/isa_lines.py), weighed like the section.
"""
import argparse
import math
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("path")
ap.add_argument("key")
ap.add_argument("--src")
for name, default in (("nd", 9), ("nv", 9), ("nt", 7), ("rows", 25), ("n_obs", 50), ("nx", 81), ("stride", 2), ("threads", 512), ("flight", 3)):
    ap.add_argument("--" + name, type=int, default=default)
ap.add_argument("--surv", type=float, default=65.2, help="work_counters: G survivors per ego")
ap.add_argument("--b-rounds", type=float, default=62.9)
ap.add_argument("--n-rounds", type=float, default=59.8)
ap.add_argument("--s-rounds", type=float, default=0.0, help="work_counters: rounds of stage S per ego (sections S + ROUNDS run once per round)")
ap.add_argument("--s-ended", type=float, default=0.0, help="work_counters: lon profiles per ego that stage S ended (they skip PREP; their B and N rounds are not in the counters)")
ap.add_argument("--walked", type=float, help="work_counters: lon profiles per ego that entered the walk (stage V skips the others at the loop's head, "
                "where they pay the loop's own statements but no FRAMES); default: all nt nv")
ap.add_argument("--whole", type=float, default=0.0, help="work_counters: share of the egos stage W ended with no table requested (every collision mask full behind the walk): "
                "they are not charged ASM and ARGMIN; WEXIT itself - the mask read - runs on every wavefront of every ego")
ap.add_argument("--scan-slices", type=float, default=0.05, help="work_counters: slices that needed the mask scan")
ap.add_argument("--tail", type=float, default=128 / 2048, help="share of the egos the tail split runs as two workgroups")
ap.add_argument("--scalar-skip", default="", help="comma list of sections whose idle wavefronts skip on a scalar test (the kCut instances: LUT,SUMS)")
ap.add_argument("--uniform", default="", help="NAME=count[@wavefronts],...: instructions of a section that are no part of its dealt work and run once on that many wavefronts, "
                "all by default (parent: FAN=38,LUT=28 - the ends of d_samples, the bucket width's divisions; kCut instances: LUT=28@3)")
ap.add_argument("--two-ends", default="", help="comma list of RANGES, ARGMIN: the section has the form of the instances that take the row ranges from the two extreme end "
                "speeds (no end-speed loop: one trip per lane) / reduce the argmin on one wavefront (the store of every lane's candidate stays on all: --uniform ARGMIN=9)")
ap.add_argument("--unrolled", default="", help="comma list of sections whose inner loop the compiler unrolled (the static count holds every trip already): RANGES in the shaped "
                "instances, where nv is a constant - the counter showed it: taking seven of nine evaluations out removed 0.2 k per ego, not 1.0 k")
ap.add_argument("--fold-trips", type=float, default=1.0, help="mean trips per N round of the loop that folds the round's hits (builds that have the loop; 1: as the static count has it)")
ap.add_argument("--counter", type=float, help="SQ_INSTS_VALU per launch")
ap.add_argument("--egos", type=int, default=2048)
a = ap.parse_args()

cmd = [sys.executable, os.path.join(HERE, "isa_lines.py"), a.path, a.key] + (["--src", a.src] if a.src else [])
out = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
static, spill = {}, {}
for line in out.splitlines():
    m = re.match(r"\s*(\w+)@\d+\s+(\d+)((?:\s+\d+)+)", line)
    if m:
        static[m.group(1)] = static.get(m.group(1), 0) + int(m.group(2))
        spill[m.group(1)] = spill.get(m.group(1), 0) + int(m.group(3).split()[5])  # (columns: f64 f32 int movsel lane spill ...)
    m = re.match(r"\s*kernel\s+(\d+)", line)
    if m:
        kernel_total = int(m.group(1))

W = a.threads // 64
v = dict(W=W, nd=a.nd, nv=a.nv, nt=a.nt, rows=a.rows, n_obs=a.n_obs, nx=a.nx, hp=a.rows * a.stride + 1, C=a.nd * a.nv * a.nt, surv=a.surv,
         flight=a.flight, threads=a.threads, ceil=math.ceil, log2=math.log2, scan=a.scan_slices, whole=a.whole)
SKIP = 4  # a vector compare, the EXEC save / restore moves around a section a wavefront has no lane in
scalar = set(filter(None, a.scalar_skip.split(",")))
two_ends = set(filter(None, a.two_ends.split(",")))
unrolled = set(filter(None, a.unrolled.split(",")))
uniform = {k: (int(c.split("@")[0]), int(c.split("@")[1]) if "@" in c else W) for k, c in (kv.split("=") for kv in filter(None, a.uniform.split(",")))}
# section -> (wavefronts x trips that execute it, as a formula of the shape)
WEIGHT = {
    "ENTRY": "W",
    "SKIPPED": "0",
    "STAGE": "W",
    "GLUE": "W",
    "LUT": "ceil((2 * nx + 1) / 64) * ceil(log2(nx)) / 2",   # (half of the section is the bisection's body)
    "VBOUND": "ceil((nx - 1) / 64)",
    "SOLVE": "ceil(nt * nv / 64)",
    "DALL": "ceil(nt * nd / 64)",
    "POWS": "1",
    "VENDS": "1",
    "RANGES": "ceil(nt * rows / 64) * (1 + (nv - 1) / 4)" if "RANGES" not in two_ends | unrolled else "ceil(nt * rows / 64)",   # (a quarter of the section is the end-speed loop's body; two ends, unrolled: no loop)
    "MASKS": "W * scan / nt",
    "SUMS": "ceil(nt * nv / 64) + ceil(nt * nd / 64)" if "SUMS" not in scalar else "1",   # (both branches in each; dealt by kind: each wavefront one of them)
    "QLAT": "ceil(nt * nd / 64)",
    "FAN": "ceil(nt * hp / 64)",
    "CIRCLES": "ceil(rows / 64)",
    "G": "W * ceil(rows * n_obs / (flight * threads))",
    "SINCOS": "ceil(surv / 64)",
    "WSETUP": "W",
    "POSTWALK": "W",
    "WEXIT": "W",
    "ASM": "ceil(C / 64) * (1 - whole)",
    "ARGMIN": "W * (1 - whole)" if "ARGMIN" not in two_ends else "1 - whole",
    "RESULTS": "1",
    "SERIES": "0",
    "APPSEARCH": "0",
}
rows_out, total, total_spill = [], 0.0, 0.0
for name, formula in WEIGHT.items():
    if name not in static:
        continue
    w = eval(formula, {}, v)
    w_all = eval(formula, {}, {**v, "whole": 0.0})  # (the wavefronts that hold the section's work in an ego W does not end)
    idle = max(0.0, W - min(W, math.ceil(w_all))) if name not in ("MASKS", "SKIPPED", "SERIES", "APPSEARCH") else 0.0
    uni, uni_w = uniform.get(name, (0, W))
    n = (static[name] - uni) * w + uni * uni_w * ((1 - a.whole) if name in ("ASM", "ARGMIN") else 1) + (0 if name in scalar else SKIP * idle)
    rows_out.append((name, static[name], spill[name], spill[name] * w, f"{formula}" + (f"; {uni} of them once on {uni_w} wavefronts" if uni else "") + ("" if name in scalar or not idle else f"; + {SKIP} x {idle:.0f} idle"), n))
    total += n
    total_spill += spill[name] * w
walk_profile = static.get("FRAMES", 0)
# the walk: per profile the loop's own statements (what lies between the sections of the pq loop) + FRAMES + PREP; per round B / N and their glue
marked = "PQ" in static
HDR = ("PQ", "PQDEC", "PQFETCH", "PQPTR", "PQEND")
hdr = sum(static.get(k, 0) for k in HDR) if marked else 28
rb, rn = static.get("ROUNDB", 0), static.get("ROUNDN", 0)
fold = 2 * (a.fold_trips - 1) * a.n_rounds
rs = static.get("S", 0) + static.get("ROUNDS", 0)
walked = a.walked if a.walked is not None else a.nt * a.nv
prep_profiles = walked - a.s_ended  # (PREP, B and N run for the profiles neither V nor S ended)
walk = a.nt * a.nv * hdr + walked * walk_profile + prep_profiles * static.get("PREP", 0) + a.s_rounds * rs + a.b_rounds * (static.get("B", 0) + rb) + a.n_rounds * (static.get("N", 0) + rn) + fold
walk_spill = a.nt * a.nv * sum(spill.get(k, 0) for k in HDR) + walked * spill.get("FRAMES", 0) + prep_profiles * spill.get("PREP", 0) + a.s_rounds * (spill.get("S", 0) + spill.get("ROUNDS", 0)) + a.b_rounds * (spill.get("B", 0) + spill.get("ROUNDB", 0)) + a.n_rounds * (spill.get("N", 0) + spill.get("ROUNDN", 0))
outside = kernel_total - sum(static.values())
print(f"{'section':10s} {'static':>7s} {'executed':>9s} {'spill':>6s} {'executed':>9s}  wavefronts x trips")
for name, s, sp, spn, f, n in rows_out:
    print(f"{name:10s} {s:7d} {n:9.0f} {sp:6d} {spn:9.0f}  {f}")
print(f"{'outside the walk, sections':52s} {total:9.0f}   (lane operations on spilled SGPRs among them: {total_spill:.0f})")
print(f"{'walk':10s} {'':7s} {walk:9.0f} {'':6s} {walk_spill:9.0f}  nt nv x {hdr} + {walked:g} walked x FRAMES {static.get('FRAMES', 0)} + {prep_profiles:g} profiles x PREP {static.get('PREP', 0)} + {a.s_rounds} S rounds x {rs} + {a.b_rounds} B rounds x ({static.get('B', 0)} + {rb}) + {a.n_rounds} N rounds x ({static.get('N', 0)} + {rn})" + (f" + fold loop 2 x ({a.fold_trips} - 1) trips per N round" if fold else ""))
for name in ("VCIRC", "VTEST"):  # stage V: two loops per section whose trip weights are not measured - NOT modelled, part of the remainder
    if name in static:
        print(f"{name:10s} {static[name]:7d} {'':9s} {spill[name]:6d} {'':9s}  (static: stage V, not modelled; in the remainder)")
if "APPSERIES" in static:
    print(f"{'APPSERIES':10s} {static['APPSERIES']:7d} {'':9s} {spill['APPSERIES']:6d} {'':9s}  (static: the appended series workgroups, two wavefronts per ego; in the remainder)")
# outside every section: what the marks leave (a source without the whole-kernel marks: entry, glue, loop headers, walk set-up, appended workgroups)
print(f"{'outside':10s} {outside:7d} {'':9s}  (static, outside every section)")
nonwalk = total
ego = nonwalk + walk
tail = a.tail * nonwalk  # (each half repeats the prologue; its walk and assembly are halves)
print(f"{'tail split':10s} {'':7s} {tail:9.0f}  {a.tail:.4f} of the egos run the sections above a second time")
print(f"{'explained per ego':52s} {ego + tail:9.0f}")
if a.counter:
    per = a.counter / a.egos
    print(f"{'SQ_INSTS_VALU / egos':52s} {per:9.0f}")
    print(f"{'unexplained remainder':52s} {per - ego - tail:9.0f}  ({100 * (per - ego - tail) / per:.1f} %: the appended series workgroups, loop trips the model counts once, branches only one wavefront takes inside sections weighed on all)")
