#!/usr/bin/env python3
"""Executed VALU instructions per ego of one lattice_fused_kernel instance, estimated section by section, beside the counter.

  python tools/nonwalk_census.py <file.s> <instance key> [--src FILE] [shape and work options] [--counter SQ_INSTS_VALU --egos B]

<file.s> and the key are what tools/isa_lines.py takes (a -gline-tables-only -S build; the template arguments as they stand in the
mangled name).  For every `// [section NAME]` of the source the static VALU count of the section is multiplied by how many wavefronts
execute it and how often - a closed form in the shape (nd, nv, nt, rows, n_obs, nx, hp, threads) and in the means of
tools/work_counters.py (survivors of G, B rounds, N rounds) that is printed beside the number.  The walk and the tail split's second
prologue are added, and the total stands beside SQ_INSTS_VALU / egos of a counter run of the same build (`rocprofv3 --pmc
SQ_INSTS_VALU` in a run of its own on `bench.py --steps 3 --warmup 1`) with the remainder it does not explain: the code outside the
sections and the appended series workgroups are not modelled and are part of that remainder.

What the model is and is not.  A section's static count is taken as ONE execution of it by a wavefront that does its work; a loop
inside a section counts once (the bisection of LUT and the end-speed loop of RANGES carry their trip counts below, as a factor on
the whole section - an over-estimate of their headers; --unrolled names the sections whose loop the compiler unrolled, so that the
static count is every trip already: RANGES wherever nv is a template argument).  A wavefront that only tests and skips a section is charged SKIP
instructions when the test is a vector compare, none when it is scalar (--scalar-skip names those sections: the kCut instances
enter LUT's divisions, the square root of `r_ego`, the cost sums, the ends of d_samples and of v_samples (VENDS) and the one-wavefront
argmin on a scalar test).  --two-ends names the sections that have the form of the instances with the two-profile RANGES and the
one-wavefront ARGMIN: RANGES then has no end-speed loop, ARGMIN runs once and only its store (--uniform ARGMIN=9) on every wavefront.  MASKS runs only for slices with an
unproven profile (0.05 of 7 on the headline workload) and is charged its share.
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
ap.add_argument("--scan-slices", type=float, default=0.05, help="work_counters: slices that needed the mask scan")
ap.add_argument("--tail", type=float, default=128 / 2048, help="share of the egos the tail split runs as two workgroups")
ap.add_argument("--scalar-skip", default="", help="comma list of sections whose idle wavefronts skip on a scalar test (the kCut instances: LUT,SUMS)")
ap.add_argument("--uniform", default="", help="NAME=count[@wavefronts],...: instructions of a section that are no part of its dealt work and run once on that many wavefronts, "
                "all by default (parent: FAN=38,LUT=28 - the ends of d_samples, the bucket width's divisions; kCut instances: LUT=28@3)")
ap.add_argument("--two-ends", default="", help="comma list of RANGES, ARGMIN: the section has the form of the instances that take the row ranges from the two extreme end "
                "speeds (no end-speed loop: one trip per lane) / reduce the argmin on one wavefront (the store of every lane's candidate stays on all: --uniform ARGMIN=9)")
ap.add_argument("--unrolled", default="", help="comma list of sections whose inner loop the compiler unrolled (the static count holds every trip already): RANGES in the shaped "
                "instances, where nv is a constant - the counter showed it: taking seven of nine evaluations out removed 0.2 k per ego, not 1.0 k")
ap.add_argument("--counter", type=float, help="SQ_INSTS_VALU per launch")
ap.add_argument("--egos", type=int, default=2048)
a = ap.parse_args()

cmd = [sys.executable, os.path.join(HERE, "isa_lines.py"), a.path, a.key] + (["--src", a.src] if a.src else [])
out = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
static = {}
for line in out.splitlines():
    m = re.match(r"\s*(\w+)@\d+\s+(\d+)", line)
    if m:
        static[m.group(1)] = static.get(m.group(1), 0) + int(m.group(2))
    m = re.match(r"\s*kernel\s+(\d+)", line)
    if m:
        kernel_total = int(m.group(1))

W = a.threads // 64
v = dict(W=W, nd=a.nd, nv=a.nv, nt=a.nt, rows=a.rows, n_obs=a.n_obs, nx=a.nx, hp=a.rows * a.stride + 1, C=a.nd * a.nv * a.nt, surv=a.surv,
         flight=a.flight, threads=a.threads, ceil=math.ceil, log2=math.log2, scan=a.scan_slices)
SKIP = 4  # a vector compare, the EXEC save / restore moves around a section a wavefront has no lane in
scalar = set(filter(None, a.scalar_skip.split(",")))
two_ends = set(filter(None, a.two_ends.split(",")))
unrolled = set(filter(None, a.unrolled.split(",")))
uniform = {k: (int(c.split("@")[0]), int(c.split("@")[1]) if "@" in c else W) for k, c in (kv.split("=") for kv in filter(None, a.uniform.split(",")))}
# section -> (wavefronts x trips that execute it, as a formula of the shape)
WEIGHT = {
    "STAGE": "W",
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
    "ASM": "ceil(C / 64)",
    "ARGMIN": "W" if "ARGMIN" not in two_ends else "1",
    "RESULTS": "1",
}
rows_out, total = [], 0.0
for name, formula in WEIGHT.items():
    if name not in static:
        continue
    w = eval(formula, {}, v)
    idle = max(0.0, W - min(W, math.ceil(w))) if name not in ("MASKS",) else 0.0
    uni, uni_w = uniform.get(name, (0, W))
    n = (static[name] - uni) * w + uni * uni_w + (0 if name in scalar else SKIP * idle)
    rows_out.append((name, static[name], f"{formula}" + (f"; {uni} of them once on {uni_w} wavefronts" if uni else "") + ("" if name in scalar or not idle else f"; + {SKIP} x {idle:.0f} idle"), n))
    total += n
walk_profile = static.get("FRAMES", 0) + static.get("PREP", 0)
# the walk: per profile the loop header (what lies between the sections of the pq loop) + FRAMES + PREP; per round B / N
hdr = 28
walk = a.nt * a.nv * (hdr + walk_profile) + a.b_rounds * static.get("B", 0) + a.n_rounds * static.get("N", 0)
outside = kernel_total - sum(static.values())
print(f"{'section':10s} {'static':>7s} {'executed':>9s}  wavefronts x trips")
for name, s, f, n in rows_out:
    print(f"{name:10s} {s:7d} {n:9.0f}  {f}")
print(f"{'prologue + group test + assembly, sections':52s} {total:9.0f}")
print(f"{'walk':10s} {'':7s} {walk:9.0f}  nt nv ({hdr} + FRAMES {static.get('FRAMES', 0)} + PREP {static.get('PREP', 0)}) + {a.b_rounds} B rounds x {static.get('B', 0)} + {a.n_rounds} N rounds x {static.get('N', 0)}")
# outside the sections: the appended workgroups' branches, entry, argument loads, loop headers, the walk's set-up, the series written by the lattice workgroup (two per CU)
print(f"{'outside':10s} {outside:7d} {'':9s}  (static, whole kernel: appended workgroups, entry, loop headers, walk set-up, series of the two-per-CU instances)")
nonwalk = total
ego = nonwalk + walk
tail = a.tail * nonwalk  # (each half repeats the prologue; its walk and assembly are halves)
print(f"{'tail split':10s} {'':7s} {tail:9.0f}  {a.tail:.4f} of the egos run the sections above a second time")
print(f"{'explained per ego':52s} {ego + tail:9.0f}")
if a.counter:
    per = a.counter / a.egos
    print(f"{'SQ_INSTS_VALU / egos':52s} {per:9.0f}")
    print(f"{'unexplained remainder':52s} {per - ego - tail:9.0f}  ({100 * (per - ego - tail) / per:.1f} %: outside the sections x 8 wavefronts, the appended series workgroups, loop trips the model counts once)")
