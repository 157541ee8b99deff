#!/usr/bin/env python3
"""Static instruction mix of one kernel instance by source line and by `// [section NAME]` (needs a -gline-tables-only -S file).

  python tools/isa_lines.py <file.s> <mangled-name substring> [lo hi] [--src FILE] [--lines]

The assembly comes from the Makefile's flags plus `-gline-tables-only -S --cuda-device-only`:

  (cd fiss_plus_planner_amd/csrc &&
  hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -mllvm -disable-machine-licm \
        -gline-tables-only -S --cuda-device-only -o /tmp/fused.s frenet_lattice_fused.hip)
  python tools/isa_lines.py /tmp/fused.s Li9ELi9ELi7ELi2ELi50ELi25ELi8ELi1ELi512ELb0ELb0ELb0E

File numbers are mapped through the `.file` directives; the main file is the one the unnumbered / number-0 directive names.  An
instruction whose .loc lies in the kernel's body keeps that line.  An instruction of an inlined helper - another file, or a line of the
main file above the kernel's own first line - goes to its outermost call site in the body when the .loc's comment names one
(`; helper.h:12:3 @[ main.hip:1188:80 ]`), else it stays with the last body line before it; either way it is counted with the
innermost `// [section NAME]` ... `// [/section NAME]` pair (read from the source: --src, or the path in the .file directive) around
that line.  A section nested in another (a branch that only some inputs take) is reported on its own, not inside the outer one.

Prints the section totals (VALU split into fp64 / fp32 / int / mov+select / lane / lane operations on spilled SGPRs / other, then SALU, LDS, VMEM, branches, waits), the
totals of [lo, hi] when given, and with --lines every line.  Static counts - loops are not weighted - but inside one loop body they are
the per-iteration mix.
"""
import argparse
import collections
import os
import re
import sys

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("path")
ap.add_argument("key")
ap.add_argument("lo", nargs="?", type=int)
ap.add_argument("hi", nargs="?", type=int)
ap.add_argument("--src")
ap.add_argument("--lines", action="store_true")
a_ = ap.parse_intermixed_args()
path, key, lo, hi, src_opt, show_lines = a_.path, a_.key, a_.lo, a_.hi, a_.src, a_.lines
if lo is not None and hi is None:
    ap.error("lo needs hi")

F64 = re.compile(r"^v_(fma|fmac|mul|add|max|min|rcp|rsq|sqrt|div_scale|div_fmas|div_fixup|fract|floor|ceil|trunc|rndne|ldexp|frexp_mant|cmp_\w+|cmpx_\w+|cvt_f64\w*|cvt_\w+_f64)_f64|^v_cvt_f64|^v_cvt_\w+_f64")
INT = re.compile(r"^v_(add|sub|subrev|mul|mad|lshl|lshr|ashr|and|or|xor|not|bfe|bfi|min|max|mul_lo|mul_hi|mul_u32|mad_u32|mad_i32|add3|lshl_add|lshl_or|and_or|or3|add_lshl|alignbit|perm|mbcnt|ffbh|ffbl|bcnt|cmp_\w+|cmpx_\w+)_(u|i)(16|24|32|64)|^v_(add|sub|subrev|addc|subb)_co|^v_(lshlrev|lshrrev|ashrrev)_b(32|64)|^v_(and|or|xor|not)_b32|^v_mul_(u32_u24|i32_i24|hi_u32_u24)|^v_mad_(u32_u24|i32_i24|u64_u32|i64_i32)|^v_mbcnt|^v_bfe|^v_bfi|^v_lshl_add|^v_add3|^v_lshl_or|^v_and_or|^v_or3|^v_xad|^v_add_lshl")
F32 = re.compile(r"^v_\w+_f(32|16)(_|$)|^v_cvt_")  # (what F64 did not take: single and half precision, and the conversions among them and integers)
MOV = re.compile(r"^v_(mov|cndmask|swap|accvgpr)")
LANE = re.compile(r"^v_(readlane|readfirstlane|writelane|permlane)|^v_\w+_dpp")
# a lane operation on a spilled SGPR: v_writelane_b32 / v_readlane_b32 whose lane select is an immediate (the register allocator's
# spill slots; a lane the program chooses - __builtin_amdgcn_readlane(x, first) - arrives in a scalar register or m0)
SPILL = re.compile(r"^v_(readlane|writelane)_b32\s+[^,]+,\s*[^,]+,\s*\d+\s*(;.*)?$")

VALU = ["f64", "f32", "int", "movsel", "lane", "spill", "vother"]
COLS = VALU + ["salu", "lds", "vmem", "branch", "wait"]


def classify(op, text=""):
    if SPILL.match(text):
        return "spill"
    if op.startswith("s_"):
        if op.startswith("s_waitcnt") or op.startswith("s_nop") or op.startswith("s_barrier"):
            return "wait"
        if op.startswith("s_cbranch") or op.startswith("s_branch"):
            return "branch"
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("v_"):
        if LANE.match(op):
            return "lane"
        if F64.match(op):
            return "f64"
        if INT.match(op):
            return "int"
        if MOV.match(op):
            return "movsel"
        if F32.match(op):
            return "f32"
        return "vother"
    return "other"


# ---- pass 1: the .file table (directives stand anywhere in the file, also after the function that uses them)
files = {}
main_no = main_name = None
for line in open(path):
    m = re.match(r'\s*\.file\s+(?:(\d+)\s+)?(?:"([^"]*)"\s+)?"([^"]*)"', line)
    if not m:
        continue
    no = int(m.group(1)) if m.group(1) is not None else None
    d, name = m.group(2) or "", m.group(3)
    if no is None:  # the translation unit's own name
        main_name = os.path.basename(name)
        continue
    files[no] = (d, name)
if main_name is None:
    main_name = files[min(files)][1]
for no, (d, name) in sorted(files.items()):
    if os.path.basename(name) == os.path.basename(main_name):
        main_no = no
        break
if main_no is None:
    sys.exit(f"no .file directive names the main file {main_name}")

# ---- the sections of the source: (name, first line, last line)
src = src_opt or os.path.join(files[main_no][0], files[main_no][1])
sections = []
if os.path.exists(src):
    open_at = {}
    for n, text in enumerate(open(src), 1):
        m = re.search(r"// \[(/?)section (\w+)\]", text)
        if not m:
            continue
        if m.group(1):
            sections.append((m.group(2), open_at.pop(m.group(2)), n))
        else:
            open_at[m.group(2)] = n
    sections.sort(key=lambda s: s[1])
else:
    print(f"(source {src} not found: no sections; pass --src)", file=sys.stderr)


def section_of(ln):  # the innermost pair around the line
    for name, a, b in reversed(sections):
        if a <= ln <= b:
            return f"{name}@{a}"
    return None


# ---- pass 2: the instructions of the instance
inside = False
body_first = None  # the kernel's own first line: lines of the main file above it are helpers
cur = None         # last body line
per = collections.defaultdict(collections.Counter)      # body line -> class counts (helpers folded in)
helper = collections.defaultdict(collections.Counter)   # (section, helper file) -> class counts
for line in open(path):
    s = line.strip()
    if not inside:
        if s.endswith(":") or ": ;" in s:
            if key in s.split(":")[0] and not s.startswith("."):
                inside = True
        continue
    if s.startswith(".Lfunc_end"):
        break
    m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
    if m:
        fno, ln = int(m.group(1)), int(m.group(2))
        if body_first is None and fno == main_no:
            body_first = ln
        if ln == 0:
            continue
        where = None if (fno == main_no and ln >= body_first) else files.get(fno, ("", f"file{fno}"))[1]
        if where is None:
            cur = ln
        else:  # the assembler comment carries the inlining chain when the compiler knows it: the outermost call site in the body
            for f_, l_ in reversed(re.findall(r"@\[ (\S+?):(\d+):\d+", s)):
                if os.path.basename(f_) == os.path.basename(main_name) and int(l_) >= body_first:
                    cur = int(l_)
                    break
        continue
    if not s or s.startswith((".", ";")) or s.endswith(":"):
        continue
    if cur is None:
        continue
    cls = classify(s.split()[0], s)
    per[cur][cls] += 1
    if where is not None:
        helper[(section_of(cur), os.path.basename(where))][cls] += 1
if not inside:
    sys.exit(f"no function whose name contains {key}")


def row(label, c):
    v = sum(c[k] for k in VALU)
    return f"{label:>24s} {v:6d} " + " ".join(f"{c[k]:7d}" for k in COLS)


head = f"{'':>24s} {'VALU':>6s} " + " ".join(f"{c:>7s}" for c in COLS)
print(head)
if show_lines:
    for ln in sorted(per):
        if lo is not None and (ln < lo or ln > hi):
            continue
        print(row(f"{ln} {section_of(ln) or ''}", per[ln]))
by_sec = collections.defaultdict(collections.Counter)
for ln, c in per.items():
    sec = section_of(ln)
    if sec:
        by_sec[sec].update(c)
for name, a, b in sections:
    k = f"{name}@{a}"
    if k in by_sec:
        print(row(k, by_sec[k]))
        for (sec, f), c in sorted(helper.items(), key=lambda kv: (kv[0][0] or '', kv[0][1])):
            if sec == k:
                print(row(f"of which {f}", c))
if lo is not None:
    tot = collections.Counter()
    for ln, c in per.items():
        if lo <= ln <= hi:
            tot.update(c)
    print(row(f"lines {lo}-{hi}", tot))
    rest = collections.Counter()
    for ln, c in per.items():
        if lo <= ln <= hi and not section_of(ln):
            rest.update(c)
    print(row("  outside sections", rest))
tot = collections.Counter()
for c in per.values():
    tot.update(c)
print(row("kernel", tot))
