#!/usr/bin/env python3
"""Instruction mix of one kernel instance by the source function each
instruction comes from.

Builds rtx_kernels.hip to device assembly with the product flags (the
Makefile's HIPFLAGS) plus -gline-tables-only, and attributes every instruction
of the named kernel to the function whose body its `.loc` line lies in (the
innermost inlined function: a line table has no call stack). Per function:
VALU, moves (v_mov*, v_readlane, v_writelane), transcendentals, v_div_scale,
SALU, SMEM and scratch loads/stores; of those, ld@1 / st@1 lie in a loop of
depth 1 (a persistent kernel's main loop) and ld@2+ / st@2+ in the loops
inside it, by the assembler's own "Loop Header: Depth=" block comments.
Static counts: what executes per iteration is for the counters to say.

    python tools/asm_by_source.py [--kernel SUBSTR] [--all | --loops] [--check make-asm.s] [--keep out.s | --asm in.s] [-DRTX_...]

--loops: instead of the table by function, one row per loop of the kernel
(its header's label and depth): the static VALU, packed VALU, SALU, LDS, VMEM
and SMEM counts of its own body and the source lines most VALU come from.

--check: the instruction stream (everything but directives, labels and
comments) must equal that of the given `make asm` output.
--asm: an assembly kept by an earlier run (--keep) instead of compiling; the
tree must still hold the sources it was built from (the functions' line
ranges are read from them).
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytrace-we-gpu_amd", "csrc")
C2 = "k_renderILb1ELb0ELb0ELb0ELb0ELb0E"  # the flagship's lane-mode render
GROUPS = [("line_test_setup",), ("grid_stretch",), ("grid_wave_mask",), ("scan_range",),
          ("resolve_pre_t", "resolve_one"), ("path_segment_m",), ("begin_sample", "start_sample"), ("shade",),
          ("refill",), ("write_pixel",)]
TRANS = ("v_rcp_", "v_rsq_", "v_sqrt_", "v_exp_", "v_log_", "v_sin_", "v_cos_")
NOT_SALU = ("s_load_", "s_buffer_load_", "s_waitcnt", "s_nop", "s_sleep", "s_endpgm", "s_barrier", "s_setprio",
            "s_code_end")


def hipflags():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    f = re.search(r"^HIPFLAGS\s*:=\s*(.*)$", mk, re.M).group(1)
    return f.replace("$(ARCH)", "gfx950").split()


def function_ranges(path):
    """[(first line, last line, name)] of the brace blocks at namespace level."""
    text = open(path, errors="replace").read()
    # blank out comments, strings and preprocessor lines, keeping the newlines
    text = re.sub(r"//[^\n]*|/\*.*?\*/|\"(?:\\.|[^\"\\\n])*\"|'(?:\\.|[^'\\\n])*'",
                  lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
    text = re.sub(r"^[ \t]*#(?:[^\n\\]|\\\n|\\.)*", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.M)
    out, stack, head, line = [], [], [], 1
    for ch in text:
        if ch == "{":
            h = "".join(head).strip()
            ns = re.match(r"(?:inline\s+)?namespace\b|extern\b", h) is not None
            inner = any(not s[0] for s in stack)
            name = None
            if not ns and not inner:
                m = re.search(r"\b(?:struct|class|union|enum)\s+(\w+)[^()]*$", h)
                if m:
                    name = m.group(1)
                else:
                    m = re.search(r"(\w+)\s*\(", re.sub(r"__attribute__\s*\(\(.*?\)\)|__launch_bounds__\s*\([^)]*\)|"
                                                        r"RTX_RENDER_BOUNDS\w*\s*\([^)]*\)|template\s*<.*?>\s*(?=\w)",
                                                        " ", h, flags=re.S))
                    name = m.group(1) if m else "?"
            stack.append((ns, name, line))
            head = []
        elif ch == "}":
            if stack:
                ns, name, first = stack.pop()
                if name is not None:
                    out.append((first, line, name))
            head = []
        elif ch == ";" and not any(not s[0] for s in stack):
            head = []
        else:
            head.append(ch)
        if ch == "\n":
            line += 1
    return out


def instruction(line):
    """The mnemonic of an assembly line, or None for labels, directives and comments."""
    t = line.split(";", 1)[0].strip()
    if not t or t.startswith(".") or t.endswith(":"):
        return None
    return t


def stream(path):
    return [t for t in map(instruction, open(path)) if t]


ap = argparse.ArgumentParser()
ap.add_argument("--kernel", default=C2)
ap.add_argument("--all", action="store_true", help="a row for every function, not only the named groups")
ap.add_argument("--check")
ap.add_argument("--keep")
ap.add_argument("--asm", help="read this -gline-tables-only assembly instead of compiling")
ap.add_argument("--loops", action="store_true",
                help="per loop header of the kernel: depth, VALU, packed VALU, SALU, LDS, VMEM, SMEM of its own "
                     "body and the source lines most of its VALU come from")
a, extra = ap.parse_known_args()

tmp = None
asm = a.asm or a.keep
if asm is None:
    tmp = tempfile.mkdtemp()
    asm = os.path.join(tmp, "k.s")
cmd = ["/opt/rocm/bin/hipcc"] + hipflags() + ["-gline-tables-only", "--offload-device-only", "-S",
                                              os.path.join(CSRC, "rtx_kernels.hip"), "-o", asm] + extra
if not a.asm:
    subprocess.run(cmd, check=True)
if a.check:
    mine, theirs = stream(asm), stream(a.check)
    if mine != theirs:
        at = next((i for i, (x, y) in enumerate(zip(mine, theirs)) if x != y), min(len(mine), len(theirs)))
        sys.exit(f"instruction streams differ at instruction {at} ({len(mine)} vs {len(theirs)})")
    print(f"# instruction stream equals {os.path.basename(a.check)}: {len(mine)} instructions")

lines = open(asm).read().splitlines()
files = {}  # .file index -> path
for l in lines:
    m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
    if m:
        files[int(m.group(1))] = os.path.join(m.group(2), m.group(3)) if m.group(3) else m.group(2)
ranges = {}


def owner(fi, ln):
    p = files.get(fi, "")
    if not os.path.isabs(p):
        p = os.path.join(ROOT, p)
    if not p.startswith(ROOT) or not os.path.exists(p):
        return "(" + os.path.basename(p) + ")"
    if p not in ranges:
        ranges[p] = function_ranges(p)
    best = None
    for first, last, name in ranges[p]:
        if first <= ln <= last and (best is None or first > best[0]):
            best = (first, name)
    return best[1] if best else "(" + os.path.basename(p) + ")"


start = next(i for i, l in enumerate(lines)
             if l.startswith("_Z") and a.kernel in l and l.split(";")[0].rstrip().endswith(":"))
end = next(i for i in range(start, len(lines)) if "-- End function" in lines[i] or ".Lfunc_end" in lines[i])
COLS = ["instrs", "valu", "moves", "trans", "div_scale", "salu", "smem", "scratch_ld", "scratch_st",
        "ld@1", "ld@2+", "st@1", "st@2+"]
rows, cur, depth = {}, "?", 0
for l in lines[start + 1:end]:
    m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", l)
    if m:
        cur = owner(int(m.group(1)), int(m.group(2)))
        continue
    # the loop depth of the basic block, from the assembler's own comments: a
    # block begins at a label (or "; %bb.N:"), which says "in Loop: Header=...
    # Depth=D" or is followed by "=> This [Inner] Loop Header: Depth=D"
    if re.match(r"\s*(\.LBB\w+:|; %bb\.\d+:)", l):
        depth = 0
    m = re.search(r"(?:in Loop: Header=\S+|=>\s*This (?:Inner )?Loop Header:) Depth=(\d+)", l)
    if m:
        depth = int(m.group(1))
    t = instruction(l)
    if t is None:
        continue
    op = t.split()[0]
    r = rows.setdefault(cur, dict.fromkeys(COLS, 0))
    r["instrs"] += 1
    if op.startswith("v_"):
        r["valu"] += 1
        r["moves"] += op.startswith(("v_mov_", "v_readlane_", "v_writelane_"))
        r["trans"] += op.startswith(TRANS)
        r["div_scale"] += op.startswith("v_div_scale_")
    elif op.startswith(("s_load_", "s_buffer_load_")):
        r["smem"] += 1
    elif op.startswith("s_"):
        r["salu"] += not op.startswith(NOT_SALU)
    elif op.startswith("scratch_load_"):
        r["scratch_ld"] += 1
        r["ld@1"] += depth == 1
        r["ld@2+"] += depth >= 2
    elif op.startswith("scratch_st"):
        r["scratch_st"] += 1
        r["st@1"] += depth == 1
        r["st@2+"] += depth >= 2

if a.loops:
    # Static body of every loop of the kernel: the instructions of the blocks
    # whose innermost loop it is (an inner loop's blocks count for the inner
    # loop alone), by the assembler's block comments; and the source lines
    # (function:line, by VALU count) they come from.
    LCOLS = ["valu", "pk_valu", "salu", "lds", "vmem", "smem"]
    loops, order, cur_loop, cur_src, label = {}, [], None, "?", None
    for l in lines[start + 1:end]:
        m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", l)
        if m:
            cur_src = f"{owner(int(m.group(1)), int(m.group(2)))}:{m.group(2)}"
            continue
        m = re.match(r"\s*\.L(BB\w+):", l)
        if m:
            label, cur_loop = m.group(1), None
        elif re.match(r"\s*; %bb\.\d+:", l):
            label, cur_loop = None, None
        m = re.search(r"in Loop: Header=(\S+) Depth=(\d+)", l)
        if m:
            cur_loop = m.group(1)
        m = re.search(r"=>\s*This (?:Inner )?Loop Header: Depth=(\d+)", l)
        if m and label:
            cur_loop = label
            if label not in loops:
                order.append(label)
            loops.setdefault(label, dict.fromkeys(LCOLS, 0) | {"src": {}})["depth"] = int(m.group(1))
        t = instruction(l)
        if t is None or cur_loop is None:
            continue
        if cur_loop not in loops:
            order.append(cur_loop)
        r = loops.setdefault(cur_loop, dict.fromkeys(LCOLS, 0) | {"src": {}, "depth": 0})
        op = t.split()[0]
        if op.startswith("v_"):
            r["valu"] += 1
            r["pk_valu"] += op.startswith("v_pk_")
            r["src"][cur_src] = r["src"].get(cur_src, 0) + 1
        elif op.startswith(("s_load_", "s_buffer_load_")):
            r["smem"] += 1
        elif op.startswith("s_"):
            r["salu"] += not op.startswith(NOT_SALU)
        elif op.startswith("ds_"):
            r["lds"] += 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            r["vmem"] += 1
    print(f"# {lines[start].split(':')[0]}: loop bodies (static; inner loops excluded)")
    print(f"{'header':12s} {'depth':>5s} " + " ".join(f"{c:>8s}" for c in LCOLS) + "  top source lines (VALU)")
    for h in order:
        r = loops[h]
        top = sorted(r["src"].items(), key=lambda kv: -kv[1])[:4]
        print(f"{h:12s} {r['depth']:>5d} " + " ".join(f"{r[c]:>8d}" for c in LCOLS) + "  " +
              ", ".join(f"{s} ({n})" for s, n in top))
    if tmp:
        os.remove(asm)
        os.rmdir(tmp)
    sys.exit(0)

table, used = [], set()
for g in GROUPS:
    table.append((" / ".join(g), {c: sum(rows.get(n, {}).get(c, 0) for n in g) for c in COLS}))
    used.update(g)
rest = sorted((n for n in rows if n not in used), key=lambda n: -rows[n]["valu"])
if a.all:
    table += [(n, rows[n]) for n in rest]
else:
    table.append(("other", {c: sum(rows[n][c] for n in rest) for c in COLS}))
table.append(("total", {c: sum(r[c] for r in rows.values()) for c in COLS}))
print(f"# {lines[start].split(':')[0]}")
print(f"{'function':32s} " + " ".join(f"{c:>10s}" for c in COLS))
for n, r in table:
    print(f"{n[:32]:32s} " + " ".join(f"{r[c]:>10d}" for c in COLS))
if tmp:
    os.remove(asm)
    os.rmdir(tmp)
