#!/usr/bin/env python3
"""The walk kernels as they compile for gfx950, counted from the assembly: no GPU needed (hipcc cross-compiles).

    python3 tools/walk_isa.py                    # every k_walk / k_walk_rows instantiation of csrc/walk.cpp
    python3 tools/walk_isa.py --only 'ILi2E'     # those whose mangled name contains the text
    python3 tools/walk_isa.py --asm walk.s       # count an assembly that is already there (made with -gline-tables-only)

Per kernel: instructions, every v_writelane_b32 and v_readlane_b32 (SGPR spills to VGPR lanes and their reloads, AND the few lane
broadcasts of the code itself: k_walk<2,64,false> has 1,605 readlanes of which 1,518 read the spill VGPRs), the compiler's own count of
spilled SGPRs (sgpr_spill, from the metadata), s_nop, 64-bit multiplies (v_mad_u64_u32), memory instructions, branches, kernarg loads, and from the metadata VGPRs,
LDS and private segment.  The same for the lean-step loop (walk.cpp: `do { lean_step<W>(...) } while (...)`): the tightest span from a label to a
branch back to it around the store that the line table attributes to lean_step's path store.  That span is NOT comparable between builds: the compiler lays the loop's blocks out differently from build to build, and the
span is what lies between the label and the branch (for the unchanged k_walk<2,64,false> 380 instructions in one build, 418 in another,
while the kernel moved by 33); it says how tight one build's loop is, no more.  The counts are STATIC: what a launch executes is a PMC
question.
The compile time of walk.cpp is printed too (device code only, as the count needs it)."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corticall_amd", "csrc")
KERNEL = re.compile(r"^_ZN4ldbg(6k_walkILi\d+ELi\d+ELb[01]EEEvNS_8WalkArgsE|11k_walk_rowsILi\d+ELi\d+EEEvNS_8WalkArgsE)$")
MEMORY = re.compile(r"^(global_|flat_|buffer_|scratch_|ds_|s_load_|s_buffer_load_)")
LABEL = re.compile(r"^([.\w$]+):")
LOC = re.compile(r"^\s+\.loc\s+(\d+)\s+(\d+)")
FILE = re.compile(r"^\s+\.file\s+(\d+)\s+\"([^\"]*)\"(?:\s+\"([^\"]*)\")?")


def hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    sys.exit("hipcc not found")


def compile_walk(out, extra=()):
    """walk.cpp -> gfx950 assembly with a line table, the flags of the product build (csrc/Makefile: HIPFLAGS); returns the seconds it took"""
    t0 = time.time()
    subprocess.check_call([hipcc(), "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function", "-gline-tables-only",
                           "--offload-device-only", "-S", *extra, os.path.join(CSRC, "walk.cpp"), "-o", out], cwd=CSRC)
    return time.time() - t0


def demangle(name):
    m = re.match(r"_ZN4ldbg6k_walkILi(\d+)ELi(\d+)ELb([01])E", name)
    if m:
        return "k_walk<%s, %s, %s>" % (m.group(1), m.group(2), "true" if m.group(3) == "1" else "false")
    m = re.match(r"_ZN4ldbg11k_walk_rowsILi(\d+)ELi(\d+)E", name)
    return "k_walk_rows<%s, %s>" % (m.group(1), m.group(2)) if m else name


def lean_store_line():
    """the line of lean_step's path store: the one store to the path pool inside the lean-step loop"""
    for i, line in enumerate(open(os.path.join(CSRC, "walk.cpp")), 1):
        if "= pack_vertex(av);" in line and "st.pw.cur" in line:
            return i
    return None


def count(ins):
    """ins: list of mnemonics"""
    c = {"instructions": len(ins), "writelane": 0, "readlane": 0, "s_nop": 0, "mul64": 0, "memory": 0, "branches": 0, "kernarg_loads": 0}
    for op in ins:
        if op == "v_writelane_b32": c["writelane"] += 1
        elif op == "v_readlane_b32": c["readlane"] += 1
        elif op == "s_nop": c["s_nop"] += 1
        elif op == "v_mad_u64_u32": c["mul64"] += 1
        if MEMORY.match(op): c["memory"] += 1
        if op.startswith("s_cbranch") or op == "s_branch": c["branches"] += 1
    return c


def lean_loop(ops, labels, branches, store):
    """the instructions of the lean-step loop: the tightest span from a label to a branch back to it that holds instruction `store`, up
    to the last branch back to that label (the loop is laid out as one stretch of the kernel: #pragma unroll 1)"""
    span = None
    for at, target in branches:
        if target in labels and labels[target] <= store <= at and (span is None or at - labels[target] < span[1] - span[0]):
            span = (labels[target], at + 1)
    if span is None:
        return None
    end = max(at + 1 for at, target in branches if labels.get(target) == span[0] and at >= span[0])
    return list(range(span[0], end))


def kernels_of(text):
    """name -> {counts, lean loop counts, metadata}"""
    lines = text.split("\n")
    files = {}
    for l in lines:
        m = FILE.match(l)
        if m:
            files[int(m.group(1))] = m.group(3) or m.group(2)
    walk_files = {n for n, f in files.items() if os.path.basename(f) == "walk.cpp"}
    store_line = lean_store_line()
    out = {}
    i = 0
    while i < len(lines):
        m = LABEL.match(lines[i])
        if not (m and KERNEL.match(m.group(1))):
            i += 1
            continue
        name = m.group(1)
        ops, locs, labels, branches = [], [], {}, []       # per instruction: mnemonic, (file, line); label -> index of the next instruction
        loc = (0, 0)
        i += 1
        while i < len(lines) and not lines[i].startswith("\t.section") and ".end_amdhsa_kernel" not in lines[i] and not lines[i].startswith(".Lfunc_end"):
            l = lines[i]
            i += 1
            lm = LABEL.match(l)
            if lm:
                labels[lm.group(1)] = len(ops)
                continue
            cm = LOC.match(l)
            if cm:
                loc = (int(cm.group(1)), int(cm.group(2)))
                continue
            s = l.strip()
            if not s or s.startswith(".") or s.startswith(";") or s.startswith("//"):
                continue
            op = s.split()[0]
            if op.startswith("s_cbranch") or op == "s_branch":
                branches.append((len(ops), s.split()[1].rstrip(",") if len(s.split()) > 1 else ""))
            ops.append(op)
            locs.append(loc)
        c = count(ops)
        c["kernarg_loads"] = sum(1 for op in ops if op.startswith("s_load_"))
        stores = [j for j, op in enumerate(ops) if op.startswith("global_store") and locs[j][0] in walk_files and locs[j][1] == store_line]
        loop = lean_loop(ops, labels, branches, stores[0]) if stores else None
        out[name] = {"all": c, "lean_loop": count([ops[j] for j in loop]) if loop else None}
    meta = text[text.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in text else ""
    for block in re.split(r"\n  - ", meta)[1:]:
        nm = re.search(r"\.name:\s+(\S+)", block)
        if not nm or nm.group(1) not in out:
            continue
        field = lambda f: int(re.search(r"\.%s:\s+(\d+)" % f, block).group(1))
        out[nm.group(1)]["meta"] = {"vgpr": field("vgpr_count"), "sgpr_spill": field("sgpr_spill_count"), "lds": field("group_segment_fixed_size"),
                                    "private": field("private_segment_fixed_size"), "kernarg": field("kernarg_segment_size")}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--asm", help="count this assembly file and compile nothing")
    ap.add_argument("--only", default="", help="only kernels whose mangled name contains this text")
    ap.add_argument("--keep", help="keep the assembly here")
    a = ap.parse_args()
    if a.asm:
        text = open(a.asm).read()
    else:
        path = a.keep or os.path.join(tempfile.mkdtemp(prefix="walk_isa_"), "walk.s")
        secs = compile_walk(path)
        print("walk.cpp (device code, gfx950, -O3): compiled in %.0f s" % secs)
        text = open(path).read()
    cols = ("instructions", "writelane", "readlane", "s_nop", "mul64", "memory", "branches", "kernarg_loads")
    head = "%-26s %-9s " % ("kernel", "span") + " ".join("%13s" % c for c in cols) + "   vgpr sgpr_spill   lds priv kernarg"
    print(head)
    for name, r in sorted(kernels_of(text).items(), key=lambda kv: demangle(kv[0])):
        if a.only not in name:
            continue
        m = r.get("meta", {})
        tail = "  %5s %10s %5s %4s %7s" % (m.get("vgpr", "?"), m.get("sgpr_spill", "?"), m.get("lds", "?"), m.get("private", "?"), m.get("kernarg", "?"))
        print("%-26s %-9s " % (demangle(name), "kernel") + " ".join("%13d" % r["all"][c] for c in cols) + tail)
        if r["lean_loop"]:
            print("%-26s %-9s " % ("", "lean loop") + " ".join("%13d" % r["lean_loop"][c] for c in cols))
        else:
            print("%-26s %-9s (no backward branch on the loop's line)" % ("", "lean loop"))


if __name__ == "__main__":
    main()
