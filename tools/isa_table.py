#!/usr/bin/env python
"""What the compiler makes of two versions of one csrc/*.hip file, kernel by kernel (a COMPILE for gfx950, no device involved):

    python tools/isa_table.py OLD_gemv.hip [NEW_gemv.hip] > profiles/gemv_unify_isa.txt
    python tools/isa_table.py --source attention.hip --hot v_mfma OLD_attention.hip [NEW_attention.hip] > profiles/attention_unify_isa.txt

--source names the file of csrc/ that NEW defaults to (gemv.hip), --hot the regular expression whose matches make a basic block a hot
block (default: gemv.hip's non-temporal weight loads and FMA / dot instructions; for attention.hip the blocks that hold an MFMA).
Both files are compiled with the library's flags plus -Rpass-analysis=kernel-resource-usage and --save-temps; a header next to a file
wins over csrc/ (an old gemv.hip travels with its gemv_common.h).  One row per instantiation, joined by demangled name: VGPRs, SGPRs,
scratch bytes per lane, occupancy (waves per SIMD), old -> new, and how the instruction streams compare after renaming labels:
    identical   the same instructions with the same registers
    registers   the same instructions, other register numbers
    outside     differences outside the hot blocks only: the basic blocks that hold a --hot instruction have the same opcode sequence
                (prologue / epilogue scheduling)
    order       the hot blocks hold the same instructions in another order (a compare and the branch on it may be inverted together)
    HOT LOOP    the hot blocks hold other instructions: their number, old -> new, and which opcodes went (-) or came (+)"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chatts_amd import build as b  # noqa: E402

FIELDS = (("VGPRs", "VGPRs"), ("SGPRs", "TotalSGPRs"), ("scratch", "ScratchSize [bytes/lane]"), ("occ", "Occupancy [waves/SIMD]"))
GEMV_HOT = r"\bnt\b|v_fma|v_pk_fma|v_dot2"      # the weight loads and the dot blocks (sumsq4 contracts to v_fmac too: its block has no
# weight load, but it is the same code in both files and costs the comparison nothing)
INVERSE = {"s_cmp_ge_i32": "s_cmp_lt_i32", "s_cmp_le_i32": "s_cmp_gt_i32", "v_cmp_le_i32_e32": "v_cmp_gt_i32_e32",
           "v_cmp_ge_i32_e32": "v_cmp_lt_i32_e32", "s_cbranch_scc0": "s_cbranch_scc1", "s_cbranch_vccz": "s_cbranch_vccnz"}
REG = re.compile(r"\b[vsa](\d+|\[\d+:\d+\])")


def compile_one(src, out):
    os.makedirs(out, exist_ok=True)
    cmd = [b._hipcc(), *b.FLAGS, "-I", os.path.dirname(os.path.abspath(src)), "-I", b.CSRC, "-Rpass-analysis=kernel-resource-usage",
           "--save-temps", "-c", os.path.abspath(src), "-o", "unit.o"]
    r = subprocess.run(cmd, cwd=out, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    asm = next(f for f in os.listdir(out) if f.endswith("gfx950.s"))
    return parse_remarks(r.stderr), parse_asm(open(os.path.join(out, asm)).read())


def parse_remarks(text):
    res, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: .*?:\d+:\d+:\s+(.*?): (\S+) \[-Rpass", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return res


def parse_asm(text):
    """mangled kernel name -> list of basic blocks, each a list of instructions (comments and directives dropped, labels renamed)"""
    kernels, cur, labels = {}, None, {}
    for line in text.splitlines():
        line = line.split(";")[0].rstrip()
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur, labels = kernels.setdefault(m.group(1), [[]]), {}
            continue
        if cur is None or not line.strip():
            continue
        if re.match(r"^\.Lfunc_end", line):
            cur = None
            continue
        if re.match(r"^\.LBB\w+:", line):
            cur.append([])
            continue
        if line.lstrip().startswith("."):
            continue
        cur[-1].append(re.sub(r"\.LBB\d+_\d+", lambda t: labels.setdefault(t.group(0), f"L{len(labels)}"), line.strip()))
    return kernels


def verdict(old, new, hot_re):
    if old == new:
        return "identical"
    mask = lambda blocks: [[REG.sub("r", i) for i in blk] for blk in blocks]          # noqa: E731
    if mask(old) == mask(new):
        return "registers"
    hot = lambda blocks: [[i.split()[0] for i in blk] for blk in blocks if any(hot_re.search(i) for i in blk)]      # noqa: E731
    ho, hn = hot(old), hot(new)
    if ho == hn:
        return "outside"
    bag = lambda blocks: collections.Counter(INVERSE.get(op, op) for blk in blocks for op in blk)          # noqa: E731
    if bag(ho) == bag(hn):
        return "order"
    delta = [f"-{n} {op}" for op, n in sorted((bag(ho) - bag(hn)).items())] + [f"+{n} {op}" for op, n in sorted((bag(hn) - bag(ho)).items())]
    return f"HOT LOOP {sum(map(len, ho))} -> {sum(map(len, hn))} ({', '.join(delta)})"


TYPES = (("DF16_", "_Float16"), ("f", "float"), ("i", "int"), ("b", "bool"))


def demangle(names):
    """_ZN6chatts16gemv_ldsx_kernelILi2ELi2ELi0ELb1EEEvNS_10GemvParamsE -> gemv_ldsx_kernel<2, 2, 0, true>: the kernel's name in
    namespace chatts and its template arguments (integer and bool literals, float / _Float16 / int / bool types); a name of another
    shape stays as it is"""
    out = {}
    for n in names:
        out[n] = n
        m = re.match(r"_ZN6chatts(\d+)", n)
        if not m:
            continue
        at = m.end() + int(m.group(1))
        name, rest, args = n[m.end():at], n[at:], []
        if rest.startswith("I"):
            rest = rest[1:]
            while rest and not rest.startswith("E"):
                lit = re.match(r"L([ib])(\d+)E", rest)
                typ = next((t for t in TYPES if rest.startswith(t[0])), None)
                if lit:
                    args.append(("true" if lit.group(2) == "1" else "false") if lit.group(1) == "b" else lit.group(2))
                    rest = rest[lit.end():]
                elif typ:
                    args.append(typ[1])
                    rest = rest[len(typ[0]):]
                else:
                    break
            if not rest.startswith("E"):
                continue
        out[n] = name + (f"<{', '.join(args)}>" if args else "")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--source", default="gemv.hip", help="the file of csrc/ that NEW defaults to")
    ap.add_argument("--hot", default=GEMV_HOT, help="regular expression: a basic block with a match is a hot block")
    ap.add_argument("old")
    ap.add_argument("new", nargs="?")
    args = ap.parse_args()
    new_src = args.new or os.path.join(b.CSRC, args.source)
    hot_re = re.compile(args.hot)
    with tempfile.TemporaryDirectory() as tmp:
        (ro, ao), (rn, an) = compile_one(args.old, os.path.join(tmp, "old")), compile_one(new_src, os.path.join(tmp, "new"))
    names = demangle(sorted(set(ro) | set(rn)))
    # joined by demangled name: a kernel whose parameter list changed has another mangled name in the new file
    for d in (ro, ao, rn, an):
        for mangled in list(d):
            d[names.get(mangled, mangled)] = d.pop(mangled)
    names = {n: n for n in names.values()}
    print("compiled for gfx950 with " + " ".join(b.FLAGS) + f"; hot blocks: /{args.hot}/; nothing in this table was run")
    print(f"{'kernel':58s} {'VGPRs':>10s} {'SGPRs':>10s} {'scratch':>8s} {'occ':>8s}  stream")
    counts, worse = {}, []
    for mangled, name in sorted(names.items(), key=lambda kv: kv[1]):
        o, n = ro.get(mangled), rn.get(mangled)
        if o is None or n is None:
            v = "only in the old file" if n is None else "only in the new file"
            cols = [(o or n)[key] + ("    -" if n is None else "") for _, key in FIELDS]
        else:
            v = verdict(ao[mangled], an[mangled], hot_re)
            cols = [f"{o[key]} -> {n[key]}" if o[key] != n[key] else o[key] for _, key in FIELDS]
            if int(n["ScratchSize [bytes/lane]"]) > int(o["ScratchSize [bytes/lane]"]) or int(n["Occupancy [waves/SIMD]"]) < int(o["Occupancy [waves/SIMD]"]):
                worse.append(name)
        kind = "HOT LOOP" if v.startswith("HOT LOOP") else v
        counts[kind] = counts.get(kind, 0) + 1
        print(f"{name:58s} {cols[0]:>10s} {cols[1]:>10s} {cols[2]:>8s} {cols[3]:>8s}  {v}")
    print("summary: " + ", ".join(f"{k}: {v}" for k, v in sorted(counts.items())))
    print("more scratch or lower occupancy than the old file: " + (", ".join(worse) if worse else "none"))
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main())
