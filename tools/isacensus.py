#!/usr/bin/env python3
"""Static census of one kernel's gfx950 assembly, by opcode class (design tool, CPU only; nothing is run).
usage: isacensus.py file.s kernel_name [--phases] [--from MARK --to MARK]
  file.s     `hipcc --cuda-device-only -S` output (add -DASM_MARKERS for the `; PHMARK n` comments of zxc_seq_lean.inc)
  --phases   one row per PHMARK segment in text order (a kernel that inlines the executor twice shows two runs of marks:
             the rows are numbered copy.mark)
  --from/--to  sum only the segments from the first `PHMARK <from>` up to the next `PHMARK <to>` behind it, e.g. the batch loop
Classes: VALU (v_*, lane moves included), SALU (s_* that is neither a wait, a nop, a branch nor scalar memory), of the SALU the
64-bit mask bookkeeping (s_and_saveexec_b64 s_or_saveexec_b64 s_or_b64 s_and_b64 s_andn2_b64 s_xor_b64 s_mov_b64 s_cselect_b64),
branches (exec branches s_cbranch_execz / execnz apart), s_waitcnt, s_nop, LDS (ds_*), vector memory (global_ / buffer_ / flat_ /
scratch_), scalar memory loads. The kernel's register, spill, LDS and scratch figures come from its .amdhsa metadata."""
import re, sys, collections

MASK_OPS = {"s_and_saveexec_b64", "s_or_saveexec_b64", "s_or_b64", "s_and_b64", "s_andn2_b64", "s_xor_b64", "s_mov_b64",
            "s_cselect_b64"}
COLS = ("all", "valu", "salu", "mask64", "xbranch", "branch", "waitcnt", "nop", "lds", "vmem", "smem")


def classify(op):
    """-> list of columns the instruction counts in (besides "all")"""
    if op.startswith("v_"): return ["valu"]
    if op.startswith("s_waitcnt"): return ["waitcnt"]
    if op.startswith("s_nop"): return ["nop"]
    if op in ("s_cbranch_execz", "s_cbranch_execnz"): return ["branch", "xbranch"]
    if op.startswith("s_cbranch") or op.startswith("s_branch"): return ["branch"]
    if op.startswith("s_load") or op.startswith("s_buffer_load"): return ["smem"]
    if op.startswith("s_"): return ["salu", "mask64"] if op in MASK_OPS else ["salu"]
    if op.startswith("ds_"): return ["lds"]
    if op.split("_")[0] in ("global", "buffer", "flat", "scratch"): return ["vmem"]
    return []


def kernel_lines(lines, kern):
    start = next(i for i, l in enumerate(lines) if l.startswith(kern + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start + 1:end]


def census(body):
    """-> list of (segment name, Counter) in text order"""
    segs, copy, seen = [("pre", collections.Counter())], 0, set()
    for l in body:
        t = l.strip()
        m = re.match(r";\s*PHMARK (\d+)", t)
        if m:
            n = int(m.group(1))
            if n in seen: copy, seen = copy + 1, set()
            seen.add(n)
            segs.append((f"{copy}.{n}", collections.Counter()))
            continue
        if not t or t[0] in ";." or t.endswith(":"): continue
        op = t.split()[0]
        c = segs[-1][1]
        c["all"] += 1
        for k in classify(op): c[k] += 1
    return segs


def metadata(lines, kern):
    """the kernel's .amdhsa figures: {key: int}"""
    want = ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "group_segment_fixed_size",
            "private_segment_fixed_size")
    i = next(i for i, l in enumerate(lines) if re.match(r"\s*\.name:\s+" + re.escape(kern) + r"\s*$", l))
    lo = max(j for j in range(i) if lines[j].lstrip().startswith("- .")) if any(lines[j].lstrip().startswith("- .") for j in range(i)) else 0
    out = {}
    for l in lines[lo:]:
        m = re.match(r"\s*(?:- )?\.(\w+):\s+(\d+)\s*$", l)
        if m and m.group(1) in want and m.group(1) not in out: out[m.group(1)] = int(m.group(2))
        if len(out) == len(want): break
    return out


def row(name, c):
    return f"{name:10s} " + " ".join(f"{c[k]:7d}" for k in COLS)


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    path, kern = args[0], args[1]
    lines = open(path).read().split("\n")
    segs = census(kernel_lines(lines, kern))
    lo = hi = None
    if "--from" in argv:
        lo, hi = argv[argv.index("--from") + 1], argv[argv.index("--to") + 1]
        args = [a for a in args if a not in (lo, hi)]
    print(f"kernel {kern}")
    print(f"{'segment':10s} " + " ".join(f"{k:>7s}" for k in COLS))
    tot = collections.Counter()
    for name, c in segs:
        tot.update(c)
        if "--phases" in argv and sum(c.values()): print(row(name, c))
    if lo is not None:
        part, on = collections.Counter(), False
        for name, c in segs:
            mark = name.split(".")[-1]
            if not on and mark == lo: on = True
            elif on and mark == hi: break
            if on: part.update(c)
        print(row(f"PH{lo}..{hi}", part))
    print(row("total", tot))
    md = metadata(lines, kern)
    print("resources  " + "  ".join(f"{k}={v}" for k, v in md.items()))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
