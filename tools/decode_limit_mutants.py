#!/usr/bin/env python3
"""Do the crafted decode-limit cases (tests/decode_limit_cases.py) have teeth? CPU only; not part of the pytest suite.

For every named single-line mutation of the sequence executors below: copy zxc_amd/csrc, include and tests/wave_emu to a temporary
directory, apply it, build the wave emulator there (~35 s) and run the crafted families (not the random one) in a child
process, every case alone on every route, until one catches it. A wrong byte, a wrong status, a guard violation, an emulator
abort and a crash all count as caught; a case that no longer reaches its path markers with the counts it names is reported
as "path only": tests/test_decode_limits_cpu.py fails on it all the same.

Two guards can only be caught that way: the far path's slot-edge guard ((qa - ma) + round_up(me, 16) + 4 <= out_pad) and the full
executor's sg + 32 <= out_pad only keep a 16-byte LOAD inside the block's slot. The bytes such a load brings from beyond the
slot are masked off or belong to output positions at or beyond out_len, which are undefined by contract. The cases
far/slot_edge/* pin their decisions with the exact counts of L_FAR_GROUP and F_FAR_PREFETCH, the markers inside the guarded
branches.

  python tools/decode_limit_mutants.py [--only NAME ...] [--jobs N] [--out profiles/decode_limit_mutants.md]
"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAN, FULL = "zxc_amd/csrc/zxc_seq_lean.inc", "zxc_amd/csrc/zxc_decode_kernel.hip"

# (name, file, the line's text, its replacement, what it breaks). `old` must occur exactly `count` times (default 1).
MUTANTS = [
    ("stepable_last_group", LEAN, "for (uint32_t go = 0; go < MATCH_MED + 4u; go += 16u) {", "for (uint32_t go = 0; go < MATCH_MED; go += 16u) {",
     "near lane-per-sequence copy: the ninth 16-byte group (ml = 128 off the dword grid) is dropped"),
    ("far_last_group", LEAN, "for (uint32_t go = 32u; go < MATCH_MED + 4u; go += 32u) {", "for (uint32_t go = 32u; go < MATCH_MED; go += 32u) {",
     "far group path: the ninth group is dropped"),
    ("literal_last_groups", LEAN, "for (uint32_t go = 48u; go < LIT_MED + 4u; go += 32u) {", "for (uint32_t go = 48u; go < LIT_MED - 16u; go += 32u) {",
     "literal groups 112..143 are dropped (go < LIT_MED itself is equivalent: the loop steps 48, 80, 112 and le <= 131)"),
    ("head_mask", LEAN, "d.x &= head_mask(la);", "d.x &= head_mask(0u);", "a literal run's first dword keeps the bytes in front of the run"),
    ("fifth_dword_literal", LEAN, "const bool lv5 = lshort && ldl != 0u && le > 12u;", "const bool lv5 = lshort && ldl != 0u && le > 14u;",
     "lv0e: the fifth aligned dword of literal group 0 (le > 13u is equivalent: the dword is needed from le > 16 - ldl, ldl <= 3)"),
    ("fifth_dword_far", LEAN, "const bool fr5 = far_ok && fdl != 0u && me > 12u;", "const bool fr5 = far_ok && fdl != 0u && me > 14u;",
     "fr0e: the fifth aligned dword of far group 0 (me > 13u is equivalent, as for lv0e)"),
    ("bytewise_bound", LEAN, "for (uint32_t t = 0; t < BYTEWISE_MAX; t++) {", "for (uint32_t t = 0; t < BYTEWISE_MAX - 1u; t++) {",
     "the bytewise copy stops one byte short of BYTEWISE_MAX"),
    ("lean_tile_plus_64", LEAN, "#define LEAN_TILE_MAX (RING_BYTES - 1056u)", "#define LEAN_TILE_MAX (RING_BYTES - 992u)",
     "a tile 64 bytes longer: more than the ring holds beside 1023 unflushed bytes (+ 32 is equivalent: 1023 + 3072 rounds up to exactly 4096)"),
    ("far_flushed_guard", LEAN, "qa >= 4u && qa + ml <= O.flushed &&", "qa >= 4u && qa + ml <= O.flushed + 1u &&",
     "a far source may end one byte beyond what has been flushed"),
    ("far_qa_guard", LEAN, "ml <= MATCH_MED && qa >= 4u &&", "ml <= MATCH_MED && qa >= 2u &&",
     "a far source may start at 2 (qa >= 3u is equivalent: qa - (M & 3) cannot go negative from 3)"),
    ("far_slot_edge_guard", LEAN, "(qa - ma) + ((me + 15u) & ~15u) + 4u <= O.out_pad;", "true;",
     "a far group may be loaded from beyond the slot's end (no defined byte can differ: caught by the exact L_FAR_GROUP count)"),
    ("wait_for_all", LEAN, "if (o2) jb = (uint32_t)lane;", "if (false && o2) jb = (uint32_t)lane;",
     "a source over three earlier matches waits for two of them"),
    ("redirect_first_period", LEAN, "qb <= jE && qb - jM <= jo;", "qb <= jE && qb - jM <= jo + 64u;",
     "redirect although the source reaches beyond the earlier match's first period"),
    ("varint_cut", LEAN, "r2 + (escM ? 1u : 0u) > LEAN_VARINTS);", "r2 + (escM ? 1u : 0u) > LEAN_VARINTS + 4u);",
     "a batch takes four more varints than the fast path's window holds (+ 1u is within the tables' slack)"),
    ("error_order", LEAN, "if (e <= k) {", "if (e < k) {", "an error at the first sequence beyond the tile is not returned"),
    ("coop_match_doubling", FULL, "            dist <<= 1;", "            dist <<= 2;",
     "the period copy quadruples its distance (dropping the doubling altogether is equivalent, only slower)"),
    ("full_error_order", FULL, "if (e <= k) {", "if (e < k) {", "full executor: an error at the first sequence beyond the tile is not returned"),
    ("full_far_prefetch_edge", FULL, "stepable && farsrc && sg + 32u <= O.out_pad;", "stepable && farsrc;",
     "full executor: far groups are requested from beyond the slot's end (caught by the exact F_FAR_PREFETCH count)"),
]

NOTE = ("\nThe two slot-edge mutants can be caught by path counts only: their guards keep a 16-byte load inside the block's slot, and what such a "
        "load brings from beyond the slot is masked off or lands at or beyond `out_len`. The cases `far/slot_edge/*` assert the exact counts of "
        "`L_FAR_GROUP` and `F_FAR_PREFETCH`, the markers inside the guarded branches.\n")


def child(tmp):
    """Runs the crafted families against the emulator built in tmp; prints one line per event, ends at the first catch."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"),
                    os.path.join(tmp, "tests", "wave_emu")]
    import ctypes as C

    import numpy as np

    import decode_limit_cases as D
    import decode_plan_cases as P
    import emu_py
    import oracle_py
    assert emu_py.HERE.startswith(tmp)
    oracle, ref, emu = oracle_py.Oracle(), oracle_py.Ref(), emu_py.Emu()
    ids = D.path_ids()
    emu.lib.emu_path_read.argtypes = [C.c_void_p, C.c_uint32]
    path_only = None
    for fam in D.FAMILIES:
        for i, c in enumerate(D.family(fam)):
            for route in c.routes:
                case, lc = D.pack(oracle, ref, [c], route, align0=i)
                size = P.guarded_layout(case)
                print(f"RUN {c.name} [{route}]", flush=True)
                emu.lib.emu_path_reset()
                kw = dict(cap_override=c.bs) if route == "strict" else {}
                st, out = emu.decode_jobs(case.comp, case.jobs, size, case.block_size, dict_=case.dict_, init=P.canary(size).tobytes(), **kw)
                o = np.frombuffer(out, dtype=np.uint8)
                try:
                    assert emu.last_pads == 0, "a store outside the output buffer"
                    P.check_guarded(case, o, st)
                except AssertionError as e:
                    kind = "guard" if "outside" in str(e) else ("status" if "status differs" in str(e) else "bytes")
                    print(f"CAUGHT {kind} | {c.name} [{route}] | {D.explain(case, lc, o, st)}", flush=True)
                    return
                a = np.zeros(len(ids), dtype=np.uint64)
                emu.lib.emu_path_read(a.ctypes.data, len(ids))
                for name, n in c.paths.get(route, []):
                    got = int(a[ids[name]])
                    if path_only is None and ((got == 0) if n is None else (got != n)):
                        path_only = f"{c.name} [{route}] | {name} = {got}, wanted {'> 0' if n is None else n}"
    print(f"PATHONLY {path_only}" if path_only else "SURVIVED", flush=True)


def run_mutant(m, keep=False):
    name, rel, old, new, what = m[:5]
    count = m[5] if len(m) > 5 else 1
    tmp = tempfile.mkdtemp(prefix="zxc_mutant_")
    try:
        for d in ("zxc_amd/csrc", "tests/wave_emu", "include"):
            shutil.copytree(os.path.join(ROOT, d), os.path.join(tmp, d), ignore=shutil.ignore_patterns("build", "*.so", "*.o", "__pycache__"))
        path = os.path.join(tmp, rel)
        src = open(path).read()
        assert src.count(old) == count, (name, "the mutation's line occurs", src.count(old), "times, expected", count)
        open(path, "w").write(src.replace(old, new, 1))
        t = time.time()
        b = subprocess.run(["make", "-C", os.path.join(tmp, "tests", "wave_emu"), "all"], capture_output=True, text=True)
        if b.returncode:
            return "does not build", (b.stderr.strip().splitlines() or [""])[-1][:200], time.time() - t
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp], capture_output=True, text=True, timeout=1800)
        lines = [ln for ln in r.stdout.splitlines() if ln]
        last_run = next((ln[4:] for ln in reversed(lines) if ln.startswith("RUN ")), "?")
        final = lines[-1] if lines else ""
        if final.startswith("CAUGHT "):
            kind, case, detail = [x.strip() for x in final[7:].split("|", 2)]
            return kind, f"{case}: {detail}", time.time() - t
        if final.startswith("PATHONLY "):
            return "path only", final[9:], time.time() - t
        if final == "SURVIVED" and r.returncode == 0:
            return "NOT CAUGHT", "", time.time() - t
        how = "emulator abort" if r.returncode in (-6, 134) else f"crash (exit {r.returncode})"
        tail = (r.stderr.strip().splitlines() or [""])[-1][:160]
        return how, f"{last_run}: {tail}", time.time() - t
    finally:
        if not keep:
            shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--jobs", type=int, default=1, help="mutants built and run at the same time")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_limit_mutants.md"))
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    import concurrent.futures
    rows = []
    todo = [m for m in MUTANTS if not a.only or m[0] in a.only]
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, a.jobs)) as pool:
        for m, (res, detail, secs) in zip(todo, pool.map(run_mutant, todo)):
            print(f"{m[0]:28s} {res:16s} {detail}  ({secs:.0f} s)", flush=True)
            rows.append((m, res, detail))
    if not a.only:
        with open(a.out, "w") as f:
            f.write("# Decode-limit mutants\n\nWritten by `tools/decode_limit_mutants.py`: every single-line mutation of the sequence executors, and the first "
                    "crafted case of `tests/decode_limit_cases.py` that catches it on the CPU wave emulator (families in their order, every case "
                    "alone, routes lean / strict / dict; the random family is not run).\n\n"
                    "| mutant | file | line -> mutation | caught by | first catching case |\n|---|---|---|---|---|\n")
            for m, res, detail in rows:
                f.write(f"| {m[0]} | {os.path.basename(m[1])} | `{m[2].strip()}` -> `{m[3].strip()}`: {m[4]} | {res} | {detail.replace('|', '/')} |\n")
            f.write(NOTE)
    return 0 if all(r[1] not in ("NOT CAUGHT", "does not build") for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
