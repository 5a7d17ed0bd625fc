"""Every decode launch plan of zxc_hip_shim.hip, on the CPU wave emulator, with guarded outputs: the slots of the job table
have gaps, start at offsets that are multiples of 16 but not of 64, and sit between guard regions filled with a canary
(tests/decode_plan_cases.py). After each launch no byte outside [out_off, out_off + round_up(out_len, 16)) of any block may
have changed, whatever the block's status, and every block has the reference's verdict. Clean and mutated inputs, 4 KiB,
64 KiB and 2 MiB blocks, archives whose last block has a short, unaligned out_len."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import decode_plan_cases as P
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "wave_emu"))

PSCRATCH_DEFAULT = 8 << 20
RSCRATCH_DEFAULT = 4 << 20
RSCRATCH_PARTIAL = 16 << 10  # the second workgroup of the launch-order pass finds it used up (test_rle_scratch_plans asserts the mix)


@pytest.fixture(scope="module")
def emu():
    import emu_py
    e = emu_py.Emu()
    L = e.lib
    L.emu_set_pscratch_bytes.argtypes = [C.c_size_t]
    L.emu_set_rscratch_bytes.argtypes = [C.c_size_t]
    for f in ("emu_last_deferred_count", "emu_last_pre_count"):
        getattr(L, f).restype = C.c_uint32
    yield e
    L.emu_set_pscratch_bytes(PSCRATCH_DEFAULT)
    L.emu_set_rscratch_bytes(RSCRATCH_DEFAULT)


@pytest.fixture(scope="module")
def cases(oracle, ref):
    """name -> Case; small inputs (the emulator runs one wavefront at a time)."""
    c = {}
    tail = -13  # every archive's last block keeps an out_len that is not a multiple of 16
    c["L1ck/64K"] = P.level_case(oracle, ref, 1, 65536, 4 * 65536 + tail, checksum=True)
    c["L1ck/64K mut"] = P.level_case(oracle, ref, 1, 65536, 4 * 65536 + tail, checksum=True, n_hit=3)
    c["L3/4K mut"] = P.level_case(oracle, ref, 3, 4096, 48 * 4096 + tail, n_hit=12)
    c["L6ck/4K"] = P.level_case(oracle, ref, 6, 4096, 48 * 4096 + tail, checksum=True)
    c["L6ck/4K mut"] = P.level_case(oracle, ref, 6, 4096, 48 * 4096 + tail, checksum=True, n_hit=9)
    c["L7/64K mut"] = P.level_case(oracle, ref, 7, 65536, 6 * 65536 + tail, n_hit=6)
    c["L7ck/4K mut"] = P.level_case(oracle, ref, 7, 4096, 48 * 4096 + tail, checksum=True, n_hit=9)
    c["L3/2M"] = P.level_case(oracle, ref, 3, 2 << 20, 300000 + tail)
    c["L7/2M"] = P.level_case(oracle, ref, 7, 2 << 20, 300000 + tail)
    for k in c:
        P.require(c[k], failed=1 if "mut" in k else 0)
    P.require(c["L6ck/4K mut"], pivco=20, failed=6)
    P.require(c["L7ck/4K mut"], pivco=20, failed=6)
    P.require(c["L7/2M"], pivco=1)
    return c


def _run(emu, case, size=None, **kw):
    size = size or P.guarded_layout(case)
    st, out = emu.decode_jobs(case.comp, case.jobs, size, case.block_size, verify_trailer=case.checksum, dict_=case.dict_,
                              dict_huf=case.dict_huf, init=P.canary(size).tobytes(), **kw)
    assert emu.last_pads == 0, (case.label, "a store landed outside the output buffer", emu.last_pads)
    P.check_guarded(case, np.frombuffer(out, dtype=np.uint8), st)
    return st


@pytest.mark.parametrize("ck_apart", [True, False], ids=["ck_apart", "ck_inline"])
def test_two_pass_plan_guarded(emu, cases, ck_apart):
    """The two-pass launch with section and RLE scratch: section kernels, lean kernel and its second entry, full kernel over
    its list; checksums by zxc_block_checksum_kernel + the merge pass, or inside the decode kernels."""
    emu.lib.emu_set_pscratch_bytes(PSCRATCH_DEFAULT)
    emu.lib.emu_set_rscratch_bytes(RSCRATCH_DEFAULT)
    pre = full = 0
    for name, case in cases.items():
        if ck_apart or case.checksum:
            _run(emu, case, ck_apart=ck_apart)
            pre += emu.lib.emu_last_pre_count()
            full += emu.lib.emu_last_deferred_count()
    assert pre >= 20, (pre, full)  # blocks through the section kernels (the full kernel's share: test_section_scratch_plans_guarded)


@pytest.mark.parametrize("pscratch", [0, 600 << 10], ids=["none", "too_small"])
def test_section_scratch_plans_guarded(emu, cases, oracle, ref, pscratch):
    """No section scratch (every coded block to the full kernel) and one that runs out after the first workgroup of the
    launch-order pass (section kernels and full kernel both take PivCo blocks in one launch)."""
    emu.lib.emu_set_rscratch_bytes(RSCRATCH_DEFAULT)
    try:
        emu.lib.emu_set_pscratch_bytes(pscratch)
        for name in ("L6ck/4K mut", "L7ck/4K mut", "L7/64K mut", "L7/2M"):
            _run(emu, cases[name], ck_apart=False)
            if pscratch == 0:
                assert emu.lib.emu_last_pre_count() == 0
        if pscratch:
            big = P.level_case(oracle, ref, 7, 4096, 300 * 4096 - 13, n_hit=20, seed=6)
            P.require(big, pivco=256, failed=10, n_jobs=257)
            _run(emu, big)
            pre, full = emu.lib.emu_last_pre_count(), emu.lib.emu_last_deferred_count()
            assert pre and full, ("the section scratch did not run out part way", pre, full)
    finally:
        emu.lib.emu_set_pscratch_bytes(PSCRATCH_DEFAULT)


def test_rle_scratch_plans_guarded(emu, oracle, ref):
    """LEAN_RLE blocks: no RLE scratch (all to the full kernel), one that runs out part way (both paths in one launch), one
    that fits (all through zxc_rle_expand_kernel + the lean kernel); clean and mutated."""
    clean = P.rle_mix_case(oracle, ref, 40, 300, n_bytes=(8 << 20) - 13)
    mut = P.rle_mix_case(oracle, ref, 40, 300, n_hit=24, n_bytes=(8 << 20) - 13)
    n_rle = P.require(clean, rle=40, n_jobs=257, unaligned_tail=False)[0]
    P.require(mut, rle=40, failed=6, n_jobs=257, unaligned_tail=False)
    try:
        for rs, want in ((0, "all"), (RSCRATCH_PARTIAL, "some"), (RSCRATCH_DEFAULT, "none")):
            emu.lib.emu_set_rscratch_bytes(rs)
            _run(emu, clean)
            deferred = emu.lib.emu_last_deferred_count()
            assert deferred == {"all": n_rle, "none": 0}.get(want, deferred) and (want != "some" or 0 < deferred < n_rle), (rs, deferred)
            _run(emu, mut)
    finally:
        emu.lib.emu_set_rscratch_bytes(RSCRATCH_DEFAULT)


def test_strict_capacity_plan_guarded(emu, cases, oracle):
    """cap_override (zxc_decompress_block_safe): the full kernel alone, verdicts of the reference's strict decoders."""
    for name in ("L1ck/64K mut", "L3/4K mut", "L6ck/4K mut", "L7ck/4K mut"):
        c = cases[name]
        cap = c.block_size
        rc = []
        want = []
        for j in c.jobs:
            blk = c.comp[int(j["comp_off"]):int(j["comp_off"]) + int(j["comp_size"])]
            r, b = oracle.decode_block(blk, c.block_size, cap=cap, checksum=c.checksum, strict_tail=True)
            rc.append(r)
            want.append(b if r >= 0 else b"")
        strict = P.Case(c.comp, c.jobs.copy(), c.block_size, c.checksum, np.array(rc, dtype=np.int32), want, label=name + " strict")
        _run(emu, strict, cap_override=cap)


def test_dictionary_plan_guarded(emu, oracle, ref):
    """zxc_decode_blocks_dict_kernel, with and without the dictionary's shared literal table, clean and mutated; verdicts
    from the reference Block API with the dictionary."""
    for level, huf, ck in ((3, False, False), (7, True, True)):
        for n_hit in (0, 12):
            c = P.dict_case(oracle, ref, level, 4096, 40 * 4096 - 13, huf, checksum=ck, n_hit=n_hit)
            P.require(c, failed=3 if n_hit else 0, pivco=10 if level == 7 else 0)
            _run(emu, c)


# ---- the plan table and the launch-order buffer layout of zxc_dev.h (what zxc_hip_shim.hip and the emulator both use) ----

class PlanIn(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("dict", "cap_override", "n_jobs", "max_slots", "debug", "verify_trailer", "block_size",
                                          "slot", "helpers", "hint", "hint0", "hint1", "ck_inline", "no_rle_scratch",
                                          "rle_lean_max_jobs", "no_pre", "order_failed", "pscratch_failed", "rscratch_failed")]


class Plan(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("ordered", C.c_uint32), ("ck_apart", C.c_uint32), ("trailer_bytes", C.c_uint32),
                ("pscratch_bytes", C.c_uint64), ("rscratch_bytes", C.c_uint64)]


class OrdLayout(C.Structure):
    _fields_ = [(f, C.c_size_t) for f in ("list", "order", "ctl", "pre_ent", "secs", "pre", "ck_bad", "words")]


FULL, DICT, TWO_PASS, PRE = range(4)
NO_TWO_PASS, NO_ORDER, ELSEWHERE = 0x40000000, 0x80000000, 0x80000000
LEAN_MAX = 16384    # ZXC_RLE_LEAN_MAX_JOBS (zxc_hip_shim.hip)
SLOTS = 8192        # max_slots of a 256-CU device at 32 workgroups per CU
GIB = 1 << 30
BASE = dict(n_jobs=1000, max_slots=SLOTS, block_size=65536, slot=1, helpers=1, hint=1, rle_lean_max_jobs=LEAN_MAX)


def pre_bytes(n, bs):
    return min(n * (bs + bs // 5 + 256), GIB)


def rle_bytes(w16, n, bs):
    return min((w16 * 16 * 5 // 4 + 65536) & ~4095, n * (bs + 96), GIB)


# (inputs on top of BASE, expected (kind, ordered, ck_apart, trailer_bytes, pscratch_bytes, rscratch_bytes))
PLAN_TABLE = [
    # dictionary: ordered iff n_jobs > max_slots, no debug NO_ORDER, a slot, the order buffer granted
    ("dict", dict(dict=1), (DICT, 0, 0, 0, 0, 0)),
    ("dict verify", dict(dict=1, verify_trailer=1), (DICT, 0, 0, 4, 0, 0)),
    ("dict max_slots-1", dict(dict=1, n_jobs=SLOTS - 1), (DICT, 0, 0, 0, 0, 0)),
    ("dict max_slots", dict(dict=1, n_jobs=SLOTS), (DICT, 0, 0, 0, 0, 0)),
    ("dict max_slots+1", dict(dict=1, n_jobs=SLOTS + 1), (DICT, 1, 0, 0, 0, 0)),
    ("dict long, no order", dict(dict=1, n_jobs=SLOTS + 1, debug=NO_ORDER), (DICT, 0, 0, 0, 0, 0)),
    ("dict long, no slot", dict(dict=1, n_jobs=SLOTS + 1, slot=0), (DICT, 0, 0, 0, 0, 0)),
    ("dict long, order buffer failed", dict(dict=1, n_jobs=SLOTS + 1, order_failed=1), (DICT, 0, 0, 0, 0, 0)),
    # strict capacity or debug NO_TWO_PASS: FULL, ordered under the same condition
    ("cap_override", dict(cap_override=4096, verify_trailer=1), (FULL, 0, 0, 4, 0, 0)),
    ("cap_override max_slots", dict(cap_override=4096, n_jobs=SLOTS), (FULL, 0, 0, 0, 0, 0)),
    ("cap_override max_slots+1", dict(cap_override=4096, n_jobs=SLOTS + 1), (FULL, 1, 0, 0, 0, 0)),
    ("cap_override long, no order", dict(cap_override=4096, n_jobs=SLOTS + 1, debug=NO_ORDER), (FULL, 0, 0, 0, 0, 0)),
    ("no two-pass", dict(debug=NO_TWO_PASS, hint0=7, hint1=100), (FULL, 0, 0, 0, 0, 0)),
    ("no two-pass long", dict(debug=NO_TWO_PASS, n_jobs=SLOTS + 1), (FULL, 1, 0, 0, 0, 0)),
    ("no two-pass long, no order", dict(debug=NO_TWO_PASS | NO_ORDER, n_jobs=SLOTS + 1), (FULL, 0, 0, 0, 0, 0)),
    # two-pass downgrades: no slot / order buffer or memset failed -> FULL unordered; no helper streams -> FULL ordered
    ("no free slot", dict(slot=0, verify_trailer=1, hint1=100), (FULL, 0, 0, 4, 0, 0)),
    ("no free slot, long", dict(slot=0, n_jobs=SLOTS + 1, hint0=3), (FULL, 0, 0, 0, 0, 0)),
    ("order buffer failed", dict(order_failed=1, hint0=5, hint1=100), (FULL, 0, 0, 0, 0, 0)),
    ("no helpers", dict(helpers=0, verify_trailer=1, hint1=100), (FULL, 1, 0, 4, 0, 0)),
    ("no helpers, no order debug", dict(helpers=0, debug=NO_ORDER), (FULL, 1, 0, 0, 0, 0)),
    # PRE: no hint page, or hint word 0 != 0 (0xFFFFFFFF: first launch on the slot)
    ("no hint page", dict(hint=0, hint1=100), (PRE, 1, 0, 0, pre_bytes(1000, 65536), 0)),
    ("first launch", dict(hint0=0xFFFFFFFF), (PRE, 1, 0, 0, pre_bytes(1000, 65536), 0)),
    ("PRE blocks last time", dict(hint0=3, verify_trailer=1), (PRE, 1, 0, 4, pre_bytes(1000, 65536), 0)),
    ("PRE capped at 1 GiB", dict(hint0=3, n_jobs=16896), (PRE, 1, 0, 0, GIB, 0)),
    ("PRE scratch failed", dict(hint0=3, pscratch_failed=1), (TWO_PASS, 1, 0, 0, 0, 0)),
    ("PRE scratch failed, verify", dict(hint0=3, pscratch_failed=1, verify_trailer=1), (TWO_PASS, 1, 1, 4 | ELSEWHERE, 0, 0)),
    ("EXP_NO_PRE", dict(hint0=3, no_pre=1, verify_trailer=1), (TWO_PASS, 1, 1, 4 | ELSEWHERE, 0, 0)),
    ("no PRE blocks last time", dict(), (TWO_PASS, 1, 0, 0, 0, 0)),
    # RLE scratch: hint page, n_jobs < ZXC_RLE_LEAN_MAX_JOBS, hint word 1 != 0, no ZXC_MI355X_NO_RLE_SCRATCH
    ("RLE", dict(hint1=1000), (TWO_PASS, 1, 0, 0, 0, rle_bytes(1000, 1000, 65536))),
    ("RLE beside PRE", dict(hint0=2, hint1=1000), (PRE, 1, 0, 0, pre_bytes(1000, 65536), rle_bytes(1000, 1000, 65536))),
    ("RLE lean max-1", dict(hint1=1000, n_jobs=LEAN_MAX - 1), (TWO_PASS, 1, 0, 0, 0, rle_bytes(1000, LEAN_MAX - 1, 65536))),
    ("RLE lean max", dict(hint1=1000, n_jobs=LEAN_MAX), (TWO_PASS, 1, 0, 0, 0, 0)),
    ("RLE lean max+1", dict(hint1=1000, n_jobs=LEAN_MAX + 1), (TWO_PASS, 1, 0, 0, 0, 0)),
    ("RLE capped by the launch", dict(hint1=10 ** 6, n_jobs=1, block_size=4096), (TWO_PASS, 1, 0, 0, 0, 4096 + 96)),
    ("RLE capped at 1 GiB", dict(hint1=1 << 28, n_jobs=16000, block_size=1 << 21), (TWO_PASS, 1, 0, 0, 0, GIB)),
    ("RLE switched off", dict(hint1=1000, no_rle_scratch=1), (TWO_PASS, 1, 0, 0, 0, 0)),
    ("RLE scratch failed", dict(hint1=1000, rscratch_failed=1), (TWO_PASS, 1, 0, 0, 0, 0)),
    ("RLE without hint page", dict(hint=0, hint0=0, hint1=1000), (PRE, 1, 0, 0, pre_bytes(1000, 65536), 0)),
    # checksums apart: TWO_PASS, verify, no ZXC_MI355X_CK_INLINE
    ("checksums apart", dict(verify_trailer=1, hint1=1000), (TWO_PASS, 1, 1, 4 | ELSEWHERE, 0, rle_bytes(1000, 1000, 65536))),
    ("checksums inline", dict(verify_trailer=1, ck_inline=1), (TWO_PASS, 1, 0, 4, 0, 0)),
    ("checksums with PRE", dict(verify_trailer=1, hint0=0xFFFFFFFF), (PRE, 1, 0, 4, pre_bytes(1000, 65536), 0)),
]


def test_plan_table(emu):
    """Every row of decode_launch()'s plan table through the product's chooser (zxc_dev_plan_choose), downgrades included."""
    L = emu.lib
    L.emu_decode_plan_choose.argtypes = [C.POINTER(PlanIn), C.POINTER(Plan)]
    for name, kw, want in PLAN_TABLE:
        p = Plan()
        L.emu_decode_plan_choose(C.byref(PlanIn(**{**BASE, **kw})), C.byref(p))
        got = (p.kind, p.ordered, p.ck_apart, p.trailer_bytes, p.pscratch_bytes, p.rscratch_bytes)
        assert got == want, (name, got, want)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 255, 16896])
def test_order_buffer_layout(emu, n):
    """zxc_dev_ord_layout: every region of a stream's launch-order buffer inside it, no two overlapping, the section records
    (zxc_dev_sec_t, 32 bytes) 32-byte aligned."""
    L = emu.lib
    L.emu_ord_layout.argtypes = [C.c_uint32, C.POINTER(OrdLayout)]
    at = OrdLayout()
    L.emu_ord_layout(n, C.byref(at))
    regions = {  # byte ranges
        "histogram": (0, 128 * 4), "list": (at.list * 4, (at.list + 2 + n) * 4), "order": (at.order * 4, (at.order + n) * 4),
        "ctl": (at.ctl * 4, (at.ctl + 32) * 4), "pre_entries": (at.pre_ent * 4, (at.pre_ent + n) * 4),
        "secs": (at.secs * 4, at.secs * 4 + 6 * n * 32), "pre": (at.pre * 4, at.pre * 4 + n * 16), "ck_bad": (at.ck_bad * 4, at.ck_bad * 4 + n)}
    assert at.list == 128  # (the list's count and cursor are the words 128, 129 the shim zeroes with the histogram)
    for k, (a, b) in regions.items():
        assert 0 <= a < b <= at.words * 4, (n, k, a, b, at.words)
    spans = sorted(regions.items(), key=lambda kv: kv[1])
    for (k0, (a0, b0)), (k1, (a1, b1)) in zip(spans, spans[1:]):
        assert b0 <= a1, (n, k0, k1, b0, a1)
    assert (at.secs * 4) % 32 == 0, (n, at.secs)
