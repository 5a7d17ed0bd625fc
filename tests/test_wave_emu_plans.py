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
