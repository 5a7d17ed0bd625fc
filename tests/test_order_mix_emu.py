"""The launch-order pass with the position transform (zxc_dev_order_mix) on the CPU wave emulator: the real order kernels at a
small residency, a launch just above 2 x residency + rows, where the head's last column is ragged and the head meets the tail,
over a mixed archive (RAW, GHI, GLO, RLE-literal and one malformed block). order[] is a permutation, and every block has the
oracle's bytes and status under the two-pass plan and under the FULL plan. No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import decode_plan_cases as P
from conftest import ROOT

SLOTS = 8
BS = 4096


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("order_mix_emu") / "libzxc_order_mix_emu.so")
    w = os.path.join(ROOT, "tests", "wave_emu")
    subprocess.run(["/opt/rocm/lib/llvm/bin/clang++", "-O1", "-g", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-I" + w,
                    "-I" + os.path.join(ROOT, "zxc_amd", "csrc"), "-include", os.path.join(w, "emu_lds_hooks.h"), "-Wno-unused-function",
                    "-Wno-unused-value", "-Wno-macro-redefined", "-shared", "-o", so, os.path.join(w, "wave_emu.cpp"),
                    os.path.join(ROOT, "tests", "order_mix", "emu_order_mix.cpp")], check=True)
    L = C.CDLL(so)
    L.emu_order_mix_decode.restype = C.c_int
    L.emu_order_mix_decode.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32,
                                       C.c_uint32, C.c_int, C.c_void_p, C.c_int]
    return L


@pytest.fixture(scope="module")
def rows():
    src = open(os.path.join(ROOT, "zxc_amd", "csrc", "zxc_dev.h")).read()
    return int(src.split("#define ZXC_DEV_ORDER_MIX_ROWS ")[1].split("u")[0])


@pytest.fixture(scope="module")
def case(oracle, ref, rows):
    rnd = np.random.default_rng(11).integers(0, 256, 4 * BS, dtype=np.uint8).tobytes()  # incompressible: RAW blocks
    pieces = []
    for level in (1, 3, 5):
        data = P.corpus_bytes(22 * BS - 13, seed=5 + level) + rnd
        comp = P.ref_archive(ref, data, level, BS)
        jobs, bs, ck = P.seek_jobs(oracle, comp)
        assert bs == BS and not ck
        pieces.append((comp, jobs))
    r = P.rle_mix_case(oracle, ref, 8, 0)
    pieces.append((r.comp, r.jobs))
    comp, jobs = P.concat(*pieces)
    comp = bytearray(comp)
    comp[int(jobs["comp_off"][30])] = 7  # no such block type
    comp = bytes(comp)
    c = P.make_case(oracle, comp, jobs, BS, False, "order mix", hit=(30,))
    P.require(c, rle=8, failed=1, n_jobs=2 * SLOTS + rows + 1)
    t, _, _ = P.block_fields(c.comp, c.jobs)
    assert (t == 0).sum() >= 4 and (t == 1).sum() >= 8 and (t == 2).sum() >= 8, "RAW, GLO and GHI blocks"
    head = c.n - 2 * SLOTS
    assert rows < head < 2 * rows and head % rows, "one full column and a ragged one in front of the tail"
    return c


def _run(emu, case, slots, full_plan):
    size = P.guarded_layout(case)
    out = C.create_string_buffer(P.canary(size).tobytes(), size)
    st = np.full(case.n, -999, dtype=np.int32)
    order = np.full(case.n, 0xFFFFFFFF, dtype=np.uint32)
    jobs = np.ascontiguousarray(case.jobs)
    pads = emu.emu_order_mix_decode(case.comp, len(case.comp), jobs.ctypes.data, case.n, out, size, st.ctypes.data, BS, slots,
                                    int(full_plan), order.ctypes.data, int(case.checksum))
    assert pads == 0, "a store landed outside the output buffer"
    assert np.array_equal(np.sort(order), np.arange(case.n, dtype=np.uint32)), "order[] is not a permutation"
    P.check_guarded(case, np.frombuffer(out.raw, dtype=np.uint8), st, what=f"slots {slots} {'FULL' if full_plan else 'two-pass'}")
    return order


@pytest.mark.parametrize("full_plan", [False, True], ids=["two_pass", "full"])
def test_mixed_order_decodes_every_block(emu, case, full_plan):
    sorted_order = _run(emu, case, 0, full_plan)
    mixed = _run(emu, case, SLOTS, full_plan)
    assert np.array_equal(mixed[-2 * SLOTS:], sorted_order[-2 * SLOTS:]), "the tail keeps the sorted order"
    assert not np.array_equal(mixed, sorted_order), "the head was not mixed"
    assert np.array_equal(_run(emu, case, case.n, full_plan), sorted_order), "a launch of <= 2 x residency blocks is left alone"


@pytest.fixture(scope="module")
def ck_case(oracle, ref, rows):
    c = P.level_case(oracle, ref, 3, BS, (2 * SLOTS + rows + 9) * BS - 13, checksum=True, n_hit=6, label="order mix ck")
    P.require(c, failed=2, n_jobs=2 * SLOTS + rows + 1)
    assert (c.n - 2 * SLOTS) % rows
    return c


def test_checksum_kernel_walks_the_mixed_order(emu, ck_case):
    """Checksums apart: zxc_block_checksum_kernel finds sorted position s in the mixed order[] and every block keeps its verdict."""
    sorted_order = _run(emu, ck_case, 0, False)
    assert not np.array_equal(_run(emu, ck_case, SLOTS, False), sorted_order)
