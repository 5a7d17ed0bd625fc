"""zxc_mi355x_seekable_open_device / zxc_mi355x_decompress_ranges_device without a GPU: the four symbols, every synchronous argument
check in its stated order (the device pointers below are never dereferenced), the index- and work-size arithmetic, and the rules the
kernels run (zxc_amd/csrc/zxc_ranges.h), compiled here with the host C compiler and driven over every golden archive and, where the
reference is built, over archives it writes: the index is accepted exactly when zxc_seekable_open accepts and holds its offsets, the
jobs of a range are Seekable.plan()'s, and a complete emulation of the call fed with the oracle decoder's blocks gives the oracle's
range result and bytes, with nothing written outside the valid ranges."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import cshim
from conftest import GOLDEN
from devtest import ERR

FAKE_SRC, FAKE_IDX, FAKE_RNG, FAKE_DST, FAKE_WORK, FAKE_RES = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
BAD_BLOCK_SIZES = (0, 1000, 2048, 4095, 5000, 3 << 12, 1 << 22)
BLOCK_SIZES = (4096, 65536, 1 << 19, 1 << 21)
JOB_BYTES, WORK_FIXED = 44, 1536  # the stated bound: n J (block_size + 64) + 44 n J + 1536
CANARY = 0xC3


@pytest.fixture(scope="module")
def L(product):
    L = product.lib()
    assert hasattr(L, "zxc_mi355x_decompress_ranges_device"), "libzxc_mi355x.so does not export zxc_mi355x_decompress_ranges_device"
    return L


def _open(L, n=1000, bs=65536, mb=10, src=FAKE_SRC, idx=FAKE_IDX, isz=None):
    isz = int(L.zxc_mi355x_seekable_index_size(mb)) if isz is None else isz
    return L.zxc_mi355x_seekable_open_device(src, n, bs, mb, idx, isz, None)


def _ws(L, n, max_len, bs):
    return int(L.zxc_mi355x_decompress_ranges_device_work_size(n, max_len, bs))


def _call(L, n=8, max_len=100000, bs=65536, cap=1 << 20, src=FAKE_SRC, idx=FAKE_IDX, rng=FAKE_RNG, dst=FAKE_DST, work=FAKE_WORK, ws=None,
          res=FAKE_RES):
    ws = max(_ws(L, n, max_len, bs), 1) if ws is None else ws
    return L.zxc_mi355x_decompress_ranges_device(src, 1000, idx, rng, n, max_len, dst, cap, bs, work, ws, res, None)


def test_symbols_exported(product):
    L = product.lib()
    for sym in ("zxc_mi355x_seekable_index_size", "zxc_mi355x_seekable_open_device", "zxc_mi355x_decompress_ranges_device_work_size",
                "zxc_mi355x_decompress_ranges_device"):
        assert hasattr(L, sym), sym
    for name in ("RANGE_DTYPE", "seekable_index_size", "seekable_open_device", "decompress_ranges_device_work_size",
                 "decompress_ranges_device"):
        assert hasattr(product, name), name
    assert product.RANGE_DTYPE.itemsize == 24 and product.RANGE_DTYPE.names == ("offset", "len", "dst_off")


def test_open_each_synchronous_error_and_their_order(L):
    assert _open(L, src=None) == ERR["NULL_INPUT"]
    assert _open(L, idx=None) == ERR["NULL_INPUT"]
    for n in (0, 1, 28, 43):
        assert _open(L, n=n) == ERR["SRC_TOO_SMALL"], n
    for bad in BAD_BLOCK_SIZES:
        assert _open(L, bs=bad) == ERR["BAD_BLOCK_SIZE"], bad
    for off in (1, 4, 8, 15):
        assert _open(L, idx=FAKE_IDX + off) == ERR["GPU_UNSUPPORTED"], off
    for mb in (0, 1, 1000, (1 << 32) - 1):
        assert _open(L, mb=mb, isz=int(L.zxc_mi355x_seekable_index_size(mb)) - 1) == ERR["MEMORY"], mb
    # each call breaks one rule and every later one; the earliest is reported
    assert _open(L, src=None, n=5, bs=5000, idx=FAKE_IDX + 1, isz=0) == ERR["NULL_INPUT"]
    assert _open(L, n=5, bs=5000, idx=FAKE_IDX + 1, isz=0) == ERR["SRC_TOO_SMALL"]
    assert _open(L, bs=5000, idx=FAKE_IDX + 1, isz=0) == ERR["BAD_BLOCK_SIZE"]
    assert _open(L, idx=FAKE_IDX + 1, isz=0) == ERR["GPU_UNSUPPORTED"]
    assert _open(L, isz=0) == ERR["MEMORY"]


def test_ranges_each_synchronous_error_and_their_order(L):
    for k in ("src", "idx", "work", "res", "rng", "dst"):
        assert _call(L, **{k: None}) == ERR["NULL_INPUT"], k
    for bad in BAD_BLOCK_SIZES:
        assert _call(L, bs=bad, ws=1 << 40) == ERR["BAD_BLOCK_SIZE"], bad
    for off in (1, 4, 8, 15):
        assert _call(L, dst=FAKE_DST + off) == ERR["GPU_UNSUPPORTED"], off
    assert _call(L, n=1 << 20, max_len=1 << 30, bs=4096, ws=1 << 62) == ERR["MEMORY"]  # 2^20 x (2^18 + 1) jobs
    assert _call(L, n=1, max_len=1 << 63, bs=4096, ws=1 << 62) == ERR["MEMORY"]
    for n, ml, bs in ((1, 1, 4096), (8, 100000, 65536), (20000, 3 << 16, 65536)):
        assert _call(L, n=n, max_len=ml, bs=bs, ws=_ws(L, n, ml, bs) - 1) == ERR["MEMORY"], (n, ml, bs)
    assert _call(L, src=None, bs=5000, dst=FAKE_DST + 1, ws=0) == ERR["NULL_INPUT"]
    assert _call(L, bs=5000, dst=FAKE_DST + 1, ws=0) == ERR["BAD_BLOCK_SIZE"]
    assert _call(L, dst=FAKE_DST + 1, ws=0) == ERR["GPU_UNSUPPORTED"]
    assert _call(L, ws=0) == ERR["MEMORY"]
    # nothing to do is fine, with or without a device and a range table; the argument checks still come first
    assert _call(L, n=0, rng=None) == 0
    assert _call(L, n=0, cap=0, dst=None) == 0
    assert _call(L, n=0, work=None) == ERR["NULL_INPUT"]
    assert _call(L, n=0, ws=0) == ERR["MEMORY"]


def test_valid_arguments_without_a_device(product, L):
    """What remains after the argument checks is the device check. Only on a machine without a device are the calls made (elsewhere
    these pointers would reach a kernel)."""
    if product.lib().zxc_mi355x_device_count() == 0:
        assert _open(L) == ERR["GPU_UNAVAILABLE"]
        assert _open(L, n=44, bs=4096, mb=0) == ERR["GPU_UNAVAILABLE"]
        assert _call(L) == ERR["GPU_UNAVAILABLE"]
        assert _call(L, cap=0, dst=None) == ERR["GPU_UNAVAILABLE"]
        with pytest.raises(product.ZxcError) as e:
            product.seekable_open_device(FAKE_SRC, 1000, 65536, 10, FAKE_IDX, 1 << 20)
        assert e.value.code == ERR["GPU_UNAVAILABLE"]


def test_python_binding_raises(product):
    with pytest.raises(product.ZxcError) as e:
        product.seekable_open_device(FAKE_SRC, 1000, 65536, 10, FAKE_IDX, 8)
    assert e.value.code == ERR["MEMORY"]
    with pytest.raises(product.ZxcError) as e:
        product.seekable_open_device(0, 1000, 65536, 10, FAKE_IDX, 1 << 20)
    assert e.value.code == ERR["NULL_INPUT"]
    with pytest.raises(product.ZxcError) as e:
        product.decompress_ranges_device(FAKE_SRC, 1000, FAKE_IDX, FAKE_RNG, 4, 1000, FAKE_DST, 1 << 20, 5000, FAKE_WORK, 1 << 30, FAKE_RES)
    assert e.value.code == ERR["BAD_BLOCK_SIZE"]
    with pytest.raises(product.ZxcError) as e:
        product.decompress_ranges_device(FAKE_SRC, 1000, FAKE_IDX, FAKE_RNG, 4, 1000, FAKE_DST, 1 << 20, 4096, FAKE_WORK, 1, FAKE_RES)
    assert e.value.code == ERR["MEMORY"]
    assert product.decompress_ranges_device_work_size(4, 1000, 5000) == 0
    assert product.decompress_ranges_device_work_size(4, 1000, 4096) > 0
    assert product.seekable_index_size(0) == 72 and product.seekable_index_size(100) == 64 + 8 * 101


def test_index_and_work_size(L):
    prev = 0
    for mb in (0, 1, 2, 1023, 1024, 1025, 1 << 20, (1 << 32) - 1):
        w = int(L.zxc_mi355x_seekable_index_size(mb))
        assert w == 64 + 8 * (mb + 1) and w > prev
        prev = w
    for bs in BLOCK_SIZES:
        for n in (0, 1, 7, 300, 20000):
            prev = 0
            for ml in sorted((0, 1, 100, bs - 1, bs, bs + 1, 2 * bs, 3 * bs + 5, 1 << 22)):
                w = _ws(L, n, ml, bs)
                J = (ml - 1) // bs + 2 if ml else 1
                assert w > 0 and w >= prev, (bs, n, ml)
                assert w >= n * J * (bs + 32 + JOB_BYTES), (bs, n, ml)
                assert w <= n * J * (bs + 64) + JOB_BYTES * n * J + WORK_FIXED, (bs, n, ml, w)
                prev = w
        assert _ws(L, 10, bs, bs) <= _ws(L, 11, bs, bs)
    for bad in BAD_BLOCK_SIZES:
        assert _ws(L, 10, 1000, bad) == 0, bad
    assert _ws(L, 1 << 20, 1 << 30, 4096) == 0 and _ws(L, 1, 1 << 63, 4096) == 0  # more jobs than a launch counts
    assert _ws(L, (1 << 31) - 2, 0, 4096) > 0 and _ws(L, (1 << 31) - 1, 0, 4096) == 0


# ---------------------------------------------------------------- the shared rules, run on the CPU
class Index(C.Structure):  # zr_index_t
    _fields_ = [("status", C.c_int32), ("nb", C.c_uint32), ("total", C.c_uint64), ("file_ck", C.c_uint32), ("dict_id", C.c_uint32),
                ("block_size", C.c_uint32), ("seek", C.c_uint32), ("eof_at", C.c_uint64), ("rsv", C.c_uint64 * 3)]


class Range(C.Structure):  # zxc_dev_range_t
    _fields_ = [("offset", C.c_uint64), ("len", C.c_uint64), ("dst_off", C.c_uint64)]


class Job(C.Structure):  # zxc_dev_job_t
    _fields_ = [("comp_off", C.c_uint64), ("out_off", C.c_uint64), ("comp_size", C.c_uint32), ("out_len", C.c_uint32)]


class Copy(C.Structure):  # zr_copy_t
    _fields_ = [("dst_at", C.c_uint64), ("from_", C.c_uint32), ("n", C.c_uint32)]


class Shape(C.Structure):  # zr_shape_t
    _fields_ = [(n, C.c_uint32) for n in ("J", "n_jobs", "slot_stride", "copy_chunks")] + \
               [(n, C.c_uint64) for n in ("o_jobs", "o_status", "o_copy", "o_stage", "bytes")]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    S = cshim.build_shim(tmp_path_factory, "ranges", "ranges/ranges_shim.c")
    for f in ("t_index_hdr_size", "t_copy_size", "t_shape_size", "t_range_size"):
        getattr(S, f).restype = C.c_size_t
    assert (S.t_index_hdr_size(), S.t_copy_size(), S.t_shape_size(), S.t_range_size()) == (64, 16, C.sizeof(Shape), 24)
    assert C.sizeof(Index) == 64 and C.sizeof(Copy) == 16 and C.sizeof(Range) == 24
    S.t_index_size.restype = C.c_uint64
    S.t_index_size.argtypes = [C.c_uint32]
    S.t_open.restype = None
    S.t_open.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
    S.t_shape.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(Shape)]
    S.t_job.restype = None
    S.t_job.argtypes = [C.c_void_p, C.POINTER(Range), C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64,
                        C.c_uint64, C.POINTER(Job), C.POINTER(Copy)]
    S.t_direct.argtypes = [C.POINTER(Range), C.c_uint64, C.c_uint32]
    S.t_verdict.restype = C.c_int64
    S.t_verdict.argtypes = [C.c_void_p, C.POINTER(Range), C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32]
    return S


def _golden_archives():
    out = []
    for d in ("conformance/valid", "conformance/invalid", "format", "synth"):
        p = os.path.join(GOLDEN, d)
        if os.path.isdir(p):
            out += [f"{d}/{f}" for f in sorted(os.listdir(p)) if f.endswith(".zxc")]
    return out


def _bs_of(comp):
    lg = comp[5] if len(comp) > 5 else 0
    return 1 << lg if 12 <= lg <= 21 else 65536


def _open_index(shim, comp, bs, max_blocks):
    """-> (Index header copy, offsets list or None, raw index buffer)"""
    buf = (C.c_uint8 * int(shim.t_index_size(max_blocks)))()
    C.memset(buf, 0xEE, len(buf))
    shim.t_open(comp, len(comp), bs, max_blocks, buf)
    ix = Index.from_buffer_copy(bytes(buf[:64]))
    offs = None
    if ix.status == 0:
        offs = list(np.frombuffer(bytes(buf), dtype="<u8", offset=64, count=ix.nb + 1))
    return ix, offs, buf


def _host_opens(product, comp):
    try:
        s = product.Seekable(comp)
    except product.ZxcError:
        return None
    return s


def _max_blocks(comp, bs):
    total = int.from_bytes(comp[-12:-4], "little") if len(comp) >= 12 else 0
    return min(-(-total // bs), 1 << 20)


def _check_open(shim, product, oracle, comp, what):
    """(a): accepted exactly when the host opens; then the host's offsets. -> (ix, offs, buf) or None"""
    bs = _bs_of(comp)
    s = _host_opens(product, comp)
    if len(comp) < 44:
        assert s is None, what
        return None
    mb = _max_blocks(comp, bs)
    ix, offs, buf = _open_index(shim, comp, bs, mb)
    if s is None:
        assert ix.status < 0 and offs is None, (what, ix.status)
        return None
    try:
        assert ix.status == 0, (what, ix.status)
        plan = s.plan()
        assert ix.nb == s.num_blocks and ix.total == s.decompressed_size, what
        assert offs[:-1] == [int(x) for x in plan["comp_off"]], what
        assert [offs[i + 1] - offs[i] for i in range(ix.nb)] == [int(x) for x in plan["comp_size"]], what
    finally:
        s.close()
    t = oracle.seek_table(comp)
    assert t is not None and offs == [int(x) for x in t["comp_offsets"]], what
    assert (ix.file_ck, ix.dict_id, ix.block_size) == (int(bool(t["has_checksum"])), t["dict_id"], bs), what
    return ix, offs, buf


def _tampered(comp, nb):
    first_entry = len(comp) - 12 - 4 * nb
    for at, delta in ((first_entry, 1), (first_entry + 4 * (nb - 1), 4), (first_entry - 1, 1), (first_entry - 5, 4)):
        bad = bytearray(comp)
        bad[at] = (bad[at] + delta) & 0xFF
        yield at, bytes(bad)


def _ranges_for(total, bs, nb, rng, cap):
    """the seeded list of (offset, len, dst_off): half with dst_off = offset (mod 16), half without; destinations do not overlap"""
    want = [(0, total), (0, 1), (total - 1, 1), (0, 0), (total, 0), (total + 5, 0), (total, 1), (total - 1, 2), (total + 1, 1),
            (min(7, total - 1), min(100, total - min(7, total - 1)))]
    if nb >= 2:
        want += [(bs - 3, 6), (bs, min(bs, total - bs)), (bs - 1, min(bs + 2, total - bs + 1)), (0, bs), (0, bs + 32), (0, bs + 31)]
    if nb >= 4:
        want += [(bs + 16, 2 * bs + 100), (5, 3 * bs), (2 * bs, bs + 40), (bs - 16, 2 * bs + 64)]
    for _ in range(12):
        a = rng.randrange(total)
        want.append((a, rng.randrange(1, min(total - a, 5 * bs) + 1)))
    out, at = [], 0
    for i, (a, n) in enumerate(want):
        at = (at + 15) // 16 * 16 + 16 * rng.randrange(3)   # a gap in front of every destination
        d = at + ((a & 15) if i % 2 == 0 else ((a & 15) + 1 + rng.randrange(15)) % 16)
        out.append((a, n, d))
        at = d + n
    max_len = max(n for a, n, d in out if a + n <= total)
    out.append((0, min(total, max_len) + 1, at + 32))              # len > max_len
    out.append((0, min(total, 50), cap - 10))                       # passes the capacity
    out.append((0, 1, cap + 1))                                     # starts behind it
    out.append((1, 1, (1 << 64) - 1))                               # dst_off + len wraps
    return out, max_len


def _emulate(shim, oracle, comp, ix_buf, ranges, max_len, cap, bs, dst_rel=1 << 40):
    """the call as the kernels make it: plan, decode (the oracle's block decoder), copy-out, verdict.
    -> (results, destination bytearray of cap + 4096 bytes, jobs per range)"""
    sh = Shape()
    assert shim.t_shape(len(ranges), max_len, bs, C.byref(sh)) == 0
    J = sh.J
    dst = bytearray([CANARY]) * (cap + 4096)
    results, all_jobs = [], []
    for r, (a, n, d) in enumerate(ranges):
        rg = Range(a, n, d)
        status = (C.c_int32 * J)()
        jobs = []
        for j in range(J):
            job, cp = Job(), Copy()
            i = r * J + j
            shim.t_job(ix_buf, C.byref(rg), j, i, len(comp), max_len, cap, bs, dst_rel, 0, C.byref(job), C.byref(cp))
            assert job.out_len == bs and job.out_off % 16 == 0
            if job.comp_size == 0:   # an empty job: answered with an error, nothing read or written
                status[j] = ERR["SRC_TOO_SMALL"]
                assert cp.n == 0
                continue
            jobs.append((job.comp_off, job.comp_size))
            rc, out = oracle.decode_block(comp[job.comp_off: job.comp_off + job.comp_size], bs)
            status[j] = rc
            if job.out_off >= dst_rel:   # straight into the destination: the slot and 32 bytes behind it belong to the range
                place = job.out_off - dst_rel
                assert cp.n == 0 and place % 16 == 0 and d <= place and place + bs + 32 <= d + n, (a, n, d, j)
                dst[place: place + len(out[:bs])] = out[:bs]
            else:
                assert job.out_off == i * sh.slot_stride and cp.n > 0 and cp.from_ + cp.n <= bs
                assert d <= cp.dst_at and cp.dst_at + cp.n <= d + n, (a, n, d, j)
                if rc >= cp.from_ + cp.n:
                    dst[cp.dst_at: cp.dst_at + cp.n] = out[cp.from_: cp.from_ + cp.n]
        results.append(int(shim.t_verdict(ix_buf, C.byref(rg), J, status, len(comp), max_len, cap, bs)))
        all_jobs.append(jobs)
    return results, dst, all_jobs


def _check_ranges(shim, product, oracle, comp, ix, buf, what, seed):
    bs, total, nb = ix.block_size, ix.total, ix.nb
    rng = random.Random(seed)
    probe, _ = _ranges_for(total, bs, nb, rng, 1 << 62)
    cap = max(d + n for a, n, d in probe[:-4] if a + n <= total) + 64
    ranges, max_len = _ranges_for(total, bs, nb, random.Random(seed), cap)
    results, dst, jobs = _emulate(shim, oracle, comp, buf, ranges, max_len, cap, bs)
    s = product.Seekable(comp) if ix.dict_id == 0 else None
    written = bytearray(len(dst))
    for (a, n, d), got, jb in zip(ranges, results, jobs):
        w = (what, a, n, d)
        if n == 0:
            want = 0
        elif n > max_len or d > cap or n > cap - d:
            want = ERR["DST_TOO_SMALL"]
        else:
            want, data = oracle.seekable_range(comp, a, n)
        assert got == want, (w, got, want)
        if got != n or n == 0:
            if got < 0 and got in (ERR["DST_TOO_SMALL"], ERR["SRC_TOO_SMALL"], ERR["DICT_REQUIRED"]):
                assert jb == [], w   # refused before any block: every job of the range is empty
            continue
        assert bytes(dst[d: d + n]) == data, w
        written[d: d + n] = b"\1" * n
        first, count = a // bs, (a + n - 1) // bs - a // bs + 1   # (b): the jobs are the host's
        plan = s.plan(first, count)
        assert jb == [(int(x), int(y)) for x, y in zip(plan["comp_off"], plan["comp_size"])], w
    if s:
        s.close()
    outside = bytes(b for b, wr in zip(dst, written) if not wr)
    assert outside == bytes([CANARY]) * len(outside), what   # (c): nothing outside the valid ranges


@pytest.mark.parametrize("rel", _golden_archives())
def test_rules_on_golden_archive(shim, product, oracle, rel):
    comp = open(os.path.join(GOLDEN, rel), "rb").read()
    opened = _check_open(shim, product, oracle, comp, rel)
    if opened is None:
        return
    ix, offs, buf = opened
    for at, bad in _tampered(comp, ix.nb):
        assert _host_opens(product, bad) is None, (rel, at)
        ix_b, offs_b, _ = _open_index(shim, bad, ix.block_size, ix.nb)
        assert ix_b.status == ERR["CORRUPT_DATA"] and offs_b is None, (rel, at, ix_b.status)
    # the additions: a block size other than the header's, one block more than the index holds
    other = 4096 if ix.block_size != 4096 else 8192
    assert _open_index(shim, comp, other, 1 << 16)[0].status == ERR["BAD_BLOCK_SIZE"], rel
    assert _open_index(shim, comp, ix.block_size, ix.nb - 1)[0].status == ERR["MEMORY"], rel
    _check_ranges(shim, product, oracle, comp, ix, buf, rel, seed=len(comp))


def test_some_golden_archive_opens(shim, product, oracle):
    n = 0
    for rel in _golden_archives():
        comp = open(os.path.join(GOLDEN, rel), "rb").read()
        n += _host_opens(product, comp) is not None
    assert n >= 3, n


def test_an_entry_above_4_mib_is_refused(shim, product):
    """the documented departure: a table the host's open accepts, with one entry of 4 MiB + 8 that cannot belong to a legal block"""
    M = (1 << 64) - 1

    def h8(b7):
        h = int.from_bytes(b7 + b"\0", "little") ^ 0x9E3779B97F4A7C15
        h ^= (h << 13) & M
        h ^= h >> 7
        h ^= (h << 17) & M
        return ((h >> 32) ^ h) & 0xFF

    def blk(t, csz):
        b = bytes([t, 0, 0]) + csz.to_bytes(4, "little")
        return b + bytes([h8(b)])

    comp = open(os.path.join(GOLDEN, "conformance/valid/seekable_4blocks.zxc"), "rb").read()
    bs = _bs_of(comp)
    s = product.Seekable(comp)
    nb, total, plan = s.num_blocks, s.decompressed_size, s.plan()
    s.close()
    sizes = [int(x) for x in plan["comp_size"]]
    body = comp[16: 16 + sum(sizes)]
    for big, ok in (((1 << 22) + 8, False), (1 << 22, True)):
        pad = big - sizes[-1]   # the last block's entry grows over padding that open never looks at
        entries = sizes[:-1] + [big]
        arc = comp[:16] + body + bytes(pad) + blk(255, 0) + blk(254, 4 * nb) + b"".join(e.to_bytes(4, "little") for e in entries) + \
            total.to_bytes(8, "little") + bytes(4)
        h = _host_opens(product, arc)
        assert h is not None, big
        h.close()
        ix, offs, _ = _open_index(shim, arc, bs, nb)
        assert (ix.status == 0) == ok and (ok or ix.status == ERR["CORRUPT_DATA"]), (big, ix.status)


@pytest.mark.parametrize("bs", [4096, 65536])
@pytest.mark.parametrize("blocks", [1, 2, 5, 40])
def test_rules_on_reference_archives(shim, product, oracle, ref, bs, blocks):
    from zxc_amd import corpus
    rng = np.random.default_rng(bs + blocks)
    n = (blocks - 1) * bs + 1 + int(rng.integers(0, bs))
    for name, data in (("text", corpus.synth_text(n, seed=blocks)), ("random", rng.integers(0, 256, n, dtype=np.uint8).tobytes())):
        for checksum in (False, True):
            what = (name, bs, blocks, checksum)
            comp = ref.compress(data[:n], 3, bs, True, checksum)
            opened = _check_open(shim, product, oracle, comp, what)
            assert opened is not None and opened[0].nb == blocks, what
            ix, offs, buf = opened
            for at, bad in _tampered(comp, ix.nb):
                assert _open_index(shim, bad, bs, ix.nb)[0].status == ERR["CORRUPT_DATA"], (what, at)
            _check_ranges(shim, product, oracle, comp, ix, buf, what, seed=blocks * 131 + bs)
            if not checksum and name == "text":
                assert oracle.seekable_range(comp, 0, n)[1] == data[:n]
    # an archive that is not seekable has no table to open
    plain = ref.compress(data[:n], 3, bs, False, False)
    assert _host_opens(product, plain) is None and _open_index(shim, plain, bs, blocks)[0].status == ERR["CORRUPT_DATA"]


def test_a_direct_slot_never_leaves_its_destination(shim):
    """(d): exhaustively over small (offset, len, dst_off) at 4 KiB blocks: a block goes straight into the destination exactly when
    all of it is wanted, its place is 16-byte aligned and the slot plus 32 bytes end inside the range's own destination"""
    bs, n_direct = 4096, 0
    offsets = [0, 1, 15, 16, 17, 4000, 4095, 4096, 4097, 8191, 8192]
    lens = [1, 31, 32, 4095, 4096, 4097, 4096 + 31, 4096 + 32, 4096 + 33, 8192, 8192 + 32, 8192 + 48, 12288 + 31, 12288 + 32, 16384 + 100]
    for a in offsets:
        for n in lens:
            for d in list(range(0, 34)) + [4096, 4097]:
                rg = Range(a, n, d)
                for b in range(0, (a + n - 1) // bs + 2):
                    got = shim.t_direct(C.byref(rg), b, bs)
                    place = d + b * bs - a
                    want = a <= b * bs and (b + 1) * bs <= a + n and place % 16 == 0 and place + bs + 32 <= d + n
                    assert bool(got) == bool(want), (a, n, d, b)
                    if got:
                        n_direct += 1
                        assert d <= place and place + bs + 32 <= d + n
    assert n_direct > 100
