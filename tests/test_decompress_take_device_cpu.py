"""The take session (zxc_mi355x_decompress_begin_device / _begin_dict_device / _take_device / _end_device) without a GPU: the five
symbols and the Python names, every synchronous argument check in its stated order (the device pointers below are never
dereferenced), the work-size arithmetic against the bound the header states, and the rules the entry points and kernels run
(zxc_amd/csrc/zxc_take.h on top of zxc_container.h), compiled here with the host C compiler. Goldens, and archives the unmodified
reference wrote, are taken back by a session replayed on the host (tests/take/take_replay.h: the real container stages, the plan
of every chunk, a stand-in decoder that copies each block's expected bytes and then scribbles 32 bytes behind them, the copies,
events and verdict) at many cut points and piece alignments, every piece with canaries around it: the pieces concatenate to the
expected bytes and the result is the reference decoder's. The same replay runs under AddressSanitizer and UBSan in a stand-alone
program."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import cshim
from conftest import GOLDEN
from cpu_take import BAD_BLOCK_SIZES, BAD_PLAN, FAKE_DST, FAKE_RES, FAKE_SRC, FAKE_WORK, Blocks, _goldens, _host_walk
from cshim import ref as _ref
from devtest import ERR
from zxc_amd.api import _DecompressOpts, _DevDict, _DevDtake as Ds  # zxc_dev_dtake_t

BLOCK_SIZES = (4096, 65536, 1 << 19, 1 << 21)
BLOCK_BYTES, TILE_BYTES, JOB_BYTES, PAD, CARRIES, WORK_FIXED = 56, 16, 48, 64, 2, 4096  # the stated bound


def _host_dict_opts():
    return cshim.host_dict(_DecompressOpts())


@pytest.fixture(scope="module")
def L(product):
    L = product.lib()
    assert hasattr(L, "zxc_mi355x_decompress_begin_device"), "libzxc_mi355x.so does not export zxc_mi355x_decompress_begin_device"
    return L


def _ws(L, n, cap, mp, bs):
    return int(L.zxc_mi355x_decompress_take_device_work_size(n, cap, mp, bs))


def _begin(L, ds="new", src=FAKE_SRC, n=1000, cap=1 << 20, mp=1 << 16, bs=65536, opts=None, work=FAKE_WORK, ws=None, dict_="none"):
    ds = Ds() if isinstance(ds, str) else ds
    if ws is None:
        ws = max(_ws(L, n, cap, mp, bs), 1)
    if isinstance(dict_, str):
        return L.zxc_mi355x_decompress_begin_device(_ref(ds), src, n, cap, mp, bs, _ref(opts), work, ws, None)
    return L.zxc_mi355x_decompress_begin_dict_device(_ref(ds), src, n, cap, mp, bs, _ref(opts), _ref(dict_), work, ws, None)


def test_symbols_and_names_exported(product):
    L = product.lib()
    for sym in ("zxc_mi355x_decompress_take_device_work_size", "zxc_mi355x_decompress_begin_device", "zxc_mi355x_decompress_begin_dict_device",
                "zxc_mi355x_decompress_take_device", "zxc_mi355x_decompress_end_device"):
        assert hasattr(L, sym), sym
    for name in ("decompress_take_device_work_size", "decompress_begin_device", "decompress_begin_dict_device", "DecompressTakeSession"):
        assert hasattr(product, name) and hasattr(product.api, name), name
    assert all(sym in product.api._PROTOTYPES for sym in ("zxc_mi355x_decompress_take_device_work_size", "zxc_mi355x_decompress_begin_device",
                                                          "zxc_mi355x_decompress_begin_dict_device", "zxc_mi355x_decompress_take_device",
                                                          "zxc_mi355x_decompress_end_device")) and hasattr(product.api, "_DevDtake")
    assert hasattr(product.api.DecompressTakeSession, "take") and hasattr(product.api.DecompressTakeSession, "end")
    assert C.sizeof(product.api._DevDtake) == 128


def test_begin_each_synchronous_error_and_their_order(L):
    for k in ("ds", "src", "work"):
        assert _begin(L, **{k: None}) == ERR["NULL_INPUT"], k
    for n in (0, 1, 27):
        assert _begin(L, n=n, ws=1 << 40) == ERR["SRC_TOO_SMALL"], n
    for bad in BAD_BLOCK_SIZES:
        assert _begin(L, bs=bad, ws=1 << 40) == ERR["BAD_BLOCK_SIZE"], bad
    assert _begin(L, mp=65535, ws=1 << 40) == ERR["BAD_BLOCK_SIZE"]                      # max_piece < block_size
    assert _begin(L, mp=0, ws=1 << 40) == ERR["BAD_BLOCK_SIZE"]
    assert _begin(L, bs=4096, mp=4096, cap=((1 << 31) - 2) * 4096 + 1, ws=1 << 62) == ERR["BAD_BLOCK_SIZE"]  # 2^31 - 1 blocks of capacity
    assert _begin(L, bs=4096, mp=4096, cap=(1 << 64) - 1, ws=1 << 62) == ERR["BAD_BLOCK_SIZE"]
    assert _begin(L, bs=4096, mp=1 << 63, ws=1 << 62) == ERR["BAD_BLOCK_SIZE"]            # more jobs in a chunk than a launch counts
    assert _begin(L, opts=_host_dict_opts(), ws=1 << 40) == ERR["GPU_UNSUPPORTED"]
    assert _begin(L, dict_=_DevDict(FAKE_SRC, None, FAKE_SRC, 65536), ws=1 << 40) == ERR["DICT_TOO_LARGE"]
    assert _begin(L, dict_=_DevDict(None, None, FAKE_SRC, 100), ws=1 << 40) == ERR["NULL_INPUT"]
    assert _begin(L, dict_=_DevDict(FAKE_SRC, None, None, 100), ws=1 << 40) == ERR["NULL_INPUT"]
    for n, cap, mp, bs in ((28, 0, 4096, 4096), (1000, 1 << 20, 1 << 16, 65536), (1 << 24, 1 << 30, 1 << 26, 4096), (28, 5, 1 << 21, 1 << 21)):
        assert _begin(L, n=n, cap=cap, mp=mp, bs=bs, ws=_ws(L, n, cap, mp, bs) - 1) == ERR["MEMORY"], (n, cap, mp, bs)
    # each call breaks one rule and every later one; the earliest is reported
    late = dict(opts=_host_dict_opts(), dict_=_DevDict(FAKE_SRC, None, FAKE_SRC, 65536), ws=0)
    assert _begin(L, src=None, n=5, bs=5000, **late) == ERR["NULL_INPUT"]
    assert _begin(L, n=5, bs=5000, **late) == ERR["SRC_TOO_SMALL"]
    assert _begin(L, bs=5000, **late) == ERR["BAD_BLOCK_SIZE"]
    assert _begin(L, mp=1, **late) == ERR["BAD_BLOCK_SIZE"]
    assert _begin(L, **late) == ERR["GPU_UNSUPPORTED"]
    assert _begin(L, dict_=late["dict_"], ws=0) == ERR["DICT_TOO_LARGE"]
    assert _begin(L, ws=0) == ERR["MEMORY"]
    ds = Ds()
    assert _begin(L, ds=ds, ws=0) == ERR["MEMORY"] and not any(ds.opaque)  # a refused begin leaves the struct alone
    junk = Ds()
    C.memset(C.byref(junk), 0xEE, C.sizeof(junk))
    assert _begin(L, ds=junk, ws=0) == ERR["MEMORY"] and all(w == 0xEEEEEEEEEEEEEEEE for w in junk.opaque)


def test_take_and_end_refuse_by_status(L):
    ds = Ds()
    assert L.zxc_mi355x_decompress_take_device(None, FAKE_DST, 10, None) == ERR["NULL_INPUT"]
    assert L.zxc_mi355x_decompress_take_device(_ref(ds), None, 10, None) == ERR["NULL_INPUT"]
    assert L.zxc_mi355x_decompress_take_device(_ref(ds), FAKE_DST, 10, None) == ERR["NULL_INPUT"]  # never begun
    assert L.zxc_mi355x_decompress_take_device(_ref(ds), None, 0, None) == ERR["NULL_INPUT"]
    assert L.zxc_mi355x_decompress_end_device(None, FAKE_RES, None) == ERR["NULL_INPUT"]
    assert L.zxc_mi355x_decompress_end_device(_ref(ds), None, None) == ERR["NULL_INPUT"]
    assert L.zxc_mi355x_decompress_end_device(_ref(ds), FAKE_RES, None) == ERR["NULL_INPUT"]       # never begun
    junk = Ds()
    C.memset(C.byref(junk), 0xEE, C.sizeof(junk))
    assert L.zxc_mi355x_decompress_take_device(_ref(junk), FAKE_DST, 10, None) == ERR["NULL_INPUT"]
    assert L.zxc_mi355x_decompress_end_device(_ref(junk), FAKE_RES, None) == ERR["NULL_INPUT"]


def test_valid_arguments_without_a_device(product, L):
    """What remains after the argument checks is the device check. Only on a machine without a device is the call made (elsewhere
    these pointers would reach a kernel)."""
    if product.lib().zxc_mi355x_device_count() == 0:
        ds = Ds()
        assert _begin(L, ds=ds) == ERR["GPU_UNAVAILABLE"] and not any(ds.opaque)
        assert _begin(L, n=28, cap=0, mp=4096, bs=4096) == ERR["GPU_UNAVAILABLE"]  # the empty-frame probe
        assert _begin(L, opts=_DecompressOpts(checksum_enabled=1), bs=4096) == ERR["GPU_UNAVAILABLE"]
        assert _begin(L, dict_=None) == ERR["GPU_UNAVAILABLE"] and _begin(L, dict_=_DevDict(None, None, None, 0)) == ERR["GPU_UNAVAILABLE"]
        assert _begin(L, dict_=_DevDict(FAKE_SRC, None, FAKE_SRC, 65535)) == ERR["GPU_UNAVAILABLE"]
        with pytest.raises(product.ZxcError) as e:
            product.decompress_begin_device(FAKE_SRC, 1000, 1 << 20, 1 << 16, 4096, FAKE_WORK, 1 << 30)
        assert e.value.code == ERR["GPU_UNAVAILABLE"]


def test_python_binding_raises(product):
    with pytest.raises(product.ZxcError) as e:
        product.decompress_begin_device(FAKE_SRC, 1000, 1 << 20, 1 << 16, 5000, FAKE_WORK, 1 << 30)
    assert e.value.code == ERR["BAD_BLOCK_SIZE"]
    with pytest.raises(product.ZxcError) as e:
        product.decompress_begin_device(FAKE_SRC, 1000, 1 << 20, 1 << 16, 4096, FAKE_WORK, 1)
    assert e.value.code == ERR["MEMORY"]
    with pytest.raises(product.ZxcError) as e:
        product.decompress_begin_device(0, 1000, 1 << 20, 1 << 16, 4096, FAKE_WORK, 1 << 30)
    assert e.value.code == ERR["NULL_INPUT"]
    with pytest.raises(product.ZxcError) as e:
        product.decompress_begin_dict_device(FAKE_SRC, 1000, 1 << 20, 1 << 16, 4096, (FAKE_SRC, 70000, 0, FAKE_SRC), FAKE_WORK, 1 << 30)
    assert e.value.code == ERR["DICT_TOO_LARGE"]
    s = product.api.DecompressTakeSession(product.api._DevDtake())  # never begun
    with pytest.raises(product.ZxcError) as e:
        s.take(FAKE_DST, 10)
    assert e.value.code == ERR["NULL_INPUT"]
    with pytest.raises(product.ZxcError) as e:
        s.end(FAKE_RES)
    assert e.value.code == ERR["NULL_INPUT"]
    assert product.decompress_take_device_work_size(1000, 1 << 30, 1 << 20, 5000) == 0
    assert product.decompress_take_device_work_size(1000, 1 << 30, 1 << 20, 4096) > 0


# ---------------------------------------------------------------- the shared rules, run on the CPU
class Shape(C.Structure):  # zt_shape_t
    _fields_ = [(n, C.c_uint32) for n in ("n_jobs", "n_tiles", "J", "slot_stride", "copy_chunks", "rsv")] + \
               [(n, C.c_uint64) for n in ("o_tile_sum", "o_tile_hash", "o_tile_bad", "o_jobs", "o_status", "o_cjobs")] + \
               [("o_carry", C.c_uint64 * 2)] + [(n, C.c_uint64) for n in ("o_slots", "bytes")]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    S = cshim.build_shim(tmp_path_factory, "take", "take/take_shim.c")
    S.t_shape_size.restype = S.t_chunk_size.restype = C.c_size_t
    assert S.t_shape_size() == C.sizeof(Shape)
    S.t_shape.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(Shape)]
    S.t_work_bound.restype = C.c_uint64
    S.t_work_bound.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
    S.t_chunk_len.restype = C.c_uint64
    S.t_chunk_len.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32]
    S.t_session.restype = C.c_int64
    S.t_session.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    S.t_head.restype = C.c_uint32
    S.t_head.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int]
    S.t_plan_check.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64]
    S.t_plan_check_range.restype = C.c_uint64
    S.t_plan_check_range.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32]
    return S


def test_work_size(product, L, shim):
    for bs in BLOCK_SIZES:
        for mp in (bs, bs + 1, 2 * bs - 1, 7 * bs, 1023 * bs, 1 << 26):
            prev = None
            for cap in sorted({0, 1, bs - 1, bs, bs + 1, 1023 * bs + 7, 1024 * bs, 1025 * bs, 1 << 30, 1 << 36}):
                w, one = _ws(L, 1000, cap, mp, bs), int(L.zxc_mi355x_decompress_device_work_size(1000, cap, bs))
                nj, J = -(-cap // bs) + 1, mp // bs + 2
                bound = BLOCK_BYTES * nj + TILE_BYTES * -(-nj // 1024) + J * (bs + PAD + JOB_BYTES) + CARRIES * (bs + PAD) + WORK_FIXED
                assert bound == int(shim.t_work_bound(cap, mp, bs))
                assert 0 < w <= bound, (bs, mp, cap, w, bound)
                assert w >= BLOCK_BYTES * nj + J * (bs + PAD + JOB_BYTES) + CARRIES * (bs + PAD), (bs, mp, cap)  # at least its parts
                sh = Shape()
                assert shim.t_shape(cap, mp, bs, C.byref(sh)) == 0 and sh.bytes == w and (sh.n_jobs, sh.J, sh.slot_stride) == (nj, J, bs + PAD)
                parts = [sh.o_tile_sum, sh.o_tile_hash, sh.o_tile_bad, sh.o_jobs, sh.o_status, sh.o_cjobs, sh.o_carry[0], sh.o_carry[1],
                         sh.o_slots, sh.bytes - 256]
                assert all(p % 256 == 0 for p in parts) and parts == sorted(parts) and parts[0] >= 256
                assert sh.o_status - sh.o_jobs >= 48 * nj and sh.o_cjobs - sh.o_status >= 8 * nj and sh.o_carry[0] - sh.o_cjobs >= 48 * J
                assert min(sh.o_carry[1] - sh.o_carry[0], sh.o_slots - sh.o_carry[1]) >= bs + PAD and sh.bytes - 256 - sh.o_slots >= J * (bs + PAD)
                assert sh.copy_chunks * 8192 >= bs + 15
                if prev is not None:  # it grows with the capacity as the one-shot call's does
                    assert abs((w - prev[0]) - (one - prev[1])) < 256 and w >= prev[0], (bs, mp, cap)
                prev = (w, one)
        assert _ws(L, 28, 10 * bs, bs, bs) == _ws(L, 1 << 30, 10 * bs, bs, bs)  # the capacity sizes the session, not the archive
    # the point of the session: a gibibyte in pieces of 64 MiB needs the index and a piece's slots, not a second destination
    assert 0 < product.decompress_take_device_work_size(1 << 29, 1 << 30, 64 << 20, 65536) < (1 << 30) // 8
    for bad in BAD_BLOCK_SIZES:  # 0 for what begin refuses
        assert _ws(L, 1000, 1 << 20, 1 << 22, bad) == 0, bad
    assert _ws(L, 27, 1 << 20, 65536, 65536) == 0 and _ws(L, 28, 1 << 20, 65536, 65536) > 0
    assert _ws(L, 1000, 1 << 20, 65535, 65536) == 0
    assert _ws(L, 1000, ((1 << 31) - 2) * 4096, 4096, 4096) > 0 and _ws(L, 1000, ((1 << 31) - 2) * 4096 + 1, 4096, 4096) == 0
    assert _ws(L, 1000, 0, 1 << 63, 4096) == 0


def test_chunk_lengths(shim):
    bs = 4096
    for mp in (bs, bs + 1, 3 * bs - 1, 8 * bs):
        for at in (0, 1, 100, bs - 1):
            for left in (1, bs - 1, mp - 1, mp, mp + 1, 5 * mp + 77):
                m = int(shim.t_chunk_len(5 * bs + at, left, mp, bs))
                assert 0 < m <= min(left, mp)
                assert m == left or (at + m) % bs == 0, (mp, at, left, m)
                assert -(-(at + m) // bs) - (1 if at else 0) <= mp // bs + 1  # the blocks a chunk decodes (not the waiting one): J keeps one more


def test_every_plan_keeps_its_promises(shim):
    """for every position in a block and every n of a range that passes three block boundaries, at block_size 4096 and piece
    addresses 0, 1, 8, 15 and 16 mod 16: every byte of the piece is written by one copy or lies in one direct block, a direct block
    is 16-aligned with its slot + 32 inside the take, a whole block that could go straight does, the chunk keeps to J jobs and
    slots (promise numbers: take_replay.h)"""
    bs = 4096
    for align in (0, 1, 8, 15, 16):
        for lo, hi in ((1, 60), (bs - 40, bs + 40), (2 * bs - 40, 2 * bs + 40), (3 * bs - 40, 3 * bs + 40)):
            bad = int(shim.t_plan_check_range(bs, lo, hi, align))
            assert bad == 0, dict(align=align, pos=bad >> 40, n=(bad >> 8) & 0xFFFFFFFF, promise=bad & 0xFF)
    for bs in (65536, 1 << 21):
        edge = (1, 31, 32, 33)
        for at in (0,) + edge + tuple(bs - e for e in edge):
            ns = set(edge)
            for k in (1, 2, 3):
                ns |= {k * bs - at + d for d in (-33, -32, -31, -1, 0, 1, 31, 32, 33)} | {k * bs + d for d in (-1, 0, 1, 32)}
            for n in sorted(x for x in ns if x > 0):
                for align in (0, 1, 8, 15, 16):
                    for room in (n, n + 31, n + 32, n + 33):
                        assert shim.t_plan_check(3 * bs + at, n, room, align, bs, max(n, bs)) == 0, (bs, at, n, align, room)


# ---------------------------------------------------------------- host replay
def _cuts(total, bs, rng):
    """name -> (take lengths, max_piece): the patterns of the append test, and many takes inside one block"""
    whole = max(total, bs)
    out = {"one": ([total], whole),
           "at block boundaries": ([bs] * (total // bs) + ([total % bs] if total % bs else []), bs),
           "the chunk loop": ([total], bs),
           "the chunk loop behind a carry": ([min(total, 5), total - min(total, 5)], 2 * bs + 17)}
    small = [min(111, bs // 3)] * min(40, total // min(111, bs // 3))
    out["many takes inside one block"] = (small + [total - sum(small)], whole)
    if total > bs:
        out["around a boundary with nothing between"] = ([bs - 1, 0, 2, 0, 0, total - bs - 1, 0], whole)
    for k in range(3):
        lens, left = [], total
        while left:
            n = min(left, rng.choice((0, 1, 16, rng.randrange(bs), bs, rng.randrange(3 * bs + 9))))
            lens.append(n)
            left -= n
        out["random %d" % k] = (lens, rng.choice((bs, 2 * bs, 3 * bs + 100, whole)))
    return out


def _session(shim, comp, bs, cap, verify, lens, max_piece, align, blocks, use_table=1, have_dict=0, dict_id=0):
    """-> (result, the pieces' bytes concatenated)"""
    ln = np.array(list(lens) + [0], dtype=np.uint64)
    out = np.zeros(cap + 1, dtype=np.uint8)
    rc = int(shim.t_session(comp, len(comp), cap, max_piece, bs, int(verify), use_table, have_dict, dict_id, blocks.bytes.ctypes.data,
                            blocks.at.ctypes.data, blocks.st.ctypes.data, blocks.n, ln.ctypes.data, len(lens), align, out.ctypes.data))
    return rc, out[:cap].tobytes()


def _check_archive(shim, oracle, comp, bs, size, seed, what, decoder=None):
    """sessions over the archive at every cut pattern, capacity and verification: the reference decoder's result and bytes"""
    rng = random.Random(seed)
    decoder = decoder or (lambda cap, verify: oracle.decompress(comp, cap, checksum=verify))
    n_sessions = 0
    for verify in (False, True):
        for cap in sorted({size, max(size - 1, 0), size + bs + 3, 0}):
            want, data = decoder(cap, verify)
            blocks = Blocks(shim, oracle, comp, bs, cap, verify)
            for k, (name, (lens, mp)) in enumerate(_cuts(cap, bs, rng).items()):
                align = (0, 1, 8, 15, 16)[(k + seed) % 5]
                rc, got = _session(shim, comp, bs, cap, verify, lens, mp, align, blocks, use_table=(k + 1) % 2)
                assert rc != BAD_PLAN, (what, name, cap, verify, align)
                assert rc == want, (what, name, cap, verify, rc, want)
                if rc >= 0:
                    assert got[:rc] == data[:rc], (what, name, cap, verify, align)
                n_sessions += 1
    return n_sessions


def test_sessions_take_the_valid_goldens_apart(shim, oracle, product):
    seen = 0
    for k, rel in enumerate(_goldens("conformance/valid")):
        comp = open(os.path.join(GOLDEN, rel), "rb").read()
        if len(comp) < 28 or not 12 <= comp[5] <= 21:
            continue
        bs, size = 1 << comp[5], product.get_decompressed_size(comp)
        exp = os.path.join(GOLDEN, rel[:-4] + ".expected")
        if os.path.exists(exp):
            size = os.path.getsize(exp)
        if size > (4 << 20):
            continue
        irregular = oracle.decompress(comp, size)[0] >= 0 and len(_host_walk(comp, comp[6] >> 7, 1 << 30)) != -(-size // bs)
        if irregular:  # (the device calls answer GPU_UNSUPPORTED where the host decodes: the one departure that changes a valid archive's result)
            continue
        seen += _check_archive(shim, oracle, comp, bs, size, k, rel)
    assert seen >= 200, seen


def test_sessions_answer_damaged_archives_as_the_reference_decoder(shim, oracle, product):
    """the invalid goldens, and a valid one truncated inside a block, with a payload byte flipped, and with a block header's check
    byte broken: no piece byte is asserted, the result is the reference decoder's and the canaries hold"""
    cases = []
    for rel in _goldens("conformance/invalid"):
        comp = open(os.path.join(GOLDEN, rel), "rb").read()
        if len(comp) >= 28 and 12 <= comp[5] <= 21:
            cases.append((rel, comp))
    good = open(os.path.join(GOLDEN, "conformance/valid/seekable_4blocks.zxc"), "rb").read()
    ck = good[6] >> 7
    walk = _host_walk(good, ck, 1 << 30)
    assert len(walk) == 4
    off, n = walk[2]
    flipped, bad_hdr = bytearray(good), bytearray(good)
    flipped[off + 8 + (n - 8 - 4 * ck) // 2] ^= 0x40
    bad_hdr[off + 7] ^= 0xFF
    cases += [("truncated", good[: off + n // 2]), ("flipped", bytes(flipped)), ("bad check byte", bytes(bad_hdr))]
    seen = 0
    for k, (rel, comp) in enumerate(cases):
        bs = 1 << comp[5]
        size = min(product.get_decompressed_size(comp) or 3 * bs + 5, 1 << 20)
        probe = oracle.decompress(comp, size + bs)[0]
        if probe >= 0 and len(_host_walk(comp, comp[6] >> 7, 1 << 30)) != -(-probe // bs):
            continue  # (irregular: the departure)
        seen += _check_archive(shim, oracle, comp, bs, size, 100 + k, rel)
    assert seen >= 100, seen


@pytest.mark.parametrize("bs", [4096, 65536])
@pytest.mark.parametrize("checksum", [0, 1])
@pytest.mark.parametrize("seekable", [0, 1])
def test_sessions_take_the_reference_archives_apart(shim, oracle, ref, bs, checksum, seekable):
    from zxc_amd import corpus
    text = corpus.synth_text(70 * bs if bs == 4096 else 4 * bs, seed=11)
    noise = np.random.default_rng(bs).integers(0, 256, 4 * bs, dtype=np.uint8).tobytes()
    for k, n in enumerate((0, 1, 33, bs - 1, bs, bs + 1, 2 * bs, 3 * bs + 5) + ((70 * bs - 3,) if bs == 4096 else ())):
        data = (noise if k % 3 == 2 and n <= len(noise) else text)[:n]
        arc = ref.compress(data, 1 + k % 5, bs, bool(seekable), bool(checksum))
        _check_archive(shim, oracle, arc, bs, n, bs + 8 * k + 2 * checksum + seekable, (n, bs, checksum, seekable),
                       decoder=lambda cap, verify, arc=arc: ref.decompress(arc, cap, checksum=verify))


def test_dictionary_rule_of_the_head(shim, oracle):
    """an archive written with a dictionary: DICT_REQUIRED without one, and nothing is decoded or copied"""
    comp = open(os.path.join(GOLDEN, "conformance/valid/dict_http.zxc"), "rb").read()
    bs, size = 1 << comp[5], os.path.getsize(os.path.join(GOLDEN, "conformance/valid/dict_http.expected"))
    blocks = Blocks(shim, oracle, comp, bs, size, False)
    rc, got = _session(shim, comp, bs, size, False, [5, size - 5], max(size, bs), 1, blocks)
    assert rc == ERR["DICT_REQUIRED"] == oracle.decompress(comp, size)[0] and got == bytes([0xC3]) * size  # (the pieces start as 0xC3)
    rc, got = _session(shim, comp, bs, size, False, [size], max(size, bs), 0, blocks, have_dict=1, dict_id=0x12345678)
    assert rc == -16 and got == bytes([0xC3]) * size  # DICT_MISMATCH


def test_rules_under_sanitizers(tmp_path):
    """the stand-alone program tests/take/take_san_main.c (its own main; nothing of it is loaded into this process)"""
    r = cshim.run_san_program(tmp_path, "take/take_san_main.c")
    assert "TAKE OK 2688" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
