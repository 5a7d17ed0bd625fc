"""zxc_mi355x_decompress_takev_device without a GPU: the two symbols and the Python names, every synchronous argument check in its
stated order on a forged live session (the device pointers below are never dereferenced), the scratch-size arithmetic against the
bound the header states, and the rules the entry point and kernels run (zxc_amd/csrc/zxc_takev.h on top of zxc_take.h and
zxc_appendv.h), compiled here with the host C compiler: the table's verdict, the in-place rule against a plain walk over the
entries, and whole sessions that mix take and takev replayed on the host (tests/take/takev_replay.h: the real container stages, the
plan of every job, a stand-in decoder that copies each block's expected bytes and then scribbles 32 bytes behind them, the copy of
every wave and lane) over goldens and archives the unmodified reference wrote, every entry a buffer of its own with canaries
around it. The same replay runs under AddressSanitizer and UBSan in a stand-alone program."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import cpu_take as T
import cshim
from conftest import GOLDEN
from devtest import ERR
from zxc_amd.api import IOV_DTYPE, _DevDtake as Ds

FAKE_IOV, FAKE_SCRATCH = 0x60000, 0x70000
TAKE_LIVE = 0x7A78632D74616B65
TAKE = 0xFFFFFFFF
BAD_PLAN = T.BAD_PLAN


@pytest.fixture(scope="module")
def L(product):
    L = product.lib()
    assert hasattr(L, "zxc_mi355x_decompress_takev_device"), "libzxc_mi355x.so does not export zxc_mi355x_decompress_takev_device"
    return L


def _ss(L, n_iov, mp, bs):
    return int(L.zxc_mi355x_decompress_takev_device_scratch_size(n_iov, mp, bs))


def _live(cap=1 << 20, mp=1 << 16, bs=4096, pos=0):
    """a session struct as begin leaves it (zxc_take_device.hip's Sess), over device pointers that are never dereferenced"""
    ds = Ds()
    words = [TAKE_LIVE, T.FAKE_SRC, 1000, cap, mp, T.FAKE_WORK, pos, 0, 0, bs << 32, 1]
    for i, w in enumerate(words):
        ds.opaque[i] = w
    return ds


def _takev(L, ds, iov=FAKE_IOV, n_iov=3, total=100, scratch=FAKE_SCRATCH, ss=1 << 40):
    return L.zxc_mi355x_decompress_takev_device(C.byref(ds) if ds is not None else None, iov, n_iov, total, scratch, ss, None)


def test_symbols_and_names_exported(product):
    L = product.lib()
    for sym in ("zxc_mi355x_decompress_takev_device_scratch_size", "zxc_mi355x_decompress_takev_device"):
        assert hasattr(L, sym), sym
    assert hasattr(product, "decompress_takev_device_scratch_size") and hasattr(product.api, "decompress_takev_device_scratch_size")
    assert all(sym in product.api._PROTOTYPES for sym in ("zxc_mi355x_decompress_takev_device_scratch_size", "zxc_mi355x_decompress_takev_device"))
    assert hasattr(product.api.DecompressTakeSession, "takev")
    assert IOV_DTYPE.itemsize == 16


def test_each_synchronous_error_and_their_order(L):
    def same(ds, before):
        return bytes(ds) == before

    ds = _live()
    before = bytes(ds)
    assert _takev(L, None) == ERR["NULL_INPUT"]
    assert _takev(L, ds, scratch=None) == ERR["NULL_INPUT"] and _takev(L, ds, iov=None) == ERR["NULL_INPUT"]
    never, junk = Ds(), Ds()
    C.memset(C.byref(junk), 0xEE, C.sizeof(junk))
    assert _takev(L, never) == ERR["NULL_INPUT"] and _takev(L, junk) == ERR["NULL_INPUT"] and not any(never.opaque)
    assert _takev(L, ds, iov=None, n_iov=0, total=1) == ERR["DST_TOO_SMALL"]
    assert _takev(L, ds, total=(1 << 20) + 1) == ERR["OVERFLOW"] and _takev(L, ds, total=(1 << 64) - 1) == ERR["OVERFLOW"]
    part = _live(pos=(1 << 20) - 10)
    assert _takev(L, part, total=11) == ERR["OVERFLOW"] and _takev(L, part, total=(1 << 64) - 5) == ERR["OVERFLOW"]  # without overflow
    for n_iov in (1, 3, 1025):
        assert _takev(L, ds, n_iov=n_iov, ss=_ss(L, n_iov, 1 << 16, 4096) - 1) == ERR["MEMORY"], n_iov
    assert _takev(L, ds, iov=None, n_iov=0, total=0, ss=0) == ERR["MEMORY"]      # the scratch is checked in front of the empty call
    assert _takev(L, ds, iov=None, n_iov=0, total=0, ss=_ss(L, 0, 1 << 16, 4096)) == 0 and same(ds, before)  # ZXC_OK, nothing enqueued
    # each call breaks one rule and every later one; the earliest is reported
    assert _takev(L, ds, scratch=None, iov=None, n_iov=0, total=1 << 30, ss=0) == ERR["NULL_INPUT"]
    assert _takev(L, never, iov=None, n_iov=0, total=1 << 30, ss=0) == ERR["NULL_INPUT"]
    assert _takev(L, ds, iov=None, n_iov=0, total=1 << 30, ss=0) == ERR["DST_TOO_SMALL"]
    assert _takev(L, ds, total=1 << 30, ss=0) == ERR["OVERFLOW"]
    assert _takev(L, ds, ss=0) == ERR["MEMORY"]
    assert same(ds, before) and bytes(part) == bytes(_live(pos=(1 << 20) - 10))    # a refused call leaves the struct as it was
    assert all(w == 0xEEEEEEEEEEEEEEEE for w in junk.opaque)


def test_valid_arguments_without_a_device(product, L):
    """What remains after the argument checks is the launch. Only on a machine without a device is the call made (elsewhere these
    pointers would reach a kernel): the launch fails and the session is spent, as in take."""
    if product.lib().zxc_mi355x_device_count() == 0:
        ds = _live()
        assert _takev(L, ds) == ERR["GPU_UNAVAILABLE"] and ds.opaque[0] == 0
        assert _takev(L, ds) == ERR["NULL_INPUT"]


def test_a_launch_error_ends_the_chunk_loop_and_spends_the_session(product, L):
    """4 KiB blocks, max_piece two blocks, a call of five blocks and 7 bytes (three chunks), on a machine without a device only. A
    take's first launch belongs to its first chunk: the loop ends behind that chunk (the position is two blocks, not the call's
    bytes) and the session is spent. A takev's first launch is its scan, in front of the loop: no chunk is planned."""
    if product.lib().zxc_mi355x_device_count() == 0:
        n = 5 * 4096 + 7
        ds = _live(mp=8192)
        assert L.zxc_mi355x_decompress_take_device(C.byref(ds), T.FAKE_DST, n, None) == ERR["GPU_UNAVAILABLE"]
        assert ds.opaque[0] == 0 and ds.opaque[6] == 8192
        assert L.zxc_mi355x_decompress_take_device(C.byref(ds), T.FAKE_DST, 1, None) == ERR["NULL_INPUT"]
        ds = _live(mp=8192)
        assert _takev(L, ds, total=n) == ERR["GPU_UNAVAILABLE"] and ds.opaque[0] == 0 and ds.opaque[6] == 0
        assert L.zxc_mi355x_decompress_end_device(C.byref(ds), T.FAKE_RES, None) == ERR["NULL_INPUT"]


def test_python_binding_raises(product):
    s = product.api.DecompressTakeSession(product.api._DevDtake())  # never begun
    with pytest.raises(product.ZxcError) as e:
        s.takev(FAKE_IOV, 3, 100, FAKE_SCRATCH, 1 << 30)
    assert e.value.code == ERR["NULL_INPUT"]
    s = product.api.DecompressTakeSession(_live())
    with pytest.raises(product.ZxcError) as e:
        s.takev(FAKE_IOV, 3, 100, FAKE_SCRATCH, 1)
    assert e.value.code == ERR["MEMORY"]
    with pytest.raises(product.ZxcError) as e:
        s.takev(0, 0, 100, FAKE_SCRATCH, 1 << 30)
    assert e.value.code == ERR["DST_TOO_SMALL"]
    assert product.decompress_takev_device_scratch_size(10, 1 << 20, 5000) == 0
    assert product.decompress_takev_device_scratch_size(10, 1 << 20, 4096) > 0


# ---------------------------------------------------------------- the shared rules, run on the CPU
class VShape(C.Structure):  # ztv_shape_t
    _fields_ = [("J", C.c_uint32), ("n_tiles", C.c_uint32)] + [(n, C.c_uint64) for n in ("o_starts", "o_tile_sum", "o_tile_flags", "o_places", "bytes")]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    S = cshim.build_shim(tmp_path_factory, "takev", "take/takev_shim.c")
    S.tv_shape_size.restype = S.tv_place_size.restype = C.c_size_t
    assert S.tv_shape_size() == C.sizeof(VShape) and S.tv_place_size() == 16
    S.tv_shape.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(VShape)]
    S.tv_scratch_bound.restype = C.c_uint64
    S.tv_scratch_bound.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32]
    S.tv_scan_serial.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    S.tv_scan_grouped.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32]
    S.tv_fold.restype = C.c_int64
    S.tv_fold.argtypes = [C.c_uint32, C.c_int64, C.c_int, C.POINTER(C.c_uint32)]
    S.tv_rule_check.restype = C.c_uint64
    S.tv_rule_check.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32]
    S.tv_session.restype = C.c_int64
    S.tv_session.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p,
                             C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    S.tv_session_bad_table.restype = C.c_int64
    S.tv_session_bad_table.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_char_p, C.POINTER(C.c_uint32)]
    S.tv_head.restype = C.c_uint32
    S.tv_head.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int]
    S.t_head = S.tv_head  # (the name Blocks of the take test asks its shim for)
    return S


def test_scratch_size(L, shim):
    for bs in (4096, 65536, 1 << 19, 1 << 21):
        for mp in (bs, bs + 1, 7 * bs, 1 << 28):
            for n_iov in (0, 1, 1024, 1025, 1 << 20):
                w, J, tiles = _ss(L, n_iov, mp, bs), mp // bs + 2, -(-n_iov // 1024)
                bound = 8 * (n_iov + 1) + 16 * tiles + 16 * J + 4096
                assert bound == int(shim.tv_scratch_bound(n_iov, mp, bs))
                sh = VShape()
                assert shim.tv_shape(n_iov, mp, bs, C.byref(sh)) == 0 and sh.bytes == w and (sh.J, sh.n_tiles) == (J, tiles)
                assert 0 < w <= bound, (bs, mp, n_iov, w, bound)
                parts = [sh.o_starts, sh.o_tile_sum, sh.o_tile_flags, sh.o_places, sh.bytes - 256]
                assert all(p % 256 == 0 for p in parts[:4]) and parts == sorted(parts) and parts[0] >= 256
                assert sh.o_tile_sum - sh.o_starts >= 8 * (n_iov + 1) and sh.o_tile_flags - sh.o_tile_sum >= 8 * tiles
                assert sh.o_places - sh.o_tile_flags >= 4 * tiles and sh.bytes - 256 - sh.o_places >= 16 * J
    for bad in T.BAD_BLOCK_SIZES:  # 0 for what begin refuses
        assert _ss(L, 10, 1 << 22, bad) == 0, bad
    assert _ss(L, 10, 65535, 65536) == 0 and _ss(L, 10, 0, 4096) == 0 and _ss(L, 10, 1 << 63, 4096) == 0
    assert _ss(L, 10, ((1 << 31) - 4) * 4096, 4096) > 0 and _ss(L, 10, ((1 << 31) - 3) * 4096, 4096) == 0  # J as zt_shape bounds it


def _table(entries):
    t = np.zeros(len(entries) + 1, dtype=IOV_DTYPE)
    for i, (b, n) in enumerate(entries):
        t[i] = (b, n)
    return t


def test_table_verdict(shim):
    M = (1 << 64) - 1

    def verdict(entries, total):
        t, starts = _table(entries), np.zeros(len(entries) + 2, dtype=np.uint64)
        v = shim.tv_scan_serial(t.ctypes.data, len(entries), total, starts.ctypes.data)
        for g in (1, 2, 3, 7, 1024):
            assert shim.tv_scan_grouped(t.ctypes.data, len(entries), total, g) == v, (entries, total, g)
        return v, starts

    v, starts = verdict([(0x1000, 5), (0, 0), (0x2000, 7), (0x3001, 1)], 13)
    assert v == 0 and list(starts[:5]) == [0, 5, 5, 12, 13]
    assert verdict([(0, 0)] * 5, 0)[0] == 0                                        # empty entries: the base is not looked at
    assert verdict([(0x1000, 5), (0x2000, 7)], 13)[0] == ERR["DST_TOO_SMALL"]      # a short table: fewer bytes than promised
    assert verdict([(0x1000, 5), (0x2000, 7)], 11)[0] == ERR["OVERFLOW"]           # a sum above total
    assert verdict([(0x1000, 12), (0x2000, 0)], 11)[0] == ERR["OVERFLOW"]          # an entry longer than total
    assert verdict([(0x1000, 1)], 0)[0] == ERR["OVERFLOW"]                         # total == 0: a non-empty entry is an error
    assert verdict([(0, 5), (0x2000, 7)], 12)[0] == ERR["NULL_INPUT"]
    # precedence: NULL over OVERFLOW over DST_TOO_SMALL
    assert verdict([(0x1000, 100), (0, 1)], 50)[0] == ERR["NULL_INPUT"] and verdict([(0, 1)], 50)[0] == ERR["NULL_INPUT"]
    assert verdict([(0x1000, 60), (0x2000, 1)], 50)[0] == ERR["OVERFLOW"]
    # sums past 2^64 stay above total, in any grouping
    assert verdict([(0x1000, M), (0x2000, M), (0x3000, 2)], 1 << 40)[0] == ERR["OVERFLOW"]
    assert verdict([(0x1000, 1 << 63), (0x2000, 1 << 63)], M - 1)[0] == ERR["OVERFLOW"]   # (the sum saturates at 2^64 - 1)
    assert verdict([(0x1000, 1 << 63), (0x2000, (1 << 63) - 1)], M)[0] == 0
    # the fold: an error becomes the result with final = 1; a result that is final already wins; no error changes nothing
    fin = C.c_uint32()
    assert shim.tv_fold(0, 0, ERR["OVERFLOW"], C.byref(fin)) == ERR["OVERFLOW"] and fin.value == 1
    assert shim.tv_fold(1, -7, ERR["OVERFLOW"], C.byref(fin)) == -7 and fin.value == 1
    assert shim.tv_fold(1, 0, ERR["NULL_INPUT"], C.byref(fin)) == 0 and fin.value == 1      # the empty-frame probe's 0 stays
    assert shim.tv_fold(0, 0, 0, C.byref(fin)) == 0 and fin.value == 0
    assert shim.tv_fold(0, 0, ERR["DST_TOO_SMALL"], C.byref(fin)) == ERR["DST_TOO_SMALL"] and fin.value == 1


def test_in_place_rule_against_a_plain_walk(shim):
    """entries of lengths around bs, bs + 31, bs + 32, bs + 33 (and two and three blocks of them), bases 0 and 1 mod 16, the call at
    every position mod 16 of a block and around its ends: a whole block goes direct exactly when it is aligned and its slot + 32
    ends inside one entry (promise numbers: takev_replay.h)"""
    bs = 4096
    around = [bs + d for d in (-1, 0, 1, 15, 16, 31, 32, 33, 48)] + [2 * bs + d for d in (0, 31, 32, 33)] + [3 * bs + 32, 5, 0, 16]
    rng = random.Random(5)
    cuts = list(range(0, 33)) + [bs - 33, bs - 32, bs - 17, bs - 16, bs - 1]
    for base_mod in (0, 1):
        for k in range(40):
            lens = [rng.choice(around) for _ in range(rng.randrange(1, 9))]
            t = _table([(0x100000 * (i + 1) + (base_mod if n else 0) if n else 0, n) for i, n in enumerate(lens)])
            for pos in cuts:
                for mp in (bs, 3 * bs, 64 * bs):
                    bad = int(shim.tv_rule_check(t.ctypes.data, len(lens), 9 * bs + pos, mp, bs))
                    assert bad == 0, dict(lens=lens, base_mod=base_mod, pos=pos, mp=mp, block=(bad >> 8) - 1, promise=bad & 0xFF)
    # the rule itself at its edges: one entry, the call at a block boundary
    for n, base in ((bs + 32, 0x100000), (bs + 31, 0x100000), (bs + 32, 0x100001), (2 * bs + 32, 0x100000), (2 * bs + 31, 0x100000)):
        t = _table([(base, n)])
        assert shim.tv_rule_check(t.ctypes.data, 1, 4 * bs, 8 * bs, bs) == 0, (n, base)
    for bs2 in (65536, 1 << 21):
        t = _table([(0x10000000, bs2 + 32), (0x20000010, bs2 + 31), (0x30000001, 3 * bs2 + 40), (0, 0), (0x40000000, 2 * bs2 + 33)])
        for pos in (0, 1, 16, bs2 - 16):
            assert shim.tv_rule_check(t.ctypes.data, 5, pos, 4 * bs2, bs2) == 0, (bs2, pos)


# ---------------------------------------------------------------- host replay
def _entry_cuts(total, bs, rng):
    """name -> (calls, max_piece); a call is ("take", n) or ("takev", [entry lengths])"""
    whole = max(total, bs)
    edge = [bs, bs + 31, bs + 32, bs + 33, 0, 2 * bs + 32, 15, 1, 4095, 4097, 16, 17, 33]

    def fill(pool, cap=10 ** 9):
        lens, left = [], total
        while left and len(lens) < cap:
            n = min(left, pool[len(lens) % len(pool)] if isinstance(pool, list) else pool())
            lens.append(n)
            left -= n
        if left:
            lens.append(left)
        return lens

    out = {"one entry": ([("takev", [total])], whole),
           "entries around a block and its spill": ([("takev", fill(edge))], whole),
           "the chunk loop": ([("takev", fill(edge[::-1]))], 2 * bs),
           "tiny entries": ([("takev", fill(lambda: rng.randrange(1, 8), 3000))], whole)}
    for k in range(3):  # take and takev mixed however the bytes are split, calls wholly inside one block included
        calls, left = [], total
        while left or not calls:
            n = min(left, rng.choice((0, 1, 16, 100, rng.randrange(bs), bs, rng.randrange(3 * bs + 9))))
            if rng.random() < 0.4:
                calls.append(("take", n))
            else:
                lens, rest = [], n
                while rest:
                    m = min(rest, rng.choice((0, 1, 5, 16, 17, rng.randrange(1, bs + 40), bs + 32)))
                    lens.append(m)
                    rest -= m
                calls.append(("takev", lens + [0] * rng.randrange(2)))
            left -= n
        out["mixed %d" % k] = (calls, rng.choice((bs, 2 * bs, 3 * bs + 100, whole)))
    return out


def _session(shim, comp, bs, cap, verify, calls, max_piece, align, blocks, use_table=1, have_dict=0, dict_id=0):
    lens, cl = [], []
    for kind, x in calls:
        if kind == "take":
            lens.append(x)
            cl.append(TAKE)
        elif x:
            lens += x
            cl.append(len(x))
    ln = np.array(lens + [0], dtype=np.uint64)
    ca = np.array(cl + [0], dtype=np.uint32)
    out = np.zeros(cap + 1, dtype=np.uint8)
    rc = int(shim.tv_session(comp, len(comp), cap, max_piece, bs, int(verify), use_table, have_dict, dict_id, blocks.bytes.ctypes.data,
                             blocks.at.ctypes.data, blocks.st.ctypes.data, blocks.n, ln.ctypes.data, ca.ctypes.data, len(cl), align,
                             out.ctypes.data))
    return rc, out[:cap].tobytes()


def _check_archive(shim, oracle, comp, bs, size, seed, what, decoder=None):
    rng = random.Random(seed)
    decoder = decoder or (lambda cap, verify: oracle.decompress(comp, cap, checksum=verify))
    n_sessions = 0
    for verify in (False, True):
        for cap in sorted({size, max(size - 1, 0), size + bs + 3, 0}):
            want, data = decoder(cap, verify)
            blocks = T.Blocks(shim, oracle, comp, bs, cap, verify)
            for k, (name, (calls, mp)) in enumerate(_entry_cuts(cap, bs, rng).items()):
                align = (0, 1, 8, 15, 16)[(k + seed) % 5]  # 16: every entry at its own address mod 16
                rc, got = _session(shim, comp, bs, cap, verify, calls, mp, align, blocks, use_table=(k + 1) % 2)
                assert rc != BAD_PLAN, (what, name, cap, verify, align)
                assert rc == want, (what, name, cap, verify, rc, want)
                if rc >= 0:
                    assert got[:rc] == data[:rc], (what, name, cap, verify, align)
                n_sessions += 1
    return n_sessions


def test_sessions_take_the_valid_goldens_apart(shim, oracle, product):
    seen = 0
    for k, rel in enumerate(T._goldens("conformance/valid")):
        comp = open(os.path.join(GOLDEN, rel), "rb").read()
        if len(comp) < 28 or not 12 <= comp[5] <= 21:
            continue
        bs, size = 1 << comp[5], product.get_decompressed_size(comp)
        exp = os.path.join(GOLDEN, rel[:-4] + ".expected")
        if os.path.exists(exp):
            size = os.path.getsize(exp)
        if size > (1 << 20):
            continue
        if oracle.decompress(comp, size)[0] >= 0 and len(T._host_walk(comp, comp[6] >> 7, 1 << 30)) != -(-size // bs):
            continue  # (irregular: the device calls answer GPU_UNSUPPORTED where the host decodes)
        seen += _check_archive(shim, oracle, comp, bs, size, k, rel)
    assert seen >= 150, seen


def test_sessions_answer_damaged_archives_as_the_reference_decoder(shim, oracle, product):
    good = open(os.path.join(GOLDEN, "conformance/valid/seekable_4blocks.zxc"), "rb").read()
    ck = good[6] >> 7
    walk = T._host_walk(good, ck, 1 << 30)
    off, n = walk[2]
    flipped, bad_hdr = bytearray(good), bytearray(good)
    flipped[off + 8 + (n - 8 - 4 * ck) // 2] ^= 0x40
    bad_hdr[off + 7] ^= 0xFF
    cases = [("truncated", good[: off + n // 2]), ("flipped", bytes(flipped)), ("bad check byte", bytes(bad_hdr))]
    for rel in ("conformance/invalid/bad_magic.zxc", "conformance/invalid/bad_block_checksum.zxc", "conformance/invalid/corrupt_payload.zxc"):
        cases.append((rel, open(os.path.join(GOLDEN, rel), "rb").read()))
    seen = 0
    for k, (rel, comp) in enumerate(cases):
        bs = 1 << comp[5]
        size = min(product.get_decompressed_size(comp) or 3 * bs + 5, 1 << 20)
        probe = oracle.decompress(comp, size + bs)[0]
        if probe >= 0 and len(T._host_walk(comp, comp[6] >> 7, 1 << 30)) != -(-probe // bs):
            continue
        seen += _check_archive(shim, oracle, comp, bs, size, 100 + k, rel)
    assert seen >= 100, seen


@pytest.mark.parametrize("bs", [4096, 65536])
@pytest.mark.parametrize("checksum", [0, 1])
def test_sessions_take_the_reference_archives_apart(shim, oracle, ref, bs, checksum):
    from zxc_amd import corpus
    text = corpus.synth_text(40 * bs if bs == 4096 else 4 * bs, seed=12)
    for k, n in enumerate((1, bs - 1, bs + 1, 3 * bs + 5) + ((40 * bs - 3,) if bs == 4096 else ())):
        arc = ref.compress(text[:n], 1 + k % 5, bs, bool(k & 1), bool(checksum))
        _check_archive(shim, oracle, arc, bs, n, bs + 8 * k + checksum, (n, bs, checksum),
                       decoder=lambda cap, verify, arc=arc: ref.decompress(arc, cap, checksum=verify))


def test_table_errors_in_a_replayed_session(shim, oracle):
    """every table error, in the first call and in a later one: the result at end, no byte of that call's entries written, the
    earlier calls' entries intact, and the later valid calls do not clear it"""
    comp = open(os.path.join(GOLDEN, "conformance/valid/seekable_4blocks.zxc"), "rb").read()
    bs, size = 1 << comp[5], os.path.getsize(os.path.join(GOLDEN, "conformance/valid/seekable_4blocks.expected"))
    want, data = oracle.decompress(comp, size)
    assert want == size
    blocks = T.Blocks(shim, oracle, comp, bs, size, False)
    rng = random.Random(3)
    lens, left = [], size
    while left:
        n = min(left, rng.choice((0, 7, 100, bs // 2, bs + 40)))
        lens.append(n)
        left -= n
    per_call = max(2, len(lens) // 4)
    ln = np.array(lens + [0], dtype=np.uint64)
    for bad_call in (0, 1, 2):
        assert sum(lens[bad_call * per_call:(bad_call + 1) * per_call]) > 1
        for kind, code in ((1, "NULL_INPUT"), (2, "OVERFLOW"), (3, "OVERFLOW"), (4, "DST_TOO_SMALL")):
            written = (C.c_uint32 * 2)()
            rc = int(shim.tv_session_bad_table(comp, len(comp), size, 2 * bs, bs, blocks.bytes.ctypes.data, blocks.at.ctypes.data,
                                               blocks.st.ctypes.data, blocks.n, ln.ctypes.data, len(lens), per_call, bad_call, kind, data,
                                               written))
            assert rc == ERR[code], (bad_call, kind, rc)
            assert written[0] == 0 and written[1] == 0, (bad_call, kind, list(written))
    written = (C.c_uint32 * 2)()  # and with no bad call: the archive's bytes and result
    rc = int(shim.tv_session_bad_table(comp, len(comp), size, 2 * bs, bs, blocks.bytes.ctypes.data, blocks.at.ctypes.data, blocks.st.ctypes.data,
                                       blocks.n, ln.ctypes.data, len(lens), per_call, 1 << 30, 1, data, written))
    assert rc == size and written[1] == 0


def test_rules_under_sanitizers(tmp_path):
    """the stand-alone program tests/take/takev_san_main.c (its own main; nothing of it is loaded into this process)"""
    r = cshim.run_san_program(tmp_path, "take/takev_san_main.c")
    assert "TAKEV OK 2016" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
