"""The append session (zxc_mi355x_compress_begin_device / _append_device / _end_device) without a GPU: the four symbols and the
Python names, every synchronous argument check in its stated order (the device pointers below are never dereferenced), the
work-size arithmetic against the bound the header states, and the rules the entry points and kernels run
(zxc_amd/csrc/zxc_append.h), compiled here with the host C compiler. Archives that the unmodified reference wrote, and this
library's goldens, are cut into their blocks (the slots and sizes an encode launch leaves) and put together again by a session
replayed on the host (tests/append/append_replay.h: piece plan, copies, jobs, advance, finish, a byte gather) at many cut points:
the output must be the archive byte for byte, with a pattern intact everywhere else. The same replay runs under AddressSanitizer
and UBSan in a stand-alone program."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import cshim
from conftest import GOLDEN
from cshim import opts as _opts, ref as _ref
from devtest import ERR
from zxc_amd.api import _DevCappend as Cs  # zxc_dev_cappend_t

FAKE_SRC, FAKE_DST, FAKE_WORK, FAKE_RES = 0x10000, 0x30000, 0x40000, 0x50000
BAD_BLOCK_SIZES = (1000, 2048, 4095, 5000, 3 << 12, 1 << 22)
BLOCK_SIZES = (4096, 65536, 1 << 19, 1 << 21)
JOB_BYTES, TILE_BYTES, AREAS, PAD, WORK_FIXED = 28, 16, 3, 64, 4096  # the stated bound: J (S + 28) + 16 ceil(J / 1024) + 3 (bs + 64) + 4 NB + 4096
CANARY = 0xC3


def _stride(bs):
    return 2 * bs + 512  # zxc_mi355x_encode_slot_stride, checked against the library below


def _host_dict_opts(**kw):
    return cshim.host_dict(_opts(**kw))


@pytest.fixture(scope="module")
def L(product):
    L = product.lib()
    assert hasattr(L, "zxc_mi355x_compress_begin_device"), "libzxc_mi355x.so does not export zxc_mi355x_compress_begin_device"
    for bs in BLOCK_SIZES:
        assert int(L.zxc_mi355x_encode_slot_stride(bs)) == _stride(bs)
    return L


def _ws(L, max_total, max_piece, o):
    return int(L.zxc_mi355x_compress_append_device_work_size(max_total, max_piece, _ref(o)))


def _begin(L, cs="new", dst=FAKE_DST, cap=1 << 20, max_total=1 << 24, max_piece=1 << 20, o="default", work=FAKE_WORK, ws=None):
    o = _opts() if isinstance(o, str) else o
    cs = Cs() if isinstance(cs, str) else cs
    if ws is None:
        ws = max(_ws(L, max_total, max_piece, o), 1)
    return L.zxc_mi355x_compress_begin_device(_ref(cs), dst, cap, max_total, max_piece, _ref(o), work, ws, None)


def test_symbols_and_names_exported(product):
    L = product.lib()
    for sym in ("zxc_mi355x_compress_append_device_work_size", "zxc_mi355x_compress_begin_device", "zxc_mi355x_compress_append_device",
                "zxc_mi355x_compress_end_device"):
        assert hasattr(L, sym), sym
    for name in ("compress_append_device_work_size", "compress_begin_device"):
        assert hasattr(product, name) and hasattr(product.api, name), name
    assert all(sym in product.api._PROTOTYPES for sym in ("zxc_mi355x_compress_append_device_work_size", "zxc_mi355x_compress_begin_device",
                                                          "zxc_mi355x_compress_append_device", "zxc_mi355x_compress_end_device"))
    assert hasattr(product.api.CompressAppendSession, "append") and hasattr(product.api.CompressAppendSession, "end")


def test_begin_each_synchronous_error_and_their_order(L):
    for k in ("cs", "dst", "work"):
        assert _begin(L, **{k: None}) == ERR["NULL_INPUT"], k
    assert _begin(L, o=_host_dict_opts(), ws=1 << 40) == ERR["GPU_UNSUPPORTED"]
    for bad in BAD_BLOCK_SIZES:
        assert _begin(L, o=_opts(block_size=bad), ws=1 << 40) == ERR["BAD_BLOCK_SIZE"], bad
    assert _begin(L, max_piece=65535, ws=1 << 40) == ERR["BAD_BLOCK_SIZE"]            # max_piece < block_size
    assert _begin(L, max_piece=0, ws=1 << 40) == ERR["BAD_BLOCK_SIZE"]
    o4 = _opts(block_size=4096)
    assert _begin(L, o=o4, max_total=((1 << 31) - 1) * 4096 + 1, ws=1 << 62) == ERR["BAD_BLOCK_SIZE"]  # 2^31 blocks
    assert _begin(L, o=o4, max_total=(1 << 64) - 1, ws=1 << 62) == ERR["BAD_BLOCK_SIZE"]
    assert _begin(L, o=o4, max_piece=1 << 63, ws=1 << 62) == ERR["BAD_BLOCK_SIZE"]     # more jobs in a piece than a launch counts
    for mt, mp, bs, sk in ((0, 4096, 4096, 0), (1 << 24, 1 << 20, 65536, 1), (1 << 40, 64 << 20, 65536, 0), (5, 1 << 21, 1 << 21, 1)):
        o = _opts(block_size=bs, seekable=sk)
        assert _begin(L, o=o, max_total=mt, max_piece=mp, ws=_ws(L, mt, mp, o) - 1) == ERR["MEMORY"], (mt, mp, bs)
    for sk, ck in ((0, 0), (1, 1)):
        assert _begin(L, o=_opts(seekable=sk, checksum=ck), cap=35) == ERR["DST_TOO_SMALL"]  # the empty archive: 16 + 8 + 12
    # each call breaks one rule and every later one; the earliest is reported
    bad_bs, hd = _host_dict_opts(block_size=5000), _host_dict_opts()
    assert _begin(L, dst=None, o=bad_bs, max_piece=1, ws=0, cap=0) == ERR["NULL_INPUT"]
    assert _begin(L, o=bad_bs, max_piece=1, ws=0, cap=0) == ERR["GPU_UNSUPPORTED"]      # the host dictionary comes first, as in compress_device
    assert _begin(L, o=hd, max_piece=1, ws=0, cap=0) == ERR["GPU_UNSUPPORTED"]
    assert _begin(L, o=_opts(block_size=5000), max_piece=1, ws=0, cap=0) == ERR["BAD_BLOCK_SIZE"]
    assert _begin(L, max_piece=1, ws=0, cap=0) == ERR["BAD_BLOCK_SIZE"]
    assert _begin(L, max_total=1 << 62, o=o4, ws=0, cap=0) == ERR["BAD_BLOCK_SIZE"]
    assert _begin(L, ws=0, cap=0) == ERR["MEMORY"]
    assert _begin(L, cap=0) == ERR["DST_TOO_SMALL"]
    cs = Cs()
    assert _begin(L, cs=cs, cap=0) == ERR["DST_TOO_SMALL"] and not any(cs.opaque)  # a refused begin leaves the struct alone


def test_append_and_end_refuse_by_status(L):
    cs = Cs()
    assert L.zxc_mi355x_compress_append_device(None, FAKE_SRC, 10, None) == ERR["NULL_INPUT"]
    assert L.zxc_mi355x_compress_append_device(_ref(cs), None, 10, None) == ERR["NULL_INPUT"]
    assert L.zxc_mi355x_compress_append_device(_ref(cs), FAKE_SRC, 10, None) == ERR["NULL_INPUT"]  # never begun
    assert L.zxc_mi355x_compress_append_device(_ref(cs), None, 0, None) == ERR["NULL_INPUT"]
    assert L.zxc_mi355x_compress_end_device(None, FAKE_RES, None) == ERR["NULL_INPUT"]
    assert L.zxc_mi355x_compress_end_device(_ref(cs), None, None) == ERR["NULL_INPUT"]
    assert L.zxc_mi355x_compress_end_device(_ref(cs), FAKE_RES, None) == ERR["NULL_INPUT"]       # never begun
    junk = Cs()
    C.memset(C.byref(junk), 0xEE, C.sizeof(junk))
    assert L.zxc_mi355x_compress_append_device(_ref(junk), FAKE_SRC, 10, None) == ERR["NULL_INPUT"]
    assert L.zxc_mi355x_compress_end_device(_ref(junk), FAKE_RES, None) == ERR["NULL_INPUT"]


def test_valid_arguments_without_a_device(product, L):
    """What remains after the argument checks is the device check. Only on a machine without a device is the call made (elsewhere
    these pointers would reach a kernel)."""
    if product.lib().zxc_mi355x_device_count() == 0:
        cs = Cs()
        assert _begin(L, cs=cs) == ERR["GPU_UNAVAILABLE"] and not any(cs.opaque)
        assert _begin(L, o=None, max_piece=1 << 19) == ERR["GPU_UNAVAILABLE"]
        assert _begin(L, o=_opts(level=7, block_size=4096, seekable=True, checksum=True), cap=36) == ERR["GPU_UNAVAILABLE"]
        with pytest.raises(product.ZxcError) as e:
            product.compress_begin_device(FAKE_DST, 1 << 20, 1 << 24, 1 << 20, FAKE_WORK, 1 << 30, block_size=4096)
        assert e.value.code == ERR["GPU_UNAVAILABLE"]


def test_python_binding_raises(product):
    with pytest.raises(product.ZxcError) as e:
        product.compress_begin_device(FAKE_DST, 1 << 20, 1 << 24, 1 << 20, FAKE_WORK, 1 << 30, block_size=5000)
    assert e.value.code == ERR["BAD_BLOCK_SIZE"]
    with pytest.raises(product.ZxcError) as e:
        product.compress_begin_device(FAKE_DST, 1 << 20, 1 << 24, 1 << 20, FAKE_WORK, 1, block_size=4096)
    assert e.value.code == ERR["MEMORY"]
    with pytest.raises(product.ZxcError) as e:
        product.compress_begin_device(0, 1 << 20, 1 << 24, 1 << 20, FAKE_WORK, 1 << 30, block_size=4096)
    assert e.value.code == ERR["NULL_INPUT"]
    s = product.api.CompressAppendSession(product.api._DevCappend())  # never begun
    with pytest.raises(product.ZxcError) as e:
        s.append(FAKE_SRC, 10)
    assert e.value.code == ERR["NULL_INPUT"]
    with pytest.raises(product.ZxcError) as e:
        s.end(FAKE_RES)
    assert e.value.code == ERR["NULL_INPUT"]
    assert product.compress_append_device_work_size(1 << 30, 1 << 20, block_size=5000) == 0
    assert product.compress_append_device_work_size(1 << 30, 1 << 20, block_size=4096) > 0


# ---------------------------------------------------------------- the shared rules, run on the CPU
class Shape(C.Structure):  # zap_shape_t
    _fields_ = [(n, C.c_uint32) for n in ("J", "n_tiles", "slot_stride", "area")] + \
               [(n, C.c_uint64) for n in ("nb_max", "o_tile_sum", "o_tile_hash", "o_tile_bad", "o_jobs", "o_sizes", "o_offsets")] + \
               [("o_carry", C.c_uint64 * 2)] + [(n, C.c_uint64) for n in ("o_stage", "o_seek", "o_slots", "bytes")]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    S = cshim.build_shim(tmp_path_factory, "append", "append/append_shim.c")
    for f in ("t_shape_size", "t_ctl_size", "t_piece_size"):
        getattr(S, f).restype = C.c_size_t
    assert S.t_shape_size() == C.sizeof(Shape) and S.t_ctl_size() <= 256
    S.t_shape.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(Shape)]
    S.t_work_bound.restype = C.c_uint64
    S.t_work_bound.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int]
    S.t_piece_len.restype = C.c_uint64
    S.t_piece_len.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32]
    S.t_session.restype = C.c_int64
    S.t_session.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p,
                            C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64]
    S.t_plan_check.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32]
    S.t_plan_check_range.restype = C.c_uint64
    S.t_plan_check_range.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64]
    S.t_hash_in_pieces.restype = C.c_uint32
    S.t_hash_in_pieces.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    S.t_hash_serial.restype = C.c_uint32
    S.t_hash_serial.argtypes = [C.c_void_p, C.c_uint32]
    return S


def test_work_size(product, L, shim):
    for bs in BLOCK_SIZES:
        S = _stride(bs)
        for sk in (0, 1):
            o = _opts(block_size=bs, seekable=sk)
            for mp in (bs, bs + 1, 2 * bs - 1, 7 * bs, 1023 * bs, 1 << 26):
                prev = None
                for mt in (0, 1, bs, bs + 1, 1 << 26, 1 << 30, 1 << 36):
                    w = _ws(L, mt, mp, o)
                    J, NB = mp // bs + 2, -(-mt // bs)
                    bound = J * (S + JOB_BYTES) + TILE_BYTES * -(-J // 1024) + AREAS * (bs + PAD) + (4 * NB if sk else 0) + WORK_FIXED
                    assert bound == int(shim.t_work_bound(mt, mp, bs, S, sk))
                    assert 0 < w <= bound, (bs, sk, mp, mt, w, bound)
                    assert w >= J * (S + JOB_BYTES) + AREAS * (bs + PAD) + (4 * NB if sk else 0), (bs, sk, mp, mt)  # at least its parts
                    sh = Shape()
                    assert shim.t_shape(mt, mp, bs, S, sk, C.byref(sh)) == 0 and sh.bytes == w and (sh.J, sh.nb_max) == (J, NB)
                    parts = [sh.o_tile_sum, sh.o_tile_hash, sh.o_tile_bad, sh.o_jobs, sh.o_sizes, sh.o_offsets, sh.o_carry[0], sh.o_carry[1],
                             sh.o_stage, sh.o_seek, sh.o_slots, sh.bytes - 256]
                    assert all(p % 256 == 0 for p in parts) and parts == sorted(parts) and parts[0] >= 256
                    assert sh.o_sizes - sh.o_jobs >= 16 * J and sh.o_offsets - sh.o_sizes >= 4 * J and sh.o_carry[0] - sh.o_offsets >= 8 * J
                    assert min(sh.o_carry[1] - sh.o_carry[0], sh.o_stage - sh.o_carry[1], sh.o_seek - sh.o_stage) >= bs + PAD
                    assert sh.o_slots - sh.o_seek >= (4 * NB if sk else 0) and sh.bytes - 256 - sh.o_slots >= J * S
                    if prev is not None:
                        if sk:  # 4 bytes per block of max_total, rounded to the work area's 256
                            assert abs((w - prev[0]) - 4 * (NB - prev[1])) < 256 and w >= prev[0]
                        else:   # without a seek table the source's size does not enter
                            assert w == prev[0]
                    prev = (w, NB)
            for level in (1, 7):  # the shape does not depend on these
                for ck in (0, 1):
                    assert _ws(L, 1 << 30, 1 << 24, _opts(level, bs, sk, ck)) == _ws(L, 1 << 30, 1 << 24, o)
    o = _opts(block_size=65536)
    a, b = (_ws(L, 64 * 65536 * k, 1 << 24, _opts(block_size=65536, seekable=True)) for k in (100, 101))
    assert b - a == 4 * 64  # 64 blocks more: 256 bytes more
    # the point of the session: the work area of a terabyte in pieces of 64 MiB is smaller than compress_device's for a gibibyte
    for sk in (False, True):
        assert 0 < product.compress_append_device_work_size(1 << 40, 64 << 20, 3, 65536, sk, False) < \
            product.compress_device_work_size(1 << 30, 3, 65536, sk, False)
    assert _ws(L, 1 << 30, 1 << 20, None) == _ws(L, 1 << 30, 1 << 20, _opts(level=0, block_size=0)) == _ws(L, 1 << 30, 1 << 20, _opts(block_size=1 << 19))
    # 0 for what begin refuses
    for bad in BAD_BLOCK_SIZES:
        assert _ws(L, 1 << 30, 1 << 22, _opts(block_size=bad)) == 0, bad
    assert _ws(L, 1 << 30, 1 << 22, _host_dict_opts()) == 0
    assert _ws(L, 1 << 30, 65535, o) == 0 and _ws(L, 1 << 30, 65536, o) > 0
    o4 = _opts(block_size=4096)
    assert _ws(L, ((1 << 31) - 1) * 4096, 4096, o4) > 0 and _ws(L, ((1 << 31) - 1) * 4096 + 1, 4096, o4) == 0
    assert _ws(L, 0, 1 << 63, o4) == 0


def test_piece_lengths(shim):
    bs = 4096
    for mp in (bs, bs + 1, 3 * bs - 1, 8 * bs):
        for carry in (0, 1, 100, bs - 1):
            for left in (1, bs - 1, mp - 1, mp, mp + 1, 5 * mp + 77):
                m = int(shim.t_piece_len(carry, left, mp, bs))
                assert 0 < m <= min(left, mp)
                assert m == left or (carry + m) % bs == 0, (mp, carry, left, m)
                assert (carry + m) // bs <= mp // bs + 1  # the jobs of a piece: J keeps one more


def test_every_plan_keeps_its_promises(shim):
    """for every carry and every n of a range that passes three block boundaries, at block_size 4096: a direct job's 32-byte
    over-read stays inside n, at most two blocks are staged, every source byte is copied once or read by one direct job, every
    copy with its padding fits its area, the jobs are the piece's blocks in order (promise numbers: append_replay.h)"""
    bs = 4096
    for lo, hi in ((1, 100), (bs - 100, bs + 100), (2 * bs - 100, 2 * bs + 100), (3 * bs - 100, 3 * bs + 100)):
        bad = int(shim.t_plan_check_range(bs, lo, hi))
        assert bad == 0, dict(carry=bad >> 40, n=(bad >> 8) & 0xFFFFFFFF, promise=bad & 0xFF)
    for bs in (65536, 1 << 21):
        for carry in (0, 1, 31, 32, 33, bs - 33, bs - 32, bs - 1):
            for n in (1, 31, 32, 33, bs - carry - 1, bs - carry, bs - carry + 1, bs - carry + 31, bs - carry + 32, bs - carry + 33, bs, bs + 32,
                      2 * bs - carry + 31, 2 * bs - carry + 32, 3 * bs + 5, 17 * bs - carry):
                if n > 0:
                    assert shim.t_plan_check(carry, n, bs) == 0, (bs, carry, n)


def test_the_carried_hash_is_the_serial_fold(shim):
    rng = np.random.default_rng(5)
    for n in (0, 1, 31, 32, 33, 64, 70, 100, 1025):
        t = rng.integers(0, 1 << 32, max(n, 1), dtype=np.uint32)
        want = int(shim.t_hash_serial(t.ctypes.data, n))
        for piece in (1, 2, 8, 31, 32, 33, 64, 2000):
            assert int(shim.t_hash_in_pieces(t.ctypes.data, n, piece)) == want, (n, piece)


class Arc:
    """an archive cut into its parts: the blocks with their headers (and trailers), and what the header and footer say"""

    def __init__(self, comp, what, data=None):
        self.comp, self.what, self.data = comp, what, data
        assert int.from_bytes(comp[0:4], "little") == 0x9CB02EF5 and comp[4] == 8
        self.bs = 1 << comp[5]
        self.checksum, self.has_dict = bool(comp[6] & 0x80), bool(comp[6] & 0x40)
        self.blocks, at = [], 16
        while comp[at] != 255:
            n = 8 + int.from_bytes(comp[at + 3: at + 7], "little") + (4 if self.checksum else 0)
            self.blocks.append(comp[at: at + n])
            at += n
        rest = len(comp) - at - 8 - 12
        self.seekable = rest > 0
        assert rest == ((8 + 4 * len(self.blocks)) if self.seekable else 0), what
        self.size = int.from_bytes(comp[-12:-4], "little")
        self.regular = len(self.blocks) == -(-self.size // self.bs)  # one block per block_size bytes of the source


def _cuts(total, bs, rng):
    """name -> (append lengths, max_piece): block boundaries, inside blocks, zero-length appends, sub-block appends in a row"""
    whole = max(total, bs)
    out = {"one": ([total], whole),
           "at block boundaries": ([bs] * (total // bs) + ([total % bs] if total % bs else []), bs),
           "the piece loop": ([total], bs),
           "the piece loop behind a carry": ([min(total, 5), total - min(total, 5)], 2 * bs + 17)}
    small = [min(111, bs // 3)] * min(40, total // min(111, bs // 3))
    out["sub-block appends in a row"] = (small + [total - sum(small)], whole)
    if total > bs:
        out["around a boundary with nothing between"] = ([bs - 1, 0, 2, 0, 0, total - bs - 1, 0], whole)
    for k in range(3):
        lens, left = [], total
        while left:
            n = min(left, rng.choice((0, 1, rng.randrange(bs), bs, rng.randrange(3 * bs + 9))))
            lens.append(n)
            left -= n
        out["random %d" % k] = (lens, rng.choice((bs, 2 * bs, 3 * bs + 100, whole)))
    return out


def _session(shim, a, lens, max_piece, cap, sizes=None, seekable=None):
    """-> (result, destination of cap + 64 bytes that started as the canary)"""
    blocks = np.frombuffer(b"".join(a.blocks) + b"\0", dtype=np.uint8)
    blk_size = np.array([len(b) for b in a.blocks] + [0], dtype=np.uint32)
    blk_at = np.concatenate(([0], np.cumsum(blk_size[:-1], dtype=np.uint64))).astype(np.uint64)
    if sizes is not None:
        blk_size = np.array(list(sizes) + [0], dtype=np.uint32)
    src = np.frombuffer(a.data + b"\0", dtype=np.uint8)
    ln = np.array(list(lens) + [0], dtype=np.uint64)
    dst = np.full(cap + 64, CANARY, dtype=np.uint8)
    sk = a.seekable if seekable is None else seekable
    rc = int(shim.t_session(src.ctypes.data, a.size, blocks.ctypes.data, blk_at.ctypes.data, blk_size.ctypes.data, len(a.blocks), a.bs,
                            int(a.checksum), int(sk), ln.ctypes.data, len(lens), max_piece, dst.ctypes.data, cap))
    return rc, dst


def _check_arc(shim, a, seed, seekable=None):
    rng = random.Random(seed)
    n = len(a.comp)
    for name, (lens, mp) in _cuts(a.size, a.bs, rng).items():
        assert sum(lens) == a.size
        rc, dst = _session(shim, a, lens, mp, n, seekable=seekable)  # a capacity of exactly the archive
        assert rc == n, (a.what, name, rc)
        assert dst[:n].tobytes() == a.comp and (dst[n:] == CANARY).all(), (a.what, name)
        rc, dst = _session(shim, a, lens, mp, n + 33, seekable=seekable)
        assert rc == n and dst[:n].tobytes() == a.comp and (dst[n:] == CANARY).all(), (a.what, name)
        rc, dst = _session(shim, a, lens, mp, n - 1, seekable=seekable)  # one byte less: refused, nothing at or past the capacity
        assert rc == ERR["DST_TOO_SMALL"] and (dst[n - 1:] == CANARY).all(), (a.what, name, rc)


_REF_ARCS = {}


def _ref_arcs(ref, bs, checksum, seekable):
    from zxc_amd import corpus
    key = (bs, checksum, seekable)
    if key not in _REF_ARCS:
        text = corpus.synth_text(70 * bs if bs == 4096 else 4 * bs, seed=11)
        noise = np.random.default_rng(bs).integers(0, 256, 4 * bs, dtype=np.uint8).tobytes()
        out = []
        for k, n in enumerate((0, 1, 33, bs - 1, bs, bs + 1, 2 * bs, 3 * bs + 5) + ((70 * bs - 3,) if bs == 4096 else ())):
            data = (noise if k % 3 == 2 and n <= len(noise) else text)[:n]
            out.append(Arc(ref.compress(data, 1 + k % 5, bs, bool(seekable), bool(checksum)), (n, bs, checksum, seekable), data))
        _REF_ARCS[key] = out
    return _REF_ARCS[key]


@pytest.mark.parametrize("bs", [4096, 65536])
@pytest.mark.parametrize("checksum", [0, 1])
@pytest.mark.parametrize("seekable", [0, 1])
def test_sessions_put_the_reference_archives_together_again(shim, ref, bs, checksum, seekable):
    arcs = _ref_arcs(ref, bs, checksum, seekable)
    assert all(a.regular and a.bs == bs and a.checksum == bool(checksum) and a.seekable == bool(seekable and a.blocks) for a in arcs)
    assert sorted(len(a.blocks) for a in arcs)[:8] == [0, 1, 1, 1, 1, 2, 2, 4]
    assert bs != 4096 or max(len(a.blocks) for a in arcs) == 70  # more than 32 blocks: the rotation of the carried hash wraps
    for k, a in enumerate(arcs):
        _check_arc(shim, a, seed=bs + 8 * k + 2 * checksum + seekable, seekable=seekable)


def test_sessions_put_the_golden_archives_together_again(shim, oracle):
    seen, kinds = 0, set()
    for d in ("conformance/valid", "format", "synth"):
        p = os.path.join(GOLDEN, d)
        for f in sorted(os.listdir(p)) if os.path.isdir(p) else ():
            if not f.endswith(".zxc"):
                continue
            try:
                a = Arc(open(os.path.join(p, f), "rb").read(), f"{d}/{f}")
            except (AssertionError, IndexError):
                continue  # (a format vector that is no complete archive)
            if not a.regular or a.has_dict or a.size > (8 << 20):  # (a dictionary header is the _dict sibling's, which does not exist yet)
                continue
            rc, a.data = oracle.decompress(a.comp, a.size, checksum=a.checksum)
            if rc != a.size:
                continue
            # an archive without blocks has no seek table whatever the option was: it goes with both kinds
            for sk in ((0, 1) if not a.blocks else (int(a.seekable),)):
                _check_arc(shim, a, seed=seen, seekable=sk)
                seen += 1
                kinds.add((a.bs, int(a.checksum), sk, min(len(a.blocks), 2)))
    assert seen >= 20 and len(kinds) >= 6, (seen, sorted(kinds))
    assert {k[0] for k in kinds} >= {4096, 65536} and {k[1] for k in kinds} == {0, 1} and {k[2] for k in kinds} == {0, 1}


def test_a_block_size_outside_the_range_is_corrupt_data(shim, ref):
    for checksum in (0, 1):
        a = _ref_arcs(ref, 4096, checksum, 1)[7]  # 3 blocks + 5 bytes
        assert len(a.blocks) == 4
        lo, hi = 8 + 4 * checksum, 4096 + 64
        real = [len(b) for b in a.blocks]
        for where in (0, 2, 3):
            for bad in (0, lo - 1, hi + 1, (1 << 32) - 1):
                sizes = list(real)
                sizes[where] = bad
                for lens, mp in (([a.size], a.size), ([4096, 4096, a.size - 8192], 4096), ([a.size], 4096)):
                    rc, dst = _session(shim, a, lens, mp, len(a.comp) + 100, sizes=sizes)
                    assert rc == ERR["CORRUPT_DATA"], (where, bad, lens)
                    assert (dst[len(a.comp) + 100:] == CANARY).all()
        # a corrupt size in a later piece wins over a capacity an earlier piece exceeded, as compress_device orders the two
        sizes = list(real)
        sizes[3] = 0
        rc, _ = _session(shim, a, [4096, 4096, a.size - 8192], 4096, 40, sizes=sizes)
        assert rc == ERR["CORRUPT_DATA"]
        rc, _ = _session(shim, a, [4096, 4096, a.size - 8192], 4096, 40)
        assert rc == ERR["DST_TOO_SMALL"]


def test_rules_under_sanitizers(tmp_path):
    """the stand-alone program tests/append/append_san_main.c (its own main; nothing of it is loaded into this process)"""
    r = cshim.run_san_program(tmp_path, "append/append_san_main.c")
    assert "APPEND OK 784" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
