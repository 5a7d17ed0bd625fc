"""zxc_mi355x_compress_appendv_device (append a table of buffers to an append session) without a GPU: the two symbols and the Python
names, every synchronous argument check in its stated order (the device pointers below are never dereferenced; a live session is
forged in the caller-owned struct, since begin needs a device), the scratch-size arithmetic against the bound the header states,
and the rules the entry point and the kernels run (zxc_amd/csrc/zxc_appendv.h), compiled here with the host C compiler: the table
check with its precedence, the placement rule against a walk over the entries, and whole sessions mixing append and appendv
replayed on the host (tests/append/appendv_replay.h) over archives that the unmodified reference wrote and this library's goldens,
cut into their blocks. The output must be the archive byte for byte, with a pattern intact everywhere else. The same replay runs
under AddressSanitizer and UBSan in a stand-alone program in which every entry is a malloc of exactly its length."""
import bisect
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

FAKE_IOV, FAKE_DST, FAKE_WORK, FAKE_SCRATCH, FAKE_DICT = 0x10000, 0x30000, 0x40000, 0x50000, 0x60000
BLOCK_SIZES = (4096, 65536, 1 << 19, 1 << 21)
BAD_BLOCK_SIZES = (1000, 2048, 4095, 5000, 3 << 12, 1 << 22)
TILE_BYTES, IMAGE_SLACK, FIXED = 16, 256, 4096  # the stated bound: 8 (n + 1) + 16 ceil(n / 1024) + J (bs + 256) + 4096
SESS_LIVE = 0x7A78632D61707064  # a session between begin and end (zxc_append_device.hip)
CANARY = 0xC3
RP_BAD_PLAN = -1000


@pytest.fixture(scope="module")
def L(product):
    L = product.lib()
    assert hasattr(L, "zxc_mi355x_compress_appendv_device"), "libzxc_mi355x.so does not export zxc_mi355x_compress_appendv_device"
    return L


def _live(total=0, max_total=1 << 24, max_piece=1 << 20, bs=65536, dict_size=0):
    """the struct begin leaves (struct Sess of zxc_append_device.hip): begin itself needs a device, these tests have none"""
    cs = Cs()
    words = [SESS_LIVE, FAKE_DST, 1 << 20, max_total, max_piece, FAKE_WORK, total, bs | 3 << 32, 0, dict_size << 32,
             FAKE_DICT if dict_size else 0, FAKE_DICT + 0x1000 if dict_size else 0]
    for k, w in enumerate(words):
        cs.opaque[k] = w
    return cs


def _ss(L, n_iov, max_piece, o):
    return int(L.zxc_mi355x_compress_appendv_device_scratch_size(n_iov, max_piece, _ref(o)))


def _appendv(L, cs, iov=FAKE_IOV, n_iov=4, total=100, scratch=FAKE_SCRATCH, ss=1 << 40):
    before = None if cs is None else list(cs.opaque)
    rc = L.zxc_mi355x_compress_appendv_device(_ref(cs), iov, n_iov, total, scratch, ss, None)
    if cs is not None and rc < 0:
        assert list(cs.opaque) == before, "a refusal changed the session struct"
    return rc


def test_symbols_and_names_exported(product):
    L = product.lib()
    for sym in ("zxc_mi355x_compress_appendv_device_scratch_size", "zxc_mi355x_compress_appendv_device"):
        assert hasattr(L, sym), sym
    for name in ("compress_appendv_device_scratch_size", "IOV_DTYPE"):
        assert hasattr(product, name) and hasattr(product.api, name), name
    assert hasattr(product.api.CompressAppendSession, "appendv")
    d = product.IOV_DTYPE
    assert d.names == ("base", "len") and d.itemsize == 16 and all(d[n] == np.dtype("<u8") for n in d.names)
    b = product.lib()
    assert b.zxc_mi355x_compress_appendv_device.argtypes is not None and b.zxc_mi355x_compress_appendv_device_scratch_size.restype is C.c_uint64


def test_each_synchronous_error_and_their_order(L):
    live = _live()
    # each rule on its own
    assert _appendv(L, None) == ERR["NULL_INPUT"]
    assert _appendv(L, live, scratch=None) == ERR["NULL_INPUT"]
    assert _appendv(L, live, iov=None) == ERR["NULL_INPUT"]
    never, junk = Cs(), Cs()
    C.memset(C.byref(junk), 0xEE, C.sizeof(junk))
    assert _appendv(L, never) == ERR["NULL_INPUT"] and _appendv(L, junk) == ERR["NULL_INPUT"]
    assert _appendv(L, _live(dict_size=100)) == ERR["GPU_UNSUPPORTED"]
    assert _appendv(L, live, iov=None, n_iov=0, total=1) == ERR["SRC_TOO_SMALL"]
    assert _appendv(L, live, total=(1 << 24) + 1) == ERR["OVERFLOW"]
    assert _appendv(L, _live(total=(1 << 24) - 5), total=6) == ERR["OVERFLOW"]
    assert _appendv(L, _live(total=1 << 24), total=(1 << 64) - 1) == ERR["OVERFLOW"]  # compared without overflow
    assert _appendv(L, live, ss=0) == ERR["MEMORY"]
    # each call breaks one rule and every later one; the earliest is reported
    dict_full = _live(total=1 << 24, dict_size=7)
    assert _appendv(L, None, iov=None, n_iov=0, total=1 << 60, scratch=None, ss=0) == ERR["NULL_INPUT"]
    assert _appendv(L, dict_full, iov=None, n_iov=3, total=1 << 60, ss=0) == ERR["NULL_INPUT"]
    assert _appendv(L, junk, iov=None, n_iov=0, total=1 << 60, ss=0) == ERR["NULL_INPUT"]          # never begun, then everything else
    assert _appendv(L, dict_full, iov=None, n_iov=0, total=1 << 60, ss=0) == ERR["GPU_UNSUPPORTED"]
    full = _live(total=1 << 24)
    assert _appendv(L, full, iov=None, n_iov=0, total=1 << 60, ss=0) == ERR["SRC_TOO_SMALL"]
    assert _appendv(L, full, n_iov=5, total=1, ss=0) == ERR["OVERFLOW"]
    assert _appendv(L, live, n_iov=5, total=1, ss=0) == ERR["MEMORY"]
    # nothing to append: ZXC_OK, nothing enqueued, with or without a table pointer, and the struct as it was
    for iov in (None, FAKE_IOV):
        cs = _live(total=77)
        before = list(cs.opaque)
        assert _appendv(L, cs, iov=iov, n_iov=0, total=0) == 0 and list(cs.opaque) == before


def test_python_binding_raises(product):
    s = product.api.CompressAppendSession(product.api._DevCappend())  # never begun
    with pytest.raises(product.ZxcError) as e:
        s.appendv(FAKE_IOV, 3, 10, FAKE_SCRATCH, 1 << 30)
    assert e.value.code == ERR["NULL_INPUT"]
    s = product.api.CompressAppendSession(_live(dict_size=9))
    with pytest.raises(product.ZxcError) as e:
        s.appendv(FAKE_IOV, 3, 10, FAKE_SCRATCH, 1 << 30)
    assert e.value.code == ERR["GPU_UNSUPPORTED"]
    s = product.api.CompressAppendSession(_live())
    with pytest.raises(product.ZxcError) as e:
        s.appendv(FAKE_IOV, 3, 10, 0, 1 << 30)
    assert e.value.code == ERR["NULL_INPUT"]
    s.appendv(0, 0, 0, FAKE_SCRATCH, 1 << 30)  # nothing to append
    assert product.compress_appendv_device_scratch_size(10, 1 << 20, block_size=5000) == 0
    assert product.compress_appendv_device_scratch_size(10, 1 << 20, block_size=4096) > 0


# ---------------------------------------------------------------- the shared rules, run on the CPU
class VShape(C.Structure):  # zav_shape_t
    _fields_ = [(n, C.c_uint32) for n in ("J", "n_tiles", "image", "rsv")] + \
               [(n, C.c_uint64) for n in ("o_starts", "o_tile_sum", "o_tile_flags", "o_images", "bytes")]


class Stats(C.Structure):  # rpv_stats_t
    _fields_ = [(n, C.c_uint64) for n in ("in_place", "images", "carried", "bytes_read")]


IOV = np.dtype([("base", "<u8"), ("len", "<u8")])


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    S = cshim.build_shim(tmp_path_factory, "appendv", "append/appendv_shim.c")
    for f in ("t_vshape_size", "t_vctl_size", "t_iov_size"):
        getattr(S, f).restype = C.c_size_t
    assert S.t_vshape_size() == C.sizeof(VShape) and S.t_vctl_size() <= 256 and S.t_iov_size() == 16 == IOV.itemsize
    S.t_vshape.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(VShape)]
    S.t_vbound.restype = C.c_uint64
    S.t_vbound.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32]
    S.t_table_check.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    S.t_table_check_tiled.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32]
    S.t_fold.restype = C.c_int64
    S.t_fold.argtypes = [C.c_int64, C.c_int]
    S.t_placement.restype = C.c_uint64
    S.t_placement.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    S.t_vsession.restype = C.c_int64
    S.t_vsession.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p,
                             C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(Stats)]
    S.t_bad_table.restype = C.c_int64
    S.t_bad_table.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_uint64, C.c_void_p,
                              C.c_uint64, C.POINTER(C.c_int)]
    return S


def test_scratch_size(product, L, shim):
    for bs in BLOCK_SIZES:
        o = _opts(block_size=bs)
        for mp in (bs, bs + 1, 2 * bs - 1, 7 * bs, 1023 * bs, 1 << 26, 256 << 20):
            if mp < bs:
                continue
            prev = 0
            for n in (0, 1, 1024, 1025, 1 << 20):
                w = _ss(L, n, mp, o)
                J = mp // bs + 2
                bound = 8 * (n + 1) + TILE_BYTES * -(-n // 1024) + J * (bs + IMAGE_SLACK) + FIXED
                assert bound == int(shim.t_vbound(n, mp, bs))
                assert 0 < w <= bound, (bs, mp, n, w, bound)
                assert w >= 8 * (n + 1) + J * (bs + 64), (bs, mp, n)  # at least its parts
                sh = VShape()
                assert shim.t_vshape(n, mp, bs, C.byref(sh)) == 0 and sh.bytes == w and (sh.J, sh.n_tiles) == (J, -(-n // 1024))
                parts = [sh.o_starts, sh.o_tile_sum, sh.o_tile_flags, sh.o_images, sh.bytes - 256]
                assert all(p % 256 == 0 for p in parts) and parts == sorted(parts) and parts[0] >= 256
                assert sh.o_tile_sum - sh.o_starts >= 8 * (n + 1) and sh.o_tile_flags - sh.o_tile_sum >= 8 * sh.n_tiles
                assert sh.o_images - sh.o_tile_flags >= 4 * sh.n_tiles and sh.image >= bs + 64 and sh.image % 256 == 0
                assert sh.bytes - 256 - sh.o_images == J * sh.image
                assert w >= prev
                prev = w
                # the call accepts exactly that size and refuses one byte less (with entries a call of that size would go on to
                # the device: the acceptance of a table with entries is the GPU tests')
                cs = _live(max_total=1 << 40, max_piece=mp, bs=bs)
                assert _appendv(L, cs, n_iov=n, total=0 if n == 0 else 5, ss=w - 1) == ERR["MEMORY"]
                if n == 0:
                    assert _appendv(L, cs, n_iov=0, total=0, ss=w) == 0
        for level, sk, ck in ((1, 0, 0), (7, 1, 1)):  # the shape does not depend on these
            assert _ss(L, 1000, 1 << 24, _opts(level, bs, sk, ck)) == _ss(L, 1000, 1 << 24, o)
    assert _ss(L, 10, 1 << 20, None) == _ss(L, 10, 1 << 20, _opts(level=0, block_size=0)) == _ss(L, 10, 1 << 20, _opts(block_size=1 << 19))
    # 0 for what begin refuses
    for bad in BAD_BLOCK_SIZES:
        assert _ss(L, 10, 1 << 22, _opts(block_size=bad)) == 0, bad
    hd = _opts()
    hd.dict, hd.dict_size = FAKE_IOV, 100
    assert _ss(L, 10, 1 << 22, hd) == 0
    o = _opts(block_size=65536)
    assert _ss(L, 10, 65535, o) == 0 and _ss(L, 10, 0, o) == 0 and _ss(L, 10, 65536, o) > 0
    assert _ss(L, 10, 1 << 63, _opts(block_size=4096)) == 0  # more jobs in a piece than a launch counts


def _iov(entries):
    a = np.zeros(max(len(entries), 1), dtype=IOV)
    for k, (b, n) in enumerate(entries):
        a[k] = (b, n)
    return a


def test_the_table_check_and_its_precedence(shim):
    X, M = 0x1000, (1 << 64) - 1  # a base (never dereferenced), the largest length
    ok = [(X, 5), (0, 0), (X, 0), (X, 4091), (X, 1)]
    cases = [
        (ok, 4097, 0),
        ([(0, 0)] * 7, 0, 0),                                           # empty entries alone: their base is not looked at
        (ok, 4098, "SRC_TOO_SMALL"), (ok, 4096, "OVERFLOW"),             # the sum one below and one above total
        ([(0, 0)] * 3, 1, "SRC_TOO_SMALL"),
        ([(X, 10), (X, 4097), (X, 1)], 4097, "OVERFLOW"),                # an entry longer than total
        ([(X, 1)], 0, "OVERFLOW"),
        ([(X, 1 << 63), (X, 1 << 63)], 1 << 63, "OVERFLOW"),             # a sum that would overflow 64 bits: 2^64 wraps to 0
        ([(X, 1 << 63), (X, 1 << 63), (X, 1 << 63)], 1 << 63, "OVERFLOW"),   # ... and to total itself
        ([(X, M - 1), (X, 3)], M - 1, "OVERFLOW"),                       # ... to 1 < total
        ([(X, 1 << 62)] * 5, 1 << 62, "OVERFLOW"),                       # ... to 2^62 = total (total is below 2^52 in a call: max_total is)
        ([(X, 5), (0, 1)], 6, "NULL_INPUT"),                             # a zero base with a length
        ([(X, 5), (0, 1)], 5, "NULL_INPUT"), ([(X, 5), (0, 1)], 7, "NULL_INPUT"),   # ... in front of both sum errors
        ([(X, M), (0, 1)], 3, "NULL_INPUT"),                             # ... and of an entry longer than total
        ([(0, M)], M, "NULL_INPUT"),
        ([(X, 100), (X, 100)], 150, "OVERFLOW"),                         # above total, each entry within it
        ([(X, 200), (X, 1)], 150, "OVERFLOW"),                           # OVERFLOW in front of SRC_TOO_SMALL cannot both hold; too long wins over nothing
    ]
    for entries, total, want in cases:
        a = _iov(entries)
        want = ERR[want] if isinstance(want, str) else want
        assert shim.t_table_check(a.ctypes.data, len(entries), total, None) == want, (entries, total)
        for tile in (1, 2, 3, 1024):
            assert shim.t_table_check_tiled(a.ctypes.data, len(entries), total, tile) == want, (entries, total, tile)
    # the start offsets: exclusive prefix sums, the total behind them
    a = _iov(ok)
    starts = np.zeros(len(ok) + 1, dtype=np.uint64)
    assert shim.t_table_check(a.ctypes.data, len(ok), 4097, starts.ctypes.data) == 0
    assert starts.tolist() == [0, 5, 5, 5, 4096, 4097]
    # a seeded table of several tiles, grouped as the kernels group it
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 1 << 20, 5000, dtype=np.uint64)
    a = np.zeros(5000, dtype=IOV)
    a["base"], a["len"] = X, lens
    tot = int(lens.sum())
    for total, want in ((tot, 0), (tot - 1, ERR["OVERFLOW"]), (tot + 1, ERR["SRC_TOO_SMALL"])):
        assert shim.t_table_check(a.ctypes.data, 5000, total, None) == shim.t_table_check_tiled(a.ctypes.data, 5000, total, 1024) == want
    a["base"][4321] = 0
    assert shim.t_table_check_tiled(a.ctypes.data, 5000, tot - 1, 1024) == ERR["NULL_INPUT"]
    # the session's sticky status: an error it already has stays, a table error is taken, a valid table changes nothing
    assert shim.t_fold(0, 0) == 0 and shim.t_fold(0, ERR["OVERFLOW"]) == ERR["OVERFLOW"]
    assert shim.t_fold(ERR["DST_TOO_SMALL"], ERR["NULL_INPUT"]) == ERR["DST_TOO_SMALL"]
    assert shim.t_fold(ERR["SRC_TOO_SMALL"], 0) == ERR["SRC_TOO_SMALL"]


def _tables(total, bs, rng):
    """name -> list of calls; a call is a list of entry lengths (one appendv) or an int (one plain append)"""
    def fill(lens):
        lens, left = list(lens), total
        out = []
        for n in lens:
            n = min(n, left)
            out.append(n)
            left -= n
        return out + ([left] if left else [])
    out = {"one entry": [[total]],
           "empty entries anywhere": [[0, 0] + fill([5, 0, bs - 5, 0, 0, bs + 7, 0]) + [0]],
           "ends 31 / 32 / 33 behind a boundary": [fill([bs + 31, bs + 1, bs + 1, 2 * bs - 1])],
           "starts 31 / 32 / 33 short of holding a block": [fill([7, bs + 31, 1, bs + 32, 1, bs + 33])]}
    tiny, left = [], total
    while left and sum(tiny) < 2 * bs + bs // 2:
        n = min(left, rng.randrange(1, 8))
        tiny.append(n)
        left -= n
    out["1-7 bytes each over several blocks"] = [tiny + ([left] if left else [])]
    for k in range(3):
        calls, left = [], total
        while left:
            if rng.random() < 0.4:
                n = min(left, rng.randrange(1, 2 * bs))
                calls.append(n)
                left -= n
            else:
                ent, want = [], rng.randrange(1, 4 * bs)
                while left and want:
                    n = min(left, want, rng.choice((0, rng.randrange(1, 8), rng.randrange(1, 40), rng.randrange(bs), rng.randrange(3 * bs))))
                    ent.append(n)
                    left -= n
                    want -= n
                calls.append(ent)
        out["mixed %d" % k] = calls
    return out


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
        self.regular = len(self.blocks) == -(-self.size // self.bs)


def _vsession(shim, a, calls, max_piece, cap, seekable=None):
    """-> (result, destination of cap + 64 bytes that started as the canary, what the stand-in encoder saw)"""
    blocks = np.frombuffer(b"".join(a.blocks) + b"\0", dtype=np.uint8)
    blk_size = np.array([len(b) for b in a.blocks] + [0], dtype=np.uint32)
    blk_at = np.concatenate(([0], np.cumsum(blk_size[:-1], dtype=np.uint64))).astype(np.uint64)
    src = np.frombuffer(a.data + b"\0", dtype=np.uint8)
    lens, counts = [], []
    for c in calls:
        if isinstance(c, int):
            lens.append(c)
            counts.append(0)
        else:
            assert len(c) > 0
            lens += c
            counts.append(len(c))
    ln, ct = np.array(lens + [0], dtype=np.uint64), np.array(counts + [0], dtype=np.uint32)
    dst = np.full(cap + 64, CANARY, dtype=np.uint8)
    st = Stats()
    sk = a.seekable if seekable is None else seekable
    rc = int(shim.t_vsession(src.ctypes.data, a.size, blocks.ctypes.data, blk_at.ctypes.data, blk_size.ctypes.data, len(a.blocks), a.bs,
                             int(a.checksum), int(sk), ln.ctypes.data, ct.ctypes.data, len(counts), max_piece, dst.ctypes.data, cap, C.byref(st)))
    return rc, dst, st


def _expected_places(calls, bs):
    """(in place, image) jobs of a session, from the rule: a whole block of an appendv that starts at offset v of its table is in
    place exactly when the entry that holds v also holds [v, v + bs + 32); blocks of plain appends are not counted by the replay's
    statistics, nor is the block a call completes from the carry"""
    at, in_place, images = 0, 0, 0
    for c in calls:
        if isinstance(c, int):
            at += c
            continue
        ends = np.cumsum(c).tolist()  # entry r is [ends[r] - c[r], ends[r])
        total = ends[-1]
        v = (bs - at % bs) % bs  # the first block that starts inside the table
        while v + bs <= total:
            r = bisect.bisect_right(ends, v)  # the first entry that ends behind v: the one that holds it (empty ones end at or before v)
            if v + bs + 32 <= ends[r]:
                in_place += 1
            else:
                images += 1
            v += bs
        at += total
    return in_place, images


def _check_arc(shim, a, seed, seekable=None):
    rng = random.Random(seed)
    n = len(a.comp)
    seen = Stats()
    for name, calls in _tables(a.size, a.bs, rng).items():
        assert sum(c if isinstance(c, int) else sum(c) for c in calls) == a.size
        want_places = _expected_places(calls, a.bs)
        for mp in (a.bs, 2 * a.bs, max(a.size, a.bs)):  # chunk loops of one and two blocks, and none
            rc, dst, st = _vsession(shim, a, calls, mp, n, seekable=seekable)  # a capacity of exactly the archive
            assert rc == n, (a.what, name, mp, rc)
            assert dst[:n].tobytes() == a.comp and (dst[n:] == CANARY).all(), (a.what, name, mp)
            assert (st.in_place, st.images) == want_places, (a.what, name, mp)  # whatever the chunk loop: a block's place is its offset's
            assert st.in_place + st.images + st.carried <= len(a.blocks)
            seen.in_place += st.in_place
            seen.images += st.images
        rc, dst, _ = _vsession(shim, a, calls, 2 * a.bs, n - 1, seekable=seekable)  # one byte less: refused, nothing at or past the capacity
        assert rc == ERR["DST_TOO_SMALL"] and (dst[n - 1:] == CANARY).all(), (a.what, name, rc)
    return seen


_REF_ARCS = {}


def _ref_arcs(ref, bs, checksum, seekable):
    from zxc_amd import corpus
    key = (bs, checksum, seekable)
    if key not in _REF_ARCS:
        text = corpus.synth_text(40 * bs if bs == 4096 else 6 * bs, seed=13)
        noise = np.random.default_rng(bs).integers(0, 256, 6 * bs, dtype=np.uint8).tobytes()
        out = []
        for k, n in enumerate((1, bs - 1, bs + 33, 3 * bs + 5, 6 * bs - 1) + ((40 * bs - 3,) if bs == 4096 else ())):
            data = (noise if k % 3 == 2 and n <= len(noise) else text)[:n]
            out.append(Arc(ref.compress(data, 1 + k % 5, bs, bool(seekable), bool(checksum)), (n, bs, checksum, seekable), data))
        _REF_ARCS[key] = out
    return _REF_ARCS[key]


@pytest.mark.parametrize("bs", [4096, 65536])
@pytest.mark.parametrize("checksum,seekable", [(0, 0), (1, 1)])
def test_sessions_put_the_reference_archives_together_again(shim, ref, bs, checksum, seekable):
    arcs = _ref_arcs(ref, bs, checksum, seekable)
    assert all(a.regular and a.bs == bs and a.checksum == bool(checksum) for a in arcs)
    in_place = images = 0
    for k, a in enumerate(arcs):
        seen = _check_arc(shim, a, seed=bs + 8 * k + 2 * checksum + seekable, seekable=seekable)
        in_place += seen.in_place
        images += seen.images
    assert in_place > 0 and images > 0  # both places were exercised


def test_sessions_put_the_golden_archives_together_again(shim, oracle):
    seen = 0
    for d in ("conformance/valid", "format", "synth"):
        p = os.path.join(GOLDEN, d)
        for f in sorted(os.listdir(p)) if os.path.isdir(p) else ():
            if not f.endswith(".zxc"):
                continue
            try:
                a = Arc(open(os.path.join(p, f), "rb").read(), f"{d}/{f}")
            except (AssertionError, IndexError):
                continue  # (a format vector that is no complete archive)
            if not a.regular or a.has_dict or a.size == 0 or a.size > (256 << 10) or seen >= 12:
                continue
            rc, a.data = oracle.decompress(a.comp, a.size, checksum=a.checksum)
            if rc != a.size:
                continue
            _check_arc(shim, a, seed=seen, seekable=int(a.seekable))
            seen += 1
    assert seen >= 8, seen


def test_placement_is_the_rule_at_every_cut_point(shim):
    bs = 4096
    rng = random.Random(9)
    tables = [[3 * bs + 40], [bs + 31], [bs + 32], [bs + 33, 0, bs + 32], [7, bs + 31, 1, bs + 32, 1, bs + 33, 0, 0, 2 * bs + 32],
              [1] * 50 + [bs + 32] + [0] * 9 + [3] * 40 + [2 * bs + 64]]
    for _ in range(6):
        tables.append([rng.choice((0, rng.randrange(1, 8), rng.randrange(bs - 40, bs + 80), rng.randrange(3 * bs))) for _ in range(rng.randrange(1, 30))])
    some = 0
    for lens in tables:
        if sum(lens) < bs:
            lens = lens + [bs]
        a = np.array(lens, dtype=np.uint64)
        n = C.c_uint64(0)
        bad = int(shim.t_placement(a.ctypes.data, len(lens), bs, C.byref(n)))
        assert bad == 0, (lens, bad - 1)
        some += n.value
    assert some > 0
    n = C.c_uint64(0)
    for lens, want in (([bs + 31], 0), ([bs + 32], 1), ([bs + 33], 2), ([bs + 31, 100], 0), ([5, bs + 32], 1)):
        a = np.array(lens, dtype=np.uint64)
        assert shim.t_placement(a.ctypes.data, len(lens), bs, C.byref(n)) == 0 and n.value == want, lens


def test_a_table_error_reads_nothing_and_stays(shim):
    bs, X = 4096, 0x10  # a base nothing lies at: reading an entry of a refused table would fault
    src = np.full(100, 7, dtype=np.uint8)
    cases = [([(X, 3 * bs), (X, 5), (0, 0), (X, bs)], 4 * bs + 6, "SRC_TOO_SMALL"),
             ([(X, 3 * bs), (X, 5), (0, 0), (X, bs)], 4 * bs + 4, "OVERFLOW"),
             ([(X, 1), (X, 3 * bs + 1)], 3 * bs, "OVERFLOW"),
             ([(X, bs), (0, 1), (X, bs)], 2 * bs + 1, "NULL_INPUT"),
             ([(X, (1 << 64) - 1), (0, 1), (X, bs)], 2 * bs, "NULL_INPUT")]
    for entries, promised, want in cases:
        a = _iov(entries)
        for mp in (bs, 8 * bs):
            for before in (0, 100):
                dst = np.full(128, CANARY, dtype=np.uint8)
                verdict = C.c_int(0)
                rc = int(shim.t_bad_table(src.ctypes.data, before, a.ctypes.data, len(entries), promised, bs, 1, 1, mp, dst.ctypes.data, 64,
                                          C.byref(verdict)))
                assert verdict.value == ERR[want] and rc == ERR[want], (entries, promised, mp, before, rc)  # never CORRUPT_DATA
                assert (dst == CANARY).all()


def test_rules_under_sanitizers(tmp_path):
    """the stand-alone program tests/append/appendv_san_main.c (its own main; nothing of it is loaded into this process)"""
    r = cshim.run_san_program(tmp_path, "append/appendv_san_main.c")
    assert "APPENDV OK 664" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
