"""zxc_mi355x_compress_appendv_dict_device (append a table of buffers to an append session begun with a dictionary) without a GPU:
the two symbols and the Python names, every synchronous argument check in its stated order (the device pointers below are never
dereferenced; a live session is forged in the caller-owned struct, since begin needs a device), the scratch-size arithmetic against
the bound the header states, and the rules the entry point and the new kernel run (zav_shape_dict, zav_prep_images of
zxc_amd/csrc/zxc_appendv.h), compiled here with the host C compiler: whole dictionary sessions mixing append and appendv_dict
replayed on the host (tests/append/appendv_dict_replay.h) over dictionary archives that the unmodified reference wrote, the
dictionary goldens and archives of stored blocks, cut into their blocks. Every image must be [dict | the block's bytes] before the
stand-in encoder runs, and the output the archive byte for byte, with a pattern intact everywhere else. The same replay runs under
AddressSanitizer and UBSan in a stand-alone program in which every entry is a malloc of exactly its length."""
import ctypes as C
import os

import numpy as np
import pytest

import cshim
from conftest import GOLDEN, load_dict
from cshim import opts as _opts, ref as _ref
from devtest import ERR
from zxc_amd.api import _DevCappend as Cs  # zxc_dev_cappend_t

FAKE_IOV, FAKE_DST, FAKE_WORK, FAKE_SCRATCH, FAKE_DICT = 0x10000, 0x30000, 0x40000, 0x50000, 0x60000
BLOCK_SIZES = (4096, 65536, 1 << 19, 1 << 21)
BAD_BLOCK_SIZES = (1000, 2048, 4095, 5000, 3 << 12, 1 << 22)
DICT_SIZES = (1, 100, 65535)
TILE_BYTES, FIXED = 16, 4096  # the stated bound: 8 (n + 1) + 16 ceil(n / 1024) + 4096
SESS_LIVE = 0x7A78632D61707064  # a session between begin and end (zxc_append_device.hip)
DICTS = (("dict_http.zxc", "dict_http.expected", "dict_http.zxd"), ("dict_seekable_l7.zxc", "dict_seekable_l7.expected", "dict_text.zxd"))
NO_UNUSED = ["-Wno-unused-function"]  # (the replay headers the C sources include serve other programs too)


@pytest.fixture(scope="module")
def L(product):
    L = product.lib()
    assert hasattr(L, "zxc_mi355x_compress_appendv_dict_device"), "libzxc_mi355x.so does not export zxc_mi355x_compress_appendv_dict_device"
    return L


def _live(total=0, max_total=1 << 24, max_piece=1 << 20, bs=65536, dict_size=100):
    """the struct begin leaves (struct Sess of zxc_append_device.hip): begin itself needs a device, these tests have none"""
    cs = Cs()
    words = [SESS_LIVE, FAKE_DST, 1 << 20, max_total, max_piece, FAKE_WORK, total, bs | 3 << 32, 0, dict_size << 32,
             FAKE_DICT if dict_size else 0, FAKE_DICT + 0x1000 if dict_size else 0]
    for k, w in enumerate(words):
        cs.opaque[k] = w
    return cs


def _ss(L, n_iov, max_piece, o, dict_size):
    return int(L.zxc_mi355x_compress_appendv_dict_device_scratch_size(n_iov, max_piece, _ref(o), dict_size))


def _ss_plain(L, n_iov, max_piece, o):
    return int(L.zxc_mi355x_compress_appendv_device_scratch_size(n_iov, max_piece, _ref(o)))


def _appendv(L, cs, iov=FAKE_IOV, n_iov=4, total=100, scratch=FAKE_SCRATCH, ss=1 << 40):
    before = None if cs is None else list(cs.opaque)
    rc = L.zxc_mi355x_compress_appendv_dict_device(_ref(cs), iov, n_iov, total, scratch, ss, None)
    if cs is not None and rc < 0:
        assert list(cs.opaque) == before, "a refusal changed the session struct"
    return rc


def test_symbols_and_names_exported(product):
    L = product.lib()
    for sym in ("zxc_mi355x_compress_appendv_dict_device_scratch_size", "zxc_mi355x_compress_appendv_dict_device"):
        assert hasattr(L, sym), sym
    name = "compress_appendv_dict_device_scratch_size"
    assert hasattr(product, name) and hasattr(product.api, name), name
    assert hasattr(product.api.CompressAppendSession, "appendv_dict")
    b = product.lib()
    f, g = b.zxc_mi355x_compress_appendv_dict_device, b.zxc_mi355x_compress_appendv_dict_device_scratch_size
    assert f.argtypes is not None and len(f.argtypes) == 7 and f.restype is C.c_int
    assert g.argtypes is not None and len(g.argtypes) == 4 and g.restype is C.c_uint64


def test_each_synchronous_error_and_their_order(L):
    for dict_size in (100, 0):  # a session with a dictionary is not refused, and one without is served too
        live = _live(dict_size=dict_size)
        # each rule on its own
        assert _appendv(L, None) == ERR["NULL_INPUT"]
        assert _appendv(L, live, scratch=None) == ERR["NULL_INPUT"]
        assert _appendv(L, live, iov=None) == ERR["NULL_INPUT"]
        never, junk = Cs(), Cs()
        C.memset(C.byref(junk), 0xEE, C.sizeof(junk))
        assert _appendv(L, never) == ERR["NULL_INPUT"] and _appendv(L, junk) == ERR["NULL_INPUT"]
        assert _appendv(L, live, iov=None, n_iov=0, total=1) == ERR["SRC_TOO_SMALL"]
        assert _appendv(L, live, total=(1 << 24) + 1) == ERR["OVERFLOW"]
        assert _appendv(L, _live(total=(1 << 24) - 5, dict_size=dict_size), total=6) == ERR["OVERFLOW"]
        assert _appendv(L, _live(total=1 << 24, dict_size=dict_size), total=(1 << 64) - 1) == ERR["OVERFLOW"]  # compared without overflow
        assert _appendv(L, live, ss=0) == ERR["MEMORY"]
        # each call breaks one rule and every later one; the earliest is reported
        full = _live(total=1 << 24, dict_size=dict_size)
        assert _appendv(L, None, iov=None, n_iov=0, total=1 << 60, scratch=None, ss=0) == ERR["NULL_INPUT"]
        assert _appendv(L, full, iov=None, n_iov=3, total=1 << 60, ss=0) == ERR["NULL_INPUT"]
        assert _appendv(L, full, iov=None, n_iov=0, total=1 << 60, scratch=None, ss=0) == ERR["NULL_INPUT"]
        assert _appendv(L, junk, iov=None, n_iov=0, total=1 << 60, ss=0) == ERR["NULL_INPUT"]  # never begun, then everything else
        assert _appendv(L, full, iov=None, n_iov=0, total=1 << 60, ss=0) == ERR["SRC_TOO_SMALL"]  # (the sibling: GPU_UNSUPPORTED with a dictionary)
        assert _appendv(L, full, n_iov=5, total=1, ss=0) == ERR["OVERFLOW"]
        assert _appendv(L, live, n_iov=5, total=1, ss=0) == ERR["MEMORY"]
        # nothing to append: ZXC_OK, nothing enqueued, with or without a table pointer, and the struct as it was
        for iov in (None, FAKE_IOV):
            cs = _live(total=77, dict_size=dict_size)
            before = list(cs.opaque)
            assert _appendv(L, cs, iov=iov, n_iov=0, total=0) == 0 and list(cs.opaque) == before
    # the sibling still refuses the dictionary session, behind the same two checks
    rc = L.zxc_mi355x_compress_appendv_device(C.byref(_live(dict_size=100)), FAKE_IOV, 4, 100, FAKE_SCRATCH, 1 << 40, None)
    assert rc == ERR["GPU_UNSUPPORTED"]


def test_python_binding_raises(product):
    s = product.api.CompressAppendSession(product.api._DevCappend())  # never begun
    with pytest.raises(product.ZxcError) as e:
        s.appendv_dict(FAKE_IOV, 3, 10, FAKE_SCRATCH, 1 << 30)
    assert e.value.code == ERR["NULL_INPUT"]
    s = product.api.CompressAppendSession(_live(dict_size=9))
    with pytest.raises(product.ZxcError) as e:
        s.appendv_dict(FAKE_IOV, 3, 10, 0, 1 << 30)
    assert e.value.code == ERR["NULL_INPUT"]
    with pytest.raises(product.ZxcError) as e:
        s.appendv_dict(FAKE_IOV, 3, 10, FAKE_SCRATCH, 16)
    assert e.value.code == ERR["MEMORY"]
    with pytest.raises(product.ZxcError) as e:
        s.appendv_dict(0, 0, 10, FAKE_SCRATCH, 1 << 30)
    assert e.value.code == ERR["SRC_TOO_SMALL"]
    s.appendv_dict(0, 0, 0, FAKE_SCRATCH, 1 << 30)  # nothing to append
    f = product.compress_appendv_dict_device_scratch_size
    assert f(10, 1 << 20, 100, block_size=5000) == 0 and f(10, 1 << 20, 65536, block_size=4096) == 0
    assert 0 < f(10, 1 << 20, 100, block_size=4096) < f(10, 1 << 20, 0, block_size=4096)
    assert f(10, 1 << 20, 0, 3, 4096, True, True) == product.compress_appendv_device_scratch_size(10, 1 << 20, 3, 4096, True, True)


# ---------------------------------------------------------------- the shared rules, run on the CPU
class VShape(C.Structure):  # zav_shape_t
    _fields_ = [(n, C.c_uint32) for n in ("J", "n_tiles", "image", "rsv")] + \
               [(n, C.c_uint64) for n in ("o_starts", "o_tile_sum", "o_tile_flags", "o_images", "bytes")]


class Stats(C.Structure):  # rpvd_stats_t
    _fields_ = [(n, C.c_uint64) for n in ("in_place", "images", "carried", "bytes_read", "max_chunks", "tails", "unused")]


IOV = np.dtype([("base", "<u8"), ("len", "<u8")])


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    S = cshim.build_shim(tmp_path_factory, "appendv_dict", "append/appendv_dict_shim.c", NO_UNUSED)
    for f in ("t_vshape_size", "t_stats_size"):
        getattr(S, f).restype = C.c_size_t
    assert S.t_vshape_size() == C.sizeof(VShape) and S.t_stats_size() == C.sizeof(Stats)
    S.t_vshape_dict.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(VShape)]
    S.t_vbound_dict.restype = C.c_uint64
    S.t_vbound_dict.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32]
    S.t_check_archive.restype = C.c_int64
    S.t_check_archive.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Stats)]
    S.t_selftest.restype = C.c_int64
    S.t_selftest.argtypes = [C.c_uint32, C.POINTER(Stats)]
    S.t_bad_table.restype = C.c_int64
    S.t_bad_table.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_uint64,
                              C.c_uint32, C.c_int, C.POINTER(C.c_int)]
    return S


def test_scratch_size(L, shim):
    for bs in BLOCK_SIZES:
        o = _opts(block_size=bs)
        for mp in (bs, bs + 1, 2 * bs - 1, 7 * bs, 1023 * bs, 1 << 26, 256 << 20):
            if mp < bs:
                continue
            for n in (0, 1, 1023, 1024, 1025, 65536, 1 << 20):
                plain = _ss_plain(L, n, mp, o)
                assert _ss(L, n, mp, o, 0) == plain > 0  # no dictionary: the sibling's value
                assert int(shim.t_vbound_dict(n, mp, bs, 0)) >= plain
                first = None
                for D in DICT_SIZES:
                    w = _ss(L, n, mp, o, D)
                    bound = 8 * (n + 1) + TILE_BYTES * -(-n // 1024) + FIXED
                    assert bound == int(shim.t_vbound_dict(n, mp, bs, D))
                    assert 0 < w <= bound, (bs, mp, n, D, w, bound)
                    assert w >= 16 + 8 * (n + 1) + 12 * -(-n // 1024)  # at least its parts
                    assert w < plain  # no images
                    first = w if first is None else first
                    assert w == first  # the size does not depend on the dictionary's size, only on there being one
                    sh = VShape()
                    assert shim.t_vshape_dict(n, mp, bs, D, C.byref(sh)) == 0 and sh.bytes == w and sh.n_tiles == -(-n // 1024)
                    parts = [sh.o_starts, sh.o_tile_sum, sh.o_tile_flags, sh.bytes - 256]
                    assert all(p % 256 == 0 for p in parts) and parts == sorted(parts) and parts[0] >= 256
                    assert sh.o_tile_sum - sh.o_starts >= 8 * (n + 1) and sh.o_tile_flags - sh.o_tile_sum >= 8 * sh.n_tiles
                    assert sh.bytes - 256 - sh.o_tile_flags >= 4 * sh.n_tiles
                    # the call requires exactly the size of the session's own dict_size
                    cs = _live(max_total=1 << 40, max_piece=mp, bs=bs, dict_size=D)
                    assert _appendv(L, cs, n_iov=n, total=0 if n == 0 else 5, ss=w - 1) == ERR["MEMORY"]
                    if n == 0:
                        assert _appendv(L, cs, n_iov=0, total=0, ss=w) == 0
                cs = _live(max_total=1 << 40, max_piece=mp, bs=bs, dict_size=0)  # ... which without a dictionary is the sibling's
                assert _appendv(L, cs, n_iov=n, total=0 if n == 0 else 5, ss=plain - 1) == ERR["MEMORY"]
                if n == 0:
                    assert _appendv(L, cs, n_iov=0, total=0, ss=plain) == 0
                assert _ss(L, n, mp, o, 65536) == 0 and _ss(L, n, mp, o, (1 << 32) - 1) == 0
        for level, sk, ck in ((1, 0, 0), (7, 1, 1)):  # the shape does not depend on these
            assert _ss(L, 1000, 1 << 24, _opts(level, bs, sk, ck), 100) == _ss(L, 1000, 1 << 24, o, 100)
    assert _ss(L, 10, 1 << 20, None, 7) == _ss(L, 10, 1 << 20, _opts(level=0, block_size=0), 7) == _ss(L, 10, 1 << 20, _opts(block_size=1 << 19), 7)
    # 0 for what begin refuses
    for bad in BAD_BLOCK_SIZES:
        for D in (0,) + DICT_SIZES:
            assert _ss(L, 10, 1 << 22, _opts(block_size=bad), D) == 0, (bad, D)
    hd = _opts()
    hd.dict, hd.dict_size = FAKE_IOV, 100
    assert _ss(L, 10, 1 << 22, hd, 100) == 0
    o = _opts(block_size=65536)
    assert _ss(L, 10, 65535, o, 100) == 0 and _ss(L, 10, 0, o, 100) == 0 and _ss(L, 10, 65536, o, 100) > 0
    assert _ss(L, 10, 1 << 63, _opts(block_size=4096), 100) == 0  # more jobs in a piece than a launch counts


def _golden_dicts():
    for arc, exp, zxd in DICTS:
        d = os.path.join(GOLDEN, "conformance", "valid")
        comp, data = open(os.path.join(d, arc), "rb").read(), open(os.path.join(d, exp), "rb").read()
        content, _ = load_dict(os.path.join(d, zxd))
        yield arc, comp, data, content


def _sessions(rc):
    assert rc > 0, "appendv_dict_replay.h line %d" % -rc
    return rc


def test_sessions_put_the_dictionary_goldens_together_again(shim):
    st = Stats()
    for k, (arc, comp, data, content) in enumerate(_golden_dicts()):
        assert comp[6] & 0x40 and int.from_bytes(comp[7:11], "little") != 0, arc  # the flag and the id the session must reproduce
        for chunk in (0, 1):
            assert _sessions(int(shim.t_check_archive(comp, len(comp), data, len(data), content, len(content), 5 + k, chunk, C.byref(st)))) == 17, arc
    # (one short block each: every call joins the carry through zxc_appendv_prep_kernel's rule and `end` builds the image; the
    # archives of several blocks are below)


def test_sessions_put_archives_of_several_blocks_together_again(shim):
    """stored blocks behind a dictionary header (rp_stored_archive with has_dict): 4 KiB and 64 KiB blocks, dictionaries of 1, 100,
    4099 and 65535 bytes, every cut set of rpvd_calls"""
    st = Stats()
    assert _sessions(int(shim.t_selftest(0, C.byref(st)))) == 30 * 17
    assert st.images > 1000 and st.carried > 100 and st.tails > 100 and st.max_chunks == 1 and st.unused == 0


def test_a_chunk_of_three_launches_and_more(shim):
    """chunk_jobs forced to two: a chunk of 40 blocks takes 20 launches, and the tail workgroup is in the first alone"""
    st = Stats()
    assert _sessions(int(shim.t_selftest(2, C.byref(st)))) == 30 * 17
    assert st.max_chunks >= 3 and st.max_chunks == 20 and st.images > 1000


def test_sessions_put_the_reference_dictionary_archives_together_again(shim, ref):
    """archives the unmodified reference writes with a dictionary, of several blocks of 4 KiB"""
    from oracle_py import CompressOpts
    from zxc_amd import corpus
    content, huf = load_dict(os.path.join(GOLDEN, "conformance", "valid", "dict_text.zxd"))
    text = corpus.synth_text(12 * 4096, seed=23)
    st = Stats()
    for k, (n, level, sk, ck, with_huf) in enumerate(((3 * 4096 + 5, 3, 1, 1, 0), (11 * 4096 + 100, 1, 0, 0, 1), (4096, 5, 1, 0, 0))):
        data = text[:n]
        keep = (C.create_string_buffer(content, len(content)), C.create_string_buffer(huf, 128))
        o = CompressOpts(level=level, block_size=4096, seekable=sk, checksum_enabled=ck, dict=C.cast(keep[0], C.c_void_p), dict_size=len(content),
                         dict_huf=C.cast(keep[1], C.c_void_p) if with_huf else None)
        cap = ref.lib.zxc_compress_bound(n)
        dst = C.create_string_buffer(cap)
        size = ref.lib.zxc_compress(data, n, dst, cap, C.byref(o))
        assert size > 0
        comp = dst.raw[:size]
        assert comp[6] & 0x40
        for chunk in (0, 2):
            assert _sessions(int(shim.t_check_archive(comp, size, data, n, content, len(content), 40 + k, chunk, C.byref(st)))) == 17, n
    assert st.max_chunks >= 3 and st.carried > 0


def _iov(entries):
    a = np.zeros(max(len(entries), 1), dtype=IOV)
    for k, (b, n) in enumerate(entries):
        a[k] = (b, n)
    return a


def test_a_table_error_reads_nothing_and_stays(shim):
    """a bad table in front of good calls, inside them, behind them with and without a carry, and behind an error the session already
    holds: no entry byte is touched, every job of the call is the unused job, nothing reaches the destination, the status stays"""
    bs, X = 4096, 0x10  # a base nothing lies at: reading an entry of a refused table would fault
    cases = [([(X, 3 * bs), (X, 5), (0, 0), (X, bs)], 4 * bs + 6, "SRC_TOO_SMALL"),
             ([(X, 3 * bs), (X, 5), (0, 0), (X, bs)], 4 * bs + 4, "OVERFLOW"),
             ([(X, 1), (X, 3 * bs + 1)], 3 * bs, "OVERFLOW"),
             ([(X, bs), (0, 1), (X, bs)], 2 * bs + 1, "NULL_INPUT"),
             ([(X, (1 << 64) - 1), (0, 1), (X, bs)], 2 * bs, "NULL_INPUT")]
    for k, (entries, promised, want) in enumerate(cases):
        a = _iov(entries)
        pad = -promised % bs
        for mp in (bs, 8 * bs):
            for place, (before, after, chunk, small) in enumerate(((0, 0 if pad else 3 * bs, 0, 0), (bs + pad, 2 * bs, 2, 0), (bs + pad, 0, 0, 0),
                                                                   (100, 0, 0, 0), (2 * bs, 0, 0, 1))):
                for D in (1, 100, 4099, 65535)[(k + place) % 2::2]:
                    verdict = C.c_int(0)
                    rc = int(shim.t_bad_table(bs, D, before, a.ctypes.data, len(entries), promised, after, 1, 1, mp, chunk, small, C.byref(verdict)))
                    assert verdict.value == ERR[want], (entries, promised, mp, place)
                    assert rc == (ERR["DST_TOO_SMALL"] if small else ERR[want]), (entries, promised, mp, place, D, rc)  # never CORRUPT_DATA


def test_rules_under_sanitizers(tmp_path):
    """the stand-alone program tests/append/appendv_dict_san_main.c (its own main; nothing of it is loaded into this process)"""
    args = []
    for k, (arc, comp, data, content) in enumerate(_golden_dicts()):
        p = tmp_path / ("dict%d.bin" % k)
        p.write_bytes(content)
        d = os.path.join(GOLDEN, "conformance", "valid")
        args += [os.path.join(d, arc), os.path.join(d, arc.replace(".zxc", ".expected")), str(p)]
    r = cshim.run_san_program(tmp_path, "append/appendv_dict_san_main.c", args, NO_UNUSED)
    want = 2 * 30 * 17 + len(DICTS) * 17 + 7 * 2 * 5  # the program's own archives twice, the goldens, the bad tables
    assert "APPENDV DICT OK %d" % want in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
