"""The byte-shuffle calls of include/zxc_mi355x_shuffle.h without a GPU: the six symbols and the Python names, the third prototype
table against that header by the rules of test_api_prototypes.py, every synchronous argument check of the four calls in its stated
order (the device pointers below are never dereferenced), the work sizes against the session size functions, and the rules the
kernels run (zxc_amd/csrc/zxc_shuffle.h), compiled here with the host C compiler: the index map against a numpy transpose, and the
per-lane plan replayed for every wave and lane (tests/shuffle/shuffle_replay.h) between canaries at every alignment. The same replay
runs under AddressSanitizer and UBSan in a stand-alone program. Where the reference is built: an archive of shuffled bytes is an
ordinary archive to it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cshim
import shuffle_support as ss
from conftest import ROOT
from devtest import ERR
from zxc_amd import api

FAKE_SRC, FAKE_DST, FAKE_WORK, FAKE_RES = 0x10000, 0x40000, 0x50000, 0x60000
BAD_BLOCK_SIZES = (1000, 2048, 4095, 5000, 3 << 12, 1 << 22)
BAD_ELEMS = (0, 1, 3, 5, 6, 7, 16, 1 << 31)
SYMS = ("zxc_mi355x_shuffle_device", "zxc_mi355x_unshuffle_device", "zxc_mi355x_compress_shuffle_device_work_size",
        "zxc_mi355x_compress_shuffle_device", "zxc_mi355x_decompress_shuffle_device_work_size", "zxc_mi355x_decompress_shuffle_device")
NAMES = ("shuffle_device", "unshuffle_device", "compress_shuffle_device", "compress_shuffle_device_work_size",
         "decompress_shuffle_device", "decompress_shuffle_device_work_size")
DEFAULT_PIECE = 64 << 20


def test_symbols_and_names_exported(product):
    L = product.lib()
    for sym in SYMS:
        assert hasattr(L, sym), sym
    for name in NAMES:
        assert hasattr(product, name) and hasattr(product.api, name), name


# ---------------------------------------------------------------- the third prototype table against the new header
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "size_t": C.c_size_t, "void": None}


def _ctype(decl):
    if "*" in decl:
        return "pointer"
    return SCALARS[[w for w in decl.split() if w != "const"][0]]


def _header():
    text = open(os.path.join(ROOT, "include", "zxc_mi355x_shuffle.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    protos = {}
    for ret, name, args in re.findall(r"ZXC_EXPORT\s+([\w\s]+?\*?)\s*(zxc_mi355x_\w+)\s*\(([^)]*)\)\s*;", text):
        protos[name] = (_ctype(ret), [] if args.strip() == "void" else [_ctype(a) for a in args.split(",")])
    return protos


def _same(want, got):
    return (got in (C.c_void_p, C.c_char_p) or hasattr(got, "contents")) if want == "pointer" else got is want


def test_prototype_table_matches_the_new_header(product):
    header, table = _header(), getattr(api, "_PROTOTYPES_SHUFFLE", None)
    assert table is not None, "zxc_amd.api has no _PROTOTYPES_SHUFFLE"
    assert sorted(header) == sorted(SYMS) == sorted(table)
    assert header[SYMS[0]] == (C.c_int, ["pointer", "pointer", C.c_uint64, C.c_uint32, C.c_uint32, "pointer"])
    assert header[SYMS[4]] == (C.c_uint64, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32])
    assert not set(table) & set(api._PROTOTYPES) and not set(table) & set(api._PROTOTYPES_RANGESV)
    L = product.lib()
    for name in SYMS:
        (want_ret, want_args), (ret, args) = header[name], table[name]
        assert _same(want_ret, ret), (name, "return type", ret)
        assert len(args) == len(want_args), (name, "arity", len(args), len(want_args))
        for i, (want, got) in enumerate(zip(want_args, args)):
            assert _same(want, got), (name, "parameter", i, got)
        f = getattr(L, name)
        assert (f.restype, list(f.argtypes)) == (ret, args), name  # bound once, at load
        assert api._prototype(name) == table[name]
    # the other headers keep their prototypes: the new calls are declared in the new header alone
    for other in ("zxc_mi355x.h", "zxc_mi355x_rangesv.h"):
        assert not re.search(r"ZXC_EXPORT[^;]*shuffle", open(os.path.join(ROOT, "include", other)).read()), other


# ---------------------------------------------------------------- synchronous errors
@pytest.fixture(scope="module")
def L(product):
    L = product.lib()
    assert hasattr(L, SYMS[3]), f"libzxc_mi355x.so does not export {SYMS[3]}"
    return L


@pytest.mark.parametrize("sym", SYMS[:2])
def test_transform_errors_in_their_order(L, sym):
    f = getattr(L, sym)

    def call(src=FAKE_SRC, dst=FAKE_DST, n=1000, e=4, unit=4096):
        return f(src, dst, n, e, unit, None)

    assert call(src=None) == call(dst=None) == ERR["NULL_INPUT"]
    for e in BAD_ELEMS:
        assert call(e=e) == ERR["GPU_UNSUPPORTED"], e
    for u in BAD_BLOCK_SIZES + (0,):
        assert call(unit=u) == ERR["BAD_BLOCK_SIZE"], u
    # each call breaks one rule and every later one; the earliest is reported
    assert call(src=None, e=3, unit=5000) == ERR["NULL_INPUT"]
    assert call(e=3, unit=5000) == ERR["GPU_UNSUPPORTED"]
    # nothing to do is fine, with or without pointers and a device; the argument checks still come first
    assert call(n=0) == 0 and call(n=0, src=None, dst=None) == 0
    assert call(n=0, e=3) == ERR["GPU_UNSUPPORTED"] and call(n=0, unit=5000) == ERR["BAD_BLOCK_SIZE"]
    for e in (2, 4, 8):
        for u in (4096, 65536, 1 << 21):
            assert call(n=0, e=e, unit=u) == 0


def _cws(L, n, mp, o, ds=0):
    return int(L.zxc_mi355x_compress_shuffle_device_work_size(n, mp, cshim.ref(o), ds))


def _ccall(L, n=100000, e=4, cap=1 << 20, mp=0, o="dflt", dict_=None, src=FAKE_SRC, dst=FAKE_DST, work=FAKE_WORK, ws=None, res=FAKE_RES):
    o = cshim.opts(block_size=4096) if isinstance(o, str) else o
    ws = max(_cws(L, n, mp, o, dict_.size if dict_ is not None and dict_.size <= 65535 else 0), 1) if ws is None else ws
    return L.zxc_mi355x_compress_shuffle_device(src, n, e, dst, cap, mp, cshim.ref(o), cshim.ref(dict_), work, ws, res, None)


@pytest.mark.parametrize("dict_", [None, "empty", "dict"])
def test_compress_errors_in_their_order(L, dict_):
    d = {"empty": cshim.dd(size=0, content=None, id_=None), "dict": cshim.dd()}.get(dict_)

    def call(**kw):
        return _ccall(L, dict_=d, **kw)

    # the new checks
    assert call(src=None) == call(res=None) == ERR["NULL_INPUT"]
    for e in BAD_ELEMS:
        assert call(e=e) == ERR["GPU_UNSUPPORTED"], e
    # the session's, in its order
    assert call(dst=None) == call(work=None) == ERR["NULL_INPUT"]
    assert call(o=cshim.host_dict(cshim.opts(block_size=4096))) == ERR["GPU_UNSUPPORTED"]
    for bad in BAD_BLOCK_SIZES:
        assert call(o=cshim.opts(block_size=bad), ws=1 << 40) == ERR["BAD_BLOCK_SIZE"], bad
    for mp in (1, 100, 4095):
        assert call(mp=mp, ws=1 << 40) == ERR["BAD_BLOCK_SIZE"], mp
    assert call(n=1 << 62, ws=1 << 62) == ERR["BAD_BLOCK_SIZE"]          # more blocks than a session counts
    for n, mp, bs in ((0, 0, 4096), (1, 0, 4096), (100000, 8192, 4096), (100000, 0, 4096), (1 << 22, 1 << 20, 65536)):
        o = cshim.opts(block_size=bs, seekable=True)
        ws = _cws(L, n, mp, o, d.size if d is not None else 0)
        assert ws > 0 and call(n=n, mp=mp, o=o, ws=ws - 1) == ERR["MEMORY"], (n, mp, bs)
    assert call(cap=10) == ERR["DST_TOO_SMALL"]
    # each call breaks one rule and every later one; the earliest is reported
    host = cshim.host_dict(cshim.opts(block_size=5000))
    assert call(src=None, e=3, dst=None, o=host, ws=0, cap=0) == ERR["NULL_INPUT"]
    assert call(e=3, dst=None, o=host, ws=0, cap=0) == ERR["GPU_UNSUPPORTED"]
    assert call(e=4, dst=None, o=host, ws=0, cap=0) == ERR["NULL_INPUT"]
    assert call(o=host, ws=0, cap=0) == ERR["GPU_UNSUPPORTED"]
    assert call(o=cshim.opts(block_size=5000), ws=0, cap=0) == ERR["BAD_BLOCK_SIZE"]
    assert call(mp=100, ws=0, cap=0) == ERR["BAD_BLOCK_SIZE"]
    assert call(ws=0, cap=0) == ERR["MEMORY"]
    assert call(n=0, src=None, cap=0) == ERR["DST_TOO_SMALL"]             # an empty source needs no pointer


def test_compress_dictionary_errors_in_their_place(L):
    """behind opts->dict, in front of the block size: the session's dictionary checks"""
    big, no_content, no_id = cshim.dd(size=65536), cshim.dd(content=None), cshim.dd(id_=None)
    assert _ccall(L, dict_=big) == ERR["DICT_TOO_LARGE"]
    assert _ccall(L, dict_=no_content) == _ccall(L, dict_=no_id) == ERR["NULL_INPUT"]
    assert _ccall(L, dict_=big, o=cshim.opts(block_size=5000), ws=0) == ERR["DICT_TOO_LARGE"]
    assert _ccall(L, dict_=big, o=cshim.host_dict(cshim.opts(block_size=4096))) == ERR["GPU_UNSUPPORTED"]
    assert _ccall(L, dict_=big, e=3) == ERR["GPU_UNSUPPORTED"]
    assert _ccall(L, dict_=cshim.dd(size=65535), ws=0) == ERR["MEMORY"]
    assert _ccall(L, dict_=cshim.dd(size=1000), ws=_cws(L, 100000, 0, cshim.opts(block_size=4096), 0)) == ERR["MEMORY"]  # the images count


def _dws(L, src_size, n, mp, bs):
    return int(L.zxc_mi355x_decompress_shuffle_device_work_size(src_size, n, mp, bs))


def _dcall(L, src_size=1000, n=100000, e=4, mp=0, bs=4096, o=None, dict_=None, src=FAKE_SRC, dst=FAKE_DST, work=FAKE_WORK, ws=None, res=FAKE_RES):
    ws = max(_dws(L, src_size, n, mp, bs), 1) if ws is None else ws
    return L.zxc_mi355x_decompress_shuffle_device(src, src_size, dst, n, e, mp, bs, cshim.ref(o), cshim.ref(dict_), work, ws, res, None)


@pytest.mark.parametrize("dict_", [None, "empty", "dict"])
def test_decompress_errors_in_their_order(L, dict_):
    d = {"empty": cshim.dd(size=0, content=None, id_=None), "dict": cshim.dd()}.get(dict_)
    host = api._DecompressOpts(dict=0x10000, dict_size=100)

    def call(**kw):
        return _dcall(L, dict_=d, **kw)

    assert call(dst=None) == call(res=None) == ERR["NULL_INPUT"]
    for e in BAD_ELEMS:
        assert call(e=e) == ERR["GPU_UNSUPPORTED"], e
    assert call(src=None) == call(work=None) == ERR["NULL_INPUT"]
    assert call(src_size=27) == ERR["SRC_TOO_SMALL"]
    for bad in BAD_BLOCK_SIZES + (0,):
        assert call(bs=bad, ws=1 << 40) == ERR["BAD_BLOCK_SIZE"], bad
    for mp in (1, 100, 4095):
        assert call(mp=mp, ws=1 << 40) == ERR["BAD_BLOCK_SIZE"], mp
    assert call(n=1 << 62, ws=1 << 62) == ERR["BAD_BLOCK_SIZE"]
    assert call(o=host) == ERR["GPU_UNSUPPORTED"]
    for n, mp, bs in ((0, 0, 4096), (1, 0, 4096), (100000, 8192, 4096), (100000, 0, 4096), (1 << 22, 1 << 20, 65536)):
        ws = _dws(L, 1000, n, mp, bs)
        assert ws > 0 and call(n=n, mp=mp, bs=bs, ws=ws - 1) == ERR["MEMORY"], (n, mp, bs)
    # each call breaks one rule and every later one; the earliest is reported
    assert call(dst=None, e=3, src=None, src_size=5, bs=5000, o=host, ws=0) == ERR["NULL_INPUT"]
    assert call(e=3, src=None, src_size=5, bs=5000, o=host, ws=0) == ERR["GPU_UNSUPPORTED"]
    assert call(src=None, src_size=5, bs=5000, o=host, ws=0) == ERR["NULL_INPUT"]
    assert call(src_size=5, bs=5000, o=host, ws=0) == ERR["SRC_TOO_SMALL"]
    assert call(bs=5000, o=host, ws=0) == ERR["BAD_BLOCK_SIZE"]
    assert call(mp=100, o=host, ws=0) == ERR["BAD_BLOCK_SIZE"]
    assert call(o=host, ws=0) == ERR["GPU_UNSUPPORTED"]
    assert call(ws=0) == ERR["MEMORY"]
    assert call(n=0, dst=None, ws=0) == ERR["MEMORY"]                      # the empty-frame probe needs no destination


def test_decompress_dictionary_errors_in_their_place(L):
    """behind opts->dict, in front of the work size"""
    big, no_content, no_id = cshim.dd(size=65536), cshim.dd(content=None), cshim.dd(id_=None)
    assert _dcall(L, dict_=big) == ERR["DICT_TOO_LARGE"]
    assert _dcall(L, dict_=no_content) == _dcall(L, dict_=no_id) == ERR["NULL_INPUT"]
    assert _dcall(L, dict_=big, ws=0) == ERR["DICT_TOO_LARGE"]
    assert _dcall(L, dict_=big, bs=5000) == ERR["BAD_BLOCK_SIZE"]
    assert _dcall(L, dict_=big, o=api._DecompressOpts(dict=0x10000, dict_size=100)) == ERR["GPU_UNSUPPORTED"]
    assert _dcall(L, dict_=cshim.dd(size=65535), ws=0) == ERR["MEMORY"]


def test_valid_arguments_without_a_device(product, L):
    """What remains after the argument checks is the device check. Only on a machine without a device are the calls made (elsewhere
    these pointers would reach a kernel)."""
    if product.lib().zxc_mi355x_device_count() == 0:
        for sym in SYMS[:2]:
            assert getattr(L, sym)(FAKE_SRC, FAKE_DST, 1000, 4, 4096, None) == ERR["GPU_UNAVAILABLE"]
        assert _ccall(L) == _ccall(L, dict_=cshim.dd()) == _ccall(L, n=0, src=None) == ERR["GPU_UNAVAILABLE"]
        assert _dcall(L) == _dcall(L, dict_=cshim.dd()) == _dcall(L, n=0, dst=None) == ERR["GPU_UNAVAILABLE"]
        with pytest.raises(product.ZxcError) as e:
            product.shuffle_device(FAKE_SRC, FAKE_DST, 1000, 2, 4096)
        assert e.value.code == ERR["GPU_UNAVAILABLE"]


def test_python_bindings_raise(product):
    def code(f, *a, **kw):
        with pytest.raises(product.ZxcError) as e:
            f(*a, **kw)
        return e.value.code

    assert code(product.shuffle_device, FAKE_SRC, FAKE_DST, 1000, 3, 4096) == ERR["GPU_UNSUPPORTED"]
    assert code(product.unshuffle_device, FAKE_SRC, 0, 1000, 4, 4096) == ERR["NULL_INPUT"]
    assert code(product.unshuffle_device, FAKE_SRC, FAKE_DST, 1000, 4, 5000) == ERR["BAD_BLOCK_SIZE"]
    product.shuffle_device(0, 0, 0, 8, 4096)
    product.unshuffle_device(0, 0, 0, 2, 1 << 21)
    assert code(product.compress_shuffle_device, FAKE_SRC, 1000, 4, FAKE_DST, 1 << 20, FAKE_WORK, 1, FAKE_RES, block_size=4096) == ERR["MEMORY"]
    assert code(product.compress_shuffle_device, FAKE_SRC, 1000, 5, FAKE_DST, 1 << 20, FAKE_WORK, 1 << 30, FAKE_RES, block_size=4096) == ERR["GPU_UNSUPPORTED"]
    assert code(product.compress_shuffle_device, FAKE_SRC, 1000, 4, FAKE_DST, 1 << 20, FAKE_WORK, 1 << 30, FAKE_RES, block_size=4096,
                dict_=(0x70000, 70000, 0, 0x90000)) == ERR["DICT_TOO_LARGE"]
    assert code(product.decompress_shuffle_device, FAKE_SRC, 1000, FAKE_DST, 5000, 4, 4096, FAKE_WORK, 1, FAKE_RES) == ERR["MEMORY"]
    assert code(product.decompress_shuffle_device, FAKE_SRC, 1000, FAKE_DST, 5000, 4, 5000, FAKE_WORK, 1 << 30, FAKE_RES) == ERR["BAD_BLOCK_SIZE"]
    assert code(product.decompress_shuffle_device, FAKE_SRC, 20, FAKE_DST, 5000, 4, 4096, FAKE_WORK, 1 << 30, FAKE_RES) == ERR["SRC_TOO_SMALL"]
    assert product.compress_shuffle_device_work_size(1000, 0, 0, 3, 5000) == 0 == product.decompress_shuffle_device_work_size(1000, 5000, 0, 5000)
    assert product.compress_shuffle_device_work_size(1000, 0, 0, 3, 4096) > 4096 < product.decompress_shuffle_device_work_size(1000, 5000, 0, 4096)


# ---------------------------------------------------------------- work sizes
def _piece(total, max_piece, bs):
    """the header's formula"""
    return min((max_piece or DEFAULT_PIECE) // bs * bs, max(1, -(-total // bs)) * bs)


def test_work_sizes_are_the_stated_formulas(L):
    for bs in (4096, 65536, 1 << 19, 1 << 21) + BAD_BLOCK_SIZES:
        for n in (0, 1, bs - 1, bs, bs + 1, 9 * bs + 1000, 1 << 27, 1 << 33, 1 << 62):
            for mp in (0, 1, bs - 1, bs, bs + 1, 2 * bs, 5 * bs + 7, 1 << 30):
                ok = bs not in BAD_BLOCK_SIZES and (mp == 0 or mp >= bs)
                piece = _piece(n, mp, bs) if ok else 0
                take = int(L.zxc_mi355x_decompress_take_device_work_size(1000, n, piece, bs)) if ok else 0
                assert _dws(L, 1000, n, mp, bs) == (take + 512 + piece if take else 0), (bs, n, mp)
                assert _dws(L, 27, n, mp, bs) == 0
                for ds in (0, 1000, 65535, 65536):
                    for level, seekable in ((3, False), (6, True)):
                        o = cshim.opts(level=level, block_size=bs, seekable=seekable)
                        app = int(L.zxc_mi355x_compress_append_dict_device_work_size(n, piece, C.byref(o), ds)) if ok else 0
                        assert _cws(L, n, mp, o, ds) == (app + 256 + piece if app else 0), (bs, n, mp, ds, level)
    # NULL options: 512 KiB blocks; and a chunk never exceeds the source rounded up to blocks
    app = int(L.zxc_mi355x_compress_append_dict_device_work_size(1000, 1 << 19, None, 0))
    assert app > 0 and _cws(L, 1000, 0, None) == app + 256 + (1 << 19)
    assert _cws(L, 1 << 33, 0, None) == int(L.zxc_mi355x_compress_append_dict_device_work_size(1 << 33, DEFAULT_PIECE, None, 0)) + 256 + DEFAULT_PIECE


# ---------------------------------------------------------------- the rules, run on the CPU
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    S = cshim.build_shim(tmp_path_factory, "shuffle", "shuffle/shuffle_shim.c", flags=("-O2",))
    S.shs_index.restype = S.shs_waves.restype = S.shs_piece.restype = C.c_uint64
    S.shs_index.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    S.shs_waves.argtypes = S.shs_ragged.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
    S.shs_ragged.restype = C.c_uint32
    S.shs_piece.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
    S.shs_by_index.restype = S.shs_replay.restype = None
    S.shs_by_index.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int]
    S.shs_replay.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int]
    S.shs_check.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    S.shs_sweep.restype = C.c_int64
    S.shs_sweep.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
    return S


N_MAX = 2 * 4096 + 40


@pytest.mark.parametrize("E", [2, 4, 8])
def test_index_map_is_the_numpy_transpose(shim, E):
    """unit 4096, every n in [0, 2 x 4096 + 40]: the map moves the bytes where a transpose of each unit's (q, E) matrix does"""
    rng = np.random.default_rng(E)
    x = rng.integers(0, 256, N_MAX, dtype=np.uint8)
    for n in range(N_MAX + 1):
        want = ss.np_shuffle(x[:n], E, 4096)
        got = np.full(n + 1, 0xEE, dtype=np.uint8)
        shim.shs_by_index(x.ctypes.data, got.ctypes.data, n, E, 4096, 0)
        assert got[n] == 0xEE and (got[:n] == want).all(), n
        back = np.full(n + 1, 0xEE, dtype=np.uint8)
        shim.shs_by_index(got.ctypes.data, back.ctypes.data, n, E, 4096, 1)
        assert back[n] == 0xEE and (back[:n] == x[:n]).all(), n
    assert (ss.np_unshuffle(ss.np_shuffle(x, E, 4096), E, 4096) == x).all()
    # the definition, literally, at a few places
    n = 4096 + 8 * 37 + 5                                              # a ragged unit of 301 bytes: r != 0 for every E
    assert shim.shs_index(3 * E + 1, n, E, 4096) == 1 * (4096 // E) + 3
    assert shim.shs_index(4096 + 5 * E + (E - 1), n, E, 4096) == 4096 + (E - 1) * (301 // E) + 5
    assert shim.shs_index(n - 1, n, E, 4096) == n - 1                  # the last r bytes are copied


@pytest.mark.parametrize("E", [2, 4, 8])
def test_plan_replay_equals_numpy_at_every_alignment(shim, E):
    """every wave and lane of the grid over every n in [0, 2 x 4096 + 40], the alignments of source and destination walking through
    0 .. 15 with n, and all 256 pairs at the sizes where a path begins or ends: each byte written once, the result the index
    map's (numpy's, by the test above), un-shuffle(shuffle(x)) == x, the canaries intact"""
    checked = C.c_uint64(0)
    assert shim.shs_sweep(E, 4096, 0, N_MAX, 0, C.byref(checked)) == 0
    assert checked.value == N_MAX + 1
    for n in sorted({0, 1, E - 1, E, E + 1, 16 * E - 1, 16 * E, 16 * E + 1, 4095, 4096, 4097, 4096 + 17 * E - 1, N_MAX}):
        assert shim.shs_sweep(E, 4096, n, n, 1, C.byref(checked)) == 0, n
    for unit, n in ((65536, 65536 + 17 * E + 3), (65536, 3 * 65536 + 8191), (1 << 21, (1 << 21) + 100)):
        assert shim.shs_check(n, E, unit, 3, 10) == 0, (unit, n)
    # through numpy as well, at the sizes of the GPU test
    rng = np.random.default_rng(7 * E)
    for n in ss.sizes(E):
        x = rng.integers(0, 256, n, dtype=np.uint8)
        got, hits = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        shim.shs_replay(x.ctypes.data, got.ctypes.data, hits.ctypes.data, n, E, 4096, 0)
        assert (hits == 1).all() and (got == ss.np_shuffle(x, E, 4096)).all(), n


def test_grid_does_not_depend_on_the_element_size(shim):
    for unit in (4096, 65536):
        for n in (0, 1, 100, 4096, 8191, 8192, 8193, 9 * 4096 + 1000, 1 << 24, (1 << 33) + 5):
            waves = {int(shim.shs_waves(n, E, unit)) for E in (2, 4, 8)}
            assert waves == {-(-n // 8192)}, (unit, n, waves)
            for E in (2, 4, 8):
                assert shim.shs_ragged(n, E, unit) == (n % unit // E % 16) * E + n % unit % E <= 127


def test_chunk_of_the_archive_calls(shim):
    for bs in (4096, 1 << 19, 1 << 21):
        for total in (0, 1, bs, bs + 1, 9 * bs + 1000, 1 << 40):
            for mp in (0, bs, bs + 1, 3 * bs - 1, 1 << 30):
                got = int(shim.shs_piece(total, mp, bs))
                assert got == _piece(total, mp, bs) and got % bs == 0 and got >= bs, (bs, total, mp)


def test_rules_under_sanitizers(tmp_path):
    """the stand-alone program tests/shuffle/shuffle_san_main.c (its own main; nothing of it is loaded into this process)"""
    r = cshim.run_san_program(tmp_path, "shuffle/shuffle_san_main.c")
    assert "SHUFFLE OK 34821" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])


# ---------------------------------------------------------------- nothing but the bytes changed
@pytest.mark.parametrize("E", [2, 4, 8])
def test_reference_reads_an_archive_of_shuffled_bytes(mockdev, ref, E):
    """this library's host zxc_compress (its host sources over the mock device) of numpy's shuffle of x is an ordinary archive: the
    unmodified reference decodes it to the shuffled bytes, and un-shuffling those gives x"""
    import oracle_py
    host = oracle_py.Ref.__new__(oracle_py.Ref)
    host.lib = oracle_py.bind_zxc_api(mockdev)
    bs = 4096
    for n in (0, 1, bs, 9 * bs + 1000):
        x = ss.tensor_bytes(n, E, seed=n + E)
        shuffled = ss.np_shuffle(np.frombuffer(x, dtype=np.uint8), E, bs).tobytes()
        for seekable, checksum in ((False, False), (True, True)):
            arc = host.compress(shuffled, 3, bs, seekable, checksum)
            assert arc[5] == 12                                        # the header's block size; nothing in it names the filter
            rc, got = ref.decompress(arc, n, checksum)
            assert rc == n and got == shuffled, (n, E, seekable)
            assert ss.np_unshuffle(np.frombuffer(got, dtype=np.uint8), E, bs).tobytes() == x
