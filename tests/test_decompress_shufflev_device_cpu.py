"""The unshufflev calls of include/zxc_mi355x_unshufflev.h without a GPU: the four symbols and the Python names, the sixth prototype
table against that header by the rules of test_api_prototypes.py, every synchronous argument check of both calls in its stated order
(the device pointers below are never dereferenced), both size functions against their stated forms, the result rule, and the rules
the kernels run (zxc_amd/csrc/zxc_unshufflev.h), compiled here with the host C compiler: the scan in series and the
scatter-un-shuffle plan replayed for every wave, turn and lane of every chunk (tests/shuffle/unshufflev_replay.h), every entry a
heap buffer of its own at every alignment between canaries, every stored byte counted, the concatenation numpy's un-shuffle of the
source. The same replay runs under AddressSanitizer and UBSan in a stand-alone program."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cshim
import dev_append
import shuffle_support as ss
import shufflev_support as sv
import unshufflev_support as uv
from conftest import ROOT
from devtest import ERR
from zxc_amd import api

FAKE_SRC, FAKE_IOV, FAKE_WORK, FAKE_RES = 0x20000, 0x10000, 0x50000, 0x60000
BAD_BLOCK_SIZES = (1000, 2048, 4095, 5000, 3 << 12, 1 << 22)
BAD_ELEMS = (0, 1, 3, 5, 6, 7, 16, 1 << 31)
SYMS = ("zxc_mi355x_unshufflev_device_scratch_size", "zxc_mi355x_unshufflev_device", "zxc_mi355x_decompress_shufflev_device_work_size",
        "zxc_mi355x_decompress_shufflev_device")
NAMES = ("unshufflev_device", "unshufflev_device_scratch_size", "decompress_shufflev_device", "decompress_shufflev_device_work_size")
N_IOVS = (0, 1, 2, 31, 32, 33, 1023, 1024, 1025, 5000, 1 << 20, (1 << 32) - 1)
OLDER_HEADERS = ("zxc_mi355x.h", "zxc_mi355x_rangesv.h", "zxc_mi355x_shuffle.h", "zxc_mi355x_rangesv_shuffle.h", "zxc_mi355x_shufflev.h")


def test_symbols_and_names_exported(product):
    L = product.lib()
    for sym in SYMS:
        assert hasattr(L, sym), sym
    for name in NAMES:
        assert hasattr(product, name) and hasattr(product.api, name), name


# ---------------------------------------------------------------- the sixth prototype table against the new header
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "size_t": C.c_size_t, "void": None}


def _ctype(decl):
    if "*" in decl:
        return "pointer"
    return SCALARS[[w for w in decl.split() if w != "const"][0]]


def _header():
    text = open(os.path.join(ROOT, "include", "zxc_mi355x_unshufflev.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    protos = {}
    for ret, name, args in re.findall(r"ZXC_EXPORT\s+([\w\s]+?\*?)\s*(zxc_mi355x_\w+)\s*\(([^)]*)\)\s*;", text):
        protos[name] = (_ctype(ret), [] if args.strip() == "void" else [_ctype(a) for a in args.split(",")])
    return protos


def _same(want, got):
    return (got in (C.c_void_p, C.c_char_p) or hasattr(got, "contents")) if want == "pointer" else got is want


def test_prototype_table_matches_the_new_header(product):
    header, table = _header(), getattr(api, "_PROTOTYPES_UNSHUFFLEV", None)
    assert table is not None, "zxc_amd.api has no _PROTOTYPES_UNSHUFFLEV"
    assert sorted(header) == sorted(SYMS) == sorted(table)
    assert header[SYMS[0]] == (C.c_uint64, [C.c_uint32])
    assert header[SYMS[1]] == (C.c_int, ["pointer", "pointer", C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, "pointer", C.c_uint64,
                                         "pointer", "pointer"])
    assert header[SYMS[2]] == (C.c_uint64, [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32])
    assert header[SYMS[3]] == (C.c_int, ["pointer", C.c_uint64, "pointer", C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32,
                                         "pointer", "pointer", "pointer", C.c_uint64, "pointer", "pointer"])
    # the five older tables stay what they are; the sixth is reached through the second tuple
    others = (api._PROTOTYPES, api._PROTOTYPES_RANGESV, api._PROTOTYPES_SHUFFLE, api._PROTOTYPES_RANGESV_SHUFFLE, api._PROTOTYPES_SHUFFLEV)
    assert api._TABLES == others and table in api._TABLES_MORE
    for other in others:
        assert not set(table) & set(other)
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
    for other in OLDER_HEADERS:
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not re.search(r"ZXC_EXPORT[^;]*(unshufflev|decompress_shufflev)", text), other


# ---------------------------------------------------------------- synchronous errors
@pytest.fixture(scope="module")
def L(product):
    L = product.lib()
    assert hasattr(L, SYMS[3]), f"libzxc_mi355x.so does not export {SYMS[3]}"
    return L


def _ss(L, n_iov):
    return int(L.zxc_mi355x_unshufflev_device_scratch_size(n_iov))


def _kcall(L, src=FAKE_SRC, iov=FAKE_IOV, n_iov=5, total=1000, e=4, unit=4096, scratch=FAKE_WORK, size=None, res=FAKE_RES):
    size = _ss(L, n_iov) if size is None else size
    return L.zxc_mi355x_unshufflev_device(src, iov, n_iov, total, e, unit, scratch, size, res, None)


def test_kernel_call_errors_in_their_order(L):
    call = lambda **kw: _kcall(L, **kw)  # noqa: E731
    assert call(iov=None) == call(src=None) == call(scratch=None) == call(res=None) == ERR["NULL_INPUT"]
    for e in BAD_ELEMS:
        assert call(e=e) == ERR["GPU_UNSUPPORTED"], e
    for u in BAD_BLOCK_SIZES + (0,):
        assert call(unit=u) == ERR["BAD_BLOCK_SIZE"], u
    assert call(n_iov=0) == call(n_iov=0, iov=None) == ERR["DST_TOO_SMALL"]
    for n_iov in (1, 5, 1024, 1025, 5000):
        assert call(n_iov=n_iov, size=_ss(L, n_iov) - 1) == call(n_iov=n_iov, size=0) == ERR["MEMORY"], n_iov
    assert call(n_iov=0, total=0, size=_ss(L, 0) - 1) == ERR["MEMORY"]
    # each call breaks one rule and every later one; the earliest is reported
    assert call(res=None, e=3, unit=5000, n_iov=0, size=0) == ERR["NULL_INPUT"]
    assert call(e=3, unit=5000, n_iov=0, size=0) == ERR["GPU_UNSUPPORTED"]
    assert call(unit=5000, n_iov=0, size=0) == ERR["BAD_BLOCK_SIZE"]
    assert call(n_iov=0, size=0) == ERR["DST_TOO_SMALL"]
    # no source is needed for nothing, no table for no entries; the other pointers are
    assert call(total=0, src=None, size=0) == ERR["MEMORY"] == call(n_iov=0, total=0, iov=None, src=None, size=0)
    assert call(n_iov=0, total=0, iov=None, src=None, res=None) == call(n_iov=0, total=0, scratch=None) == ERR["NULL_INPUT"]


def _dws(L, n_iov, src_size, n, mp, bs):
    return int(L.zxc_mi355x_decompress_shufflev_device_work_size(n_iov, src_size, n, mp, bs))


def _sibling_ws(L, src_size, n, mp, bs):
    return int(L.zxc_mi355x_decompress_shuffle_device_work_size(src_size, n, mp, bs))


def _dcall(L, src_size=1000, iov=FAKE_IOV, n_iov=5, n=100000, e=4, mp=0, bs=4096, o=None, dict_=None, src=FAKE_SRC, work=FAKE_WORK, ws=None,
           res=FAKE_RES):
    ws = max(_dws(L, n_iov, src_size, n, mp, bs), 1) if ws is None else ws
    return L.zxc_mi355x_decompress_shufflev_device(src, src_size, iov, n_iov, n, e, mp, bs, cshim.ref(o), cshim.ref(dict_), work, ws, res, None)


@pytest.mark.parametrize("dict_", [None, "empty", "dict"])
def test_archive_call_errors_in_their_order(L, dict_):
    d = {"empty": cshim.dd(size=0, content=None, id_=None), "dict": cshim.dd()}.get(dict_)
    host = api._DecompressOpts(dict=0x10000, dict_size=100)

    def call(**kw):
        return _dcall(L, dict_=d, **kw)

    # the new checks
    assert call(iov=None) == call(res=None) == ERR["NULL_INPUT"]
    for e in BAD_ELEMS:
        assert call(e=e) == ERR["GPU_UNSUPPORTED"], e
    assert call(n_iov=0) == call(n_iov=0, iov=None) == ERR["DST_TOO_SMALL"]
    # the session's, in its order
    assert call(src=None) == call(work=None) == ERR["NULL_INPUT"]
    assert call(src_size=27) == ERR["SRC_TOO_SMALL"]
    for bad in BAD_BLOCK_SIZES + (0,):
        assert call(bs=bad, ws=1 << 40) == ERR["BAD_BLOCK_SIZE"], bad
    for mp in (1, 100, 4095):
        assert call(mp=mp, ws=1 << 40) == ERR["BAD_BLOCK_SIZE"], mp
    assert call(n=1 << 62, ws=1 << 62) == ERR["BAD_BLOCK_SIZE"]          # more blocks than a session counts
    assert call(o=host) == ERR["GPU_UNSUPPORTED"]
    for n_iov, n, mp, bs in ((0, 0, 0, 4096), (1, 1, 0, 4096), (5, 100000, 8192, 4096), (3000, 100000, 0, 4096), (7, 1 << 22, 1 << 20, 65536)):
        ws = _dws(L, n_iov, 1000, n, mp, bs)
        assert ws > 0 and call(n_iov=n_iov, n=n, mp=mp, bs=bs, ws=ws - 1) == ERR["MEMORY"], (n_iov, n, mp, bs)
        # what the sibling asks for is not enough: the table's scratch counts
        sibling = _sibling_ws(L, 1000, n, mp, bs)
        assert 0 < sibling < ws and call(n_iov=n_iov, n=n, mp=mp, bs=bs, ws=sibling) == ERR["MEMORY"]
    # each call breaks one rule and every later one; the earliest is reported
    assert call(iov=None, e=3, n_iov=0, src=None, src_size=5, bs=5000, o=host, ws=0) == ERR["GPU_UNSUPPORTED"]  # (no entries need no table)
    assert call(iov=None, e=3, src=None, src_size=5, bs=5000, o=host, ws=0) == ERR["NULL_INPUT"]
    assert call(e=3, n_iov=0, src=None, src_size=5, bs=5000, o=host, ws=0) == ERR["GPU_UNSUPPORTED"]
    assert call(n_iov=0, src=None, src_size=5, bs=5000, o=host, ws=0) == ERR["DST_TOO_SMALL"]
    assert call(src=None, src_size=5, bs=5000, o=host, ws=0) == ERR["NULL_INPUT"]
    assert call(src_size=5, bs=5000, o=host, ws=0) == ERR["SRC_TOO_SMALL"]
    assert call(bs=5000, o=host, ws=0) == ERR["BAD_BLOCK_SIZE"]
    assert call(mp=100, o=host, ws=0) == ERR["BAD_BLOCK_SIZE"]
    assert call(o=host, ws=0) == ERR["GPU_UNSUPPORTED"]
    assert call(ws=0) == ERR["MEMORY"]
    assert call(n_iov=0, n=0, iov=None, ws=0) == ERR["MEMORY"]            # the empty-frame probe needs no table


def test_archive_call_dictionary_errors_in_their_place(L):
    """behind opts->dict, in front of the work size: the session's dictionary checks"""
    big, no_content, no_id = cshim.dd(size=65536), cshim.dd(content=None), cshim.dd(id_=None)
    assert _dcall(L, dict_=big) == ERR["DICT_TOO_LARGE"]
    assert _dcall(L, dict_=no_content) == _dcall(L, dict_=no_id) == ERR["NULL_INPUT"]
    assert _dcall(L, dict_=big, ws=0) == ERR["DICT_TOO_LARGE"]
    assert _dcall(L, dict_=big, bs=5000) == ERR["BAD_BLOCK_SIZE"]
    assert _dcall(L, dict_=big, o=api._DecompressOpts(dict=0x10000, dict_size=100)) == ERR["GPU_UNSUPPORTED"]
    assert _dcall(L, dict_=big, e=3) == ERR["GPU_UNSUPPORTED"]
    assert _dcall(L, dict_=big, n_iov=0) == ERR["DST_TOO_SMALL"]
    assert _dcall(L, dict_=cshim.dd(size=65535), ws=0) == ERR["MEMORY"]


def test_valid_arguments_without_a_device(product, L):
    """What remains after the argument checks is the device check. Only on a machine without a device are the calls made (elsewhere
    these pointers would reach a kernel)."""
    if product.lib().zxc_mi355x_device_count() == 0:
        assert _kcall(L) == _kcall(L, total=0, src=None) == _kcall(L, n_iov=0, total=0, iov=None, src=None) == ERR["GPU_UNAVAILABLE"]
        assert _dcall(L) == _dcall(L, dict_=cshim.dd()) == _dcall(L, n_iov=0, n=0, iov=None) == ERR["GPU_UNAVAILABLE"]
        with pytest.raises(product.ZxcError) as e:
            product.unshufflev_device(FAKE_SRC, FAKE_IOV, 5, 1000, 2, 4096, FAKE_WORK, 1 << 20, FAKE_RES)
        assert e.value.code == ERR["GPU_UNAVAILABLE"]


def test_python_bindings_raise(product):
    def code(f, *a, **kw):
        with pytest.raises(product.ZxcError) as e:
            f(*a, **kw)
        return e.value.code

    size = product.unshufflev_device_scratch_size(5)
    assert size == product.api.unshufflev_device_scratch_size(5) == product.shufflev_device_scratch_size(5) > 0
    assert code(product.unshufflev_device, FAKE_SRC, FAKE_IOV, 5, 1000, 3, 4096, FAKE_WORK, size, FAKE_RES) == ERR["GPU_UNSUPPORTED"]
    assert code(product.unshufflev_device, FAKE_SRC, 0, 5, 1000, 4, 4096, FAKE_WORK, size, FAKE_RES) == ERR["NULL_INPUT"]
    assert code(product.unshufflev_device, FAKE_SRC, FAKE_IOV, 5, 1000, 4, 5000, FAKE_WORK, size, FAKE_RES) == ERR["BAD_BLOCK_SIZE"]
    assert code(product.unshufflev_device, FAKE_SRC, FAKE_IOV, 0, 1000, 4, 4096, FAKE_WORK, size, FAKE_RES) == ERR["DST_TOO_SMALL"]
    assert code(product.unshufflev_device, FAKE_SRC, FAKE_IOV, 5, 1000, 4, 4096, FAKE_WORK, size - 1, FAKE_RES) == ERR["MEMORY"]
    assert code(product.decompress_shufflev_device, FAKE_SRC, 1000, FAKE_IOV, 5, 5000, 4, 4096, FAKE_WORK, 1, FAKE_RES) == ERR["MEMORY"]
    assert code(product.decompress_shufflev_device, FAKE_SRC, 1000, FAKE_IOV, 5, 5000, 5, 4096, FAKE_WORK, 1 << 30, FAKE_RES) == ERR["GPU_UNSUPPORTED"]
    assert code(product.decompress_shufflev_device, FAKE_SRC, 1000, FAKE_IOV, 0, 5000, 4, 4096, FAKE_WORK, 1 << 30, FAKE_RES) == ERR["DST_TOO_SMALL"]
    assert code(product.decompress_shufflev_device, FAKE_SRC, 1000, FAKE_IOV, 5, 5000, 4, 5000, FAKE_WORK, 1 << 30, FAKE_RES) == ERR["BAD_BLOCK_SIZE"]
    assert code(product.decompress_shufflev_device, FAKE_SRC, 20, FAKE_IOV, 5, 5000, 4, 4096, FAKE_WORK, 1 << 30, FAKE_RES) == ERR["SRC_TOO_SMALL"]
    assert code(product.decompress_shufflev_device, FAKE_SRC, 1000, FAKE_IOV, 5, 5000, 4, 4096, FAKE_WORK, 1 << 30, FAKE_RES,
                dict_=(0x70000, 70000, 0, 0x90000)) == ERR["DICT_TOO_LARGE"]
    assert product.decompress_shufflev_device_work_size(5, 1000, 5000, 0, 5000) == 0
    assert product.decompress_shufflev_device_work_size(5, 1000, 5000, 0, 4096) >= product.decompress_shuffle_device_work_size(1000, 5000, 0, 4096) + size


# ---------------------------------------------------------------- the sizes
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return uv.load_shim(tmp_path_factory)


def _up256(v):
    return -(-v // 256) * 256


def test_scratch_size_is_shufflevs(L, shim):
    for n in N_IOVS + tuple(range(0, 3000, 37)):
        t = -(-n // 1024)
        exact = 768 + _up256(8 * (n + 1)) + _up256(8 * t) + _up256(4 * t)
        assert _ss(L, n) == int(L.zxc_mi355x_shufflev_device_scratch_size(n)) == exact == shim.uvs_scratch_size(n) > 0, n


def test_work_size_is_the_stated_form(L, shim):
    for bs in (4096, 65536, 1 << 19, 1 << 21) + BAD_BLOCK_SIZES:
        for n in (0, 1, bs - 1, bs, bs + 1, 9 * bs + 1000, 1 << 27, 1 << 33, 1 << 62):
            for mp in (0, 1, bs - 1, bs, bs + 1, 2 * bs, 5 * bs + 7, 1 << 30):
                for src_size in (0, 27, 28, 1000, 1 << 33):
                    sibling = _sibling_ws(L, src_size, n, mp, bs)
                    for n_iov in (0, 1, 1025, 5000):
                        want = _up256(sibling) + _ss(L, n_iov) if sibling else 0
                        assert _dws(L, n_iov, src_size, n, mp, bs) == want == shim.uvs_work_size(sibling, n_iov), (bs, n, mp, src_size, n_iov)


def test_work_size_is_one_chunk_the_session_and_eight_bytes_per_entry(L):
    """the memory claim: whatever the checkpoint's size, the work area is the take session's, one chunk and the table's scratch"""
    bs, mp = 1 << 19, 1 << 26
    for total in (1 << 30, 1 << 36):
        for n_iov in (1, 1000, 1 << 20):
            session = int(L.zxc_mi355x_decompress_take_device_work_size(total // 2, total, mp, bs))
            ws = _dws(L, n_iov, total // 2, total, mp, bs)
            assert 0 < ws - session - mp <= 8 * (n_iov + 1) + 16 * -(-n_iov // 1024) + 4096 + 256 + 512 + 256, (total, n_iov)


def test_result_word_rule(shim):
    """the table's error wins, in the read direction's words; else the session's word with the sibling's size check"""
    for total in (0, 12345):
        for word in (0, 12345, 777, ERR["BAD_CHECKSUM"], ERR["CORRUPT_DATA"]):
            ok = word if (total == 0 or word < 0 or word == total) else ERR["CORRUPT_DATA"]
            assert shim.uvs_result(0, word, total) == ok, (total, word)
            for name, want in (("NULL_INPUT", "NULL_INPUT"), ("OVERFLOW", "OVERFLOW"), ("SRC_TOO_SMALL", "DST_TOO_SMALL")):
                assert shim.uvs_result(ERR[name], word, total) == ERR[want], (name, total, word)
    assert shim.uvs_result(0, 12345, 12345) == 12345 and shim.uvs_result(0, 12344, 12345) == ERR["CORRUPT_DATA"]
    assert shim.uvs_result(0, 9, 0) == 9                                  # total == 0: the probe's answer as it is


# ---------------------------------------------------------------- the rules, run on the CPU
def _replay(shim, y, lens, E, piece, what):
    """the replay at the 16 alignments: every byte of every entry stored once, none outside; the concatenation is numpy's un-shuffle
    of the source"""
    total = sum(lens)
    assert total == len(y)
    arr = np.array(lens if lens else [0], dtype=np.uint64)
    out = np.full(total + 1, 0xEE, dtype=np.uint8)
    src = np.frombuffer(y + b"\0", dtype=np.uint8)
    rc = shim.uvs_check(src.ctypes.data, arr.ctypes.data, len(lens), total, E, 4096, piece, out.ctypes.data)
    assert rc == 0, (what, E, total, piece, rc)
    assert out[total] == 0xEE and (out[:total] == ss.np_unshuffle(src[:total], E, 4096)).all(), (what, E, total, piece)


@pytest.mark.parametrize("E", sv.ELEMS)
def test_replay_equals_numpy_over_the_cuts(shim, E):
    """unit 4096, the sizes of the shuffle tests, as one chunk (the kernel call) and in chunks of two units (max_piece 8192)"""
    n_runs = 0
    for total in ss.sizes(E):
        y = ss.tensor_bytes(total, E, seed=total + E)
        for name, lens in sv.cuts(total, E, seed=total).items():
            for piece in (0, 8192):
                _replay(shim, y, lens, E, piece, name)
                n_runs += 1
    assert n_runs == len(ss.sizes(E)) * 8 * 2


@pytest.mark.parametrize("E", sv.ELEMS)
def test_replay_equals_numpy_over_the_append_orders(shim, E):
    y = ss.tensor_bytes(sv.ORDERS_TOTAL, E, seed=E)
    for name, lens in dev_append.orders().items():
        for piece in (0, 4096, 8192):
            _replay(shim, y, lens, E, piece, name)
    _replay(shim, b"", [], E, 0, "no table")
    _replay(shim, b"", [0, 0, 0], E, 0, "empty entries alone")


@pytest.mark.parametrize("case", list(dev_append.bad_table_cases()))
def test_replay_of_a_bad_table_touches_nothing(shim, case):
    lens = [4096 + 7, 3 * 4096, 50, 0, 2 * 4096 + 1]
    promised, fix, want = sv.bad_table(lens, case)
    want = {"SRC_TOO_SMALL": "DST_TOO_SMALL"}.get(want, want)            # the read direction's word (ztv_verdict)
    y = np.frombuffer(ss.tensor_bytes(sum(lens) + 1, 4, seed=3), dtype=np.uint8)
    arr = np.array(lens, dtype=np.uint64)
    for E in sv.ELEMS:
        for piece in (0, 8192):
            rc = shim.uvs_check_bad(y.ctypes.data, arr.ctypes.data, len(lens), promised, 2 if fix else 0xFFFFFFFF, E, 4096, piece)
            assert rc == ERR[want], (case, E, piece, rc)     # (a positive rc: an entry was written)


def test_rules_under_sanitizers(tmp_path):
    """the stand-alone program tests/shuffle/unshufflev_san_main.c (its own main; nothing of it is loaded into this process)"""
    r = cshim.run_san_program(tmp_path, "shuffle/unshufflev_san_main.c")
    assert "UNSHUFFLEV OK 564" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
