"""zxc_mi355x_decompress_rangesv_device / _dict_device without a GPU: the three symbols and the Python names, the second prototype
table against include/zxc_mi355x_rangesv.h by the rules of test_api_prototypes.py, every synchronous argument check of both calls in
its stated order (the device pointers below are never dereferenced), the work size against the sibling's, and the rules the kernels
run (zxc_amd/csrc/zxc_rangesv.h on top of zxc_ranges.h), compiled here with the host C compiler: the direct rule exhaustively over a
small space, and whole calls replayed on the host (tests/ranges/rangesv_replay.h: plan, a stand-in decode launch fed with the oracle
decoder's blocks, the copy-out of every wave and lane, verdict) over every seekable golden archive and, where the reference is
built, archives it writes, every destination a heap buffer of its own at every alignment between canaries. The same replay runs
under AddressSanitizer and UBSan in a stand-alone program."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import cshim
from conftest import GOLDEN, ROOT, load_dict
from devtest import ERR
from zxc_amd import api

FAKE_SRC, FAKE_IDX, FAKE_RNG, FAKE_WORK, FAKE_RES = 0x10000, 0x20000, 0x30000, 0x50000, 0x60000
BAD_BLOCK_SIZES = (0, 1000, 2048, 4095, 5000, 3 << 12, 1 << 22)
SYMS = ("zxc_mi355x_decompress_rangesv_device_work_size", "zxc_mi355x_decompress_rangesv_device", "zxc_mi355x_decompress_rangesv_dict_device")
SEEKABLE_GOLDENS = ("seekable_1block", "seekable_4blocks", "seekable_checksum", "dict_seekable_l7")
PRE_BLOCK = tuple(ERR[k] for k in ("DST_TOO_SMALL", "NULL_INPUT", "SRC_TOO_SMALL", "DICT_REQUIRED", "DICT_MISMATCH", "BAD_BLOCK_SIZE"))


def test_symbols_and_names_exported(product):
    L = product.lib()
    for sym in SYMS:
        assert hasattr(L, sym), sym
    for name in ("RANGEV_DTYPE", "decompress_rangesv_device_work_size", "decompress_rangesv_device", "decompress_rangesv_dict_device"):
        assert hasattr(product, name) and hasattr(product.api, name), name
    assert product.RANGEV_DTYPE.itemsize == 24 and product.RANGEV_DTYPE.names == ("offset", "len", "base")
    assert [product.RANGEV_DTYPE.fields[n][1] for n in ("offset", "len", "base")] == [0, 8, 16]


# ---------------------------------------------------------------- the second prototype table against the new header
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "size_t": C.c_size_t, "void": None}


def _ctype(decl):
    if "*" in decl:
        return "pointer"
    return SCALARS[[w for w in decl.split() if w != "const"][0]]


def _header():
    text = open(os.path.join(ROOT, "include", "zxc_mi355x_rangesv.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    protos = {}
    for ret, name, args in re.findall(r"ZXC_EXPORT\s+([\w\s]+?\*?)\s*(zxc_mi355x_\w+)\s*\(([^)]*)\)\s*;", text):
        protos[name] = (_ctype(ret), [] if args.strip() == "void" else [_ctype(a) for a in args.split(",")])
    return protos


def _same(want, got):
    return (got in (C.c_void_p, C.c_char_p) or hasattr(got, "contents")) if want == "pointer" else got is want


def test_prototype_table_matches_the_new_header(product):
    header, table = _header(), getattr(api, "_PROTOTYPES_RANGESV", None)
    assert table is not None, "zxc_amd.api has no _PROTOTYPES_RANGESV"
    assert sorted(header) == sorted(SYMS) == sorted(table)
    assert header[SYMS[0]] == (C.c_uint64, [C.c_uint32, C.c_uint64, C.c_uint32])
    assert not set(table) & set(api._PROTOTYPES)
    L = product.lib()
    for name in SYMS:
        (want_ret, want_args), (ret, args) = header[name], table[name]
        assert _same(want_ret, ret), (name, "return type", ret)
        assert len(args) == len(want_args), (name, "arity", len(args), len(want_args))
        for i, (want, got) in enumerate(zip(want_args, args)):
            assert _same(want, got), (name, "parameter", i, got)
        f = getattr(L, name)
        assert (f.restype, list(f.argtypes)) == (ret, args), name  # bound once, at load
    # the main header keeps its prototypes: the new calls are declared in the new header alone
    main = open(os.path.join(ROOT, "include", "zxc_mi355x.h")).read()
    assert not re.search(r"ZXC_EXPORT[^;]*rangesv", main)


# ---------------------------------------------------------------- synchronous errors
@pytest.fixture(scope="module")
def L(product):
    L = product.lib()
    assert hasattr(L, SYMS[1]), f"libzxc_mi355x.so does not export {SYMS[1]}"
    return L


def _ws(L, n, max_len, bs):
    return int(L.zxc_mi355x_decompress_rangesv_device_work_size(n, max_len, bs))


def _call(L, n=8, max_len=100000, bs=65536, src=FAKE_SRC, idx=FAKE_IDX, rng=FAKE_RNG, work=FAKE_WORK, ws=None, res=FAKE_RES, dict_=False):
    """dict_: False the plain call; else the zxc_dev_dict_t (or None) of the _dict call"""
    ws = max(_ws(L, n, max_len, bs), 1) if ws is None else ws
    if dict_ is False:
        return L.zxc_mi355x_decompress_rangesv_device(src, 1000, idx, rng, n, max_len, bs, work, ws, res, None)
    return L.zxc_mi355x_decompress_rangesv_dict_device(src, 1000, idx, rng, n, max_len, bs, cshim.ref(dict_), work, ws, res, None)


@pytest.mark.parametrize("dict_", [False, None, "empty", "dict"])
def test_each_synchronous_error_and_their_order(L, dict_):
    d = {"empty": cshim.dd(size=0, content=None, id_=None), "dict": cshim.dd()}.get(dict_, dict_)

    def call(**kw):
        return _call(L, dict_=d, **kw)

    for k in ("src", "idx", "work", "res", "rng"):
        assert call(**{k: None}) == ERR["NULL_INPUT"], k
    for bad in BAD_BLOCK_SIZES:
        assert call(bs=bad, ws=1 << 40) == ERR["BAD_BLOCK_SIZE"], bad
    assert call(n=1 << 20, max_len=1 << 30, bs=4096, ws=1 << 62) == ERR["MEMORY"]  # 2^20 x (2^18 + 1) jobs
    assert call(n=1, max_len=1 << 63, bs=4096, ws=1 << 62) == ERR["MEMORY"]
    for n, ml, bs in ((1, 1, 4096), (8, 100000, 65536), (20000, 3 << 16, 65536)):
        assert call(n=n, max_len=ml, bs=bs, ws=_ws(L, n, ml, bs) - 1) == ERR["MEMORY"], (n, ml, bs)
    # each call breaks one rule and every later one; the earliest is reported
    assert call(src=None, bs=5000, ws=0) == ERR["NULL_INPUT"]
    assert call(bs=5000, ws=0) == ERR["BAD_BLOCK_SIZE"]
    assert call(ws=0) == ERR["MEMORY"]
    # nothing to do is fine, with or without a device and a range table; the argument checks still come first
    assert call(n=0, rng=None) == 0 and call(n=0) == 0
    assert call(n=0, work=None) == ERR["NULL_INPUT"]
    assert call(n=0, bs=5000) == ERR["BAD_BLOCK_SIZE"]
    assert call(n=0, ws=0) == ERR["MEMORY"]


def test_dictionary_argument_errors_in_their_place(L):
    """behind the block size, in front of the work size: the sibling's dictionary checks"""
    big, no_content, no_id = cshim.dd(size=65536), cshim.dd(content=None), cshim.dd(id_=None)
    assert _call(L, dict_=big) == ERR["DICT_TOO_LARGE"]
    assert _call(L, dict_=no_content) == ERR["NULL_INPUT"] and _call(L, dict_=no_id) == ERR["NULL_INPUT"]
    assert _call(L, dict_=cshim.dd(size=65535), ws=0) == ERR["MEMORY"]
    assert _call(L, dict_=cshim.dd(huf=None), n=0) == 0                       # (a dictionary without a table is one)
    assert _call(L, dict_=big, src=None, bs=5000, ws=0) == ERR["NULL_INPUT"]
    assert _call(L, dict_=big, bs=5000, ws=0) == ERR["BAD_BLOCK_SIZE"]
    assert _call(L, dict_=big, ws=0) == ERR["DICT_TOO_LARGE"]
    assert _call(L, dict_=no_id, ws=0) == ERR["NULL_INPUT"]
    assert _call(L, dict_=big, n=0) == ERR["DICT_TOO_LARGE"]
    assert _call(L, dict_=cshim.dd(size=0, content=None, id_=None), ws=0) == ERR["MEMORY"]   # size 0: no dictionary, nothing to check


def test_valid_arguments_without_a_device(product, L):
    """What remains after the argument checks is the device check. Only on a machine without a device are the calls made (elsewhere
    these pointers would reach a kernel)."""
    if product.lib().zxc_mi355x_device_count() == 0:
        assert _call(L) == ERR["GPU_UNAVAILABLE"]
        assert _call(L, dict_=cshim.dd()) == ERR["GPU_UNAVAILABLE"] and _call(L, dict_=None) == ERR["GPU_UNAVAILABLE"]
        with pytest.raises(product.ZxcError) as e:
            product.decompress_rangesv_device(FAKE_SRC, 1000, FAKE_IDX, FAKE_RNG, 4, 1000, 4096, FAKE_WORK, 1 << 30, FAKE_RES)
        assert e.value.code == ERR["GPU_UNAVAILABLE"]


def test_python_binding_raises(product):
    with pytest.raises(product.ZxcError) as e:
        product.decompress_rangesv_device(FAKE_SRC, 1000, FAKE_IDX, FAKE_RNG, 4, 1000, 5000, FAKE_WORK, 1 << 30, FAKE_RES)
    assert e.value.code == ERR["BAD_BLOCK_SIZE"]
    with pytest.raises(product.ZxcError) as e:
        product.decompress_rangesv_device(FAKE_SRC, 1000, FAKE_IDX, FAKE_RNG, 4, 1000, 4096, FAKE_WORK, 1, FAKE_RES)
    assert e.value.code == ERR["MEMORY"]
    with pytest.raises(product.ZxcError) as e:
        product.decompress_rangesv_device(0, 1000, FAKE_IDX, FAKE_RNG, 4, 1000, 4096, FAKE_WORK, 1 << 30, FAKE_RES)
    assert e.value.code == ERR["NULL_INPUT"]
    with pytest.raises(product.ZxcError) as e:
        product.decompress_rangesv_dict_device(FAKE_SRC, 1000, FAKE_IDX, FAKE_RNG, 4, 1000, 4096, (0x70000, 70000, 0, 0x90000), FAKE_WORK,
                                               1 << 30, FAKE_RES)
    assert e.value.code == ERR["DICT_TOO_LARGE"]
    product.decompress_rangesv_device(FAKE_SRC, 1000, FAKE_IDX, 0, 0, 1000, 4096, FAKE_WORK, 1 << 30, FAKE_RES)   # n_ranges == 0
    product.decompress_rangesv_dict_device(FAKE_SRC, 1000, FAKE_IDX, 0, 0, 1000, 4096, None, FAKE_WORK, 1 << 30, FAKE_RES)
    assert product.decompress_rangesv_device_work_size(4, 1000, 5000) == 0
    assert product.decompress_rangesv_device_work_size(4, 1000, 4096) == product.decompress_ranges_device_work_size(4, 1000, 4096) > 0


def test_work_size_is_the_siblings(L):
    for bs in (4096, 65536, 1 << 19, 1 << 21) + BAD_BLOCK_SIZES:
        for n in (0, 1, 7, 300, 20000, 1 << 20, (1 << 31) - 2, (1 << 31) - 1):
            for ml in (0, 1, 100, max(bs, 1) - 1, bs, bs + 1, 2 * bs, 3 * bs + 5, 1 << 22, 1 << 30, 1 << 63):
                want = int(L.zxc_mi355x_decompress_ranges_device_work_size(n, ml, bs))
                assert _ws(L, n, ml, bs) == want, (n, ml, bs)
                if bs in BAD_BLOCK_SIZES:
                    assert want == 0
    assert _ws(L, 1 << 20, 1 << 30, 4096) == 0 and _ws(L, (1 << 31) - 2, 0, 4096) > 0 and _ws(L, 8, 100000, 65536) > 0


# ---------------------------------------------------------------- the shared rules, run on the CPU
class Index(C.Structure):  # zr_index_t
    _fields_ = [("status", C.c_int32), ("nb", C.c_uint32), ("total", C.c_uint64), ("file_ck", C.c_uint32), ("dict_id", C.c_uint32),
                ("block_size", C.c_uint32), ("seek", C.c_uint32), ("eof_at", C.c_uint64), ("rsv", C.c_uint64 * 3)]


class RangeV(C.Structure):  # zxc_dev_rangev_t
    _fields_ = [("offset", C.c_uint64), ("len", C.c_uint64), ("base", C.c_uint64)]


class Shape(C.Structure):  # zr_shape_t
    _fields_ = [(n, C.c_uint32) for n in ("J", "n_jobs", "slot_stride", "copy_chunks")] + \
               [(n, C.c_uint64) for n in ("o_jobs", "o_status", "o_copy", "o_stage", "bytes")]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    S = cshim.build_shim(tmp_path_factory, "rangesv", "ranges/rangesv_shim.c")
    S.rv_rangev_size.restype = C.c_size_t
    assert S.rv_rangev_size() == 24 == C.sizeof(RangeV) == api.RANGEV_DTYPE.itemsize
    S.rv_index_size.restype = C.c_uint64
    S.rv_index_size.argtypes = [C.c_uint32]
    S.rv_open.restype = None
    S.rv_open.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
    S.rv_shape.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(Shape)]
    S.rv_final.argtypes = [C.c_void_p, C.POINTER(RangeV), C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(C.c_int64)]
    S.rv_jobs.restype = None
    S.rv_jobs.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64,
                          C.c_uint64, C.c_void_p]
    S.rv_call.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32,
                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    return S


def _open_index(shim, comp, bs, max_blocks):
    buf = (C.c_uint8 * int(shim.rv_index_size(max_blocks)))()
    C.memset(buf, 0xEE, len(buf))
    shim.rv_open(comp, len(comp), bs, max_blocks, buf)
    return Index.from_buffer_copy(bytes(buf[:64])), buf


def _forged_index(nb=8, bs=4096, total=None, dict_id=0, status=0):
    """an accepted index of nb stored-size blocks, for the rules that never look at the archive"""
    buf = (C.c_uint8 * (64 + 8 * (nb + 1)))()
    ix = Index.from_buffer(buf)
    ix.status, ix.nb, ix.total, ix.dict_id, ix.block_size, ix.seek = status, nb, nb * bs if total is None else total, dict_id, bs, 2
    offs = np.frombuffer(buf, dtype="<u8", offset=64)
    offs[:] = 16 + np.arange(nb + 1, dtype=np.uint64) * (bs + 8)
    ix.eof_at = int(offs[nb])
    return buf


def test_the_direct_rule_exhaustively_over_a_small_space(shim):
    """block size 4096; offsets around 0, one block and two blocks (+- 17); lengths around one, two and three blocks (+- 33);
    base mod 16 in 0..15. A job marked direct: its address is a multiple of 16, the block is wholly wanted and
    [addr, addr + 4096 + 32) lies inside [base, base + len). A job not marked direct: one of the three fails. Through zrv_job, so
    that what the plan kernel writes is what is judged."""
    bs, out_base, n_direct, n_staged = 4096, 0x7F0000000100, 0, 0
    idx = _forged_index(nb=8, bs=bs)
    src_size = 16 + 8 * (bs + 8) + 8 + 8 + 32 + 12
    offsets = sorted({max(c + d, 0) for c in (0, bs, 2 * bs) for d in range(-17, 18)})
    lens = sorted({c + d for c in (bs, 2 * bs, 3 * bs) for d in range(-33, 34)})
    sh = Shape()
    assert shim.rv_shape(1, max(lens), bs, C.byref(sh)) == 0 and sh.J == (max(lens) - 1) // bs + 2 == 5
    U = np.uint64
    ln = np.array(lens, dtype=U)
    rows = len(lens) * sh.J
    cols = np.zeros(6 * rows, dtype=U)
    n_of, j_of = np.repeat(ln, sh.J), np.tile(np.arange(sh.J, dtype=U), len(lens))
    for k in range(16):
        for below in ((0, 1) if k in (0, 7) else (0,)):   # destinations above and below the work area: the offsets wrap
            base = (0x7F1000000000 if not below else 0x10000) + k
            for a in offsets:
                shim.rv_jobs(idx, a, ln.ctypes.data, len(lens), base, sh.J, src_size, max(lens), bs, out_base, sh.o_stage, cols.ctypes.data)
                out_off, comp_size, dst_at, from_, cn, direct = (cols[c * rows:(c + 1) * rows] for c in range(6))
                b = U(a // bs) + j_of
                lo, hi = np.maximum(U(a), b * U(bs)), np.minimum(U(a) + n_of, (b + U(1)) * U(bs))
                covered = hi > lo
                assert not comp_size[~covered].any() and not cn[~covered].any() and not direct[~covered].any(), (a, k)
                assert (comp_size[covered] == bs + 8).all() and not (out_off & U(15)).any(), (a, k)
                staged_slot = U(sh.o_stage) + j_of * U(sh.slot_stride)
                is_direct = covered & (out_off != staged_slot)
                assert (is_direct == (direct != 0)).all(), (a, k)            # the job is placed as zrv_direct says
                place = U(base) + b * U(bs) - U(a)                            # (a covered block's; wraps for an uncovered one in front)
                whole = (lo == b * U(bs)) & (hi == (b + U(1)) * U(bs))
                conds = covered & whole & (place % U(16) == 0) & (place >= U(base)) & (place + U(bs + 32) <= U(base) + n_of)
                assert (is_direct == conds).all(), (a, k, np.flatnonzero(is_direct != conds)[:5])
                assert (out_off[is_direct] + U(out_base) == place[is_direct]).all() and not cn[is_direct].any(), (a, k)
                staged = covered & ~is_direct
                assert (from_[staged] == (lo - b * U(bs))[staged]).all() and (cn[staged] == (hi - lo)[staged]).all(), (a, k)
                assert (dst_at[staged] + U(out_base) == (U(base) + lo - U(a))[staged]).all(), (a, k)
                n_direct += int(is_direct.sum())
                n_staged += int(staged.sum())
    assert n_direct > 10000 and n_staged > 10000, (n_direct, n_staged)


def test_early_verdict_order(shim):
    """the list of the header: len == 0, a failed index, another block size, DST_TOO_SMALL, NULL_INPUT, then the sibling's"""
    M, bs = (1 << 64) - 1, 4096
    ok, failed, dicted = _forged_index(), _forged_index(status=ERR["CORRUPT_DATA"]), _forged_index(dict_id=77)
    src_size = Index.from_buffer(ok).eof_at + 8 + 100

    def final(idx, a, n, base, max_len=10000, block_size=bs, have_dict=0, have_id=0, size=src_size):
        res = C.c_int64(12345)
        done = shim.rv_final(idx, C.byref(RangeV(a, n, base)), size, max_len, block_size, have_dict, have_id, C.byref(res))
        return (res.value if done else None)

    assert final(ok, 10, 100, 0x1000) is None
    # each case breaks one rule and every later one
    assert final(failed, M, 0, 0, block_size=8192, size=0) == 0
    assert final(failed, M, 20000, 0, block_size=8192, size=0) == ERR["CORRUPT_DATA"]
    assert final(dicted, M, 20000, 0, block_size=8192, size=0) == ERR["BAD_BLOCK_SIZE"]
    assert final(dicted, M, 20000, 0, size=0) == ERR["DST_TOO_SMALL"]                  # len > max_len
    assert final(dicted, M, 100, M - 98, size=0) == ERR["DST_TOO_SMALL"]               # base + len passes 2^64
    assert final(dicted, M, 100, M - 99, size=0) == ERR["DST_TOO_SMALL"]               # ... or ends at it
    assert final(dicted, M, 100, 0, size=0) == ERR["NULL_INPUT"]
    assert final(dicted, M, 100, M - 100, size=0) == ERR["SRC_TOO_SMALL"]              # the highest destination there is
    assert final(dicted, 8 * bs - 99, 100, 0x1000, size=0) == ERR["SRC_TOO_SMALL"]     # len > total - offset
    assert final(dicted, 8 * bs - 100, 100, 0x1000, size=0) == ERR["DICT_REQUIRED"]
    assert final(dicted, 8 * bs - 100, 100, 0x1000, have_dict=1, have_id=76, size=0) == ERR["DICT_MISMATCH"]
    assert final(dicted, 8 * bs - 100, 100, 0x1000, have_dict=1, have_id=77, size=0) == ERR["SRC_TOO_SMALL"]   # fewer bytes than opened
    assert final(dicted, 8 * bs - 100, 100, 0x1001, have_dict=1, have_id=77) is None
    assert final(ok, 0, 10000, 0x1003, have_dict=1, have_id=5) is None and final(ok, 0, 10001, 0x1003) == ERR["DST_TOO_SMALL"]


# ---------------------------------------------------------------- whole calls replayed on the host
def _ranges_for(total, bs, nb, rng):
    """-> [(offset, len, kind)], max_len. kind 0: a buffer of its own; 1: a zero base; 2: a base whose end wraps"""
    want = [(0, total), (0, 1), (total - 1, 1), (0, 0), (total, 0), (total + 5, 0), (total, 1), (total - 1, 2), (total + 1, 1),
            (min(7, total - 1), min(100, total - min(7, total - 1)))]
    if nb >= 2:
        want += [(bs - 3, 6), (bs, min(bs, total - bs)), (bs - 1, min(bs + 2, total - bs + 1)), (0, bs), (0, bs + 32), (0, bs + 31), (16, bs + 32)]
    if nb >= 4:
        want += [(bs + 16, 2 * bs + 100), (5, 3 * bs), (2 * bs, bs + 40), (bs - 16, 2 * bs + 64), (0, 3 * bs + 32), (bs, 2 * bs + 31)]
    for _ in range(24):
        a = rng.randrange(total)
        want.append((a, rng.randrange(1, min(total - a, 3 * bs) + 1)))
    max_len = max(n for a, n in want if a + n <= total)
    out = [(a, n, 0) for a, n in want]
    out.append((0, max_len + 1, 0))                   # len > max_len
    out.append((0, min(total, 50), 1))                # a zero base with a length
    out.append((0, 0, 1))                             # ... and without one
    out.append((1 % total, min(total - 1 % total, 40), 2))   # base + len wraps
    out.append((total, 5, 1))                         # a zero base past the end: NULL_INPUT comes first
    return out, max_len


class Blocks:
    """what the decode launch answers for every block of the index: the oracle decoder's bytes and status (with a dictionary: the
    oracle's whole decode cut into blocks)"""

    def __init__(self, oracle, comp, ix, offs, dict_=None, dict_huf=None):
        bs, parts, st = ix.block_size, [], []
        if dict_:
            rc, full = oracle.decompress(comp, ix.total, dict_=dict_, dict_huf=dict_huf)
            assert rc == ix.total
        for b in range(ix.nb):
            if dict_:
                rc, out = min(bs, ix.total - b * bs), full[b * bs:(b + 1) * bs]
            else:
                rc, out = oracle.decode_block(comp[offs[b]:offs[b + 1]], bs)
            st.append(rc)
            parts.append(bytes(out[:max(rc, 0)]).ljust(bs, b"\0"))
        self.bytes = np.frombuffer(b"".join(parts) + b"\0", dtype=np.uint8)
        self.at = np.arange(ix.nb + 1, dtype=np.uint64) * bs
        self.st = np.array(st + [0], dtype=np.int32)
        self.n = ix.nb


def _replay(shim, comp_size, buf, ranges, max_len, bs, blocks, have_dict=0, have_id=0, shift=0):
    n = len(ranges)
    offs = np.array([a for a, _, _ in ranges], dtype=np.uint64)
    lens = np.array([m for _, m, _ in ranges], dtype=np.uint64)
    kinds = np.array([k for _, _, k in ranges], dtype=np.uint32)
    results, flags = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.uint32)
    out = np.zeros(int(lens.sum()) + 1, dtype=np.uint8)
    rc = shim.rv_call(comp_size, buf, offs.ctypes.data, lens.ctypes.data, kinds.ctypes.data, n, max_len, bs, have_dict, have_id,
                      blocks.bytes.ctypes.data, blocks.at.ctypes.data, blocks.st.ctypes.data, blocks.n, shift, results.ctypes.data,
                      out.ctypes.data, flags.ctypes.data)
    assert rc == 0, rc
    cuts = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    return [int(x) for x in results], [out[cuts[i]:cuts[i + 1]].tobytes() for i in range(n)], [int(f) for f in flags]


def _check_archive(shim, oracle, comp, what, seed, dict_=None, dict_huf=None, dict_id=0):
    bs = 1 << comp[5]
    total = int.from_bytes(comp[-12:-4], "little")
    ix, buf = _open_index(shim, comp, bs, -(-total // bs))
    assert ix.status == 0 and ix.total == total, (what, ix.status)
    offs = [int(x) for x in np.frombuffer(bytes(buf), dtype="<u8", offset=64, count=ix.nb + 1)]
    ranges, max_len = _ranges_for(total, bs, ix.nb, random.Random(seed))
    blocks = Blocks(oracle, comp, ix, offs, dict_, dict_huf)
    full = oracle.decompress(comp, total, dict_=dict_, dict_huf=dict_huf)[1] if dict_ else None
    n_valid = 0
    for shift in (0, 4, 9, 14):
        results, got, flags = _replay(shim, len(comp), buf, ranges, max_len, bs, blocks, int(bool(dict_)), dict_id, shift)
        for (a, n, kind), res, data, fl in zip(ranges, results, got, flags):
            w = (what, a, n, kind, shift)
            want, want_data = oracle.seekable_range(comp, a, n)    # the host's zxc_seekable_decompress_range(offset, len, capacity = len)
            if dict_ and want == ERR["DICT_REQUIRED"]:
                want, want_data = n, full[a:a + n]
            if n and (n > max_len or kind == 2):                    # items 4 and 5 depart
                want = ERR["DST_TOO_SMALL"]
            elif n and kind == 1:
                want = ERR["NULL_INPUT"]
            assert res == want, (w, res, want)
            assert not fl & 1, (w, "a byte outside the range's destination changed")
            if res == n and n:
                assert kind == 0 and data == want_data, w
                n_valid += 1
            elif res in PRE_BLOCK or n == 0:
                assert not fl & 2, (w, "a refused range's destination changed")
    assert n_valid >= 40, (what, n_valid)


@pytest.mark.parametrize("name", SEEKABLE_GOLDENS)
def test_replay_on_golden_archive(shim, oracle, name):
    comp = open(os.path.join(GOLDEN, "conformance/valid", name + ".zxc"), "rb").read()
    if name.startswith("dict_"):
        d, huf = load_dict(os.path.join(GOLDEN, "conformance/valid", "dict_text.zxd"))
        dict_id = _index_dict_id(shim, comp)
        assert dict_id != 0
        _check_archive(shim, oracle, comp, name, 7, d, huf, dict_id)
        _check_refused_whole(shim, oracle, comp, name, have_dict=0, have_id=0, want=ERR["DICT_REQUIRED"])
        _check_refused_whole(shim, oracle, comp, name, have_dict=1, have_id=dict_id ^ 1, want=ERR["DICT_MISMATCH"])
    else:
        _check_archive(shim, oracle, comp, name, len(comp))
        _check_refused_whole(shim, oracle, comp, name, have_dict=0, have_id=0, want=ERR["BAD_BLOCK_SIZE"], other_bs=True)


def _index_dict_id(shim, comp):
    bs = 1 << comp[5]
    return _open_index(shim, comp, bs, 1 << 16)[0].dict_id


def _check_refused_whole(shim, oracle, comp, what, have_dict, have_id, want, other_bs=False):
    """every non-empty range of the call gets `want` and no destination byte changes: without the dictionary, with another one,
    through an index opened with another block size"""
    bs = 1 << comp[5]
    total = int.from_bytes(comp[-12:-4], "little")
    ix, buf = _open_index(shim, comp, bs, -(-total // bs))
    call_bs = bs
    if other_bs:
        call_bs = 8192 if bs == 4096 else 4096
    ranges = [(0, total, 0), (0, 0, 0), (1, min(total - 1, 5000), 0), (total - 1, 1, 0)]
    blocks = Blocks.__new__(Blocks)
    blocks.bytes, blocks.at, blocks.st, blocks.n = np.zeros(1, np.uint8), np.zeros(ix.nb + 1, np.uint64), np.zeros(ix.nb + 1, np.int32), ix.nb
    results, _, flags = _replay(shim, len(comp), buf, ranges, total, call_bs, blocks, have_dict, have_id)
    assert results == [want, 0, want, want], (what, results)
    assert flags == [0, 0, 0, 0], (what, flags)


def test_replay_with_a_damaged_block(shim, oracle):
    """a payload byte of block 2 of the four flipped: ranges that cover it get the oracle's error for them, every other range is exact,
    and nothing leaves a destination either way"""
    good = open(os.path.join(GOLDEN, "conformance/valid/seekable_4blocks.zxc"), "rb").read()
    bs = 1 << good[5]
    total = int.from_bytes(good[-12:-4], "little")
    ix, buf = _open_index(shim, good, bs, 4)
    offs = [int(x) for x in np.frombuffer(bytes(buf), dtype="<u8", offset=64, count=5)]
    hit = None
    for at in range(offs[2] + 8, offs[3]):   # the first payload byte whose flip the block decoder refuses
        bad = bytearray(good)
        bad[at] ^= 0x40
        if oracle.decode_block(bytes(bad[offs[2]:offs[3]]), bs)[0] < 0:
            hit = bytes(bad)
            break
    assert hit is not None
    ix, buf = _open_index(shim, hit, bs, 4)
    assert ix.status == 0
    blocks = Blocks(oracle, hit, ix, offs)
    assert blocks.st[2] < 0 and all(blocks.st[b] > 0 for b in (0, 1, 3))
    ranges, max_len = _ranges_for(total, bs, 4, random.Random(11))
    results, got, flags = _replay(shim, len(hit), buf, ranges, max_len, bs, blocks, shift=3)
    n_failed = n_exact = 0
    for (a, n, kind), res, data, fl in zip(ranges, results, got, flags):
        want, want_data = oracle.seekable_range(hit, a, n)
        if n and (n > max_len or kind == 2):
            want = ERR["DST_TOO_SMALL"]
        elif n and kind == 1:
            want = ERR["NULL_INPUT"]
        assert res == want and not fl & 1, (a, n, kind, res, want, fl)
        covers = n > 0 and kind == 0 and a + n <= total and n <= max_len and a < 3 * bs and a + n > 2 * bs
        assert covers == (res == int(blocks.st[2])), (a, n, res)
        n_failed += covers
        if res == n and n:
            assert data == want_data
            n_exact += 1
    assert n_failed >= 5 and n_exact >= 10, (n_failed, n_exact)


@pytest.mark.parametrize("blocks", [1, 2, 5, 40])
def test_replay_on_reference_archives(shim, oracle, ref, blocks):
    from zxc_amd import corpus
    bs = 4096
    rng = np.random.default_rng(blocks)
    n = (blocks - 1) * bs + 1 + int(rng.integers(0, bs))
    for name, data in (("text", corpus.synth_text(n, seed=blocks)), ("random", rng.integers(0, 256, n, dtype=np.uint8).tobytes())):
        for checksum in (False, True):
            comp = ref.compress(data[:n], 3, bs, True, checksum)
            _check_archive(shim, oracle, comp, (name, blocks, checksum), seed=blocks * 131 + checksum)


def test_rules_under_sanitizers(tmp_path):
    """the stand-alone program tests/ranges/rangesv_san_main.c (its own main; nothing of it is loaded into this process)"""
    r = cshim.run_san_program(tmp_path, "ranges/rangesv_san_main.c")
    assert "RANGESV OK 6912" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
