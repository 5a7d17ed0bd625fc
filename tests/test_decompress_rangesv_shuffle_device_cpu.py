"""zxc_mi355x_decompress_rangesv_shuffle_device without a GPU: the two symbols and the Python names, the fourth prototype table
against include/zxc_mi355x_rangesv_shuffle.h by the rules of test_api_prototypes.py, every synchronous argument check in its stated
order (the device pointers below are never dereferenced), the work size against its closed form, and the rules the kernels run
(zxc_amd/csrc/zxc_rangesv_shuffle.h), compiled here with the host C compiler: job (r, j), the gather plan against its definition
and zsh_index, and whole calls replayed on the host (tests/ranges/rangesv_shuffle_replay.h: plan, a stand-in decode launch that
leaves the shuffled bytes in the slots, the gather of every item and lane, verdict) over the seekable goldens read as shuffled
archives and over archives of shuffled typed tensors, every destination a buffer of its own at every alignment between canaries,
below and above the work area, every stored byte counted. The same replay runs under AddressSanitizer and UBSan in a stand-alone
program."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import cshim
import rangesv_shuffle_support as rs
import shuffle_support as ss
from conftest import ROOT, read
from devtest import ERR
from zxc_amd import api

FAKE_SRC, FAKE_IDX, FAKE_RNG, FAKE_WORK, FAKE_RES = 0x10000, 0x20000, 0x30000, 0x50000, 0x60000
BAD_BLOCK_SIZES = (0, 1000, 2048, 4095, 5000, 3 << 12, 1 << 22)
BAD_ELEMS = (0, 1, 3, 5, 6, 7, 16, 1 << 31)
SYMS = ("zxc_mi355x_decompress_rangesv_shuffle_device_work_size", "zxc_mi355x_decompress_rangesv_shuffle_device")
NAMES = ("decompress_rangesv_shuffle_device_work_size", "decompress_rangesv_shuffle_device")
HEADER = "zxc_mi355x_rangesv_shuffle.h"
SEEKABLE_GOLDENS = ("seekable_1block", "seekable_4blocks", "seekable_checksum", "dict_seekable_l7")


def test_symbols_and_names_exported(product):
    L = product.lib()
    for sym in SYMS:
        assert hasattr(L, sym), sym
    for name in NAMES:
        assert hasattr(product, name) and hasattr(product.api, name), name


# ---------------------------------------------------------------- the fourth prototype table against the new header
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "size_t": C.c_size_t, "void": None}


def _ctype(decl):
    if "*" in decl:
        return "pointer"
    return SCALARS[[w for w in decl.split() if w != "const"][0]]


def _header(name=HEADER):
    text = open(os.path.join(ROOT, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    protos = {}
    for ret, name, args in re.findall(r"ZXC_EXPORT\s+([\w\s]+?\*?)\s*(zxc_mi355x_\w+)\s*\(([^)]*)\)\s*;", text):
        protos[name] = (_ctype(ret), [] if args.strip() == "void" else [_ctype(a) for a in args.split(",")])
    return protos


def _same(want, got):
    return (got in (C.c_void_p, C.c_char_p) or hasattr(got, "contents")) if want == "pointer" else got is want


def test_prototype_table_matches_the_new_header(product):
    header, table = _header(), getattr(api, "_PROTOTYPES_RANGESV_SHUFFLE", None)
    assert table is not None, "zxc_amd.api has no _PROTOTYPES_RANGESV_SHUFFLE"
    assert sorted(header) == sorted(SYMS) == sorted(table)
    assert header[SYMS[0]] == (C.c_uint64, [C.c_uint32, C.c_uint64, C.c_uint32])
    assert header[SYMS[1]] == (C.c_int, ["pointer", C.c_uint64, "pointer", "pointer", C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32,
                                         "pointer", "pointer", C.c_uint64, "pointer", "pointer"])
    for other in (api._PROTOTYPES, api._PROTOTYPES_RANGESV, api._PROTOTYPES_SHUFFLE):
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


def test_the_other_headers_declare_no_rangesv_shuffle_name():
    """the new calls are declared in the new header alone, which includes the two it composes"""
    for other in ("zxc_mi355x.h", "zxc_mi355x_rangesv.h", "zxc_mi355x_shuffle.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not re.search(r"ZXC_EXPORT[^;]*rangesv_shuffle", text), other
        assert not [n for n in _header(other) if "rangesv_shuffle" in n], other
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "zxc_mi355x_rangesv.h"' in text and '#include "zxc_mi355x_shuffle.h"' in text


# ---------------------------------------------------------------- synchronous errors
@pytest.fixture(scope="module")
def L(product):
    L = product.lib()
    assert hasattr(L, SYMS[1]), f"libzxc_mi355x.so does not export {SYMS[1]}"
    return L


def _ws(L, n, max_len, bs):
    return int(L.zxc_mi355x_decompress_rangesv_shuffle_device_work_size(n, max_len, bs))


def _call(L, n=8, max_len=100000, e=4, bs=65536, src=FAKE_SRC, idx=FAKE_IDX, rng=FAKE_RNG, work=FAKE_WORK, ws=None, res=FAKE_RES, dict_=None):
    ws = max(_ws(L, n, max_len, bs), 1) if ws is None else ws
    return L.zxc_mi355x_decompress_rangesv_shuffle_device(src, 1000, idx, rng, n, max_len, e, bs, cshim.ref(dict_), work, ws, res, None)


@pytest.mark.parametrize("dict_", [None, "empty", "dict"])
def test_each_synchronous_error_and_their_order(L, dict_):
    d = {"empty": cshim.dd(size=0, content=None, id_=None), "dict": cshim.dd()}.get(dict_, dict_)

    def call(**kw):
        return _call(L, dict_=d, **kw)

    for k in ("src", "idx", "work", "res", "rng"):
        assert call(**{k: None}) == ERR["NULL_INPUT"], k
    for e in BAD_ELEMS:
        assert call(e=e) == ERR["GPU_UNSUPPORTED"], e
    for bad in BAD_BLOCK_SIZES:
        assert call(bs=bad, ws=1 << 40) == ERR["BAD_BLOCK_SIZE"], bad
    assert call(n=1 << 20, max_len=1 << 30, bs=4096, ws=1 << 62) == ERR["MEMORY"]  # 2^20 x (2^18 + 1) jobs
    assert call(n=1, max_len=1 << 63, bs=4096, ws=1 << 62) == ERR["MEMORY"]
    for n, ml, bs in ((1, 1, 4096), (8, 100000, 65536), (20000, 3 << 16, 65536)):
        assert call(n=n, max_len=ml, bs=bs, ws=_ws(L, n, ml, bs) - 1) == ERR["MEMORY"], (n, ml, bs)
    # each call breaks one rule and every later one; the earliest is reported
    assert call(src=None, e=3, bs=5000, ws=0) == ERR["NULL_INPUT"]
    assert call(e=3, bs=5000, ws=0) == ERR["GPU_UNSUPPORTED"]
    assert call(bs=5000, ws=0) == ERR["BAD_BLOCK_SIZE"]
    assert call(ws=0) == ERR["MEMORY"]
    # nothing to do is fine, with or without a device and a range table; the argument checks still come first
    assert call(n=0, rng=None) == 0 and call(n=0) == 0
    assert call(n=0, work=None) == ERR["NULL_INPUT"]
    assert call(n=0, e=5) == ERR["GPU_UNSUPPORTED"]
    assert call(n=0, bs=5000) == ERR["BAD_BLOCK_SIZE"]
    assert call(n=0, ws=0) == ERR["MEMORY"]


def test_dictionary_argument_errors_in_their_place(L):
    """behind the element size and the block size, in front of the work size: rangesv's dictionary checks"""
    big, no_content, no_id = cshim.dd(size=65536), cshim.dd(content=None), cshim.dd(id_=None)
    assert _call(L, dict_=big) == ERR["DICT_TOO_LARGE"]
    assert _call(L, dict_=no_content) == ERR["NULL_INPUT"] and _call(L, dict_=no_id) == ERR["NULL_INPUT"]
    assert _call(L, dict_=cshim.dd(size=65535), ws=0) == ERR["MEMORY"]
    assert _call(L, dict_=cshim.dd(huf=None), n=0) == 0                       # (a dictionary without a table is one)
    assert _call(L, dict_=big, src=None, e=3, bs=5000, ws=0) == ERR["NULL_INPUT"]
    assert _call(L, dict_=big, e=3, bs=5000, ws=0) == ERR["GPU_UNSUPPORTED"]
    assert _call(L, dict_=big, bs=5000, ws=0) == ERR["BAD_BLOCK_SIZE"]
    assert _call(L, dict_=big, ws=0) == ERR["DICT_TOO_LARGE"]
    assert _call(L, dict_=no_id, ws=0) == ERR["NULL_INPUT"]
    assert _call(L, dict_=big, n=0) == ERR["DICT_TOO_LARGE"]
    assert _call(L, dict_=cshim.dd(size=0, content=None, id_=None), ws=0) == ERR["MEMORY"]   # size 0: no dictionary, nothing to check


def test_valid_arguments_without_a_device(product, L):
    """What remains after the argument checks is the device check. Only on a machine without a device is the call made (elsewhere
    these pointers would reach a kernel)."""
    if product.lib().zxc_mi355x_device_count() == 0:
        for e in rs.ELEMS:
            assert _call(L, e=e) == ERR["GPU_UNAVAILABLE"] and _call(L, e=e, dict_=cshim.dd()) == ERR["GPU_UNAVAILABLE"]
        with pytest.raises(product.ZxcError) as err:
            product.decompress_rangesv_shuffle_device(FAKE_SRC, 1000, FAKE_IDX, FAKE_RNG, 4, 1000, 2, 4096, FAKE_WORK, 1 << 30, FAKE_RES)
        assert err.value.code == ERR["GPU_UNAVAILABLE"]


def test_python_binding_raises(product):
    def call(src=FAKE_SRC, e=4, bs=4096, ws=1 << 30, n=4, dict_=None):
        product.decompress_rangesv_shuffle_device(src, 1000, FAKE_IDX, FAKE_RNG if n else 0, n, 1000, e, bs, FAKE_WORK, ws, FAKE_RES, dict_)

    for kw, code in ((dict(bs=5000), "BAD_BLOCK_SIZE"), (dict(ws=1), "MEMORY"), (dict(src=0), "NULL_INPUT"), (dict(e=3), "GPU_UNSUPPORTED"),
                     (dict(dict_=(0x70000, 70000, 0, 0x90000)), "DICT_TOO_LARGE")):
        with pytest.raises(product.ZxcError) as err:
            call(**kw)
        assert err.value.code == ERR[code], kw
    call(n=0)                                       # n_ranges == 0
    call(n=0, dict_=(0x70000, 100, 0, 0x90000))
    assert product.decompress_rangesv_shuffle_device_work_size(4, 1000, 5000) == 0
    assert product.decompress_rangesv_shuffle_device_work_size(4, 1000, 4096) > 0


def _up(x):
    return (x + 255) // 256 * 256


def test_work_size_is_its_closed_form(L):
    """the header's formula; 0 where the call refuses: a block size the format has not, more jobs than a launch counts"""
    for bs in (4096, 65536, 1 << 19, 1 << 21) + BAD_BLOCK_SIZES:
        for n in (0, 1, 7, 300, 20000, 1 << 20, (1 << 31) - 2, (1 << 31) - 1):
            for ml in (0, 1, 100, max(bs, 1) - 1, bs, bs + 1, 2 * bs, 3 * bs + 5, 1 << 22, 1 << 30, 1 << 63):
                J = (ml - 1) // bs + 2 if ml and bs else 1
                N = n * J
                want = 0 if bs in BAD_BLOCK_SIZES or J > (1 << 31) - 2 or N > (1 << 31) - 2 else \
                    _up(_up(_up(24 * N) + 4 * N) + 24 * N) + N * (bs + 64) + 256
                assert _ws(L, n, ml, bs) == want, (n, ml, bs)
                assert want <= N * (bs + 64) + 52 * N + 1024
                if want:   # no less than the sibling's for the same arguments: the same jobs and slots, a larger record
                    assert want >= int(L.zxc_mi355x_decompress_rangesv_device_work_size(n, ml, bs))
    assert _ws(L, 1 << 20, 1 << 30, 4096) == 0 and _ws(L, (1 << 31) - 2, 0, 4096) > 0 and _ws(L, 8, 100000, 65536) > 0


# ---------------------------------------------------------------- the shared rules, run on the CPU
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    S = rs.load_shim(tmp_path_factory)
    assert S.rs_gather_size() == 24
    return S


def test_shape_is_the_siblings_with_a_gather_record(shim):
    sh = rs.Shape()
    assert shim.rs_shape(7, 3 * 4096 + 5, 4096, C.byref(sh)) == 0
    assert (sh.J, sh.n_jobs, sh.slot_stride, sh.chunks) == (5, 35, 4096 + 64, 1)
    assert (sh.o_jobs, sh.o_status, sh.o_gather, sh.o_stage) == (0, _up(24 * 35), _up(24 * 35) + 256, _up(_up(24 * 35) + 256 + 24 * 35))
    assert sh.bytes == sh.o_stage + 35 * 4160 + 256
    for bs, chunks in ((8192, 1), (16384, 2), (1 << 21, 256)):
        assert shim.rs_shape(1, 1, bs, C.byref(sh)) == 0 and sh.chunks == chunks
    assert shim.rs_shape(1, 1, 5000, C.byref(sh)) == ERR["BAD_BLOCK_SIZE"]
    assert shim.rs_shape(1 << 20, 1 << 30, 4096, C.byref(sh)) == ERR["MEMORY"]


def _forged_index(nb, bs, total):
    """an accepted index of nb stored-size blocks, for the rules that never look at the archive"""
    buf = (C.c_uint8 * (64 + 8 * (nb + 1)))()
    ix = rs.Index.from_buffer(buf)
    ix.status, ix.nb, ix.total, ix.dict_id, ix.block_size, ix.seek = 0, nb, total, 0, bs, 2
    offs = np.frombuffer(buf, dtype="<u8", offset=64)
    offs[:] = 16 + np.arange(nb + 1, dtype=np.uint64) * (bs + 8)
    ix.eof_at = int(offs[nb])
    return buf


def test_every_covered_block_is_staged_and_carries_its_length(shim):
    """zrv_job's lines without the direct rule: job j is block offset / bs + j while the range reaches it, always in slot j, with
    the wanted part, its address counted from the base modulo 2^64, and min(bs, total - b bs); an uncovered job is empty"""
    bs, nb, total, out_base = 4096, 6, 5 * 4096 + 1003, 0x7F0000000100
    idx = _forged_index(nb, bs, total)
    src_size = 16 + nb * (bs + 8) + 8 + 8 + 4 * nb + 12
    sh = rs.Shape()
    max_len = 3 * bs + 40
    assert shim.rs_shape(1, max_len, bs, C.byref(sh)) == 0
    J, M = sh.J, (1 << 64) - 1
    cols = np.zeros(7 * J, dtype=np.uint64)
    n_covered = 0
    for base in (0x7F1000000003, 0x10000, 0x7F1000000010):   # above and below the work area: the offsets wrap
        for a, n in ((0, total), (0, bs), (16, bs + 48), (bs, 2 * bs + 32), (5, 3 * bs), (4 * bs + 7, bs + 900), (total - 1, 1), (5 * bs, 1003),
                     (0, 3 * bs + 40), (3 * bs - 1, 2), (0, 0), (total, 1), (0, max_len + 1)):
            shim.rs_jobs(idx, a, n, base, J, src_size, max_len, bs, out_base, sh.o_stage, cols.ctypes.data)
            out_off, comp_off, comp_size, dst_at, from_, cn, m = (cols[c * J:(c + 1) * J] for c in range(7))
            valid = 0 < n <= max_len and a + n <= total
            for j in range(J):
                b = a // bs + j
                lo, hi = max(a, b * bs), min(a + n, (b + 1) * bs)
                assert out_off[j] == sh.o_stage + j * sh.slot_stride, (a, n, j)          # never the destination
                if not valid or hi <= lo:
                    assert (comp_size[j], cn[j], m[j]) == (0, 0, 0), (a, n, j)
                    continue
                assert (comp_off[j], comp_size[j]) == (16 + b * (bs + 8), bs + 8), (a, n, j)
                assert (from_[j], cn[j], m[j]) == (lo - b * bs, hi - lo, min(bs, total - b * bs)), (a, n, j)
                assert (int(dst_at[j]) + out_base) & M == base + lo - a, (a, n, j)
                n_covered += 1
    assert n_covered >= 60


def test_block_and_final_verdict(shim):
    """a covered block's status must equal the length the index gives it; the first failing covered block in block order decides,
    behind the early verdict"""
    bs, nb, total = 4096, 4, 3 * 4096 + 1003
    idx = _forged_index(nb, bs, total)
    src_size = 16 + nb * (bs + 8) + 8 + 8 + 4 * nb + 12

    def verdict(a, n, st, base=0x1000, max_len=4 * bs):
        s = np.array(list(st) + [ERR["SRC_TOO_SMALL"]] * 8, dtype=np.int32)
        return shim.rs_verdict(idx, a, n, base, 6, s.ctypes.data, src_size, max_len, bs)

    assert verdict(0, total, (bs, bs, bs, 1003)) == total
    assert verdict(0, total, (bs, bs, bs, 1004)) == verdict(0, total, (bs, bs, bs, 1002)) == ERR["CORRUPT_DATA"]
    assert verdict(0, total, (bs, bs - 1, bs, 1003)) == ERR["CORRUPT_DATA"]
    assert verdict(bs + 10, 5, (bs - 1,)) == ERR["CORRUPT_DATA"]                  # the sibling would take it: 15 bytes suffice there
    assert verdict(0, total, (bs, ERR["BAD_OFFSET"], bs - 1, ERR["OVERFLOW"])) == ERR["BAD_OFFSET"]
    assert verdict(0, total, (bs, bs - 1, ERR["BAD_OFFSET"], 1003)) == ERR["CORRUPT_DATA"]
    assert verdict(2 * bs, bs + 1003, (bs, 1003)) == bs + 1003 and verdict(3 * bs, 1003, (1003,)) == 1003
    assert verdict(0, bs, (bs, ERR["BAD_OFFSET"])) == bs                           # an uncovered job's status is not looked at
    # the early verdict comes first, whatever the statuses say
    assert verdict(0, 0, (ERR["BAD_OFFSET"],)) == 0
    assert verdict(0, total, (bs, bs, bs, 1003), max_len=total - 1) == ERR["DST_TOO_SMALL"]
    assert verdict(0, 10, (bs,), base=0) == ERR["NULL_INPUT"]
    assert verdict(total - 5, 6, (1003,)) == ERR["SRC_TOO_SMALL"]


def _around(center, d):
    return np.arange(center - d, center + d + 1, dtype=np.int64)


@pytest.mark.parametrize("E", rs.ELEMS)
def test_the_gather_plan_against_its_definition_and_zsh_index(shim, E):
    """m over the sizes of the issue; from within 17 of 0, of a group boundary, of 8192 and of m - n; n within 2 x 16 E + 1 of 1, 16 E
    and m. For every pair the shim walks every item of the block: each wanted byte has exactly one owner, is a vector byte exactly
    when the definition says so, and is read from where zsh_index puts it."""
    w, total = 16 * E, 0
    for m in (1, E - 1, E, w - 1, w, w + 1, 1003, 4096, 8192 + 397, 16384):
        unit = 4096 if m <= 4096 else 16384
        boundary = w * max(1, m // w // 2)
        ns = np.unique(np.concatenate([_around(c, 2 * w + 1) for c in (1, w, m)]))
        ns = ns[(ns >= 1) & (ns <= m)]
        froms, lens = [], []
        for n in ns:
            f = np.unique(np.concatenate([_around(c, 17) for c in (0, boundary, 8192, m - n)]))
            f = f[(f >= 0) & (f + n <= m)]
            froms.append(f)
            lens.append(np.full(len(f), n))
        f, n = np.concatenate(froms).astype(np.uint32), np.concatenate(lens).astype(np.uint32)
        checked = C.c_uint64(0)
        bad = shim.rs_plan_pairs(E, m, unit, f.ctypes.data, n.ctypes.data, len(f), C.byref(checked))
        assert bad == 0, (E, m, "check", bad // 1000000, "from, n", int(f[bad % 1000000 - 1]), int(n[bad % 1000000 - 1]))
        assert checked.value == len(f) >= 1, (E, m)
        total += len(f)
    assert total > 20000, total
    # the definition itself, at three points: zsh_index inside a block is the plane layout, and the copied tail stays
    assert shim.rs_zsh_index(E + 1, 1003, E, 4096) == 1 * (1003 // E) + 1
    assert shim.rs_zsh_index(4096 + 5 * E, 4096 + 1003, E, 4096) == 4096 + 5
    assert shim.rs_zsh_index(1003 // E * E, 1003, E, 4096) == 1003 // E * E


# ---------------------------------------------------------------- whole calls replayed on the host
def _ranges_for(total, bs, rng, n_random=24):
    """-> [(offset, len, kind)], max_len. kind 0: a buffer of its own; 1: a zero base; 2: a base whose end wraps"""
    want = rs.range_list(total, bs, rng, n_random)
    max_len = max(n for a, n in want[1:] if a + n <= total)   # (the whole archive is refused for its length when it is longer)
    out = [(a, n, 0) for a, n in want]
    out.append((0, max_len + 1, 0))                   # len > max_len
    out.append((0, min(total, 50), 1))                # a zero base with a length
    out.append((0, 0, 1))                             # ... and without one
    out.append((1 % total, min(total - 1 % total, 40), 2))   # base + len wraps
    out.append((total, 5, 1))                         # a zero base past the end: NULL_INPUT comes first
    return out, max_len


def _sibling_verdict(shim, buf, a, n, kind, blocks, bs, J, src_size, max_len, have_dict, have_id):
    """zrv_verdict for the same table entry and the statuses of the blocks the range covers"""
    base = {0: 0x1000, 1: 0, 2: rs.M64 - n // 2}[kind]
    b0 = a // bs
    st = np.array([int(blocks.st[b0 + j]) if b0 + j < blocks.n else ERR["SRC_TOO_SMALL"] for j in range(J)], dtype=np.int32)
    return shim.rs_zrv_verdict(buf, a, n, base, J, st.ctypes.data, src_size, max_len, bs, have_dict, have_id)


def _check_archive(shim, comp, decoded, E, what, seed, have_dict=0, have_id=0, shifts=range(16)):
    """decoded: what the archive decodes to, read as shuffled bytes; the plain bytes are its np_unshuffle. Range r's base is
    r + shift (mod 16): all sixteen shifts give every range every alignment, four give every fourth"""
    bs = 1 << comp[5]
    total = len(decoded)
    ix, buf, _ = rs.open_index(shim, comp, bs, -(-total // bs))
    assert ix.status == 0 and ix.total == total, (what, ix.status)
    plain = ss.np_unshuffle(np.frombuffer(decoded, dtype=np.uint8), E, bs)
    ranges, max_len = _ranges_for(total, bs, random.Random(seed))
    blocks = rs.Blocks(decoded, ix)
    J = (max_len - 1) // bs + 2
    want = [_sibling_verdict(shim, buf, a, n, kind, blocks, bs, J, len(comp), max_len, have_dict, have_id) for a, n, kind in ranges]
    n_valid = 0
    for shift in shifts:
        results, got, hits, flags, stray = rs.replay(shim, len(comp), buf, ranges, max_len, E, bs, blocks, have_dict, have_id, shift)
        assert stray == 0, (what, shift)
        for (a, n, kind), res, exp, data, hit, fl in zip(ranges, results, want, got, hits, flags):
            w = (what, E, a, n, kind, shift)
            assert res == exp, (w, res, exp)
            assert not fl & 1, (w, "a byte outside the range's destination changed")
            if res == n and n:
                assert kind == 0 and np.array_equal(data, plain[a:a + n]), w
                assert (hit == 1).all(), (w, "a byte stored twice or not at all")
                n_valid += 1
            else:
                assert res in rs.PRE_BLOCK or n == 0, w
                assert not fl & 2 and not hit.any(), (w, "a refused range's destination changed")
    assert n_valid >= len(shifts) * min(20, len(ranges) - 12), (what, n_valid)
    return ix, buf


@pytest.mark.parametrize("E", rs.ELEMS)
@pytest.mark.parametrize("name", SEEKABLE_GOLDENS)
def test_replay_on_golden_archive_read_as_shuffled(shim, name, E):
    comp, decoded = read(f"conformance/valid/{name}.zxc"), read(f"conformance/valid/{name}.expected")
    bs = 1 << comp[5]
    if name.startswith("dict_"):
        dict_id = rs.open_index(shim, comp, bs, 1 << 16)[0].dict_id
        assert dict_id != 0
        ix, buf = _check_archive(shim, comp, decoded, E, name, 7, 1, dict_id, shifts=(0, 5, 10, 15))
        refused = ((0, 0, ERR["DICT_REQUIRED"]), (1, dict_id ^ 1, ERR["DICT_MISMATCH"]))
    else:
        ix, buf = _check_archive(shim, comp, decoded, E, name, len(comp), shifts=(0, 5, 10, 15))
        refused = ()
    # every non-empty range of a call gets the early verdict and no destination byte is stored to: without the dictionary, with
    # another one, through an index opened with another block size
    total = len(decoded)
    ranges = [(0, total, 0), (0, 0, 0), (1, min(total - 1, 5000), 0), (total - 1, 1, 0)]
    blocks = rs.Blocks(decoded, ix)
    cases = [(bs, hd, hid, code) for hd, hid, code in refused]
    if not refused:
        cases.append((8192 if bs == 4096 else 4096, 0, 0, ERR["BAD_BLOCK_SIZE"]))
    for call_bs, hd, hid, code in cases:
        results, _, hits, flags, stray = rs.replay(shim, len(comp), buf, ranges, total, E, call_bs, blocks, hd, hid)
        assert results == [code, 0, code, code] and flags == [0, 0, 0, 0] and stray == 0 and not any(h.any() for h in hits), (name, code)


@pytest.mark.parametrize("E", rs.ELEMS)
@pytest.mark.parametrize("bs", sorted(rs.SIZES))
@pytest.mark.parametrize("checksum", [False, True])
def test_replay_on_archives_of_shuffled_tensors(shim, E, bs, checksum):
    """np_shuffle of a typed tensor in an archive of stored blocks (tests/container/stored_archive.h): the host compressor of this
    library needs a device, so the archive every machine can build stands in for it here; the reference's zxc_compress writes the
    same bytes into the archives of the next test"""
    plain, shuffled = rs.plain_and_shuffled(E, bs)
    assert len(plain) == rs.SIZES[bs] and (bs != 16384 or ((len(plain) % bs) // E % 16 and (len(plain) % bs) % E))
    comp = rs.stored_archive(shim, shuffled, bs, checksum)
    _check_archive(shim, comp, shuffled, E, ("stored", bs, checksum), seed=bs + E + checksum)


@pytest.mark.parametrize("E", rs.ELEMS)
@pytest.mark.parametrize("bs", sorted(rs.SIZES))
def test_replay_on_host_compressed_archives_of_shuffled_tensors(shim, ref, E, bs):
    """zxc_compress of the reference (level 3, seekable) over the shuffled tensor: an ordinary archive"""
    plain, shuffled = rs.plain_and_shuffled(E, bs)
    comp = ref.compress(shuffled, 3, bs, True, False)
    _check_archive(shim, comp, shuffled, E, ("zxc_compress", bs), seed=bs + E)


@pytest.mark.parametrize("E", rs.ELEMS)
@pytest.mark.parametrize("bs", sorted(rs.SIZES))
def test_the_departure_at_the_replay_level(shim, E, bs):
    """A middle block answers with a status one below block_size and the last block with one above its length. Every range that
    touches either gets ZXC_ERROR_CORRUPT_DATA, also where the sibling would be content with the bytes it needs, and nothing of
    such a block is stored: the bytes of those ranges that lie in the two blocks keep the fill and are never written (what of
    them lies in other blocks is undefined by the contract). Every other range is exact."""
    plain_b, shuffled = rs.plain_and_shuffled(E, bs)
    plain = np.frombuffer(plain_b, dtype=np.uint8)
    total = len(plain)
    comp = rs.stored_archive(shim, shuffled, bs)
    ix, buf, _ = rs.open_index(shim, comp, bs, -(-total // bs))
    mid, last = ix.nb // 2, ix.nb - 1
    blocks = rs.Blocks(shuffled, ix, {mid: bs - 1, last: total - last * bs + 1})
    pairs = rs.range_list(total, bs, random.Random(90 + E), 40)[1:]
    pairs += [(mid * bs + 10, 5), (mid * bs, bs - 1), (last * bs, 7), (total - 1, 1), (mid * bs - 1, 1), ((mid + 1) * bs, 1)]
    max_len = max(n for a, n in pairs if a + n <= total)
    ranges = [(a, n, 0) for a, n in pairs]
    n_failed = n_exact = 0
    for shift in (0, 5, 11):
        results, got, hits, flags, stray = rs.replay(shim, len(comp), buf, ranges, max_len, E, bs, blocks, shift=shift)
        assert stray == 0
        for (a, n, _), res, data, hit, fl in zip(ranges, results, got, hits, flags):
            w = (E, bs, a, n, shift)
            assert not fl & 1, w
            if n == 0 or a + n > total:
                assert res == (0 if n == 0 else ERR["SRC_TOO_SMALL"]) and not hit.any(), w
                continue
            touched = [b for b in (mid, last) if a < min((b + 1) * bs, total) and a + n > b * bs]
            if touched:
                assert res == ERR["CORRUPT_DATA"], (w, res)
                for b in touched:
                    lo, hi = max(a, b * bs) - a, min(a + n, (b + 1) * bs) - a
                    assert not hit[lo:hi].any() and (data[lo:hi] == 0xC3).all(), (w, b, "a failed block's bytes were stored")
                n_failed += 1
            else:
                assert res == n and np.array_equal(data, plain[a:a + n]) and (hit == 1).all(), w
                n_exact += 1
    assert n_failed >= 30 and n_exact >= 30, (n_failed, n_exact)


def test_rules_under_sanitizers(tmp_path):
    """the stand-alone program tests/ranges/rangesv_shuffle_san_main.c (its own main; nothing of it is loaded into this process):
    destinations of exactly len bytes, a work area of exactly its size"""
    r = cshim.run_san_program(tmp_path, "ranges/rangesv_shuffle_san_main.c")
    m = re.search(r"RANGESV SHUFFLE OK (\d+)", r.stdout)
    assert m and int(m.group(1)) >= 3000, (r.stdout[-300:], r.stderr[-3000:])
