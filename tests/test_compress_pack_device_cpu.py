"""zxc_mi355x_compress_pack_device without a GPU: the four symbols and the Python names, every synchronous argument check in its
stated order (the device pointers below are never dereferenced), the work-size arithmetic, and the rules the kernels run
(zxc_amd/csrc/zxc_cpack.h on top of zxc_cbatch.h), compiled here with the host C compiler and run grouped in tiles the way the
kernels group them (tests/batch/cpack_shim.c). Archives that the unmodified reference wrote, and this library's goldens, are cut
into their blocks (the "slots" and sizes an encode launch leaves) and put together again by plan, size, the tiled scan, place,
finish and a byte gather: the destination must hold every archive at the offset a few lines of Python compute on their own, with
a pattern intact in every gap, behind *d_total and behind the capacity. The same stages run under AddressSanitizer and UBSan in
a stand-alone program."""
import ctypes as C
import os

import numpy as np
import pytest

import cshim
from conftest import GOLDEN
from cpu_batch import (BAD_BLOCK_SIZES, BLOCK_SIZES, CANARY, ERR, FAKE_DICT, FAKE_DST, FAKE_HUF, FAKE_ID, FAKE_ITEMS, FAKE_RES, FAKE_SRC,
                       FAKE_WORK, IMAGE_FIXED, JOB, JOB_BYTES, M64, REC_BYTES, WORK_FIXED, Arc, Item, Rec, Shape, _dd, _host_dict_opts, _opts,
                       _ref, _ref_arcs, _stride)

FAKE_PACKED, FAKE_TOTAL = 0xA0000, 0xB0000
TILE_BYTES, PACK_FIXED = 8, 256  # the stated bound: the sibling's + 8 ceil(n / 1024) + 256
ALIGNS = (1, 16, 256, 4096)


@pytest.fixture(scope="module")
def L(product):
    L = product.lib()
    assert hasattr(L, "zxc_mi355x_compress_pack_device"), "libzxc_mi355x.so does not export zxc_mi355x_compress_pack_device"
    return L


def _ws(L, n, max_size, o, dict_size=None):
    if dict_size is None:
        return int(L.zxc_mi355x_compress_pack_device_work_size(n, max_size, _ref(o)))
    return int(L.zxc_mi355x_compress_pack_dict_device_work_size(n, max_size, _ref(o), dict_size))


def _ws_batch(L, n, max_size, o, dict_size=None):
    if dict_size is None:
        return int(L.zxc_mi355x_compress_batch_device_work_size(n, max_size, _ref(o)))
    return int(L.zxc_mi355x_compress_batch_dict_device_work_size(n, max_size, _ref(o), dict_size))


def _call(L, n=8, max_size=100000, o="default", src_cap=1 << 20, cap=1 << 20, align=16, src=FAKE_SRC, items=FAKE_ITEMS, dst=FAKE_DST,
          work=FAKE_WORK, ws=None, packed=FAKE_PACKED, res=FAKE_RES, total=FAKE_TOTAL, d=False):
    """d: False = the call without a dictionary argument, else the zxc_dev_dict_t (or None) of the _dict call"""
    o = _opts() if isinstance(o, str) else o
    if ws is None:
        ws = max(_ws(L, n, max_size, o, None if d is False or d is None else min(d.size, 65535)), 1)
    if d is False:
        return L.zxc_mi355x_compress_pack_device(src, src_cap, items, n, max_size, dst, cap, align, _ref(o), work, ws, packed, res, total, None)
    return L.zxc_mi355x_compress_pack_dict_device(src, src_cap, items, n, max_size, dst, cap, align, _ref(o), _ref(d), work, ws, packed, res,
                                                  total, None)


def test_symbols_and_names_exported(product):
    L = product.lib()
    for sym in ("zxc_mi355x_compress_pack_device_work_size", "zxc_mi355x_compress_pack_device",
                "zxc_mi355x_compress_pack_dict_device_work_size", "zxc_mi355x_compress_pack_dict_device"):
        assert hasattr(L, sym), sym
    for name in ("compress_pack_device_work_size", "compress_pack_device", "compress_pack_dict_device"):
        assert hasattr(product, name) and hasattr(product.api, name), name
    assert all(sym in product.api._PROTOTYPES for sym in ("zxc_mi355x_compress_pack_device_work_size", "zxc_mi355x_compress_pack_device",
                                                          "zxc_mi355x_compress_pack_dict_device_work_size",
                                                          "zxc_mi355x_compress_pack_dict_device"))


def test_each_synchronous_error_and_their_order(product, L):
    no_device = product.lib().zxc_mi355x_device_count() == 0
    for d in (False, None, _dd(size=0, content=None, id_=None), _dd()):
        for k in ("src", "work", "res", "packed", "total", "items", "dst"):
            assert _call(L, d=d, **{k: None}) == ERR["NULL_INPUT"], k
        for bad in BAD_BLOCK_SIZES:
            assert _call(L, d=d, o=_opts(block_size=bad), ws=1 << 40) == ERR["BAD_BLOCK_SIZE"], bad
        assert _call(L, d=d, o=_host_dict_opts(), ws=1 << 40) == ERR["GPU_UNSUPPORTED"]
        for align in (0, 3, 8192, 48, 1 << 31):
            assert _call(L, d=d, align=align) == ERR["GPU_UNSUPPORTED"], align
            assert _call(L, d=d, align=align, n=0) == ERR["GPU_UNSUPPORTED"], align  # in front of "nothing to do"
        for align in (1, 16, 4096):  # accepted: what is left is the work size and the device
            assert _call(L, d=d, align=align, ws=0) == ERR["MEMORY"], align
            assert _call(L, d=d, align=align, n=0) == 0, align
            if no_device:
                assert _call(L, d=d, align=align) == ERR["GPU_UNAVAILABLE"], align
        assert _call(L, d=d, n=1 << 20, max_size=1 << 30, o=_opts(block_size=4096), ws=1 << 62) == ERR["MEMORY"]  # 2^20 x 2^18 jobs
        assert _call(L, d=d, n=1, max_size=1 << 63, o=_opts(block_size=4096), ws=1 << 62) == ERR["MEMORY"]
        for n, ms, bs in ((1, 1, 4096), (8, 100000, 65536), (20000, 3 << 16, 65536), (5, 0, 4096)):
            o = _opts(block_size=bs)
            ds = None if d is False or d is None else d.size
            assert _call(L, d=d, n=n, max_size=ms, o=o, ws=_ws(L, n, ms, o, ds) - 1) == ERR["MEMORY"], (n, ms, bs)
        # nothing to do is fine, with or without a device and an item table; the argument checks still come first
        assert _call(L, d=d, n=0, items=None) == 0
        assert _call(L, d=d, n=0, cap=0, dst=None) == 0
        assert _call(L, d=d, n=0, max_size=1 << 63) == 0
        assert _call(L, d=d, n=0, o=None) == 0
        assert _call(L, d=d, n=0, total=None) == ERR["NULL_INPUT"]
        assert _call(L, d=d, n=0, ws=0) == ERR["MEMORY"]
        assert _call(L, d=d, n=0, o=_opts(block_size=5000)) == ERR["BAD_BLOCK_SIZE"]
        if no_device:  # the sizing run's arguments are legal
            assert _call(L, d=d, cap=0, dst=None) == ERR["GPU_UNAVAILABLE"]
    # the dictionary argument, as dict_arg judges it
    assert _call(L, d=_dd(size=65536)) == ERR["DICT_TOO_LARGE"]
    assert _call(L, d=_dd(content=None)) == ERR["NULL_INPUT"]
    assert _call(L, d=_dd(id_=None)) == ERR["NULL_INPUT"]
    # each call breaks one rule and every later one; the earliest is reported
    bad_bs, hd = _host_dict_opts(block_size=5000), _host_dict_opts()
    assert _call(L, src=None, o=bad_bs, d=_dd(size=1 << 20, id_=None), align=3, ws=0) == ERR["NULL_INPUT"]
    assert _call(L, o=bad_bs, d=_dd(size=1 << 20, id_=None), align=3, ws=0) == ERR["BAD_BLOCK_SIZE"]
    assert _call(L, o=hd, d=_dd(size=1 << 20, id_=None), align=3, ws=0) == ERR["GPU_UNSUPPORTED"]  # the host dictionary
    assert _call(L, d=_dd(size=1 << 20, id_=None), align=16, ws=0) == ERR["DICT_TOO_LARGE"]
    assert _call(L, d=_dd(size=1 << 20, id_=None), align=3, ws=0) == ERR["DICT_TOO_LARGE"]
    assert _call(L, d=_dd(id_=None), align=3, ws=0) == ERR["NULL_INPUT"]
    assert _call(L, d=_dd(), align=3, ws=0) == ERR["GPU_UNSUPPORTED"]  # the alignment
    assert _call(L, d=_dd(), ws=0) == ERR["MEMORY"]
    assert _call(L, o=bad_bs, align=3, ws=0) == ERR["BAD_BLOCK_SIZE"]
    assert _call(L, o=hd, align=16, ws=0) == ERR["GPU_UNSUPPORTED"]
    assert _call(L, align=3, ws=0) == ERR["GPU_UNSUPPORTED"]
    assert _call(L, ws=0) == ERR["MEMORY"]
    assert _call(L, n=0, ws=0) == ERR["MEMORY"]  # the work size comes in front of "nothing to do"


def test_python_binding_raises(product):
    args = (FAKE_SRC, 1 << 20, FAKE_ITEMS, 4, 1000, FAKE_DST, 1 << 20)
    tail = (FAKE_PACKED, FAKE_RES, FAKE_TOTAL)
    with pytest.raises(product.ZxcError) as e:
        product.compress_pack_device(*args, 16, FAKE_WORK, 1 << 30, *tail, block_size=5000)
    assert e.value.code == ERR["BAD_BLOCK_SIZE"]
    with pytest.raises(product.ZxcError) as e:
        product.compress_pack_device(*args, 24, FAKE_WORK, 1 << 30, *tail, block_size=4096)
    assert e.value.code == ERR["GPU_UNSUPPORTED"]
    with pytest.raises(product.ZxcError) as e:
        product.compress_pack_device(*args, 16, FAKE_WORK, 1, *tail, block_size=4096)
    assert e.value.code == ERR["MEMORY"]
    with pytest.raises(product.ZxcError) as e:
        product.compress_pack_device(*args, 16, FAKE_WORK, 1 << 30, 0, FAKE_RES, FAKE_TOTAL, block_size=4096)
    assert e.value.code == ERR["NULL_INPUT"]
    with pytest.raises(product.ZxcError) as e:
        product.compress_pack_dict_device(*args, 16, (FAKE_DICT, 70000, FAKE_HUF, FAKE_ID), FAKE_WORK, 1 << 30, *tail, block_size=4096)
    assert e.value.code == ERR["DICT_TOO_LARGE"]
    product.compress_pack_device(FAKE_SRC, 1 << 20, 0, 0, 1000, FAKE_DST, 1 << 20, 16, FAKE_WORK, 1 << 30, *tail, block_size=4096)
    assert product.compress_pack_device_work_size(4, 1000, block_size=5000) == 0
    assert product.compress_pack_device_work_size(4, 1000, block_size=4096) > product.compress_batch_device_work_size(4, 1000, block_size=4096)
    assert product.compress_pack_device_work_size(4, 1000, block_size=4096, dict_size=100) > product.compress_pack_device_work_size(
        4, 1000, block_size=4096)


def _added(n):
    """what the pack call's work area has beyond the sibling's: a word per tile of 1024 items and the end word, rounded up to 256"""
    return -(-(TILE_BYTES * -(-n // 1024) + 8) // 256) * 256


def test_work_size(L):
    for bs in BLOCK_SIZES:
        o, S = _opts(block_size=bs), _stride(bs)
        for n in (0, 1, 7, 300, 1024, 1025, 20000, 40000):
            prev = 0
            for ms in sorted((0, 1, 100, bs - 1, bs, bs + 1, 2 * bs, 3 * bs + 5, 1 << 22)):
                w = _ws(L, n, ms, o)
                J = max(1, -(-ms // bs))
                assert w > 0 and w >= prev, (bs, n, ms)
                assert w == _ws_batch(L, n, ms, o) + _added(n), (bs, n, ms)  # the sibling's plus only the stated additions
                assert w >= n * J * (S + JOB_BYTES) + REC_BYTES * n + TILE_BYTES * -(-n // 1024) + 8, (bs, n, ms)
                assert w <= n * J * (S + JOB_BYTES) + REC_BYTES * n + WORK_FIXED + TILE_BYTES * -(-n // 1024) + PACK_FIXED, (bs, n, ms, w)
                assert w == _ws(L, n, ms, o, 0)  # a dictionary of size 0 is no dictionary
                for D in (1, 1000, 65535):
                    wd = _ws(L, n, ms, o, D)
                    assert wd == _ws_batch(L, n, ms, o, D) + _added(n), (bs, n, ms, D)
                    chunk = max(4096, (256 << 20) // (bs + D))
                    images = min(n * J, chunk) * (bs + D)
                    assert w + images <= wd <= w + images + (IMAGE_FIXED if n else 0), (bs, n, ms, D)
                prev = w
        prev = 0
        for n in (0, 1, 2, 255, 256, 257, 1024, 1025, 5000):
            w = _ws(L, n, 3 * bs, o)
            assert w > prev, (bs, n)
            prev = w
        for seekable in (0, 1):  # the shape does not depend on these
            for checksum in (0, 1):
                for level in (1, 7):
                    assert _ws(L, 9, 3 * bs, _opts(level, bs, seekable, checksum)) == _ws(L, 9, 3 * bs, o)
    assert _ws(L, 10, 1 << 20, None) == _ws(L, 10, 1 << 20, _opts(level=0, block_size=0)) == _ws(L, 10, 1 << 20, _opts(block_size=1 << 19))
    # 0 for whatever the sibling's size function refuses
    for bad in BAD_BLOCK_SIZES:
        assert _ws(L, 10, 1000, _opts(block_size=bad)) == 0 and _ws(L, 10, 1000, _opts(block_size=bad), 100) == 0, bad
    assert _ws(L, 10, 1000, _host_dict_opts()) == 0 and _ws(L, 10, 1000, _opts(), 65536) == 0
    o = _opts(block_size=4096)
    assert _ws(L, 1 << 20, 1 << 30, o) == 0 and _ws(L, 1, 1 << 63, o) == 0  # more jobs than a launch counts
    assert _ws(L, (1 << 31) - 2, 0, o) > 0 and _ws(L, (1 << 31) - 1, 0, o) == 0
    assert _ws(L, (1 << 31) - 2, 4096, o) > 0 and _ws(L, (1 << 30), 4097, o) == 0


# ---------------------------------------------------------------- the shared rules, run on the CPU
class PShape(C.Structure):  # zcp_shape_t
    _fields_ = [("b", Shape), ("n_tiles", C.c_uint32), ("rsv", C.c_uint32), ("o_tiles", C.c_uint64), ("o_end", C.c_uint64),
                ("bytes", C.c_uint64)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    S = cshim.build_shim(tmp_path_factory, "cpack", "batch/cpack_shim.c")
    S.t_pshape_size.restype = C.c_size_t
    assert S.t_pshape_size() == C.sizeof(PShape)
    S.t_pshape.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(PShape)]
    S.t_align_ok.argtypes = [C.c_uint32]
    S.t_extent.restype = C.c_uint64
    S.t_extent.argtypes = [C.POINTER(Rec), C.c_uint32]
    S.t_pack_plan.restype = None
    S.t_pack_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    S.t_pack_layout.restype = None
    S.t_pack_layout.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_uint64,
                                C.c_void_p, C.POINTER(C.c_uint64)]
    S.t_pack_finish.restype = None
    S.t_pack_finish.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                C.c_int, C.c_int, C.c_int, C.c_uint32]
    S.t_pack_results.restype = None
    S.t_pack_results.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    return S


def test_shape_and_alignment(shim, L):
    for bs in (4096, 65536):
        for n, ms in ((0, 100), (1, 0), (7, 3 * bs + 5), (1024, bs), (1025, bs), (70000, bs)):
            for D in (0, 1000):
                p = PShape()
                assert shim.t_pshape(n, ms, bs, _stride(bs), D, C.byref(p)) == 0
                assert p.bytes == _ws(L, n, ms, _opts(block_size=bs), D) and p.b.bytes == _ws_batch(L, n, ms, _opts(block_size=bs), D)
                assert p.n_tiles == -(-n // 1024) and p.o_tiles == p.b.bytes - 256 and p.o_tiles % 256 == 0
                assert p.o_end == p.o_tiles + 8 * p.n_tiles and p.o_end + 8 <= p.bytes - 256
    p = PShape()
    assert shim.t_pshape(8, 100, 5000, 1, 0, C.byref(p)) == ERR["BAD_BLOCK_SIZE"]
    assert shim.t_pshape(1 << 20, 1 << 30, 4096, _stride(4096), 0, C.byref(p)) == ERR["MEMORY"]
    ok = [a for a in range(0, 9000) if shim.t_align_ok(a)]
    assert ok == [1 << k for k in range(13)] and not shim.t_align_ok(1 << 13) and not shim.t_align_ok(1 << 31)


UNSIZED = {"oob": ERR["SRC_TOO_SMALL"], "wrap": ERR["SRC_TOO_SMALL"], "big": ERR["OVERFLOW"], "corrupt": ERR["CORRUPT_DATA"]}


def _model(sizes, align, cap):
    """the layout, on its own: sizes[r] is None for an item without a size -> (at per item or None, written per item, total)"""
    at, end = [None] * len(sizes), 0
    for r, size in enumerate(sizes):
        if size is not None:
            at[r] = -(-end // align) * align
            end = at[r] + size
    return at, [a is not None and a + s <= cap for a, s in zip(at, sizes)], end


def _pack(shim, arcs, key, align, cap=None, bad=None, in_place=False):
    """the call as the kernels make it over items whose blocks are `arcs`' blocks: clear, plan, "encode" (each job's slot and size
    are the archive's block), size + reduce, scan, place, finish, gather, results; bad: {item index: kind of UNSIZED}. Compared with
    the model here; -> (results, packed table, total, destination, where each item lies or None)"""
    bs, checksum, seekable, has_dict, dict_id = key
    bad = bad or {}
    n, S = len(arcs), _stride(bs)
    max_size = max([a.size for a in arcs] + [1])
    items, src_at = (Item * max(n, 1))(), 0
    for r, a in enumerate(arcs):
        src_at += 1 + (r * 7) % 40
        items[r] = Item(src_at, a.size, 0xDEAD0000 + r, r)  # dst_off and dst_capacity are not looked at
        src_at += a.size
    src_cap = src_at + max_size + 1  # (room for the item above max_size: its source lies inside, so that rule is the one it breaks)
    for r, kind in bad.items():
        if kind == "oob":
            items[r].src_off = src_cap - arcs[r].size + 1
        elif kind == "wrap":
            items[r].src_off = M64 - 3
            items[r].src_size = 100
        elif kind == "big":
            items[r].src_size = max_size + 1
    given = [(it.src_off, it.src_size) for it in items[:n]]
    p = PShape()
    assert shim.t_pshape(n, max_size, bs, S, 0, C.byref(p)) == 0
    J, nj = p.b.J, p.b.n_jobs
    jobs = np.zeros(max(nj, 1), dtype=JOB)
    sizes = np.zeros(max(nj, 1), dtype=np.uint32)
    offsets = np.full(max(nj, 1), 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    slots = np.full(max(nj, 1) * S, 0xEE, dtype=np.uint8)
    tiles = np.full(max(p.n_tiles, 1), 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    recs = (Rec * max(n, 1))()
    C.memset(recs, 0xEE, C.sizeof(recs))
    shim.t_pack_plan(items, n, J, src_cap, max_size, bs, int(checksum), int(seekable), recs, jobs.ctypes.data)
    for r, a in enumerate(arcs):
        mine = jobs[r * J: (r + 1) * J]
        if bad.get(r) in ("oob", "wrap", "big"):
            assert recs[r].result == UNSIZED[bad[r]] and recs[r].nb == 0 and not mine["len"].any()  # refused: no job, nothing read
            continue
        assert recs[r].result == 0 and recs[r].nb == len(a.blocks) and not mine["len"][recs[r].nb:].any()
        for b, blk in enumerate(a.blocks):
            i = r * J + b
            assert int(mine["src_off"][b]) == given[r][0] + b * bs and int(mine["len"][b]) == min(bs, a.size - b * bs)
            slots[i * S: i * S + len(blk)] = np.frombuffer(blk, dtype=np.uint8)
            sizes[i] = len(blk)
        if bad.get(r) == "corrupt":
            sizes[r * J + len(a.blocks) - 1] = 3
    want_size = [None if r in bad else len(a.comp) for r, a in enumerate(arcs)]
    at, written, want_total = _model(want_size, align, 0)
    cap = want_total if cap is None else cap
    at, written, want_total = _model(want_size, align, cap)
    dst = np.full(want_total + 4096 + 64, CANARY, dtype=np.uint8)  # (a capacity above the total: nothing goes there)
    end, total = C.c_uint64(0xEEEE), C.c_uint64(0xEEEE)
    shim.t_pack_layout(recs, n, J, sizes.ctypes.data, bs, int(checksum), int(seekable), align, cap, tiles.ctypes.data, C.byref(end))
    shim.t_pack_finish(recs, n, J, sizes.ctypes.data, offsets.ctypes.data, slots.ctypes.data, S, dst.ctypes.data if cap else None, bs,
                       int(checksum), int(seekable), int(has_dict), dict_id)
    results = np.full(max(n, 1), -777, dtype=np.int64)
    packed = items if in_place else (Item * max(n, 1))()
    shim.t_pack_results(recs, n, C.byref(end), packed, results.ctypes.data, C.byref(total))
    # against the model
    assert total.value == (want_total if n else 0xEEEE), (total.value, want_total)
    keep = np.zeros(len(dst), dtype=bool)
    for r, a in enumerate(arcs):
        w = (r, a.what, key, align, cap)
        got = (packed[r].src_off, packed[r].src_size, packed[r].dst_off, packed[r].dst_capacity)
        if written[r]:
            assert results[r] == len(a.comp) and got == (at[r], len(a.comp)) + given[r], (w, results[r], got)
            assert at[r] % align == 0 and dst[at[r]: at[r] + len(a.comp)].tobytes() == a.comp, w
            keep[at[r]: at[r] + len(a.comp)] = True
        else:
            assert results[r] == (UNSIZED[bad[r]] if r in bad else ERR["DST_TOO_SMALL"]) and got == (0, 0) + given[r], (w, results[r], got)
    assert (dst[~keep] == CANARY).all(), (key, align, cap)  # every gap, behind the total, behind the capacity
    return [int(x) for x in results[:n]], packed, total.value, dst, at


def _golden_groups():
    groups = {}
    for d in ("conformance/valid", "format", "synth"):
        p = os.path.join(GOLDEN, d)
        for f in sorted(os.listdir(p)) if os.path.isdir(p) else ():
            if f.endswith(".zxc"):
                try:
                    a = Arc(open(os.path.join(p, f), "rb").read(), f"{d}/{f}")
                except (AssertionError, IndexError):
                    continue  # (a format vector that is no complete archive)
                kinds = (0, 1) if not a.blocks else (int(a.seekable),)
                if a.regular:
                    for sk in kinds:
                        groups.setdefault((a.bs, int(a.checksum), sk, int(a.has_dict), a.dict_id), []).append(a)
    return groups


@pytest.mark.parametrize("align", ALIGNS)
def test_rules_pack_the_golden_archives(shim, align):
    groups = _golden_groups()
    n = sum(len(v) for v in groups.values())
    assert n >= 30 and len(groups) >= 6, (n, sorted(groups))
    assert any(k[3] for k in groups) and {k[0] for k in groups} >= {4096, 65536}  # a dictionary header among them
    for key, arcs in sorted(groups.items()):
        _pack(shim, arcs, key, align)
        _pack(shim, arcs[::-1], key, align, cap=1 << 40)


@pytest.mark.parametrize("checksum", [0, 1])
@pytest.mark.parametrize("seekable", [0, 1])
def test_rules_pack_the_reference_archives(shim, ref, checksum, seekable):
    arcs = _ref_arcs(ref, 4096, checksum, seekable)
    assert sorted(len(a.blocks) for a in arcs) == [0, 1, 1, 1, 1, 2, 2, 4]
    for align in ALIGNS:
        results, _, total, _, at = _pack(shim, arcs + arcs, (4096, checksum, seekable, 0, 0), align)
        assert all(rc > 0 for rc in results) and at[0] == 0 and total == at[-1] + len(arcs[-1].comp)
        if align == 1:
            assert total == 2 * sum(len(a.comp) for a in arcs)  # back to back


def _small(ref):
    """the reference's archives of at most one 4 KiB block (J = 1): sizes 0, 1, 33, 4095, 4096"""
    return [a for a in _ref_arcs(ref, 4096, 1, 1) if a.size <= 4096]


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 2049])
def test_scan_grouping_and_unsized_items_at_tile_edges(shim, ref, n):
    small = _small(ref)
    assert len(small) == 5
    arcs = [small[(r * 3 + r // 1024) % 5] for r in range(n)]
    kinds = ("oob", "big", "corrupt", "wrap")
    edges = [r for r in (0, 3, 4, 255, 256, 1019, 1020, 1022, 1023, 1024, 1025, 1027, 1028, 2047, 2048) if r < n]
    bad = {}
    for k, r in enumerate(edges):
        kind = kinds[k % 4]
        bad[r] = kind if (kind != "corrupt" or arcs[r].blocks) else "big"  # (an archive without blocks has no size to corrupt)
    for align in (1, 256):
        _pack(shim, arcs, (4096, 1, 1, 0, 0), align)  # every item sized
        results, _, total, _, at = _pack(shim, arcs, (4096, 1, 1, 0, 0), align, bad=bad)
        assert all(at[r] is None and results[r] == UNSIZED[kind] for r, kind in bad.items())
        if n > len(bad):
            assert total > 0 and sum(rc > 0 for rc in results) == n - len(bad)
    if n:
        _pack(shim, arcs, (4096, 1, 1, 0, 0), 16, bad={r: "big" for r in range(n)})  # no sized item: total 0, nothing written


def test_capacity_cuts(shim, ref):
    arcs = _ref_arcs(ref, 4096, 1, 1)
    key = (4096, 1, 1, 0, 0)
    for align in (1, 256):
        _, _, total, _, at = _pack(shim, arcs, key, align)
        ends = [a + len(x.comp) for a, x in zip(at, arcs)]
        assert total == ends[-1]
        for cap in sorted({0, total} | {e - 1 for e in ends} | set(ends)):
            results, packed, t, dst, _ = _pack(shim, arcs, key, align, cap=cap)
            assert t == total  # the same every time
            ok = [rc > 0 for rc in results]
            assert ok == [e <= cap for e in ends] and ok == sorted(ok, reverse=True)  # exactly the prefix that fits
            assert all(rc == ERR["DST_TOO_SMALL"] for rc in results if rc <= 0) and (dst[cap:] == CANARY).all()


def test_in_place(shim, ref):
    arcs = _ref_arcs(ref, 4096, 0, 1)
    for align, cap, bad in ((1, None, None), (16, None, {1: "oob", 4: "corrupt"}), (4096, 20000, {0: "big"})):
        r1, p1, t1, d1, _ = _pack(shim, arcs, (4096, 0, 1, 0, 0), align, cap=cap, bad=bad)
        r2, p2, t2, d2, _ = _pack(shim, arcs, (4096, 0, 1, 0, 0), align, cap=cap, bad=bad, in_place=True)
        assert r1 == r2 and t1 == t2 and np.array_equal(d1, d2)
        assert bytes(p1)[: 32 * len(arcs)] == bytes(p2)[: 32 * len(arcs)]


def test_rules_under_sanitizers(tmp_path):
    """the stand-alone program tests/batch/cpack_san_main.c (its own main; nothing of it is loaded into this process)"""
    r = cshim.run_san_program(tmp_path, "batch/cpack_san_main.c")
    assert "CPACK OK" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
