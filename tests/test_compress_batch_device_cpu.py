"""zxc_mi355x_compress_batch_device without a GPU: the four symbols and the Python names, every synchronous argument check in its
stated order (the device pointers below are never dereferenced), the work-size arithmetic, and the rules the kernels run
(zxc_amd/csrc/zxc_cbatch.h), compiled here with the host C compiler. Archives that the unmodified reference wrote, and this
library's goldens, are cut into their blocks (the "slots" and sizes an encode launch leaves), laid as items into one arena at odd
offsets, and put together again by plan + finish + a byte gather: every item's output must be its archive byte for byte, with a
pattern intact everywhere else. The same rules run under AddressSanitizer and UBSan in a stand-alone program."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import cshim
from conftest import GOLDEN
from cpu_batch import (BAD_BLOCK_SIZES, BLOCK_SIZES, CANARY, ERR, FAKE_DICT, FAKE_DST, FAKE_ID, FAKE_ITEMS, FAKE_RES, FAKE_SRC, FAKE_WORK,
                       IMAGE_FIXED, JOB, JOB_BYTES, M64, REC_BYTES, WORK_FIXED, Arc, Item, Rec, Shape, _dd, _host_dict_opts, _opts, _ref,
                       _ref_arcs, _stride)

@pytest.fixture(scope="module")
def L(product):
    L = product.lib()
    assert hasattr(L, "zxc_mi355x_compress_batch_device"), "libzxc_mi355x.so does not export zxc_mi355x_compress_batch_device"
    for bs in BLOCK_SIZES:
        assert int(L.zxc_mi355x_encode_slot_stride(bs)) == _stride(bs)
    return L


def _ws(L, n, max_size, o, dict_size=None):
    if dict_size is None:
        return int(L.zxc_mi355x_compress_batch_device_work_size(n, max_size, _ref(o)))
    return int(L.zxc_mi355x_compress_batch_dict_device_work_size(n, max_size, _ref(o), dict_size))


def _call(L, n=8, max_size=100000, o="default", src_cap=1 << 20, cap=1 << 20, src=FAKE_SRC, items=FAKE_ITEMS, dst=FAKE_DST, work=FAKE_WORK,
          ws=None, res=FAKE_RES, d=False):
    """d: False = the call without a dictionary argument, else the zxc_dev_dict_t (or None) of the _dict call"""
    o = _opts() if isinstance(o, str) else o
    if ws is None:
        ws = max(_ws(L, n, max_size, o, None if d is False or d is None else min(d.size, 65535)), 1)
    if d is False:
        return L.zxc_mi355x_compress_batch_device(src, src_cap, items, n, max_size, dst, cap, _ref(o), work, ws, res, None)
    return L.zxc_mi355x_compress_batch_dict_device(src, src_cap, items, n, max_size, dst, cap, _ref(o), _ref(d), work, ws, res, None)


def test_symbols_and_names_exported(product):
    L = product.lib()
    for sym in ("zxc_mi355x_compress_batch_device_work_size", "zxc_mi355x_compress_batch_device",
                "zxc_mi355x_compress_batch_dict_device_work_size", "zxc_mi355x_compress_batch_dict_device"):
        assert hasattr(L, sym), sym
    for name in ("compress_batch_device_work_size", "compress_batch_device", "compress_batch_dict_device"):
        assert hasattr(product, name) and hasattr(product.api, name), name
    assert all(sym in product.api._PROTOTYPES for sym in ("zxc_mi355x_compress_batch_device_work_size", "zxc_mi355x_compress_batch_device",
                                                          "zxc_mi355x_compress_batch_dict_device_work_size",
                                                          "zxc_mi355x_compress_batch_dict_device"))


def test_each_synchronous_error_and_their_order(L):
    for d in (False, None, _dd()):
        for k in ("src", "work", "res", "items", "dst"):
            assert _call(L, d=d, **{k: None}) == ERR["NULL_INPUT"], k
        for bad in BAD_BLOCK_SIZES:
            assert _call(L, d=d, o=_opts(block_size=bad), ws=1 << 40) == ERR["BAD_BLOCK_SIZE"], bad
        assert _call(L, d=d, o=_host_dict_opts(), ws=1 << 40) == ERR["GPU_UNSUPPORTED"]
        assert _call(L, d=d, n=1 << 20, max_size=1 << 30, o=_opts(block_size=4096), ws=1 << 62) == ERR["MEMORY"]  # 2^20 x 2^18 jobs
        assert _call(L, d=d, n=1, max_size=1 << 63, o=_opts(block_size=4096), ws=1 << 62) == ERR["MEMORY"]
        for n, ms, bs in ((1, 1, 4096), (8, 100000, 65536), (20000, 3 << 16, 65536), (5, 0, 4096)):
            o = _opts(block_size=bs)
            ds = None if d is False or d is None else d.size
            assert _call(L, d=d, n=n, max_size=ms, o=o, ws=_ws(L, n, ms, o, ds) - 1) == ERR["MEMORY"], (n, ms, bs)
        # nothing to do is fine, with or without a device and an item table; the argument checks still come first
        assert _call(L, d=d, n=0, items=None) == 0
        assert _call(L, d=d, n=0, cap=0, dst=None) == 0
        assert _call(L, d=d, n=0, max_size=1 << 63) == 0  # no item: no job to count
        assert _call(L, d=d, n=0, o=None) == 0            # NULL opts: the defaults
        assert _call(L, d=d, n=0, work=None) == ERR["NULL_INPUT"]
        assert _call(L, d=d, n=0, ws=0) == ERR["MEMORY"]
        assert _call(L, d=d, n=0, o=_opts(block_size=5000)) == ERR["BAD_BLOCK_SIZE"]
    # the dictionary argument, as dict_arg judges it
    assert _call(L, d=_dd(size=65536)) == ERR["DICT_TOO_LARGE"]
    assert _call(L, d=_dd(content=None)) == ERR["NULL_INPUT"]
    assert _call(L, d=_dd(id_=None)) == ERR["NULL_INPUT"]
    # each call breaks one rule and every later one; the earliest is reported
    bad_bs, hd = _host_dict_opts(block_size=5000), _host_dict_opts()
    assert _call(L, src=None, o=bad_bs, d=_dd(size=1 << 20, id_=None), ws=0) == ERR["NULL_INPUT"]
    assert _call(L, o=bad_bs, d=_dd(size=1 << 20, id_=None), ws=0) == ERR["BAD_BLOCK_SIZE"]
    assert _call(L, o=hd, d=_dd(size=1 << 20, id_=None), ws=0) == ERR["GPU_UNSUPPORTED"]  # the host dictionary
    assert _call(L, d=_dd(size=1 << 20, id_=None), ws=0) == ERR["DICT_TOO_LARGE"]
    assert _call(L, d=_dd(id_=None), ws=0) == ERR["NULL_INPUT"]
    assert _call(L, d=_dd(), ws=0) == ERR["MEMORY"]
    assert _call(L, o=bad_bs, ws=0) == ERR["BAD_BLOCK_SIZE"]
    assert _call(L, o=hd, ws=0) == ERR["GPU_UNSUPPORTED"]
    assert _call(L, ws=0) == ERR["MEMORY"]
    assert _call(L, n=0, ws=0) == ERR["MEMORY"]  # the work size comes in front of "nothing to do"


def test_valid_arguments_without_a_device(product, L):
    """What remains after the argument checks is the device check. Only on a machine without a device is the call made (elsewhere
    these pointers would reach a kernel)."""
    if product.lib().zxc_mi355x_device_count() == 0:
        for d in (False, None, _dd(), _dd(huf=None, size=65535), _dd(size=0, content=None, id_=None)):
            assert _call(L, d=d) == ERR["GPU_UNAVAILABLE"]
            assert _call(L, d=d, cap=0, dst=None) == ERR["GPU_UNAVAILABLE"]
            assert _call(L, d=d, o=None, max_size=1 << 20) == ERR["GPU_UNAVAILABLE"]
            assert _call(L, d=d, o=_opts(level=7, block_size=4096, seekable=True, checksum=True)) == ERR["GPU_UNAVAILABLE"]
            assert _call(L, d=d, n=0) == 0
        with pytest.raises(product.ZxcError) as e:
            product.compress_batch_device(FAKE_SRC, 1 << 20, FAKE_ITEMS, 4, 1000, FAKE_DST, 1 << 20, FAKE_WORK, 1 << 30, FAKE_RES, block_size=4096)
        assert e.value.code == ERR["GPU_UNAVAILABLE"]


def test_python_binding_raises(product):
    with pytest.raises(product.ZxcError) as e:
        product.compress_batch_device(FAKE_SRC, 1 << 20, FAKE_ITEMS, 4, 1000, FAKE_DST, 1 << 20, FAKE_WORK, 1 << 30, FAKE_RES, block_size=5000)
    assert e.value.code == ERR["BAD_BLOCK_SIZE"]
    with pytest.raises(product.ZxcError) as e:
        product.compress_batch_device(FAKE_SRC, 1 << 20, FAKE_ITEMS, 4, 1000, FAKE_DST, 1 << 20, FAKE_WORK, 1, FAKE_RES, block_size=4096)
    assert e.value.code == ERR["MEMORY"]
    with pytest.raises(product.ZxcError) as e:
        product.compress_batch_device(FAKE_SRC, 1 << 20, 0, 4, 1000, FAKE_DST, 1 << 20, FAKE_WORK, 1 << 30, FAKE_RES, block_size=4096)
    assert e.value.code == ERR["NULL_INPUT"]
    with pytest.raises(product.ZxcError) as e:
        product.compress_batch_dict_device(FAKE_SRC, 1 << 20, FAKE_ITEMS, 4, 1000, FAKE_DST, 1 << 20, (FAKE_DICT, 70000, 0, FAKE_ID),
                                           FAKE_WORK, 1 << 30, FAKE_RES, block_size=4096)
    assert e.value.code == ERR["DICT_TOO_LARGE"]
    product.compress_batch_device(FAKE_SRC, 1 << 20, 0, 0, 1000, FAKE_DST, 1 << 20, FAKE_WORK, 1 << 30, FAKE_RES, block_size=4096)  # nothing to do
    assert product.compress_batch_device_work_size(4, 1000, block_size=5000) == 0
    assert product.compress_batch_device_work_size(4, 1000, block_size=4096) > 0
    assert product.compress_batch_device_work_size(4, 1000, block_size=4096, dict_size=100) > product.compress_batch_device_work_size(
        4, 1000, block_size=4096)


def test_work_size(L):
    for bs in BLOCK_SIZES:
        o, S = _opts(block_size=bs), _stride(bs)
        for n in (0, 1, 7, 300, 20000):
            prev = 0
            for ms in sorted((0, 1, 100, bs - 1, bs, bs + 1, 2 * bs, 3 * bs + 5, 1 << 22)):
                w = _ws(L, n, ms, o)
                J = max(1, -(-ms // bs))
                assert w > 0 and w >= prev, (bs, n, ms)
                assert w >= n * J * (S + JOB_BYTES) + REC_BYTES * n, (bs, n, ms)  # at least n_jobs slots
                assert w <= n * J * (S + JOB_BYTES) + REC_BYTES * n + WORK_FIXED, (bs, n, ms, w)
                assert w == _ws(L, n, ms, o, 0)  # a dictionary of size 0 is no dictionary
                for D in (1, 1000, 65535):
                    wd = _ws(L, n, ms, o, D)
                    chunk = max(4096, (256 << 20) // (bs + D))
                    images = min(n * J, chunk) * (bs + D)
                    assert w + images <= wd <= w + images + (IMAGE_FIXED if n else 0), (bs, n, ms, D)
                prev = w
        prev = 0
        for n in (0, 1, 2, 255, 256, 257, 5000):
            w = _ws(L, n, 3 * bs, o)
            assert w > prev, (bs, n)
            prev = w
        for seekable in (0, 1):  # the shape does not depend on these
            for checksum in (0, 1):
                for level in (1, 7):
                    assert _ws(L, 9, 3 * bs, _opts(level, bs, seekable, checksum)) == _ws(L, 9, 3 * bs, o)
    assert _ws(L, 10, 1 << 20, None) == _ws(L, 10, 1 << 20, _opts(level=0, block_size=0)) == _ws(L, 10, 1 << 20, _opts(block_size=1 << 19))
    for bad in BAD_BLOCK_SIZES:
        assert _ws(L, 10, 1000, _opts(block_size=bad)) == 0 and _ws(L, 10, 1000, _opts(block_size=bad), 100) == 0, bad
    assert _ws(L, 10, 1000, _host_dict_opts()) == 0 and _ws(L, 10, 1000, _opts(), 65536) == 0
    o = _opts(block_size=4096)
    assert _ws(L, 1 << 20, 1 << 30, o) == 0 and _ws(L, 1, 1 << 63, o) == 0  # more jobs than a launch counts
    assert _ws(L, (1 << 31) - 2, 0, o) > 0 and _ws(L, (1 << 31) - 1, 0, o) == 0
    assert _ws(L, (1 << 31) - 2, 4096, o) > 0 and _ws(L, (1 << 30), 4097, o) == 0


# ---------------------------------------------------------------- the shared rules, run on the CPU
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    S = cshim.build_shim(tmp_path_factory, "cbatch", "batch/cbatch_shim.c")
    for f in ("t_rec_size", "t_item_size", "t_shape_size", "t_job_size"):
        getattr(S, f).restype = C.c_size_t
    assert (S.t_rec_size(), S.t_item_size(), S.t_shape_size(), S.t_job_size()) == (REC_BYTES, 32, C.sizeof(Shape), JOB.itemsize)
    assert C.sizeof(Rec) == REC_BYTES and C.sizeof(Item) == 32 and JOB.itemsize + 4 + 8 == JOB_BYTES
    S.t_shape.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Shape)]
    S.t_cap.restype = C.c_uint64
    S.t_cap.argtypes = [C.POINTER(Item), C.c_uint64]
    S.t_src_ok.argtypes = [C.POINTER(Item), C.c_uint64]
    S.t_known_size.restype = C.c_uint64
    S.t_known_size.argtypes = [C.c_uint64, C.c_int, C.c_int]
    S.t_image_chunk.restype = C.c_uint64
    S.t_image_chunk.argtypes = [C.c_uint32, C.c_uint32]
    S.t_chunk_len.restype = C.c_uint32
    S.t_chunk_len.argtypes = [C.POINTER(Shape), C.c_uint32]
    S.t_plan_item.restype = None
    S.t_plan_item.argtypes = [C.POINTER(Item), C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_int,
                              C.POINTER(Rec), C.c_void_p]
    S.t_finish_item.restype = None
    S.t_finish_item.argtypes = [C.POINTER(Rec), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_int,
                                C.c_int, C.c_uint32]
    S.t_gathers.argtypes = [C.POINTER(Rec), C.c_uint32]
    return S


def test_shape_matches_the_library_and_the_chunks_cover_every_job(shim, L):
    for bs in BLOCK_SIZES:
        for n, ms in ((0, 100), (1, 0), (7, 3 * bs + 5), (300, bs), (70000, bs), (5000, 14 * bs + 1)):
            for D in (0, 1, 1000, 65535):
                sh = Shape()
                assert shim.t_shape(n, ms, bs, _stride(bs), D, C.byref(sh)) == 0
                J = max(1, -(-ms // bs))
                assert (sh.J, sh.n_jobs, sh.slot_stride) == (J, n * J, _stride(bs))
                assert sh.bytes == _ws(L, n, ms, _opts(block_size=bs), D)
                parts = [sh.o_rec, sh.o_jobs, sh.o_sizes, sh.o_offsets, sh.o_slots, sh.o_images, sh.bytes - 256]
                assert all(p % 256 == 0 for p in parts) and parts == sorted(parts)
                assert sh.o_jobs - sh.o_rec >= n * REC_BYTES and sh.o_sizes - sh.o_jobs >= 16 * n * J
                assert sh.o_offsets - sh.o_sizes >= 4 * n * J and sh.o_slots - sh.o_offsets >= 8 * n * J
                assert sh.o_images - sh.o_slots >= n * J * _stride(bs)
                chunk = int(shim.t_image_chunk(bs, D))
                assert chunk == max(4096, (256 << 20) // (bs + D))
                if D == 0:
                    assert sh.chunk_jobs == 0 and sh.bytes - 256 == sh.o_images
                    continue
                assert sh.chunk_jobs == min(n * J, chunk)
                assert sh.bytes - 256 - sh.o_images >= sh.chunk_jobs * (bs + D) + (64 if n else 0)  # the images and the over-read's pad
                covered, c0 = 0, 0
                while c0 < sh.n_jobs:  # the loop of the entry point
                    ln = int(shim.t_chunk_len(C.byref(sh), c0))
                    assert 0 < ln <= sh.chunk_jobs and c0 % sh.chunk_jobs == 0
                    covered, c0 = covered + ln, c0 + sh.chunk_jobs
                assert covered == sh.n_jobs
    sh = Shape()
    assert shim.t_shape(8, 100, 5000, 1, 0, C.byref(sh)) == ERR["BAD_BLOCK_SIZE"]
    assert shim.t_shape(1 << 20, 1 << 30, 4096, _stride(4096), 0, C.byref(sh)) == ERR["MEMORY"]


def _assemble(shim, arcs, bs, checksum, seekable, has_dict, dict_id, seed, caps=None):
    """the call as the kernels make it over items whose blocks are `arcs`' blocks: clear, plan, "encode" (each job's slot and size
    are the archive's block), finish, gather. -> (results, destination, items, recs); caps: capacity per item instead of exact"""
    rng = random.Random(seed)
    n, S = len(arcs), _stride(bs)
    max_size = max(a.size for a in arcs)
    items, src_at, dst_at = [], 0, 0
    for k, a in enumerate(arcs):  # sources and destinations at odd offsets, 16-aligned ones in between, with gaps
        src_at += 1 + rng.randrange(40)
        dst_at = (dst_at + 15) // 16 * 16 + 16 * rng.randrange(3) + (0 if k % 2 == 0 else 1 + rng.randrange(15))
        cap = len(a.comp) if caps is None else caps[k]
        items.append(Item(src_at, a.size, dst_at, cap))
        src_at, dst_at = src_at + a.size, dst_at + cap
    src_cap, dst_cap = src_at, dst_at + 7
    order = list(range(n))
    rng.shuffle(order)  # offsets in the table are not monotone
    items, arcs = [items[i] for i in order], [arcs[i] for i in order]
    sh = Shape()
    assert shim.t_shape(n, max_size, bs, S, 0, C.byref(sh)) == 0
    J, nj = sh.J, sh.n_jobs
    jobs = np.zeros(nj, dtype=JOB)
    sizes = np.zeros(nj, dtype=np.uint32)
    offsets = np.full(nj, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    slots = np.full(nj * S, 0xEE, dtype=np.uint8)
    dst = np.full(dst_cap + 64, CANARY, dtype=np.uint8)
    recs = []
    for r, it in enumerate(items):
        rec = Rec()
        C.memset(C.byref(rec), 0xEE, C.sizeof(rec))
        shim.t_plan_item(C.byref(it), r, J, src_cap, max_size, dst_cap, bs, int(checksum), int(seekable), C.byref(rec), jobs.ctypes.data)
        recs.append(rec)
    for r, (it, a, rec) in enumerate(zip(items, arcs, recs)):
        mine = jobs[r * J: (r + 1) * J]
        if rec.result < 0:
            assert rec.nb == 0 and not mine["len"].any()  # a refused item fills no job
            continue
        assert rec.nb == len(a.blocks) == -(-a.size // bs) and not mine["len"][rec.nb:].any()
        for b in range(rec.nb):
            assert int(mine["src_off"][b]) == it.src_off + b * bs and int(mine["len"][b]) == min(bs, a.size - b * bs)
            i = r * J + b
            blk = a.blocks[b]
            slots[i * S: i * S + len(blk)] = np.frombuffer(blk, dtype=np.uint8)
            sizes[i] = len(blk)
    for r, rec in enumerate(recs):
        shim.t_finish_item(C.byref(rec), sizes[r * J:].ctypes.data, offsets[r * J:].ctypes.data, slots[r * J * S:].ctypes.data, S,
                           dst.ctypes.data, bs, int(checksum), int(seekable), int(has_dict), dict_id)
    for i in range(nj):  # the gather, one job at a time
        rec = recs[i // J]
        if shim.t_gathers(C.byref(rec), i % J):
            at = rec.dst_off + int(offsets[i])
            dst[at: at + int(sizes[i])] = slots[i * S: i * S + int(sizes[i])]
    return [int(rec.result) for rec in recs], dst, items, arcs


def _check_exact(shim, arcs, key, seed):
    bs, checksum, seekable, has_dict, dict_id = key
    results, dst, items, arcs = _assemble(shim, arcs, bs, checksum, seekable, has_dict, dict_id, seed)
    keep = np.zeros(len(dst), dtype=bool)
    for rc, it, a in zip(results, items, arcs):
        assert rc == len(a.comp), (a.what, key, rc)
        assert dst[it.dst_off: it.dst_off + rc].tobytes() == a.comp, (a.what, key)
        keep[it.dst_off: it.dst_off + rc] = True
    assert (dst[~keep] == CANARY).all(), key  # nothing outside the items' archives


@pytest.mark.parametrize("bs", [4096, 65536])
@pytest.mark.parametrize("checksum", [0, 1])
@pytest.mark.parametrize("seekable", [0, 1])
def test_rules_put_the_reference_archives_together_again(shim, ref, bs, checksum, seekable):
    arcs = _ref_arcs(ref, bs, checksum, seekable)
    assert all(a.regular and a.bs == bs and a.checksum == bool(checksum) and a.seekable == bool(seekable and a.blocks) for a in arcs)
    assert sorted(len(a.blocks) for a in arcs) == [0, 1, 1, 1, 1, 2, 2, 4]
    _check_exact(shim, arcs + arcs, (bs, checksum, seekable, 0, 0), seed=bs + 2 * checksum + seekable)  # every archive at two places


def test_rules_put_the_golden_archives_together_again(shim):
    groups = {}
    for d in ("conformance/valid", "format", "synth"):
        p = os.path.join(GOLDEN, d)
        for f in sorted(os.listdir(p)) if os.path.isdir(p) else ():
            if f.endswith(".zxc"):
                try:
                    a = Arc(open(os.path.join(p, f), "rb").read(), f"{d}/{f}")
                except (AssertionError, IndexError):
                    continue  # (a format vector that is no complete archive)
                # an archive without blocks has no seek table whatever the option was: it goes with both kinds
                kinds = (0, 1) if not a.blocks else (int(a.seekable),)
                if a.regular:
                    for sk in kinds:
                        groups.setdefault((a.bs, int(a.checksum), sk, int(a.has_dict), a.dict_id), []).append(a)
    n = sum(len(v) for v in groups.values())
    assert n >= 30 and len(groups) >= 6, (n, sorted(groups))
    assert any(k[3] for k in groups) and {k[0] for k in groups} >= {4096, 65536}  # a dictionary header among them
    for key, arcs in sorted(groups.items()):
        _check_exact(shim, arcs, key, seed=len(arcs))


def _one(shim, a, cap, seed=1):
    results, dst, items, _ = _assemble(shim, [a], a.bs, a.checksum, a.seekable, 0, 0, seed, caps=[cap])
    return results[0], dst, items[0]


def test_rule_verdicts(shim, ref):
    for checksum in (0, 1):
        for seekable in (0, 1):
            for a in _ref_arcs(ref, 4096, checksum, seekable):
                n = len(a.comp)
                rc, dst, it = _one(shim, a, n - 1)  # one byte short: nothing of the item is written
                assert rc == ERR["DST_TOO_SMALL"] and (dst == CANARY).all(), a.what
                rc, dst, it = _one(shim, a, n + 5)
                assert rc == n and dst[it.dst_off: it.dst_off + n].tobytes() == a.comp and (dst[it.dst_off + n:] == CANARY).all()
                known = int(shim.t_known_size(len(a.blocks), checksum, seekable))
                assert known <= n and known == 16 + len(a.blocks) * (8 + 4 * checksum) + 8 + ((8 + 4 * len(a.blocks)) if seekable and a.blocks else 0) + 12
                rc, dst, it = _one(shim, a, known - 1)  # refused by the plan: no job is filled (_assemble checks it)
                assert rc == ERR["DST_TOO_SMALL"] and (dst == CANARY).all()


def _plan(shim, it, J=4, src_cap=1 << 20, max_size=4 * 4096, dst_cap=1 << 20, bs=4096, checksum=0, seekable=1):
    rec, jobs = Rec(), np.zeros(J, dtype=JOB)
    shim.t_plan_item(C.byref(it), 0, J, src_cap, max_size, dst_cap, bs, checksum, seekable, C.byref(rec), jobs.ctypes.data)
    return rec, jobs


def test_plan_verdicts_and_their_order(shim):
    bs, big = 4096, 1 << 16
    rec, jobs = _plan(shim, Item(101, 2 * bs + 5, 7, big))
    assert (rec.result, rec.nb, rec.cap, rec.dst_off, rec.src_size) == (0, 3, big, 7, 2 * bs + 5)
    assert [(int(j["src_off"]), int(j["len"])) for j in jobs] == [(101, bs), (101 + bs, bs), (101 + 2 * bs, 5), (0, 0)]
    rec, jobs = _plan(shim, Item(101, 0, 7, 36))  # an empty item: header, EOF block, footer; its one job stays unused
    assert (rec.result, rec.nb) == (0, 0) and not jobs["len"].any()
    assert _plan(shim, Item(101, 0, 7, 35))[0].result == ERR["DST_TOO_SMALL"]
    src_cap = 1 << 20
    for it in (Item(src_cap - 10, 11, 0, big), Item(src_cap + 1, 0, 0, big), Item(M64 - 10, 100, 0, big), Item(100, M64 - 50, 0, big),
               Item(M64, M64, 0, big)):  # past the capacity, and src_off + src_size wrapping 64 bits
        rec, jobs = _plan(shim, it, src_cap=src_cap)
        assert rec.result == ERR["SRC_TOO_SMALL"] and rec.nb == 0 and not jobs["len"].any() and not shim.t_src_ok(C.byref(it), src_cap)
    assert _plan(shim, Item(src_cap - 10, 10, 0, big), src_cap=src_cap)[0].result == 0  # ends exactly at the capacity
    assert _plan(shim, Item(src_cap, 0, 0, big), src_cap=src_cap)[0].result == 0
    rec, jobs = _plan(shim, Item(0, 4 * bs + 1, 0, big))
    assert rec.result == ERR["OVERFLOW"] and not jobs["len"].any()
    assert _plan(shim, Item(0, 4 * bs, 0, big))[0].nb == 4
    # dst_off behind the destination area: capacity 0, which holds no archive
    for d in ((1 << 20) + 1, M64):
        it = Item(0, 100, d, big)
        assert shim.t_cap(C.byref(it), 1 << 20) == 0 and _plan(shim, it)[0].result == ERR["DST_TOO_SMALL"]
    it = Item(0, 100, (1 << 20) - 50, big)  # the area's end binds
    assert shim.t_cap(C.byref(it), 1 << 20) == 50 and _plan(shim, it)[0].result == ERR["DST_TOO_SMALL"]
    assert shim.t_cap(C.byref(Item(0, 100, 10, 77)), 1 << 20) == 77
    # order: the source bounds, then max_size, then the capacity
    assert _plan(shim, Item(M64, 5 * bs, M64, 0))[0].result == ERR["SRC_TOO_SMALL"]
    assert _plan(shim, Item(0, 5 * bs, M64, 0))[0].result == ERR["OVERFLOW"]


def test_finish_refuses_sizes_outside_the_legal_range(shim):
    bs, S = 4096, _stride(4096)
    for checksum in (0, 1):
        lo, hi = 8 + 4 * checksum, bs + 64
        for bad, want in ((0, "CORRUPT_DATA"), (lo - 1, "CORRUPT_DATA"), (hi + 1, "CORRUPT_DATA"), (M64 >> 32, "CORRUPT_DATA"), (lo, None),
                          (hi, None)):
            for where in (0, 2):
                rec, _ = _plan(shim, Item(0, 3 * bs, 3, 1 << 16), checksum=checksum)
                sizes = np.array([100, 200, 300, 0], dtype=np.uint32)
                sizes[where] = bad
                offsets = np.zeros(4, dtype=np.uint64)
                slots = np.zeros(4 * S, dtype=np.uint8)
                dst = np.full(1 << 16, CANARY, dtype=np.uint8)
                shim.t_finish_item(C.byref(rec), sizes.ctypes.data, offsets.ctypes.data, slots.ctypes.data, S, dst.ctypes.data, bs, checksum,
                                   1, 0, 0)
                if want:
                    assert rec.result == ERR[want] and (dst == CANARY).all() and not shim.t_gathers(C.byref(rec), 0), (bad, where)
                else:
                    assert rec.result == 16 + int(sizes[:3].sum()) + 8 + 8 + 12 + 12 and shim.t_gathers(C.byref(rec), 2)
                    assert not shim.t_gathers(C.byref(rec), 3)
                    assert list(offsets[:3]) == [16, 16 + int(sizes[0]), 16 + int(sizes[0]) + int(sizes[1])]


def test_rules_under_sanitizers(tmp_path):
    """the stand-alone program tests/batch/cbatch_san_main.c (its own main; nothing of it is loaded into this process)"""
    r = cshim.run_san_program(tmp_path, "batch/cbatch_san_main.c")
    assert "CBATCH OK 128" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
