"""zxc_mi355x_decompress_batch_device without a GPU: the three symbols and the Python names, every synchronous argument check in its
stated order (the device pointers below are never dereferenced), the work-size arithmetic, and the rules the kernels run
(zxc_amd/csrc/zxc_batch.h), compiled here with the host C compiler and driven over one arena that holds every golden archive at a
random offset: each item is planned, its jobs are fed to the oracle's block decoder, its slots are copied out and its verdict is
taken, and the result must be what the oracle's whole-frame decoder (the CPU restatement of zxc_decompress) returns for the same
bytes, capacity and options, with every write inside the item's own destination or the job's own slot."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import cshim
from conftest import GOLDEN, load_dict
from cshim import FAKE_DICT, FAKE_ID, dd as _dd, ref as _ref
from devtest import ERR
from zxc_amd.api import _DecompressOpts

FAKE_SRC, FAKE_ITEMS, FAKE_DST, FAKE_WORK, FAKE_RES = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
BAD_BLOCK_SIZES = (0, 1000, 2048, 4095, 5000, 3 << 12, 1 << 22)
BLOCK_SIZES = (4096, 65536, 1 << 19, 1 << 21)
REC_BYTES, JOB_BYTES, WORK_FIXED = 128, 56, 1536  # the stated bound: n J (block_size + 64) + 56 n J + 128 n + 1536
SLOT_PAD = 64
CANARY = 0xC3
DST_REL = 1 << 40  # d_dst's distance from the launch's base in the emulation: an out_off at or above it is a place in d_dst


@pytest.fixture(scope="module")
def L(product):
    L = product.lib()
    assert hasattr(L, "zxc_mi355x_decompress_batch_device"), "libzxc_mi355x.so does not export zxc_mi355x_decompress_batch_device"
    return L


def _ws(L, n, max_cap, bs):
    return int(L.zxc_mi355x_decompress_batch_device_work_size(n, max_cap, bs))


def _call(L, n=8, max_cap=100000, bs=65536, src_cap=1 << 20, cap=1 << 20, src=FAKE_SRC, items=FAKE_ITEMS, dst=FAKE_DST, work=FAKE_WORK,
          ws=None, res=FAKE_RES, opts=None, d=False):
    """d: False = the call without a dictionary argument, else the zxc_dev_dict_t (or None) of the _dict call"""
    ws = max(_ws(L, n, max_cap, bs), 1) if ws is None else ws
    if d is False:
        return L.zxc_mi355x_decompress_batch_device(src, src_cap, items, n, max_cap, dst, cap, bs, _ref(opts), work, ws, res, None)
    return L.zxc_mi355x_decompress_batch_dict_device(src, src_cap, items, n, max_cap, dst, cap, bs, _ref(opts), _ref(d), work, ws, res, None)


def _host_dict_opts():
    return cshim.host_dict(_DecompressOpts())


def test_symbols_and_names_exported(product):
    L = product.lib()
    for sym in ("zxc_mi355x_decompress_batch_device_work_size", "zxc_mi355x_decompress_batch_device",
                "zxc_mi355x_decompress_batch_dict_device"):
        assert hasattr(L, sym), sym
    for name in ("ITEM_DTYPE", "decompress_batch_device_work_size", "decompress_batch_device", "decompress_batch_dict_device"):
        assert hasattr(product, name) and hasattr(product.api, name), name
    assert all(sym in product.api._PROTOTYPES for sym in ("zxc_mi355x_decompress_batch_device_work_size", "zxc_mi355x_decompress_batch_device",
                                                          "zxc_mi355x_decompress_batch_dict_device"))
    assert product.ITEM_DTYPE.itemsize == 32 and product.ITEM_DTYPE.names == ("src_off", "src_size", "dst_off", "dst_capacity")


def test_each_synchronous_error_and_their_order(L):
    for d in (False, None, _dd()):
        for k in ("src", "work", "res", "items", "dst"):
            assert _call(L, d=d, **{k: None}) == ERR["NULL_INPUT"], k
        for bad in BAD_BLOCK_SIZES:
            assert _call(L, d=d, bs=bad, ws=1 << 40) == ERR["BAD_BLOCK_SIZE"], bad
        assert _call(L, d=d, opts=_host_dict_opts()) == ERR["GPU_UNSUPPORTED"]
        for off in (1, 4, 8, 15):
            assert _call(L, d=d, dst=FAKE_DST + off) == ERR["GPU_UNSUPPORTED"], off
        assert _call(L, d=d, n=1 << 20, max_cap=1 << 30, bs=4096, ws=1 << 62) == ERR["MEMORY"]  # 2^20 x (2^18 + 1) jobs
        assert _call(L, d=d, n=1, max_cap=1 << 63, bs=4096, ws=1 << 62) == ERR["MEMORY"]
        for n, mc, bs in ((1, 1, 4096), (8, 100000, 65536), (20000, 3 << 16, 65536), (5, 0, 4096)):
            assert _call(L, d=d, n=n, max_cap=mc, bs=bs, ws=_ws(L, n, mc, bs) - 1) == ERR["MEMORY"], (n, mc, bs)
        # nothing to do is fine, with or without a device and an item table; the argument checks still come first
        assert _call(L, d=d, n=0, items=None) == 0
        assert _call(L, d=d, n=0, cap=0, dst=None) == 0
        assert _call(L, d=d, n=0, max_cap=1 << 63) == 0  # no item: no job to count
        assert _call(L, d=d, n=0, work=None) == ERR["NULL_INPUT"]
        assert _call(L, d=d, n=0, ws=0) == ERR["MEMORY"]
        assert _call(L, d=d, n=0, bs=5000) == ERR["BAD_BLOCK_SIZE"]
    # the dictionary argument, as dict_arg judges it
    assert _call(L, d=_dd(size=65536)) == ERR["DICT_TOO_LARGE"]
    assert _call(L, d=_dd(content=None)) == ERR["NULL_INPUT"]
    assert _call(L, d=_dd(id_=None)) == ERR["NULL_INPUT"]
    # each call breaks one rule and every later one; the earliest is reported
    late = dict(dst=FAKE_DST + 1, ws=0)
    assert _call(L, src=None, bs=5000, opts=_host_dict_opts(), d=_dd(size=1 << 20, id_=None), **late) == ERR["NULL_INPUT"]
    assert _call(L, bs=5000, opts=_host_dict_opts(), d=_dd(size=1 << 20, id_=None), **late) == ERR["BAD_BLOCK_SIZE"]
    assert _call(L, opts=_host_dict_opts(), d=_dd(size=1 << 20, id_=None), **late) == ERR["GPU_UNSUPPORTED"]  # the host dictionary
    assert _call(L, d=_dd(size=1 << 20, id_=None), **late) == ERR["DICT_TOO_LARGE"]
    assert _call(L, d=_dd(id_=None), **late) == ERR["NULL_INPUT"]
    assert _call(L, d=_dd(), **late) == ERR["GPU_UNSUPPORTED"]  # the alignment
    assert _call(L, d=_dd(), ws=0) == ERR["MEMORY"]
    assert _call(L, bs=5000, opts=_host_dict_opts(), **late) == ERR["BAD_BLOCK_SIZE"]
    assert _call(L, opts=_host_dict_opts(), **late) == ERR["GPU_UNSUPPORTED"]
    assert _call(L, **late) == ERR["GPU_UNSUPPORTED"]
    assert _call(L, ws=0) == ERR["MEMORY"]
    assert _call(L, n=0, ws=0) == ERR["MEMORY"]  # the work size comes in front of "nothing to do"


def test_valid_arguments_without_a_device(product, L):
    """What remains after the argument checks is the device check. Only on a machine without a device is the call made (elsewhere
    these pointers would reach a kernel)."""
    if product.lib().zxc_mi355x_device_count() == 0:
        for d in (False, None, _dd(), _dd(huf=None, size=65535), _dd(size=0, content=None, id_=None)):
            assert _call(L, d=d) == ERR["GPU_UNAVAILABLE"]
            assert _call(L, d=d, cap=0, dst=None) == ERR["GPU_UNAVAILABLE"]
            assert _call(L, d=d, opts=_DecompressOpts(checksum_enabled=1), bs=4096) == ERR["GPU_UNAVAILABLE"]
            assert _call(L, d=d, n=0) == 0
        with pytest.raises(product.ZxcError) as e:
            product.decompress_batch_device(FAKE_SRC, 1 << 20, FAKE_ITEMS, 4, 1000, FAKE_DST, 1 << 20, 4096, FAKE_WORK, 1 << 30, FAKE_RES)
        assert e.value.code == ERR["GPU_UNAVAILABLE"]


def test_python_binding_raises(product):
    with pytest.raises(product.ZxcError) as e:
        product.decompress_batch_device(FAKE_SRC, 1 << 20, FAKE_ITEMS, 4, 1000, FAKE_DST, 1 << 20, 5000, FAKE_WORK, 1 << 30, FAKE_RES)
    assert e.value.code == ERR["BAD_BLOCK_SIZE"]
    with pytest.raises(product.ZxcError) as e:
        product.decompress_batch_device(FAKE_SRC, 1 << 20, FAKE_ITEMS, 4, 1000, FAKE_DST, 1 << 20, 4096, FAKE_WORK, 1, FAKE_RES, checksum=True)
    assert e.value.code == ERR["MEMORY"]
    with pytest.raises(product.ZxcError) as e:
        product.decompress_batch_device(FAKE_SRC, 1 << 20, 0, 4, 1000, FAKE_DST, 1 << 20, 4096, FAKE_WORK, 1 << 30, FAKE_RES)
    assert e.value.code == ERR["NULL_INPUT"]
    with pytest.raises(product.ZxcError) as e:
        product.decompress_batch_dict_device(FAKE_SRC, 1 << 20, FAKE_ITEMS, 4, 1000, FAKE_DST, 1 << 20, 4096, (FAKE_DICT, 70000, 0, FAKE_ID),
                                             FAKE_WORK, 1 << 30, FAKE_RES)
    assert e.value.code == ERR["DICT_TOO_LARGE"]
    product.decompress_batch_device(FAKE_SRC, 1 << 20, 0, 0, 1000, FAKE_DST, 1 << 20, 4096, FAKE_WORK, 1 << 30, FAKE_RES)  # nothing to do
    assert product.decompress_batch_device_work_size(4, 1000, 5000) == 0
    assert product.decompress_batch_device_work_size(4, 1000, 4096) > 0


def test_work_size(L):
    for bs in BLOCK_SIZES:
        for n in (0, 1, 7, 300, 20000):
            prev = 0
            for mc in sorted((0, 1, 100, bs - 1, bs, bs + 1, 2 * bs, 3 * bs + 5, 1 << 22)):
                w = _ws(L, n, mc, bs)
                J = -(-mc // bs) + 1
                assert w > 0 and w >= prev, (bs, n, mc)
                assert w >= n * J * (bs + 32 + JOB_BYTES) + REC_BYTES * n, (bs, n, mc)
                assert w <= n * J * (bs + SLOT_PAD) + JOB_BYTES * n * J + REC_BYTES * n + WORK_FIXED, (bs, n, mc, w)
                prev = w
        prev = 0
        for n in (0, 1, 2, 255, 256, 257, 5000, 100000):
            w = _ws(L, n, 3 * bs, bs)
            assert w > prev, (bs, n)
            prev = w
    for bad in BAD_BLOCK_SIZES:
        assert _ws(L, 10, 1000, bad) == 0, bad
    assert _ws(L, 1 << 20, 1 << 30, 4096) == 0 and _ws(L, 1, 1 << 63, 4096) == 0  # more jobs than a launch counts
    assert _ws(L, (1 << 31) - 2, 0, 4096) > 0 and _ws(L, (1 << 31) - 1, 0, 4096) == 0
    assert _ws(L, (1 << 30) - 1, 4096, 4096) > 0 and _ws(L, 1 << 30, 4096, 4096) == 0


# ---------------------------------------------------------------- the shared rules, run on the CPU
class Ctl(C.Structure):  # zc_ctl_t
    _fields_ = [("head_result", C.c_int64), ("total", C.c_uint64), ("eof_at", C.c_uint64), ("event", C.c_uint64), ("final", C.c_uint32),
                ("file_ck", C.c_uint32), ("verify", C.c_uint32), ("sel", C.c_uint32), ("stored_hash", C.c_uint32), ("nb", C.c_uint32),
                ("seek", C.c_uint32), ("found", C.c_uint32), ("done", C.c_uint32), ("saw_eof", C.c_uint32), ("tail_err", C.c_int32),
                ("ghash", C.c_uint32)]


class Rec(C.Structure):  # zb_rec_t
    _fields_ = [("c", Ctl), ("cap", C.c_uint64), ("dst_off", C.c_uint64), ("rsv", C.c_uint64 * 4)]


class Item(C.Structure):  # zxc_dev_item_t
    _fields_ = [("src_off", C.c_uint64), ("src_size", C.c_uint64), ("dst_off", C.c_uint64), ("dst_capacity", C.c_uint64)]


class Shape(C.Structure):  # zb_shape_t
    _fields_ = [(n, C.c_uint32) for n in ("J", "n_jobs", "slot_stride", "copy_chunks")] + \
               [(n, C.c_uint64) for n in ("o_rec", "o_jobs", "o_status", "o_stage", "bytes")]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    S = cshim.build_shim(tmp_path_factory, "batch", "batch/batch_shim.c")
    for f in ("t_rec_size", "t_item_size", "t_shape_size", "t_job_size"):
        getattr(S, f).restype = C.c_size_t
    assert (S.t_rec_size(), S.t_item_size(), S.t_shape_size(), S.t_job_size()) == (REC_BYTES, 32, C.sizeof(Shape), 24)
    assert C.sizeof(Rec) == REC_BYTES and C.sizeof(Item) == 32
    S.t_shape.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(Shape)]
    S.t_cap.restype = C.c_uint64
    S.t_cap.argtypes = [C.POINTER(Item), C.c_uint64, C.c_uint64]
    S.t_src_ok.argtypes = [C.POINTER(Item), C.c_uint64]
    S.t_plan_item.restype = None
    S.t_plan_item.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(Item), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32,
                              C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.POINTER(Rec), C.c_void_p]
    S.t_direct.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64]
    S.t_copy_bytes.restype = C.c_uint32
    S.t_copy_bytes.argtypes = [C.POINTER(Rec), C.c_uint32, C.c_int32, C.c_uint32]
    S.t_verdict_item.restype = C.c_int64
    S.t_verdict_item.argtypes = [C.POINTER(Rec), C.c_void_p, C.c_uint32]
    return S


def _golden_archives():
    out = []
    for d in ("conformance/valid", "conformance/invalid", "format", "synth"):
        p = os.path.join(GOLDEN, d)
        if os.path.isdir(p):
            out += [f"{d}/{f}" for f in sorted(os.listdir(p)) if f.endswith(".zxc")]
    return out


def _bs_of(comp):
    lg = comp[5] if len(comp) > 5 else 0
    return 1 << lg if 12 <= lg <= 21 else 65536


def _size_of(product, rel, comp):
    exp = os.path.join(GOLDEN, rel[:-4] + ".expected")
    if os.path.exists(exp):
        return os.path.getsize(exp)
    return product.get_decompressed_size(comp) if len(comp) >= 28 else 0


def _dictionaries(product):
    """-> [(name, content or None, table or None, zxc_dict_id)]: none, the two golden .zxd, the format vectors' dictionary"""
    L = product.lib()
    L.zxc_dict_id.restype = C.c_uint32
    L.zxc_dict_id.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p]
    out = [("none", None, None, 0)]
    for name in ("dict_http.zxd", "dict_text.zxd"):
        content, huf = load_dict(os.path.join(GOLDEN, "conformance", "valid", name))
        out.append((name, content, huf, L.zxc_dict_id(content, len(content), huf)))
    gc = open(os.path.join(GOLDEN, "format", "gc_dict.bin"), "rb").read()
    gc_huf = open(os.path.join(GOLDEN, "format", "gc_dict_huf.bin"), "rb").read()
    out.append(("gc_dict", gc, None, L.zxc_dict_id(gc, len(gc), None)))
    out.append(("gc_dict+huf", gc, gc_huf, L.zxc_dict_id(gc, len(gc), gc_huf)))
    return out


class Arena:
    """every golden archive at a random offset of one source area, with unrelated bytes between them"""

    def __init__(self, product, seed=7):
        rng = random.Random(seed)
        buf, self.where = bytearray(), {}
        for rel in _golden_archives():
            comp = open(os.path.join(GOLDEN, rel), "rb").read()
            buf += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 200)))
            self.where[rel] = (len(buf), comp, _bs_of(comp), _size_of(product, rel, comp))
            buf += comp
        buf += bytes(64)
        self.bytes = bytes(buf)
        self.capacity = len(buf) - 64


@pytest.fixture(scope="module")
def arena(product):
    return Arena(product)


def _decode(oracle, blk, bs, checksum, content, huf):
    """the oracle's block decoder, with the dictionary the call has -> (status, bytes)"""
    import oracle_py
    if content is None:
        return oracle.decode_block(blk, bs, checksum=checksum)
    keep = (C.create_string_buffer(content, len(content)), C.create_string_buffer(huf, 128) if huf else None)
    ctx = oracle_py.OracleCtx(bs, int(checksum), C.cast(keep[0], C.c_void_p), len(content), C.cast(keep[1], C.c_void_p) if huf else None, 0)
    cap = bs + 2112
    out = C.create_string_buffer(cap + 1)
    rc = oracle.lib.zxo_decode_block(C.byref(ctx), blk, len(blk), out, cap)
    return rc, out.raw[:max(rc, 0)]


def _emulate(shim, oracle, src, src_capacity, items, max_cap, dst_capacity, bs, verify, dic):
    """the call as the kernels make it: clear, plan, decode (the oracle's block decoder), copy-out, verdict.
    -> (results, destination bytearray of dst_capacity + 4096 bytes, records)"""
    name, content, huf, did = dic
    sh = Shape()
    assert shim.t_shape(len(items), max_cap, bs, C.byref(sh)) == 0
    J, nj = sh.J, sh.n_jobs
    assert J == -(-max_cap // bs) + 1 and nj == J * len(items) and sh.slot_stride == bs + SLOT_PAD
    jobs = np.zeros(2 * nj, dtype=[("comp_off", "<u8"), ("out_off", "<u8"), ("comp_size", "<u4"), ("out_len", "<u4")])
    status = np.full(2 * nj, ERR["SRC_TOO_SMALL"], dtype=np.int32)  # what an empty job is answered with
    dst = bytearray([CANARY]) * (dst_capacity + 4096)
    recs, results, slots = [], [], set()
    for r, it in enumerate(items):
        rec = Rec()
        C.memset(C.byref(rec), 0xEE, C.sizeof(rec))
        shim.t_plan_item(src, src_capacity, C.byref(it), r, J, nj, max_cap, dst_capacity, bs, int(verify), DST_REL, 0,
                         int(content is not None), did, C.byref(rec), jobs.ctypes.data)
        recs.append(rec)
    for r, (it, rec) in enumerate(zip(items, recs)):
        cap = int(shim.t_cap(C.byref(it), max_cap, dst_capacity))
        assert rec.cap == cap and rec.dst_off == it.dst_off and rec.c.seek == 0
        assert cap <= it.dst_capacity and cap <= max_cap and (cap == 0 or it.dst_off + cap <= dst_capacity)
        sel = rec.c.sel
        assert sel in (0, 1) and (verify or sel == 0)
        assert not jobs["comp_size"][(1 - sel) * nj + r * J: (1 - sel) * nj + (r + 1) * J].any()  # the other table stays empty
        mine = jobs[sel * nj + r * J: sel * nj + (r + 1) * J]
        if rec.c.final:
            assert rec.c.found == 0 and not mine["comp_size"].any()  # answered by the head: no block is decoded
        assert rec.c.found <= -(-cap // bs) + 1 <= J and not mine["comp_size"][rec.c.found:].any()
        for i in range(rec.c.found):
            job, ji = mine[i], r * J + i
            off, n, out_off, out_len = int(job["comp_off"]), int(job["comp_size"]), int(job["out_off"]), int(job["out_len"])
            assert n > 0 and it.src_off + 16 <= off and off + n <= it.src_off + it.src_size  # inside the item's own bytes
            assert out_len == bs and out_off % 16 == 0
            window = (out_len + 15) // 16 * 16 + 16  # the decoders store 16 bytes at a time
            rc, out = _decode(oracle, src[off: off + n], bs, sel == 1, content, huf)
            status[sel * nj + ji] = rc
            if out_off >= DST_REL:  # straight into the destination: the window lies inside the item's own capacity
                place = out_off - DST_REL
                assert shim.t_direct(it.dst_off, i, bs, cap) and place == it.dst_off + i * bs
                assert it.dst_off <= place and place + window <= it.dst_off + cap, (r, i)
                assert shim.t_copy_bytes(C.byref(rec), i, rc, bs) == 0
                dst[place: place + len(out[:bs])] = out[:bs]
            else:                   # its own slot, which no other job has
                assert not shim.t_direct(it.dst_off, i, bs, cap)
                assert out_off == ji * sh.slot_stride and out_off + window <= (ji + 1) * sh.slot_stride, (r, i)
                assert ji not in slots
                slots.add(ji)
                n_copy = shim.t_copy_bytes(C.byref(rec), i, rc, bs)
                at = i * bs
                assert n_copy == (0 if rc <= 0 or at >= cap else min(rc, bs, cap - at)), (r, i)
                dst[it.dst_off + at: it.dst_off + at + n_copy] = out[:n_copy]
        st = status[sel * nj + r * J: sel * nj + (r + 1) * J].copy()
        results.append(int(shim.t_verdict_item(C.byref(rec), st.ctypes.data, bs)))
    return results, dst, recs


def _place_items(entries, rng):
    """entries: [(src_off, src_size, size)] -> items with capacities exact, exact - 1, exact + 31, exact + 32 and 0 at destinations
    16-aligned and odd, with gaps; -> (items, [(entry index, capacity)], max_capacity, dst_capacity)"""
    items, meta, at = [], [], 0
    for e, (off, n, size) in enumerate(entries):
        for k, cap in enumerate((size, max(size - 1, 0), size + 31, size + 32, 0)):
            for odd in (0, 1):
                at = (at + 15) // 16 * 16 + 16 * rng.randrange(3)
                d = at + (0 if not odd else 1 + rng.randrange(15))
                items.append(Item(off, n, d, cap))
                meta.append((e, cap))
                at = d + cap
    order = list(range(len(items)))
    rng.shuffle(order)  # offsets in the table are not monotone
    return [items[i] for i in order], [meta[i] for i in order], max(c for _, c in meta), at + 64


def _check_batch(shim, oracle, arena, names, bs, verify, dic, seed):
    name, content, huf, did = dic
    entries = [(arena.where[rel][0], len(arena.where[rel][1]), arena.where[rel][3]) for rel in names]
    items, meta, max_cap, dst_cap = _place_items(entries, random.Random(seed))
    results, dst, recs = _emulate(shim, oracle, arena.bytes, arena.capacity, items, max_cap, dst_cap, bs, verify, dic)
    written = np.zeros(len(dst), dtype=bool)
    n_ok = 0
    for it, (e, cap), got in zip(items, meta, results):
        comp = arena.where[names[e]][1]
        want, data = oracle.decompress(comp, cap, checksum=verify, dict_=content, dict_huf=huf)
        assert got == want, (names[e], bs, verify, name, cap, it.dst_off, got, want)
        if got >= 0:
            assert bytes(dst[it.dst_off: it.dst_off + got]) == data, (names[e], cap)
            n_ok += got > 0
        written[it.dst_off: it.dst_off + cap] = True  # a failing item's own bytes are undefined
    assert (np.frombuffer(dst, dtype=np.uint8)[~written] == CANARY).all(), (bs, verify, name)  # nothing outside the items' destinations
    return n_ok


@pytest.mark.parametrize("verify", [False, True])
@pytest.mark.parametrize("dict_name", ["none", "dict_http.zxd", "dict_text.zxd", "gc_dict", "gc_dict+huf"])
def test_rules_over_one_arena_of_every_golden_archive(shim, product, oracle, arena, verify, dict_name):
    dic = [d for d in _dictionaries(product) if d[0] == dict_name][0]
    by_bs = {}
    for rel, (off, comp, bs, size) in arena.where.items():
        by_bs.setdefault(bs, []).append(rel)
    assert len(by_bs) >= 2 and sum(len(v) for v in by_bs.values()) == len(_golden_archives())  # no archive is left out
    n_ok = 0
    for bs, names in sorted(by_bs.items()):
        n_ok += _check_batch(shim, oracle, arena, names, bs, verify, dic, seed=bs + verify)
    assert n_ok >= (40 if dict_name == "none" else 20), n_ok


def test_dictionary_archives_decode_only_with_their_dictionary(shim, product, oracle, arena):
    dics = {d[0]: d for d in _dictionaries(product)}
    for rel, right in (("conformance/valid/dict_http.zxc", "dict_http.zxd"), ("conformance/valid/dict_seekable_l7.zxc", "dict_text.zxd")):
        off, comp, bs, size = arena.where[rel]
        items = [Item(off, len(comp), 0, size)]
        for name, want in (("none", ERR["DICT_REQUIRED"]), (right, size), ("gc_dict", ERR["DICT_MISMATCH"])):
            results, dst, recs = _emulate(shim, oracle, arena.bytes, arena.capacity, items, size, size, bs, True, dics[name])
            assert results == [want], (rel, name, results)
            if want < 0:
                assert recs[0].c.final and bytes(dst) == bytes([CANARY]) * len(dst)  # no block is decoded, nothing is written


def test_a_header_block_size_other_than_the_argument(shim, product, oracle, arena):
    none = _dictionaries(product)[0]
    for rel in ("conformance/valid/text_8k_bs4k.zxc", "conformance/valid/text_64k.zxc", "conformance/valid/text_64k_bs2m.zxc"):
        off, comp, bs, size = arena.where[rel]
        for other in BLOCK_SIZES:
            items = [Item(off, len(comp), 16, size), Item(off, len(comp), 16 + size + 48, 0)]
            results, dst, recs = _emulate(shim, oracle, arena.bytes, arena.capacity, items, size, 2 * size + 256, other, False, none)
            if other == bs:
                assert results == [size, ERR["DST_TOO_SMALL"]], (rel, other, results)
            else:  # the departure; the empty-frame probe answers in front of the header, as in zxc_decompress
                assert results == [ERR["BAD_BLOCK_SIZE"], ERR["DST_TOO_SMALL"]], (rel, other, results)
                assert bytes(dst) == bytes([CANARY]) * len(dst)


def test_items_out_of_the_source_and_destination_areas(shim, product, oracle, arena):
    none = _dictionaries(product)[0]
    off, comp, bs, size = arena.where["conformance/valid/text_8k_bs4k.zxc"]
    n, M = len(comp), (1 << 64) - 1
    src_cap = off + n  # the arena is cut right behind this archive
    dst_cap = 4 * size + 256
    items = [
        Item(off, n, 0, size),                        # 0: fine, ends exactly at src_capacity
        Item(off, n + 1, size + 16, size),            # 1: one byte past the source area
        Item(off + 1, n, size + 16, size),            # 2: ... shifted past it
        Item(src_cap, 28, size + 16, size),           # 3: starts at its end
        Item(src_cap + 1, 0, size + 16, size),        # 4: starts behind it
        Item(M - 10, 100, size + 16, size),           # 5: src_off + src_size wraps 64 bits
        Item(100, M - 50, size + 16, size),           # 6: ... from the size
        Item(M, M, size + 16, size),                  # 7
        Item(off, 27, size + 16, size),               # 8: shorter than a header and a footer
        Item(off, 0, size + 16, size),                # 9
        Item(off, n, dst_cap + 1, size),              # 10: dst_off behind the destination area: capacity 0, the empty-frame probe
        Item(off, n, M, size),                        # 11
        Item(off, n, dst_cap, size),                  # 12: at its very end: capacity 0 as well
        Item(off, n, dst_cap - size + 1, size),       # 13: the area ends one byte short of the archive
        Item(off, n, dst_cap - size, M),              # 14: fits exactly; the item's own capacity does not bind
        Item(off, n, 2 * size + 64, size + 100),      # 15: max_capacity (= size) binds
    ]
    assert [shim.t_src_ok(C.byref(it), src_cap) for it in items] == [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1]
    assert [int(shim.t_cap(C.byref(it), size, dst_cap)) for it in items[10:]] == [0, 0, 0, size - 1, size, size]
    results, dst, recs = _emulate(shim, oracle, arena.bytes, src_cap, items, size, dst_cap, bs, False, none)
    S, D = ERR["SRC_TOO_SMALL"], ERR["DST_TOO_SMALL"]
    assert results == [size] + [S] * 9 + [D, D, D, D, size, size], results
    for r in range(1, 10):
        assert recs[r].c.final and recs[r].c.found == 0
    want = oracle.decompress(comp, size)[1]
    for r in (0, 14, 15):
        assert bytes(dst[items[r].dst_off: items[r].dst_off + size]) == want, r
    touched = bytearray(len(dst))
    for r in (0, 13, 14, 15):
        c = int(shim.t_cap(C.byref(items[r]), size, dst_cap))
        touched[items[r].dst_off: items[r].dst_off + c] = b"\1" * c
    assert all(b == CANARY for b, t in zip(dst, touched) if not t)


def test_direct_exactly_when_aligned_and_inside_the_capacity(shim):
    bs, n_direct = 4096, 0
    for d in list(range(0, 34)) + [4096, 4097, 8192 + 16]:
        for cap in (0, 1, 31, 32, 4095, 4096, 4096 + 31, 4096 + 32, 4096 + 33, 8192, 8192 + 31, 8192 + 32, 12288 + 32, 16384 + 100):
            for i in range(0, cap // bs + 2):
                got = shim.t_direct(d, i, bs, cap)
                want = (d + i * bs) % 16 == 0 and (i + 1) * bs + 32 <= cap
                assert bool(got) == bool(want), (d, cap, i)
                n_direct += bool(got)
    assert n_direct > 20
