"""The device calls that take a dictionary in device memory, without a GPU: the five symbols and Python names, every synchronous
argument check in its documented order (the device pointers below are never dereferenced), the work-size bound of the compress call,
a NULL dictionary giving the sibling's answers, and the dictionary rules the kernels run (zxc_amd/csrc/zxc_container.h,
zxc_ranges.h), compiled here with the host C compiler and driven over the golden dictionary archives: the right id proceeds, a
wrong one is DICT_MISMATCH, none is DICT_REQUIRED, and the functions of the calls that take no dictionary answer as before."""
import ctypes as C
import os

import pytest

from conftest import GOLDEN
from cshim import FAKE_DICT, FAKE_HUF, FAKE_ID, build_shim, dd as _dd, ref as _ref
from devtest import ERR
from zxc_amd.api import _CompressOpts, _DecompressOpts, _DevDict

FAKE_SRC, FAKE_DST, FAKE_WORK, FAKE_RES, FAKE_IDX, FAKE_RNG = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
BAD_BLOCK_SIZES = (1000, 4095, 5000, 3 << 12, 1 << 22)
DICT_SIZES = (1, 4096, 65535)
IMAGE_BYTES, IMAGE_MIN_BLOCKS, WORK_SLACK = 256 << 20, 4096, 4096  # the documented chunk rule and bound


@pytest.fixture(scope="module")
def L(product):
    L = product.lib()
    assert hasattr(L, "zxc_mi355x_dict_prepare_device"), "libzxc_mi355x.so does not export zxc_mi355x_dict_prepare_device"
    return L


def _copts(level=3, block_size=65536, seekable=False, checksum=False, host_dict=False):
    o = _CompressOpts(level=level, block_size=block_size, seekable=int(seekable), checksum_enabled=int(checksum))
    if host_dict:
        o.dict, o.dict_size = FAKE_SRC, 100
    return o


def _dopts(host_dict=False):
    o = _DecompressOpts()
    if host_dict:
        o.dict, o.dict_size = FAKE_SRC, 100
    return o


def test_symbols_and_names_exported(product):
    L = product.lib()
    for sym in ("zxc_mi355x_dict_prepare_device", "zxc_mi355x_compress_dict_device", "zxc_mi355x_compress_dict_device_work_size",
                "zxc_mi355x_decompress_dict_device", "zxc_mi355x_decompress_ranges_dict_device"):
        assert hasattr(L, sym), sym
    for name in ("dict_prepare_device", "compress_dict_device", "compress_dict_device_work_size", "decompress_dict_device",
                 "decompress_ranges_dict_device"):
        assert hasattr(product, name) and hasattr(product.api, name), name
    assert C.sizeof(_DevDict) == 32  # three pointers and a uint32_t, padded


# ---------------------------------------------------------------- dict_prepare_device
def _prep(L, content=FAKE_DICT, size=1000, huf=FAKE_HUF, id_=FAKE_ID):
    return L.zxc_mi355x_dict_prepare_device(content, size, huf, id_, None)


def test_prepare_synchronous_errors_and_their_order(product, L):
    assert _prep(L, content=None) == ERR["NULL_INPUT"]
    assert _prep(L, id_=None) == ERR["NULL_INPUT"]
    assert _prep(L, size=0) == ERR["NULL_INPUT"]
    for big in (65536, 1 << 20, (1 << 32) - 1):
        assert _prep(L, size=big) == ERR["DICT_TOO_LARGE"], big
    # each call breaks one rule and every later one; the earliest is reported
    assert _prep(L, content=None, size=1 << 20) == ERR["NULL_INPUT"]
    assert _prep(L, id_=None, size=0) == ERR["NULL_INPUT"]
    if product.lib().zxc_mi355x_device_count() == 0:
        assert _prep(L) == ERR["GPU_UNAVAILABLE"]
        assert _prep(L, size=65535, huf=None) == ERR["GPU_UNAVAILABLE"]
        with pytest.raises(product.ZxcError) as e:
            product.dict_prepare_device(FAKE_DICT, 10, 0, FAKE_ID)
        assert e.value.code == ERR["GPU_UNAVAILABLE"]
    with pytest.raises(product.ZxcError) as e:
        product.dict_prepare_device(FAKE_DICT, 65536, 0, FAKE_ID)
    assert e.value.code == ERR["DICT_TOO_LARGE"]


# ---------------------------------------------------------------- compress_dict_device
def _cws(L, n, o, dict_size):
    return int(L.zxc_mi355x_compress_dict_device_work_size(n, _ref(o), dict_size))


def _cws0(L, n, o):
    return int(L.zxc_mi355x_compress_device_work_size(n, _ref(o)))


def _comp(L, n=100000, cap=1 << 20, o=None, d=None, src=FAKE_SRC, dst=FAKE_DST, work=FAKE_WORK, ws=None, res=FAKE_RES):
    ws = max(_cws(L, n, o, d.size if d is not None and d.size <= 65535 else 0), 1) if ws is None else ws
    return L.zxc_mi355x_compress_dict_device(src, n, dst, cap, _ref(o), _ref(d), work, ws, res, None)


def test_compress_work_size_bound(L):
    for bs in (4096, 65536, 1 << 19, 1 << 21):
        for seekable, checksum in ((0, 0), (1, 1)):
            o = _copts(block_size=bs, seekable=seekable, checksum=checksum)
            for D in DICT_SIZES:
                chunk = max(IMAGE_MIN_BLOCKS, IMAGE_BYTES // (bs + D))
                prev = 0
                for n in sorted((0, 1, 31, bs - 1, bs, bs + 1, 5 * bs, 4095 * bs + 7, 4096 * bs, 4097 * bs, 20000 * bs + 3, 1 << 30, 1 << 32)):
                    nb = -(-n // bs)
                    plain, w = _cws0(L, n, o), _cws(L, n, o, D)
                    assert plain > 0 and w >= plain and w >= prev, (bs, D, n, w, plain)
                    assert w <= plain + min(nb, chunk) * (bs + D) + WORK_SLACK, (bs, D, n, w, plain)
                    assert nb == 0 or w >= plain + min(nb, chunk) * (bs + D), (bs, D, n, w, plain)  # the images fit
                    prev = w
            assert _cws(L, 1 << 24, o, 0) == _cws0(L, 1 << 24, o)  # no dictionary: the sibling's size
    # the point of the chunks: 4 KiB blocks under a full dictionary do not cost 17 x the source
    o = _copts(block_size=4096)
    assert _cws(L, 1 << 32, o, 65535) - _cws0(L, 1 << 32, o) <= 4096 * (4096 + 65535) + WORK_SLACK
    assert _cws(L, 1 << 20, None, 100) == _cws(L, 1 << 20, _copts(level=0, block_size=0), 100)  # NULL opts = defaults
    for bad in BAD_BLOCK_SIZES:
        assert _cws(L, 1 << 20, _copts(block_size=bad), 100) == 0, bad
    assert _cws(L, 1 << 20, _copts(host_dict=True), 100) == 0
    assert _cws(L, 1 << 20, _copts(), 65536) == 0


def test_compress_synchronous_errors_and_their_order(product, L):
    o = _copts()
    for k in ("dst", "res", "work", "src"):
        assert _comp(L, o=o, d=_dd(), **{k: None}) == ERR["NULL_INPUT"], k
    assert _comp(L, o=_copts(host_dict=True), d=_dd(), ws=1 << 30) == ERR["GPU_UNSUPPORTED"]
    for bad in BAD_BLOCK_SIZES:
        assert _comp(L, o=_copts(block_size=bad), d=_dd(), ws=1 << 30) == ERR["BAD_BLOCK_SIZE"], bad
    for big in (65536, 1 << 24):
        assert _comp(L, o=o, d=_dd(size=big), ws=1 << 40) == ERR["DICT_TOO_LARGE"], big
    assert _comp(L, o=o, d=_dd(content=None)) == ERR["NULL_INPUT"]
    assert _comp(L, o=o, d=_dd(id_=None)) == ERR["NULL_INPUT"]
    for n in (1, 100000, 1 << 24):
        for D in DICT_SIZES:
            assert _comp(L, n=n, cap=1 << 26, o=o, d=_dd(size=D), ws=_cws(L, n, o, D) - 1) == ERR["MEMORY"], (n, D)
    # the sibling's work size is not enough once there is a block and a dictionary
    assert _comp(L, o=o, d=_dd(), ws=_cws0(L, 100000, o)) == ERR["MEMORY"]
    assert _comp(L, n=10 * 65536 + 3, cap=16 + 11 * 8 + 8 + 12 - 1, o=o, d=_dd()) == ERR["DST_TOO_SMALL"]
    # each call breaks one rule and every later one; the earliest is reported
    assert _comp(L, dst=None, o=_copts(host_dict=True, block_size=5000), d=_dd(size=1 << 20, content=None), ws=0, cap=0) == ERR["NULL_INPUT"]
    assert _comp(L, o=_copts(host_dict=True, block_size=5000), d=_dd(size=1 << 20, content=None), ws=0, cap=0) == ERR["GPU_UNSUPPORTED"]
    assert _comp(L, o=_copts(block_size=5000), d=_dd(size=1 << 20, content=None), ws=0, cap=0) == ERR["BAD_BLOCK_SIZE"]
    assert _comp(L, o=o, d=_dd(size=1 << 20, content=None), ws=0, cap=0) == ERR["DICT_TOO_LARGE"]
    assert _comp(L, o=o, d=_dd(content=None), ws=0, cap=0) == ERR["NULL_INPUT"]
    assert _comp(L, o=o, d=_dd(), ws=0, cap=0) == ERR["MEMORY"]
    assert _comp(L, o=o, d=_dd(), cap=0) == ERR["DST_TOO_SMALL"]
    if product.lib().zxc_mi355x_device_count() == 0:
        assert _comp(L, o=o, d=_dd()) == ERR["GPU_UNAVAILABLE"]
        assert _comp(L, o=o, d=_dd(huf=None, size=65535), cap=1 << 21, ws=1 << 40) == ERR["GPU_UNAVAILABLE"]


def test_compress_null_dictionary_is_the_sibling(product, L):
    """no dictionary, or an empty one whose pointers are then not looked at: work size and every verdict of compress_device"""
    for d in (None, _dd(size=0, content=None, id_=None)):
        for n, o in ((0, None), (100000, _copts(seekable=True, checksum=True)), (1 << 24, _copts(block_size=4096))):
            ws = _cws0(L, n, o)
            assert _cws(L, n, o, 0) == ws
            want = L.zxc_mi355x_compress_device(FAKE_SRC, n, FAKE_DST, 1 << 26, _ref(o), FAKE_WORK, ws - 1, FAKE_RES, None)
            assert want == ERR["MEMORY"] and _comp(L, n=n, cap=1 << 26, o=o, d=d, ws=ws - 1) == want
            assert _comp(L, n=n, cap=0, o=o, d=d, ws=ws) == ERR["DST_TOO_SMALL"]
            if product.lib().zxc_mi355x_device_count() == 0:
                assert _comp(L, n=n, cap=1 << 26, o=o, d=d, ws=ws) == ERR["GPU_UNAVAILABLE"]
        assert _comp(L, o=_copts(host_dict=True), d=d, ws=1 << 30) == ERR["GPU_UNSUPPORTED"]


# ---------------------------------------------------------------- decompress_dict_device
def _dws(L, n, cap, bs):
    return int(L.zxc_mi355x_decompress_device_work_size(n, cap, bs))


def _dec(L, n=1000, cap=1 << 20, bs=65536, o=None, d=None, src=FAKE_SRC, dst=FAKE_DST, work=FAKE_WORK, ws=None, res=FAKE_RES):
    ws = max(_dws(L, n, cap, bs), 1) if ws is None else ws
    return L.zxc_mi355x_decompress_dict_device(src, n, dst, cap, bs, _ref(o), _ref(d), work, ws, res, None)


def test_decompress_synchronous_errors_and_their_order(product, L):
    for d in (None, _dd()):
        for k in ("src", "work", "res", "dst"):
            assert _dec(L, d=d, **{k: None}) == ERR["NULL_INPUT"], k
        for n in (0, 1, 27):
            assert _dec(L, d=d, n=n) == ERR["SRC_TOO_SMALL"], n
        for bad in (0,) + BAD_BLOCK_SIZES:
            assert _dec(L, d=d, bs=bad, ws=1 << 30) == ERR["BAD_BLOCK_SIZE"], bad
        assert _dec(L, d=d, o=_dopts(host_dict=True)) == ERR["GPU_UNSUPPORTED"]
        for off in (1, 4, 8, 15):
            assert _dec(L, d=d, dst=FAKE_DST + off) == ERR["GPU_UNSUPPORTED"], off
        for n, cap, bs in ((28, 1, 4096), (1000, 1 << 20, 65536), (1 << 24, 1 << 30, 4096)):
            assert _dec(L, d=d, n=n, cap=cap, bs=bs, ws=_dws(L, n, cap, bs) - 1) == ERR["MEMORY"], (n, cap, bs)
    assert _dec(L, d=_dd(size=65536)) == ERR["DICT_TOO_LARGE"]
    assert _dec(L, d=_dd(content=None)) == ERR["NULL_INPUT"]
    assert _dec(L, d=_dd(id_=None)) == ERR["NULL_INPUT"]
    late = dict(dst=FAKE_DST + 1, ws=0)
    assert _dec(L, src=None, n=5, bs=5000, o=_dopts(True), d=_dd(size=1 << 20, id_=None), **late) == ERR["NULL_INPUT"]
    assert _dec(L, n=5, bs=5000, o=_dopts(True), d=_dd(size=1 << 20, id_=None), **late) == ERR["SRC_TOO_SMALL"]
    assert _dec(L, bs=5000, o=_dopts(True), d=_dd(size=1 << 20, id_=None), **late) == ERR["BAD_BLOCK_SIZE"]
    assert _dec(L, o=_dopts(True), d=_dd(size=1 << 20, id_=None), **late) == ERR["GPU_UNSUPPORTED"]  # the host dictionary
    assert _dec(L, d=_dd(size=1 << 20, id_=None), **late) == ERR["DICT_TOO_LARGE"]
    assert _dec(L, d=_dd(id_=None), **late) == ERR["NULL_INPUT"]
    assert _dec(L, d=_dd(), **late) == ERR["GPU_UNSUPPORTED"]  # the alignment
    assert _dec(L, d=_dd(), ws=0) == ERR["MEMORY"]
    if product.lib().zxc_mi355x_device_count() == 0:
        for d in (None, _dd(), _dd(huf=None, size=65535), _dd(size=0, content=None, id_=None)):
            assert _dec(L, d=d) == ERR["GPU_UNAVAILABLE"]


# ---------------------------------------------------------------- decompress_ranges_dict_device
def _rws(L, n, max_len, bs):
    return int(L.zxc_mi355x_decompress_ranges_device_work_size(n, max_len, bs))


def _rng(L, n=8, max_len=100000, bs=65536, cap=1 << 20, d=None, src=FAKE_SRC, idx=FAKE_IDX, rng=FAKE_RNG, dst=FAKE_DST, work=FAKE_WORK,
         ws=None, res=FAKE_RES):
    ws = max(_rws(L, n, max_len, bs), 1) if ws is None else ws
    return L.zxc_mi355x_decompress_ranges_dict_device(src, 1000, idx, rng, n, max_len, dst, cap, bs, _ref(d), work, ws, res, None)


def test_ranges_synchronous_errors_and_their_order(product, L):
    for d in (None, _dd()):
        for k in ("src", "idx", "work", "res", "rng", "dst"):
            assert _rng(L, d=d, **{k: None}) == ERR["NULL_INPUT"], k
        for bad in (0,) + BAD_BLOCK_SIZES:
            assert _rng(L, d=d, bs=bad, ws=1 << 40) == ERR["BAD_BLOCK_SIZE"], bad
        for off in (1, 4, 8, 15):
            assert _rng(L, d=d, dst=FAKE_DST + off) == ERR["GPU_UNSUPPORTED"], off
        assert _rng(L, d=d, n=1 << 20, max_len=1 << 30, bs=4096, ws=1 << 62) == ERR["MEMORY"]
        for n, ml, bs in ((1, 1, 4096), (8, 100000, 65536), (20000, 3 << 16, 65536)):
            assert _rng(L, d=d, n=n, max_len=ml, bs=bs, ws=_rws(L, n, ml, bs) - 1) == ERR["MEMORY"], (n, ml, bs)
        assert _rng(L, d=d, n=0, rng=None) == 0
        assert _rng(L, d=d, n=0, work=None) == ERR["NULL_INPUT"]
    assert _rng(L, d=_dd(size=65536)) == ERR["DICT_TOO_LARGE"]
    assert _rng(L, d=_dd(content=None)) == ERR["NULL_INPUT"]
    assert _rng(L, d=_dd(id_=None)) == ERR["NULL_INPUT"]
    assert _rng(L, src=None, bs=5000, d=_dd(size=1 << 20), dst=FAKE_DST + 1, ws=0) == ERR["NULL_INPUT"]
    assert _rng(L, bs=5000, d=_dd(size=1 << 20), dst=FAKE_DST + 1, ws=0) == ERR["BAD_BLOCK_SIZE"]
    assert _rng(L, d=_dd(size=1 << 20), dst=FAKE_DST + 1, ws=0) == ERR["DICT_TOO_LARGE"]
    assert _rng(L, d=_dd(id_=None), dst=FAKE_DST + 1, ws=0) == ERR["NULL_INPUT"]
    assert _rng(L, d=_dd(), dst=FAKE_DST + 1, ws=0) == ERR["GPU_UNSUPPORTED"]
    assert _rng(L, d=_dd(), ws=0) == ERR["MEMORY"]
    if product.lib().zxc_mi355x_device_count() == 0:
        for d in (None, _dd(), _dd(huf=None), _dd(size=0, content=None, id_=None)):
            assert _rng(L, d=d) == ERR["GPU_UNAVAILABLE"]


def test_python_bindings_raise(product):
    dd = (FAKE_DICT, 100, 0, FAKE_ID)
    with pytest.raises(product.ZxcError) as e:
        product.compress_dict_device(FAKE_SRC, 100000, FAKE_DST, 1 << 20, dd, FAKE_WORK, 1, FAKE_RES)
    assert e.value.code == ERR["MEMORY"]
    with pytest.raises(product.ZxcError) as e:
        product.compress_dict_device(FAKE_SRC, 100000, FAKE_DST, 1 << 20, (FAKE_DICT, 70000, 0, FAKE_ID), FAKE_WORK, 1 << 40, FAKE_RES)
    assert e.value.code == ERR["DICT_TOO_LARGE"]
    with pytest.raises(product.ZxcError) as e:
        product.decompress_dict_device(FAKE_SRC, 1000, FAKE_DST, 1 << 20, 65536, (0, 100, 0, FAKE_ID), FAKE_WORK, 1 << 30, FAKE_RES)
    assert e.value.code == ERR["NULL_INPUT"]
    with pytest.raises(product.ZxcError) as e:
        product.decompress_ranges_dict_device(FAKE_SRC, 1000, FAKE_IDX, FAKE_RNG, 4, 1000, FAKE_DST, 1 << 20, 4096, dd, FAKE_WORK, 1, FAKE_RES)
    assert e.value.code == ERR["MEMORY"]
    assert product.compress_dict_device_work_size(100000, 0) == product.compress_device_work_size(100000)
    assert product.compress_dict_device_work_size(100000, 100) > product.compress_device_work_size(100000)
    assert product.compress_dict_device_work_size(100000, 100, block_size=5000) == 0


# ---------------------------------------------------------------- the shared rules, run on the CPU
class Ctl(C.Structure):  # zc_ctl_t
    _fields_ = [("head_result", C.c_int64), ("total", C.c_uint64), ("eof_at", C.c_uint64), ("event", C.c_uint64), ("final", C.c_uint32),
                ("file_ck", C.c_uint32), ("verify", C.c_uint32), ("sel", C.c_uint32), ("stored_hash", C.c_uint32), ("nb", C.c_uint32),
                ("seek", C.c_uint32), ("found", C.c_uint32), ("done", C.c_uint32), ("saw_eof", C.c_uint32), ("tail_err", C.c_int32),
                ("ghash", C.c_uint32)]


class Range(C.Structure):  # zxc_dev_range_t
    _fields_ = [("offset", C.c_uint64), ("len", C.c_uint64), ("dst_off", C.c_uint64)]


class Job(C.Structure):  # zxc_dev_job_t
    _fields_ = [("comp_off", C.c_uint64), ("out_off", C.c_uint64), ("comp_size", C.c_uint32), ("out_len", C.c_uint32)]


class Copy(C.Structure):  # zr_copy_t
    _fields_ = [("dst_at", C.c_uint64), ("from_", C.c_uint32), ("n", C.c_uint32)]


@pytest.fixture(scope="module")
def cshim(tmp_path_factory):
    S = build_shim(tmp_path_factory, "container_dict", "container/container_dict_shim.c")
    S.t_ctl_size.restype = C.c_size_t
    assert S.t_ctl_size() == C.sizeof(Ctl)
    S.t_head_dict.restype = None
    S.t_head_dict.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(Ctl), C.c_int, C.c_uint32]
    S.t_head.restype = None
    S.t_head.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(Ctl)]
    S.t_hdr_hash16.restype = C.c_uint16
    S.t_hdr_hash16.argtypes = [C.c_uint64, C.c_uint64]
    return S


@pytest.fixture(scope="module")
def rshim(tmp_path_factory):
    S = build_shim(tmp_path_factory, "ranges_dict", "ranges/ranges_dict_shim.c")
    S.t_index_size.restype = C.c_uint64
    S.t_index_size.argtypes = [C.c_uint32]
    S.t_open.restype = None
    S.t_open.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
    job_args = [C.c_void_p, C.POINTER(Range), C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64]
    S.t_job.restype = None
    S.t_job.argtypes = job_args + [C.POINTER(Job), C.POINTER(Copy)]
    S.t_job_dict.restype = None
    S.t_job_dict.argtypes = job_args + [C.c_int, C.c_uint32, C.POINTER(Job), C.POINTER(Copy)]
    ver_args = [C.c_void_p, C.POINTER(Range), C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32]
    S.t_verdict.restype = C.c_int64
    S.t_verdict.argtypes = ver_args
    S.t_verdict_dict.restype = C.c_int64
    S.t_verdict_dict.argtypes = ver_args + [C.c_int, C.c_uint32]
    return S


# (archive, the dictionary it was written with or None for an id nobody has)
DICT_GOLDEN = (("conformance/valid/dict_http.zxc", "conformance/valid/dict_http.zxd"),
               ("conformance/valid/dict_seekable_l7.zxc", "conformance/valid/dict_text.zxd"),
               ("conformance/invalid/dict_required.zxc", None))
PLAIN_GOLDEN = ("conformance/valid/seekable_4blocks.zxc", "conformance/valid/text_1k.zxc", "conformance/valid/seekable_checksum.zxc")


def _read(rel):
    return open(os.path.join(GOLDEN, rel), "rb").read()


def _hdr_id(comp):
    return int.from_bytes(comp[7:11], "little") if comp[6] & 0x40 else 0


def _head(S, comp, have=None, cap=1 << 20, verify=0):
    """have: None = the head of the call without a dictionary, else (have_dict, id). -> a copy of the control word's fields"""
    c = Ctl()
    C.memset(C.byref(c), 0xEE, C.sizeof(c))
    bs = 1 << comp[5]
    n_jobs = -(-cap // bs) + 1
    if have is None:
        S.t_head(comp, len(comp), cap, bs, verify, n_jobs, C.byref(c))
    else:
        S.t_head_dict(comp, len(comp), cap, bs, verify, n_jobs, C.byref(c), have[0], have[1])
    return bytes(c), c


@pytest.mark.parametrize("arc,zxd", DICT_GOLDEN)
def test_head_rule_on_dictionary_archives(product, cshim, arc, zxd):
    comp = _read(arc)
    hid = _hdr_id(comp)
    assert hid != 0
    if zxd is not None:  # the id the reference wrote into the .zxd is the one in the archive's header, and the library's own
        raw = _read(zxd)
        n = raw[6] | (raw[7] << 8)
        assert int.from_bytes(raw[8:12], "little") == hid
        L = product.lib()
        L.zxc_dict_id.restype = C.c_uint32
        L.zxc_dict_id.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p]
        assert L.zxc_dict_id(raw[16:16 + n], n, raw[16 + n:16 + n + 128]) == hid
    for verify in (0, 1):
        raw_old, old = _head(cshim, comp, None, verify=verify)
        assert (old.final, old.head_result) == (1, ERR["DICT_REQUIRED"])                 # the call without a dictionary: as before
        raw_none, none = _head(cshim, comp, (0, 0), verify=verify)
        assert raw_none == raw_old                                                        # zc_head forwards: the same control word
        assert _head(cshim, comp, (0, hid), verify=verify)[0] == raw_old                  # an id without a dictionary is no dictionary
        for wrong in (hid ^ 1, hid ^ 0x80000000, 0, 0xFFFFFFFF):
            _, bad = _head(cshim, comp, (1, wrong), verify=verify)
            assert (bad.final, bad.head_result) == (1, ERR["DICT_MISMATCH"]), hex(wrong)
            assert (bad.found, bad.seek, bad.nb) == (0, 0, 0)                              # nothing planned: no block is decoded
        _, ok = _head(cshim, comp, (1, hid), verify=verify)
        assert (ok.final, ok.head_result) == (0, 0)
        assert ok.total == int.from_bytes(comp[-12:-4], "little") and ok.nb == -(-ok.total // (1 << comp[5]))
    # the errors in front of the dictionary rule stay in front of it: a block size other than the header's, a broken header
    c = Ctl()
    other = 4096 if (1 << comp[5]) != 4096 else 8192
    cshim.t_head_dict(comp, len(comp), 1 << 20, other, 0, 300, C.byref(c), 1, hid ^ 1)
    assert (c.final, c.head_result) == (1, ERR["BAD_BLOCK_SIZE"])
    broken = bytearray(comp)
    broken[8] ^= 0x10   # the id is under the header's check bytes
    cshim.t_head_dict(bytes(broken), len(broken), 1 << 20, 1 << comp[5], 0, 300, C.byref(c), 1, hid)
    assert (c.final, c.head_result) == (1, -6)  # BAD_HEADER
    # the empty-frame probe answers before the header is read, with or without a dictionary
    cshim.t_head_dict(comp, len(comp), 0, 1 << comp[5], 0, 1, C.byref(c), 1, hid ^ 1)
    assert (c.final, c.head_result) == (1, ERR["DST_TOO_SMALL"])


@pytest.mark.parametrize("arc", PLAIN_GOLDEN)
def test_head_rule_on_archives_without_an_id(cshim, arc):
    """a dictionary given for an archive written without one changes nothing in the head stage"""
    comp = _read(arc)
    assert _hdr_id(comp) == 0
    for verify in (0, 1):
        raw_old, old = _head(cshim, comp, None, verify=verify)
        assert old.final == 0
        for have in ((0, 0), (1, 0), (1, 0x12345678)):
            assert _head(cshim, comp, have, verify=verify)[0] == raw_old, have


def test_header_check_bytes_over_a_dictionary_header(cshim):
    """what the finish pass of compress_dict_device assembles: flag 0x40, the id in bytes 7..10, the check over the two words"""
    for arc, _ in DICT_GOLDEN:
        comp = _read(arc)
        hid = _hdr_id(comp)
        hdr = bytearray(16)
        hdr[0:4] = comp[0:4]
        hdr[4], hdr[5], hdr[6] = 8, comp[5], comp[6] & 0x80
        lo, hi = int.from_bytes(hdr[:8], "little"), 0
        lo = (lo & 0x0000FFFFFFFFFFFF) | ((((lo >> 48) & 0xFF) | 0x40) << 48) | ((hid & 0xFF) << 56)
        hi = hid >> 8
        hi |= cshim.t_hdr_hash16(lo, hi) << 48
        assert lo.to_bytes(8, "little") + hi.to_bytes(8, "little") == comp[:16], arc


def _open(S, comp):
    bs = 1 << comp[5]
    total = int.from_bytes(comp[-12:-4], "little")
    mb = -(-total // bs)
    buf = (C.c_uint8 * int(S.t_index_size(mb)))()
    S.t_open(comp, len(comp), bs, mb, buf)
    status = int.from_bytes(bytes(buf[0:4]), "little", signed=True)
    return buf, status, bs, total, int.from_bytes(bytes(buf[20:24]), "little")


def _range_answers(S, comp, buf, bs, rg, have, max_len=1 << 20, cap=1 << 20):
    """-> (verdict with every covered block decoded in full, [(comp_off, comp_size)] of the non-empty jobs)"""
    J = (max_len - 1) // bs + 2
    status = (C.c_int32 * J)(*([bs] * J))
    jobs = []
    for j in range(J):
        job, cp = Job(), Copy()
        if have is None:
            S.t_job(buf, C.byref(rg), j, j, len(comp), max_len, cap, bs, 1 << 40, 0, C.byref(job), C.byref(cp))
        else:
            S.t_job_dict(buf, C.byref(rg), j, j, len(comp), max_len, cap, bs, 1 << 40, 0, have[0], have[1], C.byref(job), C.byref(cp))
        if job.comp_size:
            jobs.append((job.comp_off, job.comp_size))
        else:
            assert cp.n == 0
    if have is None:
        v = S.t_verdict(buf, C.byref(rg), J, status, len(comp), max_len, cap, bs)
    else:
        v = S.t_verdict_dict(buf, C.byref(rg), J, status, len(comp), max_len, cap, bs, have[0], have[1])
    return int(v), jobs


def test_range_rule_on_the_seekable_dictionary_archive(product, rshim):
    comp = _read("conformance/valid/dict_seekable_l7.zxc")
    hid = _hdr_id(comp)
    buf, status, bs, total, ix_id = _open(rshim, comp)
    assert status == 0 and ix_id == hid and total == 1024  # the index stores the header's id; open itself asks for no dictionary
    s = product.Seekable(comp)
    plan = [(int(a), int(b)) for a, b in zip(s.plan()["comp_off"], s.plan()["comp_size"])]
    s.close()
    for a, n in ((0, total), (0, 1), (total - 1, 1), (100, 300)):
        rg = Range(a, n, a & 15)
        old = _range_answers(rshim, comp, buf, bs, rg, None)
        assert old == (ERR["DICT_REQUIRED"], [])                                   # the call without a dictionary: as before
        assert _range_answers(rshim, comp, buf, bs, rg, (0, 0)) == old
        assert _range_answers(rshim, comp, buf, bs, rg, (0, hid)) == old
        for wrong in (hid ^ 1, 0, 0xFFFFFFFF):
            assert _range_answers(rshim, comp, buf, bs, rg, (1, wrong)) == (ERR["DICT_MISMATCH"], []), hex(wrong)  # every job empty
        assert _range_answers(rshim, comp, buf, bs, rg, (1, hid)) == (n, plan[a // bs: (a + n - 1) // bs + 1])
    # what is decided in front of the dictionary rule stays in front of it
    assert _range_answers(rshim, comp, buf, bs, Range(0, 0, 0), (1, hid ^ 1)) == (0, [])
    assert _range_answers(rshim, comp, buf, bs, Range(total, 1, 0), (1, hid ^ 1)) == (ERR["SRC_TOO_SMALL"], [])
    assert _range_answers(rshim, comp, buf, bs, Range(0, 10, (1 << 20) - 5), (1, hid ^ 1)) == (ERR["DST_TOO_SMALL"], [])


def test_range_rule_on_archives_that_do_not_open_or_have_no_id(rshim):
    for arc in ("conformance/valid/dict_http.zxc", "conformance/invalid/dict_required.zxc"):  # not seekable: the index's own status
        comp = _read(arc)
        buf, status, bs, total, _ = _open(rshim, comp)
        assert status < 0
        rg = Range(0, 1, 0)
        for have in (None, (0, 0), (1, _hdr_id(comp)), (1, 1)):
            assert _range_answers(rshim, comp, buf, bs, rg, have) == (status, []), (arc, have)
    comp = _read("conformance/valid/seekable_4blocks.zxc")
    buf, status, bs, total, ix_id = _open(rshim, comp)
    assert status == 0 and ix_id == 0
    for a, n in ((0, total), (bs - 3, 6), (5, 1)):
        rg = Range(a, n, a & 15)
        old = _range_answers(rshim, comp, buf, bs, rg, None, max_len=total)
        assert old[0] == n and old[1]
        for have in ((0, 0), (1, 0), (1, 0xABCDEF01)):  # a dictionary given for an archive written without one: decoded all the same
            assert _range_answers(rshim, comp, buf, bs, rg, have, max_len=total) == old, have
