"""zxc_mi355x_compress_device without a GPU: exported, its work-size arithmetic, and every argument check, which returns
synchronously before any device is touched (the device pointers below are never dereferenced)."""
import ctypes as C

import pytest

from cshim import opts as _opts
from devtest import ERR

FAKE_SRC, FAKE_DST, FAKE_WORK, FAKE_RES = 0x10000, 0x20000, 0x30000, 0x40000


@pytest.fixture(scope="module")
def L(product):
    return product.lib()


def _ws(L, n, o):
    return int(L.zxc_mi355x_compress_device_work_size(n, C.byref(o) if o is not None else None))


def _call(L, n, cap, o, src=FAKE_SRC, dst=FAKE_DST, work=FAKE_WORK, ws=None, res=FAKE_RES):
    ws = _ws(L, n, o) if ws is None else ws
    return L.zxc_mi355x_compress_device(src, n, dst, cap, C.byref(o) if o is not None else None, work, ws, res, None)


def _known(n, bs, seekable, checksum):
    """the part of the archive known before encoding: header, 8 (+4) bytes per block, EOF block, seek table, footer"""
    nb = -(-n // bs)
    return 16 + nb * (8 + 4 * checksum) + 8 + ((8 + 4 * nb) if seekable and nb else 0) + 12


def test_symbols_exported(product):
    L = product.lib()
    assert hasattr(L, "zxc_mi355x_compress_device") and hasattr(L, "zxc_mi355x_compress_device_work_size")
    assert hasattr(product, "compress_device") and hasattr(product, "compress_device_work_size")


def test_work_size_arithmetic(L):
    for bs in (4096, 65536, 1 << 19, 1 << 21):
        for seekable in (0, 1):
            for checksum in (0, 1):
                o = _opts(block_size=bs, seekable=seekable, checksum=checksum)
                prev = 0
                for n in (0, 1, 31, 32, 33, bs - 1, bs, bs + 1, 2 * bs + 31, 5 * bs, 1023 * bs + 7, 1025 * bs, 1 << 32):
                    w = _ws(L, n, o)
                    assert w > 0 and w >= prev, (bs, n, w, prev)
                    prev = w
                # at least one encoder slot per block
                nb = -(-(1 << 30) // bs)
                assert _ws(L, 1 << 30, o) >= nb * product_stride(L, bs)
    assert _ws(L, 1 << 20, None) == _ws(L, 1 << 20, _opts(level=0, block_size=0))  # NULL opts = defaults
    for bad in (1000, 4095, 5000, 3 << 12, 1 << 22):
        assert _ws(L, 1 << 20, _opts(block_size=bad)) == 0, bad
    o = _opts()
    o.dict, o.dict_size = FAKE_SRC, 100
    assert _ws(L, 1 << 20, o) == 0


def product_stride(L, bs):
    return int(L.zxc_mi355x_encode_slot_stride(bs))


def test_null_pointers(L):
    n, o = 100000, _opts()
    cap = 1 << 20
    assert _call(L, n, cap, o, dst=None) == ERR["NULL_INPUT"]
    assert _call(L, n, cap, o, res=None) == ERR["NULL_INPUT"]
    assert _call(L, n, cap, o, work=None) == ERR["NULL_INPUT"]
    assert _call(L, n, cap, o, src=None) == ERR["NULL_INPUT"]


def test_bad_block_size(L):
    for bad in (1000, 4095, 5000, 3 << 12, 1 << 22):
        assert _call(L, 100000, 1 << 20, _opts(block_size=bad), ws=1 << 30) == ERR["BAD_BLOCK_SIZE"], bad


def test_dictionary_is_unsupported(L):
    o = _opts()
    keep = C.create_string_buffer(b"dictionary" * 10)
    o.dict, o.dict_size = C.cast(keep, C.c_void_p), 100
    assert _call(L, 100000, 1 << 20, o, ws=1 << 30) == ERR["GPU_UNSUPPORTED"]


def test_short_work_area(L):
    for n in (0, 1, 100000, 1 << 24):
        o = _opts(seekable=True, checksum=True)
        assert _call(L, n, 1 << 26, o, ws=_ws(L, n, o) - 1) == ERR["MEMORY"], n


@pytest.mark.parametrize("bs,seekable,checksum", [(4096, 0, 0), (4096, 1, 1), (65536, 1, 0), (1 << 21, 0, 1)])
def test_capacity_below_the_known_part(L, bs, seekable, checksum):
    for n in (0, 1, bs, 10 * bs + 3):
        o = _opts(block_size=bs, seekable=seekable, checksum=checksum)
        k = _known(n, bs, seekable, checksum)
        assert _call(L, n, k - 1, o) == ERR["DST_TOO_SMALL"], n
        assert _call(L, n, 0, o) == ERR["DST_TOO_SMALL"], n


def test_valid_arguments_without_a_device(product, L):
    """Options are normalised like zxc_compress (level <= 0 -> 3, above 7 -> 7) and pass validation; what remains is the device
    check. Only on a machine without a device is the call made (elsewhere these pointers would reach a kernel)."""
    for level in (-5, 0, 1, 7, 99):
        o = _opts(level=level, block_size=0)
        assert _ws(L, 1 << 20, o) == _ws(L, 1 << 20, _opts(level=3, block_size=1 << 19))
    if product.lib().zxc_mi355x_device_count() == 0:
        for n, o in ((0, None), (1, _opts()), (100000, _opts(level=99, seekable=True, checksum=True))):
            assert _call(L, n, 1 << 20, o) == ERR["GPU_UNAVAILABLE"], n
        assert _call(L, 0, 36, _opts(seekable=True), src=None) == ERR["GPU_UNAVAILABLE"]  # empty input: NULL d_src is fine


def test_python_binding_raises(product):
    with pytest.raises(product.ZxcError) as e:
        product.compress_device(FAKE_SRC, 100000, FAKE_DST, 1 << 20, FAKE_WORK, 1, FAKE_RES)
    assert e.value.code == ERR["MEMORY"]
    with pytest.raises(product.ZxcError) as e:
        product.compress_device(FAKE_SRC, 100000, 0, 1 << 20, FAKE_WORK, 1 << 30, FAKE_RES)
    assert e.value.code == ERR["NULL_INPUT"]
    assert product.compress_device_work_size(100000, block_size=5000) == 0
    assert product.compress_device_work_size(100000) == product.compress_device_work_size(100000, 3, 1 << 19)
