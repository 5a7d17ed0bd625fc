"""The append session with a dictionary in device memory (zxc_mi355x_compress_begin_dict_device) without a GPU: the two symbols and
the Python names, every synchronous argument check of begin in its stated order (the device pointers below are never
dereferenced), the work-size arithmetic against the bound the header states, and the rules the entry points and kernels run
(the images-mode plan, the two-segment job, the shape with its image area, the finish with the dictionary flag and id, all in
zxc_amd/csrc/zxc_append.h), compiled here with the host C compiler. Archives whose header carries a dictionary id are cut into
their blocks (the slots and sizes an encode launch leaves) and put together again by a session replayed on the host
(tests/append/append_dict_replay.h) at every byte boundary of the first block and at random cuts: the output must be the archive
byte for byte, bytes 6..15 of the file header included, with a pattern intact everywhere else. The same replay runs under
AddressSanitizer and UBSan in a stand-alone program."""
import ctypes as C
import os

import pytest

import cshim
from conftest import GOLDEN, load_dict
from cshim import opts as _opts, ref as _ref
from devtest import ERR
from zxc_amd.api import _DevCappend as Cs, _DevDict  # zxc_dev_cappend_t, zxc_dev_dict_t

FAKE_SRC, FAKE_DST, FAKE_WORK, FAKE_DICT, FAKE_ID, FAKE_HUF = 0x10000, 0x30000, 0x40000, 0x60000, 0x70000, 0x80000
BLOCK_SIZES = (4096, 65536, 1 << 19, 1 << 21)
DICT_SIZES = (0, 1, 4097, 65535)
JOB_BYTES, TILE_BYTES, AREAS, PAD, WORK_FIXED, IMAGE_FIXED = 28, 16, 3, 64, 4096, 320
# the stated bound: J (S + 28) + 16 ceil(J / 1024) + 3 (bs + 64) + 4 NB (seekable) + 4096 + min(J, C) (bs + D) + 320
DICTS = (("dict_http.zxc", "dict_http.expected", "dict_http.zxd"), ("dict_seekable_l7.zxc", "dict_seekable_l7.expected", "dict_text.zxd"))
NO_UNUSED = ["-Wno-unused-function"]  # (the replay headers the C sources include serve other programs too)


def _host_dict_opts(**kw):
    return cshim.host_dict(_opts(**kw))


def _dict(size=100, content=FAKE_DICT, huf=None, did=FAKE_ID):
    return _DevDict(content, huf, did, size)


@pytest.fixture(scope="module")
def L(product):
    L = product.lib()
    assert hasattr(L, "zxc_mi355x_compress_begin_dict_device"), "libzxc_mi355x.so does not export zxc_mi355x_compress_begin_dict_device"
    assert C.sizeof(_DevDict) == 32
    return L


def _ws(L, max_total, max_piece, o, dict_size):
    return int(L.zxc_mi355x_compress_append_dict_device_work_size(max_total, max_piece, _ref(o), dict_size))


def _ws_plain(L, max_total, max_piece, o):
    return int(L.zxc_mi355x_compress_append_device_work_size(max_total, max_piece, _ref(o)))


def _begin(L, cs="new", dst=FAKE_DST, cap=1 << 20, max_total=1 << 24, max_piece=1 << 20, o="default", d="default", work=FAKE_WORK, ws=None):
    o = _opts() if isinstance(o, str) else o
    d = _dict() if isinstance(d, str) else d
    cs = Cs() if isinstance(cs, str) else cs
    if ws is None:
        ws = max(_ws(L, max_total, max_piece, o, d.size if d is not None and d.size <= 65535 else 0), 1)
    return L.zxc_mi355x_compress_begin_dict_device(_ref(cs), dst, cap, max_total, max_piece, _ref(o), _ref(d), work, ws, None)


def _begin_plain(L, dst=FAKE_DST, cap=1 << 20, max_total=1 << 24, max_piece=1 << 20, o="default", work=FAKE_WORK, ws=None):
    o = _opts() if isinstance(o, str) else o
    if ws is None:
        ws = max(_ws_plain(L, max_total, max_piece, o), 1)
    return L.zxc_mi355x_compress_begin_device(_ref(Cs()), dst, cap, max_total, max_piece, _ref(o), work, ws, None)


def test_symbols_and_names_exported(product):
    L = product.lib()
    for sym in ("zxc_mi355x_compress_append_dict_device_work_size", "zxc_mi355x_compress_begin_dict_device"):
        assert hasattr(L, sym), sym
    for name in ("compress_append_dict_device_work_size", "compress_begin_dict_device"):
        assert hasattr(product, name) and hasattr(product.api, name), name


def test_begin_each_synchronous_error_and_their_order(L):
    for k in ("cs", "dst", "work"):
        assert _begin(L, **{k: None}) == ERR["NULL_INPUT"], k
    assert _begin(L, o=_host_dict_opts(), ws=1 << 40) == ERR["GPU_UNSUPPORTED"]  # a host dictionary has no meaning here
    # the two added errors, directly behind the opts->dict check
    assert _begin(L, d=_dict(65536), ws=1 << 40) == ERR["DICT_TOO_LARGE"]
    assert _begin(L, d=_dict((1 << 32) - 1), ws=1 << 40) == ERR["DICT_TOO_LARGE"]
    assert _begin(L, d=_dict(content=None), ws=1 << 40) == ERR["NULL_INPUT"]
    assert _begin(L, d=_dict(did=None), ws=1 << 40) == ERR["NULL_INPUT"]
    assert _begin(L, d=_dict(65536, content=None, did=None), ws=1 << 40) == ERR["DICT_TOO_LARGE"]  # the size is looked at first
    # then the sibling's, in its order
    for bad in (1000, 2048, 4095, 5000, 3 << 12, 1 << 22):
        assert _begin(L, o=_opts(block_size=bad), ws=1 << 40) == ERR["BAD_BLOCK_SIZE"], bad
    assert _begin(L, max_piece=65535, ws=1 << 40) == ERR["BAD_BLOCK_SIZE"]
    o4 = _opts(block_size=4096)
    assert _begin(L, o=o4, max_total=((1 << 31) - 1) * 4096 + 1, ws=1 << 62) == ERR["BAD_BLOCK_SIZE"]
    assert _begin(L, o=o4, max_piece=1 << 63, ws=1 << 62) == ERR["BAD_BLOCK_SIZE"]
    for size in (1, 100, 65535):
        w = _ws(L, 1 << 24, 1 << 20, _opts(), size)
        assert _begin(L, d=_dict(size), ws=w - 1) == ERR["MEMORY"], size
        assert _begin(L, d=_dict(size), ws=_ws_plain(L, 1 << 24, 1 << 20, _opts())) == ERR["MEMORY"], size  # the sibling's size does not do
    assert _begin(L, cap=35) == ERR["DST_TOO_SMALL"]  # the empty archive: 16 + 8 + 12
    # each call breaks one rule and every later one; the earliest is reported
    bad_bs = _opts(block_size=5000)
    assert _begin(L, dst=None, o=_host_dict_opts(block_size=5000), d=_dict(65536), max_piece=1, ws=0, cap=0) == ERR["NULL_INPUT"]
    assert _begin(L, o=_host_dict_opts(block_size=5000), d=_dict(65536), max_piece=1, ws=0, cap=0) == ERR["GPU_UNSUPPORTED"]
    assert _begin(L, o=_host_dict_opts(), d=_dict(content=None), max_piece=1, ws=0, cap=0) == ERR["GPU_UNSUPPORTED"]
    assert _begin(L, o=bad_bs, d=_dict(65536, content=None), max_piece=1, ws=0, cap=0) == ERR["DICT_TOO_LARGE"]
    assert _begin(L, o=bad_bs, d=_dict(content=None), max_piece=1, ws=0, cap=0) == ERR["NULL_INPUT"]
    assert _begin(L, o=bad_bs, max_piece=1, ws=0, cap=0) == ERR["BAD_BLOCK_SIZE"]
    assert _begin(L, max_piece=1, ws=0, cap=0) == ERR["BAD_BLOCK_SIZE"]
    assert _begin(L, ws=0, cap=0) == ERR["MEMORY"]
    assert _begin(L, cap=0) == ERR["DST_TOO_SMALL"]
    # a refused begin leaves the struct alone, whichever check refuses
    for kw in (dict(d=_dict(65536)), dict(d=_dict(did=None)), dict(o=_host_dict_opts()), dict(max_piece=1), dict(ws=1), dict(cap=0)):
        cs = Cs()
        C.memset(C.byref(cs), 0xEE, C.sizeof(cs))
        assert _begin(L, cs=cs, **kw) < 0 and all(w == 0xEEEEEEEEEEEEEEEE for w in cs.opaque), kw


def test_no_dictionary_gives_the_siblings_answers(L):
    """dict == NULL and size == 0 (whatever the pointers): the sibling's answer for the same arguments, its work size included"""
    for d in (None, _dict(0), _dict(0, content=None, did=None)):
        for kw in (dict(dst=None), dict(o=_host_dict_opts()), dict(o=_opts(block_size=5000)), dict(max_piece=1), dict(ws=1), dict(cap=35), dict(),
                   dict(ws=_ws_plain(L, 1 << 24, 1 << 20, _opts())), dict(ws=_ws_plain(L, 1 << 24, 1 << 20, _opts()) - 1)):
            assert _begin(L, d=d, **kw) == _begin_plain(L, **kw), kw
    # plain begin is as it was: a host dictionary is still refused there
    assert _begin_plain(L, o=_host_dict_opts()) == ERR["GPU_UNSUPPORTED"]


def test_valid_arguments_without_a_device(product, L):
    """What remains after the argument checks is the device check. Only on a machine without a device is the call made (elsewhere
    these pointers would reach a kernel)."""
    if product.lib().zxc_mi355x_device_count() == 0:
        cs = Cs()
        assert _begin(L, cs=cs) == ERR["GPU_UNAVAILABLE"] and not any(cs.opaque)
        assert _begin(L, d=_dict(65535, huf=FAKE_HUF), o=_opts(level=7, block_size=4096, seekable=True, checksum=True), cap=36) == ERR["GPU_UNAVAILABLE"]
        assert _begin(L, d=None) == ERR["GPU_UNAVAILABLE"]
        with pytest.raises(product.ZxcError) as e:
            product.compress_begin_dict_device(FAKE_DST, 1 << 20, 1 << 24, 1 << 20, (FAKE_DICT, 100, 0, FAKE_ID), FAKE_WORK, 1 << 30, block_size=4096)
        assert e.value.code == ERR["GPU_UNAVAILABLE"]


def test_python_binding_raises(product):
    args = (FAKE_DST, 1 << 20, 1 << 24, 1 << 20)
    with pytest.raises(product.ZxcError) as e:
        product.compress_begin_dict_device(*args, (FAKE_DICT, 65536, 0, FAKE_ID), FAKE_WORK, 1 << 30, block_size=4096)
    assert e.value.code == ERR["DICT_TOO_LARGE"]
    with pytest.raises(product.ZxcError) as e:
        product.compress_begin_dict_device(*args, (FAKE_DICT, 100, 0, 0), FAKE_WORK, 1 << 30, block_size=4096)
    assert e.value.code == ERR["NULL_INPUT"]
    with pytest.raises(product.ZxcError) as e:
        product.compress_begin_dict_device(*args, None, FAKE_WORK, 1, block_size=4096)
    assert e.value.code == ERR["MEMORY"]
    assert product.compress_append_dict_device_work_size(1 << 30, 1 << 20, 65536, block_size=4096) == 0
    assert product.compress_append_dict_device_work_size(1 << 30, 1 << 20, 100, block_size=5000) == 0
    assert product.compress_append_dict_device_work_size(1 << 30, 1 << 20, 0, block_size=4096) == \
        product.compress_append_device_work_size(1 << 30, 1 << 20, block_size=4096) > 0
    assert product.compress_append_dict_device_work_size(1 << 30, 1 << 20, 100, 3, 4096, True, True) > \
        product.compress_append_device_work_size(1 << 30, 1 << 20, 3, 4096, True, True)


# ---------------------------------------------------------------- the shared rules, run on the CPU
class Shape(C.Structure):  # zap_shape_t
    _fields_ = [(n, C.c_uint32) for n in ("J", "n_tiles", "slot_stride", "area")] + \
               [(n, C.c_uint64) for n in ("nb_max", "o_tile_sum", "o_tile_hash", "o_tile_bad", "o_jobs", "o_sizes", "o_offsets")] + \
               [("o_carry", C.c_uint64 * 2)] + [(n, C.c_uint64) for n in ("o_stage", "o_seek", "o_slots", "bytes")]


class ShapeImages(C.Structure):  # zap_shape_images_t
    _fields_ = [("s", Shape), ("chunk_jobs", C.c_uint32), ("image", C.c_uint32), ("o_images", C.c_uint64), ("bytes", C.c_uint64)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    S = cshim.build_shim(tmp_path_factory, "append_dict", "append/append_dict_shim.c", NO_UNUSED)
    S.t_shape_images_size.restype = C.c_size_t
    assert S.t_shape_images_size() == C.sizeof(ShapeImages)
    S.t_shape_images.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(ShapeImages)]
    S.t_work_bound_images.restype = C.c_uint64
    S.t_work_bound_images.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32]
    S.t_image_chunk.restype = C.c_uint64
    S.t_image_chunk.argtypes = [C.c_uint32, C.c_uint32]
    S.t_plan_check_images.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32]
    S.t_plan_images.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32 * 7)]
    S.t_finish_header.argtypes = [C.c_uint32, C.c_int, C.c_uint32, C.c_void_p, C.c_uint64]
    S.t_check_archive.restype = C.c_int64
    S.t_check_archive.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.c_uint32, C.c_int]
    S.t_selftest.restype = C.c_int64
    return S


def test_work_size(L, shim):
    for bs in BLOCK_SIZES:
        S = 2 * bs + 512
        for sk in (0, 1):
            o = _opts(block_size=bs, seekable=sk)
            for mp in (bs, 3 * bs + 5, 17 << 20):
                mt = 1 << 30
                J, NB = mp // bs + 2, -(-mt // bs)
                plain = _ws_plain(L, mt, mp, o)
                prev = 0
                for D in DICT_SIZES:
                    w = _ws(L, mt, mp, o, D)
                    chunk = max(4096, (256 << 20) // (bs + D))
                    assert chunk == int(shim.t_image_chunk(bs, D))
                    n_img = min(J, chunk)
                    bound = J * (S + JOB_BYTES) + TILE_BYTES * -(-J // 1024) + AREAS * (bs + PAD) + (4 * NB if sk else 0) + WORK_FIXED + \
                        (n_img * (bs + D) + IMAGE_FIXED if D else 0)
                    assert bound == int(shim.t_work_bound_images(mt, mp, bs, S, sk, D))
                    assert 0 < w <= bound, (bs, sk, mp, D, w, bound)
                    if D == 0:
                        assert w == plain  # exactly the sibling's
                    else:
                        assert w >= plain + n_img * (bs + D) + PAD, (bs, sk, mp, D)  # at least the sibling's and its images
                    assert w >= prev, (bs, sk, mp, D)  # monotone in dict_size
                    prev = w
                    sh = ShapeImages()
                    assert shim.t_shape_images(mt, mp, bs, S, sk, D, C.byref(sh)) == 0
                    assert sh.bytes == w and sh.s.bytes == plain and sh.image == bs + D and sh.chunk_jobs == (n_img if D else 0)
                    # the image area lies behind the sibling's layout, which is unchanged
                    assert sh.o_images % 256 == 0 and sh.o_images >= sh.s.o_slots + J * S and sh.o_images + 256 == plain
                    assert sh.bytes - 256 - sh.o_images >= (sh.chunk_jobs * sh.image + PAD if D else 0)
                assert _ws(L, mt, mp, o, 65536) == 0 and _ws(L, mt, mp, o, (1 << 32) - 1) == 0
    # 0 for whatever the sibling refuses
    assert _ws(L, 1 << 30, 1 << 22, _opts(block_size=5000), 100) == 0
    assert _ws(L, 1 << 30, 1 << 22, _host_dict_opts(), 100) == 0
    assert _ws(L, 1 << 30, 65535, _opts(), 100) == 0 and _ws(L, 1 << 30, 65536, _opts(), 100) > 0
    assert _ws(L, ((1 << 31) - 1) * 4096 + 1, 4096, _opts(block_size=4096), 100) == 0
    assert _ws(L, 1 << 30, 1 << 20, None, 7) == _ws(L, 1 << 30, 1 << 20, _opts(level=0, block_size=0), 7) == _ws(L, 1 << 30, 1 << 20, _opts(block_size=1 << 19), 7)


def test_the_images_plan_at_4096(shim):
    """every source byte is read by exactly one job segment or by the tail copy, nothing is staged, the carried block's two segments
    sum to the block size, nb and tail are the plain plan's (promise numbers: rpd_plan_check of append_dict_replay.h)"""
    bs = 4096
    for carry in (0, 1, 4095):
        for n in (1, 31, 32, 33, 4095, 4096, 4097, 2 * 4096 + 31, 3 * 4096 + 5):
            assert shim.t_plan_check_images(carry, n, bs) == 0, (carry, n)
            out = (C.c_uint32 * 7)()
            shim.t_plan_images(carry, n, bs, C.byref(out))
            nb, n_direct, n_staged, tail, swap, seg0, seg1 = out
            assert nb == (carry + n) // bs and tail == (carry + n) % bs and n_staged == 0 and swap == (1 if nb else 0)
            if nb:
                assert n_direct == nb - (1 if carry else 0)  # every whole block direct, whatever the over-read
                assert (seg0, seg1) == ((carry, bs - carry) if carry else (bs, 0))
    for bs in (65536, 1 << 21):  # near the over-read limits of the plain plan, where it would stage a block
        for carry in (0, 1, 31, 32, bs - 33, bs - 1):
            for n in (bs - carry, bs - carry + 31, bs - carry + 32, 2 * bs - carry, 2 * bs - carry + 31, 3 * bs + 5):
                assert shim.t_plan_check_images(carry, n, bs) == 0, (bs, carry, n)


def test_the_finished_header_carries_the_flag_and_the_id(shim):
    for bs, ck, did in ((4096, 0, 0x12345678), (1 << 19, 1, 0xFFFFFFFF), (65536, 1, 1)):
        buf = (C.c_uint8 * 64)(*([0xC3] * 64))
        shim.t_finish_header(bs, ck, did, buf, 36)
        raw = bytes(buf)
        assert raw[6] == 0x40 | (0x80 if ck else 0) and int.from_bytes(raw[7:11], "little") == did and raw[5] == bs.bit_length() - 1
        assert raw[36:] == b"\xC3" * 28
    for arc, comp, _, _ in _golden_dicts():  # the 16 bytes the reference wrote, check bytes included
        buf = (C.c_uint8 * 36)()
        shim.t_finish_header(1 << comp[5], comp[6] >> 7, int.from_bytes(comp[7:11], "little"), buf, 36)
        assert bytes(buf)[:16] == comp[:16], arc


def _golden_dicts():
    for arc, exp, zxd in DICTS:
        d = os.path.join(GOLDEN, "conformance", "valid")
        comp, data = open(os.path.join(d, arc), "rb").read(), open(os.path.join(d, exp), "rb").read()
        content, _ = load_dict(os.path.join(d, zxd))
        yield arc, comp, data, content


def test_sessions_put_the_dictionary_goldens_together_again(shim):
    for k, (arc, comp, data, content) in enumerate(_golden_dicts()):
        assert comp[6] & 0x40 and int.from_bytes(comp[7:11], "little") != 0, arc  # the flag and the id the session must reproduce
        rc = int(shim.t_check_archive(comp, len(comp), data, len(data), content, len(content), 5 + k, 1))
        assert rc >= len(data) + 1 + 12, (arc, "append_dict_replay.h line %d" % -rc if rc < 0 else rc)  # every byte boundary, and the random cuts


def test_sessions_put_archives_of_several_blocks_together_again(shim):
    """stored blocks behind a dictionary header: several blocks, the carried block from two places, the hash carried over pieces,
    chunks of two jobs"""
    rc = int(shim.t_selftest())
    assert rc > 1000, "append_dict_replay.h line %d" % -rc if rc < 0 else rc


def test_sessions_put_the_reference_dictionary_archives_together_again(shim, ref):
    """archives the unmodified reference writes with a dictionary, of several blocks of 4 KiB"""
    from oracle_py import CompressOpts
    from zxc_amd import corpus
    content, huf = load_dict(os.path.join(GOLDEN, "conformance", "valid", "dict_text.zxd"))
    text = corpus.synth_text(9 * 4096, seed=23)
    for k, (n, level, sk, ck, with_huf) in enumerate(((3 * 4096 + 5, 3, 1, 1, 0), (8 * 4096 + 100, 1, 0, 0, 1), (4096, 5, 1, 0, 0))):
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
        rc = int(shim.t_check_archive(comp, size, data, n, content, len(content), 40 + k, 0))
        assert rc > 100, (n, "append_dict_replay.h line %d" % -rc if rc < 0 else rc)


def test_rules_under_sanitizers(tmp_path):
    """the stand-alone program tests/append/append_dict_san_main.c (its own main; nothing of it is loaded into this process)"""
    args, want = [], 0  # (a golden's cut sets: 70 at each end of the first block, and the random ones)
    for k, (arc, comp, data, content) in enumerate(_golden_dicts()):
        p = tmp_path / ("dict%d.bin" % k)
        p.write_bytes(content)
        d = os.path.join(GOLDEN, "conformance", "valid")
        args += [os.path.join(d, arc), os.path.join(d, arc.replace(".zxc", ".expected")), str(p)]
        want += 140 + 12
    r = cshim.run_san_program(tmp_path, "append/append_dict_san_main.c", args, NO_UNUSED)
    assert "APPEND DICT OK" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
    assert int(r.stdout.split()[-1]) > want + 1000  # the goldens' cut sets and the program's own
