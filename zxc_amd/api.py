"""ctypes binding of libzxc_mi355x.so — same function names as the reference C API
(include/zxc_buffer.h, include/zxc_seekable.h) plus the device-resident entry points of
include/zxc_mi355x.h."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# zxc_dev_job_t (include/zxc_mi355x.h)
JOB_DTYPE = np.dtype([("comp_off", "<u8"), ("out_off", "<u8"), ("comp_size", "<u4"), ("out_len", "<u4")])
# zxc_dev_range_t (include/zxc_mi355x.h)
RANGE_DTYPE = np.dtype([("offset", "<u8"), ("len", "<u8"), ("dst_off", "<u8")])
# zxc_dev_item_t (include/zxc_mi355x.h)
ITEM_DTYPE = np.dtype([("src_off", "<u8"), ("src_size", "<u8"), ("dst_off", "<u8"), ("dst_capacity", "<u8")])
IOV_DTYPE = np.dtype([("base", "<u8"), ("len", "<u8")])  # zxc_dev_iov_t
# zxc_dev_rangev_t (include/zxc_mi355x_rangesv.h)
RANGEV_DTYPE = np.dtype([("offset", "<u8"), ("len", "<u8"), ("base", "<u8")])


class ZxcError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = int(code)
        super().__init__(f"{what}: {error_name(self.code)} ({self.code})")


class _CompressOpts(C.Structure):  # include/zxc_opts.h
    _fields_ = [("n_threads", C.c_int), ("level", C.c_int), ("block_size", C.c_size_t),
                ("checksum_enabled", C.c_int), ("seekable", C.c_int), ("dict", C.c_void_p),
                ("dict_size", C.c_size_t), ("dict_huf", C.c_void_p), ("progress_cb", C.c_void_p),
                ("user_data", C.c_void_p)]


class _DecompressOpts(C.Structure):  # include/zxc_opts.h
    _fields_ = [("n_threads", C.c_int), ("checksum_enabled", C.c_int), ("dict", C.c_void_p),
                ("dict_size", C.c_size_t), ("dict_huf", C.c_void_p), ("progress_cb", C.c_void_p),
                ("user_data", C.c_void_p)]


_READ_AT = C.CFUNCTYPE(C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64)


class _Reader(C.Structure):  # zxc_reader_t, include/zxc_seekable.h
    _fields_ = [("read_at", _READ_AT), ("ctx", C.c_void_p), ("size", C.c_uint64)]


class _DevDict(C.Structure):  # zxc_dev_dict_t (include/zxc_mi355x.h): a dictionary in device memory
    _fields_ = [("d_content", C.c_void_p), ("d_huf", C.c_void_p), ("d_id", C.c_void_p), ("size", C.c_uint32)]


class _DevCappend(C.Structure):  # zxc_dev_cappend_t: the append session, a host struct of 16 words, caller-owned
    _fields_ = [("opaque", C.c_uint64 * 16)]


class _DevDtake(C.Structure):  # zxc_dev_dtake_t: the take session, a host struct of 16 words, caller-owned
    _fields_ = [("opaque", C.c_uint64 * 16)]


class _InBuf(C.Structure):  # zxc_inbuf_t (include/zxc_pstream.h)
    _fields_ = [("src", C.c_void_p), ("size", C.c_size_t), ("pos", C.c_size_t)]


class _OutBuf(C.Structure):  # zxc_outbuf_t (include/zxc_pstream.h)
    _fields_ = [("dst", C.c_void_p), ("size", C.c_size_t), ("pos", C.c_size_t)]


# ---- every prototype this module binds: C name -> (restype, argtypes). tests/test_api_prototypes.py holds the
# zxc_mi355x_* entries against include/zxc_mi355x.h.
_I, _I64, _U32, _U64, _SZ, _STR, _P = C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_size_t, C.c_char_p, C.c_void_p
_CO, _DO, _DD = C.POINTER(_CompressOpts), C.POINTER(_DecompressOpts), C.POINTER(_DevDict)
_CS, _DS, _IN, _OUT = C.POINTER(_DevCappend), C.POINTER(_DevDtake), C.POINTER(_InBuf), C.POINTER(_OutBuf)
_TAIL = [_P, _U64, _P, _P]  # d_work, work_size, d_result(s), stream
_RANGES = [_P, _U64, _P, _P, _U32, _U64, _P, _U64, _U32]  # d_src .. block_size of decompress_ranges_device
_DBATCH = [_P, _U64, _P, _U32, _U64, _P, _U64, _U32, _DO]  # d_src .. opts of decompress_batch_device
_CBATCH = [_P, _U64, _P, _U32, _U64, _P, _U64, _CO]  # d_src .. opts of compress_batch_device
_CPACK = [_P, _U64, _P, _U32, _U64, _P, _U64, _U32, _CO]  # d_src .. align, opts of compress_pack_device
_PACK_TAIL = [_P, _U64, _P, _P, _P, _P]  # d_work, work_size, d_packed, d_results, d_total, stream
_CBEGIN = [_CS, _P, _U64, _U64, _U64, _CO]  # cs .. opts of compress_begin_device
_DBEGIN = [_DS, _P, _U64, _U64, _U64, _U32, _DO]  # ds .. opts of decompress_begin_device
_IOV = [_P, _U32, _U64, _P, _U64, _P]  # d_iov, n_iov, total, d_scratch, scratch_size, stream

_PROTOTYPES = {
    # include/zxc_buffer.h, include/zxc_error.h
    "zxc_error_name": (_STR, [_I]),
    "zxc_compress_bound": (_U64, [_SZ]),
    "zxc_compress": (_I64, [_STR, _SZ, _P, _SZ, _CO]),
    "zxc_decompress": (_I64, [_STR, _SZ, _P, _SZ, _DO]),
    "zxc_get_decompressed_size": (_U64, [_STR, _SZ]),
    # include/zxc_seekable.h
    "zxc_seekable_open": (_P, [_STR, _SZ]),
    "zxc_seekable_open_reader": (_P, [C.POINTER(_Reader)]),
    "zxc_seekable_free": (None, [_P]),
    "zxc_seekable_get_num_blocks": (_U32, [_P]),
    "zxc_seekable_get_decompressed_size": (_U64, [_P]),
    "zxc_seekable_get_block_comp_size": (_U32, [_P, _U32]),
    "zxc_seekable_get_block_decomp_size": (_U32, [_P, _U32]),
    "zxc_seekable_decompress_range": (_I64, [_P, _P, _SZ, _U64, _SZ]),
    "zxc_seekable_decompress_range_mt": (_I64, [_P, _P, _SZ, _U64, _SZ, _I]),
    "zxc_seekable_set_dict": (_I, [_P, _STR, _SZ, _STR]),
    # include/zxc_mi355x.h: the block-level calls
    "zxc_mi355x_device_count": (_I, []),
    "zxc_mi355x_set_device": (_I, [_I]),
    "zxc_mi355x_plan_seekable": (_I64, [_P, _U32, _U32, _U64, _P]),
    "zxc_mi355x_decode_blocks_device": (_I, [_P, _P, _U32, _P, _P, _U32, _I, _P]),
    "zxc_mi355x_encode_slot_stride": (_U32, [_U32]),
    "zxc_mi355x_encode_blocks_device": (_I, [_P, _U64, _U32, _I, _I, _P, _P, _P]),
    # whole archives, device to device
    "zxc_mi355x_compress_device_work_size": (_U64, [_U64, _CO]),
    "zxc_mi355x_compress_device": (_I, [_P, _U64, _P, _U64, _CO] + _TAIL),
    "zxc_mi355x_decompress_device_work_size": (_U64, [_U64, _U64, _U32]),
    "zxc_mi355x_decompress_device": (_I, [_P, _U64, _P, _U64, _U32, _DO] + _TAIL),
    "zxc_mi355x_frame_info_device": (_I, [_P, _U64, C.POINTER(_U32), C.POINTER(_U64), C.POINTER(_I), _P]),
    # random access
    "zxc_mi355x_seekable_index_size": (_U64, [_U32]),
    "zxc_mi355x_seekable_open_device": (_I, [_P, _U64, _U32, _U32, _P, _U64, _P]),
    "zxc_mi355x_decompress_ranges_device_work_size": (_U64, [_U32, _U64, _U32]),
    "zxc_mi355x_decompress_ranges_device": (_I, _RANGES + _TAIL),
    # with a dictionary in device memory
    "zxc_mi355x_dict_prepare_device": (_I, [_P, _U32, _P, _P, _P]),
    "zxc_mi355x_compress_dict_device_work_size": (_U64, [_U64, _CO, _U32]),
    "zxc_mi355x_compress_dict_device": (_I, [_P, _U64, _P, _U64, _CO, _DD] + _TAIL),
    "zxc_mi355x_decompress_dict_device": (_I, [_P, _U64, _P, _U64, _U32, _DO, _DD] + _TAIL),
    "zxc_mi355x_decompress_ranges_dict_device": (_I, _RANGES + [_DD] + _TAIL),
    # many archives / many buffers per call
    "zxc_mi355x_decompress_batch_device_work_size": (_U64, [_U32, _U64, _U32]),
    "zxc_mi355x_decompress_batch_device": (_I, _DBATCH + _TAIL),
    "zxc_mi355x_decompress_batch_dict_device": (_I, _DBATCH + [_DD] + _TAIL),
    "zxc_mi355x_compress_batch_device_work_size": (_U64, [_U32, _U64, _CO]),
    "zxc_mi355x_compress_batch_dict_device_work_size": (_U64, [_U32, _U64, _CO, _U32]),
    "zxc_mi355x_compress_batch_device": (_I, _CBATCH + _TAIL),
    "zxc_mi355x_compress_batch_dict_device": (_I, _CBATCH + [_DD] + _TAIL),
    "zxc_mi355x_compress_pack_device_work_size": (_U64, [_U32, _U64, _CO]),
    "zxc_mi355x_compress_pack_dict_device_work_size": (_U64, [_U32, _U64, _CO, _U32]),
    "zxc_mi355x_compress_pack_device": (_I, _CPACK + _PACK_TAIL),
    "zxc_mi355x_compress_pack_dict_device": (_I, _CPACK + [_DD] + _PACK_TAIL),
    # one archive from many pieces: the append session
    "zxc_mi355x_compress_append_device_work_size": (_U64, [_U64, _U64, _CO]),
    "zxc_mi355x_compress_append_dict_device_work_size": (_U64, [_U64, _U64, _CO, _U32]),
    "zxc_mi355x_compress_begin_device": (_I, _CBEGIN + [_P, _U64, _P]),
    "zxc_mi355x_compress_begin_dict_device": (_I, _CBEGIN + [_DD, _P, _U64, _P]),
    "zxc_mi355x_compress_append_device": (_I, [_CS, _P, _U64, _P]),
    "zxc_mi355x_compress_end_device": (_I, [_CS, _P, _P]),
    "zxc_mi355x_compress_appendv_device_scratch_size": (_U64, [_U32, _U64, _CO]),
    "zxc_mi355x_compress_appendv_dict_device_scratch_size": (_U64, [_U32, _U64, _CO, _U32]),
    "zxc_mi355x_compress_appendv_device": (_I, [_CS] + _IOV),
    "zxc_mi355x_compress_appendv_dict_device": (_I, [_CS] + _IOV),
    # one archive into many pieces: the take session
    "zxc_mi355x_decompress_take_device_work_size": (_U64, [_U64, _U64, _U64, _U32]),
    "zxc_mi355x_decompress_begin_device": (_I, _DBEGIN + [_P, _U64, _P]),
    "zxc_mi355x_decompress_begin_dict_device": (_I, _DBEGIN + [_DD, _P, _U64, _P]),
    "zxc_mi355x_decompress_take_device": (_I, [_DS, _P, _U64, _P]),
    "zxc_mi355x_decompress_end_device": (_I, [_DS, _P, _P]),
    "zxc_mi355x_decompress_takev_device_scratch_size": (_U64, [_U32, _U64, _U32]),
    "zxc_mi355x_decompress_takev_device": (_I, [_DS] + _IOV),
    # include/zxc_stream.h (FILE* as void*)
    "zxc_stream_compress": (_I64, [_P, _P, _CO]),
    "zxc_stream_decompress": (_I64, [_P, _P, _DO]),
    "zxc_stream_get_decompressed_size": (_I64, [_P]),
    "zxc_seekable_open_file": (_P, [_P]),
    # include/zxc_pstream.h
    "zxc_cstream_create": (_P, [_CO]),
    "zxc_cstream_free": (None, [_P]),
    "zxc_cstream_compress": (_I64, [_P, _OUT, _IN]),
    "zxc_cstream_end": (_I64, [_P, _OUT]),
    "zxc_cstream_in_size": (_SZ, [_P]),
    "zxc_cstream_out_size": (_SZ, [_P]),
    "zxc_dstream_create": (_P, [_DO]),
    "zxc_dstream_free": (None, [_P]),
    "zxc_dstream_decompress": (_I64, [_P, _OUT, _IN]),
    "zxc_dstream_finished": (_I, [_P]),
    "zxc_dstream_in_size": (_SZ, [_P]),
    "zxc_dstream_out_size": (_SZ, [_P]),
}
# include/zxc_mi355x_rangesv.h, a table of its own: tests/test_decompress_rangesv_device_cpu.py holds it against that header
_RANGESV = [_P, _U64, _P, _P, _U32, _U64, _U32]  # d_src .. block_size of decompress_rangesv_device
_PROTOTYPES_RANGESV = {
    "zxc_mi355x_decompress_rangesv_device_work_size": (_U64, [_U32, _U64, _U32]),
    "zxc_mi355x_decompress_rangesv_device": (_I, _RANGESV + _TAIL),
    "zxc_mi355x_decompress_rangesv_dict_device": (_I, _RANGESV + [_DD] + _TAIL),
}
# include/zxc_mi355x_shuffle.h, a table of its own: tests/test_shuffle_device_cpu.py holds it against that header
_SHUFFLE = [_P, _P, _U64, _U32, _U32, _P]  # d_src, d_dst, n, elem_size, unit, stream
_PROTOTYPES_SHUFFLE = {
    "zxc_mi355x_shuffle_device": (_I, _SHUFFLE),
    "zxc_mi355x_unshuffle_device": (_I, _SHUFFLE),
    "zxc_mi355x_compress_shuffle_device_work_size": (_U64, [_U64, _U64, _CO, _U32]),
    "zxc_mi355x_compress_shuffle_device": (_I, [_P, _U64, _U32, _P, _U64, _U64, _CO, _DD] + _TAIL),
    "zxc_mi355x_decompress_shuffle_device_work_size": (_U64, [_U64, _U64, _U64, _U32]),
    "zxc_mi355x_decompress_shuffle_device": (_I, [_P, _U64, _P, _U64, _U32, _U64, _U32, _DO, _DD] + _TAIL),
}
# include/zxc_mi355x_rangesv_shuffle.h, a table of its own: tests/test_decompress_rangesv_shuffle_device_cpu.py holds it against that header
_PROTOTYPES_RANGESV_SHUFFLE = {
    "zxc_mi355x_decompress_rangesv_shuffle_device_work_size": (_U64, [_U32, _U64, _U32]),
    "zxc_mi355x_decompress_rangesv_shuffle_device": (_I, [_P, _U64, _P, _P, _U32, _U64, _U32, _U32, _DD] + _TAIL),
}
# include/zxc_mi355x_shufflev.h, a table of its own: tests/test_compress_shufflev_device_cpu.py holds it against that header
_PROTOTYPES_SHUFFLEV = {
    "zxc_mi355x_shufflev_device_scratch_size": (_U64, [_U32]),
    "zxc_mi355x_shufflev_device": (_I, [_P, _U32, _U64, _P, _U32, _U32, _P, _U64, _P, _P]),
    "zxc_mi355x_compress_shufflev_device_work_size": (_U64, [_U32, _U64, _U64, _CO, _U32]),
    "zxc_mi355x_compress_shufflev_device": (_I, [_P, _U32, _U64, _U32, _P, _U64, _U64, _CO, _DD] + _TAIL),
}
# include/zxc_mi355x_unshufflev.h, a table of its own: tests/test_decompress_shufflev_device_cpu.py holds it against that header
_PROTOTYPES_UNSHUFFLEV = {
    "zxc_mi355x_unshufflev_device_scratch_size": (_U64, [_U32]),
    "zxc_mi355x_unshufflev_device": (_I, [_P, _P, _U32, _U64, _U32, _U32, _P, _U64, _P, _P]),
    "zxc_mi355x_decompress_shufflev_device_work_size": (_U64, [_U32, _U64, _U64, _U64, _U32]),
    "zxc_mi355x_decompress_shufflev_device": (_I, [_P, _U64, _P, _U32, _U64, _U32, _U64, _U32, _DO, _DD] + _TAIL),
}
_TABLES = (_PROTOTYPES, _PROTOTYPES_RANGESV, _PROTOTYPES_SHUFFLE, _PROTOTYPES_RANGESV_SHUFFLE, _PROTOTYPES_SHUFFLEV)
_TABLES_MORE = (_PROTOTYPES_UNSHUFFLEV,)  # the tables behind the first five; _prototype and _bind walk both tuples
_STREAM = ("zxc_stream_compress", "zxc_stream_decompress", "zxc_stream_get_decompressed_size", "zxc_seekable_open_file")
_PSTREAM = tuple(n for n in _PROTOTYPES if n.startswith(("zxc_cstream_", "zxc_dstream_")))


def _prototype(name):
    for table in _TABLES + _TABLES_MORE:
        if name in table:
            return table[name]
    raise KeyError(name)


def _bind(L, names=None):
    """Set restype and argtypes of those of `names` (all tables unless given) that L exports (the reference and the mock-device
    library have no device calls, an experiment build may lack some): a missing symbol fails when it is called, not here. -> L"""
    for name in ([n for table in _TABLES + _TABLES_MORE for n in table] if names is None else names):
        f = getattr(L, name, None)
        if f is not None:
            f.restype, f.argtypes = _prototype(name)
    return L


# The per-call binders of earlier versions keep their names and their contract (a library in, the same library out, bound) for
# callers that hold a library of their own; each applies the whole table.
_bind_decompress_device = _bind_ranges_device = _bind_dict_device = _bind_decompress_batch_device = _bind_compress_batch_device = \
    _bind_compress_pack_device = _bind_compress_append_device = _bind_decompress_take_device = _bind_decompress_takev_device = _bind


def _bind_stream(L):
    return _bind(L, _STREAM)


def _bind_pstream(L):
    return _bind(L, _PSTREAM)


def lib_path():
    # The product library, always — unless a development harness under tools/ asks for an A/B build on purpose: both
    # ZXC_TOOLS_AB=1 and ZXC_LIB_VARIANT=<file> must be set (a stray ZXC_LIB_VARIANT alone is ignored: experiment builds may
    # produce wrong output by design, zxc_amd/csrc/zxc_experiments.h).
    if os.environ.get("ZXC_TOOLS_AB") == "1" and os.environ.get("ZXC_LIB_VARIANT"):
        return os.path.join(_HERE, os.environ["ZXC_LIB_VARIANT"])
    return os.path.join(_HERE, "libzxc_mi355x.so")


def lib():
    """The product library. Fails loudly when it has not been built."""
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise ImportError(f"{p} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _LIB = _bind(C.CDLL(p))
    return _LIB


def _call(name, *args):
    """lib().<name>(*args) by the table: where the prototype says void*, an integer device pointer or stream goes as
    c_void_p (0 stays NULL); a ctypes struct or scalar goes by reference; the rest goes as it is. Raises ZxcError(rc, name) on
    rc < 0."""
    rc = getattr(lib(), name)(*[C.c_void_p(a or None) if t is _P else C.byref(a) if isinstance(a, (C.Structure, C._SimpleCData))
                                else a for t, a in zip(_prototype(name)[1], args)])
    if rc < 0:
        raise ZxcError(rc, name)
    return rc


def error_name(code):
    try:
        return lib().zxc_error_name(int(code)).decode()
    except Exception:  # library missing: still give a readable message
        return f"zxc error {code}"


def get_decompressed_size(comp: bytes) -> int:
    return int(lib().zxc_get_decompressed_size(comp, len(comp)))


def _set_dict(o, dict_, dict_huf):
    """Point an opts struct at a dictionary (content + optional 128-byte shared table); returns the buffers to keep alive."""
    if not dict_:
        return None
    keep = (C.create_string_buffer(dict_, len(dict_)), C.create_string_buffer(dict_huf, 128) if dict_huf else None)
    o.dict = C.cast(keep[0], C.c_void_p)
    o.dict_size = len(dict_)
    o.dict_huf = C.cast(keep[1], C.c_void_p) if dict_huf else None
    return keep


def _host_result(rc, out, what, raise_on_error):
    if rc < 0:
        if raise_on_error:
            raise ZxcError(rc, what)
        return rc, b""
    return out.raw[:rc] if raise_on_error else (rc, out.raw[:rc])


def compress(data: bytes, level=3, block_size=65536, seekable=True, checksum=False, raise_on_error=True, dict_=None,
             dict_huf=None):
    """zxc_compress(): host buffer in, v8 archive out (blocks encoded on the GPU)."""
    o = _CompressOpts(level=level, block_size=block_size, seekable=int(seekable), checksum_enabled=int(checksum))
    _keep = _set_dict(o, dict_, dict_huf)
    cap = int(lib().zxc_compress_bound(len(data)))
    out = C.create_string_buffer(max(cap, 64))
    return _host_result(lib().zxc_compress(data, len(data), out, cap, C.byref(o)), out, "zxc_compress", raise_on_error)


def decompress(comp: bytes, capacity=None, checksum=False, raise_on_error=True, dict_=None, dict_huf=None):
    """zxc_decompress(): whole frame, host buffers in, host buffer out (blocks decode on the GPU)."""
    cap = get_decompressed_size(comp) if capacity is None else int(capacity)
    out = C.create_string_buffer(max(cap, 1))
    o = _DecompressOpts(checksum_enabled=int(checksum))
    _keep = _set_dict(o, dict_, dict_huf)
    rc = lib().zxc_decompress(comp, len(comp), out if cap else None, cap, C.byref(o))
    return _host_result(rc, out, "zxc_decompress", raise_on_error)


class Seekable:
    """zxc_seekable handle (include/zxc_seekable.h). Keeps `comp` alive: the C handle borrows it."""

    def __init__(self, comp: bytes = None, reader=None, size=None):
        """`comp`: the whole archive in memory (zxc_seekable_open). `reader(offset, length) -> bytes` + `size`:
        zxc_seekable_open_reader — only header, seek table and footer are read at open, so an archive whose
        blocks live elsewhere (e.g. each GPU holding its own block range) can still be opened as ONE table."""
        self._comp = comp
        if reader is not None:
            def _cb(_ctx, dst, n, off):
                try:
                    b = reader(int(off), int(n))
                    if b is None or len(b) != n:
                        return -11  # ZXC_ERROR_IO
                    C.memmove(dst, b, n)
                    return n
                except Exception:
                    return -11
            self._cb = _READ_AT(_cb)
            self._rd = _Reader(self._cb, None, int(size))
            self._h = lib().zxc_seekable_open_reader(C.byref(self._rd))
        else:
            self._h = lib().zxc_seekable_open(comp, len(comp))
        if not self._h:
            raise ZxcError(-6, "zxc_seekable_open (not a seekable archive)")

    def close(self):
        if self._h:
            lib().zxc_seekable_free(self._h)
            self._h = None

    __del__ = close

    @property
    def num_blocks(self):
        return int(lib().zxc_seekable_get_num_blocks(self._h))

    @property
    def decompressed_size(self):
        return int(lib().zxc_seekable_get_decompressed_size(self._h))

    def block_comp_size(self, i):
        return int(lib().zxc_seekable_get_block_comp_size(self._h, i))

    def block_decomp_size(self, i):
        return int(lib().zxc_seekable_get_block_decomp_size(self._h, i))

    def set_dict(self, dict_, dict_huf=None):
        return int(lib().zxc_seekable_set_dict(self._h, dict_, len(dict_), dict_huf))

    def decompress_range(self, offset, length, n_threads=None, raise_on_error=True):
        out = C.create_string_buffer(max(length, 1))
        if n_threads is None:
            rc = lib().zxc_seekable_decompress_range(self._h, out, length, offset, length)
        else:
            rc = lib().zxc_seekable_decompress_range_mt(self._h, out, length, offset, length, n_threads)
        return _host_result(rc, out, "zxc_seekable_decompress_range", raise_on_error)

    def plan(self, first=0, count=None, comp_rebase=0):
        """Job table (numpy structured array) for blocks [first, first+count)."""
        count = self.num_blocks - first if count is None else count
        jobs = np.zeros(count, dtype=JOB_DTYPE)
        _call("zxc_mi355x_plan_seekable", self._h, first, count, comp_rebase, jobs.ctypes.data)
        return jobs


def decode_blocks_device(d_comp, d_jobs, n_jobs, d_out, d_status, block_size, verify_trailer=False, stream=0):
    """zxc_mi355x_decode_blocks_device(): raw device pointers (ints), asynchronous on `stream`."""
    _call("zxc_mi355x_decode_blocks_device", d_comp, d_jobs, n_jobs, d_out, d_status, block_size, int(verify_trailer), stream)


def _copts(level, block_size, seekable, checksum):
    return _CompressOpts(level=level, block_size=block_size, seekable=int(seekable), checksum_enabled=int(checksum))


def _dopts(checksum):
    return _DecompressOpts(checksum_enabled=int(checksum))


def _dev_dict(dict_):
    """dict_: None, or (d_content, size, d_huf or 0, d_id), raw device pointers as ints. -> a zxc_dev_dict_t or None"""
    if dict_ is None:
        return None
    d_content, size, d_huf, d_id = dict_
    return _DevDict(d_content or None, d_huf or None, d_id or None, size)


def compress_device_work_size(src_size, level=3, block_size=0, seekable=False, checksum=False):
    """zxc_mi355x_compress_device_work_size(): bytes of device scratch compress_device needs (0 for invalid options)."""
    return int(_call("zxc_mi355x_compress_device_work_size", src_size, _copts(level, block_size, seekable, checksum)))


def compress_device(d_src, src_size, d_dst, dst_capacity, d_work, work_size, d_result, level=3, block_size=0,
                    seekable=False, checksum=False, stream=0):
    """zxc_mi355x_compress_device(): raw device pointers (ints, e.g. tensor.data_ptr()), asynchronous on `stream`
    (e.g. torch.cuda.current_stream().cuda_stream). The archive size or a negative zxc_error_t lands in the int64 at
    d_result; a synchronous failure raises ZxcError."""
    _call("zxc_mi355x_compress_device", d_src, src_size, d_dst, dst_capacity, _copts(level, block_size, seekable, checksum),
          d_work, work_size, d_result, stream)


def decompress_device_work_size(src_size, dst_capacity, block_size):
    """zxc_mi355x_decompress_device_work_size(): bytes of device scratch decompress_device needs (0 for refused arguments)."""
    return int(_call("zxc_mi355x_decompress_device_work_size", src_size, dst_capacity, block_size))


def decompress_device(d_src, src_size, d_dst, dst_capacity, block_size, d_work, work_size, d_result, checksum=False, stream=0):
    """zxc_mi355x_decompress_device(): raw device pointers (ints, e.g. tensor.data_ptr()), asynchronous on `stream`. The
    decoded size or the negative zxc_error_t zxc_decompress would return lands in the int64 at d_result; a synchronous
    failure raises ZxcError."""
    _call("zxc_mi355x_decompress_device", d_src, src_size, d_dst, dst_capacity, block_size, _dopts(checksum), d_work, work_size,
          d_result, stream)


def frame_info_device(d_src, src_size, stream=0):
    """zxc_mi355x_frame_info_device(): -> (block_size, decompressed_size, has_checksum) of an archive in device memory.
    Synchronises `stream`."""
    bs, n, ck = C.c_uint32(0), C.c_uint64(0), C.c_int(0)
    _call("zxc_mi355x_frame_info_device", d_src, src_size, bs, n, ck, stream)
    return int(bs.value), int(n.value), bool(ck.value)


def seekable_index_size(max_blocks):
    """zxc_mi355x_seekable_index_size(): bytes of the device index of an archive of at most max_blocks blocks."""
    return int(_call("zxc_mi355x_seekable_index_size", max_blocks))


def seekable_open_device(d_src, src_size, block_size, max_blocks, d_index, index_size, stream=0):
    """zxc_mi355x_seekable_open_device(): raw device pointers (ints), asynchronous on `stream`. Whether the archive's seek table
    was accepted lands in the index's first int32; a synchronous failure raises ZxcError."""
    _call("zxc_mi355x_seekable_open_device", d_src, src_size, block_size, max_blocks, d_index, index_size, stream)


def decompress_ranges_device_work_size(n_ranges, max_len, block_size):
    """zxc_mi355x_decompress_ranges_device_work_size(): bytes of device scratch the call needs (0 for refused arguments)."""
    return int(_call("zxc_mi355x_decompress_ranges_device_work_size", n_ranges, max_len, block_size))


def decompress_ranges_device(d_src, src_size, d_index, d_ranges, n_ranges, max_len, d_dst, dst_capacity, block_size, d_work, work_size,
                             d_results, stream=0):
    """zxc_mi355x_decompress_ranges_device(): raw device pointers (ints); d_ranges is n_ranges x RANGE_DTYPE in device memory,
    d_results n_ranges x int64. Asynchronous on `stream`; a synchronous failure raises ZxcError."""
    _call("zxc_mi355x_decompress_ranges_device", d_src, src_size, d_index, d_ranges, n_ranges, max_len, d_dst, dst_capacity,
          block_size, d_work, work_size, d_results, stream)


# ---- the device calls with a dictionary in device memory (include/zxc_mi355x.h: zxc_dev_dict_t)
def dict_prepare_device(d_content, size, d_huf, d_id, stream=0):
    """zxc_mi355x_dict_prepare_device(): the uint32 at d_id receives zxc_dict_id of the content (and the 128-byte table at d_huf,
    or 0 for none), computed on the device, asynchronously on `stream`. A synchronous failure raises ZxcError."""
    _call("zxc_mi355x_dict_prepare_device", d_content, size, d_huf, d_id, stream)


def compress_dict_device_work_size(src_size, dict_size, level=3, block_size=0, seekable=False, checksum=False):
    """zxc_mi355x_compress_dict_device_work_size(): bytes of device scratch compress_dict_device needs with a dictionary of
    dict_size bytes (0 for invalid options; dict_size 0 gives compress_device_work_size)."""
    return int(_call("zxc_mi355x_compress_dict_device_work_size", src_size, _copts(level, block_size, seekable, checksum), dict_size))


def compress_dict_device(d_src, src_size, d_dst, dst_capacity, dict_, d_work, work_size, d_result, level=3, block_size=0,
                         seekable=False, checksum=False, stream=0):
    """zxc_mi355x_compress_dict_device(): compress_device with a dictionary in device memory, dict_ = (d_content, size, d_huf or 0,
    d_id) with d_id prepared by dict_prepare_device, or None for no dictionary."""
    _call("zxc_mi355x_compress_dict_device", d_src, src_size, d_dst, dst_capacity, _copts(level, block_size, seekable, checksum),
          _dev_dict(dict_), d_work, work_size, d_result, stream)


def decompress_dict_device(d_src, src_size, d_dst, dst_capacity, block_size, dict_, d_work, work_size, d_result, checksum=False,
                           stream=0):
    """zxc_mi355x_decompress_dict_device(): decompress_device with a dictionary in device memory (dict_ as in
    compress_dict_device); the work size is decompress_device_work_size."""
    _call("zxc_mi355x_decompress_dict_device", d_src, src_size, d_dst, dst_capacity, block_size, _dopts(checksum), _dev_dict(dict_),
          d_work, work_size, d_result, stream)


def decompress_ranges_dict_device(d_src, src_size, d_index, d_ranges, n_ranges, max_len, d_dst, dst_capacity, block_size, dict_,
                                  d_work, work_size, d_results, stream=0):
    """zxc_mi355x_decompress_ranges_dict_device(): decompress_ranges_device with a dictionary in device memory (dict_ as in
    compress_dict_device); index and work size are the sibling's."""
    _call("zxc_mi355x_decompress_ranges_dict_device", d_src, src_size, d_index, d_ranges, n_ranges, max_len, d_dst, dst_capacity,
          block_size, _dev_dict(dict_), d_work, work_size, d_results, stream)


# ---- random access into a pointer table (include/zxc_mi355x_rangesv.h: zxc_dev_rangev_t)
def decompress_rangesv_device_work_size(n_ranges, max_len, block_size):
    """zxc_mi355x_decompress_rangesv_device_work_size(): bytes of device scratch the call needs (0 for refused arguments); the
    value decompress_ranges_device_work_size gives for the same arguments."""
    return int(_call("zxc_mi355x_decompress_rangesv_device_work_size", n_ranges, max_len, block_size))


def decompress_rangesv_device(d_src, src_size, d_index, d_ranges, n_ranges, max_len, block_size, d_work, work_size, d_results, stream=0):
    """zxc_mi355x_decompress_rangesv_device(): raw device pointers (ints); d_ranges is n_ranges x RANGEV_DTYPE in device memory,
    each entry with the device address of its own destination, d_results n_ranges x int64; the index is seekable_open_device's.
    Asynchronous on `stream`; a synchronous failure raises ZxcError."""
    _call("zxc_mi355x_decompress_rangesv_device", d_src, src_size, d_index, d_ranges, n_ranges, max_len, block_size, d_work, work_size,
          d_results, stream)


def decompress_rangesv_dict_device(d_src, src_size, d_index, d_ranges, n_ranges, max_len, block_size, dict_, d_work, work_size,
                                   d_results, stream=0):
    """zxc_mi355x_decompress_rangesv_dict_device(): decompress_rangesv_device with a dictionary in device memory (dict_ as in
    compress_dict_device); index and work size are the sibling's."""
    _call("zxc_mi355x_decompress_rangesv_dict_device", d_src, src_size, d_index, d_ranges, n_ranges, max_len, block_size,
          _dev_dict(dict_), d_work, work_size, d_results, stream)


# ---- the byte-shuffle pre-filter for typed tensors (include/zxc_mi355x_shuffle.h)
def shuffle_device(d_src, d_dst, n, elem_size, unit, stream=0):
    """zxc_mi355x_shuffle_device(): d_dst[0, n) = the bytes of d_src[0, n) regrouped into byte planes per unit (elem_size 2, 4 or 8;
    unit a power of two in [4 KiB, 2 MiB], the block size for the archive calls). Raw device pointers (ints) of any alignment,
    asynchronous on `stream`; a synchronous failure raises ZxcError."""
    _call("zxc_mi355x_shuffle_device", d_src, d_dst, n, elem_size, unit, stream)


def unshuffle_device(d_src, d_dst, n, elem_size, unit, stream=0):
    """zxc_mi355x_unshuffle_device(): the inverse of shuffle_device for the same n, elem_size and unit."""
    _call("zxc_mi355x_unshuffle_device", d_src, d_dst, n, elem_size, unit, stream)


def compress_shuffle_device_work_size(src_size, max_piece=0, dict_size=0, level=3, block_size=0, seekable=False, checksum=False):
    """zxc_mi355x_compress_shuffle_device_work_size(): bytes of device scratch compress_shuffle_device needs (0 for refused
    arguments): the append session's for a chunk of max_piece bytes (0: the default) plus one chunk."""
    return int(_call("zxc_mi355x_compress_shuffle_device_work_size", src_size, max_piece, _copts(level, block_size, seekable, checksum),
                     dict_size))


def compress_shuffle_device(d_src, src_size, elem_size, d_dst, dst_capacity, d_work, work_size, d_result, max_piece=0, dict_=None,
                            level=3, block_size=0, seekable=False, checksum=False, stream=0):
    """zxc_mi355x_compress_shuffle_device(): the archive compress_device (with dict_, as in compress_dict_device: that call) writes
    for the byte-shuffled source, shuffled chunk by chunk into a stage of the work area. The archive does not record the filter:
    the caller keeps elem_size. Raw device pointers (ints), asynchronous on `stream`; the archive size or a negative zxc_error_t
    lands in the int64 at d_result; a synchronous failure raises ZxcError."""
    _call("zxc_mi355x_compress_shuffle_device", d_src, src_size, elem_size, d_dst, dst_capacity, max_piece,
          _copts(level, block_size, seekable, checksum), _dev_dict(dict_), d_work, work_size, d_result, stream)


def decompress_shuffle_device_work_size(src_size, dst_size, max_piece, block_size):
    """zxc_mi355x_decompress_shuffle_device_work_size(): bytes of device scratch decompress_shuffle_device needs (0 for refused
    arguments): the take session's for a chunk of max_piece bytes (0: the default) plus one chunk."""
    return int(_call("zxc_mi355x_decompress_shuffle_device_work_size", src_size, dst_size, max_piece, block_size))


def decompress_shuffle_device(d_src, src_size, d_dst, dst_size, elem_size, block_size, d_work, work_size, d_result, max_piece=0, dict_=None,
                              checksum=False, stream=0):
    """zxc_mi355x_decompress_shuffle_device(): decodes the archive chunk by chunk into a stage of the work area and un-shuffles it
    into d_dst (any alignment). dst_size is the decoded size exactly; dst_size or a negative zxc_error_t lands in the int64 at
    d_result. Raw device pointers (ints), asynchronous on `stream`; a synchronous failure raises ZxcError."""
    _call("zxc_mi355x_decompress_shuffle_device", d_src, src_size, d_dst, dst_size, elem_size, max_piece, block_size, _dopts(checksum),
          _dev_dict(dict_), d_work, work_size, d_result, stream)


# ---- ranges of the plain bytes of a byte-shuffled archive into a pointer table (include/zxc_mi355x_rangesv_shuffle.h)
def decompress_rangesv_shuffle_device_work_size(n_ranges, max_len, block_size):
    """zxc_mi355x_decompress_rangesv_shuffle_device_work_size(): bytes of device scratch the call needs (0 for refused arguments):
    rangesv's layout with a gather record per job."""
    return int(_call("zxc_mi355x_decompress_rangesv_shuffle_device_work_size", n_ranges, max_len, block_size))


def decompress_rangesv_shuffle_device(d_src, src_size, d_index, d_ranges, n_ranges, max_len, elem_size, block_size, d_work, work_size,
                                      d_results, dict_=None, stream=0):
    """zxc_mi355x_decompress_rangesv_shuffle_device(): decompress_rangesv_device for an archive of byte-shuffled blocks (elem_size 2,
    4 or 8; unit = block_size): the ranges of d_ranges (n_ranges x RANGEV_DTYPE in device memory) count bytes of the plain tensor,
    at any offset, and every destination receives plain bytes. dict_ as in compress_dict_device, or None. Raw device pointers
    (ints), asynchronous on `stream`; a synchronous failure raises ZxcError."""
    _call("zxc_mi355x_decompress_rangesv_shuffle_device", d_src, src_size, d_index, d_ranges, n_ranges, max_len, elem_size, block_size,
          _dev_dict(dict_), d_work, work_size, d_results, stream)


# ---- the byte-shuffle of a table of typed tensors (include/zxc_mi355x_shufflev.h): the write side of the shuffled ranges
def shufflev_device_scratch_size(n_iov):
    """zxc_mi355x_shufflev_device_scratch_size(): bytes of device scratch shufflev_device needs for a table of n_iov entries."""
    return int(_call("zxc_mi355x_shufflev_device_scratch_size", n_iov))


def shufflev_device(d_iov, n_iov, total, d_dst, elem_size, unit, d_scratch, scratch_size, d_status, stream=0):
    """zxc_mi355x_shufflev_device(): d_dst[0, total) = shuffle_device's bytes for the concatenation of the n_iov x IOV_DTYPE entries
    at d_iov (device memory), `total` bytes in all, with no concatenated copy. 0 or the table's error lands in the int64 at
    d_status. Raw device pointers (ints) of any alignment, asynchronous on `stream`; a synchronous failure raises ZxcError."""
    _call("zxc_mi355x_shufflev_device", d_iov, n_iov, total, d_dst, elem_size, unit, d_scratch, scratch_size, d_status, stream)


def compress_shufflev_device_work_size(n_iov, total, max_piece=0, dict_size=0, level=3, block_size=0, seekable=False, checksum=False):
    """zxc_mi355x_compress_shufflev_device_work_size(): bytes of device scratch compress_shufflev_device needs (0 for refused
    arguments): compress_shuffle_device's rounded up to 256, the table's scratch and 256 bytes."""
    return int(_call("zxc_mi355x_compress_shufflev_device_work_size", n_iov, total, max_piece,
                     _copts(level, block_size, seekable, checksum), dict_size))


def compress_shufflev_device(d_iov, n_iov, total, elem_size, d_dst, dst_capacity, d_work, work_size, d_result, max_piece=0, dict_=None,
                             level=3, block_size=0, seekable=False, checksum=False, stream=0):
    """zxc_mi355x_compress_shufflev_device(): the archive compress_shuffle_device writes for the concatenation of the n_iov x
    IOV_DTYPE entries at d_iov (device memory), `total` bytes in all, gathered and shuffled chunk by chunk into the stage: no
    concatenated copy. Tensor r is read back with decompress_rangesv_shuffle_device at offset = the lengths in front of it. The
    archive size, a negative zxc_error_t or the table's error lands in the int64 at d_result. Raw device pointers (ints),
    asynchronous on `stream`; a synchronous failure raises ZxcError."""
    _call("zxc_mi355x_compress_shufflev_device", d_iov, n_iov, total, elem_size, d_dst, dst_capacity, max_piece,
          _copts(level, block_size, seekable, checksum), _dev_dict(dict_), d_work, work_size, d_result, stream)


# ---- the inverse byte-shuffle into a table of typed tensors (include/zxc_mi355x_unshufflev.h): the load side of shufflev
def unshufflev_device_scratch_size(n_iov):
    """zxc_mi355x_unshufflev_device_scratch_size(): bytes of device scratch unshufflev_device needs for a table of n_iov entries
    (shufflev_device_scratch_size's)."""
    return int(_call("zxc_mi355x_unshufflev_device_scratch_size", n_iov))


def unshufflev_device(d_src, d_iov, n_iov, total, elem_size, unit, d_scratch, scratch_size, d_status, stream=0):
    """zxc_mi355x_unshufflev_device(): the n_iov x IOV_DTYPE entries at d_iov (device memory), `total` bytes in all, receive
    unshuffle_device's bytes for d_src[0, total), cut by the table, with no contiguous copy. 0 or the table's error lands in the
    int64 at d_status. Raw device pointers (ints) of any alignment, asynchronous on `stream`; a synchronous failure raises
    ZxcError."""
    _call("zxc_mi355x_unshufflev_device", d_src, d_iov, n_iov, total, elem_size, unit, d_scratch, scratch_size, d_status, stream)


def decompress_shufflev_device_work_size(n_iov, src_size, total, max_piece, block_size):
    """zxc_mi355x_decompress_shufflev_device_work_size(): bytes of device scratch decompress_shufflev_device needs (0 for refused
    arguments): decompress_shuffle_device's rounded up to 256 and the table's scratch."""
    return int(_call("zxc_mi355x_decompress_shufflev_device_work_size", n_iov, src_size, total, max_piece, block_size))


def decompress_shufflev_device(d_src, src_size, d_iov, n_iov, total, elem_size, block_size, d_work, work_size, d_result, max_piece=0,
                               dict_=None, checksum=False, stream=0):
    """zxc_mi355x_decompress_shufflev_device(): decodes the archive chunk by chunk into a stage of the work area and un-shuffles it
    into the n_iov x IOV_DTYPE entries at d_iov (device memory), `total` bytes in all: what decompress_shuffle_device writes for
    dst_size = total, cut by the table. total, a negative zxc_error_t or the table's error lands in the int64 at d_result. Raw
    device pointers (ints), asynchronous on `stream`; a synchronous failure raises ZxcError."""
    _call("zxc_mi355x_decompress_shufflev_device", d_src, src_size, d_iov, n_iov, total, elem_size, max_piece, block_size, _dopts(checksum),
          _dev_dict(dict_), d_work, work_size, d_result, stream)


# ---- many archives per call (include/zxc_mi355x.h: zxc_dev_item_t)
def decompress_batch_device_work_size(n_items, max_capacity, block_size):
    """zxc_mi355x_decompress_batch_device_work_size(): bytes of device scratch the call needs (0 for refused arguments)."""
    return int(_call("zxc_mi355x_decompress_batch_device_work_size", n_items, max_capacity, block_size))


def decompress_batch_device(d_src, src_capacity, d_items, n_items, max_capacity, d_dst, dst_capacity, block_size, d_work, work_size,
                            d_results, checksum=False, stream=0):
    """zxc_mi355x_decompress_batch_device(): raw device pointers (ints); d_items is n_items x ITEM_DTYPE in device memory, d_results
    n_items x int64, each what zxc_decompress would return for that item. Asynchronous on `stream`; a synchronous failure raises
    ZxcError."""
    _call("zxc_mi355x_decompress_batch_device", d_src, src_capacity, d_items, n_items, max_capacity, d_dst, dst_capacity, block_size,
          _dopts(checksum), d_work, work_size, d_results, stream)


def decompress_batch_dict_device(d_src, src_capacity, d_items, n_items, max_capacity, d_dst, dst_capacity, block_size, dict_, d_work,
                                 work_size, d_results, checksum=False, stream=0):
    """zxc_mi355x_decompress_batch_dict_device(): decompress_batch_device with one dictionary in device memory for the whole batch
    (dict_ as in compress_dict_device); the work size is the sibling's."""
    _call("zxc_mi355x_decompress_batch_dict_device", d_src, src_capacity, d_items, n_items, max_capacity, d_dst, dst_capacity,
          block_size, _dopts(checksum), _dev_dict(dict_), d_work, work_size, d_results, stream)


# ---- many buffers per call: the write side (zxc_dev_item_t: src_* the buffer to compress, dst_* where its archive goes)
def _batch_work_size(name, n_items, max_size, o, dict_size):
    if dict_size:
        return int(_call(f"zxc_mi355x_{name}_dict_device_work_size", n_items, max_size, o, dict_size))
    return int(_call(f"zxc_mi355x_{name}_device_work_size", n_items, max_size, o))


def compress_batch_device_work_size(n_items, max_size, level=3, block_size=0, seekable=False, checksum=False, dict_size=0):
    """zxc_mi355x_compress_batch_device_work_size(), or with dict_size the _dict call's: bytes of device scratch the call needs
    (0 for refused arguments)."""
    return _batch_work_size("compress_batch", n_items, max_size, _copts(level, block_size, seekable, checksum), dict_size)


def compress_batch_device(d_src, src_capacity, d_items, n_items, max_size, d_dst, dst_capacity, d_work, work_size, d_results, level=3,
                          block_size=0, seekable=False, checksum=False, stream=0):
    """zxc_mi355x_compress_batch_device(): raw device pointers (ints); d_items is n_items x ITEM_DTYPE in device memory (src_* the
    buffer to compress, dst_* where its archive goes), d_results n_items x int64, each the item's archive size or a negative
    zxc_error_t. Asynchronous on `stream`; a synchronous failure raises ZxcError."""
    _call("zxc_mi355x_compress_batch_device", d_src, src_capacity, d_items, n_items, max_size, d_dst, dst_capacity,
          _copts(level, block_size, seekable, checksum), d_work, work_size, d_results, stream)


def compress_batch_dict_device(d_src, src_capacity, d_items, n_items, max_size, d_dst, dst_capacity, dict_, d_work, work_size, d_results,
                               level=3, block_size=0, seekable=False, checksum=False, stream=0):
    """zxc_mi355x_compress_batch_dict_device(): compress_batch_device with one dictionary in device memory for the whole batch
    (dict_ as in compress_dict_device); the work size is compress_batch_device_work_size(..., dict_size=size)."""
    _call("zxc_mi355x_compress_batch_dict_device", d_src, src_capacity, d_items, n_items, max_size, d_dst, dst_capacity,
          _copts(level, block_size, seekable, checksum), _dev_dict(dict_), d_work, work_size, d_results, stream)


# ---- many buffers per call, the archives packed back to back (d_packed: the item table of decompress_batch_device)
def compress_pack_device_work_size(n_items, max_size, level=3, block_size=0, seekable=False, checksum=False, dict_size=0):
    """zxc_mi355x_compress_pack_device_work_size(), or with dict_size the _dict call's: bytes of device scratch the call needs
    (0 for refused arguments)."""
    return _batch_work_size("compress_pack", n_items, max_size, _copts(level, block_size, seekable, checksum), dict_size)


def compress_pack_device(d_src, src_capacity, d_items, n_items, max_size, d_dst, dst_capacity, align, d_work, work_size, d_packed,
                         d_results, d_total, level=3, block_size=0, seekable=False, checksum=False, stream=0):
    """zxc_mi355x_compress_pack_device(): compress_batch_device with the archives laid back to back, each at a multiple of `align`.
    Raw device pointers (ints); of d_items (n_items x ITEM_DTYPE) only src_off / src_size are read; d_packed (n_items x ITEM_DTYPE,
    may be d_items) receives the item table of decompress_batch_device, d_results n_items x int64, d_total one uint64: the end of
    the last archive, whatever dst_capacity was. Asynchronous on `stream`; a synchronous failure raises ZxcError."""
    _call("zxc_mi355x_compress_pack_device", d_src, src_capacity, d_items, n_items, max_size, d_dst, dst_capacity, align,
          _copts(level, block_size, seekable, checksum), d_work, work_size, d_packed, d_results, d_total, stream)


def compress_pack_dict_device(d_src, src_capacity, d_items, n_items, max_size, d_dst, dst_capacity, align, dict_, d_work, work_size,
                              d_packed, d_results, d_total, level=3, block_size=0, seekable=False, checksum=False, stream=0):
    """zxc_mi355x_compress_pack_dict_device(): compress_pack_device with one dictionary in device memory for the whole batch
    (dict_ as in compress_dict_device); the work size is compress_pack_device_work_size(..., dict_size=size)."""
    _call("zxc_mi355x_compress_pack_dict_device", d_src, src_capacity, d_items, n_items, max_size, d_dst, dst_capacity, align,
          _copts(level, block_size, seekable, checksum), _dev_dict(dict_), d_work, work_size, d_packed, d_results, d_total, stream)


# ---- one archive from many pieces: a session
def compress_append_device_work_size(max_total, max_piece, level=3, block_size=0, seekable=False, checksum=False):
    """zxc_mi355x_compress_append_device_work_size(): bytes of device scratch a session needs (0 for refused arguments)."""
    return int(_call("zxc_mi355x_compress_append_device_work_size", max_total, max_piece, _copts(level, block_size, seekable, checksum)))


def compress_appendv_device_scratch_size(n_iov, max_piece, level=3, block_size=0, seekable=False, checksum=False):
    """zxc_mi355x_compress_appendv_device_scratch_size(): bytes of device scratch one appendv of n_iov entries needs in a session
    of that max_piece (0 for refused arguments)."""
    return int(_call("zxc_mi355x_compress_appendv_device_scratch_size", n_iov, max_piece, _copts(level, block_size, seekable, checksum)))


def compress_appendv_dict_device_scratch_size(n_iov, max_piece, dict_size, level=3, block_size=0, seekable=False, checksum=False):
    """zxc_mi355x_compress_appendv_dict_device_scratch_size(): bytes of device scratch one appendv_dict of n_iov entries needs in a
    session of that max_piece with a dictionary of dict_size bytes (0 for refused arguments; dict_size 0 gives
    compress_appendv_device_scratch_size)."""
    return int(_call("zxc_mi355x_compress_appendv_dict_device_scratch_size", n_iov, max_piece,
                     _copts(level, block_size, seekable, checksum), dict_size))


class CompressAppendSession:
    """A session of zxc_mi355x_compress_begin_device(): .append(d_src, n) and .appendv(d_iov, n_iov, total, d_scratch,
    scratch_size) (with a dictionary: .appendv_dict) any number of times, then .end(d_result) once. Raw device pointers (ints), asynchronous on `stream`; the calls of
    one session must be in stream order with each other. The archive size or a negative zxc_error_t lands in the int64 at d_result;
    a synchronous failure raises ZxcError."""

    def __init__(self, cs):
        self._cs = cs

    def append(self, d_src, n, stream=0):
        _call("zxc_mi355x_compress_append_device", self._cs, d_src, n, stream)

    def appendv(self, d_iov, n_iov, total, d_scratch, scratch_size, stream=0):
        """zxc_mi355x_compress_appendv_device(): appends the concatenation of the n_iov x IOV_DTYPE entries at d_iov (device
        memory), `total` bytes in all; the scratch size is compress_appendv_device_scratch_size(n_iov, max_piece, ...)."""
        _call("zxc_mi355x_compress_appendv_device", self._cs, d_iov, n_iov, total, d_scratch, scratch_size, stream)

    def appendv_dict(self, d_iov, n_iov, total, d_scratch, scratch_size, stream=0):
        """zxc_mi355x_compress_appendv_dict_device(): appendv for a session begun with a dictionary (one begun without is served as
        appendv serves it); the scratch size is compress_appendv_dict_device_scratch_size(n_iov, max_piece, dict_size, ...)."""
        _call("zxc_mi355x_compress_appendv_dict_device", self._cs, d_iov, n_iov, total, d_scratch, scratch_size, stream)

    def end(self, d_result, stream=0):
        _call("zxc_mi355x_compress_end_device", self._cs, d_result, stream)


def compress_begin_device(d_dst, dst_capacity, max_total, max_piece, d_work, work_size, level=3, block_size=0, seekable=False,
                          checksum=False, stream=0):
    """zxc_mi355x_compress_begin_device(): -> a CompressAppendSession that writes one archive to d_dst from the pieces it is
    given; the work size is compress_append_device_work_size(max_total, max_piece, ...)."""
    cs = _DevCappend()
    _call("zxc_mi355x_compress_begin_device", cs, d_dst, dst_capacity, max_total, max_piece,
          _copts(level, block_size, seekable, checksum), d_work, work_size, stream)
    return CompressAppendSession(cs)


def compress_append_dict_device_work_size(max_total, max_piece, dict_size, level=3, block_size=0, seekable=False, checksum=False):
    """zxc_mi355x_compress_append_dict_device_work_size(): bytes of device scratch a session with a dictionary of dict_size bytes
    needs (0 for refused arguments; dict_size 0 gives compress_append_device_work_size)."""
    return int(_call("zxc_mi355x_compress_append_dict_device_work_size", max_total, max_piece,
                     _copts(level, block_size, seekable, checksum), dict_size))


def compress_begin_dict_device(d_dst, dst_capacity, max_total, max_piece, dict_, d_work, work_size, level=3, block_size=0,
                               seekable=False, checksum=False, stream=0):
    """zxc_mi355x_compress_begin_dict_device(): compress_begin_device with a dictionary in device memory (dict_ as in
    compress_dict_device, or None for no dictionary) -> a CompressAppendSession; the work size is
    compress_append_dict_device_work_size(max_total, max_piece, dict_size, ...)."""
    cs = _DevCappend()
    _call("zxc_mi355x_compress_begin_dict_device", cs, d_dst, dst_capacity, max_total, max_piece,
          _copts(level, block_size, seekable, checksum), _dev_dict(dict_), d_work, work_size, stream)
    return CompressAppendSession(cs)


# ---- one archive into many pieces: a session
def decompress_takev_device_scratch_size(n_iov, max_piece, block_size):
    """zxc_mi355x_decompress_takev_device_scratch_size(): bytes of device scratch one takev of n_iov entries needs in a session
    of that max_piece and block_size (0 for refused arguments)."""
    return int(_call("zxc_mi355x_decompress_takev_device_scratch_size", n_iov, max_piece, block_size))


def decompress_take_device_work_size(src_size, dst_capacity, max_piece, block_size):
    """zxc_mi355x_decompress_take_device_work_size(): bytes of device scratch a session needs (0 for refused arguments)."""
    return int(_call("zxc_mi355x_decompress_take_device_work_size", src_size, dst_capacity, max_piece, block_size))


class DecompressTakeSession:
    """A session of zxc_mi355x_decompress_begin_device(): .take(d_dst, n) and .takev(d_iov, n_iov, total, d_scratch, scratch_size)
    until dst_capacity bytes are taken, then .end(d_result) once. Raw device pointers (ints), asynchronous on `stream`; the calls of one session must be in stream order with each other.
    The decoded size or the negative zxc_error_t decompress_device would store lands in the int64 at d_result; a synchronous
    failure raises ZxcError."""

    def __init__(self, ds):
        self._ds = ds

    def take(self, d_dst, n, stream=0):
        _call("zxc_mi355x_decompress_take_device", self._ds, d_dst, n, stream)

    def takev(self, d_iov, n_iov, total, d_scratch, scratch_size, stream=0):
        """zxc_mi355x_decompress_takev_device(): delivers the next `total` bytes into the n_iov x IOV_DTYPE entries at d_iov (device
        memory), in table order; the scratch size is decompress_takev_device_scratch_size(n_iov, max_piece, block_size)."""
        _call("zxc_mi355x_decompress_takev_device", self._ds, d_iov, n_iov, total, d_scratch, scratch_size, stream)

    def end(self, d_result, stream=0):
        _call("zxc_mi355x_decompress_end_device", self._ds, d_result, stream)


def decompress_begin_device(d_src, src_size, dst_capacity, max_piece, block_size, d_work, work_size, checksum=False, stream=0):
    """zxc_mi355x_decompress_begin_device(): -> a DecompressTakeSession that delivers the archive at d_src in the pieces it is
    asked for; the work size is decompress_take_device_work_size(src_size, dst_capacity, max_piece, block_size)."""
    ds = _DevDtake()
    _call("zxc_mi355x_decompress_begin_device", ds, d_src, src_size, dst_capacity, max_piece, block_size, _dopts(checksum), d_work,
          work_size, stream)
    return DecompressTakeSession(ds)


def decompress_begin_dict_device(d_src, src_size, dst_capacity, max_piece, block_size, dict_, d_work, work_size, checksum=False,
                                 stream=0):
    """zxc_mi355x_decompress_begin_dict_device(): decompress_begin_device with a dictionary in device memory (dict_ as in
    compress_dict_device); the work size is the sibling's."""
    ds = _DevDtake()
    _call("zxc_mi355x_decompress_begin_dict_device", ds, d_src, src_size, dst_capacity, max_piece, block_size, _dopts(checksum),
          _dev_dict(dict_), d_work, work_size, stream)
    return DecompressTakeSession(ds)


# ---- FILE* callers (include/zxc_stream.h). ctypes has no FILE*, so the C library's fopen/fclose are used.
_LIBC = None


def _libc():
    global _LIBC
    if _LIBC is None:
        L = C.CDLL(None)
        L.fopen.restype = C.c_void_p
        L.fopen.argtypes = [C.c_char_p, C.c_char_p]
        L.fclose.argtypes = [C.c_void_p]
        _LIBC = L
    return _LIBC


class _File:
    def __init__(self, path, mode):
        self.fp = _libc().fopen(os.fsencode(path), mode.encode())
        if not self.fp:
            raise OSError(f"fopen({path!r}, {mode!r}) failed")

    def __enter__(self):
        return self.fp

    def __exit__(self, *a):
        _libc().fclose(self.fp)


def stream_compress(src_path, dst_path, level=3, block_size=65536, seekable=True, checksum=False, library=None, dict_=None,
                    dict_huf=None):
    """zxc_stream_compress(): file in, archive out. Returns bytes written or a negative zxc_error_t."""
    L = _bind_stream(library) if library else lib()
    o = _copts(level, block_size, seekable, checksum)
    _keep = _set_dict(o, dict_, dict_huf)
    with _File(src_path, "rb") as fi, _File(dst_path, "wb") as fo:
        return int(L.zxc_stream_compress(fi, fo, C.byref(o)))


def stream_decompress(src_path, dst_path, checksum=False, library=None, dict_=None, dict_huf=None):
    """zxc_stream_decompress(): archive in, file out (dst_path None = integrity check only)."""
    L = _bind_stream(library) if library else lib()
    o = _dopts(checksum)
    _keep = _set_dict(o, dict_, dict_huf)
    with _File(src_path, "rb") as fi:
        if dst_path is None:
            return int(L.zxc_stream_decompress(fi, None, C.byref(o)))
        with _File(dst_path, "wb") as fo:
            return int(L.zxc_stream_decompress(fi, fo, C.byref(o)))


def stream_get_decompressed_size(path, library=None):
    L = _bind_stream(library) if library else lib()
    with _File(path, "rb") as fi:
        return int(L.zxc_stream_get_decompressed_size(fi))


# ---- push streaming (include/zxc_pstream.h). The same prototypes bind the product and (in tests) the reference library.
def pstream_compress(data: bytes, in_chunk, out_chunk, level=3, block_size=0, checksum=False, library=None):
    """Feed `data` to a zxc_cstream in chunks of in_chunk bytes, drain through an out buffer of out_chunk bytes, finish with
    zxc_cstream_end (the loop of the reference's header example, include/zxc_pstream.h:26-49).
    -> (0, archive) or (negative zxc_error_t, bytes produced so far)."""
    L = _bind_pstream(library) if library else lib()
    o = _CompressOpts(level=level, block_size=block_size, checksum_enabled=int(checksum))
    cs = L.zxc_cstream_create(C.byref(o))
    if not cs:
        return None, b""
    src = C.create_string_buffer(data, max(len(data), 1))
    base = C.addressof(src)
    out_chunk = min(out_chunk, len(data) + len(data) // 8 + (1 << 20))  # (no point in allocating more than the archive can take)
    obuf = C.create_string_buffer(max(out_chunk, 1))
    out = _OutBuf(C.addressof(obuf), out_chunk, 0)
    blob = bytearray()
    try:
        off = 0
        while off < len(data):
            n = min(in_chunk, len(data) - off)
            inb = _InBuf(base + off, n, 0)
            while inb.pos < inb.size:
                r = L.zxc_cstream_compress(cs, C.byref(out), C.byref(inb))
                if r < 0:
                    return int(r), bytes(blob)
                if out.pos:
                    blob += C.string_at(out.dst, out.pos)
                    out.pos = 0
                elif r > 0 and out.size == 0:
                    raise RuntimeError("no progress with an empty out buffer")
            off += n
        while True:
            r = L.zxc_cstream_end(cs, C.byref(out))
            if r < 0:
                return int(r), bytes(blob)
            if out.pos:
                blob += C.string_at(out.dst, out.pos)
                out.pos = 0
            if r == 0:
                return 0, bytes(blob)
    finally:
        L.zxc_cstream_free(cs)


def pstream_decompress(comp: bytes, in_chunk, out_chunk, checksum=False, library=None):
    """Feed `comp` to a zxc_dstream in chunks of in_chunk bytes, drain through an out buffer of out_chunk bytes, until the decoder
    neither consumes nor produces (reference tests/test_pstream_api.c:107-172).
    -> (rc of the last call, decoded bytes, finished flag, input bytes consumed)."""
    L = _bind_pstream(library) if library else lib()
    o = _dopts(checksum)
    ds = L.zxc_dstream_create(C.byref(o))
    if not ds:
        return None, b"", 0, 0
    src = C.create_string_buffer(comp, max(len(comp), 1))
    base = C.addressof(src)
    hint = int.from_bytes(comp[-12:-4], "little") if len(comp) >= 12 else 0  # the footer's size: a hint only (mutants lie)
    out_chunk = min(out_chunk, max(hint, 1 << 16) + (4 << 20))
    obuf = C.create_string_buffer(max(out_chunk, 1))
    out = _OutBuf(C.addressof(obuf), out_chunk, 0)
    dec = bytearray()
    try:
        off = 0
        while True:
            n = min(in_chunk, len(comp) - off)
            inb = _InBuf(base + off if n else None, n, 0)
            r = L.zxc_dstream_decompress(ds, C.byref(out), C.byref(inb))
            if out.pos:
                dec += C.string_at(out.dst, out.pos)
                out.pos = 0
            off += inb.pos
            if r < 0:
                return int(r), bytes(dec), 0, off
            if (off >= len(comp) or L.zxc_dstream_finished(ds)) and inb.pos == 0 and r == 0:
                return 0, bytes(dec), int(L.zxc_dstream_finished(ds)), off
    finally:
        L.zxc_dstream_free(ds)


def set_debug(lib_handle, flags: int) -> None:
    """tools/ only: the plan-forcing bits ZXC_DEV_DBG_* (zxc_dev.h) exist in libraries built with -DZXC_EXPERIMENT
    (tools/build_variant.sh <name>, selected with ZXC_LIB_VARIANT); the release library does not export the setter."""
    if not hasattr(lib_handle, "zxc_mi355x__set_debug"):
        if flags:
            raise RuntimeError("this library was built without -DZXC_EXPERIMENT: set ZXC_LIB_VARIANT to an experiment build")
        return
    lib_handle.zxc_mi355x__set_debug(flags)
