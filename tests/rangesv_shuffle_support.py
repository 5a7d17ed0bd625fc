"""What the tests of zxc_mi355x_decompress_rangesv_shuffle_device share (tests/test_decompress_rangesv_shuffle_device_cpu.py,
tests/test_gpu_decompress_rangesv_shuffle_device.py): the sizes and range lists of both, the rules shim
(tests/ranges/rangesv_shuffle_shim.c) with its structs, and on the GPU the guarded destinations, the open and the call. A plain
module next to the tests, imported the way devtest is."""
import ctypes as C

import numpy as np

import cshim
import shuffle_support as ss
from devtest import CANARY, ERR, UNSET, pattern

ELEMS = (2, 4, 8)
# block size -> plain bytes: nine blocks and a ragged one; three blocks and a ragged one of 8589 bytes, which spans a gather chunk's
# seam (8192), has q = 8589 // E no multiple of 16 and 8589 % E copied bytes for each E
SIZES = {4096: 9 * 4096 + 1003, 16384: 3 * 16384 + 8589}
M64 = (1 << 64) - 1
ZERO_BASE, WRAP = "zero base", "wrap"   # table entries whose base is not the allocation's
PRE_BLOCK = tuple(ERR[k] for k in ("DST_TOO_SMALL", "NULL_INPUT", "SRC_TOO_SMALL", "DICT_REQUIRED", "DICT_MISMATCH", "BAD_BLOCK_SIZE"))


def plain_and_shuffled(E, bs, seed=None):
    """a seeded typed tensor of SIZES[bs] bytes -> (plain bytes, np_shuffle of them with unit = bs)"""
    plain = ss.tensor_bytes(SIZES[bs], E, E * 100 + bs // 4096 if seed is None else seed)
    return plain, ss.np_shuffle(np.frombuffer(plain, dtype=np.uint8), E, bs).tobytes()


def range_list(total, bs, rng, n_random, span=3):
    """the fixed list of the rangesv tests and n_random seeded ranges of at most span blocks: (offset, len)"""
    nb = -(-total // bs)
    want = [(0, total), (0, 1), (total - 1, 1), (0, 0), (total, 0), (total + 5, 0), (total, 1), (total - 1, 2), (total + 1, 1),
            (min(7, total - 1), min(100, total - min(7, total - 1)))]
    if nb >= 2:
        want += [(bs - 3, 6), (bs, min(bs, total - bs)), (bs - 1, min(bs + 2, total - bs + 1)), (0, bs), (0, bs + 32), (0, bs + 31)]
    if nb >= 4:
        want += [(bs + 16, 2 * bs + 100), (5, 3 * bs), (2 * bs, bs + 40), (bs - 16, 2 * bs + 64), (0, 2 * bs), (bs, 3 * bs)]
    for _ in range(n_random):
        a = rng.randrange(total)
        want.append((a, rng.randrange(1, min(total - a, span * bs) + 1)))
    return want


# ---------------------------------------------------------------- the rules, compiled with the host C compiler
class Index(C.Structure):  # zr_index_t
    _fields_ = [("status", C.c_int32), ("nb", C.c_uint32), ("total", C.c_uint64), ("file_ck", C.c_uint32), ("dict_id", C.c_uint32),
                ("block_size", C.c_uint32), ("seek", C.c_uint32), ("eof_at", C.c_uint64), ("rsv", C.c_uint64 * 3)]


class Shape(C.Structure):  # zrs_shape_t
    _fields_ = [(n, C.c_uint32) for n in ("J", "n_jobs", "slot_stride", "chunks")] + \
               [(n, C.c_uint64) for n in ("o_jobs", "o_status", "o_gather", "o_stage", "bytes")]


def load_shim(tmp_path_factory):
    P, U32, U64, I = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    S = cshim.build_shim(tmp_path_factory, "rangesv_shuffle", "ranges/rangesv_shuffle_shim.c")
    S.rs_gather_size.restype = C.c_size_t
    S.rs_index_size.restype, S.rs_index_size.argtypes = U64, [U32]
    S.rs_open.restype, S.rs_open.argtypes = None, [C.c_char_p, U64, U32, U32, P]
    S.rs_shape.argtypes = [U32, U64, U32, C.POINTER(Shape)]
    S.rs_zsh_index.restype, S.rs_zsh_index.argtypes = U64, [U64, U64, U32, U32]
    S.rs_stored_archive.restype, S.rs_stored_archive.argtypes = U64, [C.c_char_p, U64, U32, I, P, U64]
    S.rs_jobs.restype, S.rs_jobs.argtypes = None, [P, U64, U64, U64, U32, U64, U64, U32, U64, U64, P]
    S.rs_verdict.restype, S.rs_verdict.argtypes = C.c_int64, [P, U64, U64, U64, U32, P, U64, U64, U32]
    S.rs_zrv_verdict.restype, S.rs_zrv_verdict.argtypes = C.c_int64, [P, U64, U64, U64, U32, P, U64, U64, U32, I, U32]
    S.rs_plan_pairs.restype, S.rs_plan_pairs.argtypes = C.c_int64, [U32, U32, U32, P, P, U32, C.POINTER(U64)]
    S.rs_call.argtypes = [U64, P, P, P, P, U32, U64, U32, U32, I, U32, P, P, P, U32, U32, P, P, P, P, C.POINTER(U32)]
    return S


def open_index(shim, comp, bs, max_blocks):
    """zr_open_serial -> (the index header, the index buffer, comp_offsets)"""
    buf = (C.c_uint8 * int(shim.rs_index_size(max_blocks)))()
    C.memset(buf, 0xEE, len(buf))
    shim.rs_open(comp, len(comp), bs, max_blocks, buf)
    ix = Index.from_buffer_copy(bytes(buf[:64]))
    offs = [int(x) for x in np.frombuffer(bytes(buf), dtype="<u8", offset=64, count=ix.nb + 1)] if ix.status == 0 else []
    return ix, buf, offs


def stored_archive(shim, data, bs, checksum=False):
    """the seekable archive of stored blocks of `data` (tests/container/stored_archive.h)"""
    out = (C.c_uint8 * (len(data) + 16 * (len(data) // bs + 2) + 64))()
    n = int(shim.rs_stored_archive(data, len(data), bs, int(checksum), out, len(out)))
    assert n > 0
    return bytes(out[:n])


class Blocks:
    """what the decode launch answers for every block of the index: `decoded` (what the archive decodes to: the shuffled bytes) cut
    into blocks, each with its length as status; `status` overrides those of some blocks"""

    def __init__(self, decoded, ix, status=None):
        bs = ix.block_size
        st = [min(bs, ix.total - b * bs) for b in range(ix.nb)]
        for b, v in (status or {}).items():
            st[b] = v
        self.bytes = np.frombuffer(decoded.ljust(ix.nb * bs, b"\0") + b"\0" * 64, dtype=np.uint8)
        self.at = np.arange(ix.nb + 1, dtype=np.uint64) * bs
        self.st = np.array(st + [0], dtype=np.int32)
        self.n = ix.nb


def replay(shim, comp_size, buf, ranges, max_len, E, bs, blocks, have_dict=0, have_id=0, shift=0):
    """ranges: [(offset, len, kind)], kind 0 a buffer of its own, 1 a zero base, 2 a base whose end wraps
    -> results, the ranges' bytes, how often each byte was stored (arrays), flags, stray stores"""
    n = len(ranges)
    offs = np.array([a for a, _, _ in ranges], dtype=np.uint64)
    lens = np.array([m for _, m, _ in ranges], dtype=np.uint64)
    kinds = np.array([k for _, _, k in ranges], dtype=np.uint32)
    results, flags = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.uint32)
    out, hits = np.zeros(int(lens.sum()) + 1, dtype=np.uint8), np.zeros(int(lens.sum()) + 1, dtype=np.uint8)
    stray = C.c_uint32(0)
    rc = shim.rs_call(comp_size, buf, offs.ctypes.data, lens.ctypes.data, kinds.ctypes.data, n, max_len, E, bs, have_dict, have_id,
                      blocks.bytes.ctypes.data, blocks.at.ctypes.data, blocks.st.ctypes.data, blocks.n, shift, results.ctypes.data,
                      out.ctypes.data, hits.ctypes.data, flags.ctypes.data, C.byref(stray))
    assert rc == 0, rc
    cuts = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    return ([int(x) for x in results], [out[cuts[i]:cuts[i + 1]] for i in range(n)], [hits[cuts[i]:cuts[i + 1]] for i in range(n)],
            [int(f) for f in flags], stray.value)


# ---------------------------------------------------------------- on the GPU
GROUP = 8   # ranges per torch allocation


def open_device(gpu, arc, n_arc, bs, max_blocks, stream=None):
    import torch
    s = torch.cuda.current_stream() if stream is None else stream
    isz = gpu.seekable_index_size(max_blocks)
    with torch.cuda.stream(s):
        index = torch.full(((isz + 7) // 8,), -1, dtype=torch.int64, device="cuda")
        gpu.seekable_open_device(arc.data_ptr(), n_arc, bs, max_blocks, index.data_ptr(), isz, s.cuda_stream)
    return index


def index_status(index):
    return int(index[:1].cpu().numpy().view(np.int32)[0])


class Dests:
    """One torch allocation per GROUP ranges, filled with the pattern; range i's destination starts CANARY + k behind the previous
    one's end (or the allocation's start), k making base = offset (mod 16) for even i and cycling 0..15 for odd i. kinds[i]:
    None, ZERO_BASE or WRAP: what the table says instead of that address (the allocation is judged all the same)."""

    def __init__(self, ranges, kinds=None, stream=None):
        import torch
        s = torch.cuda.current_stream() if stream is None else stream
        self.ranges, self.kinds = ranges, kinds or [None] * len(ranges)
        self.tensors, self.where = [], []
        for g in range(0, len(ranges), GROUP):
            at, offs = 0, []
            for i in range(g, min(g + GROUP, len(ranges))):
                a, n = ranges[i]
                at += CANARY
                k = (a - at) % 16 if i % 2 == 0 else (i >> 1) % 16   # (torch allocations are at least 16-byte aligned, asserted below)
                offs.append(at + k)
                at += k + n
            with torch.cuda.stream(s):
                t = torch.from_numpy(pattern(at + CANARY)).to("cuda")
            assert t.data_ptr() % 16 == 0
            self.tensors.append(t)
            self.where += [(len(self.tensors) - 1, o) for o in offs]

    def table(self, gpu):
        t = np.zeros(max(len(self.ranges), 1), dtype=gpu.RANGEV_DTYPE)
        for i, ((a, n), kind, (ti, o)) in enumerate(zip(self.ranges, self.kinds, self.where)):
            base = self.tensors[ti].data_ptr() + o
            t[i] = (a, n, {None: base, ZERO_BASE: 0, WRAP: M64 - n // 2}[kind])
        return t

    def check(self, results, data, expect, what, undefined=()):
        """results[i] == expect(i, a, n); a valid range's bytes are the plain source's; the pattern everywhere else. undefined: the
        ranges that fail by a covered block, whose own bytes [base, base + len) the contract leaves undefined. -> the valid ranges"""
        host = [t.cpu().numpy() for t in self.tensors]
        keep = [np.zeros(len(h), dtype=bool) for h in host]
        n_valid = 0
        for i, ((a, n), rc, (ti, o)) in enumerate(zip(self.ranges, results, self.where)):
            exp = expect(i, a, n)
            assert rc == exp, (what, i, a, n, self.kinds[i], rc, exp)
            if i in undefined:
                assert rc < 0, (what, i, rc)
                keep[ti][o: o + n] = True
            elif rc == n and n:
                assert host[ti][o: o + n].tobytes() == data[a: a + n], (what, i, a, n, o % 16)
                keep[ti][o: o + n] = True
                n_valid += 1
        for h, k in zip(host, keep):
            assert np.array_equal(h[~k], pattern(len(h))[~k]), what   # canaries, gaps, refused and failed-before-decode ranges
        return n_valid


def fetch(gpu, arc, n_arc, index, table, n, max_len, E, bs, stream=None, dict_=None, sync=True, d_ranges=None):
    """-> the results as a list (sync) or (res, work, d_ranges) to keep alive"""
    import torch
    s = torch.cuda.current_stream() if stream is None else stream
    ws = gpu.decompress_rangesv_shuffle_device_work_size(n, max_len, bs)
    assert ws > 0
    with torch.cuda.stream(s):
        work = torch.empty(ws + 1, dtype=torch.uint8, device="cuda")
        res = torch.full((max(n, 1),), UNSET, dtype=torch.int64, device="cuda")
        if d_ranges is None:
            d_ranges = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
        gpu.decompress_rangesv_shuffle_device(arc.data_ptr(), n_arc, index.data_ptr(), d_ranges.data_ptr(), n, max_len, E, bs,
                                              work.data_ptr() + 1, ws, res.data_ptr(), dict_, s.cuda_stream)   # (an odd work address)
    if not sync:
        return res, work, d_ranges
    s.synchronize()
    return [int(x) for x in res.cpu().numpy()[:n]]


def host_expect(host, max_len, kinds=None):
    """zxc_seekable_decompress_range(offset, len, capacity = len) of this library on a host copy of the archive, with rangesv's two
    departures: len > max_len or a wrapping base -> DST_TOO_SMALL, a zero base -> NULL_INPUT"""
    def expect(i, a, n):
        kind = kinds[i] if kinds else None
        if n == 0:
            return 0
        if n > max_len or kind == WRAP:
            return ERR["DST_TOO_SMALL"]
        if kind == ZERO_BASE:
            return ERR["NULL_INPUT"]
        return host.decompress_range(a, n, raise_on_error=False)[0]
    return expect
