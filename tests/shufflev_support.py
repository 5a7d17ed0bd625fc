"""What the tests of the shufflev calls share (tests/test_compress_shufflev_device_cpu.py, tests/test_gpu_compress_shufflev_device.py):
the lists of entry lengths a source is cut by, the rules shim (tests/shuffle/shufflev_shim.c), and on the GPU the two calls on a
dev_append.Table with guarded destination, scratch and work area. A plain module next to the tests, imported the way devtest is."""
import ctypes as C

import numpy as np

import cshim
import dev_append
import shuffle_support as ss
from devtest import UNSET

ELEMS = (2, 4, 8)
BS = ss.BS
ORDERS_TOTAL = sum(dev_append.LENS)


def cuts(total, E, seed=0):
    """name -> entry lengths that add up to total: one entry; multiples of 16 E (the last entry takes what is left); entries of
    16 E + 1 bytes, so that the boundary drifts through every byte of a group; entries of 1 to 7 bytes; empty entries first, doubled
    in the middle and last; more than 1024 entries, a second tile of the scan; a cut on a unit boundary; one on the boundary of a
    chunk of two units"""
    rng = np.random.default_rng(1000 * E + seed)

    def fill(draw):
        out, left = [], total
        while left:
            out.append(min(draw(), left))
            left -= out[-1]
        return out

    return {
        "one entry": [total],
        "multiples of 16 E": fill(lambda: 16 * E * int(rng.integers(1, 41))),
        "16 E + 1": fill(lambda: 16 * E + 1),
        "1 to 7 bytes": fill(lambda: int(rng.integers(1, 8))),
        "empty entries": [0, total // 3, 0, 0, total - total // 3, 0],
        "more than 1024 entries": [total // 1100 + (r < total % 1100) for r in range(1100)],
        "a unit boundary": [min(total, BS), total - min(total, BS)],
        "a chunk boundary": [min(total, 2 * BS), total - min(total, 2 * BS)],
    }


def starts(lens):
    """the offset of every entry in the concatenation"""
    return [int(v) for v in np.concatenate(([0], np.cumsum(lens)[:-1]))] if lens else []


def bad_table(lens, case):
    """one of dev_append.bad_table_cases() for a table of these lengths -> (the promise, the change of its rows, the error's name)"""
    delta, fix, want = dev_append.bad_table_cases()[case]
    return (lens[1] - 1 if delta is None else sum(lens) + delta), fix, want


# ---------------------------------------------------------------- the rules, compiled with the host C compiler
def load_shim(tmp_path_factory):
    P, U32, U64 = C.c_void_p, C.c_uint32, C.c_uint64
    S = cshim.build_shim(tmp_path_factory, "shufflev", "shuffle/shufflev_shim.c")
    S.svs_scratch_size.restype = S.svs_scratch_bound.restype = S.svs_work_size.restype = U64
    S.svs_scratch_size.argtypes = S.svs_scratch_bound.argtypes = [U32]
    S.svs_work_size.argtypes = [U64, U32]
    S.svs_result.restype, S.svs_result.argtypes = C.c_int64, [C.c_int, C.c_int64]
    S.svs_check.argtypes = [P, P, U32, U64, U32, U32, U64, P]
    S.svs_check_bad.argtypes = [P, P, U32, U64, U32, U32, U32, U64]
    return S


# ---------------------------------------------------------------- on the GPU
class ShuffleV:
    """shufflev_device enqueued on a stream over a dev_append.Table of `parts`; destination and scratch at odd addresses between
    canaries. total / fix: the promise and the change of the table's rows of a bad table. result() synchronises -> (the status
    word, the destination's bytes)"""

    def __init__(self, gpu, parts, E, unit=BS, dst_off=1, total=None, fix=None, stream=None, k0=0):
        import torch
        self.st = torch.cuda.current_stream() if stream is None else stream
        self.tb = dev_append.Table(gpu, parts, self.st, k0, fix)
        total = self.tb.total if total is None else total
        self.dst = ss.Guarded(total, dst_off, None, self.st)
        size = gpu.shufflev_device_scratch_size(self.tb.n)
        assert 0 < size <= 8 * (self.tb.n + 1) + 16 * -(-self.tb.n // 1024) + 4096 + 256
        self.scratch = ss.Guarded(size, 1, None, self.st)
        with torch.cuda.stream(self.st):
            self.res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        gpu.shufflev_device(self.tb.dev.data_ptr(), self.tb.n, total, self.dst.ptr if total else 0, E, unit, self.scratch.ptr, size,
                            self.res.data_ptr(), self.st.cuda_stream)

    def result(self):
        self.st.synchronize()
        self.scratch.read()                                           # nothing outside d_scratch[0, scratch_size)
        return int(self.res.item()), self.dst.read()                  # nothing outside d_dst[0, total)


class CompressV:
    """compress_shufflev_device enqueued on a stream over a dev_append.Table of `parts`, on guarded buffers (work: the Guarded work
    area of an earlier call instead of one of its own); result() synchronises -> (result word, archive bytes or None)"""

    def __init__(self, gpu, parts, E, cap, max_piece, level=3, bs=BS, seekable=False, checksum=False, dd=None, dst_off=1, stream=None,
                 total=None, fix=None, work=None, k0=0):
        import torch
        self.cap = cap
        self.st = torch.cuda.current_stream() if stream is None else stream
        self.tb = dev_append.Table(gpu, parts, self.st, k0, fix)
        total = self.tb.total if total is None else total
        self.dst = ss.Guarded(cap, dst_off, None, self.st)
        ws = gpu.compress_shufflev_device_work_size(self.tb.n, total, max_piece, dd.tup[1] if dd else 0, level, bs, seekable, checksum)
        assert ws > 0
        self.work = ss.Guarded(ws, 1, None, self.st) if work is None else work
        assert self.work.n >= ws
        with torch.cuda.stream(self.st):
            self.res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        gpu.compress_shufflev_device(self.tb.dev.data_ptr(), self.tb.n, total, E, self.dst.ptr, cap, self.work.ptr, ws, self.res.data_ptr(),
                                     max_piece, dd.tup if dd else None, level, bs, seekable, checksum, self.st.cuda_stream)

    def result(self):
        self.st.synchronize()
        rc = int(self.res.item())
        arc = self.dst.read()                                         # nothing in front of d_dst or at and past dst_capacity
        self.work.read()                                              # nothing outside d_work[0, work_size)
        if rc > 0:
            at = 256 + self.dst.off
            assert rc <= self.cap and arc[rc:] == self.dst.host[at + rc: at + self.cap].tobytes(), "bytes behind the archive changed"
        return rc, arc[:rc] if rc > 0 else None


def compress_shufflev(gpu, parts, E, cap, max_piece, **kw):
    """-> (result word or the synchronous error, archive bytes or None)"""
    try:
        c = CompressV(gpu, parts, E, cap, max_piece, **kw)
    except gpu.ZxcError as e:
        return e.code, None
    return c.result()
