"""What the tests of the unshufflev calls share (tests/test_decompress_shufflev_device_cpu.py,
tests/test_gpu_decompress_shufflev_device.py): the rules shim (tests/shuffle/unshufflev_shim.c), and on the GPU the destination
table, entries that are slices of one tensor with canaries around each in the style of dev_take.TakevSession.layout, and the two
calls on it with guarded source, scratch and work area. The cut lists are shufflev_support's. A plain module next to the tests,
imported the way devtest is."""
import ctypes as C

import numpy as np

import cshim
import shuffle_support as ss
from dev_take import GAP
from devtest import PAD, UNSET, pattern

BS = ss.BS


# ---------------------------------------------------------------- the rules, compiled with the host C compiler
def load_shim(tmp_path_factory):
    P, U32, U64 = C.c_void_p, C.c_uint32, C.c_uint64
    S = cshim.build_shim(tmp_path_factory, "unshufflev", "shuffle/unshufflev_shim.c")
    S.uvs_scratch_size.restype = S.uvs_work_size.restype = U64
    S.uvs_scratch_size.argtypes = [U32]
    S.uvs_work_size.argtypes = [U64, U32]
    S.uvs_result.restype, S.uvs_result.argtypes = C.c_int64, [C.c_int, C.c_int64, U64]
    S.uvs_check.argtypes = [P, P, U32, U64, U32, U32, U64, P]
    S.uvs_check_bad.argtypes = [P, P, U32, U64, U32, U32, U32, U64]
    return S


# ---------------------------------------------------------------- on the GPU
class DestTable:
    """entries of these lengths as slices of one tensor of pattern bytes with GAP or more canary bytes around each, 16-byte aligned
    or at odd addresses, and their table in device memory, both uploaded on `stream`. An empty entry's base is 0 or 0x10 and never
    looked at. fix(rows) may change the table's rows (never in a way that is dereferenced)."""

    def __init__(self, gpu, lens, stream, aligned=False, fix=None, k0=0):
        import torch
        at, self.places, rows = GAP, [], []
        for k, n in enumerate(lens):
            at = (at + 15) // 16 * 16 + (0 if aligned else 1 + 2 * ((k0 + k) % 7))
            self.places.append((at, n))
            at += n + GAP
        self.size = at + GAP
        with torch.cuda.stream(stream):
            self.t = torch.from_numpy(pattern(self.size)).to("cuda")
            for k, (off, n) in enumerate(self.places):
                rows.append((self.t.data_ptr() + off, n) if n else (0 if k % 2 else 0x10, 0))
            if fix:
                fix(rows)
            self.host = np.array(rows if rows else [(0, 0)], dtype=gpu.IOV_DTYPE)
            self.dev = torch.from_numpy(self.host.view(np.uint8).copy()).to("cuda")
        self.n, self.total = len(lens), sum(lens)

    def read(self):
        """-> the entries' bytes, concatenated; every byte outside the entries is what it was"""
        got = self.t.cpu().numpy()
        keep = np.ones(len(got), dtype=bool)
        for off, n in self.places:
            keep[off: off + n] = False
        assert (got[keep] == pattern(self.size)[keep]).all(), "bytes outside the entries changed"
        return b"".join(bytes(got[off: off + n]) for off, n in self.places)

    def untouched(self):
        return bool((self.t.cpu().numpy() == pattern(self.size)).all())


class UnshuffleV:
    """unshufflev_device enqueued on a stream: the source at an odd address between canaries, the scratch too. total / fix: the
    promise and the change of the table's rows of a bad table. result() synchronises -> (the status word, the entries' bytes)"""

    def __init__(self, gpu, y, lens, E, unit=BS, src_off=1, total=None, fix=None, stream=None, aligned=False, k0=0):
        import torch
        self.st = torch.cuda.current_stream() if stream is None else stream
        self.y = y
        self.tb = DestTable(gpu, lens, self.st, aligned, fix, k0)
        total = self.tb.total if total is None else total
        self.src = ss.Guarded(len(y), src_off, y, self.st)
        size = gpu.unshufflev_device_scratch_size(self.tb.n)
        assert size == gpu.shufflev_device_scratch_size(self.tb.n) > 0
        self.scratch = ss.Guarded(size, 1, None, self.st)
        with torch.cuda.stream(self.st):
            self.res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        gpu.unshufflev_device(self.src.ptr if total else 0, self.tb.dev.data_ptr(), self.tb.n, total, E, unit, self.scratch.ptr, size,
                              self.res.data_ptr(), self.st.cuda_stream)

    def result(self):
        self.st.synchronize()
        self.scratch.read()                                           # nothing outside d_scratch[0, scratch_size)
        assert self.src.read() == self.y, "the source changed"
        return int(self.res.item()), self.tb.read()                   # nothing outside the entries


class DecompressV:
    """decompress_shufflev_device enqueued on a stream into a DestTable of `lens`, the work area at an odd address between canaries
    (work: the Guarded work area of an earlier call instead of one of its own); result() synchronises -> (result word, the
    entries' bytes)"""

    def __init__(self, gpu, arc, lens, E, max_piece, bs=BS, checksum=False, dd=None, stream=None, total=None, fix=None, work=None,
                 aligned=False, k0=0):
        import torch
        self.st = torch.cuda.current_stream() if stream is None else stream
        self.tb = DestTable(gpu, lens, self.st, aligned, fix, k0)
        total = self.tb.total if total is None else total
        with torch.cuda.stream(self.st):
            self.arc = torch.from_numpy(np.frombuffer(arc + b"\xA5" * PAD, dtype=np.uint8).copy()).to("cuda")
            self.res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        ws = gpu.decompress_shufflev_device_work_size(self.tb.n, len(arc), total, max_piece, bs)
        assert ws > 0
        self.work = ss.Guarded(ws, 3, None, self.st) if work is None else work
        assert self.work.n >= ws
        gpu.decompress_shufflev_device(self.arc.data_ptr(), len(arc), self.tb.dev.data_ptr(), self.tb.n, total, E, bs, self.work.ptr, ws,
                                       self.res.data_ptr(), max_piece, dd.tup if dd else None, checksum, self.st.cuda_stream)

    def result(self):
        self.st.synchronize()
        self.work.read()                                              # nothing outside d_work[0, work_size)
        return int(self.res.item()), self.tb.read()                   # nothing outside the entries
