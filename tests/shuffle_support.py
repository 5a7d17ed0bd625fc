"""What the tests of the byte-shuffle calls share (tests/test_shuffle_device_cpu.py, tests/test_gpu_shuffle_device.py): the numpy
transform they compare with, the sizes and the typed payloads, and on the GPU the guarded buffers and the two archive calls. A plain
module next to the tests, imported the way devtest is."""
import numpy as np

from devtest import CANARY, PAD, UNSET, pattern

BS = 4096


def np_shuffle(x, E, unit):
    """x: uint8 array -> per unit of `unit` bytes, the (q, E) matrix of its whole elements transposed; the rest of the unit copied"""
    out = x.copy()
    for at in range(0, len(x), unit):
        m = min(unit, len(x) - at)
        q = m // E
        out[at: at + q * E] = x[at: at + q * E].reshape(q, E).T.reshape(-1)
    return out


def np_unshuffle(y, E, unit):
    out = y.copy()
    for at in range(0, len(y), unit):
        m = min(unit, len(y) - at)
        q = m // E
        out[at: at + q * E] = y[at: at + q * E].reshape(E, q).T.reshape(-1)
    return out


def sizes(E):
    """the sizes of the issue: nothing, less than an element, an element and one more byte, around a unit, two units and a ragged
    tail with r != 0, nine units and a tail (more than one wavefront, several chunks)"""
    return sorted({0, 1, E - 1, E, E + 1, 4095, 4096, 4097, 2 * 4096 + 3 * E + 1, 9 * 4096 + 1000})


def tensor_bytes(n, E, seed):
    """the first n bytes of a seeded typed tensor: bf16 (E = 2) or fp32 (E = 4) weights N(0, 0.02), int64 ids below 50000 (E = 8)"""
    rng = np.random.default_rng(seed)
    count = n // E + 1
    if E == 8:
        raw = rng.integers(0, 50000, count, dtype=np.int64).view(np.uint8)
    else:
        w = (rng.standard_normal(count) * 0.02).astype(np.float32)
        raw = w.view(np.uint8) if E == 4 else (w.view(np.uint32) >> 16).astype(np.uint16).view(np.uint8)
    return raw[:n].tobytes()


# ---------------------------------------------------------------- on the GPU
class Guarded:
    """n bytes at offset `off` (mod 16 what the test asks) of a pattern-filled allocation with CANARY bytes behind them"""

    def __init__(self, n, off, data=None, stream=None):
        import torch
        self.n, self.off = n, off
        host = pattern(256 + off + n + CANARY).copy()
        if data is not None:
            host[256 + off: 256 + off + n] = np.frombuffer(data, dtype=np.uint8)
        self.host = host
        if stream is None:
            self.t = torch.from_numpy(host.copy()).to("cuda")
        else:
            with torch.cuda.stream(stream):
                self.t = torch.from_numpy(host.copy()).to("cuda")
        assert self.t.data_ptr() % 256 == 0
        self.ptr = self.t.data_ptr() + 256 + off

    def read(self):
        """-> the n bytes; everything around them is what it was"""
        got = self.t.cpu().numpy()
        lo, hi = 256 + self.off, 256 + self.off + self.n
        assert (got[:lo] == self.host[:lo]).all(), "bytes in front of the buffer changed"
        assert (got[hi:] == self.host[hi:]).all(), "bytes behind the buffer changed"
        return got[lo:hi].tobytes()


class Compress:
    """compress_shuffle_device enqueued on a stream, on guarded buffers; result() synchronises -> (result word, archive bytes or
    None)"""

    def __init__(self, gpu, x, E, cap, max_piece, level=3, bs=BS, seekable=False, checksum=False, dd=None, src_off=0, dst_off=0, stream=None):
        import torch
        self.x, self.cap = x, cap
        self.st = torch.cuda.current_stream() if stream is None else stream
        self.src, self.dst = Guarded(len(x), src_off, x, self.st), Guarded(cap, dst_off, None, self.st)
        ws = gpu.compress_shuffle_device_work_size(len(x), max_piece, dd.tup[1] if dd else 0, level, bs, seekable, checksum)
        assert ws > 0
        self.work = Guarded(ws, 1, None, self.st)
        with torch.cuda.stream(self.st):
            self.res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        gpu.compress_shuffle_device(self.src.ptr, len(x), E, self.dst.ptr, cap, self.work.ptr, ws, self.res.data_ptr(), max_piece,
                                    dd.tup if dd else None, level, bs, seekable, checksum, self.st.cuda_stream)

    def result(self):
        self.st.synchronize()
        rc = int(self.res.item())
        assert self.src.read() == self.x, "the source changed"
        arc = self.dst.read()                                         # nothing in front of d_dst or at and past dst_capacity
        self.work.read()                                              # nothing outside d_work[0, work_size)
        if rc > 0:
            at = 256 + self.dst.off
            assert rc <= self.cap and arc[rc:] == self.dst.host[at + rc: at + self.cap].tobytes(), "bytes behind the archive changed"
        return rc, arc[:rc] if rc > 0 else None


def compress_shuffle(gpu, x, E, cap, max_piece, **kw):
    """-> (result word or the synchronous error, archive bytes or None)"""
    try:
        c = Compress(gpu, x, E, cap, max_piece, **kw)
    except gpu.ZxcError as e:
        return e.code, None
    return c.result()


class Decompress:
    """decompress_shuffle_device enqueued on a stream; result() synchronises -> (result word, the destination's bytes)"""

    def __init__(self, gpu, arc, n, E, max_piece, bs=BS, checksum=False, dd=None, dst_off=0, stream=None):
        import torch
        self.st = torch.cuda.current_stream() if stream is None else stream
        with torch.cuda.stream(self.st):
            self.arc = torch.from_numpy(np.frombuffer(arc + b"\xA5" * PAD, dtype=np.uint8).copy()).to("cuda")
            self.res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        self.dst = Guarded(n, dst_off, None, self.st)
        ws = gpu.decompress_shuffle_device_work_size(len(arc), n, max_piece, bs)
        assert ws > 0
        self.work = Guarded(ws, 3, None, self.st)
        gpu.decompress_shuffle_device(self.arc.data_ptr(), len(arc), self.dst.ptr if n else 0, n, E, bs, self.work.ptr, ws, self.res.data_ptr(),
                                      max_piece, dd.tup if dd else None, checksum, self.st.cuda_stream)

    def result(self):
        self.st.synchronize()
        self.work.read()
        return int(self.res.item()), self.dst.read()
