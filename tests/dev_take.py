"""What the GPU tests of the take family share (decompress_begin_device / _begin_dict_device, take, takev, end): the archives, the
one-shot reference, the begin of a session, and its two front ends: TakeSession hands over pieces, each a tensor of its own,
TakevSession tables of entries that are slices of one tensor per call. A plain module next to the tests, imported the way devtest
is."""
import numpy as np

from devtest import PAD, UNSET, pattern, to_dev

FRONT = 256   # pattern bytes in front of a piece (keeps an aligned piece 16-byte aligned)
CANARY = 256  # ... and behind it
GAP = 64      # canary bytes between two entries of a takev
BS = 4096

_ONE = {}


def oneshot(gpu, arc, cap, bs, checksum, dd=None):
    """decompress_device / decompress_dict_device -> (result word, the bytes it wrote when it succeeded); once per case"""
    import torch
    key = (arc, cap, bs, checksum, id(dd))
    if key not in _ONE:
        d_arc = to_dev(arc, PAD)
        ws = gpu.decompress_device_work_size(len(arc), cap, bs)
        work = torch.empty(max(ws, 1), dtype=torch.uint8, device="cuda")
        dst = torch.from_numpy(pattern(cap + CANARY)).to("cuda")
        res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        if dd is None:
            gpu.decompress_device(d_arc.data_ptr(), len(arc), dst.data_ptr(), cap, bs, work.data_ptr(), ws, res.data_ptr(), checksum, st)
        else:
            gpu.decompress_dict_device(d_arc.data_ptr(), len(arc), dst.data_ptr(), cap, bs, dd.tup, work.data_ptr(), ws, res.data_ptr(),
                                       checksum, st)
        torch.cuda.synchronize()
        rc = int(res.item())
        assert rc != UNSET
        _ONE[key] = (rc, bytes(dst[:rc].cpu().numpy()) if rc >= 0 else None)
    return _ONE[key]


def archive(gpu, data, level=3, bs=BS, seekable=True, checksum=True):
    return gpu.compress(data, level, bs, seekable, checksum)


def blocks_at(arc, checksum=True):
    at, out = 16, []
    while arc[at] != 255:
        n = 8 + int.from_bytes(arc[at + 3: at + 7], "little") + (4 if checksum else 0)
        out.append((at, n))
        at += n
    return out


class _Begun:
    """a session begun on a stream, with its archive, work area (at an odd address) and result word. with_dict_begin: the _dict
    begin although there is no dictionary."""

    def __init__(self, gpu, arc, cap, bs, max_piece, checksum, dd, stream=None, with_dict_begin=False):
        import torch
        self.gpu, self.cap, self.bs = gpu, cap, bs
        self.stream = torch.cuda.current_stream() if stream is None else stream
        self.st = self.stream.cuda_stream
        self.max_piece = max(bs, cap) if max_piece is None else max_piece
        ws = gpu.decompress_take_device_work_size(len(arc), cap, self.max_piece, bs)
        assert ws > 0
        with torch.cuda.stream(self.stream):
            self.arc = to_dev(arc, PAD)
            self.work = torch.empty(ws + 1, dtype=torch.uint8, device="cuda")
            self.res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        if dd is not None or with_dict_begin:
            self.s = gpu.decompress_begin_dict_device(self.arc.data_ptr(), len(arc), cap, self.max_piece, bs, dd.tup if dd else None,
                                                      self.work.data_ptr() + 1, ws, checksum, self.st)
        else:
            self.s = gpu.decompress_begin_device(self.arc.data_ptr(), len(arc), cap, self.max_piece, bs, self.work.data_ptr() + 1, ws, checksum,
                                                 self.st)

    def end(self):
        self.s.end(self.res.data_ptr(), self.st)


class TakeSession(_Begun):
    """every take gets a tensor of its own"""

    def __init__(self, gpu, arc, cap, bs=BS, max_piece=None, checksum=False, aligned=True, dd=None, stream=None, with_dict_begin=False):
        super().__init__(gpu, arc, cap, bs, max_piece, checksum, dd, stream, with_dict_begin)
        self.aligned, self.pieces = aligned, []

    def take(self, n, k=0):
        import torch
        off = FRONT + (0 if self.aligned else 1 + 2 * (k % 7))
        with torch.cuda.stream(self.stream):
            t = torch.from_numpy(pattern(off + n + CANARY)).to("cuda")
        self.s.take(t.data_ptr() + off, n, self.st)  # (a refused take raises in front of the append below)
        self.pieces.append((t, off, n))

    def result(self):
        """-> (result word, the pieces' bytes concatenated); the pattern in front of every piece and the canary behind it hold"""
        self.stream.synchronize()
        rc, out = int(self.res.item()), []
        for k, (t, off, n) in enumerate(self.pieces):
            got, whole = t.cpu().numpy(), pattern(off + n + CANARY)
            assert (got[:off] == whole[:off]).all(), "bytes in front of piece %d changed" % k
            assert (got[off + n:] == whole[off + n:]).all(), "bytes behind piece %d changed" % k
            out.append(bytes(got[off: off + n]))
        return rc, b"".join(out)

    def untouched(self):
        return all((t.cpu().numpy() == pattern(off + n + CANARY)).all() for t, off, n in self.pieces)


class TakevSession(_Begun):
    """on the current stream; every call gets a tensor of its own, whose entries are slices with canaries around each"""

    def __init__(self, gpu, arc, cap, bs=BS, max_piece=None, checksum=False, dd=None):
        from zxc_amd.api import IOV_DTYPE
        super().__init__(gpu, arc, cap, bs, max_piece, checksum, dd)
        self.calls, self.IOV = [], IOV_DTYPE

    def scratch(self, n_iov):
        import torch
        ss = self.gpu.decompress_takev_device_scratch_size(n_iov, self.max_piece, self.bs)
        assert ss > 0
        return torch.empty(ss + 3, dtype=torch.uint8, device="cuda"), ss

    def layout(self, lens, aligned):
        """-> (tensor of pattern bytes, [(offset, len)]): the entries with GAP or more canary bytes around each"""
        import torch
        at, places = GAP, []
        for k, n in enumerate(lens):
            at = (at + 15) // 16 * 16 + (0 if aligned else 1 + 2 * (k % 7))
            places.append((at, n))
            at += n + GAP
        return torch.from_numpy(pattern(at + GAP)).to("cuda"), places

    def takev(self, lens, aligned=True, total=None, mutate=None, scratch=None, via_stream_copy=False):
        """one takev over entries of these lengths; mutate(table) may damage the table (never in a way that is dereferenced)"""
        import torch
        t, places = self.layout(lens, aligned)
        table = np.zeros(max(len(lens), 1), dtype=self.IOV)
        for i, (off, n) in enumerate(places):
            table[i] = (t.data_ptr() + off if n else 0, n)  # an empty entry's base is not looked at
        if mutate:
            mutate(table)
        raw = torch.from_numpy(table.view(np.uint8).copy())
        pinned = None
        if via_stream_copy:  # the table is written on the stream by a copy enqueued just before the call
            d_iov = torch.zeros(len(raw), dtype=torch.uint8, device="cuda")
            pinned = raw.pin_memory()
            d_iov.copy_(pinned, non_blocking=True)
        else:
            d_iov = raw.to("cuda")
        sc, ss = scratch if scratch is not None else self.scratch(len(lens))
        self.s.takev(d_iov.data_ptr(), len(lens), sum(lens) if total is None else total, sc.data_ptr() + 3, ss, self.st)
        self.calls.append((t, places, (d_iov, pinned), sc))
        return len(self.calls) - 1

    def take(self, n, aligned=True):
        t, places = self.layout([n], aligned)
        self.s.take(t.data_ptr() + places[0][0], n, self.st)
        self.calls.append((t, places, None, None))
        return len(self.calls) - 1

    def result(self):
        """-> (result word, per call the entries' bytes concatenated); every byte outside the entries holds"""
        import torch
        torch.cuda.synchronize()
        rc, out = int(self.res.item()), []
        for k, (t, places, _, _) in enumerate(self.calls):
            got = t.cpu().numpy()
            keep = np.ones(len(got), dtype=bool)
            for off, n in places:
                keep[off: off + n] = False
            assert (got[keep] == pattern(len(got))[keep]).all(), "bytes outside the entries of call %d changed" % k
            out.append(b"".join(bytes(got[off: off + n]) for off, n in places))
        return rc, out

    def untouched(self, k):
        t = self.calls[k][0]
        return bool((t.cpu().numpy() == pattern(len(t))).all())
