"""What the GPU tests of the append family share (compress_begin_device / _begin_dict_device, append, appendv / appendv_dict, end):
the session with its guarded destination, the scratch and the table of an appendv, the one-shot baselines, the dictionaries and the
entry-length lists. A plain module next to the tests, imported the way devtest is. Which entry points a session, a scratch or a
baseline goes through is the `family` argument, PLAIN or DICT, never inferred from the dictionary: the DICT family is also
reached with no dictionary at all. Each test file binds its family once (plain_session, dict_session, ...)."""
import functools
import os

import numpy as np

import devtest
from conftest import GOLDEN, load_dict
from devtest import CANARY, UNSET, pattern, piece, split

PLAIN, DICT = "plain", "dict"  # compress_begin_device and its siblings, or the _dict entry points
BS = 4096
LENS = (0, 1, 3, 31, 32, 33, 4095, 4096, 4097, 4096 + 31, 4096 + 32, 2 * 4096 + 33, 3 * 4096 + 5)
SCRATCH_CANARY = 256


def text():
    return devtest.text(6 << 20)  # (the text the payloads are cut from)


_DICTS = {}


def dict_of(gpu, size, with_huf=False, seed=0):
    """a dictionary of `size` bytes of the text the payloads are cut from (so that it is used), with or without a shared table.
    Every DevDict made here stays alive in _DICTS: baseline() keys on id(dd), which must never be reused."""
    key = (size, with_huf, seed)
    if key not in _DICTS:
        at = (5 << 20) + 70001 * seed
        _, huf = load_dict(os.path.join(GOLDEN, "conformance", "valid", "dict_text.zxd"))
        _DICTS[key] = devtest.DevDict(gpu, text()[at: at + size], huf if with_huf else None, odd=True)  # at an odd address
    return _DICTS[key]


BASE = {PLAIN: {}, DICT: {}}  # the baselines of each family; a test that made a very large one clears its family's


def baseline(family, gpu, data, dd, cap, level, bs, seekable, checksum):
    """compress_device (PLAIN) or compress_dict_device (DICT) for the whole source -> (result word or the synchronous error, archive
    bytes or None); once per case and process, whichever test module asks"""
    import torch
    assert family == DICT or dd is None
    key = (data, id(dd) if dd is not None else None, cap, level, bs, seekable, checksum)
    if key not in BASE[family]:
        src = torch.frombuffer(bytearray(data + bytes(64)), dtype=torch.uint8).to("cuda")
        if family == DICT:
            ws = gpu.compress_dict_device_work_size(len(data), dd.tup[1] if dd else 0, level, bs, seekable, checksum)
        else:
            ws = gpu.compress_device_work_size(len(data), level, bs, seekable, checksum)
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        dst = torch.from_numpy(pattern(cap + CANARY)).to("cuda")
        res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        sp = torch.cuda.current_stream().cuda_stream
        try:
            if family == DICT:
                gpu.compress_dict_device(src.data_ptr(), len(data), dst.data_ptr(), cap, dd.tup if dd else None, work.data_ptr(), ws,
                                         res.data_ptr(), level, bs, seekable, checksum, sp)
            else:
                gpu.compress_device(src.data_ptr(), len(data), dst.data_ptr(), cap, work.data_ptr(), ws, res.data_ptr(), level, bs, seekable,
                                    checksum, sp)
            torch.cuda.synchronize()
            rc = int(res.item())
        except gpu.ZxcError as e:
            rc = e.code
        BASE[family][key] = (rc, bytes(dst[:rc].cpu().numpy()) if rc > 0 else None)
    return BASE[family][key]


class Table:
    """entries in device memory, each a tensor of its own at an odd offset of a buffer that ends with it, and their table, also in
    device memory (behind one spare byte row: the table itself is 8-byte aligned as its type asks)"""

    def __init__(self, gpu, parts, stream, k0=0, fix=None):
        import torch
        self.keep, rows = [], []
        with torch.cuda.stream(stream):
            for k, data in enumerate(parts):
                if len(data):
                    t, p = piece(data, k0 + k)
                    self.keep.append(t)
                else:
                    p = 0 if k % 2 else 0x10  # an empty entry's base is not looked at
                rows.append((p, len(data)))
            if fix:
                fix(rows)
            self.host = np.array(rows if rows else [(0, 0)], dtype=gpu.IOV_DTYPE)
            self.dev = torch.from_numpy(self.host.view(np.uint8).copy()).to("cuda")
        self.n, self.total = len(rows), sum(len(d) for d in parts)


class Scratch:
    """scratch_size bytes at an odd address, a pattern, with a canary behind them"""

    def __init__(self, family, gpu, n_iov, max_piece, dict_size, level, bs, seekable, checksum, stream):
        import torch
        if family == DICT:
            self.size = gpu.compress_appendv_dict_device_scratch_size(n_iov, max_piece, dict_size, level, bs, seekable, checksum)
        else:
            assert dict_size == 0
            self.size = gpu.compress_appendv_device_scratch_size(n_iov, max_piece, level, bs, seekable, checksum)
        assert self.size > 0
        if dict_size:
            assert self.size <= 8 * (n_iov + 1) + 16 * -(-n_iov // 1024) + 4096  # no images
        with torch.cuda.stream(stream):
            self.t = torch.from_numpy(pattern(1 + self.size + SCRATCH_CANARY)).to("cuda")
        self.ptr = self.t.data_ptr() + 1

    def check(self):
        tail = self.t[1 + self.size:].cpu().numpy()
        assert (tail == pattern(1 + self.size + SCRATCH_CANARY)[1 + self.size:]).all(), "bytes at or past scratch_size changed"


class AppendSession:
    """one session with its destination (pattern, canary, optionally at an odd address), work area at an odd address and result
    word. dict_: the dictionary tuple begin gets, when it is not dd's (DICT only; None: no dictionary through the _dict entry
    points). work: another session's work tensor instead of one of its own."""

    def __init__(self, family, gpu, dd, cap, max_total, max_piece, level=3, bs=BS, seekable=0, checksum=0, odd_dst=0, stream=None, work=None,
                 dict_="dd"):
        import torch
        assert family == DICT or (dd is None and dict_ == "dd")
        self.family, self.gpu, self.cap, self.odd = family, gpu, cap, odd_dst
        self.stream = torch.cuda.current_stream() if stream is None else stream
        self.keep, self.scratches, self.calls = [], [], 0
        tup = (dd.tup if dd else None) if isinstance(dict_, str) else dict_
        self.opt = (max_piece, tup[1] if tup else 0, level, bs, seekable, checksum)
        if family == DICT:
            ws = gpu.compress_append_dict_device_work_size(max_total, max_piece, tup[1] if tup else 0, level, bs, seekable, checksum)
        else:
            ws = gpu.compress_append_device_work_size(max_total, max_piece, level, bs, seekable, checksum)
        assert ws > 0
        with torch.cuda.stream(self.stream):
            self.work = torch.empty(ws + 1, dtype=torch.uint8, device="cuda") if work is None else work
            assert self.work.numel() >= ws + 1
            self.dst = torch.from_numpy(pattern(odd_dst + cap + CANARY)).to("cuda")
            self.res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        if family == DICT:
            self.s = gpu.compress_begin_dict_device(self.dst.data_ptr() + odd_dst, cap, max_total, max_piece, tup, self.work.data_ptr() + 1, ws,
                                                    level, bs, seekable, checksum, self.stream.cuda_stream)
        else:
            self.s = gpu.compress_begin_device(self.dst.data_ptr() + odd_dst, cap, max_total, max_piece, self.work.data_ptr() + 1, ws, level, bs,
                                               seekable, checksum, self.stream.cuda_stream)

    def append(self, data, k=0):
        import torch
        with torch.cuda.stream(self.stream):
            t, p = piece(data, k)
        self.keep.append(t)
        self.s.append(p, len(data), self.stream.cuda_stream)

    def appendv(self, parts, total=None, fix=None, scratch=None):
        """one appendv (PLAIN) or appendv_dict (DICT) over a list of entries (bytes) -> the scratch it used"""
        tb = Table(self.gpu, parts, self.stream, 3 * self.calls, fix)
        sc = scratch or Scratch(self.family, self.gpu, tb.n, *self.opt, self.stream)
        self.keep.append(tb)
        if sc not in self.scratches:
            self.scratches.append(sc)
        self.calls += 1
        call = self.s.appendv_dict if self.family == DICT else self.s.appendv
        call(tb.dev.data_ptr(), tb.n, tb.total if total is None else total, sc.ptr, sc.size, self.stream.cuda_stream)
        return sc

    def end(self):
        self.s.end(self.res.data_ptr(), self.stream.cuda_stream)

    def result(self):
        """-> (result word, archive bytes or None); the pattern in front of the destination and the canary behind the capacity hold,
        and the canary behind every scratch used"""
        self.stream.synchronize()
        rc, dst = int(self.res.item()), self.dst.cpu().numpy()
        whole = pattern(len(dst))
        assert (dst[: self.odd] == whole[: self.odd]).all(), "bytes in front of d_dst changed"
        assert (dst[self.odd + self.cap:] == whole[self.odd + self.cap:]).all(), "bytes at or past dst_capacity changed"
        if rc > 0:
            assert rc <= self.cap
            assert (dst[self.odd + rc:] == whole[self.odd + rc:]).all(), "bytes behind the archive changed"
        for sc in self.scratches:
            sc.check()
        return rc, bytes(dst[self.odd: self.odd + rc]) if rc > 0 else None


# each family under the signature its tests call: the plain ones have no dictionary argument
dict_session = functools.partial(AppendSession, DICT)
dict_scratch = functools.partial(Scratch, DICT)
dict_baseline = functools.partial(baseline, DICT)


def plain_session(gpu, *args, **kw):
    return AppendSession(PLAIN, gpu, None, *args, **kw)


def plain_scratch(gpu, n_iov, max_piece, *rest):
    return Scratch(PLAIN, gpu, n_iov, max_piece, 0, *rest)


def plain_baseline(gpu, data, *rest):
    return baseline(PLAIN, gpu, data, None, *rest)


def cut(data, lens):
    assert sum(lens) == len(data), (sum(lens), len(data))
    return split(data, list(lens))


def run_calls(s, data, calls):
    """calls: a list of entry-length lists (an appendv each) and ints (a plain append each), over data in order; then end
    -> the session's result"""
    at = 0
    for k, c in enumerate(calls):
        n = c if isinstance(c, int) else sum(c)
        if isinstance(c, int):
            s.append(data[at: at + n], k)
        else:
            s.appendv(cut(data[at: at + n], c))
        at += n
    assert at == len(data)
    s.end()
    return s.result()


def orders():
    rng = np.random.default_rng(5)
    out = {"as listed": list(LENS), "reversed": list(LENS)[::-1]}
    for k in range(2):
        out["shuffled %d" % k] = [int(x) for x in rng.permutation(LENS)]
    return out


def bad_table_cases():
    def null_base(rows):
        rows[2] = (0, rows[2][1])

    # name -> (delta of the promise, change of the table's rows, the code end stores)
    return {"sum one below total": (+1, None, "SRC_TOO_SMALL"), "sum one above total": (-1, None, "OVERFLOW"),
            "an entry longer than total": (None, None, "OVERFLOW"), "a zero base with a length": (0, null_base, "NULL_INPUT")}
