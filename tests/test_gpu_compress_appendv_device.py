"""zxc_mi355x_compress_appendv_device on the GPU: one call appends a table of buffers to an append session. The reference value is
always existing code: the archive and the result word zxc_mi355x_compress_device writes for the concatenation with the same
options and capacity; for round trips the unmodified reference decoder. Set-up as in test_gpu_compress_append_device.py, whose
helpers are used: every entry is a tensor of its own at an odd offset inside a buffer that ends with the entry (nothing readable
is promised behind an entry), the destination is a pattern with a canary behind dst_capacity, the table lies in device memory, and
the scratch sits at an odd address with a canary behind scratch_size. Nothing here provokes a fault: every refused input is
refused by status, and a table that breaks a rule names only buffers that exist."""
import numpy as np
import pytest

import devtest
import test_gpu_compress_append_device as A
import test_gpu_compress_append_dict_device as D
from devtest import ERR

pytestmark = pytest.mark.gpu

BS = 4096
LENS = (0, 1, 3, 31, 32, 33, 4095, 4096, 4097, 4096 + 31, 4096 + 32, 2 * 4096 + 33, 3 * 4096 + 5)
SCRATCH_CANARY = 256

gpu = devtest.gpu_fixture(session_method=("CompressAppendSession", "appendv"))


class Table:
    """entries in device memory, each a tensor of its own at an odd offset of a buffer that ends with it, and their table, also in
    device memory (behind one spare byte row: the table itself is 8-byte aligned as its type asks)"""

    def __init__(self, gpu, parts, stream, k0=0, fix=None):
        import torch
        self.keep, rows = [], []
        with torch.cuda.stream(stream):
            for k, data in enumerate(parts):
                if len(data):
                    t, p = A._piece(data, k0 + k)
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

    def __init__(self, gpu, n_iov, max_piece, level, bs, seekable, checksum, stream):
        import torch
        self.size = gpu.compress_appendv_device_scratch_size(n_iov, max_piece, level, bs, seekable, checksum)
        assert self.size > 0
        with torch.cuda.stream(stream):
            self.t = torch.from_numpy(A._pattern(1 + self.size + SCRATCH_CANARY)).to("cuda")
        self.ptr = self.t.data_ptr() + 1

    def check(self):
        tail = self.t[1 + self.size:].cpu().numpy()
        assert (tail == A._pattern(1 + self.size + SCRATCH_CANARY)[1 + self.size:]).all(), "bytes at or past scratch_size changed"


class VSession(A.Session):
    """the sibling's session with appendv: a call is a list of entries (bytes)"""

    def __init__(self, gpu, cap, max_total, max_piece, level=3, bs=BS, seekable=0, checksum=0, odd_dst=0, stream=None):
        super().__init__(gpu, cap, max_total, max_piece, level, bs, seekable, checksum, odd_dst, stream)
        self.opt = (max_piece, level, bs, seekable, checksum)
        self.scratches, self.calls = [], 0

    def appendv(self, parts, total=None, fix=None, scratch=None):
        tb = Table(self.gpu, parts, self.stream, 3 * self.calls, fix)
        sc = scratch or Scratch(self.gpu, tb.n, *self.opt, self.stream)
        self.keep.append(tb)
        if sc not in self.scratches:
            self.scratches.append(sc)
        self.calls += 1
        self.s.appendv(tb.dev.data_ptr(), tb.n, tb.total if total is None else total, sc.ptr, sc.size, self.stream.cuda_stream)
        return sc

    def result(self):
        out = super().result()
        for sc in self.scratches:
            sc.check()
        return out


def _cut(data, lens):
    assert sum(lens) == len(data), (sum(lens), len(data))
    return A._split(data, list(lens))


def _check(gpu, data, calls, level=3, bs=BS, seekable=0, checksum=0, cap=None, max_piece=None, odd_dst=0, what=""):
    """calls: a list of entry-length lists (an appendv each) and ints (a plain append each), over data in order"""
    cap = A._bound(gpu, len(data)) if cap is None else cap
    want_rc, want = A._baseline(gpu, data, cap, level, bs, seekable, checksum)
    max_piece = max(bs, len(data)) if max_piece is None else max_piece
    s = VSession(gpu, cap, len(data), max_piece, level, bs, seekable, checksum, odd_dst)
    at = 0
    for k, c in enumerate(calls):
        n = c if isinstance(c, int) else sum(c)
        if isinstance(c, int):
            s.append(data[at: at + n], k)
        else:
            s.appendv(_cut(data[at: at + n], c))
        at += n
    assert at == len(data)
    s.end()
    rc, got = s.result()
    print(what, len(data), "session", rc, "compress_device", want_rc)
    assert rc == want_rc, (what, rc, want_rc)
    assert got == want, what
    return rc, got


def _orders():
    rng = np.random.default_rng(5)
    out = {"as listed": list(LENS), "reversed": list(LENS)[::-1]}
    for k in range(2):
        out["shuffled %d" % k] = [int(x) for x in rng.permutation(LENS)]
    return out


@pytest.mark.parametrize("order", list(_orders()))
def test_entry_lengths_in_several_orders(gpu, order):
    lens = _orders()[order]
    for seed in (2, 3):  # text, stored
        _check(gpu, A._payload(sum(lens), seed), [lens], 3, BS, 1, 1, what=order)


@pytest.mark.parametrize("level", [1, 3, 6])
@pytest.mark.parametrize("seekable,checksum", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_options(gpu, level, seekable, checksum):
    lens = _orders()["shuffled 0"]
    _check(gpu, A._payload(sum(lens), 4), [lens], level, BS, seekable, checksum, what="level %d" % level)
    _check(gpu, A._payload(sum(lens), 5), [lens[::-1]], level, BS, seekable, checksum, max_piece=2 * BS, what="level %d, chunks" % level)


def test_blocks_of_64_kib(gpu):
    bs = 65536
    lens = [0, 1, bs + 31, 33, bs + 32, 0, 2 * bs + 33, 7]
    lens.append(5 * bs - 11 - sum(lens))  # five blocks in all, the last one short
    assert lens[-1] > 0
    for seed in (6, 7):
        _check(gpu, A._payload(sum(lens), seed), [lens], 3, bs, 1, 1, what="64 KiB")
    _check(gpu, A._payload(sum(lens), 6), [lens], 3, bs, 1, 1, max_piece=2 * bs, what="64 KiB, chunks")


def test_tiny_entries(gpu):
    rng = np.random.default_rng(11)
    tiny = [int(x) for x in rng.integers(1, 8, 5000)]  # about five blocks, every block gathered
    assert 4 * BS < sum(tiny) < 6 * BS
    for seed in (8, 9):
        _check(gpu, A._payload(sum(tiny), seed), [tiny], 3, BS, 1, 1, what="5000 tiny entries")
    mid = tiny[:2500] + [3 * BS + 40] + tiny[2500:]  # ... and a 3-block entry in the middle: blocks of it are encoded in place
    _check(gpu, A._payload(sum(mid), 8), [mid], 3, BS, 1, 1, what="tiny entries around a 3-block entry")
    _check(gpu, A._payload(sum(mid), 9), [mid], 3, BS, 1, 1, max_piece=2 * BS, what="tiny entries around a 3-block entry, chunks")


def test_append_and_appendv_mixed_however_the_bytes_are_split(gpu):
    n = 11 * BS - 100  # eleven blocks in all; max_piece of two blocks: every appendv is a loop of chunks
    data = A._payload(n, 10)
    splits = {"a": [BS // 2, [100, 2 * BS, 0, 7, BS + 31], 3 * BS // 2 + 1, None],
              "b": [3 * BS + 5, [1] * 300 + [BS + 32, 2 * BS + 9], 17, None],
              "c": [1, [5 * BS + 1], 4 * BS - 3, None]}
    got = []
    for name, calls in splits.items():
        used = sum(c if isinstance(c, int) else sum(c) for c in calls[:-1])
        rest = n - used
        assert used % BS and (used - calls[2]) % BS and (used - calls[2] - sum(calls[1])) % BS  # every call leaves a carry for the next
        calls = calls[:-1] + [[rest // 3, 0, rest - rest // 3]]
        got.append(_check(gpu, data, calls, 3, BS, 1, 1, max_piece=2 * BS, what="mixed " + name))
    assert got[0] == got[1] == got[2]


def test_a_table_written_on_the_stream_and_one_scratch_for_two_calls(gpu):
    """the table is filled by a device copy enqueued on the session's stream just in front of the call, with no synchronisation
    in between; two calls reuse one scratch back to back"""
    import torch
    n = 7 * BS + 50
    data = A._payload(n, 12)
    cap = A._bound(gpu, n)
    want = A._baseline(gpu, data, cap, 3, BS, 1, 1)
    lens = [[BS + 9, 0, 40, 2 * BS], [5, n - 3 * BS - 54]]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    s = VSession(gpu, cap, n, 2 * BS, 3, BS, 1, 1, stream=side)
    sc = Scratch(gpu, 4, 2 * BS, 3, BS, 1, 1, side)
    s.scratches.append(sc)
    at = 0
    with torch.cuda.stream(side):
        table = torch.zeros(4 * 16, dtype=torch.uint8, device="cuda")  # one table, rewritten in stream order
        for ln in lens:
            tb = Table(gpu, _cut(data[at: at + sum(ln)], ln), side, at)
            s.keep.append(tb)
            table[: 16 * tb.n].copy_(tb.dev, non_blocking=True)
            s.s.appendv(table.data_ptr(), tb.n, tb.total, sc.ptr, sc.size, side.cuda_stream)
            at += sum(ln)
    s.end()
    assert s.result() == want


def test_the_capacity_binds_exactly(gpu):
    lens = _orders()["shuffled 1"]
    for seed in (14, 15):
        data = A._payload(sum(lens), seed)
        size, _ = _check(gpu, data, [lens], 3, BS, 1, 1, what="bound")
        assert size > 0
        for cap, want in ((size, size), (size + 1, size), (size - 1, ERR["DST_TOO_SMALL"]), (size // 2, ERR["DST_TOO_SMALL"])):
            rc, _ = _check(gpu, data, [lens], 3, BS, 1, 1, cap=cap, max_piece=3 * BS, odd_dst=1, what="capacity %d" % cap)
            assert rc == want


def _bad_table_cases():
    def null_base(rows):
        rows[2] = (0, rows[2][1])

    # name -> (delta of the promise, change of the table's rows, the code end stores)
    return {"sum one below total": (+1, None, "SRC_TOO_SMALL"), "sum one above total": (-1, None, "OVERFLOW"),
            "an entry longer than total": (None, None, "OVERFLOW"), "a zero base with a length": (0, null_base, "NULL_INPUT")}


@pytest.mark.parametrize("case", list(_bad_table_cases()))
def test_table_errors_become_the_sessions_status_and_stay(gpu, case):
    delta, fix, want = _bad_table_cases()[case]
    lens = [BS + 7, 3 * BS, 50, 0, 2 * BS + 1]
    n = sum(lens)
    data = A._payload(n + 3 * BS, 16)
    parts = _cut(data[:n], lens)
    # an entry longer than total: the promise is smaller than the second entry (and than the sum)
    promised = lens[1] - 1 if delta is None else n + delta
    for before in (0, 100):
        s = VSession(gpu, A._bound(gpu, 3 * n), 3 * n, 2 * BS, 3, BS, 1, 1, odd_dst=1)
        if before:
            s.append(data[:before])
        s.appendv(parts, total=promised, fix=fix)
        s.appendv(_cut(data[n: n + 2 * BS + 5], [BS, 5, BS]))  # a later valid appendv: the error stays
        s.append(data[:77])
        s.end()
        rc, _ = s.result()  # the pattern outside [0, dst_capacity) and behind the scratch holds
        assert rc == ERR[want], (case, before, rc)


def test_a_table_error_behind_a_chunked_appendv_keeps_what_was_gathered(gpu):
    """max_piece of two blocks: an appendv of 3 blocks + 5 bytes in tiny entries succeeds over two chunks, each through the advance;
    the table of the next appendv sums one byte short of its promise, and the advance of its chunk must leave the state alone. `end`
    reports the table's error, the three blocks gathered so far are the one-shot archive's and nothing lies behind them; a fresh
    session on the same work area and scratch gives the one-shot archive."""
    n, more = 3 * BS + 5, 2 * BS
    rng = np.random.default_rng(23)
    tiny = [int(x) for x in rng.integers(1, 8, n)]
    tiny = tiny[: int(np.searchsorted(np.cumsum(tiny), n))]
    tiny.append(n - sum(tiny))
    data = A._payload(n + more, 22)
    cap = A._bound(gpu, n + more)
    want_rc, want = A._baseline(gpu, data[:n], cap, 3, BS, 1, 1)
    assert want_rc > 0
    s = VSession(gpu, cap, n + more, 2 * BS, 3, BS, 1, 1)
    sc = s.appendv(_cut(data[:n], tiny))
    s.appendv(_cut(data[n: n + more - 1], [BS, 7, BS - 8]), total=more, scratch=sc)
    s.end()
    rc, _ = s.result()
    assert rc == ERR["SRC_TOO_SMALL"], rc
    dst, whole = s.dst.cpu().numpy(), A._pattern(cap + A.CANARY)
    sizes = np.frombuffer(want[-12 - 4 * 4: -12], dtype="<u4")  # the seek table of the one-shot archive: four blocks
    end = 16 + int(sizes[:3].sum())
    assert bytes(dst[16: end]) == want[16: end], "the blocks gathered before the error"
    assert (dst[:16] == whole[:16]).all() and (dst[end:] == whole[end:]).all(), "bytes outside the gathered blocks changed"
    s2 = VSession(gpu, cap, n + more, 2 * BS, 3, BS, 1, 1)
    s2.s = gpu.compress_begin_device(s2.dst.data_ptr(), cap, n + more, 2 * BS, s.work.data_ptr() + 1, s.work.numel() - 1, 3, BS, 1, 1,
                                     s2.stream.cuda_stream)  # ... on the first session's work area (its own goes unused)
    s2.appendv(_cut(data[:n], tiny), scratch=sc)
    s2.end()
    assert s2.result() == (want_rc, want)


def test_refusals_leave_the_session_usable(gpu):
    import torch
    n = 3 * BS + 10
    data = A._payload(n, 18)
    cap = A._bound(gpu, n)
    # past max_total: refused synchronously, the session goes on
    s = VSession(gpu, cap, n, 2 * BS, 3, BS, 1, 1)
    s.append(data[: BS - 1])
    tb = Table(gpu, _cut(data[BS - 1:], [BS, n - 2 * BS + 1]), s.stream)
    sc = Scratch(gpu, tb.n, 2 * BS, 3, BS, 1, 1, s.stream)
    with pytest.raises(gpu.ZxcError) as e:
        s.s.appendv(tb.dev.data_ptr(), tb.n, tb.total + 1, sc.ptr, sc.size, s.stream.cuda_stream)
    assert e.value.code == ERR["OVERFLOW"]
    with pytest.raises(gpu.ZxcError) as e:
        s.s.appendv(tb.dev.data_ptr(), tb.n, tb.total, sc.ptr, sc.size - 1, s.stream.cuda_stream)
    assert e.value.code == -1  # ZXC_ERROR_MEMORY: one byte less than the size
    s.s.appendv(tb.dev.data_ptr(), tb.n, tb.total, sc.ptr, sc.size, s.stream.cuda_stream)  # exactly the size
    s.scratches.append(sc)
    s.end()
    assert s.result() == A._baseline(gpu, data, cap, 3, BS, 1, 1)
    # a session with a dictionary: refused synchronously, goes on with plain appends
    dd = D._dict(gpu, 1000)
    want = D._baseline(gpu, data, dd, cap, 3, BS, 1, 1)
    ds = D.Session(gpu, dd, cap, n, 2 * BS, 3, BS, 1, 1)
    ds.append(data[:100])
    with pytest.raises(gpu.ZxcError) as e:
        ds.s.appendv(tb.dev.data_ptr(), tb.n, tb.total, sc.ptr, sc.size, torch.cuda.current_stream().cuda_stream)
    assert e.value.code == ERR["GPU_UNSUPPORTED"]
    ds.append(data[100:])
    ds.end()
    assert ds.result() == want


def test_round_trip(gpu, ref):
    lens = _orders()["reversed"]
    n = sum(lens)
    for seed, checksum in ((20, 1), (21, 0)):
        data = A._payload(n, seed)
        rc, arc = _check(gpu, data, [lens], 3, BS, 1, checksum, max_piece=3 * BS, what="round trip")
        assert rc > 0
        size, back = ref.decompress(arc, n, checksum=bool(checksum))
        assert size == n and back == data
