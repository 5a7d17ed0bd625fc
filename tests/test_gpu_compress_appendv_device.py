"""zxc_mi355x_compress_appendv_device on the GPU: one call appends a table of buffers to an append session. The reference value is
always existing code: the archive and the result word zxc_mi355x_compress_device writes for the concatenation with the same
options and capacity; for round trips the unmodified reference decoder. Set-up as in test_gpu_compress_append_device.py, with the
helpers of tests/dev_append.py: every entry is a tensor of its own at an odd offset inside a buffer that ends with the entry (nothing
readable is promised behind an entry), the destination is a pattern with a canary behind dst_capacity, the table lies in device memory, and
the scratch sits at an odd address with a canary behind scratch_size. Nothing here provokes a fault: every refused input is
refused by status, and a table that breaks a rule names only buffers that exist."""
import numpy as np
import pytest

import devtest
from dev_append import (Table, bad_table_cases as _bad_table_cases, cut as _cut, dict_baseline as _dict_baseline, dict_of as _dict,
                        dict_session as DictSession, orders as _orders, plain_baseline as _baseline, plain_scratch as Scratch,
                        plain_session as VSession, run_calls)
from devtest import CANARY, ERR, bound as _bound, pattern as _pattern, payload as _payload

pytestmark = pytest.mark.gpu

BS = 4096

gpu = devtest.gpu_fixture(session_method=("CompressAppendSession", "appendv"))


def _check(gpu, data, calls, level=3, bs=BS, seekable=0, checksum=0, cap=None, max_piece=None, odd_dst=0, what=""):
    """calls: a list of entry-length lists (an appendv each) and ints (a plain append each), over data in order"""
    cap = _bound(gpu, len(data)) if cap is None else cap
    want_rc, want = _baseline(gpu, data, cap, level, bs, seekable, checksum)
    max_piece = max(bs, len(data)) if max_piece is None else max_piece
    rc, got = run_calls(VSession(gpu, cap, len(data), max_piece, level, bs, seekable, checksum, odd_dst), data, calls)
    print(what, len(data), "session", rc, "compress_device", want_rc)
    assert rc == want_rc, (what, rc, want_rc)
    assert got == want, what
    return rc, got


@pytest.mark.parametrize("order", list(_orders()))
def test_entry_lengths_in_several_orders(gpu, order):
    lens = _orders()[order]
    for seed in (2, 3):  # text, stored
        _check(gpu, _payload(sum(lens), seed), [lens], 3, BS, 1, 1, what=order)


@pytest.mark.parametrize("level", [1, 3, 6])
@pytest.mark.parametrize("seekable,checksum", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_options(gpu, level, seekable, checksum):
    lens = _orders()["shuffled 0"]
    _check(gpu, _payload(sum(lens), 4), [lens], level, BS, seekable, checksum, what="level %d" % level)
    _check(gpu, _payload(sum(lens), 5), [lens[::-1]], level, BS, seekable, checksum, max_piece=2 * BS, what="level %d, chunks" % level)


def test_blocks_of_64_kib(gpu):
    bs = 65536
    lens = [0, 1, bs + 31, 33, bs + 32, 0, 2 * bs + 33, 7]
    lens.append(5 * bs - 11 - sum(lens))  # five blocks in all, the last one short
    assert lens[-1] > 0
    for seed in (6, 7):
        _check(gpu, _payload(sum(lens), seed), [lens], 3, bs, 1, 1, what="64 KiB")
    _check(gpu, _payload(sum(lens), 6), [lens], 3, bs, 1, 1, max_piece=2 * bs, what="64 KiB, chunks")


def test_tiny_entries(gpu):
    rng = np.random.default_rng(11)
    tiny = [int(x) for x in rng.integers(1, 8, 5000)]  # about five blocks, every block gathered
    assert 4 * BS < sum(tiny) < 6 * BS
    for seed in (8, 9):
        _check(gpu, _payload(sum(tiny), seed), [tiny], 3, BS, 1, 1, what="5000 tiny entries")
    mid = tiny[:2500] + [3 * BS + 40] + tiny[2500:]  # ... and a 3-block entry in the middle: blocks of it are encoded in place
    _check(gpu, _payload(sum(mid), 8), [mid], 3, BS, 1, 1, what="tiny entries around a 3-block entry")
    _check(gpu, _payload(sum(mid), 9), [mid], 3, BS, 1, 1, max_piece=2 * BS, what="tiny entries around a 3-block entry, chunks")


def test_append_and_appendv_mixed_however_the_bytes_are_split(gpu):
    n = 11 * BS - 100  # eleven blocks in all; max_piece of two blocks: every appendv is a loop of chunks
    data = _payload(n, 10)
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
    data = _payload(n, 12)
    cap = _bound(gpu, n)
    want = _baseline(gpu, data, cap, 3, BS, 1, 1)
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
        data = _payload(sum(lens), seed)
        size, _ = _check(gpu, data, [lens], 3, BS, 1, 1, what="bound")
        assert size > 0
        for cap, want in ((size, size), (size + 1, size), (size - 1, ERR["DST_TOO_SMALL"]), (size // 2, ERR["DST_TOO_SMALL"])):
            rc, _ = _check(gpu, data, [lens], 3, BS, 1, 1, cap=cap, max_piece=3 * BS, odd_dst=1, what="capacity %d" % cap)
            assert rc == want


@pytest.mark.parametrize("case", list(_bad_table_cases()))
def test_table_errors_become_the_sessions_status_and_stay(gpu, case):
    delta, fix, want = _bad_table_cases()[case]
    lens = [BS + 7, 3 * BS, 50, 0, 2 * BS + 1]
    n = sum(lens)
    data = _payload(n + 3 * BS, 16)
    parts = _cut(data[:n], lens)
    # an entry longer than total: the promise is smaller than the second entry (and than the sum)
    promised = lens[1] - 1 if delta is None else n + delta
    for before in (0, 100):
        s = VSession(gpu, _bound(gpu, 3 * n), 3 * n, 2 * BS, 3, BS, 1, 1, odd_dst=1)
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
    data = _payload(n + more, 22)
    cap = _bound(gpu, n + more)
    want_rc, want = _baseline(gpu, data[:n], cap, 3, BS, 1, 1)
    assert want_rc > 0
    s = VSession(gpu, cap, n + more, 2 * BS, 3, BS, 1, 1)
    sc = s.appendv(_cut(data[:n], tiny))
    s.appendv(_cut(data[n: n + more - 1], [BS, 7, BS - 8]), total=more, scratch=sc)
    s.end()
    rc, _ = s.result()
    assert rc == ERR["SRC_TOO_SMALL"], rc
    dst, whole = s.dst.cpu().numpy(), _pattern(cap + CANARY)
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
    data = _payload(n, 18)
    cap = _bound(gpu, n)
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
    assert s.result() == _baseline(gpu, data, cap, 3, BS, 1, 1)
    # a session with a dictionary: refused synchronously, goes on with plain appends
    dd = _dict(gpu, 1000)
    want = _dict_baseline(gpu, data, dd, cap, 3, BS, 1, 1)
    ds = DictSession(gpu, dd, cap, n, 2 * BS, 3, BS, 1, 1)
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
        data = _payload(n, seed)
        rc, arc = _check(gpu, data, [lens], 3, BS, 1, checksum, max_piece=3 * BS, what="round trip")
        assert rc > 0
        size, back = ref.decompress(arc, n, checksum=bool(checksum))
        assert size == n and back == data
