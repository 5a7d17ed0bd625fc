"""zxc_mi355x_compress_appendv_dict_device on the GPU: one call appends a table of buffers to an append session begun with a
dictionary. The reference value is always existing code: the archive and the result word zxc_mi355x_compress_dict_device writes for
the concatenation with the same options, dictionary and capacity; for round trips the unmodified reference decoder and a dictionary
take session with takev. Set-up as in test_gpu_compress_append_dict_device.py and test_gpu_compress_appendv_device.py, with the
helpers of tests/dev_append.py: every entry is a tensor of its own at an odd offset inside a buffer that ends with the entry (nothing
readable is promised behind an entry), the destination is a pattern with a canary behind dst_capacity, the table lies in device memory, d_work and the
scratch sit at odd addresses, the scratch with a canary behind scratch_size. Nothing here provokes a fault: every refused input is
refused by status, and a table that breaks a rule names only buffers that exist."""
import numpy as np
import pytest

import dev_append
import devtest
from dev_append import (Table, bad_table_cases as _bad_table_cases, cut as _cut, dict_baseline as _baseline, dict_of as _dict,
                        dict_scratch as Scratch, dict_session as VSession, orders as _orders, plain_baseline as _plain_baseline,
                        plain_session as PlainVSession, run_calls as _run, text as _text)
from dev_take import TakevSession
from devtest import CANARY, ERR, bound as _bound, pattern as _pattern, payload as _payload, ref_decompress as _ref_decompress, split as _split

pytestmark = pytest.mark.gpu

BS = 4096
DICT_SIZES = (1, 100, 4099, 65535)

gpu = devtest.gpu_fixture(session_method=("CompressAppendSession", "appendv_dict"))

_BASE = dev_append.BASE[dev_append.DICT]  # (cleared behind the one very large case)


def _check(gpu, data, calls, dd, level=3, bs=BS, seekable=0, checksum=0, cap=None, max_piece=None, odd_dst=0, what=""):
    """calls: a list of entry-length lists (an appendv_dict each) and ints (a plain append each), over data in order"""
    cap = _bound(gpu, len(data)) if cap is None else cap
    want_rc, want = _baseline(gpu, data, dd, cap, level, bs, seekable, checksum)
    max_piece = max(bs, len(data)) if max_piece is None else max_piece
    rc, got = _run(VSession(gpu, dd, cap, len(data), max_piece, level, bs, seekable, checksum, odd_dst), data, calls)
    print(what, len(data), "dict", dd.tup[1], "session", rc, "compress_dict_device", want_rc)
    assert rc == want_rc, (what, rc, want_rc)
    assert got == want, what
    if rc > 0:
        assert got[6] & 0x40 and got[7:11] == bytes(dd.d_id.cpu().numpy().view(np.uint8)), what  # the flag and the id
    return rc, got


@pytest.mark.parametrize("dict_size", DICT_SIZES)
@pytest.mark.parametrize("order", list(_orders()))
def test_entry_lengths_in_several_orders(gpu, order, dict_size):
    lens = _orders()[order]
    k = DICT_SIZES.index(dict_size)
    for seed in (2, 3):  # text, stored
        _check(gpu, _payload(sum(lens), seed), [lens], _dict(gpu, dict_size, bool((k + seed) % 2)), 3, BS, 1, 1, what=order)
    cut = list(lens)
    cut[cut.index(max(cut))] -= 7  # the same bytes behind a carry of 7, in chunks of two blocks
    _check(gpu, _payload(sum(lens), 2), [7, cut], _dict(gpu, dict_size), 3, BS, 1, 1, max_piece=2 * BS, what=order + ", behind a carry, chunks")


@pytest.mark.parametrize("level", [1, 3, 7])
@pytest.mark.parametrize("seekable,checksum", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_options(gpu, level, seekable, checksum):
    lens = _orders()["shuffled 0"]
    dd = _dict(gpu, 4099, level == 7)
    _check(gpu, _payload(sum(lens), 4), [lens], dd, level, BS, seekable, checksum, what="level %d" % level)
    _check(gpu, _payload(sum(lens), 5), [lens[::-1]], dd, level, BS, seekable, checksum, max_piece=2 * BS, what="level %d, chunks" % level)


def test_blocks_of_64_kib(gpu):
    bs = 65536
    lens = [0, 1, bs + 31, 33, bs + 32, 0, 2 * bs + 33, 7]
    lens.append(5 * bs - 11 - sum(lens))  # five blocks in all, the last one short
    assert lens[-1] > 0
    dd = _dict(gpu, 65535)
    _check(gpu, _payload(sum(lens), 6), [lens], dd, 3, bs, 1, 1, what="64 KiB")
    _check(gpu, _payload(sum(lens), 7), [bs // 2 + 1, lens[:-1] + [lens[-1] - bs // 2 - 1]], dd, 3, bs, 1, 1, max_piece=2 * bs, what="64 KiB, chunks")


def test_tiny_entries(gpu):
    """behind a carry of 5 bytes, blocks made of 1-byte and 3-byte entries alone"""
    tiny = [1, 3] * (5 * BS // 8)  # two and a half blocks
    n = 5 + sum(tiny)
    assert 2 * BS < n < 3 * BS
    for seed, size in ((8, 100), (9, 65535)):
        _check(gpu, _payload(n, seed), [5, tiny], _dict(gpu, size), 3, BS, 1, 1, what="1- and 3-byte entries")
    _check(gpu, _payload(n, 8), [5, tiny], _dict(gpu, 4099), 3, BS, 1, 1, max_piece=BS, what="1- and 3-byte entries, chunks of one block")


def test_append_and_appendv_dict_mixed_however_the_bytes_are_split(gpu):
    n = 11 * BS - 100  # eleven blocks in all; max_piece of two blocks: every longer call is a loop of chunks
    data = _payload(n, 10)
    dd = _dict(gpu, 4099, True)
    splits = {"a": [BS // 2, [100, 2 * BS, 0, 7, BS + 31], 3 * BS // 2 + 1, [5, 0, 9], None],       # a call wholly inside one block
              "b": [3 * BS + 5, [1] * 300 + [BS + 32, 2 * BS + 9], 17, [BS - 400], None],              # a call that ends inside a block
              "c": [[1], [5 * BS + 1], 4 * BS - 3, [2], None],
              "d": [[BS - 1, 1], [BS + 1], BS - 2, [1], [0, 0], None]}                                  # on a boundary, and one to either side
    got = []
    for name, calls in splits.items():
        used = sum(c if isinstance(c, int) else sum(c) for c in calls[:-1])
        rest = n - used
        calls = calls[:-1] + [[rest // 3, 0, rest - rest // 3]]
        got.append(_check(gpu, data, calls, dd, 3, BS, 1, 1, max_piece=2 * BS, what="mixed " + name))
    assert got[0] == got[1] == got[2] == got[3]


def test_a_call_of_more_than_max_piece(gpu):
    mp = 2 * BS
    n = 5 * mp + 3 + 100
    lens = [BS + 31, 0, 3, 2 * BS + 32, 17, 3 * BS - 1]
    lens.append(5 * mp + 3 - sum(lens))
    assert lens[-1] > 0
    _check(gpu, _payload(n, 12), [100, lens], _dict(gpu, 4099), 3, BS, 1, 1, max_piece=mp, what="the chunk loop behind a carry")
    _check(gpu, _payload(5 * mp + 3, 13), [lens], _dict(gpu, 1), 3, BS, 1, 1, max_piece=mp, what="the chunk loop")


def test_a_chunk_of_two_launches(gpu):
    """4 KiB blocks under a dictionary of 65 535 bytes: a launch is 4096 jobs, and a chunk of 4097 blocks behind a carry of 5 bytes
    takes two, with the carried block and the tail workgroup in the first (the shape of test_a_piece_of_two_chunks). The source is
    one table of a few thousand entries of mixed lengths."""
    max_piece = 4097 * BS + 7
    n = 5 + max_piece
    base = np.frombuffer(_text()[: 4 << 20], dtype=np.uint8)
    arr = np.tile(base, n // len(base) + 1)[:n].copy()
    rng = np.random.default_rng(43)
    at = rng.integers(0, n, n // 200)
    arr[at] = rng.integers(0, 256, len(at), dtype=np.uint8)  # no two blocks alike
    data = arr.tobytes()
    kinds = rng.integers(0, 4, 3000)
    lens = [int(x) for x in np.where(kinds == 0, rng.integers(0, 8, 3000), np.where(kinds == 1, rng.integers(0, 40, 3000),
                                     np.where(kinds == 2, rng.integers(0, 2 * BS, 3000), rng.integers(0, 5 * BS, 3000))))]
    assert sum(lens) < max_piece
    lens.append(max_piece - sum(lens))
    dd = _dict(gpu, 65535)
    ss = gpu.compress_appendv_dict_device_scratch_size(len(lens), max_piece, 65535, 3, BS, True, True)
    assert 0 < ss <= 8 * (len(lens) + 1) + 16 * -(-len(lens) // 1024) + 4096
    _check(gpu, data, [5, lens], dd, 3, BS, 1, 1, max_piece=max_piece, what="4097 blocks in one chunk")
    _BASE.clear()


def test_a_table_written_on_the_stream_and_one_scratch_for_two_calls(gpu):
    """the table is filled by a device copy enqueued on the session's stream just in front of the call, with no synchronisation
    in between; two calls reuse one scratch back to back"""
    import torch
    n = 7 * BS + 50
    data = _payload(n, 12)
    dd = _dict(gpu, 4099)
    cap = _bound(gpu, n)
    want = _baseline(gpu, data, dd, cap, 3, BS, 1, 1)
    lens = [[BS + 9, 0, 40, 2 * BS], [5, n - 3 * BS - 54]]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    s = VSession(gpu, dd, cap, n, 2 * BS, 3, BS, 1, 1, stream=side)
    sc = Scratch(gpu, 4, 2 * BS, 4099, 3, BS, 1, 1, side)
    s.scratches.append(sc)
    at = 0
    with torch.cuda.stream(side):
        table = torch.zeros(4 * 16, dtype=torch.uint8, device="cuda")  # one table, rewritten in stream order
        for ln in lens:
            tb = Table(gpu, _cut(data[at: at + sum(ln)], ln), side, at)
            s.keep.append(tb)
            table[: 16 * tb.n].copy_(tb.dev, non_blocking=True)
            s.s.appendv_dict(table.data_ptr(), tb.n, tb.total, sc.ptr, sc.size, side.cuda_stream)
            at += sum(ln)
    s.end()
    assert s.result() == want


def test_the_capacity_binds_exactly(gpu):
    lens = _orders()["shuffled 1"]
    for seed in (14, 15):
        data, dd = _payload(sum(lens), seed), _dict(gpu, 100 if seed % 2 else 4099)
        size, _ = _check(gpu, data, [lens], dd, 3, BS, 1, 1, what="bound")
        assert size > 0
        for cap, want in ((size, size), (size + 1, size), (size - 1, ERR["DST_TOO_SMALL"]), (size // 2, ERR["DST_TOO_SMALL"])):
            rc, _ = _check(gpu, data, [lens], dd, 3, BS, 1, 1, cap=cap, max_piece=3 * BS, odd_dst=1, what="capacity %d" % cap)
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
    for before, size in ((0, 100), (100, 65535)):
        s = VSession(gpu, _dict(gpu, size), _bound(gpu, 3 * n), 3 * n, 2 * BS, 3, BS, 1, 1, odd_dst=1)
        if before:
            s.append(data[:before])
        s.appendv(parts, total=promised, fix=fix)
        s.appendv(_cut(data[n: n + 2 * BS + 5], [BS, 5, BS]))  # a later valid appendv_dict: the error stays
        s.append(data[:77])
        s.end()
        rc, _ = s.result()  # the pattern outside [0, dst_capacity) and behind the scratch holds
        assert rc == ERR[want], (case, before, rc)


def test_a_table_error_behind_a_chunked_call_keeps_what_was_gathered(gpu):
    """max_piece of two blocks: an appendv_dict of 3 blocks + 5 bytes in tiny entries succeeds over two chunks, each through the
    advance; the table of the next call sums one byte short of its promise, and the advance of its chunk must leave the state alone.
    `end` reports the table's error, the three blocks gathered so far are the one-shot archive's and nothing lies behind them; a
    fresh session on the same work area and scratch gives the one-shot archive."""
    n, more = 3 * BS + 5, 2 * BS
    rng = np.random.default_rng(23)
    tiny = [int(x) for x in rng.integers(1, 8, n)]
    tiny = tiny[: int(np.searchsorted(np.cumsum(tiny), n))]
    tiny.append(n - sum(tiny))
    data = _payload(n + more, 22)
    dd = _dict(gpu, 4099)
    cap = _bound(gpu, n + more)
    want_rc, want = _baseline(gpu, data[:n], dd, cap, 3, BS, 1, 1)
    assert want_rc > 0
    s = VSession(gpu, dd, cap, n + more, 2 * BS, 3, BS, 1, 1)
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
    s2 = VSession(gpu, dd, cap, n + more, 2 * BS, 3, BS, 1, 1, work=s.work)  # ... on the first session's work area
    s2.appendv(_cut(data[:n], tiny), scratch=sc)
    s2.end()
    assert s2.result() == (want_rc, want)


def test_refusals_leave_the_session_usable(gpu):
    n = 3 * BS + 10
    data = _payload(n, 18)
    dd = _dict(gpu, 100)
    cap = _bound(gpu, n)
    s = VSession(gpu, dd, cap, n, 2 * BS, 3, BS, 1, 1)
    s.append(data[: BS - 1])
    tb = Table(gpu, _cut(data[BS - 1:], [BS, n - 2 * BS + 1]), s.stream)
    sc = Scratch(gpu, tb.n, 2 * BS, 100, 3, BS, 1, 1, s.stream)
    sp = s.stream.cuda_stream
    for args, code in (((tb.dev.data_ptr(), tb.n, tb.total + 1, sc.ptr, sc.size), "OVERFLOW"),      # past max_total
                       ((tb.dev.data_ptr(), tb.n, tb.total, sc.ptr, sc.size - 1), "MEMORY"),        # one byte less than the size
                       ((0, tb.n, tb.total, sc.ptr, sc.size), "NULL_INPUT"), ((tb.dev.data_ptr(), tb.n, tb.total, 0, sc.size), "NULL_INPUT"),
                       ((0, 0, 1, sc.ptr, sc.size), "SRC_TOO_SMALL")):
        with pytest.raises(gpu.ZxcError) as e:
            s.s.appendv_dict(*args, sp)
        assert e.value.code == ERR[code], code
    s.s.appendv_dict(0, 0, 0, sc.ptr, sc.size, sp)  # nothing to append
    s.s.appendv_dict(tb.dev.data_ptr(), tb.n, tb.total, sc.ptr, sc.size, sp)  # exactly the size
    s.scratches.append(sc)
    s.end()
    assert s.result() == _baseline(gpu, data, dd, cap, 3, BS, 1, 1)


def test_without_a_dictionary_the_siblings_bytes(gpu):
    """a session begun without a dictionary through the new call: the archive of compress_device, which is the sibling's, and the
    sibling's scratch need"""
    n = 6 * BS + 77
    data = _payload(n, 30)
    calls = [BS - 3, [100, 2 * BS + 10, 0, 1], [n - 3 * BS - 108]]
    cap = _bound(gpu, n)
    want = _plain_baseline(gpu, data, cap, 3, BS, 1, 1)
    assert want[0] > 0 and not want[1][6] & 0x40
    assert gpu.compress_appendv_dict_device_scratch_size(4, 2 * BS, 0, 3, BS, True, True) == gpu.compress_appendv_device_scratch_size(4, 2 * BS, 3, BS, True, True)
    dd = _dict(gpu, 100)
    for tup in (None, (dd.tup[0], 0, dd.tup[2], dd.tup[3])):
        assert _run(VSession(gpu, None, cap, n, 2 * BS, 3, BS, 1, 1, dict_=tup), data, calls) == want, tup
    sib = PlainVSession(gpu, cap, n, 2 * BS, 3, BS, 1, 1)  # ... and the sibling itself
    sib.append(data[: BS - 3])
    sib.appendv(_cut(data[BS - 3: 3 * BS + 108], calls[1]))
    sib.appendv(_cut(data[3 * BS + 108:], calls[2]))
    sib.end()
    assert sib.result() == want


def test_two_sessions_interleaved_on_two_streams(gpu):
    import torch
    n = 9 * BS + 5
    datas = [_payload(n, 22), _payload(n, 24)]
    dds = [_dict(gpu, 4099), _dict(gpu, 65535, True)]
    lens = [[[BS + 3], [4 * BS - 9, 9], [7, 0, n - 5 * BS - 10]], [[7], [1] * 40 + [2 * BS - 40], [n - 2 * BS - 7]]]
    cap = _bound(gpu, n)
    want = [_baseline(gpu, d, dd, cap, 3, BS, 1, 1) for d, dd in zip(datas, dds)]
    torch.cuda.synchronize()
    sess = [VSession(gpu, dd, cap, n, 4 * BS, 3, BS, 1, 1, stream=torch.cuda.Stream()) for dd in dds]
    parts = [_split(d, [sum(c) for c in ln]) for d, ln in zip(datas, lens)]
    for k in range(3):
        for s, p, ln in zip(sess, parts, lens):
            s.appendv(_cut(p[k], ln[k]))
    for s in sess:
        s.end()
    for s, w in zip(sess, want):
        assert s.result() == w
    assert want[0] != want[1]


def test_round_trips(gpu, ref):
    lens = _orders()["reversed"]
    n = sum(lens)
    for seed, checksum, with_huf in ((20, 1, True), (21, 0, False)):
        data, dd = _payload(n, seed), _dict(gpu, 4099, with_huf)
        rc, arc = _check(gpu, data, [lens], dd, 3, BS, 1, checksum, max_piece=3 * BS, what="round trip")
        assert rc > 0
        size, back = _ref_decompress(ref, arc, n, dd.content, dd.huf, bool(checksum))
        assert size == n and back == data
        assert _ref_decompress(ref, arc, n)[0] == ERR["DICT_REQUIRED"]
        # read back through a dictionary take session, into a table of other entries than it was written from
        t = TakevSession(gpu, arc, n, BS, max_piece=2 * BS, checksum=bool(checksum), dd=dd)
        t.takev([BS + 5, 0, 1, 7 * BS], aligned=False)
        t.takev([n - 8 * BS - 6], aligned=True)
        t.end()
        size, parts = t.result()
        assert size == n and b"".join(parts) == data
