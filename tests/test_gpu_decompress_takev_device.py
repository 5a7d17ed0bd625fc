"""zxc_mi355x_decompress_takev_device on the GPU: the next bytes of a take session delivered into a table of destinations that lies
in device memory. The reference value is the result word and the output of zxc_mi355x_decompress_device / _dict_device for the same
archive, capacity and options (existing code, not the code under test); for one round trip the unmodified reference decoder. The
entries of a call are slices of one device tensor with at least 64 canary bytes between them, so a spill behind an entry shows;
every case checks every canary and the result word. A run with every entry 16-byte aligned takes the direct path where the rule
allows, a run with the entries at odd addresses sends everything through slots. Nothing here provokes a fault: every bad input is
refused by status, and a table in error is never dereferenced."""
import numpy as np
import pytest

import devtest
from dev_take import BS, TakevSession as VSession, archive as _archive, blocks_at as _blocks_at, oneshot as _oneshot
from devtest import ERR, PAD, UNSET, DevDict, payload as _payload, to_dev as _to_dev

pytestmark = pytest.mark.gpu

ERRV = ERR
EDGE_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 4096 + 31, 4096 + 32, 4096 + 33, 2 * 4096 + 32, 3 * 4096 + 5]

gpu = devtest.gpu_fixture(session_method=("DecompressTakeSession", "takev"))


def _check(gpu, arc, cap, calls, bs=BS, checksum=False, aligned=True, max_piece=None, dd=None, what=""):
    """calls: ("take", n) or ("takev", [lens]) -> (rc, bytes, session), compared with decompress_device"""
    assert sum(x if k == "take" else sum(x) for k, x in calls) == cap
    want_rc, want = _oneshot(gpu, arc, cap, bs, checksum, dd)
    s = VSession(gpu, arc, cap, bs, max_piece, checksum, dd)
    for kind, x in calls:
        if kind == "take":
            s.take(x, aligned)
        else:
            s.takev(x, aligned)
    s.end()
    rc, parts = s.result()
    got = b"".join(parts)
    print(what, cap, "aligned" if aligned else "odd", "session", rc, "decompress_device", want_rc)
    assert rc == want_rc, (what, rc, want_rc)
    if rc >= 0:
        assert got[:rc] == want, what
    return rc, got, s


@pytest.mark.parametrize("aligned", [True, False])
def test_entry_lengths_around_a_block_and_its_spill(gpu, aligned):
    import random
    n = sum(EDGE_LENS)
    orders = [EDGE_LENS, EDGE_LENS[::-1], random.Random(1).sample(EDGE_LENS, len(EDGE_LENS)), random.Random(2).sample(EDGE_LENS, len(EDGE_LENS))]
    for k, lens in enumerate(orders):
        data = _payload(n, 30 + k)  # text and stored blocks in turn
        arc = _archive(gpu, data)
        for verify in (True, False):
            rc, got, _ = _check(gpu, arc, n, [("takev", lens)], checksum=verify, aligned=aligned, what="order %d" % k)
            assert rc == n and got == data


def test_tiny_entries_send_every_block_through_the_scatter(gpu):
    rng = np.random.default_rng(5)
    lens = [int(x) for x in rng.integers(1, 8, 5000)]
    n = sum(lens)
    for seed in (34, 35):
        data = _payload(n, seed)
        arc = _archive(gpu, data)
        for aligned in (True, False):
            rc, got, _ = _check(gpu, arc, n, [("takev", lens)], checksum=True, aligned=aligned, what="5000 tiny entries")
            assert rc == n and got == data


def test_the_chunk_loop_with_take_and_takev_mixed(gpu):
    """max_piece of two blocks over an archive of eleven: calls of many chunks, calls that lie wholly inside one block, a take
    behind a takev that ended inside a block and the other way round"""
    n = 11 * BS - 100
    data = _payload(n, 36)
    arc = _archive(gpu, data)
    rest = n - (5 * BS + 40) - 100 - 7 - 30 - (3 * BS)
    plans = {
        "one takev": [("takev", [n])],
        "entries of a block and a half": [("takev", [BS + BS // 2] * 7 + [n - 7 * (BS + BS // 2)])],
        "mixed": [("takev", [5 * BS, 40]), ("take", 100), ("takev", [3, 0, 4]), ("take", 30), ("takev", [BS, BS + 32, BS - 32]), ("take", rest)],
        "take first": [("take", BS // 2), ("takev", [16, 17, 0, 33]), ("takev", [n - BS // 2 - 66])],
    }
    for name, calls in plans.items():
        for aligned in (True, False):
            rc, got, _ = _check(gpu, arc, n, calls, checksum=True, aligned=aligned, max_piece=2 * BS, what=name)
            assert rc == n and got == data


@pytest.mark.parametrize("seekable,checksum", [(0, 0), (0, 1), (1, 1)])
def test_seekable_checksum_and_verification(gpu, seekable, checksum):
    n = 6 * BS + 1234
    lens = [112, 0, 3 * BS, 2 * BS + 32, n - 5 * BS - 144]
    for seed in (38, 39):
        data = _payload(n, seed)
        arc = _archive(gpu, data, seekable=bool(seekable), checksum=bool(checksum))
        for verify in (True, False):
            for aligned in (True, False):
                rc, got, _ = _check(gpu, arc, n, [("takev", lens)], checksum=verify, aligned=aligned, max_piece=4 * BS,
                                    what="seekable %d checksum %d verify %d" % (seekable, checksum, verify))
                assert rc == n and got == data


def test_blocks_of_64_kib(gpu):
    bs = 65536
    n = 3 * bs + bs // 3 + 5
    data = _payload(n, 40)
    arc = _archive(gpu, data, bs=bs)
    lens = [bs // 2 + 16, bs + 32, 7, bs + 31, n - bs // 2 - 2 * bs - 86]
    for aligned in (True, False):
        rc, got, _ = _check(gpu, arc, n, [("takev", lens)], bs=bs, checksum=True, aligned=aligned, what="64 KiB blocks")
        assert rc == n and got == data


def test_a_session_begun_with_a_dictionary(gpu):
    import torch
    from zxc_amd import corpus
    n = 9 * BS + 50
    data = _payload(n, 42)
    dd = DevDict(gpu, corpus.synth_text(30000, seed=8))
    src = _to_dev(data, PAD)
    ws = gpu.compress_dict_device_work_size(n, len(dd.content), 3, BS, True, True)
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    cap_arc = 2 * n + 4096
    dst = torch.empty(cap_arc, dtype=torch.uint8, device="cuda")
    res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
    gpu.compress_dict_device(src.data_ptr(), n, dst.data_ptr(), cap_arc, dd.tup, work.data_ptr(), ws, res.data_ptr(), 3, BS, True, True,
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    arc = bytes(dst[: int(res.item())].cpu().numpy())
    calls = [("takev", [BS - 16, 4 * BS + 48, 5]), ("take", 11), ("takev", [n - 5 * BS - 48])]
    for aligned in (True, False):
        rc, got, _ = _check(gpu, arc, n, calls, checksum=True, aligned=aligned, dd=dd, what="with its dictionary")
        assert rc == n and got == data
        rc, _, s = _check(gpu, arc, n, calls, checksum=True, aligned=aligned, what="without a dictionary")
        assert rc == ERR["DICT_REQUIRED"] and all(s.untouched(k) for k in range(3))


def test_a_table_written_on_the_stream_and_one_scratch_for_two_calls(gpu):
    n = 7 * BS + 9
    data = _payload(n, 44)
    arc = _archive(gpu, data)
    s = VSession(gpu, arc, n, max_piece=3 * BS, checksum=True)
    scratch = s.scratch(6)
    a = [BS + 40, 0, 17, 2 * BS + 32, 5]
    b = [1, BS, 33, n - sum(a) - BS - 34 - 100, 100, 0]
    s.takev(a, aligned=True, scratch=scratch, via_stream_copy=True)
    s.takev(b, aligned=False, scratch=scratch, via_stream_copy=True)
    s.end()
    rc, parts = s.result()
    assert rc == n and b"".join(parts) == data


def _bad_tables():
    def null(t):
        t[1]["base"] = 0                      # len > 0 and base == 0

    def big(t):
        t[1]["len"] = int(t["len"].sum()) + 1  # an entry longer than total (never dereferenced: the error comes first)

    return {"a zero base with a length": (null, 0, "NULL_INPUT"), "an entry longer than total": (big, 0, "OVERFLOW"),
            "a sum above total": (None, -1, "OVERFLOW"), "a sum below total": (None, +1, "DST_TOO_SMALL")}


def test_every_table_error(gpu):
    """the result at end; no byte of that call's entries written; the earlier call's entries intact; a later valid takev and take
    do not clear it (and, the result being final, deliver nothing through a copy)"""
    n = 9 * BS + 77
    data = _payload(n, 46)
    arc = _archive(gpu, data)
    first, bad = [BS + 40, 100], [7, 2 * BS + 32, 0, BS]
    for name, (mutate, delta, code) in _bad_tables().items():
        for aligned in (True, False):
            s = VSession(gpu, arc, n, max_piece=2 * BS, checksum=True)
            s.takev(first, aligned)
            k = s.takev(bad, aligned, total=sum(bad) + delta, mutate=mutate)
            left = n - sum(first) - sum(bad) - delta
            s.takev([left - 50, 20], aligned)
            s.take(30, aligned)
            s.end()
            rc, parts = s.result()
            assert rc == ERRV[code], (name, aligned, rc)
            assert s.untouched(k), name
            assert parts[0] == data[: sum(first)], name
    # the table error in the first call of a session: nothing at all is delivered
    s = VSession(gpu, arc, n, checksum=True)
    k = s.takev([n - 5, 5], True, mutate=_bad_tables()["a zero base with a length"][0])
    s.end()
    assert s.result()[0] == ERRV["NULL_INPUT"] and s.untouched(k)
    # total == 0 with a non-empty entry: the scan alone, and the error
    s = VSession(gpu, arc, n, checksum=True)
    k = s.takev([0, 3], True, total=0)
    s.takev([n], True)
    s.end()
    assert s.result()[0] == ERRV["OVERFLOW"] and s.untouched(k)


def test_a_bad_file_header_keeps_its_error_over_a_table_error(gpu):
    n = 3 * BS + 5
    data = _payload(n, 48)
    arc = bytearray(_archive(gpu, data))
    arc[0] ^= 0xFF  # the magic
    arc = bytes(arc)
    want_rc, _ = _oneshot(gpu, arc, n, BS, True)
    assert want_rc < 0
    s = VSession(gpu, arc, n, checksum=True)
    k = s.takev([BS, n - BS], True, mutate=_bad_tables()["a zero base with a length"][0])
    s.end()
    assert s.result()[0] == want_rc and s.untouched(k)
    # and the archive says 4 KiB blocks, the caller 64 KiB: nothing is written
    good = _archive(gpu, data)
    s = VSession(gpu, good, n, bs=65536, checksum=True)
    k = s.takev([BS, n - BS], True)
    s.end()
    assert s.result()[0] == ERR["BAD_BLOCK_SIZE"] and s.untouched(k)


def test_a_failing_block_gives_the_result_of_decompress_device(gpu):
    n = 8 * BS + 77
    data = _payload(n, 50)
    arc = _archive(gpu, data)
    at, size = _blocks_at(arc)[4]
    bad = bytearray(arc)
    bad[at + size - 2] ^= 0x10  # the checksum trailer of block 4
    bad = bytes(bad)
    lens = [BS + 16, 0, 2 * BS + 37, 5, n - 3 * BS - 58]
    for aligned in (True, False):
        rc, _, _ = _check(gpu, bad, n, [("takev", lens)], checksum=True, aligned=aligned, max_piece=3 * BS, what="trailer flipped")
        assert rc < 0
        rc, got, _ = _check(gpu, bad, n, [("takev", lens)], checksum=False, aligned=aligned, max_piece=3 * BS, what="trailer flipped, not verified")
        assert rc == n and got == data


def test_each_synchronous_refusal_leaves_the_session_usable(gpu):
    n = 3 * BS + 10
    data = _payload(n, 52)
    arc = _archive(gpu, data)
    s = VSession(gpu, arc, n, checksum=True)
    s.takev([BS - 1, 5], False)
    sc, ss = s.scratch(2)
    refusals = [(dict(lens=[n], total=None), "OVERFLOW"),                       # more than the capacity has left
                (dict(lens=[], total=5), "DST_TOO_SMALL"),                     # no entries for 5 bytes
                (dict(lens=[10, 10], total=None, scratch=(sc, ss - 1)), "MEMORY")]
    for kw, code in refusals:
        with pytest.raises(gpu.ZxcError) as e:
            s.takev(kw["lens"], True, total=kw["total"], scratch=kw.get("scratch"))
        assert e.value.code == ERRV[code], code
    with pytest.raises(gpu.ZxcError) as e:
        s.s.takev(0, 2, 20, sc.data_ptr(), ss, s.st)
    assert e.value.code == ERRV["NULL_INPUT"]
    with pytest.raises(gpu.ZxcError) as e:
        s.s.takev(sc.data_ptr(), 2, 20, 0, ss, s.st)
    assert e.value.code == ERRV["NULL_INPUT"]
    s.takev([], True)  # n_iov == 0 with total == 0: ZXC_OK, nothing enqueued
    s.takev([n - BS - 4], True)
    s.end()
    rc, parts = s.result()
    assert rc == n and b"".join(parts) == data


def test_round_trip_appendv_then_takev(gpu, ref):
    import ctypes as C
    import torch
    from zxc_amd.api import IOV_DTYPE
    n = 11 * BS + 17
    L = gpu.lib()
    L.zxc_compress_bound.restype = C.c_uint64
    L.zxc_compress_bound.argtypes = [C.c_size_t]
    for seed, checksum in ((54, 1), (55, 0)):
        data = _payload(n, seed)
        written = [3, 5 * BS, 0, BS - 3, 40, n - 6 * BS - 40]
        cap = int(L.zxc_compress_bound(n))
        st = torch.cuda.current_stream().cuda_stream
        ws = gpu.compress_append_device_work_size(n, 5 * BS, 3, BS, True, bool(checksum))
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
        res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        a = gpu.compress_begin_device(dst.data_ptr(), cap, n, 5 * BS, work.data_ptr(), ws, 3, BS, True, bool(checksum), st)
        table, keep, at = np.zeros(len(written), dtype=IOV_DTYPE), [], 0
        for i, m in enumerate(written):
            keep.append(_to_dev(data[at: at + m], 1))
            table[i] = (keep[-1].data_ptr() if m else 0, m)
            at += m
        d_iov = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
        ss = gpu.compress_appendv_device_scratch_size(len(written), 5 * BS, 3, BS, True, bool(checksum))
        sc = torch.empty(ss, dtype=torch.uint8, device="cuda")
        a.appendv(d_iov.data_ptr(), len(written), n, sc.data_ptr(), ss, st)
        a.end(res.data_ptr(), st)
        torch.cuda.synchronize()
        size = int(res.item())
        assert size > 0
        arc = bytes(dst[:size].cpu().numpy())
        back_n, back = ref.decompress(arc, n, checksum=bool(checksum))
        assert back_n == n and back == data
        read = [2 * BS + 32, 7, 0, 3 * BS + 1, n - 5 * BS - 40]  # a differently cut table
        for aligned in (True, False):
            rc, got, s = _check(gpu, arc, n, [("takev", read)], checksum=bool(checksum), aligned=aligned, max_piece=4 * BS, what="round trip")
            assert rc == n and got == data
