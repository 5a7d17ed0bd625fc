"""zxc_mi355x_decompress_rangesv_shuffle_device on the GPU: many ranges of the plain bytes of an archive of byte-shuffled blocks
fetched in one call, each into a destination of its own at any alignment, named by its absolute device address. Every result
equals what this library's zxc_seekable_decompress_range returns for a host copy of the same archive, (offset, len) and a capacity
of len (with rangesv's two departures), every valid range's bytes equal the plain source's, and the pattern is intact everywhere
else in every allocation. Archives from zxc_compress over np_shuffle of a typed tensor and from compress_shuffle_device (opened
where they lie), each element size, 4 KiB and 16 KiB blocks; ranges refused by status; a failed open; an index opened with another
block size; a damaged block; a dictionary; the range table written on the stream right before the call; two streams sharing one
index; agreement with decompress_ranges_device followed by unshuffle_device on block-aligned ranges. Nothing here provokes a fault:
the corrupt inputs are those the host path is tested with, which the kernels refuse by status, and a refused range's address is
never dereferenced."""
import os
import random

import numpy as np
import pytest

import devtest
import rangesv_shuffle_support as rs
import shuffle_support as ss
from conftest import GOLDEN, load_dict, read
from devtest import CANARY, ERR, PAD, UNSET, DevDict, pattern
from rangesv_shuffle_support import WRAP, ZERO_BASE, Dests

pytestmark = pytest.mark.gpu

gpu = devtest.gpu_fixture(needs="decompress_rangesv_shuffle_device")

BS = 4096


def _unshuffled(decoded, E, bs):
    return ss.np_unshuffle(np.frombuffer(decoded, dtype=np.uint8), E, bs).tobytes()


def _check(gpu, arc, comp, plain, E, bs, what, n_random=230, seed=1, dict_=None, host_dict=None):
    """about 250 ranges in one call, then the whole archive as a call of its own. arc: a tensor, or the device address of the archive"""
    rng = random.Random(seed)
    total = len(plain)
    want = rs.range_list(total, bs, rng, n_random)
    ptr = arc if isinstance(arc, int) else arc.data_ptr()
    index = rs.open_device(gpu, _Ptr(ptr), len(comp), bs, -(-total // bs))
    host = gpu.Seekable(comp)
    if host_dict:
        assert host.set_dict(*host_dict) == 0
    try:
        max_len = max(n for a, n in want[1:] if a + n <= total)
        for ranges, ml in ((want, max_len), ([(0, total)], total)):
            dst = Dests(ranges)
            got = rs.fetch(gpu, _Ptr(ptr), len(comp), index, dst.table(gpu), len(ranges), ml, E, bs, dict_=dict_)
            assert rs.index_status(index) == 0, what
            n_valid = dst.check(got, plain, rs.host_expect(host, ml), (what, ml))
            assert n_valid >= min(len(ranges), n_random), (what, n_valid)
    finally:
        host.close()
    return index


class _Ptr:
    """a device address where the helpers take a tensor"""

    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


@pytest.mark.parametrize("bs", sorted(rs.SIZES))
@pytest.mark.parametrize("E", rs.ELEMS)
def test_ranges_of_a_host_written_archive(gpu, E, bs):
    plain, shuffled = rs.plain_and_shuffled(E, bs)
    comp = gpu.compress(shuffled, 3, bs, True, False)
    arc = devtest.to_dev(comp, PAD)
    _check(gpu, arc, comp, plain, E, bs, ("zxc_compress", E, bs), seed=2 + E)
    assert bytes(arc[: len(comp)].cpu().numpy()) == comp   # the archive is never written


@pytest.mark.parametrize("bs", sorted(rs.SIZES))
@pytest.mark.parametrize("E", rs.ELEMS)
def test_ranges_of_a_device_written_archive(gpu, E, bs):
    """compress_shuffle_device leaves the archive in HBM; it is opened and read where it lies, at an odd address"""
    plain, shuffled = rs.plain_and_shuffled(E, bs, seed=40 + E)
    c = ss.Compress(gpu, plain, E, devtest.bound(gpu, len(plain)), 0, level=3, bs=bs, seekable=True, dst_off=3)
    n_arc, comp = c.result()
    assert n_arc > 0 and gpu.decompress(comp) == shuffled
    _check(gpu, c.dst.ptr, comp, plain, E, bs, ("compress_shuffle_device", E, bs), seed=3 + E)
    assert c.dst.read()[:n_arc] == comp                     # the archive is never written, nor anything around it


@pytest.fixture(scope="module")
def tensor_archive(gpu):
    """fp32 weights (E = 4), nine blocks of 4 KiB and a ragged one, by zxc_compress -> (plain, comp, device tensor, index)"""
    plain, shuffled = rs.plain_and_shuffled(4, BS)
    comp = gpu.compress(shuffled, 3, BS, True, False)
    arc = devtest.to_dev(comp, PAD)
    return plain, comp, arc, rs.open_device(gpu, arc, len(comp), BS, -(-len(plain) // BS))


def test_ranges_refused_by_status_leave_their_destinations_alone(gpu, tensor_archive):
    """len > max_len, a zero base with a length, base + len wrapping, an offset past the end: each between two valid ranges, each
    answered by status with its allocation untouched, the valid ones exact"""
    plain, comp, arc, index = tensor_archive
    total, max_len = len(plain), 2 * BS
    ranges, kinds = [], []
    for i in range(40):
        a, n = (i * 3779) % (total - 2 * BS), 1 + (i * 1237) % (2 * BS)
        bad = [((a, 2 * BS + 1), None), ((a, n), ZERO_BASE), ((a, n), WRAP), ((total + 1, 4), None), ((total - 5, 10), None),
               ((total + 9, n), ZERO_BASE), ((a, 0), ZERO_BASE), ((a, 2 * BS + 5), WRAP)][(i // 2) % 8]
        (r, kind) = bad if i % 2 else ((a, n), None)
        ranges.append(r)
        kinds.append(kind)
    dst = Dests(ranges, kinds)
    got = rs.fetch(gpu, arc, len(comp), index, dst.table(gpu), len(ranges), max_len, 4, BS)
    host = gpu.Seekable(comp)
    try:
        assert dst.check(got, plain, rs.host_expect(host, max_len, kinds), "refused") == 20
    finally:
        host.close()
    assert {ERR["DST_TOO_SMALL"], ERR["NULL_INPUT"], ERR["SRC_TOO_SMALL"], 0} <= set(got), sorted(set(got))


def _expect_every_range(gpu, arc, n_arc, index, bs, want, what):
    ranges = [(0, 1), (5, 100), (0, 0), (0, 4096), (17, 5000)]
    dst = Dests(ranges)
    got = rs.fetch(gpu, arc, n_arc, index, dst.table(gpu), len(ranges), 8192, 2, bs)
    assert got == [want, want, 0, want, want], (what, got)
    dst.check(got, b"", lambda i, a, n: want if n else 0, what)   # nothing is written


def test_a_failed_open_and_an_index_of_another_block_size_answer_every_range(gpu, tensor_archive):
    plain, comp, arc, index = tensor_archive
    nb = -(-len(plain) // BS)
    bad = comp[:-16] + comp[-12:]                                      # a truncated table, as the sibling's test cuts it
    bad_arc = devtest.to_dev(bad, PAD)
    bad_index = rs.open_device(gpu, bad_arc, len(bad), BS, nb)
    _expect_every_range(gpu, bad_arc, len(bad), bad_index, BS, ERR["CORRUPT_DATA"], "truncated table")
    assert rs.index_status(bad_index) == ERR["CORRUPT_DATA"]
    assert rs.index_status(index) == 0                                 # opened with 4096, called with 8192
    _expect_every_range(gpu, arc, len(comp), index, 8192, ERR["BAD_BLOCK_SIZE"], "another block size")


@pytest.mark.parametrize("E", rs.ELEMS)
def test_a_damaged_block(gpu, E):
    """the sibling test's recipe on its text archive, read as a shuffled one: one block's n_seq field overwritten with far too many
    sequences for its payload, which the decoder refuses by status. Ranges that touch the block get the host call's code, every
    other range is exact, and nothing leaves a destination."""
    from zxc_amd import corpus
    bs, hit = 65536, 4
    data = corpus.synth_text(8 * bs + 4321, seed=25)
    plain = _unshuffled(data, E, bs)
    comp = gpu.compress(data, 3, bs, True, False)
    s = gpu.Seekable(comp)
    jobs = s.plan()
    s.close()
    bad = bytearray(comp)
    o = int(jobs["comp_off"][hit]) + 8
    bad[o:o + 4] = (0x00FFFFFF).to_bytes(4, "little")
    bad = bytes(bad)
    host = gpu.Seekable(bad)
    try:
        want_rc, _ = host.decompress_range(0, len(data), raise_on_error=False)
        assert want_rc < 0
        rng = random.Random(40)
        ranges = [(0, hit * bs), ((hit + 1) * bs, 3 * bs), (hit * bs, 1), ((hit + 1) * bs - 1, 1), ((hit - 1) * bs + 5, 2 * bs), (hit * bs - 1, 1),
                  ((hit - 2) * bs, 4 * bs), (hit * bs, bs + 32), ((hit + 1) * bs, bs + 32)]
        for _ in range(40):
            a = rng.randrange(0, len(data) - 3 * bs)
            ranges.append((a, rng.randrange(1, 3 * bs)))
        arc = devtest.to_dev(bad, PAD)
        index = rs.open_device(gpu, arc, len(bad), bs, len(jobs))
        dst = Dests(ranges)
        got = rs.fetch(gpu, arc, len(bad), index, dst.table(gpu), len(ranges), 4 * bs, E, bs)
        touched = [a // bs <= hit <= (a + n - 1) // bs for a, n in ranges]
        n_valid = dst.check(got, plain, rs.host_expect(host, 4 * bs), "damaged", undefined={i for i, t in enumerate(touched) if t})
        assert all((rc == want_rc) == t for rc, t in zip(got, touched)) and sum(touched) >= 8 and n_valid == len(ranges) - sum(touched)
    finally:
        host.close()


def test_with_a_dictionary(gpu):
    comp, data = read("conformance/valid/dict_seekable_l7.zxc"), read("conformance/valid/dict_seekable_l7.expected")
    content, huf = load_dict(os.path.join(GOLDEN, "conformance", "valid", "dict_text.zxd"))
    bs, E = 1 << comp[5], 2
    plain = _unshuffled(data, E, bs)
    right, wrong = DevDict(gpu, content, huf), DevDict(gpu, content, None)
    assert right.id() != wrong.id()
    arc = devtest.to_dev(comp, PAD)
    index = _check(gpu, arc, comp, plain, E, bs, "dict_seekable_l7", n_random=60, seed=5, dict_=right.tup, host_dict=(content, huf))
    ranges = rs.range_list(len(data), bs, random.Random(6), 20)[1:]
    max_len = max(n for a, n in ranges if a + n <= len(data))
    for dict_, code in ((None, "DICT_REQUIRED"), ((0, 0, 0, 0), "DICT_REQUIRED"), (wrong.tup, "DICT_MISMATCH")):
        dst = Dests(ranges)
        got = rs.fetch(gpu, arc, len(comp), index, dst.table(gpu), len(ranges), max_len, E, bs, dict_=dict_)

        def expect(i, a, n, code=code):   # the checks in front of the dictionary's keep their answers
            if n == 0:
                return 0
            if a > len(data) or n > len(data) - a:
                return ERR["SRC_TOO_SMALL"]
            return ERR[code]
        assert dst.check(got, plain, expect, code) == 0   # every destination untouched


def test_the_call_is_ordered_behind_the_kernel_that_writes_its_range_table(gpu, tensor_archive):
    """the table is all zeroes (every range empty) until a device copy enqueued on the call's stream right before the call has run;
    nothing synchronises between the two"""
    import torch
    plain, comp, arc, index = tensor_archive
    ranges = rs.range_list(len(plain), BS, random.Random(8), 100)[1:]
    max_len = max(n for a, n in ranges if a + n <= len(plain))
    s = torch.cuda.Stream()
    dst = Dests(ranges, stream=s)
    with torch.cuda.stream(s):
        good = torch.from_numpy(dst.table(gpu).view(np.uint8).copy()).to("cuda")
        rt = torch.zeros_like(good)
    s.synchronize()
    with torch.cuda.stream(s):
        rt.copy_(good, non_blocking=True)
        res, work, _ = rs.fetch(gpu, arc, len(comp), index, None, len(ranges), max_len, 4, BS, stream=s, sync=False, d_ranges=rt)
    s.synchronize()
    host = gpu.Seekable(comp)
    try:
        got = [int(x) for x in res.cpu().numpy()[: len(ranges)]]
        assert dst.check(got, plain, rs.host_expect(host, max_len), "stream order") >= 100
    finally:
        host.close()


def test_two_streams_share_one_index(gpu, tensor_archive):
    import torch
    plain, comp, arc, index = tensor_archive
    torch.cuda.synchronize()
    runs = []
    for k, s in enumerate((torch.cuda.Stream(), torch.cuda.Stream())):
        ranges = rs.range_list(len(plain), BS, random.Random(20 + k), 120)[1:]
        dst = Dests(ranges, stream=s)
        with torch.cuda.stream(s):
            rt = torch.from_numpy(dst.table(gpu).view(np.uint8).copy()).to("cuda")
        runs.append((s, ranges, dst, rt, max(n for a, n in ranges if a + n <= len(plain))))
    torch.cuda.synchronize()
    out = [rs.fetch(gpu, arc, len(comp), index, None, len(ranges), ml, 4, BS, stream=s, sync=False, d_ranges=rt) for s, ranges, dst, rt, ml in runs]
    host = gpu.Seekable(comp)
    try:
        for (s, ranges, dst, rt, ml), (res, work, _) in zip(runs, out):
            s.synchronize()
            got = [int(x) for x in res.cpu().numpy()[: len(ranges)]]
            assert dst.check(got, plain, rs.host_expect(host, ml), "two streams") >= 120
    finally:
        host.close()


@pytest.mark.parametrize("bs", sorted(rs.SIZES))
@pytest.mark.parametrize("E", rs.ELEMS)
def test_agreement_with_ranges_then_unshuffle_on_block_aligned_ranges(gpu, E, bs):
    """today's path for the ranges it can serve: every run of whole blocks (the one that reaches the ragged end included) fetched by
    decompress_ranges_device into one buffer and un-shuffled range by range with unit = block_size gives the bytes and the results
    the new call gives for the same (offset, len) list"""
    import torch
    plain, shuffled = rs.plain_and_shuffled(E, bs)
    total, nb = len(plain), -(-len(plain) // bs)
    comp = gpu.compress(shuffled, 3, bs, True, False)
    arc = devtest.to_dev(comp, PAD)
    index = rs.open_device(gpu, arc, len(comp), bs, nb)
    ranges = [(b * bs, min(k * bs, total - b * bs)) for b in range(nb) for k in (1, 2, 3) if b + k <= nb]
    n, max_len = len(ranges), 3 * bs
    dst = Dests(ranges)
    got = rs.fetch(gpu, arc, len(comp), index, dst.table(gpu), n, max_len, E, bs)
    assert got == [ln for _, ln in ranges]
    table, at = np.zeros(n, dtype=gpu.RANGE_DTYPE), 0
    for i, (a, ln) in enumerate(ranges):
        table[i] = (a, ln, at)
        at = (at + ln + 31) // 16 * 16
    cap = at + 64
    ws = gpu.decompress_ranges_device_work_size(n, max_len, bs)
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    one = torch.from_numpy(pattern(cap + CANARY)).to("cuda")
    two = torch.from_numpy(pattern(cap + CANARY)).to("cuda")
    res = torch.full((n,), UNSET, dtype=torch.int64, device="cuda")
    rt = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
    gpu.decompress_ranges_device(arc.data_ptr(), len(comp), index.data_ptr(), rt.data_ptr(), n, max_len, one.data_ptr(), cap, bs,
                                 work.data_ptr(), ws, res.data_ptr())
    for row in table:
        gpu.unshuffle_device(one.data_ptr() + int(row["dst_off"]), two.data_ptr() + int(row["dst_off"]), int(row["len"]), E, bs)
    torch.cuda.synchronize()
    assert [int(x) for x in res.cpu().numpy()] == got
    two, host = two.cpu().numpy(), [t.cpu().numpy() for t in dst.tensors]
    for (a, ln), (ti, o), row in zip(ranges, dst.where, table):
        d = int(row["dst_off"])
        assert host[ti][o: o + ln].tobytes() == two[d: d + ln].tobytes() == plain[a: a + ln], (a, ln)
    dst.check(got, plain, lambda i, a, ln: ln, "block-aligned")
