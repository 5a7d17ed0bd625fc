"""zxc_mi355x_decompress_rangesv_device / _dict_device on the GPU: many ranges of an archive in device memory fetched in one call,
each into a destination of its own at any alignment, named by its absolute device address. Every result equals what this library's
zxc_seekable_decompress_range returns for a host copy of the same bytes and a capacity of len, every valid range's bytes equal the
source's, and the pattern is intact everywhere else in every allocation. Archives from zxc_compress, from compress_device (opened
where they lie) and two goldens; ranges refused by status; a failed open; an index opened with another block size; a damaged block;
a dictionary; the range table written on the stream right before the call; two streams sharing one index; agreement with
zxc_mi355x_decompress_ranges_device. Nothing here provokes a fault: the corrupt inputs are those the host path is tested with,
which the kernels refuse by status, and a refused range's address is never dereferenced."""
import os
import random

import numpy as np
import pytest

import devtest
from conftest import GOLDEN, load_dict, read
from devtest import CANARY, ERR, PAD, UNSET, DevDict, pattern as _pattern

pytestmark = pytest.mark.gpu

gpu = devtest.gpu_fixture(needs="decompress_rangesv_device")

BS = 4096
GROUP = 8            # ranges per torch allocation
M64 = (1 << 64) - 1
ZERO_BASE, WRAP = "zero base", "wrap"   # table entries whose base is not the allocation's


def _text(n=9 * BS + 1000, seed=31):
    from zxc_amd import corpus
    return corpus.synth_text(n, seed=seed)


def _open(gpu, arc, n_arc, bs, max_blocks, stream=None):
    import torch
    s = torch.cuda.current_stream() if stream is None else stream
    isz = gpu.seekable_index_size(max_blocks)
    with torch.cuda.stream(s):
        index = torch.full(((isz + 7) // 8,), -1, dtype=torch.int64, device="cuda")
        gpu.seekable_open_device(arc.data_ptr(), n_arc, bs, max_blocks, index.data_ptr(), isz, s.cuda_stream)
    return index


def _index_status(index):
    return int(index[:1].cpu().numpy().view(np.int32)[0])


def _range_list(total, bs, rng, n_random, span=3):
    """the fixed list of the sibling's test and n_random seeded ranges of at most span blocks: (offset, len)"""
    nb = -(-total // bs)
    want = [(0, total), (0, 1), (total - 1, 1), (0, 0), (total, 0), (total + 5, 0), (total, 1), (total - 1, 2), (total + 1, 1),
            (min(7, total - 1), min(100, total - min(7, total - 1)))]
    if nb >= 2:
        want += [(bs - 3, 6), (bs, min(bs, total - bs)), (bs - 1, min(bs + 2, total - bs + 1)), (0, bs), (0, bs + 32), (0, bs + 31)]
    if nb >= 4:
        want += [(bs + 16, 2 * bs + 100), (5, 3 * bs), (2 * bs, bs + 40), (bs - 16, 2 * bs + 64), (0, 2 * bs), (bs, 3 * bs)]
    for _ in range(n_random):
        a = rng.randrange(total)
        want.append((a, rng.randrange(1, min(total - a, span * bs) + 1)))
    return want


class Dests:
    """One torch allocation per GROUP ranges, filled with the pattern; range i's destination starts CANARY + k behind the previous
    one's end (or the allocation's start), k making base = offset (mod 16) for even i and cycling 0..15 for odd i. kinds[i]:
    None, ZERO_BASE or WRAP: what the table says instead of that address (the allocation is judged all the same)."""

    def __init__(self, ranges, kinds=None, stream=None):
        import torch
        s = torch.cuda.current_stream() if stream is None else stream
        self.ranges, self.kinds = ranges, kinds or [None] * len(ranges)
        self.tensors, self.where = [], []
        for g in range(0, len(ranges), GROUP):
            at, offs = 0, []
            for i in range(g, min(g + GROUP, len(ranges))):
                a, n = ranges[i]
                at += CANARY
                k = (a - at) % 16 if i % 2 == 0 else (i >> 1) % 16   # (torch allocations are at least 16-byte aligned, asserted below)
                offs.append(at + k)
                at += k + n
            with torch.cuda.stream(s):
                t = torch.from_numpy(_pattern(at + CANARY)).to("cuda")
            assert t.data_ptr() % 16 == 0
            self.tensors.append(t)
            self.where += [(len(self.tensors) - 1, o) for o in offs]

    def table(self, gpu):
        t = np.zeros(max(len(self.ranges), 1), dtype=gpu.RANGEV_DTYPE)
        for i, ((a, n), kind, (ti, o)) in enumerate(zip(self.ranges, self.kinds, self.where)):
            base = self.tensors[ti].data_ptr() + o
            t[i] = (a, n, {None: base, ZERO_BASE: 0, WRAP: M64 - n // 2}[kind])
        return t

    def check(self, results, data, expect, what, undefined=()):
        """results[i] == expect(i, a, n); a valid range's bytes are the source's; the pattern everywhere else. undefined: the ranges
        that fail by a covered block, whose own bytes [base, base + len) the contract leaves undefined. -> the valid ranges"""
        host = [t.cpu().numpy() for t in self.tensors]
        keep = [np.zeros(len(h), dtype=bool) for h in host]
        n_valid = 0
        for i, ((a, n), rc, (ti, o)) in enumerate(zip(self.ranges, results, self.where)):
            exp = expect(i, a, n)
            assert rc == exp, (what, i, a, n, self.kinds[i], rc, exp)
            if i in undefined:
                assert rc < 0, (what, i, rc)
                keep[ti][o: o + n] = True
            elif rc == n and n:
                assert host[ti][o: o + n].tobytes() == data[a: a + n], (what, i, a, n, o % 16)
                keep[ti][o: o + n] = True
                n_valid += 1
        for h, k in zip(host, keep):
            assert np.array_equal(h[~k], _pattern(len(h))[~k]), what   # canaries, gaps, refused and failed-before-decode ranges
        return n_valid


def _fetch(gpu, arc, n_arc, index, table, n, max_len, bs, stream=None, dict_=False, sync=True, d_ranges=None):
    """-> the results as a list (sync) or (res, work, d_ranges) to keep alive. dict_: False the plain call, else the _dict call's tuple or None"""
    import torch
    s = torch.cuda.current_stream() if stream is None else stream
    ws = gpu.decompress_rangesv_device_work_size(n, max_len, bs)
    assert ws > 0
    with torch.cuda.stream(s):
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        res = torch.full((max(n, 1),), UNSET, dtype=torch.int64, device="cuda")
        if d_ranges is None:
            d_ranges = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
        if dict_ is False:
            gpu.decompress_rangesv_device(arc.data_ptr(), n_arc, index.data_ptr(), d_ranges.data_ptr(), n, max_len, bs, work.data_ptr(), ws,
                                          res.data_ptr(), s.cuda_stream)
        else:
            gpu.decompress_rangesv_dict_device(arc.data_ptr(), n_arc, index.data_ptr(), d_ranges.data_ptr(), n, max_len, bs, dict_,
                                               work.data_ptr(), ws, res.data_ptr(), s.cuda_stream)
    if not sync:
        return res, work, d_ranges
    s.synchronize()
    return [int(x) for x in res.cpu().numpy()[:n]]


def _host_expect(host, max_len, kinds=None):
    """zxc_seekable_decompress_range(offset, len, capacity = len) of this library on a host copy, with the two departures"""
    def expect(i, a, n):
        kind = kinds[i] if kinds else None
        if n == 0:
            return 0
        if n > max_len or kind == WRAP:
            return ERR["DST_TOO_SMALL"]
        if kind == ZERO_BASE:
            return ERR["NULL_INPUT"]
        return host.decompress_range(a, n, raise_on_error=False)[0]
    return expect


def _check(gpu, arc, comp, data, bs, what, n_random=230, seed=1, dict_=False, host_dict=None):
    rng = random.Random(seed)
    total = len(data)
    want = _range_list(total, bs, rng, n_random)
    index = _open(gpu, arc, len(comp), bs, -(-total // bs))
    host = gpu.Seekable(comp)
    if host_dict:
        assert host.set_dict(*host_dict) == 0
    try:
        # the whole archive as its own call (it would set max_len = total for every range otherwise), and then refused for its length
        max_len = max(n for a, n in want[1:] if a + n <= total)
        for ranges, ml in ((want, max_len), ([(0, total)], total)):
            dst = Dests(ranges)
            got = _fetch(gpu, arc, len(comp), index, dst.table(gpu), len(ranges), ml, bs, dict_=dict_)
            assert _index_status(index) == 0, what
            n_valid = dst.check(got, data, _host_expect(host, ml), (what, ml))
            assert n_valid >= min(len(ranges), n_random), (what, n_valid)
    finally:
        host.close()
    assert bytes(arc[: len(comp)].cpu().numpy()) == comp, what   # the archive is never written
    return index


@pytest.fixture(scope="module")
def text_archive(gpu):
    """~37 KiB of text in 4 KiB blocks by zxc_compress -> (data, comp, device tensor, index)"""
    data = _text()
    comp = gpu.compress(data, 3, BS, True, False)
    arc = devtest.to_dev(comp, PAD)
    return data, comp, arc, _open(gpu, arc, len(comp), BS, -(-len(data) // BS))


def test_ranges_of_a_host_written_archive(gpu):
    data = _text()
    assert len(data) == 9 * BS + 1000
    comp = gpu.compress(data, 3, BS, True, False)
    _check(gpu, devtest.to_dev(comp, PAD), comp, data, BS, "zxc_compress", seed=2)


def test_ranges_of_a_device_written_archive(gpu):
    """compress_device leaves the archive in HBM; it is opened and read where it lies"""
    import torch
    data = _text(seed=32)
    src = devtest.to_dev(data)
    bound = devtest.bound(gpu, len(data))
    ws = gpu.compress_device_work_size(len(data), 3, BS, True, True)
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    arc = torch.full((bound + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
    gpu.compress_device(src.data_ptr(), len(data), arc.data_ptr(), bound, work.data_ptr(), ws, res.data_ptr(), 3, BS, True, True)
    n_arc = int(res.item())
    assert n_arc > 0
    _check(gpu, arc, bytes(arc[:n_arc].cpu().numpy()), data, BS, "compress_device", seed=3)


@pytest.mark.parametrize("name", ["seekable_4blocks", "seekable_checksum"])
def test_ranges_of_golden_archives(gpu, name):
    comp, data = read(f"conformance/valid/{name}.zxc"), read(f"conformance/valid/{name}.expected")
    _check(gpu, devtest.to_dev(comp, PAD), comp, data, 1 << comp[5], name, seed=4)


def test_ranges_refused_by_status_leave_their_destinations_alone(gpu, text_archive):
    """len > max_len, a zero base with a length, base + len wrapping, an offset past the end: each between two valid ranges, each
    answered by status with its allocation untouched, the valid ones exact"""
    data, comp, arc, index = text_archive
    total, max_len = len(data), 2 * BS
    ranges, kinds = [], []
    for i in range(40):
        a, n = (i * 3779) % (total - 2 * BS), 1 + (i * 1237) % (2 * BS)
        bad = [((a, 2 * BS + 1), None), ((a, n), ZERO_BASE), ((a, n), WRAP), ((total + 1, 4), None), ((total - 5, 10), None),
               ((total + 9, n), ZERO_BASE), ((a, 0), ZERO_BASE), ((a, 2 * BS + 5), WRAP)][(i // 2) % 8]
        (r, kind) = bad if i % 2 else ((a, n), None)
        ranges.append(r)
        kinds.append(kind)
    dst = Dests(ranges, kinds)
    got = _fetch(gpu, arc, len(comp), index, dst.table(gpu), len(ranges), max_len, BS)
    host = gpu.Seekable(comp)
    try:
        assert dst.check(got, data, _host_expect(host, max_len, kinds), "refused") == 20
    finally:
        host.close()
    want = {ERR["DST_TOO_SMALL"], ERR["NULL_INPUT"], ERR["SRC_TOO_SMALL"], 0}
    assert want <= set(got), sorted(set(got))


def _expect_every_range(gpu, arc, n_arc, index, bs, want, what):
    ranges = [(0, 1), (5, 100), (0, 0), (0, 4096), (17, 5000)]
    dst = Dests(ranges)
    got = _fetch(gpu, arc, n_arc, index, dst.table(gpu), len(ranges), 8192, bs)
    assert got == [want, want, 0, want, want], (what, got)
    dst.check(got, b"", lambda i, a, n: want if n else 0, what)   # nothing is written


def test_a_failed_open_and_an_index_of_another_block_size_answer_every_range(gpu, text_archive):
    data, comp, arc, index = text_archive
    nb = -(-len(data) // BS)
    bad = comp[:-16] + comp[-12:]                                      # a truncated table, as the sibling's test cuts it
    bad_arc = devtest.to_dev(bad, PAD)
    bad_index = _open(gpu, bad_arc, len(bad), BS, nb)
    _expect_every_range(gpu, bad_arc, len(bad), bad_index, BS, ERR["CORRUPT_DATA"], "truncated table")
    assert _index_status(bad_index) == ERR["CORRUPT_DATA"]
    d = os.path.join(GOLDEN, "conformance", "invalid")
    seen = 0
    for f in sorted(os.listdir(d)):                                    # the invalid goldens whose table the host does not open
        raw = open(os.path.join(d, f), "rb").read()
        if not f.endswith(".zxc") or len(raw) < 44:
            continue
        try:
            gpu.Seekable(raw).close()
            continue
        except gpu.ZxcError:
            pass
        bs = 1 << raw[5] if 12 <= raw[5] <= 21 else 65536
        g_arc = devtest.to_dev(raw, PAD)
        g_index = _open(gpu, g_arc, len(raw), bs, 64)
        st = _index_status(g_index)
        assert st < 0, f
        _expect_every_range(gpu, g_arc, len(raw), g_index, bs, st, f)
        seen += 1
    assert seen >= 1
    assert _index_status(index) == 0                                   # opened with 4096, called with 8192
    _expect_every_range(gpu, arc, len(comp), index, 8192, ERR["BAD_BLOCK_SIZE"], "another block size")


def test_a_damaged_block(gpu):
    """the sibling test's recipe: one block's n_seq field overwritten with far too many sequences for its payload (the input of the
    host's range test), which the decoder refuses by status. Ranges that touch the block get the host call's code, every other range
    is exact, and nothing leaves a destination."""
    from zxc_amd import corpus
    bs, hit = 65536, 4
    data = corpus.synth_text(8 * bs + 4321, seed=25)
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
        index = _open(gpu, arc, len(bad), bs, len(jobs))
        dst = Dests(ranges)
        got = _fetch(gpu, arc, len(bad), index, dst.table(gpu), len(ranges), 4 * bs, bs)
        touched = [a // bs <= hit <= (a + n - 1) // bs for a, n in ranges]
        n_valid = dst.check(got, data, _host_expect(host, 4 * bs), "damaged", undefined={i for i, t in enumerate(touched) if t})
        assert all((rc == want_rc) == t for rc, t in zip(got, touched)) and sum(touched) >= 8 and n_valid == len(ranges) - sum(touched)
    finally:
        host.close()


def test_with_a_dictionary(gpu):
    comp, data = read("conformance/valid/dict_seekable_l7.zxc"), read("conformance/valid/dict_seekable_l7.expected")
    content, huf = load_dict(os.path.join(GOLDEN, "conformance", "valid", "dict_text.zxd"))
    bs = 1 << comp[5]
    right, wrong = DevDict(gpu, content, huf), DevDict(gpu, content, None)
    assert right.id() != wrong.id()
    arc = devtest.to_dev(comp, PAD)
    index = _check(gpu, arc, comp, data, bs, "dict_seekable_l7", n_random=60, seed=5, dict_=right.tup, host_dict=(content, huf))
    ranges = _range_list(len(data), bs, random.Random(6), 20)[1:]
    max_len = max(n for a, n in ranges if a + n <= len(data))
    for dict_, code in ((False, "DICT_REQUIRED"), (None, "DICT_REQUIRED"), (wrong.tup, "DICT_MISMATCH")):
        dst = Dests(ranges)
        got = _fetch(gpu, arc, len(comp), index, dst.table(gpu), len(ranges), max_len, bs, dict_=dict_)

        def expect(i, a, n, code=code):   # the checks in front of the dictionary's keep their answers
            if n == 0:
                return 0
            if a > len(data) or n > len(data) - a:
                return ERR["SRC_TOO_SMALL"]
            return ERR[code]
        assert dst.check(got, data, expect, code) == 0   # every destination untouched


def test_the_call_is_ordered_behind_the_kernel_that_writes_its_range_table(gpu, text_archive):
    """the table is all zeroes (every range empty) until a device copy enqueued on the call's stream right before the call has run;
    nothing synchronises between the two"""
    import torch
    data, comp, arc, index = text_archive
    ranges = _range_list(len(data), BS, random.Random(8), 100)[1:]
    max_len = max(n for a, n in ranges if a + n <= len(data))
    s = torch.cuda.Stream()
    dst = Dests(ranges, stream=s)
    with torch.cuda.stream(s):
        good = torch.from_numpy(dst.table(gpu).view(np.uint8).copy()).to("cuda")
        rt = torch.zeros_like(good)
    s.synchronize()
    with torch.cuda.stream(s):
        rt.copy_(good, non_blocking=True)
        res, work, _ = _fetch(gpu, arc, len(comp), index, None, len(ranges), max_len, BS, stream=s, sync=False, d_ranges=rt)
    s.synchronize()
    host = gpu.Seekable(comp)
    try:
        got = [int(x) for x in res.cpu().numpy()[: len(ranges)]]
        assert dst.check(got, data, _host_expect(host, max_len), "stream order") >= 100
    finally:
        host.close()


def test_two_streams_share_one_index(gpu, text_archive):
    import torch
    data, comp, arc, index = text_archive
    torch.cuda.synchronize()
    runs = []
    for k, s in enumerate((torch.cuda.Stream(), torch.cuda.Stream())):
        ranges = _range_list(len(data), BS, random.Random(20 + k), 120)[1:]
        dst = Dests(ranges, stream=s)
        with torch.cuda.stream(s):
            rt = torch.from_numpy(dst.table(gpu).view(np.uint8).copy()).to("cuda")
        runs.append((s, ranges, dst, rt, max(n for a, n in ranges if a + n <= len(data))))
    torch.cuda.synchronize()
    out = [_fetch(gpu, arc, len(comp), index, None, len(ranges), ml, BS, stream=s, sync=False, d_ranges=rt) for s, ranges, dst, rt, ml in runs]
    host = gpu.Seekable(comp)
    try:
        for (s, ranges, dst, rt, ml), (res, work, _) in zip(runs, out):
            s.synchronize()
            got = [int(x) for x in res.cpu().numpy()[: len(ranges)]]
            assert dst.check(got, data, _host_expect(host, ml), "two streams") >= 120
    finally:
        host.close()


def test_agreement_with_the_sibling(gpu, text_archive):
    """the same (offset, len) list fetched by decompress_ranges_device into one buffer: the same bytes and, where the checks
    coincide (every range here: none is refused for its destination), the same results"""
    import torch
    data, comp, arc, index = text_archive
    ranges = _range_list(len(data), BS, random.Random(9), 150)[1:]
    max_len = max(n for a, n in ranges if a + n <= len(data))
    n = len(ranges)
    dst = Dests(ranges)
    got = _fetch(gpu, arc, len(comp), index, dst.table(gpu), n, max_len, BS)
    table, at = np.zeros(n, dtype=gpu.RANGE_DTYPE), 0
    for i, (a, ln) in enumerate(ranges):
        d = at + ((a & 15) if i % 2 == 0 else (i >> 1) % 16)
        table[i] = (a, ln, d)
        at = (d + ln + 31) // 16 * 16
    cap = at + 64
    ws = gpu.decompress_ranges_device_work_size(n, max_len, BS)
    assert ws == gpu.decompress_rangesv_device_work_size(n, max_len, BS)
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    one = torch.from_numpy(_pattern(cap + CANARY)).to("cuda")
    res = torch.full((n,), UNSET, dtype=torch.int64, device="cuda")
    rt = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
    gpu.decompress_ranges_device(arc.data_ptr(), len(comp), index.data_ptr(), rt.data_ptr(), n, max_len, one.data_ptr(), cap, BS,
                                 work.data_ptr(), ws, res.data_ptr())
    torch.cuda.synchronize()
    sib, one = [int(x) for x in res.cpu().numpy()], one.cpu().numpy()
    assert sib == got
    host = [t.cpu().numpy() for t in dst.tensors]
    same = 0
    for (a, ln), rc, (ti, o), row in zip(ranges, got, dst.where, table):
        if rc == ln and ln:
            d = int(row["dst_off"])
            assert host[ti][o: o + ln].tobytes() == one[d: d + ln].tobytes() == data[a: a + ln], (a, ln)
            same += 1
    assert same >= 150
