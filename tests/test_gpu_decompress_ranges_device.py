"""zxc_mi355x_seekable_open_device + zxc_mi355x_decompress_ranges_device on the GPU: many ranges of an archive in device memory fetched
into device memory in one call, every result equal to what this library's zxc_seekable_decompress_range returns for a host copy of the
same bytes, every valid range's bytes equal to the source's, and a canary pattern intact everywhere outside the valid ranges. Archives
from zxc_compress, from compress_device (opened where they lie) and from the unmodified reference; failed opens; a damaged block;
many jobs; two streams sharing one index; stream order behind the kernel that wrote the range table. Nothing here provokes a fault:
the corrupt inputs are those the host path is tested with, and the kernels refuse them by status."""
import os
import random

import numpy as np
import pytest

import devtest
from conftest import GOLDEN
from devtest import CANARY, ERR, PAD, UNSET, pattern as _pattern

pytestmark = pytest.mark.gpu

DICT_ARCHIVES = ("conformance/valid/dict_http.zxc", "conformance/valid/dict_seekable_l7.zxc", "conformance/invalid/dict_required.zxc")

gpu = devtest.gpu_fixture()


def _to_dev(data: bytes, pad=PAD):
    return devtest.to_dev(data, pad)


def _open(gpu, arc, n_arc, bs, max_blocks, stream=None):
    """-> the index tensor (int64 words: 16-byte aligned like every torch allocation)"""
    import torch
    s = torch.cuda.current_stream() if stream is None else stream
    isz = gpu.seekable_index_size(max_blocks)
    with torch.cuda.stream(s):
        index = torch.full(((isz + 7) // 8,), -1, dtype=torch.int64, device="cuda")
        gpu.seekable_open_device(arc.data_ptr(), n_arc, bs, max_blocks, index.data_ptr(), isz, s.cuda_stream)
    return index


def _index_status(index):
    return int(index[:1].cpu().numpy().view(np.int32)[0])


def _range_table(ranges):
    t = np.zeros(len(ranges), dtype=[("offset", "<u8"), ("len", "<u8"), ("dst_off", "<u8")])
    for i, (a, n, d) in enumerate(ranges):
        t[i] = (a, n, d)
    return t


def _fetch(gpu, arc, n_arc, index, ranges, max_len, cap, bs, stream=None, sync=True, d_ranges=None):
    """-> (results as a list, dst as numpy of cap + CANARY bytes); dst starts as the pattern everywhere"""
    import torch
    s = torch.cuda.current_stream() if stream is None else stream
    n = len(ranges)
    ws = gpu.decompress_ranges_device_work_size(n, max_len, bs)
    assert ws > 0
    with torch.cuda.stream(s):
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        dst = torch.from_numpy(_pattern(cap + CANARY)).to("cuda")
        res = torch.full((max(n, 1),), UNSET, dtype=torch.int64, device="cuda")
        if d_ranges is None:
            d_ranges = torch.from_numpy(_range_table(ranges).view(np.uint8).copy()).to("cuda")
        gpu.decompress_ranges_device(arc.data_ptr(), n_arc, index.data_ptr(), d_ranges.data_ptr(), n, max_len, dst.data_ptr(), cap, bs,
                                     work.data_ptr(), ws, res.data_ptr(), s.cuda_stream)
    if not sync:
        return res, dst, work, d_ranges
    s.synchronize()
    return [int(x) for x in res.cpu().numpy()[:n]], dst.cpu().numpy()


def _range_list(total, bs, rng, n_random, span=3):
    """(offset, len) of the fixed list and n_random seeded ones of at most span blocks"""
    nb = -(-total // bs)
    want = [(0, total), (0, 1), (total - 1, 1), (0, 0), (total, 0), (total + 5, 0), (total, 1), (total - 1, 2), (total + 1, 1),
            (min(7, total - 1), min(100, total - min(7, total - 1)))]
    if nb >= 2:
        want += [(bs - 3, 6), (bs, min(bs, total - bs)), (bs - 1, min(bs + 2, total - bs + 1)), (0, bs), (0, bs + 32), (0, bs + 31)]
    if nb >= 4:
        want += [(bs + 16, 2 * bs + 100), (5, 3 * bs), (2 * bs, bs + 40), (bs - 16, 2 * bs + 64)]
    for _ in range(n_random):
        a = rng.randrange(total)
        want.append((a, rng.randrange(1, min(total - a, span * bs) + 1)))
    return want


def _place(want, total, rng):
    """destinations with gaps, every other one with dst_off = offset (mod 16); then the refused kinds.
    -> (ranges, max_len, capacity)"""
    out, at = [], 0
    for i, (a, n) in enumerate(want):
        at = (at + 15) // 16 * 16 + 16 * rng.randrange(3)
        d = at + ((a & 15) if i % 2 == 0 else ((a & 15) + 1 + rng.randrange(15)) % 16)
        out.append((a, n, d))
        at = d + n
    max_len = max([n for a, n, d in out if a + n <= total] + [1])
    cap = at + 64
    out.append((0, min(total, max_len) + 1, at + 32))   # len > max_len (and, where max_len == total, past the end)
    out.append((0, min(total, 50), cap - 10))            # passes the capacity
    out.append((0, 1, cap + 1))                          # starts behind it
    out.append((1, 1, (1 << 64) - 1))                    # dst_off + len wraps
    return out, max_len, cap


def _check(gpu, arc, comp, data, bs, what, n_random=200, seed=1, index=None):
    """one call with the fixed list + n_random ranges against the host's range call on `comp`"""
    rng = random.Random(seed)
    total = len(data)
    want = _range_list(total, bs, rng, n_random, span=3 if bs <= 65536 else 2)
    # the whole archive once, as its own call (it would set max_len = total for every range otherwise)
    ranges, max_len, cap = _place(want[1:], total, rng)
    if index is None:
        index = _open(gpu, arc, len(comp), bs, -(-total // bs))
    for rs, ml, cp in ((ranges, max_len, cap), ([(0, total, 0)], total, total)):
        got, dst = _fetch(gpu, arc, len(comp), index, rs, ml, cp, bs)
        assert _index_status(index) == 0, what
        host = gpu.Seekable(comp)
        keep = np.zeros(len(dst), dtype=bool)
        try:
            for (a, n, d), rc in zip(rs, got):
                w = (what, a, n, d, ml)
                if n > ml or d > cp or n > cp - d:
                    exp = ERR["DST_TOO_SMALL"] if n else 0
                else:
                    exp, _ = host.decompress_range(a, n, raise_on_error=False)
                assert rc == exp, (w, rc, exp)
                if rc == n and n:
                    assert dst[d: d + n].tobytes() == data[a: a + n], w
                    keep[d: d + n] = True
        finally:
            host.close()
        assert np.array_equal(dst[~keep], _pattern(len(dst))[~keep]), what   # gaps, refused ranges, behind the capacity
    assert bytes(arc[: len(comp)].cpu().numpy()) == comp, what               # the archive is never written
    return index


def _data(bs, blocks=5):
    from zxc_amd import corpus
    rng = np.random.default_rng(bs)
    n = blocks * bs + 1 + bs // 3
    text = corpus.synth_text(n, seed=bs & 0xFFFF)
    rnd = rng.integers(0, 256, bs + 77, dtype=np.uint8).tobytes()
    return (text[: 2 * bs + 11] + rnd + bytes(bs // 2) + text)[:n]


@pytest.mark.parametrize("bs", [4096, 65536, 1 << 19, 1 << 21])
@pytest.mark.parametrize("level", [1, 3, 6, 7])
def test_ranges_of_host_written_archives(gpu, level, bs):
    data = _data(bs, 5 if bs <= (1 << 19) else 3)
    for checksum in (False, True):
        comp = gpu.compress(data, level, bs, True, checksum)
        _check(gpu, _to_dev(comp), comp, data, bs, ("zxc_compress", level, bs, checksum), seed=level * 7 + checksum)


@pytest.mark.parametrize("bs", [4096, 65536, 1 << 19, 1 << 21])
@pytest.mark.parametrize("level", [1, 3, 6, 7])
def test_ranges_of_device_written_archives(gpu, level, bs):
    """compress_device leaves the archive in HBM; it is opened and read where it lies"""
    import torch
    data = _data(bs, 5 if bs <= (1 << 19) else 3)
    src = _to_dev(data, 0)
    for checksum in (False, True):
        bound = int(gpu.lib().zxc_compress_bound(len(data)))
        ws = gpu.compress_device_work_size(len(data), level, bs, True, checksum)
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        arc = torch.full((bound + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        gpu.compress_device(src.data_ptr(), len(data), arc.data_ptr(), bound, work.data_ptr(), ws, res.data_ptr(), level, bs, True, checksum)
        n_arc = int(res.item())
        assert n_arc > 0
        comp = bytes(arc[:n_arc].cpu().numpy())
        _check(gpu, arc, comp, data, bs, ("compress_device", level, bs, checksum), seed=level * 11 + checksum)


@pytest.mark.parametrize("bs", [4096, 65536, 1 << 19, 1 << 21])
def test_ranges_of_reference_archives(gpu, ref, bs):
    data = _data(bs, 5 if bs <= (1 << 19) else 3)
    for level in (1, 3, 6, 7):
        for checksum in (False, True):
            comp = ref.compress(data, level, bs, True, checksum)
            _check(gpu, _to_dev(comp), comp, data, bs, ("reference", level, bs, checksum), n_random=100, seed=level)


def test_valid_and_invalid_ranges_do_not_disturb_each_other(gpu):
    bs = 65536
    data = _data(bs, 6)
    comp = gpu.compress(data, 3, bs, True, False)
    arc = _to_dev(comp)
    index = _open(gpu, arc, len(comp), bs, -(-len(data) // bs))
    total = len(data)
    # good and refused ranges alternate, the refused ones' destinations lie between the good ones'
    ranges, at = [], 0
    for i in range(60):
        a = (i * 37717) % (total - 3 * bs)
        n = 1 + (i * 7919) % (2 * bs)
        bad = [(total - 5, 10), (total + 1, 4), (a, 2 * bs + 1), (a, n)][i % 4] if i % 2 else (a, n)
        d = at + (a & 15 if i % 4 == 0 else 3)
        ranges.append((bad[0], bad[1], d))
        at = (d + n + 31) // 16 * 16
    got, dst = _fetch(gpu, arc, len(comp), index, ranges, 2 * bs, at + 64, bs)
    keep = np.zeros(len(dst), dtype=bool)
    for i, ((a, n, d), rc) in enumerate(zip(ranges, got)):
        if a + n > total:
            assert rc == ERR["SRC_TOO_SMALL"], (i, rc)
        elif n > 2 * bs:
            assert rc == ERR["DST_TOO_SMALL"], (i, rc)
        else:
            assert rc == n and dst[d: d + n].tobytes() == data[a: a + n], (i, rc)
            keep[d: d + n] = True
    assert np.array_equal(dst[~keep], _pattern(len(dst))[~keep])


def _expect_failed_open(gpu, comp, bs, max_blocks, what, status=None):
    arc = _to_dev(comp)
    index = _open(gpu, arc, len(comp), bs, max_blocks)
    ranges = [(0, 1, 0), (5, 100, 16), (0, 0, 200), (0, 4096, 256)]
    got, dst = _fetch(gpu, arc, len(comp), index, ranges, 4096, 8192, bs)
    st = _index_status(index)
    assert st < 0 and (status is None or st == status), (what, st)
    assert got == [st, st, 0, st], (what, got)
    assert np.array_equal(dst, _pattern(len(dst))), what   # nothing is written


def test_a_failed_open_answers_every_range(gpu):
    d = os.path.join(GOLDEN, "conformance", "invalid")
    seen = 0
    for f in sorted(os.listdir(d)):
        comp = open(os.path.join(d, f), "rb").read()
        if not f.endswith(".zxc") or len(comp) < 44:
            continue
        try:
            gpu.Seekable(comp).close()
            continue   # (an archive whose table opens: its blocks are what is invalid)
        except gpu.ZxcError:
            pass
        lg = comp[5]
        _expect_failed_open(gpu, comp, 1 << lg if 12 <= lg <= 21 else 65536, 64, f)
        seen += 1
    assert seen >= 1
    bs = 4096
    data = _data(bs, 5)
    comp = gpu.compress(data, 3, bs, True, False)
    nb = -(-len(data) // bs)
    _expect_failed_open(gpu, comp[:-16] + comp[-12:], bs, nb, "truncated table", ERR["CORRUPT_DATA"])
    _expect_failed_open(gpu, comp, 8192, nb, "wrong block_size", ERR["BAD_BLOCK_SIZE"])
    _expect_failed_open(gpu, comp, bs, nb - 1, "max_blocks one too small", ERR["MEMORY"])
    _expect_failed_open(gpu, gpu.compress(data, 3, bs, False, False), bs, nb, "not seekable", ERR["CORRUPT_DATA"])


def test_dictionary_archives_need_a_dictionary(gpu):
    for rel in DICT_ARCHIVES:
        comp = open(os.path.join(GOLDEN, rel), "rb").read()
        try:
            host = gpu.Seekable(comp)
        except gpu.ZxcError:
            continue   # (no seek table: nothing to open on either side)
        total, nb = host.decompressed_size, host.num_blocks
        want, _ = host.decompress_range(0, 1, raise_on_error=False)
        host.close()
        assert want == ERR["DICT_REQUIRED"], rel
        arc = _to_dev(comp)
        index = _open(gpu, arc, len(comp), 1 << comp[5], nb)
        got, dst = _fetch(gpu, arc, len(comp), index, [(0, 1, 0), (0, min(total, 100), 16), (0, 0, 0)], 100, 4096, 1 << comp[5])
        assert _index_status(index) == 0 and got == [ERR["DICT_REQUIRED"], ERR["DICT_REQUIRED"], 0], (rel, got)
        assert np.array_equal(dst, _pattern(len(dst))), rel


def test_a_damaged_block(gpu):
    """one block's n_seq field overwritten with far too many sequences for its payload (the input of the host's range test): the
    decoder refuses it by status. Ranges that do not touch the block succeed, ranges that touch it return the host call's code."""
    from zxc_amd import corpus
    bs = 65536
    data = corpus.synth_text(60 * bs + 4321, seed=25)
    comp = gpu.compress(data, 3, bs, True, False)
    s = gpu.Seekable(comp)
    jobs = s.plan()
    s.close()
    bad = bytearray(comp)
    o = int(jobs["comp_off"][40]) + 8
    bad[o:o + 4] = (0x00FFFFFF).to_bytes(4, "little")
    bad = bytes(bad)
    host = gpu.Seekable(bad)
    want_rc, _ = host.decompress_range(0, len(data), raise_on_error=False)
    assert want_rc < 0
    rng = random.Random(40)
    want = [(0, 40 * bs), (41 * bs, 5 * bs), (40 * bs, 1), (41 * bs - 1, 1), (39 * bs + 5, 2 * bs), (40 * bs - 1, 1), (38 * bs, 4 * bs)]
    for _ in range(100):
        a = rng.randrange(30 * bs, 50 * bs)
        want.append((a, rng.randrange(1, 4 * bs)))
    ranges, at = [], 0
    for i, (a, n) in enumerate(want):
        d = at + (a & 15 if i % 2 else 5)
        ranges.append((a, n, d))
        at = (d + n + 47) // 16 * 16
    arc = _to_dev(bad)
    index = _open(gpu, arc, len(bad), bs, len(jobs))
    got, dst = _fetch(gpu, arc, len(bad), index, ranges, 40 * bs, at, bs)
    touched = 0
    for (a, n, d), rc in zip(ranges, got):
        exp, _ = host.decompress_range(a, n, raise_on_error=False)
        assert rc == exp, (a, n, rc, exp)
        if a // bs <= 40 <= (a + n - 1) // bs:
            assert rc == want_rc, (a, n, rc)
            touched += 1
        else:
            assert rc == n and dst[d: d + n].tobytes() == data[a: a + n], (a, n)
    host.close()
    assert touched >= 5 and np.array_equal(dst[at:], _pattern(len(dst))[at:])


def _big_archive(gpu, mib, bs):
    """-> (archive tensor, its size, the source tensor): synthetic text compressed on the device"""
    import torch
    from zxc_amd import corpus
    piece = corpus.synth_text(4 << 20, seed=77)
    data = piece * (mib // 4)
    src = _to_dev(data, 0)
    bound = int(gpu.lib().zxc_compress_bound(len(data)))
    ws = gpu.compress_device_work_size(len(data), 3, bs, True, False)
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    arc = torch.full((bound + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
    gpu.compress_device(src.data_ptr(), len(data), arc.data_ptr(), bound, work.data_ptr(), ws, res.data_ptr(), 3, bs, True, False)
    n_arc = int(res.item())
    assert n_arc > 0
    return arc, n_arc, src


def _seeded_ranges(total, bs, n, seed, max_len):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, total - max_len, n)
    ln = rng.integers(1, max_len + 1, n)
    odd = rng.integers(0, 2, n) * rng.integers(1, 16, n)
    d = np.zeros(n, dtype=np.int64)
    at = 0
    for i in range(n):
        d[i] = at + ((a[i] + odd[i]) & 15)
        at = (d[i] + ln[i] + 31) // 16 * 16
    return a, ln, d, int(at)


def _check_on_device(src, dst, a, ln, d, results, step=1):
    import torch
    assert np.array_equal(results, ln)
    for i in range(0, len(a), step):
        assert torch.equal(dst[int(d[i]): int(d[i] + ln[i])], src[int(a[i]): int(a[i] + ln[i])]), i


def test_twenty_thousand_ranges_in_one_call(gpu):
    import torch
    bs, n = 65536, 20000
    arc, n_arc, src = _big_archive(gpu, 64, bs)
    total = src.numel()
    index = _open(gpu, arc, n_arc, bs, total // bs)
    a, ln, d, cap = _seeded_ranges(total, bs, n, 5, 2 * bs)
    table = np.zeros(n, dtype=[("offset", "<u8"), ("len", "<u8"), ("dst_off", "<u8")])
    table["offset"], table["len"], table["dst_off"] = a, ln, d
    ws = gpu.decompress_ranges_device_work_size(n, 2 * bs, bs)
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(cap + CANARY, dtype=torch.uint8, device="cuda")
    res = torch.full((n,), UNSET, dtype=torch.int64, device="cuda")
    rt = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
    gpu.decompress_ranges_device(arc.data_ptr(), n_arc, index.data_ptr(), rt.data_ptr(), n, 2 * bs, dst.data_ptr(), cap, bs, work.data_ptr(),
                                 ws, res.data_ptr())
    torch.cuda.synchronize()
    assert _index_status(index) == 0
    _check_on_device(src, dst, a, ln, d, res.cpu().numpy())
    assert int(dst[cap:].sum().item()) == 0


def test_two_streams_share_one_index_and_the_call_is_ordered_behind_its_range_table(gpu):
    import torch
    bs, n = 65536, 3000
    arc, n_arc, src = _big_archive(gpu, 16, bs)
    total = src.numel()
    index = _open(gpu, arc, n_arc, bs, total // bs)
    torch.cuda.synchronize()
    runs = []
    for k, s in enumerate((torch.cuda.Stream(), torch.cuda.Stream())):
        a, ln, d, cap = _seeded_ranges(total, bs, n, 100 + k, 3 * bs)
        table = np.zeros(n, dtype=[("offset", "<u8"), ("len", "<u8"), ("dst_off", "<u8")])
        table["offset"], table["len"], table["dst_off"] = a, ln, d
        good = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
        rt = torch.zeros_like(good)   # every range empty until the copy below has run
        runs.append((s, a, ln, d, cap, good, rt))
    torch.cuda.synchronize()
    out = []
    for s, a, ln, d, cap, good, rt in runs:
        with torch.cuda.stream(s):
            rt.copy_(good, non_blocking=True)   # the kernel that writes d_ranges, on the call's stream, no synchronisation behind it
            out.append(_fetch(gpu, arc, n_arc, index, [None] * n, 3 * bs, cap, bs, stream=s, sync=False, d_ranges=rt))
    for (s, a, ln, d, cap, good, rt), (res, dst, work, _) in zip(runs, out):
        s.synchronize()
        _check_on_device(src, dst, a, ln, d, res.cpu().numpy()[:n], step=7)
        assert np.array_equal(dst[cap:].cpu().numpy(), _pattern(cap + CANARY)[cap:])


def test_open_more_tiles_than_scan_threads(gpu):
    """257 x 1024 + 5 blocks opened with room for three tiles more: more tiles than open's scan pass has threads, so each of its
    threads sums several words of the index, and tiles behind the table run too. Each block starts with its own index, so a range
    at a block's first byte shows whether comp_offsets[] of that block is right."""
    import torch
    bs, nb = 4096, 257 * 1024 + 5
    n = nb * bs - 3
    words = np.zeros(nb * (bs // 4), dtype="<u4")
    words[:: bs // 4] = np.arange(nb, dtype="<u4")
    data = words.view(np.uint8)[:n]
    comp = gpu.compress(data.tobytes(), 1, bs, True, True)
    arc = _to_dev(comp)
    index = _open(gpu, arc, len(comp), bs, nb + 3 * 1024)
    blocks = [0, 1, 1023, 1024, 1025, 256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1, 257 * 1024 - 1, 257 * 1024, nb - 1]
    ranges, at = [], 0
    for b in blocks:
        for odd in (0, 5, 11):   # destinations of every alignment class the copy-out has
            ranges.append((b * bs, 8, at + odd))
            at += 32
    ranges.append((1024 * bs - 4, 8, at + 3))   # straddles blocks 1023 / 1024
    cap = at + 32
    got, dst = _fetch(gpu, arc, len(comp), index, ranges, 8, cap, bs)
    assert _index_status(index) == 0
    keep = np.zeros(len(dst), dtype=bool)
    for (a, ln, d), rc in zip(ranges, got):
        assert rc == ln, (a, rc)
        assert np.array_equal(dst[d: d + ln], data[a: a + ln]), a
        if a % bs == 0:
            assert int(dst[d: d + 4].view("<u4")[0]) == a // bs, a
        keep[d: d + ln] = True
    assert np.array_equal(dst[~keep], _pattern(len(dst))[~keep])   # the gaps and the canary behind the destination
    del arc, index, words, data
    torch.cuda.empty_cache()
