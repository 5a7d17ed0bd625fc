"""The byte-shuffle calls of include/zxc_mi355x_shuffle.h on the GPU, at block size 4096 (the smallest at which every path exists):
the two kernels against the numpy transform at every size where a path begins or ends and at source and destination offsets sampled
over 0 .. 15 inside pattern-filled allocations; compress_shuffle_device byte for byte against compress_device (compress_dict_device)
of the numpy-shuffled source, across chunkings; decompress_shuffle_device back to the original bytes, its size check and its error
words against decompress_device's; two streams at once; and a block-aligned ranges fetch un-shuffled on its own."""
import os

import numpy as np
import pytest

import dev_append
import dev_take
import devtest
import shuffle_support as ss
from conftest import GOLDEN
from devtest import ERR, UNSET, bound
from shuffle_support import BS

pytestmark = pytest.mark.gpu
gpu = devtest.gpu_fixture(needs="compress_shuffle_device")

MAX_PIECES = (4096, 8192, 0)   # a chunk per block, two blocks (a cut on the last whole block and in front of the ragged tail), one chunk


def _x(n, E):
    return ss.tensor_bytes(n, E, seed=1000 * E + n)


def _np(b):
    return np.frombuffer(b, dtype=np.uint8)


# ---------------------------------------------------------------- the kernels
@pytest.mark.parametrize("E", [2, 4, 8])
def test_kernels_equal_numpy_at_sampled_alignments(gpu, E):
    import torch
    seen_src, seen_dst, c = set(), set(), 0
    for n in ss.sizes(E):
        x = _x(n, E)
        want = ss.np_shuffle(_np(x), E, BS).tobytes()
        for i in range(5):
            so, do = (c % 16, (7 * c + 3) % 16) if i else (0, 0)   # both aligned, then a walk through every offset of each
            c += i > 0
            seen_src.add(so)
            seen_dst.add(do)
            src, dst, back = ss.Guarded(n, so, x), ss.Guarded(n, do), ss.Guarded(n, (so + 9) % 16)
            gpu.shuffle_device(src.ptr, dst.ptr, n, E, BS, torch.cuda.current_stream().cuda_stream)
            gpu.unshuffle_device(dst.ptr, back.ptr, n, E, BS, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert dst.read() == want, (n, so, do)          # (read: the pattern around the buffer is intact)
            assert back.read() == x and src.read() == x, (n, so, do)
    assert seen_src == seen_dst == set(range(16))


def test_kernels_with_a_larger_unit(gpu):
    """unit 64 KiB: the plane stride is another, the plan is the same"""
    import torch
    for E in (2, 4, 8):
        n = 2 * 65536 + 17 * E + 3
        x = _x(n, E)
        src, dst, back = ss.Guarded(n, 5, x), ss.Guarded(n, 11), ss.Guarded(n, 0)
        gpu.shuffle_device(src.ptr, dst.ptr, n, E, 65536)
        gpu.unshuffle_device(dst.ptr, back.ptr, n, E, 65536)
        torch.cuda.synchronize()
        assert dst.read() == ss.np_shuffle(_np(x), E, 65536).tobytes() and back.read() == x, E


# ---------------------------------------------------------------- compress and decompress
def _round_trips(gpu, x, E, level, seekable, checksum, dd=None, max_pieces=MAX_PIECES, k=0):
    """compress_shuffle_device == the one-shot call on numpy's shuffle, for every chunking; the archive decodes back to x"""
    shuffled = ss.np_shuffle(_np(x), E, BS).tobytes()
    cap = bound(gpu, len(x))
    if dd is None:
        want = dev_append.plain_baseline(gpu, shuffled, cap, level, BS, seekable, checksum)
    else:
        want = dev_append.dict_baseline(gpu, shuffled, dd, cap, level, BS, seekable, checksum)
    assert want[0] > 0
    for j, mp in enumerate(max_pieces):
        what = (len(x), E, level, mp)
        got = ss.compress_shuffle(gpu, x, E, cap, mp, level=level, seekable=seekable, checksum=checksum, dd=dd, src_off=(k + 3 * j) % 16,
                                  dst_off=(k + 5 * j + 1) % 16)
        assert got[0] == want[0] and got[1] == want[1], what
        rc, out = ss.Decompress(gpu, want[1], len(x), E, mp, checksum=checksum, dd=dd, dst_off=(k + 7 * j) % 16).result()
        assert rc == len(x) and out == x, what
    return want[1]


@pytest.mark.parametrize("level", [3, 6])
@pytest.mark.parametrize("E", [2, 4, 8])
def test_archive_is_the_one_shot_calls_and_decodes_back(gpu, E, level):
    for k, n in enumerate(ss.sizes(E)):
        _round_trips(gpu, _x(n, E), E, level, True, False, k=k)


@pytest.mark.parametrize("case", ["level 7", "checksums", "non-seekable", "dictionary"])
def test_archive_with_other_options(gpu, case):
    level, seekable, checksum = (7 if case == "level 7" else 3), case != "non-seekable", case == "checksums"
    dd = dev_append.dict_of(gpu, 3000) if case == "dictionary" else None
    for k, (n, E) in enumerate(((9 * 4096 + 1000, 2), (2 * 4096 + 13, 4), (4096, 8), (0, 4))):
        _round_trips(gpu, _x(n, E), E, level, seekable, checksum, dd, k=k)


def test_capacity_one_byte_too_small(gpu):
    for E, n in ((2, 9 * 4096 + 1000), (8, 4097)):
        x = _x(n, E)
        shuffled = ss.np_shuffle(_np(x), E, BS).tobytes()
        size, _ = dev_append.plain_baseline(gpu, shuffled, bound(gpu, n), 3, BS, True, False)
        want = dev_append.plain_baseline(gpu, shuffled, size - 1, 3, BS, True, False)
        assert want[0] == ERR["DST_TOO_SMALL"]
        for mp in MAX_PIECES:
            assert ss.compress_shuffle(gpu, x, E, size - 1, mp, seekable=True, dst_off=3)[0] == want[0], (E, mp)   # (the guards hold: read())
            assert ss.compress_shuffle(gpu, x, E, size, mp, seekable=True, dst_off=3)[0] == size, (E, mp)


def test_decoded_size_must_be_the_one_given(gpu):
    for E, n in ((2, 9 * 4096 + 1000), (4, 4096), (8, 1)):
        x = _x(n, E)
        arc = dev_take.archive(gpu, ss.np_shuffle(_np(x), E, BS).tobytes(), 3, BS, True, True)
        for mp in MAX_PIECES:
            assert ss.Decompress(gpu, arc, n + 1, E, mp, checksum=True).result()[0] == ERR["CORRUPT_DATA"], (E, mp)
            want = dev_take.oneshot(gpu, arc, n - 1, BS, True)[0]
            assert want < 0 or n == 1
            rc = ss.Decompress(gpu, arc, n - 1, E, mp, checksum=True, dst_off=5).result()[0]
            assert rc == want, (E, mp, rc, want)
    # the empty-frame probe: dst_size 0 keeps the session's answer
    empty = dev_take.archive(gpu, b"", 3, BS, True, False)
    assert ss.Decompress(gpu, empty, 0, 4, 0).result()[0] == dev_take.oneshot(gpu, empty, 0, BS, False)[0] == 0


def _invalid():
    d = os.path.join(GOLDEN, "conformance", "invalid")
    return [f for f in sorted(os.listdir(d)) if f.endswith(".zxc") and os.path.getsize(os.path.join(d, f)) >= 28]


@pytest.mark.parametrize("name", _invalid())
def test_corrupt_golden_gets_the_siblings_word(gpu, name):
    """the archives the host path is tested with (tests/test_gpu_decompress_device.py): refused by status, as there"""
    comp = open(os.path.join(GOLDEN, "conformance", "invalid", name), "rb").read()
    lg = comp[5]
    bs = 1 << lg if 12 <= lg <= 21 else 65536
    size = min(gpu.get_decompressed_size(comp), 1 << 20)
    for checksum in (False, True):
        for n in sorted({size, size + 1, 100}):
            want = dev_take.oneshot(gpu, comp, n, bs, checksum)[0]
            if want >= 0 and want != n:
                want = ERR["CORRUPT_DATA"]
            rc = ss.Decompress(gpu, comp, n, 4, 0, bs=bs, checksum=checksum, dst_off=n % 16).result()[0]
            assert rc == want, (name, checksum, n, rc, want)


def test_two_streams_at_once(gpu):
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    n = 64 * 4096 + 1234
    xs = [_x(n, 2), _x(n + 4096, 8)]
    torch.cuda.synchronize()
    cs = [ss.Compress(gpu, x, E, bound(gpu, len(x)), 8192, level=3, seekable=True, stream=st, src_off=1 + i) for i, (x, E, st) in
          enumerate(zip(xs, (2, 8), streams))]
    arcs = [c.result() for c in cs]
    for (rc, arc), x, E in zip(arcs, xs, (2, 8)):
        want = dev_append.plain_baseline(gpu, ss.np_shuffle(_np(x), E, BS).tobytes(), bound(gpu, len(x)), 3, BS, True, False)
        assert (rc, arc) == want, E
    ds = [ss.Decompress(gpu, arc, len(x), E, 8192, stream=st, dst_off=7 * i + 2) for i, ((_, arc), x, E, st) in enumerate(zip(arcs, xs, (2, 8), streams))]
    for d, x in zip(ds, xs):
        rc, out = d.result()
        assert rc == len(x) and out == x


# ---------------------------------------------------------------- a ranges fetch, un-shuffled on its own
@pytest.mark.parametrize("E", [2, 4, 8])
def test_block_aligned_range_is_unshuffled_alone(gpu, E):
    import torch
    n = 9 * 4096 + 1000 + 3
    x = _x(n, E)
    cap = bound(gpu, n)
    rc, arc = ss.compress_shuffle(gpu, x, E, cap, 8192, seekable=True)
    assert rc > 0
    d_arc = devtest.to_dev(arc, devtest.PAD)
    isz = gpu.seekable_index_size(10)
    index = torch.full(((isz + 7) // 8,), -1, dtype=torch.int64, device="cuda")
    gpu.seekable_open_device(d_arc.data_ptr(), len(arc), BS, 10, index.data_ptr(), isz)
    # three whole blocks from the middle, and the range that reaches the ragged end; 16-byte aligned places in one destination
    ranges = [(2 * BS, 3 * BS, 0), (7 * BS, n - 7 * BS, 3 * BS + 64)]
    table = np.zeros(2, dtype=gpu.RANGE_DTYPE)
    for i, r in enumerate(ranges):
        table[i] = r
    d_ranges = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
    dcap = 3 * BS + 64 + (n - 7 * BS) + 64
    ws = gpu.decompress_ranges_device_work_size(2, 3 * BS, BS)
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(dcap, dtype=torch.uint8, device="cuda")
    res = torch.full((2,), UNSET, dtype=torch.int64, device="cuda")
    gpu.decompress_ranges_device(d_arc.data_ptr(), len(arc), index.data_ptr(), d_ranges.data_ptr(), 2, 3 * BS, dst.data_ptr(), dcap, BS,
                                 work.data_ptr(), ws, res.data_ptr())
    outs = []
    for k, (a, m, at) in enumerate(ranges):
        out = ss.Guarded(m, 3 + 4 * k)
        gpu.unshuffle_device(dst.data_ptr() + at, out.ptr, m, E, BS)
        outs.append(out)
    torch.cuda.synchronize()
    assert [int(v) for v in res.cpu().numpy()] == [3 * BS, n - 7 * BS]
    for (a, m, _), out in zip(ranges, outs):
        assert out.read() == x[a: a + m], (E, a)
