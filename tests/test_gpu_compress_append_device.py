"""The append session on the GPU (zxc_mi355x_compress_begin_device / _append_device / _end_device): one archive from a source that
arrives in pieces. The reference value is the archive and the result word zxc_mi355x_compress_device writes for the concatenation
of the pieces with the same options and capacity (existing code, not the code under test); for round trips the unmodified reference
decoder and decompress_device. The destination starts as a pattern and has a canary area behind dst_capacity; every piece is a
tensor of its own at an odd offset inside a buffer that ends with the piece (nothing readable is promised behind n). Payloads are
text-like, and incompressible (stored blocks). Nothing here provokes a fault: every refused input is refused by status."""
import pytest

import devtest
from dev_append import plain_baseline as _baseline, plain_session as Session
from devtest import CANARY, ERR, UNSET, bound as _bound, pattern as _pattern, payload as _payload, split as _split

pytestmark = pytest.mark.gpu

BS = 4096
SIZES = (0, 1, 4095, 4096, 4097, 3 * 4096 + 5)

gpu = devtest.gpu_fixture("compress_begin_device")


def _check(gpu, data, lens, level=3, bs=BS, seekable=0, checksum=0, cap=None, max_piece=None, odd_dst=0, what=""):
    cap = _bound(gpu, len(data)) if cap is None else cap
    want_rc, want = _baseline(gpu, data, cap, level, bs, seekable, checksum)
    max_piece = max(bs, max(lens, default=0)) if max_piece is None else max_piece
    s = Session(gpu, cap, len(data), max_piece, level, bs, seekable, checksum, odd_dst)
    for k, part in enumerate(_split(data, lens)):
        s.append(part, k)
    s.end()
    rc, got = s.result()
    print(what, len(data), lens[:8], "session", rc, "compress_device", want_rc)
    assert rc == want_rc, (what, rc, want_rc)
    assert got == want, what
    return rc, got


def _cut_patterns(n, bs=BS):
    """name -> the lengths of the appends"""
    pats = {"one": [n]}
    if n >= 2:
        pats["byte first and last"] = [1, n - 2, 1]
    full = [bs] * (n // bs) + ([n % bs] if n % bs else [])
    pats["at block boundaries"] = full
    if n > bs:
        pats["one byte before a boundary and one behind"] = [bs - 1, 2, n - bs - 1]
    small = [111] * min(37, n // 111)
    pats["37 appends of 111"] = small + [n - sum(small)]
    a = n // 3
    pats["zero-length appends between"] = [0, a, 0, 0, n - a, 0]
    return pats


@pytest.mark.parametrize("n", SIZES)
def test_every_cut_gives_the_archive_of_compress_device(gpu, n):
    for seed in (2, 3):  # text, stored
        data = _payload(n, seed)
        for name, lens in _cut_patterns(n).items():
            _check(gpu, data, lens, 3, BS, 1, 1, what=name)


@pytest.mark.parametrize("level", range(1, 8))
def test_every_level(gpu, level):
    n = 5 * BS + 77
    _check(gpu, _payload(n, 4), [BS - 3, 2 * BS + 10, 1, n - 3 * BS - 8], level, BS, 1, 1, what="level %d" % level)


@pytest.mark.parametrize("seekable,checksum", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_seekable_and_checksum(gpu, seekable, checksum):
    n = 6 * BS + 1234
    for seed in (6, 7):
        _check(gpu, _payload(n, seed), [100, 3 * BS, n - 3 * BS - 100], 3, BS, seekable, checksum, what="seekable %d checksum %d" % (seekable, checksum))


@pytest.mark.parametrize("bs", [65536, 512 * 1024])
def test_larger_blocks_with_a_cut_inside_a_block(gpu, bs):
    n = 2 * bs + bs // 3 + 5
    _check(gpu, _payload(n, 8), [bs // 2 + 1, bs + 7, n - bs // 2 - bs - 8], 3, bs, 1, 1, what="block size %d" % bs)


def test_the_hash_wraps_over_pieces_of_33_blocks(gpu):
    """70 blocks with checksums: the rotation of the carried hash passes 32 in one piece, and pieces follow each other"""
    n = 70 * BS
    data = _payload(n, 10)
    _check(gpu, data, [33 * BS, 33 * BS, 4 * BS], 3, BS, 1, 1, max_piece=33 * BS, what="pieces of 33 blocks")
    _check(gpu, data, [n], 3, BS, 1, 1, max_piece=8 * BS, what="the internal piece loop")
    _check(gpu, data, [5, n - 5], 3, BS, 0, 1, max_piece=8 * BS, what="the internal piece loop behind a carry")


def test_more_than_one_tile_in_one_piece(gpu):
    n = 1025 * BS + 7
    _check(gpu, _payload(n, 12), [n], 3, BS, 1, 1, what="1025 blocks")


def test_the_capacity_binds_exactly(gpu):
    n = 7 * BS + 99
    lens = [BS + 1, 3 * BS, n - 4 * BS - 1]
    for seed in (14, 15):
        data = _payload(n, seed)
        size, _ = _check(gpu, data, lens, 3, BS, 1, 1, what="bound")
        assert size > 0
        rc, _ = _check(gpu, data, lens, 3, BS, 1, 1, cap=size, what="capacity = size")
        assert rc == size
        rc, _ = _check(gpu, data, lens, 3, BS, 1, 1, cap=size - 1, what="capacity = size - 1")
        assert rc == ERR["DST_TOO_SMALL"]


def test_a_capacity_the_first_piece_exceeds_stays_exceeded(gpu):
    n = 8 * BS
    data = _payload(n, 17)  # stored blocks: the first piece of three blocks is larger than the capacity of two
    cap = 2 * BS
    s = Session(gpu, cap, n, 3 * BS, 3, BS, 1, 1)
    for k, part in enumerate(_split(data, [3 * BS, 100, 2 * BS, n - 5 * BS - 100])):
        s.append(part, k)
    s.end()
    rc, _ = s.result()
    assert rc == ERR["DST_TOO_SMALL"]
    assert _baseline(gpu, data, cap, 3, BS, 1, 1)[0] == rc


def test_an_odd_destination_and_odd_sources(gpu):
    n = 4 * BS + 321
    for odd in (1, 7):
        _check(gpu, _payload(n, 18), [BS // 2, 2 * BS, n - BS // 2 - 2 * BS], 3, BS, 1, 1, odd_dst=odd, what="d_dst + %d" % odd)


def test_an_append_past_max_total_is_refused_and_the_session_goes_on(gpu):
    n = BS + 10
    data = _payload(n, 20)
    s = Session(gpu, _bound(gpu, n), n, BS, 3, BS, 1, 1)
    s.append(data[:BS - 1])
    with pytest.raises(gpu.ZxcError) as e:
        s.append(data[: 12])
    assert e.value.code == ERR["OVERFLOW"]
    s.append(data[BS - 1:])
    s.end()
    assert s.result() == _baseline(gpu, data, _bound(gpu, n), 3, BS, 1, 1)


def test_two_sessions_interleaved_on_two_streams(gpu):
    import torch
    n = 9 * BS + 5
    datas = [_payload(n, 22), _payload(n, 24)]
    lens = [[BS + 3, 4 * BS, n - 5 * BS - 3], [7, 2 * BS, n - 2 * BS - 7]]
    cap = _bound(gpu, n)
    want = [_baseline(gpu, d, cap, 3, BS, 1, 1) for d in datas]
    torch.cuda.synchronize()
    sess = [Session(gpu, cap, n, 4 * BS, 3, BS, 1, 1, stream=torch.cuda.Stream()) for _ in datas]
    parts = [_split(d, ln) for d, ln in zip(datas, lens)]
    for k in range(3):
        for s, p in zip(sess, parts):
            s.append(p[k], k)
    for s in sess:
        s.end()
    for s, w in zip(sess, want):
        assert s.result() == w


def test_an_append_behind_the_copy_that_fills_its_source(gpu):
    """the source of every append is one buffer, refilled by a device copy on the session's stream in front of the append, with no
    synchronisation in between: an append has read its bytes, in stream order, when the next copy overwrites them"""
    import torch
    n = 6 * BS + 50
    data = _payload(n, 26)
    cap = _bound(gpu, n)
    want = _baseline(gpu, data, cap, 3, BS, 1, 1)
    parts = _split(data, [BS + 9, 3 * BS, n - 4 * BS - 9])
    held = [torch.frombuffer(bytearray(p), dtype=torch.uint8).to("cuda") for p in parts]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    s = Session(gpu, cap, n, 3 * BS, 3, BS, 1, 1, stream=side)
    with torch.cuda.stream(side):
        buf = torch.empty(3 * BS + 1, dtype=torch.uint8, device="cuda")
        for h in held:
            buf[1: 1 + len(h)].copy_(h, non_blocking=True)
            s.s.append(buf.data_ptr() + 1, len(h), side.cuda_stream)
    s.end()
    assert s.result() == want


def test_round_trips(gpu, ref):
    import torch
    n = 11 * BS + 17
    for seed, checksum in ((28, 1), (29, 0)):
        data = _payload(n, seed)
        rc, arc = _check(gpu, data, [3, 5 * BS, BS - 3, n - 6 * BS], 3, BS, 1, checksum, what="round trip")
        assert rc > 0
        size, back = ref.decompress(arc, n, checksum=bool(checksum))
        assert size == n and back == data
        d_arc = torch.frombuffer(bytearray(arc + bytes(64)), dtype=torch.uint8).to("cuda")
        ws = gpu.decompress_device_work_size(rc, n, BS)
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        out = torch.from_numpy(_pattern(n + CANARY)).to("cuda")
        res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        gpu.decompress_device(d_arc.data_ptr(), rc, out.data_ptr(), n, BS, work.data_ptr(), ws, res.data_ptr(), bool(checksum),
                              torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert int(res.item()) == n
        assert bytes(out[:n].cpu().numpy()) == data
