"""The append session with a dictionary in device memory on the GPU (zxc_mi355x_compress_begin_dict_device, then the sibling's
append and end): one archive from a source that arrives in pieces, every block encoded against the dictionary. The reference value
is always existing code: the archive and the result word zxc_mi355x_compress_dict_device writes for the concatenation of the pieces
with the same options, dictionary and capacity; for round trips the unmodified reference decoder and the take session. The
destination starts as a pattern and has a canary area behind dst_capacity; every piece is a tensor of its own at an odd offset
inside a buffer that ends with the piece (nothing readable is promised behind n); d_work has an odd address. Payloads are
text-like, and incompressible (stored blocks). Nothing here provokes a fault: every refused input is refused by status."""
import numpy as np
import pytest

import dev_append
import devtest
from dev_append import dict_baseline as _baseline, dict_of as _dict, dict_session as Session, text as _text
from devtest import (CANARY, ERR, UNSET, bound as _bound, pattern as _pattern, payload as _payload, piece as _piece,
                     ref_decompress as _ref_decompress, split as _split)

pytestmark = pytest.mark.gpu

BS = 4096
SIZES = (0, 1, 4095, 4096, 4097, 3 * 4096 + 5)
DICT_SIZES = (1, 100, 4096 + 3, 65535)

gpu = devtest.gpu_fixture("compress_begin_dict_device")

_BASE = dev_append.BASE[dev_append.DICT]  # (cleared behind the one very large case)


def _check(gpu, data, lens, dd, level=3, bs=BS, seekable=0, checksum=0, cap=None, max_piece=None, odd_dst=0, what=""):
    cap = _bound(gpu, len(data)) if cap is None else cap
    want_rc, want = _baseline(gpu, data, dd, cap, level, bs, seekable, checksum)
    max_piece = max(bs, max(lens, default=0)) if max_piece is None else max_piece
    s = Session(gpu, dd, cap, len(data), max_piece, level, bs, seekable, checksum, odd_dst)
    for k, part in enumerate(_split(data, lens)):
        s.append(part, k)
    s.end()
    rc, got = s.result()
    print(what, len(data), lens[:8], "dict", dd.tup[1] if dd else 0, "session", rc, "compress_dict_device", want_rc)
    assert rc == want_rc, (what, rc, want_rc)
    assert got == want, what
    if rc > 0:
        assert got[6] & 0x40 and got[7:11] == bytes(dd.d_id.cpu().numpy().view(np.uint8)), what  # the flag and the id
    return rc, got


def _cut_patterns(n, bs=BS):
    """name -> the lengths of the appends"""
    pats = {"one": [n]}
    a = n // 3
    pats["zero-length appends between"] = [0, a, 0, 0, n - a, 0]
    for behind in (1, 31):
        if n > bs + behind:
            pats["an append ends %d behind a boundary" % behind] = [bs + behind, n - bs - behind]
        if n > 2 * bs + behind:
            pats["behind a carry, an append ends %d behind a boundary" % behind] = [7, 2 * bs + behind - 7, n - 2 * bs - behind]
    if n > bs:
        pats["one byte before a boundary and one behind"] = [bs - 1, 2, n - bs - 1]
    return pats


@pytest.mark.parametrize("n", SIZES)
def test_every_cut_gives_the_archive_of_compress_dict_device(gpu, n):
    dicts = [_dict(gpu, size, with_huf) for size in DICT_SIZES for with_huf in (False, True)]
    k = 0
    for seed in (2, 3):  # text, stored
        data = _payload(n, seed)
        for dd in dicts:  # every dictionary size, with and without a table: one append, and one other pattern in turn
            _check(gpu, data, [n], dd, 3, BS, 1, 1, what="one")
        for name, lens in _cut_patterns(n).items():
            for dd in (dicts[k % 8], dicts[(k + 3) % 8]):
                _check(gpu, data, lens, dd, 3, BS, 1, 1, what=name)
            k += 1
    if 0 < n <= 4097:
        _check(gpu, _payload(n, 2), [1] * n, dicts[(n % 4) * 2 + 1], 3, BS, 1, 1, what="all single bytes")
        _check(gpu, _payload(n, 3), [1] * n, dicts[((n + 1) % 4) * 2], 3, BS, 0, 0, what="all single bytes")


@pytest.mark.parametrize("level", [1, 3, 6, 7])
def test_levels(gpu, level):
    n = 5 * BS + 77
    _check(gpu, _payload(n, 4), [BS - 3, 2 * BS + 10, 1, n - 3 * BS - 8], _dict(gpu, 4099, level == 7), level, BS, 1, 1, what="level %d" % level)


@pytest.mark.parametrize("seekable,checksum", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_seekable_and_checksum(gpu, seekable, checksum):
    n = 6 * BS + 1234
    for seed in (6, 7):
        _check(gpu, _payload(n, seed), [100, 3 * BS, n - 3 * BS - 100], _dict(gpu, 100), 3, BS, seekable, checksum,
               what="seekable %d checksum %d" % (seekable, checksum))


def test_images_of_128_kib(gpu):
    bs = 65536
    n = 2 * bs + bs // 3 + 5
    _check(gpu, _payload(n, 8), [bs // 2 + 1, bs + 7, n - bs // 2 - bs - 8], _dict(gpu, 65535), 3, bs, 1, 1, what="block size 65536, dictionary 65535")


def test_the_big_block_encoder_entry(gpu):
    bs = 512 * 1024
    n = 2 * bs + 1000
    _check(gpu, _payload(n, 10), [bs - 5, bs + 6, n - 2 * bs - 1], _dict(gpu, 4099, True), 3, bs, 1, 1, what="two blocks of 512 KiB and a tail")


def test_an_odd_destination(gpu):
    n = 4 * BS + 321
    for odd in (1, 7):
        _check(gpu, _payload(n, 18), [BS // 2, 2 * BS, n - BS // 2 - 2 * BS], _dict(gpu, 100, True), 3, BS, 1, 1, odd_dst=odd, what="d_dst + %d" % odd)


def test_a_piece_of_two_chunks(gpu):
    """4 KiB blocks under a dictionary of 65 535 bytes: a chunk is 4096 jobs, and a piece of 4097 blocks behind a carry of 5 bytes
    spans two, with the carried block in the first"""
    max_piece = 4097 * BS + 7
    n = 5 + max_piece
    base = np.frombuffer(_text()[: 4 << 20], dtype=np.uint8)
    arr = np.tile(base, n // len(base) + 1)[:n].copy()
    rng = np.random.default_rng(43)
    at = rng.integers(0, n, n // 200)
    arr[at] = rng.integers(0, 256, len(at), dtype=np.uint8)  # no two blocks alike
    data = arr.tobytes()
    dd = _dict(gpu, 65535)
    ws = gpu.compress_append_dict_device_work_size(n, max_piece, 65535, 3, BS, True, True)
    assert ws - gpu.compress_append_device_work_size(n, max_piece, 3, BS, True, True) <= 4096 * (BS + 65535) + 320  # one chunk of images for 4099 jobs
    _check(gpu, data, [5, max_piece], dd, 3, BS, 1, 1, max_piece=max_piece, what="4097 blocks in one piece")
    _BASE.clear()


def test_an_append_of_more_than_max_piece(gpu):
    mp = 2 * BS
    n = 5 * mp + 3 + 100
    _check(gpu, _payload(n, 12), [100, 5 * mp + 3], _dict(gpu, 4099), 3, BS, 1, 1, max_piece=mp, what="the internal piece loop behind a carry")
    _check(gpu, _payload(5 * mp + 3, 13), [5 * mp + 3], _dict(gpu, 1), 3, BS, 1, 1, max_piece=mp, what="the internal piece loop")


def test_the_capacity_binds_exactly(gpu):
    n = 7 * BS + 99
    lens = [BS + 1, 3 * BS, n - 4 * BS - 1]
    for seed in (14, 15):
        data, dd = _payload(n, seed), _dict(gpu, 100 if seed % 2 else 4099)
        size, _ = _check(gpu, data, lens, dd, 3, BS, 1, 1, what="bound")
        assert size > 0
        rc, _ = _check(gpu, data, lens, dd, 3, BS, 1, 1, cap=size, what="capacity = size")
        assert rc == size
        rc, _ = _check(gpu, data, lens, dd, 3, BS, 1, 1, cap=size - 1, what="capacity = size - 1")
        assert rc == ERR["DST_TOO_SMALL"]


def test_an_append_past_max_total_is_refused_and_the_session_goes_on(gpu):
    n = BS + 10
    data, dd = _payload(n, 20), _dict(gpu, 100)
    s = Session(gpu, dd, _bound(gpu, n), n, BS, 3, BS, 1, 1)
    s.append(data[:BS - 1])
    with pytest.raises(gpu.ZxcError) as e:
        s.append(data[: 12])
    assert e.value.code == ERR["OVERFLOW"]
    s.append(data[BS - 1:])
    s.end()
    assert s.result() == _baseline(gpu, data, dd, _bound(gpu, n), 3, BS, 1, 1)


def test_a_dropped_session_does_not_disturb_the_next_on_its_work_area(gpu):
    import torch
    n = 3 * BS + 700
    data, other = _payload(n, 22), _payload(n, 24)
    dd = _dict(gpu, 4099)
    cap = _bound(gpu, n)
    want = _baseline(gpu, data, dd, cap, 3, BS, 1, 1)
    dropped = Session(gpu, _dict(gpu, 4099, True), cap, n, 2 * BS, 3, BS, 1, 1)  # (another dictionary of the same size: the same work size)
    dropped.append(other[: BS + 500])
    dropped.append(other[BS + 500: 2 * BS + 600], 1)  # blocks gathered, bytes waiting in a carry area: and no end
    s = Session(gpu, dd, cap, n, 2 * BS, 3, BS, 1, 1, work=dropped.work)
    for k, part in enumerate(_split(data, [BS - 1, BS + 2, n - 2 * BS - 1])):
        s.append(part, k)
    s.end()
    assert s.result() == want
    torch.cuda.synchronize()
    assert int(dropped.res.item()) == UNSET  # nothing was written for the session without an end


def _take(gpu, arc, n, bs, dd, lens, checksum):
    """a take session over the archive -> (result word, the pieces concatenated)"""
    import torch
    d_arc = torch.frombuffer(bytearray(arc + bytes(64)), dtype=torch.uint8).to("cuda")
    mp = max(bs, max(lens, default=0))
    ws = gpu.decompress_take_device_work_size(len(arc), n, mp, bs)
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    t = gpu.decompress_begin_dict_device(d_arc.data_ptr(), len(arc), n, mp, bs, dd.tup if dd else None, work.data_ptr(), ws, bool(checksum), sp)
    outs = [torch.from_numpy(_pattern(m + 64)).to("cuda") for m in lens]
    for o, m in zip(outs, lens):
        t.take(o.data_ptr(), m, sp)
    t.end(res.data_ptr(), sp)
    torch.cuda.synchronize()
    for o, m in zip(outs, lens):
        assert (o[m:].cpu().numpy() == _pattern(m + 64)[m:]).all()
    return int(res.item()), b"".join(bytes(o[:m].cpu().numpy()) for o, m in zip(outs, lens))


def test_round_trips(gpu, ref):
    n = 11 * BS + 17
    for seed, checksum, with_huf in ((28, 1, True), (29, 0, False)):
        data, dd = _payload(n, seed), _dict(gpu, 4099, with_huf)
        rc, arc = _check(gpu, data, [3, 5 * BS, BS - 3, n - 6 * BS], dd, 3, BS, 1, checksum, what="round trip")
        assert rc > 0
        size, back = _ref_decompress(ref, arc, n, dd.content, dd.huf, bool(checksum))
        assert size == n and back == data
        assert _ref_decompress(ref, arc, n)[0] == ERR["DICT_REQUIRED"]
        # read back through the take session, in pieces of other sizes than it was written in
        size, back = _take(gpu, arc, n, BS, dd, [BS + 5, 1, 7 * BS, n - 8 * BS - 6], checksum)
        assert size == n and back == data
        assert _take(gpu, arc, n, BS, None, [n], checksum)[0] == ERR["DICT_REQUIRED"]
        assert _take(gpu, arc, n, BS, _dict(gpu, 4099, with_huf, seed=1), [n], checksum)[0] == ERR["DICT_MISMATCH"]


def test_two_sessions_interleaved_on_two_streams(gpu):
    import torch
    n = 9 * BS + 5
    datas = [_payload(n, 22), _payload(n, 24)]
    dds = [_dict(gpu, 4099), _dict(gpu, 65535, True)]
    lens = [[BS + 3, 4 * BS, n - 5 * BS - 3], [7, 2 * BS, n - 2 * BS - 7]]
    cap = _bound(gpu, n)
    want = [_baseline(gpu, d, dd, cap, 3, BS, 1, 1) for d, dd in zip(datas, dds)]
    torch.cuda.synchronize()
    sess = [Session(gpu, dd, cap, n, 4 * BS, 3, BS, 1, 1, stream=torch.cuda.Stream()) for dd in dds]
    parts = [_split(d, ln) for d, ln in zip(datas, lens)]
    for k in range(3):
        for s, p in zip(sess, parts):
            s.append(p[k], k)
    for s in sess:
        s.end()
    for s, w in zip(sess, want):
        assert s.result() == w
    assert want[0] != want[1]


def test_without_a_dictionary_the_plain_sessions_bytes(gpu):
    import torch
    n = 5 * BS + 77
    data = _payload(n, 30)
    lens = [BS - 3, 2 * BS + 10, 1, n - 3 * BS - 8]
    cap = _bound(gpu, n)
    ws = gpu.compress_append_device_work_size(n, 3 * BS, 3, BS, True, True)
    work = torch.empty(ws + 1, dtype=torch.uint8, device="cuda")
    dst = torch.from_numpy(_pattern(cap + CANARY)).to("cuda")
    res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    plain = gpu.compress_begin_device(dst.data_ptr(), cap, n, 3 * BS, work.data_ptr() + 1, ws, 3, BS, True, True, sp)
    keep = [_piece(part, k) for k, part in enumerate(_split(data, lens))]
    for (_, p), part in zip(keep, _split(data, lens)):
        plain.append(p, len(part), sp)
    plain.end(res.data_ptr(), sp)
    torch.cuda.synchronize()
    size = int(res.item())
    assert size > 0
    want = (size, bytes(dst[:size].cpu().numpy()))
    assert not want[1][6] & 0x40
    dd = _dict(gpu, 100)
    for tup in (None, (dd.tup[0], 0, dd.tup[2], dd.tup[3]), (0, 0, 0, 0)):
        assert gpu.compress_append_dict_device_work_size(n, 3 * BS, 0, 3, BS, True, True) == ws
        s = Session(gpu, None, cap, n, 3 * BS, 3, BS, 1, 1, dict_=tup)
        for k, part in enumerate(_split(data, lens)):
            s.append(part, k)
        s.end()
        assert s.result() == want, tup
