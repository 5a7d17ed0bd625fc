"""The take session on the GPU (zxc_mi355x_decompress_begin_device / _take_device / _end_device, and the _dict begin): one archive
decoded into a destination that is handed over in pieces. The reference value is the result word and the output of
zxc_mi355x_decompress_device / _dict_device for the same archive, capacity and options (existing code, not the code under test);
for one round trip the unmodified reference decoder. Every piece is a tensor of its own with a pattern in front and a canary
behind, both checked after every session; a run with every piece 16-byte aligned and every cut a multiple of 16 takes the direct
path, a run with the pieces at odd addresses sends everything through slots. Payloads are text-like, and incompressible (stored
blocks). Nothing here provokes a fault: every refused input is refused by status."""
import pytest

import devtest
from dev_take import BS, TakeSession as Session, archive as _archive, blocks_at as _blocks_at, oneshot as _oneshot
from devtest import ERR, PAD, UNSET, DevDict, payload as _payload, to_dev as _to_dev

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 4095, 4096, 4097, 3 * 4096 + 5)

gpu = devtest.gpu_fixture("decompress_begin_device")

def _check(gpu, arc, cap, lens, bs=BS, checksum=False, aligned=True, max_piece=None, dd=None, what=""):
    assert sum(lens) == cap
    want_rc, want = _oneshot(gpu, arc, cap, bs, checksum, dd)
    s = Session(gpu, arc, cap, bs, max_piece, checksum, aligned, dd)
    for k, n in enumerate(lens):
        s.take(n, k)
    s.end()
    rc, got = s.result()
    print(what, cap, lens[:8], "aligned" if aligned else "odd", "session", rc, "decompress_device", want_rc)
    assert rc == want_rc, (what, rc, want_rc)
    if rc >= 0:
        assert got[:rc] == want, what
    return rc, got, s


def _cut_patterns(n, bs=BS):
    """name -> the lengths of the takes (the cut patterns of the append test)"""
    pats = {"one": [n]}
    if n >= 2:
        pats["byte first and last"] = [1, n - 2, 1]
    full = [bs] * (n // bs) + ([n % bs] if n % bs else [])
    pats["at block boundaries"] = full
    if n > bs:
        pats["one byte before a boundary and one behind"] = [bs - 1, 2, n - bs - 1]
    small = [111] * min(37, n // 111)
    pats["37 takes of 111"] = small + [n - sum(small)]
    a = n // 3
    pats["zero-length takes between"] = [0, a, 0, 0, n - a, 0]
    return pats


def _on_16(lens):
    """the same cuts moved down to multiples of 16 (the last piece takes the rest)"""
    total, at, out = sum(lens), 0, []
    for n in lens[:-1]:
        end = (at + n) // 16 * 16
        out.append(end - at)
        at = end
    return out + [total - at]


@pytest.mark.parametrize("n", SIZES)
def test_every_cut_gives_the_bytes_of_decompress_device(gpu, n):
    for seed in (2, 3):  # text, stored
        data = _payload(n, seed)
        arc = _archive(gpu, data)
        for name, lens in _cut_patterns(n).items():
            for verify in (True, False):
                rc, got, _ = _check(gpu, arc, n, _on_16(lens), checksum=verify, aligned=True, what=name)
                assert rc == n and got == data
                rc, got, _ = _check(gpu, arc, n, lens, checksum=verify, aligned=False, what=name)
                assert rc == n and got == data


def test_cuts_16_bytes_around_a_block_boundary(gpu):
    """with a cut at 2 bs + 32 the second block's slot + 32 just fits the first piece, at 2 bs + 16 it just does not; a piece that
    starts 16 bytes before a boundary has its first whole block aligned"""
    n = 4 * BS + 100
    data = _payload(n, 4)
    arc = _archive(gpu, data)
    for cut in (2 * BS - 16, 2 * BS, 2 * BS + 16, 2 * BS + 32, 2 * BS + 48):
        for aligned in (True, False):
            rc, got, _ = _check(gpu, arc, n, [cut, n - cut], checksum=True, aligned=aligned, what="cut %d" % cut)
            assert rc == n and got == data


def test_the_chunk_loop(gpu):
    n = 70 * BS
    for seed in (10, 11):
        data = _payload(n, seed)
        arc = _archive(gpu, data)
        for aligned in (True, False):
            for lens in ([n], [5, n - 5]):
                rc, got, _ = _check(gpu, arc, n, lens, checksum=True, aligned=aligned, max_piece=8 * BS, what="chunks of 8 blocks")
                assert rc == n and got == data


def test_more_than_one_tile(gpu):
    n = 1025 * BS + 7
    data = _payload(n, 12)
    arc = _archive(gpu, data)
    rc, got, _ = _check(gpu, arc, n, [3 * BS + 16, n - 3 * BS - 16], checksum=True, aligned=True, max_piece=300 * BS, what="1025 blocks")
    assert rc == n and got == data


def test_many_takes_inside_one_block(gpu):
    n = 37 * 111
    data = _payload(n, 14)
    arc = _archive(gpu, data)
    for aligned in (True, False):
        rc, got, _ = _check(gpu, arc, n, [111] * 37, checksum=True, aligned=aligned, what="37 x 111")
        assert rc == n and got == data


@pytest.mark.parametrize("level", range(1, 8))
def test_every_level(gpu, level):
    n = 5 * BS + 77
    data = _payload(n, 4)
    arc = _archive(gpu, data, level)
    for aligned in (True, False):
        rc, got, _ = _check(gpu, arc, n, [BS - 16, 2 * BS + 32, 16, n - 3 * BS - 32], checksum=True, aligned=aligned, what="level %d" % level)
        assert rc == n and got == data


@pytest.mark.parametrize("bs", [65536, 512 * 1024])
def test_larger_blocks_with_cuts_inside_blocks(gpu, bs):
    n = 2 * bs + bs // 3 + 5
    data = _payload(n, 8)
    arc = _archive(gpu, data, bs=bs)
    for aligned in (True, False):
        rc, got, _ = _check(gpu, arc, n, [bs // 2 + 16, bs + 48, n - bs // 2 - bs - 64], bs=bs, checksum=True, aligned=aligned,
                            what="block size %d" % bs)
        assert rc == n and got == data


@pytest.mark.parametrize("seekable,checksum", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_seekable_and_checksum(gpu, seekable, checksum):
    n = 6 * BS + 1234
    for seed in (6, 7):
        data = _payload(n, seed)
        arc = _archive(gpu, data, seekable=bool(seekable), checksum=bool(checksum))
        for verify in (True, False):
            for aligned in (True, False):
                rc, got, _ = _check(gpu, arc, n, [112, 3 * BS, n - 3 * BS - 112], checksum=verify, aligned=aligned,
                                    what="seekable %d checksum %d" % (seekable, checksum))
                assert rc == n and got == data


def test_capacities(gpu):
    n = 3 * BS + 5
    data = _payload(n, 16)
    arc = _archive(gpu, data)
    for aligned in (True, False):
        rc, got, _ = _check(gpu, arc, n, [BS + 16, n - BS - 16], checksum=True, aligned=aligned, what="capacity = size")
        assert rc == n and got == data
        rc, _, _ = _check(gpu, arc, n - 1, [BS + 16, n - 1 - BS - 16], checksum=True, aligned=aligned, what="capacity = size - 1")
        assert rc == ERR["DST_TOO_SMALL"]
        cap = n + 4096 + 3
        rc, got, _ = _check(gpu, arc, cap, [BS + 16, cap - BS - 16], checksum=True, aligned=aligned, what="capacity = size + 4099")
        assert rc == n and got[:n] == data
        rc, _, _ = _check(gpu, arc, 0, [], checksum=True, aligned=aligned, what="the probe of a non-empty archive")
        assert rc == ERR["DST_TOO_SMALL"]
    rc, _, _ = _check(gpu, _archive(gpu, b""), 0, [0], what="the probe of the empty archive")
    assert rc == 0


def test_damaged_archives_give_the_result_of_decompress_device(gpu):
    n = 6 * BS + 77
    lens = [BS + 16, 2 * BS + 5, n - 3 * BS - 21]
    for seed in (18, 19):
        data = _payload(n, seed)
        arc = _archive(gpu, data)
        blocks = _blocks_at(arc)
        at, size = blocks[3]
        flipped = bytearray(arc)
        flipped[at + 8 + (size - 12) // 2] ^= 0x40
        bad_hdr = bytearray(arc)
        bad_hdr[blocks[2][0] + 7] ^= 0xFF
        cases = {"payload byte flipped": bytes(flipped), "truncated inside a block": arc[: blocks[4][0] + blocks[4][1] // 2],
                 "bad block header check byte": bytes(bad_hdr)}
        for name, bad in cases.items():
            for verify in (True, False):
                for aligned in (True, False):
                    rc, _, _ = _check(gpu, bad, n, lens, checksum=verify, aligned=aligned, what=name)
                    if name != "payload byte flipped" or verify:
                        assert rc < 0, (name, verify, rc)
        for aligned in (True, False):  # the archive says 4 KiB blocks, the caller 64 KiB
            rc, _, s = _check(gpu, arc, n, lens, bs=65536, checksum=True, aligned=aligned, what="header block size")
            assert rc == ERR["BAD_BLOCK_SIZE"] and s.untouched()


def test_dictionary(gpu):
    import torch
    from zxc_amd import corpus
    n = 9 * BS + 50
    data = _payload(n, 20)
    dd, other = DevDict(gpu, corpus.synth_text(30000, seed=8)), DevDict(gpu, corpus.synth_text(20000, seed=9))
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
    lens = [BS - 16, 4 * BS + 48, n - 5 * BS - 32]
    for aligned in (True, False):
        rc, got, _ = _check(gpu, arc, n, lens, checksum=True, aligned=aligned, dd=dd, what="with its dictionary")
        assert rc == n and got == data
        rc, _, s = _check(gpu, arc, n, lens, checksum=True, aligned=aligned, what="without a dictionary")
        assert rc == ERR["DICT_REQUIRED"] and s.untouched()
        rc, _, s = _check(gpu, arc, n, lens, checksum=True, aligned=aligned, dd=other, what="with another dictionary")
        assert rc == ERR["DICT_MISMATCH"] and s.untouched()
        plain = _archive(gpu, data)
        rc, got, _ = _check(gpu, plain, n, lens, checksum=True, aligned=aligned, dd=dd, what="a dictionary for an archive without one")
        assert rc == n and got == data
    # a NULL dictionary through the _dict begin behaves as the sibling
    s = Session(gpu, plain, n, checksum=True, with_dict_begin=True)
    s.take(n)
    s.end()
    assert s.result() == (n, data)


def test_a_take_past_the_capacity_and_an_early_end_are_refused_and_the_session_goes_on(gpu):
    n = 2 * BS + 10
    data = _payload(n, 22)
    arc = _archive(gpu, data)
    s = Session(gpu, arc, n, checksum=True, aligned=False)
    s.take(BS - 1)
    with pytest.raises(gpu.ZxcError) as e:
        s.take(n - BS + 2, 1)
    assert e.value.code == ERR["OVERFLOW"]
    with pytest.raises(gpu.ZxcError) as e:
        s.end()
    assert e.value.code == ERR["DST_TOO_SMALL"]
    s.take(n - BS + 1, 1)
    s.end()
    assert s.result() == (n, data)
    with pytest.raises(gpu.ZxcError):  # spent
        s.take(0)


def test_two_sessions_interleaved_on_two_streams(gpu):
    import torch
    n = 9 * BS + 5
    datas = [_payload(n, 24), _payload(n, 25)]
    arcs = [_archive(gpu, d) for d in datas]
    lens = [[BS + 3, 4 * BS, n - 5 * BS - 3], [7, 2 * BS, n - 2 * BS - 7]]
    torch.cuda.synchronize()
    sess = [Session(gpu, a, n, max_piece=4 * BS, checksum=True, aligned=bool(i), stream=torch.cuda.Stream()) for i, a in enumerate(arcs)]
    for k in range(3):
        for s, ln in zip(sess, lens):
            s.take(ln[k], k)
    for s in sess:
        s.end()
    for s, d in zip(sess, datas):
        assert s.result() == (n, d)


def test_every_take_into_one_reused_buffer(gpu):
    """every take goes into one buffer, drained by a device copy on the session's stream in front of the next take, with no
    synchronisation in between: a take has written its bytes, in stream order, when the copy reads them"""
    import torch
    n = 6 * BS + 50
    data = _payload(n, 26)
    arc = _archive(gpu, data)
    lens = [BS + 9, 3 * BS, n - 4 * BS - 9]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    s = Session(gpu, arc, n, max_piece=3 * BS, checksum=True, stream=side)
    with torch.cuda.stream(side):
        buf = torch.empty(3 * BS + 1, dtype=torch.uint8, device="cuda")
        held = [torch.zeros(m, dtype=torch.uint8, device="cuda") for m in lens]
        for h in held:
            s.s.take(buf.data_ptr() + 1, len(h), side.cuda_stream)
            h.copy_(buf[1: 1 + len(h)], non_blocking=True)
    s.end()
    assert s.result()[0] == n
    assert b"".join(bytes(h.cpu().numpy()) for h in held) == data


def test_round_trip_with_the_append_session(gpu, ref):
    import ctypes as C
    import torch
    n = 11 * BS + 17
    L = gpu.lib()
    L.zxc_compress_bound.restype = C.c_uint64
    L.zxc_compress_bound.argtypes = [C.c_size_t]
    for seed, checksum in ((28, 1), (29, 0)):
        data = _payload(n, seed)
        lens = [3, 5 * BS, BS - 3, n - 6 * BS]
        cap = int(L.zxc_compress_bound(n))
        st = torch.cuda.current_stream().cuda_stream
        ws = gpu.compress_append_device_work_size(n, 5 * BS, 3, BS, True, bool(checksum))
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
        res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        a = gpu.compress_begin_device(dst.data_ptr(), cap, n, 5 * BS, work.data_ptr(), ws, 3, BS, True, bool(checksum), st)
        at, keep = 0, []
        for m in lens:
            keep.append(_to_dev(data[at: at + m], PAD))
            a.append(keep[-1].data_ptr(), m, st)
            at += m
        a.end(res.data_ptr(), st)
        torch.cuda.synchronize()
        size = int(res.item())
        assert size > 0
        arc = bytes(dst[:size].cpu().numpy())
        back_n, back = ref.decompress(arc, n, checksum=bool(checksum))
        assert back_n == n and back == data
        for aligned in (True, False):
            s = Session(gpu, arc, n, max_piece=5 * BS, checksum=bool(checksum), aligned=aligned)
            for k, m in enumerate(lens):
                s.take(m, k)
            s.end()
            rc, got = s.result()
            assert rc == n and got == data
            at = 0
            for (t, off, m) in s.pieces:  # piece for piece
                assert bytes(t[off: off + m].cpu().numpy()) == data[at: at + m]
                at += m
