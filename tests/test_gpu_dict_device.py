"""The device calls that take a dictionary in device memory, on the GPU: zxc_mi355x_dict_prepare_device computes the id the
reference wrote into the golden .zxd files; zxc_mi355x_compress_dict_device writes byte for byte the archive of zxc_compress with
the same dictionary and table, which the unmodified reference decodes with that dictionary and refuses without it or with another;
zxc_mi355x_decompress_dict_device and zxc_mi355x_decompress_ranges_dict_device answer what zxc_decompress and
zxc_seekable_set_dict + zxc_seekable_decompress_range answer on the host. A canary pattern lies behind every capacity. Nothing here
provokes a fault: the corrupt inputs are those the host path is tested with, and the kernels refuse them by status."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import devtest
from conftest import GOLDEN, load_dict, read
from devtest import (CANARY, ERR, PAD, UNSET, DevDict, bound as _bound, canary as _canary, canary_ok as _canary_ok, pattern as _pattern,
                     ref_decompress as _ref_decompress, to_dev as _to_dev)

pytestmark = pytest.mark.gpu

ID_LENGTHS = (1, 3, 4, 8, 16, 17, 112, 113, 225, 65535)
BIG_BLOCKS = 20001  # more than one chunk of the compress call (4096 blocks at 4 KiB under a full dictionary), and >= 16 400


gpu = devtest.gpu_fixture("dict_prepare_device")


def _lib(gpu):
    L = gpu.lib()
    L.zxc_dict_id.restype = C.c_uint32
    L.zxc_dict_id.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p]
    return L


def _golden_dict(name):
    return load_dict(os.path.join(GOLDEN, "conformance", "valid", name))


def _text_dict(n=5000, seed=77):
    from zxc_amd import corpus
    return corpus.synth_text(n, seed=seed)


# ---------------------------------------------------------------- the id
def test_id_of_the_golden_dictionaries(gpu):
    L = _lib(gpu)
    for name in ("dict_http.zxd", "dict_text.zxd"):
        raw = read("conformance/valid/" + name)
        content, huf = _golden_dict(name)
        stored = int.from_bytes(raw[8:12], "little")  # written by the reference
        got = DevDict(gpu, content, huf).id()
        assert got == stored == L.zxc_dict_id(content, len(content), huf), (name, hex(got), hex(stored))
        got = DevDict(gpu, content, None).id()
        assert got == L.zxc_dict_id(content, len(content), None) != stored, name


def test_id_over_content_lengths(gpu):
    L = _lib(gpu)
    rng = np.random.default_rng(5)
    _, huf = _golden_dict("dict_http.zxd")
    for n in ID_LENGTHS + (2, 5, 7, 15, 32, 33, 111, 114, 224, 226, 1000, 65534):
        content = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        for h in (None, huf):
            got, want = DevDict(gpu, content, h).id(), L.zxc_dict_id(content, n, h)
            assert got == want, (n, h is not None, hex(got), hex(want))


# ---------------------------------------------------------------- compress
def _dev_compress(gpu, src, n, dd, level, bs, seekable, checksum, cap=None, stream=None):
    """-> (result, dst tensor of cap + CANARY bytes, cap); the CANARY bytes behind cap start as a known pattern"""
    import torch
    cap = _bound(gpu, n) if cap is None else cap
    ws = gpu.compress_dict_device_work_size(n, dd.tup[1] if dd else 0, level, bs, seekable, checksum)
    assert ws > 0
    s = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(s):
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        dst = torch.empty(cap + CANARY, dtype=torch.uint8, device="cuda")
        dst[cap:] = _canary().to("cuda")
        res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        gpu.compress_dict_device(src.data_ptr() if n else 0, n, dst.data_ptr(), cap, dd.tup if dd else None, work.data_ptr(), ws,
                                 res.data_ptr(), level, bs, seekable, checksum, s.cuda_stream)
    s.synchronize()
    return int(res.item()), dst, cap


@pytest.mark.parametrize("bs", [4096, 65536, 1 << 19])
@pytest.mark.parametrize("level", [1, 2, 3, 4, 5, 6, 7])
def test_byte_identity_with_zxc_compress(gpu, ref, level, bs):
    from devtest import inputs as _inputs
    http, huf = _golden_dict("dict_http.zxd")
    text = _text_dict()
    dicts = {(k, h is not None): DevDict(gpu, c, h) for k, c in (("http", http), ("text", text)) for h in (None, huf)}
    # (dictionary, table, checksum, seekable): with and without the table, checksums and the seek table, two dictionaries
    combos = (("http", True, True, True), ("http", False, False, False), ("text", True, False, True), ("text", False, True, False))
    for name, data in _inputs(bs).items():
        src = _to_dev(data)
        for k, with_huf, checksum, seekable in combos:
            dd = dicts[(k, with_huf)]
            what = (name, level, bs, k, with_huf, checksum, seekable)
            want = gpu.compress(data, level, bs, seekable, checksum, dict_=dd.content, dict_huf=dd.huf)
            rc, dst, cap = _dev_compress(gpu, src, len(data), dd, level, bs, seekable, checksum)
            print(what, rc, len(want))
            assert rc == len(want), (what, rc, len(want))
            got = bytes(dst[:rc].cpu().numpy())
            assert got[:16] == want[:16], (what, got[:16].hex(), want[:16].hex())
            assert got == want, what
            assert _canary_ok(dst, cap), what
            assert got[6] & 0x40 and int.from_bytes(got[7:11], "little") == dd.id(), what
            if name in ("text", "bs+1", "1B"):  # the unmodified reference reads it with the dictionary, and only with it
                r, out = _ref_decompress(ref, got, len(data), dd.content, dd.huf, checksum)
                assert r == len(data) and out == data, (what, r)
                assert _ref_decompress(ref, got, len(data))[0] == ERR["DICT_REQUIRED"], what
                assert _ref_decompress(ref, got, len(data), dd.content[:-1] + b"?", dd.huf)[0] == ERR["DICT_MISMATCH"], what


def test_empty_input_and_no_dictionary(gpu):
    """an empty source has no block but still a dictionary header, as zxc_compress writes it; dict None is compress_device"""
    http, huf = _golden_dict("dict_http.zxd")
    dd = DevDict(gpu, http, huf)
    want = gpu.compress(b"", 3, 65536, True, True, dict_=http, dict_huf=huf)
    rc, dst, cap = _dev_compress(gpu, None, 0, dd, 3, 65536, True, True, cap=len(want))
    assert rc == len(want) and bytes(dst[:rc].cpu().numpy()) == want and _canary_ok(dst, cap)
    from zxc_amd import corpus
    data = corpus.synth_text(3 * 65536 + 5, seed=3)
    want = gpu.compress(data, 3, 65536, True, True)
    rc, dst, cap = _dev_compress(gpu, _to_dev(data), len(data), None, 3, 65536, True, True)
    assert rc == len(want) and bytes(dst[:rc].cpu().numpy()) == want and _canary_ok(dst, cap)


@pytest.mark.parametrize("checksum", [False, True])
def test_capacity_edges(gpu, checksum):
    from zxc_amd import corpus
    data = corpus.synth_text(5 * 65536 + 123, seed=9)
    dd = DevDict(gpu, _text_dict(), None)
    src = _to_dev(data)
    want = gpu.compress(data, 3, 65536, True, checksum, dict_=dd.content)
    rc, dst, cap = _dev_compress(gpu, src, len(data), dd, 3, 65536, True, checksum, cap=len(want))
    assert rc == len(want) and bytes(dst[:rc].cpu().numpy()) == want and _canary_ok(dst, cap)
    rc, dst, cap = _dev_compress(gpu, src, len(data), dd, 3, 65536, True, checksum, cap=len(want) - 1)
    assert rc == ERR["DST_TOO_SMALL"] and _canary_ok(dst, cap)


@pytest.fixture(scope="module")
def big(gpu):
    """BIG_BLOCKS blocks of 4 KiB under a 65 535-byte dictionary, written by compress_dict_device: the image area is reused five
    times. -> (data, dictionary content, DevDict, archive tensor with PAD, archive bytes)"""
    from zxc_amd import corpus
    content = corpus.synth_text(65535, seed=41)
    base = np.frombuffer(corpus.synth_text(4 << 20, seed=42), dtype=np.uint8)
    n = BIG_BLOCKS * 4096 - 5
    arr = np.tile(base, n // len(base) + 1)[:n].copy()
    rng = np.random.default_rng(43)
    at = rng.integers(0, n, n // 200)
    arr[at] = rng.integers(0, 256, len(at), dtype=np.uint8)  # no two blocks alike
    data = arr.tobytes()
    dd = DevDict(gpu, content, None)
    rc, dst, cap = _dev_compress(gpu, _to_dev(data), n, dd, 3, 4096, True, True)
    assert rc > 0 and _canary_ok(dst, cap)
    arc = dst[: rc + PAD].clone()
    comp = bytes(arc[:rc].cpu().numpy())
    del dst
    return data, content, dd, arc, comp


def test_more_blocks_than_a_chunk(gpu, big):
    data, content, dd, arc, comp = big
    want = gpu.compress(data, 3, 4096, True, True, dict_=content)
    assert len(comp) == len(want) and comp == want
    ws = gpu.compress_dict_device_work_size(len(data), 65535, 3, 4096, True, True)
    assert ws - gpu.compress_device_work_size(len(data), 3, 4096, True, True) <= 4096 * (4096 + 65535) + 4096  # one chunk of images


# ---------------------------------------------------------------- decompress
def _dev_decompress(gpu, arc, n_arc, bs, cap, dd, checksum=False, stream=None):
    """-> (result, dst tensor of cap + CANARY bytes)"""
    import torch
    ws = gpu.decompress_device_work_size(n_arc, cap, bs)
    assert ws > 0
    s = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(s):
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        dst = torch.empty(cap + CANARY, dtype=torch.uint8, device="cuda")
        dst[cap:] = _canary().to("cuda")
        res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        gpu.decompress_dict_device(arc.data_ptr(), n_arc, dst.data_ptr(), cap, bs, dd.tup if dd else None, work.data_ptr(), ws,
                                   res.data_ptr(), checksum, s.cuda_stream)
    s.synchronize()
    return int(res.item()), dst


GOLDEN_DICT_ARCHIVES = (("dict_http", "dict_http.zxd"), ("dict_seekable_l7", "dict_text.zxd"))


def test_golden_dictionary_archives(gpu):
    for stem, zxd in GOLDEN_DICT_ARCHIVES:
        comp, want = read(f"conformance/valid/{stem}.zxc"), read(f"conformance/valid/{stem}.expected")
        content, huf = _golden_dict(zxd)
        bs = 1 << comp[5]
        arc = _to_dev(comp, PAD)
        right, other = DevDict(gpu, content, huf), DevDict(gpu, content[:-1] + b"?", huf)
        no_table = DevDict(gpu, content, None)
        for checksum in (False, True):
            for cap in (len(want), len(want) + 1000):
                rc, dst = _dev_decompress(gpu, arc, len(comp), bs, cap, right, checksum)
                assert rc == len(want) and bytes(dst[:rc].cpu().numpy()) == want and _canary_ok(dst, cap), (stem, checksum, cap, rc)
            for dd, code in ((None, ERR["DICT_REQUIRED"]), (other, ERR["DICT_MISMATCH"]), (no_table, ERR["DICT_MISMATCH"])):
                rc, dst = _dev_decompress(gpu, arc, len(comp), bs, len(want), dd, checksum)
                host = gpu.decompress(comp, len(want), checksum, False, dict_=dd.content if dd else None, dict_huf=dd.huf if dd else None)[0]
                assert rc == code == host and _canary_ok(dst, len(want)), (stem, checksum, rc, host)
    comp = read("conformance/invalid/dict_required.zxc")  # an id nobody has the dictionary of
    arc = _to_dev(comp, PAD)
    for dd, code in ((None, ERR["DICT_REQUIRED"]), (DevDict(gpu, b"whatever", None), ERR["DICT_MISMATCH"])):
        assert _dev_decompress(gpu, arc, len(comp), 1 << comp[5], 1 << 16, dd)[0] == code


def test_a_dictionary_given_for_a_plain_archive(gpu):
    from zxc_amd import corpus
    dd = DevDict(gpu, *_golden_dict("dict_http.zxd"))
    for bs, checksum in ((4096, True), (65536, False)):
        data = corpus.synth_text(7 * bs + 99, seed=bs)
        comp = gpu.compress(data, 5, bs, True, checksum)
        assert gpu.decompress(comp, len(data), checksum, dict_=dd.content, dict_huf=dd.huf) == data
        rc, dst = _dev_decompress(gpu, _to_dev(comp, PAD), len(comp), bs, len(data), dd, checksum)
        assert rc == len(data) and bytes(dst[:rc].cpu().numpy()) == data and _canary_ok(dst, len(data)), bs


def _mutants(comp, checksum):
    """header bytes, one block's payload, the footer's hash -> (what, bytes)"""
    for at in (0, 4, 5, 6, 7, 9, 14):
        b = bytearray(comp)
        b[at] ^= 0x21
        yield f"header[{at}]", bytes(b)
    csz = int.from_bytes(comp[16 + 3: 16 + 7], "little")
    second = 16 + 8 + csz + (4 if checksum else 0)  # the second block's header
    for at in (second + 8 + 3, second + 8 + 40, second + 2):
        b = bytearray(comp)
        b[at] ^= 0x5A
        yield f"block 1[{at - second}]", bytes(b)
    for at in (len(comp) - 1, len(comp) - 4, len(comp) - 12):
        b = bytearray(comp)
        b[at] ^= 0x01
        yield f"footer[{at - len(comp)}]", bytes(b)


@pytest.mark.parametrize("bs", [4096, 65536])
def test_mutated_archives_get_the_hosts_verdict(gpu, oracle, bs):
    from zxc_amd import corpus
    content, huf = _text_dict(), _golden_dict("dict_http.zxd")[1]
    dd = DevDict(gpu, content, huf)
    data = corpus.synth_text(5 * bs + 321, seed=bs + 1)
    n_err = 0
    for checksum in (True, False):
        comp = gpu.compress(data, 3, bs, True, checksum, dict_=content, dict_huf=huf)
        for what, bad in _mutants(comp, checksum):
            for verify in (True, False):
                host = gpu.decompress(bad, len(data), verify, False, dict_=content, dict_huf=huf)
                rc, dst = _dev_decompress(gpu, _to_dev(bad, PAD), len(bad), bs, len(data), dd, verify)
                print(bs, checksum, what, verify, rc, host[0])
                assert _canary_ok(dst, len(data)), (what, verify)
                assert rc == host[0], (bs, checksum, what, verify, rc, host[0])
                o_rc, _ = oracle.decompress(bad, len(data), verify, dict_=content, dict_huf=huf)
                assert rc == o_rc, (bs, checksum, what, verify, rc, o_rc)
                if rc >= 0:
                    assert bytes(dst[:rc].cpu().numpy()) == host[1], what
                n_err += rc < 0
    assert n_err >= 20


# ---------------------------------------------------------------- ranges
def _open(gpu, arc, n_arc, bs, max_blocks):
    import torch
    isz = gpu.seekable_index_size(max_blocks)
    index = torch.full(((isz + 7) // 8,), -1, dtype=torch.int64, device="cuda")
    gpu.seekable_open_device(arc.data_ptr(), n_arc, bs, max_blocks, index.data_ptr(), isz, torch.cuda.current_stream().cuda_stream)
    return index


def _fetch(gpu, arc, n_arc, index, ranges, max_len, cap, bs, dd):
    """-> (results, dst as numpy of cap + CANARY bytes); dst starts as the pattern everywhere"""
    import torch
    n = len(ranges)
    ws = gpu.decompress_ranges_device_work_size(n, max_len, bs)
    assert ws > 0
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    dst = torch.from_numpy(_pattern(cap + CANARY)).to("cuda")
    res = torch.full((n,), UNSET, dtype=torch.int64, device="cuda")
    t = np.zeros(n, dtype=gpu.RANGE_DTYPE)
    for i, r in enumerate(ranges):
        t[i] = r
    d_ranges = torch.from_numpy(t.view(np.uint8).copy()).to("cuda")
    gpu.decompress_ranges_dict_device(arc.data_ptr(), n_arc, index.data_ptr(), d_ranges.data_ptr(), n, max_len, dst.data_ptr(), cap, bs,
                                      dd.tup if dd else None, work.data_ptr(), ws, res.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [int(x) for x in res.cpu().numpy()], dst.cpu().numpy()


def _place(want, rng):
    """destinations with gaps, every other one with dst_off = offset (mod 16) -> (ranges, max_len, capacity)"""
    out, at = [], 0
    for i, (a, n) in enumerate(want):
        at = (at + 15) // 16 * 16 + 16 * rng.randrange(3)
        d = at + ((a & 15) if i % 2 == 0 else ((a & 15) + 1 + rng.randrange(15)) % 16)
        out.append((a, n, d))
        at = d + n
    return out, max(n for a, n in want), at + 64


def _check_ranges(gpu, arc, comp, data, bs, content, huf, right, wrong, n_random, span, seed):
    rng = random.Random(seed)
    total = len(data)
    want = [(0, 1), (total - 1, 1), (0, 0), (min(7, total - 1), min(100, total - 7)), (0, min(total, bs + 32))]
    if total > 2 * bs:
        want += [(bs - 3, 6), (bs, bs), (bs - 1, bs + 2), (5, 2 * bs), (bs + 16, bs + 100)]
    for _ in range(n_random):
        a = rng.randrange(total)
        want.append((a, rng.randrange(1, min(total - a, span * bs) + 1)))
    ranges, max_len, cap = _place(want, rng)
    index = _open(gpu, arc, len(comp), bs, -(-total // bs))
    s = gpu.Seekable(comp)
    assert s.set_dict(content, huf) == 0
    untouched = _pattern(cap + CANARY)
    got, dst = _fetch(gpu, arc, len(comp), index, ranges, max_len, cap, bs, right)
    written = np.zeros(len(dst), dtype=bool)
    for (a, n, d), rc in zip(ranges, got):
        h_rc, h_out = s.decompress_range(a, n, raise_on_error=False) if n else (0, b"")
        assert rc == h_rc == n, (a, n, d, rc, h_rc)
        assert bytes(dst[d: d + n]) == h_out == data[a: a + n], (a, n, d)
        written[d: d + n] = True
    assert np.array_equal(dst[~written], untouched[~written])  # nothing outside the ranges, the canary behind the capacity included
    s.close()
    for dd, code in ((wrong, ERR["DICT_MISMATCH"]), (None, ERR["DICT_REQUIRED"])):
        got, dst = _fetch(gpu, arc, len(comp), index, ranges, max_len, cap, bs, dd)
        assert got == [code if n else 0 for a, n, d in ranges], (code, sorted(set(got)))
        assert np.array_equal(dst, untouched)  # every destination untouched


def test_ranges_of_the_golden_seekable_dictionary_archive(gpu):
    comp, data = read("conformance/valid/dict_seekable_l7.zxc"), read("conformance/valid/dict_seekable_l7.expected")
    content, huf = _golden_dict("dict_text.zxd")
    right, wrong = DevDict(gpu, content, huf), DevDict(gpu, content, None)
    _check_ranges(gpu, _to_dev(comp, PAD), comp, data, 1 << comp[5], content, huf, right, wrong, n_random=40, span=1, seed=3)


def test_ranges_of_a_large_archive_written_on_the_device(gpu, big):
    data, content, dd, arc, comp = big
    assert -(-len(data) // 4096) >= 16400
    wrong = DevDict(gpu, content[:-1] + b"?", None)
    _check_ranges(gpu, arc, comp, data, 4096, content, None, dd, wrong, n_random=600, span=4, seed=11)


# ---------------------------------------------------------------- streams
def test_round_trip_all_in_device_memory_on_a_side_stream(gpu):
    """Source, dictionary, archive and decoded bytes never leave device memory. src_size is a host argument of the decoder, so the
    host reads the compressor's 8-byte result word between the two calls: the API cannot queue them back to back without that
    synchronisation, and this test does not claim it."""
    import torch
    side = torch.cuda.Stream()
    n, bs = 37 * 4096 + 1234, 4096
    content = _text_dict(20000, seed=5)
    cap = _bound(gpu, n)
    with torch.cuda.stream(side):
        dd = DevDict(gpu, content, None, stream=side)  # the id is computed on `side` too
        base = torch.arange(n, device="cuda", dtype=torch.int64)
        src = ((base * base) // 977).remainder(23).to(torch.uint8)  # produced by torch ops queued on `side`
        src[: len(content)] = dd.d_content                            # ... and some bytes the dictionary knows
        arc = torch.full((cap + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        ws_c = gpu.compress_dict_device_work_size(n, len(content), 3, bs, True, True)
        ws_d = gpu.decompress_device_work_size(cap, n, bs)
        work_c = torch.empty(ws_c, dtype=torch.uint8, device="cuda")
        work_d = torch.empty(ws_d, dtype=torch.uint8, device="cuda")
        res_c = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        res_d = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        out = torch.zeros(n + CANARY, dtype=torch.uint8, device="cuda")
        out[n:] = _canary().to("cuda")
        gpu.compress_dict_device(src.data_ptr(), n, arc.data_ptr(), cap, dd.tup, work_c.data_ptr(), ws_c, res_c.data_ptr(), 3, bs, True, True,
                                 side.cuda_stream)
        # src_size is a host argument of the decoder: the 8-byte result word is read back to hand it over; no data is copied
        n_arc = int(res_c.item())
        assert n_arc > 0
        gpu.decompress_dict_device(arc.data_ptr(), n_arc, out.data_ptr(), n, bs, dd.tup, work_d.data_ptr(), ws_d, res_d.data_ptr(), True,
                                   side.cuda_stream)
        same = torch.equal(out[:n], src)  # compared on the device
    side.synchronize()
    assert int(res_d.item()) == n and same and _canary_ok(out, n)
    assert n_arc < n  # the dictionary and the pattern compress


def test_two_streams_at_once_with_different_dictionaries(gpu):
    import torch
    from zxc_amd import corpus
    http, huf = _golden_dict("dict_http.zxd")
    jobs = []
    for i, (bs, content, h) in enumerate(((4096, _text_dict(30000, seed=8), None), (65536, http, huf))):
        data = corpus.synth_text(40 * bs + 99 * i, seed=20 + i)
        st = torch.cuda.Stream()
        n, cap = len(data), _bound(gpu, len(data))
        ws = gpu.compress_dict_device_work_size(n, len(content), 3, bs, True, True)
        ws_d = gpu.decompress_device_work_size(cap, n, bs)
        with torch.cuda.stream(st):
            dd = DevDict(gpu, content, h, stream=st)
            src = _to_dev(data)
            work = torch.empty(ws, dtype=torch.uint8, device="cuda")
            work_d = torch.empty(ws_d, dtype=torch.uint8, device="cuda")
            arc = torch.full((cap + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
            out = torch.zeros(n + CANARY, dtype=torch.uint8, device="cuda")
            out[n:] = _canary().to("cuda")
            res = torch.full((2,), UNSET, dtype=torch.int64, device="cuda")
        st.synchronize()
        jobs.append((data, bs, st, dd, src, work, work_d, arc, out, res, cap, ws, ws_d))
    for data, bs, st, dd, src, work, work_d, arc, out, res, cap, ws, ws_d in jobs:  # both enqueued before either is waited for
        gpu.compress_dict_device(src.data_ptr(), len(data), arc.data_ptr(), cap, dd.tup, work.data_ptr(), ws, res.data_ptr(), 3, bs, True,
                                 True, st.cuda_stream)
    wants = []
    for data, bs, st, dd, src, work, work_d, arc, out, res, cap, ws, ws_d in jobs:
        st.synchronize()
        want = gpu.compress(data, 3, bs, True, True, dict_=dd.content, dict_huf=dd.huf)
        rc = int(res[0].item())
        assert rc == len(want) and bytes(arc[:rc].cpu().numpy()) == want, bs
        wants.append(rc)
    for (data, bs, st, dd, src, work, work_d, arc, out, res, cap, ws, ws_d), n_arc in zip(jobs, wants):
        gpu.decompress_dict_device(arc.data_ptr(), n_arc, out.data_ptr(), len(data), bs, dd.tup, work_d.data_ptr(), ws_d,
                                   res[1:].data_ptr(), True, st.cuda_stream)
    for data, bs, st, dd, src, work, work_d, arc, out, res, cap, ws, ws_d in jobs:
        st.synchronize()
        assert int(res[1].item()) == len(data) and bytes(out[: len(data)].cpu().numpy()) == data and _canary_ok(out, len(data)), bs
    # each archive wants its own dictionary
    (d0, bs0, _, dd0, *_r0), (d1, bs1, _, dd1, *_r1) = jobs
    arc0, arc1 = jobs[0][7], jobs[1][7]
    assert _dev_decompress(gpu, arc0, wants[0], bs0, len(d0), dd1)[0] == ERR["DICT_MISMATCH"]
    assert _dev_decompress(gpu, arc1, wants[1], bs1, len(d1), dd0)[0] == ERR["DICT_MISMATCH"]
