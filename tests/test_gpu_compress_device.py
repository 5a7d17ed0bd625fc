"""zxc_mi355x_compress_device on the GPU: a whole archive from device memory to device memory, byte for byte the one
zxc_compress writes, read back by the unmodified reference decoder; capacity edges with a canary behind the capacity; stream
order on torch streams; the source left untouched."""
import random

import pytest

import devtest
from devtest import CANARY, UNSET, bound as _bound, canary_ok as _canary_ok, inputs as _inputs

pytestmark = pytest.mark.gpu

gpu = devtest.gpu_fixture()


def _to_dev(data: bytes):
    return devtest.to_dev(data, exact=True)


def _dev_compress(gpu, src, n, level, bs, seekable, checksum, cap=None, stream=None):
    """-> (result, dst tensor of cap + CANARY bytes, cap); the CANARY bytes behind cap start as a known pattern"""
    import torch
    cap = _bound(gpu, n) if cap is None else cap
    ws = gpu.compress_device_work_size(n, level, bs, seekable, checksum)
    assert ws > 0
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    dst = torch.empty(cap + CANARY, dtype=torch.uint8, device="cuda")
    dst[cap:] = torch.arange(CANARY, device="cuda", dtype=torch.int32).remainder(251).to(torch.uint8) + 1
    res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream() if stream is None else stream
    gpu.compress_device(src.data_ptr() if n else 0, n, dst.data_ptr(), cap, work.data_ptr(), ws, res.data_ptr(), level, bs,
                        seekable, checksum, s.cuda_stream)
    s.synchronize()
    return int(res.item()), dst, cap


@pytest.mark.parametrize("bs", [4096, 65536, 1 << 19, 1 << 21])
@pytest.mark.parametrize("level", [1, 2, 3, 4, 5, 6, 7])
def test_byte_identity_with_zxc_compress(gpu, ref, level, bs):
    rnd = random.Random(level * 1000 + bs)
    for name, data in _inputs(bs).items():
        src = _to_dev(data)
        for checksum in (False, True):
            for seekable in (False, True):
                what = (name, level, bs, checksum, seekable)
                want = gpu.compress(data, level, bs, seekable, checksum)
                rc, dst, cap = _dev_compress(gpu, src, len(data), level, bs, seekable, checksum)
                assert rc == len(want), (what, rc, len(want))
                assert bytes(dst[:rc].cpu().numpy()) == want, what
                assert _canary_ok(dst, cap), what
                if checksum:
                    r, out = ref.decompress(want, len(data), checksum=True)
                    assert r == len(data) and out == data, what
                if seekable and data:
                    off = rnd.randrange(len(data))
                    ln = rnd.randrange(1, len(data) - off + 1)
                    r, out = ref.seekable_range_mt(want, off, ln, 4)
                    assert r == ln and out == data[off: off + ln], (what, off, ln)


def test_empty_input_is_the_36_byte_archive(gpu):
    for seekable in (False, True):
        for checksum in (False, True):
            rc, dst, cap = _dev_compress(gpu, None, 0, 3, 0, seekable, checksum, cap=36)
            want = gpu.compress(b"", 3, 1 << 19, seekable, checksum)
            assert rc == 36 == len(want) and bytes(dst[:36].cpu().numpy()) == want and _canary_ok(dst, cap)


def test_many_tiles(gpu, ref):
    """65 536 blocks of 4 KiB, checksummed and seekable: 64 tiles of the scans and of the hash fold, and the host path cuts
    four 64 MiB pieces."""
    from zxc_amd import corpus
    import hashlib
    data = corpus.synth_silesia(256 << 20, seed=5)
    want = gpu.compress(data, 3, 4096, True, True)
    rc, dst, cap = _dev_compress(gpu, _to_dev(data), len(data), 3, 4096, True, True)
    assert rc == len(want) and bytes(dst[:rc].cpu().numpy()) == want and _canary_ok(dst, cap)
    del dst
    r, out = ref.decompress(want, len(data), checksum=True)
    assert r == len(data) and hashlib.sha256(out).digest() == hashlib.sha256(data).digest()
    r, out = ref.seekable_range_mt(want, 100 << 20, 3 << 20, 4)
    assert r == 3 << 20 and out == data[100 << 20: 103 << 20]


def test_more_tiles_than_finish_threads(gpu):
    """257 x 1024 + 5 blocks: more tiles than the finish pass has threads, so each of its threads sums several."""
    import torch
    n = (257 * 1024 + 5) * 4096 - 3
    data = bytes(n)
    want = gpu.compress(data, 1, 4096, True, True)
    src = torch.zeros(n, dtype=torch.uint8, device="cuda")
    rc, dst, cap = _dev_compress(gpu, src, n, 1, 4096, True, True, cap=len(want) + 1000)
    assert rc == len(want) and bytes(dst[:rc].cpu().numpy()) == want and _canary_ok(dst, cap)


@pytest.mark.parametrize("checksum", [False, True])
def test_capacity_edges(gpu, checksum):
    from zxc_amd import corpus
    data = corpus.synth_text(5 * 65536 + 123, seed=9)
    src = _to_dev(data)
    want = gpu.compress(data, 3, 65536, True, checksum)
    rc, dst, cap = _dev_compress(gpu, src, len(data), 3, 65536, True, checksum, cap=len(want))
    assert rc == len(want) and bytes(dst[:rc].cpu().numpy()) == want and _canary_ok(dst, cap)
    rc, dst, cap = _dev_compress(gpu, src, len(data), 3, 65536, True, checksum, cap=len(want) - 1)
    assert rc == -2 and _canary_ok(dst, cap)  # ZXC_ERROR_DST_TOO_SMALL


def test_source_produced_on_a_side_stream(gpu):
    import torch
    side = torch.cuda.Stream()
    n = 3 * 65536 + 4321
    with torch.cuda.stream(side):
        base = torch.arange(n, device="cuda", dtype=torch.int64)
        src = ((base * base) // 977).remainder(23).to(torch.uint8)  # produced by torch ops queued on `side`
        rc, dst, _ = _dev_compress(gpu, src, n, 3, 65536, True, True, stream=side)
    data = bytes(src.cpu().numpy())
    want = gpu.compress(data, 3, 65536, True, True)
    assert rc == len(want) and bytes(dst[:rc].cpu().numpy()) == want


def test_two_streams_at_once(gpu):
    import torch
    from zxc_amd import corpus
    jobs = []
    for i, bs in enumerate((4096, 65536)):
        data = corpus.synth_text(40 * bs + 99 * i, seed=20 + i)
        st = torch.cuda.Stream()
        src = _to_dev(data)
        torch.cuda.synchronize()
        n = len(data)
        cap = _bound(gpu, n)
        ws = gpu.compress_device_work_size(n, 3, bs, True, True)
        with torch.cuda.stream(st):
            work = torch.empty(ws, dtype=torch.uint8, device="cuda")
            dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
            res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        jobs.append((data, bs, st, src, work, dst, res, cap, ws))
    for data, bs, st, src, work, dst, res, cap, ws in jobs:  # both enqueued before either is waited for
        gpu.compress_device(src.data_ptr(), len(data), dst.data_ptr(), cap, work.data_ptr(), ws, res.data_ptr(), 3, bs,
                            True, True, st.cuda_stream)
    for data, bs, st, src, work, dst, res, cap, ws in jobs:
        st.synchronize()
        want = gpu.compress(data, 3, bs, True, True)
        rc = int(res.item())
        assert rc == len(want) and bytes(dst[:rc].cpu().numpy()) == want, bs


def test_source_is_read_only(gpu):
    from zxc_amd import corpus
    data = corpus.synth_text(2 * 65536 + 17, seed=4)
    src = _to_dev(data)
    before = src.clone()
    for level in (3, 7):
        rc, _, _ = _dev_compress(gpu, src, len(data), level, 65536, True, True)
        assert rc > 0
    assert bytes(src.cpu().numpy()) == data and bytes(before.cpu().numpy()) == data
