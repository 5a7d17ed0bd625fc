"""zxc_mi355x_decompress_device on the GPU: a whole archive in device memory decoded into device memory, the result word equal to
what this library's zxc_decompress returns for the same bytes, capacity and options; a canary behind the capacity; archives from
zxc_compress, from compress_device and from the unmodified reference; every golden conformance file; error precedence; many tiles;
stream order on torch streams; the archive left untouched. Nothing here provokes a fault: the corrupt inputs are those the host path
is tested with, and the kernels refuse them by status."""
import os

import pytest

import devtest
from conftest import GOLDEN
from devtest import CANARY, ERR, PAD, UNSET, bound as _bound, canary as _canary, canary_ok as _canary_ok, inputs as _inputs

pytestmark = pytest.mark.gpu

DICT_ARCHIVES = {"conformance/valid/dict_http.zxc", "conformance/valid/dict_seekable_l7.zxc", "conformance/invalid/dict_required.zxc"}

gpu = devtest.gpu_fixture()


def _to_dev(data: bytes, pad=PAD):
    return devtest.to_dev(data, pad)


def _dev_decompress(gpu, arc, n_arc, bs, cap, checksum=False, stream=None, sync=True):
    """-> (result or the result tensor, dst tensor of cap + CANARY bytes); the CANARY bytes behind cap start as a known pattern"""
    import torch
    ws = gpu.decompress_device_work_size(n_arc, cap, bs)
    assert ws > 0
    s = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(s):
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        dst = torch.empty(cap + CANARY, dtype=torch.uint8, device="cuda")
        dst[cap:] = _canary().to("cuda")
        res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        gpu.decompress_device(arc.data_ptr(), n_arc, dst.data_ptr(), cap, bs, work.data_ptr(), ws, res.data_ptr(), checksum, s.cuda_stream)
    if not sync:
        return res, dst, work
    s.synchronize()
    return int(res.item()), dst


def _check_round_trip(gpu, arc, n_arc, data, bs, checksum, what):
    for cap in sorted({len(data), len(data) + 1000, len(data) + 3 * bs + 77}):  # exact, and both sides of the k split
        rc, dst = _dev_decompress(gpu, arc, n_arc, bs, cap, checksum)
        assert rc == len(data), (what, cap, rc)
        assert bytes(dst[: len(data)].cpu().numpy()) == data, (what, cap)
        assert _canary_ok(dst, cap), (what, cap)


@pytest.mark.parametrize("bs", [4096, 65536, 1 << 19, 1 << 21])
@pytest.mark.parametrize("level", [1, 2, 3, 4, 5, 6, 7])
def test_round_trip(gpu, level, bs):
    import torch
    for name, data in _inputs(bs).items():
        src = _to_dev(data, 0)
        for checksum in (False, True):
            for seekable in (False, True):
                what = (name, level, bs, checksum, seekable)
                host_arc = gpu.compress(data, level, bs, seekable, checksum)
                _check_round_trip(gpu, _to_dev(host_arc), len(host_arc), data, bs, checksum, what + ("zxc_compress",))
                if checksum:  # an archive with checksums that the caller does not ask to verify
                    _check_round_trip(gpu, _to_dev(host_arc), len(host_arc), data, bs, False, what + ("unverified",))
                else:         # a caller who asks for verification of an archive without checksums
                    _check_round_trip(gpu, _to_dev(host_arc), len(host_arc), data, bs, True, what + ("nothing to verify",))
                # the archive compress_device leaves in device memory, decoded where it lies
                cap = _bound(gpu, len(data))
                ws = gpu.compress_device_work_size(len(data), level, bs, seekable, checksum)
                work = torch.empty(ws, dtype=torch.uint8, device="cuda")
                arc = torch.full((cap + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
                res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
                gpu.compress_device(src.data_ptr() if data else 0, len(data), arc.data_ptr(), cap, work.data_ptr(), ws, res.data_ptr(), level,
                                    bs, seekable, checksum, torch.cuda.current_stream().cuda_stream)
                n_arc = int(res.item())
                assert n_arc == len(host_arc), what
                _check_round_trip(gpu, arc, n_arc, data, bs, checksum, what + ("compress_device",))


def test_archives_written_by_the_reference(gpu, ref):
    for bs in (4096, 65536, 1 << 19):
        for name, data in _inputs(bs).items():
            for level in (1, 3, 5, 7):
                for checksum, seekable in ((False, False), (True, True), (False, True)):
                    arc = ref.compress(data, level, bs, seekable, checksum)
                    _check_round_trip(gpu, _to_dev(arc), len(arc), data, bs, checksum, (name, level, bs, checksum, seekable, "reference"))


def _golden(dirs):
    out = []
    for d in dirs:
        out += [f"{d}/{f}" for f in sorted(os.listdir(os.path.join(GOLDEN, d))) if f.endswith(".zxc")]
    return out


@pytest.mark.parametrize("rel", _golden(("conformance/valid", "conformance/invalid")))
def test_golden_conformance_file(gpu, rel):
    comp = open(os.path.join(GOLDEN, rel), "rb").read()
    lg = comp[5] if len(comp) > 5 else 0
    bs = 1 << lg if 12 <= lg <= 21 else 65536
    arc = _to_dev(comp)
    exp = os.path.join(GOLDEN, rel[:-4] + ".expected")
    size = os.path.getsize(exp) if os.path.exists(exp) else gpu.get_decompressed_size(comp)
    for checksum in (False, True):
        for cap in sorted({size, size + 1000, max(size - 1, 0), 0, 1 << 20}):
            what = (rel, checksum, cap)
            want, out = gpu.decompress(comp, cap, checksum, raise_on_error=False)
            if len(comp) < 28:  # refused before any launch (and no work size exists for it)
                assert gpu.decompress_device_work_size(len(comp), cap, bs) == 0
                with pytest.raises(gpu.ZxcError) as e:
                    gpu.decompress_device(arc.data_ptr(), len(comp), arc.data_ptr(), cap, bs, arc.data_ptr(), 1 << 30, arc.data_ptr(), checksum)
                assert e.value.code == want == ERR["SRC_TOO_SMALL"], what
                continue
            rc, dst = _dev_decompress(gpu, arc, len(comp), bs, cap, checksum)
            print(what, "device", rc, "host", want)
            if rel in DICT_ARCHIVES and cap > 0:
                assert rc == ERR["DICT_REQUIRED"], what
            assert rc == want, what
            assert _canary_ok(dst, cap), what
            if rc > 0:
                assert bytes(dst[:rc].cpu().numpy()) == out, what
    assert bytes(arc[: len(comp)].cpu().numpy()) == comp


def _both(gpu, comp, bs, cap, checksum):
    """-> (device result, host zxc_decompress return, device bytes, host bytes, canary intact)"""
    want, out = gpu.decompress(comp, cap, checksum, raise_on_error=False)
    rc, dst = _dev_decompress(gpu, _to_dev(comp), len(comp), bs, cap, checksum)
    return rc, want, bytes(dst[: max(rc, 0)].cpu().numpy()), out, _canary_ok(dst, cap)


def _block_offsets(arc, file_ck):
    out, ip = [], 16
    while arc[ip] != 255:
        n = 8 + int.from_bytes(arc[ip + 3: ip + 7], "little") + 4 * file_ck
        out.append((ip, n))
        ip += n
    return out, ip


@pytest.mark.parametrize("seekable", [False, True])
def test_error_precedence_on_built_archives(gpu, seekable):
    from zxc_amd import corpus
    bs = 65536
    data = corpus.synth_text(9 * bs + 333, seed=31)
    n = len(data)
    arc = gpu.compress(data, 3, bs, seekable, True)
    blocks, eof_at = _block_offsets(arc, 1)
    assert len(blocks) == 10
    rc, want, got, out, ok = _both(gpu, arc, bs, n, True)
    assert rc == want == n and got == out == data and ok
    for j in (0, 4, 9):  # one flipped payload byte in block j
        m = bytearray(arc)
        m[blocks[j][0] + 8 + blocks[j][1] // 2] ^= 0x10
        rc, want, _, _, ok = _both(gpu, bytes(m), bs, n, True)
        assert rc == want == ERR["BAD_CHECKSUM"] and ok, (j, rc, want)
        m[blocks[9][0] + 12] ^= 0x01  # and a second one behind it: the first in archive order still wins
        rc, want, _, _, ok = _both(gpu, bytes(m), bs, n, True)
        assert rc == want and ok, (j, rc, want)
    m = bytearray(arc)
    m[-1] ^= 0x80  # the footer's global hash
    rc, want, _, _, ok = _both(gpu, bytes(m), bs, n, True)
    assert rc == want == ERR["BAD_CHECKSUM"] and ok
    rc, want, got, out, ok = _both(gpu, bytes(m), bs, n, False)  # nothing is hashed without the option
    assert rc == want == n and got == data and ok
    for delta in (1, -1):  # the footer's size off by one
        m = bytearray(arc)
        m[-12:-4] = (n + delta).to_bytes(8, "little")
        rc, want, _, _, ok = _both(gpu, bytes(m), bs, n + 1, True)
        assert rc == want == ERR["CORRUPT_DATA"] and ok, delta
    for cap in (n - 1, n - 334, n - 335, bs, 1):  # capacities short by a byte, by the tail, by a block and more
        rc, want, _, _, ok = _both(gpu, arc, bs, cap, True)
        assert rc == want == ERR["DST_TOO_SMALL"] and ok, cap
    # a failing block in front of the block that does not fit keeps its precedence; one behind it does not
    m = bytearray(arc)
    m[blocks[2][0] + 8 + 5] ^= 0x04
    for cap in (n, 5 * bs, 3 * bs, 2 * bs, 2 * bs + 1, bs):
        rc, want, _, _, ok = _both(gpu, bytes(m), bs, cap, True)
        assert rc == want and ok, (cap, rc, want)
    # a bad block header in the chain counts only if the blocks in front of it decode
    m = bytearray(arc)
    m[blocks[6][0] + 1] ^= 0xFF
    for cap in (n, 3 * bs):
        rc, want, _, _, ok = _both(gpu, bytes(m), bs, cap, False)
        assert rc == want < 0 and ok, (cap, rc, want)
    m[blocks[3][0] + 8 + 9] ^= 0x40
    rc, want, _, _, ok = _both(gpu, bytes(m), bs, n, True)
    assert rc == want < 0 and ok, (rc, want)


def test_a_changed_seek_entry_leaves_the_bytes_right(gpu):
    from zxc_amd import corpus
    bs = 4096
    data = corpus.synth_text(2500 * bs + 9, seed=32)  # three tiles of entries
    arc = gpu.compress(data, 3, bs, True, False)
    nb = 2501
    first = len(arc) - 12 - 4 * nb
    for entry in (0, 1023, 1024, 2500):
        m = bytearray(arc)
        m[first + 4 * entry] ^= 0x01
        rc, want, got, out, ok = _both(gpu, bytes(m), bs, len(data), False)
        assert rc == want == len(data) and got == out == data and ok, entry


def test_wrong_block_size_argument(gpu):
    from zxc_amd import corpus
    data = corpus.synth_text(3 * 65536, seed=33)
    arc = gpu.compress(data, 3, 65536, True, False)
    for bs in (4096, 32768, 1 << 17, 1 << 21):
        rc, dst = _dev_decompress(gpu, _to_dev(arc), len(arc), bs, len(data))
        assert rc == ERR["BAD_BLOCK_SIZE"] and _canary_ok(dst, len(data)), bs


def test_irregular_frame_is_unsupported(gpu):
    """two blocks from zxc_compress_block, the first shorter than block_size: the host decodes it, the device call names it"""
    from oracle_py import BlockApi
    from zxc_amd import corpus
    bs = 4096
    a, b = corpus.synth_text(3000, seed=34), corpus.synth_text(4096, seed=35)
    api = BlockApi(gpu.lib())
    rc_a, blk_a = api.compress_block(a, 3, False, bs)
    rc_b, blk_b = api.compress_block(b, 3, False, bs)
    api.close()
    assert rc_a > 8 and rc_b > 8
    shell = gpu.compress(b"Q", 3, bs, False, False)
    frame = shell[:16] + blk_a + blk_b + shell[-20:-12] + (len(a) + len(b)).to_bytes(8, "little") + bytes(4)
    assert gpu.decompress(frame) == a + b
    rc, dst = _dev_decompress(gpu, _to_dev(frame), len(frame), bs, len(a) + len(b))
    assert rc == ERR["GPU_UNSUPPORTED"] and _canary_ok(dst, len(a) + len(b))
    # the same two blocks the other way round are a regular frame
    frame = shell[:16] + blk_b + blk_a + shell[-20:-12] + (len(a) + len(b)).to_bytes(8, "little") + bytes(4)
    rc, dst = _dev_decompress(gpu, _to_dev(frame), len(frame), bs, len(a) + len(b))
    assert rc == len(a) + len(b) and bytes(dst[:rc].cpu().numpy()) == b + a


@pytest.mark.parametrize("seekable", [False, True])
def test_many_tiles(gpu, seekable):
    """65 536 blocks of 4 KiB with checksums: 64 tiles of the scans, of the hash fold and of the verdict"""
    import hashlib
    from zxc_amd import corpus
    data = corpus.synth_silesia(256 << 20, seed=5)
    arc = gpu.compress(data, 3, 4096, seekable, True)
    rc, dst = _dev_decompress(gpu, _to_dev(arc), len(arc), 4096, len(data), True)
    assert rc == len(data) and _canary_ok(dst, len(data))
    assert hashlib.sha256(dst[:rc].cpu().numpy().tobytes()).digest() == hashlib.sha256(data).digest()
    m = bytearray(arc)
    m[-2] ^= 0x01
    rc, dst = _dev_decompress(gpu, _to_dev(bytes(m)), len(arc), 4096, len(data), True)
    assert rc == ERR["BAD_CHECKSUM"]


@pytest.mark.parametrize("seekable", [False, True])
def test_more_tiles_than_scan_threads(gpu, seekable):
    """257 x 1024 + 5 blocks: more tiles than the scan pass has threads, so each of its threads sums several"""
    import torch
    n = (257 * 1024 + 5) * 4096 - 3
    arc = gpu.compress(bytes(n), 1, 4096, seekable, True)
    rc, dst = _dev_decompress(gpu, _to_dev(arc), len(arc), 4096, n, True)
    assert rc == n and _canary_ok(dst, n)
    assert not bool(dst[:n].any())
    del dst
    torch.cuda.empty_cache()


def test_archive_produced_on_a_side_stream(gpu):
    """compress_device and decompress_device queued on one side stream with no synchronisation in between. The decode needs the
    archive's size as src_size on the host: a caller who parks archives in HBM keeps their sizes; here it comes from zxc_compress,
    which writes the same bytes."""
    import torch
    side = torch.cuda.Stream()
    bs, n = 65536, 3 * 65536 + 4321
    base = torch.arange(n, device="cuda", dtype=torch.int64)
    first = ((base * base) // 977).remainder(23).to(torch.uint8)
    data = bytes(first.cpu().numpy())
    want = gpu.compress(data, 3, bs, True, True)
    cap = _bound(gpu, n)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        src = ((base * base) // 977).remainder(23).to(torch.uint8)  # produced by torch ops queued on `side`
        ws = gpu.compress_device_work_size(n, 3, bs, True, True)
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        arc = torch.zeros(cap + PAD, dtype=torch.uint8, device="cuda")
        res_c = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        gpu.compress_device(src.data_ptr(), n, arc.data_ptr(), cap, work.data_ptr(), ws, res_c.data_ptr(), 3, bs, True, True, side.cuda_stream)
        res, dst, _work = _dev_decompress(gpu, arc, len(want), bs, n, True, stream=side, sync=False)
    side.synchronize()
    assert int(res_c.item()) == len(want) and int(res.item()) == n
    assert bytes(dst[:n].cpu().numpy()) == data and _canary_ok(dst, n)


def test_two_streams_at_once(gpu):
    import torch
    from zxc_amd import corpus
    calls = []
    for i, bs in enumerate((4096, 65536)):
        data = corpus.synth_text(40 * bs + 99 * i, seed=20 + i)
        arc = gpu.compress(data, 3, bs, bool(i), True)
        calls.append((data, bs, torch.cuda.Stream(), _to_dev(arc), len(arc)))
    torch.cuda.synchronize()
    flying = []
    for data, bs, st, arc, n_arc in calls:  # both enqueued before either is waited for
        flying.append(_dev_decompress(gpu, arc, n_arc, bs, len(data), True, stream=st, sync=False))
    for (data, bs, st, arc, n_arc), (res, dst, _work) in zip(calls, flying):
        st.synchronize()
        assert int(res.item()) == len(data) and bytes(dst[: len(data)].cpu().numpy()) == data and _canary_ok(dst, len(data)), bs


def test_archive_is_read_only(gpu):
    from zxc_amd import corpus
    data = corpus.synth_text(2 * 65536 + 17, seed=4)
    for seekable in (False, True):
        comp = gpu.compress(data, 3, 65536, seekable, True)
        arc = _to_dev(comp)
        before = arc.clone()
        for cap, checksum in ((len(data), True), (len(data) - 1, True), (len(data) + 5, False), (0, False)):
            _dev_decompress(gpu, arc, len(comp), 65536, cap, checksum)
        import torch
        assert torch.equal(arc, before)


def test_frame_info_device(gpu):
    from zxc_amd import corpus
    import torch
    for bs in (4096, 65536, 1 << 21):
        for checksum in (False, True):
            for n in (0, 1, bs + 5):
                comp = gpu.compress(corpus.synth_text(n, seed=6) if n else b"", 3, bs, True, checksum)
                arc = _to_dev(comp)
                got = gpu.frame_info_device(arc.data_ptr(), len(comp), torch.cuda.current_stream().cuda_stream)
                assert got == (1 << comp[5], gpu.get_decompressed_size(comp), checksum) == (bs, n, checksum)
    bad = bytearray(comp)
    bad[0] ^= 1
    with pytest.raises(gpu.ZxcError) as e:
        gpu.frame_info_device(_to_dev(bytes(bad)).data_ptr(), len(bad))
    assert e.value.code == -4  # ZXC_ERROR_BAD_MAGIC
