"""zxc_mi355x_compress_batch_device on the GPU: many buffers that lie in one device buffer compressed into many archives in another
by one call. Every successful item's archive equals zxc_amd.compress of a host copy of the same bytes with the same options (the
host API over the same encoder), for a subset also what compress_device writes, and a pattern is intact everywhere outside the
archives. Every level (each of the six job-table entries, the optimal parse, PivCo sections), seekable and checksums on and off,
text-like and incompressible payloads, items at odd source offsets with unrelated bytes between them, destinations 16-aligned and
odd; larger blocks; the same item between different neighbours; more items than a plan workgroup has threads; refused items
beside good ones; a shared dictionary; two streams; stream order behind the copy that wrote the item table; a round trip through
decompress_batch_device; the unmodified reference as the decoder. Nothing here provokes a fault: every refused input is refused
by status."""
import os
import random

import numpy as np
import pytest

import devtest
from conftest import GOLDEN, load_dict
from dev_batch import SIZES_4K, Area, host as _host, payload as _payload, run as _run
from devtest import CANARY, ERR, PAD, UNSET, bound as _bound, pattern as _pattern, to_dev as _to_dev

pytestmark = pytest.mark.gpu

gpu = devtest.gpu_fixture("compress_batch_device")


def _verify(gpu, table, datas, got, dst, level, bs, seekable, checksum, dict_=None, huf=None, want_err=None):
    """every item against the host API; want_err: {item index: error} for the items that must be refused (their destination stays
    the pattern). -> the archives of the good items. No item is left out."""
    want_err = want_err or {}
    keep = np.zeros(len(dst), dtype=bool)
    arcs = {}
    assert len(got) == len(table) == len(datas)
    for r, (row, data, rc) in enumerate(zip(table, datas, got)):
        d = int(row["dst_off"])
        w = (r, len(data), level, bs, seekable, checksum, d, int(row["src_off"]))
        if r in want_err:
            assert rc == want_err[r], (w, rc)
            continue
        want = _host(gpu, data, level, bs, seekable, checksum, dict_, huf)
        assert rc == len(want), (w, rc, len(want))
        assert rc <= int(row["dst_capacity"])
        arcs[r] = dst[d: d + rc].tobytes()
        assert arcs[r] == want, w
        keep[d: d + rc] = True
    assert np.array_equal(dst[~keep], _pattern(len(dst))[~keep])  # gaps, refused items, behind every archive
    return arcs


def _device_written(gpu, data, level, bs, seekable, checksum):
    """compress_device -> the archive's bytes"""
    return bytes(devtest.device_written(gpu, data, level, bs, seekable, checksum).cpu().numpy())


area_4k = devtest.area_4k_fixture(Area, SIZES_4K, _payload)


@pytest.mark.parametrize("level", [1, 2, 3, 4, 5, 6, 7])
def test_parity_with_the_host_api_at_4k_blocks(gpu, area_4k, level):
    area, src, table, datas = area_4k
    assert len(table) == 22 and (table["src_off"] % 2 == 1).any() and (table["src_off"] % 2 == 0).any()
    assert (table["dst_off"] % 16 == 0).any() and (table["dst_off"] % 2 == 1).any()
    for seekable, checksum in ((0, 0), (1, 0), (0, 1), (1, 1)):
        got, dst = _run(gpu, src, len(area.buf), table, max(SIZES_4K), area.dst_at, level, 4096, seekable, checksum)
        arcs = _verify(gpu, table, datas, got, dst, level, 4096, seekable, checksum)
        assert len(arcs) == 22
        if seekable and checksum:  # a subset against the single-archive call
            for r in [r for r, d in enumerate(datas) if len(d) in (1, 4097, 16 * 4096)]:
                assert arcs[r] == _device_written(gpu, datas[r], level, 4096, seekable, checksum), (r, level)
    assert bytes(src[: len(area.buf)].cpu().numpy()) == bytes(area.buf)  # d_src is never written


@pytest.mark.parametrize("bs,levels", [(65536, (1, 3, 6)), (1 << 17, (2, 3, 4, 5, 7))])
def test_larger_blocks(gpu, bs, levels):
    """two blocks plus a tail; above 64 KiB levels 3-5 take the entry with the 2^15 chain ring"""
    area = Area(gpu, bs)
    for k, size in enumerate((2 * bs + 777, bs + 1, 2 * bs + 31)):
        area.add(_payload(size, (0, 2, 3)[k]))
    src, table = area.tensor(), area.table()
    for i, level in enumerate(levels):
        seekable, checksum = i & 1, (i >> 1) & 1 ^ 1
        got, dst = _run(gpu, src, len(area.buf), table, 2 * bs + 777, area.dst_at, level, bs, seekable, checksum)
        assert len(_verify(gpu, table, area.datas, got, dst, level, bs, seekable, checksum)) == 3


def test_an_archive_does_not_depend_on_its_neighbours(gpu):
    """the same bytes twice in the source area, between different bytes: the 32 bytes the encoder reads past a block differ"""
    import zxc_amd
    bs = 4096
    datas = [_payload(n, k) for k, n in enumerate((100, 4095, 4096 + 1, 2 * 4096, 2 * 4096 + 100, 5 * 4096 - 3))]
    buf, rows, dst_at = bytearray(), [], 0
    for fill in (0x00, 0xFF):
        for k, d in enumerate(datas):
            buf += bytes([fill ^ (k * 37 & 0xFF)]) * (33 + k)
            cap = _bound(gpu, len(d))
            rows.append((len(buf), len(d), dst_at, cap))
            buf += d
            dst_at += cap + 5
        buf += bytes([fill]) * 64
    table = np.zeros(len(rows), dtype=zxc_amd.ITEM_DTYPE)
    for i, r in enumerate(rows):
        table[i] = r
    src = _to_dev(bytes(buf), PAD)
    for level, seekable, checksum in ((1, 0, 1), (3, 1, 0), (7, 1, 1)):
        got, dst = _run(gpu, src, len(buf), table, 5 * 4096, dst_at, level, bs, seekable, checksum)
        arcs = _verify(gpu, table, datas + datas, got, dst, level, bs, seekable, checksum)
        for k in range(len(datas)):
            assert arcs[k] == arcs[k + len(datas)], (k, level)


def test_three_hundred_items_cross_the_plan_workgroup(gpu):
    area = Area(gpu, 33)
    for k in range(300):
        area.add(_payload(100 + (k * 37) % 600, k))
    order = list(range(300))
    random.Random(8).shuffle(order)
    table, datas = area.table(order), [area.datas[k] for k in order]
    got, dst = _run(gpu, area.tensor(), len(area.buf), table, 700, area.dst_at, 3, 4096, 1, 1)
    assert len(_verify(gpu, table, datas, got, dst, 3, 4096, 1, 1)) == 300


def test_refused_items_beside_good_ones(gpu):
    level, bs, seekable, checksum, max_size = 3, 4096, 1, 1, 3 * 4096
    area = Area(gpu, 44)
    good = [area.add(_payload(n, k)) for k, n in enumerate((5000, 1, 3 * 4096, 4096))]
    short_data = _payload(2 * 4096 + 9, 6)
    short = area.add(short_data, cap=len(_host(gpu, short_data, level, bs, seekable, checksum)) - 1)  # one byte short: the finish refuses
    tiny = area.add(_payload(5000, 1), cap=16 + 2 * 12 + 8 + 16 + 12 - 1)                     # below the known part: the plan refuses
    over = area.add(_payload(max_size + 1, 2))                                                   # above max_size
    good.append(area.add(_payload(777, 9)))
    past = area.add(b"", src_size=100)       # its 100 bytes would end behind src_capacity: it is the last thing in the area
    wrap = area.add(b"", src_size=(1 << 64) - 5)
    src_cap = len(area.buf) + 50
    area.buf += bytes(50)
    table = area.table()
    table["src_off"][past] = src_cap - 99
    got, dst = _run(gpu, area.tensor(), src_cap, table, max_size, area.dst_at, level, bs, seekable, checksum)
    want_err = {short: ERR["DST_TOO_SMALL"], tiny: ERR["DST_TOO_SMALL"], over: ERR["OVERFLOW"], past: ERR["SRC_TOO_SMALL"],
                wrap: ERR["SRC_TOO_SMALL"]}
    arcs = _verify(gpu, table, area.datas, got, dst, level, bs, seekable, checksum, want_err=want_err)
    assert sorted(arcs) == sorted(good)


def test_the_end_of_the_destination_area_binds(gpu):
    level, bs, seekable, checksum = 3, 4096, 0, 1
    area = Area(gpu, 45)
    first = area.add(_payload(6000, 1))
    last = area.add(_payload(4096 + 50, 2), cap=1 << 40)  # the item's own capacity does not bind
    behind = area.add(_payload(10, 4))
    end = area.rows[last][2] + len(_host(gpu, area.datas[last], level, bs, seekable, checksum))
    src, table = area.tensor(), area.table()
    table["dst_off"][behind] = end + 1  # behind the area in both calls: capacity 0
    got, dst = _run(gpu, src, len(area.buf), table, 6000, end, level, bs, seekable, checksum)  # the last archive ends with the area
    arcs = _verify(gpu, table, area.datas, got, dst, level, bs, seekable, checksum, want_err={behind: ERR["DST_TOO_SMALL"]})
    assert sorted(arcs) == [first, last]
    got, dst = _run(gpu, src, len(area.buf), table, 6000, end - 1, level, bs, seekable, checksum)  # ... one byte short
    arcs = _verify(gpu, table, area.datas, got, dst, level, bs, seekable, checksum,
                   want_err={last: ERR["DST_TOO_SMALL"], behind: ERR["DST_TOO_SMALL"]})
    assert sorted(arcs) == [first]


def test_dictionary_batch(gpu):
    import torch
    bs = 4096
    content, huf = load_dict(os.path.join(GOLDEN, "conformance", "valid", "dict_http.zxd"))
    area = Area(gpu, 9)
    for k, size in enumerate((0, 1, 700, 4095, 4096, 4097, 3 * 4096 + 5, 9000)):
        area.add((content[: size // 2] + _payload(size, k))[:size])  # some bytes the dictionary knows
    src, table = area.tensor(), area.table()
    d_content, d_huf = _to_dev(content), _to_dev(huf)
    d_id = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    gpu.dict_prepare_device(d_content.data_ptr(), len(content), d_huf.data_ptr(), d_id.data_ptr(), torch.cuda.current_stream().cuda_stream)
    dd = (d_content.data_ptr(), len(content), d_huf.data_ptr(), d_id.data_ptr())
    for level, seekable, checksum in ((1, 1, 0), (3, 0, 1), (6, 1, 1), (7, 0, 0)):
        got, dst = _run(gpu, src, len(area.buf), table, 3 * 4096 + 5, area.dst_at, level, bs, seekable, checksum, dd=dd)
        arcs = _verify(gpu, table, area.datas, got, dst, level, bs, seekable, checksum, dict_=content, huf=huf)
        assert len(arcs) == 8 and all(a[6] & 0x40 for a in arcs.values())  # the header's dictionary flag
    text, text_huf = load_dict(os.path.join(GOLDEN, "conformance", "valid", "dict_text.zxd"))
    d_content, d_huf = _to_dev(text), _to_dev(text_huf)
    gpu.dict_prepare_device(d_content.data_ptr(), len(text), d_huf.data_ptr(), d_id.data_ptr(), torch.cuda.current_stream().cuda_stream)
    dd = (d_content.data_ptr(), len(text), d_huf.data_ptr(), d_id.data_ptr())
    got, dst = _run(gpu, src, len(area.buf), table, 3 * 4096 + 5, area.dst_at, 3, bs, 1, 1, dd=dd)
    _verify(gpu, table, area.datas, got, dst, 3, bs, 1, 1, dict_=text, huf=text_huf)


def test_item_table_written_on_the_stream_and_two_streams_at_once(gpu):
    import torch
    bs, n = 4096, 400
    area = Area(gpu, 12)
    for k in range(n):
        area.add(_payload(1 + (k * 1531) % (3 * bs), k))
    src = area.tensor()
    runs = []
    for s_i, s in enumerate((torch.cuda.Stream(), torch.cuda.Stream())):
        order = list(range(n))
        random.Random(70 + s_i).shuffle(order)
        table, datas = area.table(order), [area.datas[k] for k in order]
        good = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
        d_items = torch.zeros_like(good)  # every item an empty source with no room (DST_TOO_SMALL) until the copy below has run
        runs.append((s, table, datas, good, d_items))
    torch.cuda.synchronize()
    out = []
    for s, table, datas, good, d_items in runs:  # both enqueued before either is waited for
        with torch.cuda.stream(s):
            d_items.copy_(good, non_blocking=True)  # the operation that writes d_items, on the call's stream, nothing waited for
            out.append(_run(gpu, src, len(area.buf), table, 3 * bs, area.dst_at, 3, bs, 1, 1, stream=s, sync=False, d_items=d_items))
    for (s, table, datas, good, d_items), (res, dst, work, _) in zip(runs, out):
        s.synchronize()
        got = [int(x) for x in res.cpu().numpy()[:n]]
        assert len(_verify(gpu, table, datas, got, dst.cpu().numpy(), 3, bs, 1, 1)) == n
    assert bytes(src[: len(area.buf)].cpu().numpy()) == bytes(area.buf)  # d_src unchanged


def test_round_trip_through_decompress_batch_device(gpu):
    """the results and the item table of a compress batch are, with two columns swapped in on the device, the item table of the
    decompress batch. (decompress_batch_device is the other feature: a failure here that the parity tests above do not share points
    there.)"""
    import torch
    bs, level = 4096, 3
    area = Area(gpu, 77)
    for k in range(64):
        area.add(_payload((k * 2039) % (4 * bs + 1), k))
    src, table = area.tensor(), area.table()
    n, max_size = len(table), 4 * bs
    res, arc, work, d_items = _run(gpu, src, len(area.buf), table, max_size, area.dst_at, level, bs, 1, 1, sync=False)
    # decompress items: the archive lies where the compress item's destination was and is as long as its result; the decoded
    # bytes go to 16-aligned places of a new area
    out_off = torch.arange(n, dtype=torch.int64, device="cuda") * (max_size + 64)
    it = d_items.view(torch.int64).view(n, 4)
    back = torch.stack([it[:, 2], res[:n], out_off, it[:, 1]], dim=1).contiguous()
    out_cap = n * (max_size + 64)
    out = torch.from_numpy(_pattern(out_cap + CANARY)).to("cuda")
    res2 = torch.full((n,), UNSET, dtype=torch.int64, device="cuda")
    ws = gpu.decompress_batch_device_work_size(n, max_size, bs)
    work2 = torch.empty(ws, dtype=torch.uint8, device="cuda")
    gpu.decompress_batch_device(arc.data_ptr(), area.dst_at, back.data_ptr(), n, max_size, out.data_ptr(), out_cap, bs, work2.data_ptr(), ws,
                                res2.data_ptr(), True, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    sizes, decoded = res2.cpu().numpy(), out.cpu().numpy()
    assert (res[:n].cpu().numpy() > 0).all()
    for r, data in enumerate(area.datas):
        assert int(sizes[r]) == len(data), (r, int(sizes[r]), len(data))
        at = r * (max_size + 64)
        assert decoded[at: at + len(data)].tobytes() == data, r


def test_the_reference_decodes_every_archive(gpu, ref, area_4k):
    area, src, table, datas = area_4k
    for level, seekable, checksum in ((3, 1, 1), (7, 0, 1), (1, 1, 0)):
        got, dst = _run(gpu, src, len(area.buf), table, max(SIZES_4K), area.dst_at, level, 4096, seekable, checksum)
        for row, data, rc in zip(table, datas, got):
            assert rc > 0
            d = int(row["dst_off"])
            n, back = ref.decompress(dst[d: d + rc].tobytes(), len(data), checksum=bool(checksum))
            assert n == len(data) and back == data, (len(data), level, seekable, checksum)
