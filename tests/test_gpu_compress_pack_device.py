"""zxc_mi355x_compress_pack_device on the GPU: many buffers that lie in one device buffer compressed by one call into archives that
lie back to back in another, each at a multiple of `align`, with the table that zxc_mi355x_decompress_batch_device takes. Every
written archive, found through d_packed, equals zxc_amd.compress of a host copy of the item (for one configuration also what
compress_batch_device writes for the same table); the offsets are the ones a few lines of Python compute from the archive sizes;
the destination's pattern is intact in every gap, behind *d_total and behind the capacity. 4 KiB blocks and one case at 64 KiB,
levels 3 and 6, seekable and checksums on and off, text-like and incompressible payloads at odd source offsets with unrelated
bytes between them; d_dst at an odd address; more items than a scan tile; items without a size at the tile and workgroup edges;
the capacity cut inside an archive, exactly *d_total, and the sizing run without a destination; a round trip through
decompress_batch_device on one stream with nothing read back in between; the packed table written over the item table; a shared
dictionary; stream order behind the copy that wrote the item table, and two streams at once. Nothing here provokes a fault:
every refused input is refused by status."""
import os
import random

import numpy as np
import pytest

import devtest
from conftest import GOLDEN, load_dict
from dev_batch import SIZES_4K, Area, host as _host, payload as _payload, run as _run_batch  # (the batch call's)
from devtest import CANARY, ERR, UNSET, pattern as _pattern, to_dev as _to_dev

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1

gpu = devtest.gpu_fixture("compress_pack_device")


def _run(gpu, src, src_cap, table, max_size, dst_cap, align, level, bs, seekable, checksum, dd=False, stream=None, sync=True, d_items=None,
         in_place=False, odd_dst=False, no_dst=False):
    """one call. dd: False = the call without a dictionary argument, else the _dict call's (None: no dictionary). The destination
    starts as the pattern everywhere, d_packed as 0xEE, *d_total as UNSET. -> (results, packed table, total, dst as numpy of
    dst_cap + CANARY bytes from d_dst on)"""
    import torch
    import zxc_amd
    s = torch.cuda.current_stream() if stream is None else stream
    n = len(table)
    ws = gpu.compress_pack_device_work_size(n, max_size, level, bs, seekable, checksum, dict_size=dd[1] if dd else 0)
    assert ws > 0
    with torch.cuda.stream(s):
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        whole = torch.empty(dst_cap + CANARY + 1, dtype=torch.uint8, device="cuda")
        dst = whole[1:] if odd_dst else whole[:-1]
        dst.copy_(torch.from_numpy(_pattern(dst_cap + CANARY)))
        assert dst.data_ptr() % 2 == (1 if odd_dst else 0)
        res = torch.full((max(n, 1),), UNSET, dtype=torch.int64, device="cuda")
        total = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
        if d_items is None:
            d_items = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
        packed = d_items if in_place else torch.full((max(n, 1) * 32,), 0xEE, dtype=torch.uint8, device="cuda")
        args = (src.data_ptr(), src_cap, d_items.data_ptr(), n, max_size, 0 if no_dst else dst.data_ptr(), dst_cap, align)
        tail = (work.data_ptr(), ws, packed.data_ptr(), res.data_ptr(), total.data_ptr(), level, bs, seekable, checksum, s.cuda_stream)
        if dd is False:
            gpu.compress_pack_device(*args, *tail)
        else:
            gpu.compress_pack_dict_device(*args, dd, *tail)
    if not sync:
        return res, packed, total, dst, work, d_items
    s.synchronize()
    return ([int(x) for x in res.cpu().numpy()[:n]], packed.cpu().numpy()[: 32 * n].view(zxc_amd.ITEM_DTYPE), int(total.item()),
            dst.cpu().numpy())


def _model(sizes, align, cap):
    """the layout, on its own: sizes[r] is None for an item without a size -> (at per item or None, written per item, total)"""
    at, end = [None] * len(sizes), 0
    for r, size in enumerate(sizes):
        if size is not None:
            at[r] = -(-end // align) * align
            end = at[r] + size
    return at, [a is not None and a + s <= cap for a, s in zip(at, sizes)], end


def _verify(gpu, table, datas, out, dst_cap, align, level, bs, seekable, checksum, dict_=None, huf=None, unsized=None):
    """every item against the host API and the model; unsized: {item index: error}. -> ({item: archive}, at, total)"""
    res, packed, total, dst = out
    unsized = unsized or {}
    want = [None if r in unsized else _host(gpu, d, level, bs, seekable, checksum, dict_, huf) for r, d in enumerate(datas)]
    at, written, want_total = _model([None if w is None else len(w) for w in want], align, dst_cap)
    assert total == want_total, (total, want_total)
    assert len(res) == len(table) == len(datas) == len(packed)
    keep = np.zeros(len(dst), dtype=bool)
    arcs = {}
    for r, row in enumerate(table):
        got = tuple(int(packed[r][k]) for k in ("src_off", "src_size", "dst_off", "dst_capacity"))
        given = (int(row["src_off"]), int(row["src_size"]))
        w = (r, len(datas[r]), align, level, bs, seekable, checksum, dst_cap)
        if not written[r]:
            assert res[r] == unsized.get(r, ERR["DST_TOO_SMALL"]) and got == (0, 0) + given, (w, res[r], got)
            continue
        assert res[r] == len(want[r]) and got == (at[r], len(want[r])) + given, (w, res[r], got, at[r], len(want[r]))
        arcs[r] = dst[at[r]: at[r] + res[r]].tobytes()  # found through d_packed
        assert arcs[r] == want[r], w
        keep[at[r]: at[r] + res[r]] = True
    assert not keep[dst_cap:].any()
    assert np.array_equal(dst[~keep], _pattern(len(dst))[~keep])  # gaps, tail, behind the capacity
    return arcs, at, total


area_4k = devtest.area_4k_fixture(Area, SIZES_4K, _payload)


def _enough(datas):
    return sum(len(d) + len(d) // 8 + 4096 for d in datas)  # above any total: archives, their containers, 4096 of padding each


@pytest.mark.parametrize("level", [3, 6])
def test_parity_with_the_host_api_and_the_batch_call(gpu, area_4k, level):
    area, src, table, datas = area_4k
    assert len(table) == 22 and (table["src_off"] % 2 == 1).any() and (table["src_off"] % 2 == 0).any()
    cap = _enough(datas)
    for seekable, checksum in ((0, 0), (1, 0), (0, 1), (1, 1)):
        out = _run(gpu, src, len(area.buf), table, max(SIZES_4K), cap, 16, level, 4096, seekable, checksum)
        arcs, at, total = _verify(gpu, table, datas, out, cap, 16, level, 4096, seekable, checksum)
        assert len(arcs) == 22 and total < cap
        if seekable and checksum:  # the sibling over the same table, which has destinations of zxc_compress_bound
            got, dst = _run_batch(gpu, src, len(area.buf), table, max(SIZES_4K), area.dst_at, level, 4096, seekable, checksum)
            for r, row in enumerate(table):
                d = int(row["dst_off"])
                assert got[r] == len(arcs[r]) and dst[d: d + got[r]].tobytes() == arcs[r], (r, level)
            assert total < area.dst_at
    assert bytes(src[: len(area.buf)].cpu().numpy()) == bytes(area.buf)  # d_src is never written


def test_larger_blocks(gpu):
    bs = 65536
    area = Area(gpu, bs)
    for k, size in enumerate((2 * bs + 777, bs + 1, 31, 2 * bs + 31)):
        area.add(_payload(size, (0, 2, 1, 3)[k]))
    src, table, cap = area.tensor(), area.table(), _enough(area.datas)
    out = _run(gpu, src, len(area.buf), table, 2 * bs + 777, cap, 256, 3, bs, 1, 1)
    assert len(_verify(gpu, table, area.datas, out, cap, 256, 3, bs, 1, 1)[0]) == 4


@pytest.mark.parametrize("align", [1, 16, 4096])
def test_layout(gpu, area_4k, align):
    area, src, table, datas = area_4k
    cap = _enough(datas)
    out = _run(gpu, src, len(area.buf), table, max(SIZES_4K), cap, align, 3, 4096, 1, 0, odd_dst=align == 1)
    arcs, at, total = _verify(gpu, table, datas, out, cap, align, 3, 4096, 1, 0)
    assert len(arcs) == 22 and at[0] == 0 and all(a % align == 0 for a in at)
    if align == 1:
        assert total == sum(len(a) for a in arcs.values())  # back to back
    else:
        assert any(at[r + 1] > at[r] + len(arcs[r]) for r in range(21))  # a gap somewhere


def _patch_unsized(table, datas, src_cap, max_size, where):
    """items without a size at `where`: above max_size (the data is that long), behind the source area, and wrapping 64 bits"""
    unsized = {}
    for k, r in enumerate(where):
        if k % 3 == 0:
            assert len(datas[r]) > max_size
            unsized[r] = ERR["OVERFLOW"]
        elif k % 3 == 1:
            table["src_off"][r] = src_cap - int(table["src_size"][r]) + 1
            unsized[r] = ERR["SRC_TOO_SMALL"]
        else:
            table["src_off"][r], table["src_size"][r] = M64 - 5, 100
            unsized[r] = ERR["SRC_TOO_SMALL"]
    return unsized


def test_many_items_cross_the_scan_tile(gpu):
    n, max_size, bs = 1100, 8192, 4096
    where = (0, 255, 256, 1023, 1024, 1099)
    kinds = [_payload(size, k) for k, size in enumerate((0, 1, 33, 700, 4095, 4096, 4097, 5000, 8191, 8192, 100, 2000))]
    big = _payload(max_size + 1, 2)
    area = Area(gpu, 91)
    for r in range(n):
        area.add(big if r in where[::3] else kinds[(r * 7 + r // 256) % len(kinds)])
    table, datas = area.table(), area.datas
    unsized = _patch_unsized(table, datas, len(area.buf), max_size, where)
    assert sorted(unsized) == list(where)
    cap = _enough(datas)
    for align in (1, 16, 4096):
        out = _run(gpu, area.tensor(), len(area.buf), table, max_size, cap, align, 3, bs, 1, 1, odd_dst=align == 1)
        arcs, at, total = _verify(gpu, table, datas, out, cap, align, 3, bs, 1, 1, unsized=unsized)
        assert len(arcs) == n - len(where) and at[1] == 0


def test_capacity(gpu, area_4k):
    area, src, table, datas = area_4k
    level, bs, seekable, checksum, align = 3, 4096, 1, 1, 16
    sizes = [len(_host(gpu, d, level, bs, seekable, checksum)) for d in datas]
    at, _, total = _model(sizes, align, 0)
    cut = at[11] + sizes[11] // 2  # in the middle of an archive
    seen = []
    for cap, no_dst in ((cut, False), (total, False), (0, True)):
        out = _run(gpu, src, len(area.buf), table, max(SIZES_4K), cap, align, level, bs, seekable, checksum, no_dst=no_dst)
        arcs, _, got_total = _verify(gpu, table, datas, out, cap, align, level, bs, seekable, checksum)
        assert sorted(arcs) == list(range({cut: 11, total: 22, 0: 0}[cap]))  # the prefix that fits
        assert out[0][len(arcs):] == [ERR["DST_TOO_SMALL"]] * (22 - len(arcs))
        assert np.array_equal(out[3][cap:], _pattern(len(out[3]))[cap:])  # no byte at or past the capacity
        seen.append(got_total)
    assert seen == [total] * 3


def test_round_trip_through_decompress_batch_device(gpu):
    """d_packed and the packed buffer go straight into decompress_batch_device, on one stream, and nothing is read back in
    between: the host knows neither a size nor an offset. The decoded arena has the layout of the source arena."""
    import torch
    bs, level, max_size = 4096, 3, 4 * 4096
    area = Area(gpu, 77)
    for k in range(64):
        area.add(_payload((k * 2039) % (4 * bs + 1) if k != 20 else max_size + 1, k))
    src, table = area.tensor(), area.table()
    n, src_cap, cap = len(table), len(area.buf), _enough(area.datas)
    res, packed, total, arc, work, d_items = _run(gpu, src, src_cap, table, max_size, cap, 64, level, bs, 1, 1, sync=False)
    out = torch.from_numpy(_pattern(src_cap + CANARY)[::-1].copy()).to("cuda")
    res2 = torch.full((n,), UNSET, dtype=torch.int64, device="cuda")
    ws = gpu.decompress_batch_device_work_size(n, max_size, bs)
    work2 = torch.empty(ws, dtype=torch.uint8, device="cuda")
    assert arc.numel() >= cap + 64  # readable behind the capacity
    gpu.decompress_batch_device(arc.data_ptr(), cap, packed.data_ptr(), n, max_size, out.data_ptr(), src_cap, bs, work2.data_ptr(), ws,
                                res2.data_ptr(), True, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    sizes, decoded, first = res2.cpu().numpy(), out.cpu().numpy(), res.cpu().numpy()
    keep = np.zeros(len(decoded), dtype=bool)
    for r, (row, data) in enumerate(zip(table, area.datas)):
        if r == 20:
            assert int(first[r]) == ERR["OVERFLOW"] and int(sizes[r]) == ERR["SRC_TOO_SMALL"]
            continue
        at = int(row["src_off"])
        assert int(first[r]) > 0 and int(sizes[r]) == len(data), (r, int(first[r]), int(sizes[r]), len(data))
        assert decoded[at: at + len(data)].tobytes() == data, r
        keep[at: at + len(data)] = True
    assert np.array_equal(decoded[~keep], _pattern(src_cap + CANARY)[::-1][~keep])  # the bytes between the items are untouched
    assert 0 < int(total.item()) <= cap


def test_in_place(gpu, area_4k):
    area, src, table, datas = area_4k
    table = table.copy()
    unsized = {3: ERR["SRC_TOO_SMALL"]}
    table["src_off"][3] = len(area.buf) + 1
    sizes = [None if r == 3 else len(_host(gpu, d, 3, 4096, 1, 1)) for r, d in enumerate(datas)]
    cap = _model(sizes, 16, 0)[2] - 1  # the last archive does not fit
    a = _run(gpu, src, len(area.buf), table, max(SIZES_4K), cap, 16, 3, 4096, 1, 1)
    b = _run(gpu, src, len(area.buf), table, max(SIZES_4K), cap, 16, 3, 4096, 1, 1, in_place=True)
    arcs, _, _ = _verify(gpu, table, datas, a, cap, 16, 3, 4096, 1, 1, unsized=unsized)
    assert len(arcs) == 20 and a[0][21] == ERR["DST_TOO_SMALL"]
    assert a[0] == b[0] and a[2] == b[2] and np.array_equal(a[3], b[3]) and a[1].tobytes() == b[1].tobytes()


def test_dictionary(gpu):
    import torch
    bs, level, seekable, checksum, align = 4096, 3, 1, 1, 16
    content, huf = load_dict(os.path.join(GOLDEN, "conformance", "valid", "dict_http.zxd"))
    area = Area(gpu, 9)
    for k, size in enumerate((0, 1, 700, 4095, 4096, 4097, 3 * 4096 + 5, 9000)):
        area.add((content[: size // 2] + _payload(size, k))[:size])  # some bytes the dictionary knows
    src, table, max_size = area.tensor(), area.table(), 3 * 4096 + 5
    n, src_cap, cap = len(table), len(area.buf), _enough(area.datas)
    d_content, d_huf = _to_dev(content), _to_dev(huf)
    d_id = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    gpu.dict_prepare_device(d_content.data_ptr(), len(content), d_huf.data_ptr(), d_id.data_ptr(), stream)
    dd = (d_content.data_ptr(), len(content), d_huf.data_ptr(), d_id.data_ptr())
    out = _run(gpu, src, src_cap, table, max_size, cap, align, level, bs, seekable, checksum, dd=dd)
    arcs, at, total = _verify(gpu, table, area.datas, out, cap, align, level, bs, seekable, checksum, dict_=content, huf=huf)
    assert len(arcs) == n and all(a[6] & 0x40 for a in arcs.values())  # the header's dictionary flag
    got, dst = _run_batch(gpu, src, src_cap, table, max_size, area.dst_at, level, bs, seekable, checksum, dd=dd)
    for r, row in enumerate(table):
        d = int(row["dst_off"])
        assert dst[d: d + got[r]].tobytes() == arcs[r], r
    # back through decompress_batch_dict_device, nothing read back in between
    res, packed, d_total, arc, work, d_items = _run(gpu, src, src_cap, table, max_size, cap, align, level, bs, seekable, checksum, dd=dd,
                                                     sync=False)
    back = torch.from_numpy(_pattern(src_cap + CANARY)[::-1].copy()).to("cuda")
    res2 = torch.full((n,), UNSET, dtype=torch.int64, device="cuda")
    ws = gpu.decompress_batch_device_work_size(n, max_size, bs)
    work2 = torch.empty(ws, dtype=torch.uint8, device="cuda")
    gpu.decompress_batch_dict_device(arc.data_ptr(), cap, packed.data_ptr(), n, max_size, back.data_ptr(), src_cap, bs, dd, work2.data_ptr(),
                                     ws, res2.data_ptr(), True, stream)
    torch.cuda.synchronize()
    decoded = back.cpu().numpy()
    for r, (row, data) in enumerate(zip(table, area.datas)):
        o = int(row["src_off"])
        assert int(res2[r].item()) == len(data) and decoded[o: o + len(data)].tobytes() == data, r
    # a NULL dict, and one of size 0, is the plain call
    plain = _run(gpu, src, src_cap, table, max_size, cap, align, level, bs, seekable, checksum)
    _verify(gpu, table, area.datas, plain, cap, align, level, bs, seekable, checksum)
    for none in (None, (0, 0, 0, 0)):
        same = _run(gpu, src, src_cap, table, max_size, cap, align, level, bs, seekable, checksum, dd=none)
        assert same[0] == plain[0] and same[2] == plain[2] and np.array_equal(same[3], plain[3]) and same[1].tobytes() == plain[1].tobytes()


def test_item_table_written_on_the_stream_and_two_streams_at_once(gpu):
    import torch
    import zxc_amd
    bs, n = 4096, 400
    area = Area(gpu, 12)
    kinds = [_payload(1 + (k * 1531) % (3 * bs), k) for k in range(20)]
    for k in range(n):
        area.add(kinds[(k * 3) % 20])
    src, cap = area.tensor(), _enough(area.datas)
    runs = []
    for s_i, s in enumerate((torch.cuda.Stream(), torch.cuda.Stream())):
        order = list(range(n))
        random.Random(70 + s_i).shuffle(order)
        table, datas = area.table(order), [area.datas[k] for k in order]
        good = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
        d_items = torch.zeros_like(good)  # every item an empty source (an archive of 36 bytes) until the copy below has run
        runs.append((s, table, datas, good, d_items))
    torch.cuda.synchronize()
    out = []
    for s, table, datas, good, d_items in runs:  # both enqueued before either is waited for
        with torch.cuda.stream(s):
            d_items.copy_(good, non_blocking=True)  # the operation that writes d_items, on the call's stream, nothing waited for
            out.append(_run(gpu, src, len(area.buf), table, 3 * bs, cap, 16, 3, bs, 1, 1, stream=s, sync=False, d_items=d_items))
    for (s, table, datas, good, d_items), (res, packed, total, dst, work, _) in zip(runs, out):
        s.synchronize()
        got = ([int(x) for x in res.cpu().numpy()[:n]], packed.cpu().numpy()[: 32 * n].view(zxc_amd.ITEM_DTYPE), int(total.item()),
               dst.cpu().numpy())
        assert len(_verify(gpu, table, datas, got, cap, 16, 3, bs, 1, 1)[0]) == n
    assert bytes(src[: len(area.buf)].cpu().numpy()) == bytes(area.buf)  # d_src unchanged
