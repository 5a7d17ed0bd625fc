"""zxc_mi355x_decompress_batch_device on the GPU: many archives that lie in one device buffer decoded into another by one call, every
result equal to what this library's zxc_decompress returns for a host copy of the same bytes, capacity and options, every decoded
item's bytes equal to the source's, and a pattern intact everywhere outside the items' own destinations. Archives from zxc_compress,
from compress_device (decoded where they lie) and from the unmodified reference; truncated and damaged ones; every block size;
more items than a plan workgroup has threads; a shared dictionary; two streams; stream order behind the operation that wrote the item
table. Nothing here provokes a fault: the damaged inputs are of the kinds the host path and the sibling calls are tested with, and
the kernels refuse them by status."""
import os
import random

import numpy as np
import pytest

import devtest
from conftest import GOLDEN, load_dict
from devtest import CANARY, ERR, PAD, UNSET, device_written as _device_written, pattern as _pattern, to_dev as _to_dev

pytestmark = pytest.mark.gpu

SIZES_4K = (0, 1, 4095, 4096, 4097, 8192, 3 * 4096 + 5, 16 * 4096)
LEVELS = (1, 3, 6, 7)


gpu = devtest.gpu_fixture("decompress_batch_device")


def _payload(n, seed):
    """a slice of one generated text, or bytes that do not compress (stored blocks) for every fourth seed"""
    return devtest.payload(n, seed, stored_every=4, text_size=lambda n: 1 << 20 if n <= (1 << 19) else 7 << 20)


class Entry:
    """one archive of the source area: where it lies, its bytes (the host copy the oracle reads), the source it was made from
    (None for a damaged one, whose decoded bytes are the host's)"""

    def __init__(self, comp, data, what, size):
        self.comp, self.data, self.what, self.size, self.off, self.other_bs = comp, data, what, size, None, False


class Area:
    """the source area: archives at odd offsets with unrelated bytes between them"""

    def __init__(self, seed):
        self.rng, self.buf, self.entries = random.Random(seed), bytearray(), []

    def add(self, comp, data, what, size=None):
        e = Entry(comp, data, what, len(data) if size is None else size)
        self.buf += bytes(self.rng.randrange(256) for _ in range(self.rng.randrange(1, 48)))
        e.off = len(self.buf)
        self.buf += comp
        self.entries.append(e)
        return e

    def tensor(self):
        return _to_dev(bytes(self.buf), PAD)


def _place(entries, caps_of, rng, shuffle=True):
    """an item per (entry, capacity kind), destinations 16-aligned and odd in turn, with gaps.
    -> (table, [entry per item], max_capacity, dst_capacity)"""
    rows, who, at, k = [], [], 0, 0
    for e in entries:
        for cap in caps_of(e):
            at = (at + 15) // 16 * 16 + 16 * rng.randrange(3)
            d = at if k % 2 == 0 else at + 1 + rng.randrange(15)
            rows.append((e.off, len(e.comp), d, cap))
            who.append(e)
            at, k = d + cap, k + 1
    order = list(range(len(rows)))
    if shuffle:
        rng.shuffle(order)
    return _table([rows[i] for i in order]), [who[i] for i in order], max(r[3] for r in rows), at + 64


def _table(rows):
    import zxc_amd
    t = np.zeros(len(rows), dtype=zxc_amd.ITEM_DTYPE)
    for i, r in enumerate(rows):
        t[i] = r
    return t


def _run(gpu, src, src_cap, table, max_cap, dst_cap, bs, checksum, dd=None, stream=None, sync=True, d_items=None):
    """-> (results as a list, dst as numpy of dst_cap + CANARY bytes); dst starts as the pattern everywhere"""
    import torch
    s = torch.cuda.current_stream() if stream is None else stream
    n = len(table)
    ws = gpu.decompress_batch_device_work_size(n, max_cap, bs)
    assert ws > 0
    with torch.cuda.stream(s):
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        dst = torch.from_numpy(_pattern(dst_cap + CANARY)).to("cuda")
        res = torch.full((max(n, 1),), UNSET, dtype=torch.int64, device="cuda")
        if d_items is None:
            d_items = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
        args = (src.data_ptr(), src_cap, d_items.data_ptr(), n, max_cap, dst.data_ptr(), dst_cap, bs)
        if dd is None:
            gpu.decompress_batch_device(*args, work.data_ptr(), ws, res.data_ptr(), checksum, s.cuda_stream)
        else:
            gpu.decompress_batch_dict_device(*args, dd, work.data_ptr(), ws, res.data_ptr(), checksum, s.cuda_stream)
    if not sync:
        return res, dst, work, d_items
    s.synchronize()
    return [int(x) for x in res.cpu().numpy()[:n]], dst.cpu().numpy()


def _cap_of(row, max_cap, dst_cap):
    d, c = int(row["dst_off"]), int(row["dst_capacity"])
    return 0 if d > dst_cap else min(c, max_cap, dst_cap - d)


def _verify(gpu, table, who, got, dst, max_cap, dst_cap, bs, checksum, dict_=None, huf=None):
    """every item against zxc_decompress on its host copy; -> {result: count}. No item is left out."""
    keep = np.zeros(len(dst), dtype=bool)
    seen, memo = {}, {}
    for r, (row, e, rc) in enumerate(zip(table, who, got)):
        cap, d = _cap_of(row, max_cap, dst_cap), int(row["dst_off"])
        key = (id(e), cap)
        if key not in memo:
            memo[key] = gpu.decompress(e.comp, cap, checksum, False, dict_=dict_, dict_huf=huf)
        want, host = memo[key]
        if e.other_bs and cap > 0:
            want = ERR["BAD_BLOCK_SIZE"]  # the departure: this archive's header block size is not the argument's
        w = (e.what, r, cap, d)
        assert rc == want, (w, rc, want)
        if rc >= 0:
            assert dst[d: d + rc].tobytes() == host, w
            if e.data is not None:
                assert host == e.data[:rc] and rc == len(e.data), w
        keep[d: d + cap] = True
        seen[rc if rc < 0 else "ok"] = seen.get(rc if rc < 0 else "ok", 0) + 1
    assert sum(seen.values()) == len(table) == len(got)
    assert np.array_equal(dst[~keep], _pattern(len(dst))[~keep])  # gaps, other items, behind the capacity
    return seen


def _first_block(comp):
    """-> (payload offset, payload size) of the first block, or None when the archive has none"""
    if comp[16] == 255:
        return None
    return 24, int.from_bytes(comp[19:23], "little")


def _mutants(comp, checksum):
    """three truncations, one payload byte, one trailer byte -> (what, bytes)"""
    n = len(comp)
    for cut in (n - 1, n // 2, 20):
        yield f"cut {cut}", comp[:cut]
    blk = _first_block(comp)
    if blk and blk[1] > 0:
        b = bytearray(comp)
        b[blk[0] + min(blk[1] - 1, 3 + blk[1] // 3)] ^= 0x5A
        yield "payload", bytes(b)
        if checksum:
            b = bytearray(comp)
            b[blk[0] + blk[1] + 1] ^= 0x01
            yield "trailer", bytes(b)


@pytest.fixture(scope="module")
def mixed(gpu, ref):
    """the mixed batch of block size 4096: -> (area, device tensor, entries written on the device, trailer mutants)"""
    import torch
    area, dev_written, trailer = Area(41), [], []
    k = 0
    for size in SIZES_4K:
        for level in LEVELS:
            checksum, seekable, writer = bool(k & 1), bool((k >> 1) & 1), ("zxc_compress", "compress_device", "reference")[k % 3]
            data = _payload(size, k)
            what = (writer, size, level, checksum, seekable)
            if writer == "zxc_compress":
                comp = gpu.compress(data, level, 4096, seekable, checksum)
            elif writer == "reference":
                comp = ref.compress(data, level, 4096, seekable, checksum)
            else:
                t = _device_written(gpu, data, level, 4096, seekable, checksum)
                comp = bytes(t.cpu().numpy())
                dev_written.append((len(area.entries), t))
            area.add(comp, data, what)
            for m, bad in _mutants(comp, checksum):
                e = area.add(bad, None, what + (m,), size)
                if m == "trailer":
                    trailer.append(e)
            k += 1
    data = _payload(70000, 5)
    area.add(gpu.compress(data, 3, 65536, True, False), data, ("block size 65536",)).other_bs = True
    src = area.tensor()
    for i, t in dev_written:  # the archives compress_device wrote are copied device to device: they never visit the host
        e = area.entries[i]
        src[e.off: e.off + len(e.comp)] = t
    torch.cuda.synchronize()
    assert len(trailer) >= 8 and len(dev_written) >= 8
    return area, src, trailer


def _mixed_caps(entries):
    """valid archives: two of the capacity kinds exact, exact - 1, exact + 31, exact + 32, 0 in turn; damaged ones: the size of
    the archive they were made from (at least 1); the archive of another block size: exact and exact + 32"""
    turn = {id(e): i for i, e in enumerate(e for e in entries if e.data is not None)}

    def caps(e):
        if e.data is None:
            return (max(e.size, 1),)
        n = e.size
        if e.other_bs:
            return (n, n + 32)
        kinds = (n, max(n - 1, 0), n + 31, n + 32, 0)
        return (kinds[2 * turn[id(e)] % 5], kinds[(2 * turn[id(e)] + 1) % 5])
    return caps


@pytest.mark.parametrize("checksum", [True, False])
def test_mixed_batch_of_4k_blocks(gpu, mixed, checksum):
    """tests 1 and 2 of the issue: one call over every kind of archive, with and without verification"""
    area, src, trailer = mixed
    table, who, max_cap, dst_cap = _place(area.entries, _mixed_caps(area.entries), random.Random(3))
    assert 180 <= len(table) <= 320 and max_cap >= 16 * 4096 + 32
    got, dst = _run(gpu, src, len(area.buf), table, max_cap, dst_cap, 4096, checksum)
    seen = _verify(gpu, table, who, got, dst, max_cap, dst_cap, 4096, checksum)
    print(len(table), seen)
    assert seen["ok"] >= 50 and seen.get(ERR["BAD_BLOCK_SIZE"]) == 2 and seen.get(ERR["DST_TOO_SMALL"], 0) >= 10
    assert seen.get(ERR["SRC_TOO_SMALL"], 0) >= 30
    by_entry = {id(e): rc for e, rc in zip(who, got)}
    for e in trailer:  # a changed trailer fails only when it is looked at
        assert by_entry[id(e)] == (ERR["BAD_CHECKSUM"] if checksum else int.from_bytes(e.comp[-12:-4], "little")), e.what
    assert bytes(src[: len(area.buf)].cpu().numpy()) == bytes(area.buf)  # d_src is never written


@pytest.mark.parametrize("bs", [65536, 1 << 21])
def test_larger_blocks(gpu, bs):
    rng = random.Random(bs)
    area = Area(bs)
    sizes = [1, 100, bs // 3, bs - 1, bs, bs + 1, 2 * bs + 5, 3 * bs, 4097, bs // 2 + 7, 31, bs - 33]
    for k, size in enumerate(sizes):
        data = _payload(size, k)
        checksum, seekable = bool(k & 1), bool(k & 2)
        area.add(gpu.compress(data, LEVELS[k % 4], bs, seekable, checksum), data, (size, checksum, seekable))
    assert sum(len(e.data) > bs for e in area.entries) >= 2
    src = area.tensor()
    table, who, max_cap, dst_cap = _place(area.entries, lambda e: (len(e.data) + (32 if len(e.data) % 3 else 0),), rng)
    for checksum in (True, False):
        got, dst = _run(gpu, src, len(area.buf), table, max_cap, dst_cap, bs, checksum)
        seen = _verify(gpu, table, who, got, dst, max_cap, dst_cap, bs, checksum)
        assert seen == {"ok": len(sizes)}, seen


def test_five_thousand_one_block_items(gpu):
    """more items than one plan workgroup has threads; the table is shuffled, so neither offset column is monotone"""
    n, bs = 5000, 4096
    area = Area(5)
    for k in range(48):
        data = _payload(1 + (k * 977) % 4096, k)
        area.add(gpu.compress(data, LEVELS[k % 4], bs, bool(k & 2), bool(k & 1)), data, k)
    src = area.tensor()
    rng = random.Random(50)
    picks = [area.entries[rng.randrange(48)] for _ in range(n)]
    rows, at = [], 0
    for i, e in enumerate(picks):
        d = at + (0 if i % 2 == 0 else 1 + i % 15)
        rows.append((e.off, len(e.comp), d, len(e.data)))
        at = (d + len(e.data) + 15) // 16 * 16
    order = list(range(n))
    rng.shuffle(order)
    table, who = _table([rows[i] for i in order]), [picks[i] for i in order]
    assert (np.diff(table["src_off"].astype(np.int64)) < 0).any() and (np.diff(table["dst_off"].astype(np.int64)) < 0).any()
    got, dst = _run(gpu, src, len(area.buf), table, bs, at, bs, True)
    seen = _verify(gpu, table, who, got, dst, bs, at, bs, True)
    assert seen == {"ok": n}, seen


def test_dictionary_batch(gpu):
    import torch
    bs = 4096
    content, huf = load_dict(os.path.join(GOLDEN, "conformance", "valid", "dict_http.zxd"))
    other, _ = load_dict(os.path.join(GOLDEN, "conformance", "valid", "dict_text.zxd"))
    area = Area(9)
    for k, size in enumerate((1, 700, 4095, 4096, 4097, 3 * 4096 + 5, 9000, 2 * 4096)):
        data = (content[: size // 2] + _payload(size, k))[:size]  # some bytes the dictionary knows
        area.add(gpu.compress(data, LEVELS[k % 4], bs, bool(k & 2), bool(k & 1), dict_=content, dict_huf=huf), data, ("dict", size))
    n_dict = len(area.entries)
    data = _payload(5000, 1)
    wrong = area.add(gpu.compress(data, 3, bs, True, False, dict_=other), data, ("another dictionary",))
    plain = area.add(gpu.compress(data, 3, bs, True, True), data, ("no dictionary",))
    src = area.tensor()
    d_content, d_huf = _to_dev(content), _to_dev(huf)
    d_id = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    gpu.dict_prepare_device(d_content.data_ptr(), len(content), d_huf.data_ptr(), d_id.data_ptr(), torch.cuda.current_stream().cuda_stream)
    dd = (d_content.data_ptr(), len(content), d_huf.data_ptr(), d_id.data_ptr())
    table, who, max_cap, dst_cap = _place(area.entries, lambda e: (len(e.data), len(e.data) + 32), random.Random(6))
    for checksum in (True, False):
        got, dst = _run(gpu, src, len(area.buf), table, max_cap, dst_cap, bs, checksum, dd=dd)
        seen = _verify(gpu, table, who, got, dst, max_cap, dst_cap, bs, checksum, dict_=content, huf=huf)
        assert seen == {"ok": 2 * n_dict + 2, ERR["DICT_MISMATCH"]: 2}, seen
        # the call that takes no dictionary: the dictionary items are refused and their bytes stay as they were
        got, dst = _run(gpu, src, len(area.buf), table, max_cap, dst_cap, bs, checksum)
        keep = np.zeros(len(dst), dtype=bool)
        for row, e, rc in zip(table, who, got):
            d = int(row["dst_off"])
            if e is plain:
                assert rc == len(e.data) and dst[d: d + rc].tobytes() == e.data
                keep[d: d + rc] = True
            else:
                assert rc == ERR["DICT_REQUIRED"] == gpu.decompress(e.comp, len(e.data), checksum, False)[0], e.what
        assert np.array_equal(dst[~keep], _pattern(len(dst))[~keep])
    assert wrong in who


def test_item_table_written_on_the_stream_and_two_streams_at_once(gpu):
    import torch
    bs, n = 4096, 1500
    area = Area(12)
    for k in range(32):
        data = _payload(1 + (k * 1531) % (3 * bs), k)
        area.add(gpu.compress(data, LEVELS[k % 4], bs, bool(k & 1), bool(k & 2)), data, k)
    src = area.tensor()
    torch.cuda.synchronize()
    runs = []
    for s_i, s in enumerate((torch.cuda.Stream(), torch.cuda.Stream())):
        rng = random.Random(70 + s_i)
        picks = [area.entries[rng.randrange(32)] for _ in range(n)]
        table, who, max_cap, dst_cap = _place(picks, lambda e: (len(e.data) + 32 * (len(e.data) & 1),), rng)
        good = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
        d_items = torch.zeros_like(good)  # every item empty (SRC_TOO_SMALL) until the copy below has run
        runs.append((s, table, who, max_cap, dst_cap, good, d_items))
    torch.cuda.synchronize()
    out = []
    for s, table, who, max_cap, dst_cap, good, d_items in runs:  # both enqueued before either is waited for
        with torch.cuda.stream(s):
            d_items.copy_(good, non_blocking=True)  # the operation that writes d_items, on the call's stream, nothing waited for
            out.append(_run(gpu, src, len(area.buf), table, max_cap, dst_cap, bs, True, stream=s, sync=False, d_items=d_items))
    for (s, table, who, max_cap, dst_cap, good, d_items), (res, dst, work, _) in zip(runs, out):
        s.synchronize()
        got = [int(x) for x in res.cpu().numpy()[:n]]
        seen = _verify(gpu, table, who, got, dst.cpu().numpy(), max_cap, dst_cap, bs, True)
        assert seen == {"ok": n}, seen
    assert bytes(src[: len(area.buf)].cpu().numpy()) == bytes(area.buf)  # d_src unchanged
