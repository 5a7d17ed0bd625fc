"""What the GPU tests of compress_batch_device and compress_pack_device share: the sizes, the payloads, the source and destination
areas, one batch call, and the host API's archive of an item. A plain module next to the tests, imported the way devtest is."""
import random

import numpy as np

import devtest
from devtest import CANARY, PAD, UNSET, bound, pattern, to_dev

SIZES_4K = (0, 1, 31, 32, 33, 4095, 4096, 4097, 8192, 3 * 4096 + 5, 16 * 4096)


def payload(n, seed):
    """a slice of one generated text, or bytes that do not compress (stored blocks) for every fourth seed"""
    return devtest.payload(n, seed, stored_every=4, text_size=1 << 20)


class Area:
    """the source area: buffers at odd offsets with unrelated bytes between them; the destination area: one place per buffer,
    16-aligned and odd in turn, with gaps"""

    def __init__(self, gpu, seed):
        self.gpu, self.rng, self.buf, self.rows, self.datas, self.dst_at = gpu, random.Random(seed), bytearray(), [], [], 0

    def add(self, data, cap=None, src_size=None):
        self.buf += bytes(self.rng.randrange(256) for _ in range(1 + self.rng.randrange(47)))
        if (len(self.buf) & 1) == (len(self.rows) & 1):  # odd and even source offsets in turn
            self.buf += b"\x5a"
        cap = bound(self.gpu, len(data)) if cap is None else cap
        at = (self.dst_at + 15) // 16 * 16 + 16 * self.rng.randrange(3)
        d = at if len(self.rows) % 2 == 0 else at + 1 + self.rng.randrange(15)
        self.rows.append((len(self.buf), len(data) if src_size is None else src_size, d, cap))
        self.datas.append(data)
        self.buf += data
        self.dst_at = d + cap
        return len(self.rows) - 1

    def table(self, order=None):
        import zxc_amd
        order = range(len(self.rows)) if order is None else order
        t = np.zeros(len(self.rows), dtype=zxc_amd.ITEM_DTYPE)
        for i, k in enumerate(order):
            t[i] = self.rows[k]
        return t

    def tensor(self):
        return to_dev(bytes(self.buf), PAD)


def run(gpu, src, src_cap, table, max_size, dst_cap, level, bs, seekable, checksum, dd=None, stream=None, sync=True, d_items=None):
    """one compress_batch_device (or _dict_device) call -> (results as a list, dst as numpy of dst_cap + CANARY bytes); dst starts
    as the pattern everywhere"""
    import torch
    s = torch.cuda.current_stream() if stream is None else stream
    n = len(table)
    ws = gpu.compress_batch_device_work_size(n, max_size, level, bs, seekable, checksum, dict_size=dd[1] if dd else 0)
    assert ws > 0
    with torch.cuda.stream(s):
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        dst = torch.from_numpy(pattern(dst_cap + CANARY)).to("cuda")
        res = torch.full((max(n, 1),), UNSET, dtype=torch.int64, device="cuda")
        if d_items is None:
            d_items = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
        args = (src.data_ptr(), src_cap, d_items.data_ptr(), n, max_size, dst.data_ptr(), dst_cap)
        if dd is None:
            gpu.compress_batch_device(*args, work.data_ptr(), ws, res.data_ptr(), level, bs, seekable, checksum, s.cuda_stream)
        else:
            gpu.compress_batch_dict_device(*args, dd, work.data_ptr(), ws, res.data_ptr(), level, bs, seekable, checksum, s.cuda_stream)
    if not sync:
        return res, dst, work, d_items
    s.synchronize()
    return [int(x) for x in res.cpu().numpy()[:n]], dst.cpu().numpy()


_HOST = {}


def host(gpu, data, level, bs, seekable, checksum, dict_=None, huf=None):
    """zxc_amd.compress of the same bytes and options, once per (bytes, options)"""
    key = (data, level, bs, seekable, checksum, dict_ is not None and len(dict_))
    if key not in _HOST:
        _HOST[key] = gpu.compress(data, level, bs, bool(seekable), bool(checksum), dict_=dict_, dict_huf=huf)
    return _HOST[key]
