"""The block encoder at its format and table limits, on the device, against the CPU wave emulator: for every case of
tests/encode_limit_cases.py and every level, the archive must have the size and SHA-256 that the emulator's run of the same
kernel source recorded in tests/golden/encoder_limits/digests.json -- through the host zxc_compress, through compress_device, and
(job-table case) through compress_batch_device, whose items must each equal zxc_compress of the item. Plain byte equality, no
tolerance: a stale chain link, a head entry that lost a collision or a byte read before it landed gives a block that still
decodes and is only a little larger, which no round trip and no ratio bound notices.

Device sources lie in the middle of a larger tensor (4096 guard bytes on each side: the kernel reads up to 32 bytes past a
block's end and clamps lengths afterwards) and every compress_device case runs twice with different guard contents: identical
archives, guards unchanged. Every archive also round-trips through the unmodified reference decoder. Reads the digests and
oracle/_ref only; builds nothing."""
import ctypes as C
import hashlib
import json
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import devtest  # noqa: E402
import encode_limit_cases as E  # noqa: E402
import zxc_block_model as M  # noqa: E402
from devtest import UNSET, bound as _bound  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4096

gpu = devtest.gpu_fixture()


@pytest.fixture(scope="module")
def digests():
    return json.load(open(os.path.join(ROOT, E.DIGESTS)))


def _guarded(data, fill):
    """-> (tensor [guard | data | guard], the guard pattern)"""
    import torch
    g = torch.arange(GUARD, dtype=torch.int32).mul(fill).remainder(253).to(torch.uint8)
    t = torch.cat([g, torch.frombuffer(bytearray(data), dtype=torch.uint8), g.flip(0)]) if data else torch.cat([g, g.flip(0)])
    return t.to("cuda"), g


def _explain(what, got, want):
    """the first block that differs from the emulator's record, with the header fields of both sides"""
    blocks = [b + (t or b"") for a in got for b, t in zip(*M.split_blocks(a)[2:4])]
    lines = ["%s: size %d, recorded %d" % (what, sum(len(a) for a in got), want["size"])]
    for i, (b, w) in enumerate(zip(blocks, want["blocks"])):
        mine = [len(b), hashlib.sha256(b).hexdigest()[:8]] + E.block_fields(b)
        if mine != w:
            lines.append("first differing block: %d of %d (fields: bytes, sha256[:8], %s)" % (i, len(blocks), ", ".join(E.FIELDS)))
            lines.append("  device:   %s" % mine)
            lines.append("  emulator: %s" % w)
            try:
                p = M.parse_block(b[:8 + int.from_bytes(b[3:7], "little")])
                if p["seqs"]:
                    lines.append("  device sequences (first 12): %s, extras %s bytes, pad %s" % (p["seqs"][:12], p["ext_sec"], p["pad"]))
            except Exception as e:
                lines.append("  the device's block does not parse: %r" % (e,))
            break
    else:
        lines.append("blocks: device %d, emulator %d" % (len(blocks), len(want["blocks"])))
    return "\n".join(lines)


def _check(what, arcs, want):
    got = (sum(len(a) for a in arcs), hashlib.sha256(b"".join(arcs)).hexdigest())
    if got != (want["size"], want["sha256"]):
        msg = _explain(what, arcs, want)
        print(msg)
        raise AssertionError(msg)


def _ref_roundtrip(ref, arc, data, checksum, dict_):
    import oracle_py
    o = oracle_py.DecompressOpts(checksum_enabled=int(checksum))
    keep = None
    if dict_:
        keep = C.create_string_buffer(dict_, len(dict_))
        o.dict, o.dict_size = C.cast(keep, C.c_void_p), len(dict_)
    out = C.create_string_buffer(max(len(data), 1))
    rc = ref.lib.zxc_decompress(arc, len(arc), out if data else None, len(data), C.byref(o))
    assert rc == len(data) and out.raw[:rc] == data, ("reference decoder", rc, len(data))


def _compress_device(gpu, data, level, bs, checksum, fill, dd=None):
    """compress_device (with dd = (tensor, size): compress_dict_device) of data inside guards -> archive bytes"""
    import torch
    src, g = _guarded(data, fill)
    n, cap = len(data), _bound(gpu, len(data))
    ws = gpu.compress_dict_device_work_size(n, dd[1], level, bs, True, checksum) if dd else gpu.compress_device_work_size(n, level, bs, True, checksum)
    assert ws > 0
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
    res = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream()
    if dd:
        d_id = torch.zeros(1, dtype=torch.int32, device="cuda")
        gpu.dict_prepare_device(dd[0].data_ptr(), dd[1], 0, d_id.data_ptr(), s.cuda_stream)
        gpu.compress_dict_device(src.data_ptr() + GUARD, n, dst.data_ptr(), cap, (dd[0].data_ptr(), dd[1], 0, d_id.data_ptr()),
                                 work.data_ptr(), ws, res.data_ptr(), level, bs, True, checksum, s.cuda_stream)
    else:
        gpu.compress_device(src.data_ptr() + GUARD, n, dst.data_ptr(), cap, work.data_ptr(), ws, res.data_ptr(), level, bs, True,
                            checksum, s.cuda_stream)
    s.synchronize()
    rc = int(res.item())
    assert rc > 0, rc
    back = src.cpu()
    assert torch.equal(back[:GUARD], g) and torch.equal(back[GUARD + n:], g.flip(0)), "guard bytes around the source changed"
    assert bytes(back[GUARD:GUARD + n].numpy()) == data, "the source changed"
    return bytes(dst[:rc].cpu().numpy())


def _batch(gpu, items, level, bs, checksum):
    """compress_batch_device of the items, packed with odd gaps inside guards -> [archive bytes]"""
    import numpy as np
    import torch
    import zxc_amd
    buf, rows, at = bytearray(b"\x5a" * GUARD), [], 0
    for i, it in enumerate(items):
        buf += b"\xc3" * (1 + i % 3)
        cap = _bound(gpu, len(it))
        rows.append((len(buf), len(it), at, cap))
        buf += it
        at += cap + 16 + i
    buf += b"\x5a" * GUARD
    table = np.zeros(len(rows), dtype=zxc_amd.ITEM_DTYPE)
    for i, r in enumerate(rows):
        table[i] = r
    src = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to("cuda")
    max_size = max(len(it) for it in items)
    ws = gpu.compress_batch_device_work_size(len(items), max_size, level, bs, True, checksum)
    assert ws > 0
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(at + 64, dtype=torch.uint8, device="cuda")
    res = torch.full((len(items),), UNSET, dtype=torch.int64, device="cuda")
    d_items = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
    s = torch.cuda.current_stream()
    gpu.compress_batch_device(src.data_ptr(), len(buf) - 64, d_items.data_ptr(), len(items), max_size, dst.data_ptr(), at + 64, work.data_ptr(),
                              ws, res.data_ptr(), level, bs, True, checksum, s.cuda_stream)
    s.synchronize()
    rcs = [int(x) for x in res.cpu().numpy()]
    assert all(rc > 0 for rc in rcs), rcs
    out = dst.cpu().numpy()
    assert bytes(src.cpu().numpy()) == bytes(buf), "the source area changed"
    return [bytes(out[r[2]:r[2] + rc]) for r, rc in zip(rows, rcs)]


@pytest.mark.parametrize("case", E.cases(), ids=lambda c: c.name)
def test_device_archives_equal_the_emulators(gpu, ref, digests, case):
    import torch
    dd = None
    if case.dict_:
        dd = (torch.frombuffer(bytearray(case.dict_ + bytes(64)), dtype=torch.uint8).to("cuda"), len(case.dict_))
    for level, checksum in E.variants(case):
        k = E.key(case, level, checksum)
        want = digests[k]
        host = [gpu.compress(p, level, case.bs, True, checksum, dict_=case.dict_) for p in E.pieces(case)]
        _check("zxc_compress, " + k, host, want)
        for p, a in zip(E.pieces(case), host):
            _ref_roundtrip(ref, a, p, checksum, case.dict_)
        if case.items:
            got = _batch(gpu, case.items, level, case.bs, checksum)
            for i, (a, h) in enumerate(zip(got, host)):
                assert a == h, "compress_batch_device item %d (%d bytes) differs from zxc_compress of the item, %s" % (i, len(case.items[i]), k)
            _check("compress_batch_device, " + k, got, want)
        one = [_compress_device(gpu, p, level, case.bs, checksum, 7, dd) for p in E.pieces(case)]
        two = [_compress_device(gpu, p, level, case.bs, checksum, 131, dd) for p in E.pieces(case)]
        assert one == two, "compress_device: the archive depends on the bytes around the source, " + k
        _check("compress_device, " + k, one, want)


def test_digests_cover_exactly_the_cases(digests):
    assert set(digests) == {E.key(c, lv, ck) for c in E.cases() for lv, ck in E.variants(c)}
