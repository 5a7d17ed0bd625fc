"""The shufflev calls of include/zxc_mi355x_shufflev.h on the GPU, at block size 4096 unless a case says otherwise: shufflev_device
against numpy's shuffle of the concatenation over the cut lists of the CPU replay, compress_shufflev_device byte for byte and word
for word against compress_shuffle_device of the concatenation run in the same test, the capacity, tables the scan refuses, two
streams, and the round trip the calls exist for: a state dict written with shufflev and read back tensor by tensor with
decompress_rangesv_shuffle_device at offset = starts[r].

The entries are dev_append.Table's: each a tensor of its own at an odd offset of a buffer that ends with it; destination, work area
and scratch lie at odd addresses between canaries. Nothing here provokes a fault: every table, the refused ones included, names
only buffers that exist (a zero base apart, which the scan refuses before any kernel looks at an entry), and refused tables are
refused by status."""
import random

import numpy as np
import pytest

import dev_append
import devtest
import rangesv_shuffle_support as rs
import shuffle_support as ss
import shufflev_support as sv
from devtest import ERR, bound
from shuffle_support import BS

pytestmark = pytest.mark.gpu
gpu = devtest.gpu_fixture(needs="compress_shufflev_device")

TOTAL = 9 * 4096 + 1000
DST_OFFS = (0, 1, 15)


def _x(n, E):
    return ss.tensor_bytes(n, E, seed=77 * E + n)


def _np(b):
    return np.frombuffer(b, dtype=np.uint8)


def _shuffled(x, E, unit=BS):
    return ss.np_shuffle(_np(x), E, unit).tobytes()


# ---------------------------------------------------------------- the kernel call
@pytest.mark.parametrize("E", sv.ELEMS)
def test_kernel_call_equals_numpy_over_the_cuts(gpu, E):
    k = 0
    for name, lens in sv.cuts(TOTAL, E).items():
        if name == "1 to 7 bytes":
            lens = sv.cuts(2 * 4096 + 3 * E + 1, E)[name]              # (some 2000 entries: a tensor each)
        x = _x(sum(lens), E)
        rc, got = sv.ShuffleV(gpu, dev_append.cut(x, lens), E, dst_off=DST_OFFS[k % 3], k0=k).result()
        assert rc == 0 and got == _shuffled(x, E), (name, E)
        k += 1
    x = _x(sv.ORDERS_TOTAL, E)
    for name, lens in dev_append.orders().items():
        rc, got = sv.ShuffleV(gpu, dev_append.cut(x, lens), E, dst_off=DST_OFFS[k % 3], k0=k).result()
        assert rc == 0 and got == _shuffled(x, E), (name, E)
        k += 1
    for n in ss.sizes(E):                                             # where a path of the plan begins or ends
        x = _x(n, E)
        rc, got = sv.ShuffleV(gpu, dev_append.cut(x, sv.cuts(n, E)["16 E + 1"]), E, dst_off=DST_OFFS[k % 3], k0=k).result()
        assert rc == 0 and got == _shuffled(x, E), (n, E)
        k += 1


def test_kernel_call_with_nothing_and_with_a_larger_unit(gpu):
    assert sv.ShuffleV(gpu, [], 4).result() == (0, b"")               # the store of the status alone
    assert sv.ShuffleV(gpu, [b"", b"", b""], 2).result() == (0, b"")
    E, unit = 4, 65536                                                 # the plane stride is another, the plan is the same
    n = 2 * unit + 17 * E + 3
    x = _x(n, E)
    lens = [unit - 5, 10, 0, unit + 1, 16 * E + 1, n - (2 * unit + 6 + 16 * E + 1)]
    rc, got = sv.ShuffleV(gpu, dev_append.cut(x, lens), E, unit=unit, dst_off=15).result()
    assert rc == 0 and got == _shuffled(x, E, unit)


# ---------------------------------------------------------------- the archive call
def _same_as_the_sibling(gpu, x, lens, E, max_piece, k=0, **kw):
    """compress_shufflev_device over the cut == compress_shuffle_device of the concatenation: the archive and the result word"""
    cap = kw.pop("cap", None) or bound(gpu, len(x))
    want = ss.compress_shuffle(gpu, x, E, cap, max_piece, src_off=k % 16, dst_off=(k + 5) % 16, **kw)
    got = sv.compress_shufflev(gpu, dev_append.cut(x, lens), E, cap, max_piece, dst_off=(3 * k + 1) % 16, k0=k, **kw)
    assert got[0] == want[0] and got[1] == want[1], (len(x), len(lens), E, max_piece, got[0], want[0])
    return want


@pytest.mark.parametrize("max_piece", [4096, 8192, 0])
@pytest.mark.parametrize("E", sv.ELEMS)
def test_archive_is_the_siblings(gpu, E, max_piece):
    x = _x(TOTAL, E)
    cuts = sv.cuts(TOTAL, E)
    for k, name in enumerate(("one entry", "multiples of 16 E", "16 E + 1", "empty entries", "more than 1024 entries", "a unit boundary",
                              "a chunk boundary")):
        rc, arc = _same_as_the_sibling(gpu, x, cuts[name], E, max_piece, k, seekable=True)
        assert rc > 0
    x = _x(sv.ORDERS_TOTAL, E)
    _same_as_the_sibling(gpu, x, dev_append.orders()["shuffled 0"], E, max_piece, 9, seekable=True)
    for n in (0, 1, E + 1, 4097):
        _same_as_the_sibling(gpu, _x(n, E), sv.cuts(n, E)["empty entries"], E, max_piece, n, seekable=True)


@pytest.mark.parametrize("case", ["level 6", "level 7", "checksums", "non-seekable", "dictionary", "64 KiB blocks", "5000 tiny entries"])
def test_archive_with_other_options(gpu, case):
    level = {"level 6": 6, "level 7": 7}.get(case, 3)
    kw = dict(level=level, seekable=case != "non-seekable", checksum=case == "checksums")
    if case == "dictionary":
        kw["dd"] = dev_append.dict_of(gpu, 3000)
    if case == "64 KiB blocks":
        E, n = 2, 2 * 65536 + 4097
        x = _x(n, E)
        _same_as_the_sibling(gpu, x, [65536, 30000, 0, 35536 + 100, n - 2 * 65536 - 100], E, 65536, bs=65536, **kw)
        _same_as_the_sibling(gpu, x, sv.cuts(n, E)["multiples of 16 E"], E, 0, bs=65536, **kw)
        return
    if case == "5000 tiny entries":
        rng = np.random.default_rng(5)
        lens = [int(v) for v in rng.integers(0, 8, 5000)]
        _same_as_the_sibling(gpu, _x(sum(lens), 4), lens, 4, 8192, **kw)
        return
    for k, (n, E, name) in enumerate(((TOTAL, 2, "16 E + 1"), (2 * 4096 + 13, 4, "1 to 7 bytes"), (4096, 8, "empty entries"),
                                      (0, 4, "one entry"))):
        for mp in (8192, 0):
            _same_as_the_sibling(gpu, _x(n, E), sv.cuts(n, E)[name], E, mp, k, **kw)


def test_capacity_binds_exactly(gpu):
    for E, n in ((2, TOTAL), (8, 4097)):
        x = _x(n, E)
        lens = sv.cuts(n, E)["16 E + 1"]
        size, _ = ss.compress_shuffle(gpu, x, E, bound(gpu, n), 0, seekable=True)
        assert size > 0
        for mp in (4096, 8192, 0):
            short = _same_as_the_sibling(gpu, x, lens, E, mp, 3, cap=size - 1, seekable=True)
            assert short[0] == ERR["DST_TOO_SMALL"], (E, mp)
            assert _same_as_the_sibling(gpu, x, lens, E, mp, 3, cap=size, seekable=True)[0] == size, (E, mp)


# ---------------------------------------------------------------- tables the scan refuses
@pytest.mark.parametrize("case", list(dev_append.bad_table_cases()))
def test_bad_tables_are_refused_by_status(gpu, case):
    lens = [BS + 7, 3 * BS, 50, 0, 2 * BS + 1]
    n = sum(lens)
    x = _x(n, 4)
    parts = dev_append.cut(x, lens)
    promised, fix, want = sv.bad_table(lens, case)
    # the kernel call: the status is the table's error and the destination keeps its pattern
    call = sv.ShuffleV(gpu, parts, 4, total=promised, fix=fix)
    rc, got = call.result()
    assert rc == ERR[want], (case, rc)
    at = 256 + call.dst.off
    assert got == call.dst.host[at: at + promised].tobytes(), "d_dst was written after a table error"
    # the archive call: *d_result is the table's error, the canaries hold (result() reads them), and the same work area serves
    # a valid call afterwards
    cap = bound(gpu, n + 1)
    for mp in (8192, 0):
        bad = sv.CompressV(gpu, parts, 4, cap, mp, seekable=True, checksum=True, total=promised, fix=fix)
        assert bad.result()[0] == ERR[want], (case, mp)
        if promised >= n:                                              # (the work area of the larger promise holds the valid call)
            good = sv.CompressV(gpu, parts, 4, cap, mp, seekable=True, checksum=True, work=bad.work)
            assert good.result() == ss.compress_shuffle(gpu, x, 4, cap, mp, seekable=True, checksum=True), (case, mp)


# ---------------------------------------------------------------- streams
def test_two_streams_at_once_with_tables_uploaded_on_them(gpu):
    """each call has its own work area; its table and entries are uploaded on its stream right in front of it, with no
    synchronisation in between"""
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    n = 64 * 4096 + 1234
    xs = [_x(n, 2), _x(n + 4096, 8)]
    cuts = [sv.cuts(len(x), E)["multiples of 16 E"][:-1] for x, E in zip(xs, (2, 8))]
    cuts = [c + [len(x) - sum(c)] for c, x in zip(cuts, xs)]
    torch.cuda.synchronize()
    cs = [sv.CompressV(gpu, dev_append.cut(x, c), E, bound(gpu, len(x)), 8192, seekable=True, stream=st, dst_off=1 + i)
          for i, (x, c, E, st) in enumerate(zip(xs, cuts, (2, 8), streams))]
    ks = [sv.ShuffleV(gpu, dev_append.cut(x, c), E, stream=st) for x, c, E, st in zip(xs, cuts, (2, 8), streams)]
    for c, k, x, E in zip(cs, ks, xs, (2, 8)):
        assert c.result() == ss.compress_shuffle(gpu, x, E, bound(gpu, len(x)), 8192, seekable=True), E
        assert k.result() == (0, _shuffled(x, E)), E


# ---------------------------------------------------------------- save with shufflev, load with rangesv_shuffle
@pytest.mark.parametrize("E", sv.ELEMS)
def test_state_dict_round_trip(gpu, E):
    """a dozen tensors, every length a multiple of E, empty ones among them -> one seekable archive; every tensor, and a shuffled
    subset, comes back through decompress_rangesv_shuffle_device at offset = starts[r], each into an allocation of its own"""
    lens = [E * c for c in (0, 1, 100, 1024, 0, 3001, 7, 2048, 515, 4096, 33, 0)]
    total = sum(lens)
    x = _x(total, E)
    parts = dev_append.cut(x, lens)
    rc, arc = sv.compress_shufflev(gpu, parts, E, bound(gpu, total), 8192, seekable=True, checksum=True)
    assert rc > 0
    d_arc = devtest.to_dev(arc, devtest.PAD)
    nb = -(-total // BS)
    index = rs.open_device(gpu, d_arc, len(arc), BS, nb)
    starts = sv.starts(lens)
    order = list(range(len(lens)))
    random.Random(E).shuffle(order)
    for which in (list(range(len(lens))), order[:5]):
        dests = [ss.Guarded(lens[r], (3 * r + 1) % 16) for r in which]
        table = np.zeros(len(which), dtype=gpu.RANGEV_DTYPE)
        for i, (r, d) in enumerate(zip(which, dests)):
            table[i] = (starts[r], lens[r], d.ptr)
        results = rs.fetch(gpu, d_arc, len(arc), index, table, len(which), max(lens), E, BS)
        assert rs.index_status(index) == 0
        assert results == [lens[r] for r in which], which
        for r, d in zip(which, dests):
            assert d.read() == parts[r], (E, r)
    import oracle_py
    if oracle_py.Ref.available():                                      # an ordinary archive of the shuffled bytes to the reference
        got = devtest.ref_decompress(oracle_py.Ref(), arc, total, checksum=True)
        assert got == (total, _shuffled(x, E))
