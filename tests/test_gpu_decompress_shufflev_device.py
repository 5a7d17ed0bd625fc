"""The unshufflev calls of include/zxc_mi355x_unshufflev.h on the GPU, at unit and block size 4096 unless a case says otherwise:
unshufflev_device against numpy's un-shuffle over the cut lists of the CPU replay, decompress_shufflev_device byte for byte and
word for word against decompress_shuffle_device for the same archive run in the same test, the state-dict round trip the calls
exist for, a total that is not the decoded size, truncated and damaged archives, tables the scan refuses, and two streams.

The entries are unshufflev_support.DestTable's: slices of one tensor with canaries around each, aligned or at odd addresses;
source, scratch and work area lie at odd addresses between canaries. Nothing here provokes a fault: every table, the refused ones
included, names only memory that exists (a zero base apart, which the scan refuses before any kernel looks at an entry), refused
tables and damaged archives are refused by status."""
import numpy as np
import pytest

import dev_append
import dev_take
import devtest
import shuffle_support as ss
import shufflev_support as sv
import unshufflev_support as uv
from devtest import ERR, bound
from shuffle_support import BS

pytestmark = pytest.mark.gpu
gpu = devtest.gpu_fixture(needs="decompress_shufflev_device")

TOTAL = 9 * 4096 + 1000
SRC_OFFS = (0, 1, 15)
MAX_PIECES = (4096, 8192, 0)


def _x(n, E):
    return ss.tensor_bytes(n, E, seed=79 * E + n)


def _np(b):
    return np.frombuffer(b, dtype=np.uint8)


def _unshuffled(y, E, unit=BS):
    return ss.np_unshuffle(_np(y), E, unit).tobytes()


# ---------------------------------------------------------------- the kernel call
@pytest.mark.parametrize("E", sv.ELEMS)
def test_kernel_call_equals_numpy_over_the_cuts(gpu, E):
    k = 0
    for name, lens in sv.cuts(TOTAL, E).items():
        if name == "1 to 7 bytes":
            lens = sv.cuts(2 * 4096 + 3 * E + 1, E)[name]              # (some 2000 entries)
        y = _x(sum(lens), E)
        rc, got = uv.UnshuffleV(gpu, y, lens, E, src_off=SRC_OFFS[k % 3], aligned=k % 2 == 0, k0=k).result()
        assert rc == 0 and got == _unshuffled(y, E), (name, E)
        k += 1
    y = _x(sv.ORDERS_TOTAL, E)
    for name, lens in dev_append.orders().items():
        rc, got = uv.UnshuffleV(gpu, y, lens, E, src_off=SRC_OFFS[k % 3], aligned=k % 2 == 0, k0=k).result()
        assert rc == 0 and got == _unshuffled(y, E), (name, E)
        k += 1
    for n in ss.sizes(E):                                             # where a path of the plan begins or ends
        y = _x(n, E)
        rc, got = uv.UnshuffleV(gpu, y, sv.cuts(n, E)["16 E + 1"], E, src_off=SRC_OFFS[k % 3], k0=k).result()
        assert rc == 0 and got == _unshuffled(y, E), (n, E)
        k += 1


def test_kernel_call_with_nothing_a_larger_unit_and_tiny_entries(gpu):
    assert uv.UnshuffleV(gpu, b"", [], 4).result() == (0, b"")         # the store of the status alone
    assert uv.UnshuffleV(gpu, b"", [0, 0, 0], 2).result() == (0, b"")
    E, unit = 4, 65536                                                 # the plane stride is another, the plan is the same
    n = 2 * unit + 17 * E + 3
    y = _x(n, E)
    lens = [unit - 5, 10, 0, unit + 1, 16 * E + 1, n - (2 * unit + 6 + 16 * E + 1)]
    rc, got = uv.UnshuffleV(gpu, y, lens, E, unit=unit, src_off=15).result()
    assert rc == 0 and got == _unshuffled(y, E, unit)
    rng = np.random.default_rng(5)                                     # 5000 tiny entries, empty ones among them
    lens = [int(v) for v in rng.integers(0, 8, 5000)]
    y = _x(sum(lens), 2)
    rc, got = uv.UnshuffleV(gpu, y, lens, 2, src_off=1).result()
    assert rc == 0 and got == _unshuffled(y, 2)


# ---------------------------------------------------------------- the archive call
def _archive(gpu, x, E, lens=None, mp=8192, **kw):
    """the archive of the shuffled x: compress_shuffle_device, or with `lens` compress_shufflev_device over that cut"""
    cap = bound(gpu, len(x))
    if lens is None:
        rc, arc = ss.compress_shuffle(gpu, x, E, cap, mp, **kw)
    else:
        rc, arc = sv.compress_shufflev(gpu, dev_append.cut(x, lens), E, cap, mp, **kw)
    assert rc > 0
    return arc


def _same_as_the_sibling(gpu, arc, n, cuts, E, max_piece, k=0, **kw):
    """decompress_shufflev_device into each cut == decompress_shuffle_device into one buffer, run here: the bytes and the word"""
    want = ss.Decompress(gpu, arc, n, E, max_piece, dst_off=k % 16, **kw).result()
    for i, lens in enumerate(cuts):
        got = uv.DecompressV(gpu, arc, lens, E, max_piece, aligned=(k + i) % 2 == 0, k0=k + i, **kw).result()
        assert got == want, (n, len(lens), E, max_piece, got[0], want[0])
    return want


@pytest.mark.parametrize("max_piece", MAX_PIECES)
@pytest.mark.parametrize("E", sv.ELEMS)
def test_entries_are_the_siblings_bytes(gpu, E, max_piece):
    x = _x(TOTAL, E)
    cuts = sv.cuts(TOTAL, E)
    names = ("one entry", "multiples of 16 E", "16 E + 1", "empty entries", "more than 1024 entries", "a unit boundary", "a chunk boundary")
    arc = _archive(gpu, x, E, cuts["16 E + 1"] if E == 4 else None, seekable=True)
    assert _same_as_the_sibling(gpu, arc, TOTAL, [cuts[name] for name in names], E, max_piece) == (TOTAL, x)
    x = _x(sv.ORDERS_TOTAL, E)
    _same_as_the_sibling(gpu, _archive(gpu, x, E, seekable=True), len(x), [dev_append.orders()["shuffled 0"]], E, max_piece, 9)
    for n in (0, 1, E + 1, 4097):
        want = _same_as_the_sibling(gpu, _archive(gpu, _x(n, E), E, seekable=True), n, [sv.cuts(n, E)["empty entries"]], E, max_piece, n)
        assert want == (n, _x(n, E))
    # the empty-frame probe with no table at all
    empty = _archive(gpu, b"", E)
    assert _same_as_the_sibling(gpu, empty, 0, [[]], E, max_piece) == (0, b"")


@pytest.mark.parametrize("case", ["level 6", "level 7", "checksums", "non-seekable", "dictionary", "64 KiB blocks"])
def test_archive_with_other_options(gpu, case):
    level = {"level 6": 6, "level 7": 7}.get(case, 3)
    ckw = dict(level=level, seekable=case != "non-seekable", checksum=case == "checksums")
    dkw = dict(checksum=case == "checksums")
    if case == "dictionary":
        ckw["dd"] = dkw["dd"] = dev_append.dict_of(gpu, 3000)
    if case == "64 KiB blocks":
        E, n = 2, 2 * 65536 + 4097
        x = _x(n, E)
        arc = _archive(gpu, x, E, mp=65536, bs=65536, **ckw)
        cuts = [[65536, 30000, 0, 35536 + 100, n - 2 * 65536 - 100], sv.cuts(n, E)["multiples of 16 E"]]
        for mp in (65536, 0):
            assert _same_as_the_sibling(gpu, arc, n, cuts, E, mp, bs=65536, **dkw) == (n, x)
        return
    for k, (n, E, name) in enumerate(((TOTAL, 2, "16 E + 1"), (2 * 4096 + 13, 4, "1 to 7 bytes"), (4096, 8, "empty entries"),
                                      (0, 4, "one entry"))):
        x = _x(n, E)
        lens = sv.cuts(n, E)[name]
        arc = _archive(gpu, x, E, lens if k % 2 else None, **ckw)
        for mp in (8192, 0):
            assert _same_as_the_sibling(gpu, arc, n, [lens], E, mp, k, **dkw) == (n, x), (case, n, E, mp)


@pytest.mark.parametrize("E", sv.ELEMS)
def test_state_dict_round_trip(gpu, E):
    """a dozen tensors, empty ones among them -> compress_shufflev_device -> one archive -> decompress_shufflev_device into fresh
    allocations: every tensor comes out equal"""
    lens = [E * c for c in (0, 1, 100, 1024, 0, 3001, 7, 2048, 515, 4096, 33, 0)]
    total = sum(lens)
    x = _x(total, E)
    parts = dev_append.cut(x, lens)
    rc, arc = sv.compress_shufflev(gpu, parts, E, bound(gpu, total), 8192, checksum=True)   # (not seekable: the load needs no index)
    assert rc > 0
    for mp in (8192, 0):
        call = uv.DecompressV(gpu, arc, lens, E, mp, checksum=True)
        rc, out = call.result()
        assert rc == total and dev_append.cut(out, lens) == parts, (E, mp)


def test_total_must_be_the_decoded_size(gpu):
    for E, n in ((2, TOTAL), (4, 4096), (8, 1)):
        arc = _archive(gpu, _x(n, E), E, seekable=True, checksum=True)
        for mp in MAX_PIECES:
            over = sv.cuts(n, E)["16 E + 1"] + [1]                     # a valid table of n + 1 bytes
            assert uv.DecompressV(gpu, arc, over, E, mp, checksum=True).result()[0] == ERR["CORRUPT_DATA"], (E, mp)
            want = ss.Decompress(gpu, arc, n - 1, E, mp, checksum=True).result()[0]
            assert want < 0 or n == 1
            assert uv.DecompressV(gpu, arc, sv.cuts(n - 1, E)["16 E + 1"], E, mp, checksum=True).result()[0] == want, (E, mp)


def test_truncated_and_damaged_archives_get_the_siblings_word(gpu):
    """nothing outside the entries changes (result() reads the canaries); the entries' bytes are not compared after an error"""
    E = 4
    x = _x(TOTAL, E)
    arc = _archive(gpu, x, E, seekable=True, checksum=True)
    at, n = dev_take.blocks_at(arc)[3]
    flipped = bytearray(arc)
    flipped[at + 8 + (n - 12) // 2] ^= 0x40                            # one payload byte of the fourth block
    lens = sv.cuts(TOTAL, E)["16 E + 1"]
    for name, bad in (("truncated", arc[: at + n // 2]), ("flipped", bytes(flipped))):
        for mp in (8192, 0):
            want = ss.Decompress(gpu, bad, TOTAL, E, mp, checksum=True).result()[0]
            assert want < 0, (name, mp, want)
            assert uv.DecompressV(gpu, bad, lens, E, mp, checksum=True).result()[0] == want, (name, mp)


# ---------------------------------------------------------------- tables the scan refuses
@pytest.mark.parametrize("case", list(dev_append.bad_table_cases()))
def test_bad_tables_are_refused_by_status(gpu, case):
    lens = [BS + 7, 3 * BS, 50, 0, 2 * BS + 1]
    n = sum(lens)
    x = _x(n + 1, 4)
    promised, fix, want = sv.bad_table(lens, case)
    want = {"SRC_TOO_SMALL": "DST_TOO_SMALL"}.get(want, want)         # the read direction's word
    # the kernel call: the status is the table's error and every entry keeps its pattern
    call = uv.UnshuffleV(gpu, x[:max(promised, 1)], lens, 4, total=promised, fix=fix)
    assert call.result()[0] == ERR[want], case
    assert call.tb.untouched(), "an entry was written after a table error"
    # the archive call: *d_result is the table's error, no entry is written, the canaries hold (result() reads them), and the same
    # work area serves a valid call afterwards
    arc = _archive(gpu, x[:n], 4, seekable=True, checksum=True)
    for mp in (8192, 0):
        bad = uv.DecompressV(gpu, arc, lens, 4, mp, checksum=True, total=promised, fix=fix)
        assert bad.result()[0] == ERR[want], (case, mp)
        assert bad.tb.untouched(), "an entry was written after a table error"
        if promised >= n:                                              # (the work area of the larger promise holds the valid call)
            good = uv.DecompressV(gpu, arc, lens, 4, mp, checksum=True, work=bad.work)
            assert good.result() == (n, x[:n]), (case, mp)


# ---------------------------------------------------------------- streams
def test_two_streams_at_once_with_tables_uploaded_on_them(gpu):
    """each call has its own work area; its table, entries and archive are uploaded on its stream right in front of it, with no
    synchronisation in between"""
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    n = 64 * 4096 + 1234
    xs = [_x(n, 2), _x(n + 4096, 8)]
    cuts = [sv.cuts(len(x), E)["multiples of 16 E"] for x, E in zip(xs, (2, 8))]
    arcs = [_archive(gpu, x, E, seekable=True) for x, E in zip(xs, (2, 8))]
    torch.cuda.synchronize()
    ds = [uv.DecompressV(gpu, arc, c, E, 8192, stream=st, k0=i) for i, (arc, c, E, st) in enumerate(zip(arcs, cuts, (2, 8), streams))]
    ks = [uv.UnshuffleV(gpu, x, c, E, stream=st) for x, c, E, st in zip(xs, cuts, (2, 8), streams)]
    for d, k, x, E in zip(ds, ks, xs, (2, 8)):
        assert d.result() == (len(x), x), E
        assert k.result() == (0, _unshuffled(x, E)), E
