"""Blocks for the lane predicates of the lean executor's batch loop (zxc_amd/csrc/zxc_seq_lean.inc), shared by
tests/test_lean_predicates_cpu.py (the CPU wave emulator) and tests/test_gpu_lean_predicates.py (the device). Not a conftest.

The predicates are straight-line code on registers: far_ok and its five guards, the literal / far / near group predicates,
the classification of the near matches. Two sources of blocks:
* the families of tests/decode_limit_cases.py whose limit one of those predicates decides (FAMS), with their path-marker
  expectations as they stand there;
* a seeded sweep of single blocks of 4 KiB, the smallest block size, built with the helpers of tests/golden/craft.py through
  decode_limit_cases.B: 256 to 1 024 short sequences that decode to 4.2 - 5.8 KB (a 4 KiB launch has a capacity of 4096 + 2112
  bytes), so the ring's lower edge ring_lo leaves 0 in the block's last batches, the flushed mark moves through 1 - 5 KiB,
  the job's out_len ends the slot in the middle of the data (the slot-edge guard; a few blocks have an out_len below 32:
  far_en), and the last batch runs the exact checks. Every sequence's source is drawn around one of ring_lo, the flushed
  mark, output position 4 and the slot's edge, by the batch model of decode_limit_cases.py (a batch = the next 64 sequences;
  no block here has a tile or varint cut: at most 33 bytes and few escapes per sequence);
* one block of 64 KiB in which, for every KiB mark, a source starts below it and ends above it while the mark is the flushed
  mark of the batch, and again later."""
import functools
import random

import decode_limit_cases as D

FAMS = ("far", "lit_len", "match_len", "deps", "tile", "small", "errors")
CAP_4K = 4096 + D.PAD
N_SWEEP = 48
LONG_ML = (33, 64, 127, 128, 129)  # escapes (a varint each): at most four per batch


def _r16(x):
    return (x + 15) & ~15


def _lengths(r, n, per, room):
    """n (ll, ml) of about `per` bytes each and at most `room` bytes in all, fields without an escape but for a few long matches"""
    out, longs = [], 0
    for i in range(n):
        left = room - sum(a + b for a, b in out) - 5 * (n - i - 1)
        ll = r.randrange(0, max(1, min(15, int(per) - 3)))
        ml = 5 + r.randrange(0, max(1, min(15, int(per))))
        if longs < 4 and r.random() < 0.03:
            ml, longs = r.choice(LONG_ML), longs + 1
        if ll + ml > left:
            ll, ml = 0, 5
        assert ll + ml <= left, (ll, ml, left)
        out.append((ll, ml))
    return out


def sweep_block(seed):
    """-> decode_limit_cases.LCase: one 4 KiB block of the sweep"""
    r = random.Random(seed)
    n_seq = r.randrange(256, 1025)
    total = max(int(5.4 * n_seq) + 8, r.randrange(4200, CAP_4K - 400))
    out_len = r.randrange(1, 40) if seed % 8 == 7 else r.randrange(1200, 3600)
    out_pad = _r16(out_len)
    b = D.B(0x5EEB0000 + seed)
    while len(b.seqs) < n_seq:
        n = min(64, n_seq - len(b.seqs))
        p = b.pos
        lens = _lengths(r, n, (total - p) / (n_seq - len(b.seqs)), total - p - 5 * (n_seq - len(b.seqs) - n))
        tile_end = p + sum(ll + ml for ll, ml in lens)
        assert tile_end - p <= D.LEAN_TILE_MAX
        ring_lo, flushed = max(0, _r16(tile_end) - D.RING), p & ~1023
        for ll, ml in lens:
            m = b.pos + ll
            if m == 0:
                ll, m = 1, 1
            x = r.random()
            if x < 0.2:
                qa = ring_lo + r.randrange(-6, 7)
            elif x < 0.35:
                qa = flushed - ml + r.randrange(-3, 4)
            elif x < 0.45:
                qa = r.randrange(0, 9)
            elif x < 0.6:
                qa = out_pad - ml - r.randrange(0, 40)
            elif x < 0.7:
                qa = m - r.randrange(1, 17)  # a short period
            else:
                qa = m - r.randrange(1, 600)
            if ml > D.MATCH_MED and ring_lo > 8:
                qa = r.randrange(4, ring_lo)  # too long for the group path, from behind the ring
            qa = min(max(qa, 0), m - 1)
            b.add(ll, ml, m - qa)
    b.trail = r.choice((0, 1, 5, 16, 17))
    return b.case(f"sweep/{seed}", "sweep", bs=4096, out_len=out_len, routes=("lean",))


@functools.lru_cache(maxsize=1)
def sweep(oracle):
    """-> (the sweep's blocks the oracle decodes, how many it refuses). None is built to fail; the reference's reserve for its
    4x-unrolled loops may still refuse a varint-extended sequence near the capacity."""
    good, refused = [], 0
    for seed in range(N_SWEEP):
        c = sweep_block(seed)
        rc, got = oracle.decode_block(D.build_block(oracle, c), c.bs)
        if rc < 0:
            refused += 1
            continue
        assert rc == len(got) == len(D.expand(c.seqs, c.lits)) and 4200 <= rc <= CAP_4K, (c.name, rc)
        assert 256 <= len(c.seqs) <= 1024
        good.append(c)
    return good, refused


@functools.lru_cache(maxsize=1)
def straddle_block():
    """-> LCase: 64 KiB whose sources straddle every KiB mark (as the batch's flushed mark, and as an older one)"""
    r = random.Random(0x57AD)
    b = D.B(0x57AD)
    fresh, old = set(), set()
    while b.pos + 64 * 30 + 40 <= 65536:
        p = b.pos
        flushed = p & ~1023
        todo = [m for m in range(1024, flushed, 1024) if m not in fresh | old][:3]  # (stepped over by a batch of 1 920 bytes)
        marks = [flushed, flushed - 1024] + todo + [1024 * r.randrange(1, max(2, flushed >> 10)) for _ in range(4)]
        marks = [m for m in marks if 1024 <= m <= flushed]
        last = flushed
        for i in range(64):
            ll = 14 - r.randrange(0, 4)
            ml = 30 - ll
            m = b.pos + ll
            if i % 7 == 3 and marks:
                mark = marks[(i // 7) % len(marks)]
                qa = mark - r.randrange(1, ml)
                (fresh if mark == flushed else old).add(mark)
            else:
                qa = m - r.randrange(1, min(m, 900) + 1) if m > ll else 0
            b.add(ll, ml, m - qa)
    b.trail = 5
    want = set(range(1024, last + 1, 1024))  # every mark that was flushed when a batch began
    assert last >= 60 * 1024 and want <= fresh | old and len(fresh) >= 30, (sorted(want - fresh - old), len(fresh))
    return b.case("straddle_kib", "sweep", bs=65536, routes=("lean",))
