"""Inputs that put the block encoder (zxc_encode_kernel.hip: match finder, parse, serialiser) at its format and table limits,
shared by tests/test_encode_limits_cpu.py (the kernel on the CPU wave emulator, against tests/zxc_block_model.py and the
reference) and tests/test_gpu_encode_limits.py (the kernel on the device, against the emulator's recorded digests).

Every case is seeded (random.Random only: the same bytes on every machine), at most a few blocks, and carries a SUBJECT check:
hits(level, blocks) looks at zxc_block_model.parse_block of every emitted block and returns the names of the limits the archive
really reached. `must` maps every limit to the levels at which it has to be reached; a level is left out only where the format
rules the limit out, with the reason in `why`. A case whose limit is reached at no level is a failure, never a skip.

Levels 6-7 run on inputs of at most 16 KiB in 4 KiB blocks only (the emulator needs ~9 s for a full 64 KiB level-6 block)."""
import random

GLO_LEVELS, GHI_LEVELS = (3, 4, 5), (1, 2)
ALL, LOW = (1, 2, 3, 4, 5, 6, 7), (1, 2, 3, 4, 5)
NO_RLE = "GHI blocks (levels 1-2) have no RLE literal section; levels 6-7 code the literals with PivCo when that wins"
NO_OFF8 = "GHI blocks (levels 1-2) have no 8-bit offset mode"
BIG_ONLY = "needs a 64 KiB (or larger) block: levels 6-7 run on 4 KiB blocks only"


def rnd(n, seed):
    return random.Random(seed).randbytes(n)


def rnd_no(n, seed, avoid):
    """n random bytes without the byte values in `avoid` and without two equal neighbours"""
    r, out = random.Random(seed), bytearray()
    while len(out) < n:
        b = r.randrange(256)
        if b not in avoid and (not out or out[-1] != b):
            out.append(b)
    return bytes(out)


class Case:
    def __init__(self, name, family, data, bs, levels, must, hits, why="", dict_=None, items=None, small=None):
        self.name, self.family, self.data, self.bs, self.levels = name, family, data, bs, tuple(levels)
        self.must, self.hits, self.why, self.dict_, self.items = must, hits, why, dict_, items
        self.small = bs == 4096 if small is None else small  # the GPU module runs dictionary / checksum variants on these
        assert bs in (4096, 65536, 131072)
        assert all(set(v) <= set(self.levels) for v in must.values()), name
        assert max(self.levels) <= 5 or (bs == 4096 and len(data) <= 16384), name

    def block_lengths(self):
        n, bs = len(self.data), self.bs
        return [min(bs, n - o) for o in range(0, n, bs)]


def _seqs(blocks):
    return [s for b in blocks if b["seqs"] for s in b["seqs"]]


def _filled(content, bs, seed):
    """content + a filler that costs one long match (the block's first 48 bytes over and over), to exactly bs bytes"""
    assert 48 <= len(content) <= bs, len(content)
    unit = content[:48]
    fill = (unit * (bs // 48 + 2))[: bs - len(content)]
    return content + fill


# ---------------------------------------------------------------- literal-length escapes
def _ll_block(lengths, seed, bs):
    """Short runs (L < 448): a phrase, then for every L: L incompressible bytes and the phrase again. Long runs: L incompressible
    bytes whose last 72 come again at once, so the match behind the run is found at distance 72 whatever the tables hold after
    16 KiB of noise (72 > 64: a chunk's lookups do not see the chunk's own positions); it starts in a chunk the skip acceleration
    still searches (chunk index a multiple of four: the match in front is stretched until it does)."""
    r = random.Random(seed)
    ph = r.randbytes(32)
    out = bytearray(ph)
    for L in lengths:
        if L < 448:
            out += r.randbytes(L) + ph
            continue
        while (len(out) + L) % 256:
            out.append(out[-72] if len(out) > 104 else ph[len(out) % 32])
        run = bytearray(r.randbytes(L))
        run[0] = out[-72] ^ 0xA5 if len(out) >= 72 else run[0]
        out += run + run[-72:]
        out.append(out[-72] ^ 0x5A)
    return _filled(bytes(out), bs, seed)


def _ll_hits(targets):
    def hits(level, blocks):
        esc = 255 if level <= 2 else 15
        want = {esc - 1: "esc-1", esc: "esc", esc + 127: "esc+127", esc + 128: "esc+128", esc + 16383: "esc+16383",
                esc + 16384: "esc+16384"}
        got = {s[0] for s in _seqs(blocks)}
        return {"ll=" + n for v, n in want.items() if v in got and n in targets}
    return hits


def _ll_cases():
    small = ("esc-1", "esc", "esc+127", "esc+128")
    d = _ll_block([13, 14, 15, 16, 17, 141, 142, 143, 144, 145, 253, 254, 255, 256, 257], 101, 4096) + \
        _ll_block([381, 382, 383, 384, 385], 102, 4096)
    yield Case("ll_small", "literal-length escapes", d, 4096, ALL, {"ll=" + n: ALL for n in small}, _ll_hits(small))
    big = ("esc+16383", "esc+16384")
    d = _ll_block([16397, 16398, 16399], 103, 65536) + _ll_block([16400, 16638, 16639], 104, 65536) + _ll_block([16637, 16640], 105, 65536)
    yield Case("ll_big", "literal-length escapes", d, 65536, LOW, {"ll=" + n: LOW for n in big}, _ll_hits(big), why=BIG_ONLY)


# ---------------------------------------------------------------- match-length escapes
def _ml_block(lengths, seed, bs):
    """for every M: a fresh unit of 72 incompressible bytes that goes on periodically for exactly M more bytes, then one byte
    that breaks the period: a copy of exactly M bytes at distance 72, whatever the search depth (72 > 64: a chunk's lookups do
    not see the chunk's own positions)"""
    r = random.Random(seed)
    out = bytearray(r.randbytes(48))
    for M in lengths:
        u = r.randbytes(72)
        out += u
        for k in range(M):
            out.append(u[k % 72])
        out.append(u[M % 72] ^ 0x55)
    return _filled(bytes(out), bs, seed)


def _ml_hits(targets):
    def hits(level, blocks):
        esc = 255 if level <= 2 else 15
        want = {esc - 1: "esc-1", esc: "esc", esc + 127: "esc+127", esc + 128: "esc+128", esc + 16383: "esc+16383",
                esc + 16384: "esc+16384"}
        got = {s[1] - 5 for s in _seqs(blocks)}
        return {"ml-5=" + n for v, n in want.items() if v in got and n in targets}
    return hits


def _long_ml_hits(level, blocks):
    return {"ml>65536"} if any(s[1] > 65536 for s in _seqs(blocks)) else set()


def _ml_cases():
    small = ("esc-1", "esc", "esc+127", "esc+128")
    d = _ml_block([18, 19, 20, 21, 22, 146, 147, 148, 149, 150], 201, 4096) + _ml_block([258, 259, 260, 261, 262], 202, 4096) + \
        _ml_block([386, 387, 388, 389, 390], 203, 4096)
    must = {"ml-5=" + n: ALL for n in small}
    must["ml-5=esc"] = must["ml-5=esc+128"] = (1, 2, 3, 4, 5, 7)
    yield Case("ml_small", "match-length escapes", d, 4096, ALL, must, _ml_hits(small),
               why="level 6: the optimal parse prices a match of esc + 5 bytes above one a byte shorter plus a literal, and cuts it")
    big = ("esc+16383", "esc+16384")
    d = _ml_block([16402, 16403, 16404], 204, 65536) + _ml_block([16405, 16642, 16643], 205, 65536) + _ml_block([16644, 16645], 206, 65536)
    yield Case("ml_big", "match-length escapes", d, 65536, LOW, {"ml-5=" + n: LOW for n in big}, _ml_hits(big), why=BIG_ONLY)
    yield Case("ml_zeros_128k", "match-length escapes", bytes(131072), 131072, LOW, {"ml>65536": LOW}, _long_ml_hits, why=BIG_ONLY)
    yield Case("ml_period10_128k", "match-length escapes", (b"abcdefghij" * 13108)[:131072], 131072, LOW, {"ml>65536": LOW},
               _long_ml_hits, why=BIG_ONLY)


# ---------------------------------------------------------------- offsets
def _off_hits(level, blocks):
    out = set()
    for k, period in enumerate((255, 256, 257)):
        b = blocks[k]
        if b["seqs"] and max(s[2] for s in b["seqs"]) == period:
            out.add("max_off=%d" % period)
            if b["type"] == 1 and b["enc_off"] == (1 if period <= 256 else 0):
                out.add("enc_off@%d" % period)
    return out


def _far_hits(level, blocks):
    offs = [s[2] for s in _seqs(blocks)]
    out = {"off<=65536"} if offs and max(offs) <= 65536 else set()
    if any(o >= 60000 for o in offs):
        out.add("off>=60000")
    if 65535 in offs:
        out.add("off=65535")
    return out


def _off_cases():
    d = b"".join((rnd_no(p, 300 + p, ()) * 20)[:4096] for p in (255, 256, 257))
    must = {"max_off=%d" % p: ALL for p in (255, 256, 257)}
    must.update({"enc_off@%d" % p: (3, 4, 5, 6, 7) for p in (255, 256, 257)})
    yield Case("off_256", "offsets", d, 4096, ALL, must, _off_hits, why=NO_OFF8)
    # phrases at distances 60 000 and 65 535 with zeros between them: a run of zeros enters one bucket only (the chunks inside a
    # long match are not inserted), so the head entries of the phrases survive at every level
    q1, q2 = rnd(64, 311), rnd(64, 312)
    b = bytearray(131072)
    for at, q in ((0, q1), (60000, q1), (60200, q2), (60200 + 65535, q2), (60400, rnd(64, 313)), (60400 + 65537, rnd(64, 313))):
        b[at:at + 64] = q
    yield Case("off_far", "offsets", bytes(b), 131072, LOW, {"off<=65536": LOW, "off>=60000": LOW, "off=65535": LOW}, _far_hits,
               why=BIG_ONLY)


# ---------------------------------------------------------------- chain ring wrap
RING_TRIPLES, RING_B, RING_S1, RING_S2 = 14, 72, 128, 135  # (B more than a chunk behind A: a chunk's lookups do not see the chunk itself)


def _ring_c_at(R, t):
    return 64 + RING_B + R - 80 + RING_S2 * t


def _ring_data(R, seed):
    """Triples of phrases that share their first 8 bytes: A (8 + 40 bytes), B (8 + other bytes) 72 bytes behind it, and C = A's
    bytes again a (swept: R - 80 ... R + 11) bytes behind B, zeros in between (a run of zeros enters one bucket only). C's walk
    reaches B through the head table and A only through B's link in the ring, which is still there exactly while no newer
    position has taken its slot."""
    r = random.Random(seed)
    out = bytearray(_ring_c_at(R, RING_TRIPLES) + 2048)
    for t in range(RING_TRIPLES):
        w, ta, tb = r.randbytes(8), r.randbytes(40), r.randbytes(40)
        at1, at2 = 64 + RING_S1 * t, _ring_c_at(R, t)
        out[at1:at1 + 48] = w + ta
        out[at1 + RING_B:at1 + RING_B + 48] = w + tb
        out[at2:at2 + 48] = w + ta
        out[at2 + 48] = 0xFF
    return bytes(out)


def _ring_hits(R):
    """For every triple the walk from C is known: the head table gives B at distance a, and B's link leads on to A (distance
    a + 72, 48 bytes) exactly while B's ring slot cannot have been taken by a newer position: a + 64 - lane <= R, lane = C's
    place in its chunk. Otherwise the 8 bytes shared with B are all C gets. Both outcomes must occur, each at exactly the triples
    the rule names."""
    def hits(level, blocks):
        seqs = _seqs(blocks)
        kept = cut = 0
        for t in range(RING_TRIPLES):
            a, lane = R - 80 + (RING_S2 - RING_S1) * t, _ring_c_at(R, t) % 64
            through = a + 64 - lane <= R
            got_a = any(off == a + RING_B and ml >= 48 for _, ml, off in seqs)
            got_b = any(off == a and 8 <= ml < 48 for _, ml, off in seqs)
            if (got_a, got_b) != (through, not through):
                return set()
            kept += through
            cut += not through
        return ({"A through B's link: in the ring"} if kept else set()) | ({"B only: link cut off"} if cut else set())
    return hits


# (seeds searched on the emulator: a phrase whose head entry is taken by a later position of its own chunk changes the walk)
RING_SEEDS = {2048: 2, 4096: 0, 16384: 0, 32768: 0}


def _ring_cases():
    # level -> ring entries at blocks of <= 64 KiB: 2: 2^11, 3: 2^11, 4: 2^12, 5: 2^14; above 64 KiB levels 3-5 take the 2^15 entry
    for R, levels, bs in ((2048, (2, 3), 65536), (4096, (4,), 65536), (16384, (5,), 65536), (32768, (3, 4, 5), 131072)):
        lims = ("A through B's link: in the ring", "B only: link cut off")
        yield Case("ring_%d" % R, "ring wrap", _ring_data(R, RING_SEEDS[R]), bs, levels, {k: levels for k in lims}, _ring_hits(R),
                   why="only the levels whose chain ring has this size at this block size")


# ---------------------------------------------------------------- bucket collisions inside a chunk
def _period_hits(p):
    def hits(level, blocks):
        s = _seqs(blocks)
        return {"off=period"} if s and all(x[2] % p == 0 for x in s) and any(x[2] == p for x in s) else set()
    return hits


def _period_cases():
    for p in range(1, 8):
        n = 4096 + 1000 + 37 * p  # (the last chunk of both blocks' tails is short)
        yield Case("period_%d" % p, "bucket collisions", (rnd_no(p, 500 + p, ()) * (n // p + 1))[:n], 4096, ALL, {"off=period": ALL},
                   _period_hits(p))


# ---------------------------------------------------------------- RLE
def _phrase(j, salt):
    """six bytes, never a run byte (0x61-0x6F). Unique in their first two bytes; the last byte of one phrase and the first of the
    next never pair up twice, so the five bytes [last, piece of three, first] between two phrases match nothing; salt moves the
    middle bytes (and with them the buckets)"""
    f, g = 0x80 + (j & 63), 0xC0 + (j >> 6)
    return bytes([f, g, 0x10 + (j * 7 + salt) % 64, 0x11 + (j * 13 + salt * 5) % 61, g, 0x80 + j % 61])


class _RleBuilder:
    """Literal runs made the only way the encoder meets them: 1-3 equal bytes between two matches, again and again. A run of N
    bytes c is N / 3 pieces, each followed by a 6-byte phrase that was written once before (in a 'lexicon' just in front of the
    run, which is a raw literal segment) and is therefore a match here; no phrase is used twice. The lexicon's literals are cut
    by a repeated decoy every 40 phrases, which adds nothing to the literal stream."""

    def __init__(self, seed):
        self.out, self.j, self.r, self.salt = bytearray(), 0, random.Random(seed), seed

    def lexicon_and_run(self, n, c, lex_bytes=None):
        k = (n + 2) // 3
        ph = [_phrase(self.j + i, self.salt) for i in range(k)]
        self.j += k
        decoy = bytes([0x41, 0x52, 0x43, 0x54, 0x45, 0x56, 0x47, 0x58, 0x49, 0x5A])
        lex = bytearray(decoy)
        for i, q in enumerate(ph):
            if i % 40 == 39:
                lex += decoy  # a match inside the lexicon: eight chunks without a sequence would start the skip acceleration
            lex += q + bytes([0x20 + len(lex) % 31])
        if lex_bytes is not None:  # a raw segment of exactly this many LITERAL bytes in front of the run (a decoy seen before is a match)
            lits = len(lex) - len(decoy) * (lex.count(decoy) - (0 if decoy not in self.out else -1) - 1)
            assert lex_bytes >= lits, (lex_bytes, lits)
            lex += rnd_no(lex_bytes - lits, self.r.randrange(1 << 30), set(range(0x61, 0x70)) | set(range(0x80, 0x100)))
        self.out += lex
        left = n
        for q in ph:
            piece = min(3, left)
            self.out += bytes([c]) * piece + q
            left -= piece
        assert left == 0


def _lit_runs(lit):
    """[(byte, length)] of the maximal runs of >= 4 equal bytes, and the lengths of the raw stretches between / around them"""
    runs, raws, p, seg = [], [], 0, 0
    while p < len(lit):
        q = p
        while q < len(lit) and lit[q] == lit[p]:
            q += 1
        if q - p >= 4:
            raws.append(p - seg)
            runs.append(q - p)
            seg = q
        p = q
    raws.append(len(lit) - seg)
    return runs, raws


RLE_RUNS = (131, 132, 133, 134, 135, 262, 263, 264, 265, 266, 136, 393)


def _rle_hits(level, blocks):
    out = set()
    for b in blocks:
        if b["type"] != 1 or b["enc_lit"] != 1:
            continue
        runs, raws = _lit_runs(b["literals"])
        out |= {"run=%d" % n for n in runs if n in RLE_RUNS}
        out |= {"raw=%d" % n for n in raws[1:-1] if n in (128, 129)}
    return out


def _rle_edge_hits(level, blocks):
    import zxc_block_model as M
    out = set()
    for b in blocks:
        if b["type"] != 1 or b["literals"] is None:
            continue
        n = b["n_lit"]
        d = len(M.rle_encode(b["literals"])) + ((n * M.rle_premium(level)) >> 8) - n
        if d in (-1, 0, 1) and b["enc_lit"] == (1 if d < 0 else 0):
            out.add("rle+tax=lit%+d" % d)
    return out


def _room_hits(level, blocks):
    import zxc_block_model as M
    b = blocks[0]
    if b["type"] == 1 and b["literals"] is not None and 2 * b["n_lit"] > 65536 and \
            len(M.rle_encode(b["literals"])) + ((b["n_lit"] * M.rle_premium(level)) >> 8) < b["n_lit"]:
        return {"rle_wins,literals>half"} | ({"enc_lit=1"} if b["enc_lit"] == 1 else set())
    return set()


# One 4 KiB block per run length (and one per raw-segment length). A phrase is lost to the match finder when a later position of
# its chunk falls into its bucket (the chunk's highest position wins the head entry), which breaks the run; seed 0 keeps
# every block's run whole at levels 3, 4 and 5 (searched on the emulator; the subject check holds it there).


def rle_run_block(n, seed):
    B = _RleBuilder(seed)
    B.lexicon_and_run(n, 0x61 + n % 15)
    return _filled(bytes(B.out), 4096, seed)


def rle_raw_block(m, seed):
    B = _RleBuilder(seed)
    B.lexicon_and_run(40, 0x6F)
    B.lexicon_and_run(43, 0x6E, lex_bytes=m)
    return _filled(bytes(B.out), 4096, seed)


def _rle_cases():
    data = b"".join(rle_run_block(n, 0) for n in RLE_RUNS) + \
        b"".join(rle_raw_block(m, 0) for m in (128, 129))
    must = {"run=%d" % n: GLO_LEVELS for n in RLE_RUNS}
    must.update({"raw=128": GLO_LEVELS, "raw=129": GLO_LEVELS})
    yield Case("rle_runs", "RLE", data, 4096, LOW, must, _rle_hits, why=NO_RLE, small=False)
    # rle_size + tax against the literal count, one run growing byte by byte across the equality (one 4 KiB block per length)
    blocks = []
    for n in range(29, 41):
        B = _RleBuilder(620 + n)
        B.out += rnd_no(400, 640 + n, set(range(0x61, 0x70)) | set(range(0x80, 0x100)))
        B.lexicon_and_run(n, 0x61)
        B.out += rnd_no(300, 660 + n, set(range(0x61, 0x70)) | set(range(0x80, 0x100)))
        blocks.append(_filled(bytes(B.out), 4096, n))
    yield Case("rle_tax_edge", "RLE", b"".join(blocks), 4096, LOW, {"rle+tax=lit%+d" % d: GLO_LEVELS for d in (-1, 0, 1)}, _rle_edge_hits,
               why=NO_RLE, small=False)
    # literals above half of a 64 KiB block, RLE-able: four equal bytes and one that differs, the run byte changing all the time
    r, b = random.Random(680), bytearray()
    while len(b) < 65536:
        c = r.randrange(256)
        b += bytes([c]) * 4 + bytes([(c + 1 + r.randrange(254)) & 0xFF])
    yield Case("rle_room", "RLE", bytes(b[:65536]), 65536, LOW, {"rle_wins,literals>half": GLO_LEVELS, "enc_lit=1": GLO_LEVELS},
               _room_hits, why=NO_RLE + "; " + BIG_ONLY)


def _no_seq_hits(level, blocks):
    b = blocks[0]
    if b["type"] == 1 and b["n_seq"] == 0:
        return {"coded block without sequences"} | ({"enc_off=1 without sequences"} if b["enc_off"] == 1 else set())
    return set()


def _few_lit_hits(level, blocks):
    b = blocks[0]
    return {"RLE with fewer than 64 literals"} if b["type"] == 1 and 0 < b["n_lit"] < 64 and b["enc_lit"] == 1 else set()


def _rle_small_cases():
    # 128 runs of four bytes, every run byte once: nothing repeats over five bytes, so no sequence, and RLE halves the literals
    d = b"".join(bytes([c]) * 4 for c in range(128))
    lims = ("coded block without sequences", "enc_off=1 without sequences")
    yield Case("rle_no_sequence", "RLE", d, 4096, ALL, {k: GLO_LEVELS for k in lims}, _no_seq_hits,
               why=NO_OFF8 + " and no RLE, so 512 literals go RAW there; levels 6-7 may code the literals with PivCo, which changes nothing "
               "about enc_off but is not what this case pins")
    # a unit of 40 bytes with a run of 12 in it, over and over: the unit is all the literals there are
    u = rnd_no(14, 690, {0x61}) + b"a" * 12 + rnd_no(14, 691, {0x61})
    yield Case("rle_few_literals", "RLE", (u * 103)[:4096], 4096, ALL, {"RLE with fewer than 64 literals": GLO_LEVELS}, _few_lit_hits, why=NO_RLE)


# ---------------------------------------------------------------- RAW threshold
RAW_SWEEP = tuple(range(2, 16))


def _raw_sweep_block(k, seed):
    """4096 incompressible bytes with k copies of 8 bytes from 100 bytes back, all in the first 450 bytes (in front of the skip
    acceleration); -> (block, the sequences it holds by construction)"""
    r = random.Random(seed)
    out = bytearray(r.randbytes(100))
    seqs, ll = [], 100
    for _ in range(k):
        src = len(out) - 100
        out += out[src:src + 8]
        seqs.append((ll, 8, 100))
        out += r.randbytes(14)
        ll = 14
    out += r.randbytes(4096 - len(out))
    return bytes(out), seqs


def raw_sweep_intended():
    return [_raw_sweep_block(k, 700) for k in RAW_SWEEP]


def _raw_sweep_hits(level, blocks):
    import zxc_block_model as M
    out, types = set(), []
    for (data, seqs), b in zip(raw_sweep_intended(), blocks):
        lit, at = bytearray(), 0
        for ll, ml, off in seqs:
            lit += data[at:at + ll]
            at += ll + ml
        lit += data[at:]
        want = M.parse_block(M.serialise(seqs, bytes(lit), 4096, level <= 2, level, data))
        types.append(b["type"])
        if want["type"] != b["type"] or (b["type"] != 0 and b["seqs"] != seqs):
            return set()  # the rule, applied to the sequences the block holds by construction, gives another block
    for a, b in zip(types, types[1:]):
        if a == 0 and b != 0:
            out.add("RAW|coded neighbours, model agrees")
    return out


def _tail_hits(s):
    def hits(level, blocks):
        b = blocks[-1]
        ok = b["decoded"] == s if b["decoded"] is not None else True
        if ok and len(blocks) == 2 and ((b["type"] == 0) == (s < 64)):
            return {"last=%d" % s}
        return set()
    return hits


def _end_hits(level, blocks):
    out = set()
    if blocks[0]["seqs"] and blocks[0]["trailing"] == 0:
        out.add("match ends at the block end")
    if blocks[1]["seqs"] and blocks[1]["trailing"] == 16:
        out.add("match ends 16 bytes before it")
    return out


def _raw_cases():
    d = b"".join(b for b, _ in raw_sweep_intended())
    yield Case("raw_sweep", "RAW threshold", d, 4096, LOW, {"RAW|coded neighbours, model agrees": LOW}, _raw_sweep_hits, small=False,
               why="levels 6-7: a PivCo literal section moves the threshold; the sweep's sequences are pinned at levels 1-5")
    text = (b"the quick brown fox jumps over the lazy dog; " * 100)[:4096]
    for s in (1, 15, 16, 17, 23, 24, 25, 63, 64, 65, 79, 80, 81):
        yield Case("tail_%d" % s, "RAW threshold", text + (b"ab" * 41)[:s], 4096, ALL, {"last=%d" % s: ALL}, _tail_hits(s))
    ph = rnd(40, 720)
    b0 = _filled(rnd(64, 721) + ph, 4096 - 240, 1) + rnd(200, 722) + ph
    b1 = _filled(rnd(64, 723) + ph, 4096 - 256, 1) + rnd(200, 724) + ph + rnd(16, 725)
    yield Case("match_at_end", "RAW threshold", b0 + b1, 4096, ALL,
               {"match ends at the block end": ALL, "match ends 16 bytes before it": ALL}, _end_hits)


# ---------------------------------------------------------------- skip acceleration
def _dry_hits(level, blocks):
    out = set()
    for k, b in zip((7, 8, 9), blocks):
        s = b["seqs"] or []
        if any(x[0] >= 64 * k for x in s[:-1]) and len(s) >= 4:
            out.add("%d dry chunks, then repeats" % k)
    return out


def _dry_cases():
    blocks = []
    for k in (7, 8, 9):
        r = random.Random(800 + k)
        ph = r.randbytes(64)
        out = bytearray(ph + ph)  # chunk 0 literals, chunk 1 a match
        out += r.randbytes(64 * k + 10)
        for _ in range(6):
            out += ph[:24] + r.randbytes(37)
        blocks.append(_filled(bytes(out), 4096, k))
    must = {"%d dry chunks, then repeats" % k: ALL for k in (7, 8, 9)}
    yield Case("dry_chunks", "skip acceleration", b"".join(blocks), 4096, ALL, must, _dry_hits)


# ---------------------------------------------------------------- dictionary
def _dict_hits(level, blocks):
    return {"first match reaches into the dictionary"} if all(b["type"] == 0 or b["seqs"] is None or (b["seqs"] and b["seqs"][0][0] == 0)
                                                              for b in blocks) and any(b["seqs"] for b in blocks) else set()


def _dict_cases():
    for n in (1, 63, 64, 65, 4097):
        d = b"a" if n == 1 else rnd(n, 900 + n)
        head = b"a" * 24 if n == 1 else d[-min(n, 48):]
        body = b"GET /index.html HTTP/1.1\r\nHost: example.org\r\n" * 100
        data = (head + body)[:4096] + (head + rnd(300, 950 + n) + body)[:2000]
        yield Case("dict_%d" % n, "dictionary", data, 4096, ALL, {"first match reaches into the dictionary": ALL}, _dict_hits, dict_=d)


# ---------------------------------------------------------------- job table
JOB_SIZES = (1, 63, 64, 4095, 4096, 4097)


def _job_cases(src):
    items, at = [], 0
    for s in JOB_SIZES:
        items.append(src[at:at + s])
        at += s
    assert at <= len(src)

    want = [n for s in JOB_SIZES for n in [4096] * (s // 4096) + ([s % 4096] if s % 4096 else [])]

    def hits(level, blocks):
        """one archive per item, cut into blocks of 4096: the parsed blocks of all items, in order, decode to exactly these sizes
        (a block with a PivCo section is not decoded by the model: its literal and sequence counts must still fit its size)"""
        if len(blocks) != len(want):
            return set()
        for b, n in zip(blocks, want):
            if (b["decoded"] is not None and b["decoded"] != n) or (b["decoded"] is None and b["n_lit"] + 5 * b["n_seq"] > n):
                return set()
            if n < 64 and b["type"] != 0:
                return set()
        return {"items of 1, 63, 64, 4095, 4096 and 4097 bytes"}
    yield Case("jobs", "job table", b"".join(items), 4096, ALL, {"items of 1, 63, 64, 4095, 4096 and 4097 bytes": ALL}, hits, items=items)


def build_cases():
    cases = []
    for gen in (_ll_cases, _ml_cases, _off_cases, _ring_cases, _period_cases, _rle_cases, _rle_small_cases, _raw_cases, _dry_cases, _dict_cases):
        cases += list(gen())
    by = {c.name: c for c in cases}
    cases += list(_job_cases(by["ml_small"].data[4096 - 100:] + by["ll_small"].data))
    assert len({c.name for c in cases}) == len(cases)
    return cases


_CASES = None


def cases():
    """the case list, built once"""
    global _CASES
    if _CASES is None:
        _CASES = build_cases()
    return _CASES


# ---------------------------------------------------------------- shared by the generator of the digests and both test modules
DIGESTS = "tests/golden/encoder_limits/digests.json"


def variants(case):
    """[(level, checksum)]: every level of the case; the checksum variant on the 4 KiB cases only"""
    out = [(lv, False) for lv in case.levels]
    if case.small:
        out += [(lv, True) for lv in case.levels]
    return out


def key(case, level, checksum=False):
    return "%s/L%d/bs%d%s" % (case.name, level, case.bs, "+ck" if checksum else "")


def pieces(case):
    """the byte strings that are compressed on their own: the batch items of the job-table case, else the whole input"""
    return case.items if case.items else [case.data]


FIELDS = ("type", "enc_lit", "enc_tok", "enc_off", "n_seq", "n_lit", "lit_sec")


def block_fields(b):
    """the header fields of one block (trailer allowed behind it), or the parse error as text"""
    import zxc_block_model as M
    try:
        p = M.parse_block(b[:8 + int.from_bytes(b[3:7], "little")])
        return [p[k] for k in FIELDS]
    except Exception as e:  # a malformed block must not hide the comparison that found it
        return ["unparsable: %r" % (e,)]


def digest(archives):
    """the recorded entry of one (case, level, block size): size and SHA-256 over the archives of all pieces, and per block its
    size, the first 8 hex digits of its SHA-256 and its header fields (FIELDS), to name and show the first block that differs"""
    import hashlib
    import zxc_block_model as M
    blocks = [b + (t or b"") for a in archives for b, t in zip(*M.split_blocks(a)[2:4])]
    return {"size": sum(len(a) for a in archives), "sha256": hashlib.sha256(b"".join(archives)).hexdigest(),
            "blocks": [[len(b), hashlib.sha256(b).hexdigest()[:8]] + block_fields(b) for b in blocks]}


def emu_archives(emu, case, level, checksum, dict_id_of):
    """the kernel on the CPU wave emulator: one archive per piece. dict_id_of(dict bytes) -> the id the file header carries"""
    did = dict_id_of(case.dict_) if case.dict_ else 0
    return [emu.encode(p, level, case.bs, checksum=checksum, dict_=case.dict_, dict_id=did) for p in pieces(case)]
