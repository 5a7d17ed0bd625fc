"""Crafted blocks that put the two sequence executors (run_sequences_lean in zxc_amd/csrc/zxc_seq_lean.inc and
run_sequences<DICT, GHI> in zxc_amd/csrc/zxc_decode_kernel.hip) at their internal limits, shared by
tests/test_decode_limits_cpu.py (the CPU wave emulator) and tests/test_gpu_decode_limits.py (the device). Not a conftest.

A case is a name, a list of (ll, ml, off), the literal bytes (seeded random, so a shifted or repeated group shows), the block
kind (GLO with 16-bit offsets, GLO with 8-bit offsets, GHI), the block size and optionally a dictionary prefix.
* Expected bytes: expand(), a plain LZ expansion over prefix + output written here. Never the product.
* Expected status: the oracle's block decoder (the reference Block API where a dictionary is in play), per route.
* Blocks with raw sections come from tests/golden/craft.py, blocks with RLE literals / 8-bit offsets chosen by the
  reference's rules from tests/zxc_block_model.serialise (enc_lit / enc_off are asserted).
* Every case names the path markers (ZXC_PATH ids of zxc_lds.h) it exists for, per route; the CPU test asserts them on the
  emulator after that case alone: (id, None) = reached, (id, n) = by exactly n lanes / events.

Routes (which executor a route reaches is itself asserted, see ROUTES and DESIGN.md):
  lean    the default two-pass launch: raw-section blocks in the lean kernel
  strict  the strict per-block capacity (zxc_decompress_block_safe): the full kernel alone; without a dictionary it runs the
          lean executor with strict = true
  dict    the dictionary kernel: run_sequences<true, GHI>. Cases without a dictionary of their own run here behind a dummy
          dictionary (offsets of a valid block never reach it; an offset in front of the block now lands in it, and the
          reference Block API says so)

Batch model used to place things (stated in the executors): a batch is the next 64 sequences; its first k that span at most
LEAN_TILE_MAX = 3040 bytes (full: TILE_MAX = 3584) are executed, a sequence longer than that alone is a "giant"; a batch takes
at most LEAN_VARINTS = 62 varints (full: 128). The lean executor flushes whole KiB at the end of a batch, so at the top of
the next one O.flushed = p & ~1023, and a source is "far" when it starts below ring_lo = round_up(tile_end, 16) - 4096.
"""
import dataclasses
import functools
import os
import random
import re

import numpy as np

import decode_plan_cases as P
import zxc_block_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAN_TILE_MAX, TILE_MAX, RING = 3040, 3584, 4096
LIT_MED = MATCH_MED = 128
PAD = 2112  # a block's capacity is block_size + PAD

ROUTES = ("lean", "strict", "dict")
DUMMY_DICT = random.Random(0xD1C7).randbytes(777)  # (an odd size: the seam is at no aligned position)


def path_ids():
    """name -> number of enum zxc_path_id (zxc_amd/csrc/zxc_lds.h), read from the header."""
    src = open(os.path.join(ROOT, "zxc_amd", "csrc", "zxc_lds.h")).read()
    body = re.search(r"enum zxc_path_id \{(.*?)\};", src, re.S).group(1)
    names = [n.strip() for n in body.replace("\n", " ").split(",") if n.strip()]
    assert names[-1] == "ZXC_PATH_COUNT"
    return {n: i for i, n in enumerate(names[:-1])}


# ------------------------------------------------------------------ a case
@dataclasses.dataclass
class LCase:
    name: str
    family: str
    seqs: list
    lits: bytes
    kind: str = "glo16"        # glo16 | glo8 (craft.py) | glo8m (8-bit offsets chosen by zxc_block_model.serialise) | ghi
    bs: int = 4096
    out_len: int = None        # the job's out_len (None: what the block decodes to)
    dict_: bytes = None        # a dictionary of the case's own: the case runs on the dict route only
    rle: bool = False          # built by zxc_block_model.serialise, which must choose RLE literals
    ext: bytes = None          # the extras section instead of the sequences' varints (damaged streams)
    valid: bool = True         # expand() defines the bytes (False: the verdict alone is checked)
    paths: dict = dataclasses.field(default_factory=dict)  # route -> [(id name, count or None)]
    routes: tuple = ROUTES

    def need(self, route, *ids):
        for i in ids:
            self.paths.setdefault(route, []).append(i if isinstance(i, tuple) else (i, None))
        return self

    def both(self, lean_ids=(), dict_ids=()):
        """lean_ids on the lean and strict routes (one executor), dict_ids on the dict route"""
        for r in ("lean", "strict"):
            self.need(r, *lean_ids)
        return self.need("dict", *dict_ids)


def expand(seqs, lits, prefix=b""):
    """The block's bytes: plain LZ expansion over prefix + output; trailing literals last."""
    out, lp = bytearray(prefix), 0
    for ll, ml, off in seqs:
        out += lits[lp:lp + ll]
        lp += ll
        assert 1 <= off <= len(out), ("offset in front of the data", ll, ml, off, len(out))
        if off >= ml:
            out += out[len(out) - off:len(out) - off + ml]
        else:
            for _ in range(ml):
                out.append(out[-off])
    out += lits[lp:]
    return bytes(out[len(prefix):])


def build_block(oracle, c: LCase) -> bytes:
    import craft
    if c.rle or c.kind == "glo8m":
        blk = M.serialise(c.seqs, c.lits, len(expand(c.seqs, c.lits)), False, 3)
        p = M.parse_block(blk)
        assert p["type"] == M.GLO and p["enc_lit"] == (1 if c.rle else 0) and p["enc_off"] == 1, (c.name, p["type"], p["enc_lit"], p["enc_off"])
        return blk
    if c.kind == "ghi":
        return craft.ghi_block(oracle, c.seqs, c.lits, ext=c.ext)
    return craft.glo_block(oracle, c.seqs, c.lits, off8=c.kind == "glo8", ext=c.ext)


def seq_at(c: LCase, pos: int):
    """(index, (ll, ml, off), 'literal' | 'match') of the sequence that produces output byte pos"""
    at = 0
    for i, (ll, ml, off) in enumerate(c.seqs):
        if pos < at + ll:
            return i, (ll, ml, off), "literal"
        if pos < at + ll + ml:
            return i, (ll, ml, off), "match"
        at += ll + ml
    return len(c.seqs), None, "trailing literal"


# ------------------------------------------------------------------ packing cases into one guarded job table
def verdict(oracle, api, blk, c: LCase, route, checksum=False):
    """The route's reference: the oracle's block decoder at the launch's capacity (block_size + 2112; the strict route: the
    block size itself, exact checks), or the reference Block API with the dictionary. The Block API derives its decoder's
    capacity from dst_capacity rounded up to a block size: dst_capacity = block_size gives the kernels' block_size + 2112,
    and it then refuses what decodes to more than dst_capacity, so dictionary cases decode to at most the block size."""
    if route == "dict":
        d = c.dict_ if c.dict_ is not None else DUMMY_DICT
        r, b = api.decompress_block(blk, c.bs, checksum=checksum, dict_=d)
        assert r != -2, (c.name, "decodes to more than the block size: not a case for the dictionary route")
        return r, b
    if route == "strict":
        return oracle.decode_block(blk, c.bs, cap=c.bs, checksum=checksum, strict_tail=True)
    return oracle.decode_block(blk, c.bs, checksum=checksum)


def cross_check(oracle, ref, api, blk, c: LCase, route, checksum, r, b):
    """The oracle's verdict against the reference itself: the Block API, or zxc_decompress over a one-block frame where the
    block decodes to more than its block size (which the Block API refuses). A disagreement is an oracle bug."""
    import craft
    if route == "strict":
        r2, b2 = api.decompress_block(blk, c.bs, checksum=checksum, safe=True)
    elif r <= c.bs:
        r2, b2 = api.decompress_block(blk, c.bs, checksum=checksum)
        if r2 == -2:  # (the oracle says an error, the reference decodes more than a block: settle it on a frame)
            r2, b2 = ref.decompress(craft.frame(oracle, [blk], c.bs.bit_length() - 1, c.bs + PAD, checksum=checksum), c.bs + PAD, checksum)
            r2 = r if r2 < 0 and r < 0 else r2
    else:
        r2, b2 = ref.decompress(craft.frame(oracle, [blk], c.bs.bit_length() - 1, r, checksum=checksum), r, checksum)
    assert r2 == r and (r < 0 or b2 == b), (c.name, route, "oracle and reference disagree", r, r2)


def pack(oracle, ref, cases, route, checksum=False, label="", align0=0):
    """-> (decode_plan_cases.Case, the LCases in job order). One job per case, block i at comp_off = (align0 + i) mod 4 (the
    four byte alignments of a payload in the compressed buffer: lit_ph). All cases share one block size."""
    import craft
    import oracle_py
    assert cases and len({c.bs for c in cases}) == 1 and route in ROUTES
    api = oracle_py.BlockApi(ref.lib) if ref is not None else None
    assert route != "dict" or api is not None, "dictionary verdicts come from the reference Block API"
    blob, jobs = bytearray(), np.zeros(len(cases), dtype=P.JOB_DTYPE)
    rc, want = np.zeros(len(cases), dtype=np.int32), []
    for i, c in enumerate(cases):
        blk = build_block(oracle, c)
        if checksum:
            blk = craft.with_trailer(oracle, blk)
        while len(blob) % 4 != (align0 + i) % 4:
            blob.append(0xEE)
        r, b = verdict(oracle, api, blk, c, route, checksum)
        if api is not None and route != "dict" and c.dict_ is None:
            # the oracle against the reference Block API (a disagreement is an oracle bug)
            cross_check(oracle, ref, api, blk, c, route, checksum, r, b)
        if c.valid:
            exp = expand(c.seqs, c.lits, (c.dict_ if c.dict_ is not None else DUMMY_DICT) if route == "dict" else b"")
            assert r == len(exp) and b == exp, (c.name, route, "the reference's verdict differs from the plain expansion", r, len(exp))
        else:
            exp = b if r >= 0 else b""
        n = len(exp) if c.out_len is None else c.out_len
        jobs[i] = (len(blob), 0, len(blk), n)
        blob += blk
        rc[i] = r
        want.append(exp if r >= 0 else b"")
    if api is not None:
        api.close()
    d = None
    if route == "dict":
        ds = {c.dict_ for c in cases}
        assert len(ds) == 1, "one dictionary per launch"
        d = ds.pop() or DUMMY_DICT
    return P.Case(bytes(blob), jobs, cases[0].bs, checksum, rc, want, dict_=d, label=label or f"{cases[0].family}/{route}"), list(cases)


def explain(case: P.Case, lcases, out: np.ndarray, status):
    """For a failed check: the first job whose status or bytes differ, the first differing byte and its sequence."""
    raw = np.asarray(out, dtype=np.uint8).tobytes()
    for i, c in enumerate(lcases):
        if int(status[i]) != int(case.want_rc[i]):
            return f"{c.name}: status {int(status[i])}, expected {int(case.want_rc[i])}"
        if case.want_rc[i] < 0:
            continue
        o, n = int(case.jobs["out_off"][i]), min(int(case.jobs["out_len"][i]), int(case.want_rc[i]))
        got, exp = raw[o:o + n], case.want[i][:n]
        if got != exp:
            at = next(k for k in range(n) if got[k] != exp[k])
            si, s, what = seq_at(c, at)
            return f"{c.name}: byte {at} is {got[at]:#04x}, expected {exp[at]:#04x}; {what} of sequence {si} {s}"
    return "no job differs (a guard region changed)"


def groups(cases, route):
    """The cases of one route by (dictionary, block size): one job table each."""
    g = {}
    for c in cases:
        if route in c.routes:
            g.setdefault((c.dict_, c.bs), []).append(c)
    return list(g.values())


# ------------------------------------------------------------------ building sequences
class B:
    """Sequence list under construction: tracks the output position, draws literals at the end."""

    def __init__(self, seed):
        self.seqs, self.pos, self.seed, self.trail = [], 0, seed, 0

    def add(self, ll, ml, off, bad=False):
        assert ml >= 5 and (bad or 1 <= off <= self.pos + ll), (ll, ml, off, self.pos)
        self.seqs.append((ll, ml, off))
        self.pos += ll + ml
        return self

    def src(self, ll, ml, s):
        """a match whose source starts at output position s"""
        return self.add(ll, ml, self.pos + ll - s)

    @property
    def M(self):
        return self.pos

    def fill(self, n_batches, per=30):
        """n_batches whole batches of 64 plain sequences of `per` bytes (1920 a batch): no varint (ll <= 14, ml <= 19), no tile
        cut, so the next sequence opens a batch at p = pos and the lean executor has flushed pos & ~1023."""
        assert len(self.seqs) % 64 == 0 and 27 <= per <= 30
        r = random.Random(self.seed ^ 0x5EED)
        for _ in range(64 * n_batches):
            ll = 14 - r.randrange(0, 4)
            self.add(ll, per - ll, r.randrange(1, min(self.pos + ll, 900) + 1) if self.pos else ll)
        return self

    def fill_until(self, target):
        """whole plain batches up to exactly output position `target` (the last one with its lengths adjusted)"""
        assert len(self.seqs) % 64 == 0
        while target - self.pos >= 1920 + 64 * 22:
            self.fill(1)
        left = target - self.pos
        assert 64 * 20 <= left <= 64 * 33, left
        for i in range(64):
            n = left // (64 - i)
            left -= n
            ll = min(14, n - 6)
            self.add(ll, n - ll, 1 + (i % 9))
        assert self.pos == target
        return self

    def fill_to(self, n_bytes):
        return self.fill((n_bytes + 1919) // 1920)

    def pad_batch(self):
        """plain short sequences up to the next multiple of 64 sequences"""
        while len(self.seqs) % 64:
            self.add(3, 6, 2)
        return self

    def case(self, name, family, **kw):
        n_lit = sum(s[0] for s in self.seqs) + self.trail
        lits = random.Random(self.seed).randbytes(n_lit)
        kw.setdefault("bs", _bs_for(self.pos + self.trail))  # (the smallest block size the block fits, unless the case says)
        return LCase(name, family, list(self.seqs), lits, **kw)


def _phase(b, want, lo=1):
    """a literal length >= lo that makes the match start at phase `want`"""
    ll = lo
    while (b.pos + ll) & 3 != want:
        ll += 1
    return ll


def _bs_for(n):
    for bs in (4096, 65536, 131072):
        if n <= bs:
            return bs
    raise AssertionError(n)


# ------------------------------------------------------------------ families
def fam_match_len():
    out = []
    near = (300, 301, 302, 303)          # not overlapping; the four source phases against one destination phase
    ovl = (16, 17, 18, 19, 20)           # overlapping with a period of at least one 16-byte group
    for ml in (16, 17, 32, 33, 127, 128, 129, 130, 132, 133, 134, 147, 148, 149):
        for tag, offs in (("near", near), ("ovl16", ovl)):
            b = B(1000 + ml).add(330, 5, 9)
            for off in offs:
                for ph in range(4):  # (a literal run of at least the period: the source depends on no earlier match)
                    b.add(_phase(b, ph, off if off <= 20 else 1), ml, off)
            b.trail = 3
            c = b.case(f"ml{ml}/{tag}", "match_len", bs=_bs_for(b.pos + 3))
            if ml <= MATCH_MED:
                c.both(["L_STEPABLE"], ["F_STEPABLE"])
            else:
                c.both(["L_LONG"], ["F_LONG"])
                if tag == "ovl16":
                    c.both(["C_MATCH_DOUBLE"], ["C_MATCH_DOUBLE"])
            out.append(c)
    # the bytewise rule (overlap, off < 16, ml <= 32) and its two edges
    for ml in (31, 32, 33, 34):
        b = B(1100 + ml).add(40, 5, 9)
        for off in (1, 2, 3, 15, 16):
            for ph in range(4):
                b.add(_phase(b, ph, off), ml, off)
        c = b.case(f"ml{ml}/bytewise", "match_len")
        # off 16 is stepable at every ml; off < 16: bytewise up to 32, the whole-wave copy beyond
        c.both(["L_STEPABLE", "L_BYTEWISE" if ml <= 32 else "L_LONG"], ["F_STEPABLE", "F_BYTEWISE" if ml <= 32 else "F_LONG"])
        if ml == 32:
            c.both([("L_LONG", 0)], [("F_LONG", 0)])
        if ml == 33:
            c.both([("L_BYTEWISE", 0)], [("F_BYTEWISE", 0)])
        out.append(c)
    return out


LL_SET = (0, 12, 13, 14, 15, 16, 17, 29, 30, 31, 32, 33, 47, 48, 49, 127, 128, 129, 142, 143, 144, 145)


def fam_lit_len():
    out = []
    for v in range(4):  # v shifts the literal stream's phase of every run
        b = B(2000 + v).add(1 + v, 5, 1)
        for ll in LL_SET:
            for ph in range(4):
                if (b.pos & 3) != ph:           # a spacer match: the run lands at est & 3 == ph
                    ml = 5
                    while (b.pos + ml) & 3 != ph:
                        ml += 1
                    b.add(0, ml, 1)
                b.add(ll, 5, 1)
        b.trail = 5
        c = b.case(f"ll/v{v}", "lit_len", bs=65536)
        c.both(["L_LIT_GROUP", "L_LIT_5TH", "L_LIT_LONG"], ["F_LIT_GROUP", "F_LIT_LONG"])
        out.append(c)
    # the first run right behind the 12-byte sub-header: the lit_al / litm4 reads in front of the stream
    for ll in (1, 3, 13, 16, 17, 33):
        b = B(2100 + ll).add(ll, 5, 1).add(2, 7, 3)
        b.trail = 1
        out.append(b.case(f"first_run/{ll}", "lit_len").both(["L_LIT_GROUP"], ["F_LIT_GROUP"]))
    return out


def _varint_batch(seed, n_seq, plan, kind="glo16", tail=8):
    """n_seq sequences; plan[i] = (extra ll beyond the escape or None, extra ml beyond the escape or None)"""
    esc = 255 if kind == "ghi" else 15
    b = B(seed)
    for i in range(n_seq):
        xl, xm = plan.get(i, (None, None))
        ll = esc + xl if xl is not None else 1 + (i % 3)
        ml = 5 + esc + xm if xm is not None else 5 + (i % 4)
        b.add(ll, ml, 1 + (i % 7) if b.pos + ll > 8 else 1)
    for _ in range(tail):
        b.add(2, 6, 2)
    return b


def fam_varints():
    out = []
    # n single-byte varints in the first batch of 64: the lean executor takes at most 62
    for n in (61, 62, 63, 64):
        for mode in ("ll", "ml"):
            plan = {i: ((i % 5, None) if mode == "ll" else (None, i % 6)) for i in range(n)}
            c = _varint_batch(3000 + n, 64, plan).case(f"{n}x{mode}", "varints", bs=65536)
            c.both(["L_VARINT_FAST", ("L_VARINT_CUT", None if n > 62 else 0)], ["F_VARINT_FAST"])
            out.append(c)
    # both escapes on one sequence, straddling the cut: varints 62 and 63 belong to sequence 61
    plan = {i: (i % 5, None) for i in range(61)}
    plan[61] = (3, 4)
    out.append(_varint_batch(3100, 64, plan).case("straddle_62_63", "varints", bs=65536).both(["L_VARINT_CUT"], ["F_VARINT_FAST"]))
    plan = {i: (i % 5, None) for i in range(60)}
    plan[60] = (3, 4)   # varints 61, 62: exactly fits
    out.append(_varint_batch(3101, 64, plan).case("both_61_62", "varints", bs=65536).both([("L_VARINT_CUT", 0)], ["F_VARINT_FAST"]))
    # 127, 128 varints in one batch and 130 over 65 sequences: the full executor's tables hold 128
    for n in (127, 128, 129, 130):
        plan = {i: (i % 5, i % 3) for i in range(n // 2)}
        if n & 1:
            plan[n // 2] = (2, None)
        c = _varint_batch(3200 + n, max(64, (n + 1) // 2), plan).case(f"{n}_varints", "varints", bs=65536)
        out.append(c.both(["L_VARINT_CUT"], ["F_VARINT_FAST"]))
    # one two-byte varint among single-byte ones, first and last of the batch; three-byte values
    for where in (0, 9):
        plan = {i: (i % 5, None) for i in range(0, 20, 2)}
        plan[2 * where] = (128 + 7, None)
        out.append(_varint_batch(3300 + where, 64, plan).case(f"two_byte_at_{where}", "varints", bs=65536)
                   .both(["L_VARINT_GENERAL", "C_VARINT_TAIL"], ["F_VARINT_GENERAL"]))
    plan = {3: (16384 + 5, None), 5: (None, 16384 + 900), 7: (1, 129)}
    out.append(_varint_batch(3400, 20, plan).case("three_byte", "varints", bs=65536).both(["L_VARINT_GENERAL", "L_GIANT"], ["F_VARINT_GENERAL", "F_GIANT"]))
    # ext_size 0 and 1 (twelve sequences: no pad behind the extras)
    out.append(_varint_batch(3500, 12, {}, tail=0).case("ext0", "varints").both([("L_VARINT_FAST", 0), ("L_VARINT_GENERAL", 0)], []))
    out.append(_varint_batch(3501, 12, {11: (4, None)}, tail=0).case("ext1", "varints").both(["L_VARINT_FAST"], ["F_VARINT_FAST"]))
    # GHI: the escapes at 255
    for k, plan in enumerate(({5: (0, None), 6: (None, 0), 7: (1, 1)}, {i: (i % 3, None) for i in range(63)}, {2: (300, None), 3: (None, 200)})):
        c = _varint_batch(3600 + k, 64, plan, kind="ghi").case(f"ghi_{k}", "varints", kind="ghi", bs=65536)
        ids = (["L_VARINT_FAST"], ["F_VARINT_FAST"]) if k < 2 else (["L_VARINT_GENERAL"], ["F_VARINT_GENERAL"])
        out.append(c.both(*ids).both(["X_LEAN_GHI"], ["X_FULL_GHI"]))
    for k in (254, 255, 256):  # ll and ml around the GHI escape
        b = B(3700 + k).add(k, 5, 1).add(2, k + 5 - 1, 3).add(k, k + 5, 9)
        out.append(b.case(f"ghi_esc_{k}", "varints", kind="ghi").both(["X_LEAN_GHI"], ["X_FULL_GHI"]))
    return out


def fam_tile():
    out = []
    for span in (3039, 3040, 3041, 3583, 3584, 3585):
        for kind, tail in (("glo16", 0), ("ghi", 0), ("glo16", 26)):
            b = B(4000 + span)
            for _ in range(7):
                b.add(300, 120, 25)        # 2940 bytes in 7 sequences (GLO: 14 varints, far from the varint cut)
            b.add(span - 2940 - 20, 20, 7)  # sequence 7 ends the span exactly
            for _ in range(tail):
                b.add(3, 7, 2)
            b.trail = 2 if tail else 0
            c = b.case(f"span{span}/{kind}/{tail}", "tile", kind=kind, bs=65536)
            if tail == 0:  # the block ends with the span: a cut happens exactly when the span does not fit the tile
                c.both([("L_TILE_CUT", 1 if span > LEAN_TILE_MAX else 0), ("L_VARINT_CUT", 0)], [("F_TILE_CUT", 1 if span > TILE_MAX else 0)])
                if span > LEAN_TILE_MAX:   # the cut leaves seq_base = 7: the 4x condition of the group it cuts is carried over
                    c.need("lean", "L_CARRY4X")
                if span > TILE_MAX:
                    c.need("dict", "F_CARRY4X")
            else:
                c.both(["L_TILE_CUT"], ["F_TILE_CUT"] if span + 262 > TILE_MAX else [])
            out.append(c)
    # The room LEAN_TILE_MAX leaves in the ring: up to 1023 unflushed bytes of earlier batches + the tile + the partial chunk.
    # p = 8192 + 1023, a batch whose first 8 sequences span exactly 3040 bytes and whose next one would take it to 3100:
    # 1023 + 3100 bytes do not fit the ring (1023 + 3072 still would: LEAN_TILE_MAX has 32 bytes of slack).
    b = B(4050).fill_until(8192 + 1023)
    for _ in range(7):
        b.add(300, 120, 25)
    b.add(80, 20, 7).add(14, 46, 3000)
    for _ in range(20):
        b.add(3, 7, 2)
    out.append(b.case("ring_room", "tile").both([("L_TILE_CUT", 1)], []))
    # a cut that leaves seq_base off a multiple of 4, then a varint-extended sequence near the capacity (4096 + 2112):
    # whether the reference's 4x-batch reserve refuses it comes from the oracle
    for big in (2900, 3000, 3050, 3100, 3120, 3140):
        for at in (8, 9, 10, 11):
            b = B(4100 + big + at)
            for _ in range(7):
                b.add(300, 120, 25)
            b.add(81, 20, 7)           # 3041: the cut, k = 7
            while len(b.seqs) < at:
                b.add(2, 6, 2)
            b.add(big, 5, 11)
            for _ in range(6):
                b.add(1, 5, 1)
            c = b.case(f"carry4x/{big}@{at}", "tile", valid=False, routes=("lean", "strict"), bs=4096)
            c.need("lean", "L_TILE_CUT", "L_CARRY4X").need("strict", "L_TILE_CUT")
            out.append(c)
    return out


def fam_giant():
    out = []

    def g(name, b, lean, full, **kw):
        c = b.case(name, "giant", bs=_bs_for(b.pos + b.trail), **kw)
        out.append(c.both(lean, full))

    for ll in (3041, 3585, 5000):
        pieces = 1 if ll <= TILE_MAX else 2
        g(f"ll{ll}/first", B(5000 + ll).add(ll, 5, 1).add(2, 6, 2), ["L_GIANT", ("L_GIANT_LIT_PIECE", pieces)],
          ["F_GIANT", ("F_GIANT_LIT_PIECE", pieces)] if ll > TILE_MAX else [("F_GIANT", 0), "F_LIT_LONG"])
        g(f"ll{ll}/last", B(5010 + ll).add(9, 6, 2).add(2, 6, 2).add(ll, 5, 1), ["L_GIANT"], ["F_GIANT"] if ll > TILE_MAX else ["F_LIT_LONG"])
        b = B(5020 + ll)
        for _ in range(50):
            b.add(12, 18, 9)           # 1500 bytes: one KiB flushed, a partial one behind it
        g(f"ll{ll}/behind_partial_kib", b.add(ll, 5, 1).add(4, 9, 100), ["L_GIANT"], ["F_GIANT"] if ll > TILE_MAX else ["F_LIT_LONG"])
    for ml in (3041, 4096, 4097, 9000):
        for off in (1, 3, 10):
            g(f"ml{ml}/off{off}", B(5100 + ml + off).add(10, ml, off).add(3, 6, 2), ["L_GIANT", "L_GIANT_MATCH", "C_MATCH_DOUBLE"],
              ["F_GIANT", "F_GIANT_MATCH"] if ml + 10 > TILE_MAX else ["F_LONG"])
        for off in (4095, 4096, 4097):
            b = B(5200 + ml + off).fill(3)     # 5760 bytes
            g(f"ml{ml}/off{off}", b.add(7, ml, off).add(3, 6, 2), ["L_GIANT", "L_GIANT_MATCH"], ["F_GIANT_MATCH"] if ml + 7 > TILE_MAX else ["F_LONG"])
        g(f"ml{ml}/off_eq_ll", B(5300 + ml).add(3041, ml, 3041).add(3, 6, 2), ["L_GIANT", "L_GIANT_MATCH", "L_GIANT_LIT_PIECE"], ["F_GIANT_MATCH"])
    g("both", B(5400).add(5000, 9000, 10).add(3, 6, 2), ["L_GIANT", ("L_GIANT_LIT_PIECE", 2), "L_GIANT_MATCH"], ["F_GIANT", "F_GIANT_MATCH"])
    # a far match directly behind a giant, reading the giant's bytes back from memory
    for s in (4, 505, 777):
        b = B(5500 + s).add(5000, 5, 1)
        g(f"far_behind_giant/{s}", b.src(0, 40, s).src(3, 16, s + 100), ["L_GIANT", ("L_FAR_GROUP", 2)], ["F_FAR_PREFETCH"])
    return out


def fam_far():
    """More than 4 KiB of earlier output (whole plain batches), then one batch whose sources lie behind the ring."""
    out = []

    def start(seed):
        return B(seed).fill(4)  # 7680 bytes: O.flushed = 7168 at the top of the next batch; ring_lo >= 3584 + the batch's span

    # source start 0..5: the qa >= 4 guard (the dword-aligned group load reads 4 bytes in front of a phase-shifted source)
    b = start(6000)
    for s in range(6):
        b.src(_phase(b, (s + 1) & 3), 20, s)
    out.append(b.case("qa0_5", "far").need("lean", ("L_FAR_NO_QA4", 4), ("L_FAR_GROUP", 2)).need("strict", ("L_FAR_NO_QA4", 4), ("L_FAR_GROUP", 2))
               .need("dict", "F_FAR_PREFETCH", "F_LONG"))
    # The source ends 1 below, exactly at and 1 above O.flushed of this batch: bytes the previous batch's flush wrote (the
    # read-back relies on a wave's stores and loads reaching L2 in program order). A source that starts behind the ring
    # (below round_up(tile_end, 16) - 4096) and yet ends at the flushed mark (p & ~1023) needs a nearly full tile behind a
    # p just below a KiB boundary, and a match of more than 4097 - 3040 - 1023 = 34 bytes.
    for ml in (64, 128):
        b = B(6010 + ml).fill_until(8192 + 1020)
        for d in (-1, 0, 1):
            b.src(_phase(b, d & 3), ml, 8192 + d - ml)
        for _ in range(6):
            b.add(300, 120, 25)
        b.add(8192 + 1020 + 3038 - b.pos - 20, 20, 7)   # the tile ends 3038 bytes behind p; whatever follows is cut off
        b.add(3, 6, 2)
        c = b.case(f"flushed_edge/ml{ml}", "far")
        out.append(c.both([("L_FAR_GROUP", 2), ("L_FAR_NO_FLUSHED", 1), ("L_TILE_CUT", 1)], ["F_FAR_PREFETCH"]))
    # lengths x destination phase x source phase
    for ml in (5, 12, 13, 16, 17, 33, 128, 129):
        b = start(6100 + ml)
        for dph in range(4):
            for sph in range(4):
                b.src(_phase(b, dph), ml, 1000 + 52 * (4 * dph + sph) + sph)
        c = b.case(f"phases/ml{ml}", "far", bs=_bs_for(b.pos))
        if ml <= MATCH_MED:
            # (full executor: two groups are requested early, a third and later ones inside the copy loop)
            c.both([("L_FAR_GROUP", 16)] + (["L_FAR_5TH"] if ml > 12 else []), [("F_FAR_PREFETCH", 16)] + (["F_FAR_GROUP"] if ml >= 33 else []))
        else:
            c.both([("L_FAR_NO_ML", 16), ("L_FAR_GROUP", 0), "L_LONG_FAR", "C_COPY_FAR"], ["F_LONG", "C_COPY_FAR"])
        out.append(c)
    # offsets around the ring size, and the largest
    for off in (4064, 4080, 4095, 4096, 4097, 4112, 8192, 65535, 65536):
        for kind in ("glo16", "ghi"):
            bs = 131072 if off >= 65535 else 65536
            b = B(6200 + off)
            b.fill(2 + (off + 1919) // 1920)
            for ph in range(4):
                b.add(_phase(b, ph), 19 + ph, off)
            b.pad_batch().fill(1)
            b.add(2, 40, off)
            c = b.case(f"off{off}/{kind}", "far", kind=kind, bs=bs)
            out.append(c.both(["L_FAR_GROUP"], ["F_FAR_PREFETCH"]))
    # a batch in which all 64 sequences are far, and one in which exactly one is
    b = start(6300)
    for i in range(64):
        b.src(1 + (i & 3), 9 + (i % 23), 100 + 61 * i)
    out.append(b.case("all64", "far").both([("L_FAR_GROUP", 64)], [("F_FAR_PREFETCH", 64)]))
    b = start(6301)
    for i in range(64):
        b.src(3, 21, 2000 + i) if i == 29 else b.add(4 + (i & 3), 7 + (i % 9), 3 + (i % 5))
    out.append(b.case("exactly_one", "far").both([("L_FAR_GROUP", 1)], [("F_FAR_PREFETCH", 1)]))
    # the slot-edge guard: out_len is shorter than the block, the source group reaches the last 4 / 16 / 20 bytes of the
    # slot (round_up(out_len, 16)); only the bytes below out_len are defined
    for back in (4, 16, 20, 36):
        b = start(6400 + back)
        out_len = 2000
        ml = 16
        b.src(_phase(b, 1), ml, out_len - back - ml + 4)
        b.src(_phase(b, 2), 11, 900)
        c = b.case(f"slot_edge/{back}", "far", out_len=out_len, bs=65536)
        # L_FAR_GROUP and F_FAR_PREFETCH sit inside the guarded branches: their exact counts pin the guards' decisions (the
        # second match always stays far; the first does once its last group's load, + 4 bytes, fits the slot. The full
        # executor asks for sg + 32 <= out_pad, which holds from 20 bytes back.)
        c.both([("L_FAR_NO_EDGE", 1), ("L_FAR_GROUP", 1)] if back <= 20 else [("L_FAR_NO_EDGE", 0), ("L_FAR_GROUP", 2)],
               [("F_FAR_PREFETCH", 1 if back < 20 else 2)])
        out.append(c)
    return out


def fam_deps():
    out = []
    # chains: every match's source is exactly the match in front of it
    for depth in (1, 2, 3, 63):
        b = B(7000 + depth).add(40, 14, 20)
        for _ in range(depth):
            b.add(0, 14, 14)
        b.trail = 4
        c = b.case(f"chain{depth}", "deps")
        lean = ["L_REDIRECT0"] + (["L_REDIRECT1"] if depth >= 2 else [("L_REDIRECT1", 0)])
        full = ["F_REDIRECT0"] + (["F_REDIRECT1"] if depth >= 2 else [("F_REDIRECT1", 0)])
        out.append(c.both(lean, full))
    # a source spanning exactly 1, 2 and 3 earlier matches of the batch (literals between them: no redirect)
    for n in (1, 2, 3):
        b = B(7100 + n).add(30, 8, 9)
        for _ in range(3):
            b.add(2, 8, 5)
        b.src(1, 10 * n, b.pos + 1 - 10 * n)   # the last 10 n bytes: n (literals + match) units
        b.trail = 1
        c = b.case(f"span{n}", "deps")
        out.append(c.both([("L_WAIT_ALL", 1 if n == 3 else 0)], []))
    # ... over three matches of which the last finishes two rounds late (a chain A <- B <- C), while more than SPARSE_MAX
    # sequences stay pending (a twelve-deep chain in front), so the rounds and not the in-order sparse finish resolve it
    b = B(7150).add(30, 8, 9)
    for _ in range(12):
        b.add(0, 12, 5)
    b.add(24, 8, 20)                      # A: its source lies in its own literals
    b.add(2, 9, 6).add(2, 9, 6)           # B reads A's tail, C reads B's tail (overlapping: no redirect)
    b.src(1, 26, b.pos + 1 - 28)          # over A's tail, B and C
    b.trail = 2
    out.append(b.case("span3_late", "deps").both([("L_WAIT_ALL", 1)], []))
    # a source inside ONE earlier match but beyond that match's first period: not a redirect
    b = B(7160).add(20, 40, 10).add(0, 12, 14).add(0, 9, 30).add(3, 6, 2)
    out.append(b.case("beyond_first_period", "deps").both([("L_REDIRECT0", 0), ("L_REDIRECT1", 0)], [("F_REDIRECT0", 0), ("F_REDIRECT1", 0)]))
    # a source that contains an earlier match's literal run
    b = B(7200).add(30, 8, 9).add(6, 8, 5).src(0, 12, 40).add(2, 6, 3)
    out.append(b.case("over_literals", "deps").both(["L_STEPABLE"], ["F_STEPABLE"]))
    # a redirect whose new source falls behind the ring: the match in front copies from far away
    b = B(7300).fill(4)
    b.src(2, 30, 1000).add(0, 16, 20).add(0, 9, 9)
    c = b.case("redirect_behind_ring", "deps")
    # (exact counts: a redirect that went behind the ring after all would be one more L_REDIRECT0)
    out.append(c.both([("L_FAR_GROUP", 1), ("L_REDIRECT_NO_RING", 2), ("L_REDIRECT0", 1)], []))
    # 8 and 9 sequences left after round 0 (SPARSE_MAX = 8): each reads the first match and the literals in front of it
    for n in (8, 9):
        b = B(7400 + n).add(20, 12, 7)
        first_m = 20
        for i in range(n):
            b.src(3, 8 + (i % 4), first_m - 3 + (i % 3))   # [17..19, <= 30): literals and match of sequence 0 only
        b.trail = 2
        c = b.case(f"pending{n}", "deps")
        out.append(c.both([("L_SPARSE", 1 if n == 8 else 0), ("L_SPARSE_PLAIN", 8 if n == 8 else 0)],
                          [("F_SPARSE", 1 if n == 8 else 0), ("F_SPARSE_PLAIN", 8 if n == 8 else 0)]))
    # the sparse finish with overlapping matches: every period 1..20 at the longest length its copy routine takes there
    # (t = ml - 1 is where the float-reciprocal modulo is least exact)
    for lo in (1, 9, 16):
        for ml_of in ("max", "max-1"):
            b = B(7500 + lo + len(ml_of)).add(40, 12, 7)
            offs = range(lo, lo + 8) if lo < 16 else (16, 17, 18, 19, 20)
            for off in offs:
                ml = (32 if off < 16 else 128) - (ml_of != "max")
                b.add(0, ml, off)          # reads the tail of the match in front: pending after round 0, in stream order
            b.trail = 3
            c = b.case(f"sparse_ovl/{lo}/{ml_of}", "deps")
            n = len(offs)   # every one of them through the sparse finish's modulo, none through the rounds
            out.append(c.both([("L_SPARSE", 1), ("L_SPARSE_OVL", n)], [("F_SPARSE", 1), ("F_SPARSE_OVL", n)]))
    # sparse finish of matches that do not overlap, and of long ones (whole-wave copy)
    b = B(7600).add(40, 12, 7)
    for i in range(4):
        b.add(0, 12, 12 + i)
    b.add(0, 40, 3).add(0, 200, 100)
    out.append(b.case("sparse_mixed", "deps").both(["L_SPARSE", "L_SPARSE_PLAIN", "L_SPARSE_COOP"], ["F_SPARSE", "F_SPARSE_PLAIN", "F_SPARSE_COOP"]))
    return out


def fam_small():
    out = []
    for n in (0, 1, 15, 16, 17):
        b = B(8000 + n)
        b.trail = n
        out.append(b.case(f"no_seq/{n}", "small").both([], []))
    out.append(B(8050).add(3, 5, 2).case("one_seq", "small").both(["L_PARTIAL_CHUNK"], ["F_PARTIAL_CHUNK"]))
    for n in range(1, 34):  # far_en = round_up(out_len, 16) >= 32 turns on at 17
        b = B(8100 + n)
        if n >= 8:
            b.add(2, 5, 2 if n & 1 else 1)
            b.trail = n - 7
        else:
            b.trail = n
        c = b.case(f"out_len{n}", "small")
        out.append(c.both(["L_PARTIAL_CHUNK"] if n & 15 else [("L_PARTIAL_CHUNK", 0)], ["F_PARTIAL_CHUNK"] if n & 15 else []))
    # an out_len shorter than what the block decodes to (the status is the decoded size; bytes up to out_len are kept)
    for n, cut in ((100, 1), (100, 16), (100, 17), (6000, 10), (6000, 4097), (9000, 33)):
        b = B(8200 + n + cut).fill_to(n)
        b.src(2, 30, 5).src(1, 20, 64)
        c = b.case(f"short_out/{n}/{cut}", "small", out_len=cut, bs=65536)
        out.append(c.both(["L_FAR_OFF"] if cut <= 16 and n > 4096 else [], []))
    return out


def _runs(n, seed):
    """n literal bytes in runs of 5-9 equal bytes (RLE wins)"""
    r, out = random.Random(seed), bytearray()
    while len(out) < n:
        out += bytes([r.randrange(256)]) * r.randrange(5, 10)
    return bytes(out[:n])


def fam_off8():
    """match_len's and deps' shapes with every offset <= 256 as 8-bit-offset blocks (tests/golden/craft.py and the
    reference's own choice through zxc_block_model.serialise), and the same with RLE literals."""
    out = []
    src = [c for c in fam_match_len() + fam_deps() if all(s[2] <= 256 for s in c.seqs) and "redirect_behind" not in c.name]
    assert len(src) >= 30
    for c in src:
        out.append(dataclasses.replace(c, name="off8/" + c.name, family="off8", kind="glo8", paths=dict(c.paths)))
        # (the reference's serialiser stores a block that does not shrink RAW: the model-built twin exists where it is GLO)
        if M.parse_block(M.serialise(c.seqs, c.lits, len(expand(c.seqs, c.lits)), False, 3))["type"] == M.GLO:
            out.append(dataclasses.replace(c, name="off8m/" + c.name, family="off8", kind="glo8m", paths=dict(c.paths)))
        r = dataclasses.replace(c, name="off8rle/" + c.name, family="off8", kind="glo8m", rle=True, lits=_runs(len(c.lits), len(c.name)),
                                paths={k: list(v) for k, v in c.paths.items()})
        r.need("lean", "X_SETUP_RLE")
        out.append(r)
    assert sum(c.kind == "glo8m" and not c.rle for c in out) >= 20
    return out


def fam_dict():
    out = []
    D = random.Random(0xD1C8).randbytes(1500)

    def d(name, b, ids, **kw):
        c = b.case(name, "dict", dict_=D, routes=("dict",), **kw)
        out.append(c.need("dict", *ids))

    # offsets that end exactly at the dictionary's first byte
    for ll in (0, 3, 20):
        for ml in (5, 16, 200):
            d(f"first_byte/{ll}/{ml}", B(9000 + ll + ml).add(ll, ml, ll + len(D), bad=True).add(2, 6, 2), ["F_FROM_DICT"])
    # a source that straddles the dictionary / output seam by 1, 15, 16 and 17 bytes
    for n in (1, 15, 16, 17):
        for ml in (max(5, n + 1), n + 16, n + 40, 160):
            d(f"seam/{n}/{ml}", B(9100 + n + ml).add(50, ml, 50 + n, bad=True).add(2, 6, 2), ["F_FROM_DICT", "F_LONG"])
    # wholly inside the dictionary, longer than MATCH_MED
    for ml in (129, 300, 1400):
        d(f"inside/{ml}", B(9200 + ml).add(7, ml, 7 + 1450, bad=True).add(2, 6, 2), ["F_FROM_DICT", "C_COPY_DICT_GATHER"])
    # in the middle of a block, and a later match that reads a dictionary match back
    b = B(9300).add(100, 20, 30).add(5, 64, 105 + 20 + 700, bad=True).add(0, 30, 40).add(4, 9, 8)
    d("mid_block", b, ["F_FROM_DICT"])
    # off = est + ll + dict_size and one more: the second is BAD_OFFSET
    for extra, ok in ((0, True), (1, False)):
        b = B(9400 + extra).add(30, 9, 4).add(11, 25, 30 + 9 + 11 + len(D) + extra, bad=True).add(2, 6, 2)
        d(f"reach/{extra}", b, ["F_FROM_DICT"] if ok else ["F_ERR"], valid=ok)
    return out


def fam_errors():
    """Every verdict comes from the oracle (cross-checked against the reference Block API in pack())."""
    out = []

    def e(name, b, n_lit=None, ext=None, lean=("L_ERR",), full=("F_ERR",), **kw):
        kw.setdefault("bs", 4096)
        c = b.case(name, "errors", valid=False, ext=ext, **kw)
        if n_lit is not None:
            c.lits = c.lits[:n_lit] if n_lit <= len(c.lits) else c.lits + bytes(n_lit - len(c.lits))
        out.append(c.both(list(lean), list(full)))

    def base(seed, n_before):
        b = B(seed)
        for i in range(n_before):
            b.add(3 + (i & 1), 6, 2)
        return b

    for where, n_before in (("lane0", 0), ("lane63", 63), ("lane0_batch2", 64)):
        # BAD_OFFSET: one byte in front of the block (the dummy dictionary of the dict route makes it valid there)
        b = base(10000 + n_before, n_before)
        b.add(4, 8, b.pos + 4 + 1, bad=True).add(2, 6, 2)
        e(f"bad_offset/{where}", b, full=())
        # OVERFLOW: the match runs past the capacity (4096 + 2112)
        b = base(10100 + n_before, n_before)
        b.add(4, 7000, 3).add(2, 6, 2)
        e(f"overflow/{where}", b)
        # literal overrun: the sequence wants more literals than the block has
        b = base(10200 + n_before, n_before)
        b.add(40, 6, 3).add(2, 6, 2)
        e(f"lit_overrun/{where}", b, n_lit=sum(s[0] for s in b.seqs) - 12)
    # the first sequence behind a tile cut, and behind a varint cut
    for kind in ("bad_offset", "overflow", "lit_overrun"):
        b = B(10300)
        for _ in range(7):
            b.add(300, 120, 25)
        b.add(81, 20, 7)      # 3041 bytes: cut in front of this one (lean); the error is the sequence right behind it
        n_lit = None
        if kind == "bad_offset":
            b.add(4, 8, b.pos + 4 + 1, bad=True)
        elif kind == "overflow":
            b.add(4, 7000, 3)
        else:
            b.add(40, 6, 3)
            n_lit = sum(s[0] for s in b.seqs) - 12
        b.add(2, 6, 2)
        e(f"{kind}/behind_tile_cut", b, n_lit=n_lit, lean=("L_ERR", "L_TILE_CUT"), full=() if kind == "bad_offset" else ("F_ERR",))
        # ... and the failing sequence is itself the first that does not fit the tile: e == k, returned by the batch that cuts
        b = B(10350)
        for _ in range(7):
            b.add(300, 120, 25)
        n_lit = None
        if kind == "bad_offset":
            b.add(90, 20, b.pos + 90 + 1, bad=True)
        elif kind == "overflow":
            b.add(90, 7000, 3)
        else:
            b.add(140, 6, 3)
            n_lit = sum(s[0] for s in b.seqs) - 12
        b.add(2, 6, 2)
        e(f"{kind}/at_tile_cut", b, n_lit=n_lit, lean=("L_ERR", ("L_TILE_CUT", 0)), full=() if kind == "bad_offset" else ("F_ERR",))
        plan = {i: (i % 5, None) for i in range(62)}
        b = _varint_batch(10400, 62, plan, tail=0)   # 62 varints, then the failing sequence carries the 63rd
        if kind == "bad_offset":
            b.add(15 + 3, 8, b.pos + 18 + 1, bad=True)
        elif kind == "overflow":
            b.add(15 + 3, 7000, 3)
        else:
            b.add(15 + 90, 6, 3)
            n_lit = sum(s[0] for s in b.seqs) - 30
        b.add(2, 6, 2)
        e(f"{kind}/behind_varint_cut", b, n_lit=n_lit, lean=("L_ERR", "L_VARINT_CUT"), full=() if kind == "bad_offset" else ("F_ERR",), bs=4096)
    # two failing sequences of different kinds in one batch: the first in stream order wins
    b = base(10500, 10)
    b.add(4, 8, b.pos + 5, bad=True)
    b.add(4, 7000, 3).add(2, 6, 2)
    e("bad_offset_then_overflow", b, full=("F_ERR",))
    b = base(10501, 10)
    b.add(4, 7000, 3)
    b.add(4, 8, 60000, bad=True).add(2, 6, 2)
    e("overflow_then_bad_offset", b)
    # a truncated varint and a >= 0xE0 byte as the last varint of a batch and as the first of the next
    for what, last in (("truncated", b"\x85"), ("e0", b"\xE3")):
        for at in (63, 64):
            b = base(10600 + at, at)
            b.add(15, 6, 2)    # its literal-length varint is the damaged one
            ext = last
            if what == "e0":
                b.add(2, 6, 2)
                ext = last + b"\x01\x01"
            c_lits = sum(s[0] for s in b.seqs)
            e(f"varint_{what}/seq{at}", b, ext=ext, n_lit=c_lits + 200, lean=("L_VARINT_GENERAL", "C_VARINT_BAD", "L_DEAD"), full=("F_VARINT_GENERAL", "C_VARINT_BAD", "F_DEAD"))
    # trailing literals that overflow the capacity by 1, and that just fit
    for over in (0, 1):
        b = B(10700 + over).add(10, 6, 2)
        b.trail = 4096 + PAD - 16 + over
        e(f"trailing_overflow/{over}", b, lean=("L_ERR",) if over else ("L_EXACT",), full=(), routes=("lean",))
    return out


BOUND_LL = (0, 1, 12, 13, 15, 16, 17, 31, 32, 33, 47, 48, 49, 127, 128, 129, 143, 144, 300)
BOUND_ML = (5, 12, 13, 16, 17, 19, 20, 31, 32, 33, 34, 127, 128, 129, 130, 147, 148, 260, 261, 600)
BOUND_OFF = (1, 2, 3, 4, 15, 16, 17, 20, 255, 256, 257, 300, 4064, 4080, 4095, 4096, 4097, 4112, 8192, 65535, 65536)


@functools.lru_cache(maxsize=2)
def fam_random(count=400, seed=77):
    """Seeded blocks drawn from the boundary sets above mixed with short ordinary sequences; block sizes 4 KiB to 128 KiB, GLO
    (16- and 8-bit offsets) and GHI. Valid by construction: an offset that does not fit yet is replaced by the largest that does."""
    r, out = random.Random(seed), []
    for n in range(count):
        bs = r.choice((4096, 4096, 4096, 4096, 16384, 16384, 16384, 65536, 65536, 131072))
        kind = r.choice(("glo16", "glo16", "ghi", "glo8"))
        b = B(seed * 1000 + n)
        # (the emulator decodes ~0.3 MB/s: three of four large blocks stay short, every fourth fills its block size)
        target = r.randrange(bs // 3, bs - 40) if bs <= 16384 or r.random() < 0.25 else r.randrange(3000, 12000)
        giant = r.randrange(0, 60) if r.random() < 0.25 and bs >= 16384 else -1
        while b.pos < target:
            x = r.random()
            if len(b.seqs) == giant:
                ll, ml = (r.choice((3041, 3585, 5000)), 5) if r.random() < 0.5 else (r.randrange(0, 9), r.choice((3041, 4096, 4097, 9000)))
            elif x < 0.35:
                ll, ml = r.choice(BOUND_LL), r.choice(BOUND_ML)
            elif x < 0.45:
                ll, ml = r.choice(BOUND_LL), 5 + r.randrange(0, 12)
            else:
                ll, ml = r.randrange(0, 14), 5 + r.randrange(0, 14)
            if b.pos + ll + ml > bs - 8:
                ll, ml = min(ll, 3), 5
                if b.pos + ll + ml > bs - 8:
                    break
            if not b.seqs and ll == 0:
                ll = 1
            off = r.choice(BOUND_OFF) if r.random() < 0.5 else r.randrange(1, 600)
            if r.random() < 0.15:
                off = r.randrange(1, b.pos + ll + 1)
            off = min(off, b.pos + ll, 256 if kind == "glo8" else 65536)
            b.add(ll, ml, off)
        b.trail = r.choice((0, 1, 5, 16, 17)) if b.pos + 17 <= bs else 0
        out.append(b.case(f"random/{n}", "random", kind=kind, bs=bs))
    return out


FAMILIES = {"match_len": fam_match_len, "lit_len": fam_lit_len, "varints": fam_varints, "tile": fam_tile, "giant": fam_giant,
            "far": fam_far, "deps": fam_deps, "small": fam_small, "off8": fam_off8, "dict": fam_dict, "errors": fam_errors}


@functools.lru_cache(maxsize=None)
def family(name):
    """the family's cases (shared between tests: read-only)"""
    cases = FAMILIES[name]()
    assert len({c.name for c in cases}) == len(cases), "case names are unique"
    return cases


def required_ids():
    """every id some crafted case asks for (test_decode_limits_cpu requires this to be all of them, with ROUTING_IDS)"""
    ids = set()
    for f in FAMILIES:
        for c in family(f):
            for lst in c.paths.values():
                ids |= {i for i, n in lst if n != 0}
    return ids


# ids the routing test (which executor a launch setting reaches) asserts, on reference-encoded blocks where needed
ROUTING_IDS = {"X_LEAN", "X_FULL", "X_SETUP_RAW", "X_SETUP_RLE", "X_SETUP_PRE"}
