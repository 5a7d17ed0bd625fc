"""A plain model of ONE block of a v8 archive: what the bytes mean (parse_block) and which bytes a given list of
sequences and literals must become (serialise). Pure Python, written from the format specification (the v8 format
document: block header, GLO / GHI headers, descriptors, sections, the 32-byte slack, prefix varints) and from the
rules of the reference encoder's block tail; nothing here is derived from the HIP kernel.

The reference pins this model, not the product: tests/test_encode_limits_cpu.py cuts the reference encoder's archives
into blocks and requires serialise(parse_block(block)) == block for every one of them. The same identity is then asked of
every block the kernel emits, so a serialiser rule the kernel gets wrong (8-bit offsets, the RLE segmentation, the RLE tax,
the pad, the RAW rule) shows as a byte difference although the block still decodes.

Rules reproduced (reference encoder, block tail):
  * tokens (GLO: LL << 4 | ML - 5, both saturating at 15; GHI: LL << 24 | ML - 5 << 16 | offset - 1, saturating at 255),
    extras = prefix varints of LL - esc then ML - 5 - esc for every saturated field, in sequence order;
  * GLO offsets are one byte each exactly when the largest biased offset (offset - 1) is <= 255 -- which holds for a
    block without any sequence, too; GHI always writes enc_off = 0;
  * RLE literal section (GLO only): maximal runs of >= 4 equal bytes become 2-byte run tokens in chunks of <= 131 bytes, a
    remainder of 1-3 bytes a raw token of its own, everything between runs raw tokens of <= 128 bytes;
  * RLE is chosen when rle_size + ((n_literals * premium) >> 8) < n_literals, premium 8 below level 6 and 1 from level 6;
  * at least 32 bytes follow the literal section: zero pad behind the extras otherwise;
  * the block is stored RAW when 8 + payload >= the block's byte count.
PivCo sections (enc_lit = 2 / enc_tok = 2, levels 6-7) are not modelled: parse_block returns their header fields and section
sizes only; serialise writes raw or RLE literals and raw tokens, so the identity is asked at levels 1-5."""
import struct

RAW, GLO, GHI, SEK, EOF = 0, 1, 2, 254, 255
SLACK = 32
_M64 = (1 << 64) - 1


def hash8(hdr8: bytes) -> int:
    """the block header's check byte: xorshift of the header word with byte 7 zeroed"""
    v = int.from_bytes(bytes(hdr8[:7]) + b"\0", "little")
    h = v ^ 0x9E3779B97F4A7C15
    h ^= (h << 13) & _M64
    h ^= h >> 7
    h ^= (h << 17) & _M64
    return ((h >> 32) ^ h) & 0xFF


def block_header(btype: int, comp_size: int) -> bytes:
    h = bytes([btype, 0, 0]) + struct.pack("<I", comp_size)
    return h + bytes([hash8(h)])


def varint(x: int) -> bytes:
    if x < 128:
        return bytes([x])
    if x < 16384:
        return bytes([0x80 | (x & 0x3F), x >> 6])
    assert x < (1 << 21), x
    return bytes([0xC0 | (x & 0x1F), (x >> 5) & 0xFF, x >> 13])


def read_varint(b, at):
    """-> (value, next position)"""
    f = b[at]
    if f < 0x80:
        return f, at + 1
    if f < 0xC0:
        return (f & 0x3F) | (b[at + 1] << 6), at + 2
    assert f < 0xE0, "a varint of four or more bytes is out of the format"
    return (f & 0x1F) | (b[at + 1] << 5) | (b[at + 2] << 13), at + 3


def rle_encode(lit: bytes) -> bytes:
    """the reference's RLE writer: see the module docstring"""
    out = bytearray()
    n, p = len(lit), 0
    while p < n:
        b, start = lit[p], p
        p += 1
        while p < n and lit[p] == b:
            p += 1
        run = p - start
        if run >= 4:
            while run >= 4:
                c = min(run, 131)
                out += bytes([0x80 | (c - 4), b])
                run -= c
            if run:
                out += bytes([run - 1]) + bytes([b]) * run
        else:
            while p < n and not (p + 3 < n and lit[p] == lit[p + 1] == lit[p + 2] == lit[p + 3]):
                p += 1
            q = start
            while q < p:
                c = min(p - q, 128)
                out += bytes([c - 1]) + lit[q:q + c]
                q += c
    return bytes(out)


def rle_tokens(sec: bytes):
    """[(kind, length)] of an RLE section: kind 'run' or 'raw'"""
    out, p = [], 0
    while p < len(sec):
        t = sec[p]
        if t & 0x80:
            out.append(("run", (t & 0x7F) + 4))
            p += 2
        else:
            out.append(("raw", t + 1))
            p += 2 + t
    assert p == len(sec), "RLE section ends inside a token"
    return out


def rle_decode(sec: bytes) -> bytes:
    out, p = bytearray(), 0
    while p < len(sec):
        t = sec[p]
        if t & 0x80:
            out += bytes([sec[p + 1]]) * ((t & 0x7F) + 4)
            p += 2
        else:
            assert p + 2 + t <= len(sec), "RLE raw token runs past the section"
            out += sec[p + 1:p + 2 + t]
            p += 2 + t
    return bytes(out)


def rle_premium(level: int) -> int:
    return 1 if level >= 6 else 8


def parse_block(blk: bytes) -> dict:
    """blk: one block, header included, the optional checksum trailer NOT included. -> dict(type, seqs [(ll, ml, off)],
    literals, enc_lit, enc_tok, enc_off, n_seq, n_lit, desc (descriptor bytes), lit_sec / tok_sec / off_sec / ext_sec (section
    sizes, the extras without the pad), pad, trailing (literals behind the last sequence), decoded (the block's byte count).
    Blocks with a PivCo section: header fields and section sizes only (seqs / literals None)."""
    btype, csz = blk[0], struct.unpack_from("<I", blk, 3)[0]
    assert blk[1] == 0 and blk[2] == 0, "flags / reserved must be 0"
    assert blk[7] == hash8(blk[:8]), "block header check byte"
    assert len(blk) == 8 + csz, (len(blk), csz)
    if btype == RAW:
        return dict(type=RAW, seqs=[], literals=bytes(blk[8:]), enc_lit=0, enc_tok=0, enc_off=0, n_seq=0, n_lit=csz, desc=0,
                    lit_sec=csz, tok_sec=0, off_sec=0, ext_sec=0, pad=0, trailing=csz, decoded=csz)
    assert btype in (GLO, GHI), btype
    p = blk[8:]
    n_seq, n_lit, enc_lit, enc_tok, enc_mlen, enc_off = struct.unpack_from("<IIBBBB", p, 0)
    assert enc_mlen == 0
    at = 12
    r = dict(type=btype, enc_lit=enc_lit, enc_tok=enc_tok, enc_off=enc_off, n_seq=n_seq, n_lit=n_lit)
    if btype == GHI:
        assert (enc_lit, enc_tok, enc_off) == (0, 0, 0), "GHI writes raw literals and no offset mode"
        lit_sec, tok_sec, off_sec = n_lit, 4 * n_seq, 0
    else:
        assert enc_lit in (0, 1, 2) and enc_tok in (0, 2) and enc_off in (0, 1)
        lit_sec = n_lit
        if enc_lit:
            lit_sec = struct.unpack_from("<I", p, at)[0]
            at += 4
        tok_sec = n_seq
        if enc_tok:
            tok_sec = struct.unpack_from("<I", p, at)[0]
            at += 4
        off_sec = n_seq * (1 if enc_off else 2)
    r.update(desc=at - 12, lit_sec=lit_sec, tok_sec=tok_sec, off_sec=off_sec)
    lit_at = at
    tok_at = lit_at + lit_sec
    off_at = tok_at + tok_sec
    ext_at = off_at + off_sec
    assert ext_at <= csz, "sections run past the payload"
    assert csz - tok_at >= SLACK, "fewer than 32 bytes behind the literal section"
    if enc_lit == 2 or enc_tok == 2:
        r.update(seqs=None, literals=None, ext_sec=None, pad=None, trailing=None, decoded=None, ext_and_pad=csz - ext_at)
        return r
    lit = bytes(p[lit_at:tok_at])
    if enc_lit == 1:
        r["rle_section"] = lit
        lit = rle_decode(lit)
    assert len(lit) == n_lit, (len(lit), n_lit)
    esc = 255 if btype == GHI else 15
    seqs, e = [], ext_at
    for i in range(n_seq):
        if btype == GHI:
            w = struct.unpack_from("<I", p, tok_at + 4 * i)[0]
            ll, ml, off = w >> 24, (w >> 16) & 0xFF, (w & 0xFFFF) + 1
        else:
            t = p[tok_at + i]
            ll, ml = t >> 4, t & 15
            off = (p[off_at + i] if enc_off else struct.unpack_from("<H", p, off_at + 2 * i)[0]) + 1
        if ll == esc:
            v, e = read_varint(p, e)
            ll += v
        if ml == esc:
            v, e = read_varint(p, e)
            ml += v
        seqs.append((ll, ml + 5, off))
    assert e <= csz, "extras run past the payload"
    pad = csz - e
    assert not any(p[e:]), "the pad is written as zeros"
    used = sum(s[0] for s in seqs)
    assert used <= n_lit, "sequences take more literals than the block has"
    r.update(seqs=seqs, literals=lit, ext_sec=e - ext_at, pad=pad, trailing=n_lit - used,
             decoded=n_lit + sum(s[1] for s in seqs))
    return r


def serialise(seqs, literals: bytes, nblk: int, ghi: bool, level: int, data=None) -> bytes:
    """The block (without checksum trailer) that the reference's block tail writes for these sequences [(ll, ml, off)] and
    literals of a block of nblk bytes, the RAW rule included: the block's bytes are stored when 8 + payload >= nblk. `data`: the
    block's decoded bytes, needed for that only when offsets reach into a dictionary (else they follow from the sequences)."""
    esc = 255 if ghi else 15
    toks, offs, ext = bytearray(), bytearray(), bytearray()
    max_biased = 0
    for ll, ml, off in seqs:
        assert ml >= 5 and 1 <= off <= 65536, (ll, ml, off)
        m = ml - 5
        max_biased = max(max_biased, off - 1)
        if ghi:
            toks += struct.pack("<I", (min(ll, 255) << 24) | (min(m, 255) << 16) | (off - 1))
        else:
            toks.append((min(ll, 15) << 4) | min(m, 15))
        if ll >= esc:
            ext += varint(ll - esc)
        if m >= esc:
            ext += varint(m - esc)
    n_lit = len(literals)
    enc_lit, enc_off, desc, lit_sec = 0, 0, b"", bytes(literals)
    if not ghi:
        enc_off = 1 if max_biased <= 255 else 0
        for ll, ml, off in seqs:
            offs += bytes([off - 1]) if enc_off else struct.pack("<H", off - 1)
        if n_lit:
            r = rle_encode(lit_sec)
            if len(r) + ((n_lit * rle_premium(level)) >> 8) < n_lit:
                enc_lit, lit_sec, desc = 1, r, struct.pack("<I", len(r))
    behind = len(toks) + len(offs) + len(ext)
    pad = max(0, SLACK - behind)
    payload = struct.pack("<IIBBBB", len(seqs), n_lit, enc_lit, 0, 0, enc_off) + desc + lit_sec + toks + offs + ext + bytes(pad)
    if 8 + len(payload) >= nblk:
        if data is None:
            data = decode(dict(type=GHI if ghi else GLO, seqs=seqs, literals=bytes(literals)))
        assert len(data) == nblk
        return block_header(RAW, nblk) + bytes(data)
    return block_header(GHI if ghi else GLO, len(payload)) + payload


def decode(parsed: dict, prefix: bytes = b"") -> bytes:
    """the bytes a parsed block stands for (prefix: the dictionary in front of it)"""
    if parsed["type"] == RAW:
        return parsed["literals"]
    out, lit, lp = bytearray(prefix), parsed["literals"], 0
    for ll, ml, off in parsed["seqs"]:
        out += lit[lp:lp + ll]
        lp += ll
        assert off <= len(out), "offset reaches in front of the data"
        for _ in range(ml):
            out.append(out[-off])
    out += lit[lp:]
    return bytes(out[len(prefix):])


def reserialise(blk: bytes, level: int, prefix: bytes = b"") -> bytes:
    """serialise(parse_block(blk)): must reproduce blk (blocks without PivCo sections)"""
    p = parse_block(blk)
    if p["type"] == RAW:
        return serialise([], p["literals"], p["decoded"], level <= 2, level)
    data = None
    if prefix:
        data = decode(p, prefix)
    return serialise(p["seqs"], p["literals"], p["decoded"], p["type"] == GHI, level, data)


def split_blocks(arc: bytes):
    """A whole archive -> (block_size, has_checksum, [block bytes without the trailer], [trailer or None])"""
    assert arc[:4] == (0x9CB02EF5).to_bytes(4, "little") and arc[4] == 8
    bs, ck = 1 << arc[5], bool(arc[6] & 0x80)
    at, blocks, trailers = 16, [], []
    while True:
        t, csz = arc[at], struct.unpack_from("<I", arc, at + 3)[0]
        if t == EOF:
            assert csz == 0
            break
        blocks.append(arc[at:at + 8 + csz])
        at += 8 + csz
        trailers.append(arc[at:at + 4] if ck else None)
        at += 4 if ck else 0
    return bs, ck, blocks, trailers
