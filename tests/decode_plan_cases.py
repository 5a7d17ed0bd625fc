"""Shared case builder of the decode-plan tests (tests/test_wave_emu_plans.py on the CPU wave emulator,
tests/test_gpu_decode_plans.py on the device). Not a conftest: both modules import it.

A case is one job table over one archive plus what the reference says about every block of it:
* archives come from the reference encoder (levels 1, 3, 6, 7, with and without checksums, with a dictionary);
* mutants flip seeded bits in payloads, block headers and checksum trailers;
* expected verdicts come from the oracle's block decoder, or from the reference Block API for dictionary blocks;
  the product is never compared with itself;
* the guarded layout moves every block's output slot so that the slots have gaps, start at offsets that are
  multiples of 16 but not of 64, and sit between guard regions; the whole output buffer starts as a canary pattern.

After a launch, check_guarded() asserts the containment rule of include/zxc_mi355x.h exactly: no byte outside
[out_off, out_off + round_up(out_len, 16)) of any block changed, whatever the block's status; every block with a
non-negative status has the oracle's status and bytes; every failed block has the oracle's error code (its bytes are
undefined). Each scenario also asserts that its input holds what it exists to exercise (subject checks below), so
coverage cannot silently go away when the corpus or the encoder changes.
"""
import ctypes as C
import dataclasses
import functools
import os
import random

import numpy as np

JOB_DTYPE = np.dtype([("comp_off", "<u8"), ("out_off", "<u8"), ("comp_size", "<u4"), ("out_len", "<u4")])
HEAD_GUARD = 4096 + 16  # bytes in front of the first slot (the first slot starts 16 bytes past a 4 KiB boundary)
TAIL_GUARD = 4096       # bytes behind the last slot


@dataclasses.dataclass
class Case:
    comp: bytes
    jobs: np.ndarray       # JOB_DTYPE
    block_size: int
    checksum: bool         # blocks carry trailers and the launch verifies them
    want_rc: np.ndarray    # int32 per job: the reference's decoded size or error code
    want: list             # bytes per job (b"" for failed blocks)
    dict_: bytes = None
    dict_huf: bytes = None
    label: str = ""
    hit: tuple = ()        # mutated jobs

    @property
    def n(self):
        return int(self.jobs.size)


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=4)
def corpus_bytes(n: int, seed: int = 5) -> bytes:
    """n bytes of the silesia-like corpus; callers take sizes that are not multiples of 16 (a short, unaligned last block)."""
    from zxc_amd import corpus
    return corpus.synth_silesia(n, seed=seed)


def seek_jobs(oracle, comp: bytes):
    """-> (jobs in the seekable layout, block_size, has_checksum) from the archive's seek table."""
    t = oracle.seek_table(comp)
    assert t is not None, "not a seekable archive"
    n, bs = t["n_blocks"], t["block_size"]
    jobs = np.zeros(n, dtype=JOB_DTYPE)
    jobs["comp_off"] = t["comp_offsets"][:n]
    jobs["comp_size"] = t["comp_sizes"]
    jobs["out_off"] = np.arange(n, dtype=np.uint64) * np.uint64(bs)
    jobs["out_len"] = np.minimum(bs, t["total"] - np.arange(n, dtype=np.int64) * bs).astype(np.uint32)
    return jobs, bs, bool(t["has_checksum"])


def ref_archive(ref, data: bytes, level: int, block_size: int, checksum=False) -> bytes:
    return ref.compress(data, level, block_size, True, checksum)


def ref_dict_archive(ref, data: bytes, level: int, block_size: int, dict_: bytes, dict_huf=None, checksum=False) -> bytes:
    """zxc_compress of the reference with CompressOpts.dict (and .dict_huf)."""
    import oracle_py
    keep = (C.create_string_buffer(dict_, len(dict_)), C.create_string_buffer(dict_huf, 128) if dict_huf else None)
    o = oracle_py.CompressOpts(level=level, block_size=block_size, seekable=1, checksum_enabled=int(checksum))
    o.dict, o.dict_size = C.cast(keep[0], C.c_void_p), len(dict_)
    o.dict_huf = C.cast(keep[1], C.c_void_p) if dict_huf else None
    cap = ref.lib.zxc_compress_bound(len(data))
    dst = C.create_string_buffer(cap)
    n = ref.lib.zxc_compress(data, len(data), dst, cap, C.byref(o))
    assert n > 0, f"reference zxc_compress with a dictionary failed: {n}"
    return dst.raw[:n]


def subset(comp: bytes, jobs: np.ndarray, idx):
    """A compact archive body holding only the blocks jobs[idx] (blocks are self-contained), in that order, and its jobs.
    An index may repeat: the block is then decoded more than once, into distinct slots."""
    parts, rows, pos = [], np.zeros(len(idx), dtype=JOB_DTYPE), 0
    for r, i in enumerate(idx):
        o, s = int(jobs["comp_off"][i]), int(jobs["comp_size"][i])
        parts.append(comp[o:o + s])
        rows[r] = (pos, 0, s, jobs["out_len"][i])
        pos += s
    return b"".join(parts), rows


def concat(*pieces):
    """[(comp, jobs)] -> one archive body and one job table (comp_off rebased)."""
    blob, tabs = bytearray(), []
    for comp, jobs in pieces:
        j = jobs.copy()
        j["comp_off"] += np.uint64(len(blob))
        blob += comp
        tabs.append(j)
    return bytes(blob), np.concatenate(tabs)


# ------------------------------------------------------------------ mutants
def mutate(comp: bytes, jobs: np.ndarray, rng: random.Random, n_hit: int, checksum: bool):
    """Seeded bit flips in n_hit distinct blocks, in turn: the payload, the block header (type / size fields), the checksum
    trailer (checksummed archives; else the payload again). -> (mutated bytes, sorted hit job indices)."""
    m = bytearray(comp)
    hit = sorted(rng.sample(range(jobs.size), min(n_hit, jobs.size)))
    for n, k in enumerate(hit):
        off, size = int(jobs["comp_off"][k]), int(jobs["comp_size"][k])
        tb = 4 if checksum else 0
        kind = n % 3
        if kind == 1:
            at = off + rng.choice((0, 3, 4, 5, 6))                   # block type / compressed size
        elif kind == 2 and checksum:
            at = off + size - 1 - rng.randrange(4)                   # the stored checksum
        else:
            at = off + 8 + rng.randrange(max(1, size - 8 - tb))      # the payload
        m[at] ^= 1 << rng.randrange(8)
    return bytes(m), tuple(hit)


# ------------------------------------------------------------------ the reference's verdicts
def verdicts(oracle, comp: bytes, jobs: np.ndarray, block_size: int, checksum: bool, dict_=None, dict_huf=None, ref=None):
    """Per job: the oracle's block decoder (status, bytes), or the reference Block API with the dictionary."""
    rc = np.zeros(jobs.size, dtype=np.int32)
    want = []
    api = None
    if dict_ is not None:
        import oracle_py
        assert ref is not None, "dictionary verdicts come from the reference Block API"
        api = oracle_py.BlockApi(ref.lib)
    for i in range(jobs.size):
        o, s = int(jobs["comp_off"][i]), int(jobs["comp_size"][i])
        blk = comp[o:o + s]
        if api is not None:
            r, b = api.decompress_block(blk, block_size + 2112, checksum=checksum, dict_=dict_, dict_huf=dict_huf)
        else:
            r, b = oracle.decode_block(blk, block_size, checksum=checksum)
        rc[i] = r
        want.append(b if r >= 0 else b"")
    if api is not None:
        api.close()
    return rc, want


def make_case(oracle, comp, jobs, block_size, checksum, label, dict_=None, dict_huf=None, ref=None, hit=()):
    rc, want = verdicts(oracle, comp, jobs, block_size, checksum, dict_, dict_huf, ref)
    return Case(comp, jobs, block_size, checksum, rc, want, dict_, dict_huf, label, tuple(hit))


# ------------------------------------------------------------------ subject checks
def block_fields(comp: bytes, jobs: np.ndarray):
    """-> (type, enc_lit, enc_tok) arrays of every job's block (GLO / GHI header right behind the 8-byte block header)."""
    off = jobs["comp_off"].astype(np.int64)
    a = np.frombuffer(comp, dtype=np.uint8)
    return a[off], a[np.minimum(off + 16, len(a) - 1)], a[np.minimum(off + 17, len(a) - 1)]


def rle_mask(comp, jobs):
    """GLO blocks with RLE-coded literals (enc_lit = 1)."""
    t, el, _ = block_fields(comp, jobs)
    return (t == 1) & (el == 1)


def pivco_mask(comp, jobs):
    """GLO blocks with a PivCo-coded literal or token section (levels 6-7)."""
    t, el, et = block_fields(comp, jobs)
    return (t == 1) & ((el == 2) | (et == 2))


def require(case: Case, rle=0, pivco=0, failed=0, n_jobs=0, unaligned_tail=True):
    """The scenario's input holds what it exists to exercise. unaligned_tail: some block keeps an out_len that is not a
    multiple of 16 (the archive's short last block)."""
    n_rle = int(rle_mask(case.comp, case.jobs).sum())
    n_piv = int(pivco_mask(case.comp, case.jobs).sum())
    n_bad = int((case.want_rc < 0).sum())
    assert n_rle >= rle, (case.label, "RLE-literal blocks", n_rle, rle)
    assert n_piv >= pivco, (case.label, "PivCo blocks", n_piv, pivco)
    assert n_bad >= failed, (case.label, "failed blocks", n_bad, failed)
    assert case.n >= n_jobs, (case.label, "jobs", case.n, n_jobs)
    if unaligned_tail:
        assert (case.jobs["out_len"] % 16 != 0).any(), (case.label, "no block with an unaligned out_len")
    return n_rle, n_piv, n_bad


# ------------------------------------------------------------------ guarded layout
def round16(x):
    return (int(x) + 15) & ~15


def guarded_layout(case: Case, seed=0):
    """Rewrites the jobs' out_off in place: slots of round_up(out_len, 16) bytes with gaps of 16-48 bytes between them,
    every out_off a multiple of 16 but not of 64, HEAD_GUARD bytes before the first slot and TAIL_GUARD after the last.
    -> the output buffer's size."""
    rng = random.Random(seed)
    off = HEAD_GUARD
    out_off = np.zeros(case.n, dtype=np.uint64)
    for i in range(case.n):
        assert off % 16 == 0 and off % 64 != 0
        out_off[i] = off
        nxt = off + round16(case.jobs["out_len"][i])
        gaps = [g for g in (16, 32, 48) if (nxt + g) % 64]
        off = nxt + rng.choice(gaps)
    case.jobs["out_off"] = out_off
    assert any(int(o) % 1024 for o in out_off)
    return off + TAIL_GUARD


def canary(n: int) -> np.ndarray:
    """The guard pattern: position-dependent, so a shifted or misdirected copy of it shows too."""
    i = np.arange(n, dtype=np.uint32)
    return ((i * 167 + (i >> 8) * 13 + 0x5B) & 0xFF).astype(np.uint8)


def slot_mask(case: Case, size: int) -> np.ndarray:
    """True inside some block's [out_off, out_off + round_up(out_len, 16))."""
    d = np.zeros(size + 1, dtype=np.int32)
    lo = case.jobs["out_off"].astype(np.int64)
    hi = lo + ((case.jobs["out_len"].astype(np.int64) + 15) & ~15)
    np.add.at(d, lo, 1)
    np.add.at(d, hi, -1)
    return np.cumsum(d[:size]) > 0


def check_guarded(case: Case, out: np.ndarray, status: np.ndarray, what=""):
    """(a) every byte outside the blocks' slots still holds the canary; (b) blocks with a non-negative status have the
    reference's status and bytes; (c) failed blocks have the reference's error code."""
    label = f"{case.label} {what}".strip()
    out = np.asarray(out, dtype=np.uint8)
    can = canary(out.size)
    stray = np.nonzero((out != can) & ~slot_mask(case, out.size))[0]
    if stray.size:
        lo = case.jobs["out_off"].astype(np.int64)
        order = np.argsort(lo)
        k = np.searchsorted(lo[order], stray[0], side="right") - 1
        near = int(order[k]) if k >= 0 else None
        detail = "in front of the first slot" if near is None else \
            f"{stray[0] - int(lo[near]) - int(case.jobs['out_len'][near])} bytes past job {near}'s out_len (status {int(status[near])})"
        raise AssertionError(f"{label}: {stray.size} bytes outside every slot changed, first at {int(stray[0])}: {detail}")
    status = np.asarray(status, dtype=np.int32)
    bad = np.nonzero(status != case.want_rc)[0]
    assert bad.size == 0, (label, "status differs from the reference", [(int(i), int(status[i]), int(case.want_rc[i])) for i in bad[:8]])
    raw = out.tobytes()
    for i in np.nonzero(case.want_rc >= 0)[0]:
        o, L = int(case.jobs["out_off"][i]), int(case.jobs["out_len"][i])
        n = min(int(case.want_rc[i]), L)
        assert raw[o:o + n] == case.want[i][:n], (label, "bytes differ from the reference", int(i))


# ------------------------------------------------------------------ builders
def dictionary():
    """The conformance HTTP dictionary: (content, 128-byte shared literal table)."""
    from conftest import GOLDEN, load_dict
    return load_dict(os.path.join(GOLDEN, "conformance", "valid", "dict_http.zxd"))


def level_case(oracle, ref, level, block_size, n_bytes, checksum=False, n_hit=0, seed=5, label=None):
    """The corpus' first n_bytes at `level` and `block_size`, seekable layout, n_hit mutated blocks."""
    data = corpus_bytes(n_bytes, seed)
    comp = ref_archive(ref, data, level, block_size, checksum)
    jobs, bs, ck = seek_jobs(oracle, comp)
    assert bs == block_size and ck == checksum
    hit = ()
    if n_hit:
        comp, hit = mutate(comp, jobs, random.Random(1000 * level + n_hit + seed), n_hit, checksum)
    return make_case(oracle, comp, jobs, bs, checksum, label or f"L{level}{'ck' if checksum else ''}/{bs >> 10}K", hit=hit)


def dict_case(oracle, ref, level, block_size, n_bytes, use_huf, checksum=False, n_hit=0, seed=5, label=None):
    d, dh = dictionary()
    data = corpus_bytes(n_bytes, seed)
    comp = ref_dict_archive(ref, data, level, block_size, d, dh if use_huf else None, checksum)
    jobs, bs, ck = seek_jobs(oracle, comp)
    hit = ()
    if n_hit:
        comp, hit = mutate(comp, jobs, random.Random(77 + level + n_hit), n_hit, checksum)
    return make_case(oracle, comp, jobs, bs, checksum, label or f"dict L{level}{'+huf' if use_huf else ''}/{bs >> 10}K",
                     dict_=d, dict_huf=dh if use_huf else None, ref=ref, hit=hit)


def rle_mix_case(oracle, ref, n_rle_jobs, n_other, n_hit=0, n_bytes=(16 << 20) - 13, seed=5, label=None):
    """Level-3 4 KiB blocks: n_rle_jobs jobs on RLE-literal blocks (repeating blocks when the corpus has fewer) spread
    among n_other jobs on the other blocks, so the launch-order pass meets them in more than one workgroup of 256."""
    data = corpus_bytes(n_bytes, seed)
    comp = ref_archive(ref, data, 3, 4096)
    jobs, _, _ = seek_jobs(oracle, comp)
    rle = np.nonzero(rle_mask(comp, jobs))[0]
    other = np.nonzero(~rle_mask(comp, jobs))[0]
    assert rle.size and other.size
    pick_r = [int(rle[i % rle.size]) for i in range(n_rle_jobs)]
    pick_o = [int(other[i % other.size]) for i in range(n_other)]
    idx, step = [], max(1, (n_rle_jobs + n_other) // max(1, n_rle_jobs))
    ri = oi = 0
    while ri < len(pick_r) or oi < len(pick_o):  # interleave: one RLE job every `step` jobs
        if ri < len(pick_r) and (len(idx) % step == 0 or oi >= len(pick_o)):
            idx.append(pick_r[ri]); ri += 1
        else:
            idx.append(pick_o[oi]); oi += 1
    body, sj = subset(comp, jobs, idx)
    hit = ()
    if n_hit:
        body, hit = mutate(body, sj, random.Random(31 + n_hit), n_hit, False)
    return make_case(oracle, body, sj, 4096, False, label or f"RLE {n_rle_jobs}/{n_rle_jobs + n_other}", hit=hit)
