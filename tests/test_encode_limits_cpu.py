"""The block encoder at its format and table limits, on the CPU wave emulator (tests/wave_emu compiles zxc_encode_kernel.hip
unchanged and runs it lane by lane: the sequential meaning of the kernel). For every case of tests/encode_limit_cases.py and every
level of the case:

  * the archive round-trips through the unmodified reference decoder and through the oracle;
  * the case's subject check holds: the limit the case exists for was really reached, at every level listed for it;
  * at levels 1-5 every emitted block equals zxc_block_model.serialise(parse_block(block)) byte for byte, and an RLE literal
    section equals rle_encode(literals): the serialiser follows the reference's rules (8-bit offsets, RLE segmentation and tax,
    the 32-byte pad, the RAW rule);
  * the model itself is pinned to the reference: the same identity holds for every block of the REFERENCE encoder's archive of the
    same input at levels 1-5;
  * size and SHA-256 equal the entry recorded in tests/golden/encoder_limits/digests.json, which tests/test_gpu_encode_limits.py
    asks of the device.

Byte equality and exact counts only: nothing here has a tolerance."""
import ctypes as C
import json
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "wave_emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import encode_limit_cases as E  # noqa: E402
import zxc_block_model as M  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import emu_py
    return emu_py.Emu()


@pytest.fixture(scope="module")
def digests():
    return json.load(open(os.path.join(ROOT, E.DIGESTS)))


@pytest.fixture(scope="module")
def dict_id_of(ref):
    import make_encoder_limits
    return make_encoder_limits.dict_id_fn(ref.lib)


def _ref_compress(ref, data, level, bs, dict_=None):
    import oracle_py
    if not dict_:
        return ref.compress(data, level, bs, True, False)
    o = oracle_py.CompressOpts(level=level, block_size=bs, seekable=1, checksum_enabled=0)
    keep = C.create_string_buffer(dict_, len(dict_))
    o.dict, o.dict_size = C.cast(keep, C.c_void_p), len(dict_)
    cap = ref.lib.zxc_compress_bound(len(data))
    dst = C.create_string_buffer(cap)
    n = ref.lib.zxc_compress(data, len(data), dst, cap, C.byref(o))
    assert n > 0, n
    return dst.raw[:n]


def _ref_decompress(ref, comp, n, checksum, dict_=None):
    import oracle_py
    o = oracle_py.DecompressOpts(checksum_enabled=int(checksum))
    keep = None
    if dict_:
        keep = C.create_string_buffer(dict_, len(dict_))
        o.dict, o.dict_size = C.cast(keep, C.c_void_p), len(dict_)
    out = C.create_string_buffer(max(n, 1))
    rc = ref.lib.zxc_decompress(comp, len(comp), out if n else None, n, C.byref(o))
    return rc, out.raw[:max(rc, 0)]


def _model_identity(blocks, level, prefix, who):
    for i, blk in enumerate(blocks):
        p = M.parse_block(blk)
        if p["seqs"] is None:
            assert level >= 6, (who, i, "PivCo section below level 6")
            continue
        again = M.reserialise(blk, level, prefix)
        if again != blk:
            q = M.parse_block(again)
            show = ("type", "enc_lit", "enc_off", "n_seq", "n_lit", "lit_sec", "ext_sec", "pad")
            raise AssertionError("%s block %d at level %d is not what the model writes for its sequences: emitted %s, model %s"
                                 % (who, i, level, {k: p[k] for k in show}, {k: q[k] for k in show}))
        if p.get("rle_section") is not None:
            assert M.rle_encode(p["literals"]) == p["rle_section"], (who, i, "RLE segmentation")
            assert M.rle_decode(p["rle_section"]) == p["literals"]


def _run_case(emu, ref, oracle, digests, dict_id_of, case):
    """every check of one case -> {limit: levels at which the subject check saw it}"""
    seen = {}
    prefix = case.dict_ or b""
    for level, checksum in E.variants(case):
        arcs = E.emu_archives(emu, case, level, checksum, dict_id_of)
        parsed_all = []
        for data, arc in zip(E.pieces(case), arcs):
            rc, out = _ref_decompress(ref, arc, len(data), checksum, case.dict_)
            assert rc == len(data) and out == data, ("reference decoder", case.name, level, checksum, rc)
            rc, out = oracle.decompress(arc, len(data), checksum=checksum, dict_=case.dict_)
            assert rc == len(data) and out == data, ("oracle", case.name, level, checksum, rc)
            bs, ck, blocks, trailers = M.split_blocks(arc)
            assert bs == case.bs and ck == checksum
            parsed_all += [M.parse_block(b) for b in blocks]
            if level <= 5:
                _model_identity(blocks, level, prefix, "emulator, " + E.key(case, level, checksum))
        want = digests.get(E.key(case, level, checksum))
        got = E.digest(arcs)
        assert want is not None, "no recorded digest for %s: run tests/golden/make_encoder_limits.py --write" % E.key(case, level, checksum)
        assert (got["size"], got["sha256"]) == (want["size"], want["sha256"]), (E.key(case, level, checksum), got["size"], want["size"])
        if not checksum:
            for lim in case.hits(level, parsed_all):
                seen.setdefault(lim, []).append(level)
            if level <= 5:  # the reference pins the model
                for data in E.pieces(case):
                    rarc = _ref_compress(ref, data, level, case.bs, case.dict_)
                    _model_identity(M.split_blocks(rarc)[2], level, prefix, "reference, " + E.key(case, level))
    for lim, levels in case.must.items():
        assert levels, "%s: '%s' is asked of no level" % (case.name, lim)
        missing = [lv for lv in levels if lv not in seen.get(lim, [])]
        assert not missing, "%s: '%s' not reached at levels %s (reached at %s)" % (case.name, lim, missing, seen.get(lim))
    return seen


@pytest.fixture(scope="module")
def run(emu, ref, oracle, digests, dict_id_of):
    """run(case): the case's checks, made once per module whichever test asks first; a failure is kept and raised again"""
    done = {}

    def go(case):
        if case.name not in done:
            try:
                done[case.name] = _run_case(emu, ref, oracle, digests, dict_id_of, case)
            except AssertionError as e:
                done[case.name] = e
        if isinstance(done[case.name], AssertionError):
            raise done[case.name]
        return done[case.name]
    return go


@pytest.mark.parametrize("case", E.cases(), ids=lambda c: c.name)
def test_case_on_emulator(run, case):
    run(case)


def test_every_family_reached_its_limits_and_print_them(run, capsys):
    """the table of limits per level, printed once; stands on its own (cases that have not run yet in this process run here)"""
    families = {c.family for c in E.cases()}
    assert families == {"literal-length escapes", "match-length escapes", "offsets", "ring wrap", "bucket collisions", "RLE",
                        "RAW threshold", "skip acceleration", "dictionary", "job table"}
    table, failed = [], []
    for c in E.cases():
        try:
            seen = run(c)
        except AssertionError:
            failed.append(c.name)
            continue
        table += [(c.family, c.name, lim, seen.get(lim, [])) for lim in c.must]
    with capsys.disabled():
        print("\nencoder limits reached on the emulator (levels):")
        for fam, name, lim, levels in sorted(table):
            print("  %-24s %-18s %-44s %s" % (fam, name, lim, ",".join(map(str, levels))))
    assert not failed, "cases that failed their checks: %s" % failed
    for fam in families:
        assert any(levels for f, _, _, levels in table if f == fam), fam


def test_rle_model_on_constructed_streams():
    """the RLE writer's own edges, stated directly: chunks of 131, remainders of 1-3 and of >= 4, raw tokens of at most 128 bytes"""
    T = M.rle_tokens
    assert T(M.rle_encode(b"a" * 131)) == [("run", 131)]
    assert T(M.rle_encode(b"a" * 132)) == [("run", 131), ("raw", 1)]
    assert T(M.rle_encode(b"a" * 134)) == [("run", 131), ("raw", 3)]
    assert T(M.rle_encode(b"a" * 135)) == [("run", 131), ("run", 4)]
    assert T(M.rle_encode(b"a" * 262)) == [("run", 131), ("run", 131)]
    assert T(M.rle_encode(b"a" * 266)) == [("run", 131), ("run", 131), ("run", 4)]
    raw = bytes(range(1, 130))
    assert T(M.rle_encode(b"a" * 4 + raw[:128] + b"b" * 4)) == [("run", 4), ("raw", 128), ("run", 4)]
    assert T(M.rle_encode(b"a" * 4 + raw + b"b" * 4)) == [("run", 4), ("raw", 128), ("raw", 1), ("run", 4)]
    assert T(M.rle_encode(b"xyz" + b"q" * 3)) == [("raw", 6)]
    for s in (b"", b"a", b"a" * 4, raw * 3 + b"zzzzz" + raw):
        assert M.rle_decode(M.rle_encode(s)) == s
    for x in (0, 127, 128, 16383, 16384, (1 << 21) - 1):
        assert M.read_varint(M.varint(x) + b"\xff", 0) == (x, 1 + (x >= 128) + (x >= 16384))
