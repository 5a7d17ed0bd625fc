"""The decode executors at their internal limits, on the CPU wave emulator (tests/decode_limit_cases.py has the cases).

Every crafted block runs alone through each route it applies to (the default two-pass launch = the lean executor, the
strict-capacity plan = the lean executor with strict checks inside the full kernel, the dictionary kernel = the full
executor), in a guarded job table: the bytes must equal the plain Python expansion, the status the reference's verdict, no
byte outside the slot may change, and the path markers the case names must have been reached (ZXC_PATH, counted by the
emulator), with the exact count where the case says so. The seeded random family runs packed, 400 blocks."""
import pytest

import decode_limit_cases as D
import decode_plan_cases as P
from decode_harness import IDS, emu, run  # noqa: F401  (the emulator fixture, its path ids and the guarded launch)


@pytest.mark.parametrize("route", D.ROUTES)
@pytest.mark.parametrize("fam", list(D.FAMILIES))
def test_family(emu, oracle, ref, fam, route):  # noqa: F811
    cases = [c for c in D.family(fam) if route in c.routes]
    if fam == "dict":
        assert route == "dict" or not cases
    missed = []
    for i, c in enumerate(cases):
        case, lc = D.pack(oracle, ref, [c], route, align0=i, label=f"{c.name} [{route}]")
        got = run(emu, case, lc, route)
        for name, n in c.paths.get(route, []):
            if (got[name] == 0) if n is None else (got[name] != n):
                missed.append((c.name, name, "reached" if n is None else n, got[name]))
    assert not missed, ("cases that no longer reach the branch they exist for: (case, id, wanted, got)", missed[:12], len(missed))


@pytest.mark.parametrize("fam", [f for f in D.FAMILIES if f != "dict"])
def test_family_packed_and_checksummed(emu, oracle, ref, fam):  # noqa: F811
    """One guarded job table per (family, block size), blocks at all four byte alignments of the compressed buffer, each
    with a verified checksum trailer: the checksum kernel beside the decode, then checksums inside the decode kernels."""
    for group in D.groups(D.family(fam), "lean"):
        case, lc = D.pack(oracle, ref, group, "lean", checksum=True, label=f"{fam}/{group[0].bs >> 10}K packed ck")
        assert len({int(o) % 4 for o in case.jobs["comp_off"]}) == min(4, case.n)
        for apart in (True, False):
            got = run(emu, case, lc, "lean", ck_apart=apart)
            assert got["X_LEAN"] + got["X_LEAN_GHI"] == case.n and got["X_FULL"] == 0, (fam, apart)


def test_every_path_id_has_a_case():
    """A marker nobody asks for is a branch the suite does not pin."""
    asked = D.required_ids() | D.ROUTING_IDS
    assert asked <= set(IDS), sorted(asked - set(IDS))
    assert not set(IDS) - asked, ("path ids no case requires", sorted(set(IDS) - asked))


@pytest.mark.parametrize("route", ["lean", "dict", "strict"])
def test_random_family(emu, oracle, ref, route):  # noqa: F811
    """400 seeded blocks around the boundary values, GLO 16- / 8-bit and GHI, 4 KiB to 128 KiB, all valid by construction:
    packed, one job table per block size. (The strict route runs the lean executor again: every eighth block.)"""
    cases = D.fam_random(400)
    assert len(cases) == 400 and {c.bs for c in cases} == {4096, 16384, 65536, 131072}
    if route == "strict":
        cases = cases[::8]
    for group in D.groups(cases, route):
        case, lc = D.pack(oracle, ref, group, route, label=f"random/{group[0].bs >> 10}K [{route}]")
        assert (case.want_rc >= 0).all()
        run(emu, case, lc, route)


@pytest.mark.parametrize("fam", [f for f in D.FAMILIES if f != "dict"])
def test_frames_are_well_formed(oracle, fam):
    """Every valid case as a whole one-block frame through the oracle's frame decoder (file header, block, EOF, footer)."""
    import craft
    n = 0
    for c in D.family(fam):
        want = D.expand(c.seqs, c.lits) if c.valid else None
        if want is None or not 0 < len(want) <= c.bs:
            continue
        f = craft.frame(oracle, [D.build_block(oracle, c)], c.bs.bit_length() - 1, len(want))
        rc, got = oracle.decompress(f, len(want))
        assert rc == len(want) and got == want, (c.name, rc, len(want))
        fc = craft.frame(oracle, [craft.with_trailer(oracle, D.build_block(oracle, c))], c.bs.bit_length() - 1, len(want), checksum=True)
        rc, got = oracle.decompress(fc, len(want), checksum=True)
        assert rc == len(want) and got == want, (c.name, "checksummed", rc, len(want))
        n += 1
    assert n >= (0 if fam == "errors" else 5), (fam, n)  # (the errors family has no valid case by design)


# ---- which executor a launch setting reaches (recorded in DESIGN.md, "Decode executor routing") ----
def _one(oracle, ref, route, **kw):
    b = D.B(123).add(20, 9, 7).add(3, 40, 11).add(2, 6, 2)
    b.trail = 5
    return D.pack(oracle, ref, [b.case("routing", "routing", **kw)], route)


def test_routing_table(emu, oracle, ref):  # noqa: F811
    lean_only = dict(X_FULL=0, X_FULL_GHI=0)
    full_only = dict(X_LEAN=0, X_LEAN_GHI=0, X_SETUP_RAW=0, X_SETUP_RLE=0, X_SETUP_PRE=0)

    def expect(got, **want):
        bad = {k: (got[k], v) for k, v in want.items() if (got[k] == 0) != (v == 0)}
        assert not bad, bad

    # raw sections, default two-pass launch: the lean kernel's raw set-up and the lean executor
    for kind, x in (("glo16", "X_LEAN"), ("ghi", "X_LEAN_GHI")):
        case, lc = _one(oracle, ref, "lean", kind=kind)
        got = run(emu, case, lc, "lean")
        expect(got, **{x: 1, "X_SETUP_RAW": 0 if kind == "ghi" else 1, "X_SETUP_RLE": 0, "X_SETUP_PRE": 0}, **lean_only)
    # checksummed, checksum kernel apart and inline: still the lean kernel
    for apart in (True, False):
        case, lc = D.pack(oracle, ref, _one(oracle, ref, "lean")[1], "lean", checksum=True)
        expect(run(emu, case, lc, "lean", ck_apart=apart), X_LEAN=1, X_SETUP_RAW=1, **lean_only)
    # strict capacity (and every other FULL plan): the full kernel, whose non-dictionary blocks run the LEAN executor with
    # strict = true. run_sequences<false, *> is instantiated nowhere.
    case, lc = _one(oracle, ref, "strict")
    expect(run(emu, case, lc, "strict"), X_LEAN=1, X_SETUP_RAW=0, **lean_only)
    # dictionary launch: run_sequences<true, GHI>
    for kind, x in (("glo16", "X_FULL"), ("ghi", "X_FULL_GHI")):
        case, lc = _one(oracle, ref, "dict", kind=kind)
        expect(run(emu, case, lc, "dict"), **{x: 1}, **full_only)
    # RLE literals: expanded into the launch's RLE scratch, then the lean kernel's RLE set-up; without scratch the full kernel
    rle = [c for c in D.family("off8") if c.rle][:3]
    case, lc = D.pack(oracle, ref, rle, "lean")
    expect(run(emu, case, lc, "lean"), X_LEAN=1, X_SETUP_RLE=1, X_SETUP_RAW=0, **lean_only)
    try:
        emu.lib.emu_set_rscratch_bytes(0)
        expect(run(emu, case, lc, "lean"), X_LEAN=1, X_SETUP_RLE=0, X_SETUP_RAW=0, **lean_only)
    finally:
        emu.lib.emu_set_rscratch_bytes(4 << 20)
    # PivCo sections (reference-encoded level 6): section kernels + the lean kernel's second entry; without section scratch
    # the full kernel decodes the sections and runs the lean executor
    piv = P.level_case(oracle, ref, 6, 4096, 6 * 4096 - 13)
    P.require(piv, pivco=3)
    expect(run(emu, piv, [], "lean"), X_LEAN=1, X_SETUP_PRE=1, **lean_only)
    try:
        emu.lib.emu_set_pscratch_bytes(0)
        expect(run(emu, piv, [], "lean"), X_LEAN=1, X_SETUP_PRE=0, **lean_only)
    finally:
        emu.lib.emu_set_pscratch_bytes(8 << 20)
