"""The lane predicates of the lean executor's batch loop on the CPU wave emulator (which compiles zxc_seq_lean.inc as it is):
the crafted families whose limit one of them decides, with the path-marker expectations of tests/decode_limit_cases.py as the
existing limits test reads them, and the seeded sweep of tests/lean_predicate_cases.py. Status and every byte are compared with
the oracle's verdict and the plain Python expansion, in guarded job tables (no byte outside a slot may change)."""
import pytest

import decode_limit_cases as D
import lean_predicate_cases as L
from decode_harness import emu, run  # noqa: F401  (the emulator fixture and the guarded launch of the limits test)


@pytest.mark.parametrize("fam", L.FAMS)
def test_family(emu, oracle, ref, fam):  # noqa: F811
    """Every case alone on the lean route: verdict, bytes, and the markers the case names (exact counts where it says so)."""
    cases = [c for c in D.family(fam) if "lean" in c.routes]
    assert cases, fam
    missed = []
    for i, c in enumerate(cases):
        case, lc = D.pack(oracle, ref, [c], "lean", align0=i, label=f"{c.name} [lean]")
        got = run(emu, case, lc, "lean")
        for name, n in c.paths.get("lean", []):
            if (got[name] == 0) if n is None else (got[name] != n):
                missed.append((c.name, name, "reached" if n is None else n, got[name]))
    assert not missed, ("(case, id, wanted, got)", missed[:12], len(missed))


def test_far_guards_are_all_pinned():
    """The five clauses of far_ok and the flushed edge each have a case with an exact count."""
    pinned = {name for c in D.family("far") + D.family("small") for name, n in c.paths.get("lean", []) if n is not None or name == "L_FAR_OFF"}
    assert {"L_FAR_GROUP", "L_FAR_NO_QA4", "L_FAR_NO_FLUSHED", "L_FAR_NO_ML", "L_FAR_NO_EDGE", "L_FAR_OFF"} <= pinned, pinned
    assert any(c.name.startswith("flushed_edge/") for c in D.family("far"))


def test_sweep_blocks_decode(oracle):
    """The oracle alone decodes the generated blocks; the ones it refuses are left out, at most 5 % of them."""
    good, refused = L.sweep(oracle)
    assert refused <= L.N_SWEEP * 5 // 100, (refused, L.N_SWEEP)
    assert len(good) + refused == L.N_SWEEP
    c = L.straddle_block()
    blk = D.build_block(oracle, c)
    rc, got = oracle.decode_block(blk, c.bs)
    assert rc == len(got) > 60000 and got == D.expand(c.seqs, c.lits)


def test_sweep(emu, oracle, ref):  # noqa: F811
    """The sweep packed into one job table, the 64 KiB block alone; every guard of far_ok must have decided both ways."""
    good, _ = L.sweep(oracle)
    case, lc = D.pack(oracle, ref, good, "lean", label="sweep/4K")
    assert (case.want_rc >= 4200).all()
    got = run(emu, case, lc, "lean")
    assert got["X_LEAN"] == len(good) and got["X_FULL"] == 0
    # (L_FAR_NO_FLUSHED needs a batch of more than 2 944 bytes behind a p just below a KiB mark: the far family's flushed_edge
    # cases pin it; 64 short sequences never span that much)
    for name in ("L_FAR_GROUP", "L_FAR_5TH", "L_FAR_NO_QA4", "L_FAR_NO_EDGE", "L_FAR_NO_ML", "L_FAR_OFF", "L_EXACT",
                 "L_STEPABLE", "L_BYTEWISE", "L_LONG", "L_LIT_GROUP", "L_LIT_5TH"):
        assert got[name] > 0, (name, "the sweep no longer reaches it")
    case, lc = D.pack(oracle, ref, [L.straddle_block()], "lean", label="straddle_kib")
    got = run(emu, case, lc, "lean")
    assert got["L_FAR_GROUP"] >= 100 and got["L_STEPABLE"] >= 100, (got["L_FAR_GROUP"], got["L_STEPABLE"])
