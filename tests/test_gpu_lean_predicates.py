"""The lane predicates of the lean executor's batch loop on the device: the crafted blocks of tests/test_lean_predicates_cpu.py
(the families of tests/lean_predicate_cases.FAMS, the 4 KiB sweep, the 64 KiB block whose sources straddle the KiB marks) and
one launch of the first 256 level-3 blocks of corpus tile 0, reference-encoded. Status and bytes against the oracle and the
plain Python expansion, in guarded output buffers: no byte outside a block's slot may change. What the emulator cannot show is
in the loop here: the far loads' address form (a uniform base and an unsigned 32-bit lane offset), the unconditional loads of
idle lanes, the read-back of bytes an earlier batch flushed. No case is built to fault."""
import numpy as np
import pytest

import decode_limit_cases as D
import decode_plan_cases as P
import lean_predicate_cases as L
from decode_harness import dev, launch  # noqa: F401  (the device fixture and the guarded launch of the limits test)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fam", L.FAMS)
def test_families(dev, oracle, ref, fam):  # noqa: F811
    for group in D.groups(D.family(fam), "lean"):
        case, lc = D.pack(oracle, ref, group, "lean", label=f"{fam}/{group[0].bs >> 10}K [lean predicates]")
        launch(dev, case, lc, case.label)


def test_sweep(dev, oracle, ref):  # noqa: F811
    good, refused = L.sweep(oracle)
    assert refused <= L.N_SWEEP * 5 // 100, (refused, L.N_SWEEP)
    case, lc = D.pack(oracle, ref, good, "lean", label="sweep/4K")
    launch(dev, case, lc, case.label)
    case, lc = D.pack(oracle, ref, [L.straddle_block()], "lean", label="straddle_kib")
    launch(dev, case, lc, case.label)


def test_corpus_tile0_first_256_blocks(dev, oracle, ref):  # noqa: F811
    from zxc_amd import corpus
    bs, n = 65536, 256
    data = b""
    for task in corpus.tile_chunks(0, 0):  # the chunks of synth_silesia_tile(0), as many as the blocks need
        data += corpus.gen_chunk(task)
        if len(data) >= n * bs:
            break
    data = data[:n * bs]
    comp = P.ref_archive(ref, data, 3, bs)
    jobs, got_bs, ck = P.seek_jobs(oracle, comp)
    assert got_bs == bs and not ck and jobs.size == n
    case = P.make_case(oracle, comp, jobs, bs, False, "tile 0, 256 blocks, L3")
    assert (case.want_rc == bs).all() and b"".join(case.want) == data
    import torch
    size = P.guarded_layout(case, seed=n)
    d_comp = torch.frombuffer(bytearray(case.comp) + bytearray(64), dtype=torch.uint8).to("cuda")
    d_jobs = torch.frombuffer(bytearray(case.jobs.tobytes()), dtype=torch.uint8).to("cuda")
    d_out = torch.from_numpy(P.canary(size)).to("cuda")
    d_st = torch.full((n,), -999, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dev.decode_blocks_device(d_comp.data_ptr(), d_jobs.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr(), bs, False, 0)
    torch.cuda.synchronize()
    P.check_guarded(case, d_out.cpu().numpy(), d_st.cpu().numpy(), case.label)
    assert np.array_equal(d_st.cpu().numpy(), case.want_rc)
