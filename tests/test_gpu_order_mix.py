"""The mixed launch order (zxc_dev_order_mix, zxc_amd/csrc/zxc_dev.h) on the device: one launch of 4 KiB blocks just above
2 x residency + rows for the lean kernel's residency on this device, where the head of the launch is dealt into rows with a
ragged last column and meets the heaviest-first tail. Levels 1, 3 and 5 plus RAW blocks, a few of them damaged; statuses and
bytes equal the oracle's, and no byte outside a block's slot changes (tests/decode_plan_cases.py). Plain, and with per-block
checksums (a second launch on the stream then verifies them in zxc_block_checksum_kernel, which walks order[] in sorted order)."""
import os
import random

import numpy as np
import pytest

import decode_plan_cases as P
from conftest import ROOT
from decode_harness import Runner, _hip, new_stream

pytestmark = pytest.mark.gpu

BS = 4096


def _define(name, path):
    src = open(os.path.join(ROOT, "zxc_amd", "csrc", path)).read()
    return int(src.split(f"#define {name} ")[1].split()[0].rstrip("u"))


@pytest.mark.parametrize("checksum", [False, True], ids=["plain", "checksum"])
def test_launch_just_above_two_residencies(product, oracle, ref, checksum):
    import torch
    assert product.lib().zxc_mi355x_device_count() >= 1, "no HIP device"
    product.lib().zxc_mi355x_set_device(0)
    rows = _define("ZXC_DEV_ORDER_MIX_ROWS", "zxc_dev.h")
    # the lean kernel's residency: one wavefront per block, __launch_bounds__(64, LEAN_WAVES_PER_SIMD) on 4 SIMDs per CU
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    slots = cus * 4 * _define("LEAN_WAVES_PER_SIMD", "zxc_decode_kernel.hip")
    n = 2 * slots + rows + 7
    # (the library asks the runtime for the residency. Should it report fewer wavefronts per CU than the launch bounds allow, the
    #  head only grows: it still meets the tail inside this launch, and its last column is ragged for every such value)
    assert all((n - 2 * cus * w) % rows for w in range(1, slots // cus + 1)), "a ragged last column"
    # distinct blocks once (their verdicts from the oracle), repeated in a seeded shuffle up to n jobs
    rnd = np.random.default_rng(23).integers(0, 256, 6 * BS, dtype=np.uint8).tobytes()  # incompressible: RAW blocks
    pieces = []
    for level in (1, 3, 5):
        comp = P.ref_archive(ref, P.corpus_bytes(160 * BS - 13, seed=5 + level) + rnd, level, BS, checksum)
        jobs, bs, ck = P.seek_jobs(oracle, comp)
        assert bs == BS and ck == checksum
        pieces.append((comp, jobs))
    comp, jobs = P.concat(*pieces)
    comp, hit = P.mutate(comp, jobs, random.Random(7), 12, checksum)
    base = P.make_case(oracle, comp, jobs, BS, checksum, "order mix base", hit=hit)
    t, _, _ = P.block_fields(base.comp, base.jobs)
    assert (t == 0).sum() >= 6 and (t == 1).sum() >= 100 and (t == 2).sum() >= 100, "RAW, GLO and GHI blocks"
    idx = np.random.default_rng(5).integers(0, base.n, n)
    idx[:base.n] = np.arange(base.n)  # every distinct block at least once
    rows_ = base.jobs[idx].copy()
    case = P.Case(base.comp, rows_, BS, checksum, base.want_rc[idx], [base.want[i] for i in idx], label=f"order mix {n} jobs")
    P.require(case, failed=4, n_jobs=2 * slots + rows + 1)
    torch.cuda.synchronize()
    product.lib().zxc_mi355x_release_cached()  # (the host API's idle arenas give their streams' order slots back)
    stream = new_stream(_hip())
    Runner(product).run(case, stream, "mixed order")
    if checksum:  # (the stream's second launch knows there is no PivCo block: checksums by their own kernel, through order[] as well)
        Runner(product).run(case, stream, "mixed order, checksum kernel")
