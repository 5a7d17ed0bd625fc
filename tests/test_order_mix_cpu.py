"""zxc_dev_order_mix (zxc_amd/csrc/zxc_dev.h), the position transform of the launch-order pass, compiled for the host: a
bijection, the identity for short launches, the tail left heaviest-first, and on the bench corpus' block costs (tile 0's n_seq
per block as the reference encoded it, tests/golden/order_mix, tiled 41 times) every window of one residency and every XCD
gets the same share of the work. No GPU."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

SLOTS = (64, 6144)
N_BENCH, SLOTS_BENCH = 132594, 6144  # the headline launch: 41 tiles of 3 234 blocks, 256 CUs x 24 resident wavefronts


@pytest.fixture(scope="module")
def mix(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("order_mix") / "liborder_mix_shim.so")
    subprocess.run(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", so,
                    os.path.join(ROOT, "tests", "order_mix", "order_mix_shim.c")], check=True)
    S = C.CDLL(so)
    S.t_order_mix_rows.restype = C.c_uint32
    S.t_order_mix_all.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]

    def all_positions(n, slots):
        out = np.empty(n, dtype=np.uint32)
        S.t_order_mix_all(n, slots, out.ctypes.data)
        return out
    all_positions.rows = S.t_order_mix_rows()
    return all_positions


def _sizes(rows, slots):
    return sorted({1, 2, rows - 1, rows, rows + 1, 2 * slots - 1, 2 * slots, 2 * slots + 1, 2 * slots + rows + 1, N_BENCH})


@pytest.mark.parametrize("slots", SLOTS)
def test_bijection_identity_and_tail(mix, slots):
    assert mix.rows % 2 == 1 and all(mix.rows % p for p in range(3, mix.rows, 2)), "the row count is an odd prime (XCD balance)"
    for n in _sizes(mix.rows, slots):
        j = mix(n, slots)
        assert np.array_equal(np.sort(j), np.arange(n, dtype=np.uint32)), (n, slots, "not a permutation of [0, n)")
        tail = min(n, 2 * slots)
        assert np.array_equal(j[n - tail:], np.arange(n - tail, n, dtype=np.uint32)), (n, slots, "the tail moved")
        if n <= 2 * slots:
            assert np.array_equal(j, np.arange(n, dtype=np.uint32)), (n, slots, "a short launch is not left alone")
        else:
            assert np.array_equal(mix(n, 0), np.arange(n, dtype=np.uint32)), (n, "slots == 0 must not mix")


def test_bench_corpus_windows_and_xcds(mix):
    """Costs in launch order: the counting sort's key is the 64-value bucket of zxc_decode_kernel.hip (n_seq * 320 / block_size
    for blocks with raw sections), ties in any order (here: file order)."""
    n_seq = np.array(json.load(open(os.path.join(GOLDEN, "order_mix", "tile0_l3_b64k_nseq.json")))["n_seq"], dtype=np.int64)
    assert n_seq.size * 41 == N_BENCH
    cost = np.tile(n_seq, 41)
    bucket = 63 - np.minimum(cost * 320 // 65536, 63)
    sorted_cost = cost[np.argsort(bucket, kind="stable")]  # heaviest first
    launch = np.empty(N_BENCH, dtype=np.int64)
    launch[mix(N_BENCH, SLOTS_BENCH)] = sorted_cost
    head = N_BENCH - 2 * SLOTS_BENCH
    c = np.concatenate([[0], np.cumsum(launch[:head])])
    windows = c[SLOTS_BENCH:] - c[:-SLOTS_BENCH]  # every window of one residency inside the head
    dev = np.abs(windows / windows.mean() - 1).max()
    print(f"windows of {SLOTS_BENCH} head positions: {windows.size}, largest deviation from their mean {100 * dev:.2f} %")
    assert dev <= 0.05
    for name, part in (("head", launch[:head]), ("launch", launch)):
        per_xcd = np.bincount(np.arange(part.size) % 8, weights=part, minlength=8)
        dev = np.abs(per_xcd / per_xcd.mean() - 1).max()
        print(f"{name}: cost per XCD, largest deviation from the mean {100 * dev:.3f} %")
        assert dev <= 0.01
    # what the transform is for: in sorted order the same windows run from the heaviest blocks to the lightest
    c = np.concatenate([[0], np.cumsum(sorted_cost[:head])])
    windows = c[SLOTS_BENCH:] - c[:-SLOTS_BENCH]
    assert windows.max() / windows.min() > 1.5
