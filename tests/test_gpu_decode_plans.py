"""Every launch plan of decode_launch() (zxc_amd/csrc/zxc_hip_shim.hip) on the device, driven through named launch
sequences, with guarded outputs (tests/decode_plan_cases.py): after every launch no byte outside
[out_off, out_off + round_up(out_len, 16)) of any block changed, and every block has the reference's verdict.

The plan of a launch follows what the previous launch on the same stream found (pinned hint words of the stream's
launch-order slot). To make it deterministic every sequence runs on a stream of its own, created here with the HIP
runtime and never destroyed (a destroyed stream's handle can come back for a new stream and inherit the old slot), and
the device is synchronized between launches so that each hint has landed before the next launch reads it. A caller's
stream never gives its order slot back (only the library's own streams do) and a device has 16 of them: this module
takes 5 in the pytest process (S1-S5) and gives back the host API's idle ones first. S6 exhausts all 16, so it runs in a
child process: in this one it would change the plan of every later test.

  S1 PRE transitions   L7, L3, L7, L7 (64 KiB), L7 (2 MiB): full plan; PRE plan with no PRE block; plan without PRE blocks with
                       PivCo blocks in the full kernel; PRE plan again; PRE plan at the largest block size
  S2 checksums x PRE   checksummed L7, L3, L6, L7, L3, L6 with damaged blocks, the last one with ZXC_MI355X_CK_INLINE=1:
                       checksum kernel + merge pass beside PivCo blocks in the full kernel; inline checksums in the section /
                       lean_pre kernels; inline checksums in the plan without PRE blocks
  S3 RLE scratch       few RLE blocks, several hundred, the same again, then ZXC_MI355X_NO_RLE_SCRATCH=1: no RLE scratch;
                       scratch that runs out part way through the launch; scratch that fits; switched off
  S4 long launch       >= 16 400 level-3 blocks of 4 KiB with RLE blocks and mutants, twice: RLE blocks in the full kernel
                       beside the lean kernel, heaviest-first order over more than one round of workgroups
  S5 dictionary        >= 16 400 blocks of 4 KiB with a dictionary, without and with dict_huf, mutants: the dictionary kernel
                       behind the order pass, no list
  S6 no free slot      (child process) 16 streams take every slot, a 17th decodes S1's and S4's inputs: one plain kernel
"""
import os
import subprocess
import sys
import time

import pytest

if __name__ == "__main__":  # (S6's child process: the same paths conftest.py sets up)
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "oracle"), os.path.join(_ROOT, "tests")]

import decode_plan_cases as P
from decode_harness import Runner, _hip, new_stream

pytestmark = pytest.mark.gpu

BIG = (66 << 20) - 13  # 16 896 blocks of 4 KiB (> ZXC_RLE_LEAN_MAX_JOBS = 16 384, > 8 192 scratch slots), unaligned tail
MID = (8 << 20) - 13   # 128 blocks of 64 KiB


@pytest.fixture(scope="module")
def runner(product):
    import torch
    assert product.lib().zxc_mi355x_device_count() >= 1, "no HIP device"
    product.lib().zxc_mi355x_set_device(0)
    torch.cuda.synchronize()
    product.lib().zxc_mi355x_release_cached()  # (the host API's idle arenas give their streams' order slots back)
    return Runner(product)


@pytest.fixture(scope="module")
def hip(runner):
    return _hip()


def _timed(name):
    class T:
        def __enter__(self):
            self.t = time.time()

        def __exit__(self, *a):
            print(f"\n{name}: {time.time() - self.t:.1f} s")
    return T()


def s1_cases(oracle, ref):
    l7 = P.level_case(oracle, ref, 7, 65536, MID, n_hit=12)
    l3 = P.level_case(oracle, ref, 3, 65536, MID, n_hit=12)
    l7b = P.level_case(oracle, ref, 7, 2 << 20, (6 << 20) - 13, n_hit=1)
    P.require(l7, pivco=100, failed=3)
    P.require(l3, failed=3)
    assert P.pivco_mask(l3.comp, l3.jobs).sum() == 0  # (the PRE plan over it finds no PRE block)
    P.require(l7b, pivco=2)
    return l7, l3, l7b


def test_s1_pre_plan_transitions(runner, hip, oracle, ref):
    l7, l3, l7b = s1_cases(oracle, ref)
    st = new_stream(hip)
    with _timed("S1"):
        for k, case in enumerate((l7, l3, l7, l7, l7b)):
            runner.run(case, st, f"S1 launch {k + 1}")


def test_s2_checksums_across_plans(runner, hip, oracle, ref, monkeypatch):
    monkeypatch.delenv("ZXC_MI355X_CK_INLINE", raising=False)
    l7 = P.level_case(oracle, ref, 7, 65536, MID, checksum=True, n_hit=15)
    l3 = P.level_case(oracle, ref, 3, 65536, MID, checksum=True, n_hit=15)
    l6 = P.level_case(oracle, ref, 6, 65536, MID, checksum=True, n_hit=15)
    for c in (l7, l3, l6):
        P.require(c, failed=8)
    P.require(l7, pivco=100)
    P.require(l6, pivco=20)
    st = new_stream(hip)
    with _timed("S2"):
        for k, case in enumerate((l7, l3, l6, l7, l3)):
            runner.run(case, st, f"S2 launch {k + 1}")
        monkeypatch.setenv("ZXC_MI355X_CK_INLINE", "1")
        runner.run(l6, st, "S2 launch 6 (inline checksums)")


def test_s3_rle_scratch(runner, hip, oracle, ref, monkeypatch):
    monkeypatch.delenv("ZXC_MI355X_NO_RLE_SCRATCH", raising=False)
    few = P.rle_mix_case(oracle, ref, 4, 3000, n_hit=30, n_bytes=BIG, label="S3 few RLE")
    many = P.rle_mix_case(oracle, ref, 400, 3600, n_hit=40, n_bytes=BIG, label="S3 many RLE")
    P.require(few, rle=4, failed=5, unaligned_tail=False)
    P.require(many, rle=400, failed=5, n_jobs=257, unaligned_tail=False)
    assert many.n < 16384
    st = new_stream(hip)
    with _timed("S3"):
        runner.run(few, st, "S3 launch 1")
        runner.run(many, st, "S3 launch 2")
        runner.run(many, st, "S3 launch 3")
        monkeypatch.setenv("ZXC_MI355X_NO_RLE_SCRATCH", "1")
        runner.run(many, st, "S3 launch 4 (no RLE scratch)")


def s4_case(oracle, ref):
    c = P.level_case(oracle, ref, 3, 4096, BIG, n_hit=300, label="S4 L3/4K long")
    P.require(c, rle=100, failed=40, n_jobs=16400)
    return c


def test_s4_long_launch(runner, hip, oracle, ref):
    c = s4_case(oracle, ref)
    st = new_stream(hip)
    with _timed("S4"):
        runner.run(c, st, "S4 launch 1")
        runner.run(c, st, "S4 launch 2")


def test_s5_dictionary_long_launch(runner, hip, oracle, ref):
    plain = P.dict_case(oracle, ref, 3, 4096, BIG, False, n_hit=300, label="S5 dict")
    huf = P.Case(plain.comp, plain.jobs.copy(), plain.block_size, plain.checksum, *P.verdicts(oracle, plain.comp, plain.jobs, 4096, False,
                 plain.dict_, P.dictionary()[1], ref), dict_=plain.dict_, dict_huf=P.dictionary()[1], label="S5 dict+huf")
    for c in (plain, huf):
        P.require(c, rle=100, failed=40, n_jobs=16400)
    st = new_stream(hip)
    with _timed("S5"):
        runner.run(plain, st, "S5 launch 1")
        runner.run(huf, st, "S5 launch 2")


def test_s6_no_free_order_slot(runner):
    """In a child process (exhausting the slots would change the plan of every later test in this one)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "s6"], timeout=900, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "S6 ok" in r.stdout


def _s6_main():
    import oracle_py
    import torch  # (before the product library: one HIP runtime in the process)
    import zxc_amd
    zxc_amd.lib().zxc_mi355x_set_device(0)
    oracle, ref = oracle_py.Oracle(), oracle_py.Ref()
    runner = Runner(zxc_amd)
    H = _hip()
    tiny = P.level_case(oracle, ref, 3, 4096, 3 * 4096 - 13)
    streams = [new_stream(H) for _ in range(17)]
    for s in streams[:16]:  # a two-pass launch takes the stream's order slot
        runner.run(tiny, s, "S6 slot")
    l7, l3, _ = s1_cases(oracle, ref)
    for k, case in enumerate((l7, l3, s4_case(oracle, ref), l7)):
        runner.run(case, streams[16], f"S6 launch {k + 1}")
    torch.cuda.synchronize()
    print("S6 ok")


if __name__ == "__main__" and sys.argv[1:] == ["s6"]:
    _s6_main()
