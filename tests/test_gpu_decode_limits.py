"""The decode executors at their internal limits, on the device: the crafted blocks of tests/decode_limit_cases.py, packed into
one guarded job table per (family, block size) and route. After every launch no byte outside a block's slot may have changed,
every status is the reference's verdict and the bytes equal the plain Python expansion (never the product, never the
emulator). What the emulator cannot check is in the loop here: the far path's read-back of bytes the previous batch flushed
(a wave's stores and loads reach L2 in program order), the unconditional loads of idle lanes, non-temporal loads.

Routes: the default two-pass launch (lean executor); checksummed with the checksum kernel apart; checksummed with
ZXC_MI355X_CK_INLINE=1 (read on every launch); the dictionary launch (full executor; cases without a dictionary of their own
run behind a dummy one); the strict capacity of zxc_decompress_block_safe (the full kernel alone, which runs the lean
executor with strict checks: see "Decode executor routing" in DESIGN.md), one call per block.
Every launch is on the caller's default stream: the module takes no launch-order slot of its own. No case is built to fault:
every error case has a defined negative status and stays inside its slot."""
import numpy as np
import pytest

import decode_limit_cases as D
from decode_harness import dev, launch  # noqa: F401  (the device fixture and the guarded launch)

pytestmark = pytest.mark.gpu

FAMS = [f for f in D.FAMILIES if f != "dict"]


def tables(oracle, ref, fam, route, checksum=False):
    cases = D.fam_random(400) if fam == "random" else D.family(fam)
    assert D.groups(cases, route), (fam, route, "no case runs on this route")
    for group in D.groups(cases, route):
        yield D.pack(oracle, ref, group, route, checksum=checksum, label=f"{fam}/{group[0].bs >> 10}K [{route}{' ck' if checksum else ''}]")


@pytest.mark.parametrize("fam", FAMS + ["random"])
def test_two_pass_launch(dev, oracle, ref, fam, monkeypatch):  # noqa: F811
    monkeypatch.delenv("ZXC_MI355X_CK_INLINE", raising=False)
    for case, lc in tables(oracle, ref, fam, "lean"):
        launch(dev, case, lc, case.label)


@pytest.mark.parametrize("inline", [False, True], ids=["ck_apart", "ck_inline"])
@pytest.mark.parametrize("fam", FAMS + ["random"])
def test_checksummed_launch(dev, oracle, ref, fam, inline, monkeypatch):  # noqa: F811
    """The blocks carry trailers and the launch verifies them: beside the decode (zxc_block_checksum_kernel + merge), or
    inside the decode kernels. The environment is restored by monkeypatch."""
    if inline:
        monkeypatch.setenv("ZXC_MI355X_CK_INLINE", "1")
    else:
        monkeypatch.delenv("ZXC_MI355X_CK_INLINE", raising=False)
    for case, lc in tables(oracle, ref, fam, "lean", checksum=True):
        launch(dev, case, lc, case.label + (" inline" if inline else ""))


@pytest.mark.parametrize("fam", list(D.FAMILIES) + ["random"])
def test_dictionary_launch(dev, oracle, ref, fam):  # noqa: F811
    for case, lc in tables(oracle, ref, fam, "dict"):
        launch(dev, case, lc, case.label)


@pytest.mark.parametrize("fam", FAMS)
def test_strict_capacity_calls(dev, oracle, ref, fam):  # noqa: F811
    """zxc_decompress_block_safe, one call per block with dst_capacity = the block size: the strict-capacity plan (the full
    kernel alone, exact checks). Verdicts: the oracle's strict decoders, as in D.verdict(route='strict')."""
    import oracle_py
    api = oracle_py.BlockApi(dev.lib())
    try:
        for c in D.family(fam):
            if "strict" not in c.routes:
                continue
            blk = D.build_block(oracle, c)
            want_rc, want = D.verdict(oracle, None, blk, c, "strict")
            rc, got = api.decompress_block(blk, c.bs, safe=True)
            assert rc == want_rc, (c.name, "status", rc, want_rc)
            if c.valid:
                exp = D.expand(c.seqs, c.lits)
                assert want_rc == len(exp) and want == exp, (c.name, "the oracle differs from the plain expansion")
            if rc >= 0 and got != want:
                at = next(k for k in range(rc) if got[k] != want[k])
                raise AssertionError((c.name, "first differing byte", at, got[at], want[at], D.seq_at(c, at)))
    finally:
        api.close()


def _to_dev(data):
    import torch
    t = torch.full((len(data) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    t[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")
    return t


@pytest.mark.parametrize("fam", FAMS)
def test_whole_frames(dev, oracle, fam):  # noqa: F811
    """A handful of cases per family as one-block seekable frames through zxc_decompress, zxc_mi355x_decompress_device and
    zxc_mi355x_decompress_ranges_device (the whole block, and a slice out of its middle)."""
    import craft
    import torch
    picked = [c for c in D.family(fam) if c.valid and c.out_len is None and 20 <= len(D.expand(c.seqs, c.lits)) <= c.bs]
    picked = picked[:: max(1, len(picked) // 5)][:6]
    assert picked or fam == "errors", fam
    for c in picked:
        want = D.expand(c.seqs, c.lits)
        n, bs = len(want), c.bs
        f = craft.frame(oracle, [D.build_block(oracle, c)], bs.bit_length() - 1, n, seekable=True)
        assert oracle.decompress(f, n) == (n, want), (c.name, "the frame is not well-formed")
        assert dev.decompress(f) == want, (c.name, "zxc_decompress")
        arc = _to_dev(f)
        ws = dev.decompress_device_work_size(len(f), n, bs)
        assert ws > 0
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        dst = torch.full((n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        res = torch.full((1,), -999, dtype=torch.int64, device="cuda")
        dev.decompress_device(arc.data_ptr(), len(f), dst.data_ptr(), n, bs, work.data_ptr(), ws, res.data_ptr(), False, 0)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert int(res.cpu()[0]) == n and got[:n].tobytes() == want and (got[n:] == 0x5A).all(), (c.name, "decompress_device", int(res.cpu()[0]))
        isz = dev.seekable_index_size(4)
        index = torch.full(((isz + 7) // 8,), -1, dtype=torch.int64, device="cuda")
        dev.seekable_open_device(arc.data_ptr(), len(f), bs, 4, index.data_ptr(), isz, 0)
        a, ln = n // 3, max(1, n // 2)
        rt = np.zeros(2, dtype=[("offset", "<u8"), ("len", "<u8"), ("dst_off", "<u8")])
        rt[0], rt[1] = (0, n, 0), (a, ln, (n + 63) & ~63)
        cap = int(rt[1]["dst_off"]) + ln
        ws = dev.decompress_ranges_device_work_size(2, n, bs)
        assert ws > 0
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        dst = torch.full((cap + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        res = torch.full((2,), -999, dtype=torch.int64, device="cuda")
        d_rt = torch.from_numpy(rt.view(np.uint8).copy()).to("cuda")
        dev.decompress_ranges_device(arc.data_ptr(), len(f), index.data_ptr(), d_rt.data_ptr(), 2, n, dst.data_ptr(), cap, bs,
                                     work.data_ptr(), ws, res.data_ptr(), 0)
        torch.cuda.synchronize()
        got, r = dst.cpu().numpy().tobytes(), [int(x) for x in res.cpu().numpy()]
        assert r == [n, ln], (c.name, "decompress_ranges_device", r)
        assert got[:n] == want and got[int(rt[1]["dst_off"]):cap] == want[a:a + ln], (c.name, "decompress_ranges_device bytes")
