"""Throughput of zxc_mi355x_decompress_ranges_device (many ranges of a seekable archive, HBM to HBM) against its lower bound:
zxc_mi355x_decode_blocks_device over the same covered blocks with a job table the host made, into whole slots, with no cut-out at
all. hipEvent timing on one stream, warm-up runs, then --runs timed repetitions with the sides alternating; medians and p10-p90 of
both, and the baseline's own spread beside the ratio. A plain device copy of as many bytes as the call's copy-out stage moves is
timed in the same alternation. The fetched bytes are checked against the source before and after the timed runs. One JSON line per
block size and case.

    python tools/bench_decompress_ranges_device.py [--mib 1024] [--level 3] [--block-sizes 65536,524288] [--runs 20] [--warmup 3]

Cases, seeded: small = 16 384 ranges of 16 KiB (max_len 16 KiB), small_wide = the same ranges with max_len 1 MiB (what the empty
jobs cost), aligned = 4 096 ranges of 1 MiB with dst_off = offset (mod 16), shifted = the same with dst_off off by one.
The stages by kernel: `rocprofv3 --kernel-trace --stats -- python tools/bench_decompress_ranges_device.py --runs 3` lists
zxc_ranges_* beside the decode kernels."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch  # (first: the library shares torch's HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zxc_amd  # noqa: E402
from bench_decompress_device import alternating, archive_on_device, source  # noqa: E402


def make_case(name, total, seed):
    """-> (offsets, lens, dst_offs, max_len)"""
    rng = np.random.default_rng(seed)
    if name.startswith("small"):
        n, ln = 16384, 16 << 10
        max_len = ln if name == "small" else 1 << 20
    else:
        n, ln, max_len = 4096, 1 << 20, 1 << 20
    a = rng.integers(0, total - ln, n).astype(np.int64)
    lens = np.full(n, ln, dtype=np.int64)
    stride = (ln + 63) // 16 * 16
    d = np.arange(n, dtype=np.int64) * stride + (a & 15) + (1 if name == "shifted" else 0)
    return a, lens, d, max_len


def staged_bytes(a, lens, d, bs):
    """bytes the copy-out stage moves: every covered block that is not decoded straight into the destination (zr_direct)"""
    n = 0
    for off, ln, dst in zip(a.tolist(), lens.tolist(), d.tolist()):
        for b in range(off // bs, (off + ln - 1) // bs + 1):
            lo = b * bs
            direct = lo >= off and lo + bs + 32 <= off + ln and (dst + lo - off) % 16 == 0
            if not direct:
                n += min(off + ln, lo + bs) - max(off, lo)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--block-sizes", default="65536,524288")
    ap.add_argument("--cases", default="small,small_wide,aligned,shifted")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    L = zxc_amd.lib()
    if L.zxc_mi355x_device_count() < 1:
        raise SystemExit("no HIP device")
    L.zxc_mi355x_set_device(0)
    torch.cuda.set_device(0)
    n = a.mib << 20
    data = source(n)
    stream = torch.cuda.current_stream()
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")
    del data
    for bs in map(int, a.block_sizes.split(",")):
        nb = -(-n // bs)
        arc, size = archive_on_device(src, n, a.level, bs, True, False, stream)
        isz = zxc_amd.seekable_index_size(nb)
        index = torch.zeros((isz + 7) // 8, dtype=torch.int64, device="cuda")
        zxc_amd.seekable_open_device(arc.data_ptr(), size, bs, nb, index.data_ptr(), isz, stream.cuda_stream)
        stream.synchronize()
        words = index.cpu().numpy()
        assert int(words[:1].view(np.int32)[0]) == 0, "open failed"
        offs = words[8: 8 + nb + 1].astype(np.int64)  # comp_offsets[] behind the 64-byte header
        for case in a.cases.split(","):
            off, lens, dsto, max_len = make_case(case, n, seed=bs + len(case))
            nr = len(off)
            cap = int(dsto[-1] + lens[-1])
            table = np.zeros(nr, dtype=zxc_amd.RANGE_DTYPE)
            table["offset"], table["len"], table["dst_off"] = off, lens, dsto
            rt = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
            ws = zxc_amd.decompress_ranges_device_work_size(nr, max_len, bs)
            work = torch.empty(ws, dtype=torch.uint8, device="cuda")
            dst = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
            res = torch.zeros(nr, dtype=torch.int64, device="cuda")
            # the lower bound: the covered blocks of every range, whole, back to back
            first, last = off // bs, (off + lens - 1) // bs
            cnt = last - first + 1
            blk = np.concatenate([np.arange(f, l + 1) for f, l in zip(first, last)])
            nj = len(blk)
            jobs_h = np.zeros(nj, dtype=zxc_amd.JOB_DTYPE)
            jobs_h["comp_off"], jobs_h["comp_size"] = offs[blk], offs[blk + 1] - offs[blk]
            jobs_h["out_off"], jobs_h["out_len"] = np.arange(nj, dtype=np.int64) * bs, bs
            jobs = torch.from_numpy(jobs_h.view(np.uint8).copy()).to("cuda")
            status = torch.empty(nj, dtype=torch.int32, device="cuda")
            out_b = torch.zeros(nj * bs + 64, dtype=torch.uint8, device="cuda")
            moved = staged_bytes(off, lens, dsto, bs)
            cp_src = torch.zeros(max(moved, 16), dtype=torch.uint8, device="cuda")
            cp_dst = torch.zeros_like(cp_src)

            def baseline():
                zxc_amd.decode_blocks_device(arc.data_ptr(), jobs.data_ptr(), nj, out_b.data_ptr(), status.data_ptr(), bs, False,
                                             stream.cuda_stream)

            def ranges():
                zxc_amd.decompress_ranges_device(arc.data_ptr(), size, index.data_ptr(), rt.data_ptr(), nr, max_len, dst.data_ptr(), cap,
                                                 bs, work.data_ptr(), ws, res.data_ptr(), stream.cuda_stream)

            def plain_copy():
                cp_dst.copy_(cp_src)

            def check(when):
                baseline(), ranges()
                stream.synchronize()
                assert int(status.min().item()) > 0, when
                assert np.array_equal(res.cpu().numpy(), lens), (when, case)
                slot = 0
                for i in range(nr):
                    if i % 4 == 0:
                        o, ln, d = int(off[i]), int(lens[i]), int(dsto[i])
                        assert torch.equal(dst[d: d + ln], src[o: o + ln]), (when, case, i)
                        at = slot * bs + o - int(first[i]) * bs
                        assert torch.equal(out_b[at: at + ln], src[o: o + ln]), (when, case, i)
                    slot += int(cnt[i])
                dst.zero_(), out_b.zero_(), res.zero_()

            check("before")
            base_ms, rng_ms, cp_ms = alternating((baseline, ranges, plain_copy), a.runs, a.warmup, stream)
            check("after")
            qb, qr = statistics.quantiles(base_ms, n=10), statistics.quantiles(rng_ms, n=10)
            b_med, r_med, c_med = statistics.median(base_ms), statistics.median(rng_ms), statistics.median(cp_ms)
            want = int(lens.sum())
            line = {"case": case, "block_size": bs, "level": a.level, "ranges": nr, "range_len": int(lens[0]), "max_len": max_len,
                    "jobs_launched": int(nr * ((max_len - 1) // bs + 2)), "blocks_covered": nj, "bytes_wanted": want, "runs": a.runs,
                    "work_bytes": ws,
                    "decode_blocks_ms": round(b_med, 4), "decode_blocks_p10_ms": round(qb[0], 4), "decode_blocks_p90_ms": round(qb[-1], 4),
                    "decode_blocks_spread": round((qb[-1] - qb[0]) / b_med, 4),
                    "ranges_ms": round(r_med, 4), "ranges_p10_ms": round(qr[0], 4), "ranges_p90_ms": round(qr[-1], 4),
                    "ranges_gbps_wanted": round(want / r_med / 1e6, 1), "ratio_to_decode_blocks": round(r_med / b_med, 4),
                    "extra_ms": round(r_med - b_med, 4), "copy_out_bytes": moved, "plain_copy_ms": round(c_med, 4),
                    "plain_copy_gbps": round(moved / c_med / 1e6, 1) if moved else None}
            print(json.dumps(line), flush=True)
            del rt, work, dst, res, jobs, status, out_b, cp_src, cp_dst
            torch.cuda.empty_cache()
        del arc, index
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
