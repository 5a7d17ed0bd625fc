"""Throughput of zxc_mi355x_decompress_device (a whole archive, HBM to HBM) against zxc_mi355x_decode_blocks_device with a job table
the host made from the same archive (the device-resident path without this call), and the cost of the header walk that
non-seekable archives take. hipEvent timing on one stream, warm-up runs, then --runs timed repetitions with the two sides
alternating; medians, and the spread of the baseline's own repetitions beside the ratio. The decoded bytes are checked against
the source before and after the timed runs. One JSON line per block size.

    python tools/bench_decompress_device.py [--mib 1024] [--level 3] [--block-sizes 65536,524288] [--runs 30] [--warmup 3]

The source is --mib MiB of the synth_silesia class mix (corpus tiles, generated on a process pool), archived on the device by
compress_device, once seekable and once not. walk_ns_per_block is (non-seekable call - seekable call) / blocks: the two calls differ
in the container stages alone. The stages by kernel: `rocprofv3 --kernel-trace --stats -- python tools/bench_decompress_device.py
--runs 3` lists zxc_unframe_* beside the decode kernels."""
import argparse
import ctypes as C
import json
import multiprocessing
import os
import statistics
import sys

import torch  # (first: the library shares torch's HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import devbench  # noqa: E402
import zxc_amd  # noqa: E402
from zxc_amd import corpus  # noqa: E402


def source(n):
    tiles = -(-n // corpus.TILE_BYTES)
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        parts = [corpus.synth_silesia_tile(t, pool=pool) for t in range(tiles)]
    return b"".join(parts)[:n]


def alternating(fns, runs, warmup, stream):
    """-> one list of hipEvent milliseconds per function; run i times every function once, in turn"""
    return devbench.alternating(fns, runs, warmup, stream, "event")


def archive_on_device(src, n, level, bs, seekable, checksum, stream):
    """-> (tensor with the archive and 64 readable bytes behind it, archive size)"""
    cap = int(zxc_amd.lib().zxc_compress_bound(n))
    ws = zxc_amd.compress_device_work_size(n, level, bs, seekable, checksum)
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    arc = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    res = torch.zeros(1, dtype=torch.int64, device="cuda")
    zxc_amd.compress_device(src.data_ptr(), n, arc.data_ptr(), cap, work.data_ptr(), ws, res.data_ptr(), level, bs, seekable, checksum,
                            stream.cuda_stream)
    size = int(res.item())
    assert size > 0, size
    return arc, size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--block-sizes", default="65536,524288")
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--checksum", action="store_true")
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
        arc, size = archive_on_device(src, n, a.level, bs, True, a.checksum, stream)
        walk_arc, walk_size = archive_on_device(src, n, a.level, bs, False, a.checksum, stream)
        # the path without the new call: a host copy of the archive, a seekable handle, a job table, uploaded
        host = bytes(arc[:size].cpu().numpy())
        s = zxc_amd.Seekable(host)
        jobs_h = s.plan()
        s.close()
        assert len(jobs_h) == nb
        jobs = torch.frombuffer(bytearray(jobs_h.tobytes()), dtype=torch.uint8).to("cuda")
        status = torch.empty(nb, dtype=torch.int32, device="cuda")
        out_b = torch.zeros(nb * bs + 64, dtype=torch.uint8, device="cuda")
        ws = zxc_amd.decompress_device_work_size(size, n, bs)
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        out_d = torch.zeros(n, dtype=torch.uint8, device="cuda")
        out_w = torch.zeros(n, dtype=torch.uint8, device="cuda")
        res = torch.zeros(2, dtype=torch.int64, device="cuda")

        def baseline():
            zxc_amd.decode_blocks_device(arc.data_ptr(), jobs.data_ptr(), nb, out_b.data_ptr(), status.data_ptr(), bs, a.checksum,
                                         stream.cuda_stream)

        def whole():
            zxc_amd.decompress_device(arc.data_ptr(), size, out_d.data_ptr(), n, bs, work.data_ptr(), ws, res.data_ptr(), a.checksum,
                                      stream.cuda_stream)

        def walk():
            zxc_amd.decompress_device(walk_arc.data_ptr(), walk_size, out_w.data_ptr(), n, bs, work.data_ptr(), ws, res[1:].data_ptr(),
                                      a.checksum, stream.cuda_stream)

        def check(when):
            baseline(), whole(), walk()
            stream.synchronize()
            assert res.tolist() == [n, n], (when, res.tolist())
            assert int(status.min().item()) > 0, when
            for o in (out_b[:n], out_d, out_w):
                assert torch.equal(o, src), when
            out_b.zero_(), out_d.zero_(), out_w.zero_()

        check("before")
        base_ms, whole_ms, walk_ms = alternating((baseline, whole, walk), a.runs, a.warmup, stream)
        check("after")
        q, qd = statistics.quantiles(base_ms, n=10), statistics.quantiles(whole_ms, n=10)
        b_med, d_med, w_med = statistics.median(base_ms), statistics.median(whole_ms), statistics.median(walk_ms)
        line = {"block_size": bs, "level": a.level, "blocks": nb, "decoded_bytes": n, "archive_bytes": size, "runs": a.runs,
                "checksum": bool(a.checksum),
                "decode_blocks_ms": round(b_med, 4), "decode_blocks_gbps": round(n / b_med / 1e6, 1),
                "decode_blocks_p10_ms": round(q[0], 4), "decode_blocks_p90_ms": round(q[-1], 4),
                "decode_blocks_spread": round((q[-1] - q[0]) / b_med, 4),
                "decompress_device_ms": round(d_med, 4), "decompress_device_p10_ms": round(qd[0], 4), "decompress_device_p90_ms": round(qd[-1], 4),
                "decompress_device_gbps": round(n / d_med / 1e6, 1),
                "ratio_to_decode_blocks": round(d_med / b_med, 4),
                "walk_call_ms": round(w_med, 4), "walk_call_gbps": round(n / w_med / 1e6, 1),
                "walk_ns_per_block": round((w_med - d_med) * 1e6 / nb, 1),
                "decode_blocks_min_ms": round(min(base_ms), 4), "decompress_device_min_ms": round(min(whole_ms), 4),
                "walk_call_min_ms": round(min(walk_ms), 4)}
        print(json.dumps(line), flush=True)
        del arc, walk_arc, jobs, status, out_b, out_d, out_w, work, res
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
