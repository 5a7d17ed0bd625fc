"""Throughput of zxc_mi355x_compress_device (a whole archive, HBM to HBM) against the block encoder alone
(zxc_mi355x_encode_blocks_device), on the same device-resident source: hipEvent timing on one stream, warm-up runs, then the
median of --runs. One JSON line per block size.

    python tools/compress_device_bench.py [--mib 1024] [--level 3] [--block-sizes 65536,4096] [--runs 20] [--warmup 3] [--check]

The source is --mib MiB of the synth_silesia class mix (corpus tiles, generated on a process pool). What the kernels after the
encode cost shows in `rocprofv3 --kernel-trace --stats -- python tools/compress_device_bench.py --runs 3`: the zxc_frame_*
kernels against zxc_encode_blocks_kernel_l*."""
import argparse
import ctypes as C
import json
import multiprocessing
import os
import statistics
import sys

import torch  # (first: the library shares torch's HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zxc_amd  # noqa: E402
from zxc_amd import corpus  # noqa: E402


def source(n):
    tiles = -(-n // corpus.TILE_BYTES)
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        parts = [corpus.synth_silesia_tile(t, pool=pool) for t in range(tiles)]
    return b"".join(parts)[:n]


def timed(fn, runs, warmup, stream):
    for _ in range(warmup):
        fn()
    stream.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return statistics.median(ms), ms[0], ms[round(0.1 * (len(ms) - 1))], ms[round(0.9 * (len(ms) - 1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--block-sizes", default="65536,4096")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--checksum", action="store_true")
    ap.add_argument("--no-seekable", action="store_true")
    ap.add_argument("--check", action="store_true", help="compare one archive per block size with zxc_compress")
    a = ap.parse_args()
    L = zxc_amd.lib()
    if L.zxc_mi355x_device_count() < 1:
        raise SystemExit("no HIP device")
    L.zxc_mi355x_set_device(0)
    torch.cuda.set_device(0)
    L.zxc_mi355x_encode_slot_stride.restype = C.c_uint32
    L.zxc_mi355x_encode_blocks_device.restype = C.c_int
    L.zxc_mi355x_encode_blocks_device.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                  C.c_void_p]
    L.zxc_compress_bound.restype = C.c_uint64
    n = a.mib << 20
    data = source(n)
    stream = torch.cuda.current_stream()
    # (+64: the block encoder alone reads up to 32 bytes past its input; compress_device is given exactly n)
    src = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    src[:n] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")
    seekable, checksum = not a.no_seekable, a.checksum
    for bs in map(int, a.block_sizes.split(",")):
        nb = -(-n // bs)
        slots = torch.empty(nb * int(L.zxc_mi355x_encode_slot_stride(bs)), dtype=torch.uint8, device="cuda")
        sizes = torch.empty(nb, dtype=torch.int32, device="cuda")

        def encode():
            rc = L.zxc_mi355x_encode_blocks_device(src.data_ptr(), n, bs, a.level, int(checksum), slots.data_ptr(), sizes.data_ptr(),
                                                   stream.cuda_stream)
            assert rc == 0, rc

        enc_ms, enc_min, _, _ = timed(encode, a.runs, a.warmup, stream)
        del slots, sizes
        ws = zxc_amd.compress_device_work_size(n, a.level, bs, seekable, checksum)
        cap = int(L.zxc_compress_bound(n))
        work = torch.empty(ws, dtype=torch.uint8, device="cuda")
        dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
        res = torch.zeros(1, dtype=torch.int64, device="cuda")

        def whole():
            zxc_amd.compress_device(src.data_ptr(), n, dst.data_ptr(), cap, work.data_ptr(), ws, res.data_ptr(), a.level, bs,
                                    seekable, checksum, stream.cuda_stream)

        cd_ms, cd_min, cd_p10, cd_p90 = timed(whole, a.runs, a.warmup, stream)
        size = int(res.item())
        assert size > 0, size
        line = {"block_size": bs, "level": a.level, "src_bytes": n, "archive_bytes": size, "ratio": round(n / size, 3),
                "runs": a.runs, "encode_ms": round(enc_ms, 3), "encode_gbps": round(n / enc_ms / 1e6, 2),
                "compress_device_ms": round(cd_ms, 3), "compress_device_gbps": round(n / cd_ms / 1e6, 2),
                "after_encode_share": round((cd_ms - enc_ms) / enc_ms, 4), "encode_min_ms": round(enc_min, 3),
                "compress_device_min_ms": round(cd_min, 3), "compress_device_ms_p10": round(cd_p10, 3),
                "compress_device_ms_p90": round(cd_p90, 3)}
        if a.check:
            want = zxc_amd.compress(data, a.level, bs, seekable, checksum)
            line["matches_zxc_compress"] = bytes(dst[:size].cpu().numpy()) == want
        print(json.dumps(line), flush=True)
        del work, dst, res
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
