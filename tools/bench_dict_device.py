"""What a dictionary in device memory buys and costs: for one corpus of small records, at 4 KiB and 64 KiB blocks and levels 3 and 7,
the archive size with and without the dictionary, the throughput of compress_dict_device, decompress_dict_device and
decompress_ranges_dict_device beside their siblings without a dictionary on the same data, and the time of dict_prepare_device.
hipEvent timing on one stream, warm-up runs, then --runs timed repetitions with the two sides alternating; medians. Every decoded
byte is checked against the source before the timed runs. One JSON line per (block size, level), printed and appended to --out.

    python tools/bench_dict_device.py [--mib 64] [--block-sizes 4096,65536] [--levels 3,7] [--runs 10] [--warmup 2]
                                      [--out profiles/dict_device_bench.jsonl]

The corpus is --mib MiB of JSON-like log records of 150-400 bytes drawn from a fixed vocabulary (seeded); the dictionary is 65 535
bytes of records drawn the same way with another seed, used as raw content without a shared literal table. The ranges calls fetch
--ranges ranges of --range-len bytes at random offsets, dst_off = offset (mod 16)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch  # (first: the library shares torch's HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import devbench  # noqa: E402
import zxc_amd  # noqa: E402

PATHS = ["/api/v1/users", "/api/v1/orders", "/api/v2/items/search", "/static/js/app.bundle.js", "/healthz", "/api/v1/sessions/refresh",
         "/api/v2/cart/checkout", "/img/products/thumb"]
AGENTS = ["Mozilla/5.0 (X11; Linux x86_64) AppleWebKit/537.36 (KHTML, like Gecko) Chrome/126.0 Safari/537.36",
          "Mozilla/5.0 (Macintosh; Intel Mac OS X 14_5) AppleWebKit/605.1.15 (KHTML, like Gecko) Version/17.5 Safari/605.1.15",
          "curl/8.5.0", "python-requests/2.32.3", "okhttp/4.12.0"]
METHODS = ["GET", "GET", "GET", "POST", "PUT", "DELETE"]
REGIONS = ["eu-west-1", "us-east-1", "us-west-2", "ap-southeast-2"]


def records(n_bytes, seed):
    rng = np.random.default_rng(seed)
    out, size = [], 0
    while size < n_bytes:
        k = rng.integers(0, 1 << 30, 8)
        rec = ('{"ts":"2025-03-%02dT%02d:%02d:%02d.%03dZ","region":"%s","method":"%s","path":"%s/%d","status":%d,"bytes":%d,'
               '"latency_us":%d,"user":"u%08x","agent":"%s","trace":"%016x"}\n' %
               (1 + k[0] % 28, k[1] % 24, k[2] % 60, k[3] % 60, k[4] % 1000, REGIONS[k[5] % 4], METHODS[k[6] % 6], PATHS[k[7] % 8], k[0] % 100000,
                (200, 200, 200, 204, 301, 404, 500)[k[1] % 7], k[2] % 200000, k[3] % 900000, k[4], AGENTS[k[5] % 5], int(k[6]) << 20 | int(k[7])))
        out.append(rec.encode())
        size += len(out[-1])
    return b"".join(out)[:n_bytes]


def alternating(fns, runs, warmup, stream):
    """-> the median hipEvent milliseconds of every function; run i times every function once, in turn"""
    return [statistics.median(m) for m in devbench.alternating(fns, runs, warmup, stream, "event")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--block-sizes", default="4096,65536")
    ap.add_argument("--levels", default="3,7")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ranges", type=int, default=8192)
    ap.add_argument("--range-len", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dict_device_bench.jsonl"))
    a = ap.parse_args()
    L = zxc_amd.lib()
    if L.zxc_mi355x_device_count() < 1:
        raise SystemExit("no HIP device")
    L.zxc_mi355x_set_device(0)
    torch.cuda.set_device(0)
    L.zxc_compress_bound.restype = C.c_uint64
    L.zxc_dict_id.restype = C.c_uint32
    L.zxc_dict_id.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p]
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    n = a.mib << 20
    src = torch.frombuffer(bytearray(records(n, 1)), dtype=torch.uint8).to("cuda")
    content = records(65535, 2)
    d_content = torch.frombuffer(bytearray(content), dtype=torch.uint8).to("cuda")
    d_id = torch.zeros(1, dtype=torch.int32, device="cuda")

    def prepare():
        zxc_amd.dict_prepare_device(d_content.data_ptr(), len(content), 0, d_id.data_ptr(), sp)

    prepare_ms = alternating((prepare,), max(a.runs, 20), a.warmup, stream)[0]
    assert int(d_id.cpu().numpy().view(np.uint32)[0]) == L.zxc_dict_id(content, len(content), None)
    dd = (d_content.data_ptr(), len(content), 0, d_id.data_ptr())
    cap = int(L.zxc_compress_bound(n))
    rng = np.random.default_rng(3)
    table = np.zeros(a.ranges, dtype=zxc_amd.RANGE_DTYPE)
    table["offset"] = rng.integers(0, n - a.range_len, a.ranges)
    table["len"] = a.range_len
    slot = (a.range_len + 31) // 16 * 16
    table["dst_off"] = np.arange(a.ranges, dtype=np.uint64) * slot + (table["offset"] & 15)
    d_ranges = torch.from_numpy(table.view(np.uint8).copy()).to("cuda")
    rcap = a.ranges * slot + 64

    for bs in map(int, a.block_sizes.split(",")):
        nb = -(-n // bs)
        for level in map(int, a.levels.split(",")):
            ws_c = zxc_amd.compress_dict_device_work_size(n, len(content), level, bs, True, False)
            ws_p = zxc_amd.compress_device_work_size(n, level, bs, True, False)
            work_c = torch.empty(ws_c, dtype=torch.uint8, device="cuda")
            arc_d = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
            arc_p = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
            res = torch.zeros(4, dtype=torch.int64, device="cuda")

            def comp_dict():
                zxc_amd.compress_dict_device(src.data_ptr(), n, arc_d.data_ptr(), cap, dd, work_c.data_ptr(), ws_c, res.data_ptr(), level, bs,
                                             True, False, sp)

            def comp_plain():
                zxc_amd.compress_device(src.data_ptr(), n, arc_p.data_ptr(), cap, work_c.data_ptr(), ws_p, res[1:].data_ptr(), level, bs, True,
                                        False, sp)

            c_dict_ms, c_plain_ms = alternating((comp_dict, comp_plain), a.runs, a.warmup, stream)
            size_d, size_p = int(res[0].item()), int(res[1].item())
            assert size_d > 0 and size_p > 0, (size_d, size_p)
            del work_c

            ws_d = zxc_amd.decompress_device_work_size(size_d, n, bs)
            work_d = torch.empty(ws_d, dtype=torch.uint8, device="cuda")
            out = torch.zeros(n, dtype=torch.uint8, device="cuda")

            def dec_dict():
                zxc_amd.decompress_dict_device(arc_d.data_ptr(), size_d, out.data_ptr(), n, bs, dd, work_d.data_ptr(), ws_d, res[2:].data_ptr(),
                                               False, sp)

            def dec_plain():
                zxc_amd.decompress_device(arc_p.data_ptr(), size_p, out.data_ptr(), n, bs, work_d.data_ptr(), ws_d, res[3:].data_ptr(), False, sp)

            for fn, at in ((dec_dict, 2), (dec_plain, 3)):
                out.zero_()
                fn()
                stream.synchronize()
                assert int(res[at].item()) == n and torch.equal(out, src), (fn.__name__, int(res[at].item()))
            d_dict_ms, d_plain_ms = alternating((dec_dict, dec_plain), a.runs, a.warmup, stream)
            del work_d, out

            isz = zxc_amd.seekable_index_size(nb)
            ix_d = torch.zeros((isz + 7) // 8, dtype=torch.int64, device="cuda")
            ix_p = torch.zeros((isz + 7) // 8, dtype=torch.int64, device="cuda")
            zxc_amd.seekable_open_device(arc_d.data_ptr(), size_d, bs, nb, ix_d.data_ptr(), isz, sp)
            zxc_amd.seekable_open_device(arc_p.data_ptr(), size_p, bs, nb, ix_p.data_ptr(), isz, sp)
            ws_r = zxc_amd.decompress_ranges_device_work_size(a.ranges, a.range_len, bs)
            work_r = torch.empty(ws_r, dtype=torch.uint8, device="cuda")
            rdst = torch.zeros(rcap, dtype=torch.uint8, device="cuda")
            rres = torch.zeros(a.ranges, dtype=torch.int64, device="cuda")

            def rng_dict():
                zxc_amd.decompress_ranges_dict_device(arc_d.data_ptr(), size_d, ix_d.data_ptr(), d_ranges.data_ptr(), a.ranges, a.range_len,
                                                      rdst.data_ptr(), rcap, bs, dd, work_r.data_ptr(), ws_r, rres.data_ptr(), sp)

            def rng_plain():
                zxc_amd.decompress_ranges_device(arc_p.data_ptr(), size_p, ix_p.data_ptr(), d_ranges.data_ptr(), a.ranges, a.range_len,
                                                 rdst.data_ptr(), rcap, bs, work_r.data_ptr(), ws_r, rres.data_ptr(), sp)

            first = table[0]
            for fn in (rng_dict, rng_plain):
                rdst.zero_()
                fn()
                stream.synchronize()
                assert int(rres.min().item()) == a.range_len == int(rres.max().item()), fn.__name__
                o, d = int(first["offset"]), int(first["dst_off"])
                assert torch.equal(rdst[d: d + a.range_len], src[o: o + a.range_len]), fn.__name__
            r_dict_ms, r_plain_ms = alternating((rng_dict, rng_plain), a.runs, a.warmup, stream)
            rbytes = a.ranges * a.range_len

            def gbps(nbytes, ms):
                return round(nbytes / ms / 1e6, 2)

            line = {"corpus": "log records", "source_bytes": n, "block_size": bs, "level": level, "blocks": nb, "dict_bytes": len(content),
                    "runs": a.runs, "archive_bytes_dict": size_d, "archive_bytes_plain": size_p, "ratio_dict": round(n / size_d, 3),
                    "ratio_plain": round(n / size_p, 3), "dict_prepare_ms": round(prepare_ms, 4),
                    "compress_dict_ms": round(c_dict_ms, 3), "compress_dict_gbps": gbps(n, c_dict_ms),
                    "compress_plain_ms": round(c_plain_ms, 3), "compress_plain_gbps": gbps(n, c_plain_ms),
                    "decompress_dict_ms": round(d_dict_ms, 3), "decompress_dict_gbps": gbps(n, d_dict_ms),
                    "decompress_plain_ms": round(d_plain_ms, 3), "decompress_plain_gbps": gbps(n, d_plain_ms),
                    "ranges": a.ranges, "range_len": a.range_len,
                    "ranges_dict_ms": round(r_dict_ms, 3), "ranges_dict_gbps": gbps(rbytes, r_dict_ms),
                    "ranges_plain_ms": round(r_plain_ms, 3), "ranges_plain_gbps": gbps(rbytes, r_plain_ms)}
            text = json.dumps(line)
            print(text, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")
            del arc_d, arc_p, res, ix_d, ix_p, work_r, rdst, rres
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
