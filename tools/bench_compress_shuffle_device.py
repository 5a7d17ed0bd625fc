"""What the byte-shuffle filter buys and costs on tensors that lie in HBM: seeded bf16 and fp32 weights N(0, 0.02) and int64 ids below
50000, made on the device, and a generated text buffer (zxc_amd/corpus.py), where the filter must not be recommended. Per buffer,
level (3, 6, 7) and block size (64 KiB, 512 KiB), alternating in one process:
  compress_device  against  compress_shuffle_device   -> ratio (source bytes / archive bytes) and GB/s of source
  decompress_device  against  decompress_shuffle_device  -> GB/s of decoded bytes
and the two kernels alone against a device-to-device copy of the same bytes, per element size and unit, on a buffer past the
Infinity Cache: GB/s of bytes read plus bytes written. Wall-clock from the first enqueue to the stream's end for the calls, hipEvent
time for the kernels; warm-up runs, then --runs timed repetitions; medians and p10 / p90. Every round trip is compared with the
source before the timed runs. One JSON line per row, printed and appended to --out. No threshold gates anything.

    python tools/bench_compress_shuffle_device.py [--mib 64] [--kernel-mib 1024] [--levels 3,6,7] [--blocks 65536,524288]
                                                  [--runs 7] [--warmup 2] [--out profiles/compress_shuffle_device_bench.jsonl]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch  # (first: the library shares torch's HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import devbench  # noqa: E402
import zxc_amd  # noqa: E402
from devbench import pct  # noqa: E402
from zxc_amd import corpus  # noqa: E402


def buffers(n, seed):
    """-> [(name, elem_size, uint8 tensor of n bytes with 64 readable bytes behind it)]"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.randn(n // 2, device="cuda", generator=g) * 0.02
    ids = torch.randint(0, 50000, (n // 8,), device="cuda", generator=g, dtype=torch.int64)
    text = torch.frombuffer(bytearray(corpus.synth_text(min(n, 16 << 20), seed=seed)), dtype=torch.uint8).to("cuda")
    out = []
    for name, E, raw in (("bf16 weights", 2, w.to(torch.bfloat16).view(torch.uint8)), ("fp32 weights", 4, w[: n // 4].contiguous().view(torch.uint8)),
                         ("int64 ids < 50000", 8, ids.view(torch.uint8)), ("text", 4, text.repeat(-(-n // text.numel()))[:n])):
        t = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
        t[:n] = raw[:n]
        out.append((name, E, t))
    return out


def stats(ms, nbytes, prefix):
    walls = sorted(ms)
    med = statistics.median(walls)
    return {prefix + "_ms": round(med, 3), prefix + "_ms_p10": round(pct(walls, 0.1), 3), prefix + "_ms_p90": round(pct(walls, 0.9), 3),
            prefix + "_gbps": round(nbytes / med / 1e6, 2)}


def archive_case(name, E, src, n, level, bs, a, stream):
    sp = stream.cuda_stream
    cap = int(zxc_amd.lib().zxc_compress_bound(n))
    ws_c = zxc_amd.compress_device_work_size(n, level, bs, True, False)
    ws_s = zxc_amd.compress_shuffle_device_work_size(n, 0, 0, level, bs, True, False)
    ws_d = zxc_amd.decompress_device_work_size(cap, n, bs)
    ws_u = zxc_amd.decompress_shuffle_device_work_size(cap, n, 0, bs)
    work = torch.empty(max(ws_c, ws_s, ws_d, ws_u), dtype=torch.uint8, device="cuda")
    arc_p, arc_s = (torch.zeros(cap + 64, dtype=torch.uint8, device="cuda") for _ in range(2))
    res = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")

    def plain():
        zxc_amd.compress_device(src.data_ptr(), n, arc_p.data_ptr(), cap, work.data_ptr(), ws_c, res.data_ptr(), level, bs, True, False, sp)

    def shuffled():
        zxc_amd.compress_shuffle_device(src.data_ptr(), n, E, arc_s.data_ptr(), cap, work.data_ptr(), ws_s, res.data_ptr(), 0, None, level, bs,
                                        True, False, sp)

    plain()
    n_plain = int(res.item())
    shuffled()
    n_shuf = int(res.item())
    assert n_plain > 0 and n_shuf > 0, (n_plain, n_shuf)

    def unplain():
        zxc_amd.decompress_device(arc_p.data_ptr(), n_plain, out.data_ptr(), n, bs, work.data_ptr(), ws_d, res.data_ptr(), False, sp)

    def unshuffled():
        zxc_amd.decompress_shuffle_device(arc_s.data_ptr(), n_shuf, out.data_ptr(), n, E, bs, work.data_ptr(), ws_u, res.data_ptr(), 0, None,
                                          False, sp)

    for fn in (unplain, unshuffled):  # both give the source back
        out.zero_()
        fn()
        assert int(res.item()) == n and torch.equal(out[:n], src[:n]), (name, level, bs, fn.__name__)
    ms = devbench.alternating([plain, shuffled, unplain, unshuffled], a.runs, a.warmup, stream, "wall")
    line = {"kind": "archive", "data": name, "elem_size": E, "bytes": n, "level": level, "block_size": bs, "runs": a.runs,
            "ratio_plain": round(n / n_plain, 4), "ratio_shuffle": round(n / n_shuf, 4), "work_bytes_plain": ws_c, "work_bytes_shuffle": ws_s}
    for prefix, m in zip(("compress", "compress_shuffle", "decompress", "decompress_shuffle"), ms):
        line.update(stats(m, n, prefix))
    return line


def kernel_case(E, unit, src, dst, n, a, stream):
    sp = stream.cuda_stream
    fns = [lambda: zxc_amd.shuffle_device(src.data_ptr(), dst.data_ptr(), n, E, unit, sp),
           lambda: zxc_amd.unshuffle_device(src.data_ptr(), dst.data_ptr(), n, E, unit, sp),
           lambda: dst[:n].copy_(src[:n], non_blocking=True)]
    ms = devbench.alternating(fns, a.runs, a.warmup, stream, "event")
    line = {"kind": "kernel", "elem_size": E, "unit": unit, "bytes": n, "runs": a.runs}
    for prefix, m in zip(("shuffle", "unshuffle", "copy"), ms):
        line.update(stats(m, 2 * n, prefix))  # bytes read plus bytes written
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--kernel-mib", type=int, default=1024)
    ap.add_argument("--levels", default="3,6,7")
    ap.add_argument("--blocks", default="65536,524288", help="comma-separated block sizes")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "compress_shuffle_device_bench.jsonl"))
    a = ap.parse_args()
    L = zxc_amd.lib()
    if L.zxc_mi355x_device_count() < 1:
        raise SystemExit("no HIP device")
    L.zxc_mi355x_set_device(0)
    L.zxc_compress_bound.restype = ctypes.c_uint64
    L.zxc_compress_bound.argtypes = [ctypes.c_size_t]
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")

    n = a.kernel_mib << 20
    src = torch.randint(0, 256, (n,), device="cuda", dtype=torch.uint8)
    dst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    for E in (2, 4, 8):
        for unit in (int(x) for x in a.blocks.split(",")):
            emit(kernel_case(E, unit, src, dst, n, a, stream))
    del src, dst
    torch.cuda.empty_cache()
    n = a.mib << 20
    for name, E, t in buffers(n, a.seed):
        for bs in (int(x) for x in a.blocks.split(",")):
            for level in (int(x) for x in a.levels.split(",")):
                emit(archive_case(name, E, t, n, level, bs, a, stream))
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
