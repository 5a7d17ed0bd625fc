"""What a table of tensors costs the byte-shuffle calls on tensors that lie in HBM (include/zxc_mi355x_shufflev.h), alternating in
one process:
  (a) shufflev_device  against  shuffle_device  on the same bytes lying contiguous, a buffer past the Infinity Cache, per element size
      and table: 1 entry, entries of 4 MiB, entries of 4 KiB (the entries are the slots of one buffer in a seeded random order, so
      consecutive entries are not neighbours; the reference kernel reads the buffer front to back). hipEvent time of the whole call
      (the scan's three kernels, the gather-shuffle kernel, the status store); GB/s of bytes read plus bytes written; the ratio.
  (b) compress_shufflev_device  against  torch.cat into a fresh buffer + compress_shuffle_device, the path a caller had before:
      seeded bf16 weights N(0, 0.02) in --tensors tensors of their own, per level and block size. Wall-clock from the first enqueue
      to the stream's end, and the peak extra device memory of each path: the concatenated copy plus the work area, against the
      work area alone. The two archives are compared byte for byte before the timed runs.
Warm-up runs, then --runs timed repetitions; medians and p10 / p90. One JSON line per row, printed and appended to --out. No
threshold gates anything.

    python tools/bench_compress_shufflev_device.py [--mib 64] [--tensors 256] [--kernel-mib 1024] [--levels 3] [--blocks 524288,65536]
                                                   [--runs 7] [--warmup 2] [--out profiles/compress_shufflev_device_bench.jsonl]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch  # (first: the library shares torch's HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import devbench  # noqa: E402
import zxc_amd  # noqa: E402
from bench_compress_shuffle_device import stats  # noqa: E402


def table_of(rows):
    """[(address, length)] -> the table in device memory"""
    host = np.array(rows, dtype=zxc_amd.IOV_DTYPE)
    return torch.from_numpy(host.view(np.uint8).copy()).to("cuda")


def kernel_case(E, unit, src, dst, n, entry_bytes, a, stream):
    sp = stream.cuda_stream
    count = n // entry_bytes
    order = np.random.default_rng(a.seed).permutation(count) if count > 1 else np.zeros(1, dtype=np.int64)
    table = table_of([(src.data_ptr() + int(k) * entry_bytes, entry_bytes) for k in order])
    size = zxc_amd.shufflev_device_scratch_size(count)
    scratch = torch.empty(size, dtype=torch.uint8, device="cuda")
    res = torch.full((1,), -1, dtype=torch.int64, device="cuda")

    def gathered():
        zxc_amd.shufflev_device(table.data_ptr(), count, n, dst.data_ptr(), E, unit, scratch.data_ptr(), size, res.data_ptr(), sp)

    def contiguous():
        zxc_amd.shuffle_device(src.data_ptr(), dst.data_ptr(), n, E, unit, sp)

    # the same bytes as the sibling's kernel gives for the concatenation
    cat = src.view(count, entry_bytes)[torch.from_numpy(order).to("cuda")].reshape(-1)
    want = torch.empty_like(cat)
    zxc_amd.shuffle_device(cat.data_ptr(), want.data_ptr(), n, E, unit, sp)
    gathered()
    assert int(res.item()) == 0 and torch.equal(dst, want), (E, entry_bytes)
    del cat, want
    torch.cuda.empty_cache()
    ms = devbench.alternating([gathered, contiguous], a.runs, a.warmup, stream, "event")
    line = {"kind": "kernel", "elem_size": E, "unit": unit, "bytes": n, "entries": count, "entry_bytes": entry_bytes, "runs": a.runs,
            "scratch_bytes": size}
    for prefix, m in zip(("shufflev", "shuffle"), ms):
        line.update(stats(m, 2 * n, prefix))  # bytes read plus bytes written
    line["shufflev_over_shuffle"] = round(line["shufflev_ms"] / line["shuffle_ms"], 3)
    return line


def archive_case(tensors, n, level, bs, a, stream):
    sp = stream.cuda_stream
    E, count = 2, len(tensors)
    cap = int(zxc_amd.lib().zxc_compress_bound(n))
    ws_s = zxc_amd.compress_shuffle_device_work_size(n, 0, 0, level, bs, True, False)
    ws_v = zxc_amd.compress_shufflev_device_work_size(count, n, 0, 0, level, bs, True, False)
    work = torch.empty(max(ws_s, ws_v), dtype=torch.uint8, device="cuda")
    arc_s, arc_v = (torch.zeros(cap + 64, dtype=torch.uint8, device="cuda") for _ in range(2))
    res = torch.zeros(1, dtype=torch.int64, device="cuda")
    table = table_of([(t.data_ptr(), t.numel()) for t in tensors])

    def cat_then_shuffle():
        cat = torch.cat(tensors)  # a fresh buffer of n bytes: the copy the new call does without
        zxc_amd.compress_shuffle_device(cat.data_ptr(), n, E, arc_s.data_ptr(), cap, work.data_ptr(), ws_s, res.data_ptr(), 0, None, level, bs,
                                        True, False, sp)

    def shufflev():
        zxc_amd.compress_shufflev_device(table.data_ptr(), count, n, E, arc_v.data_ptr(), cap, work.data_ptr(), ws_v, res.data_ptr(), 0, None,
                                         level, bs, True, False, sp)

    cat_then_shuffle()
    n_s = int(res.item())
    shufflev()
    n_v = int(res.item())
    assert n_s == n_v > 0 and torch.equal(arc_s[:n_s], arc_v[:n_v]), (n_s, n_v)
    ms = devbench.alternating([cat_then_shuffle, shufflev], a.runs, a.warmup, stream, "wall")
    line = {"kind": "archive", "data": "bf16 weights", "elem_size": E, "bytes": n, "tensors": count, "level": level, "block_size": bs,
            "runs": a.runs, "ratio": round(n / n_v, 4), "extra_bytes_cat_shuffle": n + ws_s, "extra_bytes_shufflev": ws_v}
    for prefix, m in zip(("cat_shuffle", "shufflev"), ms):
        line.update(stats(m, n, prefix))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--tensors", type=int, default=256)
    ap.add_argument("--kernel-mib", type=int, default=1024)
    ap.add_argument("--levels", default="3")
    ap.add_argument("--blocks", default="524288,65536", help="comma-separated block sizes")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "compress_shufflev_device_bench.jsonl"))
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
    if n:
        src = torch.randint(0, 256, (n,), device="cuda", dtype=torch.uint8)
        dst = torch.zeros(n, dtype=torch.uint8, device="cuda")
        for E in (2, 4):
            for entry_bytes in (n, 4 << 20, 4096):
                emit(kernel_case(E, 524288, src, dst, n, min(entry_bytes, n), a, stream))
        del src, dst
        torch.cuda.empty_cache()
    n = a.mib << 20
    each = n // a.tensors // 2 * 2
    g = torch.Generator(device="cuda").manual_seed(a.seed)
    tensors = [(torch.randn(each // 2, device="cuda", generator=g) * 0.02).to(torch.bfloat16).view(torch.uint8) for _ in range(a.tensors)]
    n = each * a.tensors
    for bs in (int(x) for x in a.blocks.split(",")):
        for level in (int(x) for x in a.levels.split(",")):
            emit(archive_case(tensors, n, level, bs, a, stream))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
